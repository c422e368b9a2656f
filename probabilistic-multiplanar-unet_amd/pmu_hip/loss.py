"""The training losses on HIP kernels (row a6): drop-ins for the torch criteria the reference builds.

  BCELoss           nn.BCELoss on the sigmoid head (UNetTrainer, PMU/trainer/unet_trainer.py:23,33-37)
  CrossEntropyLoss  nn.CrossEntropyLoss on the logits (UNetTrainer n_classes > 1; ProbabilisticUnet.elbo
                    with reduction 'none' summed, probabilistic_unet.py:286-304)
  SoftDiceLoss      1 - mean soft Dice (dice_coeff's formula, PMU/dice_loss.py:5-12, on probabilities): not a
                    reference criterion — opt-in through the trainers' loss= / ProbabilisticUnet.recon_loss
  BoundaryLoss      mean of probability x signed distance to the target's contour (Kervadec et al. 2019), the
                    map formed on the device per step; opt-in the same way, added to a region loss

Same constructors and reductions as torch's; the forward is one deterministic streaming reduction
(pmu_bce_fwd / pmu_ce_fwd), the backward one elementwise kernel scaled on the device by the upstream
gradient (pmu_bce_bwd / pmu_ce_bwd): no host synchronisation.  Per-class weights, label smoothing
and probabilistic (float) CE targets are not used by the reference and are rejected.
"""
from __future__ import annotations

import torch
import torch.nn as nn

from . import _lib as L

_RED = {"none": 0, "mean": 1, "sum": 2}


def _red(reduction):
    if reduction not in _RED:
        raise ValueError(f"reduction {reduction!r}")
    return _RED[reduction]


def _dev_check(name, *ts):
    for t in ts:
        if not isinstance(t, torch.Tensor) or not t.is_cuda:
            raise RuntimeError(f"{name} runs on the MI355X HIP path only (there is no CPU fallback)")


class _BCE(torch.autograd.Function):
    @staticmethod
    def forward(ctx, y, t, red):
        yc, tc = y.detach().contiguous().float(), t.detach().contiguous().float()
        n = yc.numel()
        s = L.stream()
        if red == 0:
            loss = torch.empty_like(yc)
            L.call("pmu_bce_fwd", yc.data_ptr(), tc.data_ptr(), n, 0, loss.data_ptr(), None, None, s)
        else:
            loss = torch.empty((), dtype=torch.float32, device=y.device)
            ws = torch.empty(L.lib().pmu_loss_ws(n) // 8, dtype=torch.float64, device=y.device)
            L.call("pmu_bce_fwd", yc.data_ptr(), tc.data_ptr(), n, red, loss.data_ptr(), ws.data_ptr(), None, s)
        ctx.save_for_backward(yc, tc)
        ctx.red = red
        return loss

    @staticmethod
    def backward(ctx, g):
        yc, tc = ctx.saved_tensors
        gc = g.detach().contiguous().float()
        dy = torch.empty_like(yc)
        L.call("pmu_bce_bwd", yc.data_ptr(), tc.data_ptr(), yc.numel(), ctx.red, gc.data_ptr(), dy.data_ptr(),
               L.stream())
        return dy, None, None


class _CE(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, t, red, ignore):
        xc = x.detach().contiguous().float()
        tc = t.detach().contiguous().long()
        N, K = xc.shape[0], xc.shape[1]
        HW = xc[0, 0].numel()
        if tc.numel() != N * HW:
            raise RuntimeError(f"CrossEntropyLoss: target {tuple(t.shape)} does not match input {tuple(x.shape)}")
        s = L.stream()
        count = torch.empty((), dtype=torch.float32, device=x.device)
        if red == 0:
            loss = torch.empty(tc.shape, dtype=torch.float32, device=x.device)
            L.call("pmu_ce_fwd", xc.data_ptr(), tc.data_ptr(), N, K, HW, 0, ignore, loss.data_ptr(), None, None, s)
        else:
            loss = torch.empty((), dtype=torch.float32, device=x.device)
            ws = torch.empty(L.lib().pmu_loss_ws(N * HW) // 8, dtype=torch.float64, device=x.device)
            L.call("pmu_ce_fwd", xc.data_ptr(), tc.data_ptr(), N, K, HW, red, ignore, loss.data_ptr(), ws.data_ptr(),
                   count.data_ptr(), s)
        ctx.save_for_backward(xc, tc, count)
        ctx.red, ctx.ignore = red, ignore
        return loss

    @staticmethod
    def backward(ctx, g):
        xc, tc, count = ctx.saved_tensors
        gc = g.detach().contiguous().float()
        dx = torch.empty_like(xc)
        N, K = xc.shape[0], xc.shape[1]
        L.call("pmu_ce_bwd", xc.data_ptr(), tc.data_ptr(), N, K, xc[0, 0].numel(), ctx.red, ctx.ignore, gc.data_ptr(),
               count.data_ptr(), dx.data_ptr(), L.stream())
        return dx, None, None, None


class _SoftDice(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, t, act, per_image, first, ignore):
        xc = x.detach().contiguous().float()
        N, K = xc.shape[0], xc.shape[1]
        HW = xc[0, 0].numel()
        tc = t.detach().contiguous()
        tc = tc.float() if K == 1 else tc.long()
        if tc.numel() != N * HW:
            raise RuntimeError(f"SoftDiceLoss: target {tuple(t.shape)} does not match input {tuple(x.shape)}")
        loss = torch.empty((), dtype=torch.float32, device=x.device)
        ws = torch.empty(L.lib().pmu_softdice_ws(N, K, HW) // 8, dtype=torch.float64, device=x.device)
        L.call("pmu_softdice_fwd", xc.data_ptr(), tc.data_ptr(), N, K, HW, act, per_image, first, ignore,
               loss.data_ptr(), ws.data_ptr(), L.stream())
        ctx.save_for_backward(xc, tc, ws)   # ws begins with the backward's coefficient block
        ctx.args = (act, per_image, ignore)
        return loss

    @staticmethod
    def backward(ctx, g):
        xc, tc, ws = ctx.saved_tensors
        act, per_image, ignore = ctx.args
        gc = g.detach().contiguous().float()
        dx = torch.empty_like(xc)
        L.call("pmu_softdice_bwd", xc.data_ptr(), tc.data_ptr(), xc.shape[0], xc.shape[1], xc[0, 0].numel(), act,
               per_image, ignore, ws.data_ptr(), gc.data_ptr(), dx.data_ptr(), L.stream())
        return dx, None, None, None, None, None


SOFTDICE_MAX_CLASSES = 8


class SoftDiceLoss(nn.Module):
    """1 - mean Dice of the class probabilities, D = (2 sum(p t) + 1e-6) / (sum p + sum t + 1e-6): the
    formula and smoothing of dice_coeff (PMU/dice_loss.py:5-12) on probabilities, differentiable, on HIP
    kernels (pmu_softdice_fwd / _bwd).  Not in the reference, which only reports Dice.

    (N, K, *) logits with (N, *) class-index targets for K >= 2 (softmax in the kernel; ignore_index
    pixels are left out); (N, 1, *) with a same-sized float mask, used by value, for one class.
    from_logits: None = probabilities for one class (the U-Net's sigmoid head), logits for K >= 2; True
    for one class applies the sigmoid in the kernel.  include_background=False averages classes 1..K-1;
    per_image=True forms the sums per image instead of over the batch (dice_coeff's pooling).  K <= 8."""

    def __init__(self, include_background=True, per_image=False, ignore_index=-100, from_logits=None):
        super().__init__()
        self.include_background = bool(include_background)
        self.per_image = bool(per_image)
        self.ignore_index = int(ignore_index)
        self.from_logits = from_logits

    def forward(self, input, target):
        _dev_check("SoftDiceLoss", input, target)
        if input.dim() < 2 or input.numel() == 0:
            raise ValueError(f"SoftDiceLoss: input {tuple(input.shape)} is not (N, K, *)")
        K = input.shape[1]
        if K > SOFTDICE_MAX_CLASSES:
            raise ValueError(f"SoftDiceLoss supports at most {SOFTDICE_MAX_CLASSES} classes, got {K}")
        logits = (K > 1) if self.from_logits is None else bool(self.from_logits)
        if K > 1:
            if not logits:
                raise ValueError("SoftDiceLoss: K >= 2 takes logits (the softmax is part of the kernel)")
            if target.is_floating_point():
                raise ValueError("SoftDiceLoss: K >= 2 takes class-index targets")
        first = 0 if (K == 1 or self.include_background) else 1
        return _SoftDice.apply(input, target, int(logits) if K == 1 else 0, int(self.per_image), first,
                               self.ignore_index)


class CEPlusDiceLoss(nn.Module):
    """criterion(input, target) + SoftDiceLoss(input, target) — the trainers' loss="ce+dice" (BCE + Dice
    on the sigmoid head for one class); the sum is formed by autograd."""

    def __init__(self, criterion, dice):
        super().__init__()
        self.criterion, self.dice = criterion, dice

    def forward(self, input, target):
        return self.criterion(input, target) + self.dice(input, target)


class _Boundary(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, t, act, first, ignore):
        from . import boundary as B
        xc = x.detach().contiguous().float()
        N, K, H, W = xc.shape
        tc = t.detach().contiguous()
        tc = tc.float() if K == 1 else tc.long()
        if tc.numel() != N * H * W:
            raise RuntimeError(f"BoundaryLoss: target {tuple(t.shape)} does not match input {tuple(x.shape)}")
        ws = B._workspace(N, K, H, W, x.device)
        phi = B._map(tc, K, H, W, ignore, ws)
        loss = torch.empty((), dtype=torch.float32, device=x.device)
        count = torch.empty((), dtype=torch.float64, device=x.device)
        L.call("pmu_boundary_fwd", xc.data_ptr(), tc.data_ptr(), phi.data_ptr(), N, K, H * W, act, first, ignore,
               loss.data_ptr(), count.data_ptr(), ws.data_ptr(), L.stream())
        ctx.save_for_backward(xc, tc, phi, count)
        ctx.args = (act, first, ignore)
        return loss

    @staticmethod
    def backward(ctx, g):
        xc, tc, phi, count = ctx.saved_tensors
        act, first, ignore = ctx.args
        gc = g.detach().contiguous().float()
        dx = torch.empty_like(xc)
        N, K, H, W = xc.shape
        L.call("pmu_boundary_bwd", xc.data_ptr(), tc.data_ptr(), phi.data_ptr(), N, K, H * W, act, first, ignore,
               gc.data_ptr(), count.data_ptr(), dx.data_ptr(), L.stream())
        return dx, None, None, None, None


class BoundaryLoss(nn.Module):
    """The boundary loss of Kervadec et al. (MIDL 2019): the mean over the valid pixels and the classes of the
    class probability times the signed distance to the target's contour of that class (negative inside,
    positive outside; pmu_hip.boundary.signed_distance), on HIP kernels (pmu_boundary_map / _fwd / _bwd).  The
    map is formed from the target in the forward, on the device, and kept for the backward.  The value may be
    negative.  Meant to be added to a region loss with a small, growing weight (RegionPlusBoundaryLoss).

    (N, K, H, W) logits with (N, H, W) class-index targets for K >= 2 (softmax in the kernel; ignore_index
    pixels are left out and belong to no class); (N, 1, H, W) with a same-sized float mask (a member where it
    is >= 0.5) for one class.  from_logits as SoftDiceLoss: None = probabilities for one class, logits for
    K >= 2; True for one class applies the sigmoid in the kernel.  include_background=False (the paper's
    choice) averages classes 1..K-1.  K <= 8, H and W <= 1024."""

    def __init__(self, include_background=False, ignore_index=-100, from_logits=None):
        super().__init__()
        self.include_background = bool(include_background)
        self.ignore_index = int(ignore_index)
        self.from_logits = from_logits

    def forward(self, input, target):
        from .boundary import check_plane
        _dev_check("BoundaryLoss", input, target)
        if input.dim() != 4 or input.numel() == 0:
            raise ValueError(f"BoundaryLoss: input {tuple(input.shape)} is not (N, K, H, W)")
        K = input.shape[1]
        if K > SOFTDICE_MAX_CLASSES:
            raise ValueError(f"BoundaryLoss supports at most {SOFTDICE_MAX_CLASSES} classes, got {K}")
        check_plane("BoundaryLoss", K, input.shape[2], input.shape[3])
        logits = (K > 1) if self.from_logits is None else bool(self.from_logits)
        if K > 1:
            if not logits:
                raise ValueError("BoundaryLoss: K >= 2 takes logits (the softmax is part of the kernel)")
            if target.is_floating_point():
                raise ValueError("BoundaryLoss: K >= 2 takes class-index targets")
        first = 0 if (K == 1 or self.include_background) else 1
        return _Boundary.apply(input, target, int(logits) if K == 1 else 0, first, self.ignore_index)


class RegionPlusBoundaryLoss(nn.Module):
    """region(input, target) + weight * boundary(input, target) — the trainers' loss="ce+boundary" /
    "dice+boundary".  ``weight`` is a plain attribute: the training loop raises it per epoch (train.py
    --boundary-weight / --boundary-ramp, the paper's "increase" schedule with the region weight kept at 1)."""

    def __init__(self, region, boundary, weight=0.01):
        super().__init__()
        self.region, self.boundary = region, boundary
        self.weight = float(weight)

    def forward(self, input, target):
        return self.region(input, target) + self.weight * self.boundary(input, target)


BOUNDARY_WEIGHT = 0.01   # the starting weight of the boundary term (train.py --boundary-weight)
LOSS_CHOICES = ("default", "dice", "ce+dice", "ce+boundary", "dice+boundary")


def make_criterion(n_classes, loss="default"):
    """The trainers' criterion: "default" the reference's BCELoss (one class) / CrossEntropyLoss, "dice"
    SoftDiceLoss, "ce+dice" their sum; "ce+boundary" / "dice+boundary" the region loss plus BOUNDARY_WEIGHT
    times BoundaryLoss (RegionPlusBoundaryLoss)."""
    if loss not in LOSS_CHOICES:
        raise ValueError(f"loss {loss!r}: expected one of {LOSS_CHOICES}")
    base = BCELoss() if n_classes == 1 else CrossEntropyLoss()
    if loss == "default":
        return base
    if loss.endswith("+boundary"):
        return RegionPlusBoundaryLoss(base if loss == "ce+boundary" else SoftDiceLoss(), BoundaryLoss(),
                                      BOUNDARY_WEIGHT)
    return SoftDiceLoss() if loss == "dice" else CEPlusDiceLoss(base, SoftDiceLoss())


class BCELoss(nn.BCELoss):
    """nn.BCELoss(weight=None, reduction='mean') on HIP kernels."""

    def forward(self, input, target):
        if self.weight is not None:
            raise NotImplementedError("BCELoss(weight=...) is not used by the reference")
        if input.shape != target.shape:
            raise ValueError(f"Using a target size ({target.shape}) that is different to the input size ({input.shape})")
        _dev_check("BCELoss", input, target)
        return _BCE.apply(input, target, _red(self.reduction))


class CrossEntropyLoss(nn.CrossEntropyLoss):
    """nn.CrossEntropyLoss(weight=None, ignore_index=-100, reduction='mean', label_smoothing=0) on HIP
    kernels; class-index targets (N, *) for logits (N, C, *)."""

    def forward(self, input, target):
        if self.weight is not None or self.label_smoothing != 0.0:
            raise NotImplementedError("CrossEntropyLoss weight / label_smoothing are not used by the reference")
        if target.is_floating_point():
            raise NotImplementedError("CrossEntropyLoss with class-probability targets is not used by the reference")
        _dev_check("CrossEntropyLoss", input, target)
        return _CE.apply(input, target, _red(self.reduction), int(self.ignore_index))
