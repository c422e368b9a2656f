"""Forward/backward executor of the U-Net conv stack on libpmunet_hip.

Everything here only enqueues HIP kernels on the current torch stream through the C ABI;
PyTorch supplies device memory (caching allocator) and the stream.  Activations live
channels-last (NHWC) between kernels; a layer's output is kept as its *pre-BN* conv result
``z`` plus per-channel BN coefficients, and the consumer applies BN+ReLU (+pool / +concat)
while staging its operand, so post-activation tensors are never materialised.  Which kernel runs a
conv is decided in routes.py; the code here asks the route, then allocates and launches for it.

Reference call graph mirrored here (PMU/ = Probabilistic-Multiplanar-Unet/):
  UNet.forward                 PMU/model/unet/unet_model.py:31-54
  DoubleConv / Down / Up / OutConv   PMU/model/unet/unet_parts.py:9-76
"""
from __future__ import annotations

import ctypes
from dataclasses import dataclass, field

import torch

from . import _lib as L
from . import routes
from .packs import (BF16S, F32, _LAYOUTS, _PACKS, invalidate_packs, pack_convT_weights,  # noqa: F401
                    pack_convT_weights_dma, pack_weights, pack_weights_bf16,
                    pack_weights_dma, pack_weights_raw, pack_weights_wino, pack_weights_wino2h, pack_weights_wino4,
                    repack)
from .routes import CFG, EngineConfig, dxb_ok, pool_fuse_ok  # noqa: F401  (public names of the engine)
from .routes import pad8 as _pad8


# ----------------------------------------------------------------------------------------
# operand descriptors
# ----------------------------------------------------------------------------------------
@dataclass
class Src:
    """One channel source of a conv operand (see pmu_src in include/pmunet_hip.h)."""
    x: torch.Tensor                  # NHWC [N][H][W][C]
    mode: int = L.SRC_RAW
    coef: torch.Tensor | None = None
    z: torch.Tensor | None = None    # BNBWD only
    pool: int = L.POOL_NONE
    off: tuple = (0, 0)
    prod: object = None              # the ConvBNOut whose activation this is (SRC_BNRELU sources)

    @property
    def C(self) -> int:
        return self.x.shape[3]


def frame_of(srcs, N: int, H: int, W: int):
    """The pmu_frame of an operand, by reference (the kernels' first argument)."""
    f = L.PmuFrame()
    f.nsrc = len(srcs)
    f.N, f.H, f.W = N, H, W
    for i, s in enumerate(srcs):
        t = s.x
        assert t.is_contiguous() and t.dtype in (F32, BF16S) and t.dim() == 4, \
            "operand must be contiguous NHWC fp32 (or bf16 bits)"
        c = f.src[i]
        c.x = t.data_ptr()
        c.z = s.z.data_ptr() if s.z is not None else None
        c.dtype = (L.DT_X_BF16 if t.dtype == BF16S else 0) | (L.DT_Z_BF16 if s.z is not None and s.z.dtype == BF16S else 0)
        c.coef = s.coef.data_ptr() if s.coef is not None else None
        c.mode, c.pool = s.mode, s.pool
        c.C, c.H, c.W = t.shape[3], t.shape[1], t.shape[2]
        c.off_h, c.off_w = s.off
    return ctypes.byref(f)


def _f32_srcs(srcs, N, H, W):
    """srcs for a call that stages fp32 frames itself (the fused-staging kernels): unchanged when every
    source is stored in fp32, else the frame's values materialised once in fp32 as one RAW source."""
    if all(sr.x.dtype == F32 and (sr.z is None or sr.z.dtype == F32) for sr in srcs):
        return srcs
    return [Src(frame_to_f32(srcs, N, H, W))]


def _materialised(srcs, dtype):
    """The operand tensor itself when the frame is one RAW, unpooled, unshifted source already stored
    in the dtype the GEMM reads (fp32, or bf16 with channels padded to 8): no copy is needed."""
    if len(srcs) != 1:
        return None
    sr = srcs[0]
    if (sr.mode != L.SRC_RAW or sr.pool != L.POOL_NONE or sr.off != (0, 0) or sr.x.dtype != dtype
            or not sr.x.is_contiguous() or sr.x.dim() != 4):
        return None
    if dtype == BF16S and sr.C % 8 != 0:
        return None
    return sr.x


def _empty(*shape, dtype=F32, device=None):
    return torch.empty(shape, dtype=dtype, device=device)


class GradSink(dict):
    """param -> gradient tensor.  ``new(p)`` hands out the destination a kernel writes: a view
    of the network's persistent flat gradient buffer when one is attached (stable pointers for
    the fused optimizer / one-shot all-reduce), else a fresh tensor.

    ``on_ready``: called by ``flush()`` as ``on_ready(params, flat)`` with the parameters whose
    gradient kernels have been enqueued on the stream since the previous flush, so a
    data-parallel reducer (pmu_hip.dp) can learn the backward order and, for a flat-buffer sink
    (``flat``), start a bucket's all-reduce while the rest of the backward still runs."""

    def __init__(self, views=None, on_ready=None):
        super().__init__()
        self.views = views
        self.flat = views is not None
        self.on_ready = on_ready
        self._pending = []

    def new(self, p):
        t = self.views.get(p) if self.views is not None else None
        if t is None:
            t = torch.empty_like(p)
        self[p] = t
        if self.on_ready is not None:
            self._pending.append(p)
        return t

    def flush(self):
        if self.on_ready is not None and self._pending:
            ready, self._pending = self._pending, []
            self.on_ready(ready, self.flat)


# ----------------------------------------------------------------------------------------
# BatchNorm
# ----------------------------------------------------------------------------------------
@dataclass
class BNState:
    coef: torch.Tensor      # [scale | shift]
    mean: torch.Tensor | None = None     # batch statistics; None: there are none (eval mode), and the
    invstd: torch.Tensor | None = None   # routes keep the fused *_bnr paths off
    count: float = 0.0
    frozen: tuple | None = None          # eval mode, a backward follows: (running_mean, 1/sqrt(running_var + eps))


def bn_forward(part, R: int, C: int, count: int, bn: torch.nn.BatchNorm2d, training: bool, dev,
               keep: bool = False) -> BNState:
    """BatchNorm2d statistics (train) or running-stat coefficients (eval).  keep (eval): a backward
    follows, so the statistics the coefficients were made from are kept beside them (BNState.frozen:
    copies, the buffers may move before the backward runs)."""
    s = L.stream()
    use_batch = training or not bn.track_running_stats or bn.running_mean is None
    if not use_batch:
        coef = _empty(2 * C, device=dev)
        L.call("pmu_bn_eval_coef", bn.running_mean.data_ptr(), bn.running_var.data_ptr(), L.ptr(bn.weight),
               L.ptr(bn.bias), float(bn.eps), C, coef.data_ptr(), s)
        frozen = (bn.running_mean.detach().clone(), torch.rsqrt(bn.running_var.detach() + bn.eps)) if keep else None
        return BNState(coef=coef, frozen=frozen)
    G = L.lib().pmu_colsum_groups(R)
    acc = _empty(G, 2 * C, dtype=torch.float64, device=dev)
    L.call("pmu_colsum_f64", part.data_ptr(), R, 2 * C, acc.data_ptr(), G, s)
    mean, invstd, coef = _empty(C, device=dev), _empty(C, device=dev), _empty(2 * C, device=dev)
    update = training and bn.track_running_stats and bn.running_mean is not None
    momentum = bn.momentum
    nbt = None  # the finalize kernel adds 1 to num_batches_tracked (one launch fewer per layer)
    if update:
        if momentum is None:  # cumulative moving average: the host needs the count now
            bn.num_batches_tracked.add_(1)
            momentum = 1.0 / float(bn.num_batches_tracked.item())
        elif bn.num_batches_tracked.dtype == torch.int64 and bn.num_batches_tracked.device == dev:
            nbt = bn.num_batches_tracked.data_ptr()
        else:
            bn.num_batches_tracked.add_(1)
    L.call("pmu_bn_fwd_finalize", acc.data_ptr(), G, C, float(count), L.ptr(bn.weight), L.ptr(bn.bias),
           float(bn.eps), float(momentum or 0.0),
           bn.running_mean.data_ptr() if update else None, bn.running_var.data_ptr() if update else None,
           nbt, mean.data_ptr(), invstd.data_ptr(), coef.data_ptr(), s)
    return BNState(coef=coef, mean=mean, invstd=invstd, count=float(count))


def bn_backward(da: torch.Tensor, z: torch.Tensor, st: BNState, bn: torch.nn.BatchNorm2d, grads, conv_bias=None,
                pre=None):
    """Returns (bcoef, dgamma, dbeta, dbias) for BN+ReLU backward given da = dL/d relu(bn(z)).
    pre: (part, R) — the partial sums (sum g, sum g*xhat) already formed by the kernel that produced
    da (a *_bnr input gradient); else pmu_bn_bwd_reduce reads da and z for them.

    A state without batch statistics (eval mode, st.frozen) gives frozen BatchNorm's backward, the running
    statistics being constants of the graph: with xhat = (z - running_mean) / sqrt(running_var + eps),
    dgamma = sum g xhat, dbeta = sum g, dz = scale g (kx = kc = 0 in bcoef), dbias = scale sum g."""
    s = L.stream()
    dev = z.device
    N, H, W, C = z.shape
    P = N * H * W
    lb = L.lib()
    frozen = st.mean is None
    if frozen and st.frozen is None:
        raise RuntimeError("BatchNorm backward in eval mode: the forward was not told a backward follows (keep)")
    mean, invstd = st.frozen if frozen else (st.mean, st.invstd)
    if pre is not None:
        part, R = pre
    else:
        R = lb.pmu_bn_bwd_tiles(P, C)
        part = _empty(R, 2 * C, device=dev)
        if da.dtype == BF16S and (z.dtype != F32 or C % 4 != 0):
            da = frame_to_f32([Src(da)], N, H, W)   # (the bf16-da reduce takes fp32 z, channel quads)
        name = ("pmu_bn_bwd_reduce_dxb" if da.dtype == BF16S else
                "pmu_bn_bwd_reduce_zb" if z.dtype == BF16S else "pmu_bn_bwd_reduce")
        L.call(name, da.data_ptr(), z.data_ptr(), st.coef.data_ptr(), mean.data_ptr(), invstd.data_ptr(), P, C,
               part.data_ptr(), s)
    G = lb.pmu_colsum_groups(R)
    acc = _empty(G, 2 * C, dtype=torch.float64, device=dev)
    L.call("pmu_colsum_f64", part.data_ptr(), R, 2 * C, acc.data_ptr(), G, s)
    dgamma = grads.new(bn.weight) if bn.weight is not None else None
    dbeta = grads.new(bn.bias) if bn.bias is not None else None
    dbias = grads.new(conv_bias) if conv_bias is not None else _empty(C, device=dev)
    if frozen:   # (a few [C] vector ops: not a hot path)
        sg, sgx = acc.sum(0).view(2, C)
        if dgamma is not None:
            dgamma.copy_(sgx)
        if dbeta is not None:
            dbeta.copy_(sg)
        dbias.copy_(st.coef[:C].double() * sg)
        return torch.cat([st.coef, mean, torch.zeros(2 * C, device=dev)]), dgamma, dbeta, dbias
    bcoef = _empty(5 * C, device=dev)
    L.call("pmu_bn_bwd_finalize", acc.data_ptr(), G, C, float(P), L.ptr(bn.weight), st.coef.data_ptr(),
           mean.data_ptr(), invstd.data_ptr(), L.ptr(dgamma), L.ptr(dbeta), dbias.data_ptr(),
           bcoef.data_ptr(), s)
    return bcoef, dgamma, dbeta, dbias


# ----------------------------------------------------------------------------------------
# conv + BN layer
# ----------------------------------------------------------------------------------------
@dataclass
class X1Grad:
    """What a concat conv's bf16 input gradient leaves for the transposed conv behind dx1 (the *_x1b /
    *_x1b_sum entries): dx1 in bf16, and — when dx1 was written in bf16 only — the per-tile column sums
    (part, R, split) its bias gradient is reduced from."""
    bf16: torch.Tensor
    colsum: tuple | None = None


@dataclass
class ConvBNOut:
    z: torch.Tensor       # NHWC pre-BN conv output
    bn: BNState
    srcs: list = field(default_factory=list)   # the operand sources it consumed (for wgrad)
    planes: list | None = None                  # first-layer input planes
    bf16: bool = False                          # computed on the bf16-MFMA kernels
    xt: torch.Tensor | None = None              # bf16: the operand copy the forward kernel wrote (for wgrad)
    xt32: torch.Tensor | None = None            # fp32: the same, teed by pmu_conv3x3_fwd (RAW wgrad operand)
    bnr: tuple | None = None                    # (da, part, R): BN-backward partials formed by the consumer's dgrad
    x1: X1Grad | None = None                    # by-products of this (concat) conv's bf16 input gradient

    def act(self, pool=L.POOL_NONE) -> Src:
        return Src(self.z, L.SRC_BNRELU, self.bn.coef, pool=pool, prod=self)


def _check_channels(cin: int, layer) -> None:
    """The kernels take channel counts from the operand frame and index the weight by them, so an
    operand whose channel count differs from the layer's is refused here, as torch's conv would."""
    if cin != layer.in_channels:
        raise RuntimeError(f"{type(layer).__name__}: operand has {cin} channels, the layer expects "
                           f"{layer.in_channels} (weight {tuple(layer.weight.shape)})")


def conv_bn_forward(srcs, conv: torch.nn.Conv2d, bn: torch.nn.BatchNorm2d, N, H, W, training, dev,
                    planes=None, bf16=False, keep=False, zb=False) -> ConvBNOut:
    """relu(bn(conv(operand))) forward: z (pre-BN conv output, NHWC) + batch statistics.

    zb (bf16 mode, unet_forward with CFG.bf16_z): the LDS-DMA conv stores z in bf16, as torch.autocast
    keeps a conv's output, centred on the BN running mean (pmu_conv3x3_fwd_dma_zb: bf16(z - rm), so
    the rounding is relative to the channel's spread, not its mean); the layer's coefficients are
    then the centred ones (pmu_bn_center) and its consumers read z through bf16-aware frames,
    pmu_bn_bwd_reduce_zb, pmu_maxpool2_bwd_zb and the *_bnr_zb input gradient."""
    Cout = conv.out_channels
    _check_channels(len(planes) if planes is not None else sum(sr.C for sr in srcs), conv)
    s = L.stream()
    lb = L.lib()
    z = _empty(N, H, W, Cout, device=dev)
    xt = xt32 = zoff = None
    need_stats = training or not bn.track_running_stats
    route = routes.conv_fwd_route(bf16, N, H, W, sum(sr.C for sr in srcs), Cout,
                                  planes=len(planes) if planes is not None else 0)
    if planes is not None and route != "first":
        # channel counts outside the first-layer kernel: the generic 3x3 path on a raw NHWC frame
        srcs = [Src(torch.stack(planes, dim=-1).contiguous())]
        planes = None
    Cin = sum(sr.C for sr in srcs)
    Cp = _pad8(Cin)
    if routes.conv_fwd_keeps_f32(route, Cin, Cout, keep):
        # the weight gradient reads the operand the kernel staged (RAW) instead of re-deriving it.  (Taken on
        # a materialised route too, where the stored operand then replaces it: a wasted buffer the previous
        # code had as well, left in place so that peak memory is unchanged by this refactor.)
        xt32 = _empty(N, H, W, Cin, device=dev)
    R = (lb.pmu_conv_first_tiles(N, H, W) if route == "first" else
         lb.pmu_conv3x3_tiles_dma(N, H, W, Cout, Cp) if route == "dma" else
         lb.pmu_conv3x3_tiles_raw(N, H, W, Cout) if route == "raw" else
         lb.pmu_conv3x3_tiles_wino4(N, H, W) if route == "wino4" else
         lb.pmu_conv3x3_tiles_wino(N, H, W) if route in ("wino2h", "wino_fused") else
         lb.pmu_conv3x3_tiles(N, H, W))
    part = _empty(R, 2 * Cout, device=dev) if need_stats else None
    entry, bias = routes.conv_fwd_entry(route, Cout, zb), L.ptr(conv.bias)
    if route == "first":
        arr = (ctypes.c_void_p * len(planes))(*[p.data_ptr() for p in planes])
        L.call(entry, arr, len(planes), N, H, W, conv.weight.data_ptr(), bias, Cout, z.data_ptr(), L.ptr(part), s)
    elif route in routes.MATERIALISED:
        # the operand (BN+ReLU / max-pool / F.pad+cat applied) stored once, in bf16 or fp32, unless it is a
        # stored tensor already; the GEMM streams it and the weight gradient reuses it
        pack = _FWD_PACK[route]
        wp = pack(conv.weight, dgrad=False) if route == "wino4" else None   # (packs first)
        xm = _materialised(srcs, BF16S if bf16 else F32)
        if xm is None:
            xm = frame_to_bf16(srcs, N, H, W) if bf16 else frame_to_f32(srcs, N, H, W)
        wp = wp if wp is not None else pack(conv.weight, dgrad=False)
        lead = (xm.data_ptr(), Cp if bf16 else Cin, N, H, W, wp.data_ptr(), bias, Cout)
        if entry == routes.FWD_DMA_ZB:
            z = _empty(N, H, W, Cout, dtype=BF16S, device=dev)
            # the running mean before this step's update (bn_forward below moves it)
            zoff = (bn.running_mean.detach().clone() if bn.track_running_stats and bn.running_mean is not None
                    else torch.zeros(Cout, device=dev))
            L.call(entry, *lead, z.data_ptr(), zoff.data_ptr(), L.ptr(part), s)
        else:
            L.call(entry, *lead, z.data_ptr(), L.ptr(part), s)
        xt = xm if bf16 and keep else None
        xt32 = xm if xt32 is not None else None
        if bf16:
            del xm   # (not kept: released before the BN statistics' buffers are taken)
    elif route == "bf16_fused":
        wp = pack_weights_bf16(conv.weight, dgrad=False)
        xt = (torch.empty(N, H, W, Cp, dtype=torch.int16, device=dev)
              if keep else None)   # the weight gradient's operand, teed by the fused kernel
        L.call(entry, frame_of(_f32_srcs(srcs, N, H, W), N, H, W), wp.data_ptr(), bias, Cout, z.data_ptr(),
               L.ptr(part), L.ptr(xt), s)
    elif route == "wino_fused":
        wp = pack_weights_wino(conv.weight, dgrad=False)
        L.call(entry, frame_of(srcs, N, H, W), wp.data_ptr(), bias, Cout, z.data_ptr(), L.ptr(part), L.ptr(xt32), s)
    else:
        wp = pack_weights(conv.weight, dgrad=False)
        L.call(entry, frame_of(srcs, N, H, W), conv.weight.data_ptr(), wp.data_ptr(), bias, Cout, z.data_ptr(),
               L.ptr(part), L.ptr(xt32), s)
    st = bn_forward(part, R, Cout, N * H * W, bn, training, dev, keep=keep)
    if zoff is not None:   # consumers apply the coefficients to the centred stored z
        L.call("pmu_bn_center", st.coef.data_ptr(), L.ptr(st.mean), zoff.data_ptr(), Cout, st.coef.data_ptr(),
               L.ptr(st.mean), s)
        if st.frozen is not None:
            st.frozen = (st.frozen[0] - zoff, st.frozen[1])
    return ConvBNOut(z=z, bn=st, srcs=list(srcs), planes=planes, bf16=bf16 and planes is None, xt=xt, xt32=xt32)


# the weight layout of each materialised-operand route
_FWD_PACK = {"dma": pack_weights_dma, "raw": pack_weights_raw, "wino4": pack_weights_wino4,
             "wino2h": pack_weights_wino2h}


class PoolSumDa:
    """The gradient of a pooled layer's activation, da = dsk + routed dpool (MaxPool2d(2) backward,
    unet_parts.py:33, plus the skip path, unet_parts.py:66; both parts bf16 from *_dxb input gradients,
    or both fp32), left unstored: a stats-only max-pool pass (pmu_maxpool2_bwd_bnr_stats{_dxb,}) formed
    its BN-backward partial sums (prod.bnr) and dz() turns it into that layer's dz in one pass
    (pmu_maxpool2_bwd_bnbwd{_dxb,}: bf16 dz from bf16 parts, fp32 from fp32 ones) — the fp32 da is
    neither written nor re-read.  materialise() stores it (fp32) for the paths that read da itself."""

    def __init__(self, dpool: torch.Tensor, dsk: torch.Tensor, prod: ConvBNOut):
        self.dpool, self.dsk, self.prod = dpool, dsk, prod
        self.bf16_parts = dpool.dtype == BF16S
        self.shape = prod.z.shape
        self.dtype = F32
        self.device = prod.z.device

    def dz(self, bcoef: torch.Tensor, bf16: bool):
        """The layer's dz (bf16 bits or fp32), or None when the parts' storage does not match."""
        if bf16 != self.bf16_parts:
            return None
        N, H, W, C = self.shape
        dz = torch.empty(N, H, W, C, dtype=BF16S if bf16 else F32, device=self.device)
        L.call("pmu_maxpool2_bwd_bnbwd_dxb" if bf16 else "pmu_maxpool2_bwd_bnbwd", self.dpool.data_ptr(),
               self.dsk.data_ptr(), self.prod.z.data_ptr(), self.prod.bn.coef.data_ptr(), bcoef.data_ptr(), N, H, W, C,
               C, dz.data_ptr(), L.stream())
        return dz

    def materialise(self) -> torch.Tensor:
        N, H, W, C = self.shape
        p = self.prod
        part = _empty(L.lib().pmu_maxpool2_bwd_bnr_tiles(N, H, W, C), 2 * C, device=self.device)
        if self.bf16_parts:
            da = _empty(N, H, W, C, device=self.device)
            L.call("pmu_maxpool2_bwd_bnr_dxb", self.dpool.data_ptr(), self.dsk.data_ptr(), p.z.data_ptr(),
                   p.bn.coef.data_ptr(), p.bn.mean.data_ptr(), p.bn.invstd.data_ptr(), N, H, W, C, da.data_ptr(),
                   part.data_ptr(), L.stream())
        else:   # (the fp32 form accumulates in place: into a copy of the skip gradient)
            da = self.dsk.clone()
            L.call("pmu_maxpool2_bwd_bnr", self.dpool.data_ptr(), p.z.data_ptr(), p.bn.coef.data_ptr(),
                   p.bn.mean.data_ptr(), p.bn.invstd.data_ptr(), N, H, W, C, da.data_ptr(), 1, part.data_ptr(),
                   L.stream())
        return da


class HeadDa:
    """The last layer's activation gradient da = OutConv's input gradient (unet_parts.py:70-76 backward:
    sum over classes of dy_k w_k, through the sigmoid for one class) left unstored: the head backward
    (pmu_head1x1_bwd_bnr with da NULL) formed the layer's BN-backward partials and the head's weight
    gradient, and dz(bcoef, bf16) writes the layer's dz straight from dy (pmu_head1x1_bwd_dz) — the
    fp32 da is neither written nor re-read.  materialise() stores it for the paths that read da."""

    def __init__(self, dy: torch.Tensor, y: torch.Tensor, sigmoid: bool, w: torch.Tensor, K: int, prod: ConvBNOut):
        self.dy, self.y, self.sigmoid, self.w, self.K, self.prod = dy, y, sigmoid, w, K, prod
        self.shape = prod.z.shape
        self.dtype = F32
        self.device = prod.z.device

    def dz(self, bcoef: torch.Tensor, bf16: bool) -> torch.Tensor:
        N, H, W, C = self.shape
        out = torch.empty(N, H, W, C, dtype=BF16S if bf16 else F32, device=self.device)
        L.call("pmu_head1x1_bwd_dz", self.dy.data_ptr(), self.y.data_ptr(), int(self.sigmoid), self.w.data_ptr(),
               self.K, C, N, H, W, self.prod.z.data_ptr(), bcoef.data_ptr(), int(bf16), out.data_ptr(), L.stream())
        return out

    def materialise(self) -> torch.Tensor:
        N, H, W, C = self.shape
        da = _empty(N, H, W, C, device=self.device)
        dl = _empty(N, self.K, H, W, device=self.device)
        L.call("pmu_head1x1_bwd", self.dy.data_ptr(), self.y.data_ptr(), int(self.sigmoid), self.w.data_ptr(),
               self.K, C, N, H, W, dl.data_ptr(), da.data_ptr(), L.stream())
        return da


def _concrete(src: Src) -> Src:
    """src with a stored da (PoolSumDa / HeadDa materialised) for the kernels that read da itself."""
    if isinstance(src.x, (PoolSumDa, HeadDa)):
        return Src(src.x.materialise(), src.mode, src.coef, z=src.z, pool=src.pool, off=src.off, prod=src.prod)
    return src


def _bnr_producer(out: ConvBNOut, need_dx: bool, split):
    """The ConvBNOut whose BatchNorm+ReLU backward partial sums this conv's input gradient can form in
    its epilogue: the operand is that layer's unpooled activation alone and its batch statistics exist."""
    if not need_dx or split is not None or len(out.srcs) != 1:
        return None
    sr = out.srcs[0]
    p = sr.prod
    if sr.mode != L.SRC_BNRELU or sr.pool != L.POOL_NONE or p is None or p.bn.mean is None or sr.x is not p.z:
        return None
    return p


def conv_bn_backward(out: ConvBNOut, da: torch.Tensor, conv, bn, grads: dict, need_dx=True, split=None,
                     x1_bf16_only=False, dx_bf16=False):
    """Backward of relu(bn(conv(operand))) given da (NHWC; fp32, or bf16 bits from a *_dxb input
    gradient).  Writes conv/bn grads into ``grads``.

    Returns the operand gradient(s): one NHWC tensor, or (dx0, dx1) when ``split`` is given
    (channel split of a concatenated operand).  x1_bf16_only (bf16 convs): the caller needs dx1 only as
    the transposed conv's bf16 operand and its column sums; what the input gradient wrote beside dx1 is
    left in ``out.x1`` (X1Grad).  dx_bf16 (bf16
    convs, CFG.dx_bf16): the caller's consumers take dx / dx0 stored as bf16 (BF16S) — the LDS-DMA input
    gradient then writes it so (autocast's dtype for a conv's input gradient)."""
    s = L.stream()
    z = out.z
    N, H, W, Cout = z.shape
    dev = z.device
    pre = None
    if out.bnr is not None and out.bnr[0] is da:
        pre = out.bnr[1:]
    out.bnr = None
    if pre is None and isinstance(da, (PoolSumDa, HeadDa)):
        da = da.materialise()
    bcoef, _, _, _ = bn_backward(da, z, out.bn, bn, grads, conv.bias, pre=pre)
    dz_src = Src(da, L.SRC_BNBWD, bcoef, z=z)
    dw = grads.new(conv.weight)
    prod = _bnr_producer(out, need_dx, split)
    if out.bf16:
        return _conv_backward_bf16(out, dz_src, conv, dw, need_dx, split, prod, x1_bf16_only, dx_bf16)
    # (an unstored head / pooled gradient gives dz itself, fp32: a RAW source of the same values)
    dzt = da.dz(bcoef, False) if isinstance(da, (HeadDa, PoolSumDa)) else None
    dz_src = Src(dzt) if dzt is not None else _concrete(dz_src)
    first = out.planes is not None
    Cin = len(out.planes) if first else conv.in_channels
    wroute = routes.conv_wgrad_route(False, N, H, W, Cin, Cout, first=first, kept=out.xt32 is not None,
                                     need_dx=need_dx)
    # teed: the forward kept the operand it staged and the input-gradient kernel tees dz (BN+ReLU backward
    # applied) as it stages it, so the weight gradient multiplies two stored operands
    teed = wroute in routes.TEED
    entry = routes.WGRAD[wroute][0]
    res, xsrcs = None, out.srcs
    if teed:
        dzt = _materialised([dz_src], F32)   # (a dz already stored in fp32 is the tee itself)
        dzt = dzt if dzt is not None else _empty(N, H, W, Cout, device=dev)
        res = _dgrad32(dz_src, conv, N, H, W, split, dzt, prod)
        dz_src, xsrcs = Src(dzt), [Src(out.xt32)]
    ws, wsb = _wgrad_ws(wroute, N, H, W, Cin, Cout, dev)
    tail = (dw.data_ptr(), ws.data_ptr(), wsb, s)
    if first:
        arr = (ctypes.c_void_p * Cin)(*[p.data_ptr() for p in out.planes])
        L.call(entry, frame_of([dz_src], N, H, W), arr, Cin, Cout, *tail)
    elif entry == "pmu_conv3x3_wgrad":   # the direct kernel stages both operand frames itself
        L.call(entry, frame_of([dz_src], N, H, W), frame_of(xsrcs, N, H, W), Cout, *tail)
    else:
        L.call(entry, dzt.data_ptr(), out.xt32.data_ptr(), N, H, W, Cout, Cin, *tail)
    if teed:
        out.xt32 = None
    elif need_dx and not first:
        res = _dgrad32(dz_src, conv, N, H, W, split, None, prod)
    return res


def _wgrad_ws(wroute: str, N, H, W, Cin, Cout, dev):
    """(workspace, its bytes) of a weight-gradient route."""
    wsb = getattr(L.lib(), routes.WGRAD[wroute][1])(N, H, W, Cin, Cout)
    return _empty(max(1, (wsb + 3) // 4), device=dev), wsb


def _bnr_call(name, prod, R, lead, dx, s):
    """Launch a *_bnr input gradient (lead: its leading arguments up to Cin) and leave the producer's
    BN-backward partials on it for its own conv_bn_backward."""
    C = prod.z.shape[3]
    part = _empty(R, 2 * C, device=dx.device)
    L.call(name, *lead, dx.data_ptr(), prod.z.data_ptr(), prod.bn.coef.data_ptr(), prod.bn.mean.data_ptr(),
           prod.bn.invstd.data_ptr(), part.data_ptr(), s)
    prod.bnr = (dx, part, R)


def _dgrad32(dz_src, conv, N, H, W, split, tee, prod=None):
    """fp32 input gradient of a 3x3 conv (Winograd or direct); dx, or (dx0, dx1) split at ``split``.
    tee: receives dz (the BN+ReLU backward applied) for the weight gradient.  prod: the layer whose
    BN-backward partial sums the Winograd kernels form in their epilogue (see _bnr_producer)."""
    s = L.stream()
    dev = conv.weight.device
    Cin, Cout = conv.in_channels, conv.out_channels
    sp = Cin if split is None else split
    dx0 = _empty(N, H, W, sp, device=dev)
    dx1 = _empty(N, H, W, Cin - sp, device=dev) if split is not None else None
    # (the fp32 kernels' BN-backward epilogue reads an fp32 z)
    d = routes.conv_dgrad(False, N, H, W, Cin, Cout, split, bnr=prod is not None,
                          z_bf16=prod is not None and prod.z.dtype != F32)
    dz_src = _f32_srcs([dz_src], N, H, W)[0]
    dzf = frame_of([dz_src], N, H, W)
    lb = L.lib()
    # dz already stored in fp32 (an unstored head / pooled gradient's dz pass): read in place, no copy
    ready = _materialised([dz_src], F32)

    def dz_tensor():
        if ready is not None and (tee is None or tee is ready):
            return ready
        dzt = tee if tee is not None else _empty(N, H, W, Cout, device=dev)
        L.call("pmu_frame_to_f32", dzf, dzt.data_ptr(), s)
        return dzt
    if d.route in routes.MATERIALISED:
        dzt = dz_tensor()
        wp = _FWD_PACK[d.route](conv.weight, dgrad=True)
        lead = (dzt.data_ptr(), Cout, N, H, W, wp.data_ptr(), Cin)
        if d.form == "bnr":
            tiles = lb.pmu_conv3x3_tiles_wino4 if d.route == "wino4" else lb.pmu_conv3x3_tiles_wino2h
            _bnr_call(d.entry, prod, tiles(N, H, W), lead, dx0, s)
        else:
            L.call(d.entry, *lead, sp, dx0.data_ptr(), L.ptr(dx1), s)
    else:
        tee = None if (ready is not None and tee is ready) else tee   # (the tee would be the source itself)
        if d.route == "wino_fused":
            wp = pack_weights_wino(conv.weight, dgrad=True)
            L.call(d.entry, dzf, wp.data_ptr(), Cin, sp, dx0.data_ptr(), L.ptr(dx1), L.ptr(tee), s)
        else:
            wp = pack_weights(conv.weight, dgrad=True)
            L.call(d.entry, dzf, conv.weight.data_ptr(), wp.data_ptr(), Cin, sp, dx0.data_ptr(), L.ptr(dx1),
                   L.ptr(tee), s)
    return dx0 if split is None else (dx0, dx1)


def frame_to_bf16(srcs, N, H, W) -> torch.Tensor:
    """The bf16 operand of a frame, NHWC with channels padded to a multiple of 8 (pmu_frame_to_bf16)."""
    C = sum(sr.C for sr in srcs)
    out = torch.empty(N, H, W, _pad8(C), dtype=torch.int16, device=srcs[0].x.device)
    L.call("pmu_frame_to_bf16", frame_of(srcs, N, H, W), _pad8(C), out.data_ptr(), L.stream())
    return out


def _conv_backward_bf16(out: ConvBNOut, dz_src: Src, conv, dw, need_dx, split, prod=None, x1_bf16_only=False,
                        dx_bf16=False):
    """bf16-MFMA backward of one conv layer (torch.autocast(bfloat16) arithmetic).  dz after the
    BN+ReLU backward is written once in bf16 (dzt); the input gradient streams it (or, for a concat
    split that is not a multiple of 32, stages dz's frame in the fused kernel) and the weight
    gradient multiplies it with the forward's bf16 operand (out.xt)."""
    s = L.stream()
    N, H, W, Cout = out.z.shape
    dev = out.z.device
    Cin = conv.in_channels
    dzt = dz_src.x.dz(dz_src.coef, True) if isinstance(dz_src.x, (PoolSumDa, HeadDa)) else None
    if dzt is None:
        dz_src = _concrete(dz_src)
        dzt = frame_to_bf16([dz_src], N, H, W)
    Cp = dzt.shape[3]
    res = out.x1 = None
    if need_dx:
        sp = Cin if split is None else split
        d = routes.conv_dgrad(True, N, H, W, Cin, Cout, split, bnr=prod is not None,
                              z_bf16=prod is not None and prod.z.dtype == BF16S, want_dxb=dx_bf16,
                              x1_bf16_only=x1_bf16_only)
        # bf16 dx0 (the *_dxb entries; every other output formed from the rounded values)
        dx0 = _empty(N, H, W, sp, dtype=BF16S if d.dxb else F32, device=dev)
        dx1 = _empty(N, H, W, Cin - sp, device=dev) if sp < Cin and d.form != "x1b_sum" else None
        if d.route == "dma":
            wp = pack_weights_dma(conv.weight, dgrad=True)
            lead = (dzt.data_ptr(), Cp, N, H, W, wp.data_ptr(), Cin)
            if d.form in ("bnr", "bnr_zb"):
                _bnr_call(d.entry, prod, L.lib().pmu_conv3x3_tiles_dma(N, H, W, Cin, Cp), lead, dx0, s)
            elif d.form == "x1b_sum":
                # dx1 only in bf16 (the transposed conv's operand) with per-tile column sums (its bias
                # gradient): the fp32 dx1 is neither written nor re-read
                R = L.lib().pmu_conv3x3_tiles_dma(N, H, W, Cin, Cp)
                part = _empty(R, 2 * Cin, device=dev)
                dx1 = torch.empty(N, H, W, Cin - sp, dtype=BF16S, device=dev)
                L.call(d.entry, *lead, sp, dx0.data_ptr(), dx1.data_ptr(), part.data_ptr(), s)
                out.x1 = X1Grad(dx1, (part, R, sp))
            elif d.form == "x1b":
                # the up-sampled part's gradient also in bf16: the transposed conv's operand (unet_backward
                # uses it instead of a pmu_frame_to_bf16 pass over dx1)
                dx1b = torch.empty(N, H, W, Cin - sp, dtype=BF16S, device=dev)
                L.call(d.entry, *lead, sp, dx0.data_ptr(), dx1.data_ptr(), dx1b.data_ptr(), s)
                out.x1 = X1Grad(dx1b)
            else:
                L.call(d.entry, *lead, sp, dx0.data_ptr(), L.ptr(dx1), s)
        elif d.route == "raw":
            wp = pack_weights_raw(conv.weight, dgrad=True)
            L.call(d.entry, dzt.data_ptr(), Cp, N, H, W, wp.data_ptr(), Cin, sp, dx0.data_ptr(), L.ptr(dx1), s)
        else:
            wp = pack_weights_bf16(conv.weight, dgrad=True)
            dz_src = _concrete(dz_src)
            L.call(d.entry, frame_of(_f32_srcs([dz_src], N, H, W), N, H, W), wp.data_ptr(), Cin, sp, dx0.data_ptr(),
                   L.ptr(dx1), None, s)
        res = dx0 if split is None else (dx0, dx1)
    xt = out.xt if out.xt is not None else frame_to_bf16(out.srcs, N, H, W)
    out.xt = None
    wroute = routes.conv_wgrad_route(True, N, H, W, Cin, Cout)
    entry = routes.WGRAD[wroute][0]
    ws, wsb = _wgrad_ws(wroute, N, H, W, Cin, Cout, dev)
    L.call(entry, dzt.data_ptr(), xt.data_ptr(), N, H, W, Cout, Cin, dw.data_ptr(), ws.data_ptr(), wsb, s)
    return res


def frame_to_f32(srcs, N, H, W) -> torch.Tensor:
    """The fp32 operand of a frame, materialised NHWC (pmu_frame_to_f32)."""
    C = sum(sr.C for sr in srcs)
    out = _empty(N, H, W, C, device=srcs[0].x.device)
    L.call("pmu_frame_to_f32", frame_of(srcs, N, H, W), out.data_ptr(), L.stream())
    return out


# ----------------------------------------------------------------------------------------
# U-Net
# ----------------------------------------------------------------------------------------
def _dc_layers(dc):
    """(conv1, bn1, conv2, bn2) of a DoubleConv (double_conv = [conv, bn, relu, conv, bn, relu])."""
    s = dc.double_conv
    return s[0], s[1], s[3], s[4]


@dataclass
class UpState:
    u: torch.Tensor | None   # convT output, NHWC [N][2h][2w][Cup] (None: written into the concat operand)
    off: tuple               # (pad_top, pad_left) inside the skip frame
    prev: ConvBNOut          # convT input producer
    c1: ConvBNOut
    c2: ConvBNOut
    bf16: bool = False       # convT input gradient on bf16 MFMA where its shapes allow
    xt: torch.Tensor | None = None   # bf16: the convT operand the forward materialised (weight gradient)
    cskip: int = 0                   # channels of the skip half of the concat operand (backward split)


class UNetState:
    """Everything the backward needs from one forward."""

    def __init__(self):
        self.xcat = {}          # level -> Up-block concat operand whose skip half the encoder wrote
        self.x = None
        self.planes = None
        self.enc: list = []     # per level: (c1, c2) ConvBNOut
        self.ups: list = []     # per up block: UpState
        self.y = None           # head output (NCHW)
        self.feat_src = None    # last DoubleConv output producer


def _pool_skip(up, prev: ConvBNOut, srcs, N, h, w, bf16):
    """(pooled operand, concat operand) from one pass over prev's activation
    (pmu_frame_to_*_pool_skip), when the Up block ``up`` that takes prev as its skip will build its
    concat operand in place (routes.concat_in_place, asked again by unet_forward's decoder) and the
    pooled operand is a stored one too; else None.  The concat tensor's other half is the transposed conv's."""
    hs, ws_, Cskip = prev.z.shape[1], prev.z.shape[2], prev.z.shape[3]
    Cup = up.up.out_channels
    Cout1 = _dc_layers(up.conv)[0].out_channels
    if not (routes.concat_in_place(bf16, N, h, w, up.up.in_channels, Cup, hs, ws_, Cskip, Cout1, prev.z.dtype == F32)
            and routes.pool_skip_ok(bf16, N, h, w, Cskip, Cout1)):
        return None   # (the decoder then builds its concat operand from u: the skip half would go unread)
    dev = prev.z.device
    dt = BF16S if bf16 else F32
    pooled = torch.empty(N, h, w, Cskip, dtype=dt, device=dev)
    xcat = torch.empty(N, hs, ws_, Cskip + Cup, dtype=dt, device=dev)
    L.call("pmu_frame_to_bf16_pool_skip" if bf16 else "pmu_frame_to_f32_pool_skip", frame_of(srcs, N, h, w),
           pooled.data_ptr(), xcat.data_ptr(), Cskip + Cup, L.stream())
    return pooled, xcat


def unet_forward(net, x: torch.Tensor, training: bool, bf16: bool = False, keep: bool = False):
    """Forward of model.UNet on the HIP path.  Returns (output, state).

    Output: NCHW logits / sigmoid(logits) when net.apply_last_layer, else the last
    DoubleConv activation as an NCHW-shaped channels-last tensor (unet_model.py:48-54).
    bf16: the 3x3 convs (except the Cin <= 4 first layer) and the ConvTranspose2d forward / input
    gradient (where their shapes allow) run on the bf16-MFMA kernels (autocast arithmetic; see
    include/pmunet_hip.h), the 3x3 weight gradients too.  keep: a backward follows (bf16 convs keep
    their operand copies for the weight gradient)."""
    assert x.is_cuda and x.dtype == F32 and x.dim() == 4
    dev = x.device
    N, Cin, H, W = x.shape
    st = UNetState()
    st.x = x
    # first layer reads NCHW planes directly (C == 1 is also NHWC)
    xc = x.contiguous()
    if Cin <= 4:
        planes = st.planes = [xc[:, c].contiguous() for c in range(Cin)]
        first_srcs = []
    else:
        planes = None
        first_srcs = [Src(xc.permute(0, 2, 3, 1).contiguous())]
    # ---- encoder
    c1w, b1, c2w, b2 = _dc_layers(net.inc)
    zb = bf16 and routes.effective().bf16_z
    o1 = conv_bn_forward(first_srcs, c1w, b1, N, H, W, training, dev, planes=planes, bf16=bf16, keep=keep, zb=zb)
    o2 = conv_bn_forward([o1.act()], c2w, b2, N, H, W, training, dev, bf16=bf16, keep=keep, zb=zb)
    st.enc.append((o1, o2))
    h, w = H, W
    nlev = len(net.down_blocks) + 1
    for down in net.down_blocks:
        dc = down.maxpool_conv[1]
        c1w, b1, c2w, b2 = _dc_layers(dc)
        prev = st.enc[-1][1]
        h, w = h // 2, w // 2
        srcs = [prev.act(L.POOL_MAX2)]
        pre = _pool_skip(net.up_blocks[nlev - 2 - (len(st.enc) - 1)], prev, srcs, N, h, w, bf16)
        if pre is not None:
            # the pooled operand and the Up block's concat operand (skip half) in one pass over prev
            srcs = [Src(pre[0])]
            st.xcat[len(st.enc) - 1] = pre[1]
        elif bf16 and routes.pooled_f32_first(N, h, w, prev.z.shape[3]):
            # fused bf16 fallback: the max-pooled activation materialised once, read raw by every
            # column block (the pipelined fused kernel has no pooled staging)
            pooled = _empty(N, h, w, prev.z.shape[3], device=dev)
            L.call("pmu_frame_to_f32", frame_of(srcs, N, h, w), pooled.data_ptr(), L.stream())
            srcs = [Src(pooled)]
        o1 = conv_bn_forward(srcs, c1w, b1, N, h, w, training, dev, bf16=bf16, keep=keep, zb=zb)
        o2 = conv_bn_forward([o1.act()], c2w, b2, N, h, w, training, dev, bf16=bf16, keep=keep, zb=zb)
        st.enc.append((o1, o2))
    # ---- decoder
    cur = st.enc[-1][1]
    nlev = len(st.enc)
    for j, up in enumerate(net.up_blocks):
        skip = st.enc[nlev - 2 - j][1]
        xpre = st.xcat.pop(nlev - 2 - j, None)
        hs, ws_ = skip.z.shape[1], skip.z.shape[2]
        hi, wi = cur.z.shape[1], cur.z.shape[2]
        convT = up.up
        Cup = convT.out_channels
        fin = frame_of([cur.act()], N, hi, wi)
        Cin_t = cur.z.shape[3]
        _check_channels(Cin_t, convT)
        xtT = None
        dY, dX = hs - 2 * hi, ws_ - 2 * wi
        assert dY >= 0 and dX >= 0, "decoder feature map larger than skip (unsupported by reference too)"
        off = (dY // 2, dX // 2)
        c1w, b1, c2w, b2 = _dc_layers(up.conv)
        Cskip = skip.z.shape[3]
        Ccat = Cskip + Cup
        # The concat operand built in place: the transposed conv writes its half (channels Cskip..) of
        # the materialised operand directly and only the skip half is copied (no u tensor, one pass over
        # it less) — when the halves need no F.pad and the conv will stage a materialised operand.
        in_place = routes.concat_in_place(bf16, N, hi, wi, Cin_t, Cup, hs, ws_, Cskip, c1w.out_channels,
                                          skip.z.dtype == F32)
        troute = routes.convT_fwd_route(bf16, in_place, N, hi, wi, Cin_t, Cup)
        if in_place:
            # (xpre: the encoder already wrote the skip half, with the next level's pooled operand)
            dt = BF16S if bf16 else F32
            ready = xpre is not None and xpre.shape == (N, hs, ws_, Ccat) and xpre.dtype == dt
            xcat = xpre if ready else torch.empty(N, hs, ws_, Ccat, dtype=dt, device=dev)
            u, srcs = None, [Src(xcat)]
        else:
            u = _empty(N, 2 * hi, 2 * wi, Cup, device=dev)
            srcs = [skip.act(), Src(u, L.SRC_RAW, off=off)]
        bias, s = L.ptr(convT.bias), L.stream()
        if troute in ("dma_ldb", "dma"):
            # the BN+ReLU operand written once in bf16 (the weight gradient's operand too), both GEMM
            # operands by LDS-DMA
            xtT = frame_to_bf16([cur.act()], N, hi, wi)
            wpt = pack_convT_weights_dma(convT.weight, dgrad=False)
            lead = (xtT.data_ptr(), xtT.shape[3], N, hi, wi, wpt.data_ptr(), bias, Cin_t, Cup)
            if in_place:
                L.call("pmu_convT2x2_fwd_dma_ldb", *lead, xcat.data_ptr() + 2 * Cskip, Ccat, s)
            else:
                L.call("pmu_convT2x2_fwd_dma", *lead, u.data_ptr(), s)
            if not keep:
                xtT = None
        elif troute == "ld":
            wpt = pack_convT_weights(convT.weight, dgrad=False)
            L.call("pmu_convT2x2_fwd_ld", fin, convT.weight.data_ptr(), wpt.data_ptr(), bias, Cup,
                   xcat.data_ptr() + 4 * Cskip, Ccat, s)
        else:
            wpt = pack_convT_weights(convT.weight, dgrad=False)
            L.call("pmu_convT2x2_fwd", frame_of(_f32_srcs([cur.act()], N, hi, wi), N, hi, wi),
                   convT.weight.data_ptr(), wpt.data_ptr(), bias, Cup, u.data_ptr(), s)
        if in_place and not ready:   # the skip half
            fsk = frame_of([skip.act()], N, hs, ws_)
            if bf16:
                L.call("pmu_frame_to_bf16_ld", fsk, Cskip, xcat.data_ptr(), Ccat, s)
            else:
                L.call("pmu_frame_to_f32_ld", fsk, xcat.data_ptr(), Ccat, s)
        o1 = conv_bn_forward(srcs, c1w, b1, N, hs, ws_, training, dev, bf16=bf16, keep=keep, zb=zb)
        o2 = conv_bn_forward([o1.act()], c2w, b2, N, hs, ws_, training, dev, bf16=bf16, keep=keep, zb=zb)
        st.ups.append(UpState(u=u, off=off, prev=cur, c1=o1, c2=o2, bf16=bf16, xt=xtT, cskip=Cskip))
        cur = o2
    st.feat_src = cur
    if net.apply_last_layer:
        K = net.outc.conv.out_channels
        _check_channels(cur.z.shape[3], net.outc.conv)
        y = _empty(N, K, H, W, device=dev)
        L.call("pmu_head1x1_fwd", frame_of([cur.act()], N, H, W), net.outc.conv.weight.data_ptr(),
               L.ptr(net.outc.conv.bias), K, int(net.n_classes == 1), y.data_ptr(), L.stream())
        st.y = y
        return y, st
    C = cur.z.shape[3]
    if cur.z.dtype != F32:
        return frame_to_f32([cur.act()], N, H, W).permute(0, 3, 1, 2), st
    feat = _empty(N, H, W, C, device=dev)
    L.call("pmu_bnrelu_apply", cur.z.data_ptr(), cur.bn.coef.data_ptr(), N * H * W, C, feat.data_ptr(), L.stream())
    return feat.permute(0, 3, 1, 2), st


def _maxpool_backward(prev: ConvBNOut, dpool, dsk, s):
    """MaxPool2d(2) backward (unet_parts.py:33) into the pooled layer ``prev``: returns its da = dsk (the
    skip path's gradient) + dpool routed to each window's maximum.  With batch statistics the same pass
    forms prev's BN-backward partial sums (prev.bnr), and under CFG.pool_fuse da stays unstored (PoolSumDa).
    The entry (routes.maxpool_bwd) follows the parts' storage; mixed storage runs on fp32 copies."""
    N, hp, wp, Cp = prev.z.shape
    dev = prev.z.device
    entry = routes.maxpool_bwd(Cp, prev.z.dtype == F32, prev.bn.mean is not None,
                               dpool.dtype == BF16S and dsk.dtype == BF16S, prev.bf16)
    bf = entry.endswith("_dxb")
    if not bf:
        if dpool.dtype == BF16S:
            dpool = frame_to_f32([Src(dpool)], N, hp // 2, wp // 2)
        if dsk.dtype == BF16S:
            dsk = frame_to_f32([Src(dsk)], N, hp, wp)
    if "_bnr" not in entry:
        L.call(entry, dpool.data_ptr(), prev.z.data_ptr(), prev.bn.coef.data_ptr(), N, hp, wp, Cp, dsk.data_ptr(), 1, s)
        return dsk
    R = L.lib().pmu_maxpool2_bwd_bnr_tiles(N, hp, wp, Cp)
    part = _empty(R, 2 * Cp, device=dev)
    stats = (prev.z.data_ptr(), prev.bn.coef.data_ptr(), prev.bn.mean.data_ptr(), prev.bn.invstd.data_ptr(),
             N, hp, wp, Cp)
    if "_stats" in entry:
        L.call(entry, dpool.data_ptr(), dsk.data_ptr(), *stats, part.data_ptr(), s)
        da = PoolSumDa(dpool, dsk, prev)
    elif bf:   # the parts' fp32 sum written to a new tensor
        da = _empty(N, hp, wp, Cp, device=dev)
        L.call(entry, dpool.data_ptr(), dsk.data_ptr(), *stats, da.data_ptr(), part.data_ptr(), s)
    else:      # routed into the skip gradient in place
        da = dsk
        L.call(entry, dpool.data_ptr(), *stats, da.data_ptr(), 1, part.data_ptr(), s)
    prev.bnr = (da, part, R)
    return da


def unet_backward(net, st: UNetState, dy: torch.Tensor, grads: GradSink | None = None) -> dict:
    """Backward of unet_forward given dL/d(output).  Returns {parameter: grad}."""
    grads = grads if grads is not None else GradSink()
    s = L.stream()
    dev = dy.device
    x = st.x
    N, _, H, W = x.shape
    last = st.feat_src
    if net.apply_last_layer:
        K = net.outc.conv.out_channels
        C = last.z.shape[3]
        dyc = dy.contiguous()
        lb = L.lib()
        head_bnr, head_fuse = routes.head_bwd(N, H, W, C, K, last.z.dtype == F32, last.bn.mean is not None, last.bf16)
        dl = None if head_fuse else _empty(N, K, H, W, device=dev)
        da = None if head_fuse else _empty(N, H, W, C, device=dev)
        dwo = grads.new(net.outc.conv.weight)
        dbo = grads.new(net.outc.conv.bias) if net.outc.conv.bias is not None else _empty(K, device=dev)
        wsb = lb.pmu_wgrad1x1_ws(N * H * W, K, C)
        ws = _empty(max(1, (wsb + 3) // 4), device=dev)
        if head_bnr:
            # one pass over z: the head's input gradient, its weight / bias gradient and the last
            # layer's BN-backward partial sums
            R = lb.pmu_head1x1_bwd_tiles(N, H, W)
            part = _empty(R, 2 * C, device=dev)
            L.call("pmu_head1x1_bwd_bnr", dyc.data_ptr(), st.y.data_ptr(), int(net.n_classes == 1),
                   net.outc.conv.weight.data_ptr(), K, C, N, H, W, None, L.ptr(da), last.z.data_ptr(),
                   last.bn.coef.data_ptr(), last.bn.mean.data_ptr(), last.bn.invstd.data_ptr(), part.data_ptr(),
                   dwo.data_ptr(), dbo.data_ptr(), ws.data_ptr(), wsb, s)
            if head_fuse:   # da unstored: the last layer's dz comes from dy (HeadDa)
                da = HeadDa(dyc, st.y, net.n_classes == 1, net.outc.conv.weight, K, last)
            last.bnr = (da, part, R)
        else:
            L.call("pmu_head1x1_bwd", dyc.data_ptr(), st.y.data_ptr(), int(net.n_classes == 1),
                   net.outc.conv.weight.data_ptr(), K, C, N, H, W, dl.data_ptr(), da.data_ptr(), s)
            L.call("pmu_wgrad1x1", dl.data_ptr(), frame_of([last.act()], N, H, W), K, dwo.data_ptr(), dbo.data_ptr(),
                   ws.data_ptr(), wsb, s)
        grads.flush()
    else:
        da = dy.permute(0, 2, 3, 1).contiguous()   # NCHW-shaped channels-last view -> NHWC

    nlev = len(st.enc)
    dskip = [None] * nlev
    # ---- decoder, last block first
    for j in reversed(range(len(net.up_blocks))):
        up = net.up_blocks[j]
        us: UpState = st.ups[j]
        c1w, b1, c2w, b2 = _dc_layers(up.conv)
        da1 = conv_bn_backward(us.c2, da, c2w, b2, grads, dx_bf16=True)
        grads.flush()
        Cskip = us.cskip
        convT = up.up
        prev = us.prev
        hi, wi, Cin_t = prev.z.shape[1], prev.z.shape[2], prev.z.shape[3]
        Cup = convT.out_channels
        tb = routes.convT_bwd(us.bf16, Cin_t, Cup, us.off)
        dsk, dup = conv_bn_backward(us.c1, da1, c1w, b1, grads, split=Cskip, x1_bf16_only=tb.dup_bf16_only,
                                    dx_bf16=True)
        x1, us.c1.x1 = us.c1.x1, None
        grads.flush()
        dskip[nlev - 2 - j] = dsk
        Hd, Wd = dup.shape[1], dup.shape[2]
        dx = _empty(N, hi, wi, Cin_t, dtype=BF16S if tb.dx_bf16 else F32, device=dev)
        # dup in bf16: dup itself (written in bf16 only, with column sums), the concat dgrad's bf16 copy when
        # it wrote one (pmu_conv3x3_dgrad_dma_x1b), else a pass over dup
        dbpart = x1.colsum if x1 is not None else None
        dut = None
        if us.bf16:
            dut = x1.bf16 if x1 is not None else frame_to_bf16([Src(dup)], N, Hd, Wd)
        if tb.dgrad == "dma":
            wpt = pack_convT_weights_dma(convT.weight, dgrad=True)
            L.call("pmu_convT2x2_dgrad_dma_dxb" if tb.dx_bf16 else "pmu_convT2x2_dgrad_dma", dut.data_ptr(),
                   dut.shape[3], Hd, Wd, us.off[0], us.off[1], wpt.data_ptr(), N, hi, wi, Cin_t, Cup, dx.data_ptr(), s)
        else:
            wpt = pack_convT_weights(convT.weight, dgrad=True)
            L.call("pmu_convT2x2_dgrad", dup.data_ptr(), Hd, Wd, us.off[0], us.off[1], convT.weight.data_ptr(),
                   wpt.data_ptr(), N, hi, wi, Cin_t, Cup, dx.data_ptr(), s)
        dwt = grads.new(convT.weight)
        dbt = grads.new(convT.bias) if convT.bias is not None else None
        if us.bf16:
            # bf16 operands materialised (the convT input after BN+ReLU, du); the bias gradient sums fp32 du
            xt = us.xt if us.xt is not None else frame_to_bf16([prev.act()], N, hi, wi)
            us.xt = None
            wsb = L.lib().pmu_convT2x2_wgrad_ws_bf16(N, hi, wi, Cin_t, Cup)
            ws = _empty(max(1, (wsb + 3) // 4), device=dev)
            if dbpart is not None:
                L.call("pmu_convT2x2_wgrad_bf16", xt.data_ptr(), dut.data_ptr(), None, N, hi, wi, Hd, Wd,
                       0, 0, Cin_t, Cup, dwt.data_ptr(), None, ws.data_ptr(), wsb, s)
                if dbt is not None:
                    part, R, sp = dbpart
                    wsd = _empty(L.lib().pmu_convT2x2_dbias_rows_ws(Cup) // 4, device=dev)
                    L.call("pmu_convT2x2_dbias_rows", part.data_ptr() + 4 * sp, R, part.shape[1], Cup,
                           dbt.data_ptr(), wsd.data_ptr(), s)
            else:
                L.call("pmu_convT2x2_wgrad_bf16", xt.data_ptr(), dut.data_ptr(), dup.data_ptr(), N, hi, wi, Hd, Wd,
                       us.off[0], us.off[1], Cin_t, Cup, dwt.data_ptr(), L.ptr(dbt), ws.data_ptr(), wsb, s)
            del xt, dut
        else:
            wsb = L.lib().pmu_convT2x2_wgrad_ws(N, hi, wi, Cin_t, Cup)
            ws = _empty(max(1, (wsb + 3) // 4), device=dev)
            L.call("pmu_convT2x2_wgrad", dup.data_ptr(), Hd, Wd, us.off[0], us.off[1],
                   frame_of(_f32_srcs([prev.act()], N, hi, wi), N, hi, wi), Cup, dwt.data_ptr(), L.ptr(dbt),
                   ws.data_ptr(), wsb, s)
        grads.flush()
        da = dx
    # ---- encoder, deepest first; da = gradient w.r.t. the deepest encoder output
    for lev in reversed(range(nlev)):
        o1, o2 = st.enc[lev]
        if lev == 0:
            c1w, b1, c2w, b2 = _dc_layers(net.inc)
        else:
            c1w, b1, c2w, b2 = _dc_layers(net.down_blocks[lev - 1].maxpool_conv[1])
        if lev != nlev - 1:
            da = dskip[lev]   # skip grad with the pooled path accumulated below
        da1 = conv_bn_backward(o2, da, c2w, b2, grads, dx_bf16=True)
        grads.flush()
        dpool = conv_bn_backward(o1, da1, c1w, b1, grads, need_dx=(lev > 0), dx_bf16=True)
        grads.flush()
        if lev > 0:
            dskip[lev - 1] = _maxpool_backward(st.enc[lev - 1][1], dpool, dskip[lev - 1], s)
            part = None   # (the head's partial sums, read long since: let go where they always were, at the first pool)
    return grads


def unet_report_order(net) -> list:
    """The parameter groups in the order unet_backward reports them (one GradSink.flush each): the
    head, then per up block (last first) conv2, conv1 and the ConvTranspose2d, then per encoder level
    (deepest first) conv2 and conv1 — within a conv layer BN weight, BN bias, conv bias, conv weight.
    This is the layout pmu_hip.dp learns from the first data-parallel step (and what the CPU tests
    of the bucket logic replay)."""
    def conv_group(conv, bn):
        return [p for p in (bn.weight, bn.bias, conv.bias, conv.weight) if p is not None]
    groups = []
    if net.apply_last_layer:
        groups.append([p for p in (net.outc.conv.weight, net.outc.conv.bias) if p is not None])
    for j in reversed(range(len(net.up_blocks))):
        up = net.up_blocks[j]
        c1w, b1, c2w, b2 = _dc_layers(up.conv)
        groups += [conv_group(c2w, b2), conv_group(c1w, b1),
                   [p for p in (up.up.weight, up.up.bias) if p is not None]]
    blocks = [net.inc] + [d.maxpool_conv[1] for d in net.down_blocks]
    for dc in reversed(blocks):
        c1w, b1, c2w, b2 = _dc_layers(dc)
        groups += [conv_group(c2w, b2), conv_group(c1w, b1)]
    return groups
