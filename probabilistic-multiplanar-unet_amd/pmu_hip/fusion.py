"""Three-view volume fusion on the HIP path (row a14): PMU/eval.py:157-203.

The reference concatenates per-slice softmax outputs per view, permutes views 1 and 2 into the
view-0 frame (permute(2,1,0,3) / permute(2,1,3,0)), averages the three volumes, and scores each
of the four volumes with per-class Dice of the argmax one-hot (eval.py:42-49).  Here the per-view
stacks are written by the predictor straight into their final buffers and ONE kernel
(pmu_fuse3view) reads each prediction once: softmax (optional), transposition, average, argmax
label map and exact Dice counts for all four volumes.

Views along arbitrary vectors (MRI_Dataset(views=...)) are fused by fuse_oblique: one kernel
(pmu_fuse_oblique) resamples every view's probability stack onto the voxel grid, averages the views
that cover each voxel and scores every view and the average the same way.

Learned fusion (DESIGN.md "Learned fusion"): with ``weights`` (a FusionWeights) both functions fuse with
per-view, per-class weights and a per-class bias instead of the plain mean — z_c = b_c + sum_v W[v,c] p_{v,c},
fused = softmax(z) — through pmu_fusion3_eval / pmu_fusion_oblique_eval, and fit_fusion fits those weights on
held-out scans: a full-batch softmax regression whose every function evaluation is one kernel pass per scan
(loss and gradient sums, reproducible bit for bit), minimised on the host by a deterministic L-BFGS.
"""
from __future__ import annotations

import ctypes
from dataclasses import dataclass, field

import numpy as np
import torch

from . import _lib as L
from .metrics import dice_from_counts

VOLUMES = ("view0", "view1", "view2", "average")
FUSE_CMAX, FUSE_VMAX = 8, 8


@dataclass
class FusionWeights:
    """The fusion model: W (V,C) float64 per-view, per-class weights, b (C,) float64 per-class bias, and for
    oblique views the (V,3,3) frames they were fitted for (None: the three standard axes)."""
    W: np.ndarray
    b: np.ndarray
    frames: np.ndarray | None = None

    def __post_init__(self):
        self.W = np.ascontiguousarray(self.W, dtype=np.float64)
        self.b = np.ascontiguousarray(self.b, dtype=np.float64)
        if self.W.ndim != 2 or self.b.shape != (self.W.shape[1],):
            raise ValueError(f"fusion weights W {self.W.shape} and b {self.b.shape} are not (V,C) and (C,)")
        if self.frames is not None:
            self.frames = np.ascontiguousarray(self.frames, dtype=np.float64).reshape(-1, 3, 3)
            if self.frames.shape[0] != self.W.shape[0]:
                raise ValueError(f"{self.frames.shape[0]} frames for {self.W.shape[0]} views' weights")

    @property
    def V(self) -> int:
        return self.W.shape[0]

    @property
    def C(self) -> int:
        return self.W.shape[1]

    @classmethod
    def uniform(cls, V: int, C: int, frames=None) -> "FusionWeights":
        """W = 1/V, b = 0: z is the plain mean of the views."""
        return cls(np.full((V, C), 1.0 / V), np.zeros(C), frames)

    def theta(self) -> np.ndarray:
        """The parameter vector of the kernels and of the fit: W row by row, then b."""
        return np.concatenate([self.W.ravel(), self.b])

    @classmethod
    def from_theta(cls, theta, V: int, C: int, frames=None) -> "FusionWeights":
        theta = np.asarray(theta, dtype=np.float64)
        return cls(theta[:V * C].reshape(V, C).copy(), theta[V * C:].copy(), frames)

    def save(self, path) -> None:
        arrays = {"W": self.W, "b": self.b}
        if self.frames is not None:
            arrays["frames"] = self.frames
        with open(path, "wb") as f:      # (np.savez on a name would append ".npz")
            np.savez(f, **arrays)

    @classmethod
    def load(cls, path) -> "FusionWeights":
        with np.load(path, allow_pickle=False) as z:
            return cls(z["W"], z["b"], z["frames"] if "frames" in z.files else None)

    def check_frames(self, frames) -> None:
        """Refuse oblique weights on views other than those they were fitted for (and the reverse)."""
        if frames is None:
            if self.frames is not None:
                raise ValueError("these fusion weights were fitted for oblique views, not for the standard axes")
            return
        frames = np.asarray(frames, dtype=np.float64).reshape(-1, 3, 3)
        if self.frames is None:
            raise ValueError("these fusion weights were fitted for the standard axes, not for oblique views")
        if self.frames.shape != frames.shape or not np.array_equal(self.frames, frames):
            raise ValueError("these fusion weights were fitted for other view frames than the dataset's")


def _doubles(a):
    a = np.ascontiguousarray(a, dtype=np.float64).ravel()
    return (ctypes.c_double * a.size)(*a.tolist())


def _class_weight(class_weight, C):
    """None, or the (C,) float64 loss weights of the classes."""
    if class_weight is None:
        return None
    cw = np.asarray(class_weight, dtype=np.float64)
    if cw.shape != (C,) or not np.all(np.isfinite(cw)) or np.any(cw < 0):
        raise ValueError(f"class_weight must be {C} finite non-negative numbers, got {class_weight!r}")
    return cw


def _check_weights(weights, V, C):
    if C < 2:
        raise ValueError("the learned fusion is a softmax over the classes: it needs C >= 2 (C = 1 has no fusion model)")
    if C > FUSE_CMAX:
        raise ValueError(f"the learned fusion takes at most {FUSE_CMAX} classes, got {C}")
    if (weights.V, weights.C) != (V, C):
        raise ValueError(f"fusion weights for {weights.V} views x {weights.C} classes on {V} views x {C} classes")


def _sums_out(V, C, dev):
    return torch.empty(2 + C + V * C, dtype=torch.float64, device=dev)


def fuse_views(v0: torch.Tensor, v1: torch.Tensor, v2: torch.Tensor, truth: torch.Tensor, logits: bool = False,
               want_avg: bool = True, want_label: bool = True, weights: FusionWeights | None = None,
               class_weight=None) -> dict:
    """v0 (D0,C,D1,D2), v1 (D1,C,D0,D2), v2 (D2,C,D0,D1) per-view stacks; truth (D0,D1,D2) labels.

    Returns {'avg': (D0,C,D1,D2) or None, 'label': (D0,D1,D2) int32 or None,
             'counts': (4,C,3) float64, 'dice': (4,C) float32} — dice[v][c] is eval.py's
    dice(volume_v, truth, c) for v in VOLUMES.

    ``weights`` (a FusionWeights for 3 views; C >= 2): the learned fusion in place of the plain mean — 'avg' holds
    the fused softmax probabilities, 'label' their first maximum, the last row of 'counts' / 'dice' scores that
    label (the per-view rows are unchanged), and the result gains 'loss', the ``class_weight``-weighted mean
    cross-entropy of the fused softmax against truth, sum l / sum w of pmu_fusion3_eval (a float64 scalar on the
    device)."""
    for t in (v0, v1, v2, truth):
        if not t.is_cuda:
            raise RuntimeError("fuse_views runs on the MI355X HIP path only (there is no CPU fallback)")
    D0, C, D1, D2 = v0.shape
    if tuple(v1.shape) != (D1, C, D0, D2) or tuple(v2.shape) != (D2, C, D0, D1):
        raise ValueError(f"view stacks do not describe one volume: {tuple(v0.shape)}, {tuple(v1.shape)}, "
                         f"{tuple(v2.shape)}")
    if weights is not None:
        _check_weights(weights, 3, C)
        weights.check_frames(None)
    dev = v0.device
    tr = truth.reshape(D0, D1, D2).float().contiguous()
    a = [t.float().contiguous() for t in (v0, v1, v2)]
    avg = torch.empty(D0, C, D1, D2, dtype=torch.float32, device=dev) if want_avg else None
    label = torch.empty(D0, D1, D2, dtype=torch.int32, device=dev) if want_label else None
    counts = torch.empty(4, C, 3, dtype=torch.float64, device=dev)
    if weights is None:
        L.call("pmu_fuse3view", a[0].data_ptr(), a[1].data_ptr(), a[2].data_ptr(), tr.data_ptr(), D0, D1, D2, C,
               int(bool(logits)), L.ptr(avg), L.ptr(label), counts.data_ptr(), L.stream())
        return {"avg": avg, "label": label, "counts": counts, "dice": dice_from_counts(counts)}
    cw = _class_weight(class_weight, C)
    sums = _sums_out(3, C, dev)
    nbytes = int(L.lib().pmu_fusion3_ws(D0, D1, D2, C))
    ws = torch.empty(nbytes // 8, dtype=torch.float64, device=dev)
    L.call("pmu_fusion3_eval", a[0].data_ptr(), a[1].data_ptr(), a[2].data_ptr(), tr.data_ptr(), D0, D1, D2, C,
           int(bool(logits)), _doubles(weights.theta()), None if cw is None else _doubles(cw), L.ptr(avg), L.ptr(label),
           counts.data_ptr(), sums.data_ptr(), 0, ws.data_ptr(), nbytes, L.stream())
    return {"avg": avg, "label": label, "counts": counts, "dice": dice_from_counts(counts), "loss": sums[1] / sums[0]}


def oblique_volumes(V: int) -> tuple:
    """Names of fuse_oblique's V + 1 scored volumes."""
    return tuple(f"view{v}" for v in range(V)) + ("average",)


def fuse_oblique(stacks, frames, truth: torch.Tensor, sample_dim: int, spacing: float = 1.0, want_avg: bool = True,
                 want_label: bool = True, weights: FusionWeights | None = None, class_weight=None) -> dict:
    """Fusion of V (1..8) oblique views (DESIGN.md "Oblique views"; pmu_fuse_oblique).

    stacks: (V,P,C,P,P) probabilities, or a list of V (P,C,P,P) stacks (copied into one buffer);
    frames: (V,3,3) float64 rows (n,u,v) of each view (utils.mri_dataset.view_frame); truth (p0,p1,p2)
    labels; P = sample_dim, spacing in voxels.  Every view's prediction is resampled trilinearly onto the
    voxel grid and the views covering a voxel are averaged.

    Returns {'avg': (p0,C,p1,p2) or None, 'label': (p0,p1,p2) int32 or None, 'cover': (p0,p1,p2) int32
    (views covering each voxel), 'counts': (V+1,C,3) float64, 'dice': (V+1,C) float32} — the volumes are
    oblique_volumes(V) = view0..view{V-1}, average.

    ``weights`` (a FusionWeights for these V frames; C >= 2): the learned fusion over the views covering each
    voxel in place of their mean (pmu_fusion_oblique_eval) — 'avg', 'label', the last row of 'counts' / 'dice' and
    the new key 'loss' as in fuse_views; a voxel no view covers keeps probability 0 and label 0 and
    does not enter the loss."""
    if not isinstance(stacks, torch.Tensor):
        stacks = torch.stack([s.float() for s in stacks])
    for t in (stacks, truth):
        if not t.is_cuda:
            raise RuntimeError("fuse_oblique runs on the MI355X HIP path only (there is no CPU fallback)")
    P = int(sample_dim)
    if stacks.dim() != 5:
        raise ValueError(f"expected (V,P,C,P,P) stacks, got {tuple(stacks.shape)}")
    V, C = stacks.shape[0], stacks.shape[2]
    if tuple(stacks.shape) != (V, P, C, P, P):
        raise ValueError(f"view stacks {tuple(stacks.shape)} are not (V,P,C,P,P) for sample_dim {P}")
    if truth.dim() != 3:
        raise ValueError(f"expected a (p0,p1,p2) truth volume, got {tuple(truth.shape)}")
    dev = stacks.device
    fr = torch.as_tensor(frames, dtype=torch.float64).reshape(-1, 9).contiguous().to(dev)
    if fr.shape[0] != V:
        raise ValueError(f"{fr.shape[0]} frames for {V} view stacks")
    if weights is not None:
        _check_weights(weights, V, C)
        weights.check_frames(np.asarray(torch.as_tensor(frames, dtype=torch.float64).cpu()))
    p0, p1, p2 = truth.shape
    tr = truth.float().contiguous()
    st = stacks.float().contiguous()
    avg = torch.empty(p0, C, p1, p2, dtype=torch.float32, device=dev) if want_avg else None
    label = torch.empty(p0, p1, p2, dtype=torch.int32, device=dev) if want_label else None
    cover = torch.empty(p0, p1, p2, dtype=torch.int32, device=dev)
    counts = torch.empty(V + 1, C, 3, dtype=torch.float64, device=dev)
    if weights is None:
        L.call("pmu_fuse_oblique", st.data_ptr(), fr.data_ptr(), V, C, P, float(spacing), tr.data_ptr(), p0, p1, p2,
               L.ptr(avg), L.ptr(label), cover.data_ptr(), counts.data_ptr(), L.stream())
        return {"avg": avg, "label": label, "cover": cover, "counts": counts, "dice": dice_from_counts(counts)}
    cw = _class_weight(class_weight, C)
    sums = _sums_out(V, C, dev)
    nbytes = int(L.lib().pmu_fusion_oblique_ws(V, C, p0, p1, p2))
    ws = torch.empty(nbytes // 8, dtype=torch.float64, device=dev)
    L.call("pmu_fusion_oblique_eval", st.data_ptr(), fr.data_ptr(), V, C, P, float(spacing), tr.data_ptr(), p0, p1, p2,
           _doubles(weights.theta()), None if cw is None else _doubles(cw), L.ptr(avg), L.ptr(label), cover.data_ptr(),
           counts.data_ptr(), sums.data_ptr(), 0, ws.data_ptr(), nbytes, L.stream())
    return {"avg": avg, "label": label, "cover": cover, "counts": counts, "dice": dice_from_counts(counts),
            "loss": sums[1] / sums[0]}


# ------------------------------------------------------------------------------------------ the fit
class FusionItem:
    """One fitting scan: its resident per-view stacks and truth, standard (three stacks in fuse_views' layouts,
    ``logits`` as there) or oblique (``frames`` given: fuse_oblique's stacks, sample_dim and spacing)."""

    def __init__(self, stacks, truth, logits: bool = False, frames=None, sample_dim=None, spacing: float = 1.0):
        self.oblique = frames is not None
        if self.oblique:
            if not isinstance(stacks, torch.Tensor):
                stacks = torch.stack([s.float() for s in stacks])
            if not (stacks.is_cuda and truth.is_cuda):
                raise RuntimeError("the fusion fit runs on the MI355X HIP path only (there is no CPU fallback)")
            P = int(sample_dim if sample_dim is not None else stacks.shape[1])
            if stacks.dim() != 5 or tuple(stacks.shape) != (stacks.shape[0], P, stacks.shape[2], P, P):
                raise ValueError(f"view stacks {tuple(stacks.shape)} are not (V,P,C,P,P) for sample_dim {P}")
            if truth.dim() != 3:
                raise ValueError(f"expected a (p0,p1,p2) truth volume, got {tuple(truth.shape)}")
            self.V, self.C, self.P, self.h = stacks.shape[0], stacks.shape[2], P, float(spacing)
            self.frames = np.ascontiguousarray(torch.as_tensor(frames, dtype=torch.float64).cpu().numpy()).reshape(-1, 3, 3)
            if self.frames.shape[0] != self.V:
                raise ValueError(f"{self.frames.shape[0]} frames for {self.V} view stacks")
            self.fr = torch.from_numpy(self.frames.reshape(-1, 9)).to(stacks.device)
            self.stacks = stacks.float().contiguous()
            self.truth = truth.float().contiguous()
            self.shape = tuple(truth.shape)
            self.ws_bytes = int(L.lib().pmu_fusion_oblique_ws(self.V, self.C, *self.shape)) if self.C >= 2 else 0
        else:
            v0, v1, v2 = stacks
            for t in (v0, v1, v2, truth):
                if not t.is_cuda:
                    raise RuntimeError("the fusion fit runs on the MI355X HIP path only (there is no CPU fallback)")
            D0, C, D1, D2 = v0.shape
            if tuple(v1.shape) != (D1, C, D0, D2) or tuple(v2.shape) != (D2, C, D0, D1):
                raise ValueError(f"view stacks do not describe one volume: {tuple(v0.shape)}, {tuple(v1.shape)}, "
                                 f"{tuple(v2.shape)}")
            self.V, self.C, self.frames, self.logits = 3, C, None, bool(logits)
            self.stacks = [t.float().contiguous() for t in (v0, v1, v2)]
            self.truth = truth.reshape(D0, D1, D2).float().contiguous()
            self.shape = (D0, D1, D2)
            self.ws_bytes = int(L.lib().pmu_fusion3_ws(D0, D1, D2, C)) if C >= 2 else 0
        self.device = self.truth.device

    def add_sums(self, theta, cw, sums: torch.Tensor, accumulate: bool, ws: torch.Tensor) -> None:
        """One fit-mode kernel pass: this scan's loss and gradient sums stored in (or added to) ``sums``."""
        par, cwp = _doubles(theta), None if cw is None else _doubles(cw)
        if self.oblique:
            L.call("pmu_fusion_oblique_eval", self.stacks.data_ptr(), self.fr.data_ptr(), self.V, self.C, self.P, self.h,
                   self.truth.data_ptr(), *self.shape, par, cwp, None, None, None, None, sums.data_ptr(),
                   int(accumulate), ws.data_ptr(), self.ws_bytes, L.stream())
        else:
            L.call("pmu_fusion3_eval", self.stacks[0].data_ptr(), self.stacks[1].data_ptr(), self.stacks[2].data_ptr(),
                   self.truth.data_ptr(), *self.shape, self.C, int(self.logits), par, cwp, None, None, None,
                   sums.data_ptr(), int(accumulate), ws.data_ptr(), self.ws_bytes, L.stream())


@dataclass
class FusionFit:
    """fit_fusion's result: the fitted weights, the objective before and after (mean weighted cross-entropy plus
    the l2 term), the final gradient's largest component, iterations, function evaluations (one kernel pass per
    scan each), whether ||g||inf < gtol was reached, and the objective after every iteration."""
    weights: FusionWeights
    loss_initial: float
    loss: float
    grad_norm: float
    iterations: int
    evaluations: int
    converged: bool
    history: list = field(default_factory=list)


def lbfgs_minimize(fun, x0, gtol: float, max_iter: int, memory: int = 10):
    """Deterministic L-BFGS on the host in float64: two-loop recursion over the last ``memory`` pairs, Armijo
    backtracking (c1 = 1e-4, halving), a steepest-descent restart when the direction is not a descent direction or
    the line search fails on it.  fun(x) -> (f, g).  Returns (x, f, g, iterations, evaluations, converged, history).
    The Armijo test allows a rise of a few ulp of f: near the optimum the true decrease (~ ||g||^2) is below the
    rounding of f itself, and the gradient, not f, decides convergence."""
    x = np.array(x0, dtype=np.float64)
    f, g = fun(x)
    evals, hist = 1, [float(f)]
    S, Y = [], []
    it = 0
    converged = float(np.max(np.abs(g))) < gtol
    while not converged and it < max_iter:
        q = g.copy()
        alphas = []
        for s, y in zip(reversed(S), reversed(Y)):
            a = float(s @ q) / float(y @ s)
            alphas.append(a)
            q -= a * y
        if S:
            q *= float(S[-1] @ Y[-1]) / float(Y[-1] @ Y[-1])
        for (s, y), a in zip(zip(S, Y), reversed(alphas)):
            q += (a - float(y @ q) / float(y @ s)) * s
        d = -q
        first = not S
        if not float(g @ d) < 0.0:
            d, S, Y, first = -g, [], [], True
        while True:
            gd = float(g @ d)
            step = min(1.0, 1.0 / float(np.max(np.abs(g)))) if first else 1.0
            slack = 4.0 * np.finfo(np.float64).eps * max(1.0, abs(float(f)))
            ok = False
            for _ in range(40):
                xn = x + step * d
                fn, gn = fun(xn)
                evals += 1
                if np.isfinite(fn) and fn <= f + 1e-4 * step * gd + slack:
                    ok = True
                    break
                step *= 0.5
            if ok or first:
                break
            d, S, Y, first = -g, [], [], True      # the quasi-Newton direction failed: steepest descent once
        if not ok:
            break
        s, y = xn - x, gn - g
        if float(s @ y) > 1e-12 * float(np.sqrt((s @ s) * (y @ y))):   # keep the inverse Hessian positive definite
            S.append(s)
            Y.append(y)
            if len(S) > memory:
                S.pop(0)
                Y.pop(0)
        x, f, g = xn, fn, gn
        it += 1
        hist.append(float(f))
        converged = float(np.max(np.abs(g))) < gtol
    return x, float(f), g, it, evals, converged, hist


def balanced_class_weight(truths, C: int) -> np.ndarray:
    """cw_c = N / (C N_c) over the voxels with a label in [0, C) of the given truth volumes; 0 for an absent class."""
    n = np.zeros(C, dtype=np.float64)
    for t in truths:
        lab = t.reshape(-1).to(torch.int64)
        lab = lab[(lab >= 0) & (lab < C)]
        n += torch.bincount(lab, minlength=C)[:C].cpu().numpy().astype(np.float64)
    return np.where(n > 0, n.sum() / (C * np.maximum(n, 1.0)), 0.0)


def fit_fusion(items, *, class_weight=None, l2: float = 0.0, gtol: float = 1e-6, max_iter: int = 100,
               init: FusionWeights | None = None) -> FusionFit:
    """Fit the fusion model on ``items`` (FusionItem, all standard or all oblique along the same frames): minimise
    sum l / sum w over every voxel of every item (the class-weighted mean cross-entropy of the fused softmax) plus
    l2 / 2 ||theta - theta_init||^2, theta = (W, b).  The objective is convex.  Every function evaluation is one
    kernel pass per item, summed on the device in item order and read back once; the minimiser is lbfgs_minimize.

    class_weight: None (ones), "balanced" (balanced_class_weight of the items' truths) or C weights.
    init: the starting point and the centre of the l2 term (default FusionWeights.uniform)."""
    items = list(items)
    if not items:
        raise ValueError("fit_fusion needs at least one item")
    it0 = items[0]
    V, C = it0.V, it0.C
    for it in items:
        if (it.V, it.C, it.oblique) != (V, C, it0.oblique):
            raise ValueError("the fitting items do not share views and classes")
        if it.oblique and not np.array_equal(it.frames, it0.frames):
            raise ValueError("the fitting items were predicted along different view frames")
    if init is None:
        init = FusionWeights.uniform(V, C, it0.frames)
    _check_weights(init, V, C)
    init.check_frames(it0.frames)
    if isinstance(class_weight, str):
        if class_weight != "balanced":
            raise ValueError(f"class_weight {class_weight!r}: None, 'balanced' or {C} weights")
        cw = balanced_class_weight([it.truth for it in items], C)
    else:
        cw = _class_weight(class_weight, C)
    if l2 < 0 or gtol <= 0 or max_iter < 0:
        raise ValueError("fit_fusion needs l2 >= 0, gtol > 0 and max_iter >= 0")
    dev = it0.device
    sums = _sums_out(V, C, dev)
    ws = torch.empty(max(it.ws_bytes for it in items) // 8, dtype=torch.float64, device=dev)
    theta0 = init.theta()

    def fun(theta):
        for n, it in enumerate(items):
            it.add_sums(theta, cw, sums, n > 0, ws)
        s = sums.cpu().numpy()
        if not s[0] > 0:
            raise ValueError("no voxel with a positive fit weight in the fitting items")
        d = theta - theta0
        f = s[1] / s[0] + 0.5 * l2 * float(d @ d)
        g = np.concatenate([s[2 + C:], s[2:2 + C]]) / s[0] + l2 * d
        return float(f), g

    x, f, g, iters, evals, conv, hist = lbfgs_minimize(fun, theta0, gtol, max_iter)
    return FusionFit(FusionWeights.from_theta(x, V, C, it0.frames), hist[0], f, float(np.max(np.abs(g))), iters, evals,
                     conv, hist)
