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
"""
from __future__ import annotations

import torch

from . import _lib as L
from .metrics import dice_from_counts

VOLUMES = ("view0", "view1", "view2", "average")


def fuse_views(v0: torch.Tensor, v1: torch.Tensor, v2: torch.Tensor, truth: torch.Tensor, logits: bool = False,
               want_avg: bool = True, want_label: bool = True) -> dict:
    """v0 (D0,C,D1,D2), v1 (D1,C,D0,D2), v2 (D2,C,D0,D1) per-view stacks; truth (D0,D1,D2) labels.

    Returns {'avg': (D0,C,D1,D2) or None, 'label': (D0,D1,D2) int32 or None,
             'counts': (4,C,3) float64, 'dice': (4,C) float32} — dice[v][c] is eval.py's
    dice(volume_v, truth, c) for v in VOLUMES."""
    for t in (v0, v1, v2, truth):
        if not t.is_cuda:
            raise RuntimeError("fuse_views runs on the MI355X HIP path only (there is no CPU fallback)")
    D0, C, D1, D2 = v0.shape
    if tuple(v1.shape) != (D1, C, D0, D2) or tuple(v2.shape) != (D2, C, D0, D1):
        raise ValueError(f"view stacks do not describe one volume: {tuple(v0.shape)}, {tuple(v1.shape)}, "
                         f"{tuple(v2.shape)}")
    dev = v0.device
    tr = truth.reshape(D0, D1, D2).float().contiguous()
    a = [t.float().contiguous() for t in (v0, v1, v2)]
    avg = torch.empty(D0, C, D1, D2, dtype=torch.float32, device=dev) if want_avg else None
    label = torch.empty(D0, D1, D2, dtype=torch.int32, device=dev) if want_label else None
    counts = torch.empty(4, C, 3, dtype=torch.float64, device=dev)
    L.call("pmu_fuse3view", a[0].data_ptr(), a[1].data_ptr(), a[2].data_ptr(), tr.data_ptr(), D0, D1, D2, C,
           int(bool(logits)), L.ptr(avg), L.ptr(label), counts.data_ptr(), L.stream())
    return {"avg": avg, "label": label, "counts": counts, "dice": dice_from_counts(counts)}


def oblique_volumes(V: int) -> tuple:
    """Names of fuse_oblique's V + 1 scored volumes."""
    return tuple(f"view{v}" for v in range(V)) + ("average",)


def fuse_oblique(stacks, frames, truth: torch.Tensor, sample_dim: int, spacing: float = 1.0, want_avg: bool = True,
                 want_label: bool = True) -> dict:
    """Fusion of V (1..8) oblique views (DESIGN.md "Oblique views"; pmu_fuse_oblique).

    stacks: (V,P,C,P,P) probabilities, or a list of V (P,C,P,P) stacks (copied into one buffer);
    frames: (V,3,3) float64 rows (n,u,v) of each view (utils.mri_dataset.view_frame); truth (p0,p1,p2)
    labels; P = sample_dim, spacing in voxels.  Every view's prediction is resampled trilinearly onto the
    voxel grid and the views covering a voxel are averaged.

    Returns {'avg': (p0,C,p1,p2) or None, 'label': (p0,p1,p2) int32 or None, 'cover': (p0,p1,p2) int32
    (views covering each voxel), 'counts': (V+1,C,3) float64, 'dice': (V+1,C) float32} — the volumes are
    oblique_volumes(V) = view0..view{V-1}, average."""
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
    p0, p1, p2 = truth.shape
    tr = truth.float().contiguous()
    st = stacks.float().contiguous()
    avg = torch.empty(p0, C, p1, p2, dtype=torch.float32, device=dev) if want_avg else None
    label = torch.empty(p0, p1, p2, dtype=torch.int32, device=dev) if want_label else None
    cover = torch.empty(p0, p1, p2, dtype=torch.int32, device=dev)
    counts = torch.empty(V + 1, C, 3, dtype=torch.float64, device=dev)
    L.call("pmu_fuse_oblique", st.data_ptr(), fr.data_ptr(), V, C, P, float(spacing), tr.data_ptr(), p0, p1, p2,
           L.ptr(avg), L.ptr(label), cover.data_ptr(), counts.data_ptr(), L.stream())
    return {"avg": avg, "label": label, "cover": cover, "counts": counts, "dice": dice_from_counts(counts)}
