"""Signed distance maps of a batch of target planes, on the device (pmu_boundary_map): the field the boundary
loss (pmu_hip.loss.BoundaryLoss; Kervadec et al., MIDL 2019) multiplies the class probabilities with, formed per
step because the targets of a batch are sampled and warped on the fly.

For every image n and class k: 0 on the whole plane if the class has no pixel there or fills it; otherwise the
Euclidean distance (in pixels) to the nearest pixel of the class for a pixel outside it, and 1 - the distance to
the nearest pixel outside the class for a pixel of it — one_hot2dist of the paper's code.  Exact: squared
distances are integers, the square root is correctly rounded, so the map is bit-equal to the numpy restatement
tests/boundary_ref.py (include/pmunet_hip.h states the definition).
"""
from __future__ import annotations

import torch

from . import _lib as L

MAX_DIM = 1024      # PMU_SURFACE_MAX_DIM
MAX_CLASSES = 8     # pmu_hip.loss.SOFTDICE_MAX_CLASSES


def _workspace(N, K, H, W, device):
    return torch.empty(L.lib().pmu_boundary_ws(N, K, H, W) // 8, dtype=torch.float64, device=device)


def _map(tc: torch.Tensor, K: int, H: int, W: int, ignore_index: int, ws: torch.Tensor) -> torch.Tensor:
    """tc: the contiguous target, int64 (N, H, W) for K >= 2 or float32 (N, H, W) for K == 1."""
    N = tc.numel() // (H * W)
    phi = torch.empty(N, K, H, W, dtype=torch.float32, device=tc.device)
    L.call("pmu_boundary_map", tc.data_ptr(), 1 if K == 1 else 0, N, K, H, W, int(ignore_index), phi.data_ptr(),
           ws.data_ptr(), L.stream())
    return phi


def check_plane(what: str, K: int, H: int, W: int) -> None:
    if not 1 <= K <= MAX_CLASSES:
        raise ValueError(f"{what} supports at most {MAX_CLASSES} classes, got {K}")
    if not (1 <= H <= MAX_DIM and 1 <= W <= MAX_DIM):
        raise ValueError(f"{what}: plane {H} x {W} outside the kernel's range (1..{MAX_DIM} per side)")


def signed_distance(target: torch.Tensor, n_classes: int, ignore_index: int = -100) -> torch.Tensor:
    """The (N, K, H, W) float32 signed distance map of ``target``: (N, H, W) class indices for ``n_classes`` >= 2
    (a pixel equal to ``ignore_index`` belongs to no class), or an (N, 1, H, W) / (N, H, W) float mask for one
    class (a member where the mask is >= 0.5).  Negative inside a class, positive outside, 0 on a plane the
    class is absent from or fills.  Nothing synchronises with the host."""
    if not isinstance(target, torch.Tensor) or not target.is_cuda:
        raise RuntimeError("signed_distance runs on the MI355X HIP path only (there is no CPU fallback)")
    K = int(n_classes)
    if K == 1 and target.dim() == 4 and target.shape[1] == 1:
        target = target[:, 0]
    if target.dim() != 3 or target.numel() == 0:
        raise ValueError(f"signed_distance: target {tuple(target.shape)} is not (N, H, W)")
    if K > 1 and target.is_floating_point():
        raise ValueError("signed_distance: n_classes >= 2 takes class-index targets")
    N, H, W = target.shape
    check_plane("signed_distance", K, H, W)
    tc = target.detach().contiguous()
    tc = tc.float() if K == 1 else tc.long()
    return _map(tc, K, H, W, ignore_index, _workspace(N, K, H, W, tc.device))
