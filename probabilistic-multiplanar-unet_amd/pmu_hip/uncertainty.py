"""Sample-diversity metrics of the Probabilistic U-Net: the generalised energy distance (Kohl et al.
2018, https://arxiv.org/abs/1806.05034) between the sampled segmentations S and the ground truths Y,

    GED^2 = 2 E[d(S, Y)] - E[d(S, S')] - E[d(Y, Y')],        d(a, b) = 1 - mean_c IoU_c(a, b),

expectations over all ordered pairs (the diagonal included), the IoU averaged over the foreground classes
c = 1..K-1 present in either map (K = 1: the single class), d = 0 when none is.  Every IoU follows from
integer overlap counts, so the label maps are reduced on the GPU by one kernel (pmu_label_pair_counts: no
one-hot tensors) and the distance itself is a few float64 operations on (N,R,R,K) counts, on any device.
The per-sample label maps come from ProbabilisticUnet.sample_stats(n, labels=True).
"""
from __future__ import annotations

import torch

from . import _lib as L

MAX_MAPS, MAX_CLASSES = 64, 32
MAX_COUNTERS = 8192   # PMU_LABEL_PAIRS_MAX_COUNTERS: R (R + 1) / 2 * K


def _u8(t: torch.Tensor) -> torch.Tensor:
    """Labels as uint8; a value outside [0, 255] becomes 255 (>= any class count: counted nowhere)."""
    if t.dtype == torch.uint8:
        return t
    return torch.where((t < 0) | (t > 255), torch.full_like(t, 255), t).to(torch.uint8)


def label_pair_counts(maps: torch.Tensor, n_classes: int):
    """maps (R,N,...) integer label maps of the same N images -> (inter (N,R,R,K), cnt (N,R,K)) float64 exact
    counts: inter[n,i,j,c] pixels where maps i and j both have label c, cnt[n,i,c] pixels of label c in map i.
    Labels >= n_classes count nowhere."""
    if not maps.is_cuda:
        raise RuntimeError("label_pair_counts runs on the MI355X HIP path only (there is no CPU fallback)")
    if maps.dim() < 3:
        raise ValueError(f"expected (R,N,...) label maps, got {tuple(maps.shape)}")
    R, N = maps.shape[0], maps.shape[1]
    K = int(n_classes)
    if not (1 <= R <= MAX_MAPS and 1 <= K <= MAX_CLASSES and R * (R + 1) // 2 * K <= MAX_COUNTERS):
        raise ValueError(f"label_pair_counts: {R} maps x {K} classes outside the kernel's range (R <= {MAX_MAPS}, "
                         f"K <= {MAX_CLASSES}, R (R + 1) / 2 * K <= {MAX_COUNTERS})")
    m = _u8(maps.reshape(R, N, -1)).contiguous()
    HW = m.shape[2]
    inter = torch.empty(N, R, R, K, dtype=torch.float64, device=maps.device)
    cnt = torch.empty(N, R, K, dtype=torch.float64, device=maps.device)
    L.call("pmu_label_pair_counts", m.data_ptr(), R, N, HW, K, inter.data_ptr(), cnt.data_ptr(), L.stream())
    return inter, cnt


def pair_distances(inter, cnt) -> torch.Tensor:
    """d[n,i,j] = 1 - mean IoU over the foreground classes present in map i or map j (0 when none is)."""
    inter = torch.as_tensor(inter, dtype=torch.float64)
    cnt = torch.as_tensor(cnt, dtype=torch.float64, device=inter.device)
    K = cnt.shape[-1]
    c0 = 1 if K > 1 else 0
    it = inter[..., c0:]
    total = cnt[:, :, None, c0:] + cnt[:, None, :, c0:]
    present = total > 0
    iou = torch.where(present, it / (total - it).clamp_min(1.0), torch.zeros_like(it))
    npres = present.sum(-1)
    miou = iou.sum(-1) / npres.clamp_min(1)
    return torch.where(npres > 0, 1.0 - miou, torch.zeros_like(miou))


def ged_from_counts(inter, cnt, S: int) -> torch.Tensor:
    """Per-image GED^2 (float64, (N,)) from label_pair_counts of R = S + M maps: the first S are samples,
    the remaining M >= 1 ground truths."""
    d = pair_distances(inter, cnt)
    R = d.shape[1]
    if not 1 <= S < R:
        raise ValueError(f"{S} samples among {R} maps: need at least one sample and one ground truth")
    return 2.0 * d[:, :S, S:].mean((1, 2)) - d[:, :S, :S].mean((1, 2)) - d[:, S:, S:].mean((1, 2))


def ged(sample_labels: torch.Tensor, truths: torch.Tensor, n_classes: int) -> torch.Tensor:
    """GED^2 per image: sample_labels (S,N,H,W) integer label maps, truths (M,N,H,W) or (N,H,W)."""
    if truths.dim() == sample_labels.dim() - 1:
        truths = truths.unsqueeze(0)
    S = sample_labels.shape[0]
    t = _u8(truths.to(sample_labels.device))
    s = _u8(sample_labels)
    maps = torch.cat((s.reshape(S, s.shape[1], -1), t.reshape(t.shape[0], t.shape[1], -1)), 0)
    inter, cnt = label_pair_counts(maps, n_classes)
    return ged_from_counts(inter, cnt, S)
