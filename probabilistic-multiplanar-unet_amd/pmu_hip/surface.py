"""Surface-distance metrics of a label volume against its ground truth: the Hausdorff distance (HD), its
95th percentile (HD95), the average symmetric surface distance (ASSD) and the surface Dice at a tolerance
(NSD), per class, next to the Dice of pmu_hip.metrics.

The surface of a class is every voxel of it with a face neighbour outside it (mask ^ binary_erosion(mask),
6-connected; the volume's border counts as outside).  pmu_surface_edt is an exact Euclidean distance transform
to that surface — squared distances in fp32 with a fixed association, bit-equal to the brute-force minimum —
and pmu_surface_collect gathers one volume's surface voxels out of the other volume's transform.  The
gathered vectors are sorted, so every sum below runs in a fixed order: two runs agree bit for bit.
"""
from __future__ import annotations

import math

import torch

from . import _lib as L
from .uncertainty import _u8

MAX_DIM = 1024   # PMU_SURFACE_MAX_DIM


def _volume(labels: torch.Tensor, what: str) -> torch.Tensor:
    if not labels.is_cuda:
        raise RuntimeError(f"{what} runs on the MI355X HIP path only (there is no CPU fallback)")
    if labels.dim() != 3:
        raise ValueError(f"{what}: expected a (D0,D1,D2) label volume, got {tuple(labels.shape)}")
    if not all(1 <= d <= MAX_DIM for d in labels.shape) or labels.numel() >= 1 << 31:
        raise ValueError(f"{what}: volume {tuple(labels.shape)} outside the kernel's range (every dimension 1.."
                         f"{MAX_DIM}, fewer than 2^31 voxels)")
    return _u8(labels).contiguous()


def _spacing(spacing) -> tuple:
    s = tuple(float(v) for v in spacing)
    if len(s) != 3 or not all(math.isfinite(v) and v > 0 for v in s):
        raise ValueError(f"voxel sizes must be three finite positive numbers, got {spacing}")
    return s


def _edt(lab: torch.Tensor, cls: int, spacing: tuple, count: torch.Tensor):
    D0, D1, D2 = lab.shape
    d2 = torch.empty(D0, D1, D2, dtype=torch.float32, device=lab.device)
    L.call("pmu_surface_edt", lab.data_ptr(), D0, D1, D2, int(cls), spacing[0], spacing[1], spacing[2],
           d2.data_ptr(), count.data_ptr(), L.stream())
    return d2


def _collect(lab: torch.Tensor, cls: int, d2_other: torch.Tensor, n: int, count: torch.Tensor) -> torch.Tensor:
    D0, D1, D2 = lab.shape
    out = torch.empty(n, dtype=torch.float32, device=lab.device)
    L.call("pmu_surface_collect", lab.data_ptr(), D0, D1, D2, int(cls), d2_other.data_ptr(), L.ptr(out) if n else None,
           n, count.data_ptr(), L.stream())
    return out


def edt(labels: torch.Tensor, cls: int, spacing=(1.0, 1.0, 1.0)):
    """Squared distance of every voxel of ``labels`` (D0,D1,D2) to the surface of class ``cls`` under voxel sizes
    ``spacing``: (d2 (D0,D1,D2) float32 — +inf everywhere if the class has no voxel —, number of surface
    voxels).  Reading the count synchronises."""
    lab = _volume(labels, "edt")
    if not 0 <= int(cls) <= 255:
        raise ValueError(f"edt: class {cls} outside 0..255")
    count = torch.empty(1, dtype=torch.int64, device=lab.device)
    d2 = _edt(lab, cls, _spacing(spacing), count)
    return d2, int(count.item())


def _percentile(a: torch.Tensor, q: float) -> torch.Tensor:
    """numpy.percentile(a, q) of a sorted vector (linear interpolation, numpy's lerp)."""
    n = a.numel()
    pos = (n - 1) * (float(q) / 100.0)
    lo = min(max(int(math.floor(pos)), 0), n - 1)
    hi = min(lo + 1, n - 1)
    t = pos - lo
    d = a[hi] - a[lo]
    return a[hi] - d * (1.0 - t) if t >= 0.5 else a[lo] + d * t


def metrics_from_distances(d_pred_to_truth: torch.Tensor, d_truth_to_pred: torch.Tensor, tolerance: float,
                           percentile: float = 95.0) -> dict:
    """The four metrics from the two directed distance vectors, each sorted ascending (float64, any device):
    the distance of every predicted-surface voxel to the truth surface, and the reverse.

    hd: the maximum of both; hd95: the ``percentile``-th percentile of the pooled vector, interpolated linearly
    (numpy.percentile, MedPy's hd95); assd: the mean of the two directed means; nsd: the share of all
    surface voxels within ``tolerance`` (<=) of the other surface.  With an empty surface hd, hd95 and assd are
    NaN; nsd is NaN when both are empty and 0 when one is.  Returns 0-dim float64 tensors."""
    a = torch.as_tensor(d_pred_to_truth, dtype=torch.float64)
    b = torch.as_tensor(d_truth_to_pred, dtype=torch.float64, device=a.device)
    na, nb = a.numel(), b.numel()
    nan = torch.full((), float("nan"), dtype=torch.float64, device=a.device)
    if na == 0 or nb == 0:
        nsd = nan if na == nb else torch.zeros((), dtype=torch.float64, device=a.device)
        return {"hd": nan, "hd95": nan, "assd": nan, "nsd": nsd}
    pooled = torch.sort(torch.cat((a, b))).values
    within = (a <= tolerance).sum() + (b <= tolerance).sum()
    return {"hd": torch.maximum(a[-1], b[-1]), "hd95": _percentile(pooled, percentile),
            "assd": 0.5 * (a.sum() / na + b.sum() / nb), "nsd": within.double() / (na + nb)}


def surface_distances(pred_labels: torch.Tensor, truth_labels: torch.Tensor, n_classes: int,
                      spacing=(1.0, 1.0, 1.0), tolerance: float = 1.0, percentile: float = 95.0) -> dict:
    """HD, HD95, ASSD and surface Dice of the classes 1..K-1 (K = 1: the single class) of two (D0,D1,D2) label
    volumes, distances in the unit of ``spacing``: a dict of (K-1,) float64 tensors 'hd', 'hd95', 'assd', 'nsd',
    'n_pred', 'n_truth' (the surface voxel counts).  Labels may be any integer or float tensor (values outside
    0..255 belong to no class).  Per class: two distance transforms, one host read of the two surface counts
    (they size the gather buffers), two gathers, a sort of each vector and a float64 square root."""
    pred = _volume(pred_labels, "surface_distances")
    truth = _volume(truth_labels.to(pred_labels.device), "surface_distances")
    if pred.shape != truth.shape:
        raise ValueError(f"prediction {tuple(pred.shape)} and truth {tuple(truth.shape)} are not one grid")
    K = int(n_classes)
    if not 1 <= K <= 256:
        raise ValueError(f"surface_distances: {K} classes outside 1..256")
    sp = _spacing(spacing)
    classes = [0] if K == 1 else list(range(1, K))
    dev = pred.device
    counts = torch.empty(2, dtype=torch.int64, device=dev)
    scratch = torch.empty(2, dtype=torch.int64, device=dev)
    rows = {k: [] for k in ("hd", "hd95", "assd", "nsd", "n_pred", "n_truth")}
    for c in classes:
        d2_pred = _edt(pred, c, sp, counts[0:1])
        d2_truth = _edt(truth, c, sp, counts[1:2])
        n_pred, n_truth = (int(v) for v in counts.tolist())
        dirs = []
        for lab, other, n, cnt in ((pred, d2_truth, n_pred, scratch[0:1]), (truth, d2_pred, n_truth, scratch[1:2])):
            v = _collect(lab, c, other, n, cnt)
            dirs.append(torch.sort(v).values.double().sqrt())
        del d2_pred, d2_truth
        m = metrics_from_distances(dirs[0], dirs[1], tolerance, percentile)
        for k in ("hd", "hd95", "assd", "nsd"):
            rows[k].append(m[k])
        rows["n_pred"].append(torch.tensor(float(n_pred), dtype=torch.float64, device=dev))
        rows["n_truth"].append(torch.tensor(float(n_truth), dtype=torch.float64, device=dev))
    return {k: torch.stack(v) for k, v in rows.items()}
