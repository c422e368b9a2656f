"""Local thickness and volume of the segmented structures of a label volume: what a user of a cartilage
segmentation reports per compartment.

Local thickness (Hildebrand & Ruegsegger): at every voxel of a class, the diameter of the largest ball that fits
inside the class and contains the voxel.  pmu_interior_edt gives every voxel q of the class the squared distance
D2(q) to the nearest position outside it (another label, or outside the volume) — the exact fp32 transform of
pmu_hip.surface seeded from outside the class — and pmu_local_thickness covers: R2(p) is the largest D2(q) over
the voxels q whose open ball (d2(p, q) < D2(q), strict) holds p.  The thickness is 2 sqrt(R2) in float64, in the
unit of the voxel sizes.

Balls are centred on voxel centres, so a slab k voxels across reads k + 1 for odd k and k for even k (the nearest
outside voxel centre of the middle voxel is (k + 1) / 2 or k / 2 steps away): the usual behaviour of voxel
local-thickness tools, not corrected here.

The per-class numbers are float64 tensor operations on the sorted vector of a class's thickness values, so two
runs agree bit for bit.
"""
from __future__ import annotations

import torch

from . import _lib as L
from .surface import MAX_DIM, _percentile, _spacing, _volume

STATS = ("n", "volume", "mean", "std", "median", "max")


def _interior(lab: torch.Tensor, cls: int, sp: tuple, count: torch.Tensor) -> torch.Tensor:
    D0, D1, D2 = lab.shape
    d2 = torch.empty(D0, D1, D2, dtype=torch.float32, device=lab.device)
    L.call("pmu_interior_edt", lab.data_ptr(), D0, D1, D2, int(cls), sp[0], sp[1], sp[2], d2.data_ptr(),
           count.data_ptr(), L.stream())
    return d2


def _cover(d2: torch.Tensor, sp: tuple) -> torch.Tensor:
    D0, D1, D2 = d2.shape
    r2 = torch.empty_like(d2)
    nbytes = int(L.lib().pmu_local_thickness_ws(D0, D1, D2))
    ws = torch.empty(nbytes // 4, dtype=torch.int32, device=d2.device)
    L.call("pmu_local_thickness", d2.data_ptr(), D0, D1, D2, sp[0], sp[1], sp[2], r2.data_ptr(), ws.data_ptr(),
           nbytes, L.stream())
    return r2


def interior_edt(labels: torch.Tensor, cls: int, spacing=(1.0, 1.0, 1.0)):
    """Squared distance of every voxel of class ``cls`` in ``labels`` (D0,D1,D2) to the nearest position not of the
    class (outside the volume counts) under voxel sizes ``spacing``, 0 off the class: (d2 (D0,D1,D2) float32,
    number of voxels of the class).  Reading the count synchronises."""
    lab = _volume(labels, "interior_edt")
    if not 0 <= int(cls) <= 255:
        raise ValueError(f"interior_edt: class {cls} outside 0..255")
    count = torch.empty(1, dtype=torch.int64, device=lab.device)
    d2 = _interior(lab, cls, _spacing(spacing), count)
    return d2, int(count.item())


def cover(d2: torch.Tensor, spacing=(1.0, 1.0, 1.0)) -> torch.Tensor:
    """The covering pass over an interior distance field ``d2`` (D0,D1,D2) float32: the squared radius of the
    largest ball inside the structure (d2 > 0) that contains each of its voxels, 0 elsewhere."""
    if not d2.is_cuda:
        raise RuntimeError("cover runs on the MI355X HIP path only (there is no CPU fallback)")
    if d2.dim() != 3 or d2.dtype != torch.float32:
        raise ValueError(f"cover: expected a (D0,D1,D2) float32 field, got {d2.dtype} {tuple(d2.shape)}")
    if not all(1 <= d <= MAX_DIM for d in d2.shape) or d2.numel() >= 1 << 31:
        raise ValueError(f"cover: field {tuple(d2.shape)} outside the kernel's range (every dimension 1..{MAX_DIM}, "
                         "fewer than 2^31 voxels)")
    return _cover(d2.contiguous(), _spacing(spacing))


def thickness_stats(sorted_tau: torch.Tensor, voxel_volume: float) -> dict:
    """The six numbers of one class from its thickness values sorted ascending (any device): 'n' the voxel count,
    'volume' = n * ``voxel_volume``, 'mean', 'std' (population), 'median' (numpy.percentile's interpolation) and
    'max', 0-dim float64 tensors.  An empty vector gives n = volume = 0 and NaN for the other four."""
    a = torch.as_tensor(sorted_tau, dtype=torch.float64).reshape(-1)
    n = a.numel()
    f = lambda v: torch.full((), float(v), dtype=torch.float64, device=a.device)  # noqa: E731
    if n == 0:
        nan = f("nan")
        return {"n": f(0.0), "volume": f(0.0), "mean": nan, "std": nan, "median": nan, "max": nan}
    mean = a.sum() / n
    return {"n": f(n), "volume": f(n * float(voxel_volume)), "mean": mean,
            "std": (((a - mean) ** 2).sum() / n).sqrt(), "median": _percentile(a, 50.0), "max": a[-1]}


def local_thickness(labels: torch.Tensor, n_classes: int, spacing=(1.0, 1.0, 1.0)) -> dict:
    """Local thickness and volume of the classes 1..K-1 (K = 1: the single class 0) of a (D0,D1,D2) label volume:
    'map', the (D0,D1,D2) float32 thickness of every voxel of a scored class in the unit of ``spacing`` (0
    elsewhere), and 'n', 'volume', 'mean', 'std', 'median', 'max', (K-1,) float64 tensors (thickness_stats per
    class; an absent class has n = volume = 0 and NaN).  Labels may be any integer or float tensor (values outside
    0..255 belong to no class).  Per class: the interior transform, the covering pass, a sort of the class's
    values and a float64 square root."""
    lab = _volume(labels, "local_thickness")
    K = int(n_classes)
    if not 1 <= K <= 256:
        raise ValueError(f"local_thickness: {K} classes outside 1..256")
    sp = _spacing(spacing)
    classes = [0] if K == 1 else list(range(1, K))
    vox = sp[0] * sp[1] * sp[2]
    count = torch.empty(1, dtype=torch.int64, device=lab.device)
    tmap = torch.zeros(lab.shape, dtype=torch.float32, device=lab.device)
    rows = {k: [] for k in STATS}
    for c in classes:
        r2 = _cover(_interior(lab, c, sp, count), sp)
        on = r2 > 0
        tau = 2.0 * torch.sort(r2[on]).values.double().sqrt()
        tmap = torch.where(on, (2.0 * r2.double().sqrt()).float(), tmap)
        for k, v in thickness_stats(tau, vox).items():
            rows[k].append(v)
    return {"map": tmap, **{k: torch.stack(v) for k, v in rows.items()}}
