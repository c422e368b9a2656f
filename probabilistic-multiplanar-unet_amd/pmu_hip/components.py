"""Connected components of a label volume: the clean-up of a fused label map (keep the largest component or
components of each class, drop what is below a minimum size) and the object-wise detection scores (lesion-wise
sensitivity, precision and F1), next to the voxel-wise Dice of pmu_hip.metrics and the surface distances of
pmu_hip.surface.

Value 0 is background.  Two voxels are adjacent under connectivity 6 (faces), 18 (faces and edges) or 26 (faces,
edges and corners) and belong to one component when a chain of adjacent voxels of the same non-zero value joins
them; different classes never merge.  Components are numbered 1..n in the raster order of their first voxel (the
numbering of scipy.ndimage.label).  All per-voxel work is the pmu_cc_* kernels' (csrc/components.hip); every
result is an integer defined by the volume alone, so two runs agree bit for bit.
"""
from __future__ import annotations

import torch

from . import _lib as L
from .surface import _volume

CONNECTIVITIES = (6, 18, 26)


def _connectivity(connectivity) -> int:
    if connectivity not in CONNECTIVITIES:
        raise ValueError(f"connectivity must be 6, 18 or 26, got {connectivity}")
    return int(connectivity)


def _classes(n_classes, what: str, dev) -> torch.Tensor:
    K = int(n_classes)
    if not 1 <= K <= 256:
        raise ValueError(f"{what}: {K} classes outside 1..256")
    return torch.tensor([1] if K == 1 else list(range(1, K)), dtype=torch.uint8, device=dev)


def _min_voxels(min_voxels) -> int:
    if int(min_voxels) != min_voxels or min_voxels < 1:
        raise ValueError(f"min_voxels must be a positive integer, got {min_voxels}")
    return int(min_voxels)


def _components(lab: torch.Tensor, connectivity: int) -> dict:
    D0, D1, D2 = lab.shape
    V, dev = lab.numel(), lab.device
    ids = torch.empty(D0, D1, D2, dtype=torch.int32, device=dev)
    count = torch.empty(2, dtype=torch.int64, device=dev)
    nbytes = int(L.lib().pmu_cc_ws(D0, D1, D2))
    ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    L.call("pmu_cc_label", lab.data_ptr(), D0, D1, D2, connectivity, ids.data_ptr(), count[0:1].data_ptr(),
           ws.data_ptr(), nbytes, L.stream())
    L.call("pmu_cc_compact", ids.data_ptr(), V, ids.data_ptr(), count[1:2].data_ptr(), ws.data_ptr(), nbytes,
           L.stream())
    n = int(count[1].item())     # the one host read: it sizes the per-component vectors
    size = torch.empty(n, dtype=torch.int64, device=dev)
    cls = torch.empty(n, dtype=torch.uint8, device=dev)
    L.call("pmu_cc_sizes", ids.data_ptr(), lab.data_ptr(), V, n, L.ptr(size) if n else None,
           L.ptr(cls) if n else None, L.stream())
    return {"ids": ids, "n": n, "size": size, "cls": cls}


def _filter(lab: torch.Tensor, comp: dict, keep: torch.Tensor) -> torch.Tensor:
    out = torch.empty_like(lab)
    n = comp["n"]
    L.call("pmu_cc_filter", lab.data_ptr(), comp["ids"].data_ptr(), lab.numel(), L.ptr(keep) if n else None, n,
           out.data_ptr(), L.stream())
    return out


def components(labels: torch.Tensor, connectivity: int = 26) -> dict:
    """The connected components of a (D0,D1,D2) label volume (any integer or float tensor on the GPU; a value
    outside 0..255 is stored as 255 like everywhere on this path, the value no class count below 256 reaches):
    {'ids': (D0,D1,D2) int32 — 0 for background, else the component's number 1..n —, 'n': int,
    'size': (n,) int64 voxel counts, 'cls': (n,) uint8 label values}.  One host read of n sizes the
    per-component vectors; that read is the only synchronisation."""
    return _components(_volume(labels, "components"), _connectivity(connectivity))


def _rank_keep(comp: dict, classes: torch.Tensor, keep, min_voxels: int) -> torch.Tensor:
    """(n,) uint8: 1 for the components that stay.  Per class the components are ranked by size descending, ties
    to the smaller id; the first ``keep`` (all with keep=None) of them with at least ``min_voxels`` voxels stay.
    Torch ops on the (n,) vectors, no host read."""
    size, cls = comp["size"], comp["cls"]
    ok = (size >= min_voxels) & (cls[:, None] == classes[None, :]).any(1)
    if keep is None or comp["n"] == 0:
        return ok.to(torch.uint8)
    # one stable ascending sort by (class, -size): inside a class by size descending, ties in id order
    key = (cls.long() << 32) + ((1 << 31) - size)
    order = torch.sort(key, stable=True).indices
    sc = cls[order]
    pos = torch.arange(comp["n"], device=size.device)
    first = torch.ones_like(sc, dtype=torch.bool)
    first[1:] = sc[1:] != sc[:-1]
    start = torch.cummax(torch.where(first, pos, torch.zeros_like(pos)), 0).values
    stay = torch.zeros_like(ok)
    stay[order] = (pos - start) < int(keep)
    return (stay & ok).to(torch.uint8)


def keep_largest(labels: torch.Tensor, n_classes: int, keep=1, min_voxels: int = 1,
                 connectivity: int = 26) -> torch.Tensor:
    """The label volume with, for each class 1..K-1 (K = 1: label value 1), only its ``keep`` largest components
    of at least ``min_voxels`` voxels (ranked by size descending, ties to the smaller id; keep=None: every
    component that passes ``min_voxels``); everything else, values outside those classes included, becomes 0.
    Returns a (D0,D1,D2) uint8 volume."""
    lab = _volume(labels, "keep_largest")
    conn = _connectivity(connectivity)
    classes = _classes(n_classes, "keep_largest", lab.device)
    mv = _min_voxels(min_voxels)
    if keep is not None and (int(keep) != keep or keep < 1):
        raise ValueError(f"keep must be a positive integer or None, got {keep}")
    comp = _components(lab, conn)
    return _filter(lab, comp, _rank_keep(comp, classes, keep, mv))


LESION_KEYS = ("n_pred", "n_truth", "tp", "fn", "fp", "sensitivity", "precision", "f1")


def lesion_metrics(pred_labels: torch.Tensor, truth_labels: torch.Tensor, n_classes: int, connectivity: int = 26,
                   min_voxels: int = 1) -> dict:
    """Object-wise detection scores of the classes 1..K-1 (K = 1: label value 1) of two (D0,D1,D2) label volumes:
    a dict of (K-1,) float64 tensors.  Components below ``min_voxels`` are dropped from both volumes first.
    n_pred, n_truth: components per class; tp: true components touched by a predicted voxel of their class;
    fn = n_truth - tp; fp: predicted components that touch no true voxel of their class;
    sensitivity = tp / n_truth; precision = (n_pred - fp) / n_pred; f1 = 2 tp / (2 tp + fp + fn).  A ratio with a
    zero denominator is NaN (the convention of pmu_hip.surface.metrics_from_distances for empty surfaces)."""
    pred = _volume(pred_labels, "lesion_metrics")
    truth = _volume(truth_labels.to(pred_labels.device), "lesion_metrics")
    if pred.shape != truth.shape:
        raise ValueError(f"prediction {tuple(pred.shape)} and truth {tuple(truth.shape)} are not one grid")
    conn = _connectivity(connectivity)
    classes = _classes(n_classes, "lesion_metrics", pred.device)
    mv = _min_voxels(min_voxels)
    side = []
    for lab in (pred, truth):
        comp = _components(lab, conn)
        stay = _rank_keep(comp, classes, None, mv)
        side.append((comp, stay, _filter(lab, comp, stay)))
    (ca, ka, la), (cb, kb, lb) = side
    hit_a = torch.empty(ca["n"], dtype=torch.uint8, device=pred.device)
    hit_b = torch.empty(cb["n"], dtype=torch.uint8, device=pred.device)
    # the ids of the unfiltered volumes still number the components that stayed; dropped ones have no voxel left
    L.call("pmu_cc_overlap", ca["ids"].data_ptr(), la.data_ptr(), ca["n"], cb["ids"].data_ptr(), lb.data_ptr(),
           cb["n"], pred.numel(), L.ptr(hit_a) if ca["n"] else None, L.ptr(hit_b) if cb["n"] else None, L.stream())

    def per_class(comp, mask):
        return ((comp["cls"][None, :] == classes[:, None]) & mask.bool()[None, :]).sum(1).double()

    n_pred, n_truth = per_class(ca, ka), per_class(cb, kb)
    tp = per_class(cb, kb & hit_b)
    fp = per_class(ca, ka & (1 - hit_a))
    fn = n_truth - tp
    return {"n_pred": n_pred, "n_truth": n_truth, "tp": tp, "fn": fn, "fp": fp, "sensitivity": tp / n_truth,
            "precision": (n_pred - fp) / n_pred, "f1": 2.0 * tp / (2.0 * tp + fp + fn)}
