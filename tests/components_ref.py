"""numpy restatement of the connected-component kernels (csrc/components.hip) and of pmu_hip/components.py: the
canonical root map (1 + the smallest linear index of a voxel's component) by minimum propagation over the
neighbour offsets with pointer jumping, to a fixed point; the dense numbering in raster order; sizes, the
keep-largest filter, the overlap test and the lesion-wise scores.  No scipy.  No test itself:
tests/test_components_cpu.py checks it against scipy.ndimage.label and by hand, tests/test_components_gpu.py
checks the kernels against it bit for bit.  Also the volumes both files use."""
import itertools

import numpy as np

import surface_ref

MAXNZ = {6: 1, 18: 2, 26: 3}


def offsets(connectivity):
    """Every neighbour offset of the connectivity (both directions)."""
    m = MAXNZ[connectivity]
    return [o for o in itertools.product((-1, 0, 1), repeat=3) if 0 < sum(v != 0 for v in o) <= m]


def roots(lab, connectivity):
    """int32 volume: 0 where lab == 0, else 1 + the smallest linear index of the voxel's component."""
    lab = np.asarray(lab)
    shape, V = lab.shape, lab.size
    fg = lab != 0
    L = np.where(fg, np.arange(1, V + 1, dtype=np.int64).reshape(shape), 0)
    labp = np.pad(lab, 1, constant_values=0)
    offs = offsets(connectivity)
    D0, D1, D2 = shape
    while True:
        before = L.copy()
        Lp = np.pad(L, 1, constant_values=0)
        for dz, dy, dx in offs:
            sl = (slice(1 + dz, 1 + dz + D0), slice(1 + dy, 1 + dy + D1), slice(1 + dx, 1 + dx + D2))
            take = fg & (labp[sl] == lab) & (Lp[sl] < L)       # (a neighbour of the same value is foreground)
            L = np.where(take, Lp[sl], L)
        flat = L.reshape(-1)                                   # pointer jumping: the label of my label's voxel
        idx = np.flatnonzero(flat)
        while True:
            nxt = flat[flat[idx] - 1]
            if np.array_equal(nxt, flat[idx]):
                break
            flat[idx] = nxt
        L = flat.reshape(shape)
        if np.array_equal(L, before):
            return L.astype(np.int32)


def compact(root):
    """(ids int32 — the rank 1..n of each voxel's root among the distinct roots, ascending; 0 for background —, n)."""
    r = np.asarray(root)
    uniq = np.unique(r[r > 0])
    ids = np.where(r > 0, np.searchsorted(uniq, r) + 1, 0).astype(np.int32)
    return ids, len(uniq)


def sizes(ids, lab, n):
    """(size int64 (n,), cls uint8 (n,))."""
    ids, lab = np.asarray(ids), np.asarray(lab)
    size = np.bincount(ids.reshape(-1), minlength=n + 1)[1:].astype(np.int64)
    cls = np.zeros(n, dtype=np.uint8)
    cls[ids[ids > 0] - 1] = lab[ids > 0]
    return size, cls


def components(lab, connectivity=26):
    ids, n = compact(roots(lab, connectivity))
    size, cls = sizes(ids, lab, n)
    return {"ids": ids, "n": n, "size": size, "cls": cls}


def class_list(n_classes):
    return [1] if n_classes == 1 else list(range(1, n_classes))


def keep_mask(size, cls, n_classes, keep=1, min_voxels=1):
    """(n,) uint8: per class the first ``keep`` (None: all) components by (size descending, id ascending) that
    have at least min_voxels voxels."""
    out = np.zeros(len(size), dtype=np.uint8)
    for c in class_list(n_classes):
        order = sorted((i for i in range(len(size)) if cls[i] == c), key=lambda i: (-int(size[i]), i))
        if keep is not None:
            order = order[:keep]
        for i in order:
            if size[i] >= min_voxels:
                out[i] = 1
    return out


def apply_filter(lab, ids, keep):
    lab, ids = np.asarray(lab), np.asarray(ids)
    k = np.concatenate((np.zeros(1, dtype=np.uint8), np.asarray(keep, dtype=np.uint8)))
    return np.where(k[ids] != 0, lab, 0).astype(np.uint8)


def keep_largest(lab, n_classes, keep=1, min_voxels=1, connectivity=26):
    c = components(lab, connectivity)
    return apply_filter(lab, c["ids"], keep_mask(c["size"], c["cls"], n_classes, keep, min_voxels))


def overlap_hits(ids_a, lab_a, n_a, ids_b, lab_b, n_b):
    """(hit_a (n_a,), hit_b (n_b,)) uint8: component i has a voxel where the other volume carries its value."""
    ids_a, lab_a, ids_b, lab_b = (np.asarray(v) for v in (ids_a, lab_a, ids_b, lab_b))
    both = (lab_a != 0) & (lab_a == lab_b)
    hit_a, hit_b = np.zeros(n_a, dtype=np.uint8), np.zeros(n_b, dtype=np.uint8)
    ia, ib = ids_a[both & (ids_a > 0)], ids_b[both & (ids_b > 0)]
    hit_a[ia - 1] = 1
    hit_b[ib - 1] = 1
    return hit_a, hit_b


def lesion_metrics(pred, truth, n_classes, connectivity=26, min_voxels=1):
    """pmu_hip.components.lesion_metrics restated (the small components are removed, then the cleaned volumes are
    labelled afresh): dict of (K-1,) float64 arrays."""
    a = keep_largest(pred, n_classes, None, min_voxels, connectivity)
    b = keep_largest(truth, n_classes, None, min_voxels, connectivity)
    ca, cb = components(a, connectivity), components(b, connectivity)
    hit_a, hit_b = overlap_hits(ca["ids"], a, ca["n"], cb["ids"], b, cb["n"])
    rows = {k: [] for k in ("n_pred", "n_truth", "tp", "fn", "fp")}
    for c in class_list(n_classes):
        rows["n_pred"].append(float((ca["cls"] == c).sum()))
        rows["n_truth"].append(float((cb["cls"] == c).sum()))
        rows["tp"].append(float(((cb["cls"] == c) & (hit_b != 0)).sum()))
        rows["fp"].append(float(((ca["cls"] == c) & (hit_a == 0)).sum()))
        rows["fn"].append(rows["n_truth"][-1] - rows["tp"][-1])
    r = {k: np.array(v, dtype=np.float64) for k, v in rows.items()}
    with np.errstate(invalid="ignore", divide="ignore"):
        r["sensitivity"] = r["tp"] / r["n_truth"]
        r["precision"] = (r["n_pred"] - r["fp"]) / r["n_pred"]
        r["f1"] = 2.0 * r["tp"] / (2.0 * r["tp"] + r["fp"] + r["fn"])
    return r


# ------------------------------------------------------------------ volumes
def noisy_blobs(shape, seed, n_classes=3, density=0.15):
    """surface_ref.blobs with ``density`` of the background voxels set to a random class 1..n_classes-1."""
    lab = surface_ref.blobs(shape, n_classes, seed).copy()
    g = np.random.default_rng(seed)
    noise = (lab == 0) & (g.random(shape) < density)
    lab[noise] = g.integers(1, n_classes, size=int(noise.sum()), dtype=np.uint8)
    return lab


def checker(shape):
    i, j, k = np.indices(shape)
    return ((i + j + k) % 2).astype(np.uint8)


def diag(n):
    lab = np.zeros((n, n, n), dtype=np.uint8)
    r = np.arange(n)
    lab[r, r, r] = 1
    return lab


def snake(shape):
    """One voxel-wide 6-connected serpentine through the whole volume (D0, D1 odd): in every even plane the rows
    of even j, joined at alternating ends, the planes joined by one voxel at the corner where the in-plane path
    ends (at its start corner in every second plane, which is walked backwards)."""
    D0, D1, D2 = shape
    assert D0 % 2 == 1 and D1 % 2 == 1
    lab = np.zeros(shape, dtype=np.uint8)
    end = D2 - 1 if ((D1 - 1) // 2) % 2 == 0 else 0      # the column where the last row of a plane ends
    for i in range(D0):
        if i % 2 == 0:
            for j in range(D1):
                if j % 2 == 0:
                    lab[i, j, :] = 1
                elif j % 4 == 1:
                    lab[i, j, D2 - 1] = 1
                else:
                    lab[i, j, 0] = 1
        elif (i // 2) % 2 == 0:
            lab[i, D1 - 1, end] = 1
        else:
            lab[i, 0, 0] = 1
    return lab


# name -> shape; the content by name in volume()
CASES = {
    "one": (1, 1, 1),
    "flat": (5, 1, 7),
    "unit": (17, 20, 24),
    "aniso": (33, 18, 65),
    "long": (1024, 2, 3),
    "checker": (6, 7, 9),
    "diag": (11, 11, 11),
    "snake": (9, 21, 70),
    "empty": (8, 8, 8),
    "tile1": (5, 9, 65),     # one past the 4 x 8 x 64 tile of the labelling kernel in each axis
}
NOISY = ("flat", "unit", "aniso", "long", "tile1")


def volume(name, seed=None):
    """The u8 volume of a case (noisy blobs: seeded by the case's position unless ``seed`` is given)."""
    shape = CASES[name]
    if name == "one":
        return np.ones(shape, dtype=np.uint8)
    if name == "checker":
        return checker(shape)
    if name == "diag":
        return diag(shape[0])
    if name == "snake":
        return snake(shape)
    if name == "empty":
        return np.zeros(shape, dtype=np.uint8)
    return noisy_blobs(shape, sorted(CASES).index(name) if seed is None else seed)
