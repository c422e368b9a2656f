"""numpy restatement of the surface-distance kernels (csrc/surface.hip) and metrics (pmu_hip/surface.py): the
class surface by the six-neighbour rule, the brute-force squared distance to it in np.float32 with the
kernels' association, and the metrics in float64.  No test itself; tests/test_surface_cpu.py checks it against
scipy.ndimage, tests/test_surface_gpu.py checks the kernels against it bit for bit."""
import numpy as np


def surface(lab, cls):
    """Voxels labelled cls with at least one face neighbour not labelled cls (outside the volume: not cls)."""
    m = np.asarray(lab) == cls
    p = np.pad(m, 1, constant_values=False)
    inner = (p[:-2, 1:-1, 1:-1] & p[2:, 1:-1, 1:-1] & p[1:-1, :-2, 1:-1] & p[1:-1, 2:, 1:-1]
             & p[1:-1, 1:-1, :-2] & p[1:-1, 1:-1, 2:])
    return m & ~inner


def _axis_table(s, n):
    """t(d) = fl(fl(s * float(d)) * fl(s * float(d))) for d = 0..n-1, np.float32 (one rounding per operation)."""
    a = np.float32(s) * np.arange(n, dtype=np.float32)
    assert a.dtype == np.float32
    return a * a


def d2_brute(surf, spacing=(1.0, 1.0, 1.0), chunk=1024):
    """min over the surface voxels q of d2(v, q) = fl(fl(t_2 + t_1) + t_0), float32, for every voxel v; +inf
    everywhere without a surface."""
    surf = np.asarray(surf, dtype=bool)
    shape = surf.shape
    out = np.full(surf.size, np.inf, dtype=np.float32)
    q = np.argwhere(surf).astype(np.int32)
    if len(q) == 0:
        return out.reshape(shape)
    t0, t1, t2 = (_axis_table(s, n) for s, n in zip(spacing, shape))
    v = np.indices(shape, dtype=np.int32).reshape(3, -1).T
    with np.errstate(over="ignore"):
        for a in range(0, len(v), chunk):
            w = v[a:a + chunk]
            e0 = t0[np.abs(w[:, None, 0] - q[None, :, 0])]
            e1 = t1[np.abs(w[:, None, 1] - q[None, :, 1])]
            e2 = t2[np.abs(w[:, None, 2] - q[None, :, 2])]
            d = (e2 + e1) + e0
            assert d.dtype == np.float32
            out[a:a + chunk] = d.min(1)
    return out.reshape(shape)


def gather_sorted(lab, cls, d2_other):
    """The float32 d2_other values at the surface voxels of cls in lab, ascending."""
    return np.sort(np.asarray(d2_other, dtype=np.float32)[surface(lab, cls)])


def metrics(d_a, d_b, tolerance, percentile=95.0):
    """hd, hd95, assd, nsd (float64) from the two directed distance vectors (any order)."""
    a, b = np.asarray(d_a, dtype=np.float64), np.asarray(d_b, dtype=np.float64)
    nan = float("nan")
    if len(a) == 0 or len(b) == 0:
        return {"hd": nan, "hd95": nan, "assd": nan, "nsd": nan if len(a) == len(b) else 0.0}
    return {"hd": float(max(a.max(), b.max())),
            "hd95": float(np.percentile(np.concatenate((a, b)), percentile)),
            "assd": float(0.5 * (a.mean() + b.mean())),
            "nsd": float(((a <= tolerance).sum() + (b <= tolerance).sum()) / (len(a) + len(b)))}


def surface_distances(pred, truth, n_classes, spacing=(1.0, 1.0, 1.0), tolerance=1.0, percentile=95.0):
    """pmu_hip.surface.surface_distances restated: dict of (K-1,) float64 arrays."""
    classes = [0] if n_classes == 1 else range(1, n_classes)
    rows = {k: [] for k in ("hd", "hd95", "assd", "nsd", "n_pred", "n_truth")}
    for c in classes:
        sp, st = surface(pred, c), surface(truth, c)
        dp, dt = d2_brute(sp, spacing), d2_brute(st, spacing)
        a = np.sqrt(np.sort(dt[sp]).astype(np.float64))
        b = np.sqrt(np.sort(dp[st]).astype(np.float64))
        m = metrics(a, b, tolerance, percentile)
        for k in ("hd", "hd95", "assd", "nsd"):
            rows[k].append(m[k])
        rows["n_pred"].append(float(sp.sum()))
        rows["n_truth"].append(float(st.sum()))
    return {k: np.array(v, dtype=np.float64) for k, v in rows.items()}


def blobs(shape, n_classes, seed, per_class=3):
    """Seeded u8 label volume: per foreground class a few random ellipsoids (later classes overwrite earlier
    ones), centred inside the volume so that every axis length, 1 included, can hold a label."""
    g = np.random.default_rng(seed)
    lab = np.zeros(shape, dtype=np.uint8)
    ii = np.indices(shape).astype(np.float64)
    for c in range(1, n_classes):
        for _ in range(per_class):
            ctr = [g.uniform(0, n - 1) for n in shape]
            rad = [g.uniform(1.0, max(1.5, n / 3.0)) for n in shape]
            r2 = sum(((ii[a] - ctr[a]) / rad[a]) ** 2 for a in range(3))
            lab[r2 <= 1.0] = c
    return lab
