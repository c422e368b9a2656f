"""numpy restatement of the local-thickness kernels (pmu_interior_edt in csrc/surface.hip, pmu_local_thickness in
csrc/thickness.hip) and of pmu_hip/thickness.py: the interior distance by brute force over the volume padded by
one voxel of "outside", the covering pass as a loop over index offsets in np.float32 with the kernels'
association, and the statistics in float64.  No test itself; tests/test_thickness_cpu.py checks it against
scipy.ndimage and an independent integer construction, tests/test_thickness_gpu.py checks the kernels against
it bit for bit."""
import numpy as np

import surface_ref as S

STATS = ("n", "volume", "mean", "std", "median", "max")


def interior_d2(lab, cls, spacing=(1.0, 1.0, 1.0)):
    """For every voxel labelled cls the minimum of d2 over all positions not labelled cls, a position outside the
    volume counting as not cls; 0 off the class.  float32."""
    m = np.asarray(lab) == cls
    outside = np.pad(~m, 1, constant_values=True)
    d2 = S.d2_brute(outside, spacing)[1:-1, 1:-1, 1:-1]
    return np.where(m, d2, np.float32(0)).astype(np.float32)


def interior_d2_fast(lab, cls, spacing=(1.0, 1.0, 1.0), chunk=256):
    """interior_d2 evaluated at the voxels of the class only (d2_brute's arithmetic, the same padded set of
    outside positions): the same bits at a fraction of the pairs.  tests/test_thickness_cpu.py holds the two
    equal."""
    m = np.asarray(lab) == cls
    out = np.zeros(m.shape, dtype=np.float32)
    v = np.argwhere(m).astype(np.int32) + 1                       # in the padded frame
    if len(v) == 0:
        return out
    q = np.argwhere(np.pad(~m, 1, constant_values=True)).astype(np.int32)
    t0, t1, t2 = (S._axis_table(s, n + 2) for s, n in zip(spacing, m.shape))
    best = np.empty(len(v), dtype=np.float32)
    with np.errstate(over="ignore"):
        for a in range(0, len(v), chunk):
            w = v[a:a + chunk]
            d = (t2[np.abs(w[:, None, 2] - q[None, :, 2])] + t1[np.abs(w[:, None, 1] - q[None, :, 1])]) \
                + t0[np.abs(w[:, None, 0] - q[None, :, 0])]
            assert d.dtype == np.float32
            best[a:a + chunk] = d.min(1)
    out[m] = best
    return out


def _reach(t, top):
    """Largest index offset e with t[e] < top (t non-decreasing, t[0] = 0 < top)."""
    return int(np.searchsorted(t, top, side="left")) - 1


def cover_r2(d2, spacing=(1.0, 1.0, 1.0)):
    """r2(p) = max{ d2(q) : d2(q) > 0, dist2(p, q) < d2(q) } where d2(p) > 0, 0 elsewhere; float32, dist2 =
    fl(fl(t_2 + t_1) + t_0)."""
    d2 = np.asarray(d2, dtype=np.float32)
    shape = d2.shape
    r2 = np.zeros(shape, dtype=np.float32)
    top = d2.max() if d2.size else np.float32(0)
    if not top > 0:
        return r2
    t = [S._axis_table(s, n) for s, n in zip(spacing, shape)]
    reach = [_reach(t[a], top) for a in range(3)]
    member = d2 > 0
    for e0 in range(-reach[0], reach[0] + 1):
        for e1 in range(-reach[1], reach[1] + 1):
            u1 = t[1][abs(e1)]
            for e2 in range(-reach[2], reach[2] + 1):
                dist = (t[2][abs(e2)] + u1) + t[0][abs(e0)]
                assert dist.dtype == np.float32
                if not dist < top:
                    continue
                # p = q + e: the slices of p (destination) and q (source) inside the volume
                dst = tuple(slice(max(e, 0), n + min(e, 0)) for e, n in zip((e0, e1, e2), shape))
                src = tuple(slice(max(-e, 0), n + min(-e, 0)) for e, n in zip((e0, e1, e2), shape))
                q = d2[src]
                r2[dst] = np.where((dist < q) & member[dst], np.maximum(r2[dst], q), r2[dst])
    return r2


def tau_of(r2):
    """2 sqrt(double(r2)), float64."""
    return 2.0 * np.sqrt(np.asarray(r2).astype(np.float64))


def stats(tau, voxel_volume):
    """The six numbers of a class from its thickness values (any order), float64."""
    a = np.asarray(tau, dtype=np.float64).ravel()
    nan = float("nan")
    if len(a) == 0:
        return {"n": 0.0, "volume": 0.0, "mean": nan, "std": nan, "median": nan, "max": nan}
    return {"n": float(len(a)), "volume": float(len(a) * voxel_volume), "mean": float(a.mean()),
            "std": float(a.std()), "median": float(np.percentile(a, 50)), "max": float(a.max())}


def local_thickness(lab, n_classes, spacing=(1.0, 1.0, 1.0)):
    """pmu_hip.thickness.local_thickness restated: 'map' float32 and (K-1,) float64 arrays."""
    lab = np.asarray(lab)
    classes = [0] if n_classes == 1 else range(1, n_classes)
    vox = float(spacing[0]) * float(spacing[1]) * float(spacing[2])
    tmap = np.zeros(lab.shape, dtype=np.float32)
    rows = {k: [] for k in STATS}
    for c in classes:
        r2 = cover_r2(interior_d2_fast(lab, c, spacing), spacing)
        on = r2 > 0
        tmap[on] = tau_of(r2[on]).astype(np.float32)
        for k, v in stats(tau_of(r2[on]), vox).items():
            rows[k].append(v)
    out = {k: np.array(v, dtype=np.float64) for k, v in rows.items()}
    out["map"] = tmap
    return out
