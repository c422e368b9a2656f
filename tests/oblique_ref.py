"""Numpy restatement of the oblique-view geometry (DESIGN.md "Oblique views"), the yardstick of
tests/test_oblique_cpu.py and tests/test_oblique_gpu.py.  The reference has no counterpart, so the
operation order is written out here and the kernels (csrc/oblique.hip) follow it bit for bit: fp64
coordinates as c + ((ds n + da u) + db v) and ((d0 f0 + d1 f1) + d2 f2) / h + (P-1)/2, every lerp as
a + f (b - a), numpy evaluating one rounded operation at a time (nothing fused).

The fusion's interpolation cell is floor(g) with the upper neighbour clamped to P-1 — the cell
min(floor(g), P-2) for every g < P-1; on the last grid plane the weight is 0, not 1, so that a grid point
reads back its stack value exactly (a + 1 (b - a) is not b in floating point) and the axis-aligned case
equals the three-view fusion bit for bit.

A frame is the (3,3) float64 array utils.mri_dataset.view_frame returns: rows n, u, v.
"""
import numpy as np


def grid_to_voxel(pshape, frame, P, h, s, a, b):
    """Voxel coordinates (x0, x1, x2) of grid point (slice s, pixel a, b); s, a, b broadcastable."""
    half = (P - 1) / 2.0
    ds, da, db = h * (s - half), h * (a - half), h * (b - half)
    n, u, v = frame
    return tuple((pshape[i] - 1) / 2.0 + ((ds * n[i] + da * u[i]) + db * v[i]) for i in range(3))


def voxel_to_grid(pshape, frame, P, h, x0, x1, x2):
    """Grid coordinates (g_s, g_a, g_b) of voxel coordinates x."""
    half = (P - 1) / 2.0
    d = [x0 - (pshape[0] - 1) / 2.0, x1 - (pshape[1] - 1) / 2.0, x2 - (pshape[2] - 1) / 2.0]
    return tuple(((d[0] * f[0] + d[1] * f[1]) + d[2] * f[2]) / h + half for f in frame)


def _grid(pshape, frame, P, h):
    ax = np.arange(P, dtype=np.float64)
    return grid_to_voxel(pshape, frame, P, h, ax[:, None, None], ax[None, :, None], ax[None, None, :])


def sample_view(vol, frame, P, h, nearest):
    """(P,P,P) float64: every slice of the padded volume ``vol`` along ``frame`` (unnormalised)."""
    vol = np.asarray(vol, dtype=np.float64)
    p = vol.shape
    x = [np.broadcast_to(t, (P, P, P)) for t in _grid(p, frame, P, h)]
    if nearest:
        y = [t + 0.5 for t in x]
        ok = np.ones((P, P, P), dtype=bool)
        for i in range(3):
            ok &= (y[i] >= 0.0) & (y[i] < p[i])
        idx = [np.where(ok, np.floor(y[i]), 0).astype(np.int64) for i in range(3)]
        return np.where(ok, vol[idx[0], idx[1], idx[2]], 0.0)
    ok = np.ones((P, P, P), dtype=bool)
    for i in range(3):
        ok &= (x[i] > -1.0) & (x[i] < p[i])
    fl = [np.floor(t) for t in x]
    f = [x[i] - fl[i] for i in range(3)]
    i0 = [np.where(ok, fl[i], 0).astype(np.int64) + 1 for i in range(3)]   # index into the zero-bordered copy
    vp = np.zeros((p[0] + 2, p[1] + 2, p[2] + 2))
    vp[1:-1, 1:-1, 1:-1] = vol
    r = {}
    for di in (0, 1):
        for dj in (0, 1):
            a = vp[i0[0] + di, i0[1] + dj, i0[2]]
            b = vp[i0[0] + di, i0[1] + dj, i0[2] + 1]
            r[di, dj] = a + f[2] * (b - a)
    r0 = r[0, 0] + f[1] * (r[0, 1] - r[0, 0])
    r1 = r[1, 0] + f[1] * (r[1, 1] - r[1, 0])
    return np.where(ok, r0 + f[0] * (r1 - r0), 0.0)


def view_items(vol, frame, P, h, nearest):
    """((P,P,P) float32 slices as the dataset serves them, (P,) float64 per-slice maxima): images
    (nearest=False) are divided by their slice's max when it is non-zero, masks are not."""
    raw = sample_view(vol, frame, P, h, nearest)
    mx = raw.reshape(P, -1).max(1)
    if nearest:
        return raw.astype(np.float32), mx
    div = np.where(mx != 0.0, mx, 1.0)[:, None, None]
    return np.where((mx != 0.0)[:, None, None], raw / div, raw).astype(np.float32), mx


def fuse(stacks, frames, truth, P, h):
    """stacks (V,P,C,P,P) float32 probabilities, frames (V,3,3), truth (p0,p1,p2) labels ->
    avg (p0,C,p1,p2) f32, label (p0,p1,p2) i32, cover (p0,p1,p2) i32, counts (V+1,C,3) f64."""
    stacks = np.asarray(stacks, dtype=np.float32)
    V, _, C = stacks.shape[:3]
    p = truth.shape
    ii, jj, kk = np.meshgrid(*[np.arange(n, dtype=np.float64) for n in p], indexing="ij")
    total = np.zeros((C,) + p, dtype=np.float32)
    cover = np.zeros(p, dtype=np.int32)
    labels = []
    for v in range(V):
        g = voxel_to_grid(p, frames[v], P, h, ii, jj, kk)
        cov = np.ones(p, dtype=bool)
        for t in g:
            cov &= (t >= 0.0) & (t <= P - 1)
        fl = [np.where(cov, np.floor(t), 0.0) for t in g]
        w = [np.where(cov, t - f, 0.0).astype(np.float32) for t, f in zip(g, fl)]
        lo = [f.astype(np.int64) for f in fl]
        hi = [np.minimum(i + 1, P - 1) for i in lo]
        prob = np.zeros((C,) + p, dtype=np.float32)
        for c in range(C):
            q = stacks[v, :, c]
            x = {}
            for ds, s in ((0, lo[0]), (1, hi[0])):
                for da, a in ((0, lo[1]), (1, hi[1])):
                    x[ds, da] = q[s, a, lo[2]] + w[2] * (q[s, a, hi[2]] - q[s, a, lo[2]])
            y0 = x[0, 0] + w[1] * (x[0, 1] - x[0, 0])
            y1 = x[1, 0] + w[1] * (x[1, 1] - x[1, 0])
            prob[c] = y0 + w[0] * (y1 - y0)
            assert prob.dtype == np.float32
            total[c] = np.where(cov, total[c] + prob[c], total[c])
        labels.append(np.where(cov, np.argmax(prob, 0), 0).astype(np.int32))
        cover += cov
    avg = np.where(cover > 0, total / np.maximum(cover, 1).astype(np.float32), np.float32(0)).astype(np.float32)
    label = np.argmax(avg, 0).astype(np.int32)
    labels.append(label)
    t = np.asarray(truth).astype(np.int64)
    counts = np.zeros((V + 1, C, 3))
    for w_, lab in enumerate(labels):
        for c in range(C):
            counts[w_, c] = [np.sum((lab == c) & (t == c)), np.sum(lab == c), np.sum(t == c)]
    return np.ascontiguousarray(avg.transpose(1, 0, 2, 3)), label, cover, counts


def ball_round_trip(frames, P, h, size=32):
    """A ball of label 1 in size^3 (C = 2): its one-hot sliced along ``frames`` at the nearest voxel,
    the slices taken as predictions and fused.  Returns (truth, stacks (V,P,2,P,P), fuse(...))."""
    ax = np.arange(size) - (size - 1) / 2.0
    ii, jj, kk = np.meshgrid(ax, ax, ax, indexing="ij")
    truth = (ii ** 2 + jj ** 2 + kk ** 2 < (0.3 * size) ** 2).astype(np.float64)
    onehot = [(truth == c).astype(np.float64) for c in (0, 1)]
    stacks = np.stack([np.stack([view_items(onehot[c], f, P, h, True)[0] for c in (0, 1)], 1) for f in frames])
    return truth, stacks, fuse(stacks, frames, truth, P, h)
