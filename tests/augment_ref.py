"""Numpy restatement of the warped batch gather (DESIGN.md "Augmentation"), the yardstick of
tests/test_augment_cpu.py and tests/test_augment_gpu.py.  The reference has no counterpart, so the operation
order is written out here and the kernel (csrc/augment.hip) follows it bit for bit: fp64 throughout, numpy
evaluating one rounded operation at a time (nothing fused), the plane coordinates, the cubic B-spline
displacement, the affine map and grid_to_voxel in exactly the order of the contract, then the sampler of
tests/oblique_ref.py (trilinear a + f (b - a) along axis 2, 1, 0 for images, the voxel floor(x + 0.5) for
masks, zeros outside) at the warped positions.

An item is (padded image volume, padded mask volume, frame (3,3) rows n u v, par (9,) = [ds, m00, m01, m10,
m11, ta, tb, gain, bias], ctrl (2,G,G) or None, m = the un-warped slice's image maximum or None).
"""
import numpy as np

IDENTITY = np.array([0.0, 1.0, 0.0, 0.0, 1.0, 0.0, 0.0, 1.0, 0.0])


def spline_cell(p, n, G):
    """(cell index i, weights (4, len(p))) of the output indices ``p`` (float64 array) of an axis of n pixels
    over a G-point control grid: uniform cubic B-spline, u = p ((G-3) / (n-1)), i = min(floor(u), G-4)."""
    p = np.asarray(p, dtype=np.float64)
    u = p * (float(G - 3) / float(n - 1))
    i = np.minimum(np.floor(u).astype(np.int64), G - 4)
    t = u - i
    omt, t2 = 1.0 - t, t * t
    t3 = t2 * t
    w0 = ((omt * omt) * omt) / 6.0
    w1 = ((3.0 * t3 - 6.0 * t2) + 4.0) / 6.0
    w2 = (((-3.0 * t3 + 3.0 * t2) + 3.0 * t) + 1.0) / 6.0
    w3 = t3 / 6.0
    return i, np.stack([w0, w1, w2, w3])


def displacement(ctrl, H, W):
    """(2, H, W): the B-spline plane displacement of every pixel; zeros without a control grid."""
    if ctrl is None or np.shape(ctrl)[-1] == 0:
        return np.zeros((2, H, W))
    ctrl = np.asarray(ctrl, dtype=np.float64)
    G = ctrl.shape[-1]
    ia, wa = spline_cell(np.arange(H), H, G)
    ib, wb = spline_cell(np.arange(W), W, G)
    wa, wb = wa[:, :, None], wb[:, None, :]
    out = np.empty((2, H, W))
    for k in range(2):
        acc = None
        for i in range(4):
            c = [ctrl[k][ia[:, None] + i, ib[None, :] + j] for j in range(4)]
            r = ((wb[0] * c[0] + wb[1] * c[1]) + wb[2] * c[2]) + wb[3] * c[3]
            acc = wa[0] * r if i == 0 else acc + wa[i] * r
        out[k] = acc
    return out


def warp_positions(pshape, frame, H, W, h, par, ctrl):
    """Voxel coordinates (x0, x1, x2), each (H, W), of the item's output pixels."""
    ds, m00, m01, m10, m11, ta, tb = [float(v) for v in par[:7]]
    pa = (h * (np.arange(H, dtype=np.float64) - (H - 1) / 2.0))[:, None]
    pb = (h * (np.arange(W, dtype=np.float64) - (W - 1) / 2.0))[None, :]
    d = displacement(ctrl, H, W)
    pa2, pb2 = pa + d[0], pb + d[1]
    qa = (m00 * pa2 + m01 * pb2) + ta
    qb = (m10 * pa2 + m11 * pb2) + tb
    n, u, v = np.asarray(frame, dtype=np.float64)
    return tuple((pshape[i] - 1) / 2.0 + ((ds * n[i] + qa * u[i]) + qb * v[i]) for i in range(3))


def sample_points(vol, x, nearest):
    """float64 samples of the padded volume at the voxel coordinates x = (x0, x1, x2) (equal shapes):
    tests/oblique_ref.py's sampler for arbitrary positions."""
    vol = np.asarray(vol, dtype=np.float64)
    p = vol.shape
    shape = np.broadcast(*x).shape
    x = [np.broadcast_to(t, shape) for t in x]
    ok = np.ones(shape, dtype=bool)
    if nearest:
        y = [t + 0.5 for t in x]
        for i in range(3):
            ok &= (y[i] >= 0.0) & (y[i] < p[i])
        idx = [np.where(ok, np.floor(y[i]), 0).astype(np.int64) for i in range(3)]
        return np.where(ok, vol[idx[0], idx[1], idx[2]], 0.0)
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


def warp_item(img, mask, frame, H, W, h, par, ctrl=None, m=None):
    """((H,W) float32 image, (H,W) float32 mask) of one item, as pmu_warp_gather writes them."""
    x = warp_positions(np.shape(img), frame, H, W, h, par, ctrl)
    raw = sample_points(img, x, False)
    y = raw / m if (m is not None and m != 0.0) else raw
    image = (y * float(par[7]) + float(par[8])).astype(np.float32)
    return image, sample_points(mask, x, True).astype(np.float32)


def slice_offset(h, s, P):
    """ds of slice s of a P-slice view at spacing h (the oblique path's h (s - (P-1)/2))."""
    return h * (s - (P - 1) / 2.0)


def block(ds=0.0, M=((1.0, 0.0), (0.0, 1.0)), t=(0.0, 0.0), gain=1.0, bias=0.0):
    """A hand-built parameter block."""
    return np.array([ds, M[0][0], M[0][1], M[1][0], M[1][1], t[0], t[1], gain, bias], dtype=np.float64)
