"""Numpy restatement of the learned multi-planar fusion (DESIGN.md "Learned fusion"; csrc/fusion_fit.hip), the
yardstick of tests/test_fusion_fit_cpu.py and tests/test_fusion_fit_gpu.py.

Per voxel, in float64, one rounded operation at a time (numpy fuses nothing), in the kernels' order:
z_c = b_c; z_c = z_c + W[v,c] p_{v,c} for v in view order over the views that cover the voxel; m = max z;
s = sum_c exp(z_c - m) in class order; q_c = exp(z_c - m) / s; label = first maximum of z; t = (int)truth, fit
weight 0 outside [0, C), else w = cw[t]; l = w ((log s + m) - z_t); dz_c = w (q_c - [c == t]).  The standard
path transposes the three stacks into the view-0 frame; the oblique path takes geometry from
tests/oblique_ref.py and restates its fp32 trilinear read per view.  Also here: a Newton solver with the exact
Hessian (reference optima of the fit) and the seeded problems both test files use.
"""
import numpy as np

import oblique_ref as R


# ------------------------------------------------------------------ the views' probabilities on the voxel grid
def softmax32(x, axis):
    """fp32 softmax as csrc/pmu_fuse.h computes it: max, exp(x - max), the sum in class order, the quotient."""
    x = np.asarray(x, dtype=np.float32)
    x = np.moveaxis(x, axis, 0)
    m = x.max(0)
    e = np.exp(x - m).astype(np.float32)
    s = np.zeros_like(m)
    for c in range(x.shape[0]):
        s = s + e[c]
    return np.moveaxis((e / s).astype(np.float32), 0, axis)


def standard_probs(v0, v1, v2, logits=False):
    """v0 (D0,C,D1,D2), v1 (D1,C,D0,D2), v2 (D2,C,D0,D1) -> p (3,C,D0,D1,D2) float32 in the view-0 frame and the
    all-true cover (3,D0,D1,D2)."""
    st = [np.asarray(v, dtype=np.float32) for v in (v0, v1, v2)]
    if logits:
        st = [softmax32(v, 1) for v in st]
    p = np.stack([st[0].transpose(1, 0, 2, 3), st[1].transpose(1, 2, 0, 3), st[2].transpose(1, 2, 3, 0)])
    return np.ascontiguousarray(p), np.ones((3,) + p.shape[2:], dtype=bool)


def oblique_probs(stacks, frames, shape, P, h):
    """stacks (V,P,C,P,P) -> p (V,C,p0,p1,p2) float32 (each view resampled as oblique_ref.fuse does, zeros where
    it does not cover) and cover (V,p0,p1,p2) bool."""
    stacks = np.asarray(stacks, dtype=np.float32)
    V, _, C = stacks.shape[:3]
    ii, jj, kk = np.meshgrid(*[np.arange(n, dtype=np.float64) for n in shape], indexing="ij")
    p = np.zeros((V, C) + tuple(shape), dtype=np.float32)
    cover = np.zeros((V,) + tuple(shape), dtype=bool)
    for v in range(V):
        g = R.voxel_to_grid(shape, frames[v], P, h, ii, jj, kk)
        cov = np.ones(shape, dtype=bool)
        for t in g:
            cov &= (t >= 0.0) & (t <= P - 1)
        fl = [np.where(cov, np.floor(t), 0.0) for t in g]
        w = [np.where(cov, t - f, 0.0).astype(np.float32) for t, f in zip(g, fl)]
        lo = [f.astype(np.int64) for f in fl]
        hi = [np.minimum(i + 1, P - 1) for i in lo]
        for c in range(C):
            q = stacks[v, :, c]
            x = {}
            for ds, s in ((0, lo[0]), (1, hi[0])):
                for da, a in ((0, lo[1]), (1, hi[1])):
                    x[ds, da] = q[s, a, lo[2]] + w[2] * (q[s, a, hi[2]] - q[s, a, lo[2]])
            y0 = x[0, 0] + w[1] * (x[0, 1] - x[0, 0])
            y1 = x[1, 0] + w[1] * (x[1, 1] - x[1, 0])
            r = y0 + w[0] * (y1 - y0)
            assert r.dtype == np.float32
            p[v, c] = np.where(cov, r, np.float32(0))
        cover[v] = cov
    return p, cover


# ------------------------------------------------------------------ the contract
def evaluate(p, cover, truth, W, b, cw=None):
    """p (V,C,...) float32, cover (V,...) bool, truth (...) labels, W (V,C), b (C,), cw (C,) or None.

    Returns a dict: z (C,...) float64, q (C,...) float64 (0 where no view covers), prob = q as float32 in the
    (D0,C,D1,D2) layout of the kernels' output, label int32, cover_n int32, counts (V+1,C,3) float64, sums (K,)
    float64 = [sum w, sum l, sum dz_c, sum dz_c p_{v,c}], abs_sums (K,) = the same sums of absolute terms, and
    top2 (...) = the gap between the two largest z."""
    p = np.asarray(p, dtype=np.float32)
    V, C = p.shape[:2]
    W = np.asarray(W, dtype=np.float64).reshape(V, C)
    b = np.asarray(b, dtype=np.float64).reshape(C)
    cw = np.ones(C) if cw is None else np.asarray(cw, dtype=np.float64).reshape(C)
    shape = p.shape[2:]
    z = np.empty((C,) + shape)
    for c in range(C):
        zc = np.full(shape, b[c])
        for v in range(V):
            zc = np.where(cover[v], zc + W[v, c] * p[v, c].astype(np.float64), zc)
        z[c] = zc
    m = z.max(0)
    e = np.exp(z - m)
    s = np.zeros(shape)
    for c in range(C):
        s = s + e[c]
    q = e / s
    label = np.argmax(z, 0).astype(np.int32)
    anyc = cover.any(0)
    q = np.where(anyc, q, 0.0)
    label = np.where(anyc, label, 0).astype(np.int32)
    t = np.trunc(np.asarray(truth, dtype=np.float64)).astype(np.int64)
    fit = anyc & (t >= 0) & (t < C)
    tc = np.clip(t, 0, C - 1)
    w = np.where(fit, cw[tc], 0.0)
    zt = np.take_along_axis(z, tc[None], 0)[0]
    ell = np.where(fit, w * ((np.log(s) + m) - zt), 0.0)
    onehot = (np.arange(C).reshape((C,) + (1,) * len(shape)) == tc[None]).astype(np.float64)
    dz = np.where(fit, w * (q - onehot), 0.0)
    terms = [w, ell] + [dz[c] for c in range(C)]
    terms += [np.where(cover[v], dz[c] * p[v, c].astype(np.float64), 0.0) for v in range(V) for c in range(C)]
    sums = np.array([float(np.sum(x)) for x in terms])
    abs_sums = np.array([float(np.sum(np.abs(x))) for x in terms])
    labels = [np.where(cover[v], np.argmax(p[v], 0), 0).astype(np.int32) for v in range(V)] + [label]
    counts = np.zeros((V + 1, C, 3))
    for w_, lab in enumerate(labels):
        for c in range(C):
            counts[w_, c] = [np.sum((lab == c) & (t == c)), np.sum(lab == c), np.sum(t == c)]
    zs = np.sort(z, 0)
    prob = q.astype(np.float32)
    if len(shape) == 3:
        prob = np.ascontiguousarray(prob.transpose(1, 0, 2, 3))
    return {"z": z, "q": q, "prob": prob, "label": label, "cover_n": cover.sum(0).astype(np.int32), "counts": counts,
            "sums": sums, "abs_sums": abs_sums, "top2": zs[-1] - zs[-2]}


def unpack(theta, V, C):
    theta = np.asarray(theta, dtype=np.float64)
    return theta[:V * C].reshape(V, C), theta[V * C:]


def objective(p, cover, truth, theta, cw=None, l2=0.0, theta0=None):
    """(f, g) of the fit: f = sum l / sum w + l2 / 2 ||theta - theta0||^2, theta = (W row by row, b)."""
    V, C = p.shape[:2]
    W, b = unpack(theta, V, C)
    s = evaluate(p, cover, truth, W, b, cw)["sums"]
    d = np.asarray(theta, dtype=np.float64) - (0.0 if theta0 is None else theta0)
    f = s[1] / s[0] + 0.5 * l2 * float(d @ d)
    g = np.concatenate([s[2 + C:], s[2:2 + C]]) / s[0] + l2 * d
    return f, g


def dice(counts):
    """(.., C) Dice 2 I / (|pred| + |truth|) of counts (.., C, 3); 1 where both are empty."""
    den = counts[..., 1] + counts[..., 2]
    return np.where(den > 0, 2.0 * counts[..., 0] / np.maximum(den, 1.0), 1.0)


# ------------------------------------------------------------------ Newton with the exact Hessian
def hessian(p, cover, truth, theta, cw=None, l2=0.0):
    V, C = p.shape[:2]
    W, b = unpack(theta, V, C)
    r = evaluate(p, cover, truth, W, b, cw)
    cwv = np.ones(C) if cw is None else np.asarray(cw, dtype=np.float64)
    t = np.trunc(np.asarray(truth, dtype=np.float64)).astype(np.int64).reshape(-1)
    fit = cover.any(0).reshape(-1) & (t >= 0) & (t < C)
    w = np.where(fit, cwv[np.clip(t, 0, C - 1)], 0.0)
    q = r["q"].reshape(C, -1).T                                       # (N, C)
    phi = np.concatenate([np.where(cover[:, None], p.astype(np.float64), 0.0).reshape(V, C, -1),
                          np.ones((1, C, q.shape[0]))]).transpose(2, 0, 1)        # (N, V+1, C)
    M = w[:, None, None] * (q[:, :, None] * np.eye(C)[None] - q[:, :, None] * q[:, None, :])
    H = np.einsum("nac,ncd,nbd->acbd", phi, M, phi).reshape((V + 1) * C, (V + 1) * C) / r["sums"][0]
    return H + l2 * np.eye((V + 1) * C)


def newton(p, cover, truth, theta0, cw=None, l2=0.0, gtol=1e-12, max_iter=100):
    """The optimum of objective(...) by damped Newton steps with the exact Hessian.  Returns (theta, f, g)."""
    theta0 = np.asarray(theta0, dtype=np.float64)
    x = theta0.copy()
    f, g = objective(p, cover, truth, x, cw, l2, theta0)
    for _ in range(max_iter):
        if np.max(np.abs(g)) < gtol:
            break
        d = -np.linalg.solve(hessian(p, cover, truth, x, cw, l2), g)
        step = 1.0
        while step > 1e-6:
            fn, gn = objective(p, cover, truth, x + step * d, cw, l2, theta0)
            if fn <= f + 1e-4 * step * float(g @ d) + 1e-15:
                break
            step *= 0.5
        x, f, g = x + step * d, fn, gn
    return x, f, g


# ------------------------------------------------------------------ the seeded problems of both test files
def fit_problem(seed=0, shape=(5, 37, 34), sigma=(0.5, 1.5, 3.0)):
    """The fit problem: C = 3, a striped truth with 60 % forced background, view v = softmax(2 onehot(t) +
    sigma_v N(0,1)), class 1 of view 2 biased by +1.  Returns (v0, v1, v2, truth): the stacks in fuse_views'
    layouts (float32 probabilities) and the (D0,D1,D2) float32 truth."""
    rs = np.random.RandomState(seed)
    D0, D1, D2 = shape
    ii, jj, kk = np.meshgrid(np.arange(D0), np.arange(D1), np.arange(D2), indexing="ij")
    truth = ((ii + jj // 3 + kk // 4) % 3).astype(np.int64)
    truth[rs.uniform(size=shape) < 0.6] = 0
    onehot = (np.arange(3)[:, None, None, None] == truth[None]).astype(np.float64)
    views = []
    for v, sg in enumerate(sigma):
        x = 2.0 * onehot + sg * rs.standard_normal((3,) + shape)
        if v == 2:
            x[1] += 1.0
        x = x - x.max(0)
        e = np.exp(x)
        views.append((e / e.sum(0)).astype(np.float32))                # (C, D0, D1, D2)
    v0 = np.ascontiguousarray(views[0].transpose(1, 0, 2, 3))          # (D0, C, D1, D2)
    v1 = np.ascontiguousarray(views[1].transpose(2, 0, 1, 3))          # (D1, C, D0, D2)
    v2 = np.ascontiguousarray(views[2].transpose(3, 0, 1, 2))          # (D2, C, D0, D1)
    return v0, v1, v2, truth.astype(np.float32)


def standard_case(shape, C, seed, logits=False):
    """Seeded stacks (probabilities, or N(0, 3^2) logits), truth with a few labels outside [0, C), W and b with
    negative entries and class weights with one zero."""
    rs = np.random.RandomState(seed)
    D0, D1, D2 = shape
    dims = ((D0, C, D1, D2), (D1, C, D0, D2), (D2, C, D0, D1))
    if logits:
        st = [(3.0 * rs.standard_normal(d)).astype(np.float32) for d in dims]
    else:
        st = []
        for d in dims:
            x = rs.uniform(0.05, 1.0, size=d).astype(np.float32)
            st.append(x / x.sum(1, keepdims=True))
    truth = rs.randint(0, C, size=shape).astype(np.float32)
    flat = truth.reshape(-1)
    n = flat.size
    if n >= 100:
        flat[rs.randint(0, n, size=n // 50)] = C              # outside [0, C): no fit weight
        flat[rs.randint(0, n, size=n // 70)] = -1.0
    W = rs.uniform(-1.0, 2.0, size=(3, C))
    W[rs.randint(0, 3), rs.randint(0, C)] = -0.75
    b = rs.uniform(-0.5, 0.5, size=C)
    b[0] = -0.25
    cw = rs.uniform(0.5, 2.0, size=C)
    cw[C - 1] = 0.0
    return st, truth, W, b, cw


def oblique_case(shape, P, V, C, seed):
    """Seeded oblique problem: (stacks (V,P,C,P,P) probabilities, frames (V,3,3), truth, W, b, cw)."""
    from utils.mri_dataset import draw_views, view_frame
    rs = np.random.RandomState(seed)
    frames = np.stack([view_frame(n) for n in draw_views(V, seed, 30)])
    st = rs.uniform(0.05, 1.0, size=(V, P, C, P, P)).astype(np.float32)
    st = st / st.sum(2, keepdims=True)
    truth = rs.randint(0, C, size=shape).astype(np.float32)
    flat = truth.reshape(-1)
    flat[rs.randint(0, flat.size, size=max(1, flat.size // 50))] = C
    W = rs.uniform(-1.0, 2.0, size=(V, C))
    W[rs.randint(0, V), rs.randint(0, C)] = -0.75
    b = rs.uniform(-0.5, 0.5, size=C)
    b[0] = -0.25
    cw = rs.uniform(0.5, 2.0, size=C)
    cw[C - 1] = 0.0
    return st, frames, truth, W, b, cw
