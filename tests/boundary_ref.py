"""The boundary loss of include/pmunet_hip.h restated in numpy / torch (no test in here).

Signed map of one plane, from its boolean membership: 0 everywhere if there is no member or no non-member;
otherwise sqrt(min squared distance to a member) for a non-member and 1 - sqrt(min squared distance to a
non-member) for a member.  Squared distances are formed as integers (exact); the square root and the
subtraction are numpy float32 operations, each correctly rounded — the arithmetic the kernel is held to bit for
bit.  brute_plane takes the minimum over all seeds (small planes); separable_plane is the exact separable form
(rows by running nearest-seed index, columns by the minimum over all rows) for larger ones.

boundary_loss_ref is the loss formula in torch, in x's dtype, differentiable in x.
"""
import numpy as np
import torch

_FAR = 1 << 40   # "no seed": larger than any squared distance, small enough to add without overflow


def _compose(member, d2_to_member, d2_to_other):
    """phi of one plane from the two exact squared-distance fields (int64)."""
    if not member.any() or member.all():
        return np.zeros(member.shape, np.float32)
    d2 = np.where(member, d2_to_other, d2_to_member)
    assert d2.max() < 1 << 24            # exact in float32
    dist = np.sqrt(d2.astype(np.float32))
    assert dist.dtype == np.float32
    return np.where(member, np.float32(1) - dist, dist).astype(np.float32)


def _brute_d2(seeds):
    """min over seeds r of |q - r|^2 for every pixel q (int64; _FAR without a seed)."""
    H, W = seeds.shape
    ys, xs = np.nonzero(seeds)
    if ys.size == 0:
        return np.full((H, W), _FAR, np.int64)
    qy, qx = np.mgrid[0:H, 0:W]
    d2 = (qy[..., None] - ys) ** 2 + (qx[..., None] - xs) ** 2
    return d2.min(-1).astype(np.int64)


def brute_plane(member):
    member = np.asarray(member, bool)
    return _compose(member, _brute_d2(member), _brute_d2(~member))


def _row_d2(seeds):
    """squared distance along the row to the nearest seed of the row (int64; _FAR: none)."""
    H, W = seeds.shape
    idx = np.arange(W, dtype=np.int64)[None, :].repeat(H, 0)
    left = np.maximum.accumulate(np.where(seeds, idx, -_FAR), axis=1)
    right = np.minimum.accumulate(np.where(seeds, idx, _FAR)[:, ::-1], axis=1)[:, ::-1]
    r = np.minimum(idx - left, right - idx)
    return np.where(r >= _FAR // 2, _FAR, r * r)


def _separable_d2(seeds):
    H, W = seeds.shape
    r2 = _row_d2(seeds)
    rows = np.arange(H, dtype=np.int64)
    out = np.empty((H, W), np.int64)
    for y in range(H):
        out[y] = (((rows - y) ** 2)[:, None] + r2).min(0)
    return np.minimum(out, _FAR)


def separable_plane(member):
    member = np.asarray(member, bool)
    return _compose(member, _separable_d2(member), _separable_d2(~member))


def membership(target, K, ignore_index=-100):
    """(N, K, H, W) bool.  K >= 2: target (N, H, W) integers, member of k iff t == k and t != ignore_index.
    K == 1: target (N, 1, H, W) or (N, H, W) floats, member iff t >= 0.5."""
    t = target.detach().cpu().numpy() if isinstance(target, torch.Tensor) else np.asarray(target)
    if K == 1:
        t = t.reshape(t.shape[0], t.shape[-2], t.shape[-1])
        return (t >= 0.5)[:, None]
    return np.stack([(t == k) & (t != ignore_index) for k in range(K)], 1)


def signed_map(target, K, ignore_index=-100, plane=separable_plane):
    """The (N, K, H, W) float32 signed distance map of a target batch, as a torch tensor."""
    m = membership(target, K, ignore_index)
    out = np.stack([np.stack([plane(m[n, k]) for k in range(K)]) for n in range(m.shape[0])])
    return torch.from_numpy(out)


def boundary_terms(x, t, phi, include_background=False, ignore_index=-100, from_logits=None):
    """(v p_k phi_k over the included classes (N, K', HW), cnt) in x's dtype."""
    N, K = x.shape[0], x.shape[1]
    f = phi.to(x.dtype).reshape(N, K, -1)
    if K == 1:
        p = x.reshape(N, 1, -1)
        if from_logits:
            p = torch.sigmoid(p)
        valid = torch.ones(N, 1, p.shape[-1], dtype=x.dtype)
        first = 0
    else:
        p = torch.softmax(x.reshape(N, K, -1), 1)
        valid = (t.reshape(N, -1) != ignore_index).to(x.dtype)[:, None]
        first = 0 if include_background else 1
    cnt = float(valid.sum()) * (K - first)
    return (valid * p * f)[:, first:], cnt


def boundary_loss_ref(x, t, phi, **kw):
    """L = (1 / cnt) sum v p_k phi_k, 0 when cnt == 0."""
    terms, cnt = boundary_terms(x, t, phi, **kw)
    return terms.sum() / cnt if cnt > 0 else terms.sum() * 0


def boundary_scale_ref(x, t, phi, **kw):
    """A = (1 / cnt) sum v |p_k phi_k|: the scale the value's error is measured on (the signed sum cancels)."""
    terms, cnt = boundary_terms(x, t, phi, **kw)
    return float(terms.abs().sum() / cnt) if cnt > 0 else 0.0
