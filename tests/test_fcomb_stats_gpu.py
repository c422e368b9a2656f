"""pmu_fcomb_stats (csrc/fcomb.hip) by direct calls against a float64 reference: the mean class
probabilities, the predictive entropy, the mutual information and both label outputs of S samples, on both
last-layer paths of the kernel (VALU for K <= 4, MFMA up to K = 32 with its padded class rows), K = 1 (the
Bernoulli case), a feature width that is no multiple of 4, a latent width of 0 (all samples equal) and S = 1.

Method: the dyadic grid of tests/test_fcomb_abi_gpu.py (same draw order: w, b, wl, bl, feat, z), with the last
layer's weights and biases multiplied by 8: the ReLU masks of the fp32 kernel and of the float64 reference
stay identical, and the logits reach |y| ~ 2..7, so that the samples disagree and the reference mutual
information is far above its tolerance (asserted below: a kernel returning mi = 0 cannot pass).

Tolerances, from the project's Fcomb logit tolerance t_y = 1e-4 max(1, max|y_ref|) through the Lipschitz
constants of the maps: mean 0.5 t_y + 1e-6 (sum_j |dp_k/dy_j| <= 1/2), entropy 2 ln(max(K, 2)) t_y + 1e-5
(sum_j |dH/dy_j| = sum_j p_j |ln p_j + H| <= 2 H <= 2 ln K), mutual information twice the entropy bound.
The mean label is compared where the reference's top two mean probabilities differ by more than t_y, a sample's
label where its top two logits (K = 1: |y|) differ by more than 2 t_y; at most 2 % of a case's (sample-)pixels
may be left out that way.  Every output is NaN (0xFF for the u8 stack, -1 for the int32 map) on entry and is
followed by a sentinel tail; a second call passes both label pointers as NULL and must reproduce the other
three outputs bit for bit."""
import ctypes
import math

import pytest
import torch

pytestmark = pytest.mark.gpu

NAN = float("nan")
TAIL = 64
# (F, K, NH, Lz, N, H, W, S)
CASES = [
    (32, 3, 3, 6, 2, 9, 7, 16),    # the trainer's shape class, VALU path; HW = 63: groups straddle images, last partial
    (64, 32, 3, 6, 1, 33, 5, 3),   # MFMA path, all 32 class rows real
    (16, 5, 1, 12, 3, 4, 4, 7),    # MFMA path, 27 padded rows; class 4 lives in the other half-wave
    (30, 8, 2, 0, 2, 6, 11, 4),    # F % 4 != 0; L = 0: all samples equal, mi ~ 0
    (16, 1, 1, 12, 3, 4, 4, 5),    # K = 1: Bernoulli
    (64, 2, 3, 6, 1, 5, 5, 1),     # S = 1: mean = softmax, mi ~ 0
]


def _L():
    from pmu_hip import _lib as L
    return L


def _ptrs(ts):
    return (ctypes.c_void_p * 3)(*([t.data_ptr() for t in ts] + [None] * (3 - len(ts))))


def _problem(F, K, NH, Lz, N, H, W, S):
    """Quantised CPU fp32 tensors: w[l], b[l], wl, bl (both x 8), feat NHWC, z [S][N][Lz]."""
    g = torch.Generator().manual_seed(F + 3 * K + 5 * NH + 7 * Lz + N * H * W + 11 * S)
    qw = lambda *s: torch.randn(*s, generator=g).round().clamp(-2, 2) / 8
    qb = lambda *s: (torch.randn(*s, generator=g) * 1.6).round() / 16
    w = [qw(F, F + Lz if l == 0 else F) for l in range(NH)]
    b = [qb(F) for _ in range(NH)]
    wl, bl = qw(K, F), qb(K)
    feat = (torch.relu(torch.randn(N, H, W, F, generator=g)) * 4).round().clamp(0, 4) / 4
    z = (torch.randn(S, N, Lz, generator=g) * 4).round().clamp(-8, 8) / 4
    return w, b, wl * 8, bl * 8, feat, z


def _logits(w, b, wl, bl, feat, z):
    """float64 logits [S][N][K][H][W]."""
    N, H, W, F = feat.shape
    ys = []
    for zs in z.double():
        zt = zs[:, None, None, :].expand(N, H, W, zs.shape[1])
        h = torch.cat((feat.double(), zt), dim=3).reshape(N * H * W, -1)
        for wi, bi in zip(w, b):
            h = torch.relu(h @ wi.double().T + bi.double())
        ys.append((h @ wl.double().T + bl.double()).view(N, H, W, -1).permute(0, 3, 1, 2))
    return torch.stack(ys)


def _xlogx(p):
    return torch.where(p > 0, p * torch.log(p.clamp_min(1e-300)), torch.zeros_like(p))


def _reference(y):
    """float64 statistics of logits y [S][N][K][H][W]; for K = 1 the distributions are [1 - p, p]."""
    K = y.shape[2]
    if K == 1:
        p1 = torch.sigmoid(y)
        dist = torch.cat((1 - p1, p1), 2)                     # [S][N][2][H][W]
        mean_out = p1.mean(0)
        labels = (y[:, :, 0] > 0).to(torch.uint8)
        margin_s = y[:, :, 0].abs()
    else:
        dist = torch.softmax(y, 2)
        mean_out = dist.mean(0)
        labels = y.argmax(2).to(torch.uint8)
        top = y.topk(2, dim=2).values
        margin_s = top[:, :, 0] - top[:, :, 1]
    md = dist.mean(0)                                          # [N][K or 2][H][W]
    ent = -_xlogx(md).sum(1)
    hs = -_xlogx(dist).sum(2).mean(0)
    mi = (ent - hs).clamp_min(0)
    label = (mean_out[:, 0] > 0.5).int() if K == 1 else md.argmax(1).int()
    topm = md.topk(2, dim=1).values
    return dict(mean=mean_out, entropy=ent, mi=mi, label=label, labels=labels, margin=topm[:, 0] - topm[:, 1],
                margin_s=margin_s)


def _buf(shape, dtype, fill, tail_fill, dev):
    """A flat buffer of prod(shape) + TAIL elements: (view of the payload, the whole buffer)."""
    n = math.prod(shape)
    whole = torch.empty(n + TAIL, dtype=dtype, device=dev)
    whole[:n] = fill
    whole[n:] = tail_fill
    return whole[:n].view(*shape), whole


@pytest.mark.parametrize("F,K,NH,Lz,N,H,W,S", CASES)
def test_fcomb_stats_vs_fp64(dev, F, K, NH, Lz, N, H, W, S):
    L = _L()
    w, b, wl, bl, feat, z = _problem(F, K, NH, Lz, N, H, W, S)
    zb = torch.einsum("ol,snl->sno", w[0][:, F:].double(), z.double()) + b[0].double()
    assert torch.equal(zb.float().double(), zb)                      # exact on the dyadic grid
    y = _logits(w, b, wl, bl, feat, z)
    ref = _reference(y)
    t_y = 1e-4 * max(1.0, float(y.abs().max()))
    tol_mean = 0.5 * t_y + 1e-6
    tol_ent = 2 * math.log(max(K, 2)) * t_y + 1e-5
    tol_mi = 2 * tol_ent
    # conditions on the reference alone, so that the tolerances mean something
    if S > 1 and Lz > 0:
        assert float(ref["mi"].max()) >= 20 * tol_mi, (float(ref["mi"].max()), tol_mi)
    keep = ref["margin"] > t_y
    keep_s = ref["margin_s"] > 2 * t_y
    assert float((~keep).float().mean()) <= 0.02 and float((~keep_s).float().mean()) <= 0.02

    wd, bd = [t.to(dev) for t in w], [t.to(dev) for t in b]
    wld, bld, fd, zbd = wl.to(dev), bl.to(dev), feat.to(dev), zb.float().to(dev)
    s = L.stream()

    def run(with_labels):
        mean, mean_w = _buf((N, K, H, W), torch.float32, NAN, -7.0, dev)
        ent, ent_w = _buf((N, H, W), torch.float32, NAN, -7.0, dev)
        mi, mi_w = _buf((N, H, W), torch.float32, NAN, -7.0, dev)
        label, label_w = _buf((N, H, W), torch.int32, -1, -7, dev)
        labels, labels_w = _buf((S, N, H, W), torch.uint8, 0xFF, 0xA5, dev)
        L.call("pmu_fcomb_stats", fd.data_ptr(), zbd.data_ptr(), _ptrs(wd), _ptrs(bd), wld.data_ptr(), bld.data_ptr(),
               F, Lz, K, NH, S, N, H, W, mean.data_ptr(), ent.data_ptr(), mi.data_ptr(),
               label.data_ptr() if with_labels else None, labels.data_ptr() if with_labels else None, s)
        torch.cuda.synchronize()
        for name, whole, n, tf in (("mean", mean_w, mean.numel(), -7.0), ("entropy", ent_w, ent.numel(), -7.0),
                                   ("mi", mi_w, mi.numel(), -7.0), ("label", label_w, label.numel(), -7),
                                   ("labels", labels_w, labels.numel(), 0xA5)):
            assert bool((whole[n:] == tf).all()), f"the tail of {name} was written"
        return mean, ent, mi, label, labels

    mean, ent, mi, label, labels = run(True)
    worst = {}
    for name, got, want, tol in (("mean", mean, ref["mean"], tol_mean), ("entropy", ent, ref["entropy"], tol_ent),
                                 ("mi", mi, ref["mi"], tol_mi)):
        assert not torch.isnan(got).any(), f"{name}: an element was not written"
        e = float((got.double().cpu() - want).abs().max())
        worst[name] = e / tol
        print(f"fcomb_stats {(F, K, NH, Lz, N, H, W, S)} {name}: err {e:.3e} tol {tol:.3e} ({e / tol:.4f} of it), "
              f"max|ref| {float(want.abs().max()):.4f}")
    for name, tol in (("mean", tol_mean), ("entropy", tol_ent), ("mi", tol_mi)):
        assert worst[name] <= 1.0, (name, worst[name], tol)
    assert float(mi.min()) >= 0.0
    if S == 1 or Lz == 0:
        assert float(mi.max()) <= tol_mi
    if S == 1:
        assert float((mean.double().cpu() - ref["mean"]).abs().max()) <= tol_mean   # the softmax itself

    lab, labs = label.cpu(), labels.cpu()
    assert int(lab.min()) >= 0 and int(lab.max()) < max(K, 2), "label: an element was not written"
    assert int(labs.max()) < max(K, 2), "labels: an element was not written"
    assert torch.equal(lab[keep], ref["label"][keep])
    assert torch.equal(labs[keep_s], ref["labels"][keep_s])
    print(f"fcomb_stats {(F, K, NH, Lz, N, H, W, S)}: left out {float((~keep).float().mean()):.4f} of the mean labels, "
          f"{float((~keep_s).float().mean()):.4f} of the sample labels")

    mean2, ent2, mi2, label2, labels2 = run(False)
    assert torch.equal(mean2, mean) and torch.equal(ent2, ent) and torch.equal(mi2, mi)
    assert bool((label2 == -1).all()) and bool((labels2 == 0xFF).all())   # NULL: not written through a stale pointer


@pytest.mark.parametrize("F,K,NH,Lz,N,H,W,S", CASES)
def test_fcomb_stats_labels_are_the_argmax_of_the_forward_logits(dev, F, K, NH, Lz, N, H, W, S):
    """pmu_fcomb_fwd and pmu_fcomb_stats run one chain: the u8 labels stack is the first-maximum argmax of the
    forward's fp32 logits (K = 1: y > 0) at every pixel of every sample, bit for bit — both kernels form the
    logits with the same operations in the same order, so there is no reference, tolerance or margin here."""
    L = _L()
    w, b, wl, bl, feat, z = _problem(F, K, NH, Lz, N, H, W, S)
    zb = (torch.einsum("ol,snl->sno", w[0][:, F:].double(), z.double()) + b[0].double()).float().to(dev)
    wd, bd = [t.to(dev) for t in w], [t.to(dev) for t in b]
    wld, bld, fd = wl.to(dev), bl.to(dev), feat.to(dev)
    s = L.stream()
    y = torch.full((S, N, K, H, W), NAN, device=dev)
    L.call("pmu_fcomb_fwd", fd.data_ptr(), zb.data_ptr(), _ptrs(wd), _ptrs(bd), wld.data_ptr(), bld.data_ptr(),
           F, Lz, K, NH, S, N, H, W, y.data_ptr(), s)
    mean, ent, mi = (torch.empty(n, device=dev) for n in (N * K * H * W, N * H * W, N * H * W))
    labels = torch.full((S, N, H, W), 0xFF, dtype=torch.uint8, device=dev)
    L.call("pmu_fcomb_stats", fd.data_ptr(), zb.data_ptr(), _ptrs(wd), _ptrs(bd), wld.data_ptr(), bld.data_ptr(),
           F, Lz, K, NH, S, N, H, W, mean.data_ptr(), ent.data_ptr(), mi.data_ptr(), None, labels.data_ptr(), s)
    torch.cuda.synchronize()
    assert not torch.isnan(y).any()
    want = (y[:, :, 0] > 0) if K == 1 else y.argmax(2)       # (torch.argmax returns the first maximum)
    if K > 1:                                                # ... which is asserted, not assumed
        first = (y == y.max(2, keepdim=True).values).int().cumsum(2).eq(0).sum(2)
        assert torch.equal(want, first)
    assert torch.equal(labels, want.to(torch.uint8))


def test_fcomb_stats_refuses_shapes_outside_the_abi(dev):
    L = _L()
    F, K, NH, Lz, N, H, W, S = CASES[2]
    big = torch.zeros(1 << 16, device=dev)                           # stands in for every operand
    p3 = _ptrs([big, big, big])
    out = torch.full((1 << 16,), NAN, device=dev)
    lib, s, bad, p, o = L.lib(), L.stream(), L.PMU_ERR_ARG, big.data_ptr(), out.data_ptr()

    def stats(F, K, NH, S=S, mean=o):
        return lib.pmu_fcomb_stats(p, p, p3, p3, p, p, F, Lz, K, NH, S, N, H, W, mean, o, o, None, None, s)

    for args in ((16, 33, 1), (65, 5, 1), (16, 5, 0), (16, 5, 4), (16, 0, 1)):   # K = 33, F = 65, NH = 0, 4, K = 0
        assert stats(*args) == bad, args
    assert stats(16, 5, 1, S=0) == bad
    assert stats(16, 5, 1, mean=None) == bad
    torch.cuda.synchronize()
    assert torch.isnan(out).all()                                    # nothing was launched
