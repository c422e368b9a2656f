"""GPU parity of the BatchNorm2d bookkeeping kernels (nn.BatchNorm2d at PMU/model/unet/unet_parts.py:16,19)
against fp64 references on the CPU:

  pmu_colsum_f64       fp32 per-tile partials -> fp64 group sums
  pmu_bn_fwd_finalize  group sums -> mean, invstd, [scale | shift], running statistics, the batch counter
  pmu_bn_bwd_finalize  group sums of (g, g xhat) -> dgamma, dbeta, dbias and the [scale|shift|mean|kx|kc]
                       block every BN-backward consumer reads
  pmu_bn_eval_coef     running statistics -> [scale | shift]

The kernels take eps and momentum as C floats, so the references use the fp32 values of 1e-5 and 0.1.
Tolerances: a result computed in fp64 and stored in fp32 is within 2^-24 relative of the fp64 value;
the tests allow twice that (2^-23).  pmu_bn_eval_coef computes in fp32 (six operations): 1e-6.
"""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

EPS = float(np.float32(1e-5))
ULP2 = 2.0 ** -23
SENTINEL = 12345.0


def _close(got, ref, scale, tol=ULP2):
    """|got - ref| <= tol * scale elementwise (scale: the magnitude the rounding is relative to)."""
    got, ref, scale = got.double().cpu(), ref.double().cpu(), scale.double().cpu()
    bad = (got - ref).abs() > tol * scale
    assert not bool(bad.any()), (int(bad.sum()), float(((got - ref).abs() / scale.clamp_min(1e-300)).max()))


def _with_sentinel(n, dev):
    t = torch.full((n + 1,), float("nan"), device=dev)
    t[n] = SENTINEL
    return t


# ----------------------------------------------------------------------------------------
# pmu_colsum_f64
# ----------------------------------------------------------------------------------------
def test_colsum_groups(dev):
    from pmu_hip import _lib as L
    lb = L.lib()
    assert [lb.pmu_colsum_groups(r) for r in (1, 7, 100, 127)] == [1, 1, 1, 1]
    assert [lb.pmu_colsum_groups(r) for r in (8192, 8200, 1 << 20)] == [128, 128, 128]
    for r in (128, 130, 1000, 8191):
        assert 1 <= lb.pmu_colsum_groups(r) <= min(r, 128)


@pytest.mark.parametrize("R,Wd,G", [(1, 2, 1), (7, 12, 1), (130, 130, 2), (100, 64, 100), (8200, 2080, 128),
                                    (100, 64, None), (130, 130, None), (8200, 2080, None)])
def test_colsum_f64(dev, R, Wd, G):
    """Summing fp32 values in fp64 is exact up to fp64 rounding: 1e-13 of the column's sum of |part|.
    G None: the engine's own group count for R."""
    from pmu_hip import _lib as L
    G = L.lib().pmu_colsum_groups(R) if G is None else G
    g = torch.Generator().manual_seed(R + Wd)
    part = (torch.randn(R, Wd, generator=g) * torch.logspace(-3, 3, Wd)).to(dev)
    out = torch.full((G, Wd), float("nan"), dtype=torch.float64, device=dev)
    L.call("pmu_colsum_f64", part.data_ptr(), R, Wd, out.data_ptr(), G, L.stream())
    torch.cuda.synchronize()
    p64 = part.double().cpu()
    _close(out.sum(0), p64.sum(0), p64.abs().sum(0), tol=1e-13)


# ----------------------------------------------------------------------------------------
# pmu_bn_fwd_finalize
# ----------------------------------------------------------------------------------------
def _groups(P, G, g):
    """G unequal, non-empty row ranges of P rows."""
    cuts = (torch.randperm(P - 1, generator=g)[:G - 1] + 1).sort().values.tolist() if G > 1 else []
    return list(zip([0] + cuts, cuts + [P]))


def _acc(cols, P, G, g, dev):
    """acc[G][2][C]: per-group fp64 sums of the two [P][C] column sets."""
    a, b = cols
    acc = torch.stack([torch.stack([a[r0:r1].sum(0), b[r0:r1].sum(0)]) for r0, r1 in _groups(P, G, g)])
    return acc.contiguous().to(dev)


def _z(P, C, g, max_ratio):
    """fp64 z[P][C]: channel c has std in [0.1, 10] and mean / std from 0 to max_ratio."""
    std = torch.logspace(-1, 1, C, dtype=torch.float64)[torch.randperm(C, generator=g)]
    ratio = torch.linspace(0, max_ratio, C, dtype=torch.float64) if C > 1 else torch.tensor([max_ratio / 2], dtype=torch.float64)
    return (torch.randn(P, C, generator=g, dtype=torch.float64) + ratio) * std


def _fwd_finalize(acc, G, C, count, gamma, beta, momentum, rm, rv, nbt, dev):
    from pmu_hip import _lib as L
    mean, invstd, coef = _with_sentinel(C, dev), _with_sentinel(C, dev), _with_sentinel(2 * C, dev)
    L.call("pmu_bn_fwd_finalize", acc.data_ptr(), G, C, float(count), L.ptr(gamma), L.ptr(beta), EPS, float(momentum),
           L.ptr(rm), L.ptr(rv), L.ptr(nbt), mean.data_ptr(), invstd.data_ptr(), coef.data_ptr(), L.stream())
    torch.cuda.synchronize()
    for t, n in ((mean, C), (invstd, C), (coef, 2 * C)):
        assert float(t[n]) == SENTINEL and not bool(torch.isnan(t[:n]).any())
    return mean[:C], invstd[:C], coef[:2 * C]


def _check_fwd(z, mean, invstd, coef, gamma, beta):
    C = z.shape[1]
    m = z.mean(0)
    var = z.var(0, unbiased=False) if z.shape[0] > 1 else torch.zeros(C, dtype=torch.float64)
    istd = 1.0 / torch.sqrt(var + EPS)
    gm = gamma.double().cpu() if gamma is not None else torch.ones(C, dtype=torch.float64)
    bt = beta.double().cpu() if beta is not None else torch.zeros(C, dtype=torch.float64)
    _close(mean, m, m.abs())
    _close(invstd, istd, istd)
    _close(coef[:C], gm * istd, (gm * istd).abs())
    _close(coef[C:], bt - m * gm * istd, torch.maximum(bt.abs(), (m * gm * istd).abs()))
    return m, var


@pytest.mark.parametrize("G", [1, 3, 128])
@pytest.mark.parametrize("C", [1, 6, 64, 1040])
def test_bn_fwd_finalize(dev, C, G):
    """Statistics, coefficients and the running-statistics update (unbiased variance, momentum 0.1 and
    1.0, the counter 5 -> 6) from group sums of an fp64 z whose channels have mean / std from 0 to 100."""
    g = torch.Generator().manual_seed(100 * C + G)
    P = 300
    z = _z(P, C, g, 100.0)
    acc = _acc((z, z * z), P, G, g, dev)
    gamma = (torch.rand(C, generator=g) + 0.5).to(dev)
    beta = (torch.randn(C, generator=g) * 0.3).to(dev)
    for momentum in (0.1, 1.0):
        rm0, rv0 = torch.randn(C, generator=g), torch.rand(C, generator=g) + 0.5
        rm, rv = _with_sentinel(C, dev), _with_sentinel(C, dev)
        rm[:C], rv[:C] = rm0.to(dev), rv0.to(dev)
        nbt = torch.tensor([5, 777], dtype=torch.int64, device=dev)
        mean, invstd, coef = _fwd_finalize(acc, G, C, P, gamma, beta, momentum, rm, rv, nbt, dev)
        m, var = _check_fwd(z, mean, invstd, coef, gamma, beta)
        mom = float(np.float32(momentum))
        want_rm = (1.0 - mom) * rm0.double() + mom * m
        want_rv = (1.0 - mom) * rv0.double() + mom * var * P / (P - 1)
        _close(rm[:C], want_rm, want_rm.abs())
        _close(rv[:C], want_rv, want_rv.abs())
        assert float(rm[C]) == SENTINEL and float(rv[C]) == SENTINEL
        assert nbt.tolist() == [6, 777]


@pytest.mark.parametrize("C,G", [(6, 3), (64, 1), (1040, 128)])
def test_bn_fwd_finalize_null_arguments(dev, C, G):
    """gamma = beta = NULL (scale = invstd, shift = -mean invstd); running_* = NULL with a counter (only
    the counter moves); running_* given without a counter."""
    g = torch.Generator().manual_seed(7 * C + G)
    P = 200
    z = _z(P, C, g, 100.0)
    acc = _acc((z, z * z), P, G, g, dev)
    nbt = torch.tensor([5, 777], dtype=torch.int64, device=dev)
    mean, invstd, coef = _fwd_finalize(acc, G, C, P, None, None, 0.1, None, None, nbt, dev)
    m, var = _check_fwd(z, mean, invstd, coef, None, None)
    assert nbt.tolist() == [6, 777]
    rm0, rv0 = torch.randn(C, generator=g), torch.rand(C, generator=g) + 0.5
    rm, rv = rm0.to(dev), rv0.to(dev)
    beta = (torch.randn(C, generator=g) * 0.3).to(dev)
    mean, invstd, coef = _fwd_finalize(acc, G, C, P, None, beta, 0.1, rm, rv, None, dev)
    _check_fwd(z, mean, invstd, coef, None, beta)
    mom = float(np.float32(0.1))
    want_rm = (1.0 - mom) * rm0.double() + mom * m
    want_rv = (1.0 - mom) * rv0.double() + mom * var * P / (P - 1)
    _close(rm, want_rm, want_rm.abs())
    _close(rv, want_rv, want_rv.abs())
    assert nbt.tolist() == [6, 777]


def test_bn_fwd_finalize_count_one_and_constant_channel(dev):
    """count == 1: no division by zero, the (zero) variance is used as it is for the running variance.
    A constant channel: var may come out a rounding error below zero and is clamped, invstd == 1/sqrt(eps).
    (The constants are 3.7 and -12.5: E[z^2] - mean^2 in fp64 leaves an absolute error of a few 2^-52 c^2,
    which against eps = 1e-5 stays below 2^-24 relative only for |c| up to some tens.)"""
    g = torch.Generator().manual_seed(3)
    C = 6
    z = _z(1, C, g, 100.0)
    acc = _acc((z, z * z), 1, 1, g, dev)
    rv0 = torch.rand(C, generator=g) + 0.5
    rm, rv = torch.zeros(C, device=dev), rv0.to(dev)
    mean, invstd, coef = _fwd_finalize(acc, 1, C, 1, None, None, 0.1, rm, rv, None, dev)
    one = torch.ones(C, dtype=torch.float64)
    _close(mean, z[0], z[0].abs())
    _close(invstd, one / EPS ** 0.5, one / EPS ** 0.5)
    _close(rv, (1.0 - float(np.float32(0.1))) * rv0.double(), rv0.double())
    assert bool(torch.isfinite(rm).all())
    P, G = 257, 3
    z = _z(P, C, g, 100.0)
    z[:, 2] = 3.7
    z[:, 4] = -12.5
    acc = _acc((z, z * z), P, G, g, dev)
    mean, invstd, coef = _fwd_finalize(acc, G, C, P, None, None, 0.1, None, None, None, dev)
    _check_fwd(z, mean, invstd, coef, None, None)
    for c in (2, 4):
        assert abs(float(invstd[c]) - EPS ** -0.5) <= ULP2 * EPS ** -0.5


# ----------------------------------------------------------------------------------------
# pmu_bn_bwd_finalize
# ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("affine", [True, False], ids=["gamma", "gamma_null"])
@pytest.mark.parametrize("G", [1, 3, 128])
@pytest.mark.parametrize("C", [1, 6, 64, 1040])
def test_bn_bwd_finalize(dev, C, G, affine):
    """y = relu(batch_norm(z)) in fp64 autograd gives dz, dgamma, dbeta; the kernel gets the fp64 partial
    sums (sum g, sum g xhat), g = da where y > 0, in G groups, and the fp32 coef / mean / invstd of
    pmu_bn_fwd_finalize.  dz = g scale + kx (z - mean) + kc from the returned block, in fp64, to
    1e-6 max|dz| (five fp32-stored coefficients of <= 2^-24 relative error each, times 4).  z has mean / std
    up to 3 here: the block holds the mean in fp32, so z - mean carries 2^-24 x mean / std of relative
    error, which that margin covers only for well-centred channels."""
    from pmu_hip import _lib as L
    g = torch.Generator().manual_seed(1000 * C + 10 * G + affine)
    P = 300
    z = _z(P, C, g, 3.0)
    da = torch.randn(P, C, generator=g, dtype=torch.float64)
    gamma = (torch.rand(C, generator=g) + 0.5) if affine else None
    beta = torch.randn(C, generator=g) * 0.3
    zr = z.clone().requires_grad_(True)
    gr = gamma.double().requires_grad_(True) if affine else None
    br = beta.double().requires_grad_(True)
    y = torch.relu(torch.nn.functional.batch_norm(zr, None, None, gr, br, True, 0.1, EPS))
    y.backward(da)
    dz_ref = zr.grad
    gd = gamma.to(dev) if affine else None
    acc_f = _acc((z, z * z), P, G, g, dev)
    mean, invstd, coef = _fwd_finalize(acc_f, G, C, P, gd, beta.to(dev), 0.1, None, None, None, dev)
    gm = da * (y.detach() > 0)
    xhat = (z - z.mean(0)) / torch.sqrt(z.var(0, unbiased=False) + EPS)
    acc = _acc((gm, gm * xhat), P, G, g, dev)
    dgamma = _with_sentinel(C, dev) if affine else None
    dbeta, dbias, bcoef = _with_sentinel(C, dev), _with_sentinel(C, dev), _with_sentinel(5 * C, dev)
    L.call("pmu_bn_bwd_finalize", acc.data_ptr(), G, C, float(P), L.ptr(gd), coef.data_ptr(), mean.data_ptr(),
           invstd.data_ptr(), L.ptr(dgamma), dbeta.data_ptr(), dbias.data_ptr(), bcoef.data_ptr(), L.stream())
    torch.cuda.synchronize()
    for t, n in ((dgamma, C), (dbeta, C), (dbias, C), (bcoef, 5 * C)):
        if t is not None:
            assert float(t[n]) == SENTINEL and not bool(torch.isnan(t[:n]).any())
    sc, sh, mu, kx, kc = bcoef[:5 * C].double().cpu().view(5, C)
    assert torch.equal(bcoef[:2 * C], coef) and torch.equal(bcoef[2 * C:3 * C], mean)
    dz = gm * sc + kx * (z - mu) + kc
    err, top = float((dz - dz_ref).abs().max()), float(dz_ref.abs().max())
    assert err <= 1e-6 * top, (err, top)
    if affine:
        _close(dgamma[:C], gr.grad, gr.grad.abs())
    _close(dbeta[:C], br.grad, br.grad.abs())
    _close(dbias[:C], dz_ref.sum(0), dz_ref.abs().sum(0), tol=1e-6)


# ----------------------------------------------------------------------------------------
# pmu_bn_eval_coef
# ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("affine", [True, False], ids=["affine", "null"])
@pytest.mark.parametrize("C", [1, 6, 256, 1040])
def test_bn_eval_coef(dev, C, affine):
    """[scale | shift] = [gamma / sqrt(rv + eps) | beta - rm scale] with running variances 0, 1e-12, 1 and
    1e6 mixed over the channels; six fp32 operations of <= 2^-24 relative error each: 1e-6."""
    from pmu_hip import _lib as L
    g = torch.Generator().manual_seed(C + affine)
    rv = torch.tensor([0.0, 1e-12, 1.0, 1e6])[torch.randint(0, 4, (C,), generator=g)]
    if C >= 4:
        rv[:4] = torch.tensor([0.0, 1e-12, 1.0, 1e6])
    rm = torch.randn(C, generator=g) * 3
    gamma = (torch.rand(C, generator=g) + 0.5) if affine else None
    beta = (torch.randn(C, generator=g) * 0.3) if affine else None
    coef = _with_sentinel(2 * C, dev)
    rmd, rvd = rm.to(dev), rv.to(dev)
    gd, bd = (gamma.to(dev), beta.to(dev)) if affine else (None, None)
    L.call("pmu_bn_eval_coef", rmd.data_ptr(), rvd.data_ptr(), L.ptr(gd), L.ptr(bd), EPS, C, coef.data_ptr(), L.stream())
    torch.cuda.synchronize()
    assert float(coef[2 * C]) == SENTINEL
    gm = gamma.double() if affine else torch.ones(C, dtype=torch.float64)
    bt = beta.double() if affine else torch.zeros(C, dtype=torch.float64)
    scale = gm / torch.sqrt(rv.double() + EPS)
    _close(coef[:C], scale, scale.abs(), tol=1e-6)
    _close(coef[C:2 * C], bt - rm.double() * scale, torch.maximum(bt.abs(), (rm.double() * scale).abs()), tol=1e-6)
