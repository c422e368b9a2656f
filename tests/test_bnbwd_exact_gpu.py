"""The fused BatchNorm+ReLU backward passes of csrc/bn.hip and csrc/pool_bwd.hip held to float64, bit for bit: the
partial-sum reductions (pmu_bn_bwd_reduce{,_dxb}) and the encoder's AvgPool2d / spatial-mean backward forms
(pmu_avgpool2_bwd_bnr, pmu_spatial_mean_bwd_bnr) of bn.hip; MaxPool2d(2) backward fused with the sums
(pmu_maxpool2_bwd_bnr{,_dxb,_stats,_stats_dxb}) and with the layer's dz (pmu_maxpool2_bwd_bnbwd{,_dxb}) of pool_bwd.hip.

Inputs and references come from tests/bnbwd_cases.py (grids on which every product and every partial sum is an
fp32 number; tests/test_glue_exact_cpu.py checks the conditions without a GPU).  For every case: exact_headroom
holds for both sums, from the reference alone; da / dx equals the float64 reference exactly; part equals the
float64 sums of every row block (the tilings the kernels document), row by row; dz of the _bnbwd forms equals
ref_frame of Src(da_ref, BNBWD, bcoef, z) — fp32 exactly, bf16 as the reference's round-to-nearest-even bits.
Outputs are pre-filled with NaN / -7 and every call runs twice for identical bits.  No tolerance anywhere."""
import pytest
import torch

from bnbwd_cases import BNBWD_SHAPES, MEAN_SHAPES, REDUCE_SHAPES, SHAPES, inputs, ref_dz, ref_sums
from helpers import assert_exact, assert_rne_exercised, bf16_bits, bf16_exact, exact_headroom

pytestmark = pytest.mark.gpu
NAN = float("nan")


def _ids(shapes):
    return ["x".join(map(str, s)) for s in shapes]


class Dev:
    """One shape's inputs on the device (fp32, and bf16 bits of the gradients for the *_dxb entries)."""

    def __init__(self, i, dev):
        for k in ("z", "coef", "mean", "invstd", "da", "dpool", "skip", "bcoef", "dpool_avg", "dmean"):
            setattr(self, k, getattr(i, k).contiguous().to(dev))
        for k in ("da", "dpool", "skip"):
            assert bf16_exact(getattr(i, k)), k     # the bf16 storage holds exactly what the reference reads
            setattr(self, k + "_b", bf16_bits(getattr(i, k)).contiguous().to(dev))
        assert bf16_exact(i.z)


def _same_bits(a, b):
    return torch.equal(a.view(torch.int32) if a.dtype == torch.float32 else a, b.view(torch.int32) if b.dtype == torch.float32 else b)


def _twice(fn):
    """fn() -> tuple of output tensors; run twice, identical bits required."""
    a, b = fn(), fn()
    torch.cuda.synchronize()
    for x, y in zip(a, b):
        assert _same_bits(x, y), "two runs differ"
    return a


def _z_has_ties(i):
    """quant_z's purpose, asserted on the inputs actually used (maps with at least 256 window-channels): values
    exactly at the ReLU threshold, windows whose maximum is attained twice, and all-zero windows."""
    Hp, Wp = i.H // 2, i.W // 2
    if i.N * Hp * Wp * i.C < 256:
        return
    pre = i.z.double() * i.coef[:i.C].double() + i.coef[i.C:].double()
    assert int((pre == 0).sum()) > 0
    win = pre.clamp_min(0)[:, :2 * Hp, :2 * Wp].reshape(i.N, Hp, 2, Wp, 2, i.C).permute(0, 1, 3, 5, 2, 4).reshape(-1, 4)
    top = win.topk(2, dim=1).values
    assert int(((top[:, 0] == top[:, 1]) & (top[:, 0] > 0)).sum()) > 0 and int((top[:, 0] == 0).sum()) > 0


def _check_part(part, kind, i, R, where):
    """part (R, 2 * C) from a kernel against the float64 row-block sums; returns the float64 da of the case."""
    da, ref, absp, ug, ugx = ref_sums(kind, i)
    exact_headroom(absp[:, 0], ug, where + ": sum g")
    exact_headroom(absp[:, 1], ugx, where + ": sum g * xhat")
    assert R == ref.shape[0], f"{where}: {R} rows of partial sums, the documented tiling has {ref.shape[0]}"
    assert_exact(part.view(R, 2, i.C), ref, where + ": part")
    return da


# ------------------------------------------------------------------------------------------ reductions
@pytest.mark.parametrize("shape", REDUCE_SHAPES, ids=_ids(REDUCE_SHAPES))
def test_bn_bwd_reduce(dev, shape):
    from pmu_hip import _lib as L
    i = inputs(*shape)
    d = Dev(i, dev)
    P = i.N * i.H * i.W
    R = L.lib().pmu_bn_bwd_tiles(P, i.C)

    def run():
        part = torch.full((R, 2 * i.C), NAN, device=dev)
        L.call("pmu_bn_bwd_reduce", d.da.data_ptr(), d.z.data_ptr(), d.coef.data_ptr(), d.mean.data_ptr(),
               d.invstd.data_ptr(), P, i.C, part.data_ptr(), L.stream())
        return (part,)
    _z_has_ties(i)
    _check_part(_twice(run)[0], "reduce", i, R, f"pmu_bn_bwd_reduce {shape}")


@pytest.mark.parametrize("shape", SHAPES + REDUCE_SHAPES[-2:], ids=_ids(SHAPES + REDUCE_SHAPES[-2:]))
def test_bn_bwd_reduce_dxb(dev, shape):
    from pmu_hip import _lib as L
    i = inputs(*shape)
    d = Dev(i, dev)
    P = i.N * i.H * i.W
    R = L.lib().pmu_bn_bwd_tiles(P, i.C)

    def run():
        part = torch.full((R, 2 * i.C), NAN, device=dev)
        L.call("pmu_bn_bwd_reduce_dxb", d.da_b.data_ptr(), d.z.data_ptr(), d.coef.data_ptr(), d.mean.data_ptr(),
               d.invstd.data_ptr(), P, i.C, part.data_ptr(), L.stream())
        return (part,)
    _check_part(_twice(run)[0], "reduce", i, R, f"pmu_bn_bwd_reduce_dxb {shape}")


# ------------------------------------------------------------------------------------------ max-pool backward
@pytest.mark.parametrize("accumulate", [1, 0])
@pytest.mark.parametrize("shape", SHAPES, ids=_ids(SHAPES))
def test_maxpool2_bwd_bnr(dev, shape, accumulate):
    """accumulate = 0 on an odd map: mp_route stores every in-map element of a ceil-sized window (ok[k]), the
    routed gradient of a partial window being 0 (gv = 0 unless `full`), so the odd last row / column is written
    as 0, not left — the NaN pre-fill must be gone everywhere."""
    from pmu_hip import _lib as L
    i = inputs(*shape)
    d = Dev(i, dev)
    R = L.lib().pmu_maxpool2_bwd_bnr_tiles(i.N, i.H, i.W, i.C)

    def run():
        dx = d.skip.clone() if accumulate else torch.full(shape, NAN, device=dev)
        part = torch.full((R, 2 * i.C), NAN, device=dev)
        L.call("pmu_maxpool2_bwd_bnr", d.dpool.data_ptr(), d.z.data_ptr(), d.coef.data_ptr(), d.mean.data_ptr(),
               d.invstd.data_ptr(), i.N, i.H, i.W, i.C, dx.data_ptr(), accumulate, part.data_ptr(), L.stream())
        return dx, part
    _z_has_ties(i)
    dx, part = _twice(run)
    where = f"pmu_maxpool2_bwd_bnr {shape} accumulate={accumulate}"
    da = _check_part(part, "maxpool" if accumulate else "maxpool_noskip", i, R, where)
    assert_exact(dx, da, where + ": dx")
    if not accumulate:
        assert bool((dx[:, 2 * (i.H // 2):] == 0).all()) and bool((dx[:, :, 2 * (i.W // 2):] == 0).all())


@pytest.mark.parametrize("with_skip", [True, False])
@pytest.mark.parametrize("shape", SHAPES, ids=_ids(SHAPES))
def test_maxpool2_bwd_bnr_dxb(dev, shape, with_skip):
    from pmu_hip import _lib as L
    i = inputs(*shape)
    d = Dev(i, dev)
    R = L.lib().pmu_maxpool2_bwd_bnr_tiles(i.N, i.H, i.W, i.C)

    def run():
        dx = torch.full(shape, NAN, device=dev)
        part = torch.full((R, 2 * i.C), NAN, device=dev)
        L.call("pmu_maxpool2_bwd_bnr_dxb", d.dpool_b.data_ptr(), d.skip_b.data_ptr() if with_skip else None,
               d.z.data_ptr(), d.coef.data_ptr(), d.mean.data_ptr(), d.invstd.data_ptr(), i.N, i.H, i.W, i.C,
               dx.data_ptr(), part.data_ptr(), L.stream())
        return dx, part
    dx, part = _twice(run)
    where = f"pmu_maxpool2_bwd_bnr_dxb {shape} skip={with_skip}"
    da = _check_part(part, "maxpool" if with_skip else "maxpool_noskip", i, R, where)
    assert_exact(dx, da, where + ": dx")


@pytest.mark.parametrize("shape", SHAPES, ids=_ids(SHAPES))
def test_maxpool2_bwd_bnr_stats(dev, shape):
    from pmu_hip import _lib as L
    i = inputs(*shape)
    d = Dev(i, dev)
    R = L.lib().pmu_maxpool2_bwd_bnr_tiles(i.N, i.H, i.W, i.C)

    def run():
        part = torch.full((R, 2 * i.C), NAN, device=dev)
        L.call("pmu_maxpool2_bwd_bnr_stats", d.dpool.data_ptr(), d.skip.data_ptr(), d.z.data_ptr(), d.coef.data_ptr(),
               d.mean.data_ptr(), d.invstd.data_ptr(), i.N, i.H, i.W, i.C, part.data_ptr(), L.stream())
        return (part,)
    _check_part(_twice(run)[0], "maxpool", i, R, f"pmu_maxpool2_bwd_bnr_stats {shape}")


@pytest.mark.parametrize("shape", SHAPES, ids=_ids(SHAPES))
def test_maxpool2_bwd_bnr_stats_dxb(dev, shape):
    from pmu_hip import _lib as L
    i = inputs(*shape)
    d = Dev(i, dev)
    R = L.lib().pmu_maxpool2_bwd_bnr_tiles(i.N, i.H, i.W, i.C)

    def run():
        part = torch.full((R, 2 * i.C), NAN, device=dev)
        L.call("pmu_maxpool2_bwd_bnr_stats_dxb", d.dpool_b.data_ptr(), d.skip_b.data_ptr(), d.z.data_ptr(),
               d.coef.data_ptr(), d.mean.data_ptr(), d.invstd.data_ptr(), i.N, i.H, i.W, i.C, part.data_ptr(),
               L.stream())
        return (part,)
    _check_part(_twice(run)[0], "maxpool", i, R, f"pmu_maxpool2_bwd_bnr_stats_dxb {shape}")


def _dz_reference(i, where, bf):
    da, _, absp, ug, ugx = ref_sums("maxpool", i)
    exact_headroom(absp[:, 0], ug, where + ": sum g")
    exact_headroom(absp[:, 1], ugx, where + ": sum g * xhat")
    dz = ref_dz(i, da)
    assert torch.equal(dz.float().double(), dz), where
    if bf and dz.numel() >= 2000:
        assert_rne_exercised(dz, where)
    return dz


@pytest.mark.parametrize("shape", BNBWD_SHAPES, ids=_ids(BNBWD_SHAPES))
def test_maxpool2_bwd_bnbwd(dev, shape):
    """fp32 dpool / skip, fp32 dz (ldo == C)."""
    from pmu_hip import _lib as L
    i = inputs(*shape)
    d = Dev(i, dev)

    def run():
        dz = torch.full(shape, NAN, device=dev)
        L.call("pmu_maxpool2_bwd_bnbwd", d.dpool.data_ptr(), d.skip.data_ptr(), d.z.data_ptr(), d.coef.data_ptr(),
               d.bcoef.data_ptr(), i.N, i.H, i.W, i.C, i.C, dz.data_ptr(), L.stream())
        return (dz,)
    where = f"pmu_maxpool2_bwd_bnbwd {shape}"
    assert_exact(_twice(run)[0], _dz_reference(i, where, False), where + ": dz")


@pytest.mark.parametrize("shape", BNBWD_SHAPES, ids=_ids(BNBWD_SHAPES))
def test_maxpool2_bwd_bnbwd_dxb(dev, shape):
    """bf16 dpool / skip, bf16 dz: the reference's round-to-nearest-even bits."""
    from pmu_hip import _lib as L
    i = inputs(*shape)
    d = Dev(i, dev)

    def run():
        dz = torch.full(shape, -7, dtype=torch.int16, device=dev)
        L.call("pmu_maxpool2_bwd_bnbwd_dxb", d.dpool_b.data_ptr(), d.skip_b.data_ptr(), d.z.data_ptr(),
               d.coef.data_ptr(), d.bcoef.data_ptr(), i.N, i.H, i.W, i.C, i.C, dz.data_ptr(), L.stream())
        return (dz,)
    where = f"pmu_maxpool2_bwd_bnbwd_dxb {shape}"
    ref = _dz_reference(i, where, True)
    got = _twice(run)[0].cpu()
    want = bf16_bits(ref)
    if not torch.equal(got, want):
        assert_exact(got.view(torch.bfloat16).float(), want.view(torch.bfloat16).double(), where + ": dz (bf16, RNE)")
        raise AssertionError(f"{where}: bf16 bits differ from the reference's only in the sign of a zero")


def test_maxpool2_bwd_bnbwd_refuses_96_channels(dev):
    """C / 4 = 24 neither divides 256 nor is a multiple of it: PMU_ERR_ARG from both forms, before any launch."""
    from pmu_hip import _lib as L
    i = inputs(1, 7, 9, 96)
    d = Dev(i, dev)
    dz = torch.full((1, 7, 9, 96), NAN, device=dev)
    dzb = torch.full((1, 7, 9, 96), -7, dtype=torch.int16, device=dev)
    assert L.lib().pmu_maxpool2_bwd_bnbwd(d.dpool.data_ptr(), d.skip.data_ptr(), d.z.data_ptr(), d.coef.data_ptr(),
                                          d.bcoef.data_ptr(), 1, 7, 9, 96, 96, dz.data_ptr(), L.stream()) == L.PMU_ERR_ARG
    assert L.lib().pmu_maxpool2_bwd_bnbwd_dxb(d.dpool_b.data_ptr(), d.skip_b.data_ptr(), d.z.data_ptr(),
                                              d.coef.data_ptr(), d.bcoef.data_ptr(), 1, 7, 9, 96, 96, dzb.data_ptr(),
                                              L.stream()) == L.PMU_ERR_ARG
    torch.cuda.synchronize()
    assert bool(torch.isnan(dz).all()) and bool((dzb == -7).all())


# ------------------------------------------------------------------------------------------ encoder forms
@pytest.mark.parametrize("shape", SHAPES, ids=_ids(SHAPES))
def test_avgpool2_bwd_bnr(dev, shape):
    """Odd maps: the windows of 4, 2 and 1 elements all divide exactly."""
    from pmu_hip import _lib as L
    i = inputs(*shape)
    d = Dev(i, dev)
    R = L.lib().pmu_bn_bwd_tiles(i.N * i.H * i.W, i.C)

    def run():
        da = torch.full(shape, NAN, device=dev)
        part = torch.full((R, 2 * i.C), NAN, device=dev)
        L.call("pmu_avgpool2_bwd_bnr", d.dpool_avg.data_ptr(), d.z.data_ptr(), d.coef.data_ptr(), d.mean.data_ptr(),
               d.invstd.data_ptr(), i.N, i.H, i.W, i.C, da.data_ptr(), part.data_ptr(), L.stream())
        return da, part
    da, part = _twice(run)
    where = f"pmu_avgpool2_bwd_bnr {shape}"
    assert_exact(da, _check_part(part, "avgpool", i, R, where), where + ": da")


@pytest.mark.parametrize("shape", MEAN_SHAPES, ids=_ids(MEAN_SHAPES))
def test_spatial_mean_bwd_bnr(dev, shape):
    """H * W a power of two, and 63 with dmean on multiples of 63 * 2^-4 (the division returns the exact quotient)."""
    from pmu_hip import _lib as L
    i = inputs(*shape)
    d = Dev(i, dev)
    R = L.lib().pmu_bn_bwd_tiles(i.N * i.H * i.W, i.C)

    def run():
        da = torch.full(shape, NAN, device=dev)
        part = torch.full((R, 2 * i.C), NAN, device=dev)
        L.call("pmu_spatial_mean_bwd_bnr", d.dmean.data_ptr(), d.z.data_ptr(), d.coef.data_ptr(), d.mean.data_ptr(),
               d.invstd.data_ptr(), i.N, i.H, i.W, i.C, da.data_ptr(), part.data_ptr(), L.stream())
        return da, part
    da, part = _twice(run)
    where = f"pmu_spatial_mean_bwd_bnr {shape}"
    assert_exact(da, _check_part(part, "mean", i, R, where), where + ": da")
