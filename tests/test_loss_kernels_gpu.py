"""pmu_bce_fwd / _bwd and pmu_ce_fwd / _bwd (csrc/loss.hip) by direct calls, against float64 restatements of
the formulas in include/pmunet_hip.h built from the fp32 inputs (tests/tail_refs.py).  tests/test_loss_gpu.py
keeps the wrapper-level parity with torch's criteria; this module holds every element to a bound derived
from fp32 rounding, at the launch geometries the wrappers' tests never reach.

Element level (reduction 0), u = 2^-24:

  BCE forward   l = -(t max(log y, -100) + (1 - t) max(log(1 - y), -100)).  Each log is good to a few u of
                its value, the two products and the sum round once each: the unit is
                B = u (|t ly| + |(1 - t) l1y|) + u (1 - t); the last term is the rounding of 1 - y for
                small y (log(1 - y) ~ -y moves by up to u when 1 - y rounds).
  BCE backward  dy = g (y - t) / max(y (1 - y), float32(1e-12)): five roundings, each relative, so the
                unit is u |ref|, plus 2^-149 / 1e-12 max(1, |g|) absolute for a numerator that underflows
                gradually before the division by the floor.  No element is masked; y in {0, 1} with
                t != y (both sides divide by the floor, |dy| ~ 1e12 |g|) is also checked for finiteness and
                sign.
  CE forward    l = (M + log sum exp(x - M)) - x_t: unit u (2 |M| + 2 log sum + |x_t| + K + 4) (the
                subtractions x - M, K exps and K - 1 adds, the log, and the two outer roundings).
  CE backward   dx = g (softmax - onehot): unit u |g| (K + 6), absolute (softmax <= 1: K adds, exp,
                reciprocal, product, subtraction, product).

The admitted multiple of each unit is twice the worst err / unit measured on an MI355X, rounded up, and
never above the ceilings of tests/tail_refs.py (16 forward and BCE backward, 4 CE backward); the fp32
torch restatements on the CPU reach 2.8, 2.8, 0.73 and 0.43 (tests/test_tail_bounds_cpu.py).  Measured on
the GPU (worst over every case below):

  BCE forward   3.650 B        (n = 2,101,249)           -> multiple 8
  BCE backward  2.807 u |ref|  (n = 2,101,249)           -> multiple 6
  CE forward    0.730 unit     (4, 3, 524289)            -> multiple 2
  CE backward   0.429 unit     (2, 8, 300001)            -> multiple 1

and per case, forward / backward: BCE n = 1: 0.000 / 0.304; 255: 2.322 / 1.740; 256: 2.299 / 1.801; 257: 2.299 /
1.912; 2049: 2.980 / 2.167; 600,001: 3.484 / 2.705; 2,101,249: 3.650 / 2.807.  CE (worst over the three
ignore_index values) (1,1,1): 0 / 0; (65,3,1): 0.330 / 0.263; (3,2,357): 0.531 / 0.225; (2,8,300001): 0.669 /
0.429; (1,33,2049): 0.295 / 0.171; (4,3,524289): 0.730 / 0.353.  Every reduced loss was 0 ulp32 from
float32(sum64(each) [/ denominator]) and every mode 1 / 2 backward bit-equal to the reduction-0 kernel.  The
denormal y = 1e-40 is not flushed (loss 92.1 t).

Reduction level (modes 1 and 2): the kernel sums, in float64, the same l it would store, so with `each`
the stored reduction-0 losses, loss == float32(sum64(each) [/ denominator]) within 1 ulp32 (the float64
partial sums differ from the reference's order by ~1e-16 relative: they can only move the final rounding
across a tie) — a dropped element, a lost partial block or a wrong denominator is far outside that.
count_out is the exact number of non-ignored pixels (n for BCE).  The backward of modes 1 and 2 is the
reduction-0 backward with g = gout (sum) or float32(gout / denominator) (mean) on every element: within
2 ulp32 per element of that kernel's own output.  pmu_ce_bwd forms gout / count in one fp32 division, so
any gout gives exactly that g; pmu_bce_bwd multiplies gout by float32(1 / n), which is that g exactly for
a power-of-two gout — the mean case uses gout = -0.5 (training passes 1.0), the sum case 0.7.  The BCE mean with
gout = 0.7 is held to float64 directly, at two more units (the scale's two roundings): measured 3.868 u |ref| at worst (n = 600,001).

Sizes.  BCE n: 1; 255, 256, 257 (one block, around the thread count); 2049 (first two-block launch);
600,001 (G = 293 partials: a ragged second pass of loss_final_kernel's 256 threads); 2,097,152 + 4097 (the
cap of 1024 blocks binds, every thread strides twice).  CE (N, K, HW): see tail_refs.CE_CASES; ignore_index
-100, 255 and 0 (a valid class ignored, as torch does); image 0 wholly ignored and image 1 not at all when
N >= 2; targets 2^32 + 1 (which a 32-bit cast would turn into class 1) and -1 give NaN for that pixel's
loss and K gradients and for the reduced loss, every other pixel unchanged."""
import numpy as np
import pytest
import torch

import tail_refs as R
from helpers import ulp32

pytestmark = pytest.mark.gpu

NAN = float("nan")
BCE_FWD_MULT, BCE_BWD_MULT, CE_FWD_MULT, CE_BWD_MULT = 8, 6, 2, 1
assert BCE_FWD_MULT <= R.CEIL_FWD and CE_FWD_MULT <= R.CEIL_FWD
assert BCE_BWD_MULT <= R.CEIL_BCE_BWD and CE_BWD_MULT <= R.CEIL_CE_BWD


def _L():
    from pmu_hip import _lib as L
    return L


def _ws(L, n, dev):
    return torch.full((L.lib().pmu_loss_ws(n) // 8,), NAN, dtype=torch.float64, device=dev)


def _reduced_ok(got, each64, denom, mean):
    """got (fp32 scalar tensor) == float32(sum64(each) [/ denom]) within 1 ulp32; NaN for an empty mean."""
    s = float(each64.sum())
    if mean and denom == 0:
        return bool(torch.isnan(got).all()), NAN
    want = np.float64(np.float32(s / denom if mean else s))
    d = abs(float(got.double()) - float(want)) / float(ulp32(torch.tensor(float(want), dtype=torch.float64)))
    return d <= 1.0, d


def _ulps(a, b):
    """max |a - b| in ulp32 of b (fp32 device tensors)."""
    a6, b6 = a.double().cpu(), b.double().cpu()
    return float(((a6 - b6).abs() / ulp32(b6)).max())


# ------------------------------------------------------------------------------------------- BCE
def _bce_fwd(L, yd, td, n, red, dev):
    out = torch.full((n if red == 0 else 1,), NAN, device=dev)
    ws = _ws(L, n, dev) if red else None
    cnt = torch.full((1,), NAN, device=dev) if red else None
    L.call("pmu_bce_fwd", yd.data_ptr(), td.data_ptr(), n, red, out.data_ptr(), L.ptr(ws), L.ptr(cnt), L.stream())
    return out, cnt


def _bce_bwd(L, yd, td, n, red, gd, dev):
    dy = torch.full((n,), NAN, device=dev)
    L.call("pmu_bce_bwd", yd.data_ptr(), td.data_ptr(), n, red, gd.data_ptr(), dy.data_ptr(), L.stream())
    return dy


@pytest.mark.parametrize("n", R.BCE_SIZES)
def test_bce_kernels_vs_float64(dev, n):
    L = _L()
    y, t, g = R.bce_inputs(n)
    yd, td, gd = y.to(dev), t.to(dev), g.to(dev)
    each, _ = _bce_fwd(L, yd, td, n, 0, dev)
    mean, cnt1 = _bce_fwd(L, yd, td, n, 1, dev)
    total, cnt2 = _bce_fwd(L, yd, td, n, 2, dev)
    dy0 = _bce_bwd(L, yd, td, n, 0, gd, dev)
    torch.cuda.synchronize()

    ref, unit = R.bce_fwd_ref(y, t)
    e6 = each.double().cpu()
    assert torch.isfinite(e6).all()
    wf = R.worst_ratio(e6, ref, unit)
    if n > 6:   # y = 1e-40, t = 1: -log y = 92.1; 100 means the denormal was flushed to zero before the log
        assert float(y[6]) == R.f32(1e-40) and float(t[6]) == 1.0
        assert abs(float(e6[6]) - 92.1) < 0.01, f"loss at the denormal y = 1e-40: {float(e6[6])} (100 = flushed)"
    rb, ub, ab = R.bce_bwd_ref(y, t, g)
    d6 = dy0.double().cpu()
    assert torch.isfinite(d6).all()
    wb = R.worst_ratio(d6, rb, ub, ab)
    floor = ((y == 0) | (y == 1)) & (t != y)
    if floor.any():
        assert bool((torch.sign(d6[floor]) == torch.sign(rb[floor])).all())
        assert R.worst_ratio(d6[floor], rb[floor], ub[floor], ab[floor]) <= BCE_BWD_MULT
    print(f"bce n={n}: fwd worst {wf:.3f} B, bwd worst {wb:.3f} u|ref|")
    assert wf <= BCE_FWD_MULT, wf
    assert wb <= BCE_BWD_MULT, wb

    ok1, d1 = _reduced_ok(mean, e6, n, True)
    ok2, d2 = _reduced_ok(total, e6, n, False)
    print(f"bce n={n}: mean off by {d1:.2f} ulp32, sum off by {d2:.2f} ulp32")
    assert ok1 and ok2, (d1, d2)
    assert float(cnt1) == float(n) and float(cnt2) == float(n)

    # modes 1 and 2 backward == the reduction-0 kernel with the scalar upstream gradient on every element
    for red, gout in ((1, -0.5), (2, 0.7)):
        gs = np.float32(gout / n) if red == 1 else np.float32(gout)
        got = _bce_bwd(L, yd, td, n, red, torch.tensor([gout], device=dev), dev)
        want = _bce_bwd(L, yd, td, n, 0, torch.full((n,), float(gs), device=dev), dev)
        torch.cuda.synchronize()
        assert torch.isfinite(got).all()
        d = _ulps(got, want)
        print(f"bce n={n}: reduction {red} backward within {d:.2f} ulp32 of the reduction-0 kernel")
        assert d <= 2.0, (red, d)
    # the mean with a gout that is no power of two, against float64 with g = gout / n: the scale
    # gout * float32(1 / n) adds two roundings to the element's five, so two more units are admitted
    gout = np.float32(0.7)
    got = _bce_bwd(L, yd, td, n, 1, torch.tensor([float(gout)], device=dev), dev)
    torch.cuda.synchronize()
    rm, um, am = R.bce_bwd_ref(y, t, torch.full((n,), 1.0).double() * (float(gout) / n))
    wm = R.worst_ratio(got.double().cpu(), rm, um, am)
    print(f"bce n={n}: mean backward, gout 0.7: worst {wm:.3f} u|ref|")
    assert wm <= BCE_BWD_MULT + 2, wm


# -------------------------------------------------------------------------------------------- CE
def _ce_fwd(L, xd, td, N, K, HW, red, ignore, dev):
    out = torch.full((N * HW if red == 0 else 1,), NAN, device=dev)
    ws = _ws(L, N * HW, dev) if red else None
    cnt = torch.full((1,), NAN, device=dev) if red else None
    L.call("pmu_ce_fwd", xd.data_ptr(), td.data_ptr(), N, K, HW, red, ignore, out.data_ptr(), L.ptr(ws), L.ptr(cnt),
           L.stream())
    return out, cnt


def _ce_bwd(L, xd, td, N, K, HW, red, ignore, gd, cnt, dev):
    dx = torch.full((N, K, HW), NAN, device=dev)
    L.call("pmu_ce_bwd", xd.data_ptr(), td.data_ptr(), N, K, HW, red, ignore, gd.data_ptr(), L.ptr(cnt), dx.data_ptr(),
           L.stream())
    return dx


@pytest.mark.parametrize("ignore", R.CE_IGNORES)
@pytest.mark.parametrize("N,K,HW", R.CE_CASES)
def test_ce_kernels_vs_float64(dev, N, K, HW, ignore):
    L = _L()
    x, tgt, g, bad = R.ce_inputs(N, K, HW, ignore)
    P = N * HW
    xd, td, gd = x.to(dev), tgt.to(dev), g.to(dev)
    each, _ = _ce_fwd(L, xd, td, N, K, HW, 0, ignore, dev)
    mean, cnt1 = _ce_fwd(L, xd, td, N, K, HW, 1, ignore, dev)
    total, cnt2 = _ce_fwd(L, xd, td, N, K, HW, 2, ignore, dev)
    dx0 = _ce_bwd(L, xd, td, N, K, HW, 0, ignore, gd, None, dev)
    torch.cuda.synchronize()

    loss, ul, dx, ud, valid, nan = R.ce_ref(x, tgt, g, ignore)
    assert not nan.any()
    count = int(valid.sum())
    if N >= 2:
        assert not valid[0].any() and valid[1].all()
    e6 = each.double().cpu().view(N, HW)
    d6 = dx0.double().cpu()
    assert torch.isfinite(e6).all() and torch.isfinite(d6).all()
    assert not e6[~valid].any() and not d6.permute(0, 2, 1)[~valid].any()    # ignored pixels: exactly 0
    wf, wb = R.worst_ratio(e6, loss, ul), R.worst_ratio(d6, dx, ud)
    print(f"ce {(N, K, HW)} ignore={ignore}: fwd worst {wf:.3f}, bwd worst {wb:.3f} of the unit")
    assert wf <= CE_FWD_MULT, wf
    assert wb <= CE_BWD_MULT, wb

    ok1, d1 = _reduced_ok(mean, e6, count, True)
    ok2, d2 = _reduced_ok(total, e6, count, False)
    print(f"ce {(N, K, HW)} ignore={ignore}: count {count} of {P}, mean off by {d1:.2f} ulp32, sum by {d2:.2f}")
    assert ok1 and ok2, (d1, d2)
    assert float(cnt1) == float(count) and float(cnt2) == float(count)

    for red, gout in ((1, 0.7), (2, 0.7)):
        got = _ce_bwd(L, xd, td, N, K, HW, red, ignore, torch.tensor([gout], device=dev), cnt1, dev)
        torch.cuda.synchronize()
        if red == 1 and count == 0:
            assert not got.any()        # nothing but ignored pixels: all zeros, as torch
            continue
        gs = np.float32(np.float32(gout) / np.float32(count)) if red == 1 else np.float32(gout)
        want = _ce_bwd(L, xd, td, N, K, HW, 0, ignore, torch.full((P,), float(gs), device=dev), None, dev)
        torch.cuda.synchronize()
        assert torch.isfinite(got).all()
        d = _ulps(got, want)
        print(f"ce {(N, K, HW)} ignore={ignore}: reduction {red} backward within {d:.2f} ulp32 of reduction 0")
        assert d <= 2.0, (red, d)

    if not bad:
        return
    # targets that only fit in 64 bits / negative, neither being ignore_index: NaN there, nothing else moves
    tb = tgt.clone()
    for i, v in zip(bad, R.CE_BAD_TARGETS):
        tb.view(-1)[i] = v
    tbd = tb.to(dev)
    eachb, _ = _ce_fwd(L, xd, tbd, N, K, HW, 0, ignore, dev)
    totalb, _ = _ce_fwd(L, xd, tbd, N, K, HW, 2, ignore, dev)
    dxb = _ce_bwd(L, xd, tbd, N, K, HW, 0, ignore, gd, None, dev)
    torch.cuda.synchronize()
    lossb, ulb, dxr, udb, validb, nanb = R.ce_ref(x, tb, g, ignore)
    assert int(nanb.sum()) == len(bad)
    eb, db = eachb.double().cpu().view(N, HW), dxb.double().cpu().permute(0, 2, 1)    # db [N][HW][K]
    assert torch.isnan(eb[nanb]).all() and torch.isnan(db[nanb]).all()
    assert torch.isnan(totalb).all()
    assert torch.isfinite(eb[~nanb]).all() and torch.isfinite(db[~nanb]).all()
    keep = ~nanb
    assert R.worst_ratio(eb[keep], lossb[keep], ulb[keep]) <= CE_FWD_MULT
    assert R.worst_ratio(db[keep], dxr.permute(0, 2, 1)[keep], udb.permute(0, 2, 1)[keep]) <= CE_BWD_MULT
    if L.debug_build():     # the bounds-checked build recorded the bad targets: take the record, as test_loss_gpu does
        with pytest.raises(RuntimeError, match="index out of range"):
            L.debug_check()


@pytest.mark.parametrize("ignore", R.CE_IGNORES)
def test_ce_wholly_ignored_and_wholly_valid_images(dev, ignore):
    """One image with every pixel ignored: sum 0, count 0, mean NaN (0 / 0, as torch), dx all zeros in every
    mode.  One image with no pixel ignored: the count is exactly the pixel count."""
    L = _L()
    K, HW = 3, 2500
    gen = torch.Generator().manual_seed(11)
    x = (torch.randn(1, K, HW, generator=gen) * 3).to(dev)
    for all_ignored in (True, False):
        tgt = torch.full((1, HW), ignore) if all_ignored else torch.randint(1, K, (1, HW), generator=gen)
        td = tgt.to(dev)
        mean, cnt = _ce_fwd(L, x, td, 1, K, HW, 1, ignore, dev)
        total, _ = _ce_fwd(L, x, td, 1, K, HW, 2, ignore, dev)
        torch.cuda.synchronize()
        assert float(cnt) == (0.0 if all_ignored else float(HW))
        if not all_ignored:
            assert torch.isfinite(mean).all() and torch.isfinite(total).all()
            continue
        assert torch.isnan(mean).all() and float(total) == 0.0
        for red in (0, 1, 2):
            gd = torch.ones(HW if red == 0 else 1, device=dev)
            dx = _ce_bwd(L, x, td, 1, K, HW, red, ignore, gd, cnt, dev)
            torch.cuda.synchronize()
            assert not torch.isnan(dx).any() and not dx.any(), red


def test_loss_entries_refuse_bad_arguments(dev):
    L = _L()
    lib, s, bad = L.lib(), L.stream(), L.PMU_ERR_ARG
    a = torch.full((64,), 0.5, device=dev)
    t = torch.zeros(8, dtype=torch.int64, device=dev)
    out = torch.full((64,), NAN, device=dev)
    ws = _ws(L, 64, dev)
    p = lambda v: v.data_ptr()
    assert lib.pmu_bce_fwd(p(a), p(a), 0, 0, p(out), None, None, s) == bad              # n = 0
    assert lib.pmu_bce_fwd(p(a), p(a), 64, 3, p(out), p(ws), None, s) == bad            # reduction 3
    assert lib.pmu_bce_fwd(p(a), p(a), 64, 1, p(out), None, None, s) == bad             # mean without ws
    assert lib.pmu_bce_fwd(p(a), p(a), 64, 2, p(out), None, None, s) == bad             # sum without ws
    assert lib.pmu_bce_bwd(p(a), p(a), 0, 0, p(a), p(out), s) == bad
    assert lib.pmu_bce_bwd(p(a), p(a), 64, 3, p(a), p(out), s) == bad
    assert lib.pmu_ce_fwd(p(a), p(t), 1, 8, 0, 0, -100, p(out), None, None, s) == bad   # no pixels
    assert lib.pmu_ce_fwd(p(a), p(t), 1, 8, 8, 3, -100, p(out), p(ws), None, s) == bad
    assert lib.pmu_ce_fwd(p(a), p(t), 1, 8, 8, 1, -100, p(out), None, None, s) == bad
    assert lib.pmu_ce_bwd(p(a), p(t), 1, 8, 8, 3, -100, p(a), p(a), p(out), s) == bad
    assert lib.pmu_ce_bwd(p(a), p(t), 1, 8, 8, 1, -100, p(a), None, p(out), s) == bad   # mean without count
    torch.cuda.synchronize()
    assert torch.isnan(out).all()       # nothing was launched
