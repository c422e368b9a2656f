"""The bounds of tests/test_loss_kernels_gpu.py and tests/test_sgd_kernel_gpu.py are attainable (no GPU).

Those modules hold the HIP loss and SGD kernels to float64 references within derived bounds (tests/
tail_refs.py).  Here a float32 torch restatement of each kernel's formula, on the same generated inputs,
is held to the same references at the same hard ceilings (16 units for the forward losses and the BCE
backward, 4 for the CE backward, the SGD bounds as stated): so a GPU failure at those bounds is the
kernel's, not fp32 arithmetic's.  The exact SGD case's float64 reference is checked to be representable in
float32 at every step, which is what makes the GPU comparison bit for bit.

Measured here (worst error / unit over every case): BCE forward 2.80, BCE backward 2.81, CE forward 0.73,
CE backward 0.43, SGD buf 0.62 and p 0.49 of their bounds."""
import itertools

import pytest
import torch

import tail_refs as R


@pytest.mark.parametrize("n", R.BCE_SIZES)
def test_bce_fp32_restatement_within_ceiling(n):
    y, t, g = R.bce_inputs(n)
    ref, unit = R.bce_fwd_ref(y, t)
    got = R.bce_fwd_f32(y, t).double()
    assert torch.isfinite(ref).all() and torch.isfinite(got).all()
    wf = R.worst_ratio(got, ref, unit)
    # the denormal 1e-40: its true log (-92.1) is above the -100 clamp
    i = 6 if n > 6 else None
    if i is not None:
        assert float(y[i]) == R.f32(1e-40) and abs(float(ref[i]) - 92.1 * float(t[i])) < 0.01 * max(1.0, float(t[i]))
    rb, ub, ab = R.bce_bwd_ref(y, t, g)
    gb = R.bce_bwd_f32(y, t, g).double()
    assert torch.isfinite(gb).all()
    wb = R.worst_ratio(gb, rb, ub, ab)
    print(f"bce n={n}: fwd {wf:.3f} B, bwd {wb:.3f} u|ref|")
    assert wf <= R.CEIL_FWD and wb <= R.CEIL_BCE_BWD


@pytest.mark.parametrize("ignore", R.CE_IGNORES)
@pytest.mark.parametrize("N,K,HW", R.CE_CASES)
def test_ce_fp32_restatement_within_ceiling(N, K, HW, ignore):
    x, tgt, g, bad = R.ce_inputs(N, K, HW, ignore)
    for i, v in zip(bad, R.CE_BAD_TARGETS):
        tgt.view(-1)[i] = v
    loss, ul, dx, ud, valid, nan = R.ce_ref(x, tgt, g, ignore)
    assert int(nan.sum()) == len(bad)
    if N >= 2:
        assert not valid[0].any() and valid[1].all()
    wf = R.worst_ratio(R.ce_fwd_f32(x, tgt, ignore).double(), loss, ul)
    wb = R.worst_ratio(R.ce_bwd_f32(x, tgt, g, ignore).double(), dx, ud)
    print(f"ce {(N, K, HW)} ignore={ignore}: fwd {wf:.3f}, bwd {wb:.3f} of the unit")
    assert wf <= R.CEIL_FWD and wb <= R.CEIL_CE_BWD


@pytest.mark.parametrize("n", [1, 5, 4094, 16384, 40000])
def test_sgd_exact_reference_is_representable(n):
    """Multiples of 2^-8 in [-4, 4], lr 2^-4, momenta with two fraction bits, power-of-two gscale and clip: after
    two steps buf is a multiple of 2^-12 below 16 and p a multiple of 2^-16 below 8 — under 24 bits, so every
    intermediate (and the fused multiply-add's unrounded product) is a float32 value."""
    p0, b0, g1, g2 = R.sgd_exact_inputs(n)
    for m, gs, clip in itertools.product(R.SGD_EXACT_MOMENTA, R.SGD_EXACT_GSCALES, R.SGD_EXACT_CLIPS):
        p, b = p0, b0
        for g in (g1, g2):
            pn, bn, _, _ = R.sgd_ref(p, g, b, gs, R.SGD_EXACT_LR, m, clip)
            for name, v in (("p", pn), ("buf", bn), ("m*buf", m * b.double()), ("lr*buf", R.SGD_EXACT_LR * bn)):
                assert torch.equal(v.float().double(), v), (name, m, gs, clip)
            pf, bf = R.sgd_f32(p, g, b, gs, R.SGD_EXACT_LR, m, clip)
            assert torch.equal(pf.double(), pn) and torch.equal(bf.double(), bn), (m, gs, clip)
            p, b = pn.float(), bn.float()


@pytest.mark.parametrize("clip", [R.SGD_CLIP, 0.0])
@pytest.mark.parametrize("n", [1, 5, 4094, 16384, 40000])
def test_sgd_fp32_restatement_within_bound(n, clip):
    p, g, b = R.sgd_bounded_inputs(n)
    pn, bn, bb, bp = R.sgd_ref(p, g, b, R.SGD_GSCALE, R.SGD_LR, R.SGD_MOMENTUM, clip)
    pf, bf = R.sgd_f32(p, g, b, R.SGD_GSCALE, R.SGD_LR, R.SGD_MOMENTUM, clip)
    assert bool(R.within(bf.double(), bn, bb).all()) and bool(R.within(pf.double(), pn, bp).all())
    print(f"sgd n={n} clip={clip}: buf {R.worst_ratio(bf.double(), bn, bb):.3f}, "
          f"p {R.worst_ratio(pf.double(), pn, bp):.3f} of the bound")
    if n >= 8:
        c = clip if clip > 0 else float("inf")
        idx = torch.tensor([1, 2, n // 2])
        sign = torch.tensor([1.0, -1.0, 1.0], dtype=torch.float64)
        assert torch.equal(bn[idx], R.SGD_MOMENTUM * b.double()[idx] + sign * c)
        assert torch.isnan(bn[n - 1]) and torch.isnan(pn[n - 1]) and torch.isnan(bf[n - 1]) and torch.isnan(pf[n - 1])
