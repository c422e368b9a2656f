"""CPU checks of the exact-comparison helpers (tests/helpers.py: grid_data / grid_stats / grid_f4,
exact_headroom, wino_conv / wino_wgrad, assert_exact) and of every case of tests/test_exact_gpu.py: a case
whose sums could leave fp32's 24 bits would make an exact comparison on the GPU meaningless, so each one's
condition is asserted here from the float64 reference alone, without a GPU."""
import pytest
import torch
import torch.nn.functional as TF

import test_exact_gpu as E
from helpers import (EXACT_LIMIT, F4_UW, WINO, assert_exact, bf16_exact, exact_headroom, grid_data, grid_f4, grid_stats,
                     wino_conv, wino_wgrad)


def _multiples(t, unit):
    return bool(((t.double() / unit).round() * unit == t.double()).all())


@pytest.mark.parametrize("make,ux,xmax,xnz,uw,wmax,wnz,ub", [(grid_data, 0.25, 2.0, 0.5, 0.125, 1.0, 1.0, 0.25),
                                                           (grid_stats, 0.5, 1.0, 0.4, 0.5, 1.0, 0.6, 0.5),
                                                           (grid_f4, 1.0, 1.0, 0.4, F4_UW, F4_UW, 0.6, F4_UW)])
def test_grids_are_bf16_exact_and_on_their_grid(make, ux, xmax, xnz, uw, wmax, wnz, ub):
    g = make(5)
    x, w, b = g.operand(3, 17, 19, 24), g.weight(40, 24, 3, 3), g.bias(40)
    for t in (x, w, b):
        assert t.dtype == torch.float32 and t.device.type == "cpu"
        assert torch.equal(t.to(torch.bfloat16).float(), t) and bf16_exact(t)
    assert _multiples(x, ux) and float(x.abs().max()) == xmax
    assert _multiples(w, uw) and float(w.abs().max()) == wmax
    assert _multiples(b, ub)
    assert abs(float((x != 0).float().mean()) - xnz) < 0.03
    assert abs(float((w != 0).float().mean()) - wnz) < 0.03
    # every product is a multiple of the result grid, a power of two
    assert _multiples(x.flatten()[:500, None] * w.flatten()[None, :500], g.unit)
    assert _multiples(b, g.unit) and float(torch.tensor(g.unit).log2()) % 1 == 0
    # seeded: the same seed draws the same tensors, another seed different ones
    assert torch.equal(make(5).operand(3, 17, 19, 24), x) and not torch.equal(make(6).operand(3, 17, 19, 24), x)


def test_f4_weights_transform_to_integers():
    """G g G^T of grid_f4 weights is an integer of 2^-10 (the reason for the factor 576)."""
    w = grid_f4(3).weight(8, 8, 3, 3).double()
    G = torch.tensor(WINO[4][1], dtype=torch.float64)
    U = torch.einsum("ia,ocab,jb->ocij", G, w, G) * 2.0 ** 10
    assert float((U - U.round()).abs().max()) < 1e-9 and float(U.abs().max()) > 0


_CONDITIONS = E.all_conditions()


@pytest.mark.parametrize("label", [c[0] for c in _CONDITIONS])
def test_case_meets_its_condition(label):
    """Building the case asserts every condition (helpers.exact_headroom); what it returns is the headroom."""
    cond = dict(_CONDITIONS)[label]()
    assert cond and all(0 < v < EXACT_LIMIT for v in cond.values()), cond


def test_every_listed_shape_has_a_condition():
    labels = " ".join(c[0] for c in _CONDITIONS)
    for shapes in (E.DMA_FWD, E.DMA_DGRAD, E.RAW, E.FUSED, E.WGRAD_BF16, E.CONVT_FWD, E.CONVT_DGRAD, E.CONVT_WGRAD, E.W2H,
                   E.WINO_FUSED, E.WGRAD_WINO, E.W4_DGRAD, E.FIRST):
        for s in shapes:
            assert str(tuple(s[:5]))[1:-1] in labels, s
    assert len(_CONDITIONS) == len(set(c[0] for c in _CONDITIONS))


def test_exact_headroom_refuses_a_case_past_24_bits():
    assert exact_headroom(torch.tensor([3.0, -5.0]), 0.25, "x") == 20.0
    with pytest.raises(AssertionError, match="limit"):
        exact_headroom(torch.tensor([2.0 ** 22]), 0.25, "x")
    # F(4x4) at 256 reduction channels of grid_f4's density does not fit (64 channels reach about 6e6 units of
    # 2^-10): such a case is refused, not compared loosely
    g = grid_f4(1)
    dz, w = g.operand(1, 256, 16, 16).double(), g.weight(256, 16, 3, 3).double()
    with pytest.raises(AssertionError, match="limit"):
        exact_headroom(wino_conv(4, dz, E._flip(w), absolute=True), 2.0 ** -10, "F(4x4), 256 channels")


@pytest.mark.parametrize("m", [2, 4])
def test_wino_restatement_is_the_convolution(m):
    g = (grid_data if m == 2 else grid_f4)(7)
    x, w = g.operand(2, 12, 11, 9).double(), g.weight(10, 12, 3, 3).double()   # NCHW; 11 x 9: ragged tiles
    ref = TF.conv2d(x, w, padding=1)
    y = wino_conv(m, x, w)
    if m == 2:
        assert torch.equal(y, ref)            # F(2x2)'s matrices are exact in binary
    else:
        assert float((y - ref).abs().max()) < 1e-9   # (sixths in G: float64 rounding only)
    bound = wino_conv(m, x, w, absolute=True)
    assert bool((bound >= ref.abs() - 1e-9).all())
    dz = g.operand(2, 10, 11, 9).double()
    if m == 2:
        dw = torch.nn.grad.conv2d_weight(x, (10, 12, 3, 3), dz, padding=1)
        assert torch.equal(wino_wgrad(x, dz), dw)
        assert bool((wino_wgrad(x, dz, absolute=True) >= dw.abs()).all())


def _message(got, ref, **kw):
    with pytest.raises(AssertionError) as e:
        assert_exact(got, ref, "case", **kw)
    return str(e.value)


def test_assert_exact_names_position_and_class():
    N, H, W, C = 2, 20, 37, 40
    got = grid_data(9).operand(N, H, W, C)
    unit = 2.0 ** -5
    assert_exact(got, got.double(), "same")
    # one grid unit at one interior element (off every 16 x 32 tile edge, first channel block)
    ref = got.double()
    ref[1, 5, 9, 3] += unit
    msg = _message(got, ref, tile=(16, 32), cblock=32)
    assert "1 of %d elements differ" % got.numel() in msg and "(1, 5, 9, 3)" in msg and "[interior]" in msg
    assert repr(float(got[1, 5, 9, 3])) in msg and repr(float(ref[1, 5, 9, 3])) in msg
    # a corner element: image border and tile edge
    ref = got.double()
    ref[0, H - 1, W - 1, 0] -= unit
    msg = _message(got, ref, tile=(16, 32), cblock=32)
    assert f"(0, {H - 1}, {W - 1}, 0)" in msg and "image border" in msg and "interior" not in msg
    assert f"tile edge (h % 16 = {(H - 1) % 16}, w % 32 = {(W - 1) % 32})" not in msg   # (19 % 16 = 3, 36 % 32 = 4: no tile edge)
    ref = got.double()
    ref[0, 0, 0, 0] -= unit
    msg = _message(got, ref, tile=(16, 32), cblock=32)
    assert "(0, 0, 0, 0)" in msg and "image border" in msg and "tile edge (h % 16 = 0, w % 32 = 0)" in msg
    # the last channel: in the ragged block (40 = 32 + 8)
    ref = got.double()
    ref[1, 7, 33, C - 1] += unit
    msg = _message(got, ref, tile=(16, 32), cblock=32)
    assert f"(1, 7, 33, {C - 1})" in msg and "last ragged channel block (8 of 32)" in msg and "image border" not in msg
    # a tile edge off the border, and no ragged block when C is a multiple of the block
    ref = got.double()
    ref[0, 15, 31, 1] += unit
    msg = _message(got, ref, tile=(16, 32), cblock=8)
    assert "tile edge (h % 16 = 15, w % 32 = 31)" in msg and "ragged" not in msg and "image border" not in msg
    # more than eight: all counted, eight listed; an unwritten (NaN) element differs
    ref = got.double() + unit
    msg = _message(got, ref)
    assert "%d of %d elements differ" % (got.numel(), got.numel()) in msg and msg.count("got ") == 8
    nan = got.clone()
    nan[0, 3, 3, 3] = float("nan")
    assert "(0, 3, 3, 3)" in _message(nan, got.double())
    # other ranks report the raw index
    assert "(2, 1)" in _message(torch.zeros(3, 2), torch.tensor([[0., 0.], [0., 0.], [0., 1.]], dtype=torch.float64))
