"""The conditions under which tests/test_frame_exact_gpu.py and tests/test_bnbwd_exact_gpu.py may demand equality
with float64, checked without a GPU: the grids are what their docstrings claim (bf16-exact where a tensor is
stored as bf16; ties, zeros and both rounding directions present); every stats case has headroom; fp32 torch
restatements of the BN-backward formula and of the partial sums, evaluated on the CPU on the same inputs, equal
the float64 references bit for bit (so the references, not only the kernels, satisfy the exactness claim); and
helpers.ref_maxpool_bwd is pinned to max_pool2d's autograd."""
import pytest
import torch
import torch.nn.functional as F

import bnbwd_cases as B
from helpers import (EXACT_LIMIT, assert_rne_exercised, bf16_bits, bf16_exact, exact_headroom, quant_bn, quant_grad,
                     quant_invstd, quant_z, ref_bn_bwd_sums, ref_frame, ref_maxpool_bwd, rne_census, rows_bn_bwd,
                     rows_maxpool_bwd)
from test_frame_exact_gpu import bnbwd


# ------------------------------------------------------------------------------------------ grids
def test_gradient_grids():
    g = torch.Generator().manual_seed(1)
    coarse, fine = quant_grad((4000,), g), quant_grad((4000,), g, fine=True)
    assert torch.equal(coarse * 16, (coarse * 16).round()) and float(coarse.abs().max()) == 2.0
    assert torch.equal(fine * 64, (fine * 64).round()) and float(fine.abs().max()) == 4.0
    assert bf16_exact(coarse) and bf16_exact(fine)
    assert int((coarse == 0).sum()) > 0 and int((fine == 0).sum()) > 0
    assert not bf16_exact(torch.tensor([1.0 + 2.0 ** -8]))
    assert bf16_exact(quant_z(2, 6, 10, 32, g))           # the bf16-stored z sources of the frame tests


def test_dyadic_bn_backward_block_and_invstd():
    g = torch.Generator().manual_seed(2)
    C = 512
    c = quant_bn(C, g, bwd=True, dyadic=True).view(5, C)
    assert set(c[0].tolist()) == {0.5, 1.0, 2.0}
    for row, lim in ((c[1], 0.5), (c[2], 0.5), (c[3], 1.0), (c[4], 1.0)):
        assert torch.equal(row * 16, (row * 16).round()) and float(row.abs().max()) == lim
    assert set(quant_invstd(C, g).tolist()) == {0.5, 1.0, 2.0}
    # the default block is unchanged: ordinary randn kx, kc
    d = quant_bn(C, torch.Generator().manual_seed(2), bwd=True).view(5, C)
    assert torch.equal(d[:3], c[:3]) and not torch.equal(d[3] * 16, (d[3] * 16).round())


def test_rne_census_by_hand():
    """bf16 keeps 8 significant bits: 1 + k * 2^-9 for k = 1 (down), 2 (tie, down to even), 3 (up), 6 (tie, up to
    even), and the same mirrored."""
    v = torch.tensor([1 + 2.0 ** -9, 1 + 2.0 ** -8, 1 + 3 * 2.0 ** -9, 1 + 6 * 2.0 ** -9, 1.5], dtype=torch.float64)
    assert rne_census(v) == {"tie_up": 1, "tie_down": 1, "up": 1, "down": 1, "exact": 1}
    assert rne_census(-v) == {"tie_up": 1, "tie_down": 1, "up": 1, "down": 1, "exact": 1}
    assert bf16_bits(v.float()).tolist() == [0x3f80, 0x3f80, 0x3f81, 0x3f82, 0x3fc0]
    with pytest.raises(AssertionError):
        assert_rne_exercised(v[:2], "ties down only")


@pytest.mark.parametrize("N,H,W,C", [(2, 13, 11, 64), (5, 3, 3, 16), (3, 17, 23, 128), (1, 8, 8, 1024), (2, 6, 10, 32)])
def test_bnbwd_frame_values_round_both_ways_and_restate_in_fp32(N, H, W, C):
    """The BN-backward frames of test_frame_exact_gpu.py: the float64 value is an fp32 number, the fp32
    restatement (one rounding per operation, as torch evaluates it; the kernels' fmaf rounds less often) equals
    it, and storing it as bf16 rounds ties in both directions and other values up and down."""
    g = torch.Generator().manual_seed(600 + C)
    s = bnbwd(g, N, H, W, C)
    assert bf16_exact(s.x) and bf16_exact(s.z)
    ref = ref_frame([s], N, H, W)
    sc, sh, mu, kx, kc = s.coef.view(5, C)
    gate = torch.where(s.z * sc + sh > 0, s.x, torch.zeros_like(s.x))
    got32 = sc * gate + (kx * (s.z - mu) + kc)
    assert got32.dtype == torch.float32 and torch.equal(got32.double(), ref)
    assert_rne_exercised(ref, f"BNBWD frame {(N, H, W, C)}")


def test_flat_raw_fine_values_round_both_ways():
    g = torch.Generator().manual_seed(203)
    x = torch.randint(-1024, 1025, (3, 7, 9, 3), generator=g).float() / 256
    assert_rne_exercised(x.double(), "RAW multiples of 2^-8")


def test_quant_z_ties_in_the_stats_cases():
    for shape in B.SHAPES:
        i = B.inputs(*shape)
        pre = i.z.double() * i.coef[:i.C].double() + i.coef[i.C:].double()
        assert torch.equal((i.z * i.coef[:i.C] + i.coef[i.C:]).double(), pre)     # exact in fp32
        if i.N * (i.H // 2) * (i.W // 2) * i.C >= 256:
            assert int((pre == 0).sum()) > 0
        for t in (i.da, i.dpool, i.skip, i.z):
            assert bf16_exact(t)


# ------------------------------------------------------------------------------------------ headroom + restatement
@pytest.mark.parametrize("kind,shape", B.stats_cases(), ids=[f"{k}-{'x'.join(map(str, s))}" for k, s in B.stats_cases()])
def test_stats_case_has_headroom_and_restates_in_fp32(kind, shape):
    i = B.inputs(*shape)
    da, part, absp, ug, ugx = B.ref_sums(kind, i)
    assert exact_headroom(absp[:, 0], ug, "sum g") < EXACT_LIMIT
    assert exact_headroom(absp[:, 1], ugx, "sum g * xhat") < EXACT_LIMIT
    # every term and every sum lies on its grid
    assert torch.equal(da.float().double(), da) and torch.equal(da / ug, (da / ug).round())
    assert torch.equal(part[:, 0] / ug, (part[:, 0] / ug).round()) and torch.equal(part[:, 1] / ugx, (part[:, 1] / ugx).round())
    # the same sums in fp32 (torch's own order), from fp32 inputs
    da32 = da.float()
    gate = torch.where(i.z * i.coef[:i.C] + i.coef[i.C:] > 0, da32, torch.zeros_like(da32))
    gx = gate * ((i.z - i.mean) * i.invstd)
    rows = B.da_of(kind, i)[1].reshape(-1)
    p32 = torch.zeros(part.shape, dtype=torch.float32)
    p32[:, 0].index_add_(0, rows, gate.reshape(-1, i.C))
    p32[:, 1].index_add_(0, rows, gx.reshape(-1, i.C))
    assert torch.equal(p32.double(), part)


def test_row_blocks_follow_the_documented_tilings():
    r = rows_bn_bwd(3, 33, 45, 32)            # 65536 / (4 * 32) = 512 pixels per block, 4455 pixels
    assert r.reshape(-1)[511] == 0 and r.reshape(-1)[512] == 1 and int(r.max()) + 1 == 9
    assert int(rows_bn_bwd(1, 2, 2, 32768).max()) == 3                       # at least one pixel per block
    m = rows_maxpool_bwd(2, 9, 11, 192)       # 8192 / 192 = 42 windows per block, 2 * 5 * 6 = 60 windows
    assert int(m.max()) + 1 == 2 and m[0, 8, 10] == (4 * 6 + 5) // 42 and m[1, 0, 0] == 30 // 42
    assert torch.equal(m[:, 0:8:2, 0:10:2], m[:, 1:9:2, 1:11:2])             # the four pixels of a window share a row
    assert int(rows_maxpool_bwd(1, 2, 2, 16384).max()) == 0


def test_dz_references_of_the_bnbwd_forms():
    for shape in B.BNBWD_SHAPES:
        i = B.inputs(*shape)
        da = B.ref_sums("maxpool", i)[0]
        dz = B.ref_dz(i, da)
        assert torch.equal(dz.float().double(), dz)
        sc, sh, mu, kx, kc = i.bcoef.view(5, i.C)
        gate = torch.where(i.z * sc + sh > 0, da.float(), torch.zeros_like(i.z))
        assert torch.equal((sc * gate + (kx * (i.z - mu) + kc)).double(), dz)
        if dz.numel() >= 2000:
            assert_rne_exercised(dz, f"dz {shape}")


# ------------------------------------------------------------------------------------------ ref_maxpool_bwd pinned
@pytest.mark.parametrize("N,H,W,C", [(2, 8, 8, 5), (1, 9, 11, 3), (2, 7, 4, 4), (1, 2, 2, 1), (1, 3, 2, 2)])
def test_ref_maxpool_bwd_matches_autograd_without_ties(N, H, W, C):
    """On inputs whose activations are positive and pairwise different (no ties, so the winner is unique) the
    routed gradient is autograd's of max_pool2d(a, 2) with respect to a = relu(z * scale + shift); the odd last
    row / column receives the skip gradient only."""
    g = torch.Generator().manual_seed(H * 17 + W)
    z = torch.rand(N, H, W, C, generator=g) + 0.5
    coef = torch.cat([torch.rand(C, generator=g) + 0.5, torch.rand(C, generator=g) * 0.1])
    dpool = torch.randn(N, H // 2, W // 2, C, generator=g)
    skip = torch.randn(N, H, W, C, generator=g)
    act = torch.relu(z.double() * coef[:C].double() + coef[C:].double()).requires_grad_(True)
    win = act.detach()[:, :2 * (H // 2), :2 * (W // 2)].reshape(N, H // 2, 2, W // 2, 2, C).permute(0, 1, 3, 5, 2, 4)
    top = win.reshape(-1, 4).topk(2, dim=1).values
    assert bool((top[:, 0] > top[:, 1]).all()) and bool((act > 0).all())
    pooled = F.max_pool2d(act.permute(0, 3, 1, 2), 2).permute(0, 2, 3, 1)
    (pooled * dpool.double()).sum().backward()
    got = ref_maxpool_bwd(dpool, None, z, coef)
    assert torch.equal(got, act.grad)
    assert bool((got[:, 2 * (H // 2):] == 0).all()) and bool((got[:, :, 2 * (W // 2):] == 0).all())
    assert torch.equal(ref_maxpool_bwd(dpool, skip, z, coef), skip.double() + got)


def test_ref_maxpool_bwd_ties_route_to_the_first_element():
    coef = torch.tensor([1.0, 0.0])                                        # C = 1: scale 1, shift 0
    dpool = torch.tensor([3.0]).view(1, 1, 1, 1)
    for z, winner in (([1.0, 1.0, 1.0, 1.0], 0),                           # a constant window
                      ([-1.0, -2.0, -0.5, -3.0], 0),                       # all zero after ReLU
                      ([0.0, 0.0, 0.0, 0.0], 0),
                      ([0.5, 1.0, 1.0, 0.25], 1),                          # the first of two equal maxima
                      ([0.5, 0.25, 1.0, 1.0], 2)):
        dx = ref_maxpool_bwd(dpool, None, torch.tensor(z).view(1, 2, 2, 1), coef).reshape(-1).tolist()
        assert dx == [3.0 if k == winner else 0.0 for k in range(4)], (z, dx)


def test_ref_bn_bwd_sums_by_hand():
    z = torch.tensor([1.0, -1.0, 0.5, 0.25]).view(1, 2, 2, 1)
    da = torch.tensor([2.0, 5.0, -1.0, 0.5], dtype=torch.float64).view(1, 2, 2, 1)
    coef, mean, invstd = torch.tensor([1.0, -0.25]), torch.tensor([0.5]), torch.tensor([2.0])
    rows = torch.tensor([0, 0, 1, 1]).view(1, 2, 2)
    part, absp = ref_bn_bwd_sums(da, z, coef, mean, invstd, rows)
    # masks: 1 - .25 > 0, -1.25 no, .25 > 0, 0 no ;  xhat = 1, -3, 0, -.5
    assert part.reshape(-1).tolist() == [2.0, 2.0, -1.0, 0.0]
    assert absp.reshape(-1).tolist() == [2.0, 2.0, 1.0, 0.0]
