"""The conditions under which tests/test_head_exact_gpu.py may demand equality with float64, checked without a GPU on
every case of tests/head_cases.py: each case passes its headroom assertions (they sit inside the reference builders);
a plain fp32 torch restatement of each formula — the forward FMA chain, dy * (y * (1 - y)), da, the BN-backward sums,
dz, and the block slabs summed in fp64 — gives the float64 reference bit for bit on the same inputs, so a miss on the
GPU is the kernel's; the fp32 restatement of the sigmoid meets the fixed 8-unit ceiling on the same logits; rows_head
follows pmu_head1x1_bwd_tiles's arithmetic; and the bf16 dz inputs round ties in both directions."""
import os

import pytest
import torch

import head_cases as HC
from head_cases import DEEP, GEOMETRIES, RAGGED, gid
from helpers import EXACT_LIMIT, assert_rne_exercised, bf16_exact, ref_frame, rne_census, ulp32


# ------------------------------------------------------------------------------------------ grids and tilings
def test_grids_are_what_the_docstring_claims():
    l = HC.layer(*RAGGED, 64)
    a = ref_frame([HC.act_src(l)], *RAGGED)
    assert torch.equal(a / HC.U_A, (a / HC.U_A).round()) and float(a.max()) <= 3.5 and int((a == 0).sum()) > 0
    pre = l.z.double() * l.coef[:64].double() + l.coef[64:].double()
    assert torch.equal((l.z * l.coef[:64] + l.coef[64:]).double(), pre) and int((pre == 0).sum()) > 0   # exact masks, ties
    xhat = (l.z.double() - l.mean.double()) * l.invstd.double()
    assert torch.equal(xhat / HC.U_X, (xhat / HC.U_X).round()) and float(xhat.abs().max()) <= 4.0
    assert bf16_exact(l.z)                                                       # the bf16-stored x of the forward
    w, b = HC.fwd_params(8, 64)
    assert torch.equal(w * 8, (w * 8).round()) and float(w.abs().max()) == 1.0
    assert torch.equal(b * 4, (b * 4).round()) and float(b.abs().max()) <= 2.0
    ws, bs = HC.fwd_params(8, 256, sparse=True, sat=-1)
    assert 8 <= float((ws != 0).sum(1).float().mean()) <= 40 and bs[7] == -40.0 and bs[6] == 40.0
    for K, levels in ((4, {0.0, 0.25, 0.5, 0.75, 1.0}), (5, {0.0, 0.5, 1.0})):
        gr = HC.grads(2, K, 7, 9, 16, 1)
        assert set(gr.y.unique().tolist()) == levels and set(gr.w.unique().tolist()) == {-1.0, -0.5, 0.0, 0.5, 1.0}
        assert torch.equal(gr.dy * 4, (gr.dy * 4).round()) and float(gr.dy.abs().max()) == 2.0
        g = HC.ref_g(gr, 1)
        assert bool((g[(gr.y == 0) | (gr.y == 1)] == 0).all())                   # the endpoints give exact zeros
    c = HC.layer(*RAGGED, 16).bcoef.view(5, 16)
    assert torch.equal(c[3:] * 16, (c[3:] * 16).round())                          # dyadic kx, kc


def test_rows_head_follows_the_tile_arithmetic():
    """pmu_head1x1_bwd_tiles = cdiv(N * H * W, 2048); the generic weight gradient's blocks hold 1024 pixels."""
    for geom, R, R1 in ((HC.ONE, 1, 1), (RAGGED, 2, 3), (HC.FULL, 1, 2), (HC.OVER, 2, 3), (HC.SMALL, 1, 1), (DEEP, 66, 131)):
        P = geom[0] * geom[1] * geom[2]
        r = HC.rows_head(*geom)
        assert r.shape == geom and int(r.max()) + 1 == R == -(-P // 2048)
        assert int(HC.rows_head(*geom, ppb=HC.W1_PPB).max()) + 1 == R1 == -(-P // 1024)
        flat = r.reshape(-1)
        assert flat[0] == 0 and (P <= 2048 or (flat[2047] == 0 and flat[2048] == 1))
    # the deep case reaches pmu_colsum64x16's four-way loop (rows r + 48 < R for r < 16): once, and twice
    assert 65 <= 66 < 129 <= 131 < 193
    from pmu_hip._lib import LIB_PATH, load_library
    if os.path.exists(LIB_PATH):              # a host function: no GPU needed
        cdll = load_library()
        for geom in GEOMETRIES + (DEEP,):
            assert cdll.pmu_head1x1_bwd_tiles(*geom) == int(HC.rows_head(*geom).max()) + 1
        for C in range(1, 300):
            assert bool(cdll.pmu_head1x1_bwd_bnr_ok(2, 7, 9, C)) == HC.fast_shape(C)


# ------------------------------------------------------------------------------------------ forward
def _fma_chain32(a32, w32, b32):
    """The kernels' sum in fp32, one channel after the other (every operation rounds; on these grids none has to)."""
    N, H, W, C = a32.shape
    acc = torch.zeros(N, w32.shape[0], H, W) if b32 is None else b32.view(1, -1, 1, 1).expand(N, -1, H, W).clone()
    for c in range(C):
        acc = acc + a32[..., c].unsqueeze(1) * w32[:, c].view(1, -1, 1, 1)
    return acc


def _sigmoid32(v32):
    return 1.0 / (1.0 + torch.exp(-v32))


def _fwd_conditions(srcs, N, H, W, C, K, ua, sat, where, chain):
    a32 = ref_frame(srcs, N, H, W).float()
    w, b = HC.fwd_params(K, C)
    for bias in (b, None):
        ref = HC.ref_fwd(srcs, N, H, W, w, bias, where, ua)                       # (asserts the headroom)
        if chain:
            got = _fma_chain32(a32, w, bias)
        else:
            got = torch.einsum("nhwc,kc->nkhw", a32, w) + (0 if bias is None else bias.view(1, -1, 1, 1))
        assert got.dtype == torch.float32 and torch.equal(got.double(), ref), where
    ws, bs = HC.fwd_params(K, C, sparse=True, sat=sat)
    v = HC.ref_fwd(srcs, N, H, W, ws, bs, where + " sigmoid", ua)
    assert float(v.abs().max()) <= HC.SIG_VMAX, where
    ref = torch.sigmoid(v)
    assert float(ref.min()) >= 2.0 ** -126                                       # normal numbers only
    err = float(((_sigmoid32(v.float()).double() - ref).abs() / ulp32(ref)).max())
    assert err <= HC.SIG_CEILING, f"{where}: fp32 sigmoid off by {err} ulp32"
    if sat:
        assert bool((v >= 40).any()) or bool((v <= -30).any())
        assert bool((_sigmoid32(v.float())[v >= 40] == 1.0).all())
    return err


@pytest.mark.parametrize("C,K", HC.FWD_FAST, ids=[f"C{c}-K{k}" for c, k in HC.FWD_FAST])
def test_fwd_fast_cases(C, K):
    _fwd_conditions([HC.act_src(HC.layer(*RAGGED, C))], *RAGGED, C, K, HC.U_A, HC.sat_of("fast", C, K),
                    f"fwd fast C={C} K={K}", chain=C <= 64)


def test_fwd_geometry_and_generic_cases():
    for geom in GEOMETRIES:
        if geom == RAGGED:
            continue
        for C, K in HC.FWD_FAST_GEOM:
            _fwd_conditions([HC.act_src(HC.layer(*geom, C))], *geom, C, K, HC.U_A, HC.sat_of("geom", C, K),
                            f"fwd fast {gid(geom)} C={C} K={K}", chain=False)
    for geom, name, K in HC.FWD_GENERIC:
        srcs, ua = HC.generic_frame(name, *geom)
        C = sum(s.x.shape[3] for s in srcs)
        assert not (len(srcs) == 1 and srcs[0].mode == 1 and srcs[0].pool == 0 and srcs[0].off == (0, 0) and HC.fast_shape(C))
        _fwd_conditions(srcs, *geom, C, K, ua, HC.sat_of("generic", C, K), f"fwd generic {name} {gid(geom)} K={K}", chain=False)
    assert HC.HEADROOM["forward logit"] < EXACT_LIMIT


# ------------------------------------------------------------------------------------------ backward
def _bwd_conditions(geom, C, K, sig, where, sums=False, wgrad=False, dz=False):
    N, H, W = geom
    gr = HC.grads(N, K, H, W, C, sig)
    g64 = HC.ref_g(gr, sig)
    g32 = gr.dy * (gr.y * (1.0 - gr.y)) if sig else gr.dy
    assert g32.dtype == torch.float32 and torch.equal(g32.double(), g64), where
    da64 = HC.ref_da(g64, gr.w, gr.ug, where)
    da32 = torch.einsum("nkhw,kc->nhwc", g32, gr.w)
    assert torch.equal(da32.double(), da64), where
    if not (sums or wgrad or dz):
        return
    l = HC.layer(N, H, W, C)
    rows = HC.rows_head(N, H, W).reshape(-1)
    if sums:
        part = HC.ref_part(da64, l, gr.ug, where)
        gate = torch.where(l.z * l.coef[:C] + l.coef[C:] > 0, da32, torch.zeros_like(da32))
        gx = gate * ((l.z - l.mean) * l.invstd)
        p32 = torch.zeros(part.shape, dtype=torch.float32)
        p32[:, 0].index_add_(0, rows, gate.reshape(-1, C))
        p32[:, 1].index_add_(0, rows, gx.reshape(-1, C))
        assert torch.equal(p32.double(), part), where
    if wgrad:
        a64 = ref_frame([HC.act_src(l)], N, H, W)
        _slabs_restate(g64, a64, HC.HPPB, gr.ug, HC.U_A, where)
    if dz:
        for bf in (False, True):
            if bf and C % 8:
                continue
            grd = HC.grads(N, K, H, W, C, sig, fine=bf)
            da = HC.ref_da(HC.ref_g(grd, sig), grd.w, grd.ug, where)
            ref = HC.ref_dz(l, da)
            sc, sh, mu, kx, kc = l.bcoef.view(5, C)
            gate = torch.where(l.z * sc + sh > 0, da.float(), torch.zeros_like(l.z))
            assert torch.equal((sc * gate + (kx * (l.z - mu) + kc)).double(), ref), where
            if bf and ref.numel() >= 2000:
                c = assert_rne_exercised(ref, where)                              # ties in both directions, up and down
                assert c["tie_up"] > 0 and c["tie_down"] > 0


def _slabs_restate(g64, a64, ppb, ug, ua, where):
    """dw, db as the kernels form them — an fp32 slab per block of ppb pixels, the slabs summed in fp64, one cast —
    against the float64 sum over the whole map rounded to fp32."""
    dw64, db64 = HC.ref_wgrad(g64, a64, ppb, ug, ua, where)                       # (asserts the headroom per block)
    K, C = dw64.shape
    gp, ap = g64.float().permute(0, 2, 3, 1).reshape(-1, K), a64.float().reshape(-1, C)
    dw, db = torch.zeros(K, C, dtype=torch.float64), torch.zeros(K, dtype=torch.float64)
    for p0 in range(0, gp.shape[0], ppb):
        dw += (gp[p0:p0 + ppb].t() @ ap[p0:p0 + ppb]).double()
        db += gp[p0:p0 + ppb].sum(0).double()
    assert torch.equal(dw, dw64) and torch.equal(db, db64), where
    assert torch.equal(dw.float().double(), dw64.float().double())


@pytest.mark.parametrize("sig", [0, 1])
def test_bwd_cases(sig):
    for geom in (RAGGED, HC.SMALL):
        for C, K in HC.BWD:
            _bwd_conditions(geom, C, K, sig, f"bwd {gid(geom)} C={C} K={K} sig={sig}")


@pytest.mark.parametrize("C,K,sig", HC.BNR, ids=[f"C{c}-K{k}-sig{s}" for c, k, s in HC.BNR])
def test_bwd_bnr_cases(C, K, sig):
    _bwd_conditions(RAGGED, C, K, sig, f"bnr C={C} K={K} sig={sig}", sums=True, wgrad=True)


@pytest.mark.parametrize("C,K,sig", HC.DZ, ids=[f"C{c}-K{k}-sig{s}" for c, k, s in HC.DZ])
def test_bwd_dz_cases(C, K, sig):
    _bwd_conditions(RAGGED, C, K, sig, f"dz C={C} K={K} sig={sig}", dz=True)


def test_bwd_geometry_and_deep_cases():
    for geom in GEOMETRIES:
        if geom == RAGGED:
            continue
        for C, K, sig in HC.BNR_GEOM:
            _bwd_conditions(geom, C, K, sig, f"bnr {gid(geom)} C={C} K={K}", sums=True, wgrad=True)
        for C, K, sig in HC.DZ_GEOM:
            _bwd_conditions(geom, C, K, sig, f"dz {gid(geom)} C={C} K={K}", dz=True)
    _bwd_conditions(DEEP, 8, 3, 1, "bnr deep", sums=True, wgrad=True)
    for k in ("da", "sum g", "sum g * xhat", "dw", "db"):
        assert HC.HEADROOM[k] < EXACT_LIMIT


def test_dz_rounding_census_by_hand():
    """What the bf16 dz test relies on: truncation and round-half-away both differ from RNE on such values."""
    l = HC.layer(*RAGGED, 16)
    gr = HC.grads(*RAGGED[:1], 2, *RAGGED[1:], 16, 0, fine=True)
    ref = HC.ref_dz(l, HC.ref_da(HC.ref_g(gr, 0), gr.w, gr.ug, "census"))
    c = rne_census(ref)
    assert min(c["tie_up"], c["tie_down"], c["up"], c["down"]) > 0, c
    trunc = (ref.float().view(torch.int32) & -65536).view(torch.float32)
    assert not torch.equal(trunc.double(), ref.float().to(torch.bfloat16).double())


# ------------------------------------------------------------------------------------------ weight gradient
@pytest.mark.parametrize("geom,name,K", HC.WGRAD, ids=[f"{gid(g)}-{n}-K{k}" for g, n, k in HC.WGRAD])
def test_wgrad_cases(geom, name, K):
    N, H, W = geom
    srcs, ua, xb, ppb = HC.wgrad_sources(name, N, H, W)
    C = sum(s.x.shape[3] for s in srcs)
    assert C <= 256 and (not xb or bf16_exact(srcs[0].x))
    gr = HC.grads(N, K, H, W, C, 0)
    _slabs_restate(HC.ref_g(gr, 0), ref_frame(srcs, N, H, W), ppb, gr.ug, ua, f"wgrad {gid(geom)} {name} K={K}")
    if geom == DEEP:
        assert -(-N * H * W // ppb) == (66 if ppb == HC.HPPB else 131)
