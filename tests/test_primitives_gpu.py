"""The unfused fp32 primitives — the baselines tests/test_bnr_gpu.py and tests/test_pool_fuse_gpu.py assert
their fused twins bit-equal to, and the small entry points of the probabilistic path — each against torch's
own operator or a float64 restatement of the formula in include/pmunet_hip.h:

  pmu_maxpool2_bwd      F.max_pool2d backward (first maximum in row-major order), bit-equal; scalar (C % 4
                        != 0) and vector kernels, BN+ReLU and raw (coef == NULL) inputs, accumulate 0 / 1
  pmu_avgpool2_bwd      backward of F.avg_pool2d(2, 2, ceil_mode=True), bit-equal (divisors 1, 2, 4)
  pmu_spatial_mean(_bwd), pmu_linear_fwd / _bwd, pmu_fcomb_zbias   float64, worst-case fp32 summation bounds
  pmu_bnrelu_apply      fp32 relu(z*scale + shift) on exactly representable inputs, bit-equal
  pmu_head1x1_bwd, pmu_wgrad1x1   float64; fast (C = 4 * 2^k <= 256) and generic kernels
  pmu_dice_sums         exact on 0/1 inputs, 1e-12 relative on random ones

Inputs that decide a ReLU mask or a max-pool winner come from helpers.quant_z / quant_bn (exact in fp32,
with deliberate ties and all-zero windows); values that only enter sums are ordinary randn.  u = 2^-24 is
fp32's unit roundoff: a sum of n fp32 terms in any order, each term rounded once, is within (n + 1) u
sum|terms| of the exact sum to first order; the bounds below use (n + 2) u sum|terms|."""
import pytest
import torch
import torch.nn.functional as F

from helpers import SRC_BNRELU, SRC_RAW, quant_bn, quant_z, ulp32

pytestmark = pytest.mark.gpu

U = 2.0 ** -24
MAPS = [(2, 7, 9), (3, 33, 45), (1, 2, 2)]
NAN = float("nan")


def _nchw(t):
    return t.permute(0, 3, 1, 2)


def _nhwc(t):
    return t.permute(0, 2, 3, 1).contiguous()


def _L():
    from pmu_hip import _lib as L
    return L


# ------------------------------------------------------------------------------------------ pooling
@pytest.mark.parametrize("accumulate", [0, 1])
@pytest.mark.parametrize("with_coef", [True, False])
@pytest.mark.parametrize("C", [6, 64])
@pytest.mark.parametrize("N,H,W", MAPS)
def test_maxpool2_bwd_equals_torch(dev, N, H, W, C, with_coef, accumulate):
    L = _L()
    g = torch.Generator().manual_seed(N * H * W + C + 2 * with_coef + accumulate)
    z, coef = quant_z(N, H, W, C, g), quant_bn(C, g)
    dpool = torch.randn(N, H // 2, W // 2, C, generator=g)
    pre = torch.randn(N, H, W, C, generator=g)
    a = (torch.relu(z * coef[:C] + coef[C:]) if with_coef else z.clone()).requires_grad_(True)   # exact in fp32
    F.max_pool2d(_nchw(a), 2).backward(_nchw(dpool))
    want = pre + a.grad if accumulate else a.grad
    if H % 2:
        assert not a.grad[:, H - 1].any()           # the trailing odd row / column belongs to no window
    if W % 2:
        assert not a.grad[:, :, W - 1].any()
    dx = pre.to(dev) if accumulate else torch.full((N, H, W, C), NAN, device=dev)
    dpd, zd, cd = dpool.to(dev), z.to(dev), coef.to(dev)
    L.call("pmu_maxpool2_bwd", dpd.data_ptr(), zd.data_ptr(), cd.data_ptr() if with_coef else None, N, H, W, C,
           dx.data_ptr(), accumulate, L.stream())
    torch.cuda.synchronize()
    assert not torch.isnan(dx).any()
    assert torch.equal(dx.cpu(), want)


@pytest.mark.parametrize("C", [6, 64])
@pytest.mark.parametrize("N,H,W", MAPS + [(2, 8, 6), (2, 7, 6), (2, 8, 9)])
def test_avgpool2_bwd_equals_torch(dev, N, H, W, C):
    L = _L()
    g = torch.Generator().manual_seed(N * H * W + C)
    dpool = torch.randn(N, (H + 1) // 2, (W + 1) // 2, C, generator=g)
    a = torch.zeros(N, H, W, C, requires_grad=True)
    F.avg_pool2d(_nchw(a), 2, 2, ceil_mode=True).backward(_nchw(dpool))
    dx = torch.full((N, H, W, C), NAN, device=dev)
    dpd = dpool.to(dev)
    L.call("pmu_avgpool2_bwd", dpd.data_ptr(), N, H, W, C, dx.data_ptr(), L.stream())
    torch.cuda.synchronize()
    assert torch.equal(dx.cpu(), a.grad)


# ------------------------------------------------------------------------------------- latent head
@pytest.mark.parametrize("C", [6, 64, 192])
@pytest.mark.parametrize("N,H,W", MAPS)
def test_spatial_mean_fwd_bwd_vs_float64(dev, N, H, W, C):
    L = _L()
    g = torch.Generator().manual_seed(N * H * W + C)
    z, coef = quant_z(N, H, W, C, g), quant_bn(C, g)
    act = torch.relu(z.double() * coef[:C].double() + coef[C:].double())
    ref = act.mean(dim=(1, 2))
    bound = H * W * U * act.abs().mean(dim=(1, 2))      # worst case of any fp32 summation order
    assert float(bound.max()) < 1.0 / (H * W) or H * W <= 4   # below a dropped pixel of value 1
    out = torch.full((N, C), NAN, device=dev)
    dmean = torch.randn(N, C, generator=g)
    zd, cd, dmd = z.to(dev), coef.to(dev), dmean.to(dev)
    L.call("pmu_spatial_mean", zd.data_ptr(), cd.data_ptr(), N, H, W, C, out.data_ptr(), L.stream())
    da = torch.full((N, H, W, C), NAN, device=dev)
    L.call("pmu_spatial_mean_bwd", dmd.data_ptr(), N, H, W, C, da.data_ptr(), L.stream())
    torch.cuda.synchronize()
    err = (out.double().cpu() - ref).abs()
    print(f"spatial_mean {(N, H, W, C)}: max err/bound {float((err / bound.clamp_min(1e-300)).max()):.3f}")
    assert bool((err <= bound).all()), float((err - bound).max())
    rb = (dmean.double() / (H * W))[:, None, None, :].expand(N, H, W, C)
    eb = (da.double().cpu() - rb).abs() / ulp32(rb)
    print(f"spatial_mean_bwd {(N, H, W, C)}: {float(eb.max()):.3f} ulp")
    assert float(eb.max()) <= 2.0


@pytest.mark.parametrize("opts", ["all", "no_b", "no_dx", "no_db"])
@pytest.mark.parametrize("N,K,M", [(1, 6, 12), (4, 192, 12), (3, 300, 256), (65, 37, 5)])
def test_linear_fwd_bwd_vs_float64(dev, N, K, M, opts):
    L = _L()
    g = torch.Generator().manual_seed(N + K + M)
    x, w, b = torch.randn(N, K, generator=g), torch.randn(M, K, generator=g), torch.randn(M, generator=g)
    dy = torch.randn(N, M, generator=g)
    xd, wd, bd, dyd = x.to(dev), w.to(dev), b.to(dev), dy.to(dev)
    x6, w6, b6, dy6 = x.double(), w.double(), b.double(), dy.double()
    has_b = opts != "no_b"
    y = torch.full((N, M), NAN, device=dev)
    L.call("pmu_linear_fwd", xd.data_ptr(), wd.data_ptr(), bd.data_ptr() if has_b else None, N, K, M, y.data_ptr(),
           L.stream())
    dx = torch.full((N, K), NAN, device=dev)
    dw = torch.full((M, K), NAN, device=dev)
    db = torch.full((M,), NAN, device=dev)
    L.call("pmu_linear_bwd", xd.data_ptr(), wd.data_ptr(), dyd.data_ptr(), N, K, M,
           None if opts == "no_dx" else dx.data_ptr(), dw.data_ptr(), None if opts == "no_db" else db.data_ptr(),
           L.stream())
    torch.cuda.synchronize()
    ref_y = x6 @ w6.T + (b6 if has_b else 0)
    mag_y = x6.abs() @ w6.abs().T + (b6.abs() if has_b else 0)
    worst = {}

    def close(name, got, ref, mag, n):
        e = (got.double().cpu() - ref).abs() / ((n + 2) * U * mag)
        worst[name] = float(e.max())
        assert worst[name] <= 1.0, (name, worst[name])

    close("y", y, ref_y, mag_y, K)
    close("dw", dw, dy6.T @ x6, dy6.abs().T @ x6.abs(), N)
    if opts == "no_dx":
        assert torch.isnan(dx).all()
    else:
        close("dx", dx, dy6 @ w6, dy6.abs() @ w6.abs(), M)
    if opts == "no_db":
        assert torch.isnan(db).all()
    else:
        close("db", db, dy6.sum(0), dy6.abs().sum(0), N)
    print(f"linear {(N, K, M)} {opts}: err/bound {worst}")


def test_linear_bwd_refuses_wide_output(dev):
    L = _L()
    N, K, M = 2, 8, 257
    t = lambda *s: torch.zeros(*s, device=dev)
    x, w, dy, dx, dw, db = t(N, K), t(M, K), t(N, M), t(N, K), t(M, K), t(M)
    rc = L.lib().pmu_linear_bwd(x.data_ptr(), w.data_ptr(), dy.data_ptr(), N, K, M, dx.data_ptr(), dw.data_ptr(),
                                db.data_ptr(), L.stream())
    assert rc == L.PMU_ERR_ARG


@pytest.mark.parametrize("SN,Fw,Lz", [(1, 8, 2), (6, 64, 6), (48, 32, 0)])
def test_fcomb_zbias_vs_float64(dev, SN, Fw, Lz):
    L = _L()
    g = torch.Generator().manual_seed(SN + Fw + Lz)
    w1, b1 = torch.randn(Fw, Fw + Lz, generator=g), torch.randn(Fw, generator=g)
    z = torch.randn(SN, max(Lz, 1), generator=g)[:, :Lz].contiguous()
    zd = z.to(dev) if Lz else torch.zeros(1, device=dev)   # L == 0: no element of z is read
    zb = torch.full((SN, Fw), NAN, device=dev)
    w1d, b1d = w1.to(dev), b1.to(dev)
    L.call("pmu_fcomb_zbias", zd.data_ptr(), w1d.data_ptr(), b1d.data_ptr(), SN, Fw, Lz, zb.data_ptr(),
           L.stream())
    torch.cuda.synchronize()
    wz = w1[:, Fw:].double()
    ref = z.double() @ wz.T + b1.double()
    if Lz == 0:
        assert torch.equal(zb.cpu(), b1[None].expand(SN, Fw))
        return
    mag = z.double().abs() @ wz.abs().T + b1.double().abs()
    e = float(((zb.double().cpu() - ref).abs() / ((Lz + 2) * U * mag)).max())
    print(f"fcomb_zbias {(SN, Fw, Lz)}: err/bound {e:.3f}")
    assert e <= 1.0


@pytest.mark.parametrize("C", [6, 64])
def test_bnrelu_apply_equals_fp32(dev, C):
    L = _L()
    P = 1234
    g = torch.Generator().manual_seed(C)
    z, coef = quant_z(1, 1, P, C, g).view(P, C), quant_bn(C, g)
    want = torch.relu(z * coef[:C] + coef[C:])           # exact in fp32, fused or not
    assert torch.equal(want.double(), torch.relu(z.double() * coef[:C].double() + coef[C:].double()))
    out = torch.full((P, C), NAN, device=dev)
    zd, cd = z.to(dev), coef.to(dev)
    L.call("pmu_bnrelu_apply", zd.data_ptr(), cd.data_ptr(), P, C, out.data_ptr(), L.stream())
    torch.cuda.synchronize()
    assert torch.equal(out.cpu(), want)


# ------------------------------------------------------------------------------------------ 1x1 head
HEAD_FAST = [(1, 64), (3, 32), (8, 256)]      # C = 4 * 2^k <= 256: the channel-quad kernels
HEAD_GENERIC = [(2, 24), (3, 6), (8, 20)]     # any other C: one pixel per thread / frame_value4
HEAD_MAPS = [(2, 37, 45), (1, 3, 5)]


@pytest.mark.parametrize("sig", [True, False])
@pytest.mark.parametrize("K,C", HEAD_FAST + HEAD_GENERIC)
@pytest.mark.parametrize("N,H,W", HEAD_MAPS)
def test_head1x1_bwd_vs_float64(dev, N, H, W, K, C, sig):
    L = _L()
    g = torch.Generator().manual_seed(N * H * W + 10 * K + C + sig)
    dy = torch.randn(N, K, H, W, generator=g)
    y = torch.sigmoid(torch.randn(N, K, H, W, generator=g) * 2)
    w = torch.randn(K, C, generator=g) * 0.3
    dl_ref = dy.double() * y.double() * (1 - y.double()) if sig else dy.double()
    da_ref = torch.einsum("nkhw,kc->nhwc", dl_ref, w.double())
    dl = torch.full((N, K, H, W), NAN, device=dev)
    da = torch.full((N, H, W, C), NAN, device=dev)
    dyd, yd, wd = dy.to(dev), y.to(dev), w.to(dev)
    L.call("pmu_head1x1_bwd", dyd.data_ptr(), yd.data_ptr(), int(sig), wd.data_ptr(), K, C, N, H,
           W, dl.data_ptr(), da.data_ptr(), L.stream())
    torch.cuda.synchronize()
    assert not torch.isnan(dl).any() and not torch.isnan(da).any()
    e_dl = float((dl.double().cpu() - dl_ref).abs().max()) / max(1.0, float(dl_ref.abs().max()))
    e_da = float((da.double().cpu() - da_ref).abs().max()) / max(1.0, float(da_ref.abs().max()))
    print(f"head1x1_bwd {(N, H, W, K, C)} sigmoid={sig}: dl {e_dl:.3e} da {e_da:.3e}")
    assert e_dl <= 1e-5 and e_da <= 1e-5, (e_dl, e_da)


@pytest.mark.parametrize("K,C,mode", [(k, c, SRC_BNRELU) for k, c in HEAD_FAST + HEAD_GENERIC] +
                         [(3, 32, SRC_RAW), (2, 24, SRC_RAW)])    # RAW: host_head_fast false at a fast C
@pytest.mark.parametrize("N,H,W", HEAD_MAPS)
def test_wgrad1x1_vs_float64(dev, N, H, W, K, C, mode):
    L = _L()
    from pmu_hip.engine import Src, frame_of
    g = torch.Generator().manual_seed(N * H * W + 10 * K + C + mode)
    dl = torch.randn(N, K, H, W, generator=g)
    if mode == SRC_BNRELU:
        z, coef = quant_z(N, H, W, C, g), quant_bn(C, g)
        act = torch.relu(z.double() * coef[:C].double() + coef[C:].double())
        src = Src(z.to(dev), SRC_BNRELU, coef.to(dev))
    else:
        z = torch.randn(N, H, W, C, generator=g)
        act = z.double()
        src = Src(z.to(dev))
    dw_ref = torch.einsum("nkhw,nhwc->kc", dl.double(), act)
    dw_mag = torch.einsum("nkhw,nhwc->kc", dl.double().abs(), act.abs())
    db_ref, db_mag = dl.double().sum(dim=(0, 2, 3)), dl.double().abs().sum(dim=(0, 2, 3))
    wsb = L.lib().pmu_wgrad1x1_ws(N * H * W, K, C)
    ws = torch.full((max(1, (wsb + 3) // 4),), NAN, device=dev)
    dw = torch.full((K, C), NAN, device=dev)
    db = torch.full((K,), NAN, device=dev)
    dld = dl.to(dev)
    L.call("pmu_wgrad1x1", dld.data_ptr(), frame_of([src], N, H, W), K, dw.data_ptr(), db.data_ptr(),
           ws.data_ptr(), wsb, L.stream())
    torch.cuda.synchronize()
    assert not torch.isnan(dw).any() and not torch.isnan(db).any()
    e_w = float(((dw.double().cpu() - dw_ref).abs() / dw_mag.clamp_min(1e-30)).max())
    e_b = float(((db.double().cpu() - db_ref).abs() / db_mag).max())
    print(f"wgrad1x1 {(N, H, W, K, C)} mode={mode}: dw {e_w:.3e} db {e_b:.3e} (of sum|terms|)")
    assert bool(((dw.double().cpu() - dw_ref).abs() <= 1e-5 * dw_mag).all()), e_w
    assert e_b <= 1e-5, e_b


def test_head_refusals(dev):
    """K above 8 (both entries) and C above 256 (pmu_wgrad1x1) are refused on the host, before any launch."""
    L = _L()
    from pmu_hip.engine import Src, frame_of
    N, H, W = 1, 3, 5
    t = lambda *s: torch.zeros(*s, device=dev)
    dl9, y9, w9, da8, db9 = t(N, 9, H, W), t(N, 9, H, W), t(9, 8), t(N, H, W, 8), t(9)
    rc = L.lib().pmu_head1x1_bwd(dl9.data_ptr(), y9.data_ptr(), 1, w9.data_ptr(), 9, 8, N, H, W, y9.data_ptr(),
                                 da8.data_ptr(), L.stream())
    assert rc == L.PMU_ERR_ARG
    ws = t(1 << 20)
    act8, act260 = Src(t(N, H, W, 8)), Src(t(N, H, W, 260))
    rc = L.lib().pmu_wgrad1x1(dl9.data_ptr(), frame_of([act8], N, H, W), 9, w9.data_ptr(), db9.data_ptr(),
                              ws.data_ptr(), 4 * ws.numel(), L.stream())
    assert rc == L.PMU_ERR_ARG
    dw260 = t(2, 260)
    rc = L.lib().pmu_wgrad1x1(dl9.data_ptr(), frame_of([act260], N, H, W), 2, dw260.data_ptr(), db9.data_ptr(),
                              ws.data_ptr(), 4 * ws.numel(), L.stream())
    assert rc == L.PMU_ERR_ARG
    torch.cuda.synchronize()


# ------------------------------------------------------------------------------- batched weight packs
@pytest.mark.parametrize("dgrad", [False, True])
@pytest.mark.parametrize("layout", ["f32", "dma"])
def test_convT_pack_multi_equals_single(dev, layout, dgrad):
    """pmu_convT2x2_pack_multi / pmu_convT2x2_pack_dma_multi (the re-pack after an optimizer step): one batched
    launch over several ConvTranspose2d weights, each job's blocks from the *_blocks query, equals the
    single-tensor packs bit for bit (job fields as pmu_hip.packs.repack fills them)."""
    L = _L()
    sfx = "" if layout == "f32" else "_dma"
    shapes = [(128, 64), (24, 12), (6, 5)] if layout == "f32" else [(128, 32), (256, 64), (128, 96)]
    g = torch.Generator().manual_seed(3 + int(dgrad))
    ws = [torch.randn(ci, co, 2, 2, generator=g).to(dev) for ci, co in shapes]
    size = getattr(L.lib(), "pmu_convT2x2_packed_size" + sfx)
    outs = [torch.full((size(ci, co),), 0x55, dtype=torch.uint8, device=dev) for ci, co in shapes]
    jobs = (L.PmuPackJob * len(ws))()
    b0 = 0
    for i, (w, o) in enumerate(zip(ws, outs)):
        nb = getattr(L.lib(), f"pmu_convT2x2_pack{sfx}_blocks")(w.shape[0], w.shape[1], int(dgrad))
        jobs[i] = L.PmuPackJob(w.data_ptr(), o.data_ptr(), w.shape[0], w.shape[1], b0, nb)
        b0 += nb
    jt = torch.frombuffer(bytearray(bytes(jobs)), dtype=torch.uint8).to(dev)
    if layout == "f32":
        L.call("pmu_convT2x2_pack_multi", jt.data_ptr(), len(ws), b0, int(dgrad), L.stream())
    else:
        L.call("pmu_convT2x2_pack_dma_multi", jt.data_ptr(), len(ws), b0, int(dgrad), L.stream())
    torch.cuda.synchronize()
    for w, o in zip(ws, outs):
        single = torch.full_like(o, 0x55)
        if layout == "f32":
            L.call("pmu_convT2x2_pack", w.data_ptr(), w.shape[0], w.shape[1], int(dgrad), single.data_ptr(), L.stream())
        else:
            L.call("pmu_convT2x2_pack_dma", w.data_ptr(), w.shape[0], w.shape[1], int(dgrad), single.data_ptr(),
                   L.stream())
        torch.cuda.synchronize()
        assert torch.equal(o, single), tuple(w.shape)
    # the fp32 layout itself (csrc/convT.hip): forward [ab][co][ci], input gradient [ci][ab][co]
    if layout == "f32":
        for w, o in zip(ws, outs):
            want = w.permute(2, 3, 1, 0) if not dgrad else w.permute(0, 2, 3, 1)
            assert torch.equal(o.view(torch.float32), want.contiguous().flatten())


# ------------------------------------------------------------------------------------------- metrics
@pytest.mark.parametrize("n", [1, 1000, 70001])
def test_dice_sums_exact_and_float64(dev, n):
    L = _L()
    g = torch.Generator().manual_seed(n)
    out = torch.full((3,), NAN, dtype=torch.float64, device=dev)
    a = (torch.rand(n, generator=g) > 0.5).float()
    b = (torch.rand(n, generator=g) > 0.3).float()
    ad, bd = a.to(dev), b.to(dev)
    L.call("pmu_dice_sums", ad.data_ptr(), bd.data_ptr(), n, out.data_ptr(), L.stream())
    torch.cuda.synchronize()
    assert out.cpu().tolist() == [float((a * b).sum()), float(a.sum()), float(b.sum())]
    # random fp32 inputs: every product is exact in fp64, only the order of the fp64 sums is free
    a, b = torch.rand(n, generator=g) + 0.1, torch.rand(n, generator=g) + 0.1
    ad, bd = a.to(dev), b.to(dev)
    L.call("pmu_dice_sums", ad.data_ptr(), bd.data_ptr(), n, out.data_ptr(), L.stream())
    torch.cuda.synchronize()
    ref = torch.stack([(a.double() * b.double()).sum(), a.double().sum(), b.double().sum()])
    e = float(((out.cpu() - ref).abs() / ref.abs()).max())
    print(f"dice_sums n={n}: {e:.3e}")
    assert e <= 1e-12, e
