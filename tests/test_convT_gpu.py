"""ConvTranspose2d(k2, s2) of Up (PMU/model/unet/unet_parts.py:41-67) on the pipelined fp32 kernels,
against a float64 CPU reference: the forward with the producer's BN+ReLU applied while staging
(pmu_convT2x2_fwd), and the input gradient (pmu_convT2x2_dgrad) and the weight/bias gradient (pmu_convT2x2_wgrad).  Power-of-two maps take the
shift/mask epilogue, the odd ones the division epilogue; M = N*H*W is not a multiple of the
128-row tile in the odd cases."""
import os
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "probabilistic-multiplanar-unet_amd"))

TOL = 2e-5   # fp32 MFMA sums vs float64, relative to the output's max magnitude


@pytest.mark.gpu
@pytest.mark.parametrize("N,H,W,Cin,Cout", [(2, 16, 16, 128, 64), (3, 13, 10, 128, 64), (1, 8, 32, 256, 128),
                                            (2, 7, 9, 64, 32)])
def test_convT_fwd_dgrad_match_float64(dev, N, H, W, Cin, Cout):
    from pmu_hip import _lib as L
    from pmu_hip.engine import Src, frame_of, pack_convT_weights
    g = torch.Generator().manual_seed(N * 1000 + H * 10 + W)
    z = torch.randn(N, H, W, Cin, generator=g)
    sc, sh = torch.rand(Cin, generator=g) + 0.5, torch.randn(Cin, generator=g) * 0.2
    w = torch.randn(Cin, Cout, 2, 2, generator=g) * 0.05
    b = torch.randn(Cout, generator=g) * 0.1
    du = torch.randn(N, 2 * H, 2 * W, Cout, generator=g)
    # float64 reference
    act = torch.relu(z.double() * sc.double() + sh.double()).permute(0, 3, 1, 2)
    ref = torch.nn.functional.conv_transpose2d(act, w.double(), b.double(), stride=2).permute(0, 2, 3, 1)
    a = act.clone().requires_grad_(True)
    wr = w.double().requires_grad_(True)
    br = b.double().requires_grad_(True)
    torch.nn.functional.conv_transpose2d(a, wr, br, stride=2).backward(du.double().permute(0, 3, 1, 2))
    ref_dx = a.grad.permute(0, 2, 3, 1)
    # HIP
    zd, wd, bd, dud = z.to(dev), w.to(dev), b.to(dev), du.to(dev)
    coef = torch.cat([sc, sh]).to(dev)
    u = torch.empty(N, 2 * H, 2 * W, Cout, device=dev)
    dx = torch.empty(N, H, W, Cin, device=dev)
    s = L.stream()
    L.call("pmu_convT2x2_fwd", frame_of([Src(zd, L.SRC_BNRELU, coef)], N, H, W), wd.data_ptr(),
           pack_convT_weights(wd, False).data_ptr(), bd.data_ptr(), Cout, u.data_ptr(), s)
    L.call("pmu_convT2x2_dgrad", dud.data_ptr(), 2 * H, 2 * W, 0, 0, wd.data_ptr(),
           pack_convT_weights(wd, True).data_ptr(), N, H, W, Cin, Cout, dx.data_ptr(), s)
    dw = torch.empty_like(wd)
    db = torch.empty(Cout, device=dev)
    wsb = L.lib().pmu_convT2x2_wgrad_ws(N, H, W, Cin, Cout)
    ws = torch.empty(max(1, (wsb + 3) // 4), device=dev)
    L.call("pmu_convT2x2_wgrad", dud.data_ptr(), 2 * H, 2 * W, 0, 0, frame_of([Src(zd, L.SRC_BNRELU, coef)], N, H, W),
           Cout, dw.data_ptr(), db.data_ptr(), ws.data_ptr(), wsb, s)
    torch.cuda.synchronize()
    e_w = ((dw.cpu().double() - wr.grad).abs().max() / wr.grad.abs().max()).item()
    e_b = ((db.cpu().double() - br.grad).abs().max() / br.grad.abs().max()).item()
    assert e_w <= TOL and e_b <= TOL, (e_w, e_b)
    e_u = ((u.cpu().double() - ref).abs().max() / ref.abs().max()).item()
    e_dx = ((dx.cpu().double() - ref_dx).abs().max() / ref_dx.abs().max()).item()
    assert e_u <= TOL and e_dx <= TOL, (e_u, e_dx)


@pytest.mark.gpu
@pytest.mark.parametrize("N,H,W,Cin,Cup,Cskip", [(2, 16, 16, 128, 64, 64), (1, 8, 32, 256, 128, 128),
                                                  (1, 7, 9, 128, 64, 64)])  # odd pixel count (pair stores)
def test_concat_operand_built_in_place(dev, N, H, W, Cin, Cup, Cskip):
    """The Up block's concat operand written in place (unet_parts.py:52,66): pmu_convT2x2_fwd_ld /
    pmu_convT2x2_fwd_dma_ldb fill channels [Cskip, Cskip + Cup) and pmu_frame_to_f32_ld /
    pmu_frame_to_bf16_ld channels [0, Cskip) of one tensor — bit-equal to materialising the two-source
    frame (skip activation, convT output) with pmu_frame_to_f32 / pmu_frame_to_bf16."""
    from pmu_hip import _lib as L
    from pmu_hip.engine import (BF16S, Src, frame_of, frame_to_bf16, frame_to_f32, pack_convT_weights,
                                pack_convT_weights_dma)
    g = torch.Generator().manual_seed(H * 7 + Cin)
    z = torch.randn(N, H, W, Cin, generator=g).to(dev)
    coef = torch.cat([torch.rand(Cin, generator=g) + 0.5, torch.randn(Cin, generator=g) * 0.2]).to(dev)
    zs = torch.randn(N, 2 * H, 2 * W, Cskip, generator=g).to(dev)
    cs = torch.cat([torch.rand(Cskip, generator=g) + 0.5, torch.randn(Cskip, generator=g) * 0.2]).to(dev)
    w = (torch.randn(Cin, Cup, 2, 2, generator=g) * 0.05).to(dev)
    b = (torch.randn(Cup, generator=g) * 0.1).to(dev)
    Ho, Wo, Cc = 2 * H, 2 * W, Cskip + Cup
    act, skip = Src(z, L.SRC_BNRELU, coef), Src(zs, L.SRC_BNRELU, cs)
    s = L.stream()
    # fp32
    fin = frame_of([act], N, H, W)
    assert L.lib().pmu_convT2x2_fwd_ld_ok(fin, Cup)
    wp = pack_convT_weights(w, dgrad=False)
    u = torch.empty(N, Ho, Wo, Cup, device=dev)
    L.call("pmu_convT2x2_fwd", fin, w.data_ptr(), wp.data_ptr(), b.data_ptr(), Cup, u.data_ptr(), s)
    ref = frame_to_f32([skip, Src(u)], N, Ho, Wo)
    xcat = torch.full((N, Ho, Wo, Cc), float("nan"), device=dev)
    L.call("pmu_convT2x2_fwd_ld", fin, w.data_ptr(), wp.data_ptr(), b.data_ptr(), Cup, xcat.data_ptr() + 4 * Cskip,
           Cc, s)
    L.call("pmu_frame_to_f32_ld", frame_of([skip], N, Ho, Wo), xcat.data_ptr(), Cc, s)
    # bf16
    xt = frame_to_bf16([act], N, H, W)
    wpd = pack_convT_weights_dma(w, dgrad=False)
    ub = torch.empty(N, Ho, Wo, Cup, device=dev)
    L.call("pmu_convT2x2_fwd_dma", xt.data_ptr(), xt.shape[3], N, H, W, wpd.data_ptr(), b.data_ptr(), Cin, Cup,
           ub.data_ptr(), s)
    refb = frame_to_bf16([skip, Src(ub)], N, Ho, Wo)
    xcatb = torch.full((N, Ho, Wo, Cc), -1, dtype=BF16S, device=dev)
    L.call("pmu_convT2x2_fwd_dma_ldb", xt.data_ptr(), xt.shape[3], N, H, W, wpd.data_ptr(), b.data_ptr(), Cin, Cup,
           xcatb.data_ptr() + 2 * Cskip, Cc, s)
    L.call("pmu_frame_to_bf16_ld", frame_of([skip], N, Ho, Wo), Cskip, xcatb.data_ptr(), Cc, s)
    torch.cuda.synchronize()
    assert torch.equal(xcat, ref)
    assert torch.equal(xcatb, refb)


# ---------------------------------------------------------------------------------------------------
# The generic GEMM / generic weight-gradient kernels (channel counts or frames the pipelined kernels do
# not take, or wp == NULL) and the F.pad placement (off_h, off_w) of an odd-sized skip, against the same
# float64 reference and bound.  Which kernel runs is csrc/convT.hip's host dispatch, restated per case.
# ---------------------------------------------------------------------------------------------------
def _rel(got, ref):
    return ((got.double().cpu() - ref).abs().max() / ref.abs().max()).item()


def _convT_ref(act, w, b, du_win):
    """float64: (u, dx, dw, db) of conv_transpose2d(act, w, b, stride 2) with upstream gradient du_win; act
    and du_win NHWC float64, the results NHWC / PyTorch's weight layout."""
    a = act.permute(0, 3, 1, 2).clone().requires_grad_(True)
    wr = w.double().requires_grad_(True)
    br = b.double().requires_grad_(True)
    u = torch.nn.functional.conv_transpose2d(a, wr, br, stride=2)
    u.backward(du_win.permute(0, 3, 1, 2))
    return u.detach().permute(0, 2, 3, 1), a.grad.permute(0, 2, 3, 1), wr.grad, br.grad


def _fwd_case(kind, N, H, W, Cin, g):
    """(sources as dicts of CPU tensors, use packed weights?) of a forward case."""
    from helpers import POOL_MAX2, SRC_BNRELU, SRC_RAW, quant_bn, quant_z
    if kind == "raw":
        return [dict(x=torch.randn(N, H, W, Cin, generator=g), mode=SRC_RAW)], True
    if kind == "max":
        return [dict(x=quant_z(N, 2 * H + 1, 2 * W, Cin, g), mode=SRC_BNRELU, coef=quant_bn(Cin, g), pool=POOL_MAX2)], True
    return [dict(x=quant_z(N, H, W, Cin, g), mode=SRC_BNRELU, coef=quant_bn(Cin, g))], kind == "packed"


def _dev_srcs(srcs, dev):
    from pmu_hip.engine import Src
    return [Src(**{k: (v.to(dev) if torch.is_tensor(v) else v) for k, v in d.items()}) for d in srcs]


@pytest.mark.gpu
@pytest.mark.parametrize("N,H,W,Cin,Cout,kind", [
    (2, 7, 9, 24, 12, "wp_none"),    # wp == NULL; Cin % 16 != 0 as well
    (1, 5, 3, 6, 5, "packed"),       # channel counts not multiples of 4 (scalar frame_value / du loads)
    (2, 6, 5, 64, 32, "wp_none"),    # a pipelined shape forced down the generic GEMM by wp == NULL
    (2, 6, 5, 64, 32, "raw"),        # pipelined channel counts and wp given, but a RAW source
    (2, 6, 5, 64, 32, "max"),        # ... and a POOL_MAX2 BN+ReLU source (odd source height)
])
def test_convT_fwd_generic_gemm_vs_float64(dev, N, H, W, Cin, Cout, kind):
    from helpers import ref_frame
    from pmu_hip import _lib as L
    from pmu_hip.engine import Src, frame_of, pack_convT_weights
    g = torch.Generator().manual_seed(N * 1000 + H * 10 + W + Cin)
    srcs, use_wp = _fwd_case(kind, N, H, W, Cin, g)
    w = torch.randn(Cin, Cout, 2, 2, generator=g) * 0.05
    b = torch.randn(Cout, generator=g) * 0.1
    act = ref_frame([Src(**d) for d in srcs], N, H, W)
    ref = _convT_ref(act, w, b, torch.zeros(N, 2 * H, 2 * W, Cout, dtype=torch.float64))[0]
    wd, bd = w.to(dev), b.to(dev)
    sd = _dev_srcs(srcs, dev)
    u = torch.full((N, 2 * H, 2 * W, Cout), float("nan"), device=dev)
    wp = pack_convT_weights(wd, False).data_ptr() if use_wp else None
    L.call("pmu_convT2x2_fwd", frame_of(sd, N, H, W), wd.data_ptr(), wp, bd.data_ptr(), Cout, u.data_ptr(), L.stream())
    torch.cuda.synchronize()
    assert not torch.isnan(u).any()
    e = _rel(u, ref)
    print(f"convT fwd generic {kind} {(N, H, W, Cin, Cout)}: {e:.3e}")
    assert e <= TOL, e
    if kind == "wp_none" and Cin == 64:   # the pipelined kernel on the same operands
        up = torch.empty_like(u)
        L.call("pmu_convT2x2_fwd", frame_of(sd, N, H, W), wd.data_ptr(), pack_convT_weights(wd, False).data_ptr(),
               bd.data_ptr(), Cout, up.data_ptr(), L.stream())
        torch.cuda.synchronize()
        assert _rel(up, ref) <= TOL
        assert float((up - u).abs().max() / u.abs().max()) <= 2e-5


OFFSETS = [(1, 0), (0, 2)]   # du is (2H + 1) x (2W + 2): both placements fit, neither fills it


def _placed_du(N, H, W, Cout, off, g):
    """du [N][2H+1][2W+2][Cout] with 1e3 outside the convT output's window at off, and the window (float64)."""
    du = torch.full((N, 2 * H + 1, 2 * W + 2, Cout), 1e3)
    win = torch.randn(N, 2 * H, 2 * W, Cout, generator=g)
    du[:, off[0]:off[0] + 2 * H, off[1]:off[1] + 2 * W] = win
    return du, win.double()


@pytest.mark.gpu
@pytest.mark.parametrize("off", OFFSETS)
@pytest.mark.parametrize("Cin,Cout,packed", [(128, 32, True),    # pipelined: wp, Cout % 16 == 0, Cin % 128 == 0
                                             (24, 12, False)])   # generic GEMM
def test_convT_dgrad_placement_vs_float64(dev, Cin, Cout, packed, off):
    from pmu_hip import _lib as L
    from pmu_hip.engine import pack_convT_weights
    N, H, W = 2, 6, 5
    g = torch.Generator().manual_seed(Cin + 7 * off[0] + off[1])
    w = torch.randn(Cin, Cout, 2, 2, generator=g) * 0.05
    du, win = _placed_du(N, H, W, Cout, off, g)
    ref = _convT_ref(torch.zeros(N, H, W, Cin, dtype=torch.float64), w, torch.zeros(Cout), win)[1]
    wd, dud = w.to(dev), du.to(dev)
    dx = torch.full((N, H, W, Cin), float("nan"), device=dev)
    wp = pack_convT_weights(wd, True).data_ptr() if packed else None
    L.call("pmu_convT2x2_dgrad", dud.data_ptr(), 2 * H + 1, 2 * W + 2, off[0], off[1], wd.data_ptr(), wp, N, H, W, Cin,
           Cout, dx.data_ptr(), L.stream())
    torch.cuda.synchronize()
    assert not torch.isnan(dx).any()
    e = _rel(dx, ref)
    print(f"convT dgrad {'pipelined' if packed else 'generic'} {(Cin, Cout)} off {off}: {e:.3e}")
    assert e <= TOL, e


def _convT_wgrad(dev, N, H, W, Cin, Cout, off, Hd, Wd, g, du, win):
    """Runs pmu_convT2x2_wgrad with and without dbias (dw, the workspace and dbias start as NaN); returns
    the errors of dw and dbias against float64."""
    from helpers import SRC_BNRELU, quant_bn, quant_z, ref_frame
    from pmu_hip import _lib as L
    from pmu_hip.engine import Src, frame_of
    src = dict(x=quant_z(N, H, W, Cin, g), mode=SRC_BNRELU, coef=quant_bn(Cin, g))
    act = ref_frame([Src(**src)], N, H, W)
    _, _, ref_w, ref_b = _convT_ref(act, torch.zeros(Cin, Cout, 2, 2), torch.zeros(Cout), win)
    sd = _dev_srcs([src], dev)
    dud = du.to(dev)
    wsb = L.lib().pmu_convT2x2_wgrad_ws(N, H, W, Cin, Cout)
    out = []
    for with_bias in (True, False):
        ws = torch.full((max(1, (wsb + 3) // 4),), float("nan"), device=dev)
        dw = torch.full((Cin, Cout, 2, 2), float("nan"), device=dev)
        db = torch.full((Cout,), float("nan"), device=dev)
        L.call("pmu_convT2x2_wgrad", dud.data_ptr(), Hd, Wd, off[0], off[1], frame_of(sd, N, H, W), Cout,
               dw.data_ptr(), db.data_ptr() if with_bias else None, ws.data_ptr(), wsb, L.stream())
        torch.cuda.synchronize()
        assert not torch.isnan(dw).any()
        out.append((dw, db))
    assert not torch.isnan(out[0][1]).any()
    assert torch.equal(out[0][0], out[1][0])        # dbias == NULL: the same dw, bit for bit
    assert torch.isnan(out[1][1]).all()             # ... and nothing written through a bias pointer
    return _rel(out[0][0], ref_w), _rel(out[0][1], ref_b)


@pytest.mark.gpu
@pytest.mark.parametrize("off", OFFSETS)
@pytest.mark.parametrize("Cin,Cout", [(64, 64),             # pipelined (Cin % 64 == Cout % 64 == 0, plain BN+ReLU source)
                                      (24, 12), (6, 5)])    # generic; (6, 5): scalar du loads
def test_convT_wgrad_placement_vs_float64(dev, Cin, Cout, off):
    N, H, W = 2, 6, 5
    g = torch.Generator().manual_seed(Cin * 3 + 7 * off[0] + off[1])
    du, win = _placed_du(N, H, W, Cout, off, g)
    e_w, e_b = _convT_wgrad(dev, N, H, W, Cin, Cout, off, 2 * H + 1, 2 * W + 2, g, du, win)
    print(f"convT wgrad {(Cin, Cout)} off {off}: dw {e_w:.3e} dbias {e_b:.3e}")
    assert e_w <= TOL and e_b <= TOL, (e_w, e_b)


@pytest.mark.gpu
@pytest.mark.parametrize("N,H,W,Cin,Cout", [(3, 9, 4, 64, 64), (3, 9, 3, 24, 12)])
def test_convT_wgrad_narrow_map_vs_float64(dev, N, H, W, Cin, Cout):
    """W <= 4: convT_wgrad_geometry's 4-wide (8 x 4 pixel) tile, on the pipelined and the generic kernel."""
    g = torch.Generator().manual_seed(H * W + Cin)
    win = torch.randn(N, 2 * H, 2 * W, Cout, generator=g)
    e_w, e_b = _convT_wgrad(dev, N, H, W, Cin, Cout, (0, 0), 2 * H, 2 * W, g, win, win.double())
    print(f"convT wgrad narrow {(N, H, W, Cin, Cout)}: dw {e_w:.3e} dbias {e_b:.3e}")
    assert e_w <= TOL and e_b <= TOL, (e_w, e_b)
