"""GPU parity of the fp32 Winograd F(2x2,3x3) conv kernels (pmu_conv3x3_fwd_wino / _dgrad_wino).

Reference: the same operand (pmu_frame_to_f32 of the frame: BN+ReLU, max-pool, F.pad+cat, or the
BN+ReLU backward of dz) convolved in fp64 on the CPU.  Winograd's fp32 transforms round differently
from a direct sum: tolerance max|d| / max|ref| <= 2e-5 (the model-level bound is 1e-3).
"""
import pytest
import torch
import torch.nn.functional as TF

pytestmark = pytest.mark.gpu

TOL = 2e-5


def _rel(a, b):
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    return float((a - b).abs().max() / b.abs().max().clamp_min(1e-30))


def _to_f32(srcs, N, H, W):
    from pmu_hip import _lib as L
    from pmu_hip.engine import frame_of
    C = sum(sr.C for sr in srcs)
    out = torch.empty(N, H, W, C, device=srcs[0].x.device)
    L.call("pmu_frame_to_f32", frame_of(srcs, N, H, W), out.data_ptr(), L.stream())
    return out


def _coef(C, g, dev):
    return torch.cat([torch.rand(C, generator=g) + 0.5, torch.randn(C, generator=g) * 0.2]).to(dev)


def _frame(kind, N, H, W, C, g, dev):
    from pmu_hip import _lib as L
    from pmu_hip.engine import Src
    if kind == "raw":
        return [Src(torch.randn(N, H, W, C, generator=g).to(dev))]
    if kind == "bnrelu":
        return [Src(torch.randn(N, H, W, C, generator=g).to(dev), L.SRC_BNRELU, _coef(C, g, dev))]
    if kind == "maxpool":
        return [Src(torch.randn(N, 2 * H + 1, 2 * W, C, generator=g).to(dev), L.SRC_BNRELU, _coef(C, g, dev),
                    pool=L.POOL_MAX2)]
    if kind == "avgpool":  # AvgPool2d(2, 2, ceil_mode=True) of an odd-height map (the encoders' pooling)
        return [Src(torch.randn(N, 2 * H - 1, 2 * W, C, generator=g).to(dev), L.SRC_BNRELU, _coef(C, g, dev),
                    pool=L.POOL_AVG2CEIL)]
    if kind == "concat":
        c0 = C // 2
        z = torch.randn(N, H, W, c0, generator=g).to(dev)
        u = torch.randn(N, H - 1, W - 2, C - c0, generator=g).to(dev)
        return [Src(z, L.SRC_BNRELU, _coef(c0, g, dev)), Src(u, off=(0, 1))]
    raise ValueError(kind)


@pytest.mark.parametrize("kind,N,H,W,Cin,Cout", [("bnrelu", 2, 32, 32, 64, 64), ("raw", 1, 37, 45, 20, 40),
                                                 ("maxpool", 2, 24, 20, 64, 128), ("concat", 2, 33, 17, 128, 64),
                                                 ("bnrelu", 3, 16, 16, 512, 96), ("raw", 1, 7, 9, 6, 10),
                                                 ("avgpool", 2, 20, 24, 64, 64), ("avgpool", 1, 9, 5, 128, 32)])
def test_conv3x3_fwd_wino(dev, kind, N, H, W, Cin, Cout):
    from pmu_hip import _lib as L
    from pmu_hip.engine import frame_of, pack_weights_wino
    g = torch.Generator().manual_seed(31 + H + Cin)
    srcs = _frame(kind, N, H, W, Cin, g, dev)
    w = (torch.randn(Cout, Cin, 3, 3, generator=g) * 0.1).to(dev)
    b = torch.randn(Cout, generator=g).to(dev)
    z = torch.empty(N, H, W, Cout, device=dev)
    R = L.lib().pmu_conv3x3_tiles_wino(N, H, W)
    part = torch.empty(R, 2 * Cout, device=dev)
    tee = torch.full((N, H, W, Cin), float("nan"), device=dev) if Cin % 4 == 0 else None
    wp = pack_weights_wino(w, False)
    L.call("pmu_conv3x3_fwd_wino", frame_of(srcs, N, H, W), wp.data_ptr(), b.data_ptr(), Cout, z.data_ptr(),
           part.data_ptr(), L.ptr(tee), L.stream())
    torch.cuda.synchronize()
    op = _to_f32(srcs, N, H, W)
    if tee is not None:
        assert torch.equal(tee, op)
    ref = TF.conv2d(op.permute(0, 3, 1, 2).double().cpu(), w.double().cpu(), b.double().cpu(), padding=1)
    ref = ref.permute(0, 2, 3, 1)
    assert _rel(z, ref) <= TOL
    # BN partials: per-tile sums over the pixels sum to the channel totals
    tot = part.double().sum(0).cpu()
    scale = ref.abs().sum((0, 1, 2))
    assert float(((tot[:Cout] - ref.sum((0, 1, 2))).abs() / scale).max()) <= 1e-5
    assert float(((tot[Cout:] - (ref * ref).sum((0, 1, 2))).abs() / (ref * ref).sum((0, 1, 2))).max()) <= 1e-5


@pytest.mark.parametrize("N,H,W,Cin,Cout,split", [(2, 40, 36, 64, 64, 64), (2, 17, 33, 128, 64, 64),
                                                  (1, 16, 16, 96, 128, 32), (2, 9, 7, 12, 20, 12)])
def test_conv3x3_dgrad_wino(dev, N, H, W, Cin, Cout, split):
    from pmu_hip import _lib as L
    from pmu_hip.engine import Src, frame_of, pack_weights_wino
    g = torch.Generator().manual_seed(7 + H + Cout)
    da = torch.randn(N, H, W, Cout, generator=g).to(dev)
    z = torch.randn(N, H, W, Cout, generator=g).to(dev)
    bco = torch.cat([torch.rand(Cout, generator=g) + 0.5, torch.randn(Cout, generator=g) * 0.1,
                     torch.randn(Cout, generator=g) * 0.1, torch.randn(Cout, generator=g) * 0.01,
                     torch.randn(Cout, generator=g) * 0.01]).to(dev)
    dsrc = [Src(da, L.SRC_BNBWD, bco, z=z)]
    w = (torch.randn(Cout, Cin, 3, 3, generator=g) * 0.1).to(dev)
    wp = pack_weights_wino(w, True)
    dx0 = torch.empty(N, H, W, split, device=dev)
    dx1 = torch.empty(N, H, W, Cin - split, device=dev) if split < Cin else None
    dzt = torch.full((N, H, W, Cout), float("nan"), device=dev)
    L.call("pmu_conv3x3_dgrad_wino", frame_of(dsrc, N, H, W), wp.data_ptr(), Cin, split, dx0.data_ptr(),
           L.ptr(dx1), dzt.data_ptr(), L.stream())
    torch.cuda.synchronize()
    dz = _to_f32(dsrc, N, H, W)
    assert torch.equal(dzt, dz)
    ref = torch.nn.grad.conv2d_input((N, Cin, H, W), w.double().cpu(), dz.permute(0, 3, 1, 2).double().cpu(),
                                     padding=1).permute(0, 2, 3, 1)
    got = dx0 if dx1 is None else torch.cat([dx0, dx1], dim=3)
    assert _rel(got, ref) <= TOL


@pytest.mark.parametrize("N,H,W,Cin,Cout", [(2, 32, 32, 64, 64), (2, 17, 33, 128, 32), (3, 9, 13, 64, 96),
                                            (1, 40, 36, 192, 64)])
def test_conv3x3_wgrad_wino(dev, N, H, W, Cin, Cout):
    from pmu_hip import _lib as L
    g = torch.Generator().manual_seed(3 + H + Cin + Cout)
    x = torch.randn(N, H, W, Cin, generator=g).to(dev)
    dz = torch.randn(N, H, W, Cout, generator=g).to(dev)
    wsb = L.lib().pmu_conv3x3_wgrad_ws_wino(N, H, W, Cin, Cout)
    assert wsb > 0
    ws = torch.empty(wsb // 4, device=dev)
    dw = torch.empty(Cout, Cin, 3, 3, device=dev)
    L.call("pmu_conv3x3_wgrad_wino", dz.data_ptr(), x.data_ptr(), N, H, W, Cout, Cin, dw.data_ptr(), ws.data_ptr(),
           wsb, L.stream())
    torch.cuda.synchronize()
    ref = torch.nn.grad.conv2d_weight(x.permute(0, 3, 1, 2).double().cpu(), (Cout, Cin, 3, 3),
                                      dz.permute(0, 3, 1, 2).double().cpu(), padding=1)
    assert _rel(dw, ref) <= TOL
    assert L.lib().pmu_conv3x3_wgrad_ws_wino(N, H, W, 32, Cout) == 0  # Cin % 64 != 0: not taken


@pytest.mark.parametrize("fused", [False, True])
def test_unet_wino_matches_direct(dev, exp_lib, monkeypatch, fused):
    """The whole c2 architecture, one training step, with the Winograd kernels (default: materialised
    operands; or the fused-staging variant) and with the direct-sum kernels, both against the fp64
    CPU oracle: the Winograd gradients are as close to fp64 as the direct ones (within 2x of the
    direct path's own error, which is BN-amplified fp32 rounding at batch 2), outputs within 1e-4."""
    from helpers import grad_err
    from model import UNet
    from oracle.unet_ref import unet_forward, unet_loss, unet_param_keys
    torch.manual_seed(0)
    net = UNet(1, 1, [64, 128, 256, 512, 1024])
    sd0 = {k: v.clone() for k, v in net.state_dict().items()}
    g = torch.Generator().manual_seed(4)
    x = torch.rand(2, 1, 48, 64, generator=g)
    target = (torch.rand(2, 1, 48, 64, generator=g) > 0.5).float()
    keys = unet_param_keys(sd0)
    sd = {k: (v.double() if v.is_floating_point() else v.clone()) for k, v in sd0.items()}
    params = {k: sd[k].clone().requires_grad_(True) for k in keys}
    work = dict(sd)
    work.update(params)
    unet_loss(unet_forward(work, x.double(), 5, 1), target.double(), 1).backward()
    g64 = {k: params[k].grad for k in keys}

    net = net.to(dev).train()
    xd, td = x.to(dev), target.to(dev)

    def step(mode):
        from pmu_hip import engine
        monkeypatch.setattr(engine.CFG, "fp32_conv", mode)
        net.load_state_dict(sd0)
        for p in net.parameters():
            p.grad = None
        out = net(xd)
        torch.nn.functional.binary_cross_entropy(out, td).backward()
        torch.cuda.synchronize()
        return out.detach().clone(), {n: p.grad.detach().cpu().double() for n, p in net.named_parameters()}

    o_d, g_d = step("direct")
    o_w, g_w = step("wino_fused" if fused else "wino")
    assert _rel(o_w, o_d) <= 1e-4
    e_d, _ = grad_err(g_d, g64)
    e_w, k_w = grad_err(g_w, g64)
    assert e_w <= max(2 * e_d, 1e-4), (e_w, e_d, k_w)
