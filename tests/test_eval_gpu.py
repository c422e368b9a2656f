"""GPU parity of the inference path: model.UNet in eval mode (BN running statistics, every forward
kernel without its BN partial sums) in fp32 and under torch.autocast(bfloat16), against the CPU oracle
on a calibrated state (helpers.calibrated_eval_state) — outputs, features, label maps by location,
buffers untouched, the entries launched; the forward entries called directly with and without their
optional outputs; eval mode with autograd on (frozen BatchNorm's backward); predict_volume's stacks.

Tolerances: fp32 ACT_TOL against the oracle in fp32 (itself within 2e-6 of its fp64 evaluation here),
GRAD_TOL against the oracle's autograd in fp64.  bf16: the project's rule
(tests/test_bf16_gpu.py _c5_step_vs_oracle) — the reference is the oracle's bf16 arithmetic evaluated
in fp64, the tolerance max(ACT_TOL, 2 x floor), floor the distance between the oracle's fp32 and fp64
evaluations of that arithmetic (bf16 rounding turns last-bit fp32 differences into operand flips),
measured on the spot.
"""
import os

import numpy as np
import pytest
import torch

from helpers import ACT_TOL, GRAD_TOL, calibrated_eval_state, dice_bounds, grad_err, max_abs

pytestmark = pytest.mark.gpu

# id -> (filters, Cin, K, N, H, W)
CASES = {
    "E1": ([64, 128, 256, 512, 1024], 3, 3, 2, 64, 48),   # full depth, 3-pixel-wide deepest maps, MFMA first layer
    "E2": ([64, 128, 256, 512, 1024], 3, 3, 2, 37, 45),   # odd sizes: F.pad in every Up block
    "E3": ([64, 128, 256], 3, 3, 2, 96, 80),              # two LDS-DMA levels, in-place concat, pool+skip pass
    "E4": ([64, 128, 256], 3, 3, 3, 90, 70),              # one Up block padded and one in place; N = 3
    "E5": ([64, 128], 1, 1, 2, 40, 72),                   # sigmoid head, one input plane
    "E6": ([16, 32, 64], 3, 3, 2, 64, 64),                # narrow channels
    "E7": ([6, 12, 24], 1, 3, 2, 40, 36),                 # channel counts off every fast path (fp32 only)
    "E8": ([32, 64, 128], 3, 3, 2, 37, 45),               # first layer Cin = 3, Cout = 32 (MT = 2)
}
FWD_PARAMS = [(c, b) for c in CASES for b in (False, True) if not (c == "E7" and b)]
_IDS = [f"{c}-{'bf16' if b else 'fp32'}" for c, b in FWD_PARAMS]
REQUIRED = {"pmu_bn_eval_coef", "pmu_conv_first_fwd", "pmu_head1x1_fwd", "pmu_conv3x3_fwd_wino2h",
            "pmu_conv3x3_fwd_wino", "pmu_conv3x3_fwd_dma", "pmu_conv3x3_fwd_raw", "pmu_convT2x2_fwd",
            "pmu_convT2x2_fwd_ld", "pmu_convT2x2_fwd_dma", "pmu_convT2x2_fwd_dma_ldb"}
_SEEN = set()     # entries launched by test_unet_eval_forward_vs_oracle over all its cases
_RAN = set()      # its cases that ran
_ORACLE = {}      # (case, bf16, last) -> (ref, floor)
_HIP_OUT = {}     # (case, bf16) -> the no_grad output of the HIP net (CPU copy)


def _say(capsys, msg):
    with capsys.disabled():
        print(msg, flush=True)


def _dbl(sd):
    return {k: (v.double() if v.is_floating_point() else v) for k, v in sd.items()}


def _oracle(cid, bf16, last=True):
    """(reference, floor): fp32 — the oracle in fp32, floor None; bf16 — the oracle's bf16 arithmetic in
    fp64 and its distance to the same arithmetic in fp32."""
    key = (cid, bf16, last)
    if key not in _ORACLE:
        from oracle.unet_ref import unet_forward
        f, C, K, N, H, W = CASES[cid]
        sd, x, _ = calibrated_eval_state(f, C, K, N, H, W)
        torch.set_num_threads(min(16, os.cpu_count() or 1))
        with torch.no_grad():
            o32 = unet_forward(dict(sd), x, len(f), K, apply_last_layer=last, training=False, bf16=bf16)
            if bf16:
                ref = unet_forward(_dbl(sd), x.double(), len(f), K, apply_last_layer=last, training=False, bf16=True)
                _ORACLE[key] = (ref, max_abs(o32, ref))
            else:
                _ORACLE[key] = (o32, None)
    return _ORACLE[key]


def _net(cid, dev, sd=None):
    from model import UNet
    f, C, K, N, H, W = CASES[cid]
    if sd is None:
        sd = calibrated_eval_state(f, C, K, N, H, W)[0]
    net = UNet(C, K, list(f))
    net.load_state_dict(sd)
    return net.to(dev).eval()


def _buffers(net):
    return {k: v.detach().clone() for k, v in net.named_buffers()}


def _assert_buffers_unchanged(net, before):
    after = dict(net.named_buffers())
    assert len(before) >= 3 and set(before) == set(after)
    for k, v in before.items():
        assert torch.equal(v, after[k]), f"eval mode wrote {k}"


def _forward(net, x, bf16):
    with torch.autocast("cuda", dtype=torch.bfloat16, enabled=bf16):
        return net(x)


def _margin(ref, K):
    if K == 1:
        return (ref - 0.5).abs()[:, 0]
    top = ref.topk(2, dim=1).values
    return top[:, 0] - top[:, 1]


def _labels(y, K):
    return (y[:, 0] > 0.5).long() if K == 1 else y.argmax(1)


@pytest.mark.parametrize("cid,bf16", FWD_PARAMS, ids=_IDS)
def test_unet_eval_forward_vs_oracle(cid, bf16, dev, capsys):
    from pmu_hip import _lib as L
    f, C, K, N, H, W = CASES[cid]
    _, x, _ = calibrated_eval_state(f, C, K, N, H, W)
    ref, floor = _oracle(cid, bf16)
    feat_ref, feat_floor = _oracle(cid, bf16, last=False)
    tol = max(ACT_TOL, 2 * floor) if bf16 else ACT_TOL
    feat_tol = max(ACT_TOL, 2 * feat_floor) if bf16 else ACT_TOL

    # conditions on the reference alone, so that the tolerance means something
    mg = _margin(ref, K)
    near = mg <= 2 * tol
    lab_ref = _labels(ref, K)
    if K == 1:
        assert float(ref.min()) < 0.1 and float(ref.max()) > 0.9
    else:
        assert float(ref.abs().max()) >= 1.0
        shares = [float((lab_ref == k).float().mean()) for k in range(K)]
        assert min(shares) >= 0.01, shares
    assert float(near.float().mean()) <= 0.05

    net = _net(cid, dev)
    before = _buffers(net)
    xd = x.to(dev)
    names = []
    L.set_call_observer(lambda name, args, e0, e1: names.append(name))
    try:
        with torch.no_grad():
            out = _forward(net, xd, bf16)
            net.apply_last_layer = False
            feat = _forward(net, xd, bf16)
        torch.cuda.synchronize()
    finally:
        L.set_call_observer(None)
        net.apply_last_layer = True
    _SEEN.update(names)
    _RAN.add((cid, bf16))
    _HIP_OUT[(cid, bf16)] = out.cpu()
    assert out.dtype == torch.float32 and out.shape == ref.shape and feat.shape == feat_ref.shape
    err, feat_err = max_abs(out, ref), max_abs(feat, feat_ref)
    lab = _labels(out.cpu(), K)
    flips = lab != lab_ref
    _say(capsys, f"EVAL_FWD {cid} {'bf16' if bf16 else 'fp32'}: out err {err:.3e} (tol {tol:.3e}, floor "
         f"{floor if floor is None else format(floor, '.3e')}) feat err {feat_err:.3e} (tol {feat_tol:.3e}) "
         f"max|ref| {float(ref.abs().max()):.2f} near-tie share {float(near.float().mean()):.4f} "
         f"flipped labels {int(flips.sum())}")
    assert err <= tol, (err, tol)
    assert feat_err <= feat_tol, (feat_err, feat_tol)
    # by location: a label differs from the reference's only inside the near-tie zone
    assert not bool((flips & ~near).any()), float(mg[flips].max())
    _assert_buffers_unchanged(net, before)
    assert "pmu_bn_fwd_finalize" not in names and "pmu_colsum_f64" not in names


def test_unet_eval_forward_entry_coverage():
    """Over all the cases above, eval mode reached every forward entry of the default dispatch."""
    if _RAN != set(FWD_PARAMS):
        pytest.skip("needs every case of test_unet_eval_forward_vs_oracle in the same session")
    missing = REQUIRED - _SEEN
    assert not missing, sorted(missing)
    assert any(n.startswith("pmu_frame_to_") and n.endswith("_pool_skip") for n in _SEEN), sorted(_SEEN)


# ----------------------------------------------------------------------------------------
# forward entries called directly: the BN partial sums and the operand tee are optional outputs
# ----------------------------------------------------------------------------------------
def _wb(Cout, Cin, g, dev):
    return (torch.randn(Cout, Cin, 3, 3, generator=g) * 0.1).to(dev), torch.randn(Cout, generator=g).to(dev)


def _bn_src(N, H, W, C, g, dev):
    from pmu_hip import _lib as L
    from pmu_hip.engine import Src
    coef = torch.cat([torch.rand(C, generator=g) + 0.5, torch.randn(C, generator=g) * 0.2]).to(dev)
    return Src(torch.randn(N, H, W, C, generator=g).to(dev), L.SRC_BNRELU, coef)


def _variants(run, has_tee):
    """run(part: bool, tee: bool) -> (z, tee or None) for every null / non-null combination: every z is
    bit-equal to the one computed with all outputs, and so is every tee."""
    z0, t0 = run(True, has_tee)
    assert not torch.isnan(z0).any()
    combos = [(False, has_tee)] + ([(True, False), (False, False)] if has_tee else [])
    for with_part, with_tee in combos:
        z, t = run(with_part, with_tee)
        assert torch.equal(z, z0), (with_part, with_tee)
        if with_tee:
            assert torch.equal(t, t0), (with_part, with_tee)


def test_forward_entries_with_null_part(dev):
    """In eval mode the engine passes part == NULL to every forward entry (conv_bn_forward: need_stats
    false), and a forward no backward follows passes tee / xt == NULL: z must not depend on either."""
    import ctypes
    from pmu_hip import _lib as L
    from pmu_hip.engine import (Src, frame_of, frame_to_bf16, pack_weights_bf16, pack_weights_dma, pack_weights_raw,
                                pack_weights_wino, pack_weights_wino2h)
    lb, s = L.lib(), L.stream
    g = torch.Generator().manual_seed(77)

    def outputs(N, H, W, Cout, R, with_part):
        z = torch.full((N, H, W, Cout), float("nan"), device=dev)
        part = torch.full((R, 2 * Cout), float("nan"), device=dev) if with_part else None
        return z, part

    # F(2x2), 1024-thread workgroups, materialised operand
    N, H, W, Cin, Cout = 1, 37, 45, 16, 40
    x = torch.randn(N, H, W, Cin, generator=g).to(dev)
    w, b = _wb(Cout, Cin, g, dev)
    wp = pack_weights_wino2h(w, False)

    def wino2h(with_part, _):
        z, part = outputs(N, H, W, Cout, lb.pmu_conv3x3_tiles_wino2h(N, H, W), with_part)
        L.call("pmu_conv3x3_fwd_wino2h", x.data_ptr(), Cin, N, H, W, wp.data_ptr(), b.data_ptr(), Cout, z.data_ptr(),
               L.ptr(part), s())
        return z, None
    _variants(wino2h, False)

    # F(2x2), the fused frame operand: BN+ReLU skip next to a shifted, smaller raw map (F.pad + cat)
    N, H, W, Cin, Cout = 2, 33, 17, 128, 64
    c0 = Cin // 2
    srcs = [_bn_src(N, H, W, c0, g, dev), Src(torch.randn(N, H - 1, W - 2, Cin - c0, generator=g).to(dev), off=(0, 1))]
    w, b = _wb(Cout, Cin, g, dev)
    wpw = pack_weights_wino(w, False)

    def wino(with_part, with_tee):
        z, part = outputs(N, H, W, Cout, lb.pmu_conv3x3_tiles_wino(N, H, W), with_part)
        tee = torch.full((N, H, W, Cin), float("nan"), device=dev) if with_tee else None
        L.call("pmu_conv3x3_fwd_wino", frame_of(srcs, N, H, W), wpw.data_ptr(), b.data_ptr(), Cout, z.data_ptr(),
               L.ptr(part), L.ptr(tee), s())
        return z, tee
    _variants(wino, True)

    # bf16, both operands by LDS-DMA
    N, H, W, Cin, Cout = 1, 33, 45, 128, 96
    xt = frame_to_bf16([_bn_src(N, H, W, Cin, g, dev)], N, H, W)
    assert lb.pmu_conv3x3_dma_ok(H, W, xt.shape[3], Cout, Cout) == 1
    w, b = _wb(Cout, Cin, g, dev)
    wpd = pack_weights_dma(w, False)

    def dma(with_part, _):
        z, part = outputs(N, H, W, Cout, lb.pmu_conv3x3_tiles_dma(N, H, W, Cout, xt.shape[3]), with_part)
        L.call("pmu_conv3x3_fwd_dma", xt.data_ptr(), xt.shape[3], N, H, W, wpd.data_ptr(), b.data_ptr(), Cout,
               z.data_ptr(), L.ptr(part), s())
        return z, None
    _variants(dma, False)

    # bf16 on the materialised operand
    N, H, W, Cin, Cout = 1, 33, 17, 40, 64
    xr = frame_to_bf16([_bn_src(N, H, W, Cin, g, dev)], N, H, W)
    w, b = _wb(Cout, Cin, g, dev)
    wpr = pack_weights_raw(w, False)

    def raw(with_part, _):
        z, part = outputs(N, H, W, Cout, lb.pmu_conv3x3_tiles_raw(N, H, W, Cout), with_part)
        L.call("pmu_conv3x3_fwd_raw", xr.data_ptr(), xr.shape[3], N, H, W, wpr.data_ptr(), b.data_ptr(), Cout,
               z.data_ptr(), L.ptr(part), s())
        return z, None
    _variants(raw, False)

    # bf16, the operand frame staged inside the kernel: the scalar-staging kernel (6 channels, a 7-wide map)
    # and the software-pipelined one (32-channel chunks)
    for N, H, W, Cin, Cout in ((2, 9, 7, 6, 10), (2, 40, 40, 32, 96)):
        xs = [Src(torch.randn(N, H, W, Cin, generator=g).to(dev))]
        w, b = _wb(Cout, Cin, g, dev)
        wpb = pack_weights_bf16(w, False)
        Cp = (Cin + 7) // 8 * 8

        def fused(with_part, with_tee):
            z, part = outputs(N, H, W, Cout, lb.pmu_conv3x3_tiles(N, H, W), with_part)
            tee = torch.zeros(N, H, W, Cp, dtype=torch.int16, device=dev) if with_tee else None
            L.call("pmu_conv3x3_fwd_bf16", frame_of(xs, N, H, W), wpb.data_ptr(), b.data_ptr(), Cout, z.data_ptr(),
                   L.ptr(part), L.ptr(tee), s())
            return z, tee
        _variants(fused, True)

    # first layer: NCHW planes, Cin = 3, Cout = 32
    N, Cin, H, W, Cout = 2, 3, 37, 45, 32
    xp = torch.randn(N, Cin, H, W, generator=g)
    planes = [xp[:, c].contiguous().to(dev) for c in range(Cin)]
    arr = (ctypes.c_void_p * Cin)(*[p.data_ptr() for p in planes])
    w, b = _wb(Cout, Cin, g, dev)

    def first(with_part, _):
        z, part = outputs(N, H, W, Cout, lb.pmu_conv_first_tiles(N, H, W), with_part)
        L.call("pmu_conv_first_fwd", arr, Cin, N, H, W, w.data_ptr(), b.data_ptr(), Cout, z.data_ptr(), L.ptr(part), s())
        return z, None
    _variants(first, False)
    torch.cuda.synchronize()


# ----------------------------------------------------------------------------------------
# eval mode with autograd on: frozen BatchNorm's backward
# ----------------------------------------------------------------------------------------
def _oracle_grads(cid, bf16, dt):
    from oracle.unet_ref import unet_forward, unet_loss, unet_param_keys
    f, C, K, N, H, W = CASES[cid]
    sd, x, t = calibrated_eval_state(f, C, K, N, H, W)
    sd = {k: (v.to(dt) if v.is_floating_point() else v) for k, v in sd.items()}
    keys = unet_param_keys(sd)
    params = {k: sd[k].clone().requires_grad_(True) for k in keys}
    work = dict(sd)
    work.update(params)
    out = unet_forward(work, x.to(dt), len(f), K, training=False, bf16=bf16)
    unet_loss(out, t.to(dt) if K == 1 else t, K).backward()
    return {k: params[k].grad for k in keys}


@pytest.mark.parametrize("cid,bf16", [("E3", False), ("E7", False), ("E3", True)], ids=["E3-fp32", "E7-fp32", "E3-bf16"])
def test_unet_eval_mode_with_autograd(cid, bf16, dev, capsys):
    """net.eval() with grad enabled: the output is the no_grad output bit for bit (keep=True with eval),
    the parameter gradients are the oracle's autograd through its eval-mode forward (the running
    statistics are constants: dz = scale g, dgamma = sum g xhat_running, dbeta = sum g), and no buffer
    is written."""
    from oracle.unet_ref import unet_loss, unet_param_keys
    f, C, K, N, H, W = CASES[cid]
    sd, x, t = calibrated_eval_state(f, C, K, N, H, W)
    torch.set_num_threads(min(16, os.cpu_count() or 1))
    # the reference is the oracle's autograd evaluated in fp64, in both precisions: in fp32 the oracle's
    # own eval-mode gradients are up to 1.5e-3 from it (E7: one activation of the 6-channel first layer
    # within rounding of zero changes its bias gradient's sum by one term), more than GRAD_TOL itself
    gref = _oracle_grads(cid, bf16, torch.float64)
    floor = grad_err(_oracle_grads(cid, bf16, torch.float32), gref)[0]
    tol = max(GRAD_TOL, 2 * floor) if bf16 else GRAD_TOL
    net = _net(cid, dev)
    before = _buffers(net)
    xd = x.to(dev)
    if (cid, bf16) not in _HIP_OUT:
        with torch.no_grad():
            _HIP_OUT[(cid, bf16)] = _forward(net, xd, bf16).cpu()
    assert all(p.requires_grad for p in net.parameters()) and not net.training
    out = _forward(net, xd, bf16)
    assert out.requires_grad
    assert torch.equal(out.detach().cpu(), _HIP_OUT[(cid, bf16)])
    unet_loss(out, t.to(dev), K).backward()
    torch.cuda.synchronize()
    named = dict(net.named_parameters())
    keys = unet_param_keys(sd)
    missing = [k for k in keys if named[k].grad is None]
    assert not missing, missing[:4]
    err, worst = grad_err({k: named[k].grad for k in keys}, gref)
    _say(capsys, f"EVAL_BWD {cid} {'bf16' if bf16 else 'fp32'}: grad err {err:.3e} at {worst} (tol {tol:.3e}; the "
         f"oracle's fp32 evaluation is {floor:.3e} from its fp64 one)")
    assert err <= tol, (err, worst, tol)
    _assert_buffers_unchanged(net, before)


def test_double_conv_eval_mode_with_autograd(dev, capsys):
    """A standalone DoubleConv(16, 32).eval() at 17 x 23 (pmu_hip.blocks): output, parameter gradients
    and the input gradient against the oracle's eval-mode double_conv."""
    from model.unet.unet_parts import DoubleConv
    from oracle.unet_ref import double_conv
    torch.manual_seed(0)
    dc = DoubleConv(16, 32)
    g = torch.Generator().manual_seed(13)
    for m in dc.modules():
        if isinstance(m, torch.nn.BatchNorm2d):
            m.running_mean.copy_(torch.rand(32, generator=g) * 0.4 - 0.2)
            m.running_var.copy_(torch.rand(32, generator=g) + 0.5)
            m.weight.data.copy_(torch.rand(32, generator=g) + 0.5)
            m.bias.data.copy_(torch.randn(32, generator=g) * 0.2)
    sd = {k: v.detach().clone() for k, v in dc.state_dict().items()}
    x = torch.randn(2, 16, 17, 23, generator=g)
    wgt = torch.randn(2, 32, 17, 23, generator=g)
    keys = [k for k in sd if "running" not in k and "num_batches" not in k]
    params = {k: sd[k].clone().requires_grad_(True) for k in keys}
    work = dict(sd)
    work.update(params)
    xr = x.clone().requires_grad_(True)
    ref = double_conv(xr, work, "", False)
    (ref * wgt).sum().backward()
    gref = {k: params[k].grad for k in keys}
    gref["input"] = xr.grad
    dc = dc.to(dev).eval()
    before = _buffers(dc)
    xd = x.to(dev).requires_grad_(True)
    out = dc(xd)
    assert max_abs(out, ref) <= ACT_TOL
    (out * wgt.to(dev)).sum().backward()
    torch.cuda.synchronize()
    named = dict(dc.named_parameters())
    got = {k: named[k].grad for k in keys}
    got["input"] = xd.grad
    err, worst = grad_err(got, gref)
    _say(capsys, f"EVAL_BWD DoubleConv(16, 32) 17x23: out err {max_abs(out, ref):.3e} grad err {err:.3e} at {worst}")
    assert err <= GRAD_TOL, (err, worst)
    _assert_buffers_unchanged(dc, before)


def test_gaussian_encoder_eval_mode_with_autograd(dev, capsys):
    """The posterior AxisAlignedConvGaussian (pmu_hip.prob_engine: first-layer kernel on 2 input planes,
    AvgPool2d(2, ceil) at odd sizes, spatial mean, latent head) in eval mode with grad enabled, against
    the oracle's eval-mode gaussian_forward: mu_log_sigma and every parameter gradient."""
    from model.probabilistic_unet.probabilistic_unet import AxisAlignedConvGaussian
    from oracle.probunet_ref import gaussian_forward
    from pmu_hip.functions import gaussian_apply
    torch.manual_seed(1)
    m = AxisAlignedConvGaussian(1, [8, 16, 32], 2, 6, {"w": "he_normal", "b": "normal"}, posterior=True)
    g = torch.Generator().manual_seed(17)
    for bn in m.modules():
        if isinstance(bn, torch.nn.BatchNorm2d):
            C = bn.num_features
            bn.running_mean.copy_(torch.rand(C, generator=g) * 0.4 - 0.2)
            bn.running_var.copy_(torch.rand(C, generator=g) + 0.5)
    sd = {k: v.detach().clone() for k, v in m.state_dict().items()}
    keys = [k for k, _ in m.named_parameters()]
    params = {k: sd[k].clone().requires_grad_(True) for k in keys}
    work = dict(sd)
    work.update(params)
    x = torch.rand(2, 1, 21, 19, generator=g)
    segm = torch.randint(0, 3, (2, 1, 21, 19), generator=g).float()
    wgt = torch.randn(2, 12, generator=g)
    ref = torch.cat(gaussian_forward(work, "", x, 3, 6, segm=segm, training=False), 1)
    (ref * wgt).sum().backward()
    m = m.to(dev).eval()
    before = _buffers(m)
    out = gaussian_apply(m, x.to(dev), segm.to(dev))
    assert out.requires_grad and max_abs(out, ref) <= ACT_TOL
    (out * wgt.to(dev)).sum().backward()
    torch.cuda.synchronize()
    named = dict(m.named_parameters())
    err, worst = grad_err({k: named[k].grad for k in keys}, {k: params[k].grad for k in keys})
    _say(capsys, f"EVAL_BWD posterior encoder 21x19: out err {max_abs(out, ref):.3e} grad err {err:.3e} at {worst}")
    assert err <= GRAD_TOL, (err, worst)
    _assert_buffers_unchanged(m, before)


# ----------------------------------------------------------------------------------------
# predict_volume: the per-slice predictions inside it against the oracle
# ----------------------------------------------------------------------------------------
def _scan(shape, seed):
    """One synthetic scan, as tests/test_data_gpu.py's _synthetic_scans builds them."""
    g = np.random.default_rng(seed)
    img = g.random(shape) * 100.0
    ii, jj, kk = np.meshgrid(*[np.arange(d) for d in shape], indexing="ij")
    r2 = (ii - shape[0] / 2) ** 2 + (jj - shape[1] / 2) ** 2 + (kk - shape[2] / 2) ** 2
    lab = np.zeros(shape)
    lab[r2 < (min(shape) / 3) ** 2] = 1.0
    lab[r2 < (min(shape) / 6) ** 2] = 2.0
    return {"scan0.nii": (img, lab)}


@pytest.mark.parametrize("bf16", [False, True], ids=["fp32", "bf16"])
def test_predict_volume_matches_oracle(bf16, dev, capsys):
    """predict_volume on a (40, 36, 44) scan (padded to 40 x 44 x 44: 40 slices of 44 x 44, 44 of 40 x 44
    twice; batches of 16, the last of each view partial): every view's stack against the oracle's
    eval-mode forward of the same slices, and the Dice of the views and of their fusion inside the
    interval the oracle's fused softmax volumes allow.  A voxel may take either of its top two labels
    where their fused probabilities are within the stacks' tolerance of each other: softmax moves a
    probability by at most half the largest logit error, so a margin by at most that error, and the
    average of three views by no more."""
    from oracle.data_ref import fuse
    from oracle.unet_ref import unet_forward
    from predict import predict_volume
    from utils.mri_dataset import MRI_Dataset
    filters, K = [16, 32, 64], 3
    scans = _scan((40, 36, 44), 5)
    ds = MRI_Dataset("/imgs", "/labs", 3, filter=True, files=sorted(scans),
                     loader=lambda p: scans[os.path.basename(p)][0 if "imgs" in p else 1], device=dev)
    sd = calibrated_eval_state(filters, 1, K, 2, 40, 44)[0]
    from model import UNet
    net = UNet(1, K, filters)
    net.load_state_dict(sd)
    net = net.to(dev)
    before = _buffers(net)
    with torch.autocast("cuda", dtype=torch.bfloat16, enabled=bf16):
        res = predict_volume(net, ds, 0, batch_size=16)
    torch.cuda.synchronize()
    assert [tuple(s.shape) for s in res["stacks"]] == [(40, K, 44, 44), (44, K, 40, 44), (44, K, 40, 44)]
    torch.set_num_threads(min(16, os.cpu_count() or 1))
    refs, tols = [], []
    for v in range(3):
        n = res["stacks"][v].shape[0]
        x = ds.get_slices([(0, v, s) for s in range(n)])["image"].cpu()
        with torch.no_grad():
            o32 = unet_forward(dict(sd), x, 3, K, training=False, bf16=bf16)
            if bf16:
                ref = unet_forward(_dbl(sd), x.double(), 3, K, training=False, bf16=True)
                floor = max_abs(o32, ref)
                tol = max(ACT_TOL, 2 * floor)
            else:
                ref, floor, tol = o32, None, ACT_TOL
        err = max_abs(res["stacks"][v], ref)
        _say(capsys, f"EVAL_VOLUME {'bf16' if bf16 else 'fp32'} view {v}: stack err {err:.3e} (tol {tol:.3e}, floor "
             f"{floor if floor is None else format(floor, '.3e')}) max|ref| {float(ref.abs().max()):.2f}")
        assert err <= tol, (v, err, tol)
        refs.append(ref)
        tols.append(tol)
    vols = fuse(*[torch.softmax(r.double(), 1) for r in refs])
    truth = res["truth"].cpu()
    tie = max(tols) + 1e-5
    for v in range(4):
        for k in (1, 2):
            lo, hi, n_tie = dice_bounds(vols[v], truth, k, tie=tie)
            got = float(res["dice"][v, k])
            assert lo - 1e-5 <= got <= hi + 1e-5, (v, k, got, lo, hi, n_tie)
    _say(capsys, f"EVAL_VOLUME {'bf16' if bf16 else 'fp32'}: fused Dice {[round(float(d), 4) for d in res['dice'][3]]}")
    _assert_buffers_unchanged(net, before)
