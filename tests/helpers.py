"""Shared comparison helpers for parity tests (tolerances from SURVEY.md §4)."""
import torch

ACT_TOL = 1e-3    # forward activations / outputs, absolute
LOSS_RTOL = 1e-3  # losses, relative
GRAD_TOL = 1e-3   # gradients: max |dg| / max |g_ref| over the tensor set (globally normalised)


def max_abs(a, b):
    return float((a.detach().double().cpu() - b.detach().double().cpu()).abs().max())


def grad_err(got: dict, ref: dict):
    """Globally normalised max-abs gradient error and the worst key."""
    gmax = max(float(v.abs().max()) for v in ref.values())
    worst, wk = 0.0, None
    for k, r in ref.items():
        e = max_abs(got[k], r) / gmax
        if e > worst:
            worst, wk = e, k
    return worst, wk


def dice_bounds(vol, truth, k, tie=1e-5):
    """eval.py's dice(volume, truth, k) (:42-49) as an interval over the fp32 near-ties: voxels whose
    top-two probabilities are within ``tie`` (softmax / averaging rounding can order them either
    way) may take either of those two labels.  Without near-ties lo == hi == the reference's Dice."""
    s = 1e-6
    top = torch.topk(vol, 2, dim=1)
    amb = (top.values[:, 0] - top.values[:, 1]) < tie
    lab = top.indices[:, 0]
    t = truth.reshape(lab.shape) == k
    sure = (lab == k) & ~amb
    cand = amb & ((top.indices[:, 0] == k) | (top.indices[:, 1] == k))
    i0, p0, tt = float((sure & t).sum()), float(sure.sum()), float(t.sum())
    a, b = float((cand & t).sum()), float((cand & ~t).sum())
    return (2 * i0 + s) / (p0 + b + tt + s), (2 * (i0 + a) + s) / (p0 + a + tt + s), int(amb.sum())


# ----------------------------------------------------------------------------------------
# eval-mode state: a briefly trained U-Net whose BN running statistics match its activations
# ----------------------------------------------------------------------------------------
def phantom_batch(N, C, H, W, K, seed):
    """(x, target): N slices of C noisy contrasts over a seeded elliptical two-shell label map with
    K <= 3 classes (tests/test_bf16_gpu.py's _phantom_slices made 2-D: slice n cuts the ellipsoid at its
    own depth).  Channel c is 0.5 * rand + (0.15 + 0.1 c) * label.  target: (N, 1, H, W), the class index
    (long) for K > 1, the float foreground mask for K == 1."""
    assert 1 <= K <= 3
    g = torch.Generator().manual_seed(seed)
    cy, cx = (torch.rand(2, generator=g) - 0.5) * 0.1
    ay = (torch.arange(H, dtype=torch.float32) - H / 2) / H - cy
    ax = (torch.arange(W, dtype=torch.float32) - W / 2) / W - cx
    depth = torch.linspace(-0.45, 0.45, N) if N > 1 else torch.zeros(1)
    r2 = (ay[None, :, None] / 0.40) ** 2 + (ax[None, None, :] / 0.36) ** 2 + depth[:, None, None] ** 2
    lab = ((r2 < 1.0).long() + (r2 < 0.4).long()).clamp_max(max(K - 1, 1))
    x = torch.stack([0.5 * torch.rand(N, H, W, generator=g) + (0.15 + 0.1 * c) * lab.float() for c in range(C)], 1)
    target = lab[:, None]
    return x, (target.float() if K == 1 else target)


_EVAL_STATES = {}


def calibrated_eval_state(filters, C, K, N, H, W):
    """(state_dict, x, target) for eval-mode tests of model.UNet(C, K, filters), everything on the CPU in
    fp32: the seed-0 initial state after a few oracle training steps (clip + SGD, lr 0.05) on
    phantom_batch(seed=21), with running statistics that describe its activations — reset to (0, 1),
    one training-mode oracle forward on phantom_batch(seed=23), the momentum 0.1 un-mixed.  (Statistics
    drawn at random let the eval activations shrink layer by layer until an absolute tolerance proves
    little.)  x, target: the evaluation batch, phantom_batch(seed=22).  Computed once per argument set;
    callers do not write into what they get."""
    key = (tuple(filters), C, K, N, H, W)
    if key not in _EVAL_STATES:
        from model import UNet
        from oracle.unet_ref import unet_forward, unet_param_keys, unet_train_step
        nlev = len(filters)
        torch.manual_seed(0)
        sd = {k: v.detach().clone() for k, v in UNet(C, K, list(filters)).state_dict().items()}
        bufs = {k: torch.zeros_like(sd[k]) for k in unet_param_keys(sd)}
        x, t = phantom_batch(N, C, H, W, K, 21)
        for _ in range(4 if nlev <= 3 else 3):
            unet_train_step(sd, x, t, nlev, K, lr=0.05, bufs=bufs)
        for k in sd:
            if k.endswith("running_mean"):
                sd[k] = torch.zeros_like(sd[k])
            elif k.endswith("running_var"):
                sd[k] = torch.ones_like(sd[k])
        with torch.no_grad():
            unet_forward(sd, phantom_batch(N, C, H, W, K, 23)[0], nlev, K, training=True)
        for k in sd:
            if k.endswith("running_mean"):
                sd[k] = sd[k] / 0.1
            elif k.endswith("running_var"):
                sd[k] = ((sd[k] - 0.9) / 0.1).clamp_min(1e-6)
        _EVAL_STATES[key] = ({k: v.detach() for k, v in sd.items()},) + phantom_batch(N, C, H, W, K, 22)
    sd, x, t = _EVAL_STATES[key]
    return dict(sd), x, t


# ----------------------------------------------------------------------------------------
# model.UNet's conv layers by shape, for the dispatch-policy tests (pmu_hip.routes)
# ----------------------------------------------------------------------------------------
def unet_convs(cin, filters, N, H, W):
    """The 3x3 convs and transposed convs of model.UNet(cin, _, filters) on an N x cin x H x W input, in
    forward order, as dicts: kind "conv" (name, N, H, W, Cin, Cout, planes, split, bnr) or "convT" (name,
    N, h, w, Cin, Cup, hs, ws, Cskip, Cout1).  planes: NCHW planes offered to the first-layer kernel;
    split: the concat split; bnr: the operand is one layer's unpooled activation (so its input gradient
    can form that layer's BN-backward partials)."""
    def conv(name, h, w, ci, co, **kw):
        return dict(kind="conv", name=name, N=N, H=h, W=w, Cin=ci, Cout=co,
                    **{"planes": 0, "split": None, "bnr": False, **kw})
    out = [conv("inc.c1", H, W, cin, filters[0], planes=cin if cin <= 4 else 0),
           conv("inc.c2", H, W, filters[0], filters[0], bnr=True)]
    dims = [(H, W)]
    for lev in range(1, len(filters)):
        h, w = dims[-1][0] // 2, dims[-1][1] // 2
        dims.append((h, w))
        out += [conv(f"down{lev}.c1", h, w, filters[lev - 1], filters[lev]),
                conv(f"down{lev}.c2", h, w, filters[lev], filters[lev], bnr=True)]
    hi, wi = dims[-1]
    for j, lev in enumerate(reversed(range(len(filters) - 1))):
        hs, ws = dims[lev]
        cup = filters[lev + 1] // 2
        out += [dict(kind="convT", name=f"up{j}.up", N=N, h=hi, w=wi, Cin=filters[lev + 1], Cup=cup, hs=hs, ws=ws,
                     Cskip=filters[lev], Cout1=filters[lev], off=((hs - 2 * hi) // 2, (ws - 2 * wi) // 2)),
                conv(f"up{j}.c1", hs, ws, filters[lev] + cup, filters[lev], split=filters[lev]),
                conv(f"up{j}.c2", hs, ws, filters[lev], filters[lev], bnr=True)]
        hi, wi = hs, ws
    return out


def unet_launch_plan(bf16, cin, filters, N, H, W):
    """The 3x3-conv and transposed-conv entries one training step of model.UNet launches, in order, as
    pmu_hip.routes gives them (forward, then backward as engine.unet_backward walks it)."""
    from pmu_hip import routes as R
    layers = unet_convs(cin, filters, N, H, W)
    fwd, info = [], {}
    for c in layers:
        if c["kind"] == "convT":
            inp = R.concat_in_place(bf16, N, c["h"], c["w"], c["Cin"], c["Cup"], c["hs"], c["ws"], c["Cskip"], c["Cout1"])
            fwd.append({"dma_ldb": "pmu_convT2x2_fwd_dma_ldb", "ld": "pmu_convT2x2_fwd_ld", "dma": "pmu_convT2x2_fwd_dma",
                        "bf16": "pmu_convT2x2_fwd_bf16", "f32": "pmu_convT2x2_fwd"}[
                            R.convT_fwd_route(bf16, inp, N, c["h"], c["w"], c["Cin"], c["Cup"])])
            continue
        route = R.conv_fwd_route(bf16, N, c["H"], c["W"], c["Cin"], c["Cout"], planes=c["planes"])
        fwd.append(R.FWD_ENTRY[route])
        info[c["name"]] = route
    by = {c["name"]: c for c in layers}

    def conv_bwd(name, need_dx=True, x1only=False):
        c = by[name]
        first = info[name] == "first"
        b = bf16 and not first
        ci = c["planes"] or c["Cin"]
        wroute = R.conv_wgrad_route(b, N, c["H"], c["W"], ci, c["Cout"], first=first, need_dx=need_dx,
                                    kept=R.conv_fwd_keeps_f32(info[name], ci, c["Cout"], True))
        wg, teed = R.WGRAD[wroute][0], wroute in R.TEED
        if not need_dx or first:
            return [wg]
        dg = R.conv_dgrad(b, N, c["H"], c["W"], ci, c["Cout"], c["split"], bnr=c["bnr"], want_dxb=True,
                          x1_bf16_only=x1only).entry
        return [dg, wg] if b or teed else [wg, dg]
    bwd = []
    nup = len(filters) - 1
    for j in reversed(range(nup)):
        t = by[f"up{j}.up"]
        tb = R.convT_bwd(bf16, t["Cin"], t["Cup"], t["off"])
        bwd += conv_bwd(f"up{j}.c2") + conv_bwd(f"up{j}.c1", x1only=tb.dup_bf16_only)
        bwd.append({"dma": "pmu_convT2x2_dgrad_dma" + ("_dxb" if tb.dx_bf16 else ""), "bf16": "pmu_convT2x2_dgrad_bf16",
                    "f32": "pmu_convT2x2_dgrad"}[tb.dgrad])
        bwd.append("pmu_convT2x2_wgrad_bf16" if bf16 else "pmu_convT2x2_wgrad")
    for lev in reversed(range(len(filters))):
        blk = "inc" if lev == 0 else f"down{lev}"
        bwd += conv_bwd(blk + ".c2") + conv_bwd(blk + ".c1", need_dx=lev > 0)
    return fwd + bwd


# ----------------------------------------------------------------------------------------
# pmu_frame restated on the CPU in float64 (include/pmunet_hip.h: pmu_src / pmu_frame), and inputs
# on exactly representable grids for the kernel tests that compare against it
# ----------------------------------------------------------------------------------------
SRC_RAW, SRC_BNRELU, SRC_BNBWD = 0, 1, 2
POOL_NONE, POOL_MAX2, POOL_AVG2CEIL = 0, 1, 2


def ref_frame(srcs, N, H, W):
    """The operand values of a pmu_frame as a float64 NHWC CPU tensor, from the stored tensors alone.
    srcs: up to two objects with the fields of pmu_hip.engine.Src (x NHWC, mode, coef, z, pool, off).
    Per source: the mode's transform (RAW x; BNRELU max(0, x*scale + shift); BNBWD scale*g + kx*(z - mean)
    + kc with g = x where z*scale + shift > 0, else 0), then the pool over the transformed values
    (POOL_MAX2: floor mode, a trailing odd row / column is ignored; POOL_AVG2CEIL: ceil mode, the divisor
    is the number of in-bounds elements), then placement at (off_h, off_w) inside the N x H x W frame;
    everything outside a source reads as zero; the sources are concatenated on channels.  No torch pooling
    operator is used, so tests/test_frame_ref_cpu.py can pin this to them."""
    assert 1 <= len(srcs) <= 2
    outs = []
    for s in srcs:
        x = s.x.detach().double().cpu()
        assert x.dim() == 4 and x.shape[0] == N
        _, Hs, Ws, C = x.shape
        coef = s.coef.detach().double().cpu() if s.coef is not None else None
        if s.mode == SRC_RAW:
            v = x
        elif s.mode == SRC_BNRELU:
            v = (x * coef[:C] + coef[C:2 * C]).clamp_min(0.0)
        else:
            assert s.mode == SRC_BNBWD
            z = s.z.detach().double().cpu()
            sc, sh, mu, kx, kc = coef.view(5, C)
            g = torch.where(z * sc + sh > 0, x, torch.zeros_like(x))
            v = sc * g + kx * (z - mu) + kc
        if s.pool == POOL_MAX2:
            Hp, Wp = Hs // 2, Ws // 2
            v = v[:, :2 * Hp, :2 * Wp].reshape(N, Hp, 2, Wp, 2, C).amax(dim=(2, 4))
        elif s.pool == POOL_AVG2CEIL:
            Hp, Wp = (Hs + 1) // 2, (Ws + 1) // 2
            pad = torch.zeros(N, 2 * Hp, 2 * Wp, C, dtype=torch.float64)
            cnt = torch.zeros(1, 2 * Hp, 2 * Wp, 1, dtype=torch.float64)
            pad[:, :Hs, :Ws] = v
            cnt[:, :Hs, :Ws] = 1.0
            v = pad.reshape(N, Hp, 2, Wp, 2, C).sum(dim=(2, 4)) / cnt.reshape(1, Hp, 2, Wp, 2, 1).sum(dim=(2, 4))
        else:
            assert s.pool == POOL_NONE
            Hp, Wp = Hs, Ws
        oh, ow = s.off
        out = torch.zeros(N, H, W, C, dtype=torch.float64)
        h0, h1, w0, w1 = max(oh, 0), min(oh + Hp, H), max(ow, 0), min(ow + Wp, W)
        if h1 > h0 and w1 > w0:
            out[:, h0:h1, w0:w1] = v[:, h0 - oh:h1 - oh, w0 - ow:w1 - ow]
        outs.append(out)
    return torch.cat(outs, dim=3)


def quant_z(N, H, W, C, gen):
    """Pre-BN values on the grid of multiples of 2^-4 in [-1.5, 1.5], with deliberate exact ties: of the
    (floor-mode) 2 x 2 windows about one in eight is constant and another one in eight repeats its first
    value in its second element.  With quant_bn coefficients z*scale + shift is exact in fp32 (multiples
    of 2^-5 below 4), so fp32 and fp64 agree on every ReLU mask and every max-pool winner; about half the
    activations are exact zeros, and all-zero windows occur."""
    z = torch.randint(-24, 25, (N, H, W, C), generator=gen).float() / 16
    Hp, Wp = H // 2, W // 2
    if Hp and Wp:
        kind = torch.randint(0, 8, (N, Hp, Wp, C), generator=gen)
        a = z[:, 0:2 * Hp:2, 0:2 * Wp:2]
        for dh, dw in ((0, 1), (1, 0), (1, 1)):
            t = z[:, dh:2 * Hp:2, dw:2 * Wp:2]
            m = (kind == 0) | ((kind == 1) & (dh == 0))
            t[m] = a[m]
    return z


def quant_bn(C, gen, bwd=False):
    """[scale | shift] with scale in {0.5, 1, 2} and shift a multiple of 2^-4 in [-0.5, 0.5]; with bwd the
    BN-backward block [scale | shift | mean | kx | kc]: mean on the same grid (z - mean is then exact),
    kx and kc ordinary randn (they only enter sums)."""
    scale = torch.tensor([0.5, 1.0, 2.0])[torch.randint(0, 3, (C,), generator=gen)]
    shift = torch.randint(-8, 9, (C,), generator=gen).float() / 16
    if not bwd:
        return torch.cat([scale, shift])
    mean = torch.randint(-8, 9, (C,), generator=gen).float() / 16
    return torch.cat([scale, shift, mean, torch.randn(C, generator=gen) * 0.1, torch.randn(C, generator=gen) * 0.1])


def ulp32(t):
    """Spacing of fp32 at the magnitude of each element of the float64 tensor t (the smallest normal's for
    smaller values)."""
    a = t.abs().clamp_min(2.0 ** -126)
    return torch.exp2(torch.floor(torch.log2(a)) - 23)
