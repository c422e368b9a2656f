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
                        "f32": "pmu_convT2x2_fwd"}[
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
        bwd.append({"dma": "pmu_convT2x2_dgrad_dma" + ("_dxb" if tb.dx_bf16 else ""), "f32": "pmu_convT2x2_dgrad"}[tb.dgrad])
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


def ref_frame(srcs, N, H, W, device="cpu"):
    """The operand values of a pmu_frame as a float64 NHWC tensor (on the CPU unless ``device`` names another
    place to evaluate the same expressions), from the stored tensors alone.
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
        x = s.x.detach().to(device).double()
        assert x.dim() == 4 and x.shape[0] == N
        _, Hs, Ws, C = x.shape
        coef = s.coef.detach().to(device).double() if s.coef is not None else None
        if s.mode == SRC_RAW:
            v = x
        elif s.mode == SRC_BNRELU:
            v = (x * coef[:C] + coef[C:2 * C]).clamp_min(0.0)
        else:
            assert s.mode == SRC_BNBWD
            z = s.z.detach().to(device).double()
            sc, sh, mu, kx, kc = coef.view(5, C)
            g = torch.where(z * sc + sh > 0, x, torch.zeros_like(x))
            v = sc * g + kx * (z - mu) + kc
        if s.pool == POOL_MAX2:
            Hp, Wp = Hs // 2, Ws // 2
            v = v[:, :2 * Hp, :2 * Wp].reshape(N, Hp, 2, Wp, 2, C).amax(dim=(2, 4))
        elif s.pool == POOL_AVG2CEIL:
            Hp, Wp = (Hs + 1) // 2, (Ws + 1) // 2
            pad = torch.zeros(N, 2 * Hp, 2 * Wp, C, dtype=torch.float64, device=device)
            cnt = torch.zeros(1, 2 * Hp, 2 * Wp, 1, dtype=torch.float64, device=device)
            pad[:, :Hs, :Ws] = v
            cnt[:, :Hs, :Ws] = 1.0
            v = pad.reshape(N, Hp, 2, Wp, 2, C).sum(dim=(2, 4)) / cnt.reshape(1, Hp, 2, Wp, 2, 1).sum(dim=(2, 4))
        else:
            assert s.pool == POOL_NONE
            Hp, Wp = Hs, Ws
        oh, ow = s.off
        out = torch.zeros(N, H, W, C, dtype=torch.float64, device=device)
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


def quant_bn(C, gen, bwd=False, dyadic=False):
    """[scale | shift] with scale in {0.5, 1, 2} and shift a multiple of 2^-4 in [-0.5, 0.5]; with bwd the
    BN-backward block [scale | shift | mean | kx | kc]: mean on the same grid (z - mean is then exact),
    kx and kc ordinary randn (they only enter sums) — or, with dyadic, multiples of 2^-4 in [-1, 1], so
    that kx * (z - mean) + kc (a multiple of 2^-8 below 4) and the whole BN-backward value are exact in fp32."""
    scale = torch.tensor([0.5, 1.0, 2.0])[torch.randint(0, 3, (C,), generator=gen)]
    shift = torch.randint(-8, 9, (C,), generator=gen).float() / 16
    if not bwd:
        return torch.cat([scale, shift])
    mean = torch.randint(-8, 9, (C,), generator=gen).float() / 16
    if dyadic:
        return torch.cat([scale, shift, mean, torch.randint(-16, 17, (C,), generator=gen).float() / 16,
                          torch.randint(-16, 17, (C,), generator=gen).float() / 16])
    return torch.cat([scale, shift, mean, torch.randn(C, generator=gen) * 0.1, torch.randn(C, generator=gen) * 0.1])


def quant_invstd(C, gen):
    """1 / std on {0.5, 1, 2}: xhat = (z - mean) * invstd is then an exact multiple of 2^-5."""
    return torch.tensor([0.5, 1.0, 2.0])[torch.randint(0, 3, (C,), generator=gen)]


def quant_grad(shape, gen, fine=False):
    """Gradients (da, dpool, skip) on a grid: multiples of 2^-4 in [-2, 2] (the partial sums of the BN
    backward then stay exact), or with fine multiples of 2^-6 in [-4, 4] — every value is still a bf16
    number (at most 2^8 units), but scale * g + kx * (z - mean) + kc then has up to ten significant bits,
    so storing it as bf16 rounds: to even on ties, up and down elsewhere (rne_census counts them)."""
    if fine:
        return torch.randint(-256, 257, tuple(shape), generator=gen).float() / 64
    return torch.randint(-32, 33, tuple(shape), generator=gen).float() / 16


def bf16_bits(t):
    """The bf16 (round to nearest, ties to even) bit patterns of a float tensor as int16, the kernels' storage."""
    return t.float().to(torch.bfloat16).view(torch.int16)


def rne_census(ref64):
    """How the values of the float64 tensor ref64 (each an fp32 number) round to bf16: a dict of counts —
    tie_up / tie_down (exactly half way, rounded away from / towards zero to the even neighbour), up / down
    (the other inexact values, by the direction of the magnitude) and exact."""
    r = ref64.detach().double().cpu().reshape(-1)
    assert torch.equal(r.float().double(), r), "rne_census: the values are not fp32 numbers"
    b = r.float().to(torch.bfloat16).double()
    d = b.abs() - r.abs()
    half = torch.exp2(torch.floor(torch.log2(r.abs().clamp_min(2.0 ** -126))) - 8)   # half a bf16 ulp at |r|
    tie = (d.abs() == half) & (d != 0)
    return {"tie_up": int((tie & (d > 0)).sum()), "tie_down": int((tie & (d < 0)).sum()),
            "up": int((~tie & (d > 0)).sum()), "down": int((~tie & (d < 0)).sum()), "exact": int((d == 0).sum())}


def assert_rne_exercised(ref64, what):
    """The values a kernel rounds to bf16 must tell round-to-nearest-even from truncation and from rounding
    half away: ties resolved in both directions, and other values rounded up and down."""
    c = rne_census(ref64)
    assert min(c["tie_up"], c["tie_down"], c["up"], c["down"]) > 0, f"{what}: bf16 rounding not exercised: {c}"
    return c


def ulp32(t):
    """Spacing of fp32 at the magnitude of each element of the float64 tensor t (the smallest normal's for
    smaller values)."""
    a = t.abs().clamp_min(2.0 ** -126)
    return torch.exp2(torch.floor(torch.log2(a)) - 23)


# ----------------------------------------------------------------------------------------
# exact comparisons: inputs on grids where every product and every partial sum of a kernel is a
# representable number, so a correct kernel returns the float64 reference bit for bit
# ----------------------------------------------------------------------------------------
EXACT_LIMIT = 2.0 ** 24   # integers of magnitude below 2^24 are fp32 values; so are their sums in any order


class Grid:
    """A seeded source of CPU fp32 tensors on exactly representable grids.  operand(): the values a conv
    multiplies (activations, upstream gradients), multiples of ``ux``; weight(): multiples of ``uw``;
    bias(): multiples of ``ub``.  Every value is a bf16 number, every product a multiple of ux * uw."""

    def __init__(self, name, seed, ux, x_steps, x_nonzero, uw, w_steps, w_nonzero, ub, b_steps, unit=None):
        self.name, self.ux, self.uw, self.ub = name, ux, uw, ub
        self._unit = ux * uw if unit is None else unit
        self._x, self._w, self._b = (x_steps, x_nonzero), (w_steps, w_nonzero), b_steps
        self.gen = torch.Generator().manual_seed(seed)

    @property
    def unit(self):
        """The power-of-two grid of a conv's results: every product of an operand and a weight, and the
        bias, is a multiple of it."""
        return self._unit

    def _draw(self, shape, steps, nonzero, unit):
        mag = torch.randint(1, steps + 1, shape, generator=self.gen).float()
        sign = torch.randint(0, 2, shape, generator=self.gen).float() * 2 - 1
        keep = (torch.rand(shape, generator=self.gen) < nonzero).float()
        return mag * sign * keep * unit

    def operand(self, *shape):
        return self._draw(shape, self._x[0], self._x[1], self.ux)

    def weight(self, *shape):
        return self._draw(shape, self._w[0], self._w[1], self.uw)

    def bias(self, C):
        return torch.randint(-self._b, self._b + 1, (C,), generator=self.gen).float() * self.ub


def grid_data(seed):
    """Operands on multiples of 2^-2 in [-2, 2], about half of them zero; weights on multiples of 2^-3 in
    [-1, 1]; bias on multiples of 2^-2 in [-2, 2].  Results are multiples of 2^-5."""
    return Grid("data", seed, 0.25, 8, 0.5, 0.125, 8, 1.0, 0.25, 8)


def grid_stats(seed):
    """Operands in {0, +-1/2, +-1} (about 40 % non-zero), weights in {0, +-1/2, +-1} (about 60 % non-zero), bias
    on multiples of 1/2 in [-1, 1]: small enough that the sums over a whole map of z (multiples of 2^-2) and
    of z^2 (multiples of 2^-4) stay below 2^24 units, so the BN partial sums are exact too."""
    return Grid("stats", seed, 0.5, 2, 0.4, 0.5, 2, 0.6, 0.5, 2)


F4_UW = 576.0 * 2.0 ** -10


def grid_f4(seed):
    """For F(4x4, 3x3): operands in {0, +-1} (about 40 % non-zero), weights in {0, +-576 * 2^-10} (about 60 %
    non-zero).  G g G^T has denominators up to 24 * 24 = 576, so the transformed weights are integers of
    2^-10 and every Winograd-domain value is a multiple of 2^-10.  Products are multiples of 9 * 2^-4: the
    result grid is 2^-4."""
    return Grid("f4", seed, 1.0, 1, 0.4, F4_UW, 1, 0.6, F4_UW, 0, unit=2.0 ** -4)


def bf16_exact(t):
    """True where a value survives the round trip through bfloat16."""
    return bool((t.to(torch.bfloat16).float() == t.float()).all())


def exact_headroom(abs_sum64, unit, what):
    """The condition of an exact comparison.  abs_sum64: per result element, the float64 sum of the absolute
    values of every term the kernel adds up for it (the reference operator run on absolute values; it bounds
    every partial sum of every summation order).  Asserts that it stays below 2^24 units of the result
    grid and returns the largest value in units.  A case that fails here is a mistake in the test."""
    units = float(abs_sum64.abs().max()) / unit
    assert units < EXACT_LIMIT, f"{what}: sum of |terms| reaches {units:.3g} units of {unit:g}, limit {EXACT_LIMIT:.3g}"
    return units


# Winograd F(m x m, 3 x 3) as Lavin & Gray state it and csrc/conv3x3_wino*.hip restates it: y = A^T [(G g G^T)
# o (B^T d B)] A per tile of m x m outputs.  (rows of A^T, G, B^T)
WINO = {
    2: (((1, 1, 1, 0), (0, 1, -1, -1)),
        ((1, 0, 0), (.5, .5, .5), (.5, -.5, .5), (0, 0, 1)),
        ((1, 0, -1, 0), (0, 1, 1, 0), (0, -1, 1, 0), (0, 1, 0, -1))),
    4: (((1, 1, 1, 1, 1, 0), (0, 1, -1, 2, -2, 0), (0, 1, 1, 4, 4, 0), (0, 1, -1, 8, -8, 1)),
        ((1 / 4, 0, 0), (-1 / 6, -1 / 6, -1 / 6), (-1 / 6, 1 / 6, -1 / 6), (1 / 24, 1 / 12, 1 / 6), (1 / 24, -1 / 12, 1 / 6),
         (0, 0, 1)),
        ((4, 0, -5, 0, 1, 0), (0, -4, -4, 1, 1, 0), (0, 4, -4, -1, 1, 0), (0, -2, -1, 2, 1, 0), (0, 2, -1, -2, 1, 0),
         (0, 4, 0, -5, 0, 1))),
}


def _wino_mats(m):
    return tuple(torch.tensor(t, dtype=torch.float64) for t in WINO[m])


def _patches(x, m):
    """(N, C, H, W) -> (N, C, th, tw, m + 2, m + 2): the zero-padded input patch of every m x m output tile."""
    N, C, H, W = x.shape
    th, tw = -(-H // m), -(-W // m)
    xp = torch.zeros(N, C, th * m + 2, tw * m + 2, dtype=x.dtype)
    xp[:, :, 1:H + 1, 1:W + 1] = x
    return xp.unfold(2, m + 2, m).unfold(3, m + 2, m)


def wino_conv(m, x, w, absolute=False):
    """conv2d(x, w, padding=1) of float64 NCHW x and [Cout][Cin][3][3] w evaluated as F(m x m, 3 x 3) in
    float64: A^T [(G g G^T) o (B^T d B)] A summed over the input channels.

    absolute: the same on absolute values, stage by stage — |A|^T [sum_c |G g G^T| o |B^T d B|] |A|.  Each
    result bounds every partial sum the kernel can form for that output, in any order, given that the stage
    before it is exact: the transformed weights U (formed once per weight; integers of the grid by the
    grids' construction) and operands V (sums of at most (row sum of |B^T|)^2 operand values: 4 for F(2x2),
    100 for F(4x4), far below 2^24 units) are exact, then the channel sum's partial sums are at most
    sum_c |U| |V|, and the output transform's at most |A|^T (that) |A|.  Growth over one product |g| |d|, from
    the row sums of |B^T|, |G| and |A^T|: 2 * 3/2 * 3 = 9 per dimension for F(2x2) (81 in two), 10 * 1 * 19 =
    190 for F(4x4) (36100 in two); the restatement evaluates the bound on the actual data, far below that."""
    AT, G, BT = _wino_mats(m)
    N, C, H, W = x.shape
    U = torch.einsum("ia,ocab,jb->ocij", G, w.double(), G)
    V = torch.einsum("ia,ncyxab,jb->ncyxij", BT, _patches(x.double(), m), BT)
    if absolute:
        AT, U, V = AT.abs(), U.abs(), V.abs()
    M = torch.einsum("ocij,ncyxij->noyxij", U, V)
    Y = torch.einsum("ai,noyxij,bj->noyaxb", AT, M, AT)
    return Y.reshape(N, w.shape[0], Y.shape[2] * m, Y.shape[4] * m)[:, :, :H, :W]


def wino_wgrad(x, dz, absolute=False):
    """conv2d's weight gradient evaluated as csrc/wgrad3x3_wino.hip does, in float64: dw = G^T [sum over the
    2 x 2 tiles of (A dY A^T) o (B^T X B)] G with F(2x2, 3x3)'s matrices.  x (N, Cin, H, W), dz (N, Cout, H,
    W).  absolute: the stage-by-stage bound, as wino_conv: |G|^T [sum over tiles |A dY A^T| o |B^T X B|] |G|."""
    AT, G, BT = _wino_mats(2)
    N, Co, H, W = dz.shape
    th, tw = -(-H // 2), -(-W // 2)
    dp = torch.zeros(N, Co, th * 2, tw * 2, dtype=torch.float64)
    dp[:, :, :H, :W] = dz
    dY = dp.unfold(2, 2, 2).unfold(3, 2, 2)
    D = torch.einsum("ai,noyxab,bj->noyxij", AT, dY, AT)
    V = torch.einsum("ia,ncyxab,jb->ncyxij", BT, _patches(x.double(), 2), BT)
    if absolute:
        D, V, G = D.abs(), V.abs(), G.abs()
    M = torch.einsum("noyxij,ncyxij->ocij", D, V)
    return torch.einsum("ia,ocij,jb->ocab", G, M, G)


def assert_exact(got, ref64, where, tile=None, cblock=None):
    """got (any float dtype, any device) must equal the float64 reference element for element.  On failure
    the message counts the differing elements and lists the first eight as (index, got, ref); for an NHWC
    tensor each also says whether it lies on the image border, on an edge of the kernel's th x tw pixel tile
    (tile = (th, tw): h % th or w % tw in {0, th - 1 / tw - 1}) and in the last, ragged block of cblock
    channels (C % cblock != 0)."""
    g = got.detach().double().cpu()
    assert g.shape == ref64.shape, f"{where}: shape {tuple(g.shape)} != {tuple(ref64.shape)}"
    bad = ~(g == ref64)    # (a NaN left in the output differs from everything)
    nbad = int(bad.sum())
    if not nbad:
        return
    lines = []
    for idx in bad.nonzero()[:8].tolist():
        notes = []
        if g.dim() == 4:
            n, h, w, c = idx
            _, H, W, C = g.shape
            if h in (0, H - 1) or w in (0, W - 1):
                notes.append("image border")
            if tile is not None:
                th, tw = tile
                if h % th in (0, th - 1) or w % tw in (0, tw - 1):
                    notes.append(f"tile edge (h % {th} = {h % th}, w % {tw} = {w % tw})")
            if cblock is not None and C % cblock and c >= C // cblock * cblock:
                notes.append(f"last ragged channel block ({C % cblock} of {cblock})")
        lines.append(f"  {tuple(idx)}: got {float(g[tuple(idx)])!r}, ref {float(ref64[tuple(idx)])!r}"
                     + (" [" + ", ".join(notes) + "]" if notes else " [interior]"))
    raise AssertionError(f"{where}: {nbad} of {g.numel()} elements differ from the float64 reference\n" + "\n".join(lines))


# ----------------------------------------------------------------------------------------
# BatchNorm+ReLU backward partial sums and MaxPool2d(2) backward restated in float64 (bn.hip, pool_bwd.hip)
# ----------------------------------------------------------------------------------------
def rows_bn_bwd(N, H, W, C):
    """Row block of every pixel under pmu_bn_bwd_tiles: consecutive blocks of 65536 / (4 C) pixels (at least
    one) in (n, h, w) order.  (N, H, W) long."""
    ppb = max(1, 65536 // (4 * C))
    return (torch.arange(N * H * W) // ppb).view(N, H, W)


def rows_maxpool_bwd(N, H, W, C):
    """Row block of every pixel under pmu_maxpool2_bwd_bnr_tiles: consecutive blocks of max(1, 8192 / C)
    ceil-sized 2 x 2 windows in (n, hc, wc) order; a pixel belongs to the window (h // 2, w // 2)."""
    wpb = max(1, 8192 // C)
    Hc, Wc = (H + 1) // 2, (W + 1) // 2
    n = torch.arange(N).view(N, 1, 1)
    hc = (torch.arange(H) // 2).view(1, H, 1)
    wc = (torch.arange(W) // 2).view(1, 1, W)
    return ((n * Hc + hc) * Wc + wc) // wpb


def ref_bn_bwd_sums(da64, z, coef, mean, invstd, rows):
    """The BN+ReLU backward partial sums in float64: part[r][0][c] = sum g, part[r][1][c] = sum g * xhat over
    the pixels whose rows[n][h][w] == r, with g = da where z * scale + shift > 0 (else 0) and xhat = (z - mean)
    * invstd.  da64, z: (N, H, W, C); coef = [scale | shift | ...]; rows: (N, H, W) long.  Returns (part
    (R, 2, C), the same two sums over absolute values (R, 2, C)) — the second bounds every partial sum of every
    summation order, for exact_headroom."""
    N, H, W, C = da64.shape
    z = z.detach().double().cpu()
    da = da64.detach().double().cpu()
    coef, mean, invstd = coef.double().cpu(), mean.double().cpu(), invstd.double().cpu()
    g = torch.where(z * coef[:C] + coef[C:2 * C] > 0, da, torch.zeros_like(da))
    gx = g * ((z - mean) * invstd)
    idx = rows.reshape(-1)
    R = int(idx.max()) + 1
    out = []
    for a, b in ((g, gx), (g.abs(), gx.abs())):
        part = torch.zeros(R, 2, C, dtype=torch.float64)
        part[:, 0].index_add_(0, idx, a.reshape(-1, C))
        part[:, 1].index_add_(0, idx, b.reshape(-1, C))
        out.append(part)
    return out[0], out[1]


def ref_maxpool_bwd(dpool, skip, z, coef):
    """MaxPool2d(2) backward of relu(z * scale + shift) added to the skip gradient, in float64 and without
    torch's pooling backward: dx = skip (zeros when None) + dpool routed to the first maximum of each floor-mode
    2 x 2 window in the order (0,0), (0,1), (1,0), (1,1).  The odd last row / column lies in no window and
    receives the skip gradient only.  dpool (N, H // 2, W // 2, C); skip, z (N, H, W, C)."""
    z = z.detach().double().cpu()
    N, H, W, C = z.shape
    Hp, Wp = H // 2, W // 2
    coef = coef.double().cpu()
    a = (z * coef[:C] + coef[C:2 * C]).clamp_min(0.0)
    dx = torch.zeros_like(z) if skip is None else skip.detach().double().cpu().clone()
    dp = dpool.detach().double().cpu()
    assert dp.shape == (N, Hp, Wp, C)
    pos = ((0, 0), (0, 1), (1, 0), (1, 1))
    best = a[:, 0:2 * Hp:2, 0:2 * Wp:2].clone()
    arg = torch.zeros(N, Hp, Wp, C, dtype=torch.long)
    for k in (1, 2, 3):
        v = a[:, pos[k][0]:2 * Hp:2, pos[k][1]:2 * Wp:2]
        m = v > best
        arg[m] = k
        best = torch.where(m, v, best)
    for k, (dh, dw) in enumerate(pos):
        dx[:, dh:2 * Hp:2, dw:2 * Wp:2] += torch.where(arg == k, dp, torch.zeros_like(dp))
    return dx
