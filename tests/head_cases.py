"""Inputs and float64 references of the 1x1 head cases (csrc/head1x1.hip), shared by tests/test_head_exact_gpu.py
(which runs pmu_head1x1_fwd / _bwd / _bwd_bnr / _bwd_dz and pmu_wgrad1x1 on them) and tests/test_head_exact_cpu.py
(which checks, without a GPU, that every case satisfies the conditions of an exact comparison).

Grids (helpers.py): z multiples of 2^-4 in [-1.5, 1.5] with deliberate ties (quant_z); scale, invstd in {0.5, 1, 2};
shift, mean multiples of 2^-4 in [-0.5, 0.5] (quant_bn(bwd=True), quant_invstd).  Then
  * the activation a = relu(z * scale + shift) is a multiple of 2^-5 (U_A) below 4 and every ReLU mask is decided
    exactly; xhat = (z - mean) * invstd is a multiple of 2^-5 (U_X) of magnitude at most 4;
  * forward: weights multiples of 2^-3 in [-1, 1], bias multiples of 2^-2, so a logit is a multiple of U_A * 2^-3;
  * backward: weights in {0, +-1/2, +-1}, dy multiples of 2^-2 in [-2, 2] (2^-4 with fine), y in {0, 1/4, 1/2, 3/4, 1}
    for K <= 4 and in {0, 1/2, 1} for K >= 5: y * (1 - y) is 0, 3/16 or 1/4, g = dy * (y * (1 - y)) is exact and the
    endpoints give exact zeros; da = sum_k g_k w_k is a multiple of half g's unit;
  * dz = scale * [mask] da + kx * (z - mean) + kc with the dyadic bcoef of quant_bn(bwd=True, dyadic=True) is an fp32
    number; stored as bf16 it rounds, ties in both directions.
Every sum is exact as long as the sum of absolute values stays below 2^24 units of its grid (exact_headroom): per
logit; per 2048-pixel block (rows_head) for the BN-backward sums, dw and db of the fast kernels; per 1024-pixel block
for the generic weight gradient.  The block slabs are summed in fp64 and cast once, so dw and db equal the float64
sum over the whole map rounded to fp32 (which need not itself be an fp32 number).

HEADROOM keeps the largest sum of |terms| seen per quantity, in units, for the figures DESIGN.md quotes."""
from collections import namedtuple

import torch

from helpers import (POOL_AVG2CEIL, POOL_MAX2, POOL_NONE, SRC_BNBWD, SRC_BNRELU, SRC_RAW, exact_headroom, quant_bn,
                     quant_grad, quant_invstd, quant_z, ref_bn_bwd_sums, ref_frame)

S = namedtuple("S", "x mode coef z pool off", defaults=(SRC_RAW, None, None, POOL_NONE, (0, 0)))

HPPB, W1_PPB = 2048, 1024          # pixels per block: the fast head kernels; the generic weight gradient
U_A, U_X, U_W = 2.0 ** -5, 2.0 ** -5, 2.0 ** -3   # grids of the activation, of xhat and of the forward weights
FAST_C = (4, 8, 16, 32, 64, 128, 256)
SIG_CEILING = 8.0                  # fixed ceiling of the sigmoid's admitted error, in ulp32 of the reference
SIG_VMAX = 80.0                    # |logit| limit of the sigmoid cases: every result is a normal fp32 number

# N x H x W: a block of one pixel; a ragged second block (91 pixels); exactly one full block; one pixel over a full
# block; P mod (4 * PG) != 0 with N > 1; the deep slab reduction (R = 66 fast, 131 generic)
ONE, RAGGED, FULL, OVER, SMALL, DEEP = (1, 1, 1), (3, 23, 31), (2, 32, 32), (1, 1, 2049), (2, 7, 9), (2, 260, 257)
GEOMETRIES = (ONE, RAGGED, FULL, OVER, SMALL)

HEADROOM = {}


def _note(what, units):
    HEADROOM[what] = max(HEADROOM.get(what, 0.0), units)
    return units


def gid(shape):
    return "x".join(map(str, shape))


def fast_shape(C):
    """head_fast_shape's channel rule: C = 4 * CQ, CQ a power of two <= 64."""
    cq = C >> 2
    return C % 4 == 0 and 1 <= cq <= 64 and cq & (cq - 1) == 0


def rows_head(N, H, W, ppb=HPPB):
    """Row block of every pixel under pmu_head1x1_bwd_tiles: consecutive blocks of 2048 pixels in (n, h, w) order
    (ppb = W1_PPB: the 1024-pixel blocks of the generic pmu_wgrad1x1 kernel).  (N, H, W) long."""
    return (torch.arange(N * H * W) // ppb).view(N, H, W)


# ------------------------------------------------------------------------------------------ the layer feeding the head
Layer = namedtuple("Layer", "N H W C z coef mean invstd bcoef")
_LAYERS = {}


def layer(N, H, W, C):
    """The CPU fp32 tensors of the last layer at one shape, drawn once (seeded by the shape) and never written to:
    z; coef = [scale | shift] and mean of one quant_bn(bwd=True) block; invstd; bcoef, an independent dyadic
    BN-backward block [scale | shift | mean | kx | kc] for dz."""
    key = (N, H, W, C)
    if key not in _LAYERS:
        g = torch.Generator().manual_seed(((N * 137 + H) * 139 + W) * 4111 + C)
        z = quant_z(N, H, W, C, g)
        c5 = quant_bn(C, g, bwd=True)
        _LAYERS[key] = Layer(N, H, W, C, z, c5[:2 * C].clone(), c5[2 * C:3 * C].clone(), quant_invstd(C, g),
                             quant_bn(C, g, bwd=True, dyadic=True))
    return _LAYERS[key]


def act_src(l):
    """The head's operand on the fast path: one unpooled BN+ReLU source."""
    return S(l.z, SRC_BNRELU, l.coef)


# ------------------------------------------------------------------------------------------ forward
def fwd_params(K, C, sparse=False, sat=0):
    """(w (K, C) on multiples of 2^-3 in [-1, 1], b (K,) on multiples of 2^-2 in [-2, 2]).  sparse: about 24 weights
    per class are non-zero, so a logit stays small whatever C is (the sigmoid cases).  sat = +-1: the last class's
    bias is sat * 40 (fp32's sigmoid saturates to exactly 1 at +40) and, from three classes on, the one before it
    -sat * 40."""
    g = torch.Generator().manual_seed(7001 + 131 * K + C + (977 if sparse else 0))
    w = torch.randint(-8, 9, (K, C), generator=g).float() / 8
    if sparse:
        w = w * (torch.rand(K, C, generator=g) < min(1.0, 24.0 / C)).float()
    b = torch.randint(-8, 9, (K,), generator=g).float() / 4
    if sat:
        b[K - 1] = 40.0 * sat
        if K >= 3:
            b[K - 2] = -40.0 * sat
    return w, b


def sat_of(kind, C, K):
    """Which sign the saturating bias of a sigmoid case takes (0: none, every logit mid-range): the sweep over the
    fast path alternates, and leaves K = 1 mid-range except at C = 16 and 128; the geometry cases push up, the
    generic ones down (from two classes on)."""
    if kind == "fast":
        return (1 if (C // 4 + K) % 2 else -1) if (K > 1 or C in (16, 128)) else 0
    return 0 if K == 1 else 1 if kind == "geom" else -1


def ref_fwd(srcs, N, H, W, w, b, where, ua=U_A):
    """The float64 logits (N, K, H, W) of the head over ref_frame(srcs); asserts the headroom of every logit in units
    of ua * 2^-3 (ua: the grid of the frame's values: U_A, or U_A / 4 under an average pool)."""
    a = ref_frame(srcs, N, H, W)
    w64 = w.double()
    v = torch.einsum("nhwc,kc->nkhw", a, w64)
    absv = torch.einsum("nhwc,kc->nkhw", a.abs(), w64.abs())
    if b is not None:
        v = v + b.double().view(1, -1, 1, 1)
        absv = absv + b.double().abs().view(1, -1, 1, 1)
    _note("forward logit", exact_headroom(absv, ua * U_W, where + ": logit"))
    assert torch.equal(v.float().double(), v), where
    return v


GENERIC_FRAMES = ("C1", "C6", "C20", "C255", "C260", "raw16", "two_6+10", "max2", "avg2ceil", "offset")
_FRAMES = {}


def generic_frame(name, N, H, W):
    """(sources, grid of the frame's values) of a frame only head_fwd_kernel / wgrad1x1_kernel take, drawn once per
    (name, shape): "C<n>" one BN+ReLU source of n channels (no fast shape); "raw16" a RAW source at a fast C;
    "two_6+10" BN+ReLU (6) and RAW (10) concatenated; "max2" / "avg2ceil" a pooled BN+ReLU source of 8 channels (the
    odd last row / column ignored; windows of 4, 2 and 1 elements); "offset" a source of (H - 2) x (W - 1) placed at
    (1, 1), zeros in rows 0 and H - 1 and in column 0."""
    key = (name, N, H, W)
    if key in _FRAMES:
        return _FRAMES[key]
    assert name in GENERIC_FRAMES and (name != "offset" or (H > 2 and W > 1))
    gen = torch.Generator().manual_seed(9100 + 31 * GENERIC_FRAMES.index(name) + 7 * H + W)

    def bnrelu(Hs, Ws, C, pool=POOL_NONE, off=(0, 0)):
        return S(quant_z(N, Hs, Ws, C, gen), SRC_BNRELU, quant_bn(C, gen), None, pool, off)
    if name[0] == "C":
        assert not fast_shape(int(name[1:]))
        out = [bnrelu(H, W, int(name[1:]))], U_A
    elif name == "raw16":
        out = [S(quant_grad((N, H, W, 16), gen))], 2.0 ** -4
    elif name == "two_6+10":
        out = [bnrelu(H, W, 6), S(quant_grad((N, H, W, 10), gen))], U_A
    elif name == "max2":
        out = [bnrelu(2 * H + 1, 2 * W + 1, 8, POOL_MAX2)], U_A
    elif name == "avg2ceil":
        out = [bnrelu(2 * H - 1, 2 * W - 1, 8, POOL_AVG2CEIL)], U_A / 4
    else:
        out = [bnrelu(H - 2, W - 1, 12, off=(1, 1))], U_A
    _FRAMES[key] = out
    return out


# ------------------------------------------------------------------------------------------ backward
Grads = namedtuple("Grads", "dy y w ug")


def grads(N, K, H, W, C, sig, fine=False):
    """dy, y (N, K, H, W), w (K, C) and the grid of g = dy * y * (1 - y) (sig) or dy.  fine: dy on multiples of 2^-4."""
    g = torch.Generator().manual_seed((((N * 149 + H) * 151 + W) * 17 + K) * 521 + C + (3 if sig else 0) + (5 if fine else 0))
    shape = (N, K, H, W)
    dy = (torch.randint(-32, 33, shape, generator=g).float() / 16 if fine
          else torch.randint(-8, 9, shape, generator=g).float() / 4)
    levels = torch.tensor([0.0, 0.25, 0.5, 0.75, 1.0]) if K <= 4 else torch.tensor([0.0, 0.5, 1.0])
    y = levels[torch.randint(0, len(levels), shape, generator=g)]
    w = torch.randint(-2, 3, (K, C), generator=g).float() / 2
    ug = (2.0 ** -4 if fine else 2.0 ** -2) * ((2.0 ** -4 if K <= 4 else 2.0 ** -2) if sig else 1.0)
    return Grads(dy, y, w, ug)


def ref_g(gr, sig):
    """dl in float64: dy * (y * (1 - y)) or dy."""
    dy, y = gr.dy.double(), gr.y.double()
    g = dy * (y * (1.0 - y)) if sig else dy
    assert torch.equal(g / gr.ug, (g / gr.ug).round())
    return g


def ref_da(g64, w, ug, where):
    """da (N, H, W, C) = sum_k g_k w[k] in float64, a multiple of ug / 2."""
    w64 = w.double()
    da = torch.einsum("nkhw,kc->nhwc", g64, w64)
    _note("da", exact_headroom(torch.einsum("nkhw,kc->nhwc", g64.abs(), w64.abs()), ug / 2, where + ": da"))
    return da


def ref_part(da64, l, ug, where):
    """The BN+ReLU backward sums per 2048-pixel block, (R, 2, C) float64; headroom asserted for both."""
    part, absp = ref_bn_bwd_sums(da64, l.z, l.coef, l.mean, l.invstd, rows_head(l.N, l.H, l.W))
    _note("sum g", exact_headroom(absp[:, 0], ug / 2, where + ": sum g"))
    _note("sum g * xhat", exact_headroom(absp[:, 1], ug / 2 * U_X, where + ": sum g * xhat"))
    return part


def ref_wgrad(g64, a64, ppb, ug, ua, where):
    """(dw (K, C), db (K,)) in float64 over the whole map; the headroom of dw and db asserted per block of ppb pixels
    (a block's fp32 slab is then exact, and so is the fp64 sum of the slabs)."""
    K, C = g64.shape[1], a64.shape[3]
    gp, ap = g64.permute(0, 2, 3, 1).reshape(-1, K), a64.reshape(-1, C)
    for p0 in range(0, gp.shape[0], ppb):
        gb, ab = gp[p0:p0 + ppb].abs(), ap[p0:p0 + ppb].abs()
        _note("dw", exact_headroom(gb.t() @ ab, ug * ua, where + f": dw, block {p0 // ppb}"))
        _note("db", exact_headroom(gb.sum(0), ug, where + f": db, block {p0 // ppb}"))
    return gp.t() @ ap, gp.sum(0)


def ref_dz(l, da64):
    """The last layer's dz: ref_frame of Src(da, BNBWD, bcoef, z); an fp32 number everywhere."""
    dz = ref_frame([S(da64, SRC_BNBWD, l.bcoef, l.z)], l.N, l.H, l.W)
    assert torch.equal(dz.float().double(), dz)
    return dz


# ------------------------------------------------------------------------------------------ case lists
# pmu_head1x1_fwd, fast path: every fast C at K = 1 (HU = 4) and 3; every K at C = 8, 64
FWD_FAST = sorted({(C, K) for C in FAST_C for K in (1, 3)} | {(C, K) for C in (8, 64) for K in range(1, 9)})
FWD_FAST_GEOM = [(4, 1), (8, 3), (64, 1), (256, 3)]
# pmu_head1x1_bwd: fast at C = 4, 256; generic at C = 1, 5 (scalar stores), 20, 260 (float4 stores)
BWD = [(C, K) for C in (4, 256, 1, 5, 20, 260) for K in (1, 8)]
# pmu_head1x1_bwd_bnr: every K with both sigmoid settings at C = 16 (all 32 head_dispatch instantiations with and
# without the da store); every fast C at K = 3
BNR = [(16, K, s) for K in range(1, 9) for s in (0, 1)] + [(C, 3, s) for C in FAST_C if C != 16 for s in (0, 1)]
BNR_GEOM = [(8, 3, 1), (64, 1, 0)]
# pmu_head1x1_bwd_dz: every K with both sigmoid settings at C = 16; every fast C at K = 2
DZ = [(16, K, s) for K in range(1, 9) for s in (0, 1)] + [(C, 2, s) for C in FAST_C if C != 16 for s in (0, 1)]
DZ_GEOM = [(8, 2, 1), (64, 1, 0)]
# pmu_head1x1_fwd, generic path: (geometry, frame, K)
FWD_GENERIC = [(geom, name, K) for geom in (SMALL, RAGGED) for name in GENERIC_FRAMES if name != "C255"
               for K in (1, 8)]
# pmu_wgrad1x1: (geometry, frame, K); "fast<C>[_xbf]" is the fast path's single BN+ReLU source (x stored as bf16)
WGRAD = [(RAGGED, "fast8", 3), (RAGGED, "fast256", 8), (RAGGED, "fast64_xbf", 1), (SMALL, "fast8", 1), (ONE, "fast8", 3),
         (OVER, "fast64_xbf", 2), (RAGGED, "C6", 3), (RAGGED, "C255", 8), (RAGGED, "two_6+10", 1), (RAGGED, "max2", 5),
         (SMALL, "C6", 1), (OVER, "C1", 2), (DEEP, "fast8", 3), (DEEP, "C6", 3)]


def wgrad_sources(name, N, H, W):
    """(sources, grid of the frame's values, x stored as bf16, pixels per block) of a WGRAD case."""
    if name.startswith("fast"):
        C = int(name[4:].split("_")[0])
        return [act_src(layer(N, H, W, C))], U_A, name.endswith("_xbf"), HPPB
    return generic_frame(name, N, H, W) + (False, W1_PPB)
