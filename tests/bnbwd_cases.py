"""Inputs and float64 references of the fused BatchNorm+ReLU backward cases, shared by
tests/test_bnbwd_exact_gpu.py (which runs the kernels of csrc/bn.hip and csrc/pool_bwd.hip on them) and
tests/test_glue_exact_cpu.py (which checks, without a GPU, that every case satisfies the conditions of an exact
comparison).

Grids (helpers.py): z multiples of 2^-4 in [-1.5, 1.5] with deliberate ties (quant_z); scale, invstd in {0.5, 1, 2};
shift, mean multiples of 2^-4 in [-0.5, 0.5]; gradients multiples of 2^-4 in [-2, 2] (quant_grad).  Then
  * z * scale + shift is exact, so fp32 and fp64 agree on every ReLU mask and every max-pool winner;
  * da = skip + routed dpool is a multiple of 2^-4 (U_G) below 4;
  * xhat = (z - mean) * invstd is a multiple of 2^-5 below 4, g * xhat a multiple of 2^-9 (U_GX);
  * AvgPool2d(2, ceil_mode) backward divides by 4, 2 or 1: da multiples of 2^-6; the spatial mean's backward by
    H * W, a power of two — or 63 with dmean drawn as multiples of 63 * 2^-4, where IEEE division returns the
    exact quotient;
so every partial sum is exact as long as the sum of absolute values stays below 2^24 units (exact_headroom)."""
from collections import namedtuple

import torch

from helpers import (SRC_BNBWD, quant_bn, quant_grad, quant_invstd, quant_z, ref_bn_bwd_sums, ref_frame,
                     ref_maxpool_bwd, rows_bn_bwd, rows_maxpool_bwd)

U_G, U_X = 2.0 ** -4, 2.0 ** -5   # grids of the gradients and of xhat

# (N, H, W, C): plain; CQ = 24 (npg = 10, sixteen idle threads); CQ = 516 (three channel-quad rounds, the last
# with four quads); odd maps; several tiles with a ragged last one (ppb = 512, 4455 pixels); a single window
# (Hp - 1 = 0 clamps in mp_load); 3 x 2
SHAPES = [(2, 8, 8, 64), (1, 7, 9, 96), (1, 6, 8, 2064), (2, 9, 11, 192), (3, 33, 45, 32), (1, 2, 2, 8), (1, 3, 2, 4)]
# pmu_bn_bwd_reduce alone also takes C % 4 != 0 (bn_bwd_reduce1_kernel; one tile and two), P = 1 and P = ppb + 1
REDUCE_SHAPES = SHAPES + [(2, 9, 11, 6), (1, 7, 9, 3), (1, 3, 911, 6), (1, 1, 1, 64), (1, 1, 257, 64)]
# pmu_maxpool2_bwd_bnbwd{,_dxb}: C / 4 divides 256 or is a multiple of it
BNBWD_SHAPES = [(1, 2, 2, 8), (1, 3, 2, 8), (2, 8, 8, 64), (2, 9, 11, 64), (3, 33, 45, 64), (1, 7, 9, 1024),
                (1, 6, 8, 2048), (1, 5, 5, 2048)]
# pmu_spatial_mean_bwd_bnr: H * W = 32, 32 and 63
MEAN_SHAPES = [(2, 4, 8, 64), (1, 2, 16, 96), (2, 7, 9, 32)]

Inputs = namedtuple("Inputs", "N H W C z coef mean invstd da dpool skip bcoef dpool_avg dmean")
_CACHE = {}


def inputs(N, H, W, C):
    """The CPU fp32 tensors of one shape, drawn once (seeded by the shape) and never written to: z, coef =
    [scale | shift], mean, invstd; da (N, H, W, C), dpool (N, H // 2, W // 2, C) and skip (N, H, W, C) on the 2^-4
    grid; bcoef, an independent dyadic BN-backward block [scale | shift | mean | kx | kc]; dpool_avg (N, ceil(H / 2),
    ceil(W / 2), C); dmean (N, C) — multiples of 2^-4, times H * W when that is no power of two."""
    key = (N, H, W, C)
    if key not in _CACHE:
        g = torch.Generator().manual_seed(((N * 131 + H) * 131 + W) * 4099 + C)
        hw = H * W
        _CACHE[key] = Inputs(
            N, H, W, C, quant_z(N, H, W, C, g), quant_bn(C, g), torch.randint(-8, 9, (C,), generator=g).float() / 16,
            quant_invstd(C, g), quant_grad((N, H, W, C), g), quant_grad((N, H // 2, W // 2, C), g),
            quant_grad((N, H, W, C), g), quant_bn(C, g, bwd=True, dyadic=True),
            quant_grad((N, (H + 1) // 2, (W + 1) // 2, C), g),
            quant_grad((N, C), g) * (1.0 if hw & (hw - 1) == 0 else float(hw)))
    return _CACHE[key]


def avgpool_bwd(i):
    """AvgPool2d(2, 2, ceil_mode=True) backward in float64: da[n][h][w] = dpool[n][h // 2][w // 2] / (the number
    of in-bounds elements of that window)."""
    h, w = torch.arange(i.H), torch.arange(i.W)
    cnt = ((torch.clamp(2 * (h // 2) + 2, max=i.H) - 2 * (h // 2)).view(i.H, 1)
           * (torch.clamp(2 * (w // 2) + 2, max=i.W) - 2 * (w // 2)).view(1, i.W)).double()
    assert set(cnt.unique().tolist()) <= {1.0, 2.0, 4.0}
    return i.dpool_avg.double()[:, h // 2][:, :, w // 2] / cnt.view(1, i.H, i.W, 1)


def mean_bwd(i):
    """The spatial mean's backward in float64: da[n][h][w][c] = dmean[n][c] / (H * W)."""
    return (i.dmean.double() / (i.H * i.W)).view(i.N, 1, 1, i.C).expand(i.N, i.H, i.W, i.C).contiguous()


def da_of(kind, i):
    """(float64 da, rows, unit of sum g, unit of sum g * xhat) of one stats case.  kind: "reduce" (da given),
    "maxpool" (skip + routed dpool), "maxpool_noskip" (the routed dpool alone), "avgpool", "mean"."""
    if kind == "reduce":
        return i.da.double(), rows_bn_bwd(i.N, i.H, i.W, i.C), U_G, U_G * U_X
    if kind in ("maxpool", "maxpool_noskip"):
        da = ref_maxpool_bwd(i.dpool, i.skip if kind == "maxpool" else None, i.z, i.coef)
        return da, rows_maxpool_bwd(i.N, i.H, i.W, i.C), U_G, U_G * U_X
    if kind == "avgpool":
        return avgpool_bwd(i), rows_bn_bwd(i.N, i.H, i.W, i.C), U_G / 4, U_G / 4 * U_X
    assert kind == "mean"
    hw = i.H * i.W
    u = U_G / hw if hw & (hw - 1) == 0 else U_G
    return mean_bwd(i), rows_bn_bwd(i.N, i.H, i.W, i.C), u, u * U_X


def stats_cases():
    """Every (kind, shape) whose partial sums tests/test_bnbwd_exact_gpu.py compares."""
    out = [("reduce", s) for s in REDUCE_SHAPES]
    out += [(k, s) for k in ("maxpool", "maxpool_noskip", "avgpool") for s in SHAPES]
    out += [("maxpool", s) for s in BNBWD_SHAPES if s not in SHAPES]
    return out + [("mean", s) for s in MEAN_SHAPES]


def ref_sums(kind, i):
    """(da64, part64 (R, 2, C), the sums of absolute values (R, 2, C), unit of sum g, unit of sum g * xhat)."""
    da, rows, ug, ugx = da_of(kind, i)
    part, absp = ref_bn_bwd_sums(da, i.z, i.coef, i.mean, i.invstd, rows)
    return da, part, absp, ug, ugx


def ref_dz(i, da64):
    """The BN+ReLU backward of da with the dyadic bcoef: ref_frame of Src(da, BNBWD, bcoef, z)."""
    S = namedtuple("S", "x mode coef z pool off")
    return ref_frame([S(da64, SRC_BNBWD, i.bcoef, i.z, 0, (0, 0))], i.N, i.H, i.W)
