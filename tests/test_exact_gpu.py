"""The kernels the default dispatch launches, held to the float64 reference bit for bit.

A bf16 MFMA multiplies bf16 values exactly and adds in fp32; F(2x2)'s transforms use 0, +-1, +-1/2; the
first-layer kernel is fp32 FMAs; F(4x4)'s U = G g G^T is formed in double and rounded once.  On operands
that are bf16 numbers on a coarse grid (helpers.grid_data / grid_stats / grid_f4), with every sum of
absolute terms below 2^24 units of the result grid (checked per case from the reference alone,
helpers.exact_headroom — tests/test_exact_cpu.py runs the same check without a GPU), every partial sum of
every summation order is an fp32 number, so a correct kernel returns the float64 reference exactly:
a dropped tap, a mis-addressed border pixel, a stale LDS unit or a ragged-block slip shows at full
precision at a known (n, h, w, c).

Every output starts as NaN (0xFFFF for bf16 bits) and must be written; every case runs twice and must
repeat its bits; every workspace has its queried size plus a 4096-byte 0xA5 guard that must come back
untouched; BN partial rows are allocated with one extra NaN row that must stay NaN.

Shapes: the smallest that leave a partial tile in every tiled dimension of the kernel (rows, columns,
output-channel block, reduction chunk), plus one whole-tile case per family.  Tile constants, from csrc/:
  conv3x3_bf16_dma   16 x 32 pixels, 64 output channels (128 when NOUT > 64 and the reduction > 128), 16-channel chunks
  conv3x3_bf16_raw   256 pixels, 32 / 16 / 8 wide (W > 16 / > 8 / else), 64 output channels, 32-channel chunks
  conv3x3_bf16       as _raw with 16-channel chunks
  wgrad3x3_bf16_dma  16-pixel strips, 32 x 32 channel fragments;  wgrad3x3_bf16: 64 input channels per block
  convT_bf16_dma     GEMM rows = input pixels in blocks of 256 / 512, 32-channel chunks
  conv3x3_wino2h     16 x 16 pixels, 64 output channels, 8-channel chunks;  conv3x3_wino: 32 output, 16-channel chunks
  wgrad3x3_wino      8 x 16 pixel K-tiles, 32 x 64 channels
  conv3x3_wino4      32 x 32 pixels, 32 output channels, 8-channel chunks
  conv_first         8 x 32 pixels
"""
import ctypes
import functools
import zlib
from types import SimpleNamespace as NS

import pytest
import torch
import torch.nn.functional as TF

from helpers import (POOL_MAX2, POOL_NONE, SRC_BNBWD, SRC_BNRELU, SRC_RAW, assert_exact, bf16_exact, exact_headroom, grid_data,
                     grid_f4, grid_stats, quant_bn, quant_z, ref_frame, wino_conv, wino_wgrad)

pytestmark = pytest.mark.gpu

GUARD = 4096
_GRIDS = {"data": grid_data, "stats": grid_stats, "f4": grid_f4}


# ---------------------------------------------------------------------------------------------------
# cases: inputs, float64 references and conditions, on the CPU, computed once per argument set
# ---------------------------------------------------------------------------------------------------
def _grid(name, *key):
    return _GRIDS[name](zlib.crc32(repr((name,) + key).encode()))


def _nchw(t):
    return t.permute(0, 3, 1, 2)


def _nhwc(t):
    return t.permute(0, 2, 3, 1).contiguous()


def _wino_unit(g, wino):
    """Grid of the Winograd-domain values: F(2x2)'s G halves twice; F(4x4) on grid_f4 works in 2^-10."""
    return g.unit / 4 if wino == 2 else 2.0 ** -10


@functools.lru_cache(maxsize=None)
def fwd_case(grid, N, H, W, Cin, Cout, wino=0):
    """3x3 / pad 1 forward: x NHWC, w, b, z64 NHWC.  Conditions: sum |x| |w| + |b| per output; on grid_stats
    also sum |z| and sum z^2 per channel (the BN partial sums); wino: the Winograd restatement on
    absolute values."""
    g = _grid(grid, "fwd", N, H, W, Cin, Cout)
    x, w, b = g.operand(N, H, W, Cin), g.weight(Cout, Cin, 3, 3), g.bias(Cout)
    xc, wd, bd = _nchw(x).double(), w.double(), b.double()
    z64 = _nhwc(TF.conv2d(xc, wd, bd, padding=1))
    where = f"fwd {grid} {(N, H, W, Cin, Cout)}"
    cond = {"z": exact_headroom(TF.conv2d(xc.abs(), wd.abs(), bd.abs(), padding=1), g.unit, where)}
    if grid == "stats":
        cond["sum z"] = exact_headroom(z64.abs().sum((0, 1, 2)), g.unit, where + " sum z")
        cond["sum z^2"] = exact_headroom((z64 * z64).sum((0, 1, 2)), g.unit ** 2, where + " sum z^2")
    if wino:
        bound = wino_conv(wino, xc, wd, absolute=True) + bd.abs()[None, :, None, None]
        cond[f"F({wino}x{wino})"] = exact_headroom(bound, _wino_unit(g, wino), where + " winograd")
    return NS(x=x, w=w, b=b, z64=z64, cond=cond, grid=g)


def _flip(w):
    """The input gradient as a forward conv: weights [Cin][Cout][3][3], taps rotated by 180 degrees."""
    return w.flip(2, 3).transpose(0, 1).contiguous()


@functools.lru_cache(maxsize=None)
def dgrad_case(grid, N, H, W, Cin, Cout, wino=0, bnr=False, xb=False):
    """3x3 input gradient: dz NHWC (Cout channels), w, dx64 NHWC (Cin channels).  bnr: also the producer
    layer's z (quant_z), [scale | shift] and mean (quant_bn) and invstd in {1/2, 1, 2}, with the float64
    sums (sum g, sum g xhat) per channel, g = dx where z scale + shift > 0, xhat = (z - mean) invstd.
    xb (the *_dxb entries): dxr, dx rounded to bf16 (RNE; still on the result grid, a coarser multiple of its
    unit), and the column sums (grid_stats) and the bnr sums taken over dxr instead of dx."""
    g = _grid(grid, "dgrad", N, H, W, Cin, Cout)
    dz, w = g.operand(N, H, W, Cout), g.weight(Cout, Cin, 3, 3)
    dzc, wd = _nchw(dz).double(), w.double()
    dx64 = _nhwc(torch.nn.grad.conv2d_input((N, Cin, H, W), wd, dzc, padding=1))
    where = f"dgrad {grid} {(N, H, W, Cin, Cout)}"
    absdx = _nhwc(torch.nn.grad.conv2d_input((N, Cin, H, W), wd.abs(), dzc.abs(), padding=1))
    cond = {"dx": exact_headroom(absdx, g.unit, where)}
    if wino:
        bound = wino_conv(wino, dzc, _flip(wd), absolute=True)
        cond[f"F({wino}x{wino})"] = exact_headroom(bound, _wino_unit(g, wino), where + " winograd")
    c = NS(dz=dz, w=w, dx64=dx64, cond=cond, grid=g)
    dxs = dx64            # (dx itself is exact by the conditions above: the sums below add its actual values)
    if xb:
        dxs = c.dxr = dx64.float().to(torch.bfloat16).double()
    absdx = dxs.abs()
    if grid == "stats":
        c.col = dxs.sum((0, 1, 2))
        cond["sum dx"] = exact_headroom(absdx.sum((0, 1, 2)), g.unit, where + " column sums")
    if bnr:
        gen = g.gen
        c.z = quant_z(N, H, W, Cin, gen)
        bn = quant_bn(Cin, gen, bwd=True)
        c.coef, c.mean = bn[:2 * Cin].clone(), bn[2 * Cin:3 * Cin].clone()
        c.invstd = torch.tensor([0.5, 1.0, 2.0])[torch.randint(0, 3, (Cin,), generator=gen)]
        zd = c.z.double()
        mask = (zd * c.coef[:Cin].double() + c.coef[Cin:].double()) > 0
        xhat = (zd - c.mean.double()) * c.invstd.double()       # multiples of 2^-5
        gg = dxs * mask
        c.s1, c.s2 = gg.sum((0, 1, 2)), (gg * xhat).sum((0, 1, 2))
        cond["sum g"] = exact_headroom((absdx * mask).sum((0, 1, 2)), g.unit, where + " sum g")
        cond["sum g xhat"] = exact_headroom((absdx * mask * xhat.abs()).sum((0, 1, 2)), g.unit * 2.0 ** -5,
                                            where + " sum g xhat")
    return c


@functools.lru_cache(maxsize=None)
def wgrad_case(grid, N, H, W, Cin, Cout, wino=False):
    """3x3 weight gradient: x (Cin) and dz (Cout) NHWC, dw64 [Cout][Cin][3][3]."""
    g = _grid(grid, "wgrad", N, H, W, Cin, Cout)
    x, dz = g.operand(N, H, W, Cin), g.operand(N, H, W, Cout)
    xc, dzc = _nchw(x).double(), _nchw(dz).double()
    dw64 = torch.nn.grad.conv2d_weight(xc, (Cout, Cin, 3, 3), dzc, padding=1)
    where = f"wgrad {grid} {(N, H, W, Cin, Cout)}"
    unit = g.ux * g.ux
    cond = {"dw": exact_headroom(torch.nn.grad.conv2d_weight(xc.abs(), (Cout, Cin, 3, 3), dzc.abs(), padding=1), unit, where)}
    if wino:
        cond["F(2x2)"] = exact_headroom(wino_wgrad(xc, dzc, absolute=True), unit / 4, where + " winograd")
    return NS(x=x, dz=dz, dw64=dw64, cond=cond, grid=g)


def _hd(H, o):
    return 2 * H + o + (1 if o else 0)


@functools.lru_cache(maxsize=None)
def convT_case(grid, N, H, W, Cin, Cout, oh=0, ow=0):
    """ConvTranspose2d(k 2, s 2): x NHWC (Cin), w [Cin][Cout][2][2], b, u64 (N, 2H, 2W, Cout); backward from du
    (N, Hd, Wd, Cout) whose region at (oh, ow) is the conv's output: dx64, dw64, db64."""
    g = _grid(grid, "convT", N, H, W, Cin, Cout, oh, ow)
    x, w, b = g.operand(N, H, W, Cin), g.weight(Cin, Cout, 2, 2), g.bias(Cout)
    du = g.operand(N, _hd(H, oh), _hd(W, ow), Cout)
    xc, wd, bd = _nchw(x).double(), w.double(), b.double()
    u64 = _nhwc(TF.conv_transpose2d(xc, wd, bd, stride=2))
    dui = _nchw(du[:, oh:oh + 2 * H, ow:ow + 2 * W]).double()
    dx64 = _nhwc(TF.conv2d(dui, wd, stride=2))
    dr = _nhwc(dui).reshape(N, H, 2, W, 2, Cout)
    dw64 = torch.einsum("nijc,niajbk->ckab", x.double(), dr)
    db64 = dui.sum((0, 2, 3))
    where = f"convT {grid} {(N, H, W, Cin, Cout, oh, ow)}"
    cond = {"u": exact_headroom(TF.conv_transpose2d(xc.abs(), wd.abs(), bd.abs(), stride=2), g.unit, where + " u"),
            "dx": exact_headroom(TF.conv2d(dui.abs(), wd.abs(), stride=2), g.unit, where + " dx"),
            "dw": exact_headroom(torch.einsum("nijc,niajbk->ckab", x.double().abs(), dr.abs()), g.ux * g.ux, where + " dw"),
            "dbias": exact_headroom(dui.abs().sum((0, 2, 3)), g.ux, where + " dbias")}
    return NS(x=x, w=w, b=b, du=du, u64=u64, dx64=dx64, dw64=dw64, db64=db64, cond=cond, grid=g)


@functools.lru_cache(maxsize=None)
def first_case(grid, N, Cin, H, W, Cout):
    """First layer: x NCHW planes (Cin <= 4), w, b, z64 NHWC.  Its weight gradient from a raw dz source (the
    general kernel) and from a BN-backward source (da, z, [scale | shift | mean | kx | kc]: the tiled kernels
    of the default route) whose coefficients keep scale g + kx (z - mean) + kc on the grid of 2^-5: scale,
    shift and mean from quant_bn, kx in {0, +-1/2}, kc on multiples of 1/4."""
    g = _grid(grid, "first", N, Cin, H, W, Cout)
    x, w, b = g.operand(N, Cin, H, W), g.weight(Cout, Cin, 3, 3), g.bias(Cout)
    dz = g.operand(N, H, W, Cout)
    xd, wd, bd, dzc = x.double(), w.double(), b.double(), _nchw(dz).double()
    z64 = _nhwc(TF.conv2d(xd, wd, bd, padding=1))
    dw64 = torch.nn.grad.conv2d_weight(xd, (Cout, Cin, 3, 3), dzc, padding=1)
    where = f"first {grid} {(N, Cin, H, W, Cout)}"
    gen = g.gen
    zb = quant_z(N, H, W, Cout, gen)
    bn = quant_bn(Cout, gen, bwd=True)
    bn[3 * Cout:4 * Cout] = torch.randint(-1, 2, (Cout,), generator=gen).float() / 2
    bn[4 * Cout:] = torch.randint(-2, 3, (Cout,), generator=gen).float() / 4
    src = NS(x=dz, mode=SRC_BNBWD, coef=bn, z=zb, pool=POOL_NONE, off=(0, 0))
    dzb64 = ref_frame([src], N, H, W)
    assert bool(((dzb64 * 32).round() == dzb64 * 32).all())
    dwb64 = torch.nn.grad.conv2d_weight(xd, (Cout, Cin, 3, 3), _nchw(dzb64), padding=1)
    cond = {"z": exact_headroom(TF.conv2d(xd.abs(), wd.abs(), bd.abs(), padding=1), g.unit, where),
            "dw": exact_headroom(torch.nn.grad.conv2d_weight(xd.abs(), (Cout, Cin, 3, 3), dzc.abs(), padding=1),
                                 g.ux * g.ux, where + " dw"),
            "dw bnbwd": exact_headroom(torch.nn.grad.conv2d_weight(xd.abs(), (Cout, Cin, 3, 3), _nchw(dzb64).abs(), padding=1),
                                       g.ux * 2.0 ** -5, where + " dw, BN-backward source")}
    if grid == "stats":
        cond["sum z"] = exact_headroom(z64.abs().sum((0, 1, 2)), g.unit, where + " sum z")
        cond["sum z^2"] = exact_headroom((z64 * z64).sum((0, 1, 2)), g.unit ** 2, where + " sum z^2")
    return NS(x=x, w=w, b=b, dz=dz, zb=zb, bn=bn, z64=z64, dw64=dw64, dwb64=dwb64, cond=cond, grid=g)


FRAME_UNIT = 2.0 ** -8   # BN+ReLU of quant_z / quant_bn: multiples of 2^-5 up to 3.5; grid_data weights: 2^-3


@functools.lru_cache(maxsize=None)
def frame_case(kind, N, H, W, Cin, Cout):
    """The fused-staging forward's operand as a frame of stored tensors: kind raw (grid_data values), bnrelu
    (quant_z through quant_bn's BN+ReLU), maxpool (the same, max-pooled from a (2H+1) x 2W map: floor mode)
    or concat ([BN+ReLU skip | raw up-sampled part one row short, two columns narrow, at offset (0, 1)]).
    op64 = helpers.ref_frame of the sources; it must be made of bf16 numbers."""
    g = _grid("data", "frame", kind, N, H, W, Cin, Cout)
    gen = g.gen
    if kind == "raw":
        srcs = [NS(x=g.operand(N, H, W, Cin), mode=SRC_RAW, coef=None, z=None, pool=POOL_NONE, off=(0, 0))]
    elif kind == "bnrelu":
        srcs = [NS(x=quant_z(N, H, W, Cin, gen), mode=SRC_BNRELU, coef=quant_bn(Cin, gen), z=None, pool=POOL_NONE, off=(0, 0))]
    elif kind == "maxpool":
        srcs = [NS(x=quant_z(N, 2 * H + 1, 2 * W, Cin, gen), mode=SRC_BNRELU, coef=quant_bn(Cin, gen), z=None,
                   pool=POOL_MAX2, off=(0, 0))]
    else:
        assert kind == "concat"
        c0 = Cin * 3 // 8
        srcs = [NS(x=quant_z(N, H, W, c0, gen), mode=SRC_BNRELU, coef=quant_bn(c0, gen), z=None, pool=POOL_NONE, off=(0, 0)),
                NS(x=g.operand(N, H - 1, W - 2, Cin - c0), mode=SRC_RAW, coef=None, z=None, pool=POOL_NONE, off=(0, 1))]
    op64 = ref_frame(srcs, N, H, W)
    assert bf16_exact(op64.float()) and bool((op64.float().double() == op64).all())
    w, b = g.weight(Cout, Cin, 3, 3), g.bias(Cout)
    z64 = _nhwc(TF.conv2d(_nchw(op64), w.double(), b.double(), padding=1))
    where = f"frame {kind} {(N, H, W, Cin, Cout)}"
    cond = {"z": exact_headroom(TF.conv2d(_nchw(op64).abs(), w.double().abs(), b.double().abs(), padding=1), FRAME_UNIT, where)}
    return NS(srcs=srcs, op64=op64, w=w, b=b, z64=z64, cond=cond, grid=g)


# (N, H, W, Cin, Cout[, split]); the last of each list is the whole-tile case
DMA_FWD = [(1, 33, 45, 32, 64), (2, 17, 40, 64, 96), (1, 33, 32, 128, 40), (1, 17, 33, 144, 160), (1, 16, 64, 64, 64)]
DMA_DGRAD = [(1, 33, 45, 32, 64, 32), (2, 17, 40, 64, 96, 64), (1, 33, 32, 128, 40, 128), (1, 32, 48, 96, 128, 32),
             (2, 17, 40, 128, 64, 64), (1, 17, 33, 160, 144, 64), (1, 16, 64, 64, 64, 64)]
# the epilogue forms of the input gradient (*_dxb, *_x1b_sum_dxb, *_bnr, *_bnr_dxb) at two ragged tile rows and
# columns and a ragged last channel block, in the 4-wave (64-channel) and the 8-wave (128-channel) workgroup
DMA_FORMS = [(1, 19, 40, 96, 32, 64), (1, 19, 40, 160, 144, 64)]
RAW = [(1, 33, 17, 40, 64), (2, 9, 7, 6, 10), (3, 12, 20, 128, 128), (1, 8, 32, 32, 64)]
RAW_SPLIT = {(3, 12, 20, 128, 128): 64}
FUSED = [(2, 9, 7, 6, 10), (2, 17, 33, 64, 64), (1, 8, 32, 16, 64)]
FUSED_FWD = ([("raw",) + s for s in FUSED] + [("bnrelu",) + s for s in FUSED[:2]] + [("maxpool",) + s for s in FUSED[:2]]
             + [("concat",) + FUSED[1]])
WGRAD_BF16 = [(3, 19, 21, 32, 64), (2, 24, 40, 64, 128), (1, 11, 7, 12, 20), (1, 16, 16, 64, 64)]
CONVT_FWD = [(3, 9, 7, 64, 32), (2, 13, 11, 96, 256), (2, 10, 9, 256, 32), (2, 16, 16, 64, 32)]
# the input gradient's GEMM has Cin columns, a multiple of 128 (pmu_convT2x2_dma_ok): the forward's Cin = 64 and
# 96 become 128 and 384; (N, H, W, Cin, Cout, oh, ow)
CONVT_DGRAD = [(3, 9, 7, 128, 32, 0, 0), (2, 13, 11, 384, 96, 1, 0), (2, 10, 9, 256, 32, 0, 1), (3, 5, 7, 128, 64, 1, 1),
               (2, 16, 16, 128, 32, 0, 0)]
CONVT_WGRAD = [(3, 9, 7, 64, 32, 1, 1), (2, 13, 11, 96, 256, 0, 1), (2, 10, 9, 256, 32, 1, 0), (2, 8, 8, 128, 64, 0, 0)]
W2H = [(1, 37, 45, 16, 40), (2, 20, 13, 64, 32), (1, 45, 37, 24, 16), (1, 17, 18, 24, 72), (1, 16, 32, 16, 64)]
W2H_SPLIT = {(1, 45, 37, 24, 16): 8}
WINO_FUSED = [(1, 37, 45, 20, 40), (1, 16, 16, 16, 32)]
WGRAD_WINO = [(2, 17, 33, 64, 64), (1, 9, 13, 128, 64), (1, 8, 16, 64, 32)]
W4_DGRAD = [(1, 35, 37, 40, 48, 40), (2, 32, 32, 64, 64, 32)]
FIRST = [(2, 3, 37, 45, 64), (3, 4, 9, 70, 16), (1, 1, 16, 64, 32)]   # (N, Cin, H, W, Cout)
BNR_DMA = (1, 17, 40, 64, 32)
X1B_SUM = (1, 17, 40, 96, 32, 64)
BNR_W2H = (1, 20, 13, 64, 32)
BNR_W4 = (1, 35, 37, 40, 48)


def all_conditions():
    """(label, thunk) for every case of this file: the thunk builds the case on the CPU, which asserts its
    conditions, and returns them (name -> largest sum of |terms| in units of the result grid)."""
    out = []

    def add(label, fn, *a, **kw):
        out.append((f"{label} {a}", lambda: fn(*a, **kw).cond))
    for s in DMA_FWD:
        add("fwd_dma data", fwd_case, "data", *s)
        add("fwd_dma stats", fwd_case, "stats", *s)
    for s in DMA_DGRAD:
        add("dgrad_dma", dgrad_case, "data", *s[:5])
    for s in RAW:
        add("fwd_raw data", fwd_case, "data", *s)
        add("fwd_raw stats", fwd_case, "stats", *s)
        add("dgrad_raw", dgrad_case, "data", *s)
    for s in FUSED_FWD:
        add("fwd_bf16", frame_case, *s)
    for s in FUSED:
        add("dgrad_bf16", dgrad_case, "data", *s)
    for s in WGRAD_BF16:
        add("wgrad_bf16", wgrad_case, "data", *s)
    for s in CONVT_FWD:
        add("convT fwd", convT_case, "data", *s)
    for s in CONVT_DGRAD + CONVT_WGRAD:
        add("convT bwd", convT_case, "data", *s)
    for s in W2H:
        add("wino2h fwd data", fwd_case, "data", *s, wino=2)
        add("wino2h fwd stats", fwd_case, "stats", *s, wino=2)
        add("wino2h dgrad", dgrad_case, "data", *s, wino=2)
    for s in WINO_FUSED:
        add("wino fwd data", fwd_case, "data", *s, wino=2)
        add("wino fwd stats", fwd_case, "stats", *s, wino=2)
        add("wino dgrad", dgrad_case, "data", *s, wino=2)
    for s in WGRAD_WINO:
        add("wgrad_wino", wgrad_case, "data", *s, wino=True)
    for s in W4_DGRAD:
        add("wino4 dgrad", dgrad_case, "f4", *s[:5], wino=4)
    for s in FIRST:
        add("first data", first_case, "data", *s)
        add("first stats", first_case, "stats", *s)
    add("dgrad_dma_bnr", dgrad_case, "stats", *BNR_DMA, bnr=True)
    add("dgrad_dma_x1b_sum", dgrad_case, "stats", *X1B_SUM[:5])
    for s in DMA_FORMS:
        add("dgrad_dma dxb", dgrad_case, "stats", *s[:5], xb=True)
        add("dgrad_dma bnr", dgrad_case, "stats", *s[:5], bnr=True)
        add("dgrad_dma bnr_dxb", dgrad_case, "stats", *s[:5], bnr=True, xb=True)
    add("dgrad_wino2h_bnr", dgrad_case, "stats", *BNR_W2H, wino=2, bnr=True)
    add("dgrad_wino4_bnr", dgrad_case, "f4", *BNR_W4, wino=4, bnr=True)
    return out


# ---------------------------------------------------------------------------------------------------
# GPU side
# ---------------------------------------------------------------------------------------------------
def _nan(dev, *shape):
    return torch.full(shape, float("nan"), device=dev)


def _ffff(dev, *shape):
    return torch.full(shape, -1, dtype=torch.int16, device=dev)


def _bits16(t, Cp, dev):
    """NHWC fp32 values that are bf16 numbers -> their bf16 bits, channels zero-padded to Cp."""
    assert bf16_exact(t)
    out = torch.zeros(*t.shape[:3], Cp, dtype=torch.bfloat16)
    out[..., :t.shape[3]] = t.to(torch.bfloat16)
    return out.view(torch.int16).to(dev)


def _pad(c, m):
    return (c + m - 1) // m * m


def _ws(nbytes, dev):
    """A workspace of exactly nbytes (NaN) with the guard behind it."""
    assert nbytes > 0 and nbytes % 4 == 0, nbytes
    buf = torch.full((nbytes + GUARD,), 0xA5, dtype=torch.uint8, device=dev)
    buf[:nbytes].view(torch.float32).fill_(float("nan"))
    return buf


def _guard_ok(buf, nbytes, where):
    assert bool((buf[nbytes:] == 0xA5).all()), f"{where}: wrote past its {nbytes}-byte workspace"


def _raw_bits(t):
    return t.view(torch.int32) if t.dtype == torch.float32 else t


def _twice(run):
    """run() allocates fresh NaN outputs, launches, synchronises and returns them: both calls' bits agree."""
    a, b = run(), run()
    for i, (u, v) in enumerate(zip(a, b)):
        if u is not None:
            assert torch.equal(_raw_bits(u), _raw_bits(v)), f"output {i}: the second call's bits differ from the first's"
    return a


def _check_part(part, R, C, z64, where, exact):
    """part: (R + 1, 2 C), the last row a canary.  Rows finite, the canary untouched; exact: their float64
    sums are sum z and sum z^2 per channel."""
    p = part.double().cpu()
    assert bool(torch.isnan(p[R]).all()), f"{where}: more partial rows written than the tiles query returns ({R})"
    assert bool(torch.isfinite(p[:R]).all()), f"{where}: a partial row was left unwritten"
    if exact:
        s = p[:R].view(R, 2, C).sum(0)
        zz = z64.reshape(-1, C)
        assert_exact(s[0], zz.sum(0), where + " part: sum z")
        assert_exact(s[1], (zz * zz).sum(0), where + " part: sum z^2")


def _cat(dx0, dx1):
    return dx0 if dx1 is None else torch.cat([dx0, dx1], dim=3)


def _dma_block(NOUT, KC):
    return 64 if NOUT <= 64 or _pad(KC, 16) <= 128 else 128


# ---- LDS-DMA bf16 conv --------------------------------------------------------------------------------
@pytest.mark.parametrize("grid", ["data", "stats"])
@pytest.mark.parametrize("N,H,W,Cin,Cout", DMA_FWD)
def test_conv3x3_fwd_dma_exact(dev, grid, N, H, W, Cin, Cout):
    from pmu_hip import _lib as L
    from pmu_hip.engine import pack_weights_dma
    c = fwd_case(grid, N, H, W, Cin, Cout)
    xt, w, b = _bits16(c.x, Cin, dev), c.w.to(dev), c.b.to(dev)
    assert L.lib().pmu_conv3x3_dma_ok(H, W, Cin, Cout, Cout) == 1
    wp = pack_weights_dma(w, False)
    R = L.lib().pmu_conv3x3_tiles_dma(N, H, W, Cout, Cin)

    def run():
        z, part = _nan(dev, N, H, W, Cout), _nan(dev, R + 1, 2 * Cout)
        L.call("pmu_conv3x3_fwd_dma", xt.data_ptr(), Cin, N, H, W, wp.data_ptr(), b.data_ptr(), Cout, z.data_ptr(),
               part.data_ptr(), L.stream())
        torch.cuda.synchronize()
        return z, part
    z, part = _twice(run)
    where = f"pmu_conv3x3_fwd_dma {grid} {(N, H, W, Cin, Cout)}"
    assert_exact(z, c.z64, where, tile=(16, 32), cblock=_dma_block(Cout, Cin))
    _check_part(part, R, Cout, c.z64, where, grid == "stats")


@pytest.mark.parametrize("N,H,W,Cin,Cout,split", DMA_DGRAD)
def test_conv3x3_dgrad_dma_exact(dev, N, H, W, Cin, Cout, split):
    from pmu_hip import _lib as L
    from pmu_hip.engine import pack_weights_dma
    c = dgrad_case("data", N, H, W, Cin, Cout)
    Cp = _pad(Cout, 16)    # (the operand's channels padded with zeros to the 16-channel chunk)
    dzt, w = _bits16(c.dz, Cp, dev), c.w.to(dev)
    assert L.lib().pmu_conv3x3_dma_ok(H, W, Cp, Cin, split) == 1
    wp = pack_weights_dma(w, True)

    def run():
        dx0 = _nan(dev, N, H, W, split)
        dx1 = _nan(dev, N, H, W, Cin - split) if split < Cin else None
        L.call("pmu_conv3x3_dgrad_dma", dzt.data_ptr(), Cp, N, H, W, wp.data_ptr(), Cin, split, dx0.data_ptr(),
               L.ptr(dx1), L.stream())
        torch.cuda.synchronize()
        return dx0, dx1
    dx0, dx1 = _twice(run)
    assert_exact(_cat(dx0, dx1), c.dx64, f"pmu_conv3x3_dgrad_dma {(N, H, W, Cin, Cout, split)}", tile=(16, 32),
                 cblock=_dma_block(Cin, Cout))


def _check_bnr(part, R, c, Cin, where):
    p = part.double().cpu()
    assert bool(torch.isnan(p[R]).all()), f"{where}: more partial rows written than the tiles query returns ({R})"
    assert bool(torch.isfinite(p[:R]).all()), f"{where}: a partial row was left unwritten"
    s = p[:R].view(R, 2, Cin).sum(0)
    assert_exact(s[0], c.s1, where + " part: sum g")
    assert_exact(s[1], c.s2, where + " part: sum g xhat")


def test_conv3x3_dgrad_dma_bnr_exact(dev):
    """The input gradient fused with the producer's BN+ReLU backward sums, on grid_stats: dx exact, and the
    float64 sums of the partial rows equal (sum g, sum g xhat) exactly."""
    from pmu_hip import _lib as L
    from pmu_hip.engine import pack_weights_dma
    N, H, W, Cin, Cout = BNR_DMA
    c = dgrad_case("stats", N, H, W, Cin, Cout, bnr=True)
    dzt, w = _bits16(c.dz, Cout, dev), c.w.to(dev)
    z, coef, mean, invstd = c.z.to(dev), c.coef.to(dev), c.mean.to(dev), c.invstd.to(dev)
    wp = pack_weights_dma(w, True)
    R = L.lib().pmu_conv3x3_tiles_dma(N, H, W, Cin, Cout)

    def run():
        dx, part = _nan(dev, N, H, W, Cin), _nan(dev, R + 1, 2 * Cin)
        L.call("pmu_conv3x3_dgrad_dma_bnr", dzt.data_ptr(), Cout, N, H, W, wp.data_ptr(), Cin, dx.data_ptr(), z.data_ptr(),
               coef.data_ptr(), mean.data_ptr(), invstd.data_ptr(), part.data_ptr(), L.stream())
        torch.cuda.synchronize()
        return dx, part
    dx, part = _twice(run)
    where = f"pmu_conv3x3_dgrad_dma_bnr {BNR_DMA}"
    assert_exact(dx, c.dx64, where, tile=(16, 32), cblock=64)
    _check_bnr(part, R, c, Cin, where)


def test_conv3x3_dgrad_dma_x1b_sum_exact(dev):
    """The concat-split input gradient that keeps only the bf16 copy of dx1 and per-tile column sums, with
    pmu_convT2x2_dbias_rows over them: dx0 exact, dx1b the RNE bf16 of the exact dx1, the sums of the rows
    and the reduced bias gradient equal to the float64 column sums, the second half of every row zero."""
    from pmu_hip import _lib as L
    from pmu_hip.engine import pack_weights_dma
    N, H, W, Cin, Cout, split = X1B_SUM
    Cup = Cin - split
    c = dgrad_case("stats", N, H, W, Cin, Cout)
    dzt, w = _bits16(c.dz, Cout, dev), c.w.to(dev)
    wp = pack_weights_dma(w, True)
    R = L.lib().pmu_conv3x3_tiles_dma(N, H, W, Cin, Cout)
    wsb = L.lib().pmu_convT2x2_dbias_rows_ws(Cup)

    def run():
        dx0, dx1b, part = _nan(dev, N, H, W, split), _ffff(dev, N, H, W, Cup), _nan(dev, R + 1, 2 * Cin)
        db, ws = _nan(dev, Cup), _ws(wsb, dev)
        L.call("pmu_conv3x3_dgrad_dma_x1b_sum", dzt.data_ptr(), Cout, N, H, W, wp.data_ptr(), Cin, split, dx0.data_ptr(),
               dx1b.data_ptr(), part.data_ptr(), L.stream())
        L.call("pmu_convT2x2_dbias_rows", part.data_ptr() + 4 * split, R, 2 * Cin, Cup, db.data_ptr(), ws.data_ptr(),
               L.stream())
        torch.cuda.synchronize()
        _guard_ok(ws, wsb, "pmu_convT2x2_dbias_rows")
        return dx0, dx1b, part, db
    dx0, dx1b, part, db = _twice(run)
    where = f"pmu_conv3x3_dgrad_dma_x1b_sum {X1B_SUM}"
    assert_exact(dx0, c.dx64[..., :split], where + " dx0", tile=(16, 32), cblock=64)
    want_b = c.dx64[..., split:].float().to(torch.bfloat16)
    assert_exact(dx1b.view(torch.bfloat16).float(), want_b.double(), where + " dx1b", tile=(16, 32), cblock=64)
    p = part.double().cpu()
    assert bool(torch.isnan(p[R]).all()) and bool((p[:R, Cin:] == 0).all())
    col = c.dx64.sum((0, 1, 2))
    assert_exact(p[:R, :Cin].sum(0), col, where + " part: column sums")
    assert_exact(db, col[split:], where + " pmu_convT2x2_dbias_rows")


@pytest.mark.parametrize("kind", ["dxb", "x1b_sum_dxb", "bnr", "bnr_dxb"])
@pytest.mark.parametrize("N,H,W,Cin,Cout,split", DMA_FORMS)
def test_conv3x3_dgrad_dma_forms_exact(dev, kind, N, H, W, Cin, Cout, split):
    """The input gradient's other epilogues in both workgroup shapes, on grid_stats: fp32 dx exact, bf16 dx the
    RNE bf16 of the exact dx, fp32-stored dx1 holding the rounded values, and the column sums / BN-backward
    sums of the partial rows equal to the float64 sums over the values that were stored."""
    from pmu_hip import _lib as L
    from pmu_hip.engine import pack_weights_dma
    bnr, xb = kind.startswith("bnr"), kind.endswith("dxb")
    c = dgrad_case("stats", N, H, W, Cin, Cout, bnr=bnr, xb=xb)
    Cp = _pad(Cout, 16)
    dzt, w = _bits16(c.dz, Cp, dev), c.w.to(dev)
    assert L.lib().pmu_conv3x3_dma_ok(H, W, Cp, Cin, Cin if bnr else split) == 1
    wp = pack_weights_dma(w, True)
    R = L.lib().pmu_conv3x3_tiles_dma(N, H, W, Cin, Cp)
    where = f"pmu_conv3x3_dgrad_dma_{kind} {(N, H, W, Cin, Cout, split)}"
    cblock = _dma_block(Cin, Cout)
    want = c.dxr if xb else c.dx64

    def bf(t):
        return t.view(torch.bfloat16).float()
    if bnr:
        z, coef, mean, invstd = c.z.to(dev), c.coef.to(dev), c.mean.to(dev), c.invstd.to(dev)

        def run():
            dx = _ffff(dev, N, H, W, Cin) if xb else _nan(dev, N, H, W, Cin)
            part = _nan(dev, R + 1, 2 * Cin)
            L.call("pmu_conv3x3_dgrad_dma_" + kind, dzt.data_ptr(), Cp, N, H, W, wp.data_ptr(), Cin, dx.data_ptr(),
                   z.data_ptr(), coef.data_ptr(), mean.data_ptr(), invstd.data_ptr(), part.data_ptr(), L.stream())
            torch.cuda.synchronize()
            return dx, part
        dx, part = _twice(run)
        assert_exact(bf(dx) if xb else dx, want, where, tile=(16, 32), cblock=cblock)
        _check_bnr(part, R, c, Cin, where)
        return
    Cup = Cin - split

    def run():
        dx0, part = _ffff(dev, N, H, W, split), _nan(dev, R + 1, 2 * Cin)
        if kind == "dxb":
            dx1 = _nan(dev, N, H, W, Cup)
            L.call("pmu_conv3x3_dgrad_dma_dxb", dzt.data_ptr(), Cp, N, H, W, wp.data_ptr(), Cin, split, dx0.data_ptr(),
                   dx1.data_ptr(), L.stream())
        else:
            dx1 = _ffff(dev, N, H, W, Cup)
            L.call("pmu_conv3x3_dgrad_dma_x1b_sum_dxb", dzt.data_ptr(), Cp, N, H, W, wp.data_ptr(), Cin, split,
                   dx0.data_ptr(), dx1.data_ptr(), part.data_ptr(), L.stream())
        torch.cuda.synchronize()
        return dx0, dx1, part
    dx0, dx1, part = _twice(run)
    assert_exact(bf(dx0), want[..., :split], where + " dx0", tile=(16, 32), cblock=cblock)
    assert_exact(dx1 if kind == "dxb" else bf(dx1), want[..., split:], where + " dx1", tile=(16, 32), cblock=cblock)
    if kind == "x1b_sum_dxb":
        p = part.double().cpu()
        assert bool(torch.isnan(p[R]).all()) and bool((p[:R, Cin:] == 0).all())
        assert_exact(p[:R, :Cin].sum(0), c.col, where + " part: column sums")


# ---- bf16 conv on a materialised operand ----------------------------------------------------------
def _raw_tile(W):
    tw = 32 if W > 16 else 16 if W > 8 else 8
    return 256 // tw, tw


@pytest.mark.parametrize("grid", ["data", "stats"])
@pytest.mark.parametrize("N,H,W,Cin,Cout", RAW)
def test_conv3x3_fwd_raw_exact(dev, grid, N, H, W, Cin, Cout):
    from pmu_hip import _lib as L
    from pmu_hip.engine import pack_weights_raw
    c = fwd_case(grid, N, H, W, Cin, Cout)
    Cp = _pad(Cin, 8)
    xt, w, b = _bits16(c.x, Cp, dev), c.w.to(dev), c.b.to(dev)
    wp = pack_weights_raw(w, False)
    R = L.lib().pmu_conv3x3_tiles_raw(N, H, W, Cout)

    def run():
        z, part = _nan(dev, N, H, W, Cout), _nan(dev, R + 1, 2 * Cout)
        L.call("pmu_conv3x3_fwd_raw", xt.data_ptr(), Cp, N, H, W, wp.data_ptr(), b.data_ptr(), Cout, z.data_ptr(),
               part.data_ptr(), L.stream())
        torch.cuda.synchronize()
        return z, part
    z, part = _twice(run)
    where = f"pmu_conv3x3_fwd_raw {grid} {(N, H, W, Cin, Cout)}"
    assert_exact(z, c.z64, where, tile=_raw_tile(W), cblock=64)
    _check_part(part, R, Cout, c.z64, where, grid == "stats")


@pytest.mark.parametrize("N,H,W,Cin,Cout", RAW)
def test_conv3x3_dgrad_raw_exact(dev, N, H, W, Cin, Cout):
    from pmu_hip import _lib as L
    from pmu_hip.engine import pack_weights_raw
    c = dgrad_case("data", N, H, W, Cin, Cout)
    split = RAW_SPLIT.get((N, H, W, Cin, Cout), Cin)
    Cp = _pad(Cout, 8)
    dzt, w = _bits16(c.dz, Cp, dev), c.w.to(dev)
    wp = pack_weights_raw(w, True)

    def run():
        dx0 = _nan(dev, N, H, W, split)
        dx1 = _nan(dev, N, H, W, Cin - split) if split < Cin else None
        L.call("pmu_conv3x3_dgrad_raw", dzt.data_ptr(), Cp, N, H, W, wp.data_ptr(), Cin, split, dx0.data_ptr(), L.ptr(dx1),
               L.stream())
        torch.cuda.synchronize()
        return dx0, dx1
    dx0, dx1 = _twice(run)
    assert_exact(_cat(dx0, dx1), c.dx64, f"pmu_conv3x3_dgrad_raw {(N, H, W, Cin, Cout, split)}", tile=_raw_tile(W), cblock=64)


# ---- bf16 conv that stages its frame itself -------------------------------------------------------
@pytest.mark.parametrize("kind,N,H,W,Cin,Cout", FUSED_FWD)
def test_conv3x3_fwd_bf16_exact(dev, kind, N, H, W, Cin, Cout):
    """z against the float64 conv of helpers.ref_frame's operand (BN+ReLU, floor-mode max-pool, concat with
    an offset source), and the tee against that operand's bf16 bits."""
    from pmu_hip import _lib as L
    from pmu_hip.engine import Src, frame_of, pack_weights_bf16
    c = frame_case(kind, N, H, W, Cin, Cout)
    srcs = [Src(s.x.to(dev), s.mode, None if s.coef is None else s.coef.to(dev), pool=s.pool, off=s.off) for s in c.srcs]
    w, b = c.w.to(dev), c.b.to(dev)
    wp = pack_weights_bf16(w, False)
    R = L.lib().pmu_conv3x3_tiles(N, H, W)
    Cp = _pad(Cin, 8)

    def run():
        z, part, tee = _nan(dev, N, H, W, Cout), _nan(dev, R + 1, 2 * Cout), _ffff(dev, N, H, W, Cp)
        L.call("pmu_conv3x3_fwd_bf16", frame_of(srcs, N, H, W), wp.data_ptr(), b.data_ptr(), Cout, z.data_ptr(),
               part.data_ptr(), tee.data_ptr(), L.stream())
        torch.cuda.synchronize()
        return z, part, tee
    z, part, tee = _twice(run)
    where = f"pmu_conv3x3_fwd_bf16 {kind} {(N, H, W, Cin, Cout)}"
    assert_exact(tee.view(torch.bfloat16)[..., :Cin].float(), c.op64, where + " tee", tile=_raw_tile(W), cblock=16)
    assert_exact(z, c.z64, where, tile=_raw_tile(W), cblock=64)
    _check_part(part, R, Cout, c.z64, where, False)


@pytest.mark.parametrize("N,H,W,Cin,Cout", FUSED)
def test_conv3x3_dgrad_bf16_exact(dev, N, H, W, Cin, Cout):
    from pmu_hip import _lib as L
    from pmu_hip.engine import Src, frame_of, pack_weights_bf16
    c = dgrad_case("data", N, H, W, Cin, Cout)
    split = 32 if Cin == 64 else Cin
    dz, w = c.dz.to(dev), c.w.to(dev)
    wp = pack_weights_bf16(w, True)
    Cp = _pad(Cout, 8)

    def run():
        dx0 = _nan(dev, N, H, W, split)
        dx1 = _nan(dev, N, H, W, Cin - split) if split < Cin else None
        tee = _ffff(dev, N, H, W, Cp)
        L.call("pmu_conv3x3_dgrad_bf16", frame_of([Src(dz)], N, H, W), wp.data_ptr(), Cin, split, dx0.data_ptr(),
               L.ptr(dx1), tee.data_ptr(), L.stream())
        torch.cuda.synchronize()
        return dx0, dx1, tee
    dx0, dx1, tee = _twice(run)
    where = f"pmu_conv3x3_dgrad_bf16 {(N, H, W, Cin, Cout, split)}"
    assert_exact(tee.view(torch.bfloat16)[..., :Cout].float(), c.dz.double(), where + " tee")
    assert_exact(_cat(dx0, dx1), c.dx64, where, tile=_raw_tile(W), cblock=64)


# ---- bf16 weight gradients ------------------------------------------------------------------------
@pytest.mark.parametrize("N,H,W,Cin,Cout", WGRAD_BF16)
def test_conv3x3_wgrad_bf16_exact(dev, N, H, W, Cin, Cout):
    """Both bf16 weight gradients (the LDS-DMA one where it takes the map: W >= 16) on the same operands."""
    from pmu_hip import _lib as L
    c = wgrad_case("data", N, H, W, Cin, Cout)
    xt, dzt = _bits16(c.x, _pad(Cin, 8), dev), _bits16(c.dz, _pad(Cout, 8), dev)
    where = f"{(N, H, W, Cin, Cout)}"
    wsb = L.lib().pmu_conv3x3_wgrad_ws_bf16(N, H, W, Cin, Cout)

    def run():
        dw, ws = _nan(dev, Cout, Cin, 3, 3), _ws(wsb, dev)
        L.call("pmu_conv3x3_wgrad_bf16", dzt.data_ptr(), xt.data_ptr(), N, H, W, Cout, Cin, dw.data_ptr(), ws.data_ptr(),
               wsb, L.stream())
        torch.cuda.synchronize()
        _guard_ok(ws, wsb, "pmu_conv3x3_wgrad_bf16 " + where)
        return (dw,)
    assert_exact(_twice(run)[0], c.dw64, "pmu_conv3x3_wgrad_bf16 " + where)
    if not L.lib().pmu_conv3x3_wgrad_dma_ok(N, H, W, Cin, Cout):
        assert W < 16
        return
    wsd = L.lib().pmu_conv3x3_wgrad_ws_bf16_dma(N, H, W, Cin, Cout)

    def run_dma():
        dw, ws = _nan(dev, Cout, Cin, 3, 3), _ws(wsd, dev)
        L.call("pmu_conv3x3_wgrad_bf16_dma", dzt.data_ptr(), xt.data_ptr(), N, H, W, Cout, Cin, dw.data_ptr(),
               ws.data_ptr(), wsd, L.stream())
        torch.cuda.synchronize()
        _guard_ok(ws, wsd, "pmu_conv3x3_wgrad_bf16_dma " + where)
        return (dw,)
    assert_exact(_twice(run_dma)[0], c.dw64, "pmu_conv3x3_wgrad_bf16_dma " + where)


# ---- bf16 transposed conv -------------------------------------------------------------------------
@pytest.mark.parametrize("N,H,W,Cin,Cout", CONVT_FWD)
def test_convT_fwd_dma_exact(dev, N, H, W, Cin, Cout):
    from pmu_hip import _lib as L
    from pmu_hip.engine import pack_convT_weights_dma
    c = convT_case("data", N, H, W, Cin, Cout)
    assert L.lib().pmu_convT2x2_dma_ok(Cin, Cout, 0) == 1
    xt, w, b = _bits16(c.x, Cin, dev), c.w.to(dev), c.b.to(dev)
    wp = pack_convT_weights_dma(w, False)

    def run():
        u = _nan(dev, N, 2 * H, 2 * W, Cout)
        L.call("pmu_convT2x2_fwd_dma", xt.data_ptr(), Cin, N, H, W, wp.data_ptr(), b.data_ptr(), Cin, Cout, u.data_ptr(),
               L.stream())
        torch.cuda.synchronize()
        return (u,)
    assert_exact(_twice(run)[0], c.u64, f"pmu_convT2x2_fwd_dma {(N, H, W, Cin, Cout)}")


@pytest.mark.parametrize("N,H,W,Cin,Cout,oh,ow", CONVT_DGRAD)
def test_convT_dgrad_dma_exact(dev, N, H, W, Cin, Cout, oh, ow):
    from pmu_hip import _lib as L
    from pmu_hip.engine import pack_convT_weights_dma
    c = convT_case("data", N, H, W, Cin, Cout, oh, ow)
    assert L.lib().pmu_convT2x2_dma_ok(Cin, Cout, 1) == 1
    Hd, Wd = _hd(H, oh), _hd(W, ow)
    dut, w = _bits16(c.du, Cout, dev), c.w.to(dev)
    wp = pack_convT_weights_dma(w, True)

    def run():
        dx = _nan(dev, N, H, W, Cin)
        L.call("pmu_convT2x2_dgrad_dma", dut.data_ptr(), Cout, Hd, Wd, oh, ow, wp.data_ptr(), N, H, W, Cin, Cout,
               dx.data_ptr(), L.stream())
        torch.cuda.synchronize()
        return (dx,)
    assert_exact(_twice(run)[0], c.dx64, f"pmu_convT2x2_dgrad_dma {(N, H, W, Cin, Cout, oh, ow)}")


@pytest.mark.parametrize("N,H,W,Cin,Cout,oh,ow", CONVT_WGRAD)
def test_convT_wgrad_bf16_exact(dev, N, H, W, Cin, Cout, oh, ow):
    from pmu_hip import _lib as L
    c = convT_case("data", N, H, W, Cin, Cout, oh, ow)
    Hd, Wd = _hd(H, oh), _hd(W, ow)
    xt, dut, du = _bits16(c.x, Cin, dev), _bits16(c.du, Cout, dev), c.du.to(dev)
    wsb = L.lib().pmu_convT2x2_wgrad_ws_bf16(N, H, W, Cin, Cout)
    where = f"pmu_convT2x2_wgrad_bf16 {(N, H, W, Cin, Cout, oh, ow)}"

    def run():
        dw, db, ws = _nan(dev, Cin, Cout, 2, 2), _nan(dev, Cout), _ws(wsb, dev)
        L.call("pmu_convT2x2_wgrad_bf16", xt.data_ptr(), dut.data_ptr(), du.data_ptr(), N, H, W, Hd, Wd, oh, ow, Cin, Cout,
               dw.data_ptr(), db.data_ptr(), ws.data_ptr(), wsb, L.stream())
        torch.cuda.synchronize()
        _guard_ok(ws, wsb, where)
        return dw, db
    dw, db = _twice(run)
    assert_exact(dw, c.dw64, where + " dw")
    assert_exact(db, c.db64, where + " dbias")


# ---- fp32 Winograd F(2x2) -------------------------------------------------------------------------
@pytest.mark.parametrize("grid", ["data", "stats"])
@pytest.mark.parametrize("N,H,W,Cin,Cout", W2H)
def test_conv3x3_fwd_wino2h_exact(dev, grid, N, H, W, Cin, Cout):
    from pmu_hip import _lib as L
    from pmu_hip.engine import pack_weights_wino2h
    c = fwd_case(grid, N, H, W, Cin, Cout, wino=2)
    x, w, b = c.x.to(dev), c.w.to(dev), c.b.to(dev)
    wp = pack_weights_wino2h(w, False)
    R = L.lib().pmu_conv3x3_tiles_wino2h(N, H, W)

    def run():
        z, part = _nan(dev, N, H, W, Cout), _nan(dev, R + 1, 2 * Cout)
        L.call("pmu_conv3x3_fwd_wino2h", x.data_ptr(), Cin, N, H, W, wp.data_ptr(), b.data_ptr(), Cout, z.data_ptr(),
               part.data_ptr(), L.stream())
        torch.cuda.synchronize()
        return z, part
    z, part = _twice(run)
    where = f"pmu_conv3x3_fwd_wino2h {grid} {(N, H, W, Cin, Cout)}"
    assert_exact(z, c.z64, where, tile=(16, 16), cblock=64)
    _check_part(part, R, Cout, c.z64, where, grid == "stats")


@pytest.mark.parametrize("N,H,W,Cin,Cout", W2H)
def test_conv3x3_dgrad_wino2h_exact(dev, N, H, W, Cin, Cout):
    from pmu_hip import _lib as L
    from pmu_hip.engine import pack_weights_wino2h
    c = dgrad_case("data", N, H, W, Cin, Cout, wino=2)
    split = W2H_SPLIT.get((N, H, W, Cin, Cout), Cin)
    dz, w = c.dz.to(dev), c.w.to(dev)
    wp = pack_weights_wino2h(w, True)

    def run():
        dx0 = _nan(dev, N, H, W, split)
        dx1 = _nan(dev, N, H, W, Cin - split) if split < Cin else None
        L.call("pmu_conv3x3_dgrad_wino2h", dz.data_ptr(), Cout, N, H, W, wp.data_ptr(), Cin, split, dx0.data_ptr(),
               L.ptr(dx1), L.stream())
        torch.cuda.synchronize()
        return dx0, dx1
    dx0, dx1 = _twice(run)
    assert_exact(_cat(dx0, dx1), c.dx64, f"pmu_conv3x3_dgrad_wino2h {(N, H, W, Cin, Cout, split)}", tile=(16, 16), cblock=64)


def test_conv3x3_dgrad_wino2h_bnr_exact(dev):
    from pmu_hip import _lib as L
    from pmu_hip.engine import pack_weights_wino2h
    N, H, W, Cin, Cout = BNR_W2H
    c = dgrad_case("stats", N, H, W, Cin, Cout, wino=2, bnr=True)
    dz, w = c.dz.to(dev), c.w.to(dev)
    z, coef, mean, invstd = c.z.to(dev), c.coef.to(dev), c.mean.to(dev), c.invstd.to(dev)
    wp = pack_weights_wino2h(w, True)
    R = L.lib().pmu_conv3x3_tiles_wino2h(N, H, W)

    def run():
        dx, part = _nan(dev, N, H, W, Cin), _nan(dev, R + 1, 2 * Cin)
        L.call("pmu_conv3x3_dgrad_wino2h_bnr", dz.data_ptr(), Cout, N, H, W, wp.data_ptr(), Cin, dx.data_ptr(), z.data_ptr(),
               coef.data_ptr(), mean.data_ptr(), invstd.data_ptr(), part.data_ptr(), L.stream())
        torch.cuda.synchronize()
        return dx, part
    dx, part = _twice(run)
    where = f"pmu_conv3x3_dgrad_wino2h_bnr {BNR_W2H}"
    assert_exact(dx, c.dx64, where, tile=(16, 16), cblock=64)
    _check_bnr(part, R, c, Cin, where)


@pytest.mark.parametrize("grid", ["data", "stats"])
@pytest.mark.parametrize("N,H,W,Cin,Cout", WINO_FUSED)
def test_conv3x3_fwd_wino_exact(dev, grid, N, H, W, Cin, Cout):
    """The F(2x2) forward that stages its frame itself (a raw source; Cin % 16 != 0 takes its general path)."""
    from pmu_hip import _lib as L
    from pmu_hip.engine import Src, frame_of, pack_weights_wino
    c = fwd_case(grid, N, H, W, Cin, Cout, wino=2)
    x, w, b = c.x.to(dev), c.w.to(dev), c.b.to(dev)
    wp = pack_weights_wino(w, False)
    R = L.lib().pmu_conv3x3_tiles_wino(N, H, W)

    def run():
        z, part, tee = _nan(dev, N, H, W, Cout), _nan(dev, R + 1, 2 * Cout), _nan(dev, N, H, W, Cin)
        L.call("pmu_conv3x3_fwd_wino", frame_of([Src(x)], N, H, W), wp.data_ptr(), b.data_ptr(), Cout, z.data_ptr(),
               part.data_ptr(), tee.data_ptr(), L.stream())
        torch.cuda.synchronize()
        return z, part, tee
    z, part, tee = _twice(run)
    where = f"pmu_conv3x3_fwd_wino {grid} {(N, H, W, Cin, Cout)}"
    assert_exact(tee, c.x.double(), where + " tee")
    assert_exact(z, c.z64, where, tile=(16, 16), cblock=32)
    _check_part(part, R, Cout, c.z64, where, grid == "stats")


@pytest.mark.parametrize("N,H,W,Cin,Cout", WINO_FUSED)
def test_conv3x3_dgrad_wino_exact(dev, N, H, W, Cin, Cout):
    from pmu_hip import _lib as L
    from pmu_hip.engine import Src, frame_of, pack_weights_wino
    c = dgrad_case("data", N, H, W, Cin, Cout, wino=2)
    split = 8 if Cin == 20 else Cin
    dz, w = c.dz.to(dev), c.w.to(dev)
    wp = pack_weights_wino(w, True)

    def run():
        dx0 = _nan(dev, N, H, W, split)
        dx1 = _nan(dev, N, H, W, Cin - split) if split < Cin else None
        tee = _nan(dev, N, H, W, Cout)
        L.call("pmu_conv3x3_dgrad_wino", frame_of([Src(dz)], N, H, W), wp.data_ptr(), Cin, split, dx0.data_ptr(),
               L.ptr(dx1), tee.data_ptr(), L.stream())
        torch.cuda.synchronize()
        return dx0, dx1, tee
    dx0, dx1, tee = _twice(run)
    where = f"pmu_conv3x3_dgrad_wino {(N, H, W, Cin, Cout, split)}"
    assert_exact(tee, c.dz.double(), where + " tee")
    assert_exact(_cat(dx0, dx1), c.dx64, where, tile=(16, 16), cblock=32)


@pytest.mark.parametrize("N,H,W,Cin,Cout", WGRAD_WINO)
def test_conv3x3_wgrad_wino_exact(dev, N, H, W, Cin, Cout):
    from pmu_hip import _lib as L
    c = wgrad_case("data", N, H, W, Cin, Cout, wino=True)
    x, dz = c.x.to(dev), c.dz.to(dev)
    wsb = L.lib().pmu_conv3x3_wgrad_ws_wino(N, H, W, Cin, Cout)
    where = f"pmu_conv3x3_wgrad_wino {(N, H, W, Cin, Cout)}"

    def run():
        dw, ws = _nan(dev, Cout, Cin, 3, 3), _ws(wsb, dev)
        L.call("pmu_conv3x3_wgrad_wino", dz.data_ptr(), x.data_ptr(), N, H, W, Cout, Cin, dw.data_ptr(), ws.data_ptr(), wsb,
               L.stream())
        torch.cuda.synchronize()
        _guard_ok(ws, wsb, where)
        return (dw,)
    assert_exact(_twice(run)[0], c.dw64, where)


# ---- fp32 Winograd F(4x4) -------------------------------------------------------------------------
@pytest.mark.parametrize("N,H,W,Cin,Cout,split", W4_DGRAD)
def test_conv3x3_dgrad_wino4_exact(dev, N, H, W, Cin, Cout, split):
    """On grid_f4: weights that are multiples of 576 * 2^-10 make U = G g G^T integers of 2^-10."""
    from pmu_hip import _lib as L
    from pmu_hip.engine import pack_weights_wino4
    c = dgrad_case("f4", N, H, W, Cin, Cout, wino=4)
    dz, w = c.dz.to(dev), c.w.to(dev)
    wp = pack_weights_wino4(w, True)

    def run():
        dx0 = _nan(dev, N, H, W, split)
        dx1 = _nan(dev, N, H, W, Cin - split) if split < Cin else None
        L.call("pmu_conv3x3_dgrad_wino4", dz.data_ptr(), Cout, N, H, W, wp.data_ptr(), Cin, split, dx0.data_ptr(),
               L.ptr(dx1), L.stream())
        torch.cuda.synchronize()
        return dx0, dx1
    dx0, dx1 = _twice(run)
    assert_exact(_cat(dx0, dx1), c.dx64, f"pmu_conv3x3_dgrad_wino4 {(N, H, W, Cin, Cout, split)}", tile=(32, 32), cblock=32)


def test_conv3x3_dgrad_wino4_bnr_exact(dev):
    """dz and weights from grid_f4, not grid_stats: weights in {0, +-1/2, +-1} are not exact under F(4x4)'s G
    (sixths); z, mean and invstd as for the other fused reductions.  dx is a multiple of 9 * 2^-4 and
    g xhat of 9 * 2^-9, below 2^24 units of 2^-10 * 2^-5."""
    from pmu_hip import _lib as L
    from pmu_hip.engine import pack_weights_wino4
    N, H, W, Cin, Cout = BNR_W4
    c = dgrad_case("f4", N, H, W, Cin, Cout, wino=4, bnr=True)
    dz, w = c.dz.to(dev), c.w.to(dev)
    z, coef, mean, invstd = c.z.to(dev), c.coef.to(dev), c.mean.to(dev), c.invstd.to(dev)
    wp = pack_weights_wino4(w, True)
    R = L.lib().pmu_conv3x3_tiles_wino4(N, H, W)

    def run():
        dx, part = _nan(dev, N, H, W, Cin), _nan(dev, R + 1, 2 * Cin)
        L.call("pmu_conv3x3_dgrad_wino4_bnr", dz.data_ptr(), Cout, N, H, W, wp.data_ptr(), Cin, dx.data_ptr(), z.data_ptr(),
               coef.data_ptr(), mean.data_ptr(), invstd.data_ptr(), part.data_ptr(), L.stream())
        torch.cuda.synchronize()
        return dx, part
    dx, part = _twice(run)
    where = f"pmu_conv3x3_dgrad_wino4_bnr {BNR_W4}"
    assert_exact(dx, c.dx64, where, tile=(32, 32), cblock=32)
    _check_bnr(part, R, c, Cin, where)


# ---- first layer ------------------------------------------------------------------------------------
@pytest.mark.parametrize("grid", ["data", "stats"])
@pytest.mark.parametrize("N,Cin,H,W,Cout", FIRST)
def test_conv_first_exact(dev, grid, N, Cin, H, W, Cout):
    """pmu_conv_first_fwd (z, partial sums) and pmu_conv_first_wgrad on the same planes: from a raw dz source
    (its general kernel) and from a BN-backward source on the grid (the tiled kernels the default route runs)."""
    from pmu_hip import _lib as L
    from pmu_hip.engine import Src, frame_of
    c = first_case(grid, N, Cin, H, W, Cout)
    planes = [c.x[:, k].contiguous().to(dev) for k in range(Cin)]
    arr = (ctypes.c_void_p * Cin)(*[p.data_ptr() for p in planes])
    w, b, dz = c.w.to(dev), c.b.to(dev), c.dz.to(dev)
    bsrc = Src(dz, L.SRC_BNBWD, c.bn.to(dev), z=c.zb.to(dev))
    R = L.lib().pmu_conv_first_tiles(N, H, W)
    wsb = L.lib().pmu_conv_first_wgrad_ws(N, H, W, Cin, Cout)
    where = f"{grid} {(N, Cin, H, W, Cout)}"

    def run():
        z, part = _nan(dev, N, H, W, Cout), _nan(dev, R + 1, 2 * Cout)
        L.call("pmu_conv_first_fwd", arr, Cin, N, H, W, w.data_ptr(), b.data_ptr(), Cout, z.data_ptr(), part.data_ptr(),
               L.stream())
        dw, ws = _nan(dev, Cout, Cin, 3, 3), _ws(wsb, dev)
        L.call("pmu_conv_first_wgrad", frame_of([Src(dz)], N, H, W), arr, Cin, Cout, dw.data_ptr(), ws.data_ptr(), wsb,
               L.stream())
        dwb, wsd = _nan(dev, Cout, Cin, 3, 3), _ws(wsb, dev)
        L.call("pmu_conv_first_wgrad", frame_of([bsrc], N, H, W), arr, Cin, Cout, dwb.data_ptr(), wsd.data_ptr(), wsb,
               L.stream())
        torch.cuda.synchronize()
        _guard_ok(ws, wsb, "pmu_conv_first_wgrad " + where)
        _guard_ok(wsd, wsb, "pmu_conv_first_wgrad, BN-backward source " + where)
        return z, part, dw, dwb
    z, part, dw, dwb = _twice(run)
    assert_exact(z, c.z64, "pmu_conv_first_fwd " + where, tile=(8, 32))
    _check_part(part, R, Cout, c.z64, "pmu_conv_first_fwd " + where, grid == "stats")
    assert_exact(dw, c.dw64, "pmu_conv_first_wgrad " + where)
    assert_exact(dwb, c.dwb64, "pmu_conv_first_wgrad, BN-backward source " + where)
