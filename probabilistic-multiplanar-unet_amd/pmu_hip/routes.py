"""Which kernel runs each conv: the one place the engine's dispatch policy is written down.

Pure functions of shapes and config: nothing here allocates, launches or touches torch.cuda.  The only
library calls are host-side shape predicates, so the table is checkable on a CPU with
``_lib._LIB = load_library()`` (tests/test_cpu_host.py).  engine.py asks, then allocates and launches.
The routes of a 3x3 conv are listed with FWD_ENTRY below.
"""
from __future__ import annotations

import ctypes
import os
from dataclasses import dataclass, replace

from . import _lib as L


@dataclass
class EngineConfig:
    """Implementation choices of the fp32 3x3 convs, read ONCE from the environment at import (never
    on the per-call hot path).  Tests switch them by assigning ``CFG``'s fields; the routes read them
    through effective(), which clamps what only an experiments build of the library honours.

    fp32_conv: "wino" (default: Winograd on materialised operands), "wino_fused" (the fused-staging
        Winograd kernels everywhere) or "direct" (direct-sum MFMA kernels) — PMU_FP32_CONV;
    wino4: where F(4x4,3x3) runs — "dgrad" (default: the input gradient of maps >= 32x32) or "0"
        (nowhere) — PMU_WINO4.  "1" (the forward too) breaks the model-level 1e-3 contract (see
        _wino4_ok) and is honoured only by an experiments build of the library (make EXPERIMENTS=1);
    bf16_z: bf16 mode (unet_forward) stores the LDS-DMA convs' pre-BN output z in bf16, centred on the
        BN running mean — the dtype torch.autocast gives a conv's output.  Off by default: it breaks
        the c5 Dice contract (eval Dice gap 6.8e-3 centred / 5.4e-3 uncentred vs 2.2e-4 with fp32 z,
        tests/test_bf16_gpu.py::test_c5_bf16_dice_gap_vs_fp32_oracle), so PMU_BF16_Z=1
        is honoured only by an experiments build of the library, as PMU_WINO4=1;
    dx_bf16: bf16 mode keeps the activation gradients the LDS-DMA input gradients produce inside the
        UNet backward in bf16 (the *_dxb entries) — the dtype torch.autocast's conv backward returns
        them in — and their consumers read them so (PMU_DX_BF16=0: fp32, the round-4 path);
    wgrad_dma: the bf16 weight gradient on the LDS-DMA strip kernel (pmu_conv3x3_wgrad_bf16_dma) where
        its shapes allow, else the register-staged one (PMU_WGRAD_DMA=0: always the latter);
    pool_fuse: a pooled layer's da (skip + routed pooled gradient, both bf16) is not stored: a
        stats-only pass forms its BN-backward partials and its bf16 dz is made from the two parts
        directly (PoolSumDa; PMU_POOL_FUSE=0: stored in fp32 and streamed, the round-5 path);
    head_fuse: the head's input gradient (the last layer's da) is not stored: the head backward forms
        the last layer's BN-backward partials and the head's weight gradient, and that layer's dz (bf16 or
        fp32) is made from dy directly (HeadDa; PMU_HEAD_FUSE=0: da stored, then streamed);
    prob_streams: the Probabilistic U-Net's forward runs its UNet, prior and posterior on three HIP
        streams (functions.run_concurrent; their backwards follow autograd's stream of the forward), so
        the parts' tile-starved deep layers and small launches overlap (PMU_PROB_STREAMS=0: one stream)."""
    fp32_conv: str = "wino"
    wino4: str = "dgrad"
    bf16_z: bool = False
    dx_bf16: bool = True
    wgrad_dma: bool = True
    pool_fuse: bool = True
    head_fuse: bool = True
    prob_streams: bool = True

    @classmethod
    def from_env(cls):
        env = os.environ.get
        return cls(fp32_conv=env("PMU_FP32_CONV", "wino"), wino4=env("PMU_WINO4", "dgrad"),
                   bf16_z=env("PMU_BF16_Z", "0") == "1", dx_bf16=env("PMU_DX_BF16", "1") != "0",
                   wgrad_dma=env("PMU_WGRAD_DMA", "1") != "0", pool_fuse=env("PMU_POOL_FUSE", "1") != "0",
                   head_fuse=env("PMU_HEAD_FUSE", "1") != "0", prob_streams=env("PMU_PROB_STREAMS", "1") != "0")


CFG = EngineConfig.from_env()


def effective() -> EngineConfig:
    """CFG as the loaded library honours it, evaluated per call (tests assign CFG's fields and swap the
    library mid-process).  The shipped library has only the default dispatch's kernels: it runs fp32_conv
    "direct" as "wino", wino4 "1" as "dgrad", and bf16_z never; an experiments build (make EXPERIMENTS=1)
    honours every switch."""
    c = CFG
    if L.experiments_build() or (c.fp32_conv != "direct" and c.wino4 != "1" and not c.bf16_z):
        return c   # (nothing to clamp: the usual case, no copy)
    return replace(c, fp32_conv="wino" if c.fp32_conv == "direct" else c.fp32_conv,
                   wino4="dgrad" if c.wino4 == "1" else c.wino4, bf16_z=False)


def pad8(c: int) -> int:
    return (c + 7) // 8 * 8


# ----------------------------------------------------------------------------------------
# shape rules of the kernels
# ----------------------------------------------------------------------------------------
def first_layer_ok(cin: int, cout: int) -> bool:
    """Shapes pmu_conv_first_fwd/_wgrad take (include/pmunet_hip.h): Cin <= 4, Cout = 4q with 256 % q == 0."""
    return 1 <= cin <= 4 and cout % 4 == 0 and 4 <= cout <= 1024 and 256 % (cout // 4) == 0 and cout <= 256


def pool_fuse_ok(C: int) -> bool:
    """Channel counts pmu_maxpool2_bwd_bnbwd_dxb takes: C % 4 == 0, C / 4 dividing 256 or a multiple of it."""
    q = C // 4
    return C % 4 == 0 and q > 0 and (256 % q == 0 if q < 256 else q % 256 == 0)


def dma_ok(H, W, Cp, NOUT, split) -> bool:
    """Shapes of the LDS-DMA bf16 conv (pmu_conv3x3_{fwd,dgrad}_dma): maps >= 32 wide, Cp % 16 == 0,
    a concat split on a 32-channel boundary."""
    return bool(L.lib().pmu_conv3x3_dma_ok(H, W, Cp, NOUT, split))


def raw_ok(N, H, W, Cp) -> bool:
    """Shapes the materialised-operand bf16 conv takes (pmu_conv3x3_fwd_raw / _dgrad_raw)."""
    return N * H * W * Cp < 2 ** 31


def dxb_ok(H, W, Cout, Cin, split) -> bool:
    """The conv's input gradient runs on the LDS-DMA kernel and may store dx in bf16 (the *_dxb entries):
    maps >= 32 wide, pad8(Cout) % 16 == 0, a concat split on a 32-channel boundary, Cin and the split
    multiples of 8.  oracle/unet_ref.py's _dma_dxb models the same rule (tests/test_cpu_host.py)."""
    return dma_ok(H, W, pad8(Cout), Cin, split) and Cin % 8 == 0 and split % 8 == 0


def _wino4_ok(cfg, C: int, H: int, W: int, kind: str) -> bool:
    """Winograd F(4x4,3x3) on a materialised operand (pmu_conv3x3_*_wino4): reduction channels C % 8 == 0
    and images of at least 32 x 32 (its blocks are 32 x 32 output pixels; smaller maps keep F(2x2)).
    Default: the input gradient only — in the forward its fp32 rounding enters the BatchNorm statistics
    and breaks the model-level 1e-3 contract (the F(4x4) section), so wino4 "1" is an
    experiments-build A/B (kernel parity in tests/test_wino4_gpu.py)."""
    return C % 8 == 0 and H >= 32 and W >= 32 and cfg.wino4 in ("1", kind) and cfg.fp32_conv == "wino"


def _fp32_route(cfg, C: int, H: int, W: int, kind: str) -> str:
    """fp32 route of a forward (C = Cin) or input gradient (C = Cout) — C is the reduction's channels.
    The 1024-thread F(2x2) kernels take C % 16 == 0 operands materialised once."""
    if cfg.fp32_conv == "direct":
        return "direct"
    if _wino4_ok(cfg, C, H, W, kind):
        return "wino4"
    if C % 16 == 0 and cfg.fp32_conv == "wino":
        return "wino2h"
    return "wino_fused"


MATERIALISED = ("dma", "raw", "wino4", "wino2h")   # routes that read one stored NHWC operand

# route of a 3x3 conv's forward / input gradient -> forward entry
FWD_ENTRY = {
    "first": "pmu_conv_first_fwd",              # Cin <= 4 NCHW planes (forward and weight gradient only)
    "dma": "pmu_conv3x3_fwd_dma",               # bf16, both operands by LDS-DMA (maps >= 32 wide, pad8(C) % 16 == 0)
    "raw": "pmu_conv3x3_fwd_raw",               # bf16 on the materialised operand
    "bf16_fused": "pmu_conv3x3_fwd_bf16",       # bf16, the operand frame staged inside the kernel
    "wino4": "pmu_conv3x3_fwd_wino4",           # fp32 Winograd F(4x4,3x3), materialised operand (maps >= 32 x 32)
    "wino2h": "pmu_conv3x3_fwd_wino2h",         # fp32 F(2x2), 1024-thread workgroups, materialised operand
    "wino_fused": "pmu_conv3x3_fwd_wino",       # fp32 F(2x2), the operand frame staged inside the kernel
    "direct": "pmu_conv3x3_fwd"}                # fp32 direct-sum MFMA kernels (experiments build)
FWD_DMA_ZB = "pmu_conv3x3_fwd_dma_zb"   # the LDS-DMA forward storing z in bf16 (bf16_z)
# weight-gradient route -> (entry, its workspace query); "direct_teed": the direct kernel on two stored operands
WGRAD = {"first": ("pmu_conv_first_wgrad", "pmu_conv_first_wgrad_ws"),
         "bf16_dma": ("pmu_conv3x3_wgrad_bf16_dma", "pmu_conv3x3_wgrad_ws_bf16_dma"),
         "bf16": ("pmu_conv3x3_wgrad_bf16", "pmu_conv3x3_wgrad_ws_bf16"),
         "wino": ("pmu_conv3x3_wgrad_wino", "pmu_conv3x3_wgrad_ws_wino"),
         "direct": ("pmu_conv3x3_wgrad", "pmu_conv3x3_wgrad_ws"), "direct_teed": ("pmu_conv3x3_wgrad", "pmu_conv3x3_wgrad_ws")}
TEED = ("wino", "direct_teed")   # weight-gradient routes whose input gradient tees dz


# ----------------------------------------------------------------------------------------
# 3x3 conv
# ----------------------------------------------------------------------------------------
def conv_fwd_route(bf16: bool, N, H, W, Cin, Cout, planes: int = 0) -> str:
    """planes: how many NCHW input planes the caller offers instead of an NHWC operand (they are
    stacked into one when the first-layer kernel does not take the shape; Cin is then ignored)."""
    if planes and first_layer_ok(planes, Cout):
        return "first"
    Cin = planes or Cin
    if not bf16:
        return _fp32_route(effective(), Cin, H, W, "fwd")
    Cp = pad8(Cin)
    return "dma" if dma_ok(H, W, Cp, Cout, Cout) else "raw" if raw_ok(N, H, W, Cp) else "bf16_fused"


def conv_fwd_entry(route: str, Cout, zb=False) -> str:
    """zb: unet_forward runs with effective().bf16_z (the bf16-z consumers take channel quads)."""
    return FWD_DMA_ZB if route == "dma" and zb and Cout % 8 == 0 else FWD_ENTRY[route]


def conv_fwd_keeps_f32(route: str, Cin, Cout, keep: bool) -> bool:
    """An fp32 forward that a backward follows (keep) keeps the operand it staged, for the weight gradient
    on two stored operands: channel counts on its 64 x 64 blocks."""
    return keep and route in ("wino4", "wino2h", "wino_fused", "direct") and Cin % 64 == 0 and Cout % 64 == 0


def conv_dgrad_route(bf16: bool, N, H, W, Cin, Cout, split=None) -> str:
    """split: the channel where a concatenated operand's gradient is cut in two (bf16: the streaming
    kernels cut on 32-channel boundaries only)."""
    if not bf16:
        return _fp32_route(effective(), Cout, H, W, "dgrad")
    sp, Cp = Cin if split is None else split, pad8(Cout)
    if dma_ok(H, W, Cp, Cin, sp):
        return "dma"
    return "raw" if raw_ok(N, H, W, Cp) and (sp == Cin or sp % 32 == 0) else "bf16_fused"


@dataclass(frozen=True)
class Dgrad:
    """An input gradient's route and epilogue.  form: "" (plain), "bnr" (also the producer layer's
    BN-backward partial sums), "bnr_zb" (the same over a bf16 z), "x1b" (dx1 also in bf16) or "x1b_sum"
    (dx1 only in bf16, with per-tile column sums); dxb: dx / dx0 stored in bf16."""
    route: str
    form: str = ""
    dxb: bool = False

    # entry: pmu_conv3x3_dgrad_<kernel>[_<form>][_dxb], that is (tests/test_cpu_host.py checks each is declared)
    #   pmu_conv3x3_dgrad_dma         pmu_conv3x3_dgrad_dma_dxb          pmu_conv3x3_dgrad_dma_bnr
    #   pmu_conv3x3_dgrad_dma_bnr_dxb pmu_conv3x3_dgrad_dma_bnr_zb       pmu_conv3x3_dgrad_dma_x1b
    #   pmu_conv3x3_dgrad_dma_x1b_dxb pmu_conv3x3_dgrad_dma_x1b_sum      pmu_conv3x3_dgrad_dma_x1b_sum_dxb
    #   pmu_conv3x3_dgrad_raw         pmu_conv3x3_dgrad_bf16             pmu_conv3x3_dgrad_wino4
    #   pmu_conv3x3_dgrad_wino4_bnr   pmu_conv3x3_dgrad_wino2h           pmu_conv3x3_dgrad_wino2h_bnr
    #   pmu_conv3x3_dgrad_wino        pmu_conv3x3_dgrad
    @property
    def entry(self) -> str:
        kernel = {"bf16_fused": "bf16", "wino_fused": "wino", "direct": ""}.get(self.route, self.route)
        return "_".join(p for p in ("pmu_conv3x3_dgrad", kernel, self.form, "dxb" if self.dxb else "") if p)


def conv_dgrad(bf16: bool, N, H, W, Cin, Cout, split=None, bnr=False, z_bf16=False, want_dxb=False,
               x1_bf16_only=False) -> Dgrad:
    """bnr: the operand is one layer's unpooled activation with batch statistics, so the epilogue can
    form that layer's BN-backward partials (z_bf16: its z is stored in bf16); want_dxb: the consumers
    take dx in bf16; x1_bf16_only: the caller needs dx1 only as the transposed conv's bf16 operand."""
    route = conv_dgrad_route(bf16, N, H, W, Cin, Cout, split)
    if not bf16:
        return Dgrad(route, "bnr" if bnr and not z_bf16 and route in ("wino4", "wino2h") else "")
    if route != "dma":
        return Dgrad(route)
    sp = Cin if split is None else split
    dxb = want_dxb and CFG.dx_bf16 and dxb_ok(H, W, Cout, Cin, sp)
    x1b = sp < Cin and (Cin - sp) % 8 == 0
    if x1_bf16_only and x1b:
        return Dgrad(route, "x1b_sum", dxb)
    if bnr:   # (a bf16 z — experiments build — keeps its dx in fp32)
        return Dgrad(route, "bnr_zb") if z_bf16 else Dgrad(route, "bnr", dxb)
    return Dgrad(route, "x1b" if x1b else "", dxb)


def conv_wgrad_route(bf16: bool, N, H, W, Cin, Cout, first=False, kept=False, need_dx=True) -> str:
    """A key of WGRAD.  first: the layer ran on the first-layer kernel; kept (fp32): the forward kept its
    staged operand (conv_fwd_keeps_f32) — with an input gradient to tee dz from, the weight gradient then
    multiplies two stored operands (TEED); else the direct kernel stages both operand frames itself."""
    if first:
        return "first"
    if bf16:
        return "bf16_dma" if CFG.wgrad_dma and L.lib().pmu_conv3x3_wgrad_dma_ok(N, H, W, Cin, Cout) else "bf16"
    if not (kept and need_dx):
        return "direct"
    if effective().fp32_conv != "direct" and L.lib().pmu_conv3x3_wgrad_ws_wino(N, H, W, Cin, Cout):
        return "wino"
    return "direct_teed"


# ----------------------------------------------------------------------------------------
# transposed conv and the Up block's concat operand
# ----------------------------------------------------------------------------------------
_PROBE = ctypes.c_int()   # any non-null address: the frame predicates do not dereference pointers


def _probe_frame(N, H, W, C, pool=L.POOL_NONE) -> L.PmuFrame:
    """A frame of one BN+ReLU source of C channels, as the engine would describe it."""
    f = L.PmuFrame()
    f.nsrc, f.N, f.H, f.W = 1, N, H, W
    c = f.src[0]
    c.x = c.coef = ctypes.addressof(_PROBE)
    c.mode, c.pool, c.dtype, c.C = L.SRC_BNRELU, pool, 0, C
    c.H, c.W = (2 * H, 2 * W) if pool == L.POOL_MAX2 else (H, W)
    return f


def concat_in_place(bf16: bool, N, hi, wi, Cin_t, Cup, hs, ws, Cskip, Cout1, skip_f32=True) -> bool:
    """Does this Up block build its concat operand in place — the transposed conv (N x hi x wi x Cin_t
    -> Cup) writing its half of the stored operand, only the skip half (Cskip x hs x ws) being copied?
    Needs no F.pad, 8-channel halves, an fp32-stored skip, a transposed conv with a strided output and a
    concat conv (-> Cout1) reading a stored operand (fp32: a materialised Winograd route; bf16: LDS-DMA).
    Asked by the encoder (which then writes the skip half with the pooled operand) and by the decoder."""
    if hs != 2 * hi or ws != 2 * wi or Cskip % 8 or Cup % 8 or not skip_f32:
        return False
    route = conv_fwd_route(bf16, N, hs, ws, Cskip + Cup, Cout1)
    if bf16:
        return route == "dma" and bool(L.lib().pmu_convT2x2_dma_ok(Cin_t, Cup, 0))
    return (route in ("wino4", "wino2h")
            and bool(L.lib().pmu_convT2x2_fwd_ld_ok(ctypes.byref(_probe_frame(N, hi, wi, Cin_t)), Cup)))


def pool_skip_ok(bf16: bool, N, h, w, Cskip, Cout1) -> bool:
    """One pass (pmu_frame_to_*_pool_skip) can write a level's max-pooled operand (N x h x w x Cskip)
    together with the skip half of an in-place concat operand: the pooled operand must be a stored one
    too (bf16: the LDS-DMA or raw route; asked, as ever, with the Up block's conv width Cout1)."""
    if bf16 and conv_fwd_route(True, N, h, w, Cskip, Cout1) not in ("dma", "raw"):
        return False
    return bool(L.lib().pmu_frame_pool_skip_ok(ctypes.byref(_probe_frame(N, h, w, Cskip, L.POOL_MAX2))))


def pooled_f32_first(N, h, w, C) -> bool:
    """bf16 beyond the materialised kernels' index range: the pooled activation is stored once, in fp32."""
    return not raw_ok(N, h, w, pad8(C))


def convT_fwd_route(bf16: bool, in_place: bool, N, h, w, Cin, Cup) -> str:
    """"dma_ldb" / "ld" (in place, see concat_in_place), "dma" or "f32".  (N x h x w: the input map, as every
    route question here is asked; the LDS-DMA kernel's shape rule reads the channel counts only.)"""
    if in_place:
        return "dma_ldb" if bf16 else "ld"
    return "dma" if bf16 and L.lib().pmu_convT2x2_dma_ok(Cin, Cup, 0) else "f32"


@dataclass(frozen=True)
class ConvTBwd:
    """dgrad: "dma" or "f32"; dx_bf16: dx stored in bf16 (the next layer's BN backward reads it);
    dup_bf16_only: dup is needed only in bf16, its column sums coming from the concat input gradient."""
    dgrad: str
    dx_bf16: bool
    dup_bf16_only: bool


def convT_bwd(bf16: bool, Cin, Cup, off=(0, 0)) -> ConvTBwd:
    dma = bool(bf16 and L.lib().pmu_convT2x2_dma_ok(Cin, Cup, 1))
    return ConvTBwd("dma" if dma else "f32", dma and CFG.dx_bf16, dma and tuple(off) == (0, 0))


# ----------------------------------------------------------------------------------------
# head
# ----------------------------------------------------------------------------------------
def head_bwd(N, H, W, C, K, z_f32: bool, stats: bool, bf16: bool):
    """(bnr, fuse).  bnr: one pass over z gives the head's input gradient, its weight / bias gradient and
    the last layer's BN-backward partials (pmu_head1x1_bwd_bnr); fuse: da is then left unstored (HeadDa)."""
    bnr = bool(z_f32 and stats and L.lib().pmu_head1x1_bwd_bnr_ok(N, H, W, C))
    return bnr, bool(bnr and CFG.head_fuse and K <= 8 and (not bf16 or C % 8 == 0))


def maxpool_bwd(C, z_f32: bool, stats: bool, parts_bf16: bool, layer_bf16: bool) -> str:
    """Entry of MaxPool2d(2)'s backward into a pooled layer: plain; *_bnr, forming the layer's BN-backward
    partials too; *_bnr_stats, its da = skip + routed pooled gradient left unstored (PoolSumDa).  *_dxb: both
    parts stored in bf16 (parts_bf16; else the fp32 kernels, on fp32 copies where need be)."""
    if not (z_f32 and stats and C % 4 == 0):
        return "pmu_maxpool2_bwd" if z_f32 else "pmu_maxpool2_bwd_zb"
    if CFG.pool_fuse and pool_fuse_ok(C) and (layer_bf16 or not parts_bf16):
        return "pmu_maxpool2_bwd_bnr_stats_dxb" if parts_bf16 else "pmu_maxpool2_bwd_bnr_stats"
    return "pmu_maxpool2_bwd_bnr_dxb" if parts_bf16 else "pmu_maxpool2_bwd_bnr"
