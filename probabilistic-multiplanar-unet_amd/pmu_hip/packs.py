"""Packed weights: the kernels' re-laid-out copies of a conv's weights, cached across calls and
re-packed in one launch per layout by the optimizer.

A conv's weights are re-laid out (Winograd U = G g G^T, bf16 tiles, ...) for its kernels.  They only
change in the optimizer step, so each pack is kept and reused until its tensor changes: the entry
records the parameter's storage, torch's in-place version counter and a pack epoch that
pmu_hip.optim.FusedSGD bumps (its kernel writes the parameters through raw pointers, which torch's
version counter does not see).  After its update FusedSGD calls repack(), which refreshes every
cached pack of the updated parameters in one batched launch per layout (pmu_*_pack_*_multi): the
forward and backward then launch no pack kernel.  (Writes through ``param.data`` bypass the version
counter: call invalidate_packs() after them.)
"""
from __future__ import annotations

import weakref
from functools import partial

import torch

from . import _lib as L

F32 = torch.float32
BF16S = torch.int16   # bf16 values kept as their 16-bit patterns (the kernels' unsigned short)


def _pack_now(pack_entry: str, size_entry, size_dgrad: bool, dtype, w: torch.Tensor, dgrad: bool) -> torch.Tensor:
    """One launch of ``pack_entry`` on w ([Cout][Cin][3][3], or a ConvTranspose2d's [Cin][Cout][2][2]) into
    a new tensor of ``size_entry``'s bytes (asked with dgrad when size_dgrad; None: 4 * Cin * Cout elements).
    dgrad: the input gradient's layout."""
    a, b = w.shape[0], w.shape[1]
    args = (a, b, int(dgrad)) if size_dgrad else (a, b)
    n = 4 * a * b if size_entry is None else getattr(L.lib(), size_entry)(*args) // dtype.itemsize
    wp = torch.empty(n, dtype=dtype, device=w.device)
    L.call(pack_entry, w.data_ptr(), a, b, int(dgrad), wp.data_ptr(), L.stream())
    return wp


# fp32 direct-sum conv: the kernel's per-block B tiles (one launch, ~2x the weight bytes of traffic, so
# staging inside the conv is a straight copy)
pack_weights = partial(_pack_now, "pmu_conv3x3_pack", "pmu_conv3x3_packed_size", True, F32)
# Winograd-transformed weights U = G g G^T in the fp32 F(2x2) kernels' blocks
pack_weights_wino = partial(_pack_now, "pmu_conv3x3_pack_wino", "pmu_conv3x3_packed_size_wino", True, F32)
# weights rounded to bf16: the fused bf16 conv's B tiles; the materialised-operand conv's B tiles
pack_weights_bf16 = partial(_pack_now, "pmu_conv3x3_pack_bf16", "pmu_conv3x3_packed_size_bf16", True, BF16S)
pack_weights_raw = partial(_pack_now, "pmu_conv3x3_pack_raw", "pmu_conv3x3_packed_size_raw", True, BF16S)

class _Pack:
    __slots__ = ("w", "ptr", "ver", "epoch", "t")


_PACKS: dict = {}
_TABLES: dict = {}
# layout -> (single-tensor packer, batched-launch C entries (blocks query, multi launch)):
#   dma        bf16 in the LDS-DMA conv's swizzled unit order
#   wino4      F(4x4,3x3) U = G g G^T in the F(4x4) kernel's blocks
#   wino2h     F(2x2,3x3) weights in the 1024-thread kernel's 64-channel blocks
#   convT_dma  ConvT weights, bf16 in the LDS-DMA GEMMs' swizzled unit order
#   convT      ConvT weights [Cin][Cout][2][2] k-contiguous for the pipelined GEMMs
_LAYOUTS = {
    "dma": (partial(_pack_now, "pmu_conv3x3_pack_dma", "pmu_conv3x3_packed_size_dma", True, BF16S),
            ("pmu_conv3x3_pack_dma_blocks", "pmu_conv3x3_pack_dma_multi")),
    "wino4": (partial(_pack_now, "pmu_conv3x3_pack_wino4", "pmu_conv3x3_packed_size_wino4", True, F32),
              ("pmu_conv3x3_pack_wino4_blocks", "pmu_conv3x3_pack_wino4_multi")),
    "wino2h": (partial(_pack_now, "pmu_conv3x3_pack_wino2h", "pmu_conv3x3_packed_size_wino2h", True, F32),
               ("pmu_conv3x3_pack_wino2h_blocks", "pmu_conv3x3_pack_wino2h_multi")),
    "convT_dma": (partial(_pack_now, "pmu_convT2x2_pack_dma", "pmu_convT2x2_packed_size_dma", False, BF16S),
                  ("pmu_convT2x2_pack_dma_blocks", "pmu_convT2x2_pack_dma_multi")),
    "convT": (partial(_pack_now, "pmu_convT2x2_pack", "pmu_convT2x2_packed_size", False, F32),
              ("pmu_convT2x2_pack_blocks", "pmu_convT2x2_pack_multi")),
}


def _cached_pack(layout: str, w: torch.Tensor, dgrad: bool) -> torch.Tensor:
    key = (id(w), layout, bool(dgrad))
    e = _PACKS.get(key)
    ep = getattr(w, "_pmu_epoch", 0)
    if e is not None and e.w() is w and e.ptr == w.data_ptr() and e.ver == w._version and e.epoch == ep:
        return e.t
    e = _Pack()
    e.w = weakref.ref(w, lambda _r, k=key: _PACKS.pop(k, None))
    e.ptr, e.ver, e.epoch = w.data_ptr(), w._version, ep
    e.t = _LAYOUTS[layout][0](w, dgrad)
    _PACKS[key] = e
    return e.t


pack_weights_dma = partial(_cached_pack, "dma")
pack_weights_wino4 = partial(_cached_pack, "wino4")
pack_weights_wino2h = partial(_cached_pack, "wino2h")
pack_convT_weights_dma = partial(_cached_pack, "convT_dma")
pack_convT_weights = partial(_cached_pack, "convT")


def invalidate_packs() -> None:
    """Forget every cached pack (after writing parameters through ``.data``)."""
    _PACKS.clear()
    _TABLES.clear()


def repack(params) -> int:
    """After an optimizer step that wrote ``params`` in place: bump their pack epoch and refresh all
    their cached packs, one batched launch per (layout, direction).  Returns the launch count."""
    ids = set()
    for p in params:
        p._pmu_epoch = getattr(p, "_pmu_epoch", 0) + 1
        ids.add(id(p))
    groups = {}
    for key, e in list(_PACKS.items()):
        w = e.w()
        if w is None or id(w) not in ids or e.ptr != w.data_ptr() or e.ver != w._version:
            continue   # not updated here, or changed elsewhere: re-packed on its next use
        groups.setdefault((key[1], key[2]), []).append((w, e))
    launches = 0
    s = L.stream()
    lb = L.lib()
    for (layout, dgrad), items in groups.items():
        blocks_fn, multi = _LAYOUTS[layout][1]
        sig = tuple((w.data_ptr(), e.t.data_ptr(), w.shape[0], w.shape[1]) for w, e in items)
        tab = _TABLES.get((layout, dgrad, sig))
        if tab is None:
            jobs = (L.PmuPackJob * len(items))()
            b0 = 0
            for i, (w, e) in enumerate(items):
                nb = getattr(lb, blocks_fn)(w.shape[0], w.shape[1], int(dgrad))
                jobs[i] = L.PmuPackJob(w.data_ptr(), e.t.data_ptr(), w.shape[0], w.shape[1], b0, nb)
                b0 += nb
            dev_jobs = torch.frombuffer(bytearray(jobs), dtype=torch.uint8).to(items[0][0].device)
            tab = (dev_jobs, len(items), b0)
            if len(_TABLES) > 64:
                _TABLES.clear()
            _TABLES[(layout, dgrad, sig)] = tab
        L.call(multi, tab[0].data_ptr(), tab[1], tab[2], int(dgrad), s)
        launches += 1
        for w, e in items:
            e.epoch = w._pmu_epoch
    return launches
