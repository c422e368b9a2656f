"""The 1x1 head kernels of csrc/head1x1.hip (pmu_head1x1_fwd, _bwd, _bwd_bnr, _bwd_dz and pmu_wgrad1x1) held to
float64, bit for bit, on every path and class count.

Inputs and references come from tests/head_cases.py: grids on which every product and every partial sum of these
kernels is an fp32 number (tests/test_head_exact_cpu.py checks the conditions without a GPU).  Compared without any
tolerance: the pre-sigmoid y, dl, da and the fp32 dz with the float64 reference; the BN-backward `part` rows with the
float64 sums over the 2048-pixel blocks of pmu_head1x1_bwd_tiles, row by row; dw and db with the float64 sum over the
whole map rounded once to fp32 (a block's fp32 slab is exact — headroom is asserted per block — the slabs are summed
in fp64 and cast once); the bf16 dz with the reference's round-to-nearest-even bits.  exact_headroom is asserted in
every case, from the reference alone.

The sigmoid is the only inexact step: y = 1 / (1 + expf(-v)) on exact logits v, |v| <= 80, with one class's bias at
+-40 (where fp32 saturates to exactly 1), is compared with float64 sigmoid(v) in units of ulp32(reference).  The worst
error measured on the MI355X is SIG_WORST_MI355X = 1.80 units (1.798; the release and the debug library alike); the tests
admit SIG_ADMIT = 4 units, twice that rounded up, under the fixed ceiling of 8 (head_cases.SIG_CEILING).

Every call is made under the entry's own name, with outputs and workspaces pre-filled with NaN (-7 for bf16 bits) and
a guard tail that must stay untouched, and runs twice for identical bits.  The geometries are the smallest that reach
each branch (head_cases: a block of one pixel, a ragged second block, exactly one block, one pixel over a block,
P mod (4 * PG) != 0, and 133,640 pixels at C = 8 / 6 for the unrolled loop of the slab reduction)."""
import math

import pytest
import torch

import head_cases as HC
from head_cases import DEEP, GEOMETRIES, RAGGED, SMALL, gid
from helpers import assert_exact, assert_rne_exercised, bf16_bits, bf16_exact, ref_frame, ulp32

pytestmark = pytest.mark.gpu
NAN = float("nan")
GUARD = 64
SIG_WORST_MI355X = 1.80
SIG_ADMIT = min(HC.SIG_CEILING, float(math.ceil(2 * SIG_WORST_MI355X)))


# ------------------------------------------------------------------------------------------ plumbing
def _buf(n, dev, bits=False):
    """n elements and a guard tail, pre-filled: NaN, or -7 for bf16 bits."""
    return torch.full((n + GUARD,), -7 if bits else NAN, dtype=torch.int16 if bits else torch.float32, device=dev)


def _untouched(t):
    return bool((t == -7).all()) if t.dtype == torch.int16 else bool(torch.isnan(t).all())


def _take(buf, shape, where):
    n = math.prod(shape)
    assert _untouched(buf[n:]), f"{where}: wrote past the end of the output"
    return buf[:n].view(shape)


def _same_bits(a, b):
    return torch.equal(a, b) if a.dtype == torch.int16 else torch.equal(a.view(torch.int32), b.view(torch.int32))


def _twice(fn, where):
    """fn() -> tuple of raw output buffers (None allowed); run twice, identical bits required."""
    a, b = fn(), fn()
    torch.cuda.synchronize()
    for x, y in zip(a, b):
        assert x is None or _same_bits(x, y), f"{where}: two runs differ"
    return a


def _on(dev, s, xb=False):
    """The engine's descriptor of source s on the device; xb: x stored as bf16 bits (the values are bf16 numbers)."""
    from pmu_hip.engine import Src
    x = s.x
    if xb:
        assert bf16_exact(x)
        x = bf16_bits(x)
    return Src(x.contiguous().to(dev), s.mode, None if s.coef is None else s.coef.to(dev),
               z=None if s.z is None else s.z.contiguous().to(dev), pool=s.pool, off=s.off)


class DevLayer:
    def __init__(self, l, dev):
        for k in ("z", "coef", "mean", "invstd", "bcoef"):
            setattr(self, k, getattr(l, k).contiguous().to(dev))


class DevGrads:
    def __init__(self, gr, dev):
        self.dy, self.y, self.w = gr.dy.contiguous().to(dev), gr.y.contiguous().to(dev), gr.w.contiguous().to(dev)


# ------------------------------------------------------------------------------------------ forward
_SIG_WORST = {"units": 0.0, "where": None}


def _fwd(dev, srcs, N, H, W, w, b, K, sig, where):
    from pmu_hip import _lib as L
    from pmu_hip.engine import frame_of
    f = frame_of(srcs, N, H, W)
    wd, bd = w.to(dev), None if b is None else b.to(dev)

    def run():
        y = _buf(N * K * H * W, dev)
        L.call("pmu_head1x1_fwd", f, wd.data_ptr(), L.ptr(bd), K, sig, y.data_ptr(), L.stream())
        return (y,)
    return _take(_twice(run, where)[0], (N, K, H, W), where)


def _check_sigmoid(y, v64, where):
    """y = sigmoid of the exact logits v64 on the device against float64, in ulp32 of the reference."""
    assert float(v64.abs().max()) <= HC.SIG_VMAX, f"{where}: |logit| {float(v64.abs().max())} > {HC.SIG_VMAX}"
    ref = torch.sigmoid(v64)
    assert float(ref.min()) >= 2.0 ** -126
    got = y.double().cpu()
    assert not bool(torch.isnan(got).any()), f"{where}: NaN left in y"
    err = ((got - ref).abs() / ulp32(ref)).max().item()
    if err > _SIG_WORST["units"]:
        _SIG_WORST.update(units=err, where=where)
    print(f"sigmoid {where}: worst {err:.3f} ulp32 (admitted {SIG_ADMIT:g}; running worst {_SIG_WORST['units']:.3f})")
    sat = v64 >= 40.0
    if bool(sat.any()):
        assert bool((got[sat] == 1.0).all()), f"{where}: sigmoid of a logit >= 40 is not exactly 1"
    assert err <= SIG_ADMIT, f"{where}: sigmoid off by {err:.3f} ulp32 of the float64 reference, admitted {SIG_ADMIT:g}"


def _fwd_case(dev, cpu_srcs, N, H, W, K, C, where, ua=HC.U_A, xbs=(False,), sat=0):
    """Sigmoid off (dense weights, b given and NULL: bit equality) and on (sparse weights, one class saturated)."""
    for xb in xbs:
        srcs = [_on(dev, s, xb) for s in cpu_srcs]
        w, b = HC.fwd_params(K, C)
        for bias in (b, None):
            tag = f"{where} xbf={int(xb)} b={'given' if bias is not None else 'NULL'}"
            ref = HC.ref_fwd(cpu_srcs, N, H, W, w, bias, tag, ua)
            assert_exact(_fwd(dev, srcs, N, H, W, w, bias, K, 0, tag), ref, tag + ": y")
        ws, bs = HC.fwd_params(K, C, sparse=True, sat=sat)
        tag = f"{where} xbf={int(xb)} sigmoid sat={sat}"
        _check_sigmoid(_fwd(dev, srcs, N, H, W, ws, bs, K, 1, tag), HC.ref_fwd(cpu_srcs, N, H, W, ws, bs, tag, ua), tag)


@pytest.mark.parametrize("C,K", HC.FWD_FAST, ids=[f"C{c}-K{k}" for c, k in HC.FWD_FAST])
def test_fwd_fast(dev, C, K):
    """head_fwd_fast_kernel: every CQ = 1 .. 64 (all stages of pmu_group_sum) at K = 1 (four pixels per round) and 3;
    every K at C = 8 and 64; x in fp32 and bf16; b given and NULL; sigmoid off and on.  3 x 23 x 31: a ragged second
    block of 91 pixels."""
    l = HC.layer(*RAGGED, C)
    _fwd_case(dev, [HC.act_src(l)], *RAGGED, K, C, f"pmu_head1x1_fwd fast C={C} K={K}", xbs=(False, True),
              sat=HC.sat_of("fast", C, K))


@pytest.mark.parametrize("C,K", HC.FWD_FAST_GEOM, ids=[f"C{c}-K{k}" for c, k in HC.FWD_FAST_GEOM])
@pytest.mark.parametrize("geom", [g for g in GEOMETRIES if g != RAGGED], ids=gid)
def test_fwd_fast_geometries(dev, geom, C, K):
    l = HC.layer(*geom, C)
    _fwd_case(dev, [HC.act_src(l)], *geom, K, C, f"pmu_head1x1_fwd fast {gid(geom)} C={C} K={K}",
              sat=HC.sat_of("geom", C, K))


@pytest.mark.parametrize("geom,name,K", HC.FWD_GENERIC, ids=[f"{gid(g)}-{n}-K{k}" for g, n, k in HC.FWD_GENERIC])
def test_fwd_generic(dev, geom, name, K):
    """head_fwd_kernel through frame_value4, against ref_frame: C % 4 != 0 (scalar reads), C = 260 (beyond the fast
    path), a RAW source at a fast C, two sources with C0 = 6, MaxPool2d(2) and AvgPool2d(2, ceil) sources, and a
    smaller source placed at (1, 1) with zeros outside."""
    srcs, ua = HC.generic_frame(name, *geom)
    C = sum(s.x.shape[3] for s in srcs)
    _fwd_case(dev, srcs, *geom, K, C, f"pmu_head1x1_fwd generic {name} {gid(geom)} K={K}", ua=ua,
              sat=HC.sat_of("generic", C, K))


# ------------------------------------------------------------------------------------------ backward
@pytest.mark.parametrize("sig", [0, 1])
@pytest.mark.parametrize("C,K", HC.BWD, ids=[f"C{c}-K{k}" for c, k in HC.BWD])
@pytest.mark.parametrize("geom", [RAGGED, SMALL], ids=gid)
def test_bwd(dev, geom, C, K, sig):
    """pmu_head1x1_bwd: head_bwd_fast_kernel<false> at C = 4 and 256, head_bwd_kernel at C = 1, 5 (scalar stores), 20
    and 260 (float4 stores)."""
    from pmu_hip import _lib as L
    N, H, W = geom
    gr = HC.grads(N, K, H, W, C, sig)
    d = DevGrads(gr, dev)
    where = f"pmu_head1x1_bwd {gid(geom)} C={C} K={K} sig={sig}"

    def run():
        dl, da = _buf(N * K * H * W, dev), _buf(N * H * W * C, dev)
        L.call("pmu_head1x1_bwd", d.dy.data_ptr(), d.y.data_ptr() if sig else None, sig, d.w.data_ptr(), K, C, N, H, W,
               dl.data_ptr(), da.data_ptr(), L.stream())
        return dl, da
    dl, da = _twice(run, where)
    g64 = HC.ref_g(gr, sig)
    assert_exact(_take(dl, (N, K, H, W), where), g64, where + ": dl")
    assert_exact(_take(da, (N, H, W, C), where), HC.ref_da(g64, gr.w, gr.ug, where), where + ": da")


def _diff(bad, got, ref64, where):
    """assert_exact, its message collected in bad instead of raised."""
    try:
        assert_exact(got, ref64, where)
    except AssertionError as e:
        bad.append(str(e))


def _bnr_case(dev, geom, C, K, sig, modes=("dl+da", "dw+da", "dw", "dw-db")):
    """pmu_head1x1_bwd_bnr in its three modes (and dw with db == NULL) against one set of references."""
    from pmu_hip import _lib as L
    N, H, W = geom
    l, gr = HC.layer(N, H, W, C), HC.grads(N, K, H, W, C, sig)
    dl_, dg = DevLayer(l, dev), DevGrads(gr, dev)
    base = f"pmu_head1x1_bwd_bnr {gid(geom)} C={C} K={K} sig={sig}"
    g64 = HC.ref_g(gr, sig)
    da64 = HC.ref_da(g64, gr.w, gr.ug, base)
    part64 = HC.ref_part(da64, l, gr.ug, base)
    R = L.lib().pmu_head1x1_bwd_tiles(N, H, W)
    assert R == part64.shape[0], f"{base}: {R} rows of partial sums, the documented tiling has {part64.shape[0]}"
    dw64 = db64 = None
    if any(m.startswith("dw") for m in modes):
        dw64, db64 = HC.ref_wgrad(g64, ref_frame([HC.act_src(l)], N, H, W), HC.HPPB, gr.ug, HC.U_A, base)
    need = R * K * (C + 1) * 4
    bad = []
    for mode in modes:
        where = f"{base} mode={mode}"
        wg, st_da, st_db = mode.startswith("dw"), mode in ("dl+da", "dw+da"), mode != "dw-db"

        def run():
            dl = _buf(N * K * H * W, dev)       # (dw modes: handed over only to show that it is not written)
            da = _buf(N * H * W * C, dev) if st_da else None
            part = _buf(R * 2 * C, dev)
            dw, db = (_buf(K * C, dev), _buf(K, dev) if st_db else None) if wg else (None, None)
            ws = _buf(need // 4, dev) if wg else None
            L.call("pmu_head1x1_bwd_bnr", dg.dy.data_ptr(), dg.y.data_ptr() if sig else None, sig, dg.w.data_ptr(), K, C,
                   N, H, W, dl.data_ptr() if (not wg or mode == "dw+da") else None, L.ptr(da), dl_.z.data_ptr(),
                   dl_.coef.data_ptr(), dl_.mean.data_ptr(), dl_.invstd.data_ptr(), part.data_ptr(), L.ptr(dw), L.ptr(db),
                   L.ptr(ws), need if wg else 0, L.stream())
            if ws is not None:
                torch.cuda.synchronize()
                assert _untouched(ws[need // 4:]), f"{where}: wrote past the end of the workspace"
            return dl, da, part, dw, db
        dl, da, part, dw, db = _twice(run, where)
        _diff(bad, _take(part, (R, 2, C), where), part64, where + ": part")
        if st_da:
            _diff(bad, _take(da, (N, H, W, C), where), da64, where + ": da")
        if wg:
            assert _untouched(dl), f"{where}: dl written although dw was asked for"
            _diff(bad, _take(dw, (K, C), where), dw64.float().double(), where + ": dw")
            if st_db:
                _diff(bad, _take(db, (K,), where), db64.float().double(), where + ": db")
        else:
            _diff(bad, _take(dl, (N, K, H, W), where), g64, where + ": dl")
    assert not bad, "\n".join(bad)       # (every output of every mode is compared before the case fails)


@pytest.mark.parametrize("C,K,sig", HC.BNR, ids=[f"C{c}-K{k}-sig{s}" for c, k, s in HC.BNR])
def test_bwd_bnr(dev, C, K, sig):
    """Every K with both sigmoid settings at C = 16 — with and without the da store, all 32 head_dispatch
    instantiations of head_bwd_fused_kernel — and every fast C at K = 3, on the ragged second block (91 pixels
    against batches of B * PG)."""
    _bnr_case(dev, RAGGED, C, K, sig)


@pytest.mark.parametrize("C,K,sig", HC.BNR_GEOM, ids=[f"C{c}-K{k}-sig{s}" for c, k, s in HC.BNR_GEOM])
@pytest.mark.parametrize("geom", [g for g in GEOMETRIES if g != RAGGED], ids=gid)
def test_bwd_bnr_geometries(dev, geom, C, K, sig):
    _bnr_case(dev, geom, C, K, sig, modes=("dl+da", "dw+da", "dw"))


def test_bwd_bnr_deep_reduction(dev):
    """133,640 pixels at C = 8, K = 3: R = 66 block rows, so pmu_colsum64x16's unrolled loop runs once and a tail
    follows."""
    from pmu_hip import _lib as L
    assert L.lib().pmu_head1x1_bwd_tiles(*DEEP) == 66
    _bnr_case(dev, DEEP, 8, 3, 1, modes=("dw+da", "dw"))


def _dz_case(dev, geom, C, K, sig):
    from pmu_hip import _lib as L
    N, H, W = geom
    l = HC.layer(N, H, W, C)
    dl_ = DevLayer(l, dev)
    for bf in (False, True):
        if bf and C % 8:
            continue
        gr = HC.grads(N, K, H, W, C, sig, fine=bf)
        dg = DevGrads(gr, dev)
        where = f"pmu_head1x1_bwd_dz {gid(geom)} C={C} K={K} sig={sig} bf16={int(bf)}"
        ref = HC.ref_dz(l, HC.ref_da(HC.ref_g(gr, sig), gr.w, gr.ug, where))
        if bf and ref.numel() >= 2000:
            assert_rne_exercised(ref, where)

        def run():
            dz = _buf(N * H * W * C, dev, bits=bf)
            L.call("pmu_head1x1_bwd_dz", dg.dy.data_ptr(), dg.y.data_ptr() if sig else None, sig, dg.w.data_ptr(), K, C,
                   N, H, W, dl_.z.data_ptr(), dl_.bcoef.data_ptr(), int(bf), dz.data_ptr(), L.stream())
            return (dz,)
        got = _take(_twice(run, where)[0], (N, H, W, C), where)
        if not bf:
            assert_exact(got, ref, where + ": dz")
            continue
        got, want = got.cpu(), bf16_bits(ref)
        if not torch.equal(got, want):
            assert_exact(got.view(torch.bfloat16).float(), want.view(torch.bfloat16).double(), where + ": dz (bf16, RNE)")
            raise AssertionError(f"{where}: bf16 bits differ from the reference's only in the sign of a zero")


@pytest.mark.parametrize("C,K,sig", HC.DZ, ids=[f"C{c}-K{k}-sig{s}" for c, k, s in HC.DZ])
def test_bwd_dz(dev, C, K, sig):
    """Every K with both sigmoid settings at C = 16 and every fast C at K = 2: fp32 dz exactly, bf16 dz (C % 8 == 0)
    as the reference's round-to-nearest-even bits, ties in both directions."""
    _dz_case(dev, RAGGED, C, K, sig)


@pytest.mark.parametrize("C,K,sig", HC.DZ_GEOM, ids=[f"C{c}-K{k}-sig{s}" for c, k, s in HC.DZ_GEOM])
@pytest.mark.parametrize("geom", [g for g in GEOMETRIES if g != RAGGED], ids=gid)
def test_bwd_dz_geometries(dev, geom, C, K, sig):
    _dz_case(dev, geom, C, K, sig)


# ------------------------------------------------------------------------------------------ weight gradient
@pytest.mark.parametrize("geom,name,K", HC.WGRAD, ids=[f"{gid(g)}-{n}-K{k}" for g, n, k in HC.WGRAD])
def test_wgrad1x1(dev, geom, name, K):
    """pmu_wgrad1x1: wgrad1x1_fast_kernel (2048-pixel blocks; fp32 and bf16 x; C = 256) and wgrad1x1_kernel (1024-pixel
    blocks; C = 6, C = 255, a two-source frame, a pooled frame), with db given and NULL.  At 133,640 pixels the slab
    reduction sees R = 66 (fast) and 131 (generic: two unrolled rounds and a tail) rows."""
    from pmu_hip import _lib as L
    from pmu_hip.engine import frame_of
    N, H, W = geom
    cpu_srcs, ua, xb, ppb = HC.wgrad_sources(name, N, H, W)
    C = sum(s.x.shape[3] for s in cpu_srcs)
    fast = ppb == HC.HPPB
    gr = HC.grads(N, K, H, W, C, 0)
    where = f"pmu_wgrad1x1 {gid(geom)} {name} K={K}"
    g64 = HC.ref_g(gr, 0)
    dw64, db64 = HC.ref_wgrad(g64, ref_frame(cpu_srcs, N, H, W), ppb, gr.ug, ua, where)
    R = -(-N * H * W // ppb)
    if geom == DEEP:
        assert R == (66 if fast else 131)
    need = R * K * (C + 1) * 4
    assert L.lib().pmu_wgrad1x1_ws(N * H * W, K, C) >= need
    srcs = [_on(dev, s, xb) for s in cpu_srcs]
    f = frame_of(srcs, N, H, W)
    dl = gr.dy.contiguous().to(dev)
    for with_db in (True, False):
        def run():
            dw, db, ws = _buf(K * C, dev), _buf(K, dev) if with_db else None, _buf(need // 4, dev)
            L.call("pmu_wgrad1x1", dl.data_ptr(), f, K, dw.data_ptr(), L.ptr(db), ws.data_ptr(), need, L.stream())
            torch.cuda.synchronize()
            assert _untouched(ws[need // 4:]), f"{where}: wrote past the end of the workspace"
            return dw, db
        dw, db = _twice(run, where)
        assert_exact(_take(dw, (K, C), where), dw64.float().double(), f"{where} db={int(with_db)}: dw")
        if with_db:
            assert_exact(_take(db, (K,), where), db64.float().double(), where + ": db")


# ------------------------------------------------------------------------------------------ refusals
def test_refusals(dev):
    """Host-side PMU_ERR_ARG, before any launch: K = 0 and 9 on the four head entries; the fused entries at C = 12 and
    260; bf16 dz at C = 4; ws_bytes one byte short; dw with ws == NULL; dw == NULL with da == NULL; do_sigmoid with
    y == NULL.  Every output stays as pre-filled."""
    from pmu_hip import _lib as L
    from pmu_hip.engine import frame_of
    lib, st = L.lib(), L.stream()
    N, H, W = SMALL
    P = N * H * W
    out = torch.full((P * 260 * 2 + 4096,), NAN, device=dev)       # every output and workspace pointer
    o = out.data_ptr()
    bad = []

    def refused(what, rc):
        if rc != L.PMU_ERR_ARG:
            bad.append(f"{what}: returned {rc}")

    def entries(C, K, sig=0, y=True, dl=True, da=True, dw=True, ws=True, short=0, bf=0):
        """The four head entries' return codes for one argument set (fwd only where a frame of C channels exists)."""
        l, gr = HC.layer(N, H, W, C), HC.grads(N, max(1, min(K, 8)), H, W, C, 1)
        d, g = DevLayer(l, dev), DevGrads(gr, dev)
        yp = g.y.data_ptr() if y else None
        need = lib.pmu_head1x1_bwd_tiles(N, H, W) * max(K, 1) * (C + 1) * 4
        src = _on(dev, HC.act_src(l))
        keep.append((d, g, src))
        return {
            "fwd": lambda: lib.pmu_head1x1_fwd(frame_of([src], N, H, W), g.w.data_ptr(), None, K, sig, o, st),
            "bwd": lambda: lib.pmu_head1x1_bwd(g.dy.data_ptr(), yp, sig, g.w.data_ptr(), K, C, N, H, W, o, o, st),
            "bnr": lambda: lib.pmu_head1x1_bwd_bnr(g.dy.data_ptr(), yp, sig, g.w.data_ptr(), K, C, N, H, W,
                                                   o if dl else None, o if da else None, d.z.data_ptr(), d.coef.data_ptr(),
                                                   d.mean.data_ptr(), d.invstd.data_ptr(), o, o if dw else None, o,
                                                   o if ws else None, need - short, st),
            "dz": lambda: lib.pmu_head1x1_bwd_dz(g.dy.data_ptr(), yp, sig, g.w.data_ptr(), K, C, N, H, W, d.z.data_ptr(),
                                                 d.bcoef.data_ptr(), bf, o, st),
        }
    keep = []
    for K in (0, 9):
        for name, fn in entries(16, K).items():
            refused(f"pmu_head1x1_{name} K={K}", fn())
    for C in (12, 260):
        e = entries(C, 3)
        refused(f"pmu_head1x1_bwd_bnr C={C}", e["bnr"]())
        refused(f"pmu_head1x1_bwd_dz C={C}", e["dz"]())
    refused("bf16 dz at C=4", entries(4, 2, bf=1)["dz"]())
    refused("ws_bytes one byte short", entries(16, 3, short=1)["bnr"]())
    refused("dw with ws == NULL", entries(16, 3, ws=False)["bnr"]())
    refused("dw == NULL with da == NULL", entries(16, 3, dw=False, da=False)["bnr"]())
    refused("dw == NULL with dl == NULL", entries(16, 3, dw=False, dl=False)["bnr"]())
    e = entries(16, 3, sig=1, y=False)
    for name in ("bwd", "bnr", "dz"):
        refused(f"pmu_head1x1_{name} do_sigmoid with y == NULL", e[name]())
    torch.cuda.synchronize()
    assert not bad, bad
    assert bool(torch.isnan(out).all()), "a refused call wrote to its output"
