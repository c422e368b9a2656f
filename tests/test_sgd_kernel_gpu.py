"""pmu_sgd_clip (csrc/sgd.hip) by direct calls with hand-built pointer and chunk tables.

pmu_hip.optim.FusedSGD only ever builds chunks that start at multiples of 16384 elements of torch-aligned
tensors, with gscale = 1 unless data-parallel: the float4 path on full chunks.  Here the tensors are
sub-ranges of three fp32 arenas (p, g, buf) whose every other word holds a sentinel bit pattern, so the
kernel's alignment test, its scalar path, its partly filled float4 round and its tail all run, and a store
outside a chunk shows.  The step, from include/pmunet_hip.h:

    gv = g * gscale;  clip > 0: gv = clamp(gv, -clip, clip) (NaN stays NaN);  buf = momentum * buf + gv;
    p = p - lr * buf

Exact case (bit-equal).  p, buf and g are multiples of 2^-8 in [-4, 4], lr = 2^-4, momentum in {0, 1/2, 3/4},
gscale in {1, 1/2, 1/4}, clip in {2^-3, 0, -1}, two consecutive steps with a new gradient each.  gv is a
multiple of 2^-10 of magnitude <= 4; after step one buf is a multiple of 2^-10 below 8 and p a multiple of
2^-14 below 5; after step two buf is a multiple of 2^-12 below 10 and p a multiple of 2^-16 below 6: at most
20 significant bits, so every product, sum and intermediate is a float32 value, fused and unfused
multiply-adds agree, and p and buf must equal the float64 restatement bit for bit
(tests/test_tail_bounds_cpu.py asserts the representability on the CPU; so does this module per case).

Bounded case.  The project's constants (lr 0.05, momentum 0.9, clip 0.1, gscale 1/3, as float32 values),
randn inputs, one step against float64.  gv rounds once (u |gv|; clamping does not amplify it), the fused
momentum * buf + gv rounds once (u |buf'| <= u (|m b| + |gv|)): |dbuf| <= 3 u (|m b| + |gv|) holds with a
unit to spare.  p' = fma(-lr, buf', p) rounds once on top of lr times buf's error:
|dp| <= 2 u (|p| + |lr buf'|) + lr (buf bound).  Gradients +inf / -inf give buf from +clip / -clip, NaN stays
NaN in buf and p, and with clip <= 0 an infinite gradient passes through unclipped (buf = +-inf, p = -+inf).
Measured on an MI355X: worst 0.553 of the buf bound, 0.492 of the p bound.

Layouts (each in both cases): 16-byte aligned tensors of 1, 3, 4, 5, 4094 (n4 = 1023: a partly filled
unrolled float4 round, then a 2-element tail), 16383 and 16384 elements; only g offset by one float (the
whole chunk goes scalar); all three offset by two floats; one 40,000-element tensor at a two-float offset cut
into chunks of 16384, 16384 and 7232; two aligned tensors whose chunks are interleaved and out of order in
the table.  After every call the sentinels of the p and buf arenas and the whole g arena are unchanged bit
for bit."""
import ctypes
import itertools

import pytest
import torch

import tail_refs as R

pytestmark = pytest.mark.gpu

SENTINEL = 0x7FA5C3D2   # the int32 bit pattern of a NaN with a payload: no computed value carries it
GAP = 12        # sentinel words between (and around) tensors
CHUNK = 16384

# name -> (tensors [(len, p_off, g_off, buf_off)] with offsets in floats from a 16-byte boundary,
#          chunk order as (tensor, chunk index) or None for tensor order)
LAYOUTS = {
    "aligned": ([(n, 0, 0, 0) for n in (1, 3, 4, 5, 4094, 16383, 16384)], None),
    "g_off1": ([(5000, 0, 1, 0), (7, 0, 1, 0)], None),
    "all_off2": ([(4099, 2, 2, 2), (16384, 2, 2, 2)], None),
    "big_off2": ([(40000, 2, 2, 2)], None),
    "interleaved": ([(20000, 0, 0, 0), (33000, 0, 0, 0)], [(1, 2), (0, 1), (1, 0), (0, 0), (1, 1)]),
}


class _Arena:
    """Three fp32 arenas with the layout's tensors at their offsets, sentinels elsewhere, and the device
    pointer / chunk tables of one pmu_sgd_clip call."""

    def __init__(self, L, name, dev):
        tensors, order = LAYOUTS[name]
        self.lens = [t[0] for t in tensors]
        self.base = []                                  # per tensor: (p, g, buf) start index in its arena
        pos = [GAP, GAP, GAP]
        for n, *offs in tensors:
            st = []
            for a in range(3):
                b = (pos[a] + 3) // 4 * 4 + offs[a]
                st.append(b)
                pos[a] = b + n + GAP
            self.base.append(tuple(st))
        self.size = max(pos) + 4
        self.dev = dev
        self.arenas = [torch.full((self.size,), SENTINEL, dtype=torch.int32, device=dev) for _ in range(3)]
        for a in self.arenas:
            assert a.data_ptr() % 16 == 0
        self.inside = torch.zeros(3, self.size, dtype=torch.bool)
        for (n, *_), st in zip(tensors, self.base):
            for a in range(3):
                assert not self.inside[a, st[a]:st[a] + n].any()
                self.inside[a, st[a]:st[a] + n] = True
        ptrs, chunks = [], []
        for i, st in enumerate(self.base):
            ptrs += [self.arenas[a].data_ptr() + 4 * st[a] for a in range(3)]
            per = [(i, min(CHUNK, self.lens[i] - s), s) for s in range(0, self.lens[i], CHUNK)]
            chunks.append(per)
        flat = [c for per in chunks for c in per] if order is None else [chunks[t][k] for t, k in order]
        assert sorted(flat) == sorted(c for per in chunks for c in per)
        for i, (n, po, go, bo) in enumerate(tensors):        # the alignment each layout is there for
            for a, off in enumerate((po, go, bo)):
                assert ptrs[3 * i + a] % 16 == 4 * off
        self.nchunks = len(flat)
        self.ptr_t = torch.tensor(ptrs, dtype=torch.int64).to(dev)
        ck = (L.PmuSgdChunk * len(flat))(*[L.PmuSgdChunk(t, ln, s) for t, ln, s in flat])
        self.ck_t = torch.frombuffer(bytearray(ck), dtype=torch.uint8).to(dev)

    def put(self, a, vals):
        """Write one fp32 CPU tensor per layout tensor into arena a (0 p, 1 g, 2 buf)."""
        host = self.arenas[a].cpu()
        for st, n, v in zip(self.base, self.lens, vals):
            host[st[a]:st[a] + n] = v.view(torch.int32)
        self.arenas[a].copy_(host)

    def get(self, a):
        host = self.arenas[a].cpu()
        assert bool((host[~self.inside[a]] == SENTINEL).all()), f"arena {a}: a sentinel word was overwritten"
        return host, [host[st[a]:st[a] + n].view(torch.float32) for st, n in zip(self.base, self.lens)]

    def step(self, L, gscale, lr, momentum, clip):
        L.call("pmu_sgd_clip", self.ck_t.data_ptr(), self.nchunks, self.ptr_t.data_ptr(), gscale, lr, momentum, clip,
               L.stream())
        torch.cuda.synchronize()


def _bits_equal(a, b):
    return torch.equal(a.view(torch.int32), b.view(torch.int32))


@pytest.mark.parametrize("layout", list(LAYOUTS))
def test_sgd_clip_exact_two_steps(dev, layout):
    from pmu_hip import _lib as L
    ar = _Arena(L, layout, dev)
    data = [R.sgd_exact_inputs(n, seed=i) for i, n in enumerate(ar.lens)]      # per tensor: p, buf, g1, g2
    for m, gs, clip in itertools.product(R.SGD_EXACT_MOMENTA, R.SGD_EXACT_GSCALES, R.SGD_EXACT_CLIPS):
        ar.put(0, [d[0] for d in data])
        ar.put(2, [d[1] for d in data])
        p = [d[0] for d in data]
        b = [d[1] for d in data]
        for stepno in (0, 1):
            g = [d[2 + stepno] for d in data]
            ar.put(1, g)
            g_before = ar.arenas[1].cpu()
            ar.step(L, gs, R.SGD_EXACT_LR, m, clip)
            _, pg = ar.get(0)
            _, bg = ar.get(2)
            assert torch.equal(ar.arenas[1].cpu(), g_before), "the gradient arena was written"
            for i in range(len(ar.lens)):
                pn, bn, _, _ = R.sgd_ref(p[i], g[i], b[i], gs, R.SGD_EXACT_LR, m, clip)
                assert torch.equal(pn.float().double(), pn) and torch.equal(bn.float().double(), bn)
                what = (layout, "tensor", i, "len", ar.lens[i], "step", stepno, "momentum", m, "gscale", gs,
                        "clip", clip)
                assert _bits_equal(bg[i], bn.float()), ("buf",) + what
                assert _bits_equal(pg[i], pn.float()), ("p",) + what
                p[i], b[i] = pn.float(), bn.float()


@pytest.mark.parametrize("clip", [R.SGD_CLIP, 0.0, -1.0])
@pytest.mark.parametrize("layout", list(LAYOUTS))
def test_sgd_clip_vs_float64(dev, layout, clip):
    from pmu_hip import _lib as L
    ar = _Arena(L, layout, dev)
    data = [R.sgd_bounded_inputs(n, seed=i) for i, n in enumerate(ar.lens)]    # per tensor: p, g, buf
    for a in range(3):
        ar.put(a, [d[a] for d in data])
    g_before = ar.arenas[1].cpu()
    ar.step(L, R.SGD_GSCALE, R.SGD_LR, R.SGD_MOMENTUM, clip)
    _, pg = ar.get(0)
    _, bg = ar.get(2)
    assert torch.equal(ar.arenas[1].cpu(), g_before), "the gradient arena was written"
    wb = wp = 0.0
    for i, n in enumerate(ar.lens):
        p, g, b = data[i]
        pn, bn, bb, bp = R.sgd_ref(p, g, b, R.SGD_GSCALE, R.SGD_LR, R.SGD_MOMENTUM, clip)
        b6, p6 = bg[i].double(), pg[i].double()
        wb, wp = max(wb, R.worst_ratio(b6, bn, bb)), max(wp, R.worst_ratio(p6, pn, bp))
        assert bool(R.within(b6, bn, bb).all()), ("buf", layout, i, n, R.worst_ratio(b6, bn, bb))
        assert bool(R.within(p6, pn, bp).all()), ("p", layout, i, n, R.worst_ratio(p6, pn, bp))
        if n >= 8:
            idx = torch.tensor([1, 2, n // 2])
            sign = torch.tensor([1.0, -1.0, 1.0], dtype=torch.float64)
            mb = R.SGD_MOMENTUM * b.double()[idx]
            if clip > 0:      # +-inf clamps to +-clip: buf = momentum * buf +- clip
                assert bool(((b6[idx] - (mb + sign * clip)).abs() <= bb[idx]).all())
                assert torch.isfinite(p6[idx]).all()
            else:             # no clipping: the infinity reaches buf, and p with the opposite sign
                assert torch.equal(b6[idx], sign * float("inf")) and torch.equal(p6[idx], -sign * float("inf"))
            assert torch.isnan(b6[n - 1]) and torch.isnan(p6[n - 1])
            fin = torch.ones(n, dtype=torch.bool)
            fin[idx] = clip > 0
            fin[n - 1] = False
            assert torch.isfinite(b6[fin]).all() and torch.isfinite(p6[fin]).all()
    print(f"sgd {layout} clip={clip}: worst {wb:.3f} of the buf bound, {wp:.3f} of the p bound")


def test_sgd_clip_refuses_empty_and_null_tables(dev):
    from pmu_hip import _lib as L
    ar = _Arena(L, "g_off1", dev)
    lib, s = L.lib(), L.stream()
    f = ctypes.c_float
    before = [a.cpu() for a in ar.arenas]
    assert lib.pmu_sgd_clip(ar.ck_t.data_ptr(), 0, ar.ptr_t.data_ptr(), f(1), f(1), f(0.9), f(0.1), s) == L.PMU_ERR_ARG
    assert lib.pmu_sgd_clip(ar.ck_t.data_ptr(), -1, ar.ptr_t.data_ptr(), f(1), f(1), f(0.9), f(0.1), s) == L.PMU_ERR_ARG
    assert lib.pmu_sgd_clip(None, ar.nchunks, ar.ptr_t.data_ptr(), f(1), f(1), f(0.9), f(0.1), s) == L.PMU_ERR_ARG
    assert lib.pmu_sgd_clip(ar.ck_t.data_ptr(), ar.nchunks, None, f(1), f(1), f(0.9), f(0.1), s) == L.PMU_ERR_ARG
    torch.cuda.synchronize()
    for a, b in zip(ar.arenas, before):
        assert torch.equal(a.cpu(), b)
