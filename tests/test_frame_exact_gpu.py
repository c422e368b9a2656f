"""The operand-frame kernels (csrc/frame.hip: pmu_frame_to_bf16 / _f32, their _ld and _pool_skip
forms) held to helpers.ref_frame, the float64 restatement of pmu_frame, bit for bit.

Inputs lie on grids where every formula of the family is an exact fp32 number (helpers.quant_z / quant_bn /
quant_grad): fmaf(z, scale, shift) is a multiple of 2^-5 below 4; max-pool winners and ReLU masks agree
between fp32 and fp64; average-pool divisors are 1, 2 or 4; scale * g + (kx * (z - mean) + kc) with dyadic kx,
kc is a multiple of 2^-8 below 16.  So the fp32 result equals the reference exactly and the bf16 result is the
reference's round-to-nearest-even bits — no tolerance anywhere.  The gradient grid (multiples of 2^-6 in
[-4, 4]) makes the values that are rounded to bf16 hit ties in both directions (helpers.assert_rne_exercised,
checked on the CPU reference).

Every case calls the entry under its own name, pre-fills the output (NaN / -7), keeps sentinel channels and a
guard tail that must stay untouched, requires the padding channels [C, Cpad) of the bf16 operand to be +0, runs
twice for identical bits, and runs with PMU_FRAME_STREAM unset (the streaming kernel where stream_ok admits
the frame) and "0" (the generic kernels).

Three large cases make frame_stream_kernel's loop body repeat (P > 2 * U * (256 >> lg) * 8 * CUs pixels, so the
register set loaded at base + 2 * stride is consumed one iteration later) and reach the nontemporal
instantiations the shipped library launches for bf16 output once the source counts 128 MiB at 4 bytes per
element; their reference is the same ref_frame evaluated by torch on the GPU."""
import contextlib
import os
from collections import namedtuple

import pytest
import torch

from helpers import (POOL_AVG2CEIL, POOL_MAX2, POOL_NONE, SRC_BNBWD, SRC_BNRELU, SRC_RAW, assert_exact,
                     assert_rne_exercised, bf16_bits, bf16_exact, quant_bn, quant_grad, quant_z, ref_frame)

pytestmark = pytest.mark.gpu

S = namedtuple("S", "x mode coef z pool off", defaults=(SRC_RAW, None, None, POOL_NONE, (0, 0)))
GUARD = 64   # elements after the output that no kernel may touch


@contextlib.contextmanager
def _env(name, value):
    """name=value (None: unset) for the calls inside, restored afterwards."""
    old = os.environ.get(name)
    if value is None:
        os.environ.pop(name, None)
    else:
        os.environ[name] = value
    try:
        yield
    finally:
        if old is None:
            os.environ.pop(name, None)
        else:
            os.environ[name] = old


# ------------------------------------------------------------------------------------------ sources
def bnrelu(g, N, Hs, Ws, C, pool=POOL_NONE, off=(0, 0)):
    return S(quant_z(N, Hs, Ws, C, g), SRC_BNRELU, quant_bn(C, g), None, pool, off)


def raw(g, N, Hs, Ws, C, pool=POOL_NONE, off=(0, 0)):
    return S(quant_grad((N, Hs, Ws, C), g, fine=True), SRC_RAW, None, None, pool, off)


def bnbwd(g, N, H, W, C):
    return S(quant_grad((N, H, W, C), g, fine=True), SRC_BNBWD, quant_bn(C, g, bwd=True, dyadic=True),
             quant_z(N, H, W, C, g))


def _on(dev, s, xb=False, zb=False):
    """The engine's descriptor of source s on the device; xb / zb: x / z stored as bf16 bits (the values must
    be bf16 numbers, so the stored tensor holds exactly what the reference reads)."""
    from pmu_hip.engine import Src
    x, z = s.x, s.z
    if xb:
        assert bf16_exact(x)
        x = bf16_bits(x)
    if zb:
        assert bf16_exact(z)
        z = bf16_bits(z)
    return Src(x.contiguous().to(dev), s.mode, None if s.coef is None else s.coef.to(dev),
               z=None if z is None else z.contiguous().to(dev), pool=s.pool, off=s.off)


# ------------------------------------------------------------------------------------------ launch + compare
def _launch(srcs, N, H, W, bf, Cpad, ldo, dev):
    """One call of the entry the arguments select, into a pre-filled flat buffer of N*H*W*ld + GUARD elements."""
    from pmu_hip import _lib as L
    from pmu_hip.engine import frame_of
    C = sum(s.x.shape[3] for s in srcs)
    ld = ldo or (Cpad if bf else C)
    buf = torch.full((N * H * W * ld + GUARD,), -7 if bf else float("nan"),
                     dtype=torch.int16 if bf else torch.float32, device=dev)
    f = frame_of(srcs, N, H, W)
    if bf and ldo:
        L.call("pmu_frame_to_bf16_ld", f, Cpad, buf.data_ptr(), ldo, L.stream())
    elif bf:
        L.call("pmu_frame_to_bf16", f, Cpad, buf.data_ptr(), L.stream())
    elif ldo:
        L.call("pmu_frame_to_f32_ld", f, buf.data_ptr(), ldo, L.stream())
    else:
        L.call("pmu_frame_to_f32", f, buf.data_ptr(), L.stream())
    torch.cuda.synchronize()
    return buf


def _untouched(t):
    return bool((t == -7).all()) if t.dtype == torch.int16 else bool(torch.isnan(t).all())


def _same_bits(a, b):
    return torch.equal(a, b) if a.dtype == torch.int16 else torch.equal(a.view(torch.int32), b.view(torch.int32))


def _compare(out, ref64, bf, where):
    """out (..., C) against the float64 reference: fp32 exactly; bf16 the reference's RNE bits."""
    if not bf:
        assert_exact(out, ref64, where)
        return
    want = bf16_bits(ref64)
    got = out.cpu()
    if not torch.equal(got, want):
        assert_exact(got.view(torch.bfloat16).float(), want.view(torch.bfloat16).double(), where + " (bf16, RNE)")
        raise AssertionError(f"{where}: bf16 bits differ from the reference's only in the sign of a zero")


def _check(dev, cpu_srcs, N, H, W, bf, stream, where, xb=(False, False), zb=(False, False), Cpad=None, ldo=None,
           census=False):
    C = sum(s.x.shape[3] for s in cpu_srcs)
    width = (Cpad or (C + 3) // 4 * 4) if bf else C
    ld = ldo or width
    ref = ref_frame(cpu_srcs, N, H, W)
    assert torch.equal(ref.float().double(), ref), where      # the reference is an fp32 number everywhere
    if census and bf:
        assert_rne_exercised(ref, where)
    srcs = [_on(dev, s, xb[i], zb[i]) for i, s in enumerate(cpu_srcs)]
    with _env("PMU_FRAME_STREAM", stream):
        a = _launch(srcs, N, H, W, bf, width, ldo, dev)
        b = _launch(srcs, N, H, W, bf, width, ldo, dev)
    assert _same_bits(a, b), f"{where}: two runs differ"
    P = N * H * W
    out = a[:P * ld].view(N, H, W, ld)
    assert _untouched(a[P * ld:]), f"{where}: wrote past the end of the output"
    assert _untouched(out[..., width:]), f"{where}: wrote channels outside [0, {width})"
    if bf and width > C:
        assert bool((out[..., C:width] == 0).all()), f"{where}: padding channels [{C}, {width}) are not +0"
    _compare(out[..., :C], ref, bf, where)


STREAM = [None, "0"]
BF = [True, False]


# ------------------------------------------------------------------------------------------ small cases
@pytest.mark.parametrize("stream", STREAM)
@pytest.mark.parametrize("bf", BF)
@pytest.mark.parametrize("C", [8, 16, 32, 64, 128, 256, 512, 1024, 2048])
def test_flat_bnrelu_every_unit_count(dev, C, bf, stream):
    g = torch.Generator().manual_seed(100 + C)
    _check(dev, [bnrelu(g, 2, 5, 7, C)], 2, 5, 7, bf, stream, f"flat BNRELU C={C}")


@pytest.mark.parametrize("stream", STREAM)
@pytest.mark.parametrize("bf", BF)
@pytest.mark.parametrize("C", [24, 12, 6, 3])
def test_flat_raw_generic_paths(dev, C, bf, stream):
    """Unit counts that are no power of two (generic fast kernel), C % 8 != 0 (float4 kernel) and C % 4 != 0
    (scalar reads; the bf16 operand padded to a multiple of 4).  RAW values here are multiples of 2^-8 in
    [-4, 4] (up to eleven significant bits), so these kernels' bf16 stores round, with ties in both directions."""
    g = torch.Generator().manual_seed(200 + C)
    src = S(torch.randint(-1024, 1025, (3, 7, 9, C), generator=g).float() / 256)
    _check(dev, [src], 3, 7, 9, bf, stream, f"flat RAW C={C}", census=True)


@pytest.mark.parametrize("stream", STREAM)
@pytest.mark.parametrize("bf", BF)
@pytest.mark.parametrize("C", [64, 1024])
@pytest.mark.parametrize("Hs,Ws", [(8, 12), (9, 13)])
def test_max2_of_bnrelu(dev, Hs, Ws, C, bf, stream):
    g = torch.Generator().manual_seed(300 + Hs + C)
    _check(dev, [bnrelu(g, 2, Hs, Ws, C, POOL_MAX2)], 2, 4, 6, bf, stream, f"MAX2 BNRELU {Hs}x{Ws} C={C}")


@pytest.mark.parametrize("stream", STREAM)
@pytest.mark.parametrize("bf", BF)
def test_max2_of_raw(dev, bf, stream):
    g = torch.Generator().manual_seed(400)
    _check(dev, [raw(g, 1, 6, 10, 16, POOL_MAX2)], 1, 3, 5, bf, stream, "MAX2 RAW")


@pytest.mark.parametrize("stream", STREAM)
@pytest.mark.parametrize("bf", BF)
@pytest.mark.parametrize("C", [8, 12, 6])
def test_avg2ceil_of_bnrelu_odd_source(dev, C, bf, stream):
    """7 x 9 -> 4 x 5: windows of 4, 2 (last column), 2 (last row) and 1 (the corner) elements."""
    g = torch.Generator().manual_seed(500 + C)
    _check(dev, [bnrelu(g, 2, 7, 9, C, POOL_AVG2CEIL)], 2, 4, 5, bf, stream, f"AVG2CEIL BNRELU C={C}")


@pytest.mark.parametrize("stream", STREAM)
@pytest.mark.parametrize("bf", BF)
@pytest.mark.parametrize("N,H,W,C", [(2, 13, 11, 64), (5, 3, 3, 16)])
def test_bnbwd_f32_da(dev, N, H, W, C, bf, stream):
    g = torch.Generator().manual_seed(600 + C)
    _check(dev, [bnbwd(g, N, H, W, C)], N, H, W, bf, stream, f"BNBWD fp32 da C={C}", census=True)


@pytest.mark.parametrize("stream", STREAM)
@pytest.mark.parametrize("bf", BF)
@pytest.mark.parametrize("N,H,W,C", [(3, 17, 23, 128), (1, 8, 8, 1024)])
def test_bnbwd_bf16_da(dev, N, H, W, C, bf, stream):
    """da stored as bf16 (PMU_DT_X_BF16): the streaming XB kernel and the generic one."""
    g = torch.Generator().manual_seed(700 + C)
    _check(dev, [bnbwd(g, N, H, W, C)], N, H, W, bf, stream, f"BNBWD bf16 da C={C}", xb=(True, False), census=True)


@pytest.mark.parametrize("stream", STREAM)
@pytest.mark.parametrize("bf", BF)
@pytest.mark.parametrize("kind", ["bnrelu_xb", "bnbwd_zb", "bnbwd_xb_zb"])
def test_bf16_stored_sources(dev, kind, bf, stream):
    """A BN+ReLU source whose z is stored as bf16, and BN-backward sources with a bf16 z (and a bf16 da as well):
    stream_ok refuses all three, so both settings run the generic kernels' bf16 reads."""
    g = torch.Generator().manual_seed(800 + len(kind))
    N, H, W, C = 2, 6, 10, 32
    if kind == "bnrelu_xb":
        _check(dev, [bnrelu(g, N, H, W, C)], N, H, W, bf, stream, kind, xb=(True, False))
    else:
        _check(dev, [bnbwd(g, N, H, W, C)], N, H, W, bf, stream, kind, xb=(kind == "bnbwd_xb_zb", False),
               zb=(True, False), census=True)


@pytest.mark.parametrize("stream", STREAM)
@pytest.mark.parametrize("bf", BF)
@pytest.mark.parametrize("off", [(0, 1), (1, 2)])
@pytest.mark.parametrize("C0,C1", [(8, 12), (12, 8)])
def test_concat_skip_and_padded_up(dev, C0, C1, off, bf, stream):
    """torch.cat([skip, F.pad(up)], 1): the up-sampled source (8 x 10) sits at off inside the 9 x 12 frame and
    reads as zero around it."""
    g = torch.Generator().manual_seed(900 + C0 + off[0])
    N, H, W = 2, 9, 12
    _check(dev, [bnrelu(g, N, H, W, C0), raw(g, N, 8, 10, C1, off=off)], N, H, W, bf, stream,
           f"concat {C0}+{C1} at {off}")


@pytest.mark.parametrize("stream", STREAM)
@pytest.mark.parametrize("bf", BF)
@pytest.mark.parametrize("C0,C1", [(16, 8), (8, 4)])
def test_concat_pooled_skip_and_up(dev, C0, C1, bf, stream):
    g = torch.Generator().manual_seed(1000 + C0)
    N, H, W = 2, 5, 6
    _check(dev, [bnrelu(g, N, 10, 12, C0, POOL_MAX2), raw(g, N, 5, 4, C1, off=(0, 1))], N, H, W, bf, stream,
           f"concat pooled {C0}+{C1}")


@pytest.mark.parametrize("bf", BF)
@pytest.mark.parametrize("C", [16, 12, 6])
def test_max2_of_odd_source_inside_a_larger_frame(dev, C, bf):
    """Floor-mode pooling of a 9 x 13 map gives 4 x 6; in a 5 x 7 frame the last row and column lie outside the
    pooled source and read as zero — the window that would start on the odd last row / column is no window.
    (The stored tensor is followed by one more image of large values inside the same allocation, so a kernel
    that formed that window anyway would read those, in bounds, and return them.)"""
    from pmu_hip.engine import Src
    g = torch.Generator().manual_seed(1500 + C)
    N, Hs, Ws, H, W = 2, 9, 13, 5, 7
    s = bnrelu(g, N, Hs, Ws, C, POOL_MAX2)
    ref = ref_frame([s], N, H, W)
    assert bool((ref[:, 4] == 0).all()) and bool((ref[:, :, 6] == 0).all()) and float(ref.max()) > 0
    buf = torch.cat([s.x.reshape(-1), torch.full((Hs * Ws * C,), 1.5)]).to(dev)
    src = Src(buf[:s.x.numel()].view(N, Hs, Ws, C), s.mode, s.coef.to(dev), pool=POOL_MAX2)
    width = (C + 3) // 4 * 4 if bf else C
    a = _launch([src], N, H, W, bf, width, None, dev)
    b = _launch([src], N, H, W, bf, width, None, dev)
    assert _same_bits(a, b) and _untouched(a[N * H * W * width:])
    _compare(a[:N * H * W * width].view(N, H, W, width)[..., :C], ref, bf, f"MAX2 of odd source in a larger frame C={C}")


@pytest.mark.parametrize("stream", STREAM)
@pytest.mark.parametrize("Cs,Cpad", [((8, 12), 24), ((12,), 16), ((8, 4), 16)])
def test_bf16_operand_padding_channels_are_zero(dev, Cs, Cpad, stream):
    g = torch.Generator().manual_seed(1100 + Cpad + len(Cs))
    N, H, W = 2, 5, 7
    srcs = [bnrelu(g, N, H, W, Cs[0])] + [raw(g, N, H, W, c) for c in Cs[1:]]
    _check(dev, srcs, N, H, W, True, stream, f"Cpad {sum(Cs)} -> {Cpad}", Cpad=Cpad)


@pytest.mark.parametrize("stream", STREAM)
@pytest.mark.parametrize("bf", BF)
@pytest.mark.parametrize("kind,C,ldo", [("flat", 64, 128), ("flat", 256, 512), ("pool", 128, 256)])
def test_ld_forms(dev, kind, C, ldo, bf, stream):
    """The frame into the first channels of a wider tensor: channels [C, ldo) keep their sentinel."""
    g = torch.Generator().manual_seed(1200 + C)
    N, H, W = 2, 10, 6
    src = bnrelu(g, N, 2 * H, 2 * W, C, POOL_MAX2) if kind == "pool" else bnrelu(g, N, H, W, C)
    _check(dev, [src], N, H, W, bf, stream, f"_ld {kind} C={C} ldo={ldo}", ldo=ldo)


@pytest.mark.parametrize("stream", STREAM)
def test_f32_ld_with_unaligned_stride(dev, stream):
    """ldo % 8 == 4: pmu_frame_to_f32_ld's non-streaming branch whatever the setting."""
    g = torch.Generator().manual_seed(1300)
    _check(dev, [bnrelu(g, 2, 5, 7, 8)], 2, 5, 7, False, stream, "fp32 _ld C=8 ldo=12", ldo=12)


def _pool_skip(dev, src_cpu, N, H, W, Ccat, bf, ref_pool=None, ref_skip=None, ref_device="cpu"):
    """pmu_frame_to_{bf16,f32}_pool_skip on the pooled frame of src_cpu (source 2H x 2W): the pooled operand and
    the unpooled activation in the first C channels of an (N, 2H, 2W, Ccat) tensor, both against ref_frame."""
    from pmu_hip import _lib as L
    from pmu_hip.engine import frame_of
    C = src_cpu.x.shape[3]
    src = src_cpu if src_cpu.x.device.type != "cpu" else _on(dev, src_cpu)
    f = frame_of([src], N, H, W)
    assert L.lib().pmu_frame_pool_skip_ok(f)
    dt, fill = (torch.int16, -7) if bf else (torch.float32, float("nan"))
    bufs = []
    for _ in range(2):
        pooled = torch.full((N * H * W * C + GUARD,), fill, dtype=dt, device=dev)
        cat = torch.full((N * 4 * H * W * Ccat + GUARD,), fill, dtype=dt, device=dev)
        if bf:
            L.call("pmu_frame_to_bf16_pool_skip", f, pooled.data_ptr(), cat.data_ptr(), Ccat, L.stream())
        else:
            L.call("pmu_frame_to_f32_pool_skip", f, pooled.data_ptr(), cat.data_ptr(), Ccat, L.stream())
        torch.cuda.synchronize()
        bufs.append((pooled, cat))
    (pooled, cat), (p2, c2) = bufs
    assert _same_bits(pooled, p2) and _same_bits(cat, c2), "two runs differ"
    assert _untouched(pooled[-GUARD:]) and _untouched(cat[-GUARD:])
    cat4 = cat[:-GUARD].view(N, 2 * H, 2 * W, Ccat)
    assert _untouched(cat4[..., C:]), "pool_skip wrote concat channels beyond the skip half"
    if ref_pool is None:
        ref_pool = ref_frame([src_cpu], N, H, W, device=ref_device)
        ref_skip = ref_frame([src_cpu._replace(pool=POOL_NONE)], N, 2 * H, 2 * W, device=ref_device)
    return pooled[:-GUARD].view(N, H, W, C), cat4[..., :C], ref_pool, ref_skip


@pytest.mark.parametrize("bf", BF)
@pytest.mark.parametrize("N,H,W,C,Ccat", [(2, 8, 8, 64, 128), (3, 5, 7, 128, 192), (1, 16, 4, 8, 16)])
def test_pool_skip_forms(dev, N, H, W, C, Ccat, bf):
    """(Streaming only: with PMU_FRAME_STREAM=0 pmu_frame_pool_skip_ok refuses the frame.)"""
    g = torch.Generator().manual_seed(1400 + C)
    src = bnrelu(g, N, 2 * H, 2 * W, C, POOL_MAX2)
    with _env("PMU_FRAME_STREAM", None):
        pooled, skip, ref_pool, ref_skip = _pool_skip(dev, src, N, H, W, Ccat, bf)
    _compare(pooled, ref_pool, bf, "pool_skip pooled operand")
    _compare(skip, ref_skip, bf, "pool_skip skip half")


# ------------------------------------------------------------------------------------------ large cases
def _loop_repeats(dev, P, C, U):
    """The strict inequality under which frame_stream_kernel's loop body runs a second time for block 0."""
    cus = torch.cuda.get_device_properties(dev).multi_processor_count
    lg = (C // 8).bit_length() - 1
    need = 2 * U * (256 >> lg) * 8 * cus
    assert P > need, (f"{P} frame pixels do not make the streaming loop repeat on {cus} CUs (needs more than {need}): "
                      "enlarge this case")


def _large_compare(out, ref64_dev, bf, where):
    """As _compare with the reference on the device (the failure message is formed on the CPU)."""
    if bf:
        ok = torch.equal(out, bf16_bits(ref64_dev))
    else:
        ok = torch.equal(out.double(), ref64_dev)
    if not ok:
        _compare(out, ref64_dev.cpu(), bf, where)
        raise AssertionError(where)


def _large_run(dev, src, N, H, W, bf, where, ref):
    C = src.x.shape[3]
    with _env("PMU_FRAME_STREAM", None):
        a = _launch([src], N, H, W, bf, C, None, dev)
        b = _launch([src], N, H, W, bf, C, None, dev)
    assert _same_bits(a, b), f"{where}: two runs differ"
    assert _untouched(a[-GUARD:]), f"{where}: wrote past the end of the output"
    _large_compare(a[:-GUARD].view(N, H, W, C), ref, bf, where)


def _dev_src(dev, s, xb=False):
    from pmu_hip.engine import Src
    x = bf16_bits(s.x) if xb else s.x
    return Src(x.contiguous().to(dev), s.mode, s.coef.to(dev), z=None if s.z is None else s.z.to(dev), pool=s.pool)


def test_large_flat_bnrelu_second_iteration(dev):
    """C = 2048 (one pixel per U-slice), 91 x 91 = 8281 pixels > 2 * 2 * 1 * 8 * 256: the plain flat kernel's
    second loop iteration, bf16 and fp32 output (source 68 MB: plain loads and stores)."""
    N, H, W, C = 1, 91, 91, 2048
    _loop_repeats(dev, N * H * W, C, 2)
    g = torch.Generator().manual_seed(2001)
    s = bnrelu(g, N, H, W, C)
    src = _dev_src(dev, s)
    ref = ref_frame([S(src.x, s.mode, src.coef)], N, H, W, device=dev)
    for bf in BF:
        _large_run(dev, src, N, H, W, bf, f"large flat BNRELU bf={bf}", ref)


def test_large_bnbwd_bf16_da_nontemporal(dev):
    """C = 2048, 129 x 128 = 16512 pixels (no multiple of the 4096-pixel step), da stored as bf16, bf16 output:
    the shipped library's nontemporal XB kernel (the source counts 128 MiB at 4 bytes per element) in its second
    iteration."""
    N, H, W, C = 1, 129, 128, 2048
    assert N * H * W * C * 4 >= 128 << 20
    _loop_repeats(dev, N * H * W, C, 2)
    g = torch.Generator().manual_seed(2002)
    s = bnbwd(g, N, H, W, C)
    assert bf16_exact(s.x)
    src = _dev_src(dev, s, xb=True)
    ref = ref_frame([S(s.x.to(dev), s.mode, src.coef, src.z)], N, H, W, device=dev)
    _large_run(dev, src, N, H, W, True, "large BNBWD bf16 da", ref)


def test_large_max2_nontemporal_and_pool_skip(dev):
    """C = 2048, source 130 x 134 -> 65 x 67 = 4355 pooled pixels > 2 * 1 * 1 * 8 * 256 and 35.7 M source elements
    (>= 128 MiB): the nontemporal pooled kernel in its second iteration (bf16), the same through
    pmu_frame_to_bf16_pool_skip (the nontemporal SKIP instantiation), and the plain pooled kernel (fp32)."""
    N, H, W, C = 1, 65, 67, 2048
    assert N * 2 * H * 2 * W * C * 4 >= 128 << 20
    _loop_repeats(dev, N * H * W, C, 1)
    g = torch.Generator().manual_seed(2003)
    s = bnrelu(g, N, 2 * H, 2 * W, C, POOL_MAX2)
    src = _dev_src(dev, s)
    on_dev = S(src.x, s.mode, src.coef, None, POOL_MAX2)
    ref = ref_frame([on_dev], N, H, W, device=dev)
    for bf in BF:
        _large_run(dev, src, N, H, W, bf, f"large MAX2 bf={bf}", ref)
    ref_skip = ref_frame([on_dev._replace(pool=POOL_NONE)], N, 2 * H, 2 * W, device=dev)
    with _env("PMU_FRAME_STREAM", None):
        pooled, skip, _, _ = _pool_skip(dev, src, N, H, W, C, True, ref, ref_skip)
    _large_compare(pooled, ref, True, "large pool_skip pooled operand")
    _large_compare(skip, ref_skip, True, "large pool_skip skip half")


# ------------------------------------------------------------------------------------------ nontemporal, small
@pytest.mark.parametrize("bf", BF)
@pytest.mark.parametrize("kind", ["flat", "pool", "pool_odd", "bnbwd", "bnbwd_xb", "raw"])
def test_small_cases_nontemporal(exp_lib, dev, kind, bf):
    """The experiments library honours PMU_FRAME_NT: the small cases once more with every streaming launch
    nontemporal — the ragged tails of those kernels and their fp32-output forms, against the same references."""
    g = torch.Generator().manual_seed(3000 + len(kind))
    N, H, W, C = 2, 5, 7, 64
    xb = False
    if kind == "flat":
        src = bnrelu(g, N, H, W, C)
    elif kind == "raw":
        src = raw(g, N, H, W, C)
    elif kind in ("pool", "pool_odd"):
        odd = int(kind == "pool_odd")
        src = bnrelu(g, N, 2 * H + odd, 2 * W + odd, C, POOL_MAX2)
    else:
        src, xb = bnbwd(g, N, H, W, C), kind == "bnbwd_xb"
    with _env("PMU_FRAME_NT", "3"):
        _check(dev, [src], N, H, W, bf, None, f"nontemporal {kind}", xb=(xb, False))
