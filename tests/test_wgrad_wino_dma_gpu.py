"""The F(2x2) weight gradient's K-tile staging (csrc/wgrad3x3_wino.hip): buffer loads to LDS whose addresses
are a descriptor, a scalar offset per wave-instruction and a per-lane offset set once, zeros coming from the
descriptors' range check.

Exact cases: operands on helpers.grid_data, where every partial sum of every summation order is an fp32
number (the conditions of tests/test_exact_gpu.py::wgrad_case, checked there per case from the float64
reference alone), so the kernel must return the float64 direct sum bit for bit: a pixel fetched from the
wrong row, a halo column that is not zero, a unit left unwritten in LDS shows at a known (co, ci, kh, kw).
Shapes (N, H, W, Cin, Cout), K-tiles of 8 x 16 pixels, blocks of 64 input x 32 / 64 output channels:
  (1, 5, 7, 64, 32)      a map smaller than one K-tile; the 32-channel (512-thread) kernel
  (2, 8, 16, 64, 64)     exactly one K-tile per image: every halo edge outside the image
  (3, 9, 17, 64, 64)     one row and one column past a tile; three images: split-K ranges of unequal length
  (1, 24, 48, 128, 128)  3 x 3 K-tiles with an interior one; channel blocks with non-zero origins on both operands
  (1, 16, 32, 64, 128)   a second output-channel block
  (2, 17, 33, 64, 64)    both edges ragged
Stray reads: the same cases with dz and x as views into the middle of NaN-filled allocations (at least one
image row of NaN on either side) and NaN in the workspace and dw: a source address that leaves the tensor
puts a NaN into dw.  Each case runs twice and must repeat its bits.  Random data: one case per kernel width
against float64 at tests/test_wino_gpu.py's bound.  Operands of 2^31 bytes or more keep the per-lane 64-bit
addresses: the host predicate is checked on computed sizes, and in the experiments library PMU_WGW_SDMA=0
forces that path, which must give the bits of the descriptor path.
"""
import os

import pytest
import torch

from helpers import assert_exact
from test_exact_gpu import wgrad_case

pytestmark = pytest.mark.gpu

TOL = 2e-5   # of max |ref| (tests/test_wino_gpu.py)
GUARD = 4096
SHAPES = [(1, 5, 7, 64, 32), (2, 8, 16, 64, 64), (3, 9, 17, 64, 64), (1, 24, 48, 128, 128), (1, 16, 32, 64, 128),
          (2, 17, 33, 64, 64)]


def _inside_nan(t, dev):
    """t (N, H, W, C) on the device as a view into the middle of a NaN-filled allocation: two image rows of
    NaN before and after it."""
    pad = 2 * t.shape[2] * t.shape[3]
    buf = torch.full((pad + t.numel() + pad,), float("nan"), device=dev)
    v = buf[pad:pad + t.numel()].view(t.shape)
    v.copy_(t)
    assert v.data_ptr() % 16 == 0 and bool(torch.isnan(buf[:pad]).all()) and bool(torch.isnan(buf[-pad:]).all())
    return buf, v


def _wgrad(L, dz, x, dev, where):
    """One call with a NaN workspace of the queried size (and a guard behind it) and a NaN dw."""
    N, H, W, Cout = dz.shape
    Cin = x.shape[3]
    wsb = L.lib().pmu_conv3x3_wgrad_ws_wino(N, H, W, Cin, Cout)
    assert wsb > 0 and wsb % 4 == 0
    ws = torch.full((wsb + GUARD,), 0xA5, dtype=torch.uint8, device=dev)
    ws[:wsb].view(torch.float32).fill_(float("nan"))
    dw = torch.full((Cout, Cin, 3, 3), float("nan"), device=dev)
    L.call("pmu_conv3x3_wgrad_wino", dz.data_ptr(), x.data_ptr(), N, H, W, Cout, Cin, dw.data_ptr(), ws.data_ptr(), wsb,
           L.stream())
    torch.cuda.synchronize()
    assert bool((ws[wsb:] == 0xA5).all()), f"{where}: wrote past its {wsb}-byte workspace"
    return dw


def _twice(L, dz, x, dev, where):
    a, b = _wgrad(L, dz, x, dev, where), _wgrad(L, dz, x, dev, where)
    assert torch.equal(a.view(torch.int32), b.view(torch.int32)), f"{where}: the second call's bits differ from the first's"
    return a


@pytest.mark.parametrize("N,H,W,Cin,Cout", SHAPES)
def test_wgrad_wino_staging_exact(dev, N, H, W, Cin, Cout):
    from pmu_hip import _lib as L
    assert L.lib().pmu_conv3x3_wgrad_wino_dma_ok(N, H, W, Cin, Cout) == 1
    c = wgrad_case("data", N, H, W, Cin, Cout, wino=True)
    where = f"pmu_conv3x3_wgrad_wino {(N, H, W, Cin, Cout)}"
    assert_exact(_twice(L, c.dz.to(dev), c.x.to(dev), dev, where), c.dw64, where)


@pytest.mark.parametrize("N,H,W,Cin,Cout", SHAPES)
def test_wgrad_wino_staging_reads_inside_the_tensors(dev, N, H, W, Cin, Cout):
    from pmu_hip import _lib as L
    c = wgrad_case("data", N, H, W, Cin, Cout, wino=True)
    where = f"pmu_conv3x3_wgrad_wino {(N, H, W, Cin, Cout)}, operands inside NaN"
    dbuf, dz = _inside_nan(c.dz, dev)
    xbuf, x = _inside_nan(c.x, dev)
    dw = _twice(L, dz, x, dev, where)
    assert not bool(torch.isnan(dw).any()), f"{where}: a NaN from outside the operands reached dw"
    assert_exact(dw, c.dw64, where)
    assert torch.equal(dz.cpu(), c.dz) and torch.equal(x.cpu(), c.x)


@pytest.mark.parametrize("N,H,W,Cin,Cout", [(2, 19, 37, 64, 96), (2, 19, 37, 128, 64)])
def test_wgrad_wino_staging_random(dev, N, H, W, Cin, Cout):
    """The 32-channel kernel (Cout % 64 != 0) and the 64-channel one on random data, against float64."""
    from pmu_hip import _lib as L
    g = torch.Generator().manual_seed(11 + Cin + Cout)
    x = torch.randn(N, H, W, Cin, generator=g)
    dz = torch.randn(N, H, W, Cout, generator=g)
    ref = torch.nn.grad.conv2d_weight(x.permute(0, 3, 1, 2).double(), (Cout, Cin, 3, 3), dz.permute(0, 3, 1, 2).double(),
                                      padding=1)
    dw = _wgrad(L, dz.to(dev), x.to(dev), dev, f"random {(N, H, W, Cin, Cout)}")
    err = float((dw.double().cpu() - ref).abs().max() / ref.abs().max())
    print(f"wgrad_wino random {(N, H, W, Cin, Cout)}: max |d| / max |ref| = {err:.3g} (bound {TOL:g})")
    assert err <= TOL


def test_wgrad_wino_dma_ok_sizes(dev):
    """The descriptor path takes operands below 2^31 bytes each (4 N H W C): c2's largest (1.07 GB) pass, an
    operand of exactly 2^31 bytes does not, and either operand alone decides."""
    from pmu_hip import _lib as L
    ok = L.lib().pmu_conv3x3_wgrad_wino_dma_ok
    assert ok(32, 256, 256, 64, 128) == 1 and ok(32, 256, 256, 128, 64) == 1      # 2^30 bytes
    assert 4 * 8191 * 1024 * 64 == 2 ** 31 - 4 * 1024 * 64
    assert ok(1, 8191, 1024, 64, 64) == 1
    assert ok(1, 8192, 1024, 64, 64) == 0                                           # 2^31 bytes each
    assert ok(64, 256, 256, 128, 64) == 0 and ok(64, 256, 256, 64, 128) == 0        # x / dz alone at 2^31
    assert ok(32, 512, 512, 64, 64) == 0
    assert ok(0, 8, 16, 64, 64) == 0


@pytest.mark.parametrize("N,H,W,Cin,Cout", [SHAPES[0], SHAPES[2]])
def test_wgrad_wino_per_lane_path_same_bits(dev, exp_lib, N, H, W, Cin, Cout):
    """Experiments library: PMU_WGW_SDMA=0 (read per call) stages with per-lane addresses, the path of the
    large operands; its bits are the descriptor path's, and both are exact."""
    from pmu_hip import _lib as L
    c = wgrad_case("data", N, H, W, Cin, Cout, wino=True)
    dz, x = c.dz.to(dev), c.x.to(dev)
    where = f"pmu_conv3x3_wgrad_wino {(N, H, W, Cin, Cout)}"
    assert "PMU_WGW_SDMA" not in os.environ
    new = _twice(L, dz, x, dev, where + " descriptors")
    os.environ["PMU_WGW_SDMA"] = "0"
    try:
        old = _twice(L, dz, x, dev, where + " per-lane addresses")
    finally:
        del os.environ["PMU_WGW_SDMA"]
    assert torch.equal(new.view(torch.int32), old.view(torch.int32)), where + ": the two staging paths differ"
    assert_exact(old, c.dw64, where + " per-lane addresses")
