"""helpers.ref_frame — the float64 CPU restatement of pmu_frame (include/pmunet_hip.h) the kernel tests
compare against — pinned to torch's own operators, so the reference does not depend on the library:
BN+ReLU, F.max_pool2d(., 2), F.avg_pool2d(., 2, 2, ceil_mode=True), F.pad + torch.cat, on odd and even
source sizes; and the BN+ReLU backward source against autograd of the same expression."""
from collections import namedtuple

import pytest
import torch
import torch.nn.functional as F

from helpers import (POOL_AVG2CEIL, POOL_MAX2, POOL_NONE, SRC_BNBWD, SRC_BNRELU, SRC_RAW, quant_bn, quant_z,
                     ref_frame, ulp32)

S = namedtuple("S", "x mode coef z pool off", defaults=(SRC_RAW, None, None, POOL_NONE, (0, 0)))


def _nchw(t):
    return t.permute(0, 3, 1, 2)


def _nhwc(t):
    return t.permute(0, 2, 3, 1)


def _act(z, coef):
    C = z.shape[3]
    return torch.relu(z.double() * coef[:C].double() + coef[C:].double())


@pytest.mark.parametrize("Hs,Ws", [(6, 8), (7, 9), (7, 8), (2, 3), (1, 1)])
@pytest.mark.parametrize("C", [3, 8])
def test_ref_frame_modes_and_pools_match_torch(Hs, Ws, C):
    g = torch.Generator().manual_seed(Hs * 100 + Ws * 10 + C)
    N = 2
    z, coef = quant_z(N, Hs, Ws, C, g), quant_bn(C, g)
    x = torch.randn(N, Hs, Ws, C, generator=g)
    assert torch.equal(ref_frame([S(x)], N, Hs, Ws), x.double())
    act = _act(z, coef)
    assert torch.equal(ref_frame([S(z, SRC_BNRELU, coef)], N, Hs, Ws), act)
    if Hs >= 2 and Ws >= 2:
        want = _nhwc(F.max_pool2d(_nchw(act), 2))
        assert torch.equal(ref_frame([S(z, SRC_BNRELU, coef, None, POOL_MAX2)], N, Hs // 2, Ws // 2), want)
    want = _nhwc(F.avg_pool2d(_nchw(act), 2, 2, ceil_mode=True))
    got = ref_frame([S(z, SRC_BNRELU, coef, None, POOL_AVG2CEIL)], N, (Hs + 1) // 2, (Ws + 1) // 2)
    assert want.shape == got.shape and float((got - want).abs().max()) <= 1e-15
    # the same on ordinary randn inputs (no exact grid)
    zr = torch.randn(N, Hs, Ws, C, generator=g)
    cr = torch.cat([torch.rand(C, generator=g) + 0.5, torch.randn(C, generator=g) * 0.2])
    want = _nhwc(F.avg_pool2d(_nchw(_act(zr, cr)), 2, 2, ceil_mode=True))
    got = ref_frame([S(zr, SRC_BNRELU, cr, None, POOL_AVG2CEIL)], N, (Hs + 1) // 2, (Ws + 1) // 2)
    assert float((got - want).abs().max()) <= 1e-15


@pytest.mark.parametrize("H,W,off", [(8, 10, (0, 0)), (9, 11, (1, 0)), (9, 12, (0, 2)), (9, 12, (1, 1))])
def test_ref_frame_pad_and_concat_match_torch(H, W, off):
    """torch.cat([skip, F.pad(up)], 1) of Up (unet_parts.py:58-66): the up-sampled source is smaller than
    the frame and sits at (off_h, off_w); the pooled skip of a Down block likewise."""
    g = torch.Generator().manual_seed(H * 31 + W)
    N, C0, C1 = 2, 5, 3
    Hu, Wu = 8, 10
    zs, cs = quant_z(N, H, W, C0, g), quant_bn(C0, g)
    up = torch.randn(N, Hu, Wu, C1, generator=g)
    oh, ow = off
    padded = _nhwc(F.pad(_nchw(up.double()), (ow, W - Wu - ow, oh, H - Hu - oh)))
    want = torch.cat([_act(zs, cs), padded], dim=3)
    got = ref_frame([S(zs, SRC_BNRELU, cs), S(up, off=off)], N, H, W)
    assert torch.equal(got, want)
    # a max-pooled source placed with an offset
    zp = quant_z(N, 2 * Hu + 1, 2 * Wu, C0, g)
    wantp = _nhwc(F.pad(F.max_pool2d(_nchw(_act(zp, cs)), 2), (ow, W - Wu - ow, oh, H - Hu - oh)))
    assert torch.equal(ref_frame([S(zp, SRC_BNRELU, cs, None, POOL_MAX2, off)], N, H, W), wantp)


def test_ref_frame_bnbwd_matches_autograd_form():
    """BNBWD = scale*g + kx*(z - mean) + kc with g = da where relu'(z*scale + shift) is 1: the first term is
    autograd's gradient of sum(da * relu(z*scale + shift)) w.r.t. z."""
    g = torch.Generator().manual_seed(5)
    N, H, W, C = 2, 5, 7, 6
    z, coef = quant_z(N, H, W, C, g), quant_bn(C, g, bwd=True)
    da = torch.randn(N, H, W, C, generator=g)
    sc, sh, mu, kx, kc = coef.double().view(5, C)
    zz = z.double().requires_grad_(True)
    (da.double() * torch.relu(zz * sc + sh)).sum().backward()
    want = zz.grad + kx * (z.double() - mu) + kc
    got = ref_frame([S(da, SRC_BNBWD, coef, z)], N, H, W)
    assert float((got - want).abs().max()) <= 1e-14


def test_quantised_inputs_are_exact_in_fp32_and_hold_ties():
    g = torch.Generator().manual_seed(1)
    N, H, W, C = 2, 9, 11, 8
    z, coef = quant_z(N, H, W, C, g), quant_bn(C, g)
    pre32 = z * coef[:C] + coef[C:]
    pre64 = z.double() * coef[:C].double() + coef[C:].double()
    assert torch.equal(pre32.double(), pre64)
    act = torch.relu(pre64)
    win = act[:, :8, :10].reshape(N, 4, 2, 5, 2, C).permute(0, 1, 3, 5, 2, 4).reshape(-1, 4)
    top = win.topk(2, dim=1).values
    assert int((top[:, 0] == top[:, 1]).sum()) > win.shape[0] // 8       # exact ties at the maximum
    assert int((win.max(dim=1).values == 0).sum()) > 0                   # all-zero windows after ReLU
    assert int((pre64 == 0).sum()) > 0                                   # z*scale + shift exactly zero
    assert float(ulp32(torch.tensor([1.0, 1.5, 0.75, 3.0], dtype=torch.float64)).sub(
        torch.tensor([2.0 ** -23, 2.0 ** -23, 2.0 ** -24, 2.0 ** -22], dtype=torch.float64)).abs().max()) == 0
