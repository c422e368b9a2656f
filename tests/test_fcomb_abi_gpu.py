"""pmu_fcomb_fwd and pmu_fcomb_bwd (csrc/fcomb.hip) by direct calls at the bounds of the ABI in
include/pmunet_hip.h: K up to 32 classes (the MFMA last layer pads to 32 rows; tests elsewhere stop at 5),
latent widths other than 6 (0: the first layer has no z columns and z is never read; 12), a feature width
that is no multiple of 4 (guarded scalar row loads), 1 to 3 hidden layers, and S = 3 samples with distinct z
in one forward launch.

Method: that of test_probunet_gpu.py::test_fcomb_fwd_bwd_vs_fp64_oracle's quantised case.  Weights are
multiples of 1/8 in [-1/4, 1/4], biases multiples of 1/16, features multiples of 1/4 in [0, 1], z multiples of
1/4 in [-2, 2]: layer 1's pre-activations are multiples of 1/32 below 2^5, layer 2's multiples of 2^-8 below
2^9, layer 3's multiples of 2^-11 below 2^13 — float32 values in any summation order — so the ReLU masks of
the fp32 kernels and of the float64 reference are identical (zb = W_1z . z + b_1 is formed on the CPU and is
exact too).  What is left is the fp32 rounding of the last layer and of the gradient sums, held to the
project's Fcomb tolerance 1e-4 max(1, max|ref|) per tensor; a skipped class row, a wrong stride or a sample
reading another sample's zb is an O(1) error there.  Every output is NaN on entry (dw, db, dwl, dbl are
overwritten, not accumulated), the workspace has pmu_fcomb_bwd_ws bytes followed by a sentinel tail that
must stay untouched, and dz is passed as NULL once."""
import ctypes

import pytest
import torch

pytestmark = pytest.mark.gpu

NAN = float("nan")
S = 3
TAIL = 64
# (F, K, NH, Lz, N, H, W)
CASES = [(64, 32, 3, 6, 2, 9, 7), (64, 9, 3, 6, 1, 33, 5), (30, 8, 2, 0, 2, 6, 11), (16, 5, 1, 12, 3, 4, 4)]


def _L():
    from pmu_hip import _lib as L
    return L


def _ptrs(ts):
    return (ctypes.c_void_p * 3)(*([t.data_ptr() for t in ts] + [None] * (3 - len(ts))))


def _problem(F, K, NH, Lz, N, H, W):
    """Quantised CPU fp32 tensors: w[l], b[l], wl, bl, feat NHWC, z [S][N][Lz], dl [N][K][H][W]."""
    g = torch.Generator().manual_seed(F + 3 * K + 5 * NH + 7 * Lz + N * H * W)
    qw = lambda *s: torch.randn(*s, generator=g).round().clamp(-2, 2) / 8
    qb = lambda *s: (torch.randn(*s, generator=g) * 1.6).round() / 16
    w = [qw(F, F + Lz if l == 0 else F) for l in range(NH)]
    b = [qb(F) for _ in range(NH)]
    wl, bl = qw(K, F), qb(K)
    feat = (torch.relu(torch.randn(N, H, W, F, generator=g)) * 4).round().clamp(0, 4) / 4
    z = (torch.randn(S, N, Lz, generator=g) * 4).round().clamp(-8, 8) / 4
    dl = torch.randn(N, K, H, W, generator=g)
    return w, b, wl, bl, feat, z, dl


def _reference(w, b, wl, bl, feat, z):
    """float64 logits [N][K][H][W] of one sample z [N][Lz], with autograd leaves for every gradient."""
    N, H, W, F = feat.shape
    leaves = dict(w=[t.double().requires_grad_(True) for t in w], b=[t.double().requires_grad_(True) for t in b],
                  wl=wl.double().requires_grad_(True), bl=bl.double().requires_grad_(True),
                  feat=feat.double().requires_grad_(True), z=z.double().requires_grad_(True))
    zt = leaves["z"][:, None, None, :].expand(N, H, W, z.shape[1])
    h = torch.cat((leaves["feat"], zt), dim=3).reshape(N * H * W, -1)
    for wi, bi in zip(leaves["w"], leaves["b"]):
        h = torch.relu(h @ wi.T + bi)
    y = (h @ leaves["wl"].T + leaves["bl"]).view(N, H, W, -1).permute(0, 3, 1, 2)
    return y, leaves


def _close(name, got, ref, worst):
    e = float((got.double().cpu() - ref).abs().max()) if ref.numel() else 0.0
    tol = 1e-4 * max(1.0, float(ref.abs().max()) if ref.numel() else 0.0)
    worst[name] = e / tol
    assert not torch.isnan(got).any(), name
    assert e <= tol, (name, e, tol)


@pytest.mark.parametrize("F,K,NH,Lz,N,H,W", CASES)
def test_fcomb_fwd_bwd_at_abi_bounds(dev, F, K, NH, Lz, N, H, W):
    L = _L()
    w, b, wl, bl, feat, z, dl = _problem(F, K, NH, Lz, N, H, W)
    zb = torch.einsum("ol,snl->sno", w[0][:, F:].double(), z.double()) + b[0].double()
    assert torch.equal(zb.float().double(), zb)                      # exact on the dyadic grid
    wd, bd = [t.to(dev) for t in w], [t.to(dev) for t in b]
    wld, bld, fd, dld, zbd = wl.to(dev), bl.to(dev), feat.to(dev), dl.to(dev), zb.float().to(dev)
    zd = z.to(dev) if Lz else torch.zeros(S, 1, device=dev)           # Lz = 0: passed, never read
    s = L.stream()

    y = torch.full((S, N, K, H, W), NAN, device=dev)
    L.call("pmu_fcomb_fwd", fd.data_ptr(), zbd.data_ptr(), _ptrs(wd), _ptrs(bd), wld.data_ptr(), bld.data_ptr(),
            F, Lz, K, NH, S, N, H, W, y.data_ptr(), s)
    torch.cuda.synchronize()
    worst = {}
    refs = [_reference(w, b, wl, bl, feat, z[i]) for i in range(S)]
    for i in range(S):
        _close(f"y[{i}]", y[i], refs[i][0].detach(), worst)
    if Lz:       # the samples differ: one sample's zb applied to all of them cannot pass
        assert float((refs[0][0] - refs[1][0]).abs().max()) > 0.1

    sb = 1      # backward of the middle sample
    yr, leaves = refs[sb]
    (yr * dl.double()).sum().backward()
    wsb = L.lib().pmu_fcomb_bwd_ws(N, H, W)
    assert wsb > 0 and wsb % 4 == 0
    for with_dz in (True, False):
        ws = torch.full((wsb // 4 + TAIL,), NAN, device=dev)
        ws[wsb // 4:] = -7.0
        dfeat = torch.full((N, H, W, F), NAN, device=dev)
        dz = torch.full((N, max(Lz, 1)), NAN if Lz else -3.0, device=dev)
        dw = [torch.full(t.shape, NAN, device=dev) for t in w]
        db = [torch.full(t.shape, NAN, device=dev) for t in b]
        dwl, dbl = torch.full((K, F), NAN, device=dev), torch.full((K,), NAN, device=dev)
        zs = zd[sb].contiguous()
        L.call("pmu_fcomb_bwd", fd.data_ptr(), zs.data_ptr(), zbd[sb].data_ptr(), dld.data_ptr(), _ptrs(wd), _ptrs(bd),
                wld.data_ptr(), bld.data_ptr(), F, Lz, K, NH, N, H, W, dfeat.data_ptr(),
                dz.data_ptr() if with_dz else None, _ptrs(dw), _ptrs(db), dwl.data_ptr(), dbl.data_ptr(), ws.data_ptr(),
                wsb, s)
        torch.cuda.synchronize()
        assert bool((ws[wsb // 4:] == -7.0).all()), "the workspace tail was written"
        tag = "" if with_dz else " (dz NULL)"
        _close("dfeat" + tag, dfeat, leaves["feat"].grad, worst)
        for l in range(NH):
            _close(f"dw[{l}]" + tag, dw[l], leaves["w"][l].grad, worst)
            _close(f"db[{l}]" + tag, db[l], leaves["b"][l].grad, worst)
        _close("dwl" + tag, dwl, leaves["wl"].grad, worst)
        _close("dbl" + tag, dbl, leaves["bl"].grad, worst)
        if Lz and with_dz:
            _close("dz", dz, leaves["z"].grad, worst)
        elif Lz:
            assert torch.isnan(dz).all()                             # NULL: not written through a stale pointer
        else:
            assert bool((dz == -3.0).all())                          # Lz = 0: there is no dz to write
    k = max(worst, key=worst.get)
    print(f"fcomb {(F, K, NH, Lz, N, H, W)}: worst err / tol {worst[k]:.4f} at {k}")


def test_fcomb_entries_refuse_shapes_outside_the_abi(dev):
    L = _L()
    F, K, NH, Lz, N, H, W = CASES[3]
    big = torch.zeros(1 << 16, device=dev)                           # stands in for every operand
    p3 = _ptrs([big, big, big])
    out = torch.full((1 << 16,), NAN, device=dev)
    o3 = _ptrs([out, out, out])
    wsb = L.lib().pmu_fcomb_bwd_ws(N, H, W)
    ws = torch.full((wsb // 4,), NAN, device=dev)
    lib, s, bad, p = L.lib(), L.stream(), L.PMU_ERR_ARG, big.data_ptr()

    def fwd(F, K, NH):
        return lib.pmu_fcomb_fwd(p, p, p3, p3, p, p, F, Lz, K, NH, 1, N, H, W, out.data_ptr(), s)

    def bwd(F, K, NH, ws_bytes):
        o = out.data_ptr()
        return lib.pmu_fcomb_bwd(p, p, p, p, p3, p3, p, p, F, Lz, K, NH, N, H, W, o, o, o3, o3, o, o, ws.data_ptr(),
                                 ws_bytes, s)

    for args in ((16, 33, 1), (65, 5, 1), (16, 5, 0), (16, 5, 4)):   # K = 33, F = 65, NH = 0, NH = 4
        assert fwd(*args) == bad, args
        assert bwd(*args, wsb) == bad, args
    assert bwd(16, 5, 1, wsb - 1) == bad                             # workspace one byte short
    torch.cuda.synchronize()
    assert torch.isnan(out).all() and torch.isnan(ws).all()          # nothing was launched
