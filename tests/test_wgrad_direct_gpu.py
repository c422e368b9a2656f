"""pmu_conv3x3_wgrad (csrc/wgrad3x3.hip, the direct-sum fp32 weight gradient every conv with Cin % 64 or
Cout % 64 != 0 takes, and the baseline of the Winograd / bf16 weight-gradient tests) against
torch.nn.grad.conv2d_weight in float64 over helpers.ref_frame of both operands.

Cases A-G reach the generic staging (frame_value4 per item), H-M the fast single-source staging, N-O the
raw staging; W <= 8 selects the 8 x 8 pixel tile, wider maps the 16 x 4 one.  Bound: max|d| / max|ref| <=
2e-5 (the sibling weight-gradient tests' bound) over the whole tensor and over each of the nine taps
against that tap's own maximum.  The stored gradient of the dz frame (da of a BN-backward source, dz
itself of a raw one) is multiplied by 4 on the outermost ring of pixels, so a wrong border tap moves the
result by far more than the bound.  dw and the workspace start as NaN.  Every operand is also checked
against ref_frame through pmu_frame_to_f32: bit-exact for RAW / BN+ReLU / max-pool sources of the
quantised inputs, within 2 ulp for avg-pool and BN-backward sources (the ulp of a BN-backward value taken
at its larger term: scale*g and kx*(z - mean) + kc are rounded once each and may cancel).

Largest errors observed on an MI355X (whole tensor / worst of the nine taps), bound 2e-5:
  A generic 16x4  9.9e-08 / 1.6e-07      F generic 16x4  1.4e-07 / 1.8e-07      K fast 16x4  1.4e-07 / 1.8e-07
  B generic 8x8   1.8e-07 / 2.5e-07      G generic 16x4  1.8e-07 / 2.3e-07      L fast 16x4  1.5e-07 / 1.7e-07
  C generic 16x4  1.9e-07 / 2.3e-07      H fast 16x4     9.8e-08 / 1.1e-07      M fast 16x4  1.2e-07 / 1.2e-07
  D generic 16x4  9.8e-08 / 1.5e-07      I fast 8x8      2.2e-07 / 2.9e-07      N raw 16x4   2.3e-07 / 2.9e-07
  E generic 16x4  2.3e-07 / 3.6e-07      J fast 16x4     1.3e-07 / 1.5e-07      O raw 8x8    2.5e-07 / 3.4e-07
Every operand frame matched ref_frame within its bound; the repeated call was bit-identical in all cases.
"""
import pytest
import torch

from helpers import (POOL_AVG2CEIL, POOL_MAX2, POOL_NONE, SRC_BNBWD, SRC_BNRELU, SRC_RAW, quant_bn, quant_z,
                     ref_frame, ulp32)

pytestmark = pytest.mark.gpu

TOL = 2e-5   # as tests/test_wino_gpu.py and tests/test_convT_gpu.py: max|d| / max|ref|


def _bnrelu(N, H, W, C, g, pool=POOL_NONE, off=(0, 0)):
    return dict(x=quant_z(N, H, W, C, g), mode=SRC_BNRELU, coef=quant_bn(C, g), pool=pool, off=off)


def _raw(N, H, W, C, g, off=(0, 0)):
    return dict(x=torch.randn(N, H, W, C, generator=g), mode=SRC_RAW, off=off)


def _act_sources(kind, N, H, W, Cin, g):
    """The activation frame's sources for a case (dicts of CPU tensors, the fields of engine.Src)."""
    if kind == "raw":
        return [_raw(N, H, W, Cin, g)]
    if kind == "bnrelu":
        return [_bnrelu(N, H, W, Cin, g)]
    if kind[0] == "max":           # POOL_MAX2 of a BN+ReLU source of kind[1] = (Hs, Ws)
        return [_bnrelu(N, kind[1][0], kind[1][1], Cin, g, pool=POOL_MAX2)]
    if kind[0] == "avg":           # POOL_AVG2CEIL of a BN+ReLU source of kind[1]
        return [_bnrelu(N, kind[1][0], kind[1][1], Cin, g, pool=POOL_AVG2CEIL)]
    if kind[0] == "cat_up":        # BN+ReLU skip of kind[1] channels + RAW up-sampled (H-1) x (W-2) at (0, 1)
        return [_bnrelu(N, H, W, kind[1], g), _raw(N, H - 1, W - 2, Cin - kind[1], g, off=(0, 1))]
    assert kind[0] == "cat"        # two BN+ReLU sources, kind[1] + rest channels
    return [_bnrelu(N, H, W, kind[1], g), _bnrelu(N, H, W, Cin - kind[1], g)]


# id: (N, H, W, Cin, Cout, activation frame, dz frame raw?)
CASES = {
    # generic staging
    "A": (1, 7, 9, 6, 10, "raw", False),
    "B": (2, 9, 7, 12, 20, "bnrelu", False),
    "C": (1, 20, 20, 96, 160, "bnrelu", False),
    "D": (2, 17, 33, 24, 32, ("cat_up", 16), False),
    "E": (2, 12, 10, 16, 32, ("max", (25, 20)), False),
    "F": (2, 10, 12, 32, 48, ("avg", (19, 23)), False),
    "G": (1, 12, 12, 96, 64, ("cat", 40), False),
    # fast staging
    "H": (2, 40, 36, 64, 64, "bnrelu", False),
    "I": (1, 8, 8, 64, 64, "bnrelu", False),
    "J": (2, 24, 20, 64, 128, ("max", (49, 40)), False),
    "K": (2, 12, 10, 64, 64, ("avg", (23, 19)), False),
    "L": (2, 33, 17, 128, 64, ("cat_up", 64), False),
    "M": (4, 20, 40, 192, 256, "bnrelu", False),
    # raw staging
    "N": (2, 17, 33, 64, 128, "raw", True),
    "O": (1, 8, 8, 64, 64, "raw", True),
}


def _staging(N, H, W, Cin, Cout, act, dz_raw):
    """The staging mode pmu_conv3x3_wgrad's host dispatch picks (csrc/wgrad3x3.hip), restated."""
    vec = all(s["x"].shape[3] % 4 == 0 for s in act) and Cout % 4 == 0
    blocks = vec and Cout % 64 == 0 and Cin % 64 == 0
    if blocks and dz_raw and len(act) == 1 and act[0]["mode"] == SRC_RAW and act[0].get("pool", 0) == POOL_NONE:
        return "raw"
    fast = blocks and not dz_raw and act[0]["x"].shape[3] % 64 == 0
    fast = fast and all(s.get("pool", 0) == POOL_NONE or s["mode"] == SRC_BNRELU for s in act)
    return "fast" if fast else "generic"


EXPECT_STAGING = {**{k: "generic" for k in "ABCDEFG"}, **{k: "fast" for k in "HIJKLM"}, "N": "raw", "O": "raw"}


def _to_src(d, dev):
    from pmu_hip.engine import Src
    t = lambda v: None if v is None else v.to(dev)
    return Src(t(d["x"]), d["mode"], t(d.get("coef")), t(d.get("z")), d.get("pool", POOL_NONE), d.get("off", (0, 0)))


def _check_frame(srcs_cpu, srcs_dev, N, H, W):
    """pmu_frame_to_f32 of the frame against ref_frame (see the module docstring for the bounds)."""
    from pmu_hip.engine import Src, frame_to_f32
    got = frame_to_f32(srcs_dev, N, H, W).double().cpu()
    ref = ref_frame([Src(**d) for d in srcs_cpu], N, H, W)
    c0 = 0
    for d in srcs_cpu:
        C = d["x"].shape[3]
        gs, rs = got[..., c0:c0 + C], ref[..., c0:c0 + C]
        c0 += C
        if d["mode"] == SRC_BNBWD:
            sc, sh, mu, kx, kc = d["coef"].double().view(5, C)
            z = d["z"].double()
            first = sc * torch.where(z * sc + sh > 0, d["x"].double(), torch.zeros_like(z))
            scale = torch.maximum(torch.maximum(first.abs(), (kx * (z - mu) + kc).abs()), rs.abs())
            assert bool(((gs - rs).abs() <= 2 * ulp32(scale)).all()), float(((gs - rs).abs() / ulp32(scale)).max())
        elif d.get("pool", 0) == POOL_AVG2CEIL:
            assert bool(((gs - rs).abs() <= 2 * ulp32(rs)).all()), float(((gs - rs).abs() / ulp32(rs)).max())
        else:
            assert torch.equal(gs, rs)
    return ref


def _build(case, dev):
    N, H, W, Cin, Cout, kind, dz_raw = CASES[case]
    g = torch.Generator().manual_seed(1000 + ord(case))
    act = _act_sources(kind, N, H, W, Cin, g)
    grad = torch.randn(N, H, W, Cout, generator=g)
    ring = torch.full((H, W), 4.0)
    ring[1:H - 1, 1:W - 1] = 1.0
    grad = grad * ring[None, :, :, None]
    if dz_raw:
        dz = [dict(x=grad, mode=SRC_RAW)]
    else:
        dz = [dict(x=grad, mode=SRC_BNBWD, coef=quant_bn(Cout, g, bwd=True), z=quant_z(N, H, W, Cout, g))]
    assert _staging(N, H, W, Cin, Cout, act, dz_raw) == EXPECT_STAGING[case]
    return act, dz, [_to_src(d, dev) for d in act], [_to_src(d, dev) for d in dz]


def _run(act_dev, dz_dev, N, H, W, Cin, Cout, dev):
    from pmu_hip import _lib as L
    from pmu_hip.engine import frame_of
    wsb = L.lib().pmu_conv3x3_wgrad_ws(N, H, W, Cin, Cout)
    assert wsb > 0 and wsb % 4 == 0
    ws = torch.full((wsb // 4,), float("nan"), device=dev)
    dw = torch.full((Cout, Cin, 3, 3), float("nan"), device=dev)
    L.call("pmu_conv3x3_wgrad", frame_of(dz_dev, N, H, W), frame_of(act_dev, N, H, W), Cout, dw.data_ptr(),
           ws.data_ptr(), wsb, L.stream())
    torch.cuda.synchronize()
    return dw


@pytest.mark.parametrize("case", sorted(CASES))
def test_conv3x3_wgrad_direct_vs_float64(dev, case):
    N, H, W, Cin, Cout, _, _ = CASES[case]
    act, dz, act_dev, dz_dev = _build(case, dev)
    x = _check_frame(act, act_dev, N, H, W)
    d = _check_frame(dz, dz_dev, N, H, W)
    ref = torch.nn.grad.conv2d_weight(x.permute(0, 3, 1, 2), (Cout, Cin, 3, 3), d.permute(0, 3, 1, 2), padding=1)
    dw = _run(act_dev, dz_dev, N, H, W, Cin, Cout, dev)
    assert not torch.isnan(dw).any(), int(torch.isnan(dw).sum())
    diff = (dw.double().cpu() - ref).abs()
    e_all = float(diff.max() / ref.abs().max())
    e_tap = (diff.amax(dim=(0, 1)) / ref.abs().amax(dim=(0, 1))).flatten()
    print(f"wgrad3x3 case {case} [{EXPECT_STAGING[case]}, tile {'16x4' if W > 8 else '8x8'}]: "
          f"whole {e_all:.3e} worst tap {float(e_tap.max()):.3e} (tap {int(e_tap.argmax())})")
    assert e_all <= TOL, e_all
    assert float(e_tap.max()) <= TOL, e_tap.tolist()
    # deterministic (fixed-shape slabs, no float atomics): the same call gives the same bits
    assert torch.equal(_run(act_dev, dz_dev, N, H, W, Cin, Cout, dev), dw)


def test_conv3x3_wgrad_refusals(dev):
    """Checked on the host before any launch: a workspace one byte short, a two-source dz frame, and
    dz.C != Cout each return PMU_ERR_ARG."""
    from pmu_hip import _lib as L
    from pmu_hip.engine import Src, frame_of
    N, H, W, Cin, Cout = 1, 7, 9, 8, 12
    x = Src(torch.zeros(N, H, W, Cin, device=dev))
    d = Src(torch.zeros(N, H, W, Cout, device=dev))
    half = Src(torch.zeros(N, H, W, Cout // 2, device=dev))
    wsb = L.lib().pmu_conv3x3_wgrad_ws(N, H, W, Cin, Cout)
    ws = torch.zeros(wsb // 4, device=dev)
    dw = torch.zeros(Cout, Cin, 3, 3, device=dev)
    fn = L.lib().pmu_conv3x3_wgrad
    fx = frame_of([x], N, H, W)
    assert fn(frame_of([d], N, H, W), fx, Cout, dw.data_ptr(), ws.data_ptr(), wsb - 1, L.stream()) == L.PMU_ERR_ARG
    assert fn(frame_of([half, half], N, H, W), fx, Cout, dw.data_ptr(), ws.data_ptr(), wsb, L.stream()) == L.PMU_ERR_ARG
    assert fn(frame_of([half], N, H, W), fx, Cout, dw.data_ptr(), ws.data_ptr(), wsb, L.stream()) == L.PMU_ERR_ARG
    assert fn(frame_of([d], N, H, W), fx, Cout, dw.data_ptr(), ws.data_ptr(), wsb, L.stream()) == L.PMU_OK
    torch.cuda.synchronize()
    assert not dw.any()
