"""Surface distances without a GPU: the numpy restatement tests/surface_ref.py against scipy.ndimage,
pmu_hip.surface.metrics_from_distances on hand-computed vectors, the ctypes table, the host-side argument
checks of pmu_surface_edt / pmu_surface_collect (PMU_ERR_ARG before any launch) and eval.py's flags."""
import ctypes
import inspect
import math
import os

import numpy as np
import pytest
import torch

import surface_ref as R

ANISO = (0.7, 1.25, 3.0)


# ------------------------------------------------------------------ the restatement against scipy
@pytest.mark.parametrize("shape,seed", [((17, 20, 24), 1), ((33, 18, 65), 2), ((5, 1, 7), 3)])
def test_restatement_matches_scipy(shape, seed):
    ndi = pytest.importorskip("scipy.ndimage")
    lab = R.blobs(shape, 3, seed)
    for cls in (1, 2):
        mask = lab == cls
        surf = R.surface(lab, cls)
        assert np.array_equal(surf, mask ^ ndi.binary_erosion(mask))
        if not surf.any():
            assert np.isinf(R.d2_brute(surf)).all()
            continue
        d2 = R.d2_brute(surf)
        want = ndi.distance_transform_edt(~surf)
        assert d2.dtype == np.float32 and np.array_equal(d2, np.round(want ** 2).astype(np.float32))
        d2a = R.d2_brute(surf, ANISO)
        wa = ndi.distance_transform_edt(~surf, sampling=ANISO)
        # fp32 against fp64: three roundings of about 6e-8 each on d2, halved by the square root
        assert np.all(np.abs(np.sqrt(d2a.astype(np.float64)) - wa) <= 1e-5 * wa)


def test_restatement_surface_at_the_volume_border_and_when_absent():
    lab = np.ones((3, 4, 5), dtype=np.uint8)          # a structure filling the volume: its surface is the border
    s = R.surface(lab, 1)
    assert s.sum() == 60 - 1 * 2 * 3 and not s[1, 1:3, 1:4].any()
    assert not R.surface(lab, 2).any() and np.isinf(R.d2_brute(R.surface(lab, 2), ANISO)).all()
    one = np.zeros((40, 3, 130), dtype=np.uint8)
    one[39, 2, 129] = 1
    d2 = R.d2_brute(R.surface(one, 1), ANISO)
    f = np.float32
    assert d2[0, 0, 0] == (f(f(3.0) * f(129)) ** 2 + f(f(1.25) * f(2)) ** 2) + f(f(0.7) * f(39)) ** 2


# ------------------------------------------------------------------ metrics_from_distances by hand
def _m(a, b, tol, pct=95.0):
    from pmu_hip.surface import metrics_from_distances
    out = metrics_from_distances(torch.tensor(a, dtype=torch.float64), torch.tensor(b, dtype=torch.float64), tol, pct)
    assert all(v.dtype == torch.float64 and v.dim() == 0 for v in out.values())
    return {k: float(v) for k, v in out.items()}


def test_metrics_hand_vectors():
    # pooled [1, 2, 2, 3, 4]: the 95th percentile sits at index 3.8, between 3 and 4
    m = _m([1.0, 2.0, 3.0], [2.0, 4.0], tol=2.0)
    assert m["hd"] == 4.0 and m["assd"] == 0.5 * (2.0 + 3.0)
    assert m["hd95"] == pytest.approx(3.8, rel=1e-14)
    assert m["nsd"] == 3 / 5                          # 1, 2 and 2: a distance equal to the tolerance counts
    assert _m([1.0, 2.0, 3.0], [2.0, 4.0], tol=1.9999)["nsd"] == 1 / 5
    assert _m([1.0, 2.0, 3.0], [2.0, 4.0], 2.0, pct=50.0)["hd95"] == 2.0      # exactly on an element
    assert _m([1.0, 2.0, 3.0], [2.0, 4.0], 2.0, pct=100.0)["hd95"] == 4.0
    assert _m([1.0, 2.0, 3.0], [2.0, 4.0], 2.0, pct=0.0)["hd95"] == 1.0
    # one voxel on each surface: pooled [3, 5], index 0.95
    m = _m([3.0], [5.0], tol=3.0)
    assert m["hd"] == 5.0 and m["assd"] == 4.0 and m["nsd"] == 0.5 and m["hd95"] == pytest.approx(4.9, rel=1e-14)
    m = _m([0.0], [0.0], tol=0.0)
    assert (m["hd"], m["hd95"], m["assd"], m["nsd"]) == (0.0, 0.0, 0.0, 1.0)
    g = np.random.default_rng(0)
    a, b = np.sort(g.random(37) * 9), np.sort(g.random(12) * 5)
    m, want = _m(a.tolist(), b.tolist(), 1.5, 95.0), R.metrics(a, b, 1.5, 95.0)
    for k in want:
        assert m[k] == pytest.approx(want[k], rel=1e-12), k


def test_metrics_empty_surface_conventions():
    for a, b in (([], [1.0, 2.0]), ([3.0], [])):
        m = _m(a, b, tol=1.0)
        assert math.isnan(m["hd"]) and math.isnan(m["hd95"]) and math.isnan(m["assd"]) and m["nsd"] == 0.0
        w = R.metrics(a, b, 1.0)
        assert math.isnan(w["hd"]) and w["nsd"] == 0.0
    m = _m([], [], tol=1.0)
    assert all(math.isnan(v) for v in m.values())
    assert all(math.isnan(v) for v in R.metrics([], [], 1.0).values())


def test_surface_module_refuses_cpu_tensors():
    from pmu_hip.surface import edt, surface_distances
    z = torch.zeros(2, 3, 4, dtype=torch.uint8)
    with pytest.raises(RuntimeError):
        edt(z, 1)
    with pytest.raises(RuntimeError):
        surface_distances(z, z, 3)


# ------------------------------------------------------------------ the ABI
def test_surface_entries_are_declared_and_not_mfma():
    from pmu_hip import _lib as L
    for n in ("pmu_surface_edt", "pmu_surface_collect"):
        assert n in L.SIGNATURES and n not in L.MFMA_ENTRY_POINTS and n not in L.MFMA_UNCOUNTED
        assert L.SIGNATURES[n][0] is ctypes.c_int
    assert L.SIGNATURES["pmu_surface_edt"][1][5:8] == [ctypes.c_float] * 3
    assert L.SIGNATURES["pmu_surface_collect"][1][7] is ctypes.c_longlong
    assert L.MFMA_UNCOUNTED == ("pmu_fcomb_stats",)


def test_surface_entries_reject_bad_arguments_without_gpu():
    """Every bound is checked on the host before any launch or runtime call: safe without a GPU.  The pointers
    are host buffers the entries never read (each call below is refused)."""
    from pmu_hip._lib import LIB_PATH, PMU_ERR_ARG, load_library
    if not os.path.exists(LIB_PATH):
        pytest.skip("library not built")
    cdll = load_library()
    buf = (ctypes.c_char * 64)()
    p = ctypes.addressof(buf)
    f = ctypes.c_float

    def edt(lab=p, D=(4, 4, 4), cls=1, s=(1.0, 1.0, 1.0), d2=p, n=p):
        return cdll.pmu_surface_edt(lab, D[0], D[1], D[2], cls, f(s[0]), f(s[1]), f(s[2]), d2, n, None)

    def collect(lab=p, D=(4, 4, 4), cls=1, other=p, out=p, cap=4, n=p):
        return cdll.pmu_surface_collect(lab, D[0], D[1], D[2], cls, other, out, cap, n, None)

    dims = [(0, 4, 4), (4, 0, 4), (4, 4, 0), (1025, 4, 4), (4, 1025, 4), (4, 4, 1025), (-1, 4, 4),
            (2048, 1024, 1024)]                        # the last: 2^31 voxels
    for D in dims:
        assert edt(D=D) == PMU_ERR_ARG, D
        assert collect(D=D) == PMU_ERR_ARG, D
    for cls in (-1, 256):
        assert edt(cls=cls) == PMU_ERR_ARG and collect(cls=cls) == PMU_ERR_ARG, cls
    for bad in (0.0, -1.0, float("nan"), float("inf")):
        for a in range(3):
            s = [1.0, 1.0, 1.0]
            s[a] = bad
            assert edt(s=s) == PMU_ERR_ARG, s
    for kw in ({"lab": None}, {"d2": None}, {"n": None}):
        assert edt(**kw) == PMU_ERR_ARG, kw
    for kw in ({"lab": None}, {"other": None}, {"out": None}, {"n": None}, {"cap": -1}):
        assert collect(**kw) == PMU_ERR_ARG, kw


# ------------------------------------------------------------------ the switches
def test_eval_parser_surface_flags():
    import eval as E
    a = E.get_args([])
    assert a.surface is False and a.voxel_size == [1.0, 1.0, 1.0] and a.surface_tolerance == 1.0
    assert a.views == 0 and a.uncertainty is False and a.batch == 32        # the old defaults
    a = E.get_args(["--surface", "--voxel-size", "0.7", "1.25", "3", "--surface-tolerance", "2.5", "-m", "probunet"])
    assert a.surface is True and a.voxel_size == [0.7, 1.25, 3.0] and a.surface_tolerance == 2.5
    with pytest.raises(SystemExit):
        E.get_args(["--voxel-size", "1", "2"])


def test_eval_surface_summary_skips_absent_classes():
    import eval as E
    nan = float("nan")
    per = {k: [np.array([1.0, nan]), np.array([3.0, nan])] for k in E.SURFACE_METRICS}
    per["hd"][1] = np.array([nan, nan])
    lines = E.surface_summary(per)
    assert len(lines) == 4 and lines[0].startswith("average: hd mean [ 1. nan] std [ 0. nan]")
    assert "hd95 mean [ 2. nan] std [ 1. nan]" in lines[1]


def test_predict_volume_surface_defaults_off():
    from predict import predict_volume
    p = inspect.signature(predict_volume).parameters
    assert p["surface"].default is False and tuple(p["voxel_size"].default) == (1.0, 1.0, 1.0)
    assert p["surface_tolerance"].default == 1.0
