"""Local thickness without a GPU: the numpy restatement tests/thickness_ref.py against scipy.ndimage and against
an independent integer construction of the covering, pmu_hip.thickness.thickness_stats on CPU tensors, the
ctypes table, the host-side argument checks of pmu_interior_edt / pmu_local_thickness and eval.py's flag."""
import ctypes
import inspect
import math
import os

import numpy as np
import pytest
import torch

import surface_ref as S
import thickness_ref as R

ANISO = (0.7, 1.25, 3.0)


def _solid(shape):
    return np.ones(shape, dtype=np.uint8)


# ------------------------------------------------------------------ the interior distance against scipy
@pytest.mark.parametrize("shape,seed", [((17, 20, 24), 1), ((12, 9, 33), 2), ((9, 10, 11), 4), ((5, 1, 7), 3),
                                        ((1, 1, 1), 0), ((6, 7, 8), 0)])
def test_interior_d2_matches_scipy_on_the_padded_mask(shape, seed):
    ndi = pytest.importorskip("scipy.ndimage")
    lab = S.blobs(shape, 3, seed) if seed else _solid(shape)       # seed 0: the volume is all class 1
    # the literal d2_brute form where it is quick; the evaluation at the class's voxels only is held to its bits
    # there and to scipy everywhere
    literal = lab.size <= 1200
    for cls in (1, 2, 7):
        mask = np.pad(lab == cls, 1, constant_values=False)
        d2 = R.interior_d2_fast(lab, cls)
        assert d2.dtype == np.float32 and d2.shape == lab.shape
        want = ndi.distance_transform_edt(mask)[1:-1, 1:-1, 1:-1]
        assert np.array_equal(d2, np.round(want ** 2).astype(np.float32))
        assert np.array_equal(d2 > 0, lab == cls)
        d2a = R.interior_d2_fast(lab, cls, ANISO)
        wa = ndi.distance_transform_edt(mask, sampling=ANISO)[1:-1, 1:-1, 1:-1]
        # fp32 against fp64: three roundings of about 6e-8 each on d2, halved by the square root
        assert np.all(np.abs(np.sqrt(d2a.astype(np.float64)) - wa) <= 1e-5 * wa)
        if literal:
            assert np.array_equal(R.interior_d2(lab, cls).view(np.uint32), d2.view(np.uint32))
            assert np.array_equal(R.interior_d2(lab, cls, ANISO).view(np.uint32), d2a.view(np.uint32))


def test_interior_d2_border_term_by_hand():
    f = np.float32
    one = R.interior_d2(_solid((1, 1, 1)), 1, ANISO)
    assert one[0, 0, 0] == f(0.7) * f(0.7)                           # min s_i^2
    full = R.interior_d2(_solid((6, 7, 8)), 1)                       # no seed inside: straight out to the border
    i = np.indices((6, 7, 8))
    out = np.minimum.reduce([np.minimum(i[a] + 1, n - i[a]) for a, n in enumerate((6, 7, 8))])
    assert np.array_equal(full, (out ** 2).astype(np.float32))
    assert not R.interior_d2(_solid((3, 3, 3)), 2).any()


# ------------------------------------------------------------------ the covering against an integer construction
def _paint(d2i):
    """For every voxel q of the structure, D2(q) painted with maximum over its open ball: integers only."""
    r2 = np.zeros(d2i.shape, dtype=np.int64)
    D = d2i.shape
    for q0, q1, q2 in np.argwhere(d2i > 0):
        v = int(d2i[q0, q1, q2])
        r = math.isqrt(v - 1)                                        # the largest e with e * e < v
        a0, a1, a2 = max(q0 - r, 0), max(q1 - r, 0), max(q2 - r, 0)
        g = np.ogrid[a0:min(q0 + r + 1, D[0]), a1:min(q1 + r + 1, D[1]), a2:min(q2 + r + 1, D[2])]
        ball = (g[0] - q0) ** 2 + (g[1] - q1) ** 2 + (g[2] - q2) ** 2 < v
        win = r2[a0:a0 + ball.shape[0], a1:a1 + ball.shape[1], a2:a2 + ball.shape[2]]
        np.maximum(win, np.where(ball, v, 0), out=win)
    return np.where(d2i > 0, r2, 0)


@pytest.mark.parametrize("shape,seed", [((17, 20, 24), 1), ((12, 9, 33), 2), ((5, 1, 7), 3), ((9, 10, 11), 0)])
def test_cover_r2_equals_painted_balls_at_unit_voxels(shape, seed):
    lab = S.blobs(shape, 3, seed) if seed else _solid(shape)
    for cls in (1, 2):
        d2 = R.interior_d2_fast(lab, cls)
        r2 = R.cover_r2(d2)
        assert r2.dtype == np.float32
        want = _paint(d2.astype(np.int64))
        assert np.array_equal(r2.astype(np.int64), want) and np.array_equal(r2, want.astype(np.float32))
        assert np.array_equal(r2 > 0, lab == cls) and np.all(r2 >= d2)


def test_cover_r2_strict_inequality_and_slab_by_hand():
    # a slab 5 voxels across axis 0, voxel size (2, 1, 1): the middle plane lies 3 voxels = 6 from the outside
    lab = np.zeros((9, 40, 40), dtype=np.uint8)
    lab[2:7] = 1
    sp = (2.0, 1.0, 1.0)
    d2 = R.interior_d2_fast(lab, 1, sp)
    assert d2[4, 20, 20] == 36.0 and d2[2, 20, 20] == 4.0
    tau = R.tau_of(R.cover_r2(d2, sp))
    assert tau[4, 20, 20] == 12.0 and tau[2, 20, 20] == 12.0         # k = 5 across reads k + 1 = 6 voxels of 2
    out = R.local_thickness(lab, 2, sp)
    assert out["volume"][0] == 5 * 40 * 40 * 2 and out["n"][0] == 5 * 40 * 40 and out["max"][0] == 12.0
    # across a bar 3 voxels wide D2 is 1, 4, 1 and the middle ball reaches both sides (1 < 4)
    bar = np.ones((5, 5, 3), dtype=np.uint8)
    d2 = R.interior_d2(bar, 1)
    assert d2[2, 2].tolist() == [1.0, 4.0, 1.0] and R.cover_r2(d2)[2, 2].tolist() == [4.0, 4.0, 4.0]
    two = np.ones((5, 5, 2), dtype=np.uint8)
    assert R.cover_r2(R.interior_d2(two, 1))[2, 2].tolist() == [1.0, 1.0]
    # a single voxel with D2 = 2 (a plus-shaped neighbourhood): its ball holds the 6 face neighbours (1 < 2) and
    # not the 12 edge neighbours (2 is not < 2)
    f = np.zeros((5, 5, 5), dtype=np.float32)
    f[1:4, 1:4, 1:4] = 1.0
    f[2, 2, 2] = 2.0
    r2 = R.cover_r2(f)
    assert r2[2, 2, 1] == 2.0 and r2[2, 1, 2] == 2.0 and r2[1, 2, 2] == 2.0 and r2[2, 1, 1] == 1.0 and r2[0, 0, 0] == 0.0


# ------------------------------------------------------------------ thickness_stats
def _stats(v, vox):
    from pmu_hip.thickness import thickness_stats
    out = thickness_stats(torch.tensor(sorted(v), dtype=torch.float64), vox)
    assert list(out) == list(R.STATS)
    assert all(t.dtype == torch.float64 and t.dim() == 0 for t in out.values())
    return {k: float(t) for k, t in out.items()}


def test_thickness_stats_against_restatement():
    g = np.random.default_rng(0)
    for n in (1, 2, 5, 38):
        v = (g.random(n) * 9).tolist()
        got, want = _stats(v, 0.7 * 1.25 * 3.0), R.stats(v, 0.7 * 1.25 * 3.0)
        for k in want:
            assert got[k] == pytest.approx(want[k], rel=1e-12, abs=1e-15), (n, k)
    one = _stats([3.5], 2.0)
    assert one == {"n": 1.0, "volume": 2.0, "mean": 3.5, "std": 0.0, "median": 3.5, "max": 3.5}
    assert _stats([1.0, 2.0, 4.0, 9.0], 1.0)["median"] == 3.0
    empty = _stats([], 2.0)
    assert empty["n"] == 0.0 and empty["volume"] == 0.0
    assert all(math.isnan(empty[k]) for k in ("mean", "std", "median", "max"))
    w = R.stats([], 2.0)
    assert w["n"] == 0.0 and w["volume"] == 0.0 and math.isnan(w["mean"]) and math.isnan(w["max"])


def test_thickness_module_refuses_cpu_tensors():
    from pmu_hip.thickness import cover, interior_edt, local_thickness
    z = torch.zeros(2, 3, 4, dtype=torch.uint8)
    with pytest.raises(RuntimeError):
        interior_edt(z, 1)
    with pytest.raises(RuntimeError):
        local_thickness(z, 3)
    with pytest.raises(RuntimeError):
        cover(z.float())


# ------------------------------------------------------------------ the ABI
def test_thickness_entries_are_declared_and_not_mfma():
    from pmu_hip import _lib as L
    for n in ("pmu_interior_edt", "pmu_local_thickness", "pmu_local_thickness_ws"):
        assert n in L.SIGNATURES and n not in L.MFMA_ENTRY_POINTS and n not in L.MFMA_UNCOUNTED
    assert L.SIGNATURES["pmu_interior_edt"] == L.SIGNATURES["pmu_surface_edt"]
    assert L.SIGNATURES["pmu_local_thickness"][1][4:7] == [ctypes.c_float] * 3
    assert L.SIGNATURES["pmu_local_thickness_ws"][0] is ctypes.c_size_t


def test_thickness_entries_reject_bad_arguments_without_gpu():
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
        return cdll.pmu_interior_edt(lab, D[0], D[1], D[2], cls, f(s[0]), f(s[1]), f(s[2]), d2, n, None)

    def cover(d2=p, D=(4, 4, 4), s=(1.0, 1.0, 1.0), r2=p, ws=p, nbytes=64):
        return cdll.pmu_local_thickness(d2, D[0], D[1], D[2], f(s[0]), f(s[1]), f(s[2]), r2, ws, nbytes, None)

    dims = [(0, 4, 4), (4, 0, 4), (4, 4, 0), (1025, 4, 4), (4, 1025, 4), (4, 4, 1025), (-1, 4, 4),
            (2048, 1024, 1024)]                        # the last: 2^31 voxels
    for D in dims:
        assert edt(D=D) == PMU_ERR_ARG and cover(D=D) == PMU_ERR_ARG, D
        assert cdll.pmu_local_thickness_ws(*D) == 0, D
    for cls in (-1, 256):
        assert edt(cls=cls) == PMU_ERR_ARG, cls
    for bad in (0.0, -1.0, float("nan"), float("inf")):
        for a in range(3):
            s = [1.0, 1.0, 1.0]
            s[a] = bad
            assert edt(s=s) == PMU_ERR_ARG and cover(s=s) == PMU_ERR_ARG, s
    for kw in ({"lab": None}, {"d2": None}, {"n": None}):
        assert edt(**kw) == PMU_ERR_ARG, kw
    for kw in ({"d2": None}, {"r2": None}, {"ws": None}, {"nbytes": 7}):
        assert cover(**kw) == PMU_ERR_ARG, kw
    # one word for the field's maximum and one per 8 x 8 x 8 tile
    assert cdll.pmu_local_thickness_ws(4, 4, 4) == 8 and cdll.pmu_local_thickness_ws(9, 8, 17) == 4 * (1 + 2 * 1 * 3)


# ------------------------------------------------------------------ the switches
def test_eval_parser_thickness_flag():
    import eval as E
    a = E.get_args([])
    assert a.thickness is False and a.surface is False and a.voxel_size == [1.0, 1.0, 1.0]
    a = E.get_args(["--thickness", "--voxel-size", "0.7", "1.25", "3"])
    assert a.thickness is True and a.surface is False and a.voxel_size == [0.7, 1.25, 3.0]
    a = E.get_args(["--thickness", "--surface", "--postprocess"])
    assert a.thickness and a.surface and a.postprocess


def test_eval_thickness_summary_leaves_out_absent_classes():
    import eval as E
    nan = float("nan")
    per = {"pred": {"volume": [np.array([10.0, 0.0]), np.array([14.0, 0.0])],
                    "mean": [np.array([2.0, nan]), np.array([4.0, nan])]},
           "truth": {"volume": [np.array([11.0, 0.0]), np.array([11.0, 2.0])],
                     "mean": [np.array([3.0, nan]), np.array([3.0, 1.0])]}}
    lines = E.thickness_summary(per)
    assert len(lines) == 6
    assert lines[0] == "thickness: volume pred mean [12.  0.] std [2. 0.] scans left out [0 0]"
    assert lines[2] == "thickness: volume abs diff mean [2. 1.] std [1. 1.] scans left out [0 0]"
    assert lines[3] == "thickness: mean pred mean [ 3. nan] std [ 1. nan] scans left out [0 2]"
    assert lines[4] == "thickness: mean truth mean [3. 1.] std [0. 0.] scans left out [0 1]"
    assert lines[5] == "thickness: mean abs diff mean [ 1. nan] std [ 0. nan] scans left out [0 2]"


def test_predict_volume_thickness_defaults_off():
    from predict import predict_volume
    p = inspect.signature(predict_volume).parameters
    assert p["thickness"].default is False
