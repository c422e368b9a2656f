"""The numpy restatement tests/components_ref.py of the connected-component kernels: against scipy.ndimage.label
per class (where scipy is installed), by hand on the checkerboard, the diagonal and the serpentine, keep_largest's
tie rule and lesion_metrics on hand-placed boxes with the NaN conventions; and the header / ctypes signatures
of the pmu_cc_* entries.  No GPU."""
import ctypes
import functools
import re

import numpy as np
import pytest

import components_ref as R

CONNS = (6, 18, 26)


@functools.lru_cache(maxsize=None)
def _comp(name, conn):
    return R.components(R.volume(name), conn)


def _scipy_ids(lab, conn):
    """scipy.ndimage.label per class, merged and renumbered in the raster order of each component's first voxel."""
    ndi = pytest.importorskip("scipy.ndimage")
    st = ndi.generate_binary_structure(3, R.MAXNZ[conn])
    first = np.zeros(lab.shape, dtype=np.int64)        # 1 + the first linear index of the voxel's component
    lin = np.arange(1, lab.size + 1, dtype=np.int64).reshape(lab.shape)
    for c in np.unique(lab[lab != 0]):
        ids, n = ndi.label(lab == c, structure=st)
        if n:
            mins = ndi.minimum(lin, ids, index=np.arange(1, n + 1)).astype(np.int64)
            first = np.where(ids > 0, mins[np.maximum(ids, 1) - 1], first)
    uniq = np.unique(first[first > 0])
    return first.astype(np.int32), np.where(first > 0, np.searchsorted(uniq, first) + 1, 0).astype(np.int32), len(uniq)


@pytest.mark.parametrize("conn", CONNS)
@pytest.mark.parametrize("name", list(R.CASES))
def test_restatement_equals_scipy_label(name, conn):
    lab = R.volume(name)
    root, ids, n = _scipy_ids(lab, conn)
    got = _comp(name, conn)
    assert np.array_equal(R.roots(lab, conn), root)
    assert got["n"] == n and np.array_equal(got["ids"], ids)
    assert got["size"].sum() == (lab != 0).sum() and len(got["size"]) == n
    for i in range(min(n, 50)):
        where = ids == i + 1
        assert got["size"][i] == where.sum() and (lab[where] == got["cls"][i]).all()


def test_scipy_numbers_in_raster_order():
    """The claim pmu_cc_compact rests on: on one mask scipy's own numbering is the raster order of first voxels."""
    ndi = pytest.importorskip("scipy.ndimage")
    lab = R.volume("unit")
    for conn in CONNS:
        ids, n = ndi.label(lab == 1, structure=ndi.generate_binary_structure(3, R.MAXNZ[conn]))
        mine = R.components((lab == 1).astype(np.uint8), conn)
        assert n == mine["n"] and np.array_equal(ids, mine["ids"])


def test_hand_built_counts():
    assert [_comp("checker", c)["n"] for c in CONNS] == [189, 1, 1]
    assert [_comp("diag", c)["n"] for c in CONNS] == [11, 11, 1]
    assert _comp("one", 6)["n"] == 1 and _comp("empty", 26)["n"] == 0
    assert not _comp("empty", 26)["ids"].any() and len(_comp("empty", 26)["size"]) == 0
    d = _comp("diag", 26)
    assert d["size"].tolist() == [11] and d["cls"].tolist() == [1]
    assert np.array_equal(R.roots(R.volume("diag"), 26), R.volume("diag").astype(np.int32))   # root: voxel 0


def test_noisy_blobs_differ_by_connectivity_and_class():
    for name in R.NOISY:
        n = [_comp(name, c)["n"] for c in CONNS]
        assert n[0] >= n[1] >= n[2] >= 2, (name, n)
    n = [_comp("unit", c)["n"] for c in CONNS]
    assert n[0] > n[1] > n[2] and n[0] < 4500
    merged = (R.volume("unit") != 0).astype(np.uint8)
    for c in CONNS:
        assert R.components(merged, c)["n"] < _comp("unit", c)["n"]        # classes do not merge


def test_snake_is_one_component_until_cut():
    lab = R.volume("snake")
    assert lab.sum() == 3904
    c = R.components(lab, 6)
    assert c["n"] == 1 and c["size"].tolist() == [3904]
    r = R.roots(lab, 6)
    assert r[lab != 0].min() == 1 and r[lab != 0].max() == 1               # the far end carries the root of voxel 0
    cut = lab.copy()
    cut[4, 10, 35] = 0                                                     # one voxel out of one row
    c = R.components(cut, 6)
    assert c["n"] == 2 and c["size"].sum() == 3903
    cut = lab.copy()
    cut[4, 10, :] = 0                                                      # the whole row
    assert R.components(cut, 6)["n"] == 2


def test_keep_largest_ties_and_min_voxels():
    lab = np.zeros((4, 4, 12), dtype=np.uint8)
    lab[0, 0, 0:3] = 1          # id 1, 3 voxels
    lab[0, 0, 4:7] = 1          # id 2, 3 voxels: the tie goes to id 1
    lab[0, 0, 8:10] = 2         # id 3
    lab[2, 2, 0:5] = 2          # id 4, 5 voxels
    lab[3, 0, 11] = 1           # id 5, 1 voxel
    c = R.components(lab, 6)
    assert c["size"].tolist() == [3, 3, 2, 5, 1] and c["cls"].tolist() == [1, 1, 2, 2, 1]
    assert R.keep_mask(c["size"], c["cls"], 3, 1, 1).tolist() == [1, 0, 0, 1, 0]
    assert R.keep_mask(c["size"], c["cls"], 3, 2, 1).tolist() == [1, 1, 1, 1, 0]
    assert R.keep_mask(c["size"], c["cls"], 3, 2, 3).tolist() == [1, 1, 0, 1, 0]
    assert R.keep_mask(c["size"], c["cls"], 3, None, 2).tolist() == [1, 1, 1, 1, 0]
    assert R.keep_mask(c["size"], c["cls"], 3, 1, 4).tolist() == [0, 0, 0, 1, 0]    # the largest itself too small
    assert R.keep_mask(c["size"], c["cls"], 2, None, 1).tolist() == [1, 1, 0, 0, 1]  # K = 2: class 2 is no class
    assert R.keep_mask(c["size"], c["cls"], 1, 1, 1).tolist() == [1, 0, 0, 0, 0]     # K = 1: label value 1
    out = R.keep_largest(lab, 3, 1, 1, 6)
    assert out.dtype == np.uint8 and out.sum() == 3 * 1 + 5 * 2 and out[0, 0, 0] == 1 and out[0, 0, 4] == 0
    assert np.array_equal(R.keep_largest(out, 3, 1, 1, 6), out)                      # idempotent
    assert np.array_equal(R.keep_largest(lab, 3, None, 1, 26), lab)


def test_lesion_metrics_hand_boxes():
    truth = np.zeros((12, 12, 12), dtype=np.uint8)
    pred = np.zeros((12, 12, 12), dtype=np.uint8)
    truth[1:3, 1:3, 1:3] = 1        # found
    truth[6:8, 6:8, 6:8] = 1        # missed
    truth[9:11, 1:3, 1:3] = 2       # covered by the wrong class only: missed
    pred[2:4, 2:4, 2:4] = 1         # touches the first
    pred[9:11, 1:3, 1:3] = 1        # spurious for class 1
    pred[0, 11, 11] = 1             # spurious, one voxel
    m = R.lesion_metrics(pred, truth, 4)
    assert m["n_pred"].tolist() == [3, 0, 0] and m["n_truth"].tolist() == [2, 1, 0]
    assert m["tp"].tolist() == [1, 0, 0] and m["fn"].tolist() == [1, 1, 0] and m["fp"].tolist() == [2, 0, 0]
    assert m["sensitivity"][0] == 0.5 and m["precision"][0] == 1.0 / 3.0 and m["f1"][0] == 2.0 / 5.0
    assert m["sensitivity"][1] == 0.0 and np.isnan(m["precision"][1]) and m["f1"][1] == 0.0
    assert np.isnan(m["sensitivity"][2]) and np.isnan(m["precision"][2]) and np.isnan(m["f1"][2])
    m = R.lesion_metrics(pred, truth, 4, min_voxels=2)          # the one-voxel island is dropped first
    assert m["n_pred"].tolist() == [2, 0, 0] and m["fp"].tolist() == [1, 0, 0] and m["precision"][0] == 0.5
    one = R.lesion_metrics(pred, truth, 1)                      # K = 1: label value 1
    assert one["n_pred"].tolist() == [3] and one["tp"].tolist() == [1]


def _decl(name):
    from pmu_hip._lib import HEADER_PATH
    src = re.sub(r"/\*.*?\*/", "", open(HEADER_PATH).read(), flags=re.S)
    m = re.search(r"(\w[\w ]*?)\s*\b%s\s*\(([^)]*)\)\s*;" % name, src)
    assert m, name
    return m.group(1).strip(), [a.strip() for a in m.group(2).split(",")]


def test_header_and_table_signatures():
    from pmu_hip import _lib
    v, i, ll, sz = ctypes.c_void_p, ctypes.c_int, ctypes.c_longlong, ctypes.c_size_t
    want = {
        "pmu_cc_ws": (sz, [i, i, i]),
        "pmu_cc_label": (i, [v, i, i, i, i, v, v, v, sz, v]),
        "pmu_cc_compact": (i, [v, ll, v, v, v, sz, v]),
        "pmu_cc_sizes": (i, [v, v, ll, ll, v, v, v]),
        "pmu_cc_filter": (i, [v, v, ll, v, ll, v, v]),
        "pmu_cc_overlap": (i, [v, v, ll, v, v, ll, ll, v, v, v]),
    }
    for name, (res, args) in want.items():
        assert _lib.SIGNATURES[name] == (res, args), name
        ret, decl = _decl(name)
        assert ret == ("size_t" if res is sz else "int"), name
        assert len(decl) == len(args), name
        for d, a in zip(decl, args):
            if "*" in d:
                assert a is v, (name, d)
            elif d.startswith("long long"):
                assert a is ll, (name, d)
            elif d.startswith("size_t"):
                assert a is sz, (name, d)
            else:
                assert d.startswith("int ") and a is i, (name, d)
    assert "#define PMU_CC_MAX_DIM 1024" in open(_lib.HEADER_PATH).read()
