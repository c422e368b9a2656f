"""The pmu_cc_* entries (csrc/components.hip) against the numpy restatement tests/components_ref.py, bit for bit,
and pmu_hip.components / predict_volume(postprocess=..., lesions=...) on top of them.

The volumes are those of components_ref.CASES: the smallest shapes at which the kernels take another path — one
voxel, a degenerate axis, sizes off the tile and off the 256-thread and 2048-voxel chunks, the longest
admissible axis, the 3-D checkerboard (189 / 1 / 1 components at 6 / 18 / 26), the diagonal (11 / 11 / 1), a
voxel-wide serpentine whose root has to travel the whole path across every tile boundary, an empty volume, and
'tile1' (5, 9, 65): one past the 4 x 8 x 64 tile of the labelling kernel in each axis.  Noisy blobs are
surface_ref.blobs with 15 % of the background set to a random class, so the count differs at each connectivity
and a kernel with the wrong neighbourhood cannot pass."""
import functools
import os

import numpy as np
import pytest
import torch

import components_ref as R

pytestmark = pytest.mark.gpu

CONNS = (6, 18, 26)
K = 3
POISON = -7


@functools.lru_cache(maxsize=None)
def _vol(name, seed=None):
    v = R.volume(name, seed)
    v.setflags(write=False)
    return v


@functools.lru_cache(maxsize=None)
def _ref(name, conn, seed=None):
    """(root, components dict) of the restatement, computed once per (case, connectivity)."""
    lab = _vol(name, seed)
    root = R.roots(lab, conn)
    ids, n = R.compact(root)
    size, cls = R.sizes(ids, lab, n)
    for a in (root, ids, size, cls):
        a.setflags(write=False)
    return root, {"ids": ids, "n": n, "size": size, "cls": cls}


def _np(t):
    return t.cpu().numpy()


def _ws(L, shape, dev):
    nbytes = int(L.lib().pmu_cc_ws(*shape))
    assert nbytes > 0
    return torch.full((nbytes,), 0xA5, dtype=torch.uint8, device=dev), nbytes


def _label(L, lab_d, shape, conn, dev):
    root = torch.full(shape, POISON, dtype=torch.int32, device=dev)
    n = torch.full((1,), POISON, dtype=torch.int64, device=dev)
    ws, nbytes = _ws(L, shape, dev)
    L.call("pmu_cc_label", lab_d.data_ptr(), *shape, conn, root.data_ptr(), n.data_ptr(), ws.data_ptr(), nbytes,
           L.stream())
    return root, n


def _compact(L, root, dev, in_place):
    shape = tuple(root.shape)
    ids = root.clone() if in_place else torch.full(shape, POISON, dtype=torch.int32, device=dev)
    src = ids if in_place else root
    n = torch.full((1,), POISON, dtype=torch.int64, device=dev)
    ws, nbytes = _ws(L, shape, dev)
    L.call("pmu_cc_compact", src.data_ptr(), root.numel(), ids.data_ptr(), n.data_ptr(), ws.data_ptr(), nbytes,
           L.stream())
    return ids, n


def _sizes(L, ids, lab_d, n, dev):
    size = torch.full((n,), POISON, dtype=torch.int64, device=dev)
    cls = torch.full((n,), 0xEE, dtype=torch.uint8, device=dev)
    L.call("pmu_cc_sizes", ids.data_ptr(), lab_d.data_ptr(), ids.numel(), n, L.ptr(size) if n else None,
           L.ptr(cls) if n else None, L.stream())
    return size, cls


@pytest.mark.parametrize("conn", CONNS)
@pytest.mark.parametrize("name", list(R.CASES))
def test_raw_entries_bit_equal_to_restatement(dev, name, conn):
    from pmu_hip import _lib as L
    shape = R.CASES[name]
    lab = _vol(name)
    want_root, want = _ref(name, conn)
    lab_d = torch.tensor(lab, device=dev)
    root, n = _label(L, lab_d, shape, conn, dev)
    root2, n2 = _label(L, lab_d, shape, conn, dev)
    ids, m = _compact(L, root, dev, in_place=False)
    ids2, m2 = _compact(L, root, dev, in_place=True)
    size, cls = _sizes(L, ids, lab_d, want["n"], dev)
    torch.cuda.synchronize()
    print(name, conn, "components", int(n.item()), "expected", want["n"])
    assert int(n.item()) == want["n"] and int(n2.item()) == want["n"]
    assert _np(root).dtype == np.int32 and np.array_equal(_np(root), want_root)   # (the poison is negative)
    assert torch.equal(root, root2)                                               # two calls, identical bits
    assert int(m.item()) == want["n"] and int(m2.item()) == want["n"]
    assert np.array_equal(_np(ids), want["ids"])
    assert torch.equal(ids, ids2)                                                 # ids aliasing root
    assert np.array_equal(_np(size), want["size"]) and np.array_equal(_np(cls), want["cls"])
    if name == "checker":
        assert want["n"] == {6: 189, 18: 1, 26: 1}[conn]
    if name == "diag":
        assert want["n"] == {6: 11, 18: 11, 26: 1}[conn]
    if name == "snake":
        assert want["n"] == 1 and want["size"].tolist() == [3904]
    if name == "empty":
        assert want["n"] == 0 and not root.any() and not ids.any()


@pytest.mark.parametrize("conn", CONNS)
@pytest.mark.parametrize("name", ["unit", "tile1"])
def test_classes_do_not_merge(dev, name, conn):
    from pmu_hip import _lib as L
    shape = R.CASES[name]
    lab = _vol(name)
    merged = (lab != 0).astype(np.uint8)
    want_root = R.roots(merged, conn)
    n_want = R.compact(want_root)[1]
    root, n = _label(L, torch.tensor(merged, device=dev), shape, conn, dev)
    root_mc, n_mc = _label(L, torch.tensor(lab, device=dev), shape, conn, dev)
    torch.cuda.synchronize()
    assert int(n.item()) == n_want and np.array_equal(_np(root), want_root)
    assert int(n_mc.item()) == _ref(name, conn)[1]["n"] and n_want < int(n_mc.item())


@pytest.mark.parametrize("conn", [6, 26])
@pytest.mark.parametrize("name", ["flat", "unit", "aniso", "tile1", "snake", "empty"])
def test_filter_and_overlap(dev, name, conn):
    from pmu_hip import _lib as L
    shape = R.CASES[name]
    noisy = name in R.NOISY
    a, ca = _vol(name), _ref(name, conn)[1]
    b, cb = (_vol(name, 77), _ref(name, conn, 77)[1]) if noisy else (a, ca)       # two different seeds
    V = a.size
    a_d, b_d = torch.tensor(a, device=dev), torch.tensor(b, device=dev)
    ia_d, ib_d = torch.tensor(ca["ids"], device=dev), torch.tensor(cb["ids"], device=dev)
    keep = (np.random.default_rng(3).random(ca["n"]) < 0.5).astype(np.uint8)
    keep_d = torch.tensor(keep, device=dev)
    want = R.apply_filter(a, ca["ids"], keep)
    out = torch.full(shape, 0xEE, dtype=torch.uint8, device=dev)
    kp = L.ptr(keep_d) if ca["n"] else None
    L.call("pmu_cc_filter", a_d.data_ptr(), ia_d.data_ptr(), V, kp, ca["n"], out.data_ptr(), L.stream())
    inplace = a_d.clone()
    L.call("pmu_cc_filter", inplace.data_ptr(), ia_d.data_ptr(), V, kp, ca["n"], inplace.data_ptr(), L.stream())
    hit_a = torch.full((ca["n"],), 0xEE, dtype=torch.uint8, device=dev)
    hit_b = torch.full((cb["n"],), 0xEE, dtype=torch.uint8, device=dev)
    L.call("pmu_cc_overlap", ia_d.data_ptr(), a_d.data_ptr(), ca["n"], ib_d.data_ptr(), b_d.data_ptr(), cb["n"], V,
           L.ptr(hit_a) if ca["n"] else None, L.ptr(hit_b) if cb["n"] else None, L.stream())
    torch.cuda.synchronize()
    assert np.array_equal(_np(out), want) and np.array_equal(_np(inplace), want)
    wa, wb = R.overlap_hits(ca["ids"], a, ca["n"], cb["ids"], b, cb["n"])
    assert np.array_equal(_np(hit_a), wa) and np.array_equal(_np(hit_b), wb)
    if name in ("unit", "aniso"):
        assert 0 < wa.sum() < len(wa) and 0 < keep.sum() < len(keep)              # both outcomes occur


def _same_metrics(got, want):
    assert set(got) == set(want)
    for k in want:
        g = _np(got[k])
        assert g.dtype == np.float64 and g.shape == want[k].shape, k
        assert np.array_equal(g, want[k], equal_nan=True), (k, g, want[k])        # one fp64 division: equal


@pytest.mark.parametrize("name", ["one", "flat", "unit", "aniso", "tile1", "checker", "snake", "empty"])
def test_components_keep_largest_lesion_metrics(dev, name):
    from pmu_hip.components import components, keep_largest, lesion_metrics
    conn = 26 if name != "snake" else 6
    noisy = name in R.NOISY
    a = _vol(name)
    b = _vol(name, 77) if noisy else a
    want = _ref(name, conn)[1]
    a_d, b_d = torch.tensor(a, device=dev), torch.tensor(b, device=dev)
    got = components(a_d, conn)
    assert set(got) == {"ids", "n", "size", "cls"} and got["n"] == want["n"]
    assert got["ids"].dtype == torch.int32 and got["size"].dtype == torch.int64 and got["cls"].dtype == torch.uint8
    for k in ("ids", "size", "cls"):
        assert np.array_equal(_np(got[k]), want[k]), k
    for dt in (torch.int64, torch.float32):                                       # any label dtype, the same bits
        again = components(a_d.to(dt), conn)
        assert again["n"] == got["n"] and all(torch.equal(again[k], got[k]) for k in ("ids", "size", "cls"))
    for keep in (1, 2, None):
        for mv in (1, 5):
            mask = R.keep_mask(want["size"], want["cls"], K, keep, mv)
            out = keep_largest(a_d, K, keep=keep, min_voxels=mv, connectivity=conn)
            assert out.dtype == torch.uint8 and np.array_equal(_np(out), R.apply_filter(a, want["ids"], mask)), (keep, mv)
            assert torch.equal(keep_largest(out, K, keep=keep, min_voxels=mv, connectivity=conn), out)   # idempotent
            assert torch.equal(keep_largest(a_d.float(), K, keep=keep, min_voxels=mv, connectivity=conn), out)
    for mv in (1, 5):
        _same_metrics(lesion_metrics(a_d, b_d, K, connectivity=conn, min_voxels=mv),
                      R.lesion_metrics(a, b, K, conn, mv))
    _same_metrics(lesion_metrics(a_d.long(), b_d.float(), K, connectivity=conn), R.lesion_metrics(a, b, K, conn))


def test_single_blobs_unchanged_and_hand_boxes(dev):
    from pmu_hip.components import keep_largest, lesion_metrics
    lab = np.zeros((20, 14, 70), dtype=np.uint8)
    lab[2:9, 3:12, 5:68] = 1                                                      # one blob per class
    lab[12:18, 2:6, 60:70] = 2
    lab_d = torch.tensor(lab, device=dev)
    assert torch.equal(keep_largest(lab_d, K), lab_d)
    assert torch.equal(keep_largest(lab_d, K, keep=None, min_voxels=200, connectivity=6), lab_d)
    island = lab.copy()
    island[19, 13, 0] = 1
    island[0, 0, 69] = 2
    assert torch.equal(keep_largest(torch.tensor(island, device=dev), K), lab_d)  # the islands go, nothing else
    one = keep_largest(torch.tensor(island, device=dev), 1)                       # K = 1: label value 1 only
    assert np.array_equal(_np(one), np.where(lab == 1, 1, 0).astype(np.uint8))
    truth = np.zeros((12, 12, 12), dtype=np.uint8)
    pred = np.zeros((12, 12, 12), dtype=np.uint8)
    truth[1:3, 1:3, 1:3] = 1
    truth[6:8, 6:8, 6:8] = 1
    truth[9:11, 1:3, 1:3] = 2
    pred[2:4, 2:4, 2:4] = 1
    pred[9:11, 1:3, 1:3] = 1
    pred[0, 11, 11] = 1
    m = lesion_metrics(torch.tensor(pred, device=dev), torch.tensor(truth, device=dev), 4)
    _same_metrics(m, R.lesion_metrics(pred, truth, 4))
    assert _np(m["tp"]).tolist() == [1, 0, 0] and _np(m["fp"]).tolist() == [2, 0, 0]
    assert _np(m["sensitivity"])[0] == 0.5 and np.isnan(_np(m["precision"])[1]) and np.isnan(_np(m["f1"])[2])


def test_bad_arguments_launch_nothing(dev):
    from pmu_hip import _lib as L
    from pmu_hip.components import components, keep_largest, lesion_metrics
    V = 1 << 12
    lab = torch.ones(V, dtype=torch.uint8, device=dev)
    root = torch.full((V,), POISON, dtype=torch.int32, device=dev)
    out8 = torch.full((V,), 0xEE, dtype=torch.uint8, device=dev)
    cnt = torch.full((1,), POISON, dtype=torch.int64, device=dev)
    per = torch.full((V,), POISON, dtype=torch.int64, device=dev)
    ws = torch.full((4096,), 0xA5, dtype=torch.uint8, device=dev)
    lib, s, E = L.lib(), L.stream(), L.PMU_ERR_ARG
    p, r, o, c, q, w = (t.data_ptr() for t in (lab, root, out8, cnt, per, ws))
    assert lib.pmu_cc_ws(16, 16, 16) >= 8 and lib.pmu_cc_ws(16, 16, 16) <= 4096
    for D in ((0, 4, 4), (4, 0, 4), (4, 4, 0), (1025, 2, 2), (2, 1025, 2), (2, 2, 1025), (2048, 1024, 1024)):
        assert lib.pmu_cc_ws(*D) == 0, D
        assert lib.pmu_cc_label(p, *D, 26, r, c, w, 4096, s) == E, D
    for conn in (0, 4, 8, 27, -6):
        assert lib.pmu_cc_label(p, 16, 16, 16, conn, r, c, w, 4096, s) == E, conn
    assert lib.pmu_cc_label(None, 16, 16, 16, 26, r, c, w, 4096, s) == E
    assert lib.pmu_cc_label(p, 16, 16, 16, 26, None, c, w, 4096, s) == E
    assert lib.pmu_cc_label(p, 16, 16, 16, 26, r, None, w, 4096, s) == E
    assert lib.pmu_cc_label(p, 16, 16, 16, 26, r, c, None, 4096, s) == E
    assert lib.pmu_cc_label(p, 16, 16, 16, 26, r, c, w, lib.pmu_cc_ws(16, 16, 16) - 1, s) == E
    assert lib.pmu_cc_compact(None, V, r, c, w, 4096, s) == E
    assert lib.pmu_cc_compact(r, V, None, c, w, 4096, s) == E
    assert lib.pmu_cc_compact(r, V, r, None, w, 4096, s) == E
    assert lib.pmu_cc_compact(r, V, r, c, None, 4096, s) == E
    assert lib.pmu_cc_compact(r, V, r, c, w, 7, s) == E
    assert lib.pmu_cc_compact(r, 0, r, c, w, 4096, s) == E
    assert lib.pmu_cc_compact(r, 1 << 31, r, c, w, 1 << 30, s) == E
    assert lib.pmu_cc_sizes(None, p, V, 4, q, o, s) == E
    assert lib.pmu_cc_sizes(r, None, V, 4, q, o, s) == E
    assert lib.pmu_cc_sizes(r, p, V, 4, None, o, s) == E
    assert lib.pmu_cc_sizes(r, p, V, 4, q, None, s) == E
    assert lib.pmu_cc_sizes(r, p, V, -1, q, o, s) == E
    assert lib.pmu_cc_sizes(r, p, 0, 0, q, o, s) == E
    assert lib.pmu_cc_filter(None, r, V, p, 4, o, s) == E
    assert lib.pmu_cc_filter(p, None, V, p, 4, o, s) == E
    assert lib.pmu_cc_filter(p, r, V, None, 4, o, s) == E
    assert lib.pmu_cc_filter(p, r, V, p, 4, None, s) == E
    assert lib.pmu_cc_filter(p, r, V, p, -1, o, s) == E
    assert lib.pmu_cc_filter(p, r, 1 << 31, p, 4, o, s) == E
    assert lib.pmu_cc_overlap(None, p, 4, r, p, 4, V, o, o, s) == E
    assert lib.pmu_cc_overlap(r, None, 4, r, p, 4, V, o, o, s) == E
    assert lib.pmu_cc_overlap(r, p, 4, None, p, 4, V, o, o, s) == E
    assert lib.pmu_cc_overlap(r, p, 4, r, None, 4, V, o, o, s) == E
    assert lib.pmu_cc_overlap(r, p, 4, r, p, 4, V, None, o, s) == E
    assert lib.pmu_cc_overlap(r, p, 4, r, p, 4, V, o, None, s) == E
    assert lib.pmu_cc_overlap(r, p, -1, r, p, 4, V, o, o, s) == E
    assert lib.pmu_cc_overlap(r, p, 4, r, p, 4, 0, o, o, s) == E
    torch.cuda.synchronize()
    assert (root == POISON).all() and (out8 == 0xEE).all() and (cnt == POISON).all() and (per == POISON).all()
    assert (ws == 0xA5).all()                                                      # nothing was launched or cleared
    vol = lab.view(16, 16, 16)
    with pytest.raises(ValueError):
        components(vol, 8)
    with pytest.raises(ValueError):
        components(lab)                                                            # not a volume
    with pytest.raises(ValueError):
        keep_largest(vol, 3, keep=0)
    with pytest.raises(ValueError):
        keep_largest(vol, 3, min_voxels=0)
    with pytest.raises(ValueError):
        keep_largest(vol, 300)
    with pytest.raises(ValueError):
        lesion_metrics(vol, lab.view(16, 256, 1), 3)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        components(vol.cpu())


# ------------------------------------------------------------------ predict_volume(postprocess=..., lesions=...)
def _phantom(shape, seed):
    g = np.random.default_rng(seed)
    img = g.random(shape) * 100.0
    ii, jj, kk = np.meshgrid(*[np.arange(d) for d in shape], indexing="ij")
    r2 = (ii - shape[0] / 2) ** 2 + (jj - shape[1] / 2) ** 2 + (kk - shape[2] / 2) ** 2
    lab = np.zeros(shape)
    lab[r2 < (min(shape) / 3) ** 2] = 1.0
    lab[r2 < (min(shape) / 6) ** 2] = 2.0
    return {"scan0.nii": (img, lab)}


def _same(a, b, key):
    if isinstance(a, torch.Tensor):
        assert a.dtype == b.dtype and np.array_equal(_np(a), _np(b), equal_nan=a.is_floating_point()), key
    elif isinstance(a, dict):
        assert set(a) == set(b), key
        for k in a:
            _same(a[k], b[k], (key, k))
    elif isinstance(a, (list, tuple)):
        assert len(a) == len(b), key
        for x, y in zip(a, b):
            _same(x, y, key)
    else:
        assert a == b, key


def _bits_equal(got, want):
    assert set(got) == set(want)
    for k in want:
        assert np.array_equal(_np(got[k]), _np(want[k]), equal_nan=True), k


@pytest.mark.parametrize("oblique", [False, True], ids=["standard", "oblique"])
def test_predict_volume_postprocess_and_lesions(dev, oblique):
    from helpers import calibrated_eval_state
    from model import UNet
    from pmu_hip.surface import surface_distances
    from predict import predict_volume
    from utils.mri_dataset import MRI_Dataset, draw_views
    filters, C = [4, 8], 3
    scans = _phantom((24, 20, 16), 5)
    kw = {"views": draw_views(3, 1, 30)} if oblique else {}
    ds = MRI_Dataset("/imgs", "/labs", 3, filter=False, files=sorted(scans),
                     loader=lambda p: scans[os.path.basename(p)][0 if "imgs" in p else 1], device=dev, **kw)
    net = UNet(1, C, filters)
    net.load_state_dict(calibrated_eval_state(filters, 1, C, 2, 24, 24)[0])
    net = net.to(dev).eval()
    sp, tol = (0.7, 1.25, 3.0), 1.5
    surf = dict(surface=True, voxel_size=sp, surface_tolerance=tol)
    off = predict_volume(net, ds, 0, batch_size=8, **surf)
    plain = predict_volume(net, ds, 0, batch_size=8, postprocess=None, lesions=False, **surf)
    assert set(plain) == set(off)                                     # without the new arguments: key for key
    for k in off:
        _same(off[k], plain[k], k)
    lab, truth = _np(off["label"]), _np(off["truth"])
    print("raw components per class:", R.lesion_metrics(lab, truth, C)["n_pred"])

    keep_all = predict_volume(net, ds, 0, batch_size=8, postprocess=dict(keep=None, min_voxels=1), **surf)
    assert set(keep_all) == set(off) | {"label_pp", "dice_pp", "surface_raw"}
    for k in off:
        if k != "surface":
            _same(off[k], keep_all[k], k)
    assert keep_all["label_pp"].dtype == torch.int32 and torch.equal(keep_all["label_pp"], off["label"])
    assert keep_all["dice_pp"].dtype == torch.float32 and tuple(keep_all["dice_pp"].shape) == (C,)
    assert torch.equal(keep_all["dice_pp"], off["dice"][-1])          # the average row: pins the class convention
    _bits_equal(keep_all["surface"], off["surface"])
    _bits_equal(keep_all["surface_raw"], off["surface"])

    on = predict_volume(net, ds, 0, batch_size=8, postprocess=dict(keep=1), lesions=True, **surf)
    assert set(on) == set(off) | {"label_pp", "dice_pp", "surface_raw", "lesions"}
    want_pp = R.keep_largest(lab.astype(np.uint8), C, 1, 1, 26)
    assert np.array_equal(_np(on["label_pp"]), want_pp.astype(np.int32))
    cnt = np.array([[((want_pp == c) & (truth == c)).sum(), (want_pp == c).sum(), (truth == c).sum()]
                    for c in range(C)], dtype=np.float32)
    smooth = np.float32(0.000001)
    dice = (np.float32(2.0) * cnt[:, 0] + smooth) / (cnt[:, 1] + cnt[:, 2] + smooth)
    assert dice.dtype == np.float32 and np.array_equal(_np(on["dice_pp"]), dice)
    _bits_equal(on["surface"], surface_distances(on["label_pp"], on["truth"], C, spacing=sp, tolerance=tol))
    _bits_equal(on["surface_raw"], surface_distances(on["label"], on["truth"], C, spacing=sp, tolerance=tol))
    _same_metrics(on["lesions"], R.lesion_metrics(want_pp, truth, C))
    assert _np(on["lesions"]["n_pred"]).max() <= 1                    # keep=1: at most one component per class

    raw = predict_volume(net, ds, 0, batch_size=8, lesions=True)      # no clean-up: the lesions of 'label'
    assert set(raw) == (set(off) - {"surface"}) | {"lesions"}
    _same_metrics(raw["lesions"], R.lesion_metrics(lab, truth, C))
    _same_metrics(predict_volume(net, ds, 0, batch_size=8, lesions={})["lesions"], R.lesion_metrics(lab, truth, C))
    six = predict_volume(net, ds, 0, batch_size=8, lesions=dict(connectivity=6, min_voxels=2))
    _same_metrics(six["lesions"], R.lesion_metrics(lab, truth, C, 6, 2))
