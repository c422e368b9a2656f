"""Oblique view planes on the GPU: pmu_oblique_slice_max, pmu_oblique_gather and pmu_fuse_oblique
(csrc/oblique.hip) through MRI_Dataset(views=...), pmu_hip.fusion.fuse_oblique and predict_volume,
against the numpy restatement of tests/oblique_ref.py — bit for bit — and, along the standard axes,
against the existing standard-axis path.  Inputs are seeded integer-valued volumes."""
import os

import numpy as np
import pytest
import torch

import oblique_ref as R

pytestmark = pytest.mark.gpu

NAMED = ([1.0, 1.0, 0.0], [1.0, 2.0, 3.0], [-0.3, 0.1, 0.9])


def _views9():
    from utils.mri_dataset import draw_views
    return [np.array(n) for n in NAMED] + draw_views(6, 0, 30)


def _scan(shape, seed, classes=3):
    """(image 0..255, mask 0..classes-1 inside a sub-box and 0 around it so some slices are empty)."""
    rs = np.random.RandomState(seed)
    img = rs.randint(0, 256, size=shape).astype(np.float64)
    lab = np.zeros(shape)
    box = tuple(slice(n // 4, n - n // 4) for n in shape)
    lab[box] = rs.randint(0, classes, size=lab[box].shape)
    return img, lab


def _dataset(scans, dev, **kw):
    from utils.mri_dataset import MRI_Dataset
    names = [f"s{i}" for i in range(len(scans))]
    store = dict(zip(names, scans))
    return MRI_Dataset("/imgs", "/labs", 3, loader=lambda p: store[os.path.basename(p)][0 if "imgs" in p else 1],
                       files=names, device=dev, **kw)


def _padded(vol):
    from utils.mri_dataset import padded_shape
    out = np.zeros(padded_shape(vol.shape))
    out[:vol.shape[0], :vol.shape[1], :vol.shape[2]] = vol
    return out


def _prob_stacks(V, P, C, seed):
    st = np.random.RandomState(seed).uniform(0.05, 1.0, size=(V, P, C, P, P)).astype(np.float32)
    return st / st.sum(2, keepdims=True)


# ------------------------------------------------------------------ 1. axis-aligned == the existing path
def test_axis_aligned_equals_standard_path(dev):
    from pmu_hip.fusion import fuse_oblique, fuse_views
    scans = [_scan((24, 24, 24), 1), _scan((24, 24, 24), 2)]
    for filt in (True, False):
        std = _dataset(scans, dev, filter=filt)
        obl = _dataset(scans, dev, filter=filt, views=np.eye(3))
        assert obl.oblique and not std.oblique and obl.sample_dim == 24 and obl.spacing == 1.0
        assert obl.index_map == std.index_map and len(obl) == len(std)
    assert 0 < len(_dataset(scans, dev, filter=True, views=np.eye(3))) < 2 * 3 * 24   # the filter dropped slices
    keys = [(s, v, i) for s in range(2) for v in range(3) for i in range(24)]
    for k0 in range(0, len(keys), 24):     # one (scan, view) per batch: the standard path needs one shape
        a, b = std.get_slices(keys[k0:k0 + 24]), obl.get_slices(keys[k0:k0 + 24])
        assert torch.equal(a["image"], b["image"]) and torch.equal(a["mask"], b["mask"])
    assert torch.equal(obl[5]["image"], std[5]["image"]) and tuple(obl[5]["mask"].shape) == (1, 24, 24)
    st = torch.from_numpy(_prob_stacks(3, 24, 3, 3)).to(dev)
    truth = torch.from_numpy(scans[0][1]).to(dev)
    want = fuse_views(st[0], st[1], st[2], truth)
    for stacks in (st, list(st)):
        got = fuse_oblique(stacks, obl.frames, truth, 24)
        assert torch.equal(got["avg"], want["avg"]) and torch.equal(got["label"], want["label"])
        assert torch.equal(got["counts"], want["counts"]) and torch.equal(got["dice"], want["dice"])
        assert int(got["cover"].min()) == 3 and int(got["cover"].max()) == 3


# ------------------------------------------------------------------ 2. gather and maxima vs the restatement
@pytest.mark.parametrize("P,h", [(20, 1.0), (20, 0.75), (29, 1.0), (29, 0.75)])
def test_oblique_gather_and_maxima_bitexact(P, h, dev):
    from pmu_hip import _lib as L
    scans = [_scan((20, 17, 13), 3), _scan((20, 17, 13), 4)]
    views = _views9()
    ds = _dataset(scans, dev, filter=False, views=views, sample_dim=P, spacing=h)
    assert ds.scans[0].pshape == (20, 17, 20) and len(ds) == 2 * 9 * P and ds.frames.shape == (9, 3, 3)
    pads = [(_padded(i), _padded(m)) for i, m in scans]
    ref = {(s, v): (R.view_items(pads[s][0], ds.frames[v], P, h, False), R.view_items(pads[s][1], ds.frames[v], P, h, True))
           for s in range(2) for v in range(9)}
    # the per-slice maxima, both modes, through the dataset and through the entry itself
    for (s, v), ((_, mx_i), (_, mx_m)) in ref.items():
        assert np.array_equal(ds.scans[s].img_max[v].cpu().numpy(), mx_i), (s, v)
        assert np.array_equal(ds.scans[s].mask_max[v].cpu().numpy(), mx_m), (s, v)
    fr = torch.from_numpy(ds.frames[1].reshape(9)).to(dev)
    out = torch.empty(P, dtype=torch.float64, device=dev)
    for nearest, vol, want in ((0, ds.scans[1].img, ref[1, 1][0][1]), (1, ds.scans[1].mask, ref[1, 1][1][1])):
        L.call("pmu_oblique_slice_max", vol.data_ptr(), 20, 17, 20, fr.data_ptr(), P, h, nearest, out.data_ptr(),
               L.stream())
        assert np.array_equal(out.cpu().numpy(), want)
    # slices none of whose samples is inside the volume: max 0, served as zeros (no division)
    inside = {v: R.sample_view(np.ones((20, 17, 20)), ds.frames[v], P, h, False).reshape(P, -1).max(1) for v in range(9)}
    empty = [(v, s) for v in range(9) for s in range(P) if inside[v][s] == 0.0]
    assert bool(empty) == (P == 29 and h == 1.0), empty
    # two batches of 7 over both scans, all nine views, first and last slices (and an empty one)
    keys = [(0, 0, 0), (1, 1, P - 1), (0, 2, P // 2), (1, 3, 3), (0, 4, P - 1), (1, 5, 0), (0, 6, 7),
            (1, 7, P // 2 + 1), (0, 8, P - 2), (1, 0, P // 3), (1, 2, 0), (0, 1, P - 1), (1, 8, 11), (0, 3, 1)]
    if empty:
        keys[6] = (1,) + empty[0]
        assert ref[1, empty[0][0]][0][1][empty[0][1]] == 0.0
    for batch in (keys[:7], keys[7:]):
        got = ds.get_slices(batch)
        assert tuple(got["image"].shape) == (7, 1, P, P) and got["image"].dtype == torch.float32
        for b, (s, v, sl) in enumerate(batch):
            assert np.array_equal(got["image"][b, 0].cpu().numpy(), ref[s, v][0][0][sl]), (s, v, sl)
            assert np.array_equal(got["mask"][b, 0].cpu().numpy(), ref[s, v][1][0][sl]), (s, v, sl)
    # the gather entry under its own name: unnormalised image samples of one batch
    ids = torch.tensor([(s * 9 + v) * P + sl for s, v, sl in keys[:7]], dtype=torch.int32, device=dev)
    raw = torch.empty(7, P, P, dtype=torch.float32, device=dev)
    L.call("pmu_oblique_gather", ds._vaddr_img.data_ptr(), ds._dims.data_ptr(), ds._frames.data_ptr(), None,
           ids.data_ptr(), 7, 18, P, h, 0, raw.data_ptr(), L.stream())
    for b, (s, v, sl) in enumerate(keys[:7]):
        want = R.sample_view(pads[s][0], ds.frames[v], P, h, False)[sl].astype(np.float32)
        assert np.array_equal(raw[b].cpu().numpy(), want), (s, v, sl)


def test_set_views_rebuilds_maxima_and_map(dev):
    scans = [_scan((20, 17, 13), 3)]
    views = _views9()
    ds = _dataset(scans, dev, filter=True, views=views[:3])
    first = (list(ds.index_map), ds.get_slices([(0, 1, 9)])["image"].clone())
    ds.set_views(views[3:7])
    assert len(ds.views) == 4 and {k[1] for k in ds.index_map} == {0, 1, 2, 3}
    want = R.view_items(_padded(scans[0][0]), ds.frames[2], 20, 1.0, False)[0][9]
    assert np.array_equal(ds.get_slices([(0, 2, 9)])["image"][0, 0].cpu().numpy(), want)
    fg = R.view_items(_padded(scans[0][1]), ds.frames[3], 20, 1.0, True)[1] > 0
    assert [k[2] for k in ds.index_map if k[1] == 3] == np.nonzero(fg)[0].tolist()
    ds.set_views(views[:3])
    assert ds.index_map == first[0] and torch.equal(ds.get_slices([(0, 1, 9)])["image"], first[1])


# ------------------------------------------------------------------ 3. fusion vs the restatement
@pytest.mark.parametrize("C", [1, 3, 8])
@pytest.mark.parametrize("V", [1, 3, 6])
@pytest.mark.parametrize("shape,P,h", [((20, 17, 20), 20, 1.0), ((20, 17, 20), 29, 1.0), ((20, 17, 20), 29, 0.75),
                                       ((40, 33, 36), 20, 1.0), ((40, 33, 36), 29, 1.0), ((40, 33, 36), 40, 1.0)])
def test_oblique_fusion_bitexact(shape, P, h, V, C, dev):
    from pmu_hip import _lib as L
    from pmu_hip.fusion import fuse_oblique
    from pmu_hip.metrics import dice_from_counts
    from utils.mri_dataset import view_frame
    frames = np.stack([view_frame(n) for n in _views9()[:V]])
    st = _prob_stacks(V, P, C, 10 * V + C)
    truth = np.random.RandomState(V + C).randint(0, C, size=shape).astype(np.float32)
    avg, label, cover, counts = R.fuse(st, frames, truth, P, h)
    # both branches are known to run: partly covered voxels where the grid is no larger than the volume,
    # none uncovered at P = 29 over the 20 x 17 x 20 volume
    if P == max(shape) or P < max(shape):
        assert (cover < V).any()
    if shape == (20, 17, 20) and P == 29 and h == 1.0:
        assert (cover > 0).all()
    if P < max(shape):
        assert (cover == 0).any()
    got = fuse_oblique(torch.from_numpy(st).to(dev), frames, torch.from_numpy(truth).to(dev), P, h)
    assert np.array_equal(got["cover"].cpu().numpy(), cover)
    assert np.array_equal(got["avg"].cpu().numpy(), avg)
    assert np.array_equal(got["label"].cpu().numpy(), label)
    assert np.array_equal(got["counts"].cpu().numpy(), counts)
    assert torch.equal(got["dice"], dice_from_counts(got["counts"])) and tuple(got["dice"].shape) == (V + 1, C)
    if V == 3 and C == 3:   # the entry under its own name, optional outputs left out
        cnt = torch.empty(V + 1, C, 3, dtype=torch.float64, device=dev)
        d = {k: torch.from_numpy(np.ascontiguousarray(x)).to(dev) for k, x in (("st", st), ("fr", frames), ("t", truth))}
        L.call("pmu_fuse_oblique", d["st"].data_ptr(), d["fr"].data_ptr(), V, C, P, h, d["t"].data_ptr(), *shape,
               None, None, None, cnt.data_ptr(), L.stream())
        assert np.array_equal(cnt.cpu().numpy(), counts)


# ------------------------------------------------------------------ 4. round trip
def test_ball_round_trip_equals_restatement(dev):
    """A ball (C = 2) in 32^3: its one-hot sliced along six views by the gather kernel's mask mode, the
    slices used as predictions and fused.  The fused label's Dice equals the restatement's, whatever
    it is (DESIGN.md records it)."""
    from pmu_hip.fusion import fuse_oblique
    from pmu_hip.metrics import dice_from_counts
    from utils.mri_dataset import draw_views, view_frame
    P = 32
    views = draw_views(6, 0, 30)
    frames = np.stack([view_frame(n) for n in views])
    truth, stacks, (avg, label, cover, counts) = R.ball_round_trip(frames, P, 1.0)
    onehot = [((truth == c).astype(np.float64),) * 2 for c in (0, 1)]   # scan c: channel c as image and mask
    ds = _dataset(onehot, dev, filter=False, views=views)
    assert np.array_equal(ds.frames, frames)
    got = torch.empty(6, P, 2, P, P, dtype=torch.float32, device=dev)
    for v in range(6):
        for c in (0, 1):
            got[v, :, c] = ds.get_slices([(c, v, s) for s in range(P)])["mask"][:, 0]
    assert np.array_equal(got.cpu().numpy(), stacks)
    res = fuse_oblique(got, ds.frames, torch.from_numpy(truth).to(dev), P)
    want = dice_from_counts(torch.from_numpy(counts))
    print(f"ball round trip: fused Dice {res['dice'][6].tolist()} (restatement {want[6].tolist()})")
    assert np.array_equal(res["label"].cpu().numpy(), label) and np.array_equal(res["counts"].cpu().numpy(), counts)
    assert torch.equal(res["dice"].cpu(), want)


# ------------------------------------------------------------------ 5. end to end
def test_predict_volume_oblique_end_to_end(dev):
    from model import UNet
    from predict import predict_volume
    from utils.mri_dataset import draw_views
    torch.manual_seed(0)
    net = UNet(1, 3, [4, 8]).to(dev).eval()
    ds = _dataset([_scan((24, 20, 16), 6)], dev, filter=False, views=draw_views(4, 1, 30))
    assert ds.scans[0].pshape == (24, 20, 24) and ds.sample_dim == 24
    res = predict_volume(net, ds, 0, batch_size=8)
    assert tuple(res["dice"].shape) == (5, 3) and tuple(res["label"].shape) == (24, 20, 24)
    assert tuple(res["avg"].shape) == (24, 3, 20, 24) and len(res["stacks"]) == 4
    with torch.no_grad():
        for v in range(4):
            for s0 in range(0, 24, 8):
                b = ds.get_slices([(0, v, s) for s in range(s0, s0 + 8)])
                assert torch.equal(res["stacks"][v][s0:s0 + 8], torch.softmax(net(b["image"]), 1)), (v, s0)
    truth = _padded(_scan((24, 20, 16), 6)[1])
    assert np.array_equal(res["truth"].cpu().numpy(), truth.astype(np.float32))
    st = np.stack([s.cpu().numpy() for s in res["stacks"]])
    avg, label, cover, counts = R.fuse(st, ds.frames, truth, 24, 1.0)
    assert np.array_equal(res["label"].cpu().numpy(), label) and np.array_equal(res["counts"].cpu().numpy(), counts)
    assert np.array_equal(res["cover"].cpu().numpy(), cover) and np.array_equal(res["avg"].cpu().numpy(), avg)


# ------------------------------------------------------------------ 6. refusals
def test_oblique_refusals(dev):
    from pmu_hip import _lib as L
    from pmu_hip.fusion import fuse_oblique
    from utils.mri_dataset import MRI_Dataset
    lib = L.lib()
    E = L.PMU_ERR_ARG
    P, C, V = 8, 2, 2
    st = torch.zeros(V, P, C, P, P, device=dev)
    fr = torch.from_numpy(np.stack([np.eye(3)] * 8).reshape(8, 9)).to(dev)
    tr = torch.zeros(6, 6, 6, device=dev)
    cnt = torch.zeros(9, 8, 3, dtype=torch.float64, device=dev)
    s, f, t, c = st.data_ptr(), fr.data_ptr(), tr.data_ptr(), cnt.data_ptr()
    fuse = lib.pmu_fuse_oblique
    assert fuse(s, f, V, C, P, 1.0, t, 6, 6, 6, None, None, None, c, None) == 0
    for bad in ((s, f, 0, C, P, 1.0, t), (s, f, 9, C, P, 1.0, t), (s, f, V, 9, P, 1.0, t), (s, f, V, 0, P, 1.0, t),
                (s, f, V, C, 1, 1.0, t), (s, f, V, C, P, 0.0, t), (s, f, V, C, P, -1.0, t),
                (s, f, V, C, P, float("nan"), t), (None, f, V, C, P, 1.0, t), (s, None, V, C, P, 1.0, t),
                (s, f, V, C, P, 1.0, None)):
        assert fuse(*bad, 6, 6, 6, None, None, None, c, None) == E, bad
    assert fuse(s, f, V, C, P, 1.0, t, 6, 6, 6, None, None, None, None, None) == E
    assert fuse(s, f, V, C, P, 1.0, t, 6, 0, 6, None, None, None, c, None) == E
    vol = torch.zeros(6 * 6 * 6, dtype=torch.float64, device=dev)
    out = torch.zeros(P, dtype=torch.float64, device=dev)
    smax = lib.pmu_oblique_slice_max
    assert smax(vol.data_ptr(), 6, 6, 6, f, P, 1.0, 0, out.data_ptr(), None) == 0
    for bad in ((None, 6, 6, 6, f, P, 1.0), (vol.data_ptr(), 6, 6, 6, None, P, 1.0), (vol.data_ptr(), 6, 6, 6, f, 1, 1.0),
                (vol.data_ptr(), 6, 6, 6, f, P, 0.0), (vol.data_ptr(), 0, 6, 6, f, P, 1.0)):
        assert smax(*bad, 0, out.data_ptr(), None) == E, bad
    assert smax(vol.data_ptr(), 6, 6, 6, f, P, 1.0, 0, None, None) == E
    va = torch.tensor([vol.data_ptr()], dtype=torch.int64, device=dev)
    dm = torch.tensor([6, 6, 6], dtype=torch.int32, device=dev)
    ids = torch.zeros(1, dtype=torch.int32, device=dev)
    img = torch.zeros(1, P, P, device=dev)
    gat = lib.pmu_oblique_gather
    good = (va.data_ptr(), dm.data_ptr(), f, None, ids.data_ptr(), 1, 1, P, 1.0, 0, img.data_ptr(), None)
    assert gat(*good) == 0
    for i, v in ((0, None), (1, None), (2, None), (4, None), (5, 0), (6, 0), (7, 1), (8, 0.0), (8, -2.0), (10, None)):
        bad = list(good)
        bad[i] = v
        assert gat(*bad) == E, (i, v)
    torch.cuda.synchronize()
    with pytest.raises(RuntimeError):
        L.call("pmu_fuse_oblique", s, f, 9, C, P, 1.0, t, 6, 6, 6, None, None, None, c, None)
    # the Python surface: no CPU fallback, no degenerate views
    scan = _scan((8, 8, 8), 0)
    with pytest.raises(RuntimeError):
        _dataset([scan], "cpu", views=np.eye(3))
    with pytest.raises(ValueError):
        _dataset([scan], dev, views=[[1, 0, 0], [0, 0, 0]])
    with pytest.raises(ValueError):
        _dataset([scan], dev, views=np.eye(3), sample_dim=1)
    with pytest.raises(ValueError):
        _dataset([scan], dev, views=np.eye(3), spacing=0.0)
    with pytest.raises(RuntimeError):
        fuse_oblique(st.cpu(), np.stack([np.eye(3)] * 2), tr.cpu(), P)
    with pytest.raises(ValueError):
        fuse_oblique(st, np.stack([np.eye(3)] * 3), tr, P)
    with pytest.raises(ValueError):
        fuse_oblique(st, np.stack([np.eye(3)] * 2), tr, P + 1)
    with pytest.raises(RuntimeError):
        _dataset([scan], dev).set_views(np.eye(3))
    assert isinstance(MRI_Dataset.initialize_views(None, False, n_views=2), list)
