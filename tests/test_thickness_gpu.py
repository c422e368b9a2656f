"""pmu_interior_edt (csrc/surface.hip) and pmu_local_thickness (csrc/thickness.hip) against the numpy restatement
tests/thickness_ref.py, bit for bit, and pmu_hip.thickness.local_thickness / predict_volume(thickness=True) on
top of them.  Volumes are the seeded u8 blobs of surface_ref (K = 3); the shapes are the smallest at which a path
can go wrong: a single voxel and a volume that is all one class (the border term alone), a degenerate axis, a row
one past a 64-voxel ballot word, integer ties in d2 < D2 at unit voxels, the longest admissible line, and a box
with a cube of another class nested in its middle (the nested class counts as outside).  The box volume is
(25,23,25) so that every extent is off the covering kernel's tile edge 8 by one (25 = 3 * 8 + 1, 23 = 3 * 8 - 1).
With the cube in its middle the box's largest ball has radius sqrt(27), below the tile edge, so a further case
fills that volume with one class: its largest ball (radius 12) spans several tiles along every axis.  Every case
also runs for a class that is absent."""
import functools
import os

import numpy as np
import pytest
import torch

import surface_ref as S
import thickness_ref as R

pytestmark = pytest.mark.gpu

K = 3
ABSENT = 7
UNIT, ANISO = (1.0, 1.0, 1.0), (0.7, 1.25, 3.0)
# name -> (shape, spacing)
CASES = {
    "one": ((1, 1, 1), ANISO),
    "flat": ((5, 1, 7), ANISO),
    "unit": ((17, 20, 24), UNIT),
    "aniso": ((33, 18, 65), ANISO),
    "full": ((6, 7, 8), UNIT),
    "box": ((25, 23, 25), UNIT),
    "long": ((1024, 2, 3), ANISO),
    "solid": ((25, 23, 25), UNIT),
}
NAN = float("nan")


@functools.lru_cache(maxsize=None)
def _volume(name):
    shape, _ = CASES[name]
    if name in ("one", "full", "solid"):
        lab = np.full(shape, 1, dtype=np.uint8)
    elif name == "box":
        lab = np.zeros(shape, dtype=np.uint8)
        lab[1:22, 1:22, 2:23] = 1
        lab[9:14, 9:14, 10:15] = 2                                    # a 5^3 cube in the middle: outside for class 1
    else:
        lab = S.blobs(shape, K, 30 + sorted(CASES).index(name))
    lab.setflags(write=False)
    return lab


@functools.lru_cache(maxsize=None)
def _ref_d2(name, cls):
    d2 = R.interior_d2_fast(_volume(name), cls, CASES[name][1])
    d2.setflags(write=False)
    return d2


@functools.lru_cache(maxsize=None)
def _ref_r2(name, cls):
    r2 = R.cover_r2(_ref_d2(name, cls), CASES[name][1])
    r2.setflags(write=False)
    return r2


@functools.lru_cache(maxsize=None)
def _ref_local(name):
    """thickness_ref.local_thickness of the case for K + 1 classes (class 3 is absent), from the cached fields."""
    sp = CASES[name][1]
    vox = float(sp[0]) * float(sp[1]) * float(sp[2])
    tmap = np.zeros(CASES[name][0], dtype=np.float32)
    rows = {k: [] for k in R.STATS}
    for c in (1, 2, 3):
        r2 = _ref_r2(name, c)
        on = r2 > 0
        tmap[on] = R.tau_of(r2[on]).astype(np.float32)
        for k, v in R.stats(R.tau_of(r2[on]), vox).items():
            rows[k].append(v)
    out = {k: np.array(v, dtype=np.float64) for k, v in rows.items()}
    out["map"] = tmap
    return out


def _bits(t):
    return t.cpu().numpy()


def _same_bits(a, b):
    return a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))


def _edt_raw(L, lab_d, shape, cls, sp, dev):
    d2 = torch.full(shape, NAN, dtype=torch.float32, device=dev)
    n = torch.full((1,), -1, dtype=torch.int64, device=dev)
    L.call("pmu_interior_edt", lab_d.data_ptr(), *shape, cls, *sp, d2.data_ptr(), n.data_ptr(), L.stream())
    torch.cuda.synchronize()
    return _bits(d2), int(n.item())


def _cover_raw(L, d2_d, shape, sp, dev):
    r2 = torch.full(shape, NAN, dtype=torch.float32, device=dev)
    nbytes = int(L.lib().pmu_local_thickness_ws(*shape))
    assert nbytes >= 8 and nbytes % 4 == 0
    ws = torch.full((nbytes // 4 + 2,), NAN, dtype=torch.float32, device=dev)      # two guard words behind it
    L.call("pmu_local_thickness", d2_d.data_ptr(), *shape, *sp, r2.data_ptr(), ws.data_ptr(), nbytes, L.stream())
    torch.cuda.synchronize()
    assert torch.isnan(ws[-2:]).all()
    return _bits(r2)


@pytest.mark.parametrize("cls", [1, 2, ABSENT])
@pytest.mark.parametrize("name", list(CASES))
def test_interior_edt_bit_equal_to_brute_force(dev, name, cls):
    from pmu_hip import _lib as L
    shape, sp = CASES[name]
    lab = _volume(name)
    want = _ref_d2(name, cls)
    lab_d = torch.tensor(lab, device=dev)
    got, n = _edt_raw(L, lab_d, shape, cls, sp, dev)
    got2, n2 = _edt_raw(L, lab_d, shape, cls, sp, dev)
    assert not np.isnan(got).any()                                    # the NaN prefill is fully overwritten
    assert n == int((lab == cls).sum()) and n2 == n
    assert np.array_equal(got, want)
    assert _same_bits(got, got2)                                      # two calls, identical bits
    assert np.isfinite(got).all() and np.array_equal(got > 0, lab == cls)
    if cls == ABSENT:
        assert n == 0 and not got.any()
    if name == "one" and cls == 1:
        assert got[0, 0, 0] == np.float32(0.7) * np.float32(0.7)       # the border term only: min s_i^2


@pytest.mark.parametrize("cls", [1, 2, ABSENT])
@pytest.mark.parametrize("name", list(CASES))
def test_cover_bit_equal_to_restatement(dev, name, cls):
    from pmu_hip import _lib as L
    shape, sp = CASES[name]
    lab = _volume(name)
    d2, want = _ref_d2(name, cls), _ref_r2(name, cls)
    d2_d = torch.tensor(d2, device=dev)
    got = _cover_raw(L, d2_d, shape, sp, dev)                          # fed the restatement's field: this kernel alone
    got2 = _cover_raw(L, d2_d, shape, sp, dev)
    assert not np.isnan(got).any()
    assert np.array_equal(got, want)
    assert _same_bits(got, got2)
    assert np.array_equal(got > 0, lab == cls) and np.all(got >= d2)
    own, _ = _edt_raw(L, torch.tensor(lab, device=dev), shape, cls, sp, dev)
    assert np.array_equal(_cover_raw(L, torch.tensor(own, device=dev), shape, sp, dev), want)
    if name == "solid" and cls == 1:
        assert want.max() == 144.0 and (want == 144.0).sum() > 512     # one ball over more than a tile of voxels


def _close(got, want):
    for k in R.STATS:
        g = got[k].cpu().numpy()
        assert g.dtype == np.float64 and g.shape == want[k].shape, k
        # the same fp32 r2 and fp64 square roots; only the float64 sums may run in another order
        np.testing.assert_allclose(g, want[k], rtol=1e-12, atol=0, equal_nan=True, err_msg=k)


@pytest.mark.parametrize("name", list(CASES))
def test_local_thickness_matches_restatement(dev, name):
    from pmu_hip.thickness import cover, interior_edt, local_thickness
    _, sp = CASES[name]
    lab = _volume(name)
    want = _ref_local(name)
    lab_d = torch.tensor(lab, device=dev)
    got = local_thickness(lab_d, K + 1, spacing=sp)
    assert set(got) == {"map", *R.STATS}
    assert got["map"].dtype == torch.float32 and _same_bits(_bits(got["map"]), want["map"])
    _close(got, want)
    for k in ("mean", "std", "median", "max"):
        assert np.isnan(got[k][K - 1].item()), k                     # class 3 is absent
    assert got["n"][K - 1].item() == 0 and got["volume"][K - 1].item() == 0
    for other in (lab_d.long(), lab_d.float(), lab_d.to(torch.int16)):  # any label dtype; the same bits
        again = local_thickness(other, K + 1, spacing=sp)
        for k in got:
            assert np.array_equal(_bits(got[k]), _bits(again[k]), equal_nan=True), k
    d2, n = interior_edt(lab_d, 1, sp)
    assert n == int((lab == 1).sum()) and np.array_equal(_bits(d2), _ref_d2(name, 1))
    assert np.array_equal(_bits(cover(d2, sp)), _ref_r2(name, 1))


def test_single_class_and_hand_slab(dev):
    from pmu_hip.thickness import interior_edt, local_thickness
    lab = np.zeros((9, 40, 40), dtype=np.uint8)
    lab[2:7] = 1                                                      # a slab 5 voxels of edge 2 across axis 0
    sp = (2.0, 1.0, 1.0)
    lab_d = torch.tensor(lab, device=dev)
    d2, n = interior_edt(lab_d, 1, sp)
    assert n == 5 * 40 * 40 and d2[4, 20, 20].item() == 36.0
    got = local_thickness(lab_d, 2, spacing=sp)
    assert tuple(got["n"].shape) == (1,)
    assert got["map"][4, 20, 20].item() == 12.0 and got["map"][2, 20, 20].item() == 12.0
    assert got["map"][1, 20, 20].item() == 0.0
    assert got["volume"].item() == 5 * 40 * 40 * 2 and got["n"].item() == 5 * 40 * 40 and got["max"].item() == 12.0
    want = R.local_thickness(lab, 2, sp)
    assert _same_bits(_bits(got["map"]), want["map"])
    _close(got, want)
    # K = 1: the single class 0 (here the background around the slab)
    one = local_thickness(lab_d, 1, spacing=sp)
    assert tuple(one["n"].shape) == (1,) and one["n"].item() == 4 * 40 * 40
    want = R.local_thickness(lab, 1, sp)
    assert _same_bits(_bits(one["map"]), want["map"])
    _close(one, want)


def test_bad_arguments_launch_nothing(dev):
    from pmu_hip import _lib as L
    from pmu_hip.thickness import cover, interior_edt, local_thickness
    lab = torch.ones(1 << 12, dtype=torch.uint8, device=dev)
    fld = torch.ones(1 << 12, dtype=torch.float32, device=dev)
    out = torch.full((1 << 12,), NAN, dtype=torch.float32, device=dev)
    ws = torch.full((1 << 12,), NAN, dtype=torch.float32, device=dev)
    cnt = torch.full((1,), NAN, dtype=torch.float64, device=dev)
    lib, s, E = L.lib(), L.stream(), L.PMU_ERR_ARG
    p, d, o, w, c = lab.data_ptr(), fld.data_ptr(), out.data_ptr(), ws.data_ptr(), cnt.data_ptr()
    f = __import__("ctypes").c_float
    one = (f(1), f(1), f(1))
    for D in ((0, 4, 4), (4, 0, 4), (4, 4, 0), (1025, 2, 2), (2, 1025, 2), (2, 2, 1025), (2048, 1024, 1024)):
        assert lib.pmu_interior_edt(p, *D, 1, *one, o, c, s) == E, D
        assert lib.pmu_local_thickness(d, *D, *one, o, w, 1 << 14, s) == E, D
    for sp in ((0.0, 1.0, 1.0), (1.0, NAN, 1.0), (1.0, 1.0, -2.0), (float("inf"), 1.0, 1.0)):
        sp = tuple(f(v) for v in sp)
        assert lib.pmu_interior_edt(p, 16, 16, 16, 1, *sp, o, c, s) == E
        assert lib.pmu_local_thickness(d, 16, 16, 16, *sp, o, w, 1 << 14, s) == E
    assert lib.pmu_interior_edt(p, 16, 16, 16, 256, *one, o, c, s) == E
    assert lib.pmu_interior_edt(None, 16, 16, 16, 1, *one, o, c, s) == E
    assert lib.pmu_interior_edt(p, 16, 16, 16, 1, *one, None, c, s) == E
    assert lib.pmu_interior_edt(p, 16, 16, 16, 1, *one, o, None, s) == E
    assert lib.pmu_local_thickness(None, 16, 16, 16, *one, o, w, 1 << 14, s) == E
    assert lib.pmu_local_thickness(d, 16, 16, 16, *one, None, w, 1 << 14, s) == E
    assert lib.pmu_local_thickness(d, 16, 16, 16, *one, o, None, 1 << 14, s) == E
    need = lib.pmu_local_thickness_ws(16, 16, 16)
    assert need == 4 * (1 + 8)
    assert lib.pmu_local_thickness(d, 16, 16, 16, *one, o, w, need - 1, s) == E
    torch.cuda.synchronize()
    assert torch.isnan(out).all() and torch.isnan(cnt).all() and torch.isnan(ws).all()   # nothing launched or cleared
    vol = lab.view(16, 16, 16)
    with pytest.raises(ValueError):
        interior_edt(vol, 1, spacing=(1.0, 0.0, 1.0))
    with pytest.raises(ValueError):
        interior_edt(vol, 256)
    with pytest.raises(ValueError):
        interior_edt(lab, 1)                                          # not a volume
    with pytest.raises(ValueError):
        local_thickness(vol, 3, spacing=(1.0, NAN, 1.0))
    with pytest.raises(ValueError):
        local_thickness(vol, 0)
    with pytest.raises(ValueError):
        local_thickness(lab, 3)
    with pytest.raises(ValueError):
        cover(fld.view(16, 16, 16), spacing=(1.0, 1.0, float("inf")))
    with pytest.raises(ValueError):
        cover(fld)


# ------------------------------------------------------------------ predict_volume(thickness=True)
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
        assert torch.equal(a, b), key
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


def _equal_nan(a, b, key):
    assert np.array_equal(_bits(a), _bits(b), equal_nan=True), key


@pytest.mark.parametrize("oblique", [False, True], ids=["standard", "oblique"])
def test_predict_volume_thickness_switch(dev, oblique):
    from helpers import calibrated_eval_state
    from model import UNet
    from pmu_hip.thickness import local_thickness
    from predict import predict_volume
    from utils.mri_dataset import MRI_Dataset, draw_views
    filters, C = [4, 8], 3
    scans = _phantom((24, 20, 16), 5)
    kw = {"views": draw_views(3, 1, 30)} if oblique else {}
    ds = MRI_Dataset("/imgs", "/labs", 3, filter=False, files=sorted(scans),
                     loader=lambda p: scans[os.path.basename(p)][0 if "imgs" in p else 1], device=dev, **kw)
    assert ds.oblique == oblique
    net = UNet(1, C, filters)
    net.load_state_dict(calibrated_eval_state(filters, 1, C, 2, 24, 24)[0])
    net = net.to(dev).eval()
    sp = (0.7, 1.25, 3.0)
    off = predict_volume(net, ds, 0, batch_size=8)
    on = predict_volume(net, ds, 0, batch_size=8, thickness=True, voxel_size=sp)
    assert "thickness" not in off and set(on) == set(off) | {"thickness"}
    for k in off:
        _same(off[k], on[k], k)
    th = on["thickness"]
    assert set(th) == {"map", "pred", "truth"} and set(th["pred"]) == set(R.STATS) == set(th["truth"])
    want_p = local_thickness(on["label"], C, spacing=sp)
    want_t = local_thickness(on["truth"], C, spacing=sp)
    _equal_nan(th["map"], want_p["map"], "map")
    for k in R.STATS:
        _equal_nan(th["pred"][k], want_p[k], k)
        _equal_nan(th["truth"][k], want_t[k], k)
        assert tuple(th["pred"][k].shape) == (C - 1,)
    lab, truth = on["label"].cpu().numpy(), on["truth"].cpu().numpy()
    assert lab.shape == truth.shape == tuple(ds.scans[0].pshape) == tuple(th["map"].shape)
    ref_p, ref_t = R.local_thickness(lab, C, sp), R.local_thickness(truth, C, sp)
    assert _same_bits(_bits(th["map"]), ref_p["map"])
    _close(th["pred"], ref_p)
    _close(th["truth"], ref_t)
    assert th["truth"]["n"].min().item() > 0
    if not oblique:
        pp = predict_volume(net, ds, 0, batch_size=8, thickness=True, voxel_size=sp, postprocess={})
        want = local_thickness(pp["label_pp"], C, spacing=sp)
        _equal_nan(pp["thickness"]["map"], want["map"], "map")
        for k in R.STATS:
            _equal_nan(pp["thickness"]["pred"][k], want[k], k)
            _equal_nan(pp["thickness"]["truth"][k], want_t[k], k)
        assert set(pp) == set(on) | {"label_pp", "dice_pp"}
