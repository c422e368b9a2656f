"""pmu_surface_edt and pmu_surface_collect (csrc/surface.hip) against the numpy restatement
tests/surface_ref.py, bit for bit, and pmu_hip.surface.surface_distances / predict_volume(surface=True) on
top of them.  Volumes are seeded u8 blobs (a few random ellipsoids per class, K = 3); the shapes are the
smallest at which the kernels take another path: degenerate axes, a row one past a 64-voxel ballot word, line
counts off the tile sizes, the longest admissible line, and one labelled voxel in a far corner (distances no
short pruning window reaches).  Every case also runs for a class that is absent."""
import functools
import os

import numpy as np
import pytest
import torch

import surface_ref as R

pytestmark = pytest.mark.gpu

K = 3
ABSENT = 7
UNIT, ANISO = (1.0, 1.0, 1.0), (0.7, 1.25, 3.0)
# name -> (shape, spacing)
CASES = {
    "one": ((1, 1, 1), UNIT),
    "flat": ((5, 1, 7), ANISO),
    "unit": ((17, 20, 24), UNIT),
    "aniso": ((33, 18, 65), ANISO),
    "corner": ((40, 3, 130), ANISO),
    "long": ((1024, 2, 3), ANISO),
}
NAN = float("nan")


@functools.lru_cache(maxsize=None)
def _volumes(name):
    """(prediction, truth) u8 volumes of a case (read-only)."""
    shape, _ = CASES[name]
    if name == "corner":
        a, b = np.zeros(shape, dtype=np.uint8), np.zeros(shape, dtype=np.uint8)
        a[39, 2, 129] = 1
        b[0, 0, 0] = 1
        b[20, 1, 64] = 2
    elif name == "one":
        a, b = np.full(shape, 1, dtype=np.uint8), np.full(shape, 1, dtype=np.uint8)
    else:
        seed = sorted(CASES).index(name)
        a, b = R.blobs(shape, K, 10 + seed), R.blobs(shape, K, 20 + seed)
    for v in (a, b):
        v.setflags(write=False)
    return a, b


@functools.lru_cache(maxsize=None)
def _ref(name, which, cls):
    """(d2 float32, surface count) of the restatement, computed once per (case, volume, class)."""
    lab = _volumes(name)[which]
    s = R.surface(lab, cls)
    d2 = R.d2_brute(s, CASES[name][1])
    d2.setflags(write=False)
    return d2, int(s.sum())


@functools.lru_cache(maxsize=None)
def _ref_metrics(name, tol):
    a, b = _volumes(name)
    return R.surface_distances(a, b, K + 1, CASES[name][1], tol)      # class 3 is absent from both


def _bits(t):
    return t.cpu().numpy()


def _edt_raw(L, lab_d, shape, cls, sp, dev):
    d2 = torch.full(shape, NAN, dtype=torch.float32, device=dev)
    n = torch.full((1,), -1, dtype=torch.int64, device=dev)
    L.call("pmu_surface_edt", lab_d.data_ptr(), *shape, cls, *sp, d2.data_ptr(), n.data_ptr(), L.stream())
    torch.cuda.synchronize()
    return _bits(d2), int(n.item())


@pytest.mark.parametrize("cls", [1, 2, ABSENT])
@pytest.mark.parametrize("name", list(CASES))
def test_edt_bit_equal_to_brute_force(dev, name, cls):
    from pmu_hip import _lib as L
    shape, sp = CASES[name]
    lab = _volumes(name)[0]
    want, n_want = _ref(name, 0, cls)
    lab_d = torch.tensor(lab, device=dev)
    got, n = _edt_raw(L, lab_d, shape, cls, sp, dev)
    got2, n2 = _edt_raw(L, lab_d, shape, cls, sp, dev)
    assert not np.isnan(got).any()                                    # the NaN prefill is fully overwritten
    assert n == n_want and n2 == n_want
    assert np.array_equal(got, want)
    assert np.array_equal(got.view(np.uint32), got2.view(np.uint32))  # two calls, identical bits
    if cls == ABSENT:
        assert n == 0 and np.isposinf(got).all()
    elif name == "corner" and cls == 1:
        f = np.float32
        assert got[0, 0, 0] == (f(f(3.0) * f(129)) ** 2 + f(f(1.25) * f(2)) ** 2) + f(f(0.7) * f(39)) ** 2


@pytest.mark.parametrize("cls", [1, 2, ABSENT])
@pytest.mark.parametrize("name", list(CASES))
def test_collect_multiset_count_and_cap(dev, name, cls):
    from pmu_hip import _lib as L
    shape, _ = CASES[name]
    lab = _volumes(name)[0]
    other = _ref(name, 1, cls if cls != ABSENT else 1)[0]             # the truth's transform (absent: any field)
    n_want = _ref(name, 0, cls)[1]
    want = R.gather_sorted(lab, cls, other)
    assert len(want) == n_want
    lab_d, other_d = torch.tensor(lab, device=dev), torch.tensor(other, device=dev)

    def run(cap):
        out = torch.full((n_want + 8,), NAN, dtype=torch.float32, device=dev)
        n = torch.full((1,), -1, dtype=torch.int64, device=dev)
        L.call("pmu_surface_collect", lab_d.data_ptr(), *shape, cls, other_d.data_ptr(), out.data_ptr(), cap,
               n.data_ptr(), L.stream())
        torch.cuda.synchronize()
        return _bits(out), int(n.item())

    out, n = run(n_want)
    assert n == n_want and np.isnan(out[n_want:]).all()
    assert np.array_equal(np.sort(out[:n_want]).view(np.uint32), want.view(np.uint32))
    out, n = run(n_want + 8)                                          # room to spare: the same values
    assert n == n_want and np.isnan(out[n_want:]).all()
    assert np.array_equal(np.sort(out[:n_want]).view(np.uint32), want.view(np.uint32))
    cap = n_want // 2
    out, n = run(cap)                                                 # too small: the full count, nothing past cap
    assert n == n_want and np.isnan(out[cap:]).all() and not np.isnan(out[:cap]).any()
    assert np.isin(out[:cap], want).all()
    if cls == ABSENT:
        assert n_want == 0


def _close(got, want):
    for k in want:
        g = got[k].cpu().numpy()
        assert g.dtype == np.float64 and g.shape == want[k].shape, k
        # the same fp32 d2 and fp64 square roots; only the float64 sums may run in another order
        np.testing.assert_allclose(g, want[k], rtol=1e-12, atol=0, equal_nan=True, err_msg=k)


@pytest.mark.parametrize("name", list(CASES))
def test_surface_distances_match_restatement(dev, name):
    from pmu_hip.surface import edt, surface_distances
    _, sp = CASES[name]
    a, b = _volumes(name)
    tol = 2.0
    want = _ref_metrics(name, tol)
    ad, bd = torch.tensor(a, device=dev), torch.tensor(b, device=dev)
    got = surface_distances(ad, bd, K + 1, spacing=sp, tolerance=tol)
    assert set(got) == {"hd", "hd95", "assd", "nsd", "n_pred", "n_truth"}
    _close(got, want)
    for k in ("hd", "hd95", "assd", "nsd"):
        assert np.isnan(got[k][K - 1].item()), k                     # class 3: absent from both volumes
    assert got["n_pred"][K - 1].item() == 0 and got["n_truth"][K - 1].item() == 0
    again = surface_distances(ad.long(), bd.float(), K + 1, spacing=sp, tolerance=tol)   # any label dtype; same bits
    swapped = surface_distances(bd, ad, K + 1, spacing=sp, tolerance=tol)
    for k in ("hd", "hd95", "assd", "nsd"):
        assert np.array_equal(_bits(got[k]), _bits(again[k]), equal_nan=True), k
        assert np.array_equal(_bits(got[k]), _bits(swapped[k]), equal_nan=True), k
    assert torch.equal(got["n_pred"], swapped["n_truth"]) and torch.equal(got["n_truth"], swapped["n_pred"])
    d2, n = edt(ad, 1, sp)
    assert n == _ref(name, 0, 1)[1] and np.array_equal(_bits(d2), _ref(name, 0, 1)[0])


def test_single_class_and_hand_boxes(dev):
    from pmu_hip.surface import surface_distances
    a, b = np.zeros((20, 14, 14), dtype=np.uint8), np.zeros((20, 14, 14), dtype=np.uint8)
    a[4:10, 4:10, 4:10] = 1
    b[7:13, 4:10, 4:10] = 1                                           # the same box, 3 voxels along axis 0
    ad, bd = torch.tensor(a, device=dev), torch.tensor(b, device=dev)
    got = surface_distances(ad, bd, 2, spacing=(2.0, 1.0, 1.0), tolerance=6.0)
    assert tuple(got["hd"].shape) == (1,)
    assert got["hd"].item() == 6.0 and got["nsd"].item() == 1.0
    assert got["n_pred"].item() == 6 ** 3 - 4 ** 3 and got["n_truth"].item() == 6 ** 3 - 4 ** 3
    _close(got, R.surface_distances(a, b, 2, (2.0, 1.0, 1.0), 6.0))
    same = surface_distances(ad, ad, 2)
    assert (same["hd"].item(), same["hd95"].item(), same["assd"].item(), same["nsd"].item()) == (0.0, 0.0, 0.0, 1.0)
    # K = 1: the single class 0 (here the background, whose surface includes the volume border)
    one = surface_distances(ad, bd, 1, spacing=(2.0, 1.0, 1.0), tolerance=1.0)
    assert tuple(one["hd"].shape) == (1,)
    _close(one, R.surface_distances(a, b, 1, (2.0, 1.0, 1.0), 1.0))


def test_bad_arguments_launch_nothing(dev):
    from pmu_hip import _lib as L
    from pmu_hip.surface import edt, surface_distances
    lab = torch.ones(1 << 12, dtype=torch.uint8, device=dev)
    out = torch.full((1 << 12,), NAN, dtype=torch.float32, device=dev)
    cnt = torch.full((1,), NAN, dtype=torch.float64, device=dev)
    lib, s, E = L.lib(), L.stream(), L.PMU_ERR_ARG
    p, o, c = lab.data_ptr(), out.data_ptr(), cnt.data_ptr()
    f = __import__("ctypes").c_float
    for D in ((0, 4, 4), (4, 0, 4), (4, 4, 0), (1025, 2, 2), (2, 1025, 2), (2, 2, 1025), (2048, 1024, 1024)):
        assert lib.pmu_surface_edt(p, *D, 1, f(1), f(1), f(1), o, c, s) == E, D
        assert lib.pmu_surface_collect(p, *D, 1, o, o, 16, c, s) == E, D
    for sp in ((0.0, 1.0, 1.0), (1.0, NAN, 1.0), (1.0, 1.0, -2.0), (float("inf"), 1.0, 1.0)):
        assert lib.pmu_surface_edt(p, 16, 16, 16, 1, f(sp[0]), f(sp[1]), f(sp[2]), o, c, s) == E, sp
    assert lib.pmu_surface_edt(p, 16, 16, 16, 256, f(1), f(1), f(1), o, c, s) == E
    assert lib.pmu_surface_edt(None, 16, 16, 16, 1, f(1), f(1), f(1), o, c, s) == E
    assert lib.pmu_surface_edt(p, 16, 16, 16, 1, f(1), f(1), f(1), None, c, s) == E
    assert lib.pmu_surface_edt(p, 16, 16, 16, 1, f(1), f(1), f(1), o, None, s) == E
    assert lib.pmu_surface_collect(None, 16, 16, 16, 1, o, o, 16, c, s) == E
    assert lib.pmu_surface_collect(p, 16, 16, 16, 1, None, o, 16, c, s) == E
    assert lib.pmu_surface_collect(p, 16, 16, 16, 1, o, None, 16, c, s) == E
    assert lib.pmu_surface_collect(p, 16, 16, 16, 1, o, o, -1, c, s) == E
    assert lib.pmu_surface_collect(p, 16, 16, 16, 1, o, o, 16, None, s) == E
    torch.cuda.synchronize()
    assert torch.isnan(out).all() and torch.isnan(cnt).all()          # nothing was launched or cleared
    vol = lab.view(16, 16, 16)
    with pytest.raises(ValueError):
        edt(vol, 1, spacing=(1.0, 0.0, 1.0))
    with pytest.raises(ValueError):
        edt(vol, 300)
    with pytest.raises(ValueError):
        edt(lab, 1)                                                   # not a volume
    with pytest.raises(ValueError):
        surface_distances(vol, lab.view(16, 256, 1), 3)


# ------------------------------------------------------------------ predict_volume(surface=True)
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
    elif isinstance(a, (list, tuple)):
        assert len(a) == len(b), key
        for x, y in zip(a, b):
            _same(x, y, key)
    else:
        assert a == b, key


@pytest.mark.parametrize("oblique", [False, True], ids=["standard", "oblique"])
def test_predict_volume_surface_switch(dev, oblique):
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
    assert ds.oblique == oblique
    net = UNet(1, C, filters)
    net.load_state_dict(calibrated_eval_state(filters, 1, C, 2, 24, 24)[0])
    net = net.to(dev).eval()
    sp, tol = (0.7, 1.25, 3.0), 1.5
    off = predict_volume(net, ds, 0, batch_size=8)
    on = predict_volume(net, ds, 0, batch_size=8, surface=True, voxel_size=sp, surface_tolerance=tol)
    assert "surface" not in off and set(on) == set(off) | {"surface"}
    for k in off:
        _same(off[k], on[k], k)
    want = surface_distances(on["label"], on["truth"], C, spacing=sp, tolerance=tol)
    for k in want:
        assert np.array_equal(_bits(on["surface"][k]), _bits(want[k]), equal_nan=True), k
    assert tuple(on["surface"]["hd"].shape) == (C - 1,)
    lab, truth = on["label"].cpu().numpy(), on["truth"].cpu().numpy()
    assert lab.shape == truth.shape == tuple(ds.scans[0].pshape)       # the padded grid of the Dice counts
    _close(on["surface"], R.surface_distances(lab, truth, C, sp, tol))
    assert on["surface"]["n_truth"].min().item() > 0
