"""On-the-fly slice augmentation on the GPU: pmu_warp_gather (csrc/augment.hip) through
MRI_Dataset.get_slices / get_batch(augment=...) and train_net(augment=...), against the plain gathers (identity
block, bit for bit), the numpy restatement of tests/augment_ref.py (bit for bit) and plain numpy indexing of the
un-augmented slices (lattice moves, bit for bit).  Inputs are seeded integer-valued volumes."""
import os

import numpy as np
import pytest
import torch

import augment_ref as A
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


class Fixed:
    """An augmenter that hands out given blocks (the dataset only calls ``draw``)."""

    def __init__(self, par, ctrl=None):
        self.par, self.ctrl, self.seen = np.asarray(par, dtype=np.float64), ctrl, []

    def draw(self, keys, epoch, H, W, h):
        self.seen.append((list(keys), epoch, H, W, h))
        return self.par.copy(), self.ctrl


SCANS = [_scan((20, 17, 13), 3), _scan((20, 17, 13), 4)]
PADS = [(_padded(i), _padded(m)) for i, m in SCANS]


@pytest.fixture(scope="module")
def std(dev):
    return _dataset(SCANS, dev, filter=False)


def _zero_strength():
    from pmu_hip.augment import Augment
    return Augment(rotate_deg=0, scale=(1, 1), shift=0, elastic=0, gain=0, bias=0)


# ------------------------------------------------------------------ 1. identity == the plain path
def test_identity_equals_standard_gather(std):
    assert std.scans[0].pshape == (20, 17, 20)
    shapes = {0: (17, 20), 1: (20, 20), 2: (20, 17)}
    for v, n in ((0, 20), (1, 17), (2, 20)):
        keys = [(0, v, 0), (1, v, n - 1), (0, v, n // 2), (1, v, 1), (0, v, n - 1), (1, v, 0), (1, v, n // 3)]
        want = std.get_slices(keys)
        for aug in (_zero_strength(), Fixed(np.tile(A.IDENTITY, (7, 1))), Fixed(np.tile(A.IDENTITY, (7, 1)), np.zeros((7, 2, 5, 5)))):
            got = std.get_slices(keys, augment=aug, epoch=3)
            assert tuple(got["image"].shape) == (7, 1) + shapes[v] and got["image"].dtype == torch.float32
            assert tuple(got["mask"].shape) == (7, 1) + shapes[v] and got["mask"].dtype == torch.float32
            assert torch.equal(got["image"], want["image"]) and torch.equal(got["mask"], want["mask"]), v
        assert float(want["image"].max()) == 1.0 and float(want["mask"].max()) == 2.0
    # get_batch: dataset indices, the same items
    idx = [5, 0, 11]
    a, b = std.get_batch(idx), std.get_batch(idx, augment=_zero_strength(), epoch=1)
    assert torch.equal(a["image"], b["image"]) and torch.equal(a["mask"], b["mask"])
    with pytest.raises(RuntimeError):
        std.get_slices([(0, 0, 1), (0, 1, 1)], augment=_zero_strength())     # two shapes in one batch
    with pytest.raises(KeyError):
        std.get_slices([(0, 0, 20)], augment=_zero_strength())


def test_identity_equals_oblique_gather(dev):
    P, h = 20, 0.75
    ds = _dataset(SCANS, dev, filter=False, views=_views9(), sample_dim=P, spacing=h)
    keys = [(0, 0, 0), (1, 1, P - 1), (0, 2, P // 2), (1, 3, 3), (0, 4, P - 1), (1, 8, 0), (0, 6, 7)]
    want = ds.get_slices(keys)
    fixed = Fixed(np.tile(A.IDENTITY, (7, 1)))
    for aug in (_zero_strength(), fixed):
        got = ds.get_slices(keys, augment=aug, epoch=2)
        assert tuple(got["image"].shape) == (7, 1, P, P)
        assert torch.equal(got["image"], want["image"]) and torch.equal(got["mask"], want["mask"])
    assert fixed.seen == [(keys, 2, P, P, h)]
    assert float(want["image"].abs().max()) > 0 and float(want["mask"].max()) == 2.0
    with pytest.raises(KeyError):
        ds.get_slices([(0, 9, 0)], augment=_zero_strength())


# ------------------------------------------------------------------ 2. the kernel vs the restatement
def _rot(deg, s=1.0, mirror=False):
    t = np.deg2rad(deg)
    c, sn, k = np.cos(t) * s, np.sin(t) * s, -1.0 if mirror else 1.0
    return ((c, -sn * k), (sn, c * k))


def _blocks(H, W, h):
    """Seven hand-built blocks (ds left 0): rotation and scale, a mirrored item, a translation that pushes part
    of the slice outside the volume, one that pushes all of it outside, gain and bias, the identity, a mix."""
    ea, eb = h * (H - 1), h * (W - 1)
    return np.stack([A.block(0.0, _rot(17.3, 1.07)),
                     A.block(0.0, _rot(-8.0, 0.93, mirror=True)),
                     A.block(0.0, t=(0.45 * ea, -0.35 * eb)),
                     A.block(0.0, t=(0.0, 4.0 * eb + 40.0)),
                     A.block(0.0, _rot(3.0), gain=1.1, bias=-0.03),
                     A.block(),
                     A.block(0.0, _rot(31.0, 1.2), t=(-2.25, 1.5), gain=0.9, bias=0.02)])


def _ctrl(G, H, W, h, seed):
    if not G:
        return None
    spacing = h * (min(H, W) - 1) / (G - 3)
    return np.random.RandomState(seed).uniform(-0.3 * spacing, 0.3 * spacing, size=(7, 2, G, G))


def _check_against_restatement(got, items, H, W, h, par, ctrl):
    """items: per batch entry (padded image, padded mask, frame, ds, slice max)."""
    for b, (img, lab, frame, ds, m) in enumerate(items):
        blk = par[b].copy()
        blk[0] = ds
        wi, wm = A.warp_item(img, lab, frame, H, W, h, blk, None if ctrl is None else ctrl[b], m)
        assert np.array_equal(got["image"][b, 0].cpu().numpy(), wi), b
        assert np.array_equal(got["mask"][b, 0].cpu().numpy(), wm), b
    out = got["image"][3], got["mask"][3]           # the item translated wholly outside the volume
    assert not bool(out[0].any()) and not bool(out[1].any())
    part = got["image"][2, 0]                       # the item pushed partly outside: zeros and samples
    assert bool(got["mask"][0].any()) and bool(part.any()) and bool((part == 0).any())


@pytest.mark.parametrize("G", [0, 4, 7])
@pytest.mark.parametrize("P,h", [(20, 1.0), (29, 0.75)])
def test_warp_gather_bitexact_oblique(P, h, G, dev):
    from pmu_hip import _lib as L
    views = _views9()
    ds = _dataset(SCANS, dev, filter=False, views=views, sample_dim=P, spacing=h)
    keys = [(0, 0, P // 2), (1, 1, P // 2 + 1), (0, 2, P // 2 - 2), (1, 3, P // 2), (0, 4, P // 3), (1, 5, P - 1), (0, 8, P // 2 + 3)]
    par, ctrl = _blocks(P, P, h), _ctrl(G, P, P, h, 10 * P + G)
    items = [(PADS[s][0], PADS[s][1], ds.frames[v], A.slice_offset(h, sl, P),
              R.sample_view(PADS[s][0], ds.frames[v], P, h, False)[sl].max()) for s, v, sl in keys]
    got = ds.get_slices(keys, augment=Fixed(par, ctrl), epoch=0)
    assert tuple(got["image"].shape) == (7, 1, P, P) and tuple(got["mask"].shape) == (7, 1, P, P)
    _check_against_restatement(got, items, P, P, h, par, ctrl)
    # the entry under its own name: no maxima, one output at a time
    blk = par.copy()
    blk[:, 0] = [it[3] for it in items]
    d_par = torch.from_numpy(blk).to(dev)
    d_ctrl = None if ctrl is None else torch.from_numpy(ctrl).to(dev)
    item = torch.tensor([[s * 9 + v, (s * 9 + v) * P + sl] for s, v, sl in keys], dtype=torch.int32, device=dev)
    raw = torch.full((7, P, P), -7.0, dtype=torch.float32, device=dev)
    msk = torch.full((7, P, P), -7.0, dtype=torch.float32, device=dev)
    args = (ds._vaddr_img.data_ptr(), ds._vaddr_mask.data_ptr(), ds._dims.data_ptr(), ds._frames.data_ptr(), 18,
            item.data_ptr(), None, d_par.data_ptr(), L.ptr(d_ctrl), G, 7, P, P, h)
    L.call("pmu_warp_gather", *args, raw.data_ptr(), None, L.stream())
    L.call("pmu_warp_gather", *args, None, msk.data_ptr(), L.stream())
    for b, (img, lab, frame, _, _) in enumerate(items):
        wi, wm = A.warp_item(img, lab, frame, P, P, h, blk[b], None if ctrl is None else ctrl[b], None)
        assert np.array_equal(raw[b].cpu().numpy(), wi) and np.array_equal(msk[b].cpu().numpy(), wm), b


@pytest.mark.parametrize("G", [0, 4, 7])
def test_warp_gather_bitexact_standard_rectangular(G, std):
    """The standard dataset's 17 x 20 view (slices along axis 0 of the 20 x 17 x 20 padded scans)."""
    from utils.mri_dataset import view_frame
    H, W, h = 17, 20, 1.0
    keys = [(0, 0, 9), (1, 0, 10), (0, 0, 7), (1, 0, 9), (0, 0, 12), (1, 0, 19), (0, 0, 0)]
    par, ctrl = _blocks(H, W, h), _ctrl(G, H, W, h, 77 + G)
    f = view_frame([1, 0, 0])
    items = [(PADS[s][0], PADS[s][1], f, sl - 19 / 2.0, PADS[s][0][sl].max()) for s, _, sl in keys]
    got = std.get_slices(keys, augment=Fixed(par, ctrl), epoch=0)
    assert tuple(got["image"].shape) == (7, 1, H, W)
    _check_against_restatement(got, items, H, W, h, par, ctrl)


def test_default_augment_runs_bitexact_and_changes_the_slices(dev):
    """The real draws end to end: Augment's blocks through the dataset equal the restatement fed the same
    blocks, differ from the plain slices, and repeat."""
    from pmu_hip.augment import Augment
    P, h = 20, 1.0
    ds = _dataset(SCANS, dev, filter=False, views=_views9()[:3], sample_dim=P, spacing=h)
    keys = [(0, 0, 9), (1, 1, 10), (0, 2, 8), (1, 0, 11)]
    aug = Augment(seed=9, flip=True)
    got = ds.get_slices(keys, augment=aug, epoch=4)
    par, ctrl = aug.draw(keys, 4, P, P, h)
    for b, (s, v, sl) in enumerate(keys):
        blk = par[b].copy()
        blk[0] = A.slice_offset(h, sl, P)
        m = R.sample_view(PADS[s][0], ds.frames[v], P, h, False)[sl].max()
        wi, wm = A.warp_item(PADS[s][0], PADS[s][1], ds.frames[v], P, P, h, blk, ctrl[b], m)
        assert np.array_equal(got["image"][b, 0].cpu().numpy(), wi) and np.array_equal(got["mask"][b, 0].cpu().numpy(), wm)
    plain, again, other = ds.get_slices(keys), ds.get_slices(keys, augment=aug, epoch=4), ds.get_slices(keys, augment=aug, epoch=5)
    assert torch.equal(again["image"], got["image"]) and torch.equal(again["mask"], got["mask"])
    assert not torch.equal(plain["image"], got["image"]) and not torch.equal(other["image"], got["image"])
    assert set(got["mask"].unique().tolist()) <= {0.0, 1.0, 2.0}


# ------------------------------------------------------------------ 3. lattice moves vs numpy indexing
def _shifted(plain, da, db):
    """out[..., a, b] = plain[..., a + da, b + db], zeros outside."""
    H, W = plain.shape[-2:]
    out = np.zeros_like(plain)
    a0, a1, b0, b1 = max(0, -da), min(H, H - da), max(0, -db), min(W, W - db)
    out[..., a0:a1, b0:b1] = plain[..., a0 + da:a1 + da, b0 + db:b1 + db]
    return out


def test_lattice_moves_equal_numpy_indexing(dev):
    """24^3, standard axes: a quarter turn (M = [[0,-1],[1,0]] reads pixel (a, b) at plane position (-b, a):
    np.rot90 with k = -1), a mirror of the second axis and the integer shift (3, -5) of the plain slices."""
    ds = _dataset([_scan((24, 24, 24), 1), _scan((24, 24, 24), 2)], dev, filter=False)
    moves = ((((0.0, -1.0), (1.0, 0.0)), (0.0, 0.0), lambda p: np.rot90(p, -1, axes=(-2, -1))),
             (((1.0, 0.0), (0.0, -1.0)), (0.0, 0.0), lambda p: np.flip(p, -1)),
             (((1.0, 0.0), (0.0, 1.0)), (3.0, -5.0), lambda p: _shifted(p, 3, -5)))
    for v in range(3):
        keys = [(0, v, 0), (1, v, 23), (0, v, 11), (1, v, 6), (0, v, 17)]
        plain = ds.get_slices(keys)
        for M, t, op in moves:
            got = ds.get_slices(keys, augment=Fixed(np.tile(A.block(0.0, M, t), (5, 1))))
            for k in ("image", "mask"):
                assert np.array_equal(got[k].cpu().numpy(), op(plain[k].cpu().numpy())), (v, M, t, k)
        assert float(plain["mask"].max()) == 2.0


# ------------------------------------------------------------------ 4. refusals
def test_warp_gather_refusals(std):
    from pmu_hip import _lib as L
    dev = std.device
    vi, vm, dims, frames, nrows, maxv = std._warp_tables()
    keys = [(0, 1, 4), (1, 1, 9)]
    want = std.get_slices(keys)
    par = np.tile(A.IDENTITY, (2, 1))
    par[:, 0] = [4 - 16 / 2.0, 9 - 16 / 2.0]
    d_par = torch.from_numpy(par).to(dev)
    d_ctrl = torch.zeros(2, 2, 16, 16, dtype=torch.float64, device=dev)
    item = torch.tensor([[1, std._gid[keys[0]]], [4, std._gid[keys[1]]]], dtype=torch.int32, device=dev)
    img = torch.zeros(2, 1, 20, 20, device=dev)
    msk = torch.zeros(2, 1, 20, 20, device=dev)
    # (vaddr_img, vaddr_mask, dims, frames, nrows, item, maxv, par, ctrl, G, B, H, W, h, img, mask)
    good = [vi.data_ptr(), vm.data_ptr(), dims.data_ptr(), frames.data_ptr(), nrows, item.data_ptr(), maxv.data_ptr(),
            d_par.data_ptr(), d_ctrl.data_ptr(), 0, 2, 20, 20, 1.0, img.data_ptr(), msk.data_ptr()]
    bad_cases = [{9: 1}, {9: 3}, {9: 17}, {9: -1}, {11: 1}, {12: 1}, {10: 0}, {10: -2}, {14: None, 15: None}, {13: 0.0},
                 {13: -1.0}, {13: float("nan")}, {9: 4, 8: None}, {0: None}, {1: None}, {2: None}, {3: None}, {5: None},
                 {7: None}, {4: 0}]
    for case in bad_cases:
        args = list(good)
        for i, v in case.items():
            args[i] = v
        with pytest.raises(RuntimeError, match="invalid argument"):
            L.call("pmu_warp_gather", *args, L.stream())
    torch.cuda.synchronize()
    assert not bool(img.any()) and not bool(msk.any())     # nothing was launched
    for G in (0, 16):                                      # a following valid call is right (a zero grid moves nothing)
        args = list(good)
        args[9] = G
        L.call("pmu_warp_gather", *args, L.stream())
        assert torch.equal(img, want["image"]) and torch.equal(msk, want["mask"])
        img.zero_(), msk.zero_()


# ------------------------------------------------------------------ 5. training wiring
class _Recording:
    """A dataset wrapper that records how train_net asks for batches."""

    def __init__(self, ds, net):
        self.ds, self.net, self.calls = ds, net, []

    def __len__(self):
        return len(self.ds)

    def get_batch(self, *args, **kw):
        self.calls.append((len(args), dict(kw), self.net.training))
        return self.ds.get_batch(*args, **kw)


def test_train_net_wiring(dev, tmp_path):
    import train as train_mod
    from pmu_hip.augment import Augment
    from trainer import UNetTrainer
    ds = train_mod.bench_dataset(1, 32, 1, dev)
    train_mod.dir_checkpoint = str(tmp_path) + "/"

    def run(augment):
        torch.manual_seed(0)
        tr = UNetTrainer(dev, n_channels=1, n_classes=1, num_filters=[8, 16])
        rec = _Recording(ds, tr.net)
        train_mod.train_net(tr, dev, epochs=1, batch_size=4, lr=0.01, dataset=rec, writer=train_mod._NullWriter(),
                            augment=augment)
        return rec.calls, [p.detach().clone() for p in tr.net.parameters()]

    aug = Augment(seed=3)
    calls, p3 = run(aug)
    train_calls = [c for c in calls if c[2]]
    val_calls = [c for c in calls if not c[2]]
    assert len(train_calls) >= 4 and len(val_calls) >= 1
    assert all(n == 1 and kw == {"augment": aug, "epoch": 0} for n, kw, _ in train_calls)
    assert all(n == 1 and kw == {} for n, kw, _ in val_calls)
    _, p3b = run(Augment(seed=3))
    assert all(torch.equal(a, b) for a, b in zip(p3, p3b))
    _, p4 = run(Augment(seed=4))
    assert any(not torch.equal(a, b) for a, b in zip(p3, p4))
    calls0, p0 = run(None)
    assert all(n == 1 and kw == {} for n, kw, _ in calls0)
    assert any(not torch.equal(a, b) for a, b in zip(p3, p0))
