"""CPU checks of the slice augmentation's host side: the keyed parameter draws of pmu_hip.augment.Augment and
the numpy restatement of the warped gather (tests/augment_ref.py) against plain numpy indexing.  Nothing is
launched."""
import numpy as np
import pytest

import augment_ref as A
import oblique_ref as R

KEYS = [(0, 0, 3), (1, 2, 7), (0, 1, 19), (1, 0, 0), (0, 2, 11), (1, 1, 5), (0, 0, 4)]


def _scan(shape, seed, classes=3):
    rs = np.random.RandomState(seed)
    img = rs.randint(0, 256, size=shape).astype(np.float64)
    lab = np.zeros(shape)
    box = tuple(slice(n // 4, n - n // 4) for n in shape)
    lab[box] = rs.randint(0, classes, size=lab[box].shape)
    return img, lab


# ------------------------------------------------------------------ draws
def test_draws_are_deterministic_and_keyed_per_item():
    from pmu_hip.augment import Augment
    aug = Augment(seed=5, flip=True, p=0.7)
    par, ctrl = aug.draw(KEYS, 2, 20, 17, 0.75)
    assert par.shape == (7, 9) and par.dtype == np.float64 and ctrl.shape == (7, 2, 6, 6) and ctrl.dtype == np.float64
    assert np.all(par[:, 0] == 0.0)
    par2, ctrl2 = Augment(seed=5, flip=True, p=0.7).draw(KEYS, 2, 20, 17, 0.75)
    assert np.array_equal(par, par2) and np.array_equal(ctrl, ctrl2)
    # an item's block does not depend on the batch it is drawn in, nor on the order
    for b, k in enumerate(KEYS):
        p1, c1 = aug.draw([k], 2, 20, 17, 0.75)
        assert np.array_equal(p1[0], par[b]) and np.array_equal(c1[0], ctrl[b]), k
    perm = [4, 0, 6, 2, 5, 1, 3]
    pp, cp = aug.draw([KEYS[i] for i in perm] + [(3, 1, 2)], 2, 20, 17, 0.75)
    assert np.array_equal(pp[:7], par[perm]) and np.array_equal(cp[:7], ctrl[perm])
    # other epochs, seeds and items give other numbers
    for other in (aug.draw(KEYS, 3, 20, 17, 0.75), Augment(seed=6, flip=True, p=0.7).draw(KEYS, 2, 20, 17, 0.75),
                  aug.draw([(s, v, sl + 1) for s, v, sl in KEYS], 2, 20, 17, 0.75)):
        assert not np.array_equal(other[0], par) and not np.array_equal(other[1], ctrl)
    # distinct items never share a stream (the item words sit above the stream's own block counter)
    a, _ = Augment(seed=1).draw([(0, 0, 0), (1, 0, 0), (0, 1, 0), (0, 0, 1)], 0, 32, 32, 1.0)
    assert len({tuple(r) for r in a}) == 4


def test_draw_leaves_the_global_generators_alone():
    import torch
    from pmu_hip.augment import Augment
    t0, n0 = torch.get_rng_state(), np.random.get_state()
    Augment(seed=3).draw(KEYS, 0, 32, 32, 1.0)
    n1 = np.random.get_state()
    assert torch.equal(torch.get_rng_state(), t0)
    assert n0[0] == n1[0] and np.array_equal(n0[1], n1[1]) and n0[2:] == n1[2:]


def test_zero_strength_is_the_exact_identity():
    from pmu_hip.augment import Augment
    par, ctrl = Augment(rotate_deg=0, scale=(1, 1), shift=0, elastic=0, gain=0, bias=0).draw(KEYS, 4, 20, 17, 0.75)
    assert ctrl is None
    want = np.tile(A.IDENTITY, (7, 1))
    assert np.array_equal(par, want) and not np.any(np.signbit(par))
    # p = 0: every item gets the identity block and a zero control grid
    par, ctrl = Augment(p=0.0).draw(KEYS, 4, 20, 17, 0.75)
    assert np.array_equal(par, want) and not np.any(ctrl)


def test_draw_ranges():
    from pmu_hip.augment import Augment
    keys = [(s, v, sl) for s in range(2) for v in range(3) for sl in range(40)]
    for H, W, h, G, el in ((20, 20, 0.75, 6, 0.25), (17, 20, 1.0, 4, 0.4), (64, 48, 1.0, 16, 0.1)):
        aug = Augment(rotate_deg=20, scale=(0.8, 1.25), shift=0.1, flip=True, elastic=el, grid=G, gain=0.2, bias=0.1)
        par, ctrl = aug.draw(keys, 1, H, W, h)
        spacing = min(h * (H - 1) / (G - 3), h * (W - 1) / (G - 3))
        assert ctrl.shape == (len(keys), 2, G, G) and np.max(np.abs(ctrl)) <= el * spacing
        assert np.max(np.abs(ctrl)) > 0.5 * el * spacing
        M = par[:, 1:5].reshape(-1, 2, 2)
        det = M[:, 0, 0] * M[:, 1, 1] - M[:, 0, 1] * M[:, 1, 0]
        s = np.sqrt(np.abs(det))
        assert np.all(s >= 0.8 - 1e-12) and np.all(s <= 1.25 + 1e-12)
        assert np.any(det < 0) and np.any(det > 0)                        # mirrored and not
        assert np.max(np.abs(M @ M.transpose(0, 2, 1) - (s * s)[:, None, None] * np.eye(2))) <= 1e-12
        ang = np.rad2deg(np.arctan2(M[:, 1, 0], M[:, 0, 0]))
        assert np.max(np.abs(ang)) <= 20 + 1e-9 and np.max(np.abs(ang)) > 10
        assert np.max(np.abs(par[:, 5])) <= 0.1 * h * (H - 1) and np.max(np.abs(par[:, 6])) <= 0.1 * h * (W - 1)
        assert np.max(np.abs(par[:, 7] - 1.0)) <= 0.2 + 1e-15 and np.max(np.abs(par[:, 8])) <= 0.1


def test_augment_refusals():
    from pmu_hip.augment import Augment
    for bad in (dict(elastic=0.41), dict(elastic=-0.1), dict(grid=3), dict(grid=17), dict(grid=5.5), dict(p=1.5),
                dict(scale=(1.2, 0.9)), dict(scale=(0.0, 1.0)), dict(seed=-1)):
        with pytest.raises(ValueError):
            Augment(**bad)
    Augment(elastic=0.4, grid=4)
    Augment(elastic=0.0, grid=16)


# ------------------------------------------------------------------ the restatement against numpy indexing
@pytest.mark.parametrize("P,h", [(20, 1.0), (20, 0.75)])
def test_restatement_identity_is_the_oblique_restatement(P, h):
    from utils.mri_dataset import draw_views, view_frame
    img, lab = _scan((20, 17, 20), 3)
    for n in [np.array([1.0, 2.0, 3.0])] + draw_views(2, 0, 30):
        f = view_frame(n)
        (want_i, mx), (want_m, _) = R.view_items(img, f, P, h, False), R.view_items(lab, f, P, h, True)
        for s in (0, 3, P // 2, P - 1):
            gi, gm = A.warp_item(img, lab, f, P, P, h, A.block(A.slice_offset(h, s, P)), None, mx[s])
            assert np.array_equal(gi, want_i[s]) and np.array_equal(gm, want_m[s]), (n, s)
            zero = np.zeros((2, 5, 5))   # a zero control grid displaces nothing
            gi, gm = A.warp_item(img, lab, f, P, P, h, A.block(A.slice_offset(h, s, P)), zero, mx[s])
            assert np.array_equal(gi, want_i[s]) and np.array_equal(gm, want_m[s]), (n, s)


def _shifted(plain, da, db):
    """out[a, b] = plain[a + da, b + db], zeros outside."""
    H, W = plain.shape
    out = np.zeros_like(plain)
    a0, a1, b0, b1 = max(0, -da), min(H, H - da), max(0, -db), min(W, W - db)
    out[a0:a1, b0:b1] = plain[a0 + da:a1 + da, b0 + db:b1 + db]
    return out


LATTICE = (("rot90", ((0.0, -1.0), (1.0, 0.0)), (0.0, 0.0), lambda p: np.rot90(p, -1)),
           ("flip", ((1.0, 0.0), (0.0, -1.0)), (0.0, 0.0), lambda p: np.flip(p, 1)),
           ("shift", ((1.0, 0.0), (0.0, 1.0)), (3.0, -5.0), lambda p: _shifted(p, 3, -5)))


def test_restatement_lattice_moves_are_numpy_indexing():
    """On 24^3 along the standard axes a quarter turn, a mirror and an integer shift of the sampling grid land
    on voxels: the restatement is then plain numpy indexing of the slice, for image and mask.  M = [[0,-1],[1,0]]
    reads pixel (a, b) at plane position (-b, a): np.rot90 by one clockwise quarter turn (k = -1)."""
    from utils.mri_dataset import view_frame
    img, lab = _scan((24, 24, 24), 1)
    moved = lambda vol: [vol, vol.transpose(1, 0, 2), vol.transpose(2, 0, 1)]
    for v, f in enumerate(view_frame(e) for e in np.eye(3)):
        for s in (0, 7, 23):
            pi, pm = moved(img)[v][s], moved(lab)[v][s]
            m = pi.max()
            plain_i, plain_m = (pi / m).astype(np.float32), pm.astype(np.float32)
            for name, M, t, op in LATTICE:
                gi, gm = A.warp_item(img, lab, f, 24, 24, 1.0, A.block(s - 23 / 2.0, M, t), None, m)
                assert np.array_equal(gi, op(plain_i)) and np.array_equal(gm, op(plain_m)), (v, s, name)


# ------------------------------------------------------------------ spline weights
def test_spline_weights_partition_unity():
    rs = np.random.RandomState(11)
    for G in (4, 7, 16):
        n = 1001
        p = rs.uniform(0.0, n - 1.0, size=1000)
        i, w = A.spline_cell(p, n, G)
        assert np.all(i >= 0) and np.all(i <= G - 4)
        t = p * (float(G - 3) / float(n - 1)) - i
        assert np.all(t >= 0.0) and np.all(t < 1.0) and np.all(w >= 0.0)
        total = ((w[0] + w[1]) + w[2]) + w[3]
        assert np.max(np.abs(total - 1.0)) <= 2 * np.finfo(np.float64).eps, G
    # the ends of the axis: the last pixel belongs to the last cell with t = 1 (to rounding)
    for G, n in ((4, 20), (6, 17), (16, 29)):
        i, w = A.spline_cell(np.arange(n), n, G)
        assert i[0] == 0 and i[-1] == G - 4 and np.array_equal(w[:, 0], [1 / 6.0, 4 / 6.0, 1 / 6.0, 0.0])
        assert abs(w[3, -1] - 1 / 6.0) <= 1e-15 and abs(w[0, -1]) <= 1e-30
    assert not np.any(A.spline_cell(np.arange(50), 50, 4)[0])   # G = 4: one cell


def test_constant_control_grid_is_a_translation():
    """A control grid of one value displaces every pixel by that value (partition of unity), to rounding."""
    ctrl = np.empty((2, 6, 6))
    ctrl[0], ctrl[1] = 1.25, -0.5
    d = A.displacement(ctrl, 20, 17)
    assert np.max(np.abs(d[0] - 1.25)) <= 1e-15 and np.max(np.abs(d[1] + 0.5)) <= 1e-15
