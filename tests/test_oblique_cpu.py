"""CPU checks of the oblique views' host side: view_frame, the seeded view draw, and the numpy
restatement's geometry (tests/oblique_ref.py).  Nothing is launched."""
import numpy as np
import pytest

import oblique_ref as R


def _directions(n, seed=5):
    return np.random.RandomState(seed).normal(size=(n, 3))


def test_view_frame_is_orthonormal():
    from utils.mri_dataset import view_frame
    for n in _directions(100):
        f = view_frame(n)
        assert f.shape == (3, 3) and f.dtype == np.float64
        assert np.max(np.abs(f @ f.T - np.eye(3))) <= 1e-15, n
        m = int(np.argmax(np.abs(f[0])))
        assert f[0][m] > 0
        a, b = [i for i in range(3) if i != m]
        assert f[1][a] > 0 and f[2][b] > 0      # u leans to +e_a, v to +e_b


def test_view_frame_standard_axes_exact():
    from utils.mri_dataset import view_frame
    e = np.eye(3)
    for m, (a, b) in enumerate(((1, 2), (0, 2), (0, 1))):
        for scale in (1.0, 3.0, -2.0):
            f = view_frame(scale * e[m])
            assert np.array_equal(f, np.stack([e[m], e[a], e[b]])), (m, scale)
            assert not np.any(np.signbit(f))


def test_view_frame_sign_invariant_and_refuses_zero():
    from utils.mri_dataset import view_frame
    for n in _directions(100, seed=6):
        assert np.array_equal(view_frame(n), view_frame(-n))
    for bad in ([0, 0, 0], [np.nan, 1, 0], [1, 0], [np.inf, 0, 0]):
        with pytest.raises(ValueError):
            view_frame(bad)


def test_initialize_views_oblique_draw():
    from utils.mri_dataset import MRI_Dataset, draw_views, view_frame
    views = MRI_Dataset.initialize_views(None, False, n_views=6, seed=0)
    again = MRI_Dataset.initialize_views(None, False, n_views=6, seed=0)
    assert len(views) == 6 and all(np.array_equal(a, b) for a, b in zip(views, again))
    assert all(np.array_equal(a, b) for a, b in zip(views, draw_views(6, 0, 30)))
    lim = np.cos(np.deg2rad(30.0))
    for i, n in enumerate(views):
        assert abs(np.sqrt(np.sum(n * n)) - 1.0) <= 1e-15
        assert np.array_equal(view_frame(n)[0], n) or np.max(np.abs(view_frame(n)[0] - n)) <= 1e-15   # canonical
        assert n[int(np.argmax(np.abs(n)))] > 0
        for o in views[:i]:
            assert abs(float(np.dot(n, o))) <= lim
    other = draw_views(6, 1, 30)
    assert not all(np.array_equal(a, b) for a, b in zip(views, other))
    assert len(draw_views(3, 0, 60)) == 3
    with pytest.raises(ValueError):
        draw_views(20, 0, 60)     # twenty lines pairwise 60 degrees apart do not exist


def test_initialize_views_standard_unchanged():
    from utils.mri_dataset import MRI_Dataset
    std = MRI_Dataset.initialize_views(None, use_standard_axis=True)
    assert len(std) == 3
    for got, want in zip(std, ([1, 0, 0], [0, 1, 0], [0, 0, 1])):
        assert isinstance(got, np.ndarray) and got.dtype == np.array([1]).dtype and got.tolist() == want


@pytest.mark.parametrize("P,h", [(20, 1.0), (29, 0.75)])
def test_restatement_maps_are_mutual_inverses(P, h):
    from utils.mri_dataset import view_frame
    pshape = (20, 17, 20)
    rs = np.random.RandomState(7)
    for n in _directions(10, seed=8):
        f = view_frame(n)
        s, a, b = rs.uniform(-3.0, P + 2.0, size=(3, 500))
        x = R.grid_to_voxel(pshape, f, P, h, s, a, b)
        g = R.voxel_to_grid(pshape, f, P, h, *x)
        assert max(np.max(np.abs(g[0] - s)), np.max(np.abs(g[1] - a)), np.max(np.abs(g[2] - b))) <= 1e-12
        x0, x1, x2 = rs.uniform(-5.0, 25.0, size=(3, 500))
        g = R.voxel_to_grid(pshape, f, P, h, x0, x1, x2)
        y = R.grid_to_voxel(pshape, f, P, h, *g)
        assert max(np.max(np.abs(y[0] - x0)), np.max(np.abs(y[1] - x1)), np.max(np.abs(y[2] - x2))) <= 1e-12


def test_restatement_axis_aligned_is_plain_slicing():
    """Along the standard axes at the defaults the restatement is image[i,:,:], image[:,j,:], image[:,:,k]
    with preprocess' max normalisation, and its fusion of grid-aligned stacks is their plain average."""
    from utils.mri_dataset import view_frame
    rs = np.random.RandomState(9)
    D = 12
    img = rs.randint(0, 256, size=(D, D, D)).astype(np.float64)
    lab = rs.randint(0, 3, size=(D, D, D)).astype(np.float64)
    frames = [view_frame(e) for e in np.eye(3)]
    moved = [img, img.transpose(1, 0, 2), img.transpose(2, 0, 1)]
    for f, want in zip(frames, moved):
        items, mx = R.view_items(img, f, D, 1.0, False)
        assert np.array_equal(mx, want.reshape(D, -1).max(1))
        assert np.array_equal(items, (want / mx[:, None, None]).astype(np.float32))
    assert np.array_equal(R.view_items(lab, frames[1], D, 1.0, True)[0], lab.transpose(1, 0, 2).astype(np.float32))
    C = 3
    st = rs.uniform(size=(3, D, C, D, D)).astype(np.float32)
    st /= st.sum(2, keepdims=True)
    avg, label, cover, counts = R.fuse(st, frames, lab, D, 1.0)
    v0, v1, v2 = st[0], st[1].transpose(2, 1, 0, 3), st[2].transpose(2, 1, 3, 0)
    assert np.array_equal(avg, (v0 + v1 + v2) / np.float32(3.0))
    assert np.all(cover == 3) and np.array_equal(label, np.argmax(avg, 1))
    assert counts[:, :, 2].sum(1).tolist() == [D ** 3] * 4 and counts[:, :, 1].sum(1).tolist() == [D ** 3] * 4


def test_restatement_ball_round_trip_value():
    """The round trip of tests/test_oblique_gpu.py on the restatement alone: a ball sliced along six views
    at the nearest voxel and fused back scores the Dice DESIGN.md records (the value is what the
    geometry gives, not a threshold: nearest-voxel slices resampled trilinearly blur the surface)."""
    import torch
    from pmu_hip.metrics import dice_from_counts
    from utils.mri_dataset import draw_views, view_frame
    frames = np.stack([view_frame(n) for n in draw_views(6, 0, 30)])
    truth, stacks, (avg, label, cover, counts) = R.ball_round_trip(frames, 32, 1.0)
    d = dice_from_counts(torch.from_numpy(counts))[6].numpy()
    print(f"ball round trip, six views, 32^3: fused Dice {d.tolist()}, uncovered voxels {int((cover == 0).sum())}")
    assert counts[6, 1, 2] == truth.sum() and 0.0 < d[1] <= 1.0
