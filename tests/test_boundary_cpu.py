"""CPU-only checks of the boundary loss: the numpy restatement of the signed distance map against itself (the
separable form against the brute-force minimum) and against scipy's exact Euclidean transform, host-side
argument validation of the C entries (nothing is launched), and the opt-in wiring (train.py --loss /
--boundary-weight / --boundary-ramp, make_criterion)."""
import os

import numpy as np
import pytest
import torch

import boundary_ref as R


def _planes():
    """Small boolean planes: random at several densities and odd shapes, a single member, a single non-member,
    a member touching every border, lines one pixel wide, and the two degenerate ones."""
    rng = np.random.default_rng(5)
    out = []
    for shape in ((21, 17), (1, 40), (33, 1), (16, 16), (7, 70)):
        for density in (0.05, 0.5, 0.95):
            out.append(rng.random(shape) < density)
    one = np.zeros((19, 23), bool)
    one[0, 0] = True
    frame = np.zeros((12, 15), bool)
    frame[0, :] = frame[-1, :] = frame[:, 0] = frame[:, -1] = True
    out += [one, ~one, frame, ~frame, np.zeros((5, 6), bool), np.ones((5, 6), bool)]
    return out


def test_separable_map_equals_brute_force_bit_for_bit():
    for m in _planes():
        a, b = R.separable_plane(m), R.brute_plane(m)
        assert a.dtype == b.dtype == np.float32 and a.shape == m.shape
        assert np.array_equal(a.view(np.uint32), b.view(np.uint32)), m.shape


def test_map_equals_scipy_edt_cast_to_float32():
    """edt(neg) * neg - (edt(pos) - 1) * pos with scipy's float64 transforms cast to float32 first: rounding
    the float64 square root of an integer to float32 gives the correctly rounded float32 square root."""
    ndi = pytest.importorskip("scipy.ndimage")
    one = np.float32(1)
    for m in _planes():
        if not m.any() or m.all():
            continue   # phi = 0 by definition (scipy's transform of a plane without background is not a distance)
        to_member = ndi.distance_transform_edt(~m).astype(np.float32)
        to_other = ndi.distance_transform_edt(m).astype(np.float32)
        want = np.where(m, one - to_other, to_member).astype(np.float32)
        for got in (R.separable_plane(m), R.brute_plane(m)):
            assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), m.shape


def test_absent_and_full_planes_are_zero():
    for fn in (R.separable_plane, R.brute_plane):
        assert not fn(np.zeros((9, 11), bool)).any()
        assert not fn(np.ones((9, 11), bool)).any()
    t = torch.zeros(2, 6, 7, dtype=torch.long)
    t[1, 2:4, 3:5] = 2
    phi = R.signed_map(t, 3)
    assert phi.shape == (2, 3, 6, 7) and phi.dtype == torch.float32
    assert not phi[0].any()                       # image 0: class 0 fills it, classes 1 and 2 are absent
    assert not phi[1, 1].any() and phi[1, 0].any() and phi[1, 2].any()
    assert float(phi[1, 2, 2, 3]) == 0.0 and float(phi[1, 2, 0, 3]) == 2.0   # 1 - 1 inside, distance outside
    # an ignored pixel belongs to no class: it is a non-member of every plane
    t[0, 0, 0] = -100
    phi = R.signed_map(t, 3)
    assert float(phi[0, 0, 0, 0]) == 1.0 and float(phi[0, 0, 0, 1]) == 0.0 and not phi[0, 1].any()


def test_signed_map_of_a_float_mask():
    m = torch.zeros(1, 1, 5, 5)
    m[0, 0, 2, 2] = 0.5
    m[0, 0, 0, 0] = 0.49
    phi = R.signed_map(m, 1)
    assert float(phi[0, 0, 2, 2]) == 0.0 and float(phi[0, 0, 2, 0]) == 2.0
    assert float(phi[0, 0, 0, 0]) == np.sqrt(np.float32(8))


def test_boundary_entries_reject_bad_arguments_without_gpu():
    """Null pointers, K = 9, a side of 1025 and bad flags return PMU_ERR_ARG before any launch; the workspace
    query is a host function: 0 for a shape the kernels refuse."""
    from pmu_hip._lib import LIB_PATH, PMU_ERR_ARG, load_library
    if not os.path.exists(LIB_PATH):
        pytest.skip("library not built")
    cdll = load_library()
    p = 4096   # a non-null address: never dereferenced, the argument checks return first
    assert cdll.pmu_boundary_map(None, 0, 2, 3, 8, 8, -100, None, None, None) == PMU_ERR_ARG
    assert cdll.pmu_boundary_map(p, 0, 2, 9, 8, 8, -100, p, p, None) == PMU_ERR_ARG        # K
    assert cdll.pmu_boundary_map(p, 0, 2, 3, 1025, 8, -100, p, p, None) == PMU_ERR_ARG     # H
    assert cdll.pmu_boundary_map(p, 0, 2, 3, 8, 0, -100, p, p, None) == PMU_ERR_ARG        # W
    assert cdll.pmu_boundary_map(p, 1, 2, 3, 8, 8, -100, p, p, None) == PMU_ERR_ARG        # a float mask with K = 3
    assert cdll.pmu_boundary_map(p, 0, 2, 1, 8, 8, -100, p, p, None) == PMU_ERR_ARG        # class indices with K = 1
    assert cdll.pmu_boundary_map(p, 0, 2, 3, 8, 8, -100, p, p + 4, None) == PMU_ERR_ARG    # ws alignment
    assert cdll.pmu_boundary_fwd(None, None, None, 2, 3, 64, 0, 0, -100, None, None, None, None) == PMU_ERR_ARG
    assert cdll.pmu_boundary_fwd(p, p, p, 2, 9, 64, 0, 0, -100, p, p, p, None) == PMU_ERR_ARG
    assert cdll.pmu_boundary_fwd(p, p, p, 2, 3, 64, 2, 0, -100, p, p, p, None) == PMU_ERR_ARG       # act
    assert cdll.pmu_boundary_fwd(p, p, p, 2, 3, 64, 0, 2, -100, p, p, p, None) == PMU_ERR_ARG       # first_class
    assert cdll.pmu_boundary_fwd(p, None, p, 2, 3, 64, 0, 0, -100, p, p, p, None) == PMU_ERR_ARG    # K >= 2 needs tgt
    assert cdll.pmu_boundary_fwd(p, p, p, 2, 3, 64, 0, 0, -100, p, p + 4, p, None) == PMU_ERR_ARG   # count alignment
    assert cdll.pmu_boundary_bwd(None, None, None, 2, 3, 64, 0, 0, -100, None, None, None, None) == PMU_ERR_ARG
    assert cdll.pmu_boundary_bwd(p, p, p, 0, 3, 64, 0, 0, -100, p, p, p, None) == PMU_ERR_ARG       # N
    assert cdll.pmu_boundary_bwd(p, p, p, 2, 3, (1 << 20) + 1, 0, 0, -100, p, p, p, None) == PMU_ERR_ARG
    assert cdll.pmu_boundary_ws(2, 9, 8, 8) == 0 and cdll.pmu_boundary_ws(2, 3, 8, 1025) == 0
    # one partial row (2 doubles) per block, a flag word per plane (padded to 8 bytes), a 64-bit word per
    # class, row and 64 columns
    assert cdll.pmu_boundary_ws(2, 3, 8, 8) == 2 * 1 * 16 + 24 + 2 * 3 * 8 * 1 * 8
    assert cdll.pmu_boundary_ws(1, 1, 256, 70) == 9 * 16 + 8 + 256 * 2 * 8


def test_boundary_loss_refuses_cpu_tensors_and_bad_inputs():
    from pmu_hip.boundary import signed_distance
    from pmu_hip.loss import BoundaryLoss
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        BoundaryLoss()(torch.rand(2, 3, 4, 4), torch.zeros(2, 4, 4, dtype=torch.long))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        signed_distance(torch.zeros(2, 4, 4, dtype=torch.long), 3)
    m = BoundaryLoss()
    assert (m.include_background, m.ignore_index, m.from_logits) == (False, -100, None)
    m = BoundaryLoss(True, 255, True)
    assert (m.include_background, m.ignore_index, m.from_logits) == (True, 255, True)


def test_train_parser_boundary_flags():
    import train as T
    a = T.get_args([])
    assert (a.loss, a.boundary_weight, a.boundary_ramp) == ("default", 0.01, 0.01)
    a = T.get_args(["--loss", "ce+boundary", "--boundary-weight", "0.05", "--boundary-ramp", "0.002"])
    assert (a.loss, a.boundary_weight, a.boundary_ramp) == ("ce+boundary", 0.05, 0.002)
    assert T.get_args(["--loss", "dice+boundary", "-m", "probunet"]).loss == "dice+boundary"
    with pytest.raises(SystemExit):
        T.get_args(["--loss", "boundary+ce"])
    assert [T.boundary_weight_at(e, 0.01, 0.01) for e in range(3)] == [0.01, 0.02, 0.03]


def test_make_criterion_builds_the_boundary_choices():
    from pmu_hip.loss import (LOSS_CHOICES, BCELoss, BoundaryLoss, CrossEntropyLoss, RegionPlusBoundaryLoss,
                              SoftDiceLoss, make_criterion)
    assert LOSS_CHOICES == ("default", "dice", "ce+dice", "ce+boundary", "dice+boundary")
    c = make_criterion(3, "ce+boundary")
    assert type(c) is RegionPlusBoundaryLoss and type(c.region) is CrossEntropyLoss and type(c.boundary) is BoundaryLoss
    assert c.weight == 0.01 and not c.boundary.include_background
    c = make_criterion(1, "ce+boundary")
    assert type(c.region) is BCELoss
    c = make_criterion(3, "dice+boundary")
    assert type(c) is RegionPlusBoundaryLoss and type(c.region) is SoftDiceLoss
    with pytest.raises(ValueError):
        make_criterion(3, "boundary")


def test_boundary_weight_is_set_where_the_trainer_keeps_it():
    """train.set_boundary_weight: the criterion of a "+boundary" trainer, the net of a "+boundary" ELBO; any
    other trainer is left alone (nothing of the schedule runs without the new choices)."""
    import train as T
    from pmu_hip.loss import make_criterion
    from model import ProbabilisticUnet

    class Net:
        pass

    class Tr:
        pass

    tr = Tr()
    tr.net, tr.criterion = Net(), make_criterion(3, "ce+boundary")
    assert T.set_boundary_weight(tr, 0.25) and tr.criterion.weight == 0.25
    tr.criterion = make_criterion(3, "ce+dice")
    assert not T.set_boundary_weight(tr, 0.5) and not hasattr(tr.criterion, "weight")
    tr.net.recon_loss = "dice+boundary"
    assert T.set_boundary_weight(tr, 0.5) and tr.net.boundary_weight == 0.5
    tr.net = Net()
    tr.net.recon_loss = "ce+dice"
    assert not T.set_boundary_weight(tr, 0.5) and not hasattr(tr.net, "boundary_weight")
    assert ProbabilisticUnet.boundary_weight == 0.01
