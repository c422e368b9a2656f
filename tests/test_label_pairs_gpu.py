"""pmu_label_pair_counts (csrc/label_pairs.hip) against numpy, exactly: random u8 label maps with some
labels >= K (counted nowhere), one 256-pixel step and several, a partial last step, HW = 1, the largest map
count, K = 1 and K = 32; the symmetry of inter, its diagonal against cnt, bitwise repeatability of two
calls, the argument bounds, and pmu_hip.uncertainty.ged on the GPU against ged_from_counts fed the numpy
counts."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

# (R, N, HW, K)
CASES = [(17, 2, 63, 3), (5, 3, 1, 32), (64, 1, 130, 2), (2, 1, 4097, 1)]


def _maps(R, N, HW, K):
    g = np.random.default_rng(R + 3 * N + 5 * HW + 7 * K)
    m = g.integers(0, K + 2, size=(R, N, HW)).astype(np.uint8)      # about 2 / (K + 2) of the labels are >= K
    m[g.random((R, N, HW)) < 0.05] = 255
    if HW > 8:
        m[: R // 2, :, : HW // 2] = 0                               # a shared background region
    m[0, 0, 0], m[-1, -1, -1] = K, 0                                # (HW = 1: both kinds of label are present)
    return m


def _numpy_counts(m, K):
    R, N, HW = m.shape
    onehot = (m[..., None] == np.arange(K)).astype(np.float64)      # [R][N][HW][K]
    inter = np.einsum("inpc,jnpc->nijc", onehot, onehot)
    cnt = onehot.sum(2).transpose(1, 0, 2)
    return inter, cnt


@pytest.mark.parametrize("R,N,HW,K", CASES)
def test_label_pair_counts_exact(dev, R, N, HW, K):
    from pmu_hip import _lib as L
    m = _maps(R, N, HW, K)
    assert (m >= K).any() and (m < K).any()
    md = torch.from_numpy(m).to(dev)
    outs = []
    for _ in range(2):
        inter = torch.full((N, R, R, K), float("nan"), dtype=torch.float64, device=dev)
        cnt = torch.full((N, R, K), float("nan"), dtype=torch.float64, device=dev)
        L.call("pmu_label_pair_counts", md.data_ptr(), R, N, HW, K, inter.data_ptr(), cnt.data_ptr(), L.stream())
        torch.cuda.synchronize()
        outs.append((inter.cpu(), cnt.cpu()))
    (inter, cnt), (inter2, cnt2) = outs
    assert torch.equal(inter, inter2) and torch.equal(cnt, cnt2)      # the same integers on every run
    ri, rc = _numpy_counts(m, K)
    assert np.array_equal(inter.numpy(), ri)
    assert np.array_equal(cnt.numpy(), rc)
    assert torch.equal(inter, inter.transpose(1, 2))
    assert torch.equal(torch.diagonal(inter, dim1=1, dim2=2).permute(0, 2, 1), cnt)
    assert float(cnt.sum()) < R * N * HW                              # labels >= K were counted nowhere


@pytest.mark.parametrize("R,N,HW,K", CASES)
def test_ged_on_gpu_matches_numpy_counts(dev, R, N, HW, K):
    from pmu_hip.uncertainty import ged, ged_from_counts
    m = _maps(R, N, HW, K)
    S = R - 1 if R < 4 else R - 3                                     # 1 or 3 ground truths
    md = torch.from_numpy(m).to(dev)
    got = ged(md[:S], md[S:], K)
    torch.cuda.synchronize()
    want = ged_from_counts(*_numpy_counts(m, K), S)
    assert got.dtype == torch.float64 and got.shape == (N,)
    # the counts are the same integers; the float64 means over at most 64 x 64 distances in [0, 1] are summed
    # in another order on the GPU: at most 4096 x 2^-53 apart per mean
    assert float((got.cpu() - want).abs().max()) <= 1e-12


def test_label_pair_counts_refuses_shapes_outside_its_bounds(dev):
    from pmu_hip import _lib as L
    from pmu_hip.uncertainty import label_pair_counts
    big = torch.zeros(1 << 12, dtype=torch.uint8, device=dev)
    out = torch.full((1 << 16,), float("nan"), dtype=torch.float64, device=dev)
    lib, s, p, o = L.lib(), L.stream(), big.data_ptr(), out.data_ptr()
    for R, N, HW, K in ((65, 1, 4, 1), (4, 1, 4, 33), (64, 1, 1, 4), (0, 1, 4, 2), (4, 0, 4, 2), (4, 1, 0, 2)):
        assert lib.pmu_label_pair_counts(p, R, N, HW, K, o, o, s) == L.PMU_ERR_ARG, (R, N, HW, K)
    assert lib.pmu_label_pair_counts(None, 4, 1, 4, 2, o, o, s) == L.PMU_ERR_ARG
    torch.cuda.synchronize()
    assert torch.isnan(out).all()                                     # nothing was launched or cleared
    with pytest.raises(ValueError):
        label_pair_counts(big.view(64, 1, 64), 4)                     # 2080 pairs x 4 classes > 8192 counters
