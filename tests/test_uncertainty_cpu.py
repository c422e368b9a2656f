"""pmu_hip.uncertainty's generalised energy distance on the CPU (no GPU is used): ged_from_counts against a
brute-force numpy evaluation of the definition on small random maps, its fixed points, and the place of
the two new entry points in the ctypes tables."""
import numpy as np
import pytest
import torch


def _counts(maps, K):
    onehot = (maps[..., None] == np.arange(K)).astype(np.float64)      # [R][N][HW][K]
    return np.einsum("inpc,jnpc->nijc", onehot, onehot), onehot.sum(2).transpose(1, 0, 2)


def _dist(a, b, K):
    """1 - mean IoU over the foreground classes present in a or b (K = 1: the single class); 0 if none is."""
    ious = []
    for c in (range(1, K) if K > 1 else [0]):
        u = np.logical_or(a == c, b == c).sum()
        if u:
            ious.append(np.logical_and(a == c, b == c).sum() / u)
    return 1.0 - float(np.mean(ious)) if ious else 0.0


def _brute_ged(samples, truths, K):
    out = []
    for n in range(samples.shape[1]):
        s, t = samples[:, n], truths[:, n]
        st = np.mean([_dist(a, b, K) for a in s for b in t])
        ss = np.mean([_dist(a, b, K) for a in s for b in s])
        tt = np.mean([_dist(a, b, K) for a in t for b in t])
        out.append(2 * st - ss - tt)
    return np.array(out)


@pytest.mark.parametrize("S,M,N,HW,K", [(4, 1, 2, 37, 3), (3, 2, 1, 16, 1), (5, 3, 2, 50, 6), (1, 1, 3, 9, 2)])
def test_ged_from_counts_matches_brute_force(S, M, N, HW, K):
    from pmu_hip.uncertainty import ged_from_counts
    g = np.random.default_rng(S + 3 * M + 5 * N + 7 * HW + 11 * K)
    maps = g.integers(0, K + 1, size=(S + M, N, HW)).astype(np.uint8)   # label K: counted nowhere
    maps[0, 0] = 0                                                       # a map without foreground
    if K > 2:
        maps[maps == K - 1] = 1                                          # a class absent from every map
    got = ged_from_counts(*_counts(maps, K), S)
    want = _brute_ged(maps[:S], maps[S:], K)
    assert got.dtype == torch.float64 and tuple(got.shape) == (N,)
    assert np.abs(got.numpy() - want).max() <= 1e-12
    assert float(got.min()) >= -1e-12                                    # an energy distance


def test_ged_fixed_points():
    from pmu_hip.uncertainty import ged_from_counts
    K, HW = 3, 40
    g = np.random.default_rng(3)
    A = g.integers(0, K, size=HW).astype(np.uint8)
    B = g.integers(0, K, size=HW).astype(np.uint8)
    assert (A != B).any() and (A > 0).any() and (B > 0).any()
    stack = lambda maps: np.stack(maps)[:, None, :]                      # [R][N = 1][HW]
    # identical samples equal to the truth
    assert float(ged_from_counts(*_counts(stack([A, A, A, A]), K), 3)[0]) == 0.0
    # all background: no foreground class anywhere, every distance is 0
    Z = np.zeros(HW, np.uint8)
    assert float(ged_from_counts(*_counts(stack([Z, Z, Z]), K), 2)[0]) == 0.0
    # samples all equal to A, truth B: 2 d(A, B) - d(A, A) - d(B, B) = 2 d(A, B)
    got = float(ged_from_counts(*_counts(stack([A, A, A, B]), K), 3)[0])
    assert abs(got - 2 * _dist(A, B, K)) <= 1e-12 and got > 0
    with pytest.raises(ValueError):
        ged_from_counts(*_counts(stack([A, B]), K), 2)                   # no ground truth left


def test_new_entries_are_declared_and_not_counted_as_benchmark_mfma():
    from pmu_hip import _lib
    for name in ("pmu_fcomb_stats", "pmu_label_pair_counts"):
        assert name in _lib.SIGNATURES
        assert name not in _lib.MFMA_ENTRY_POINTS
    assert _lib.MFMA_UNCOUNTED == ("pmu_fcomb_stats",)
    assert len(_lib.SIGNATURES["pmu_fcomb_stats"][1]) == len(_lib.SIGNATURES["pmu_fcomb_fwd"][1]) + 4
