"""Learned multi-planar fusion without a GPU: the numpy restatement (tests/fusion_fit_ref.py) is consistent with
itself — its gradient against central differences, its Newton solver on the fit problem — and the host side of
pmu_hip.fusion: the deterministic L-BFGS on the restatement's objective, FusionWeights, the refusals, the flags."""
import numpy as np
import pytest
import torch

import fusion_fit_ref as F


def _standard(shape, C, seed, logits=False):
    st, truth, W, b, cw = F.standard_case(shape, C, seed, logits)
    p, cover = F.standard_probs(*st, logits=logits)
    return p, cover, truth, W, b, cw


def test_restatement_gradient_matches_central_differences():
    """d(sum l / sum w) / d theta from the restatement's sums against (f(theta + e) - f(theta - e)) / 2e, e = 1e-6:
    the truncation error is O(e^2) = 1e-12 and the rounding of f (1e-16) divided by 2e is 5e-11."""
    p, cover, truth, W, b, cw = _standard((3, 7, 9), 3, 1)
    theta = np.concatenate([W.ravel(), b])
    f, g = F.objective(p, cover, truth, theta, cw, l2=1e-2, theta0=np.zeros_like(theta))
    num = np.zeros_like(theta)
    for n in range(theta.size):
        e = np.zeros_like(theta)
        e[n] = 1e-6
        num[n] = (F.objective(p, cover, truth, theta + e, cw, 1e-2, np.zeros_like(theta))[0]
                  - F.objective(p, cover, truth, theta - e, cw, 1e-2, np.zeros_like(theta))[0]) / 2e-6
    assert np.max(np.abs(num - g)) < 1e-9, np.max(np.abs(num - g))
    # an oblique problem: partly covered voxels change which weights a voxel's z depends on
    st, frames, truth, W, b, cw = F.oblique_case((9, 12, 10), 12, 2, 3, 4)
    p, cover = F.oblique_probs(st, frames, truth.shape, 12, 1.0)
    assert (cover.sum(0) == 0).any() and (cover.sum(0) == 1).any() and (cover.sum(0) == 2).any()
    theta = np.concatenate([W.ravel(), b])
    f, g = F.objective(p, cover, truth, theta, cw)
    for n in range(theta.size):
        e = np.zeros_like(theta)
        e[n] = 1e-6
        num = (F.objective(p, cover, truth, theta + e, cw)[0] - F.objective(p, cover, truth, theta - e, cw)[0]) / 2e-6
        assert abs(num - g[n]) < 1e-9, (n, num, g[n])


def test_restatement_conventions():
    """Voxels with a truth outside [0, C) or no covering view have no fit weight; the zero class weight removes its
    class; uniform weights give the plain mean's label wherever the mean has no tie."""
    p, cover, truth, W, b, cw = _standard((3, 7, 9), 3, 2)
    t = truth.astype(np.int64)
    r = F.evaluate(p, cover, truth, W, b, cw)
    inside = (t >= 0) & (t < 3)
    assert (~inside).sum() >= 2
    assert r["sums"][0] == pytest.approx(float(cw[np.clip(t, 0, 2)][inside].sum()), rel=1e-14)
    u = F.evaluate(p, cover, truth, np.full((3, 3), 1 / 3), np.zeros(3))
    mean = p.astype(np.float64).mean(0)
    srt = np.sort(mean, 0)
    clear = srt[-1] - srt[-2] > 1e-9
    assert clear.mean() > 0.99 and np.array_equal(u["label"][clear], np.argmax(mean, 0)[clear])
    assert np.allclose(r["q"].sum(0), 1.0, atol=1e-15) and r["prob"].shape == (3, 3, 7, 9)


def test_newton_and_lbfgs_reach_the_optimum_of_the_fit_problem():
    """The fit problem of the GPU test (5 x 37 x 34, C = 3, l2 = 1e-3): Newton with the exact Hessian reaches
    ||g||inf < 1e-12; the package's L-BFGS on the same objective converges below gtol = 1e-9 within 300 iterations
    to within gtol / l2 of it (strong convexity: ||theta - theta*|| <= ||g|| / l2); the learned fusion's Dice
    exceeds the plain mean's on every class."""
    from pmu_hip.fusion import FusionWeights, lbfgs_minimize
    v0, v1, v2, truth = F.fit_problem()
    p, cover = F.standard_probs(v0, v1, v2)
    th0 = FusionWeights.uniform(3, 3).theta()
    xs, fs, gs = F.newton(p, cover, truth, th0, l2=1e-3)
    assert np.max(np.abs(gs)) < 1e-12, np.max(np.abs(gs))
    x, f, g, iters, evals, conv, hist = lbfgs_minimize(lambda t: F.objective(p, cover, truth, t, None, 1e-3, th0), th0,
                                                       1e-9, 300)
    print(f"L-BFGS: {iters} iterations, {evals} evaluations, ||g||inf {np.max(np.abs(g)):.2e}, loss {hist[0]:.6f} -> "
          f"{f:.6f}; |theta - theta*| {np.linalg.norm(x - xs):.2e}")
    assert conv and np.max(np.abs(g)) < 1e-9 and iters <= 300
    assert np.linalg.norm(x - xs) <= 1e-9 / 1e-3
    assert f <= hist[0] and all(b <= a + 1e-12 for a, b in zip(hist, hist[1:]))
    again = lbfgs_minimize(lambda t: F.objective(p, cover, truth, t, None, 1e-3, th0), th0, 1e-9, 300)
    assert np.array_equal(again[0], x) and again[3:5] == (iters, evals)          # deterministic
    W, b = F.unpack(xs, 3, 3)
    mean = F.dice(F.evaluate(p, cover, truth, np.full((3, 3), 1 / 3), np.zeros(3))["counts"][3])
    fit = F.dice(F.evaluate(p, cover, truth, W, b)["counts"][3])
    print(f"Dice plain mean {np.round(mean, 4)} learned {np.round(fit, 4)}")
    assert np.all(fit > mean), (mean, fit)


def test_logits_case_margin_share_stays_under_its_cap():
    """The GPU test's logits case compares labels only where the restatement's top-two z gap exceeds 1e-5 and may
    leave out at most 1 % of the voxels: for seeded N(0, 3^2) logits the share is far below that."""
    for shape, C in (((5, 37, 34), 3), ((3, 33, 65), 8), ((5, 37, 34), 2)):
        st, truth, W, b, cw = F.standard_case(shape, C, 11, logits=True)
        p, cover = F.standard_probs(*st, logits=True)
        share = float((F.evaluate(p, cover, truth, W, b, cw)["top2"] <= 1e-5).mean())
        print(f"logits case {shape} C={C}: share of voxels within 1e-5 of a tie {share:.2e}")
        assert share <= 0.01


def test_fusion_weights_round_trip(tmp_path):
    from pmu_hip.fusion import FusionWeights
    rs = np.random.RandomState(0)
    w = FusionWeights(rs.randn(3, 4), rs.randn(4))
    w.save(tmp_path / "std.npz")
    r = FusionWeights.load(tmp_path / "std.npz")
    assert np.array_equal(r.W, w.W) and np.array_equal(r.b, w.b) and r.frames is None
    assert r.W.dtype == np.float64 and (r.V, r.C) == (3, 4)
    from utils.mri_dataset import draw_views, view_frame
    frames = np.stack([view_frame(n) for n in draw_views(2, 0, 30)])
    o = FusionWeights(rs.randn(2, 3), rs.randn(3), frames)
    o.save(tmp_path / "obl.npz")
    r = FusionWeights.load(tmp_path / "obl.npz")
    assert np.array_equal(r.frames, frames) and np.array_equal(r.W, o.W)
    r.check_frames(frames)
    with pytest.raises(ValueError):
        r.check_frames(frames[::-1])
    with pytest.raises(ValueError):
        r.check_frames(None)
    with pytest.raises(ValueError):
        w.check_frames(frames)
    u = FusionWeights.uniform(3, 2)
    assert np.array_equal(u.W, np.full((3, 2), 1 / 3)) and np.array_equal(u.b, np.zeros(2))
    assert np.array_equal(FusionWeights.from_theta(w.theta(), 3, 4).W, w.W)
    with pytest.raises(ValueError):
        FusionWeights(np.zeros((3, 2)), np.zeros(3))
    with pytest.raises(ValueError):
        FusionWeights(np.zeros((3, 2)), np.zeros(2), frames)


def test_cpu_tensors_and_one_class_are_refused():
    from pmu_hip.fusion import FusionItem, FusionWeights, fit_fusion, fuse_oblique, fuse_views
    v0, v1, v2, t = (torch.zeros(2, 3, 4, 5), torch.zeros(4, 3, 2, 5), torch.zeros(5, 3, 2, 4), torch.zeros(2, 4, 5))
    w = FusionWeights.uniform(3, 3)
    with pytest.raises(RuntimeError):
        fuse_views(v0, v1, v2, t, weights=w)
    with pytest.raises(RuntimeError):
        fuse_oblique(torch.zeros(2, 4, 3, 4, 4), np.stack([np.eye(3)] * 2), torch.zeros(4, 4, 4), 4,
                     weights=FusionWeights.uniform(2, 3, np.stack([np.eye(3)] * 2)))
    with pytest.raises(RuntimeError):
        FusionItem([v0, v1, v2], t)
    with pytest.raises(RuntimeError):
        FusionItem(torch.zeros(2, 4, 3, 4, 4), torch.zeros(4, 4, 4), frames=np.stack([np.eye(3)] * 2))
    with pytest.raises(ValueError):
        fit_fusion([])


def test_one_class_is_refused_before_any_launch():
    """C = 1 has no fusion model: the host-side check that fuse_views, fuse_oblique and fit_fusion all pass their
    weights through refuses it, as it refuses too many classes, a shape mismatch and bad class weights
    (tests/test_fusion_fit_gpu.py raises the same through fuse_views on device tensors)."""
    from pmu_hip import fusion as M
    with pytest.raises(ValueError, match="C >= 2"):
        M._check_weights(M.FusionWeights.uniform(3, 1), 3, 1)
    with pytest.raises(ValueError, match="C >= 2"):
        M._check_weights(M.FusionWeights.uniform(2, 1), 2, 1)
    with pytest.raises(ValueError):
        M._check_weights(M.FusionWeights.uniform(3, 9), 3, 9)
    with pytest.raises(ValueError):
        M._check_weights(M.FusionWeights.uniform(3, 3), 3, 4)
    with pytest.raises(ValueError):
        M._class_weight([1.0, -1.0, 1.0], 3)
    with pytest.raises(ValueError):
        M._class_weight([1.0, 1.0], 3)


def test_eval_flags_exist():
    import eval as E
    a = E.get_args(["--fusion", "w.npz", "--fit-fusion", "data/val"])
    assert a.fusion == "w.npz" and a.fit_fusion == "data/val"
    a = E.get_args([])
    assert a.fusion is None and a.fit_fusion is None
