"""Learned multi-planar fusion on the GPU: pmu_fusion3_eval and pmu_fusion_oblique_eval (csrc/fusion_fit.hip)
called under their own names against the numpy restatement of tests/fusion_fit_ref.py and against the plain-mean
kernels, the reproducibility of the sums, pmu_hip.fusion.fit_fusion against a Newton optimum, predict_volume with
``fusion``, and the refusals.  Every test needs the new entries.

Bounds.  label, counts, cover: bit-equal (z is evaluated in one order in fp64 on both sides; the counters are
integers).  prob: 2^-22 relative — the fp64 error of q sits far below fp32 rounding, so at most a double-rounding
ulp can differ.  Each sum: 1e-10 x sum |terms| — fp64 eps x N with N <= 1e4 terms plus a few ulp for exp / log is
about 1e-12; the bound leaves 100 x over that.  With logits the restatement's fp32 softmax differs from the device's
expf by ulps (~1e-7 of a probability), so every sum is held to 1e-5 relative to the restatement's sum itself (on
the seeded cases no sum cancels below a twentieth of its sum |terms|) and labels are compared where the
restatement's two largest z differ by more than 1e-5, which may leave out at most 1 % of the voxels
(tests/test_fusion_fit_cpu.py: far fewer).
"""
import ctypes
import os

import numpy as np
import pytest
import torch

import fusion_fit_ref as F

pytestmark = pytest.mark.gpu

_REF = {}


def _dbl(a):
    a = np.ascontiguousarray(a, dtype=np.float64).ravel()
    return (ctypes.c_double * a.size)(*a.tolist())


def _theta(W, b):
    return np.concatenate([np.asarray(W, dtype=np.float64).ravel(), np.asarray(b, dtype=np.float64).ravel()])


def _dev(dev, *arrays):
    return [torch.from_numpy(np.ascontiguousarray(a)).to(dev) for a in arrays]


def _eval3(dev, st, truth, W, b, cw, logits, sums=None, accumulate=0, outputs=True):
    """pmu_fusion3_eval under its own name.  Returns numpy outputs (and the device sums tensor)."""
    from pmu_hip import _lib as L
    v0, v1, v2, tr = _dev(dev, *st, truth)
    D0, C, D1, D2 = v0.shape
    prob = torch.full((D0, C, D1, D2), float("nan"), device=dev) if outputs else None
    label = torch.full((D0, D1, D2), -7, dtype=torch.int32, device=dev) if outputs else None
    counts = torch.full((4, C, 3), float("nan"), dtype=torch.float64, device=dev) if outputs else None
    if sums is None:
        sums = torch.full((2 + C + 3 * C,), float("nan"), dtype=torch.float64, device=dev)
    nbytes = int(L.lib().pmu_fusion3_ws(D0, D1, D2, C))
    assert nbytes > 0 and nbytes % 8 == 0
    ws = torch.empty(nbytes // 8, dtype=torch.float64, device=dev)
    L.call("pmu_fusion3_eval", v0.data_ptr(), v1.data_ptr(), v2.data_ptr(), tr.data_ptr(), D0, D1, D2, C, int(logits),
           _dbl(_theta(W, b)), None if cw is None else _dbl(cw), L.ptr(prob), L.ptr(label), L.ptr(counts),
           sums.data_ptr(), int(accumulate), ws.data_ptr(), nbytes, L.stream())
    torch.cuda.synchronize()
    out = {"sums": sums.cpu().numpy(), "sums_dev": sums}
    if outputs:
        out.update(prob=prob.cpu().numpy(), label=label.cpu().numpy(), counts=counts.cpu().numpy())
    return out


def _eval_oblique(dev, st, frames, truth, P, h, W, b, cw, outputs=True):
    """pmu_fusion_oblique_eval under its own name."""
    from pmu_hip import _lib as L
    s, fr, tr = _dev(dev, st, np.asarray(frames, dtype=np.float64).reshape(-1, 9), truth)
    V, C = st.shape[0], st.shape[2]
    p0, p1, p2 = truth.shape
    prob = torch.full((p0, C, p1, p2), float("nan"), device=dev) if outputs else None
    label = torch.full((p0, p1, p2), -7, dtype=torch.int32, device=dev) if outputs else None
    cover = torch.full((p0, p1, p2), -7, dtype=torch.int32, device=dev) if outputs else None
    counts = torch.full((V + 1, C, 3), float("nan"), dtype=torch.float64, device=dev) if outputs else None
    sums = torch.full((2 + C + V * C,), float("nan"), dtype=torch.float64, device=dev)
    nbytes = int(L.lib().pmu_fusion_oblique_ws(V, C, p0, p1, p2))
    assert nbytes > 0 and nbytes % 8 == 0
    ws = torch.empty(nbytes // 8, dtype=torch.float64, device=dev)
    L.call("pmu_fusion_oblique_eval", s.data_ptr(), fr.data_ptr(), V, C, P, float(h), tr.data_ptr(), p0, p1, p2,
           _dbl(_theta(W, b)), None if cw is None else _dbl(cw), L.ptr(prob), L.ptr(label), L.ptr(cover), L.ptr(counts),
           sums.data_ptr(), 0, ws.data_ptr(), nbytes, L.stream())
    torch.cuda.synchronize()
    out = {"sums": sums.cpu().numpy()}
    if outputs:
        out.update(prob=prob.cpu().numpy(), label=label.cpu().numpy(), cover=cover.cpu().numpy(),
                   counts=counts.cpu().numpy())
    return out


def _check(got, ref, capsys, tag, sums_rel=1e-10, labels_where=None):
    err = np.abs(got["sums"] - ref["sums"])
    worst = float(np.max(err / np.maximum(ref["abs_sums"], 1e-300)))
    if labels_where is not None:       # the logits case: relative to each sum of the restatement itself
        own = float(np.max(err / np.abs(ref["sums"])))
        with capsys.disabled():
            print(f"FUSION {tag}: sums err / |sum| {own:.2e} (bound {sums_rel:.0e}); least |sum| / sum|terms| "
                  f"{float(np.min(np.abs(ref['sums']) / ref['abs_sums'])):.3f}", flush=True)
        assert np.all(err <= sums_rel * np.abs(ref["sums"])), (err, ref["sums"])
    want = ref["prob"].astype(np.float64)
    rel = np.abs(got["prob"].astype(np.float64) - want) / np.maximum(np.abs(want), 1e-300)
    rel = np.where(ref["prob"] == got["prob"], 0.0, rel)
    with capsys.disabled():
        print(f"FUSION {tag}: sums err / sum|terms| {worst:.2e} (bound {sums_rel:.0e}); prob rel err {rel.max():.2e} "
              f"(bound {2.0 ** -22:.2e})", flush=True)
    assert np.all(err <= sums_rel * ref["abs_sums"]), (err, ref["abs_sums"])
    if labels_where is None:
        assert np.array_equal(got["label"], ref["label"])
        assert np.array_equal(got["counts"], ref["counts"])
        assert rel.max() <= 2.0 ** -22
    else:
        assert np.array_equal(got["label"][labels_where], ref["label"][labels_where])


# ------------------------------------------------------------------ 1. the standard kernel vs the restatement
@pytest.mark.parametrize("C", [2, 3, 8])
@pytest.mark.parametrize("shape", [(1, 1, 1), (5, 37, 34), (3, 33, 65)])
def test_standard_kernel_matches_restatement(shape, C, dev, capsys):
    st, truth, W, b, cw = F.standard_case(shape, C, 100 * C + shape[1])
    p, cover = F.standard_probs(*st)
    ref = F.evaluate(p, cover, truth, W, b, cw)
    t = truth.astype(np.int64)
    if shape != (1, 1, 1):
        assert ((t < 0) | (t >= C)).sum() >= 2 and (W < 0).any() and (b < 0).any() and (cw == 0).any()
    got = _eval3(dev, st, truth, W, b, cw, 0)
    _check(got, ref, capsys, f"standard {shape} C={C}")
    # every output is optional: the sums alone (the fit's pass) are the same bits
    alone = _eval3(dev, st, truth, W, b, cw, 0, outputs=False)
    assert np.array_equal(alone["sums"], got["sums"])


# ------------------------------------------------------------------ 2. the per-view rows are pmu_fuse3view's
@pytest.mark.parametrize("logits", [0, 1])
@pytest.mark.parametrize("shape,C", [((5, 37, 34), 3), ((3, 33, 65), 8)])
def test_uniform_weights_keep_the_plain_kernels_view_rows(shape, C, logits, dev):
    from pmu_hip.fusion import fuse_views
    st, truth, _, _, _ = F.standard_case(shape, C, 7, logits=bool(logits))
    got = _eval3(dev, st, truth, np.full((3, C), 1.0 / 3.0), np.zeros(C), None, logits)
    v0, v1, v2, tr = _dev(dev, *st, truth)
    plain = fuse_views(v0, v1, v2, tr, logits=bool(logits))
    want = plain["counts"].cpu().numpy()
    assert np.array_equal(got["counts"][:3], want[:3])
    assert np.array_equal(got["counts"][:, :, 2], want[:, :, 2])


# ------------------------------------------------------------------ 3. logits
@pytest.mark.parametrize("shape,C", [((5, 37, 34), 3), ((3, 33, 65), 8)])
def test_logits_case_matches_restatement(shape, C, dev, capsys):
    st, truth, W, b, cw = F.standard_case(shape, C, 11, logits=True)
    p, cover = F.standard_probs(*st, logits=True)
    ref = F.evaluate(p, cover, truth, W, b, cw)
    clear = ref["top2"] > 1e-5
    assert 1.0 - clear.mean() <= 0.01
    got = _eval3(dev, st, truth, W, b, cw, 1)
    _check(got, ref, capsys, f"logits {shape} C={C}", sums_rel=1e-5, labels_where=clear)


# ------------------------------------------------------------------ 4. determinism
def test_sums_are_reproducible_and_accumulate_in_call_order(dev):
    a = F.standard_case((5, 37, 34), 3, 21)
    c = F.standard_case((3, 33, 65), 3, 22)
    W, b, cw = a[2], a[3], a[4]
    s1 = _eval3(dev, a[0], a[1], W, b, cw, 0, outputs=False)["sums"]
    s1a = _eval3(dev, a[0], a[1], W, b, cw, 0, outputs=False)["sums"]      # the same call twice
    s1b = _eval3(dev, a[0], a[1], W, b, cw, 0)["sums"]                     # and with every output asked for
    s2 = _eval3(dev, c[0], c[1], W, b, cw, 0, outputs=False)["sums"]
    assert np.array_equal(s1, s1a) and np.array_equal(s1, s1b)
    assert np.all(np.isfinite(s1)) and np.all(np.isfinite(s2))
    first = _eval3(dev, a[0], a[1], W, b, cw, 0, outputs=False)
    both = _eval3(dev, c[0], c[1], W, b, cw, 0, sums=first["sums_dev"], accumulate=1, outputs=False)["sums"]
    assert np.array_equal(both, s1 + s2)
    assert not np.array_equal(both, s1)


# ------------------------------------------------------------------ 5. the oblique kernel vs the restatement
@pytest.mark.parametrize("C", [2, 3])
@pytest.mark.parametrize("V", [1, 2, 6, 8])
@pytest.mark.parametrize("h", [1.0, 0.75])
def test_oblique_kernel_matches_restatement(h, V, C, dev, capsys):
    from pmu_hip.fusion import fuse_oblique
    shape, P = (9, 12, 10), 12
    st, frames, truth, W, b, cw = F.oblique_case(shape, P, V, C, 10 * V + C)
    p, cover = F.oblique_probs(st, frames, shape, P, h)
    ref = F.evaluate(p, cover, truth, W, b, cw)
    none = ~cover.any(0)
    if h == 0.75:
        assert none.any()            # the 9-voxel-wide grid does not reach the ends of the 12- and 10-voxel axes
    if V > 1:
        assert (cover.sum(0) < V).any() and (cover.sum(0) > 0).any()
    got = _eval_oblique(dev, st, frames, truth, P, h, W, b, cw)
    _check(got, ref, capsys, f"oblique h={h} V={V} C={C}")
    assert np.array_equal(got["cover"], ref["cover_n"])
    # voxels no view covers: label 0, probability 0, absent from sum w (the restatement leaves them out)
    assert np.all(got["label"][none] == 0) and np.all(got["prob"].transpose(1, 0, 2, 3)[:, none] == 0)
    t = truth.astype(np.int64)
    w_all = np.where((t >= 0) & (t < C), cw[np.clip(t, 0, C - 1)], 0.0)
    assert abs(got["sums"][0] - w_all[~none].sum()) <= 1e-10 * w_all.sum()
    if none.any() and w_all[none].sum() > 0:
        assert got["sums"][0] < w_all.sum() - 0.5 * w_all[none].sum()
    # the per-view rows and the cover are pmu_fuse_oblique's
    s, tr = _dev(dev, st, truth)
    plain = fuse_oblique(s, frames, tr, P, h)
    assert np.array_equal(got["counts"][:V], plain["counts"].cpu().numpy()[:V])
    assert np.array_equal(got["cover"], plain["cover"].cpu().numpy())
    alone = _eval_oblique(dev, st, frames, truth, P, h, W, b, cw, outputs=False)
    assert np.array_equal(alone["sums"], got["sums"])


# ------------------------------------------------------------------ 6. the fit
def _newton_standard():
    if "std" not in _REF:
        v0, v1, v2, truth = F.fit_problem()
        p, cover = F.standard_probs(v0, v1, v2)
        th0 = np.concatenate([np.full(9, 1.0 / 3.0), np.zeros(3)])
        xs, fs, gs = F.newton(p, cover, truth, th0, l2=1e-3)
        assert np.max(np.abs(gs)) < 1e-12
        _REF["std"] = (v0, v1, v2, truth, p, cover, th0, xs)
    return _REF["std"]


def test_fit_reaches_the_newton_optimum(dev, capsys):
    from pmu_hip.fusion import FusionItem, FusionWeights, fit_fusion, fuse_views
    v0, v1, v2, truth, p, cover, th0, xs = _newton_standard()
    d = _dev(dev, v0, v1, v2, truth)
    fit = fit_fusion([FusionItem(d[:3], d[3])], l2=1e-3, gtol=1e-9, max_iter=300)
    x = fit.weights.theta()
    f_ref, g_ref = F.objective(p, cover, truth, x, None, 1e-3, th0)
    dist = float(np.linalg.norm(x - xs))
    with capsys.disabled():
        print(f"FUSION fit: {fit.iterations} iterations, {fit.evaluations} evaluations, loss {fit.loss_initial:.6f} -> "
              f"{fit.loss:.6f}, |g|inf {fit.grad_norm:.2e} (restatement {np.max(np.abs(g_ref)):.2e}), "
              f"|theta - theta*| {dist:.2e} (bound {1e-9 / 1e-3:.0e})", flush=True)
    assert fit.converged and fit.grad_norm < 1e-9 and fit.iterations <= 300
    assert np.max(np.abs(g_ref)) < 1e-9
    assert dist <= 1e-9 / 1e-3
    assert fit.loss <= fit.loss_initial and len(fit.history) == fit.iterations + 1
    assert abs(fit.loss - f_ref) <= 1e-12
    plain = fuse_views(*d[:3], d[3])
    learned = fuse_views(*d[:3], d[3], weights=fit.weights)
    dp, dl = plain["dice"][3].cpu().numpy(), learned["dice"][3].cpu().numpy()
    with capsys.disabled():
        print(f"FUSION fit: Dice plain mean {np.round(dp, 4)} learned {np.round(dl, 4)}", flush=True)
    assert np.all(dl > dp), (dp, dl)
    assert torch.equal(plain["counts"][:3], learned["counts"][:3])
    assert abs(float(learned["loss"]) + 0.5e-3 * float((x - th0) @ (x - th0)) - fit.loss) <= 1e-12
    # the fit is deterministic
    again = fit_fusion([FusionItem(d[:3], d[3])], l2=1e-3, gtol=1e-9, max_iter=300)
    assert np.array_equal(again.weights.theta(), x) and again.evaluations == fit.evaluations
    # "balanced" class weights: N / (C N_c) of the fitting scans
    from pmu_hip.fusion import balanced_class_weight
    n = np.bincount(truth.astype(np.int64).ravel(), minlength=3).astype(np.float64)
    assert np.allclose(balanced_class_weight([d[3]], 3), n.sum() / (3 * n), rtol=1e-15)
    bal = fit_fusion([FusionItem(d[:3], d[3])], class_weight="balanced", l2=1e-3, gtol=1e-6, max_iter=300)
    assert bal.converged and bal.loss <= bal.loss_initial
    with pytest.raises(ValueError):
        fit_fusion([FusionItem(d[:3], d[3])], init=FusionWeights.uniform(3, 4))


def test_fit_through_an_oblique_item(dev, capsys):
    from pmu_hip.fusion import FusionItem, FusionWeights, fit_fusion
    shape, P, V, C = (9, 12, 10), 12, 2, 3
    st, frames, truth, _, _, _ = F.oblique_case(shape, P, V, C, 5)
    p, cover = F.oblique_probs(st, frames, shape, P, 1.0)
    th0 = FusionWeights.uniform(V, C).theta()
    xs, fs, gs = F.newton(p, cover, truth, th0, l2=1e-3)
    assert np.max(np.abs(gs)) < 1e-12
    s, tr = _dev(dev, st, truth)
    two = fit_fusion([FusionItem(s, tr, frames=frames, sample_dim=P)] * 2, l2=1e-3, gtol=1e-9, max_iter=300)
    fit = fit_fusion([FusionItem(s, tr, frames=frames, sample_dim=P)], l2=1e-3, gtol=1e-9, max_iter=300)
    x = fit.weights.theta()
    g_ref = F.objective(p, cover, truth, x, None, 1e-3, th0)[1]
    dist = float(np.linalg.norm(x - xs))
    with capsys.disabled():
        print(f"FUSION oblique fit: {fit.iterations} iterations, loss {fit.loss_initial:.6f} -> {fit.loss:.6f}, |g|inf "
              f"{fit.grad_norm:.2e} (restatement {np.max(np.abs(g_ref)):.2e}), |theta - theta*| {dist:.2e}", flush=True)
    assert fit.converged and np.max(np.abs(g_ref)) < 1e-9 and dist <= 1e-9 / 1e-3
    assert fit.loss <= fit.loss_initial
    assert np.array_equal(fit.weights.frames, frames)
    # the same scan twice: twice the sums, the same objective up to rounding, the same optimum
    assert two.converged and np.linalg.norm(two.weights.theta() - xs) <= 1e-9 / 1e-3


# ------------------------------------------------------------------ 7. predict_volume
def _scan(shape, seed):
    rs = np.random.RandomState(seed)
    img = rs.randint(0, 256, size=shape).astype(np.float64)
    lab = np.zeros(shape)
    box = tuple(slice(n // 4, n - n // 4) for n in shape)
    lab[box] = rs.randint(0, 3, size=lab[box].shape)
    return img, lab


def _dataset(scans, dev, **kw):
    from utils.mri_dataset import MRI_Dataset
    names = [f"s{i}" for i in range(len(scans))]
    store = dict(zip(names, scans))
    return MRI_Dataset("/imgs", "/labs", 3, loader=lambda p: store[os.path.basename(p)][0 if "imgs" in p else 1],
                       files=names, device=dev, **kw)


def test_predict_volume_with_fusion(dev, capsys):
    from model import UNet
    from pmu_hip.fusion import FusionWeights, fuse_oblique, fuse_views
    from predict import fit_fusion_model, predict_volume
    from utils.mri_dataset import draw_views
    torch.manual_seed(0)
    net = UNet(1, 3, [4, 8]).to(dev).eval()
    ds = _dataset([_scan((16, 12, 10), 6), _scan((16, 12, 10), 7)], dev, filter=False)
    res = predict_volume(net, ds, 0, batch_size=8)
    assert set(res) == {"avg", "label", "counts", "dice", "stacks", "truth"}
    parent = fuse_views(*res["stacks"], res["truth"], logits=True)
    for k in ("avg", "label", "counts", "dice"):
        assert torch.equal(res[k], parent[k]), k
    rs = np.random.RandomState(3)
    W = FusionWeights(rs.uniform(0.0, 1.0, size=(3, 3)), rs.uniform(-0.2, 0.2, size=3))
    got = predict_volume(net, ds, 0, batch_size=8, fusion=W)
    want = fuse_views(*got["stacks"], got["truth"], logits=True, weights=W)
    assert set(got) == set(res) | {"loss"}
    for k in ("avg", "label", "counts", "dice", "loss"):
        assert torch.equal(got[k], want[k]), k
    for a, b_ in zip(got["stacks"], res["stacks"]):
        assert torch.equal(a, b_)
    assert torch.equal(got["counts"][:3], res["counts"][:3])
    fit = fit_fusion_model(net, ds, [0, 1], batch_size=8, l2=1e-3, max_iter=30)
    with capsys.disabled():
        print(f"FUSION fit_fusion_model: loss {fit.loss_initial:.6f} -> {fit.loss:.6f} in {fit.iterations} iterations",
              flush=True)
    assert fit.loss < fit.loss_initial and fit.weights.frames is None and (fit.weights.V, fit.weights.C) == (3, 3)
    # oblique views: the weights carry the frames and are refused on others
    ob = _dataset([_scan((16, 12, 10), 6)], dev, filter=False, views=draw_views(2, 1, 30))
    ofit = fit_fusion_model(net, ob, [0], batch_size=8, l2=1e-3, max_iter=30)
    assert ofit.loss < ofit.loss_initial and np.array_equal(ofit.weights.frames, ob.frames)
    ores = predict_volume(net, ob, 0, batch_size=8, fusion=ofit.weights)
    owant = fuse_oblique(torch.stack(ores["stacks"]), ob.frames, ores["truth"], ob.sample_dim, ob.spacing,
                         weights=ofit.weights)
    for k in ("avg", "label", "cover", "counts", "loss"):
        assert torch.equal(ores[k], owant[k]), k
    with pytest.raises(ValueError):
        predict_volume(net, ob, 0, batch_size=8, fusion=W)
    with pytest.raises(ValueError):
        predict_volume(net, ds, 0, batch_size=8, fusion=ofit.weights)


def test_fit_and_apply_on_sample_mean_stacks(dev):
    """uncertainty=True: the stacks are the mean probabilities of the prior samples, not logits.  fit_fusion_model
    fits on that kind of stacks (the same draws give the same stacks as predict_volume's), the weights apply to them
    with logits off, and the entropy and mutual-information maps keep the plain mean."""
    from model import ProbabilisticUnet
    from pmu_hip.fusion import FusionItem, fit_fusion, fuse_views
    from predict import fit_fusion_model, predict_volume
    torch.manual_seed(0)
    net = ProbabilisticUnet(1, 3, [8, 16], latent_dim=6, no_convs_fcomb=4).to(dev).eval()
    ds = _dataset([_scan((16, 12, 10), 6)], dev, filter=False)
    mode = dict(batch_size=8, prob=True, n_samples=3, faithful=False, uncertainty=True)
    torch.manual_seed(1)
    plain = predict_volume(net, ds, 0, **mode)
    torch.manual_seed(1)
    fit = fit_fusion_model(net, ds, [0], l2=1e-3, max_iter=20, **mode)
    want = fit_fusion([FusionItem(plain["stacks"], plain["truth"], logits=False)], l2=1e-3, max_iter=20)
    assert np.array_equal(fit.weights.theta(), want.weights.theta()) and fit.loss < fit.loss_initial
    torch.manual_seed(1)
    got = predict_volume(net, ds, 0, fusion=fit.weights, **mode)
    ref = fuse_views(*plain["stacks"], plain["truth"], logits=False, weights=fit.weights)
    assert set(got) == set(plain) | {"loss"}
    for k in ("avg", "label", "counts", "dice", "loss"):
        assert torch.equal(got[k], ref[k]), k
    for k in ("entropy", "mutual_info"):
        assert torch.equal(got[k], plain[k]), k
    d = fit.weights.theta() - np.concatenate([np.full(9, 1.0 / 3.0), np.zeros(3)])
    assert abs(float(got["loss"]) + 0.5e-3 * float(d @ d) - fit.loss) <= 1e-12


# ------------------------------------------------------------------ 8. refusals
def test_refusals_before_any_launch(dev):
    from pmu_hip import _lib as L
    lib, E = L.lib(), L.PMU_ERR_ARG
    C, D = 3, (4, 5, 6)
    v0, v1, v2 = (torch.zeros(4, C, 5, 6, device=dev), torch.zeros(5, C, 4, 6, device=dev),
                  torch.zeros(6, C, 4, 5, device=dev))
    tr = torch.zeros(*D, device=dev)
    par = _dbl(np.zeros(8 * 9 + 9))
    sums = torch.zeros(2 + 9 + 81, dtype=torch.float64, device=dev)
    need = int(lib.pmu_fusion3_ws(*D, C))
    ws = torch.zeros(need // 8 + 1024, dtype=torch.float64, device=dev)
    f3 = lib.pmu_fusion3_eval
    p = (v0.data_ptr(), v1.data_ptr(), v2.data_ptr(), tr.data_ptr())

    def std(C_=C, par_=par, ws_=ws.data_ptr(), nbytes=need, sums_=sums.data_ptr(), ptrs=p):
        return f3(*ptrs, *D, C_, 0, par_, None, None, None, None, sums_, 0, ws_, nbytes, None)

    assert std() == 0
    assert std(C_=1) == E and std(C_=9) == E and std(C_=0) == E
    assert std(par_=None) == E
    assert std(nbytes=need - 8) == E and std(ws_=None) == E
    assert std(ws_=ws.data_ptr() + 4) == E                      # rows of doubles: 8-byte aligned
    assert std(ptrs=(None,) + p[1:]) == E and std(ptrs=p[:3] + (None,)) == E
    assert std(par_=_dbl(np.full(12, np.nan))) == E
    assert f3(*p, *D, C, 0, par, None, None, None, None, None, 0, None, 0, None) == 0      # no sums: no workspace
    assert lib.pmu_fusion3_ws(*D, 1) == 0 and lib.pmu_fusion3_ws(*D, 9) == 0 and lib.pmu_fusion3_ws(0, 5, 6, C) == 0
    P, V = 8, 2
    st = torch.zeros(8, P, C, P, P, device=dev)
    fr = torch.from_numpy(np.stack([np.eye(3)] * 8).reshape(8, 9)).to(dev)
    t6 = torch.zeros(6, 6, 6, device=dev)
    oneed = int(lib.pmu_fusion_oblique_ws(V, C, 6, 6, 6))
    fo = lib.pmu_fusion_oblique_eval

    def obl(V_=V, C_=C, par_=par, nbytes=oneed, h=1.0, P_=P, s=st.data_ptr()):
        return fo(s, fr.data_ptr(), V_, C_, P_, h, t6.data_ptr(), 6, 6, 6, par_, None, None, None, None, None,
                  sums.data_ptr(), 0, ws.data_ptr(), nbytes, None)

    assert obl() == 0
    assert obl(V_=9) == E and obl(V_=0) == E and obl(C_=1) == E and obl(C_=9) == E
    assert obl(par_=None) == E and obl(nbytes=oneed - 8) == E and obl(h=0.0) == E and obl(P_=1) == E and obl(s=None) == E
    assert obl(V_=8, nbytes=int(lib.pmu_fusion_oblique_ws(8, C, 6, 6, 6))) == 0
    assert lib.pmu_fusion_oblique_ws(9, C, 6, 6, 6) == 0 and lib.pmu_fusion_oblique_ws(V, 1, 6, 6, 6) == 0
    torch.cuda.synchronize()
    with pytest.raises(RuntimeError):
        L.call("pmu_fusion3_eval", *p, *D, 1, 0, par, None, None, None, None, sums.data_ptr(), 0, ws.data_ptr(), need,
               None)
    # the Python surface
    from pmu_hip.fusion import FusionWeights, fuse_views
    one = [torch.zeros(4, 1, 5, 6, device=dev), torch.zeros(5, 1, 4, 6, device=dev), torch.zeros(6, 1, 4, 5, device=dev)]
    with pytest.raises(ValueError):
        fuse_views(*one, tr, weights=FusionWeights.uniform(3, 1))
    with pytest.raises(ValueError):
        fuse_views(v0, v1, v2, tr, weights=FusionWeights.uniform(3, 4))
    with pytest.raises(ValueError):
        fuse_views(v0, v1, v2, tr, weights=FusionWeights.uniform(3, 3), class_weight=[1.0, 2.0])
