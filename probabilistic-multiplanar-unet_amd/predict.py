"""Prediction — drop-in for PMU/predict.py:15-19, plus the volume prediction of eval.py:131-203.

``predict(net, imgs, masks, train=True, prob=False)`` keeps the reference signature (for the
probabilistic net: forward, then one prior sample) and returns the prediction (the reference's
body stops before returning it).

``predict_volume`` runs a network over every slice of every view of one resident scan in batches
(the reference feeds eval.py one slice at a time through a DataLoader) and fuses the three views
with one kernel (pmu_hip.fusion): per-view and averaged Dice, the averaged probability volume and
its argmax label map.  A dataset with oblique views (MRI_Dataset(views=...)) is predicted along each
of its views and fused by pmu_hip.fusion.fuse_oblique.  ``fusion`` (a pmu_hip.fusion.FusionWeights) replaces the plain
mean of the views by the learned fusion model; ``fit_fusion_model`` fits one on held-out scans.
"""
from __future__ import annotations

import torch

from pmu_hip.fusion import FusionItem, fit_fusion, fuse_oblique, fuse_views


def predict(net, imgs, masks, train=True, prob=False):
    if prob:
        net.forward(imgs, masks, training=train)
        return net.sample(testing=(not train))
    return net(imgs)


def _predict_slices(net, b, prob, n_samples, faithful):
    """The network's output for one get_slices batch (see predict_volume for ``faithful``)."""
    if prob:
        net.forward(b["image"], b["mask"], training=False)
        if faithful:
            return net.sample(testing=True) / n_samples
        return net.sample_many(n_samples).mean(0)
    return net(b["image"])


def _predict_volume_uncertainty(net, dataset, scan, batch_size, n_samples, fusion=None, stacks_only=False):
    """predict_volume(uncertainty=True): every slice batch goes through ProbabilisticUnet.sample_stats, so a
    view's stack holds the mean class probabilities of ``n_samples`` prior samples and two more one-channel
    stacks hold the predictive entropy and the mutual information.  The probability stacks are fused as
    usual (logits=False); the two maps are fused by the same kernels as C = 1 stacks, of which only the
    average over the views is kept.  ``fusion`` applies to the probability stacks only: the two maps keep the plain
    mean.  ``stacks_only``: nothing is fused; returns (the probability stacks, truth, logits=False)."""
    from utils.mri_dataset import view_slice_shape
    sv = dataset.scans[scan]
    C = net.n_classes
    dev = dataset.device
    names = ("entropy", "mutual_info")

    def run(keys, out, maps, s0):
        b = dataset.get_slices(keys)
        net.forward(b["image"], b["mask"], training=False)
        st = net.sample_stats(n_samples)
        out[s0:s0 + len(keys)] = st["mean"]
        for k in names:
            maps[k][s0:s0 + len(keys), 0] = st[k]

    if dataset.oblique:
        P, V = dataset.sample_dim, len(dataset.views)
        out = torch.empty(V, P, C, P, P, dtype=torch.float32, device=dev)
        maps = {k: torch.empty(V, P, 1, P, P, dtype=torch.float32, device=dev) for k in names}
        for v in range(V):
            for s0 in range(0, P, batch_size):
                keys = [(scan, v, s) for s in range(s0, min(P, s0 + batch_size))]
                run(keys, out[v], {k: maps[k][v] for k in names}, s0)
        truth = sv.mask.view(sv.pshape).float()
        if stacks_only:
            return out, truth, False
        res = fuse_oblique(out, dataset.frames, truth, P, dataset.spacing, weights=fusion)
        res["stacks"] = list(out)
        for k in names:
            res[k] = fuse_oblique(maps[k], dataset.frames, truth, P, dataset.spacing, want_label=False)["avg"][:, 0]
            res[k + "_stacks"] = [m[:, 0] for m in maps[k]]
        res["truth"] = truth
        return res
    stacks, mstacks = [], {k: [] for k in names}
    for v in range(3):
        n = sv.pshape[v]
        ha, hb = view_slice_shape(sv.pshape, v)
        out = torch.empty(n, C, ha, hb, dtype=torch.float32, device=dev)
        maps = {k: torch.empty(n, 1, ha, hb, dtype=torch.float32, device=dev) for k in names}
        for s0 in range(0, n, batch_size):
            run([(scan, v, s) for s in range(s0, min(n, s0 + batch_size))], out, maps, s0)
        stacks.append(out)
        for k in names:
            mstacks[k].append(maps[k])
    truth = dataset.get_slices([(scan, 0, s) for s in range(sv.pshape[0])])["mask"][:, 0]
    if stacks_only:
        return stacks, truth, False
    res = fuse_views(stacks[0], stacks[1], stacks[2], truth, logits=False, weights=fusion)
    res["stacks"] = stacks
    for k in names:
        m = mstacks[k]
        res[k] = fuse_views(m[0], m[1], m[2], truth, logits=False, want_label=False)["avg"][:, 0]
        res[k + "_stacks"] = [t[:, 0] for t in m]
    res["truth"] = truth
    return res


@torch.no_grad()
def predict_volume(net, dataset, scan, batch_size=32, prob=False, n_samples=5, faithful=True, uncertainty=False,
                   surface=False, voxel_size=(1.0, 1.0, 1.0), surface_tolerance=1.0, postprocess=None, lesions=False,
                   thickness=False, fusion=None):
    """Predict all slices of ``scan`` along the three views and fuse them.

    ``prob``: net is a ProbabilisticUnet; eval.py averages ``n_samples`` prior samples but, as
    written (:148-154), keeps only the first sample divided by n_samples — ``faithful`` reproduces
    that, otherwise the mean of the samples is used.  Returns fuse_views' dict plus the stacks.

    With oblique views every view's stack is (P,C,P,P) probabilities (the softmax over C > 1 classes is
    applied per batch as the stack is written) and the result is fuse_oblique's dict plus the stacks.

    ``uncertainty`` (needs prob=True, faithful=False): the stacks hold the mean class probabilities of the
    ``n_samples`` samples (ProbabilisticUnet.sample_stats; not the softmax of the mean logits), and the
    result gains 'entropy' and 'mutual_info', the predictive entropy and the mutual information fused over
    the views on the voxel grid, with their per-view stacks 'entropy_stacks' and 'mutual_info_stacks'.

    ``surface``: the result gains 'surface', pmu_hip.surface.surface_distances of the fused label volume against
    the truth on the padded grid (the grid of the Dice counts) — HD, HD95, ASSD and surface Dice at
    ``surface_tolerance`` per foreground class, in the unit of ``voxel_size`` (the voxel edge along each axis of
    that grid).  Nothing else changes, and without it nothing of this runs.

    ``postprocess``: a dict of pmu_hip.components.keep_largest's keyword arguments ({}: its defaults — the largest
    26-connected component of each class).  The result gains 'label_pp', the cleaned label volume (int32 like
    'label'), and 'dice_pp', its (C,) float32 Dice against 'truth' with the arithmetic and the class convention of
    the average row of 'dice'; 'surface' is then scored on the cleaned volume and 'surface_raw' on 'label'.
    ``lesions``: the result gains 'lesions', pmu_hip.components.lesion_metrics of the cleaned volume if there is
    one, else of 'label', against 'truth' (True: its defaults; a dict: its keyword arguments).
    Without either nothing of this runs and the result is unchanged.

    ``thickness``: the result gains 'thickness', the local thickness and volume of every foreground class under
    ``voxel_size`` (pmu_hip.thickness.local_thickness): 'map', the thickness map of the volume that is scored
    ('label_pp' with ``postprocess``, else 'label'), 'pred', that volume's per-class 'n', 'volume', 'mean', 'std',
    'median', 'max', and 'truth', the same of 'truth'.  Without it nothing of this runs and no key is added.

    ``fusion``: a pmu_hip.fusion.FusionWeights (n_classes >= 2; for oblique views: fitted for the dataset's frames).
    The views are fused by the learned model instead of their plain mean: 'avg' holds the fused softmax, 'label' its
    first maximum, the last row of 'counts' / 'dice' scores it, and the result gains 'loss' (fuse_views).
    With ``uncertainty`` the weights apply to the mean-probability stacks only; the entropy and mutual-information
    maps keep the plain mean.  None: the plain mean, exactly as before."""
    res = _predict_volume(net, dataset, scan, batch_size, prob, n_samples, faithful, uncertainty, fusion)
    C = net.n_classes
    scored = res["label"]
    if postprocess is not None:
        from pmu_hip.components import keep_largest
        from pmu_hip.metrics import dice_from_counts
        from pmu_hip.uncertainty import label_pair_counts
        clean = keep_largest(res["label"], C, **postprocess)
        inter, cnt = label_pair_counts(torch.stack((clean, res["truth"].to(torch.uint8)))[:, None], C)
        res["label_pp"] = scored = clean.to(torch.int32)
        res["dice_pp"] = dice_from_counts(torch.stack((inter[0, 0, 1], cnt[0, 0], cnt[0, 1]), 1))
    if surface:
        from pmu_hip.surface import surface_distances
        res["surface"] = surface_distances(scored, res["truth"], C, spacing=voxel_size, tolerance=surface_tolerance)
        if postprocess is not None:
            res["surface_raw"] = surface_distances(res["label"], res["truth"], C, spacing=voxel_size,
                                                   tolerance=surface_tolerance)
    if lesions or isinstance(lesions, dict):
        from pmu_hip.components import lesion_metrics
        res["lesions"] = lesion_metrics(scored, res["truth"], C, **(lesions if isinstance(lesions, dict) else {}))
    if thickness:
        from pmu_hip.thickness import local_thickness
        pred = local_thickness(scored, C, spacing=voxel_size)
        truth = local_thickness(res["truth"], C, spacing=voxel_size)
        truth.pop("map")
        res["thickness"] = {"map": pred.pop("map"), "pred": pred, "truth": truth}
    return res


def _predict_volume(net, dataset, scan, batch_size, prob, n_samples, faithful, uncertainty, fusion=None,
                    stacks_only=False):
    """predict_volume without its optional scores.  ``stacks_only``: the views are predicted and nothing is fused;
    returns (stacks, truth, logits) — the three stacks, or the (V,P,C,P,P) buffer of an oblique dataset, and whether
    they hold logits (what fuse_views is told)."""
    from utils.mri_dataset import view_slice_shape
    net.eval()
    if uncertainty:
        if not prob or faithful:
            raise ValueError("predict_volume(uncertainty=True) needs prob=True and faithful=False: the maps are "
                             "statistics over the prior samples of a ProbabilisticUnet")
        return _predict_volume_uncertainty(net, dataset, scan, batch_size, n_samples, fusion, stacks_only)
    sv = dataset.scans[scan]
    C = net.n_classes
    if dataset.oblique:
        P, V = dataset.sample_dim, len(dataset.views)
        out = torch.empty(V, P, C, P, P, dtype=torch.float32, device=dataset.device)
        for v in range(V):
            for s0 in range(0, P, batch_size):
                keys = [(scan, v, s) for s in range(s0, min(P, s0 + batch_size))]
                y = _predict_slices(net, dataset.get_slices(keys), prob, n_samples, faithful)
                out[v, s0:s0 + len(keys)] = torch.softmax(y.float(), 1) if C > 1 else y
        truth = sv.mask.view(sv.pshape).float()
        if stacks_only:
            return out, truth, False
        res = fuse_oblique(out, dataset.frames, truth, P, dataset.spacing, weights=fusion)
        res["stacks"] = list(out)
        res["truth"] = truth
        return res
    stacks = []
    for v in range(3):
        n = sv.pshape[v]
        ha, hb = view_slice_shape(sv.pshape, v)
        out = torch.empty(n, C, ha, hb, dtype=torch.float32, device=dataset.device)
        for s0 in range(0, n, batch_size):
            keys = [(scan, v, s) for s in range(s0, min(n, s0 + batch_size))]
            out[s0:s0 + len(keys)] = _predict_slices(net, dataset.get_slices(keys), prob, n_samples, faithful)
        stacks.append(out)
    truth = dataset.get_slices([(scan, 0, s) for s in range(sv.pshape[0])])["mask"][:, 0]
    if stacks_only:
        return stacks, truth, C > 1
    res = fuse_views(stacks[0], stacks[1], stacks[2], truth, logits=(C > 1), weights=fusion)
    res["stacks"] = stacks
    res["truth"] = truth
    return res


@torch.no_grad()
def fit_fusion_model(net, dataset, scans, batch_size=32, prob=False, n_samples=5, faithful=True, uncertainty=False,
                     **fit_kwargs):
    """Fit the learned fusion model (pmu_hip.fusion.fit_fusion) on the scans ``scans`` of ``dataset``: each is
    predicted as predict_volume predicts it under the same ``prob``, ``n_samples``, ``faithful`` and ``uncertainty``
    (so the model is fitted on the kind of stacks it will be applied to: logits, or with ``uncertainty`` the mean
    probabilities of the prior samples), only its per-view stacks and truth stay resident (no view is fused, no
    stack copied), and the fit runs over all of them (one kernel pass per scan per function evaluation).
    ``fit_kwargs``: fit_fusion's (class_weight, l2, gtol, max_iter, init).  Returns its FusionFit; the weights of an
    oblique dataset carry its frames."""
    if net.n_classes < 2:
        raise ValueError("the learned fusion is a softmax over the classes: it needs n_classes >= 2")
    items = []
    for scan in scans:
        stacks, truth, logits = _predict_volume(net, dataset, scan, batch_size, prob, n_samples, faithful, uncertainty,
                                                stacks_only=True)
        if dataset.oblique:
            items.append(FusionItem(stacks, truth, frames=dataset.frames, sample_dim=dataset.sample_dim,
                                    spacing=dataset.spacing))
        else:
            items.append(FusionItem(stacks, truth, logits=logits))
    return fit_fusion(items, **fit_kwargs)
