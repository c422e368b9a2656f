"""Volume evaluation — drop-in for PMU/eval.py (same CLI: -f/--load, -d/--dir, -m/--model).

The reference script does not parse (eval.py:137-138); this is its evident intent, restated:
predict every slice of every test scan along the three standard views, compare each view's
volume and the 3-view average against the ground truth (Dice of classes 1 and 2), and save the
averaged label volume.  Prediction is batched on resident scans and the fusion is one kernel
(predict.predict_volume / pmu_hip.fusion).  --views N evaluates along N seeded oblique views instead
(MRI_Dataset(views=...), fused by pmu_hip.fusion.fuse_oblique).  --surface also scores the fused label volume
with the surface-distance metrics of pmu_hip.surface (HD, HD95, ASSD, surface Dice) under --voxel-size.
--thickness logs the volume and the mean local thickness of every foreground class of the prediction and of the
truth (pmu_hip.thickness, under --voxel-size) and saves the thickness map as <id>_thickness.
--postprocess cleans the fused label volume first (pmu_hip.components.keep_largest: the --keep largest components
of each class with at least --min-voxels voxels, under --connectivity) and logs the Dice of the cleaned volume
and, with --surface, the surface metrics of both; --lesions logs the lesion-wise detection scores.
--fusion FILE fuses the views with a learned fusion model (per-view, per-class weights, pmu_hip.fusion) instead
of their plain mean; --fit-fusion DIR fits that model first on the scans under DIR (and writes it to --fusion).
"""
import argparse
import logging
import os

import numpy as np
import torch

from pmu_hip.fusion import VOLUMES, oblique_volumes
from predict import predict_volume
from trainer import ProbUNetTrainer, UNetTrainer
from utils.mri_dataset import MRI_Dataset, draw_views


def get_args(argv=None):
    parser = argparse.ArgumentParser(description="Predict using a trained UNet",
                                     formatter_class=argparse.ArgumentDefaultsHelpFormatter)
    parser.add_argument("-f", "--load", dest="load", type=str, default=None, help="Load model from a .pth file")
    parser.add_argument("-d", "--dir", dest="dir", type=str, default=None, help="image and label superdirs.")
    parser.add_argument("-m", "--model", dest="net", type=str, default="unet", help="what model to use: unet or probunet")
    parser.add_argument("-o", "--out", dest="out", type=str, default="predictions", help="output directory")
    parser.add_argument("-b", "--batch-size", dest="batch", type=int, default=32, help="slices per launch")
    parser.add_argument("--views", dest="views", type=int, default=0,
                        help="evaluate along this many seeded oblique views instead of the three standard axes")
    parser.add_argument("--view-seed", dest="view_seed", type=int, default=0, help="seed of the oblique views")
    parser.add_argument("--sample-dim", dest="sample_dim", type=int, default=None,
                        help="oblique views: edge P of the P x P slices (default: the largest padded dim)")
    parser.add_argument("--uncertainty", dest="uncertainty", action="store_true",
                        help="probunet: also save the fused predictive-entropy and mutual-information volumes "
                             "(<id>_entropy, <id>_mutual_info) next to the label volume")
    parser.add_argument("--surface", dest="surface", action="store_true",
                        help="also log the surface-distance metrics of the fused label volume per class: "
                             "Hausdorff distance, its 95th percentile, average symmetric surface distance and "
                             "surface Dice (pmu_hip.surface)")
    parser.add_argument("--voxel-size", dest="voxel_size", type=float, nargs=3, default=[1.0, 1.0, 1.0],
                        metavar=("A", "B", "C"),
                        help="--surface / --thickness: voxel edge along the three volume axes (e.g. mm)")
    parser.add_argument("--surface-tolerance", dest="surface_tolerance", type=float, default=1.0, metavar="MM",
                        help="--surface: tolerance of the surface Dice, in the unit of --voxel-size")
    parser.add_argument("--postprocess", dest="postprocess", action="store_true",
                        help="clean the fused label volume before it is scored and saved: keep the --keep largest "
                             "connected components of each class that have at least --min-voxels voxels "
                             "(pmu_hip.components); logs the Dice of the cleaned volume beside the raw one")
    parser.add_argument("--keep", dest="keep", type=int, default=1, metavar="N",
                        help="--postprocess: components kept per class (0: every one that passes --min-voxels)")
    parser.add_argument("--min-voxels", dest="min_voxels", type=int, default=1, metavar="N",
                        help="--postprocess / --lesions: components below this many voxels are dropped")
    parser.add_argument("--connectivity", dest="connectivity", type=int, default=26, choices=(6, 18, 26),
                        help="--postprocess / --lesions: voxel adjacency (faces; faces and edges; and corners)")
    parser.add_argument("--lesions", dest="lesions", action="store_true",
                        help="also log the lesion-wise detection scores per class: components found, missed and "
                             "spurious, sensitivity, precision and F1 (pmu_hip.components.lesion_metrics)")
    parser.add_argument("--thickness", dest="thickness", action="store_true",
                        help="also log, per class, the volume and the mean local thickness of the fused label volume "
                             "and of the truth with their absolute differences, in the unit of --voxel-size, and "
                             "save the thickness map (<id>_thickness) next to the label volume "
                             "(pmu_hip.thickness)")
    parser.add_argument("--fusion", dest="fusion", type=str, default=None, metavar="FILE",
                        help="fuse the views with the learned fusion model in FILE (an .npz of per-view, per-class "
                             "weights W and per-class biases b, pmu_hip.fusion.FusionWeights) instead of their plain "
                             "mean; with --fit-fusion: where the fitted model is written")
    parser.add_argument("--fit-fusion", dest="fit_fusion", type=str, default=None, metavar="DIR",
                        help="first fit the fusion model on the scans under DIR/images and DIR/labels (held-out "
                             "scans, predicted with the same network and views), then evaluate with it")
    return parser.parse_args(argv)


def fusion_weights(args, net, views):
    """The FusionWeights of --fusion / --fit-fusion, or None: fitted on the scans of --fit-fusion (and saved to
    --fusion when given), else loaded from --fusion.  Logs the model and, for a fit, the loss before and after."""
    from pmu_hip.fusion import FusionWeights
    from predict import fit_fusion_model
    if args.fit_fusion:
        fit_set = MRI_Dataset(os.path.join(args.fit_fusion, "images"), os.path.join(args.fit_fusion, "labels"),
                              net.n_classes, filter=False, views=views, sample_dim=args.sample_dim)
        # the fitting scans are predicted exactly as the evaluation below predicts: with --uncertainty the stacks
        # are the mean probabilities of the prior samples, else the network's logits
        mode = dict(prob=True, faithful=False, uncertainty=True) if args.uncertainty else \
            dict(prob=(args.net == "probunet"))
        fit = fit_fusion_model(net, fit_set, range(len(fit_set.ids)), batch_size=args.batch, **mode)
        weights = fit.weights
        logging.info(f"learned fusion: fitted on {len(fit_set.ids)} scans, loss {fit.loss_initial:.6f} -> {fit.loss:.6f} "
                     f"in {fit.iterations} iterations ({fit.evaluations} evaluations), |g|inf {fit.grad_norm:.2e}, "
                     f"converged {fit.converged}")
        if args.fusion:
            weights.save(args.fusion)
    elif args.fusion:
        weights = FusionWeights.load(args.fusion)
    else:
        return None
    logging.info(f"learned fusion: W (views x classes)\n{weights.W}\nb {weights.b}")
    return weights


SURFACE_METRICS = ("hd", "hd95", "assd", "nsd")


def surface_summary(per_scan):
    """Log lines of the fused volume's surface metrics: per class, mean and standard deviation over the scans
    that have both surfaces (a scan where the class is absent from the prediction or the truth is NaN and
    skipped: nanmean / nanstd; a class absent everywhere stays NaN).  per_scan: metric -> list of per-scan
    (K-1,) arrays."""
    import warnings
    lines = []
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)   # all-NaN column: the NaN is the answer
        for k in SURFACE_METRICS:
            v = np.array(per_scan[k], dtype=np.float64)
            lines.append(f"average: {k} mean {np.nanmean(v, 0)} std {np.nanstd(v, 0)}")
    return lines


LESION_METRICS = ("n_pred", "n_truth", "tp", "fn", "fp", "sensitivity", "precision", "f1")


def nan_mean_lines(per_scan, keys, prefix):
    """Log lines of per-class means over the scans: a NaN scan (a ratio without a denominator, a class without a
    surface) is left out of its mean and counted, as in surface_summary.  per_scan: key -> list of per-scan
    (K-1,) arrays."""
    import warnings
    lines = []
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)   # all-NaN column: the NaN is the answer
        for k in keys:
            v = np.array(per_scan[k], dtype=np.float64)
            lines.append(f"{prefix}: {k} mean {np.nanmean(v, 0)} scans left out {np.isnan(v).sum(0)}")
    return lines


THICKNESS_KEYS = ("volume", "mean")


def thickness_summary(per_scan):
    """Log lines of --thickness: per class, mean and standard deviation over the scans of the predicted and the
    true volume and mean thickness and of their absolute difference.  A NaN scan (the class is absent: it has
    no thickness) is left out and counted, as in nan_mean_lines.  per_scan: 'pred' / 'truth' -> key -> list of
    per-scan (K-1,) arrays."""
    import warnings
    lines = []
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)   # all-NaN column: the NaN is the answer
        for k in THICKNESS_KEYS:
            a = np.array(per_scan["pred"][k], dtype=np.float64)
            b = np.array(per_scan["truth"][k], dtype=np.float64)
            for name, v in (("pred", a), ("truth", b), ("abs diff", np.abs(a - b))):
                lines.append(f"thickness: {k} {name} mean {np.nanmean(v, 0)} std {np.nanstd(v, 0)} "
                             f"scans left out {np.isnan(v).sum(0)}")
    return lines


def save_label(label, title):
    arr = label.cpu().numpy().astype(np.float32)
    try:
        import nibabel as nib
        nib.save(nib.Nifti1Image(arr, affine=np.eye(4)), title)
    except ImportError:
        np.save(title + ".npy", arr)


def main():
    logging.basicConfig(level=logging.INFO, format="%(levelname)s: %(message)s")
    args = get_args()
    device = torch.device("cuda")
    if args.net == "unet":
        train = UNetTrainer(device, n_channels=1, n_classes=3, load_model=args.load)
    elif args.net == "probunet":
        train = ProbUNetTrainer(device, n_channels=1, n_classes=3, load_model=args.load, latent_dim=6, beta=10)
    else:
        raise SystemExit(f"Error! {args.net} is not a valid model")
    dir_img = os.path.join(args.dir, "images") if args.dir else "data/test/images"
    dir_mask = os.path.join(args.dir, "labels") if args.dir else "data/test/labels"
    views = draw_views(args.views, args.view_seed) if args.views else None
    dataset = MRI_Dataset(dir_img, dir_mask, train.net.n_classes, filter=False, views=views,
                          sample_dim=args.sample_dim)
    os.makedirs(args.out, exist_ok=True)
    per_volume = {k: [] for k in (oblique_volumes(args.views) if views else VOLUMES)}
    if args.uncertainty and args.net != "probunet":
        raise SystemExit("Error! --uncertainty needs -m probunet")
    surf = dict(surface=True, voxel_size=tuple(args.voxel_size), surface_tolerance=args.surface_tolerance) \
        if args.surface else {}
    per_surface = {k: [] for k in SURFACE_METRICS}
    if args.keep < 0 or args.min_voxels < 1:
        raise SystemExit("Error! --keep must be >= 0 and --min-voxels >= 1")
    fusion = fusion_weights(args, train.net, views)          # (after the refusals above: a fit is not cheap)
    if fusion is not None:
        try:
            fusion.check_frames(dataset.frames if views else None)
        except ValueError as e:
            raise SystemExit(f"Error! --fusion {args.fusion}: {e}")
    post = {}
    if args.postprocess:
        post["postprocess"] = dict(keep=args.keep or None, min_voxels=args.min_voxels, connectivity=args.connectivity)
    if args.lesions:
        post["lesions"] = dict(min_voxels=args.min_voxels, connectivity=args.connectivity)
    per_surface_raw = {k: [] for k in SURFACE_METRICS}
    per_lesion = {k: [] for k in LESION_METRICS}
    thick = dict(thickness=True, voxel_size=tuple(args.voxel_size)) if args.thickness else {}
    extra = {**surf, **thick, **post}                         # (--surface and --thickness share --voxel-size)
    if fusion is not None:
        extra["fusion"] = fusion
    per_thickness = {w: {k: [] for k in THICKNESS_KEYS} for w in ("pred", "truth")}
    dice_pp = []
    for scan in range(len(dataset.ids)):
        if args.uncertainty:
            res = predict_volume(train.net, dataset, scan, batch_size=args.batch, prob=True, faithful=False,
                                 uncertainty=True, **extra)
        else:
            res = predict_volume(train.net, dataset, scan, batch_size=args.batch, prob=(args.net == "probunet"),
                                 **extra)
        if args.surface:
            for k in SURFACE_METRICS:
                per_surface[k].append(res["surface"][k].cpu().numpy())
                if args.postprocess:
                    per_surface_raw[k].append(res["surface_raw"][k].cpu().numpy())
        if args.postprocess:
            dice_pp.append(res["dice_pp"].cpu().numpy()[1:3])
        if args.lesions:
            for k in LESION_METRICS:
                per_lesion[k].append(res["lesions"][k].cpu().numpy())
        if args.thickness:
            for w in ("pred", "truth"):
                for k in THICKNESS_KEYS:
                    per_thickness[w][k].append(res["thickness"][w][k].cpu().numpy())
        d = res["dice"].cpu().numpy()
        for i, k in enumerate(per_volume):
            per_volume[k].append(d[i, 1:3])
        save_label(res["label_pp"] if args.postprocess else res["label"], os.path.join(args.out, dataset.ids[scan]))
        stem, dot, ext = dataset.ids[scan].partition(".")       # scan0.nii.gz -> scan0_entropy.nii.gz
        if args.uncertainty:
            for k in ("entropy", "mutual_info"):
                save_label(res[k], os.path.join(args.out, f"{stem}_{k}{dot}{ext}"))
        if args.thickness:
            save_label(res["thickness"]["map"], os.path.join(args.out, f"{stem}_thickness{dot}{ext}"))
    for k, v in per_volume.items():
        v = np.array(v)
        name = "learned fusion" if fusion is not None and k == "average" else k
        logging.info(f"{name}: dice mean {v.mean(0)} std {v.std(0)}")
    if args.postprocess:
        v = np.array(dice_pp)
        logging.info(f"average, cleaned: dice mean {v.mean(0)} std {v.std(0)}")
    if args.surface:
        for line in surface_summary(per_surface):
            logging.info(line)
        if args.postprocess:
            for line in nan_mean_lines(per_surface_raw, SURFACE_METRICS, "average, before the clean-up"):
                logging.info(line)
    if args.lesions:
        for line in nan_mean_lines(per_lesion, LESION_METRICS, "lesions"):
            logging.info(line)
    if args.thickness:
        for line in thickness_summary(per_thickness):
            logging.info(line)


if __name__ == "__main__":
    main()
