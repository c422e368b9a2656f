"""ProbabilisticUnet.sample_stats and predict_volume(uncertainty=True) at model level, on a small
Probabilistic U-Net (3 classes, filters [8, 16], 16 x 16 inputs, batch 2).

sample_stats against the torch float64 evaluation of sample_many's logits after the same seed (which shows
that the two draw the same z), with the tolerances of tests/test_fcomb_stats_gpu.py: t_y = 1e-4 max(1, max|y|),
mean 0.5 t_y + 1e-6, entropy 2 ln K t_y + 1e-5, mutual information twice that; the per-sample labels where
the top two logits differ by more than 2 t_y.  predict_volume(uncertainty=True) on a synthetic resident scan
(built as in tests/test_eval_gpu.py): the fused entropy and mutual-information volumes against the
transposed average of their per-view stacks computed in torch, within 1e-6 (one fp32 sum of three values
below ln 3 and a division)."""
import math
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

K = 3


def _net(dev):
    from model import ProbabilisticUnet
    torch.manual_seed(0)
    return ProbabilisticUnet(1, K, [8, 16], latent_dim=6, no_convs_fcomb=4).to(dev).eval()


def _stats64(y):
    p = torch.softmax(y.double(), 2)
    xlogx = lambda q: torch.where(q > 0, q * torch.log(q.clamp_min(1e-300)), torch.zeros_like(q))
    mean = p.mean(0)
    ent = -xlogx(mean).sum(1)
    mi = (ent + xlogx(p).sum(2).mean(0)).clamp_min(0)
    return mean, ent, mi


def _check(st, y):
    mean, ent, mi = _stats64(y)
    t_y = 1e-4 * max(1.0, float(y.abs().max()))
    tol_ent = 2 * math.log(K) * t_y + 1e-5
    for name, got, want, tol in (("mean", st["mean"], mean, 0.5 * t_y + 1e-6), ("entropy", st["entropy"], ent, tol_ent),
                                 ("mutual_info", st["mutual_info"], mi, 2 * tol_ent)):
        assert got.shape == want.shape and got.dtype == torch.float32, name
        e = float((got.double() - want).abs().max())
        print(f"sample_stats {name}: err {e:.3e} tol {tol:.3e}")
        assert e <= tol, (name, e, tol)
    top = mean.topk(2, dim=1).values
    keep = (top[:, 0] - top[:, 1]) > t_y
    assert float(keep.float().mean()) >= 0.9
    assert st["label"].dtype == torch.int32
    assert torch.equal(st["label"][keep].long(), mean.argmax(1)[keep])
    return t_y


def test_sample_stats_draws_like_sample_many(dev):
    net = _net(dev)
    g = torch.Generator().manual_seed(1)
    x = torch.rand(2, 1, 16, 16, generator=g).to(dev)
    with torch.no_grad():
        net.forward(x, None, training=False)
        torch.manual_seed(5)
        y = net.sample_many(8)
        torch.manual_seed(5)
        st = net.sample_stats(8, labels=True)
        torch.manual_seed(5)
        st2 = net.sample_stats(8)
    torch.cuda.synchronize()
    assert tuple(y.shape) == (8, 2, K, 16, 16)
    assert set(st) == {"mean", "entropy", "mutual_info", "label", "labels"} and set(st2) == set(st) - {"labels"}
    # the samples differ (another draw would not pass the mean tolerance below)
    assert float((torch.softmax(y, 2)[0] - torch.softmax(y, 2)[1]).abs().max()) > 1e-3
    t_y = _check(st, y)
    assert torch.equal(st2["mean"], st["mean"]) and torch.equal(st2["mutual_info"], st["mutual_info"])
    top = y.topk(2, dim=2).values
    keep = (top[:, :, 0] - top[:, :, 1]) > 2 * t_y
    assert st["labels"].dtype == torch.uint8 and tuple(st["labels"].shape) == (8, 2, 16, 16)
    assert float(keep.float().mean()) >= 0.9
    assert torch.equal(st["labels"][keep].long(), y.argmax(2)[keep])


def test_sample_stats_honours_zs(dev):
    net = _net(dev)
    g = torch.Generator().manual_seed(2)
    x = torch.rand(2, 1, 16, 16, generator=g).to(dev)
    zs = torch.randn(4, 2, 6, generator=g)
    with torch.no_grad():
        net.forward(x, None, training=False)
        y = net.fcomb.forward_samples(net.unet_features, zs.to(dev))
        st = net.sample_stats(4, zs=zs)               # a CPU tensor is moved to the features' device
        other = net.sample_stats(4, zs=(zs + 1.0).to(dev))
    torch.cuda.synchronize()
    _check(st, y)
    assert float((other["mean"] - st["mean"]).abs().max()) > 1e-4


def _scan(shape, seed):
    """One synthetic scan, as tests/test_eval_gpu.py builds them."""
    g = np.random.default_rng(seed)
    img = g.random(shape) * 100.0
    ii, jj, kk = np.meshgrid(*[np.arange(d) for d in shape], indexing="ij")
    r2 = (ii - shape[0] / 2) ** 2 + (jj - shape[1] / 2) ** 2 + (kk - shape[2] / 2) ** 2
    lab = np.zeros(shape)
    lab[r2 < (min(shape) / 3) ** 2] = 1.0
    lab[r2 < (min(shape) / 6) ** 2] = 2.0
    return {"scan0.nii": (img, lab)}


def test_predict_volume_uncertainty(dev):
    from predict import predict_volume
    from utils.mri_dataset import MRI_Dataset
    scans = _scan((16, 12, 16), 5)
    ds = MRI_Dataset("/imgs", "/labs", 3, filter=True, files=sorted(scans),
                     loader=lambda p: scans[os.path.basename(p)][0 if "imgs" in p else 1], device=dev)
    net = _net(dev)
    res = predict_volume(net, ds, 0, batch_size=6, prob=True, n_samples=3, faithful=False, uncertainty=True)
    plain = predict_volume(net, ds, 0, batch_size=6, prob=True, n_samples=3, faithful=False)
    torch.cuda.synchronize()
    assert set(plain) == {"avg", "label", "counts", "dice", "stacks", "truth"}
    assert set(res) == set(plain) | {"entropy", "mutual_info", "entropy_stacks", "mutual_info_stacks"}
    grid = tuple(res["truth"].shape)
    D0, D1, D2 = grid
    assert tuple(res["label"].shape) == grid and tuple(res["avg"].shape) == (D0, K, D1, D2)
    for s in res["stacks"]:                            # mean class probabilities
        assert float((s.sum(1) - 1).abs().max()) <= 1e-5 and float(s.min()) >= 0
    for k in ("entropy", "mutual_info"):
        s0, s1, s2 = res[k + "_stacks"]
        assert tuple(s0.shape) == grid and tuple(s1.shape) == (D1, D0, D2) and tuple(s2.shape) == (D2, D0, D1)
        want = (s0.double() + s1.double().permute(1, 0, 2) + s2.double().permute(1, 2, 0)) / 3
        assert tuple(res[k].shape) == grid and res[k].dtype == torch.float32
        assert float((res[k].double() - want).abs().max()) <= 1e-6
        assert float(res[k].min()) >= 0 and float(res[k].max()) <= math.log(K) + 1e-5
    assert float(res["entropy"].max()) > 0.1           # (not a volume of zeros)
    assert float((res["entropy"] - res["mutual_info"]).min()) >= -1e-5   # I <= H
    for kwargs in (dict(prob=True), dict(prob=True, faithful=True), dict(prob=False, faithful=False)):
        with pytest.raises(ValueError):
            predict_volume(net, ds, 0, uncertainty=True, **kwargs)
