"""pmu_dice_counts and pmu_dice_counts_many (csrc/dice_counts.hip) by direct calls: exact integer counters
against a float64 count on the CPU.  counts[k] = (sum pred_k t_k, sum pred_k, sum t_k), include/pmunet_hip.h.

K > 1: pred = onehot(first argmax of softmax(y)), t_k = (mask == k).  The logits are multiples of 1/4 in
[-4, 4].  The kernel compares p_k = exp(y_k - m) / sum, one fp32 division of the same denominator per
class: equal logits give bit-equal p_k, and a logit at least 1/4 below the maximum gives exp <= e^-1/4 < 0.78
against exactly 1 for the maximum, so the fp32 order of the probabilities is the order of the logits and
the reference is simply the first maximum of the logits.  About a third of the pixels are forced into
ties at the row maximum — two classes, three classes, all K — placed at random classes, so "first maximum"
is decided at every class index and a `>=` in the kernel's argmax (last maximum) changes the counts.  Mask
labels are drawn from {0 .. K-1} and from K, 255, -1 and 0.5, which belong to no class.

K == 1: pred = (y > 0.5), t = mask summed by value.  y holds 0.5 exactly (not above), nextafter(0.5, 1)
(above) and NaN (not above); the mask takes 0, 1 and 2.

The counters are integers below 2^53 added in float64: exact in any order, so equality is exact.  counts is
NaN on entry: the entry zeroes it itself.  Shapes: one pixel; 255 pixels (one partly filled block); 3 x 86
(images narrower than a wave); and 1025 x 1024 = 1,049,600 pixels, past the cap of 512 blocks x 256
threads x 8 pixels = 1,048,576, so the grid-stride loop runs a second, ragged round whose out-of-range
lanes are clamped to the last pixel for their loads and must not be counted."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

NAN = float("nan")
SHAPES = [(1, 1, 1), (1, 15, 17), (3, 1, 86)]
CAPPED = (1, 1025, 1024)
TAIL = -12345.0


def _L():
    from pmu_hip import _lib as L
    return L


def _inputs(N, K, H, W, seed):
    """(y [N][K][H][W] fp32, mask [N][H][W] fp32, counts [K][3] float64) on the CPU."""
    gen = torch.Generator().manual_seed(seed)
    HW = H * W
    P = N * HW
    if K == 1:
        y = torch.rand(P, generator=gen)
        above = float(np.nextafter(np.float32(0.5), np.float32(1.0)))
        y[0::11], y[1::11], y[2::11] = above, 0.5, NAN
        mask = torch.randint(0, 3, (P,), generator=gen).float()
        pr = (y > 0.5).double()
        assert pr[0] == 1 and (P < 3 or (pr[1] == 0 and pr[2] == 0))
        t = mask.double()
        ref = torch.stack([(pr * t).sum(), pr.sum(), t.sum()]).view(1, 3)
        return y.view(N, 1, H, W), mask.view(N, H, W), ref
    yf = torch.randint(-16, 17, (P, K), generator=gen).float() / 4          # [pixel][class]
    top = yf.max(dim=1).values
    r = torch.rand(P, generator=gen)
    order = torch.rand(P, K, generator=gen).argsort(dim=1)                  # random distinct classes per pixel
    for lo, hi, ways in ((0.0, 1 / 9, 2), (1 / 9, 2 / 9, 3), (2 / 9, 1 / 3, K)):
        rows = ((r >= lo) & (r < hi)).nonzero().squeeze(1)
        for j in range(min(ways, K)):
            yf[rows, order[rows, j]] = top[rows]
    am = torch.from_numpy(np.argmax(yf.numpy(), axis=1))                    # numpy: the first maximum
    labels = torch.tensor([float(k) for k in range(K)] + [float(K), 255.0, -1.0, 0.5])
    mask = labels[torch.randint(0, len(labels), (P,), generator=gen)]
    ref = torch.zeros(K, 3, dtype=torch.float64)
    for k in range(K):
        pr, tk = am == k, mask == float(k)
        ref[k] = torch.tensor([float((pr & tk).sum()), float(pr.sum()), float(tk.sum())])
    if P >= 255:        # the ties decide something: the last maximum gives other counts
        last = K - 1 - torch.from_numpy(np.argmax(yf.numpy()[:, ::-1], axis=1))
        assert int((last != am).sum()) > P // 6
    y = yf.view(N, HW, K).permute(0, 2, 1).contiguous().view(N, K, H, W)
    return y, mask.view(N, H, W), ref


def _run_one(dev, N, K, H, W, seed):
    L = _L()
    y, mask, ref = _inputs(N, K, H, W, seed)
    yd, md = y.to(dev), mask.to(dev)
    counts = torch.full((K * 3 + 4,), NAN, dtype=torch.float64, device=dev)
    counts[K * 3:] = TAIL
    L.call("pmu_dice_counts", yd.data_ptr(), md.data_ptr(), N, K, H, W, counts.data_ptr(), L.stream())
    torch.cuda.synchronize()
    got = counts.cpu()
    assert bool((got[K * 3:] == TAIL).all())
    got = got[:K * 3].view(K, 3)
    print(f"dice_counts {(N, K, H, W)}: max |count - ref| = {float((got - ref).abs().max())}")
    assert torch.equal(got, ref), (got - ref)


@pytest.mark.parametrize("K", [1, 2, 5, 8])
@pytest.mark.parametrize("N,H,W", SHAPES)
def test_dice_counts_exact(dev, N, H, W, K):
    _run_one(dev, N, K, H, W, seed=N * H * W + K)


@pytest.mark.parametrize("K", [1, 8])
def test_dice_counts_exact_past_block_cap(dev, K):
    N, H, W = CAPPED
    assert N * H * W > 512 * 256 * 8 and (N * H * W) % (512 * 256) != 0
    _run_one(dev, N, K, H, W, seed=K)


@pytest.mark.parametrize("S,N,K,H,W", [(3, 2, 4, 5, 7), (3, 1, 1, 9, 31), (2,) + CAPPED[:1] + (3,) + CAPPED[1:]])
def test_dice_counts_many_equals_float64_counts_per_sample(dev, S, N, K, H, W):
    L = _L()
    ys, refs, mask = [], [], None
    for s in range(S):
        y, m, _ = _inputs(N, K, H, W, seed=100 + s)
        mask = m if mask is None else mask
        ys.append(y)
    for s in range(S):      # every sample against the one shared mask: recount on the CPU
        yf = ys[s].view(N, K, H * W).permute(0, 2, 1).reshape(N * H * W, K)
        t = mask.reshape(-1)
        ref = torch.zeros(K, 3, dtype=torch.float64)
        if K == 1:
            pr = (yf[:, 0] > 0.5).double()
            ref[0] = torch.stack([(pr * t.double()).sum(), pr.sum(), t.double().sum()])
        else:
            am = torch.from_numpy(np.argmax(yf.numpy(), axis=1))
            for k in range(K):
                pr, tk = am == k, t == float(k)
                ref[k] = torch.tensor([float((pr & tk).sum()), float(pr.sum()), float(tk.sum())])
        refs.append(ref)
    refs = torch.stack(refs)
    assert not torch.equal(refs[0], refs[1])
    yd, md = torch.stack(ys).to(dev), mask.to(dev)
    counts = torch.full((S * K * 3 + 5,), NAN, dtype=torch.float64, device=dev)
    counts[S * K * 3:] = TAIL
    L.call("pmu_dice_counts_many", yd.data_ptr(), md.data_ptr(), S, N, K, H, W, counts.data_ptr(), L.stream())
    torch.cuda.synchronize()
    got = counts.cpu()
    assert bool((got[S * K * 3:] == TAIL).all()), "slots past counts[S][K][3] were written"
    got = got[:S * K * 3].view(S, K, 3)
    print(f"dice_counts_many {(S, N, K, H, W)}: max |count - ref| = {float((got - refs).abs().max())}")
    assert torch.equal(got, refs), (got - refs)


def test_dice_counts_refuse_bad_arguments(dev):
    L = _L()
    lib, s = L.lib(), L.stream()
    y = torch.zeros(9 * 16, device=dev)
    m = torch.zeros(16, device=dev)
    counts = torch.full((64,), NAN, dtype=torch.float64, device=dev)
    assert lib.pmu_dice_counts(y.data_ptr(), m.data_ptr(), 1, 9, 4, 4, counts.data_ptr(), s) == L.PMU_ERR_ARG
    assert lib.pmu_dice_counts(y.data_ptr(), m.data_ptr(), 1, 0, 4, 4, counts.data_ptr(), s) == L.PMU_ERR_ARG
    assert lib.pmu_dice_counts_many(y.data_ptr(), m.data_ptr(), 0, 1, 2, 4, 4, counts.data_ptr(), s) == L.PMU_ERR_ARG
    assert lib.pmu_dice_counts_many(y.data_ptr(), m.data_ptr(), 1, 1, 9, 4, 4, counts.data_ptr(), s) == L.PMU_ERR_ARG
    torch.cuda.synchronize()
    assert torch.isnan(counts).all()
