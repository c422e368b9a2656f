#!/usr/bin/env python3
"""Timing and peak memory of the fused sample statistics and of the GED counts beside the torch code
they replace, at the benchmark's c4 Fcomb shape (F = 32, three hidden layers, K = 3, S = 16 samples of N = 32
images of 256 x 256) and at R = 17 label maps of those images:

    fused    pmu_hip.prob_engine.fcomb_stats (pmu_fcomb_zbias + pmu_fcomb_stats): mean, entropy, mutual
             information, label and the S per-sample label maps, no logits stored
    torch    the same five outputs from pmu_fcomb_fwd's (S,N,K,H,W) logits: softmax, mean, the two entropies
             (torch.xlogy), clamp, argmax of the mean and of every sample
    counts   pmu_hip.uncertainty.label_pair_counts        vs  one-hot (fp32: the counts stay below 2^24) and
             einsum('inpc,jnpc->nijc')

    python tools/kbench_uncertainty.py [--samples 16] [--batch 32] [--size 256] [--maps 17] [--repeats 3]

Method: device events around windows of calls (allocations of the outputs included: the caching allocator
serves them after the warm-up), every path warmed up first, the two paths of a pair timed alternately
--repeats times in one process, median and min..max printed.  Peak memory is torch's max_memory_allocated
over one call above what is allocated on entry (inputs and weights).  The two paths' outputs are compared
first: a path that computed something else is not a comparison.  A run without a GPU fails."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "probabilistic-multiplanar-unet_amd"))


def window(fn, n):
    import torch
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(n):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e3 / n    # microseconds per call


def peak_above_entry(fn):
    import torch
    torch.cuda.synchronize()
    base = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    out = fn()
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated() - base
    del out
    return peak


def pair(name, fns, launches, repeats):
    for fn in fns.values():
        window(fn, 2)
    times = {k: [] for k in fns}
    for _ in range(repeats):
        for k, fn in fns.items():
            times[k].append(window(fn, launches[k]))
    rows = []
    for k, fn in fns.items():
        rows.append({"pair": name, "path": k, "us": statistics.median(times[k]), "us_min": min(times[k]),
                     "us_max": max(times[k]), "launches": launches[k], "peak_bytes": peak_above_entry(fn)})
    return rows


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--samples", type=int, default=16)
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--size", type=int, default=256)
    ap.add_argument("--maps", type=int, default=17, help="label maps R of the counts pair (samples + truths)")
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--json", default=None, help="also write the rows to this file")
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        sys.exit("kbench_uncertainty.py times kernels on the GPU; there is none here (no CPU fallback)")
    from model.probabilistic_unet.probabilistic_unet import Fcomb
    from pmu_hip import prob_engine
    from pmu_hip.uncertainty import label_pair_counts
    dev = torch.device("cuda")
    S, N, H, K, F, Lz, R = args.samples, args.batch, args.size, 3, 32, 6, args.maps
    torch.manual_seed(0)
    fc = Fcomb([F, 64, 128, 192], Lz, 1, K, 4, {"w": "orthogonal", "b": "normal"}).to(dev)
    with torch.no_grad():
        fc.last_layer.weight.mul_(8)         # logits of a few units: the samples disagree
    g = torch.Generator(device=dev).manual_seed(1)
    feat = torch.relu(torch.randn(N, H, H, F, device=dev, generator=g)).permute(0, 3, 1, 2)   # channels-last storage
    z = torch.randn(S, N, Lz, device=dev, generator=g)

    def fused():
        return prob_engine.fcomb_stats(fc, feat, z, want_label=True, want_labels=True)

    def torch_path():
        y = prob_engine.fcomb_forward(fc, feat, z)[0]
        p = torch.softmax(y, 2)
        mean = p.mean(0)
        ent = -torch.xlogy(mean, mean).sum(1)
        mi = (ent + torch.xlogy(p, p).sum(2).mean(0)).clamp_min(0)
        return {"mean": mean, "entropy": ent, "mutual_info": mi, "label": mean.argmax(1).int(),
                "labels": y.argmax(2).to(torch.uint8)}

    with torch.no_grad():
        a, b = fused(), torch_path()
        for k in ("mean", "entropy", "mutual_info"):
            print(f"fused vs torch {k}: max diff {float((a[k] - b[k]).abs().max()):.2e} (max {float(b[k].max()):.3f})")
        for k in ("label", "labels"):
            print(f"fused vs torch {k}: {float((a[k] != b[k]).float().mean()):.2e} of the elements differ")
        maps = torch.cat((a["labels"], torch.randint(0, K, (R - S, N, H, H), device=dev, generator=g).to(torch.uint8)))
        maps = maps[:R].reshape(R, N, -1).contiguous()
        del a, b

        def counts():
            return label_pair_counts(maps, K)

        def counts_torch():
            oh = torch.nn.functional.one_hot(maps.long(), K).float()
            return torch.einsum("inpc,jnpc->nijc", oh, oh), oh.sum(2).permute(1, 0, 2)

        ia, ca = counts()
        ib, cb = counts_torch()
        print(f"counts vs torch: equal {bool((ia == ib.double()).all()) and bool((ca == cb.double()).all())}")
        del ia, ca, ib, cb
        rows = pair("stats", {"fused": fused, "torch": torch_path}, {"fused": 20, "torch": 10}, args.repeats)
        rows += pair("counts", {"kernel": counts, "torch": counts_torch}, {"kernel": 50, "torch": 5}, args.repeats)
    print(f"S={S} N={N} {H}x{H} K={K} F={F}; R={R}; logits tensor {4 * S * N * K * H * H / 2 ** 20:.0f} MiB")
    print(f"{'pair':7s} {'path':7s} {'us/call':>10s} {'min..max':>21s} {'peak MiB':>9s}")
    for r in rows:
        print(f"{r['pair']:7s} {r['path']:7s} {r['us']:10.1f} {r['us_min']:10.1f}..{r['us_max']:<10.1f}"
              f"{r['peak_bytes'] / 2 ** 20:9.1f}", flush=True)
    if args.json:
        with open(args.json, "w") as f:
            json.dump(rows, f, indent=1)


if __name__ == "__main__":
    main()
