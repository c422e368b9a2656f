#!/usr/bin/env python3
"""Timing of the surface-distance kernels on a seeded blob phantom (K = 3 classes: per foreground class a few
random ellipsoids; the "truth" is the same phantom drawn with jittered centres) at 256^3 and 512^3:

    edt        pmu_surface_edt of one class (pmu_hip.surface._edt: the row pass and two column passes)
    collect    pmu_surface_collect of one class's surface out of the other volume's transform
    distances  pmu_hip.surface.surface_distances, both foreground classes, everything included (four transforms,
               four gathers, the sorts, the float64 metrics and the host reads of the surface counts)

beside the two yardsticks of DESIGN.md "Surface distances":

    bytes bound  three in-place passes move 6 x 4 B per voxel per field; at the box's copy rate (6.29 TB/s,
                 DESIGN.md) that is the least time a separable transform of this layout can take
    scipy        scipy.ndimage.distance_transform_edt of the same surface mask on the host (the route a user
                 has without these kernels), one call per size; "not available" when scipy cannot be imported

    python tools/kbench_surface.py [--sizes 256 512] [--repeats 3] [--no-scipy] [--kernels] [--json out.json]

Method: device events around windows of calls, every path warmed up first, median and min..max over --repeats
windows; surface_distances ends in host reads, so its window is also closed by a synchronise.  --kernels adds
the device time per kernel of one transform (torch.profiler), which tells the passes apart.  The transform of
the first size is compared with scipy's squared distances before anything is timed (unit voxels: equal as
integers).  A run without a GPU fails."""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "probabilistic-multiplanar-unet_amd"))

COPY_RATE = 6.29e12     # B/s, DESIGN.md
K = 3


def phantom(n, seed, jitter, dev):
    """(n,n,n) u8 labels 0..K-1: three ellipsoids per foreground class, centres moved by up to ``jitter`` voxels
    (the same seed with another jitter seed gives a prediction-like neighbour of a volume)."""
    import torch
    g = torch.Generator().manual_seed(seed)
    gj = torch.Generator().manual_seed(seed + 1000 + int(jitter * 7))
    ax = torch.arange(n, dtype=torch.float32, device=dev)
    lab = torch.zeros(n, n, n, dtype=torch.uint8, device=dev)
    for c in range(1, K):
        for _ in range(3):
            ctr = (0.25 + 0.5 * torch.rand(3, generator=g)) * n + (torch.rand(3, generator=gj) - 0.5) * 2 * jitter
            rad = (0.08 + 0.14 * torch.rand(3, generator=g)) * n
            r2 = (((ax - ctr[0]) / rad[0]) ** 2)[:, None, None] + (((ax - ctr[1]) / rad[1]) ** 2)[None, :, None] \
                + (((ax - ctr[2]) / rad[2]) ** 2)[None, None, :]
            lab[r2 <= 1.0] = c
    return lab


def window(fn, n):
    import torch
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(n):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e3 / n    # microseconds per call


def timed(fn, launches, repeats):
    window(fn, 2)
    t = [window(fn, launches) for _ in range(repeats)]
    return {"us": statistics.median(t), "us_min": min(t), "us_max": max(t), "launches": launches}


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--sizes", type=int, nargs="+", default=[256, 512])
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--no-scipy", action="store_true", help="skip the host yardstick")
    ap.add_argument("--kernels", action="store_true", help="device time per kernel of one transform")
    ap.add_argument("--json", default=None, help="also write the rows to this file")
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        sys.exit("kbench_surface.py times kernels on the GPU; there is none here (no CPU fallback)")
    from pmu_hip import surface as S
    dev = torch.device("cuda")
    ndi = None
    if not args.no_scipy:
        try:
            import scipy.ndimage as ndi
        except ImportError:
            ndi = None
    print(f"device: {torch.cuda.get_device_name(0)}; scipy: {'yes' if ndi else 'not available'}", flush=True)
    sp = (1.0, 1.0, 1.0)
    rows = []
    for i, n in enumerate(args.sizes):
        truth, pred = phantom(n, 1, 0.0, dev), phantom(n, 1, 0.03 * n, dev)
        cnt = torch.empty(2, dtype=torch.int64, device=dev)
        d2_truth = S._edt(truth, 1, sp, cnt[0:1])
        n_truth = int(cnt[0].item())
        d2_pred = S._edt(pred, 1, sp, cnt[1:2])
        n_pred = int(cnt[1].item())
        print(f"{n}^3: class 1 has {int((truth == 1).sum())} voxels, {n_truth} on the surface (prediction: {n_pred})",
              flush=True)
        scipy_s = None
        if ndi is not None:
            import numpy as np
            mask = (truth == 1).cpu().numpy()
            surf = mask ^ ndi.binary_erosion(mask)
            t0 = time.perf_counter()
            want = ndi.distance_transform_edt(~surf)
            scipy_s = time.perf_counter() - t0
            if i == 0:
                same = np.array_equal(d2_truth.cpu().numpy(), np.round(want ** 2).astype(np.float32))
                print(f"{n}^3: transform equals scipy's squared distances: {same}", flush=True)
                if not same:
                    sys.exit("the transform differs from scipy's: nothing to time")
            del want, surf, mask
        bound_us = 6 * 4 * n ** 3 / COPY_RATE * 1e6
        r = {"size": n, "bytes_bound_us": bound_us, "scipy_s": scipy_s}
        r["edt"] = timed(lambda: S._edt(truth, 1, sp, cnt[0:1]), 10, args.repeats)
        r["collect"] = timed(lambda: S._collect(pred, 1, d2_truth, n_pred, cnt[1:2]), 20, args.repeats)
        r["distances"] = timed(lambda: S.surface_distances(pred, truth, K, sp, 1.0), 3, args.repeats)
        if args.kernels:
            try:
                from torch.profiler import ProfilerActivity, profile
                with profile(activities=[ProfilerActivity.CUDA]) as prof:
                    S._edt(truth, 1, sp, cnt[0:1])
                    torch.cuda.synchronize()
                r["kernels"] = {}
                for ev in prof.events():
                    t = ev.device_time if hasattr(ev, "device_time") else ev.cuda_time
                    if t and ("kernel" in ev.name or "Memset" in ev.name or "memset" in ev.name):
                        r["kernels"].setdefault(ev.name, []).append(float(t))
            except Exception as e:   # the profiler is an extra: the timings above stand without it
                r["kernels"] = f"not available ({type(e).__name__}: {e})"
        rows.append(r)
        e = r["edt"]
        print(f"{n}^3 edt        {e['us']:10.1f} us  ({e['us_min']:.1f}..{e['us_max']:.1f})   bytes bound "
              f"{bound_us:.1f} us: {e['us'] / bound_us:.2f}x"
              + (f"   scipy {scipy_s:.2f} s: {scipy_s * 1e6 / e['us']:.0f}x" if scipy_s else "   scipy: not available"))
        c = r["collect"]
        print(f"{n}^3 collect    {c['us']:10.1f} us  ({c['us_min']:.1f}..{c['us_max']:.1f})")
        d = r["distances"]
        print(f"{n}^3 distances  {d['us']:10.1f} us  ({d['us_min']:.1f}..{d['us_max']:.1f})   K = {K}: four transforms, "
              f"four gathers" + (f"   four scipy transforms {4 * scipy_s:.2f} s: {4 * scipy_s * 1e6 / d['us']:.0f}x"
                                 if scipy_s else ""))
        if args.kernels:
            if isinstance(r["kernels"], dict):
                for name, ts in r["kernels"].items():
                    print(f"{n}^3   kernel {name[:60]:60s} " + " ".join(f"{t:9.1f}" for t in ts) + " us")
            else:
                print(f"{n}^3   kernels: {r['kernels']}")
        sys.stdout.flush()
        del truth, pred, d2_truth, d2_pred
        torch.cuda.empty_cache()
    if args.json:
        with open(args.json, "w") as f:
            json.dump(rows, f, indent=1)


if __name__ == "__main__":
    main()
