#!/usr/bin/env python3
"""Kernel timing of the warped batch gather beside the two launches it replaces, on one D^3 scan (default
256^3, six seeded views, P = D, B = 32 items per batch; image and mask written by both sides):

    oblique_pair     pmu_oblique_gather (image, max normalisation) + pmu_oblique_gather (mask, nearest)
    warp_identity    pmu_warp_gather, identity blocks, G = 0: the same loads in one launch
    warp_default     pmu_warp_gather, the default Augment's draws, G = 6

    python tools/kbench_augment.py [--size 256] [--views 6] [--batch 32] [--repeats 3] [--plan] [--json F]

Method (tools/kbench_oblique.py's): device events around windows of launches of one case; every case is warmed
up first; the cases are timed alternately --repeats times in one process, so the spread between the windows
of one case is on the table next to the difference between the cases.  Consecutive launches cycle through
the scan's slices and views, so they read different data.  GB/s are algorithmic bytes over the time: per
pixel 16 bytes read (one image and one mask voxel's share) and 8 written.  The last rows are host times:
to enqueue one call, and Augment.draw for one batch.

--plan prints shapes and bytes without touching a device.  A run without a GPU fails."""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "probabilistic-multiplanar-unet_amd"))

CASES = ("oblique_pair", "warp_identity", "warp_default")


def algorithmic_bytes(D, B):
    return 24 * B * D * D


def window(fn, n):
    import torch
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    h0 = time.perf_counter()
    for i in range(n):
        fn(i)
    host = (time.perf_counter() - h0) * 1e6 / n
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e3 / n, host    # microseconds per call: on the device, to enqueue


def draw_time(aug, keys, D, n=50):
    aug.draw(keys, 0, D, D, 1.0)
    t0 = time.perf_counter()
    for e in range(n):
        aug.draw(keys, e, D, D, 1.0)
    return (time.perf_counter() - t0) * 1e6 / n


def bench(D, V, B, repeats, dev):
    import numpy as np
    import torch
    from pmu_hip import _lib as L
    from pmu_hip.augment import IDENTITY, Augment
    from utils.mri_dataset import draw_views, view_frame
    g = torch.Generator(device=dev).manual_seed(D)
    s = L.stream()
    vol = torch.randint(0, 256, (D, D, D), device=dev, generator=g).double()
    lab = torch.randint(0, 3, (D, D, D), device=dev, generator=g).double()
    frames = torch.from_numpy(np.stack([view_frame(n) for n in draw_views(V, 0, 30)]).reshape(V, 9)).to(dev)
    omax = torch.empty(V * D, dtype=torch.float64, device=dev)
    for v in range(V):
        L.call("pmu_oblique_slice_max", vol.data_ptr(), D, D, D, frames[v].data_ptr(), D, 1.0, 0,
               omax[v * D:].data_ptr(), s)
    vimg = torch.tensor([vol.data_ptr()] * V, dtype=torch.int64, device=dev)
    vmask = torch.tensor([lab.data_ptr()] * V, dtype=torch.int64, device=dev)
    dims = torch.tensor([D, D, D] * V, dtype=torch.int32, device=dev)
    nb = D // B
    batches = [[(0, v, k * B + j) for j in range(B)] for v in range(V) for k in range(nb)]
    ids = [torch.tensor([v * D + sl for _, v, sl in b], dtype=torch.int32, device=dev) for b in batches]
    item = [torch.tensor([[v, v * D + sl] for _, v, sl in b], dtype=torch.int32, device=dev) for b in batches]
    aug = Augment(seed=1)
    G = aug.grid
    par_id, par_aug, ctrl = [], [], []
    for b in batches:
        ds = np.array([sl - (D - 1) / 2.0 for _, _, sl in b])
        p0 = np.tile(IDENTITY, (B, 1))
        p1, c1 = aug.draw(b, 0, D, D, 1.0)
        p0[:, 0], p1[:, 0] = ds, ds
        par_id.append(torch.from_numpy(p0).to(dev))
        par_aug.append(torch.from_numpy(p1).to(dev))
        ctrl.append(torch.from_numpy(c1).to(dev))
    img = torch.empty(B, 1, D, D, device=dev)
    mask = torch.empty(B, 1, D, D, device=dev)
    nbat = len(batches)

    def pair(i):
        k = i % nbat
        L.call("pmu_oblique_gather", vimg.data_ptr(), dims.data_ptr(), frames.data_ptr(), omax.data_ptr(),
               ids[k].data_ptr(), B, V, D, 1.0, 0, img.data_ptr(), s)
        L.call("pmu_oblique_gather", vmask.data_ptr(), dims.data_ptr(), frames.data_ptr(), None, ids[k].data_ptr(), B, V,
               D, 1.0, 1, mask.data_ptr(), s)

    def warp(par, ctl, grid):
        def fn(i):
            k = i % nbat
            L.call("pmu_warp_gather", vimg.data_ptr(), vmask.data_ptr(), dims.data_ptr(), frames.data_ptr(), V,
                   item[k].data_ptr(), omax.data_ptr(), par[k].data_ptr(), ctl[k].data_ptr() if grid else None, grid, B, D,
                   D, 1.0, img.data_ptr(), mask.data_ptr(), s)
        return fn

    fns = {"oblique_pair": pair, "warp_identity": warp(par_id, ctrl, 0), "warp_default": warp(par_aug, ctrl, G)}
    # the identity case computes what the pair computes
    pair(3)
    want = (img.clone(), mask.clone())
    fns["warp_identity"](3)
    if not (torch.equal(img, want[0]) and torch.equal(mask, want[1])):
        sys.exit("kbench_augment.py: the identity warp differs from the pair of oblique gathers")
    launches = 1000   # ~50 ms per window
    for fn in fns.values():
        window(fn, launches // 10)
    times, hosts = {n: [] for n in fns}, {n: [] for n in fns}
    for _ in range(repeats):
        for name, fn in fns.items():
            us, host = window(fn, launches)
            times[name].append(us)
            hosts[name].append(host)
    rows = []
    for name in fns:
        us = statistics.median(times[name])
        rows.append({"size": D, "views": V, "batch": B, "grid": {"warp_default": G}.get(name, 0), "case": name, "us": us,
                     "us_min": min(times[name]), "us_max": max(times[name]),
                     "gbps": algorithmic_bytes(D, B) / (us * 1e-6) / 1e9, "launches": launches,
                     "host_enqueue_us": statistics.median(hosts[name])})
    rows.append({"size": D, "batch": B, "grid": G, "case": "Augment.draw (host)", "us": draw_time(aug, batches[0], D)})
    return rows


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--size", type=int, default=256, help="volume edge D (and sample_dim P)")
    ap.add_argument("--views", type=int, default=6, help="oblique views V")
    ap.add_argument("--batch", type=int, default=32, help="items per launch")
    ap.add_argument("--repeats", type=int, default=3, help="alternations of the cases (at least 3)")
    ap.add_argument("--plan", action="store_true", help="print shapes and bytes; no device needed")
    ap.add_argument("--json", default=None, help="also write the rows to this file")
    args = ap.parse_args()
    D, V, B = args.size, args.views, args.batch
    if args.repeats < 3 or V < 1 or D % B:
        ap.error("--repeats must be at least 3, --views at least 1, and --batch must divide --size")
    if args.plan:
        for c in CASES:
            print(f"{c:14s} D={D} V={V} B={B}: {algorithmic_bytes(D, B) / 1e6:.1f} MB per batch, "
                  f"{'2 launches' if c == 'oblique_pair' else '1 launch'}")
        print(f"image and mask volumes {2 * 8 * D ** 3 / 2 ** 20:.0f} MiB, {V * (D // B)} batches in the cycle")
        return
    import torch
    if not torch.cuda.is_available():
        sys.exit("kbench_augment.py times kernels on the GPU; there is none here (no CPU fallback)")
    rows = bench(D, V, B, args.repeats, torch.device("cuda"))
    print(f"{'case':20s} {'us/batch':>10s} {'min..max':>21s} {'GB/s':>7s} {'enqueue us':>10s}")
    for r in rows:
        if "us_min" in r:
            print(f"{r['case']:20s} {r['us']:10.1f} {r['us_min']:10.1f}..{r['us_max']:<10.1f}{r['gbps']:7.0f} "
                  f"{r['host_enqueue_us']:10.1f}", flush=True)
        else:
            print(f"{r['case']:20s} {r['us']:10.1f}", flush=True)
    if args.json:
        with open(args.json, "w") as f:
            json.dump(rows, f, indent=1)


if __name__ == "__main__":
    main()
