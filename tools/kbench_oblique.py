#!/usr/bin/env python3
"""Kernel timing of the oblique-view kernels beside the standard-axis kernels they generalise, on one
D^3 volume (default 256^3, C = 3, six seeded views, P = D):

    pmu_gather_slices   vs  pmu_oblique_gather   a batch of B slices (image mode, max normalisation)
    pmu_fuse3view       vs  pmu_fuse_oblique     the whole volume (probabilities in; avg, label, counts out)

    python tools/kbench_oblique.py [--size 256] [--views 6] [--classes 3] [--batch 32] [--repeats 3] [--plan]

Method: device events around windows of launches of one entry; every entry is warmed up first; the two
kernels of a pair are timed alternately --repeats times in one process, so the spread between the windows
of one entry is on the table next to the difference between the pair.  The gather cycles through the
volume's slices (and through the views), so consecutive launches read different data; one fusion pass
reads more than the 256 MiB Infinity Cache holds at the default size.

GB/s are algorithmic bytes over the time: a gathered pixel is 8 bytes read and 4 written (the oblique
gather reads up to eight voxels per pixel; the figure counts each pixel's share of the volume once); the
fusions read every stack element and the truth once and write avg, label (and cover).  The last column is
the host's time to enqueue one call.

--plan prints shapes and bytes without touching a device.  A run without a GPU fails."""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "probabilistic-multiplanar-unet_amd"))


def algorithmic_bytes(entry, D, C, V, B):
    n = D ** 3
    return {"pmu_gather_slices": 12 * B * D * D, "pmu_oblique_gather": 12 * B * D * D,
            "pmu_fuse3view": (12 * C + 4 + 4 * C + 4) * n,
            "pmu_fuse_oblique": (4 * V * C + 4 + 4 * C + 8) * n}[entry]


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


def bench(D, C, V, B, repeats, dev):
    import numpy as np
    import torch
    from pmu_hip import _lib as L
    from utils.mri_dataset import draw_views, view_frame
    g = torch.Generator(device=dev).manual_seed(D)
    s = L.stream()
    vol = torch.randint(0, 256, (D, D, D), device=dev, generator=g).double()
    frames = torch.from_numpy(np.stack([view_frame(n) for n in draw_views(V, 0, 30)]).reshape(V, 9)).to(dev)
    # standard path: the volume itself is view 0's layout; slice table and maxima as MRI_Dataset builds them
    addr = torch.tensor([vol.data_ptr() + i * D * D * 8 for i in range(D)], dtype=torch.int64, device=dev)
    smax = torch.empty(D, dtype=torch.float64, device=dev)
    L.call("pmu_slice_max", vol.data_ptr(), D, D * D, smax.data_ptr(), s)
    omax = torch.empty(V * D, dtype=torch.float64, device=dev)
    for v in range(V):
        L.call("pmu_oblique_slice_max", vol.data_ptr(), D, D, D, frames[v].data_ptr(), D, 1.0, 0,
               omax[v * D:].data_ptr(), s)
    vaddr = torch.tensor([vol.data_ptr()] * V, dtype=torch.int64, device=dev)
    dims = torch.tensor([D, D, D] * V, dtype=torch.int32, device=dev)
    nb = D // B
    ids_std = [torch.arange(k * B, (k + 1) * B, dtype=torch.int32, device=dev) for k in range(nb)]
    ids_obl = [torch.arange(k * B, (k + 1) * B, dtype=torch.int32, device=dev) + v * D for v in range(V) for k in range(nb)]
    out = torch.empty(B, 1, D, D, device=dev)
    st = torch.rand(V, D, C, D, D, device=dev, generator=g)
    st /= st.sum(2, keepdim=True)
    truth = torch.randint(0, C, (D, D, D), device=dev, generator=g).float()
    avg = torch.empty(D, C, D, D, device=dev)
    label = torch.empty(D, D, D, dtype=torch.int32, device=dev)
    cover = torch.empty(D, D, D, dtype=torch.int32, device=dev)
    counts = torch.empty(V + 1, C, 3, dtype=torch.float64, device=dev)
    fns = {
        "pmu_gather_slices": lambda i: L.call("pmu_gather_slices", addr.data_ptr(), smax.data_ptr(),
                                              ids_std[i % nb].data_ptr(), B, D * D, 1, out.data_ptr(), s),
        "pmu_oblique_gather": lambda i: L.call("pmu_oblique_gather", vaddr.data_ptr(), dims.data_ptr(), frames.data_ptr(),
                                               omax.data_ptr(), ids_obl[i % (V * nb)].data_ptr(), B, V, D, 1.0, 0,
                                               out.data_ptr(), s),
        "pmu_fuse3view": lambda i: L.call("pmu_fuse3view", st[0].data_ptr(), st[1].data_ptr(), st[2].data_ptr(),
                                          truth.data_ptr(), D, D, D, C, 0, avg.data_ptr(), label.data_ptr(),
                                          counts.data_ptr(), s),
        "pmu_fuse_oblique": lambda i: L.call("pmu_fuse_oblique", st.data_ptr(), frames.data_ptr(), V, C, D, 1.0,
                                             truth.data_ptr(), D, D, D, avg.data_ptr(), label.data_ptr(),
                                             cover.data_ptr(), counts.data_ptr(), s),
    }
    launches = {"pmu_gather_slices": 200, "pmu_oblique_gather": 200, "pmu_fuse3view": 20, "pmu_fuse_oblique": 20}
    for name, fn in fns.items():
        window(fn, max(3, launches[name] // 10))
    times = {n: [] for n in fns}
    hosts = {n: [] for n in fns}
    for _ in range(repeats):
        for name, fn in fns.items():
            us, host = window(fn, launches[name])
            times[name].append(us)
            hosts[name].append(host)
    rows = []
    for name in fns:
        us = statistics.median(times[name])
        rows.append({"size": D, "classes": C, "views": V, "batch": B, "entry": name, "us": us, "us_min": min(times[name]),
                     "us_max": max(times[name]), "gbps": algorithmic_bytes(name, D, C, V, B) / (us * 1e-6) / 1e9,
                     "launches": launches[name], "host_enqueue_us": statistics.median(hosts[name])})
    return rows


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--size", type=int, default=256, help="volume edge D (and sample_dim P)")
    ap.add_argument("--views", type=int, default=6, help="oblique views V (1..8)")
    ap.add_argument("--classes", type=int, default=3, help="classes C (1..8)")
    ap.add_argument("--batch", type=int, default=32, help="slices per gather launch")
    ap.add_argument("--repeats", type=int, default=3, help="alternations of each pair (at least 3)")
    ap.add_argument("--plan", action="store_true", help="print shapes and bytes; no device needed")
    ap.add_argument("--json", default=None, help="also write the rows to this file")
    args = ap.parse_args()
    D, C, V, B = args.size, args.classes, args.views, args.batch
    if args.repeats < 3 or not 1 <= V <= 8 or not 1 <= C <= 8 or D % B:
        ap.error("--repeats must be at least 3, views and classes within 1..8, and --batch must divide --size")
    if args.plan:
        for e in ("pmu_gather_slices", "pmu_oblique_gather", "pmu_fuse3view", "pmu_fuse_oblique"):
            print(f"{e:19s} D={D} C={C} V={V} B={B}: {algorithmic_bytes(e, D, C, V, B) / 1e6:.1f} MB per call")
        print(f"stacks {4 * V * C * D ** 3 / 2 ** 20:.0f} MiB, volume {8 * D ** 3 / 2 ** 20:.0f} MiB")
        return
    import torch
    if not torch.cuda.is_available():
        sys.exit("kbench_oblique.py times kernels on the GPU; there is none here (no CPU fallback)")
    rows = bench(D, C, V, B, args.repeats, torch.device("cuda"))
    print(f"{'entry':19s} {'us/call':>10s} {'min..max':>21s} {'GB/s':>7s} {'enqueue us':>10s}")
    for r in rows:
        print(f"{r['entry']:19s} {r['us']:10.1f} {r['us_min']:10.1f}..{r['us_max']:<10.1f}{r['gbps']:7.0f} "
              f"{r['host_enqueue_us']:10.1f}", flush=True)
    if args.json:
        with open(args.json, "w") as f:
            json.dump(rows, f, indent=1)


if __name__ == "__main__":
    main()
