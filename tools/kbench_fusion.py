#!/usr/bin/env python3
"""Kernel timing of the learned-fusion kernels beside the plain-mean kernels whose stacks they read, on one
D^3 volume (default 256^3, C = 3; six seeded oblique views, P = D), all in one process:

    pmu_fuse3view     vs  pmu_fusion3_eval         fit mode (the sums alone) and apply mode (prob, label, counts)
    pmu_fuse_oblique  vs  pmu_fusion_oblique_eval  the same two modes

    python tools/kbench_fusion.py [--size 256] [--views 6] [--classes 3] [--repeats 3] [--plan]

Method (tools/kbench_oblique.py's): device events around windows of launches of one entry; every entry is warmed
up first; the entries are timed alternately --repeats times, so the spread between the windows of one entry is on
the table next to the difference between the entries (median, min..max).  One pass reads more than the 256 MiB
Infinity Cache holds at the default size.  The ratio column is the entry's median over the median of the
plain-mean kernel of its group.

GB/s are algorithmic bytes over the time: every stack element and the truth read once; apply mode writes prob and
label (the oblique kernels also cover); fit mode writes one row of sums per workgroup (not counted).  The fp64
arithmetic of a voxel (C exp, one log, one divide per class) is what the fit pass adds to the plain kernel's
traffic; GFLOP-free, it shows as a lower GB/s.

--plan prints shapes and bytes without touching a device.  A run without a GPU fails."""
import argparse
import ctypes
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "probabilistic-multiplanar-unet_amd"))

ENTRIES = ("pmu_fuse3view", "pmu_fusion3_eval fit", "pmu_fusion3_eval apply",
           "pmu_fuse_oblique", "pmu_fusion_oblique_eval fit", "pmu_fusion_oblique_eval apply")
BASE = {e: ("pmu_fuse3view" if "3" in e.split()[0] else "pmu_fuse_oblique") for e in ENTRIES}


def algorithmic_bytes(entry, D, C, V):
    n = D ** 3
    read3, readv = 12 * C + 4, 4 * V * C + 4
    return {"pmu_fuse3view": (read3 + 4 * C + 4) * n, "pmu_fusion3_eval fit": read3 * n,
            "pmu_fusion3_eval apply": (read3 + 4 * C + 4) * n, "pmu_fuse_oblique": (readv + 4 * C + 8) * n,
            "pmu_fusion_oblique_eval fit": readv * n, "pmu_fusion_oblique_eval apply": (readv + 4 * C + 8) * n}[entry]


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


def bench(D, C, V, repeats, launches, dev):
    import numpy as np
    import torch
    from pmu_hip import _lib as L
    from utils.mri_dataset import draw_views, view_frame
    g = torch.Generator(device=dev).manual_seed(D)
    s = L.stream()
    frames = torch.from_numpy(np.stack([view_frame(n) for n in draw_views(V, 0, 30)]).reshape(V, 9)).to(dev)
    st = torch.rand(max(V, 3), D, C, D, D, device=dev, generator=g)
    st /= st.sum(2, keepdim=True)
    truth = torch.randint(0, C, (D, D, D), device=dev, generator=g).float()
    avg = torch.empty(D, C, D, D, device=dev)
    label = torch.empty(D, D, D, dtype=torch.int32, device=dev)
    cover = torch.empty(D, D, D, dtype=torch.int32, device=dev)
    counts = torch.empty(V + 1, C, 3, dtype=torch.float64, device=dev)
    sums = torch.empty(2 + C + max(V, 3) * C, dtype=torch.float64, device=dev)
    rs = np.random.RandomState(0)

    def doubles(a):
        return (ctypes.c_double * a.size)(*a.tolist())

    par3 = doubles(np.concatenate([rs.uniform(0.2, 1.0, 3 * C), rs.uniform(-0.1, 0.1, C)]))
    parv = doubles(np.concatenate([rs.uniform(0.2, 1.0, V * C), rs.uniform(-0.1, 0.1, C)]))
    n3 = int(L.lib().pmu_fusion3_ws(D, D, D, C))
    nv = int(L.lib().pmu_fusion_oblique_ws(V, C, D, D, D))
    ws = torch.empty(max(n3, nv) // 8, dtype=torch.float64, device=dev)
    p3 = (st[0].data_ptr(), st[1].data_ptr(), st[2].data_ptr(), truth.data_ptr(), D, D, D, C, 0)
    pv = (st.data_ptr(), frames.data_ptr(), V, C, D, 1.0, truth.data_ptr(), D, D, D)
    fns = {
        "pmu_fuse3view": lambda i: L.call("pmu_fuse3view", *p3, avg.data_ptr(), label.data_ptr(), counts.data_ptr(), s),
        "pmu_fusion3_eval fit": lambda i: L.call("pmu_fusion3_eval", *p3, par3, None, None, None, None, sums.data_ptr(),
                                                 0, ws.data_ptr(), n3, s),
        "pmu_fusion3_eval apply": lambda i: L.call("pmu_fusion3_eval", *p3, par3, None, avg.data_ptr(), label.data_ptr(),
                                                   counts.data_ptr(), None, 0, None, 0, s),
        "pmu_fuse_oblique": lambda i: L.call("pmu_fuse_oblique", *pv, avg.data_ptr(), label.data_ptr(),
                                             cover.data_ptr(), counts.data_ptr(), s),
        "pmu_fusion_oblique_eval fit": lambda i: L.call("pmu_fusion_oblique_eval", *pv, parv, None, None, None, None,
                                                        None, sums.data_ptr(), 0, ws.data_ptr(), nv, s),
        "pmu_fusion_oblique_eval apply": lambda i: L.call("pmu_fusion_oblique_eval", *pv, parv, None, avg.data_ptr(),
                                                          label.data_ptr(), cover.data_ptr(), counts.data_ptr(), None, 0,
                                                          None, 0, s),
    }
    for fn in fns.values():
        window(fn, max(3, launches // 10))
    times = {n: [] for n in fns}
    hosts = {n: [] for n in fns}
    for _ in range(repeats):
        for name, fn in fns.items():
            us, host = window(fn, launches)
            times[name].append(us)
            hosts[name].append(host)
    med = {n: statistics.median(times[n]) for n in fns}
    rows = []
    for name in fns:
        rows.append({"size": D, "classes": C, "views": V, "entry": name, "us": med[name], "us_min": min(times[name]),
                     "us_max": max(times[name]), "ratio": med[name] / med[BASE[name]],
                     "gbps": algorithmic_bytes(name, D, C, V) / (med[name] * 1e-6) / 1e9, "launches": launches,
                     "host_enqueue_us": statistics.median(hosts[name])})
    return rows


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--size", type=int, default=256, help="volume edge D (and sample_dim P)")
    ap.add_argument("--views", type=int, default=6, help="oblique views V (1..8)")
    ap.add_argument("--classes", type=int, default=3, help="classes C (2..8)")
    ap.add_argument("--repeats", type=int, default=3, help="alternations of the entries (at least 3)")
    ap.add_argument("--launches", type=int, default=20, help="launches per window")
    ap.add_argument("--plan", action="store_true", help="print shapes and bytes; no device needed")
    ap.add_argument("--json", default=None, help="also write the rows to this file")
    args = ap.parse_args()
    D, C, V = args.size, args.classes, args.views
    if args.repeats < 3 or not 1 <= V <= 8 or not 2 <= C <= 8 or args.launches < 1:
        ap.error("--repeats must be at least 3, views within 1..8, classes within 2..8")
    if args.plan:
        for e in ENTRIES:
            print(f"{e:30s} D={D} C={C} V={V}: {algorithmic_bytes(e, D, C, V) / 1e6:.1f} MB per call")
        print(f"stacks: three views {12 * C * D ** 3 / 2 ** 20:.0f} MiB, {V} oblique views {4 * V * C * D ** 3 / 2 ** 20:.0f} MiB")
        return
    import torch
    if not torch.cuda.is_available():
        sys.exit("kbench_fusion.py times kernels on the GPU; there is none here (no CPU fallback)")
    rows = bench(D, C, V, args.repeats, args.launches, torch.device("cuda"))
    print(f"{'entry':30s} {'us/call':>10s} {'min..max':>21s} {'ratio':>6s} {'GB/s':>7s} {'enqueue us':>10s}")
    for r in rows:
        print(f"{r['entry']:30s} {r['us']:10.1f} {r['us_min']:10.1f}..{r['us_max']:<10.1f}{r['ratio']:6.2f} "
              f"{r['gbps']:7.0f} {r['host_enqueue_us']:10.1f}", flush=True)
    if args.json:
        with open(args.json, "w") as f:
            json.dump(rows, f, indent=1)


if __name__ == "__main__":
    main()
