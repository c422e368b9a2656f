#!/usr/bin/env python3
"""Kernel timing of the soft Dice loss and the boundary loss beside the cross-entropy kernels they sit next to:
pmu_ce_fwd (reduction sum) / pmu_ce_bwd, pmu_softdice_fwd / pmu_softdice_bwd and pmu_boundary_map / pmu_boundary_fwd /
pmu_boundary_bwd on the same tensors.  The targets are blobs (the argmax of coarse random fields, upsampled), not
noise: the map's scan length depends on the distances, and the other entries do not care.

    python tools/kbench_loss.py [--launches 200] [--repeats 3] [--plan]

Method: device events around windows of --launches launches of one entry; every shape is warmed up first;
the families are timed alternately --repeats times in one process, so the spread between the
repeat windows of one entry is on the table next to the difference between the families.  Each launch takes
the next of R copies of the tensors, R chosen so that the copies together exceed 1 GiB: the 256 MiB
Infinity Cache cannot hold a pass's operands for the next, and the rate is an HBM rate.

Output per shape and entry: microseconds per call (median of the repeat windows, and their min..max),
GB/s from the algorithmic bytes — forward (4K + 8) N HW (logits and int64 targets read once), backward
(8K + 8) N HW (the same plus dx written); the boundary entries read phi as well, (8K + 8) and (12K + 8) N HW, and
the map reads the targets and writes phi, (4K + 8) N HW (its membership bits, K / 4 bytes per pixel written and
read, are left out: the map is bounded by its LDS scan, about 2 sqrt(d2) reads per pixel, not by bytes) — and
that rate as a share of the 6.3 TB/s the device reaches on a float4 copy.  The CE kernels are the yardstick: they read and write the same bytes.  The last column is the
host's time to enqueue one call: where it is not well below the device time, the window measured the
host's launch rate, not the kernel (a forward is two launches: the streaming kernel and its finalizer).

--plan prints the shapes, bytes and copies without touching a device.  A run without a GPU fails."""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "probabilistic-multiplanar-unet_amd"))

SHAPES = [(32, 2, 256, 256), (32, 3, 256, 256), (16, 3, 512, 512)]   # (N, K, H, W)
COPY_RATE = 6.3e12      # bytes/s, float4 copy
ROTATE_BYTES = 1 << 30
ENTRIES = ("pmu_ce_fwd", "pmu_ce_bwd", "pmu_softdice_fwd", "pmu_softdice_bwd", "pmu_boundary_map", "pmu_boundary_fwd",
           "pmu_boundary_bwd")


def algorithmic_bytes(entry, N, K, HW):
    phi = 4 * K if entry in ("pmu_boundary_fwd", "pmu_boundary_bwd") else 0    # the map read next to the logits
    return (((8 * K + 8) if entry.endswith("_bwd") else (4 * K + 8)) + phi) * N * HW


def copies(N, K, HW):
    per_set = (12 * K + 8) * N * HW    # x, t, dx, phi
    return max(2, -(-ROTATE_BYTES // per_set))


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


def bench_shape(N, K, H, W, launches, repeats, dev):
    import torch
    from pmu_hip import _lib as L
    HW, R = H * W, copies(N, K, H * W)
    g = torch.Generator(device=dev).manual_seed(H + K)
    xs = [torch.randn(N, K, H, W, device=dev, generator=g) * 3 for _ in range(R)]
    ts = [torch.nn.functional.interpolate(torch.randn(N, K, H // 32, W // 32, device=dev, generator=g), size=(H, W),
                                          mode="bilinear").argmax(1).contiguous() for _ in range(R)]
    dxs = [torch.empty_like(x) for x in xs]
    phis = [torch.empty_like(x) for x in xs]
    loss = torch.empty((), device=dev)
    count = torch.empty((), device=dev)
    gout = torch.ones((), device=dev)
    ce_ws = torch.empty(L.lib().pmu_loss_ws(N * HW) // 8, dtype=torch.float64, device=dev)
    dice_ws = torch.empty(L.lib().pmu_softdice_ws(N, K, HW) // 8, dtype=torch.float64, device=dev)
    bd_ws = torch.empty(L.lib().pmu_boundary_ws(N, K, H, W) // 8, dtype=torch.float64, device=dev)
    bd_count = torch.empty((), dtype=torch.float64, device=dev)
    s = L.stream()
    for i in range(R):                        # every phi filled once: the loss entries read real maps
        L.call("pmu_boundary_map", ts[i].data_ptr(), 0, N, K, H, W, -100, phis[i].data_ptr(), bd_ws.data_ptr(), s)
    fns = {
        "pmu_ce_fwd": lambda i: L.call("pmu_ce_fwd", xs[i % R].data_ptr(), ts[i % R].data_ptr(), N, K, HW, 2, -100,
                                       loss.data_ptr(), ce_ws.data_ptr(), count.data_ptr(), s),
        "pmu_ce_bwd": lambda i: L.call("pmu_ce_bwd", xs[i % R].data_ptr(), ts[i % R].data_ptr(), N, K, HW, 2, -100,
                                       gout.data_ptr(), count.data_ptr(), dxs[i % R].data_ptr(), s),
        "pmu_softdice_fwd": lambda i: L.call("pmu_softdice_fwd", xs[i % R].data_ptr(), ts[i % R].data_ptr(), N, K, HW,
                                             0, 0, 0, -100, loss.data_ptr(), dice_ws.data_ptr(), s),
        "pmu_softdice_bwd": lambda i: L.call("pmu_softdice_bwd", xs[i % R].data_ptr(), ts[i % R].data_ptr(), N, K, HW,
                                             0, 0, -100, dice_ws.data_ptr(), gout.data_ptr(), dxs[i % R].data_ptr(), s),
        "pmu_boundary_map": lambda i: L.call("pmu_boundary_map", ts[i % R].data_ptr(), 0, N, K, H, W, -100,
                                             phis[i % R].data_ptr(), bd_ws.data_ptr(), s),
        "pmu_boundary_fwd": lambda i: L.call("pmu_boundary_fwd", xs[i % R].data_ptr(), ts[i % R].data_ptr(),
                                             phis[i % R].data_ptr(), N, K, HW, 0, 1, -100, loss.data_ptr(),
                                             bd_count.data_ptr(), bd_ws.data_ptr(), s),
        "pmu_boundary_bwd": lambda i: L.call("pmu_boundary_bwd", xs[i % R].data_ptr(), ts[i % R].data_ptr(),
                                             phis[i % R].data_ptr(), N, K, HW, 0, 1, -100, gout.data_ptr(),
                                             bd_count.data_ptr(), dxs[i % R].data_ptr(), s),
    }
    for name in ENTRIES:                      # warm-up: code objects loaded, every copy touched
        window(fns[name], 2 * R)
    times = {name: [] for name in ENTRIES}
    hosts = {name: [] for name in ENTRIES}
    for _ in range(repeats):                  # CE family, Dice family, boundary family, CE family, ...
        for name in ENTRIES:
            us, host = window(fns[name], launches)
            times[name].append(us)
            hosts[name].append(host)
    rows = []
    for name in ENTRIES:
        us = statistics.median(times[name])
        rate = algorithmic_bytes(name, N, K, HW) / (us * 1e-6)
        rows.append({"shape": [N, K, H, W], "entry": name, "us": us, "us_min": min(times[name]),
                     "us_max": max(times[name]), "windows_us": times[name], "gbps": rate / 1e9,
                     "share_of_copy_rate": rate / COPY_RATE, "copies": R, "launches": launches,
                     "host_enqueue_us": statistics.median(hosts[name])})
    return rows


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--launches", type=int, default=200, help="launches per timed window (at least 200)")
    ap.add_argument("--repeats", type=int, default=3, help="alternations of the two families (at least 3)")
    ap.add_argument("--plan", action="store_true", help="print shapes, bytes and copies; no device needed")
    ap.add_argument("--json", default=None, help="also write the rows to this file")
    args = ap.parse_args()
    if args.launches < 200 or args.repeats < 3:
        ap.error("--launches must be at least 200 and --repeats at least 3")
    if args.plan:
        for N, K, H, W in SHAPES:
            print(f"N={N} K={K} {H}x{W}: forward {algorithmic_bytes('f_fwd', N, K, H * W) / 1e6:.1f} MB, "
                  f"backward {algorithmic_bytes('f_bwd', N, K, H * W) / 1e6:.1f} MB, {copies(N, K, H * W)} copies")
        return
    import torch
    if not torch.cuda.is_available():
        sys.exit("kbench_loss.py times kernels on the GPU; there is none here (no CPU fallback)")
    dev = torch.device("cuda")
    rows = []
    print(f"{'shape (N,K,H,W)':18s} {'entry':17s} {'us/call':>8s} {'min..max':>15s} {'GB/s':>6s} {'of 6.3 TB/s':>11s} "
          f"{'enqueue us':>10s}")
    for N, K, H, W in SHAPES:
        for r in bench_shape(N, K, H, W, args.launches, args.repeats, dev):
            rows.append(r)
            print(f"{str(tuple(r['shape'])):18s} {r['entry']:17s} {r['us']:8.1f} {r['us_min']:7.1f}..{r['us_max']:<7.1f}"
                  f"{r['gbps']:6.0f} {100 * r['share_of_copy_rate']:10.1f}% {r['host_enqueue_us']:10.1f}", flush=True)
    if args.json:
        with open(args.json, "w") as f:
            json.dump(rows, f, indent=1)


if __name__ == "__main__":
    main()
