#!/usr/bin/env python3
"""Timing of the connected-component kernels at 256^3 and 512^3 on two volumes:

    noisy   the blob phantom of tools/kbench_surface.py (K = 3 classes) with 15 % of the background voxels set to a
            random class 1..2 — the density of the test volumes: millions of small components
    ball    one solid ball of class 1 (radius 0.4 n): one huge component, which stresses the merge phase

    label        pmu_cc_label (the tile pass, the merge across tile faces, the flatten pass)
    components   pmu_hip.components.components: label, compact, the host read of n, sizes
    keep_largest pmu_hip.components.keep_largest (keep = 1): components, the ranking on the (n,) vectors, the filter

beside the two yardsticks of DESIGN.md "Connected components":

    bytes bound  one read of lab (1 B per voxel) and one write of root (4 B per voxel) at the box's copy rate
                 (6.29 TB/s): the least a labelling that writes a root map can take
    scipy        scipy.ndimage.label per class on the host (the route a user has without these kernels), one call per
                 class; "not available" when scipy cannot be imported

    python tools/kbench_components.py [--sizes 256 512] [--repeats 3] [--connectivity 26] [--no-scipy] [--kernels]
                                      [--json out.json]

Method: device events around windows of calls, every path warmed up first, median and min..max over --repeats
windows; components and keep_largest contain a host read, so their windows are also closed by a synchronise.
--kernels adds the device time per kernel of one label + compact + sizes (torch.profiler), which tells the phases
apart.  The numbering of the first size is compared with scipy's, class by class, before anything is timed.  A
run without a GPU fails."""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "probabilistic-multiplanar-unet_amd"))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from kbench_surface import phantom, timed  # noqa: E402

COPY_RATE = 6.29e12     # B/s, DESIGN.md
K = 3
MAXNZ = {6: 1, 18: 2, 26: 3}


def noisy(n, dev, density=0.15):
    import torch
    lab = phantom(n, 1, 0.0, dev)
    g = torch.Generator(device=dev).manual_seed(5)
    noise = (lab == 0) & (torch.rand(n, n, n, device=dev, generator=g) < density)
    cls = torch.randint(1, K, (n, n, n), device=dev, generator=g, dtype=torch.uint8)
    return torch.where(noise, cls, lab)


def ball(n, dev):
    import torch
    ax = (torch.arange(n, dtype=torch.float32, device=dev) - (n - 1) / 2) ** 2
    r2 = ax[:, None, None] + ax[None, :, None] + ax[None, None, :]
    return (r2 <= (0.4 * n) ** 2).to(torch.uint8)


def scipy_route(ndi, lab_np, ids_np, conn, check):
    """Seconds of scipy.ndimage.label over the classes present; with ``check`` also whether our numbering,
    restricted to each class, is scipy's."""
    import numpy as np
    st = ndi.generate_binary_structure(3, MAXNZ[conn])
    total, same, count = 0.0, True, 0
    for c in range(1, K):
        mask = lab_np == c
        if not mask.any():
            continue
        t0 = time.perf_counter()
        ids_c, n_c = ndi.label(mask, structure=st)
        total += time.perf_counter() - t0
        count += n_c
        if check:
            inv = np.unique(ids_np[mask], return_inverse=True)[1]
            same = same and np.array_equal(inv.reshape(-1) + 1, ids_c[mask])
    return total, same, count


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--sizes", type=int, nargs="+", default=[256, 512])
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--connectivity", type=int, default=26, choices=(6, 18, 26))
    ap.add_argument("--no-scipy", action="store_true", help="skip the host yardstick")
    ap.add_argument("--kernels", action="store_true", help="device time per kernel of one label + compact + sizes")
    ap.add_argument("--json", default=None, help="also write the rows to this file")
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        sys.exit("kbench_components.py times kernels on the GPU; there is none here (no CPU fallback)")
    from pmu_hip import _lib as L
    from pmu_hip import components as C
    dev = torch.device("cuda")
    ndi = None
    if not args.no_scipy:
        try:
            import scipy.ndimage as ndi
        except ImportError:
            ndi = None
    conn = args.connectivity
    print(f"device: {torch.cuda.get_device_name(0)}; connectivity {conn}; scipy: {'yes' if ndi else 'not available'}",
          flush=True)
    rows = []
    for i, n in enumerate(args.sizes):
        for what, lab in (("noisy", noisy(n, dev)), ("ball", ball(n, dev))):
            comp = C.components(lab, conn)
            print(f"{n}^3 {what}: {int((lab != 0).sum())} labelled voxels, {comp['n']} components, largest "
                  f"{int(comp['size'].max())}", flush=True)
            scipy_s = None
            if ndi is not None:
                scipy_s, same, count = scipy_route(ndi, lab.cpu().numpy(), comp["ids"].cpu().numpy(), conn, i == 0)
                if i == 0:
                    print(f"{n}^3 {what}: numbering equals scipy's per class: {same} ({count} components)", flush=True)
                    if not same or count != comp["n"]:
                        sys.exit("the labelling differs from scipy's: nothing to time")
            del comp
            D = (n, n, n)
            root = torch.empty(D, dtype=torch.int32, device=dev)
            cnt = torch.empty(1, dtype=torch.int64, device=dev)
            nbytes = int(L.lib().pmu_cc_ws(*D))
            ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)

            def label():
                L.call("pmu_cc_label", lab.data_ptr(), *D, conn, root.data_ptr(), cnt.data_ptr(), ws.data_ptr(),
                       nbytes, L.stream())

            bound_us = 5 * n ** 3 / COPY_RATE * 1e6
            r = {"size": n, "volume": what, "bytes_bound_us": bound_us, "scipy_s": scipy_s}
            r["label"] = timed(label, 10, args.repeats)
            r["components"] = timed(lambda: C.components(lab, conn), 3, args.repeats)
            r["keep_largest"] = timed(lambda: C.keep_largest(lab, K, connectivity=conn), 3, args.repeats)
            if args.kernels:
                try:
                    from torch.profiler import ProfilerActivity, profile
                    with profile(activities=[ProfilerActivity.CUDA]) as prof:
                        C.components(lab, conn)
                        torch.cuda.synchronize()
                    r["kernels"] = {}
                    for ev in prof.events():
                        t = ev.device_time if hasattr(ev, "device_time") else ev.cuda_time
                        if t and "cc_" in ev.name:
                            r["kernels"].setdefault(ev.name, []).append(float(t))
                except Exception as e:   # the profiler is an extra: the timings above stand without it
                    r["kernels"] = f"not available ({type(e).__name__}: {e})"
            rows.append(r)
            for k in ("label", "components", "keep_largest"):
                e = r[k]
                print(f"{n}^3 {what:5s} {k:12s} {e['us']:10.1f} us  ({e['us_min']:.1f}..{e['us_max']:.1f})   bytes bound "
                      f"{bound_us:.1f} us: {e['us'] / bound_us:.1f}x"
                      + (f"   scipy {scipy_s:.2f} s: {scipy_s * 1e6 / e['us']:.0f}x" if scipy_s
                         else "   scipy: not available"))
            if args.kernels:
                if isinstance(r["kernels"], dict):
                    for name, ts in r["kernels"].items():
                        print(f"{n}^3 {what:5s}   kernel {name[:48]:48s} " + " ".join(f"{t:9.1f}" for t in ts) + " us")
                else:
                    print(f"{n}^3 {what:5s}   kernels: {r['kernels']}")
            sys.stdout.flush()
            del lab, root, ws
            torch.cuda.empty_cache()
    if args.json:
        with open(args.json, "w") as f:
            json.dump(rows, f, indent=1)


if __name__ == "__main__":
    main()
