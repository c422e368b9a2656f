#!/usr/bin/env python3
"""Timing of the local-thickness kernels at 256^3 on two seeded phantoms (K = 3 classes):

    blobs      the phantom of tools/kbench_surface.py: three ellipsoids per foreground class with half-axes of
               20..56 voxels — thick structures, the hard case of the covering pass (its reach is the largest
               interior distance)
    cartilage  two curved shells 4..8 voxels thick facing each other (caps of spherical shells whose thickness
               varies smoothly over the cap): the shape of the tibial and femoral cartilage, the real case

    interior   pmu_interior_edt of one class (row pass, two column passes, the border step)
    cover      pmu_local_thickness of that class's field (tile maxima, then the tiled covering search)
    thickness  pmu_hip.thickness.local_thickness, both foreground classes, everything included (the two kernels
               per class, the sorts, the float64 roots and statistics)

beside pmu_surface_edt of the same class in the same process, and scipy.ndimage.distance_transform_edt of the
class mask on the host (the route a user has without these kernels; "not available" when scipy cannot be
imported).

    python tools/kbench_thickness.py [--size 256] [--repeats 3] [--no-scipy] [--kernels] [--json out.json]

Method: device events around windows of calls, every path warmed up first, median and min..max over --repeats
windows, one process.  The interior transform of each phantom is compared with scipy's squared distances of the
padded mask before anything is timed (unit voxels: equal as integers).  A run without a GPU fails."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "probabilistic-multiplanar-unet_amd"))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from kbench_surface import phantom as blobs, timed  # noqa: E402

K = 3


def cartilage(n, dev):
    """(n,n,n) u8 labels: class 1 a cap of a spherical shell bulging up along axis 0 (the tibial side, nearly
    flat), class 2 a cap of a tighter shell above it (the femoral side); each 4..8 voxels thick."""
    import torch
    ax = torch.arange(n, dtype=torch.float32, device=dev)
    i0, i1, i2 = ax[:, None, None], ax[None, :, None], ax[None, None, :]
    lab = torch.zeros(n, n, n, dtype=torch.uint8, device=dev)
    lateral = ((i1 - 0.5 * n) ** 2 + (i2 - 0.5 * n) ** 2).sqrt()
    wave = 6.0 + 2.0 * torch.sin(i1 * (6.283 / (0.45 * n))) * torch.cos(i2 * (6.283 / (0.6 * n)))   # 4..8 voxels
    for cls, c0, rad, width in ((1, -1.6 * n, 2.05 * n, 0.36 * n), (2, 1.12 * n, 0.62 * n, 0.30 * n)):
        d = ((i0 - c0) ** 2 + (i1 - 0.5 * n) ** 2 + (i2 - 0.5 * n) ** 2).sqrt()
        shell = (d >= rad - wave) & (d < rad) if cls == 2 else (d >= rad) & (d < rad + wave)
        side = i0 > c0 if cls == 1 else i0 < c0
        lab[shell & side & (lateral < width) & (lab == 0)] = cls
    return lab


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--size", type=int, default=256)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--no-scipy", action="store_true", help="skip the host yardstick")
    ap.add_argument("--kernels", action="store_true", help="device time per kernel of one class")
    ap.add_argument("--json", default=None, help="also write the rows to this file")
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        sys.exit("kbench_thickness.py times kernels on the GPU; there is none here (no CPU fallback)")
    from pmu_hip import surface as S
    from pmu_hip import thickness as T
    dev = torch.device("cuda")
    ndi = None
    if not args.no_scipy:
        try:
            import scipy.ndimage as ndi
        except ImportError:
            ndi = None
    print(f"device: {torch.cuda.get_device_name(0)}; scipy: {'yes' if ndi else 'not available'}", flush=True)
    sp = (1.0, 1.0, 1.0)
    n = args.size
    rows = []
    for name, lab in (("blobs", blobs(n, 1, 0.0, dev)), ("cartilage", cartilage(n, dev))):
        cnt = torch.empty(1, dtype=torch.int64, device=dev)
        for cls in range(1, K):
            d2 = T._interior(lab, cls, sp, cnt)
            nvox = int(cnt.item())
            r2 = T._cover(d2, sp)
            dmax, rmean = float(d2.max()), float((2.0 * r2[r2 > 0].double().sqrt()).mean()) if nvox else float("nan")
            print(f"{name} {n}^3 class {cls}: {nvox} voxels, largest interior distance {dmax ** 0.5:.2f}, mean "
                  f"thickness {rmean:.2f}", flush=True)
            scipy_s = None
            if ndi is not None:
                import numpy as np
                mask = np.pad((lab == cls).cpu().numpy(), 1, constant_values=False)
                t0 = time.perf_counter()
                want = ndi.distance_transform_edt(mask)
                scipy_s = time.perf_counter() - t0
                same = np.array_equal(d2.cpu().numpy(), np.round(want[1:-1, 1:-1, 1:-1] ** 2).astype(np.float32))
                print(f"{name} {n}^3 class {cls}: interior transform equals scipy's squared distances: {same}",
                      flush=True)
                if not same:
                    sys.exit("the interior transform differs from scipy's: nothing to time")
                del want, mask
            r = {"phantom": name, "size": n, "class": cls, "voxels": nvox, "d_max": dmax ** 0.5, "scipy_s": scipy_s}
            r["surface_edt"] = timed(lambda: S._edt(lab, cls, sp, cnt), 10, args.repeats)
            r["interior"] = timed(lambda: T._interior(lab, cls, sp, cnt), 10, args.repeats)
            r["cover"] = timed(lambda: T._cover(d2, sp), 5, args.repeats)
            if args.kernels:
                try:
                    from torch.profiler import ProfilerActivity, profile
                    with profile(activities=[ProfilerActivity.CUDA]) as prof:
                        T._cover(T._interior(lab, cls, sp, cnt), sp)
                        torch.cuda.synchronize()
                    r["kernels"] = {}
                    for ev in prof.events():
                        t = ev.device_time if hasattr(ev, "device_time") else ev.cuda_time
                        if t and ("kernel" in ev.name or "emset" in ev.name):
                            r["kernels"].setdefault(ev.name, []).append(float(t))
                except Exception as e:   # the profiler is an extra: the timings above stand without it
                    r["kernels"] = f"not available ({type(e).__name__}: {e})"
            rows.append(r)
            for k in ("surface_edt", "interior", "cover"):
                e = r[k]
                print(f"{name} {n}^3 class {cls} {k:12s} {e['us']:10.1f} us  ({e['us_min']:.1f}..{e['us_max']:.1f})"
                      + (f"   scipy {scipy_s:.2f} s" if scipy_s and k == "interior" else ""), flush=True)
            if isinstance(r.get("kernels"), dict):
                for kn, ts in r["kernels"].items():
                    print(f"{name} {n}^3 class {cls}   kernel {kn[:60]:60s} " + " ".join(f"{t:9.1f}" for t in ts)
                          + " us")
            elif args.kernels:
                print(f"{name} {n}^3 class {cls}   kernels: {r['kernels']}")
            del d2, r2
        r = {"phantom": name, "size": n, "class": "1..2"}
        r["thickness"] = timed(lambda: T.local_thickness(lab, K, sp), 3, args.repeats)
        rows.append(r)
        e = r["thickness"]
        print(f"{name} {n}^3 thickness (K = {K}, both classes) {e['us']:10.1f} us  ({e['us_min']:.1f}..{e['us_max']:.1f})",
              flush=True)
        del lab
        torch.cuda.empty_cache()
    if args.json:
        with open(args.json, "w") as f:
            json.dump(rows, f, indent=1)


if __name__ == "__main__":
    main()
