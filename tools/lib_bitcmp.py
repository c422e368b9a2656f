"""Bit-for-bit comparison of two builds on model steps.  Either two libraries in this tree — the release
library (libpmunet_hip.so) against another one selected by --other (default "prev": a previous
revision's release build, e.g. built from a `git worktree` of HEAD into pmu_hip/libpmunet_hip_prev.so) —
or, with --other-root DIR, this tree against another checkout with its own built library (a `git
worktree` of the parent commit): the check for a host-side change meant to launch the same kernels with
the same arguments.  Both children then inherit PMU_LIB and the engine's PMU_* switches from the
environment.

Each side runs in its own child process on the same seeded models and inputs: UNet training steps under
autocast (bf16) and in fp32 at geometries whose levels take every route of the dispatch (LDS-DMA / raw /
fused bf16, F(2x2) / F(4x4) / fused Winograd, F.pad geometry, odd channel counts), an eval-mode forward
in each precision, Probabilistic U-Net training steps with injected posterior noise, and direct calls of
pmu_fcomb_fwd, pmu_fcomb_stats and pmu_fcomb_bwd on the problems of tests/test_fcomb_abi_gpu.py and
tests/test_fcomb_stats_gpu.py and at one shape of the trainer's widths (F = 32, K = 3, three hidden layers)
large enough that a wave walks several 32-pixel groups and crosses image boundaries.  Per case a
child records every output, gradient and buffer, the launch trace (entry name, its integer / float
arguments and each frame argument's non-pointer fields) and the peak allocated device memory.  Prints
one line per case and exits 1 unless all tensors have equal bit patterns, the traces are identical and the
peaks equal (a differing peak is printed with the peak of the bytes requested, which leaves out the
allocator's block rounding).  A change that resizes a workspace on purpose (pmu_fcomb_bwd_ws) therefore shows
as DIFFER in the byte-count argument of that entry's trace line and in the peaks of the cases that allocate
it; the tool does not judge a direction, the reader compares the printed sizes with the formula.
A change meant to move no bits (scheduling, addressing, layouts, host refactors) is checked with this
before it is measured.

usage: python tools/lib_bitcmp.py [--other prev | --other-root DIR]"""
import argparse
import os
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

CHILD = r'''
import ctypes, gc, sys, torch
sys.path[:0] = [sys.argv[2], sys.argv[2] + "/probabilistic-multiplanar-unet_amd"]
from model import ProbabilisticUnet, UNet
from pmu_hip import _lib as L
dev = torch.device("cuda")
out = {}
SIG = {**L.SIGNATURES, **L.EXP_SIGNATURES}
NUM = (ctypes.c_int, ctypes.c_longlong, ctypes.c_size_t, ctypes.c_float, ctypes.c_double)
trace = []


def observe(name, args, e0, e1):
    rec = [name]
    for t, a in zip(SIG[name][1], args):
        if t in NUM:
            rec.append(repr(a))
        elif t is L._FP:
            f = a._obj
            rec.append("frame(%d,%d,%d,%d;%s)" % (f.nsrc, f.N, f.H, f.W, ";".join(
                ",".join(str(getattr(f.src[i], k)) for k in ("mode", "pool", "C", "H", "W", "off_h", "off_w", "dtype"))
                for i in range(f.nsrc))))
    trace.append(" ".join(rec))


def observed(name, fn):
    gc.collect()
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    del trace[:]
    L.set_call_observer(observe)
    try:
        res = fn()
        torch.cuda.synchronize()
    finally:
        L.set_call_observer(None)
    out[name + "/trace"] = list(trace)
    out[name + "/peak"] = torch.cuda.max_memory_allocated()
    # (what was asked of the allocator, without its block rounding: printed beside a differing peak)
    out[name + "/peak_requested"] = torch.cuda.memory_stats().get("requested_bytes.all.peak", -1)
    return res


def direct(name, fn):   # a case of direct library calls: fn returns {name: tensor}
    for k, v in observed(name, fn).items():
        out[name + "/" + k] = v.cpu()


def case(name, fn):
    net, y = observed(name, fn)
    out[name + "/out"] = y.float().cpu()
    for k, p in net.named_parameters():
        if p.grad is not None:
            out[name + "/grad/" + k] = p.grad.cpu()
    for k, b in net.named_buffers():
        out[name + "/buf/" + k] = b.cpu()


def unet_step(bf16, ch, cl, filters, N, H, W, train=True):
    def fn():
        torch.manual_seed(0)
        net = UNet(ch, cl, filters).to(dev).train(train)
        g = torch.Generator().manual_seed(8)
        x = torch.rand(N, ch, H, W, generator=g).to(dev)
        r = torch.randn(N, cl, H, W, generator=g).to(dev)
        with torch.set_grad_enabled(train), torch.autocast("cuda", dtype=torch.bfloat16, enabled=bf16):
            y = net(x)
        if train:
            (y.float() * r).sum().backward()
        return net, y.detach()
    return fn


def prob_step(filters, H):
    def fn():   # one training step with injected posterior noise (__graft_entry__.smoke's recipe)
        torch.manual_seed(0)
        net = ProbabilisticUnet(1, 3, filters, latent_dim=6, no_convs_fcomb=4, beta=10.0).to(dev).train()
        g = torch.Generator().manual_seed(2)
        x = torch.rand(2, 1, H, H, generator=g).to(dev)
        segm = torch.randint(0, 3, (2, 1, H, H), generator=g).float().to(dev)
        eps = torch.randn(2, 6, generator=g).to(dev)
        net.forward(x, segm, training=True)
        d = net.posterior_latent_space
        d.rsample = lambda sample_shape=torch.Size(): d.base_dist.loc + d.base_dist.scale * eps
        loss = -net.elbo(segm)
        loss.backward()
        return net, loss.detach().reshape(1)
    return fn


big = [64, 128, 256, 512, 1024]
case("c5_bf16", unet_step(True, 3, 3, big, 4, 128, 128))
case("c2_fp32", unet_step(False, 1, 1, big, 4, 128, 128))
# (model.UNet needs doubling filters — the concat of skip and up-sampled halves must match the Up block's
# conv — so the channel counts off the 16- and 8-channel grids come as [24, 48] and [12, 24])
case("fp32_24_48", unet_step(False, 1, 1, [24, 48], 2, 72, 40))
case("fp32_16_32_64", unet_step(False, 1, 1, [16, 32, 64], 2, 48, 48))
case("bf16_16_32_64", unet_step(True, 3, 3, [16, 32, 64], 2, 64, 64))
case("bf16_64_128_256", unet_step(True, 3, 3, [64, 128, 256], 2, 64, 48))
case("bf16_12_24", unet_step(True, 3, 3, [12, 24], 2, 40, 40))
case("fp32_5ch_12_24", unet_step(False, 5, 1, [12, 24], 2, 40, 40))
case("fp32_pad", unet_step(False, 1, 1, [16, 32, 64], 2, 50, 46))
case("bf16_pad", unet_step(True, 1, 1, [16, 32, 64], 2, 50, 46))
case("fp32_eval", unet_step(False, 1, 1, [16, 32, 64], 2, 48, 48, train=False))
case("bf16_eval", unet_step(True, 3, 3, [16, 32, 64], 2, 64, 64, train=False))
case("prob_4_8_16", prob_step([4, 8, 16], 32))
case("prob_32_64_128", prob_step([32, 64, 128], 64))


def fcomb_direct(F, K, NH, Lz, N, H, W, S, w, b, wl, bl, feat, z, dl):
    def fn():   # pmu_fcomb_fwd and pmu_fcomb_stats over the S samples, pmu_fcomb_bwd of one of them
        p3 = lambda ts: (ctypes.c_void_p * 3)(*([t.data_ptr() for t in ts] + [None] * (3 - len(ts))))
        zb = (torch.einsum("ol,snl->sno", w[0][:, F:].double(), z.double()) + b[0].double()).float().to(dev)
        wd, bd, wld, bld, fd, dld = [t.to(dev) for t in w], [t.to(dev) for t in b], wl.to(dev), bl.to(dev), feat.to(dev), dl.to(dev)
        zd = z.to(dev) if Lz else torch.zeros(S, 1, device=dev)
        wargs = (p3(wd), p3(bd), wld.data_ptr(), bld.data_ptr(), F, Lz, K, NH)
        nan = lambda *s: torch.full(s, float("nan"), device=dev)
        r = dict(y=nan(S, N, K, H, W), mean=nan(N, K, H, W), entropy=nan(N, H, W), mi=nan(N, H, W),
                 label=torch.full((N, H, W), -1, dtype=torch.int32, device=dev),
                 labels=torch.full((S, N, H, W), 0xFF, dtype=torch.uint8, device=dev),
                 dfeat=nan(N, H, W, F), dz=nan(N, max(Lz, 1)), dwl=nan(K, F), dbl=nan(K))
        dw, db = [nan(*t.shape) for t in w], [nan(*t.shape) for t in b]
        r.update({f"dw{l}": t for l, t in enumerate(dw)}, **{f"db{l}": t for l, t in enumerate(db)})
        s = L.stream()
        L.call("pmu_fcomb_fwd", fd.data_ptr(), zb.data_ptr(), *wargs, S, N, H, W, r["y"].data_ptr(), s)
        L.call("pmu_fcomb_stats", fd.data_ptr(), zb.data_ptr(), *wargs, S, N, H, W, r["mean"].data_ptr(),
               r["entropy"].data_ptr(), r["mi"].data_ptr(), r["label"].data_ptr(), r["labels"].data_ptr(), s)
        sb = min(1, S - 1)
        wsb = L.lib().pmu_fcomb_bwd_ws(N, H, W)
        ws = torch.empty(wsb // 4, device=dev)
        L.call("pmu_fcomb_bwd", fd.data_ptr(), zd[sb].contiguous().data_ptr(), zb[sb].data_ptr(), dld.data_ptr(), *wargs,
               N, H, W, r["dfeat"].data_ptr(), r["dz"].data_ptr(), p3(dw), p3(db), r["dwl"].data_ptr(),
               r["dbl"].data_ptr(), ws.data_ptr(), wsb, s)
        return r
    return fn


# the direct-call shapes of the Fcomb tests (their quantised problems), then one at the trainer's widths whose
# 264 455 pixels make 8 265 groups: the forward's 2 048 waves walk four or five of them each, and a backward
# wave's nine consecutive groups cross image boundaries (52 891 pixels per image: no multiple of 32)
sys.path.insert(0, sys.argv[2] + "/tests")
import test_fcomb_abi_gpu as TA, test_fcomb_stats_gpu as TS
for c in TA.CASES:
    direct("fcomb_abi_" + "_".join(map(str, c)), fcomb_direct(*c, TA.S, *TA._problem(*c)))
for c in TS.CASES:
    dl = torch.randn(c[4], c[1], c[5], c[6], generator=torch.Generator().manual_seed(5))
    direct("fcomb_stats_" + "_".join(map(str, c)), fcomb_direct(*c, *TS._problem(*c), dl))
F, K, NH, Lz, N, H, W, S = 32, 3, 3, 6, 5, 233, 227, 4
g = torch.Generator().manual_seed(9)
rn = lambda *s: torch.randn(*s, generator=g)
direct("fcomb_32_3_3_5x233x227", fcomb_direct(
    F, K, NH, Lz, N, H, W, S, [rn(F, F + Lz if l == 0 else F) / 6 for l in range(NH)], [rn(F) / 4 for _ in range(NH)],
    rn(K, F), rn(K), torch.relu(rn(N, H, W, F)), rn(S, N, Lz), rn(N, K, H, W)))
torch.save(out, sys.argv[1])
'''


def same_bits(x, y):
    """Equal shape, dtype and bit pattern: a NaN left in an output that a call does not write (dz of a case
    without latent columns) equals itself, and -0.0 does not equal 0.0."""
    import torch
    return (x.shape == y.shape and x.dtype == y.dtype and
            torch.equal(x.contiguous().reshape(-1).view(torch.uint8), y.contiguous().reshape(-1).view(torch.uint8)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--other", default="prev", help="PMU_LIB of the second child (two libraries of this tree)")
    ap.add_argument("--other-root", default=None,
                    help="another checkout with its own built library: the second child imports from it, and both "
                         "children inherit PMU_LIB from the environment")
    args = ap.parse_args()
    import torch
    if args.other_root:
        sides = [("this", ROOT, dict(os.environ)), ("other", os.path.abspath(args.other_root), dict(os.environ))]
    else:
        sides = [("release", ROOT, dict(os.environ, PMU_LIB="")), (args.other, ROOT, dict(os.environ, PMU_LIB=args.other))]
    res = []
    with tempfile.TemporaryDirectory() as td:
        for tag, root, env in sides:
            path = os.path.join(td, f"out_{tag}.pt")
            r = subprocess.run([sys.executable, "-c", CHILD, path, root], env=env, capture_output=True, text=True,
                               timeout=600)
            if r.returncode != 0:
                print(r.stderr[-3000:])
                return 2
            res.append(torch.load(path, weights_only=True))
    a, b = res
    ok = set(a) == set(b)
    for c in sorted({k.split("/")[0] for k in a}):
        keys = [k for k in a if k.startswith(c + "/") and k.split("/")[1] not in ("trace", "peak", "peak_requested")]
        bad = [k for k in keys if k not in b or not same_bits(a[k], b[k])]
        ta, tb = a[c + "/trace"], b.get(c + "/trace", [])
        at = next((i for i, (u, v) in enumerate(zip(ta, tb)) if u != v), None if len(ta) == len(tb) else min(len(ta), len(tb)))
        pa, pb = a[c + "/peak"], b.get(c + "/peak")
        print(f"{c}: {len(keys)} tensors, {len(bad)} differ" + (f" (first: {bad[:3]})" if bad else "") +
              f"; {len(ta)} launches, trace " +
              ("identical" if at is None else f"differs at {at}: {ta[at:at + 1]} vs {tb[at:at + 1]}") +
              f"; peak {pa} vs {pb} bytes" +
              ("" if pa == pb else f" (requested {a[c + '/peak_requested']} vs {b.get(c + '/peak_requested')})"))
        ok = ok and not bad and at is None and pa == pb
    print("BITCMP", "OK" if ok else "DIFFER")
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
