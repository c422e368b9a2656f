"""Rehearsal of the overlapped data-parallel step on ONE GPU (row e): N ranks share cuda:0 over gloo.

Each rank runs the HIP forward/backward of a small network on a fresh batch per iteration twice: once
alone (its local gradient: no reducer attached, the Probabilistic U-Net's parts on one stream) and once
with pmu_hip.dp.BucketAllReduce issuing the bucket all-reduces from inside the backward.  The
synchronised gradient must equal the sum of all ranks' local gradients (all-gathered) bit for bit, on
every rank.  Between the two passes the flat gradient buffer is zeroed, so a bucket that is reduced
before its gradient kernels have run sums zeros and the check fails.

  --model unet|probunet   the UNet of the bench's small filters, or the G3 Probabilistic U-Net, whose
                          UNet, prior and posterior run on three streams (functions.run_concurrent) and
                          write one flat buffer; its step is ProbUNetTrainer's (forward, a prior sample
                          that is dropped, -elbo with a fixed posterior draw)
  --bf16                  forward and loss under torch.autocast("cuda", dtype=torch.bfloat16)
  --delay                 (probunet) after two plain iterations on the learned bucket layout, one
                          iteration per producing stream in which a bounded busy kernel holds that stream
                          back from sync.begin() on, for 3x the begin->finish time of a plain iteration (the
                          shorter of the two; more than 0.5 s fails the run):
                          its gradient kernels run only after the other streams' flushes have issued
                          their buckets, so a bucket issued without waiting for every producing stream
                          is reduced too early, every time
  --bucket-bytes N        bucket size (default 65536)

Launch:

  PMU_DIST_BACKEND=gloo python -m torch.distributed.run --nproc-per-node 2 --master-addr 127.0.0.1 \
      --master-port 29533 tools/dp_check.py [--model probunet] [--bf16] [--delay]

The last line is ``DP_CHECK <backend> world <n> OK|FAIL model <m> dtype <fp32|bf16> delay <on|off>``;
the exit status follows it.
"""
import argparse
import contextlib
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "probabilistic-multiplanar-unet_amd"))

import torch  # noqa: E402
import torch.distributed as dist  # noqa: E402

MAX_DELAY_S = 0.5     # a longer delay means the net is too large for this check: shrink the net
CAL_CYCLES = 10_000_000


def _sleep_cycles_per_s(dev):
    """torch.cuda._sleep's cycle counter in cycles per second, from one timed call."""
    torch.cuda._sleep(1000)
    torch.cuda.synchronize(dev)
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    torch.cuda._sleep(CAL_CYCLES)
    b.record()
    torch.cuda.synchronize(dev)
    return CAL_CYCLES / (a.elapsed_time(b) * 1e-3)


def _matmul_rate(dev):
    """Fallback busy kernel: (matrices, seconds per 2048^3 matmul)."""
    m = torch.rand(2048, 2048, device=dev) * 1e-3
    torch.mm(m, m)
    torch.cuda.synchronize(dev)
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(8):
        torch.mm(m, m)
    b.record()
    torch.cuda.synchronize(dev)
    return m, a.elapsed_time(b) * 1e-3 / 8


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--model", choices=("unet", "probunet"), default="unet")
    ap.add_argument("--bf16", action="store_true")
    ap.add_argument("--delay", action="store_true")
    ap.add_argument("--bucket-bytes", type=int, default=64 << 10)
    args = ap.parse_args()
    if args.delay and args.model != "probunet":
        ap.error("--delay needs --model probunet (a plain UNet runs on one stream)")
    prob = args.model == "probunet"
    world = int(os.environ["WORLD_SIZE"])
    rank = int(os.environ["RANK"])
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    # gloo: N ranks sharing cuda:0; nccl (RCCL): one rank per device, so on a 1-GPU box world 1 — the
    # real RCCL communicator and collectives under the overlapped buckets
    backend = os.environ.get("PMU_DIST_BACKEND", "gloo")
    if backend == "nccl":
        dist.init_process_group("nccl", rank=rank, world_size=world, device_id=dev)
    else:
        dist.init_process_group(backend, rank=rank, world_size=world)
    cdev = dev if backend == "nccl" else torch.device("cpu")   # RCCL collectives take device tensors
    from model import ProbabilisticUnet, UNet
    from pmu_hip import functions
    from pmu_hip.dp import BucketAllReduce
    from pmu_hip.engine import CFG, unet_report_order
    torch.manual_seed(0)
    if prob:
        net = ProbabilisticUnet(1, 3, [4, 8, 16, 32, 64], latent_dim=6, no_convs_fcomb=4, beta=10.0).to(dev).train()
        no_grad_expected = {"unet.outc." + k for k, _ in net.unet.outc.named_parameters()}
    else:
        net = UNet(1, 2, [16, 32, 64]).to(dev).train()
        no_grad_expected = set()
    named = list(net.named_parameters())
    plist = [p for _, p in named]
    crit = torch.nn.CrossEntropyLoss()
    precision = (lambda: torch.autocast("cuda", dtype=torch.bfloat16)) if args.bf16 else contextlib.nullcontext

    def batch(it):
        """Iteration ``it``'s batch of this rank: generator seeded with (100 + rank, it)."""
        g = torch.Generator().manual_seed((100 + rank) * 1_000_003 + it)
        x = torch.rand(4, 1, 64, 64, generator=g).to(dev)
        if prob:
            m = torch.randint(0, 3, (4, 1, 64, 64), generator=g).float().to(dev)
            return x, m, torch.randn(4, 6, generator=g).to(dev)
        return x, torch.randint(0, 2, (4, 64, 64), generator=g).to(dev), None

    def loss_of(x, m, eps):
        with precision():
            if not prob:
                return crit(net(x), m)
            # ProbUNetTrainer.predict + .loss (train.py's step): the prediction's graph is dropped
            net.forward(x, m, training=True)
            pred = net.sample(testing=False)
            del pred
            d = net.posterior_latent_space     # a fixed posterior draw: what Normal.rsample computes for eps
            d.rsample = lambda sample_shape=torch.Size(): d.base_dist.loc + d.base_dist.scale * eps
            return -net.elbo(m)

    def grads():
        have = [(n, p) for n, p in named if p.grad is not None]
        return have, {n for n, p in named if p.grad is None}

    sync = BucketAllReduce(net, bucket_bytes=args.bucket_bytes)
    hook = net.__dict__["_pmu_grad_ready"]
    # the backward's real report order and streams, seen through the reducer's flush callback
    reports = []      # per flush: (param ids, stream, buckets it issued)

    def ready(ps, flat=True):
        before = sync.next if sync.active and sync.buckets is not None else None
        cur = torch.cuda.current_stream(dev)
        at = torch.cuda.Event(enable_timing=True)    # where this stream stands when the flush arrives
        at.record(cur)
        hook(ps, flat)
        out = list(range(before, sync.next)) if before is not None else []
        reports.append(([id(p) for p in ps], cur, out, at))

    buf_zero = lambda: net.__dict__["_pmu_grad_flat"].zero_()   # noqa: E731
    plan = [None, None, None]       # the stream each iteration delays (None: a plain iteration)
    if args.delay:
        plan += [0, 1, 2]
    names = ["main", "side1", "side2"]
    plain_s, rate, mm = None, None, None
    ok = True
    for it, delayed in enumerate(plan):
        x, m, eps = batch(it)
        # ---- this rank's local gradient: no reducer attached, the parts on one stream
        net.__dict__.pop("_pmu_grad_ready")
        prev, CFG.prob_streams = CFG.prob_streams, False
        for p in plist:
            p.grad = None
        loss_of(x, m, eps).backward()
        CFG.prob_streams = prev
        have, none_local = grads()
        local = torch.cat([p.grad.reshape(-1) for _, p in have]).to(cdev)
        allg = [torch.empty_like(local) for _ in range(world)]
        dist.all_gather(allg, local)
        want = allg[0].clone()
        for a in allg[1:]:
            want += a
        want = want.cpu()
        for p in plist:
            p.grad = None
        buf_zero()      # a slot read before its kernel has run must not find this batch's gradient
        net.__dict__["_pmu_grad_ready"] = ready
        # ---- the same batch with the reducer
        reports.clear()
        loss = loss_of(x, m, eps)
        streams = functions.last_streams() if prob else [torch.cuda.current_stream(dev)]
        label = lambda s: names[streams.index(s)] if s in streams else str(s)   # noqa: E731
        delay_s, ev = 0.0, None
        if delayed is not None:
            delay_s = 3.0 * plain_s
            if delay_s > MAX_DELAY_S:   # fails the run; the iteration still runs (the ranks stay in step)
                print(f"rank {rank} iter {it}: delay {delay_s:.3f} s > {MAX_DELAY_S} s: the net is too large", flush=True)
                ok, delay_s = False, MAX_DELAY_S
            if rate is None and mm is None:
                if hasattr(torch.cuda, "_sleep"):
                    rate = _sleep_cycles_per_s(dev)
                else:
                    mm = _matmul_rate(dev)
        torch.cuda.synchronize(dev)
        t0 = time.perf_counter()
        sync.begin()
        if delayed is not None:
            ev = (torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True))
            with torch.cuda.stream(streams[delayed]):
                ev[0].record()
                if rate is not None:
                    torch.cuda._sleep(int(delay_s * rate))
                else:
                    for _ in range(max(1, int(delay_s / mm[1]))):
                        torch.mm(mm[0], mm[0])
                ev[1].record()
        loss.backward()
        issued, first, flushes = sync.issued_in_backward, (sync.issued_at or [None])[0], sync.flushes
        sync.finish()
        torch.cuda.synchronize(dev)
        step_s = time.perf_counter() - t0
        if delayed is None and it > 0:   # the learned layout; the shortest, so that a stall does not set the delay
            plain_s = step_s if plain_s is None else min(plain_s, step_s)
        have, none_sync = grads()
        got = torch.cat([p.grad.reshape(-1) for _, p in have]).cpu()
        err = (got - want).abs().max().item() if got.shape == want.shape else float("inf")
        none_ok = none_local == none_sync == no_grad_expected
        buf = net.__dict__["_pmu_grad_flat"]
        adopted = all(buf.data_ptr() <= p.grad.data_ptr() < buf.data_ptr() + 4 * buf.numel() for _, p in have)
        seen = [r[0] for r in reports]
        if prob:    # the order the layout was learned from holds in every later backward
            learned = [id(p) for p in net.__dict__.get("_pmu_dp_order", [])]
            order_ok = it == 0 or [i for ids in seen for i in ids] == learned
        else:
            order_ok = seen == [[id(p) for p in grp] for grp in unet_report_order(net)]
        nb = len(sync.buckets)
        what = "plain" if delayed is None else f"delay {names[delayed]} {delay_s * 1e3:.1f} ms (ran {ev[0].elapsed_time(ev[1]):.1f} ms)"
        lines = [f"rank {rank} iter {it} [{what}]: begin->finish {step_s * 1e3:.1f} ms buckets {nb} issued in backward "
                 f"{issued} (bucket 0 at flush {first} of {flushes}) max|sync - sum(local)| {err:.3e} adopted {adopted} "
                 f"no-grad set {none_ok} report order {order_ok}"]
        ok = ok and err == 0.0 and adopted and order_ok and none_ok
        if it > 0:   # condition A, the learned layout: every bucket from inside the backward, bucket 0 early
            ok = ok and issued == nb and nb > 2 and first is not None and first < flushes // 2
            producers, issuer, reached = [set() for _ in range(nb)], [None] * nb, [None] * nb
            for ids, s, out, at in reports:
                for i in ids:
                    b = sync.bucket_of.get(i)
                    if b is not None:
                        producers[b].add(s)
                for b in out:
                    issuer[b], reached[b] = s, at
            berr, o = [0.0] * nb, 0
            for _, p in have:
                b = sync.bucket_of.get(id(p))
                if b is not None and got.shape == want.shape:
                    berr[b] = max(berr[b], (got[o:o + p.numel()] - want[o:o + p.numel()]).abs().max().item())
                o += p.numel()
            if delayed is not None or it == 1:
                for b in range(nb):
                    # where the issuing stream stood, against the end of the delay on the delayed stream: a
                    # negative time means the flush arrived while the delayed stream was still held back
                    rel = f" its stream {ev[1].elapsed_time(reached[b]):+.1f} ms from the delay's end" \
                        if ev is not None and reached[b] is not None else ""
                    lines.append(f"  rank {rank} iter {it} bucket {b}: produced on {sorted(label(s) for s in producers[b])} "
                                 f"issued on {label(issuer[b]) if issuer[b] is not None else 'finish'}{rel} err {berr[b]:.3e}")
            if delayed is not None:
                # condition B: a bucket with a member produced on the delayed stream goes out from a
                # flush on another stream — the case a missing wait gets wrong
                s = streams[delayed]
                hit = [b for b in range(nb) if s in producers[b] and issuer[b] is not None and issuer[b] != s]
                lines.append(f"rank {rank} iter {it}: condition B stream {names[delayed]}: "
                             f"{'OK buckets ' + str(hit) if hit else 'MISSING'}")
                ok = ok and bool(hit)
        print("\n".join(lines), flush=True)
    flag = torch.tensor([1 if ok else 0], device=cdev)
    dist.all_reduce(flag, op=dist.ReduceOp.MIN)
    if rank == 0:
        print("DP_CHECK", backend, "world", world, "OK" if flag.item() == 1 else "FAIL", "model", args.model,
              "dtype", "bf16" if args.bf16 else "fp32", "delay", "on" if args.delay else "off", flush=True)
    dist.destroy_process_group()
    sys.exit(0 if flag.item() == 1 else 1)


if __name__ == "__main__":
    main()
