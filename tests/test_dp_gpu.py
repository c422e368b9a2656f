"""Row e on the GPU: the backward-overlapped bucket all-reduce (pmu_hip.dp) around the real HIP
backward, rehearsed with 2 ranks sharing cuda:0 over gloo (tools/dp_check.py; RCCL needs one
device per rank, the driver's multi-GPU bench runs it over RCCL).  Launched as a child process."""
import os
import socket
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    return port


def _dp_check(backend, nproc, *args):
    """One launch of tools/dp_check.py under torch.distributed.run: (return code, output)."""
    env = dict(os.environ, PMU_DIST_BACKEND=backend)
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", str(nproc),
           "--master-addr", "127.0.0.1", "--master-port", str(_free_port()),
           os.path.join(ROOT, "tools", "dp_check.py"), *args]
    r = subprocess.run(cmd, cwd=ROOT, env=env, capture_output=True, text=True, timeout=300)
    return r.returncode, r.stdout + r.stderr


def _delayed_iterations_shown(out, ranks):
    """Every rank ran the three delayed iterations, and each shows condition B for its stream: a bucket
    with a member produced on the delayed stream was issued from a flush on another stream."""
    for rank in range(ranks):
        for it, stream in ((3, "main"), (4, "side1"), (5, "side2")):
            assert f"rank {rank} iter {it} [delay {stream} " in out, (rank, stream, out[-6000:])
            assert f"rank {rank} iter {it}: condition B stream {stream}: OK" in out, (rank, stream, out[-6000:])


@pytest.mark.gpu
def test_bucketed_allreduce_overlapped_with_hip_backward():
    rc, out = _dp_check("gloo", 2)
    assert rc == 0 and "DP_CHECK gloo world 2 OK" in out, out[-4000:]


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
def test_bucketed_allreduce_probunet_streams_gloo2(dtype):
    """The Probabilistic U-Net's three parts run their backwards on three streams and write one flat
    buffer, so a bucket can hold gradients of two streams.  Two gloo ranks, a fresh batch per iteration,
    and one iteration per stream in which that stream is held back behind a bounded busy kernel: the
    synchronised gradient equals the sum of the ranks' local gradients bit for bit only if every bucket's
    all-reduce waits for all the streams that produced its members.

    The backward visits Fcomb (main), the posterior (side2), the prior (side1) and the UNet (main), so at
    64 KiB bucket 0 holds main + side2 and goes out on side2, bucket 3 side2 + side1 on side1, bucket 6
    side1 + main on main: one bucket per delayed stream that is issued from another stream."""
    rc, out = _dp_check("gloo", 2, "--model", "probunet", "--delay", *(["--bf16"] if dtype == "bf16" else []))
    assert rc == 0 and f"DP_CHECK gloo world 2 OK model probunet dtype {dtype} delay on" in out, out[-6000:]
    _delayed_iterations_shown(out, 2)


@pytest.mark.gpu
def test_bucketed_allreduce_unet_bf16_gloo2():
    """Bucketed all-reduce around a backward whose forward ran under torch.autocast(bfloat16)."""
    rc, out = _dp_check("gloo", 2, "--model", "unet", "--bf16")
    assert rc == 0 and "DP_CHECK gloo world 2 OK model unet dtype bf16 delay off" in out, out[-4000:]


@pytest.mark.gpu
def test_bucketed_allreduce_probunet_rccl_one_rank():
    """The delayed three-stream check over RCCL with the one rank a single GPU allows.  One rank's sum is
    the identity, so this says nothing about the ordering of a bucket behind its producers; it shows that
    the reducer's stream waits coexist with RCCL's own stream and the learned bucket layout."""
    rc, out = _dp_check("nccl", 1, "--model", "probunet", "--delay")
    assert rc == 0 and "DP_CHECK nccl world 1 OK model probunet dtype fp32 delay on" in out, out[-6000:]
    _delayed_iterations_shown(out, 1)


@pytest.mark.gpu
def test_bucketed_allreduce_over_rccl_one_rank():
    """The same check over RCCL (backend nccl) with the one rank this box's single GPU allows: the RCCL
    communicator, the bucket all-reduces issued from inside the HIP backward on RCCL's stream behind the
    compute stream's events, and the learned bucket layout; the synchronised gradient equals the local one
    bit for bit."""
    rc, out = _dp_check("nccl", 1)
    assert rc == 0 and "DP_CHECK nccl world 1 OK" in out, out[-4000:]


@pytest.mark.gpu
def test_bench_gpus_2_launches_two_ranks():
    """bench.py --gpus 2 outside torchrun starts 2 ranks itself and the line reports the
    whole job: n_gpus 2, global batch 64, dp2.  Rehearsed on the 1-GPU box over gloo (both ranks on
    cuda:0); the driver's N-GPU node runs the same path over RCCL."""
    import json
    env = dict(os.environ, PMU_DIST_BACKEND="gloo")
    for k in ("WORLD_SIZE", "RANK", "LOCAL_RANK"):
        env.pop(k, None)
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "2", "--steps", "2", "--warmup", "1",
           "--no-cpu-baseline", "--no-kernel-timing"]
    r = subprocess.run(cmd, cwd=ROOT, env=env, capture_output=True, text=True, timeout=400)
    assert r.returncode == 0, (r.stdout + r.stderr)[-4000:]
    lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, r.stdout[-4000:]
    res = json.loads(lines[0])
    assert res["n_gpus"] == 2 and res["config"]["global_batch"] == 64 and res["config"]["parallelism"] == "dp2"
    assert res["value"] > 0 and res["steps"] == 2
    # the line records its topology: gloo, 2 ranks, each rank's GPU identity (both cuda:0 on this box)
    d = res["dist"]
    assert d["backend"] == "gloo" and d["world"] == 2 and len(d["devices"]) == 2, d


@pytest.mark.gpu
def test_bench_refuses_two_rccl_ranks_on_one_gpu():
    """The same launch over RCCL on a box with one GPU: each rank exits 2 before forming a process group
    (two RCCL ranks on one device would time one GPU as two), and no JSON line is printed."""
    import torch
    if torch.cuda.device_count() >= 2:
        pytest.skip("more than one GPU visible")
    env = dict(os.environ, PMU_DIST_BACKEND="nccl")
    for k in ("WORLD_SIZE", "RANK", "LOCAL_RANK"):
        env.pop(k, None)
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "2", "--steps", "1", "--warmup", "0",
           "--no-cpu-baseline", "--no-kernel-timing"]
    r = subprocess.run(cmd, cwd=ROOT, env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode != 0, (r.stdout + r.stderr)[-4000:]
    assert "RCCL ranks but 1 visible GPU" in r.stderr, r.stderr[-4000:]
    assert not [l for l in r.stdout.splitlines() if l.startswith("{")]
