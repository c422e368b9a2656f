"""CPU-only checks: oracle vs the reference's golden vectors, drop-in surface, C ABI exports.

No GPU compute here: the library is loaded and its symbols resolved, nothing is launched.
"""
import os
import re

import numpy as np
import pytest
import torch

from helpers import ACT_TOL, GRAD_TOL, LOSS_RTOL, grad_err, max_abs

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def _load(name):
    return np.load(os.path.join(GOLD, name), allow_pickle=False)


def _sd(z, prefix):
    pre = prefix + "/"
    return {k[len(pre):]: torch.from_numpy(np.array(z[k])) for k in z.files if k.startswith(pre)}


# ----------------------------------------------------------------------------- oracle pinning
def test_oracle_matches_reference_g1_step():
    """G1 (config c1): one train step of UNet(1,1,[16,32]) — outputs, loss, grads, BN stats."""
    from oracle.unet_ref import unet_forward, unet_loss, unet_param_keys
    z = _load("g1_unet_c1.npz")
    sd = _sd(z, "init")
    x, t = torch.from_numpy(z["x0"]), torch.from_numpy(z["t0"])
    keys = unet_param_keys(sd)
    params = {k: sd[k].clone().requires_grad_(True) for k in keys}
    work = dict(sd)
    work.update(params)
    y = unet_forward(work, x, 2, 1)
    loss = unet_loss(y, t, 1)
    loss.backward()
    assert max_abs(y, torch.from_numpy(z["y0"])) <= 1e-6
    assert abs(float(loss) - float(z["loss0"])) <= 1e-6
    gref = _sd(z, "grad0")
    err, key = grad_err({k: params[k].grad for k in keys}, gref)
    assert err <= 1e-5, (err, key)
    after = _sd(z, "after0")
    for k in after:
        if "running" in k:
            assert max_abs(work[k], after[k]) <= 1e-6, k


def test_oracle_matches_reference_g1_ten_steps():
    """G1: params after 10 clip(0.1)+SGD(lr 1e-3, momentum 0.9) steps (train.py:85-110)."""
    from oracle.unet_ref import unet_param_keys, unet_train_step
    z = _load("g1_unet_c1.npz")
    sd = _sd(z, "init")
    bufs = {k: torch.zeros_like(sd[k]) for k in unet_param_keys(sd)}
    losses = []
    for i in range(10):
        _, loss, _ = unet_train_step(sd, torch.from_numpy(z[f"x{i}"]), torch.from_numpy(z[f"t{i}"]), 2, 1,
                                     lr=1e-3, bufs=bufs)
        losses.append(float(loss))
    assert np.allclose(losses, z["losses"], rtol=1e-5, atol=1e-6)
    final = _sd(z, "final")
    for k, v in final.items():
        assert max_abs(sd[k], v) <= 1e-5, k


@pytest.mark.parametrize("tag", ["s64", "s170"])
def test_oracle_matches_reference_g2(tag):
    """G2: all 5 levels at small width, CE loss; 170x170 exercises the F.pad branch."""
    from oracle.unet_ref import unet_forward, unet_loss, unet_param_keys
    z = _load("g2_unet_multiclass.npz")
    sd = _sd(z, f"{tag}/init")
    x, t = torch.from_numpy(z[f"{tag}/x"]), torch.from_numpy(z[f"{tag}/t"])
    keys = unet_param_keys(sd)
    params = {k: sd[k].clone().requires_grad_(True) for k in keys}
    work = dict(sd)
    work.update(params)
    y = unet_forward(work, x, 5, 3)
    loss = unet_loss(y, t, 3)
    loss.backward()
    assert max_abs(y, torch.from_numpy(z[f"{tag}/y"])) <= 1e-5
    assert torch.equal(torch.argmax(torch.softmax(y.detach(), 1), 1), torch.from_numpy(z[f"{tag}/argmax"]))
    assert abs(float(loss) - float(z[f"{tag}/loss"])) <= 1e-5 * abs(float(z[f"{tag}/loss"]))
    err, key = grad_err({k: params[k].grad for k in keys}, _sd(z, f"{tag}/grad"))
    assert err <= 1e-4, (err, key)


def test_oracle_dice_matches_reference_g4():
    from oracle.unet_ref import dice_coeff, trainer_dice
    z = _load("g4_dice.npz")
    for case in ("rand", "empty", "ones", "disjoint"):
        d = dice_coeff(torch.from_numpy(z[f"{case}/pred"]), torch.from_numpy(z[f"{case}/target"]))
        assert float(d) == pytest.approx(float(z[f"{case}/dice"]), abs=1e-7), case
    mc = trainer_dice(torch.from_numpy(z["mc/y"]), torch.from_numpy(z["mc/mask"]), 3)
    assert np.allclose(mc, z["mc/dice"], atol=1e-7)
    b = trainer_dice(torch.from_numpy(z["bin/y"]), torch.from_numpy(z["bin/mask"]), 1)
    assert np.allclose(b, z["bin/dice"], atol=1e-7)


# ----------------------------------------------------------------------------- drop-in surface
def test_unet_state_dict_matches_reference_g1():
    """Same construction order => torch.manual_seed(0) reproduces the reference's weights/keys."""
    from model import UNet
    z = _load("g1_unet_c1.npz")
    ref = _sd(z, "init")
    torch.manual_seed(0)
    sd = UNet(1, 1, [16, 32]).state_dict()
    assert list(sd.keys()) == list(ref.keys())
    for k in ref:
        assert torch.equal(sd[k], ref[k]), k


def test_unet_state_dict_matches_reference_g2():
    from model import UNet
    z = _load("g2_unet_multiclass.npz")
    ref = _sd(z, "s64/init")
    torch.manual_seed(0)
    sd = UNet(1, 3, [4, 8, 16, 32, 64]).state_dict()
    assert list(sd.keys()) == list(ref.keys())
    assert all(torch.equal(sd[k], ref[k]) for k in ref)


def test_unet_default_is_c2_architecture():
    from model import UNet
    net = UNet(1, 1)
    assert net.num_filters == [64, 128, 256, 512, 1024]
    assert sum(p.numel() for p in net.parameters()) == 31042369
    assert len(net.state_dict()) == 136


def test_unet_forward_refuses_cpu():
    """No CPU fallback: the product path must fail loudly without the GPU."""
    from model import UNet
    net = UNet(1, 1, [4, 8])
    with pytest.raises(RuntimeError):
        net(torch.rand(1, 1, 8, 8))


def test_bilinear_up_rejected_like_reference():
    from model import UNet
    with pytest.raises(TypeError):
        UNet(1, 1, [4, 8], bilinear=True)


# ----------------------------------------------------------------------------- C ABI
def _header_functions(path=None):
    from pmu_hip._lib import HEADER_PATH
    src = open(path or HEADER_PATH).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    return sorted(set(re.findall(r"\b(pmu_[A-Za-z0-9_]+)\s*\(", src)))


def test_library_exports_every_header_symbol():
    """The shipped library exports exactly include/pmunet_hip.h (every declaration resolves, the ctypes
    table mirrors it, and none of include/pmunet_hip_experiments.h is exported); the experiments library
    exports both headers."""
    from pmu_hip._lib import EXP_HEADER_PATH, EXP_LIB_PATH, EXP_SIGNATURES, LIB_PATH, SIGNATURES, load_library
    if not os.path.exists(LIB_PATH):
        pytest.skip("libpmunet_hip.so not built (run __graft_entry__.build())")
    cdll = load_library()
    names = _header_functions()
    exp_names = _header_functions(EXP_HEADER_PATH)
    assert len(names) >= 25 and len(exp_names) >= 10
    assert not set(names) & set(exp_names)
    for n in names:
        assert hasattr(cdll, n), f"{n} declared in include/pmunet_hip.h but not exported"
    assert set(SIGNATURES) == set(names), "ctypes SIGNATURES out of sync with the header"
    assert set(EXP_SIGNATURES) == set(exp_names), "ctypes EXP_SIGNATURES out of sync with the experiments header"
    shipped_exp = [n for n in exp_names if hasattr(cdll, n)]
    assert not shipped_exp, f"experiments entries exported by the shipped library: {shipped_exp}"
    if os.path.exists(EXP_LIB_PATH):
        exp = load_library(EXP_LIB_PATH)
        for n in names + exp_names:
            assert hasattr(exp, n), f"{n} not exported by the experiments library"


# Launching entry points no test calls under its literal name: reached through a Python wrapper, or called
# by a test under a computed name.  name -> (test that exercises it, text that test's file must contain).
_REACHED_INDIRECTLY = {
    # pmu_hip.fusion
    "pmu_fuse3view": ("test_data_gpu.py::test_fusion_matches_g6", "pmu_fuse3view"),
    # utils.mri_dataset (the device slicer)
    "pmu_slice_view_layout": ("test_data_gpu.py::test_slicer_matches_reference_g5", "MRI_Dataset"),
    "pmu_slice_max": ("test_data_gpu.py::test_slicer_matches_reference_g5", "MRI_Dataset"),
    "pmu_gather_slices": ("test_data_gpu.py::test_slicer_matches_reference_g5", "MRI_Dataset"),
    # pmu_hip.packs (weight packs and the batched re-pack after an optimizer step)
    "pmu_conv3x3_pack_wino": ("test_wino_gpu.py::test_conv3x3_fwd_wino", "pack_weights_wino("),
    "pmu_conv3x3_pack_wino2h_multi": ("test_pack_gpu.py::test_packs_cached_and_batch_repacked_after_fused_sgd", "FusedSGD"),
    "pmu_conv3x3_pack_wino4_multi": ("test_pack_gpu.py::test_packs_cached_and_batch_repacked_after_fused_sgd", "FusedSGD"),
}
# The fallback fp32 kernels and small entry points with a kernel-level reference test of their own
# (tests/test_wgrad_direct_gpu.py, test_convT_gpu.py, test_primitives_gpu.py; the losses, the fused SGD step,
# the Dice counters and Fcomb at the bounds of its ABI in tests/test_loss_kernels_gpu.py, test_sgd_kernel_gpu.py,
# test_dice_counts_gpu.py and test_fcomb_abi_gpu.py), the default routes' kernels (tests/test_exact_gpu.py), the
# operand-frame kernels (tests/test_frame_exact_gpu.py), the fused BN+ReLU backward passes
# (tests/test_bnbwd_exact_gpu.py), the 1x1 head on every path and class count (tests/test_head_exact_gpu.py) and the
# BN bookkeeping entries (tests/test_bn_finalize_gpu.py): never allow-listed.
_ANCHORED_DIRECTLY = (
    "pmu_conv3x3_wgrad", "pmu_convT2x2_fwd", "pmu_convT2x2_dgrad", "pmu_convT2x2_wgrad", "pmu_maxpool2_bwd",
    "pmu_avgpool2_bwd", "pmu_spatial_mean", "pmu_spatial_mean_bwd", "pmu_linear_fwd", "pmu_linear_bwd",
    "pmu_fcomb_zbias", "pmu_bnrelu_apply", "pmu_head1x1_bwd", "pmu_wgrad1x1", "pmu_dice_sums",
    "pmu_bce_fwd", "pmu_bce_bwd", "pmu_ce_fwd", "pmu_ce_bwd", "pmu_sgd_clip", "pmu_dice_counts",
    "pmu_dice_counts_many", "pmu_fcomb_fwd", "pmu_fcomb_bwd",
    # the default routes' kernels, held to the float64 reference bit for bit (tests/test_exact_gpu.py)
    "pmu_conv3x3_fwd_dma", "pmu_conv3x3_dgrad_dma", "pmu_conv3x3_dgrad_dma_bnr", "pmu_conv3x3_dgrad_dma_x1b_sum",
    "pmu_convT2x2_dbias_rows", "pmu_conv3x3_fwd_raw", "pmu_conv3x3_dgrad_raw", "pmu_conv3x3_fwd_bf16",
    "pmu_conv3x3_dgrad_bf16", "pmu_conv3x3_wgrad_bf16_dma", "pmu_conv3x3_wgrad_bf16", "pmu_convT2x2_fwd_dma",
    "pmu_convT2x2_dgrad_dma", "pmu_convT2x2_wgrad_bf16", "pmu_conv3x3_fwd_wino2h", "pmu_conv3x3_dgrad_wino2h",
    "pmu_conv3x3_dgrad_wino2h_bnr", "pmu_conv3x3_fwd_wino", "pmu_conv3x3_dgrad_wino", "pmu_conv3x3_wgrad_wino",
    "pmu_conv3x3_dgrad_wino4", "pmu_conv3x3_dgrad_wino4_bnr", "pmu_conv_first_fwd", "pmu_conv_first_wgrad",
    # the operand frames (tests/test_frame_exact_gpu.py) and the fused BN+ReLU backward passes
    # (tests/test_bnbwd_exact_gpu.py), equal to float64 bit for bit on representable grids
    "pmu_frame_to_bf16", "pmu_frame_to_f32", "pmu_frame_to_bf16_ld", "pmu_frame_to_f32_ld",
    "pmu_frame_to_bf16_pool_skip", "pmu_frame_to_f32_pool_skip", "pmu_bn_bwd_reduce", "pmu_bn_bwd_reduce_dxb",
    "pmu_maxpool2_bwd_bnr", "pmu_maxpool2_bwd_bnr_dxb", "pmu_maxpool2_bwd_bnr_stats", "pmu_maxpool2_bwd_bnr_stats_dxb",
    "pmu_maxpool2_bwd_bnbwd", "pmu_maxpool2_bwd_bnbwd_dxb", "pmu_avgpool2_bwd_bnr", "pmu_spatial_mean_bwd_bnr",
    # the 1x1 head, equal to float64 bit for bit but for the sigmoid's expf (tests/test_head_exact_gpu.py; with
    # pmu_head1x1_bwd and pmu_wgrad1x1 above), and the BN finalizers against float64 (tests/test_bn_finalize_gpu.py)
    "pmu_head1x1_fwd", "pmu_head1x1_bwd_bnr", "pmu_head1x1_bwd_dz",
    "pmu_colsum_f64", "pmu_bn_fwd_finalize", "pmu_bn_bwd_finalize", "pmu_bn_eval_coef")
_QUERIES = ("*_ws", "*_ws_*", "*_ok", "*_tiles*", "*_blocks", "*_packed_size*", "pmu_occupancy_*",
            "pmu_build_flags", "pmu_debug_*")


def test_every_launching_entry_point_is_called_by_a_test():
    """Every launching entry point of include/pmunet_hip.h (all but the size / shape / occupancy queries) is
    called under its own name — L.call("<name>", ...) or lib().<name>(...) — by some file under tests/, or
    is listed in _REACHED_INDIRECTLY with the test that reaches it.  A new entry point fails here until a
    test calls it."""
    import fnmatch
    import glob
    tests_dir = os.path.dirname(os.path.abspath(__file__))
    files = {os.path.basename(p): open(p).read() for p in sorted(glob.glob(os.path.join(tests_dir, "*.py")))}
    me = os.path.basename(__file__)
    text = "\n".join(v for k, v in files.items() if k != me)
    names = [n for n in _header_functions() if not any(fnmatch.fnmatch(n, q) for q in _QUERIES)]
    assert len(names) >= 80

    def called(n):
        return re.search(r'L\.call\(\s*"%s"|lib\(\)\.%s\(' % (n, n), text) is not None

    assert not set(_REACHED_INDIRECTLY) & set(_ANCHORED_DIRECTLY)
    for n in _ANCHORED_DIRECTLY:
        assert n in names and called(n), n
    missing = [n for n in names if not called(n) and n not in _REACHED_INDIRECTLY]
    assert not missing, f"entry points no test calls: {missing}"
    for n, (test_id, needle) in _REACHED_INDIRECTLY.items():
        assert n in names, f"{n}: not a launching entry point of the header"
        assert not called(n), f"{n}: called directly by a test, drop it from _REACHED_INDIRECTLY"
        fname, test = test_id.split("::")
        assert fname in files and re.search(r"^def %s\(" % test, files[fname], flags=re.M), test_id
        assert needle in files[fname], (n, test_id, needle)


def test_library_rejects_bad_arguments_without_gpu():
    """Host-side validation returns PMU_ERR_ARG before any launch (safe without a GPU)."""
    import ctypes
    from pmu_hip._lib import LIB_PATH, PMU_ERR_ARG, load_library
    if not os.path.exists(LIB_PATH):
        pytest.skip("library not built")
    cdll = load_library()
    assert cdll.pmu_conv3x3_fwd_wino(None, None, None, 0, None, None, None, None) == PMU_ERR_ARG
    assert cdll.pmu_conv3x3_fwd_dma(None, 16, 1, 32, 32, None, None, 64, None, None, None) == PMU_ERR_ARG
    assert cdll.pmu_sgd_clip(None, 0, None, ctypes.c_float(1), ctypes.c_float(1), ctypes.c_float(0.9),
                             ctypes.c_float(0.1), None) == PMU_ERR_ARG
    assert cdll.pmu_conv3x3_tiles(32, 256, 256) == 32 * 32 * 8


def test_wgrad_dma_shape_rule_without_gpu():
    """The bf16 weight gradient's buffer descriptors need each operand below 2^31 bytes (their
    out-of-range marker is voffset 0x80000000) and 16-wide maps: pmu_conv3x3_wgrad_dma_ok, a host
    function, admits c5's largest shapes and refuses what would overflow (the engine then takes the
    register-staged kernel)."""
    from pmu_hip._lib import LIB_PATH, load_library
    if not os.path.exists(LIB_PATH):
        pytest.skip("library not built")
    cdll = load_library()
    ok = cdll.pmu_conv3x3_wgrad_dma_ok
    assert ok(16, 512, 512, 128, 64) and ok(16, 512, 512, 64, 64)       # c5's 512^2 layers: 1.07 GB operands
    assert not ok(32, 512, 512, 128, 64)                                  # x at 2.1 GB
    assert not ok(64, 512, 512, 64, 128)                                  # dz at 4.3 GB
    assert not ok(2, 64, 15, 64, 64)                                      # narrower than a strip


def test_bench_roofline_peak_by_kernel_family():
    """bench.py prices the dominant kernel against the MFMA peak of the dtype it computes in."""
    import bench
    for k in ("pmu_conv3x3_wgrad_bf16", "pmu_conv3x3_fwd_raw", "pmu_conv3x3_dgrad_raw", "pmu_convT2x2_fwd_bf16"):
        assert bench.roofline_peak(k) == bench.BF16_MFMA_PEAK_TF, k
    for k in ("pmu_conv3x3_fwd_wino_raw", "pmu_conv3x3_dgrad_wino_raw", "pmu_conv3x3_wgrad_wino",
              "pmu_convT2x2_wgrad", "pmu_fcomb_bwd"):
        assert bench.roofline_peak(k) == bench.FP32_MFMA_PEAK_TF, k


def _fake_args(name):
    """Arguments of the ctypes signature of ``name`` as bench.KernelTimer sees them: every int 64, every
    frame a 2-image 64x64 frame of one 64-channel source, pointers None."""
    import ctypes
    from pmu_hip import _lib
    res, types = {**_lib.SIGNATURES, **_lib.EXP_SIGNATURES}[name]
    args = []
    for t in types:
        if t is ctypes.c_int or t is ctypes.c_longlong or t is ctypes.c_size_t:
            args.append(64)
        elif t is _lib._FP:
            f = _lib.PmuFrame()
            f.nsrc, f.N, f.H, f.W = 1, 2, 64, 64
            f.src[0].C, f.src[0].H, f.src[0].W = 64, 64, 64
            args.append(ctypes.byref(f))
        else:
            args.append(None)
    return args


def test_bench_counts_every_mfma_entry_point():
    """Every C-ABI entry whose kernels issue MFMAs (pmu_hip._lib.MFMA_ENTRY_POINTS, next to the ctypes
    table) is declared in the table, counted by bench.KernelTimer and has a non-zero FLOP formula — no
    MFMA kernel prints "tflops": null and step_mfma_busy_frac sees all of them."""
    import bench
    from pmu_hip import _lib
    assert bench.KernelTimer.MFMA is _lib.MFMA_ENTRY_POINTS
    for name in _lib.MFMA_ENTRY_POINTS:
        assert name in _lib.SIGNATURES or name in _lib.EXP_SIGNATURES, name
        fl = bench.KernelTimer._flops(name, _fake_args(name))
        assert fl > 0, name
        # the direct-sum basis of a Winograd launch is larger than its executed products, never zero
        assert bench.KernelTimer._direct(name, _fake_args(name), fl) >= fl, name
    # the fused variants count as their base call (same shapes, same MFMA work)
    for v, base in (("pmu_conv3x3_dgrad_dma_x1b_sum", "pmu_conv3x3_dgrad_dma"),
                    ("pmu_conv3x3_dgrad_dma_x1b", "pmu_conv3x3_dgrad_dma"),
                    ("pmu_convT2x2_fwd_dma_ldb", "pmu_convT2x2_fwd_dma"), ("pmu_convT2x2_fwd_ld", "pmu_convT2x2_fwd")):
        assert bench.KernelTimer._flops(v, _fake_args(v)) == bench.KernelTimer._flops(base, _fake_args(base)), v
    # and each has a kernel family for the PMC traffic lookup
    for name in _lib.MFMA_ENTRY_POINTS:
        assert name in bench.KERNEL_FAMILY, name


def test_debug_build_exports_and_identifies_itself():
    """The bounds-checked debug library (csrc `make DEBUG=1`, selected by PMU_LIB=debug) exports the
    same C ABI and reports its build flags; the shipped library is neither a debug nor an experiments
    build (kernel-variant A/B switches ignored)."""
    import ctypes
    from pmu_hip import _lib
    if not os.path.exists(_lib.LIB_PATH):
        pytest.skip("library not built")
    rel = _lib.load_library(os.path.join(os.path.dirname(_lib.LIB_PATH), "libpmunet_hip.so"))
    assert rel.pmu_build_flags() == 0
    out = (ctypes.c_int * 5)(*([7] * 5))
    assert rel.pmu_debug_read(out, None) == 0 and list(out) == [0] * 5
    dbg_path = os.path.join(os.path.dirname(_lib.LIB_PATH), "libpmunet_hip_debug.so")
    if not os.path.exists(dbg_path):
        pytest.skip("debug library not built (make -C csrc DEBUG=1)")
    dbg = _lib.load_library(dbg_path)   # every SIGNATURES export must resolve
    assert dbg.pmu_build_flags() == _lib.BUILD_DEBUG


def test_bench_gpus_launch_plan():
    """bench.py --gpus N: outside torchrun N > 1 becomes a torch.distributed.run child
    with N ranks on this node and the same argv; under torchrun --gpus must equal WORLD_SIZE."""
    import bench
    assert bench.launch_plan(1, [], {}) is None
    cmd = bench.launch_plan(4, ["--gpus", "4", "--steps", "3"], {})
    assert cmd[1:3] == ["-m", "torch.distributed.run"]
    assert "--nproc-per-node=4" in cmd and "--nnodes=1" in cmd and "--master-addr=127.0.0.1" in cmd
    assert cmd[-4:] == ["--gpus", "4", "--steps", "3"] and cmd[-5].endswith("bench.py")
    assert bench.launch_plan(2, [], {"WORLD_SIZE": "2"}) is None
    assert bench.launch_plan(1, [], {"WORLD_SIZE": "1"}) is None
    for gpus, world in ((1, "8"), (8, "1"), (2, "4")):
        with pytest.raises(ValueError):
            bench.launch_plan(gpus, [], {"WORLD_SIZE": world})
    with pytest.raises(ValueError):
        bench.launch_plan(0, [], {})


def test_bench_refuses_gpus_world_mismatch():
    """The mismatch check runs before anything touches torch.cuda: rc 2 and a message, no JSON line."""
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ, WORLD_SIZE="2", RANK="0", LOCAL_RANK="0")
    r = subprocess.run([sys.executable, os.path.join(root, "bench.py"), "--gpus", "4"], env=env,
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 2, r.stderr[-2000:]
    assert "WORLD_SIZE=2" in r.stderr and r.stdout.strip() == ""


def test_bench_roofline_by_kernel_family():
    """bench.py groups the MFMA entries into kernel families before picking the dominant one (VERDICT r5
    #3): c5's input gradient runs as three entries (_bnr_dxb, _x1b_sum_dxb, _dxb) whose summed time beats
    the forward's, so the line names the input gradient, with the forward as the runner-up."""
    import bench
    per = {  # name: [launches, executed FLOPs, seconds, direct-sum FLOPs] (c5-like proportions)
        "pmu_conv3x3_dgrad_dma_bnr_dxb": [9, 2.7e12, 3.4e-3, 2.7e12],
        "pmu_conv3x3_dgrad_dma_x1b_sum_dxb": [4, 1.6e12, 2.1e-3, 1.6e12],
        "pmu_conv3x3_dgrad_dma_dxb": [3, 0.8e12, 1.0e-3, 0.8e12],
        "pmu_conv3x3_fwd_dma": [17, 5.9e12, 5.4e-3, 5.9e12],
        "pmu_conv3x3_wgrad_bf16_dma": [17, 5.5e12, 4.7e-3, 5.5e12],
        "pmu_frame_to_bf16": [30, 0.0, 2.8e-3, 0.0],   # not an MFMA entry: never a family
    }
    fams = bench.mfma_families(per)
    assert [f[0] for f in fams] == ["pmu_conv3x3_dgrad_dma", "pmu_conv3x3_fwd_dma", "pmu_conv3x3_wgrad_bf16_dma"]
    fam, d, members = fams[0]
    assert members == sorted(["pmu_conv3x3_dgrad_dma_bnr_dxb", "pmu_conv3x3_dgrad_dma_x1b_sum_dxb",
                              "pmu_conv3x3_dgrad_dma_dxb"])
    assert d[0] == 16 and abs(d[2] - 6.5e-3) < 1e-12
    roof = bench.roofline_entry("c5", *fams[0])
    assert roof["kernel"] == "pmu_conv3x3_dgrad_dma" and roof["launches"] == 16
    assert roof["peak"] == bench.BF16_MFMA_PEAK_TF
    assert abs(roof["frac"] - 5.1e12 / 6.5e-3 / 1e12 / bench.BF16_MFMA_PEAK_TF) < 1e-4
    # a Winograd family carries its direct-sum figure beside the executed-product utilisation
    w = bench.roofline_entry("unet", "pmu_conv3x3_dgrad_wino4", [15, 1.0e12, 9.8e-3, 2.25e12],
                             ["pmu_conv3x3_dgrad_wino4", "pmu_conv3x3_dgrad_wino4_bnr"])
    assert w["peak"] == bench.FP32_MFMA_PEAK_TF and w["direct_sum_equiv_frac"] > w["frac"]


def test_bench_refuses_bad_rank_layouts():
    """Under RCCL every rank needs its own GPU: world > visible devices, or two ranks reporting the same
    PCI identity, is refused (exit 2); gloo may rehearse N ranks on one device."""
    import bench
    assert bench.check_layout("nccl", 8, 8) is None
    assert bench.check_layout(None, 1, 1) is None and bench.check_layout(None, 1, 0) is None
    assert bench.check_layout("gloo", 2, 1) is None
    assert "2 RCCL ranks but 1" in bench.check_layout("nccl", 2, 1)
    assert bench.check_layout("nccl", 4, 0)
    assert bench.check_devices("nccl", ["0000:05:00.0 a", "0000:15:00.0 b"]) is None
    assert bench.check_devices("gloo", ["0000:05:00.0 a", "0000:05:00.0 a"]) is None
    assert "share a GPU" in bench.check_devices("nccl", ["0000:05:00.0 a", "0000:05:00.0 a"])


def test_bench_refuses_rccl_ranks_beyond_devices():
    """End to end: a rank of a 2-rank RCCL run on a host with fewer GPUs exits 2 with the reason before
    any process group is formed (here: no GPU at all), and prints no JSON line."""
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ, WORLD_SIZE="2", RANK="0", LOCAL_RANK="0", MASTER_ADDR="127.0.0.1",
               MASTER_PORT="29599", PMU_DIST_BACKEND="nccl")
    r = subprocess.run([sys.executable, os.path.join(root, "bench.py"), "--gpus", "2"], env=env,
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 2, r.stderr[-2000:]
    assert "RCCL ranks but" in r.stderr and r.stdout.strip() == ""


def test_bench_dump_outputs_float_arrays_fixed_sample(tmp_path):
    """bench.py --dump-outputs: one <name>.npy per array, float32 (float64 kept), shapes kept up to the
    per-array cap; a larger array is written as a sample at positions that depend only on its size, so two
    runs (or two builds) write comparable files."""
    import numpy as np
    import bench
    big = torch.arange(5000, dtype=torch.float32).reshape(50, 100)
    outs = {"loss": torch.tensor(1.5, dtype=torch.float64), "out": torch.ones(2, 3, 4, dtype=torch.bfloat16),
            "counts": torch.arange(6).reshape(2, 3), "big": big}
    for d in ("a", "b"):
        bench.dump_outputs(str(tmp_path / d), outs, max_elems=1000)
    a = {n: np.load(tmp_path / "a" / f"{n}.npy") for n in outs}
    assert sorted(os.listdir(tmp_path / "a")) == sorted(f"{n}.npy" for n in outs)
    assert a["loss"].dtype == np.float64 and a["loss"].shape == () and float(a["loss"]) == 1.5
    assert a["out"].dtype == np.float32 and a["out"].shape == (2, 3, 4)
    assert a["counts"].dtype == np.float32 and a["counts"].tolist() == [[0, 1, 2], [3, 4, 5]]
    assert a["big"].dtype == np.float32 and a["big"].shape == (1000,)
    assert np.all(np.diff(a["big"]) >= 0) and a["big"].max() < 5000 and len(np.unique(a["big"])) > 800
    assert np.array_equal(a["big"], np.load(tmp_path / "b" / "big.npy"))
    assert 6 * bench.DUMP_MAX_ELEMS * 4 < 64 * 2 ** 20   # the largest step (c4) writes 6 arrays


def test_oracle_bf16_dx_rule_matches_engine(monkeypatch):
    """oracle/unet_ref.py models the HIP path's bf16 activation gradients (BF16_DX) by the same rule the
    engine uses to pick the *_dxb input gradients (engine.dxb_ok, through the library's
    pmu_conv3x3_dma_ok; the transposed conv: pmu_convT2x2_dma_ok) — checked here over a grid of shapes so
    the parity tests compare like with like."""
    import oracle.unet_ref as ur
    from pmu_hip import _lib as L
    from pmu_hip.engine import dxb_ok
    if not os.path.exists(L.LIB_PATH):
        pytest.skip("library not built")
    lb = L.load_library()   # host-side shape predicates only (no GPU call)
    monkeypatch.setattr(L, "_LIB", lb)
    assert ur.BF16_DX
    x = torch.empty(1, 1, 1, 1)
    for W in (16, 31, 32, 45, 64):
        xx = x.expand(1, 1, 1, W)
        for cin in (3, 8, 12, 32, 40, 64, 96, 128, 1024):
            for cout in (8, 12, 16, 20, 32, 64, 1024):
                for split in (None, 8, 16, 32, 64):
                    if split is not None and split >= cin:
                        continue
                    want = dxb_ok(7, W, cout, cin, cin if split is None else split)
                    assert ur._dma_dxb(xx, cin, cout, split) == want, (W, cin, cout, split)
    for cin in (32, 64, 96, 128, 256, 1024):
        for cout in (16, 32, 64, 512):
            assert bool(lb.pmu_convT2x2_dma_ok(cin, cout, 1)) == (cin % 128 == 0 and cout % 32 == 0), (cin, cout)


def _routes_of(bf16, cin, filters, N, H, W):
    """name -> (forward route, input-gradient Dgrad or None, weight-gradient entry) of every 3x3 conv of
    model.UNet(cin, _, filters) on an N x cin x H x W batch, as pmu_hip.routes gives them for a training step
    (engine.unet_backward: every consumer takes dx in bf16 where its kernel can store it so)."""
    from helpers import unet_convs
    from pmu_hip import routes as R
    out = {}
    for c in unet_convs(cin, filters, N, H, W):
        if c["kind"] != "conv":
            continue
        fwd = R.conv_fwd_route(bf16, N, c["H"], c["W"], c["Cin"], c["Cout"], planes=c["planes"])
        first = fwd == "first"
        b, ci = bf16 and not first, c["planes"] or c["Cin"]
        need_dx = c["name"] != "inc.c1"
        dg = (R.conv_dgrad(b, N, c["H"], c["W"], ci, c["Cout"], c["split"], bnr=c["bnr"], want_dxb=True)
              if need_dx and not first else None)
        wg = R.WGRAD[R.conv_wgrad_route(b, N, c["H"], c["W"], ci, c["Cout"], first=first, need_dx=need_dx,
                                              kept=R.conv_fwd_keeps_f32(fwd, ci, c["Cout"], True))][0]
        out[c["name"]] = (fwd, dg, wg, c)
    return out


def _in_place(bf16, cin, filters, N, H, W):
    """routes.concat_in_place of every Up block, deepest first."""
    from helpers import unet_convs
    from pmu_hip import routes as R
    return [R.concat_in_place(bf16, N, c["h"], c["w"], c["Cin"], c["Cup"], c["hs"], c["ws"], c["Cskip"], c["Cout1"])
            for c in unet_convs(cin, filters, N, H, W) if c["kind"] == "convT"]


@pytest.fixture
def host_lib(monkeypatch):
    """The release library's host-side shape predicates without a GPU (no launch, no torch.cuda call)."""
    from pmu_hip import _lib as L
    from pmu_hip import routes as R
    if not os.path.exists(L.LIB_PATH):
        pytest.skip("library not built")
    monkeypatch.setattr(L, "_LIB", L.load_library(os.path.join(os.path.dirname(L.LIB_PATH), "libpmunet_hip.so")))
    monkeypatch.setattr(R, "CFG", R.EngineConfig())   # the defaults, whatever PMU_* this process inherited
    return L


def test_route_table_c2_c5(host_lib):
    """The dispatch policy (pmu_hip.routes) on the two benchmark configs, release library, default CFG."""
    r = _routes_of(False, 1, [64, 128, 256, 512, 1024], 32, 256, 256)   # c2: fp32
    assert len(r) == 18
    for name, (fwd, dg, wg, c) in r.items():
        if name == "inc.c1":
            assert (fwd, dg, wg) == ("first", None, "pmu_conv_first_wgrad")
            continue
        assert fwd == "wino2h", name
        assert dg.route == ("wino4" if c["H"] >= 32 else "wino2h"), name     # levels 256..32: F(4x4); 16^2: F(2x2)
        assert dg.form == ("bnr" if c["bnr"] else "") and not dg.dxb, name
        assert wg == "pmu_conv3x3_wgrad_wino", name
    assert sorted({c["H"] for _, _, _, c in r.values()}) == [16, 32, 64, 128, 256]
    r = _routes_of(True, 3, [64, 128, 256, 512, 1024], 16, 512, 512)    # c5: bf16
    for name, (fwd, dg, wg, c) in r.items():
        if name == "inc.c1":
            assert (fwd, dg, wg) == ("first", None, "pmu_conv_first_wgrad")
            continue
        assert fwd == "dma" and dg.route == "dma" and dg.dxb, name
        assert wg == "pmu_conv3x3_wgrad_bf16_dma", name
    assert [r[f"up{j}.c1"][3]["split"] for j in range(4)] == [512, 256, 128, 64]
    assert all(r[f"up{j}.c1"][1].entry == "pmu_conv3x3_dgrad_dma_x1b_dxb" for j in range(4))
    assert r["up0.c2"][1].entry == "pmu_conv3x3_dgrad_dma_bnr_dxb" and r["down1.c1"][1].entry == "pmu_conv3x3_dgrad_dma_dxb"
    # every Up block of both builds its concat operand in place
    assert _in_place(False, 1, [64, 128, 256, 512, 1024], 32, 256, 256) == [True] * 4
    assert _in_place(True, 3, [64, 128, 256, 512, 1024], 16, 512, 512) == [True] * 4


def test_route_table_small_shapes(host_lib):
    """Small shapes that reach the other branches of the policy."""
    DIRECT, WINO = "pmu_conv3x3_wgrad", "pmu_conv3x3_wgrad_wino"
    r = _routes_of(False, 1, [8, 24, 40], 2, 72, 40)
    for name, (fwd, dg, wg, c) in r.items():
        if name == "inc.c1":
            assert fwd == "first"
            continue
        assert fwd == "wino_fused" and wg == DIRECT, name
        assert dg.route == ("wino4" if (c["H"], c["W"]) == (72, 40) else "wino_fused"), name
    assert {(c["H"], c["W"]) for _, _, _, c in r.values()} == {(72, 40), (36, 20), (18, 10)}

    r = _routes_of(False, 1, [16, 32, 64], 2, 48, 48)
    for name, (fwd, dg, wg, c) in r.items():
        if name == "inc.c1":
            assert fwd == "first"
            continue
        assert fwd == "wino2h", name
        assert dg.route == ("wino4" if c["H"] == 48 else "wino2h"), name
        assert wg == (WINO if (c["Cin"], c["Cout"]) == (64, 64) else DIRECT), name
    assert r["down2.c2"][2] == WINO

    r = _routes_of(True, 3, [16, 32, 64], 2, 64, 64)
    for name, (fwd, dg, wg, c) in r.items():
        if name in ("inc.c1", "up1.c1"):
            continue
        want = "raw" if c["H"] == 16 else "dma"
        assert fwd == want and dg.route == want, name
        assert dg.dxb == (want == "dma"), name
    assert r["inc.c1"][0] == "first"
    fwd, dg, _, c = r["up1.c1"]        # concat conv 32 -> 16, split 16
    assert (c["Cin"], c["Cout"], c["split"]) == (32, 16, 16)
    assert fwd == "dma" and dg.route == "bf16_fused" and dg.entry == "pmu_conv3x3_dgrad_bf16"

    r = _routes_of(True, 3, [64, 128, 256], 2, 64, 48)
    for name, (fwd, dg, wg, c) in r.items():
        if name == "inc.c1":
            continue
        want = "dma" if (c["H"], c["W"]) == (64, 48) else "raw"
        assert fwd == want and dg.route == want, name
        assert wg == ("pmu_conv3x3_wgrad_bf16" if c["H"] == 16 else "pmu_conv3x3_wgrad_bf16_dma"), name

    r = _routes_of(True, 3, [12, 20], 2, 40, 40)
    assert r["inc.c1"][0] == "raw" and r["inc.c1"][3]["planes"] == 3     # Cout = 12 fails first_layer_ok
    for name in ("inc.c2", "up0.c2"):                                    # the 12 -> 12 convs
        fwd, dg, _, _ = r[name]
        assert fwd == "dma" and dg.route == "dma" and not dg.dxb, name
    for name in ("down1.c1", "down1.c2"):                                # the 20 x 20 level
        assert r[name][0] == "raw" and r[name][1].route == "raw", name
    assert r["up0.c1"][3]["split"] == 12 and r["up0.c1"][1].route == "bf16_fused"

    r = _routes_of(False, 5, [12, 20], 2, 40, 40)                        # five input channels: no planes
    assert r["inc.c1"][3]["planes"] == 0
    for name, (fwd, dg, wg, c) in r.items():
        assert fwd == "wino_fused" and (dg is None or dg.route == "wino_fused"), name

    # in-place concat: not with F.pad (odd sizes), not with halves off the 8-channel grid
    for bf16, cin in ((False, 1), (True, 3)):
        assert _in_place(bf16, cin, [16, 32, 64], 2, 50, 46) == [False, False]
    assert _in_place(True, 3, [12, 20], 2, 40, 40) == [False]
    assert _in_place(False, 5, [12, 20], 2, 40, 40) == [False]
    assert _in_place(False, 1, [16, 32, 64], 2, 48, 48) == [True, False]   # (the 8-channel transposed conv: no _ld)


def test_route_config_clamped_by_shipped_library(host_lib, monkeypatch):
    """The switches only an experiments build honours: with one loaded they move the routes, with the
    shipped library they are clamped to the default dispatch (routes.effective)."""
    from pmu_hip import routes as R
    R.CFG.fp32_conv = "direct"
    shape = (False, 2, 48, 48, 64, 64)
    assert R.effective().fp32_conv == "wino"
    assert R.conv_fwd_route(*shape) == "wino2h" and R.conv_dgrad_route(*shape) == "wino4"
    R.CFG.fp32_conv, R.CFG.wino4 = "wino", "1"
    R.CFG.bf16_z = True
    eff = R.effective()
    assert (eff.wino4, eff.bf16_z) == ("dgrad", False)
    assert R.conv_fwd_route(*shape) == "wino2h" and R.conv_fwd_route(False, 2, 16, 16, 64, 64) == "wino2h"
    assert R.conv_wgrad_route(*shape, kept=True) == "wino" and R.conv_wgrad_route(*shape, kept=True, need_dx=False) == "direct"
    monkeypatch.setattr(host_lib, "experiments_build", lambda: True)
    assert R.effective() is R.CFG
    assert R.conv_fwd_route(*shape) == "wino4"                               # wino4 = "1": the forward too
    R.CFG.fp32_conv = "direct"
    assert R.conv_fwd_route(*shape) == "direct" and R.conv_dgrad_route(*shape) == "direct"
    assert R.conv_wgrad_route(*shape, kept=True) == "direct_teed"
    assert not R.concat_in_place(False, 32, 128, 128, 128, 64, 256, 256, 64, 64)


def test_route_entries_are_declared():
    """Every entry name the policy can hand the engine is in the ctypes tables (an input gradient's name is
    composed from its route, epilogue form and dx storage: a misspelt combination fails here, not at launch)."""
    from pmu_hip import _lib as L
    from pmu_hip import routes as R
    known = {**L.SIGNATURES, **L.EXP_SIGNATURES}
    names = list(R.FWD_ENTRY.values()) + [R.FWD_DMA_ZB] + [n for pair in R.WGRAD.values() for n in pair]
    forms = [("dma", f, x) for f in ("", "bnr", "x1b", "x1b_sum") for x in (False, True)] + [("dma", "bnr_zb", False)]
    forms += [(r, "", False) for r in ("raw", "bf16_fused", "wino4", "wino2h", "wino_fused", "direct")]
    forms += [("wino4", "bnr", False), ("wino2h", "bnr", False)]
    names += [R.Dgrad(*f).entry for f in forms]
    assert len(set(names)) == 9 + 10 + 17   # forward, weight gradient (+ queries; "direct" twice), input gradient
    for n in names:
        assert n in known, n
    assert R.Dgrad("dma", "x1b_sum", True).entry == "pmu_conv3x3_dgrad_dma_x1b_sum_dxb"
    assert R.Dgrad("bf16_fused").entry == "pmu_conv3x3_dgrad_bf16" and R.Dgrad("direct").entry == "pmu_conv3x3_dgrad"
    assert set(R.TEED) < set(R.WGRAD) and set(R.MATERIALISED) < set(R.FWD_ENTRY)
    # MaxPool2d(2) backward: (C, z in fp32, batch statistics, both parts bf16, bf16 layer) -> entry
    pool = {(64, True, True, True, True): "pmu_maxpool2_bwd_bnr_stats_dxb", (64, True, True, False, False): "pmu_maxpool2_bwd_bnr_stats",
            (64, True, True, True, False): "pmu_maxpool2_bwd_bnr_dxb", (12, True, True, True, True): "pmu_maxpool2_bwd_bnr_dxb",
            (12, True, True, False, True): "pmu_maxpool2_bwd_bnr", (64, True, False, True, True): "pmu_maxpool2_bwd",
            (6, True, True, False, False): "pmu_maxpool2_bwd", (64, False, True, True, True): "pmu_maxpool2_bwd_zb"}
    for args, want in pool.items():
        assert R.maxpool_bwd(*args) == want and want in known, args
    R.CFG.pool_fuse, keep = False, R.CFG.pool_fuse
    try:
        assert R.maxpool_bwd(64, True, True, True, True) == "pmu_maxpool2_bwd_bnr_dxb"
        assert R.maxpool_bwd(64, True, True, False, False) == "pmu_maxpool2_bwd_bnr"
    finally:
        R.CFG.pool_fuse = keep


def test_variant_switches_are_documented():
    """Every name the kernel sources pass to pmu_variant_env / pmu_variant_int (the experiments-build
    switches) is named in INTEGRATION.md's Builds section.  Text only: nothing is compiled."""
    import glob
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    names = set()
    for path in glob.glob(os.path.join(root, "probabilistic-multiplanar-unet_amd", "csrc", "*.hip")):
        with open(path) as f:
            names |= set(re.findall(r'pmu_variant_(?:env|int)\(\s*"(\w+)"', f.read()))
    assert "PMU_WGW_SDMA" in names and "PMU_FRAME_NT" in names, sorted(names)   # (the regex finds both forms)
    with open(os.path.join(root, "INTEGRATION.md")) as f:
        doc = f.read()
    builds = doc[doc.index("\nBuilds:\n"):doc.index("\nEngine choices")]
    words = set(re.findall(r"PMU_\w+", builds))
    missing = sorted(n for n in names if n not in words)
    assert not missing, f"experiments-build switches missing from INTEGRATION.md's Builds section: {missing}"


def test_fcomb_kernels_keep_their_registers():
    """csrc/fcomb.hip compiled for gfx950 (device pass only, nothing is run): the forward and the statistics
    kernels are bound to two waves per SIMD and fcomb_fwd_kernel<true> sits a register below that limit, so a
    compiler or source change that makes one of them spill has to show here and not as lost time.  No kernel
    spills, except the NH = 3 backward, which keeps at most the 4 registers it has always spilled; the
    occupancies are those of the launch bounds."""
    import importlib.util
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    spec = importlib.util.spec_from_file_location("pmu_tools_regs", os.path.join(root, "tools", "regs.py"))
    regs = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(regs)
    rows = regs.table(os.path.join(root, "probabilistic-multiplanar-unet_amd", "csrc", "fcomb.hip"))
    want = {"fcomb_fwd_kernel<true>": (0, 2), "fcomb_fwd_kernel<false>": (0, 2), "fcomb_stats_kernel<true>": (0, 2),
            "fcomb_stats_kernel<false>": (0, 2), "fcomb_bwd_reg_kernel<1>": (0, 1), "fcomb_bwd_reg_kernel<2>": (0, 1),
            "fcomb_bwd_reg_kernel<3>": (4, 1)}       # kernel: (most spilled VGPRs, waves per SIMD)
    seen = {}
    for name, v in rows.items():
        key = re.sub(r"^void ", "", name).split("(")[0]
        if key in want:
            seen[key] = (v["VGPRs Spill"], v["Occupancy [waves/SIMD]"])
            print(f"{key}: {v['VGPRs']} VGPRs, {v['AGPRs']} AGPRs, {v['VGPRs Spill']} spilled, occupancy {seen[key][1]}")
    assert set(seen) == set(want), sorted(set(want) - set(seen))
    for key, (spill, occ) in want.items():
        assert seen[key][0] <= spill and seen[key][1] == occ, (key, seen[key], (spill, occ))
