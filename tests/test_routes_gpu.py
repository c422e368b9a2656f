"""The engine launches what the dispatch policy (pmu_hip.routes) says: one training step of a small UNet
in each precision, its launch trace against the sequence derived from the policy alone."""
import re

import pytest
import torch

from helpers import unet_launch_plan

CONV = re.compile(r"pmu_(conv3x3|conv_first|convT2x2)_(fwd|dgrad|wgrad)")


@pytest.mark.gpu
@pytest.mark.parametrize("bf16,ch,filters,N,H,W", [(False, 1, [16, 32, 64], 2, 48, 48), (True, 3, [16, 32, 64], 2, 64, 64)],
                         ids=["fp32", "bf16"])
def test_engine_obeys_the_route_policy(dev, bf16, ch, filters, N, H, W):
    from model import UNet
    from pmu_hip import _lib as L
    torch.manual_seed(0)
    net = UNet(ch, ch, filters).to(dev).train()
    x = torch.rand(N, ch, H, W, device=dev)
    calls = []
    L.set_call_observer(lambda name, args, e0, e1: calls.append((name, args)))
    try:
        with torch.autocast("cuda", dtype=torch.bfloat16, enabled=bf16):
            y = net(x)
        nfwd = len(calls)
        y.float().sum().backward()
        torch.cuda.synchronize()
    finally:
        L.set_call_observer(None)
    got = [n for n, _ in calls if CONV.match(n)]
    assert got == unet_launch_plan(bf16, ch, filters, N, H, W)
    # an Up block's concat operand built in place (the transposed conv writes its half at a pixel stride)
    # is the concat conv's operand as it stands: no pmu_frame_to_* pass copies it again
    built = 0
    xcat = None
    for name, args in calls[:nfwd]:
        if name == "pmu_convT2x2_fwd_ld":          # (in, w, wp, bias, Cup, u, ldo, stream)
            xcat = args[5] - 4 * (args[6] - args[4])
        elif name == "pmu_convT2x2_fwd_dma_ldb":   # (xt, Cip, N, H, W, wp, bias, Cin, Cup, ub, ldo, stream)
            xcat = args[9] - 2 * (args[10] - args[8])
        elif xcat is not None and name in ("pmu_frame_to_f32", "pmu_frame_to_bf16"):
            f = args[0]._obj
            assert all(f.src[i].x != xcat for i in range(f.nsrc)), name
        elif xcat is not None and name.startswith("pmu_conv3x3_fwd"):
            assert args[0] == xcat, name           # the materialised-operand entries take the operand first
            built, xcat = built + 1, None
    assert built >= 1
