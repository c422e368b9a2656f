"""GPU tests of the soft Dice training loss (pmu_hip.loss.SoftDiceLoss on pmu_softdice_fwd / _bwd).

The reference everywhere is the formula of include/pmunet_hip.h written in plain torch (soft_dice_ref
below), on the CPU with autograd for the gradients: in float64 for the kernel-level tests, in float32
behind oracle.unet_ref.unet_forward for the model-level ones.

Kernel-level tolerances are the ones tests/test_loss_gpu.py holds the CE to: 1e-5 relative on the value,
1e-5 of max |g_ref| on the gradient.  (The kernel's arithmetic — fp32 softmax, fp64 sums, fp32
coefficients, fp32 backward — emulated on the CPU stays within 8.4e-7 of the float64 formula on both
measures over K in {2, 3, 5, 8}, both poolings, both include_background values, ignored pixels and an
absent class at 3 x K x 21 x 17.)  Model-level bounds are helpers.ACT_TOL / LOSS_RTOL / GRAD_TOL.
"""
import pytest
import torch

from helpers import ACT_TOL, GRAD_TOL, LOSS_RTOL, grad_err, max_abs, phantom_batch

pytestmark = pytest.mark.gpu

EPS = 1e-6
VAL_RTOL = 1e-5
GRAD_RTOL = 1e-5


def soft_dice_ref(x, t, include_background=True, per_image=False, ignore_index=-100, from_logits=None):
    """loss = 1 - mean D, D = (2 I + eps) / (P + T + eps), in x's dtype.  K >= 2: x (N, K, *) logits,
    p = softmax, t (N, *) class indices, pixels with t == ignore_index left out.  K == 1: x a probability
    (a logit with from_logits: sigmoid), t a float mask used by value.  Sums over the batch or per image;
    the mean over the classes 0 (1 without the background) .. K - 1 and, per image, the images."""
    N, K = x.shape[0], x.shape[1]
    if K == 1:
        p = x.reshape(N, 1, -1)
        if from_logits:
            p = torch.sigmoid(p)
        tt = t.to(x.dtype).reshape(N, 1, -1)
        valid = torch.ones_like(tt)
        first = 0
    else:
        p = torch.softmax(x.reshape(N, K, -1), 1)
        ti = t.reshape(N, -1)
        valid = (ti != ignore_index).to(x.dtype)[:, None]
        tt = torch.stack([ti == k for k in range(K)], 1).to(x.dtype)
        first = 0 if include_background else 1
    dims = (2,) if per_image else (0, 2)
    inter, ps, ts = (p * tt * valid).sum(dims), (p * valid).sum(dims), (tt * valid).sum(dims)
    d = (2 * inter + EPS) / (ps + ts + EPS)
    return 1 - d[..., first:].mean()


_REF = {}


def _reference(key, x, t, scale, **kw):
    """(loss, dx) of scale * soft_dice_ref in float64 on the CPU, computed once per key."""
    if key not in _REF:
        xr = x.double().requires_grad_(True)
        loss = soft_dice_ref(xr, t, **kw)
        (loss * scale).backward()
        _REF[key] = (loss.detach(), xr.grad.detach())
    return _REF[key]


def _hip(dev, x, t, scale, **kw):
    from pmu_hip.loss import SoftDiceLoss
    xd = x.to(dev).requires_grad_(True)
    loss = SoftDiceLoss(**kw)(xd, t.to(dev))
    (loss * scale).backward()
    return loss.detach().cpu(), xd.grad.detach().cpu()


def _check(got, ref, what=""):
    (loss, dx), (loss_ref, dx_ref) = got, ref
    verr = abs(float(loss) - float(loss_ref)) / abs(float(loss_ref))
    gerr = float((dx.double() - dx_ref).abs().max()) / float(dx_ref.abs().max())
    print(f"{what} loss {float(loss):.8f} ref {float(loss_ref):.8f} rel {verr:.2e}  grad err {gerr:.2e}")
    assert loss.dtype == torch.float32 and loss.shape == ()
    assert verr <= VAL_RTOL, (what, verr)
    assert dx.shape == dx_ref.shape and gerr <= GRAD_RTOL, (what, gerr)


def _mc_inputs(shape, seed, absent=False):
    """randn * 3 logits of ``shape`` (N, K, H, W), random class targets with a run of ignored pixels;
    absent: class K - 1 never occurs in the target."""
    N, K, H, W = shape
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(N, K, H, W, generator=g) * 3
    t = torch.randint(0, K - 1 if absent else K, (N, H, W), generator=g)
    t[N // 2, 2, :6] = -100
    return x, t


# ----------------------------------------------------------------------------- kernel level
@pytest.mark.parametrize("absent", [False, True])
@pytest.mark.parametrize("include_background", [True, False])
@pytest.mark.parametrize("per_image", [False, True])
@pytest.mark.parametrize("K", [2, 3, 5, 8])
def test_soft_dice_odd_plane(dev, K, per_image, include_background, absent):
    """HW = 357: odd, so every second class plane is misaligned and the scalar path runs."""
    x, t = _mc_inputs((3, K, 21, 17), K, absent)
    assert int(t[1, 2, 0]) == -100
    scale = 0.7 if (K + per_image + include_background + absent) % 2 else 1.0
    kw = dict(per_image=per_image, include_background=include_background)
    ref = _reference(("odd", K, per_image, include_background, absent, scale), x, t, scale, **kw)
    _check(_hip(dev, x, t, scale, **kw), ref, f"K={K}")


VEC_SHAPES = [(2, 3, 32, 40), (4, 2, 256, 256), (1, 3, 8, 4), (4, 2, 1024, 1024)]


@pytest.mark.parametrize("per_image", [False, True])
@pytest.mark.parametrize("shape", VEC_SHAPES)
def test_soft_dice_vector_path(dev, shape, per_image):
    """HW % 4 == 0: the 16-byte loads.  (1, 3, 8, 4) is a single partial block.  The forward gives a block
    2048 pixels until the launch reaches 1024 blocks, so (4, 2, 256, 256) runs 32 blocks per image, each
    looping twice, below the cap of 256 per image; 1024 x 1024 is the smallest power-of-two square that
    reaches it at N = 4 (512 wanted, 256 launched, eight rounds per thread)."""
    x, t = _mc_inputs(shape, 7)
    kw = dict(per_image=per_image)
    ref = _reference(("vec", shape, per_image), x, t, 0.7, **kw)
    _check(_hip(dev, x, t, 0.7, **kw), ref, str(shape))


def _binary_inputs(logits, soft):
    g = torch.Generator().manual_seed(1)
    if logits:
        y = torch.randn(4, 1, 33, 29, generator=g) * 4
    else:
        y = torch.rand(4, 1, 33, 29, generator=g)
        y[0, 0, 0, :5] = torch.tensor([0.0, 1.0, 1e-30, 1 - 1e-7, 0.5])
    t = torch.rand(4, 1, 33, 29, generator=g)
    return y, (t if soft else (t > 0.5).float())


@pytest.mark.parametrize("per_image", [False, True])
@pytest.mark.parametrize("logits,soft", [(False, False), (True, False), (False, True), (True, True)])
def test_soft_dice_binary(dev, logits, soft, per_image):
    """One class: probabilities (the sigmoid head; exact 0 / 1 values included) or logits with the sigmoid
    in the kernel, a 0/1 mask or a soft one used by value."""
    y, t = _binary_inputs(logits, soft)
    kw = dict(per_image=per_image, from_logits=logits)
    ref = _reference(("bin", logits, soft, per_image), y, t, 0.7, **kw)
    _check(_hip(dev, y, t, 0.7, **kw), ref, f"logits={logits} soft={soft}")


def test_soft_dice_of_hard_inputs_is_one_minus_dice_coeff(dev):
    """For y in {0, 1} the loss is 1 - dice_coeff(y, t), the metric G4 pins bit-exactly."""
    from dice_loss import dice_coeff, dice_loss
    g = torch.Generator().manual_seed(4)
    y = (torch.rand(4, 1, 33, 29, generator=g) > 0.4).float().to(dev)
    t = (torch.rand(4, 1, 33, 29, generator=g) > 0.5).float().to(dev)
    loss = dice_loss(y, t)
    assert abs((1.0 - float(loss)) - float(dice_coeff(y, t))) <= 1e-6
    assert float(dice_loss(t, t)) <= 1e-6


def test_soft_dice_image_with_every_pixel_ignored(dev):
    """per_image with one image fully ignored: its D_k are eps / eps = 1, so it adds 0 to the loss (the
    loss is (N - 1) / N of the other images' alone), its dx is exactly 0 and everything is finite."""
    x, t = _mc_inputs((3, 3, 21, 17), 5)
    t[1] = -100
    ref = _reference("ignored_image", x, t, 1.0, per_image=True)
    got = _hip(dev, x, t, 1.0, per_image=True)
    _check(got, ref)
    others = soft_dice_ref(x[[0, 2]].double(), t[[0, 2]], per_image=True)
    assert abs(float(got[0]) * 3 - float(others) * 2) <= 3 * VAL_RTOL * float(others)
    assert torch.isfinite(got[0]) and torch.isfinite(got[1]).all()
    assert torch.equal(got[1][1], torch.zeros_like(got[1][1]))
    assert float(got[1][0].abs().max()) > 0


def test_soft_dice_is_deterministic(dev):
    """No float atomics: two runs are bit-identical, value and gradient."""
    x, t = _mc_inputs(VEC_SHAPES[-1], 7)
    for per_image in (False, True):
        a = _hip(dev, x, t, 0.7, per_image=per_image)
        b = _hip(dev, x, t, 0.7, per_image=per_image)
        assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])


def test_soft_dice_out_of_range_target_is_loud(dev):
    """A class target outside [0, K) that is not ignore_index, as test_cross_entropy_out_of_range_target_is_loud:
    NaN loss, NaN gradient at that pixel only, and the debug build records the index."""
    from pmu_hip import _lib as L
    from pmu_hip.loss import SoftDiceLoss
    g = torch.Generator().manual_seed(3)
    x = torch.randn(2, 3, 8, 8, generator=g)
    t = torch.randint(0, 3, (2, 8, 8), generator=g)
    t[0, 0, 0] = 3
    xd = x.to(dev).requires_grad_(True)
    got = SoftDiceLoss()(xd, t.to(dev))
    got.backward()
    assert torch.isnan(got).item()
    bad = torch.isnan(xd.grad)
    assert bad[0, :, 0, 0].all() and int(bad.sum()) == 3
    if L.debug_build():
        with pytest.raises(RuntimeError, match="index out of range"):
            L.debug_check()


@pytest.mark.parametrize("K,per_image", [(3, False), (3, True), (1, True)])
def test_soft_dice_raw_abi_stays_inside_its_workspace(dev, K, per_image):
    """pmu_softdice_fwd / _bwd called directly on a workspace of exactly pmu_softdice_ws bytes followed by a
    sentinel-filled guard: the guard is untouched, the results equal the wrapper's bit for bit, and the
    workspace begins with the coefficients a = 2 / (M S), b = (2 I + eps) / (M S^2) of the formula."""
    from pmu_hip import _lib as L
    from pmu_hip.loss import SoftDiceLoss
    N, H, W = 3, 24, 20
    g = torch.Generator().manual_seed(11)
    if K == 1:
        x = torch.rand(N, 1, H, W, generator=g)
        t = (torch.rand(N, 1, H, W, generator=g) > 0.5).float()
    else:
        x, t = _mc_inputs((N, K, H, W), 11)
    xd, td = x.to(dev), t.to(dev)
    nbytes = L.lib().pmu_softdice_ws(N, K, H * W)
    assert nbytes > 0 and nbytes % 8 == 0
    GUARD = 4096
    buf = torch.full((nbytes + GUARD,), 0xA5, dtype=torch.uint8, device=dev)
    loss = torch.zeros((), device=dev)
    dx = torch.empty_like(xd)
    gout = torch.tensor(0.7, device=dev)
    L.call("pmu_softdice_fwd", xd.data_ptr(), td.data_ptr(), N, K, H * W, 0, int(per_image), 0, -100,
           loss.data_ptr(), buf.data_ptr(), L.stream())
    L.call("pmu_softdice_bwd", xd.data_ptr(), td.data_ptr(), N, K, H * W, 0, int(per_image), -100,
           buf.data_ptr(), gout.data_ptr(), dx.data_ptr(), L.stream())
    torch.cuda.synchronize()
    assert bool((buf[nbytes:] == 0xA5).all())
    xw = xd.clone().requires_grad_(True)
    lw = SoftDiceLoss(per_image=per_image)(xw, td)
    (lw * 0.7).backward()
    assert torch.equal(lw.detach(), loss) and torch.equal(xw.grad, dx)
    # the coefficient block against the formula's sums
    R = N if per_image else 1
    coef = buf[:R * K * 8].view(torch.float32).view(R, K, 2).double().cpu()
    xr = x.double()
    if K == 1:
        p, tt = xr.reshape(N, 1, -1), t.double().reshape(N, 1, -1)
        valid = torch.ones_like(tt)
    else:
        p = torch.softmax(xr.reshape(N, K, -1), 1)
        ti = t.reshape(N, -1)
        valid = (ti != -100).double()[:, None]
        tt = torch.stack([ti == k for k in range(K)], 1).double()
    dims = (2,) if per_image else (0, 2)
    inter, S = (p * tt * valid).sum(dims), (p * valid).sum(dims) + (tt * valid).sum(dims) + EPS
    M = R * K
    want = torch.stack([2 / (M * S), (2 * inter + EPS) / (M * S * S)], -1).reshape(R, K, 2)
    assert float(((coef - want).abs() / want.abs()).max()) <= 1e-6


def test_soft_dice_rejects_more_than_eight_classes(dev):
    from pmu_hip.loss import SoftDiceLoss
    with pytest.raises(ValueError, match="at most 8"):
        SoftDiceLoss()(torch.zeros(1, 9, 4, 4, device=dev), torch.zeros(1, 4, 4, dtype=torch.long, device=dev))


def test_soft_dice_accepts_bf16_logits_under_autocast(dev):
    """Inputs are converted as _CE converts them: bf16 logits give the loss of their fp32 values."""
    from pmu_hip.loss import SoftDiceLoss
    x, t = _mc_inputs((2, 3, 16, 12), 2)
    xb = x.bfloat16()
    with torch.autocast("cuda", dtype=torch.bfloat16):
        xd = xb.to(dev).requires_grad_(True)
        got = SoftDiceLoss()(xd, t.to(dev))
    got.backward()
    ref = soft_dice_ref(xb.double(), t)
    assert abs(float(got) - float(ref)) <= VAL_RTOL * float(ref)
    assert xd.grad.dtype == torch.bfloat16 and torch.isfinite(xd.grad).all()


# ----------------------------------------------------------------------------- model level
def _oracle_step(sd, x, t, nlev, K, dtype=torch.float32, **kw):
    """unet_forward + soft_dice_ref on the CPU in ``dtype``: (out, loss, grads, work)."""
    from oracle.unet_ref import unet_forward, unet_param_keys
    keys = unet_param_keys(sd)
    sdt = {k: (v.to(dtype) if v.is_floating_point() else v.clone()) for k, v in sd.items()}
    params = {k: sdt[k].clone().requires_grad_(True) for k in keys}
    work = dict(sdt)
    work.update(params)
    out = unet_forward(work, x.to(dtype), nlev, K)
    loss = soft_dice_ref(out, t if K == 1 else t.squeeze(1), **kw)
    loss.backward()
    return out.detach(), loss.detach(), {k: params[k].grad for k in keys}, work


@pytest.mark.parametrize("filters,K,N,H,W", [([8, 16, 32], 3, 2, 40, 36), ([4, 8], 1, 3, 33, 29)])
def test_unet_dice_train_step_parity(dev, filters, K, N, H, W):
    """One training step of model.UNet under the Dice loss vs the fp32 oracle: output, loss, every
    parameter gradient.  (The oracle's own fp32-against-fp64 gradient noise at these cases is 5.8e-7 and
    3.5e-7 on the CPU: GRAD_TOL is a real bound.)"""
    from model import UNet
    from pmu_hip.loss import SoftDiceLoss
    torch.manual_seed(0)
    net = UNet(1, K, filters)
    sd = {k: v.clone() for k, v in net.state_dict().items()}
    x, t = phantom_batch(N, 1, H, W, K, 21)
    kw = dict(include_background=False) if K > 1 else {}
    out_ref, loss_ref, gref, _ = _oracle_step(sd, x, t, len(filters), K, **kw)
    net = net.to(dev).train()
    out = net(x.to(dev))
    loss = SoftDiceLoss(**kw)(out, t.to(dev) if K == 1 else t.to(dev).squeeze(1))
    loss.backward()
    named = dict(net.named_parameters())
    err, key = grad_err({k: named[k].grad for k in gref}, gref)
    print(f"out {max_abs(out, out_ref):.2e} loss {float(loss):.6f} ref {float(loss_ref):.6f} grad {err:.2e} {key}")
    assert max_abs(out, out_ref) <= ACT_TOL
    assert abs(float(loss) - float(loss_ref)) <= LOSS_RTOL * abs(float(loss_ref))
    assert err <= GRAD_TOL, (err, key)


def test_unet_dice_five_step_trajectory(dev):
    """Five steps of UNetTrainer(loss="dice") + FusedSGD(lr 0.05, momentum 0.9, clip 0.1) on one batch vs
    unet_forward + the formula + oracle.unet_ref.sgd_clip_step on the CPU in fp32: every step's loss within
    LOSS_RTOL, the final parameters within ACT_TOL."""
    from oracle.unet_ref import sgd_clip_step, unet_param_keys
    from pmu_hip.optim import FusedSGD
    from trainer import UNetTrainer
    torch.manual_seed(0)
    tr = UNetTrainer(dev, n_channels=1, n_classes=3, num_filters=[8, 16], loss="dice")
    sd = {k: v.detach().cpu().clone() for k, v in tr.net.state_dict().items()}
    keys = unet_param_keys(sd)
    bufs = {k: torch.zeros_like(sd[k]) for k in keys}
    x, t = phantom_batch(4, 1, 32, 32, 3, 21)
    xd, td = x.to(dev), t.to(dev)
    tr.net.train()
    opt = FusedSGD(tr.net.parameters(), lr=0.05, momentum=0.9, clip=0.1)
    for step in range(5):
        _, loss_ref, grads, work = _oracle_step(sd, x, t, 2, 3)
        cur = {k: sd[k].detach() for k in keys}
        sgd_clip_step(cur, grads, bufs, 0.05)
        sd = {k: (cur[k] if k in cur else work[k].detach()) for k in sd}
        opt.zero_grad()
        loss = tr.loss(xd, td, tr.predict(xd, td))
        loss.backward()
        opt.step()
        print(f"step {step}: loss {float(loss):.6f} ref {float(loss_ref):.6f}")
        assert abs(float(loss) - float(loss_ref)) <= LOSS_RTOL * abs(float(loss_ref)), step
    named = dict(tr.net.named_parameters())
    perr = max(max_abs(named[k], sd[k]) for k in keys)
    print(f"final parameters: max |d| {perr:.2e}")
    assert perr <= ACT_TOL


def test_trainers_loss_keyword(dev):
    """loss="ce+dice" is CrossEntropyLoss + SoftDiceLoss formed by autograd; "default" keeps the criterion
    types; "dice" on the one-class trainer takes the sigmoid head's probabilities."""
    from pmu_hip.loss import BCELoss, CrossEntropyLoss, SoftDiceLoss
    from trainer import UNetTrainer
    torch.manual_seed(0)
    tr = UNetTrainer(dev, n_classes=3, num_filters=[8, 16], loss="ce+dice")
    x, t = phantom_batch(2, 1, 32, 32, 3, 21)
    xd, td = x.to(dev), t.to(dev)
    pred = tr.predict(xd, td)
    got = tr.loss(xd, td, pred)
    want = CrossEntropyLoss()(pred, td.squeeze(1)) + SoftDiceLoss()(pred, td.squeeze(1))
    assert torch.equal(got.detach(), want.detach())
    got.backward()
    assert all(p.grad is not None and torch.isfinite(p.grad).all() for p in tr.net.parameters())
    assert type(UNetTrainer(dev, n_classes=3, num_filters=[8, 16]).criterion) is CrossEntropyLoss
    assert type(UNetTrainer(dev, n_classes=3, num_filters=[8, 16], loss="default").criterion) is CrossEntropyLoss
    one = UNetTrainer(dev, n_classes=1, num_filters=[8, 16], loss="default")
    assert type(one.criterion) is BCELoss
    one = UNetTrainer(dev, n_classes=1, num_filters=[8, 16], loss="dice")
    x1, t1 = phantom_batch(2, 1, 32, 32, 1, 21)
    p1 = one.predict(x1.to(dev), t1.to(dev))
    l1 = one.loss(x1.to(dev), t1.to(dev), p1)
    ref = soft_dice_ref(p1.detach().double().cpu(), t1)
    assert abs(float(l1) - float(ref)) <= VAL_RTOL * float(ref)


def _prob_net(dev, **kw):
    from model import ProbabilisticUnet
    torch.manual_seed(0)
    return ProbabilisticUnet(1, 3, [6, 12, 24], latent_dim=5, no_convs_fcomb=3, beta=10.0, **kw).to(dev).train()


def test_elbo_with_dice_reconstruction_term(dev):
    """recon_loss="ce+dice": -elbo = CE_sum + dice_weight * P * L_dice + beta * kl, recomputed on the CPU in
    float64 from net.reconstruction and net.kl; every parameter that takes part gets a finite gradient.
    "dice" alone drops the CE term.  The default recon_loss is the summed CE, unchanged."""
    import torch.nn.functional as F
    from trainer import ProbUNetTrainer
    g = torch.Generator().manual_seed(9)
    N, H, W = 2, 33, 29
    x = torch.rand(N, 1, H, W, generator=g).to(dev)
    segm = torch.randint(0, 3, (N, 1, H, W), generator=g).float().to(dev)
    tgt = segm.long().squeeze(1).cpu()

    def terms(net):
        rec = net.reconstruction.detach().double().cpu()
        return F.cross_entropy(rec, tgt, reduction="sum"), segm.numel() * soft_dice_ref(rec, tgt), float(net.kl)

    net = _prob_net(dev, recon_loss="ce+dice", dice_weight=0.5)
    net.forward(x, segm, training=True)
    loss = -net.elbo(segm)
    ce, dice, kl = terms(net)
    want = float(ce + 0.5 * dice + 10.0 * kl)
    assert abs(float(loss) - want) <= LOSS_RTOL * abs(want)
    assert abs(float(net.reconstruction_loss) - float(ce + 0.5 * dice)) <= LOSS_RTOL * float(ce + 0.5 * dice)
    loss.backward()
    named = dict(net.named_parameters())
    for part in ("unet.", "prior.", "posterior.", "fcomb."):
        ps = [p for k, p in named.items() if k.startswith(part) and not k.startswith("unet.outc")]
        assert ps and all(p.grad is not None and torch.isfinite(p.grad).all() for p in ps), part

    net = _prob_net(dev)
    assert net.recon_loss == "ce" and net.dice_weight == 1.0
    net.recon_loss = "dice"            # set after construction
    net.forward(x, segm, training=True)
    loss = -net.elbo(segm)
    ce, dice, kl = terms(net)
    assert abs(float(loss) - float(dice + 10.0 * kl)) <= LOSS_RTOL * float(dice + 10.0 * kl)

    net = _prob_net(dev)
    net.forward(x, segm, training=True)
    net.elbo(segm)
    ce, _, _ = terms(net)
    assert abs(float(net.reconstruction_loss) - float(ce)) <= 1e-5 * float(ce)
    net.recon_loss = "foo"
    with pytest.raises(ValueError):
        net.elbo(segm)

    tr = ProbUNetTrainer(dev, n_classes=3, num_filters=[6, 12, 24], loss="ce+dice")
    assert tr.net.recon_loss == "ce+dice"
    assert ProbUNetTrainer(dev, n_classes=3, num_filters=[6, 12, 24]).net.recon_loss == "ce"
