"""GPU tests of the boundary loss: the signed distance map (pmu_hip.boundary.signed_distance on
pmu_boundary_map), the loss and its gradient (pmu_hip.loss.BoundaryLoss on pmu_boundary_fwd / _bwd) and the
wiring into the trainers and the ELBO.

The map is held to the numpy restatement tests/boundary_ref.py bit for bit.  The loss and gradient are held to
the formula of include/pmunet_hip.h in float64 on the CPU (autograd for the gradient), with phi taken from the
restatement, at the tolerances tests/test_dice_loss_gpu.py and tests/test_loss_gpu.py hold the soft Dice loss and
the CE to:
    value      |L - L_ref| <= 1e-5 A,   A = (1 / cnt) sum v |p_k phi_k|   (the signed sum cancels, L can be near 0)
    gradient   max |dx - dx_ref| <= 1e-5 max |dx_ref|.
(The kernel's arithmetic — fp32 softmax / sigmoid, fp64 products and sums, the fp32 backward with g / cnt rounded
to fp32 — emulated on the CPU over every loss case of this file stays within 3.1e-8 A on the value and 9.5e-7 of
max |dx_ref| on the gradient, the worst at K = 8 on the odd plane; the kernels themselves measured 3.1e-8 and
1.5e-6 on the same cases, the device's expf being the difference.)  Model-level bounds are helpers.LOSS_RTOL / GRAD_TOL.
"""
import pytest
import torch
import torch.nn.functional as F

import boundary_ref as R
from helpers import GRAD_TOL, LOSS_RTOL, grad_err, phantom_batch

pytestmark = pytest.mark.gpu

VAL_RTOL = 1e-5
GRAD_RTOL = 1e-5


def blobs(N, K, H, W, seed):
    """(N, H, W) class indices in blobs: the argmax of K coarse random fields, upsampled."""
    g = torch.Generator().manual_seed(seed)
    coarse = torch.randn(N, K, max(2, H // 32), max(2, W // 32), generator=g)
    return F.interpolate(coarse, size=(H, W), mode="bilinear", align_corners=False).argmax(1)


# ----------------------------------------------------------------------------- the map
def _case_random(K):
    g = torch.Generator().manual_seed(K)
    if K == 1:
        return torch.rand(3, 1, 21, 17, generator=g), K, None
    t = torch.randint(0, K, (3, 21, 17), generator=g)
    t[1, 2, :6] = -100

    def check(m):
        assert not m[1, :, 2, :6].any()     # the ignored run belongs to no class
    return t, K, check


def _case_width(W):
    g = torch.Generator().manual_seed(W)
    return torch.randint(0, 3, (2, 9, W), generator=g), 3, None


def _case_line(H, W):
    t = torch.zeros(1, H, W, dtype=torch.long)
    flat = t.view(-1)
    flat[5] = 1
    flat[700:703] = 1
    flat[1023] = 1
    return t, 2, None


def _case_single_member():
    t = torch.zeros(1, 300, 300, dtype=torch.long)
    t[0, 0, 0] = 1

    def check(m):
        assert int(m[0, 1].sum()) == 1 and m[0, 1, 0, 0]
    return t, 2, check


def _case_single_non_member():
    t = torch.ones(1, 300, 300, dtype=torch.long)
    t[0, 299, 0] = 0

    def check(m):
        assert int((~m[0, 1]).sum()) == 1 and not m[0, 1, 299, 0]
    return t, 2, check


def _case_absent_in_one_image():
    g = torch.Generator().manual_seed(3)
    t = torch.randint(0, 3, (2, 16, 20), generator=g)
    t[0][t[0] == 2] = 1

    def check(m):
        assert not m[0, 2].any() and m[1, 2].any() and not m[1, 2].all()
    return t, 3, check


def _case_full_in_one_image():
    g = torch.Generator().manual_seed(4)
    t = torch.randint(0, 2, (2, 16, 20), generator=g)
    t[0] = 1

    def check(m):
        assert m[0, 1].all() and not m[0, 0].any() and m[1, 1].any() and not m[1, 1].all()
    return t, 2, check


def _case_borders():
    t = torch.zeros(1, 20, 24, dtype=torch.long)
    t[0, :, 11:13] = 1
    t[0, 9:11, :] = 1

    def check(m):
        f = m[0, 1]
        assert f[0].any() and f[-1].any() and f[:, 0].any() and f[:, -1].any() and not f.all()
    return t, 2, check


MAP_CASES = {
    "random_K1": lambda: _case_random(1), "random_K2": lambda: _case_random(2), "random_K3": lambda: _case_random(3),
    "random_K8": lambda: _case_random(8),
    "W70": lambda: _case_width(70),          # a partial second ballot word
    "W130": lambda: _case_width(130),        # a partial third
    "1x1024": lambda: _case_line(1, 1024), "1024x1": lambda: _case_line(1024, 1),
    "single_member_300": _case_single_member, "single_non_member_300": _case_single_non_member,
    "absent_in_one_image": _case_absent_in_one_image, "full_in_one_image": _case_full_in_one_image,
    "touching_all_borders": _case_borders,
    "blobs_4x3x256x320": lambda: (blobs(4, 3, 256, 320, 6), 3, None),
}
_MAPS = {}


def _map_ref(name):
    """(target, K, restated map) of a map case, computed once."""
    if name not in _MAPS:
        t, K, check = MAP_CASES[name]()
        if check is not None:
            check(torch.from_numpy(R.membership(t, K)))
        _MAPS[name] = (t, K, R.signed_map(t, K))
    return _MAPS[name]


def _bits_equal(a, b):
    return a.dtype == b.dtype == torch.float32 and a.shape == b.shape and torch.equal(a.view(torch.int32),
                                                                                    b.view(torch.int32))


@pytest.mark.parametrize("name", list(MAP_CASES))
def test_signed_distance_is_bit_equal_to_the_restatement(dev, name):
    from pmu_hip.boundary import signed_distance
    t, K, want = _map_ref(name)
    got = signed_distance(t.to(dev), K).cpu()
    bad = int((got.view(torch.int32) != want.view(torch.int32)).sum())
    print(f"{name}: {tuple(want.shape)} range {float(want.min()):.3f}..{float(want.max()):.3f} mismatches {bad}")
    assert _bits_equal(got, want)


def test_small_maps_equal_the_brute_force_minimum(dev):
    """The restatement's separable form is itself checked against the brute force on the CPU; here the kernel
    meets the brute force directly on the small random cases."""
    from pmu_hip.boundary import signed_distance
    for name in ("random_K1", "random_K3"):
        t, K, _ = _map_ref(name)
        assert _bits_equal(signed_distance(t.to(dev), K).cpu(), R.signed_map(t, K, plane=R.brute_plane))


# ----------------------------------------------------------------------------- loss and gradient
def _loss_inputs(name):
    """(x, t, kw, scale) of a loss case; targets in blobs (or random classes at the small odd planes), a run of
    ignored pixels where the case says so."""
    g = torch.Generator().manual_seed(len(name))
    kind, *rest = name.split(":")
    if kind == "odd":          # HW = 357: odd, every second class plane misaligned, the scalar path
        K, bg = int(rest[0]), rest[1] == "bg"
        x = torch.randn(3, K, 21, 17, generator=g) * 3
        t = torch.randint(0, K, (3, 21, 17), generator=g)
        t[1, 2, :6] = -100
        return x, t, dict(include_background=bg), 0.7 if (K + bg) % 2 else 1.0
    if kind == "vec":          # HW % 4 == 0: the 16-byte loads
        N, K, H, W = (int(v) for v in rest)
        x = torch.randn(N, K, H, W, generator=g) * 3
        t = blobs(N, K, H, W, 8)
        t[N // 2, 2, :6] = -100
        return x, t, {}, 0.7
    if kind == "bin":          # one class: probabilities, or logits with the sigmoid in the kernel
        logits = rest[0] == "logits"
        x = torch.randn(4, 1, 33, 29, generator=g) * 4 if logits else torch.rand(4, 1, 33, 29, generator=g)
        t = (blobs(4, 2, 33, 29, 9) == 1).float()[:, None]
        return x, t, dict(from_logits=logits), 0.7
    if kind == "all_ignored":
        x = torch.randn(2, 3, 8, 12, generator=g)
        return x, torch.full((2, 8, 12), -100, dtype=torch.long), {}, 1.0
    raise KeyError(name)


LOSS_CASES = [f"odd:{K}:{bg}" for K in (2, 3, 5, 8) for bg in ("bg", "nobg")] + \
    ["vec:2:3:32:40", "vec:4:2:256:256", "bin:probs", "bin:logits"]
_LOSS_REF = {}


def _loss_ref(name):
    """(x, t, kw, scale, L_ref, A, dx_ref) in float64 on the CPU with the restated map, computed once."""
    if name not in _LOSS_REF:
        x, t, kw, scale = _loss_inputs(name)
        phi = R.signed_map(t, x.shape[1])
        xr = x.double().requires_grad_(True)
        loss = R.boundary_loss_ref(xr, t, phi, **kw)
        (loss * scale).backward()
        _LOSS_REF[name] = (x, t, kw, scale, float(loss.detach()), R.boundary_scale_ref(x.double(), t, phi, **kw),
                           xr.grad.detach())
    return _LOSS_REF[name]


def _hip(dev, x, t, scale, **kw):
    from pmu_hip.loss import BoundaryLoss
    xd = x.to(dev).requires_grad_(True)
    loss = BoundaryLoss(**kw)(xd, t.to(dev))
    (loss * scale).backward()
    return loss.detach().cpu(), xd.grad.detach().cpu()


@pytest.mark.parametrize("name", LOSS_CASES)
def test_boundary_loss_and_gradient(dev, name):
    x, t, kw, scale, loss_ref, A, dx_ref = _loss_ref(name)
    loss, dx = _hip(dev, x, t, scale, **kw)
    verr = abs(float(loss) - loss_ref) / A
    gerr = float((dx.double() - dx_ref).abs().max()) / float(dx_ref.abs().max())
    print(f"{name}: loss {float(loss):.8f} ref {loss_ref:.8f} A {A:.6f} err/A {verr:.2e}  grad err {gerr:.2e}")
    assert loss.dtype == torch.float32 and loss.shape == () and A > 0
    assert verr <= VAL_RTOL, (name, verr)
    assert dx.shape == dx_ref.shape and gerr <= GRAD_RTOL, (name, gerr)
    ignored = (t == -100) if x.shape[1] > 1 else torch.zeros(0, dtype=torch.bool)
    if ignored.any():
        assert not dx.movedim(1, -1)[ignored].any()     # exactly 0 at the ignored pixels
    if x.shape[1] > 1 and not kw.get("include_background", False):
        assert float(dx[:, 0].abs().max()) > 0           # the background logit still moves (through the softmax)


def test_boundary_loss_of_an_all_ignored_batch_is_zero(dev):
    x, t, kw, scale = _loss_inputs("all_ignored")
    loss, dx = _hip(dev, x, t, scale, **kw)
    assert float(loss) == 0.0 and not dx.any() and torch.isfinite(dx).all()


def test_boundary_loss_is_deterministic(dev):
    """No float atomics: two runs give the same bits for phi, L and dx."""
    from pmu_hip.boundary import signed_distance
    x, t, kw, scale = _loss_inputs("vec:4:2:256:256")
    a, b = _hip(dev, x, t, scale, **kw), _hip(dev, x, t, scale, **kw)
    assert torch.equal(a[0], b[0]) and _bits_equal(a[1], b[1])
    td = t.to(dev)
    assert _bits_equal(signed_distance(td, 2), signed_distance(td, 2))


@pytest.mark.parametrize("K", [3, 1])
def test_boundary_raw_abi_stays_inside_its_workspace(dev, K):
    """pmu_boundary_map / _fwd / _bwd called directly on a workspace of exactly pmu_boundary_ws bytes followed by
    a sentinel-filled guard: the guard is untouched and phi, L and dx equal the wrappers' bit for bit; the count
    the forward leaves for the backward is (valid pixels) x (classes)."""
    from pmu_hip import _lib as L
    from pmu_hip.boundary import signed_distance
    from pmu_hip.loss import BoundaryLoss
    N, H, W = 3, 24, 70
    g = torch.Generator().manual_seed(11)
    if K == 1:
        x = torch.rand(N, 1, H, W, generator=g)
        t = (blobs(N, 2, H, W, 12) == 1).float()[:, None]
    else:
        x = torch.randn(N, K, H, W, generator=g)
        t = blobs(N, K, H, W, 12)
        t[1, 2, :6] = -100
    xd, td = x.to(dev), t.to(dev)
    nbytes = L.lib().pmu_boundary_ws(N, K, H, W)
    assert nbytes > 0 and nbytes % 8 == 0
    GUARD = 4096
    buf = torch.full((nbytes + GUARD,), 0xA5, dtype=torch.uint8, device=dev)
    phi = torch.empty(N, K, H, W, device=dev)
    loss = torch.zeros((), device=dev)
    count = torch.zeros((), dtype=torch.float64, device=dev)
    dx = torch.empty_like(xd)
    gout = torch.tensor(0.7, device=dev)
    first = 0 if K == 1 else 1
    L.call("pmu_boundary_map", td.data_ptr(), int(K == 1), N, K, H, W, -100, phi.data_ptr(), buf.data_ptr(), L.stream())
    L.call("pmu_boundary_fwd", xd.data_ptr(), td.data_ptr(), phi.data_ptr(), N, K, H * W, 0, first, -100,
           loss.data_ptr(), count.data_ptr(), buf.data_ptr(), L.stream())
    L.call("pmu_boundary_bwd", xd.data_ptr(), td.data_ptr(), phi.data_ptr(), N, K, H * W, 0, first, -100,
           gout.data_ptr(), count.data_ptr(), dx.data_ptr(), L.stream())
    torch.cuda.synchronize()
    assert bool((buf[nbytes:] == 0xA5).all())
    assert _bits_equal(phi, signed_distance(td, K))
    xw = xd.clone().requires_grad_(True)
    lw = BoundaryLoss()(xw, td)
    (lw * 0.7).backward()
    assert torch.equal(lw.detach(), loss) and _bits_equal(xw.grad, dx)
    assert float(count) == (N * H * W - (6 if K > 1 else 0)) * (K - first)


def test_boundary_loss_input_rules(dev):
    from pmu_hip.loss import BoundaryLoss
    z = torch.zeros(1, 4, 4, dtype=torch.long, device=dev)
    with pytest.raises(ValueError, match="at most 8"):
        BoundaryLoss()(torch.zeros(1, 9, 4, 4, device=dev), z)
    with pytest.raises(ValueError, match="class-index targets"):
        BoundaryLoss()(torch.zeros(1, 3, 4, 4, device=dev), z.float())
    with pytest.raises(ValueError, match="takes logits"):
        BoundaryLoss(from_logits=False)(torch.zeros(1, 3, 4, 4, device=dev), z)
    with pytest.raises(ValueError, match=r"not \(N, K, H, W\)"):
        BoundaryLoss()(torch.zeros(1, 3, 16, device=dev), torch.zeros(1, 16, dtype=torch.long, device=dev))
    with pytest.raises(RuntimeError, match="does not match"):
        BoundaryLoss()(torch.zeros(1, 3, 4, 4, device=dev), torch.zeros(1, 4, 5, dtype=torch.long, device=dev))


# ----------------------------------------------------------------------------- wiring
def test_unet_trainer_ce_plus_boundary(dev):
    """loss="ce+boundary": the criterion is CrossEntropyLoss + weight * BoundaryLoss formed by autograd, the two
    terms recomputed separately; changing ``weight`` between two calls changes the value as the formula says."""
    from pmu_hip.loss import BoundaryLoss, CrossEntropyLoss, RegionPlusBoundaryLoss
    from trainer import UNetTrainer
    torch.manual_seed(0)
    tr = UNetTrainer(dev, n_classes=3, num_filters=[8, 16], loss="ce+boundary")
    assert type(tr.criterion) is RegionPlusBoundaryLoss and tr.criterion.weight == 0.01
    x, t = phantom_batch(2, 1, 32, 32, 3, 21)
    xd, td = x.to(dev), t.to(dev)
    pred = tr.predict(xd, td)
    ce = CrossEntropyLoss()(pred, td.squeeze(1)).detach()
    bd = BoundaryLoss()(pred, td.squeeze(1)).detach()
    assert float(bd) != 0.0
    got = tr.loss(xd, td, pred)
    assert torch.equal(got.detach(), ce + 0.01 * bd)
    tr.criterion.weight = 0.3
    assert torch.equal(tr.loss(xd, td, pred).detach(), ce + 0.3 * bd)
    got.backward()
    assert all(p.grad is not None and torch.isfinite(p.grad).all() for p in tr.net.parameters())


def test_unet_trainer_ce_plus_boundary_step_matches_the_oracle(dev):
    """One forward / backward of UNetTrainer(loss="ce+boundary") against oracle.unet_ref's forward with CE +
    weight * the restated loss under autograd on the CPU: the loss and every parameter gradient."""
    from oracle.unet_ref import unet_forward, unet_param_keys
    from trainer import UNetTrainer
    torch.manual_seed(0)
    tr = UNetTrainer(dev, n_classes=3, num_filters=[8, 16], loss="ce+boundary")
    tr.criterion.weight = 0.05
    sd = {k: v.detach().cpu().clone() for k, v in tr.net.state_dict().items()}
    x, t = phantom_batch(2, 1, 32, 32, 3, 21)
    keys = unet_param_keys(sd)
    params = {k: sd[k].clone().requires_grad_(True) for k in keys}
    work = dict(sd)
    work.update(params)
    out = unet_forward(work, x, 2, 3)
    tt = t.squeeze(1)
    loss_ref = F.cross_entropy(out, tt) + 0.05 * R.boundary_loss_ref(out, tt, R.signed_map(tt, 3))
    loss_ref.backward()
    tr.net.train()
    xd, td = x.to(dev), t.to(dev)
    loss = tr.loss(xd, td, tr.predict(xd, td))
    loss.backward()
    named = dict(tr.net.named_parameters())
    err, key = grad_err({k: named[k].grad for k in keys}, {k: params[k].grad for k in keys})
    loss, loss_ref = float(loss.detach()), float(loss_ref.detach())
    print(f"loss {loss:.6f} ref {loss_ref:.6f} grad {err:.2e} {key}")
    assert abs(loss - loss_ref) <= LOSS_RTOL * abs(loss_ref)
    assert err <= GRAD_TOL, (err, key)


def _soft_dice(x, t, eps=1e-6):
    """1 - mean Dice of softmax(x) against the one-hot target, pooled over the batch, every class (SoftDiceLoss's
    defaults; tests/test_dice_loss_gpu.py soft_dice_ref)."""
    N, K = x.shape[0], x.shape[1]
    p = torch.softmax(x.reshape(N, K, -1), 1)
    tt = torch.stack([t.reshape(N, -1) == k for k in range(K)], 1).to(x.dtype)
    d = (2 * (p * tt).sum((0, 2)) + eps) / (p.sum((0, 2)) + tt.sum((0, 2)) + eps)
    return 1 - d.mean()


def test_elbo_with_boundary_reconstruction_term(dev):
    """recon_loss="dice+boundary", boundary_weight 0.5: -elbo = dice_weight P L_dice + boundary_weight P L_boundary
    + beta kl, recomputed on the CPU in float64 from net.reconstruction and net.kl; "ce+boundary" swaps the Dice
    term for the summed CE; the weight is a plain attribute."""
    from model import ProbabilisticUnet
    from trainer import ProbUNetTrainer
    g = torch.Generator().manual_seed(9)
    N, H, W = 2, 33, 29
    x = torch.rand(N, 1, H, W, generator=g).to(dev)
    tgt = blobs(N, 3, H, W, 13)
    segm = tgt[:, None].float().to(dev)
    phi = R.signed_map(tgt, 3)
    P = segm.numel()

    def terms(net):
        rec = net.reconstruction.detach().double().cpu()
        return (F.cross_entropy(rec, tgt, reduction="sum"), P * _soft_dice(rec, tgt),
                P * R.boundary_loss_ref(rec, tgt, phi), float(net.kl))

    torch.manual_seed(0)
    net = ProbabilisticUnet(1, 3, [6, 12, 24], latent_dim=5, no_convs_fcomb=3, beta=10.0,
                            recon_loss="dice+boundary").to(dev).train()
    assert net.boundary_weight == 0.01
    net.boundary_weight = 0.5
    net.forward(x, segm, training=True)
    loss = -net.elbo(segm)
    ce, dice, bd, kl = terms(net)
    want = float(dice + 0.5 * bd + 10.0 * kl)
    print(f"-elbo {float(loss):.4f} want {want:.4f} (dice {float(dice):.4f} boundary {float(bd):.4f} kl {kl:.4f})")
    assert float(bd) != 0.0 and abs(float(loss) - want) <= LOSS_RTOL * abs(want)
    loss.backward()
    named = dict(net.named_parameters())
    for part in ("unet.", "prior.", "posterior.", "fcomb."):
        ps = [p for k, p in named.items() if k.startswith(part) and not k.startswith("unet.outc")]
        assert ps and all(p.grad is not None and torch.isfinite(p.grad).all() for p in ps), part

    net.zero_grad()
    net.recon_loss, net.boundary_weight = "ce+boundary", 2.0
    net.forward(x, segm, training=True)
    loss = -net.elbo(segm)
    ce, dice, bd, kl = terms(net)
    want = float(ce + 2.0 * bd + 10.0 * kl)
    assert abs(float(loss) - want) <= LOSS_RTOL * abs(want)
    assert abs(float(net.reconstruction_loss) - float(ce + 2.0 * bd)) <= LOSS_RTOL * abs(float(ce + 2.0 * bd))

    tr = ProbUNetTrainer(dev, n_classes=3, num_filters=[6, 12, 24], loss="ce+boundary")
    assert tr.net.recon_loss == "ce+boundary" and tr.net.boundary_weight == 0.01
