"""Inputs, float64 references and error-bound units shared by tests/test_loss_kernels_gpu.py,
tests/test_sgd_kernel_gpu.py and tests/test_tail_bounds_cpu.py: the GPU modules hold the HIP kernels to
these bounds, the CPU module shows that a plain fp32 restatement of each kernel's formula meets the same
bounds on the same inputs (so no bound fails for fp32 arithmetic as such).

Everything here is CPU torch.  References are float64 functions of the fp32 inputs; scalar kernel
arguments (lr, momentum, clip, gscale, the 1e-12 floor) enter as their float32 values (f32()).
u = 2^-24 is fp32's unit roundoff."""
import torch

U = 2.0 ** -24
DENORM_MIN = 2.0 ** -149


def f32(v):
    """The float32 value of the Python float v, as a Python float (what a `float` kernel argument holds)."""
    return float(torch.tensor(v, dtype=torch.float32))


# ------------------------------------------------------------------------------------------- BCE
# hard ceilings on the admitted multiple of each unit (forward units and the BCE backward: 16; CE backward: 4)
CEIL_FWD, CEIL_BCE_BWD, CEIL_CE_BWD = 16, 16, 4
BCE_FLOOR = f32(1e-12)
# 0 and 1: the -100 clamp; 1e-30: log(1 - y) rounds to log 1; 1 - 2^-24: the largest y below 1; 2^-149: the
# smallest denormal, log below the clamp either way; 1e-40: a denormal whose log (-92.1) is above the clamp
BCE_EDGES = (0.0, 1.0, 1e-30, 1.0 - 2.0 ** -24, 0.5, DENORM_MIN, 1e-40)
BCE_SIZES = (1, 255, 256, 257, 2049, 600001, 2097152 + 4097)


def bce_inputs(n, seed=0):
    """(y, t, g) fp32 of n elements: y = rand with the edge list at the head (targets 1, 0, soft) and at the
    tail (soft), the first half of the other targets binary, the second half soft in (0, 1); g = randn."""
    gen = torch.Generator().manual_seed(1000 + seed)
    y = torch.rand(n, generator=gen)
    soft = torch.rand(n, generator=gen).clamp(2.0 ** -20, 1 - 2.0 ** -20)
    hard = (torch.rand(n, generator=gen) > 0.5).float()
    t = torch.where(torch.arange(n) < (n + 1) // 2, hard, soft)
    ne = len(BCE_EDGES)
    edges = torch.tensor(BCE_EDGES, dtype=torch.float64).float()
    head = min(n, 3 * ne)
    i = torch.arange(head)
    y[:head] = edges[i % ne]
    t[:head] = torch.where(i < ne, torch.ones(head), torch.where(i < 2 * ne, torch.zeros(head), soft[:head]))
    if n >= 4 * ne:
        y[n - ne:] = edges
        t[n - ne:] = soft[n - ne:]
    g = torch.randn(n, generator=gen)
    return y, t, g


def bce_fwd_ref(y, t):
    """float64 loss per element and its bound unit B = u (|t ly| + |(1 - t) l1y|) + u (1 - t)."""
    y6, t6 = y.double(), t.double()
    ly = torch.log(y6).clamp_min(-100.0)
    l1y = torch.log(1.0 - y6).clamp_min(-100.0)
    a, b = t6 * ly, (1.0 - t6) * l1y
    return -(a + b), U * (a.abs() + b.abs()) + U * (1.0 - t6)


def bce_bwd_ref(y, t, g):
    """float64 g (y - t) / max(y (1 - y), float32(1e-12)); (unit u |ref|, absolute gradual-underflow term)."""
    y6, t6, g6 = y.double(), t.double(), g.double()
    ref = g6 * (y6 - t6) / (y6 * (1.0 - y6)).clamp_min(BCE_FLOOR)
    return ref, U * ref.abs(), (DENORM_MIN / 1e-12) * g6.abs().clamp_min(1.0)


def bce_fwd_f32(y, t):
    """The kernel's formula in fp32 torch (csrc/loss.hip bce_elem)."""
    ly = torch.log(y).clamp_min(-100.0)
    l1y = torch.log(1.0 - y).clamp_min(-100.0)
    return -(t * ly + (1.0 - t) * l1y)


def bce_bwd_f32(y, t, g):
    return g * (y - t) / ((1.0 - y) * y).clamp_min(torch.tensor(1e-12, dtype=torch.float32))


# -------------------------------------------------------------------------------------------- CE
# (N, K, HW): one pixel; HW == 1 over 65 images; two classes on an odd map; G = 293 partial blocks (a ragged
# second pass of the final kernel) at K = 8; K = 33 on two blocks; P = 2,097,156 > 1024 * 2048 (block cap)
CE_CASES = ((1, 1, 1), (65, 3, 1), (3, 2, 357), (2, 8, 300001), (1, 33, 2049), (4, 3, 524289))
CE_IGNORES = (-100, 255, 0)
CE_BAD_TARGETS = (2 ** 32 + 1, -1)


def ce_inputs(N, K, HW, ignore, seed=0):
    """(x, tgt, g, bad): logits x [N][K][HW] = 3 randn with a dyadic patch (multiples of 1/4) and a patch
    where one class leads by 200; class targets [N][HW] with about 1 in 8 pixels ignored, image 0 ignored
    entirely and image 1 not at all when N >= 2; g = randn per pixel.  bad: pixel indices (into N * HW) whose
    targets the caller may overwrite with CE_BAD_TARGETS — none when there are fewer than 8 pixels."""
    gen = torch.Generator().manual_seed(2000 + seed + 7 * K + N)
    P = N * HW
    xf = torch.randn(P, K, generator=gen) * 3                 # [pixel][class]
    q = P // 4
    if q:
        xf[:q] = torch.randint(-16, 17, (q, K), generator=gen).float() / 4
        xf[q + torch.arange(q), torch.randint(0, K, (q,), generator=gen)] += 200.0
    x = xf.reshape(N, HW, K).permute(0, 2, 1).contiguous()
    if ignore == 0 and K > 1:
        tgt = torch.randint(1, K, (N, HW), generator=gen)
    else:
        tgt = torch.randint(0, K, (N, HW), generator=gen)
    ign = torch.rand(N, HW, generator=gen) < 0.125
    if N >= 2:
        ign[0] = True
        ign[1] = False
    tgt[ign] = ignore
    g = torch.randn(N, HW, generator=gen)
    bad = [P - 1, P - 1 - P // 3] if P >= 8 else []
    return x, tgt, g, bad


def ce_ref(x, tgt, g, ignore):
    """float64 per-pixel loss [N][HW], dx [N][K][HW], their bound units, the valid mask and the NaN mask
    (targets outside [0, K) that are not ignore_index)."""
    N, K, HW = x.shape
    x6 = x.double()
    M = x6.max(dim=1).values
    sumexp = torch.exp(x6 - M[:, None]).sum(dim=1)
    lse = torch.log(sumexp)
    valid = tgt != ignore
    nan = valid & ((tgt < 0) | (tgt >= K))
    ok = valid & ~nan
    tc = torch.where(ok, tgt, torch.zeros_like(tgt))
    xt = x6.gather(1, tc[:, None]).squeeze(1)
    loss = torch.where(ok, (M + lse) - xt, torch.zeros_like(M))
    unit_l = U * (2 * M.abs() + 2 * lse + xt.abs() + K + 4)
    sm = torch.exp(x6 - M[:, None]) / sumexp[:, None]
    onehot = torch.zeros_like(sm).scatter_(1, tc[:, None], 1.0)
    dx = g.double()[:, None] * (sm - onehot) * ok[:, None]
    unit_d = (U * g.double().abs() * (K + 6))[:, None].expand_as(dx)
    return loss, unit_l, dx, unit_d, valid, nan


def ce_fwd_f32(x, tgt, ignore):
    """The kernel's forward in fp32 torch (valid, in-range targets; others 0)."""
    K = x.shape[1]
    m = x.max(dim=1).values
    se = torch.zeros_like(m)
    for k in range(K):
        se = se + torch.exp(x[:, k] - m)
    ok = (tgt != ignore) & (tgt >= 0) & (tgt < K)
    tc = torch.where(ok, tgt, torch.zeros_like(tgt))
    return torch.where(ok, (m + torch.log(se)) - x.gather(1, tc[:, None]).squeeze(1), torch.zeros_like(m))


def ce_bwd_f32(x, tgt, g, ignore):
    K = x.shape[1]
    m = x.max(dim=1).values
    se = torch.zeros_like(m)
    for k in range(K):
        se = se + torch.exp(x[:, k] - m)
    inv = 1.0 / se
    ok = (tgt != ignore) & (tgt >= 0) & (tgt < K)
    tc = torch.where(ok, tgt, torch.zeros_like(tgt))
    sm = torch.exp(x - m[:, None]) * inv[:, None]
    onehot = torch.zeros_like(sm).scatter_(1, tc[:, None], 1.0)
    return g[:, None] * (sm - onehot) * ok[:, None]


# ------------------------------------------------------------------------------------------- SGD
SGD_EXACT_LR = 2.0 ** -4
SGD_EXACT_MOMENTA = (0.0, 0.5, 0.75)
SGD_EXACT_GSCALES = (1.0, 0.5, 0.25)
SGD_EXACT_CLIPS = (2.0 ** -3, 0.0, -1.0)
SGD_LR, SGD_MOMENTUM, SGD_CLIP, SGD_GSCALE = f32(0.05), f32(0.9), f32(0.1), f32(1.0 / 3.0)


def sgd_exact_inputs(n, seed=0):
    """p, buf and two steps' gradients: multiples of 2^-8 in [-4, 4] (see tests/test_sgd_kernel_gpu.py)."""
    gen = torch.Generator().manual_seed(3000 + seed)
    return tuple(torch.randint(-1024, 1025, (n,), generator=gen).float() / 256 for _ in range(4))


def sgd_bounded_inputs(n, seed=0):
    """p, g, buf = randn; gradients +inf, -inf, +inf and NaN at elements 1, 2, n // 2 and n - 1 of a tensor of
    8 or more elements."""
    gen = torch.Generator().manual_seed(4000 + seed)
    p, g, b = (torch.randn(n, generator=gen) for _ in range(3))
    if n >= 8:
        g[1], g[2], g[n // 2], g[n - 1] = float("inf"), float("-inf"), float("inf"), float("nan")
    return p, g, b


def sgd_ref(p, g, b, gscale, lr, momentum, clip):
    """float64 step -> (p', buf', bound on buf', bound on p'); non-finite gradients follow IEEE arithmetic
    (clip > 0 clamps +-inf to +-clip, NaN stays NaN)."""
    p6, g6, b6 = p.double(), g.double(), b.double()
    gv = g6 * gscale
    if clip > 0:
        gv = torch.where(torch.isnan(gv), gv, gv.clamp(-clip, clip))
    mb = momentum * b6
    bv = mb + gv
    pn = p6 - lr * bv
    bb = 3 * U * (mb.abs() + gv.abs())
    bp = 2 * U * (p6.abs() + (lr * bv).abs()) + lr * bb
    return pn, bv, bb, bp


def sgd_f32(p, g, b, gscale, lr, momentum, clip):
    """The kernel's arithmetic in fp32 torch, unfused (csrc/sgd.hip sgd_one fuses both multiply-adds)."""
    one = lambda v: torch.tensor(v, dtype=torch.float32)
    gv = g * one(gscale)
    if clip > 0:
        gv = torch.where(torch.isnan(gv), gv, gv.clamp(-clip, clip))
    bv = one(momentum) * b + gv
    return p - one(lr) * bv, bv


def within(got64, ref, bound):
    """|got - ref| <= bound wherever ref is finite; the same infinity / NaN wherever it is not."""
    fin = torch.isfinite(ref)
    ok = torch.where(fin, (got64 - ref).abs() <= bound,
                     (got64 == ref) | (torch.isnan(got64) & torch.isnan(ref)))
    return ok


def worst_ratio(got64, ref, unit, absolute=None):
    """max over finite ref of (|got - ref| - absolute) / unit (0 where the unit is 0 and the error is too)."""
    fin = torch.isfinite(ref)
    err = (got64 - ref).abs()
    if absolute is not None:
        err = (err - absolute).clamp_min(0.0)
    r = torch.where(unit > 0, err / unit.clamp_min(1e-300), torch.where(err > 0, torch.full_like(err, float("inf")),
                                                                        torch.zeros_like(err)))
    r = torch.where(fin, r, torch.zeros_like(r))
    return float(r.max()) if r.numel() else 0.0
