"""Kernel-level tests of the fused fusion-block kernels (csrc/fusion.hip), of the kernels that join them
(vrnet_bn_coef_{fwd,bwd}_from_chunks, vrnet_sa_cat_sums_f32) and of three small kernels no other test calls
(vrnet_enhance_fwd_f32, vrnet_cluster_ab_reduce_multi, vrnet_mt_copy_f32).

Every stage of the two chains is compared with a plain fp64 reference of that stage alone, fed with the device outputs of
the stage before it.  The references themselves are pinned against torch autograd in fp64 by the tests that need no GPU.

Tolerances:
  elementwise outputs   max |got - ref| <= 2e-6 max |ref|: at most eight fp32 roundings (6e-8 each) of terms no larger than the
                        tensor's scale, with a factor of four above that worst case.
  partial sums          against fp64 sums of the kernel's OWN fp32 outputs (a product of two fp32 values is exact in fp64, so only
                        the order of the additions differs): n 2^-52 sum |terms|, the worst case of two fp64 summation orders of n
                        terms.
  coefficients          1e-6 of the largest entry against the fp64 formulas applied to those reference sums (the figure
                        test_batch_norm_relu_chain uses for the same coefficient kernel).
  counts, (min, max), copies: exact.
The ReLU masks the backward kernels recompute from z are exact too: the inputs keep every fp64 pre-activation at least 1e-3
away from zero (a hundred times the fp32 evaluation error at this scale), asserted on the reference before any kernel runs."""
import functools
import math
from types import SimpleNamespace as NS

import numpy as np
import pytest
import torch
import torch.nn.functional as F

ELEM_TOL = 2e-6
COEF_TOL = 1e-6
MARGIN = 1e-3
EPS, MOMENTUM = 1e-3, 0.03

# (rows, C, chunks, fold chunks): the smallest shapes at which each mechanism of the kernels is live
SHAPES = [
    (3, 4, 1, 1),              # CV = 1, 3 live threads
    (7, 24, 3, 3),             # CV = 6: the column owners rotate between workgroups; two idle workgroups
    (2, 480, 15, 15),          # CV = 120, m = 15: 14 of 15 workgroups idle
    (513, 12, 6, 6),           # CV = 3, ragged tail
    (360, 40, 10, 10),         # CV = 10, m = 5 (stage 2 of `s`)
    (2000, 80, 80, 80),        # nano stage 2 width at 128 px scale
    (5, 1024, 3, 3),           # CV = 256, the upper bound
    (300, 1020, 255, 255),     # CV = 255, m = 255
    (53760, 40, 1050, 1025),   # 2 x 168 x 160 x 40: fold cap reached and rounded past it, the counts differ, 3 float4 per thread
]
VARIANTS = ["plain", "positive", "tiedmax"]      # positive: beta += 8 (unique minimum); tiedmax: the maximum of p on two elements
SHAPE_IDS = [f"{r}x{c}" for r, c, _, _ in SHAPES]


@pytest.fixture(scope="module")
def hip():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    import asy_vrnet_amd.hip as h
    return h


# ----------------------------------------------------------------------------------------------- fp64 references
def f64(t):
    return t.detach().double().cpu()


def ref_pre(z, A, D, S):
    """Pre-activation A (z - S) + D of the BatchNorm apply, per channel (last dimension)."""
    return f64(A) * (f64(z) - f64(S)) + f64(D)


def ref_bn_relu(z, A, D, S, res=None):
    y = torch.relu(ref_pre(z, A, D, S))
    return y if res is None else y + f64(res)


def ref_gain(p, x):
    """ImageEnhanceByRadar's gain: (1 + data_normal(p)) x with the batch-wide minimum and maximum of p."""
    p, x = f64(p), f64(x)
    mn, mx = p.min(), p.max()
    return (1.0 + (p - mn) / (mx - mn)) * x


def ref_gain_bwd(dt, x, p):
    """(dx, dp) of ref_gain: the gradient through min p and max p is spread evenly over the tied elements."""
    dt, x, p = f64(dt), f64(x), f64(p)
    mn, mx = p.min(), p.max()
    d = mx - mn
    dn = dt * x
    at_mn, at_mx = p == mn, p == mx
    g_mn = (-dn.sum() / d + (dn * (p - mn)).sum() / d ** 2) / at_mn.sum()
    g_mx = (-(dn * (p - mn)).sum() / d ** 2) / at_mx.sum()
    dx = dt * (1.0 + (p - mn) / d)
    dp = dn / d + at_mn * g_mn + at_mx * g_mx
    return dx, dp


def ref_col_sums(v, w=None):
    """Column (sum v, sum v w) of (rows, C) tensors; w = None: (sum v, sum v^2)."""
    v = f64(v)
    w = v if w is None else f64(w)
    return v.sum(0), (v * w).sum(0)


def ref_bn_coef_fwd(s1, s2, count, gamma, beta, eps, momentum, rmean, rvar):
    """Train-mode BatchNorm from column (sum, sumsq): y = A (z - S) + D, (mean, rstd) and the updated running statistics."""
    mean = s1 / count
    var = (s2 / count - mean * mean).clamp_min(0.0)
    rstd = 1.0 / torch.sqrt(var + eps)
    return NS(A=rstd * f64(gamma), D=f64(beta), S=mean, mean_rstd=torch.stack([mean, rstd], 1),
              rmean=(1.0 - momentum) * f64(rmean) + momentum * mean,
              rvar=(1.0 - momentum) * f64(rvar) + momentum * var * (count / (count - 1.0)))


def ref_bn_coef_bwd(s1, s2, count, mean_rstd, gamma):
    """Train-mode BatchNorm backward from column (sum dy', sum dy' z): dz = A dy' + E (z - S) + D, d gamma, d beta."""
    mu, r, g = f64(mean_rstd)[:, 0], f64(mean_rstd)[:, 1], f64(gamma)
    dxh = r * (s2 - mu * s1)
    m1, m2 = s1 / count, dxh / count
    return NS(A=g * r, E=-g * r * r * m2, D=-g * r * m1, S=mu, dgamma=dxh, dbeta=s1)


def ref_bn_bwd_apply(g, t, A, E, D, S, mask=None):
    g = f64(g)
    if mask is not None:
        g = g * mask
    return f64(A) * g + f64(E) * (f64(t) - f64(S)) + f64(D)


def ref_sa_coefs(x, prm, G):
    """Per-(sample, channel) gate coefficients of ShuffleAttention for x (B, HW, C): gate = sigmoid(P (x - Mn) + Q)."""
    B, HW, C = x.shape
    cp = C // (2 * G)
    x = f64(x)
    mean = x.mean(1)
    rstd = 1.0 / torch.sqrt(((x - mean[:, None, :]) ** 2).mean(1) + 1e-5)
    q = torch.arange(C)
    half, i = (q % (2 * cp)) // cp, q % cp
    cw, cb, sw, sb, gnw, gnb = (f64(t).reshape(-1)[i] for t in prm)
    P = torch.where(half == 0, torch.zeros(()).double(), sw * gnw * rstd)
    Q = torch.where(half == 0, cw * mean + cb, (sw * gnb + sb).expand(B, C))
    Mn = torch.where(half == 0, torch.zeros(()).double(), mean)
    return P, Q, Mn


def ref_sa_cat(x, P, Q, Mn, r):
    """cat[4 q .. 4 q + 3] = {x'[q], r[2 q], x'[C / 2 + q], r[2 q + 1]}, x' = x sigmoid(P (x - Mn) + Q); (B, HW, C) -> (B, HW, 2 C)."""
    x, r = f64(x), f64(r)
    B, HW, C = x.shape
    xp = x * torch.sigmoid(f64(P)[:, None, :] * (x - f64(Mn)[:, None, :]) + f64(Q)[:, None, :])
    out = torch.empty(B, HW, 2 * C, dtype=torch.float64)
    out[..., 0::4] = xp[..., :C // 2]
    out[..., 1::4] = r[..., 0::2]
    out[..., 2::4] = xp[..., C // 2:]
    out[..., 3::4] = r[..., 1::2]
    return out


# ----------------------------------------------------------------------------------------------- inputs
def _f32(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32))


@functools.lru_cache(maxsize=None)
def make_inputs(rows, C, variant="plain"):
    """z ~ 40 + 1.5 N(0, 1) (|mean| >> std: the cancellation-prone regime), explicit per-channel coefficients A = gamma r, D = beta,
    S ~ 40; elements whose fp64 pre-activation lies within MARGIN of zero are moved away from it by 2e-3 / A.  Shared, read-only."""
    rng = np.random.default_rng([rows, C, 20250])
    N = lambda *s: rng.standard_normal(s)
    z = _f32(40.0 + 1.5 * N(rows, C))
    S = _f32(40.0 + 0.1 * N(C))
    r = _f32(1.0 / (1.5 + 0.2 * rng.random(C)))
    gamma = _f32(1.0 + 0.3 * N(C))
    beta = _f32(0.5 * N(C) + (8.0 if variant == "positive" else 0.0))
    A, D = (gamma.double() * r.double()).float(), beta.clone()
    pre = ref_pre(z, A, D, S)
    bad = pre.abs() < MARGIN
    step = torch.where(pre >= 0, 1.0, -1.0).double() * (2e-3 / A.double())
    z = torch.where(bad, (z.double() + step).float(), z)
    return NS(rows=rows, C=C, n=rows * C, variant=variant, nudged=int(bad.sum()),
              z=z, A=A, D=D, S=S, gamma=gamma, ms1=torch.stack([S, r], 1).contiguous(),
              x=_f32(N(rows, C)), g=_f32(N(rows, C)), res=_f32(N(rows, C)), dx0=_f32(N(rows, C)),
              gamma2=_f32(1.0 + 0.3 * N(C)), beta2=_f32(0.5 * N(C)), rmean=_f32(0.1 * N(C)), rvar=_f32(rng.random(C) + 0.5))


def relu_mask(inp):
    """The ReLU mask of the reference; the margin makes it the mask of any fp32 evaluation too."""
    pre = ref_pre(inp.z, inp.A, inp.D, inp.S)
    assert pre.abs().min().item() >= MARGIN, "a pre-activation within the margin of zero has no defined mask bit"
    return pre > 0


# ----------------------------------------------------------------------------------------------- comparisons
def close(a, b, tol, what="", floor=1e-6):
    a, b = f64(a), f64(b)
    assert a.shape == b.shape, (what, a.shape, b.shape)
    assert torch.isfinite(a).all(), f"{what}: not finite"
    scale = max(b.abs().max().item(), floor)
    err = (a - b).abs().max().item() / scale
    print(f"{what}: rel err {err:.3e} (scale {scale:.3e})")
    assert err < tol, f"{what}: rel err {err:.3e} (scale {scale:.3e})"


def elem_close(got, ref, what):
    got, ref = f64(got), f64(ref)
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    assert torch.isfinite(got).all(), f"{what}: not finite"
    scale, err = ref.abs().max().item(), (got - ref).abs().max().item()
    print(f"{what}: max err {err:.3e}, {err / max(scale, 1e-300):.3e} of max |ref| = {scale:.3e}")
    assert err <= ELEM_TOL * scale, f"{what}: max err {err:.3e} > {ELEM_TOL} x {scale:.3e}"


def sums_close(got, terms, what):
    """got: sums over dimension 0 of `terms` (fp64, exact products of the kernel's own fp32 values) in another order."""
    got, terms = f64(got), f64(terms)
    ref, bound = terms.sum(0), terms.shape[0] * 2.0 ** -52 * terms.abs().sum(0)
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    assert torch.isfinite(got).all(), f"{what}: not finite"
    err = (got - ref).abs()
    worst = (err / bound.clamp_min(1e-300)).max().item()
    print(f"{what}: max err {err.max().item():.3e}, {worst:.3e} of the bound")
    assert (err <= bound).all(), f"{what}: {worst:.3e} of the fp64 summation bound"


def same_bits(a, b):
    a, b = a.detach().cpu().contiguous(), b.detach().cpu().contiguous()
    as_int = {torch.float32: torch.int32, torch.float64: torch.int64}
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(a.view(as_int.get(a.dtype, a.dtype)),
                                                                     b.view(as_int.get(b.dtype, b.dtype)))


# ----------------------------------------------------------------------------------------------- references against autograd (CPU)
def test_ref_bn_relu_and_column_sums_match_autograd():
    inp = make_inputs(37, 12)
    z, res = inp.z.double(), inp.res.double()
    gamma, beta, rm, rv = inp.gamma.double(), inp.beta2.double(), inp.rmean.double(), inp.rvar.double()
    rm_t, rv_t = rm.clone(), rv.clone()
    y = torch.relu(F.batch_norm(z, rm_t, rv_t, gamma, beta, True, MOMENTUM, EPS)) + res
    s1, s2 = ref_col_sums(z)
    assert torch.allclose(s1, z.sum(0), rtol=1e-14) and torch.allclose(s2, (z * z).sum(0), rtol=1e-14)
    c = ref_bn_coef_fwd(s1, s2, 37, gamma, beta, EPS, MOMENTUM, rm, rv)
    assert torch.allclose(ref_bn_relu(z, c.A, c.D, c.S, res), y, rtol=0, atol=1e-9)      # (sumsq - mean^2 at mean 40: ~1e-11)
    assert torch.allclose(ref_bn_relu(z, c.A, c.D, c.S), y - res, rtol=0, atol=1e-9)
    assert torch.allclose(c.rmean, rm_t, rtol=0, atol=1e-12) and torch.allclose(c.rvar, rv_t, rtol=0, atol=1e-11)
    assert torch.allclose(c.mean_rstd[:, 0], z.mean(0), rtol=1e-13)
    assert torch.allclose(c.mean_rstd[:, 1], 1.0 / torch.sqrt(z.var(0, unbiased=False) + EPS), rtol=1e-10)


def _gain_cases():
    rng = np.random.default_rng(5)
    base = _f32(rng.standard_normal((23, 8)))
    many_zeros = torch.relu(base)                                    # ReLU zeros: the minimum is tied on about half the elements
    unique = base.abs() + 0.25
    unique.view(-1)[17] = 0.125                                      # a unique minimum
    tied_max = many_zeros.clone()
    tied_max.view(-1)[(int(tied_max.argmax()) + 1) % tied_max.numel()] = tied_max.max()      # the maximum on two elements
    return {"tied_min": many_zeros, "unique_min": unique, "tied_max": tied_max}, _f32(rng.standard_normal((23, 8))), \
        _f32(rng.standard_normal((23, 8)))


@pytest.mark.parametrize("case", ["tied_min", "unique_min", "tied_max"])
def test_ref_gain_and_its_backward_match_autograd(case):
    ps, x, g = _gain_cases()
    p = ps[case].double().requires_grad_(True)
    x = x.double().requires_grad_(True)
    n_min, n_max = int((p == p.min()).sum()), int((p == p.max()).sum())
    assert {"tied_min": n_min > 20 and n_max == 1, "unique_min": n_min == 1 and n_max == 1, "tied_max": n_min > 20 and n_max == 2}[case]
    out = (1 + (p - p.min()) / (p.max() - p.min())) * x
    out.backward(g.double())
    assert torch.allclose(ref_gain(p, x), out.detach(), rtol=0, atol=1e-14)
    dx, dp = ref_gain_bwd(g, x, p)
    assert torch.allclose(dx, x.grad, rtol=0, atol=1e-13)
    assert torch.allclose(dp, p.grad, rtol=0, atol=1e-12), (dp - p.grad).abs().max()


def test_ref_bn_backward_matches_autograd():
    inp = make_inputs(37, 12)
    z = inp.z.double().requires_grad_(True)
    gamma, beta = inp.gamma.double().requires_grad_(True), inp.D.double().requires_grad_(True)
    y = torch.relu(F.batch_norm(z, None, None, gamma, beta, True, MOMENTUM, EPS))
    g = inp.g.double()
    y.backward(g)
    zd = z.detach()
    mu, r = zd.mean(0), 1.0 / torch.sqrt(zd.var(0, unbiased=False) + EPS)      # the true statistics of z
    fwd = (gamma.detach() * r, beta.detach(), mu)
    mask = ref_pre(zd, *fwd) > 0
    assert 0 < int(mask.sum()) < mask.numel()
    s1, s2 = ref_col_sums(g * mask, zd)
    c = ref_bn_coef_bwd(s1, s2, 37, torch.stack([mu, r], 1), gamma)
    assert torch.allclose(ref_bn_bwd_apply(g, zd, c.A, c.E, c.D, c.S, mask), z.grad, rtol=0, atol=1e-10)
    assert torch.allclose(c.dgamma, gamma.grad, rtol=0, atol=1e-10) and torch.allclose(c.dbeta, beta.grad, rtol=0, atol=1e-12)
    # without a ReLU (BatchNorm `norm`): the same formulas with no mask
    z2 = inp.x.double().requires_grad_(True)
    F.batch_norm(z2, None, None, gamma, beta, True, MOMENTUM, EPS).backward(g)
    z2d = z2.detach()
    ms = torch.stack([z2d.mean(0), 1.0 / torch.sqrt(z2d.var(0, unbiased=False) + EPS)], 1)
    c2 = ref_bn_coef_bwd(*ref_col_sums(g, z2d), 37, ms, gamma)
    assert torch.allclose(ref_bn_bwd_apply(g, z2d, c2.A, c2.E, c2.D, c2.S), z2.grad, rtol=0, atol=1e-12)


def _sa_params(C, G, seed=0):
    rng = np.random.default_rng([C, G, seed])
    cp = C // (2 * G)
    prm = [_f32(rng.standard_normal(cp)) for _ in range(4)]                                  # cweight, cbias, sweight, sbias
    return prm + [_f32(1.0 + 0.3 * rng.standard_normal(cp)), _f32(rng.standard_normal(cp))]     # gn.weight, gn.bias


@pytest.mark.parametrize("C,G", [(4, 2), (24, 4), (16, 1)])
def test_ref_sa_cat_matches_the_oracle_composition(C, G):
    from oracle import vrnet_oracle as O
    B, H, W = 2, 3, 5
    rng = np.random.default_rng([C, G])
    x, r = _f32(2.0 + rng.standard_normal((B, H * W, C))).double(), _f32(rng.standard_normal((B, H * W, C))).double()
    prm = [t.double() for t in _sa_params(C, G)]
    names = ["m.cweight", "m.cbias", "m.sweight", "m.sbias"]
    P = {k: t.reshape(1, -1, 1, 1) for k, t in zip(names, prm)}
    P["m.gn.weight"], P["m.gn.bias"] = prm[4], prm[5]
    nchw = lambda t: t.reshape(B, H, W, -1).permute(0, 3, 1, 2)
    want = O.shuffle2(torch.cat([O.shuffle_attention(P, "m", nchw(x), G), nchw(r)], 1))
    got = ref_sa_cat(x, *ref_sa_coefs(x, prm, G), r)
    assert torch.allclose(nchw(got), want, rtol=0, atol=1e-12)


@pytest.mark.parametrize("variant", VARIANTS)
@pytest.mark.parametrize("shape", SHAPES, ids=SHAPE_IDS)
def test_inputs_keep_every_pre_activation_away_from_zero(shape, variant):
    rows, C = shape[:2]
    inp = make_inputs(rows, C, variant)
    pre = ref_pre(inp.z, inp.A, inp.D, inp.S)
    print(f"{rows} x {C} {variant}: {inp.nudged} elements nudged, min |pre| {pre.abs().min().item():.3e}")
    assert pre.abs().min().item() >= MARGIN
    assert inp.nudged <= 8 + inp.n // 1000                               # (|pre| < 1e-3 has a probability of about 6e-4)
    p = torch.relu(pre)
    if variant == "positive":
        assert (pre > 0).all() and int((p == p.min()).sum()) == 1        # no ReLU zero: the minimum is unique
    elif inp.n >= 100:
        assert int((p == 0).sum()) > 1                                   # ReLU zeros: the minimum is tied


# ----------------------------------------------------------------------------------------------- device helpers
def nan32(*shape):
    return torch.full(shape, float("nan"), dtype=torch.float32, device="cuda")


def nan64(*shape):
    return torch.full(shape, float("nan"), dtype=torch.float64, device="cuda")


def live_workgroups(n, chunks):
    """Workgroups of a `chunks`-wide launch that own at least one float4 (workgroup b starts at float4 256 b)."""
    return min(chunks, -(-(n // 4) // 256))


def plan(hip, inp, shape):
    nch, nfold = hip.fusion_chunks(inp.n, inp.C), hip.fusion_fold_chunks(inp.n, inp.C)
    assert (nch, nfold) == tuple(shape[2:]), (nch, nfold, shape)
    return nch, nfold


def to_dev(inp, *names):
    return [getattr(inp, k).cuda() for k in names]


# ----------------------------------------------------------------------------------------------- image chain
def run_image_chain(hip, inp, nch, nfold):
    """The launches of program.image_enhance (forward, then backward) with its arguments: n = rows C, the (min, max) and four-sum
    partials with the fold count, the column partials with the chunk count.  Every output and partial starts as NaN."""
    rows, C, n = inp.rows, inp.C, inp.n
    z, A, D, S, x, g, gamma, ms1, gamma2, beta2 = to_dev(inp, "z", "A", "D", "S", "x", "g", "gamma", "ms1", "gamma2", "beta2")
    d = NS(z=z, A=A, D=D, S=S, x=x, g=g, gamma=gamma, ms1=ms1, gamma2=gamma2)
    d.mmpart, d.p = nan32(nfold, 2), nan32(rows, C)
    hip.bn_relu_minmax(z, A, D, S, d.p, n, C, d.mmpart)
    d.p_raw = d.p.clone()
    if inp.variant == "tiedmax":       # the maximum of p on a second element (the partials hold the same maximum)
        top = torch.topk(d.p.view(-1), 2).indices
        d.p.view(-1)[top[1]] = d.p.view(-1)[top[0]]
    d.colpart_t, d.mm, d.t = nan64(nch, C, 2), nan32(2), nan32(rows, C)
    hip.enhance_stats(d.p, x, d.mmpart, nfold, d.mm, d.t, n, C, d.colpart_t)
    d.rmean, d.rvar, d.nbt = inp.rmean.cuda(), inp.rvar.cuda(), torch.full((), 5, dtype=torch.int64, device="cuda")
    d.A2f, d.D2f, d.S2f, d.ms2 = nan32(C), nan32(C), nan32(C), nan32(C, 2)
    hip.bn_coef_fwd_from_chunks(d.colpart_t, nch, rows, gamma2, beta2, EPS, MOMENTUM, d.rmean, d.rvar, d.nbt, C, d.A2f, d.D2f, d.S2f, d.ms2)
    d.y = nan32(rows, C)
    hip.affine(d.y, C, 1, rows, C, x1=d.t, ld1=C, A=d.A2f, D1=d.D2f, S1=d.S2f)
    # backward of `norm`: its coefficients as program.bn_bwd_coef gets them
    d.A2, d.E2, d.D2, d.S2, d.dg2, d.db2 = (nan32(C) for _ in range(6))
    hip.bn_stats_bwd(g, C, d.t, C, None, 0, d.ms2, gamma2, True, 1, rows, C, d.A2, d.E2, d.D2, d.S2, d.dg2, d.db2, 0)
    d.sums4, d.dt = nan64(nfold, 4), nan32(rows, C)
    hip.bn_bwd_enhance(g, d.t, d.A2, d.E2, d.D2, d.S2, x, d.p, d.mm, d.dt, n, C, d.sums4)
    d.bwd = []
    for acc in (0, 1):
        b = NS(acc=acc, dx=inp.dx0.cuda() if acc else nan32(rows, C), dp=nan32(rows, C), colpart=nan64(nch, C, 2))
        hip.enhance_bwd_stats(d.dt, x, d.p, d.mm, d.sums4, nfold, z, A, D, S, b.dx, b.dp, n, C, acc, b.colpart)
        b.A1, b.E1, b.D1, b.S1 = (nan32(C) for _ in range(4))
        b.dg, b.db = (torch.full((C,), 3.0, device="cuda") if acc else nan32(C) for _ in range(2))
        hip.bn_coef_bwd_from_chunks(b.colpart, nch, rows, ms1, gamma, True, C, b.A1, b.E1, b.D1, b.S1, b.dg, b.db, acc)
        b.dz = nan32(rows, C)
        hip.bn_apply_bwd_zmask(b.dp, C, z, C, (A, D, S), b.A1, b.E1, b.D1, b.S1, b.dz, C, 1, rows, C)
        d.bwd.append(b)
    torch.cuda.synchronize()
    return d


def check_partials_of_idle_workgroups(part, live, what, value=0.0):
    part = part.detach().cpu()
    assert not torch.isnan(part).any(), f"{what}: a partial entry was not written"
    if live < part.shape[0]:
        idle = part[live:].reshape(part.shape[0] - live, -1)
        assert (idle == torch.as_tensor(value, dtype=part.dtype)).all(), f"{what}: entries of idle workgroups"


def check_bn_bwd_coefs(b, s1, s2, rows, ms, gamma, acc, tol, what, floor=1e-6):
    c = ref_bn_coef_bwd(s1, s2, rows, ms, gamma)
    for k in "AEDS":
        close(getattr(b, k + "1"), getattr(c, k), tol, f"{what} {k}", floor)
    close(b.dg, c.dgamma + (3.0 if acc else 0.0), tol, what + " dgamma", floor)
    close(b.db, c.dbeta + (3.0 if acc else 0.0), tol, what + " dbeta", floor)


@pytest.mark.gpu
@pytest.mark.parametrize("variant", VARIANTS)
@pytest.mark.parametrize("shape", SHAPES, ids=SHAPE_IDS)
def test_image_chain_stage_by_stage(hip, shape, variant):
    rows, C = shape[:2]
    inp = make_inputs(rows, C, variant)
    mask = relu_mask(inp)                                   # (asserts the margin on the reference alone)
    nch, nfold = plan(hip, inp, shape)
    n = inp.n
    d = run_image_chain(hip, inp, nch, nfold)
    # -- bn_relu_minmax
    p_raw = d.p_raw.cpu()
    elem_close(p_raw, ref_bn_relu(inp.z, inp.A, inp.D, inp.S), "p")
    assert torch.equal(p_raw > 0, mask), "ReLU mask of p"
    live_f, live_c = live_workgroups(n, nfold), live_workgroups(n, nch)
    if (rows, C) == (7, 24):
        assert nch - live_c == 2
    if (rows, C) == (2, 480):
        assert nch - live_c == 14
    mmpart = d.mmpart.cpu()
    assert not torch.isnan(mmpart).any(), "mmpart: an entry was not written"
    assert same_bits(torch.stack([mmpart[:, 0].min(), mmpart[:, 1].max()]), torch.stack([p_raw.min(), p_raw.max()])), "mmpart folded"
    assert (mmpart[live_f:, 0] == math.inf).all() and (mmpart[live_f:, 1] == -math.inf).all(), "mmpart of idle workgroups"
    pu = nan32(rows, C)
    hip.affine(pu, C, 1, rows, C, x1=d.z, ld1=C, A=d.A, D1=d.D, S1=d.S, pre=1)
    elem_close(d.p_raw, pu, "p against affine pre=1")
    # -- enhance_stats
    p = d.p.cpu()
    mn, mx = p.min(), p.max()
    assert same_bits(d.mm, torch.stack([mn, mx])), "mm"
    n_min, n_max = int((p == mn).sum()), int((p == mx).sum())
    if variant == "positive":
        assert n_min == 1
    if variant == "tiedmax":
        assert n_max == 2
    elem_close(d.t, ref_gain(p, inp.x), "t")
    check_partials_of_idle_workgroups(d.colpart_t, live_c, "colpart of t")
    t = f64(d.t)
    colsum = d.colpart_t.sum(0).cpu()
    sums_close(colsum[:, 0], t, "column sum of t")
    sums_close(colsum[:, 1], t * t, "column sumsq of t")
    mmu, tu = nan32(2), nan32(rows, C)
    hip.minmax(d.p, n, mmu)
    assert same_bits(mmu, d.mm), "mm against minmax"
    hip.enhance_mul(d.p, d.x, d.mm, tu, n)
    elem_close(d.t, tu, "t against enhance_mul")
    mm3, t3 = nan32(2), nan32(rows, C)
    hip.enhance_fwd(d.p, d.x, mm3, t3, n)
    assert same_bits(mm3, d.mm), "mm against enhance_fwd"
    elem_close(d.t, t3, "t against enhance_fwd")
    elem_close(t3, ref_gain(p, inp.x), "enhance_fwd")
    # -- bn_coef_fwd_from_chunks (BatchNorm `norm`) and its apply
    c = ref_bn_coef_fwd(*ref_col_sums(t), rows, inp.gamma2, inp.beta2, EPS, MOMENTUM, inp.rmean, inp.rvar)
    for got, ref, nm in ((d.A2f, c.A, "A"), (d.D2f, c.D, "D"), (d.S2f, c.S, "S"), (d.ms2, c.mean_rstd, "mean_rstd"),
                         (d.rmean, c.rmean, "running_mean"), (d.rvar, c.rvar, "running_var")):
        close(got, ref, COEF_TOL, "norm forward " + nm)
    assert int(d.nbt.item()) == 6
    elem_close(d.y, ref_pre(t, d.A2f, d.D2f, d.S2f), "y")
    # -- coefficients of the backward of `norm` (bn_stats_bwd: 1e-5 with floor 1e-3, as test_batch_norm_relu_chain)
    b2 = NS(A1=d.A2, E1=d.E2, D1=d.D2, S1=d.S2, dg=d.dg2, db=d.db2)
    check_bn_bwd_coefs(b2, *ref_col_sums(inp.g, t), rows, d.ms2, inp.gamma2, 0, 1e-5, "norm backward", floor=1e-3)
    # -- bn_bwd_enhance
    elem_close(d.dt, ref_bn_bwd_apply(inp.g, t, d.A2, d.E2, d.D2, d.S2), "dt")
    check_partials_of_idle_workgroups(d.sums4, live_f, "sums4")
    dt = f64(d.dt)
    dn = (dt * f64(inp.x)).reshape(-1)
    p_mn = (p - mn).double().reshape(-1)                   # (p - mn) in fp32, as the kernel forms it
    s4 = d.sums4.sum(0).cpu()
    sums_close(s4[0], dn, "sum dn")
    sums_close(s4[1], dn * p_mn, "sum dn (p - mn)")
    assert s4[2].item() == n_min and s4[3].item() == n_max, ("tie counts", s4[2:].tolist(), n_min, n_max)
    # -- enhance_bwd_stats -> bn_coef_bwd_from_chunks -> bn_apply_bwd_zmask, dx written and accumulated
    dx_ref, dp_ref = ref_gain_bwd(dt, inp.x, p)
    for b in d.bwd:
        w = f"accumulate {b.acc}: "
        elem_close(b.dx, dx_ref + (f64(inp.dx0) if b.acc else 0.0), w + "dx")
        elem_close(b.dp, dp_ref, w + "dp")
        check_partials_of_idle_workgroups(b.colpart, live_c, w + "colpart of dp'")
        dpm = f64(b.dp) * mask
        colsum = b.colpart.sum(0).cpu()
        sums_close(colsum[:, 0], dpm, w + "column sum of dp'")
        sums_close(colsum[:, 1], dpm * f64(inp.z), w + "column sum of dp' z")
        dxu, dpu = inp.dx0.cuda() if b.acc else nan32(rows, C), nan32(rows, C)
        hip.enhance_bwd(d.dt, d.x, d.p, d.mm, dxu, dpu, n, accumulate_dx=b.acc)
        elem_close(b.dx, dxu, w + "dx against enhance_bwd")
        elem_close(b.dp, dpu, w + "dp against enhance_bwd")
        check_bn_bwd_coefs(b, *ref_col_sums(dpm, inp.z), rows, inp.ms1, inp.gamma, b.acc, COEF_TOL, w + "bn1 backward")
        u = NS(dg=torch.full((C,), 3.0, device="cuda") if b.acc else nan32(C), db=torch.full((C,), 3.0, device="cuda") if b.acc else nan32(C))
        u.A1, u.E1, u.D1, u.S1 = (nan32(C) for _ in range(4))
        hip.bn_stats_bwd_zmask(b.dp, C, d.z, C, (d.A, d.D, d.S), d.ms1, d.gamma, True, 1, rows, C, u.A1, u.E1, u.D1, u.S1, u.dg, u.db, b.acc)
        for k in ("A1", "E1", "D1", "S1", "dg", "db"):
            elem_close(getattr(b, k), getattr(u, k), w + k + " against bn_stats_bwd_zmask")
        elem_close(b.dz, ref_bn_bwd_apply(b.dp, inp.z, b.A1, b.E1, b.D1, b.S1, mask), w + "dz")


# ----------------------------------------------------------------------------------------------- radar chain
def run_radar_chain(hip, inp, nch):
    """The fused launches of program.radar_enhance behind the inverse projection's conv, forward then backward."""
    rows, C, n = inp.rows, inp.C, inp.n
    z, A, D, S, res, g, gamma, ms1, gamma2, beta2 = to_dev(inp, "z", "A", "D", "S", "res", "g", "gamma", "ms1", "gamma2", "beta2")
    d = NS(z=z, A=A, D=D, S=S, res=res)
    d.colpart_s, d.s = nan64(nch, C, 2), nan32(rows, C)
    hip.bn_relu_res_stats(z, A, D, S, res, d.s, n, C, d.colpart_s)
    d.rmean, d.rvar, d.nbt = inp.rmean.cuda(), inp.rvar.cuda(), torch.full((), 5, dtype=torch.int64, device="cuda")
    d.A2f, d.D2f, d.S2f, d.ms2 = nan32(C), nan32(C), nan32(C), nan32(C, 2)
    hip.bn_coef_fwd_from_chunks(d.colpart_s, nch, rows, gamma2, beta2, EPS, MOMENTUM, d.rmean, d.rvar, d.nbt, C, d.A2f, d.D2f, d.S2f, d.ms2)
    d.A2, d.E2, d.D2, d.S2, d.dg2, d.db2 = (nan32(C) for _ in range(6))
    hip.bn_stats_bwd(g, C, d.s, C, None, 0, d.ms2, gamma2, True, 1, rows, C, d.A2, d.E2, d.D2, d.S2, d.dg2, d.db2, 0)
    d.colpart, d.ds = nan64(nch, C, 2), nan32(rows, C)
    hip.bn_bwd_next_stats(g, d.s, d.A2, d.E2, d.D2, d.S2, z, (A, D, S), d.ds, n, C, d.colpart)
    d.bwd = []
    for acc in (0, 1):
        b = NS(acc=acc)
        b.A1, b.E1, b.D1, b.S1 = (nan32(C) for _ in range(4))
        b.dg, b.db = (torch.full((C,), 3.0, device="cuda") if acc else nan32(C) for _ in range(2))
        hip.bn_coef_bwd_from_chunks(d.colpart, nch, rows, ms1, gamma, True, C, b.A1, b.E1, b.D1, b.S1, b.dg, b.db, acc)
        d.bwd.append(b)
    b = d.bwd[0]
    d.dz = nan32(rows, C)
    hip.bn_apply_bwd_zmask(d.ds, C, z, C, (A, D, S), b.A1, b.E1, b.D1, b.S1, d.dz, C, 1, rows, C)
    torch.cuda.synchronize()
    return d


@pytest.mark.gpu
@pytest.mark.parametrize("variant", ["plain", "positive"])
@pytest.mark.parametrize("shape", SHAPES, ids=SHAPE_IDS)
def test_radar_chain_stage_by_stage(hip, shape, variant):
    rows, C = shape[:2]
    inp = make_inputs(rows, C, variant)
    mask = relu_mask(inp)
    nch, _ = plan(hip, inp, shape)
    live = live_workgroups(inp.n, nch)
    d = run_radar_chain(hip, inp, nch)
    # -- bn_relu_res_stats
    elem_close(d.s, ref_bn_relu(inp.z, inp.A, inp.D, inp.S, inp.res), "s")
    check_partials_of_idle_workgroups(d.colpart_s, live, "colpart of s")
    s = f64(d.s)
    colsum = d.colpart_s.sum(0).cpu()
    sums_close(colsum[:, 0], s, "column sum of s")
    sums_close(colsum[:, 1], s * s, "column sumsq of s")
    su = nan32(rows, C)
    hip.affine(su, C, 1, rows, C, x1=d.z, ld1=C, A=d.A, D1=d.D, S1=d.S, pre=1, x2=d.res, ld2=C)
    elem_close(d.s, su, "s against affine pre=1 + residual")
    # -- bn_coef_fwd_from_chunks
    c = ref_bn_coef_fwd(*ref_col_sums(s), rows, inp.gamma2, inp.beta2, EPS, MOMENTUM, inp.rmean, inp.rvar)
    for got, ref, nm in ((d.A2f, c.A, "A"), (d.D2f, c.D, "D"), (d.S2f, c.S, "S"), (d.ms2, c.mean_rstd, "mean_rstd"),
                         (d.rmean, c.rmean, "running_mean"), (d.rvar, c.rvar, "running_var")):
        close(got, ref, COEF_TOL, "norm forward " + nm)
    assert int(d.nbt.item()) == 6
    b2 = NS(A1=d.A2, E1=d.E2, D1=d.D2, S1=d.S2, dg=d.dg2, db=d.db2)
    check_bn_bwd_coefs(b2, *ref_col_sums(inp.g, s), rows, d.ms2, inp.gamma2, 0, 1e-5, "norm backward", floor=1e-3)
    # -- bn_bwd_next_stats
    elem_close(d.ds, ref_bn_bwd_apply(inp.g, s, d.A2, d.E2, d.D2, d.S2), "ds")
    check_partials_of_idle_workgroups(d.colpart, live, "colpart of ds'")
    dsm = f64(d.ds) * mask
    colsum = d.colpart.sum(0).cpu()
    sums_close(colsum[:, 0], dsm, "column sum of ds'")
    sums_close(colsum[:, 1], dsm * f64(inp.z), "column sum of ds' z")
    # -- bn_coef_bwd_from_chunks, bn_apply_bwd_zmask
    for b in d.bwd:
        check_bn_bwd_coefs(b, *ref_col_sums(dsm, inp.z), rows, inp.ms1, inp.gamma, b.acc, COEF_TOL, f"accumulate {b.acc}: bn1 backward")
    b = d.bwd[0]
    elem_close(d.dz, ref_bn_bwd_apply(d.ds, inp.z, b.A1, b.E1, b.D1, b.S1, mask), "dz")


# ----------------------------------------------------------------------------------------------- repeatability
def _tensors(d):
    out = {}
    for k, v in vars(d).items():
        if torch.is_tensor(v):
            out[k] = v
        elif isinstance(v, list):
            for i, b in enumerate(v):
                out.update({f"{k}{i}.{kk}": vv for kk, vv in vars(b).items() if torch.is_tensor(vv)})
    return out


@pytest.mark.gpu
@pytest.mark.parametrize("shape", SHAPES, ids=SHAPE_IDS)
def test_fused_kernels_repeat_bitwise(hip, shape):
    """fusion.hip promises fixed summation orders: a second run leaves the same bits in every output and every partial."""
    inp = make_inputs(*shape[:2])
    nch, nfold = plan(hip, inp, shape)
    for run in (lambda: run_image_chain(hip, inp, nch, nfold), lambda: run_radar_chain(hip, inp, nch)):
        a, b = _tensors(run()), _tensors(run())
        assert a.keys() == b.keys() and len(a) > 15
        for k in a:
            assert same_bits(a[k], b[k]), k


# ----------------------------------------------------------------------------------------------- enhance_fwd alone
@pytest.mark.gpu
@pytest.mark.parametrize("n", [2 * 5 * 7 * 3, 7 * 24, 513 * 12 + 2, 2 * 168 * 160 * 3, 53760 * 40])
def test_enhance_fwd_vector_and_scalar_paths(hip, n):
    """The unfused gain of the 3-channel input level: float4 path (n % 4 == 0) and scalar path, one and many workgroups."""
    rng = np.random.default_rng(n)
    p, x = torch.relu(_f32(rng.standard_normal(n))), _f32(rng.standard_normal(n))
    pg, xg = p.cuda(), x.cuda()
    mm, out = nan32(2), torch.full((n + 8,), -7.0, device="cuda")
    hip.enhance_fwd(pg, xg, mm, out, n)
    assert same_bits(mm, torch.stack([p.min(), p.max()])), "mm as left by enhance_fwd"
    elem_close(out[:n], ref_gain(p, x), "enhance_fwd")
    assert (out[n:] == -7.0).all(), "enhance_fwd wrote past the end"
    mm2, out2 = nan32(2), nan32(n)
    hip.minmax(pg, n, mm2)
    hip.enhance_mul(pg, xg, mm2, out2, n)
    assert same_bits(mm, mm2)
    elem_close(out[:n], out2, "enhance_fwd against minmax + enhance_mul")


# ----------------------------------------------------------------------------------------------- sa_cat_sums
@pytest.mark.gpu
@pytest.mark.parametrize("HW", [1, 37, 1024])
@pytest.mark.parametrize("C,G", [(4, 2), (24, 4), (80, 4), (512, 4)])      # 512: 256 threads per row, one row per pass
def test_sa_cat_sums(hip, C, G, HW):
    B = 2
    rng = np.random.default_rng([C, HW])
    x, r = _f32(2.0 + rng.standard_normal((B, HW, C))), _f32(rng.standard_normal((B, HW, C)))
    P, Q, Mn = (t.float() for t in ref_sa_coefs(x, _sa_params(C, G), G))
    ldx, ldr, ldc = C + 12, C + 2, 2 * C
    xw, rw = nan32(B * HW, ldx), nan32(B * HW, ldr)              # x: a column block of a wider buffer; r: an even row stride > C
    xv, rv = xw[:, 5:5 + C], rw[:, :C]
    xv.copy_(x.reshape(-1, C))
    rv.copy_(r.reshape(-1, C))
    cat = nan32(B, HW, ldc)
    mom = hip.sa_cat_sums(xv, ldx, P.cuda(), Q.cuda(), Mn.cuda(), rv, ldr, cat, ldc, B, HW, C)
    torch.cuda.synchronize()
    elem_close(cat, ref_sa_cat(x, P, Q, Mn, r), "cat")
    assert same_bits(cat[..., 1::2], r), "the radar lanes of cat are copies"
    assert mom.shape == (B, 2 * C, 2) and (mom[..., 1] == 0).all()
    for b in range(B):
        sums_close(mom[b, :, 0], cat[b], f"channel sums of cat, sample {b}")
    cat2 = nan32(B, HW, ldc)
    mom2 = hip.sa_cat_sums(xv, ldx, P.cuda(), Q.cuda(), Mn.cuda(), rv, ldr, cat2, ldc, B, HW, C)
    assert same_bits(cat, cat2) and same_bits(mom, mom2), "a second run leaves other bits"


# ----------------------------------------------------------------------------------------------- rejected calls
def _fusion_calls(hip, first, o, n, C):
    """The six fused wrappers with `first` as their first tensor argument and (n, C) as given; o: valid buffers."""
    fwd = (o.c[4], o.c[5], o.c[6])
    return {
        "bn_relu_minmax": lambda: hip.bn_relu_minmax(first, o.c[0], o.c[1], o.c[2], o.out[0], n, C, o.mmpart),
        "bn_relu_res_stats": lambda: hip.bn_relu_res_stats(first, o.c[0], o.c[1], o.c[2], o.t[1], o.out[0], n, C, o.colpart),
        "enhance_stats": lambda: hip.enhance_stats(first, o.t[1], o.mmpart, 1, o.mm, o.out[0], n, C, o.colpart),
        "bn_bwd_enhance": lambda: hip.bn_bwd_enhance(first, o.t[1], o.c[0], o.c[1], o.c[2], o.c[3], o.t[2], o.t[3], o.mm, o.out[0], n, C,
                                                     o.sums4),
        "enhance_bwd_stats": lambda: hip.enhance_bwd_stats(first, o.t[1], o.t[2], o.mm, o.sums4, 1, o.t[3], *fwd, o.out[0], o.out[1], n, C,
                                                           0, o.colpart),
        "bn_bwd_next_stats": lambda: hip.bn_bwd_next_stats(first, o.t[1], o.c[0], o.c[1], o.c[2], o.c[3], o.t[3], fwd, o.out[0], n, C,
                                                           o.colpart),
    }


@pytest.mark.gpu
def test_fusion_wrappers_reject_unsupported_shapes_and_unaligned_tensors(hip):
    """A rejected call launches nothing: the outputs keep their fill."""
    bad = [(42, 6), (2 * 1028, 1028), (100, 24)]          # C % 4 != 0, C > 1024, n % C != 0
    for n, C in bad:
        assert hip.fusion_chunks(n, C) == 0 and hip.fusion_fold_chunks(n, C) == 0, (n, C)
    assert hip.fusion_chunks(168, 24) == 3
    size = 4096
    o = NS(t=[torch.ones(size, device="cuda") for _ in range(4)], c=[torch.ones(1028, device="cuda") for _ in range(7)],
           out=[torch.full((size,), -7.0, device="cuda") for _ in range(2)], mm=torch.tensor([0.0, 1.0], device="cuda"),
           mmpart=torch.full((64, 2), -7.0, device="cuda"), colpart=torch.full((64, 1028, 2), -7.0, dtype=torch.float64, device="cuda"),
           sums4=torch.full((64, 4), -7.0, dtype=torch.float64, device="cuda"))
    shifted = torch.ones(size + 1, device="cuda")[1:]      # offset by one float: not 16-byte aligned
    assert shifted.data_ptr() % 16 == 4
    for n, C in bad:
        for name, call in _fusion_calls(hip, o.t[0], o, n, C).items():
            with pytest.raises(RuntimeError):
                call()
    for name, call in _fusion_calls(hip, shifted, o, 168, 24).items():
        with pytest.raises(RuntimeError):
            call()
    torch.cuda.synchronize()
    for t in o.out + [o.mmpart, o.colpart, o.sums4]:
        assert (t == -7.0).all(), "a rejected call wrote something"
    for name, call in _fusion_calls(hip, o.t[0], o, 168, 24).items():      # ... and the same calls are accepted with valid arguments
        call()
    torch.cuda.synchronize()


@pytest.mark.gpu
def test_sa_cat_sums_rejects_unsupported_shapes_and_layouts(hip):
    B, HW = 1, 2
    big = torch.ones(B * HW, 1100, device="cuda")
    coef = torch.zeros(B, 600, device="cuda")
    cat = torch.full((B * HW, 1100), -7.0, device="cuda")

    def call(C, r, ldr):
        return hip.sa_cat_sums(big, 1100, coef, coef, coef, r, ldr, cat, 1100, B, HW, C)

    for C in (6, 516):
        with pytest.raises(RuntimeError):
            call(C, big, 1100)
    with pytest.raises(RuntimeError):
        call(24, big, 1099)                                 # odd row stride of r
    shifted = torch.ones(B * HW * 1100 + 1, device="cuda")[1:]
    assert shifted.data_ptr() % 8 == 4
    with pytest.raises(RuntimeError):
        call(24, shifted, 1100)                             # r offset by one float: not 8-byte aligned
    torch.cuda.synchronize()
    assert (cat == -7.0).all(), "a rejected call wrote something"
    call(24, big, 1100)
    torch.cuda.synchronize()
    assert not (cat[:, :48] == -7.0).any()


# ----------------------------------------------------------------------------------------------- small companions
@pytest.mark.gpu
@pytest.mark.parametrize("entries", [1, 32, 33, 70])       # the by-value table of one launch holds 32
def test_cluster_ab_reduce_multi(hip, entries):
    """out = (accumulate ? out : 0) + float(sum): the fp64 sum in any order (blocks 2^-52 sum |terms|), its rounding to fp32 and the
    fp32 addition (2^-24 each of |sum| + |out|)."""
    rng = np.random.default_rng(entries)
    sizes = [1, 255, 256, 257, 4097]
    blocks = [sizes[(i + entries) % 5] for i in range(entries)]
    acc = [(i * 7 + entries) % 3 != 0 for i in range(entries)]
    parts = [_f32(rng.standard_normal((b, 2))) for b in blocks]
    parts_g = [t.cuda() for t in parts]
    fill = _f32(rng.standard_normal((2, entries)))
    grads = torch.full((2, entries + 1), -7.0, device="cuda")       # (one guard element behind each row)
    grads[:, :entries] = fill.cuda()
    hip.cluster_ab_reduce_multi([(parts_g[i], blocks[i], grads[0, i:i + 1], grads[1, i:i + 1], acc[i]) for i in range(entries)])
    torch.cuda.synchronize()
    got = grads.cpu().double()
    assert (got[:, entries] == -7.0).all()
    for i in range(entries):
        s, sabs = parts[i].double().sum(0), parts[i].double().abs().sum(0)
        old = fill[:, i].double() if acc[i] else torch.zeros(2, dtype=torch.float64)
        bound = 2.0 ** -23 * (s.abs() + old.abs()) + blocks[i] * 2.0 ** -52 * sabs
        assert ((got[:, i] - (old + s)).abs() <= bound).all(), (i, blocks[i], acc[i], got[:, i], old + s)


@pytest.mark.gpu
def test_mt_copy(hip):
    from asy_vrnet_amd.optim import CHUNK
    rng = np.random.default_rng(9)
    sizes = [1, 255, 256, 257, CHUNK + 1]
    src = [_f32(rng.standard_normal(s)).cuda() for s in sizes]
    guard = 3
    buf = torch.full((sum(sizes) + guard * len(sizes),), -7.0, device="cuda")
    dst, o = [], 0
    for s in sizes:
        dst.append(buf[o:o + s])
        o += s + guard
    ct, ci = [], []                                    # the chunk table as optim.py builds it
    for i, s in enumerate(sizes):
        k = (s + CHUNK - 1) // CHUNK
        ct += [i] * k
        ci += list(range(k))
    assert len(ct) == 6
    addrs = torch.tensor([t.data_ptr() for t in dst] + [t.data_ptr() for t in src], dtype=torch.int64, device="cuda")
    hip.mt_copy(addrs, torch.tensor(sizes, dtype=torch.int64, device="cuda"), torch.tensor(ct, dtype=torch.int32, device="cuda"),
                torch.tensor(ci, dtype=torch.int32, device="cuda"), len(sizes), len(ct), CHUNK)
    torch.cuda.synchronize()
    o = 0
    for s, a, b in zip(sizes, dst, src):
        assert same_bits(a, b), s
        assert (buf[o + s:o + s + guard] == -7.0).all(), f"guard behind the {s}-element tensor"
        o += s + guard
