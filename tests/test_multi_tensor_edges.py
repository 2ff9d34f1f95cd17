"""The multi-tensor update kernels (optim.hip: mt_sgd, mt_adam, mt_ema, mt_copy) called directly, on tables built by hand.

tests/test_optim.py reaches them through optim.SGD / Adam / ModelEMA only (CHUNK = 4096, first_step = 0, nesterov, momentum > 0,
a weight-decay vector, the chunks in tensor order) and tests/test_train_graph.py compares the `_dev` forms with the scalar forms,
one kernel body with itself.  Here: chunk_elems 256 and 4096; tensor sizes around a chunk's edges; every tensor of every role a
slice at float offset 1 of its own buffer with PAT in front and behind and finite floats behind that (a chunk that runs past
sizes[t] shows there: Table); the chunk
list shuffled, with one entry (tensor 0, chunk 5) that lies past its tensor; first_step, momentum 0, plain momentum, wd = NULL,
n_chunks = 0 and the refusals.

Reference and bound of the arithmetic: the update formulas restated in float64 on the same fp32 inputs (scalars rounded to fp32
first), in the operation order of the comments in optim.hip.  The kernels round to fp32 and the compiler may fuse multiply-adds,
so the measure is a distance: for the parameters max |a - b| / max |b| of a tensor, for the state tensors max |a - b| /
max(1, |b|) (close_stats of tests/test_optim.py), the largest over the tensors of the table.  Per state the project's fp32
oracle (oracle/optim_oracle.py on the CPU) is measured against the float64 restatement (d32); the kernel is allowed
max(4 d32, 2^-23): four times the oracle's own error for another legitimate rounding order, floored at one fp32 ulp of the
scale (tests/test_loss_edges.py: bounds, tests/test_spatial_edges.py: bound_of).  first_step = 1 and momentum = 0 take the
float64 restatement as reference and the bound of the neighbouring state (same weight decay; momentum 0.937, first_step 0).  The
state inputs are O(1) so that max(1, |b|) is about |b|.  test_oracle_bounds_are_finite_and_tight is the CPU half.

Measured on an MI355X (kernel distances over all states, weight-decay modes and both chunk sizes, beside the oracle's d32):
  mt_sgd   parameters  4.1e-8 .. 5.3e-8 (d32 4.1e-8 .. 4.8e-8, bounds 1.7e-7 .. 1.9e-7)
           buffer      5.7e-8 .. 1.4e-7 (d32 1.2e-7 .. 2.0e-7, bounds 4.8e-7 .. 7.9e-7); first_step = 1 with wd = NULL: 0 (buf = g)
  mt_adam  parameters  4.2e-8 .. 5.7e-8 (d32 the same to two digits, bounds 1.7e-7 .. 2.3e-7)
           exp_avg     6.3e-8 .. 7.4e-8, exp_avg_sq 5.7e-8 .. 5.9e-8 (d32 1.0e-7 .. 1.1e-7, bounds 4.0e-7 .. 4.5e-7)
  mt_ema   d = 0, 1: 0; d = 0.5: 6.0e-8 (d32 6.0e-8, bound 2.4e-7); d = 0.9999: 5.9e-8 (d32 1.1e-7, bound 4.5e-7)
No kernel distance exceeds 0.33 of its bound."""
import functools
import random
import types

import numpy as np
import pytest
import torch

from oracle import optim_oracle as OO
from tests.test_hip_ops import rnd
from tests.test_strided_rows import NAN, PAT, hip, refused      # noqa: F401  (hip: the fixture)

gpu = pytest.mark.gpu
NS = types.SimpleNamespace
ULP = 2.0 ** -23
GUARD = 4          # floats of PAT behind every tensor; one in front
SENTINEL = 4       # finite floats behind those
CES = (256, 4096)


def f32(x):
    return float(np.float32(x))


LR, MU, WD = f32(0.05), f32(0.937), f32(5e-4)
B1, B2, EPS = f32(0.9), f32(0.999), f32(1e-8)
WDS = (0.0, WD, WD, 0.0, WD, 0.0, 0.0, WD)          # the per-tensor weight decay of the "mixed" runs
SGD_STATES = [(MU, 1, 0), (MU, 0, 0), (MU, 1, 1), (0.0, 0, 0)]          # (momentum, nesterov, first_step); first: the product's
ADAM_STEPS = [1, 2, 1000]
EMA_DECAYS = [0.0, 0.5, f32(0.9999), 1.0]


def sizes_of(ce):
    return (1, 255, 256, 257, ce - 1, ce, ce + 1, 3 * ce + 3)


# ------------------------------------------------------------------------------------------------ inputs and references
@functools.lru_cache(maxsize=None)
def inputs(ce):
    """fp32 CPU tensors per role, one per tensor of the table: p, g, buf / m (O(1), signed), v (in [0.5, 3.5]), e, mod."""
    sz = sizes_of(ce)
    role = lambda k, **kw: [rnd(n, seed=100 * k + i, **kw) for i, n in enumerate(sz)]
    return NS(p=role(1), g=role(2), buf=role(3), m=role(4), v=[3 * t + 0.5 for t in role(5, kind="uniform")], e=role(6),
              mod=role(7))


def wd_of(mode, i):
    return WDS[i] if mode == "mixed" else 0.0


def sgd64(p, g, buf, lr, mu, wd, nesterov, first):
    """optim.hip: d = g + wd p; buf = first ? d : mu buf + d; d = nesterov ? d + mu buf : buf; p -= lr d -> (p, buf): on the first
    step buf = d, with momentum 0 it is not part of the update."""
    p, g, buf = p.double(), g.double(), buf.double()
    d = g + wd * p if wd != 0 else g
    if mu != 0:
        buf = d if first else mu * buf + d
        d = d + mu * buf if nesterov else buf
    return p - lr * d, buf


def adam64(p, g, m, v, step, lr, b1, b2, eps, wd):
    """optim.hip: g' = g + wd p; m = m + (g' - m)(1 - b1); v = b2 v + (1 - b2) g' g'; p -= (lr / bc1) (m / (sqrt(v) / sqrt(bc2) +
    eps)), bc = 1 - beta^step."""
    p, g, m, v = p.double(), g.double(), m.double(), v.double()
    if wd != 0:
        g = g + wd * p
    m = m + (g - m) * (1.0 - b1)
    v = b2 * v + (1.0 - b2) * g * g
    bc1, bc2 = 1.0 - b1 ** step, 1.0 - b2 ** step
    return p - (lr / bc1) * (m / (v.sqrt() / np.sqrt(bc2) + eps)), m, v


def ema64(e, mod, d):
    """optim.hip: e = e d + (1 - d) model."""
    return e.double() * d + (1.0 - d) * mod.double()


def rel(a, b):
    """Parameters: max |a - b| / max |b|."""
    a, b = a.detach().double().cpu(), b.double()
    return ((a - b).abs().max() / max(b.abs().max().item(), 1e-30)).item()


def scaled(a, b):
    """State tensors: max |a - b| / max(1, |b|)."""
    a, b = a.detach().double().cpu(), b.double()
    return ((a - b).abs() / b.abs().clamp(min=1.0)).max().item()


def bound_of(d32):
    return max(4 * d32, ULP)


def worst(metric, got, ref):
    return max(metric(a, b) for a, b in zip(got, ref))


@functools.lru_cache(maxsize=None)
def sgd_ref(ce, mode, mu, nesterov, first):
    """The float64 results and, where the oracle has the state (first_step = 0, momentum > 0), its distance from them."""
    D = inputs(ce)
    r64 = [sgd64(D.p[i], D.g[i], D.buf[i], LR, mu, wd_of(mode, i), nesterov, first) for i in range(len(D.p))]
    R = NS(p=[r[0] for r in r64], buf=[r[1] for r in r64])
    if first or mu == 0:
        N = sgd_ref(ce, mode, MU, nesterov, 0)          # the neighbouring state's bound
        R.d32_p, R.d32_s = N.d32_p, N.d32_s
    else:
        p32, b32 = [t.clone() for t in D.p], [t.clone() for t in D.buf]
        for i in range(len(p32)):
            OO.sgd_step(p32[i], D.g[i], b32[i], LR, mu, wd_of(mode, i), bool(nesterov))
        R.d32_p, R.d32_s = worst(rel, p32, R.p), worst(scaled, b32, R.buf)
    R.bound_p, R.bound_s = bound_of(R.d32_p), bound_of(R.d32_s)
    return R


@functools.lru_cache(maxsize=None)
def adam_ref(ce, mode, step):
    D = inputs(ce)
    n = len(D.p)
    r64 = [adam64(D.p[i], D.g[i], D.m[i], D.v[i], step, LR, B1, B2, EPS, wd_of(mode, i)) for i in range(n)]
    R = NS(p=[r[0] for r in r64], m=[r[1] for r in r64], v=[r[2] for r in r64])
    p32, m32, v32 = ([t.clone() for t in role] for role in (D.p, D.m, D.v))
    for i in range(n):
        OO.adam_step(p32[i], D.g[i], m32[i], v32[i], step, LR, B1, B2, EPS, wd_of(mode, i))
    R.d32_p, R.d32_s = worst(rel, p32, R.p), max(worst(scaled, m32, R.m), worst(scaled, v32, R.v))
    R.bound_p, R.bound_s = bound_of(R.d32_p), bound_of(R.d32_s)
    return R


@functools.lru_cache(maxsize=None)
def ema_ref(ce, d):
    D = inputs(ce)
    R = NS(e=[ema64(D.e[i], D.mod[i], d) for i in range(len(D.e))])
    e32 = {str(i): t.clone() for i, t in enumerate(D.e)}
    OO.ema_update(e32, {str(i): t for i, t in enumerate(D.mod)}, d)
    R.d32_s = worst(scaled, list(e32.values()), R.e)
    R.bound_s = bound_of(R.d32_s)
    return R


# ------------------------------------------------------------------------------------------------ the CPU half
def test_oracle_bounds_are_finite_and_tight():
    """The fp32 oracle against the float64 restatement for every state below: each formula is a handful of fp32 roundings of
    O(1) values, so d32 is a few 2^-24 -- a bound past 64 ulp would mean the two restate different formulas, a d32 of exactly 0
    on a rounding formula that the oracle was compared with itself."""
    for ce in CES:
        for mode in ("none", "mixed"):
            for mu, nesterov, first in SGD_STATES:
                R = sgd_ref(ce, mode, mu, nesterov, first)
                print(f"sgd ce {ce} wd {mode} mu {mu:.3f} nesterov {nesterov} first {first}: d32 p {R.d32_p:.2e} buf {R.d32_s:.2e} "
                      f"bounds {R.bound_p:.2e} {R.bound_s:.2e}")
                assert 0 < R.d32_p and ULP <= R.bound_p <= 64 * ULP and 0 < R.d32_s and ULP <= R.bound_s <= 64 * ULP
            for step in ADAM_STEPS:
                R = adam_ref(ce, mode, step)
                print(f"adam ce {ce} wd {mode} step {step}: d32 p {R.d32_p:.2e} m, v {R.d32_s:.2e} bounds {R.bound_p:.2e} "
                      f"{R.bound_s:.2e}")
                assert 0 < R.d32_p and ULP <= R.bound_p <= 64 * ULP and 0 < R.d32_s and ULP <= R.bound_s <= 64 * ULP
        for d in EMA_DECAYS:
            R = ema_ref(ce, d)
            print(f"ema ce {ce} d {d}: d32 {R.d32_s:.2e} bound {R.bound_s:.2e}")
            assert (R.d32_s == 0) == (d in (0.0, 1.0)) and ULP <= R.bound_s <= 64 * ULP          # d = 0, 1: exact copies


# ------------------------------------------------------------------------------------------------ tables on the device
class Table:
    """K roles x n tensors: each tensor a slice [1, 1 + size) of its own buffer of size + 1 + GUARD + SENTINEL floats: PAT in
    front, GUARD floats of PAT behind, then SENTINEL finite floats (1000 + the role's index).  A chunk that runs past sizes[t]
    updates what lies behind the tensor with what lies behind the other roles' tensors: PAT is a NaN, and a NaN that meets
    NaNs may come out with PAT's own bits; the finite floats change for certain (the last chunk of the tensors of 1, 257,
    ce + 1 and 3 ce + 3 elements would run far past them).  A role is a list of CPU tensors, or a float / the int PAT: that
    fill.  The chunk list is shuffled (fixed seed) and holds one entry (tensor 0, chunk 5) that lies wholly past its tensor."""

    def __init__(self, ce, roles):
        self.ce, self.sz = ce, sizes_of(ce)
        self.n = len(self.sz)
        self.bufs, self.views = [], []
        for r, role in enumerate(roles):
            bs = [torch.empty(s + 1 + GUARD + SENTINEL, device="cuda") for s in self.sz]
            vs = [b[1:1 + s] for b, s in zip(bs, self.sz)]
            for i, (b, v) in enumerate(zip(bs, vs)):
                b.view(torch.int32).fill_(PAT)
                b[-SENTINEL:] = 1000.0 + r
                if isinstance(role, list):
                    v.copy_(role[i])
                elif not isinstance(role, int):
                    v.fill_(role)
            self.bufs.append(bs)
            self.views.append(vs)
        chunks = [(t, c) for t, s in enumerate(self.sz) for c in range((s + ce - 1) // ce)] + [(0, 5)]
        random.Random(7).shuffle(chunks)
        assert chunks != sorted(chunks)
        dev = lambda x, dt: torch.tensor(x, dtype=dt, device="cuda")
        self.addrs = dev([[v.data_ptr() for v in vs] for vs in self.views], torch.int64)
        self.sizes = dev(self.sz, torch.int64)
        self.ct, self.ci = dev([c[0] for c in chunks], torch.int32), dev([c[1] for c in chunks], torch.int32)
        self.n_chunks = len(chunks)

    def args(self, n=None, n_chunks=None, ce=None):
        return (self.addrs, self.sizes, self.ct, self.ci), (self.n if n is None else n,
                                                            self.n_chunks if n_chunks is None else n_chunks,
                                                            self.ce if ce is None else ce)

    def role(self, r):
        return [v.cpu() for v in self.views[r]]

    def all_buffers(self):
        return [b for bs in self.bufs for b in bs]

    def guards_intact(self, what):
        torch.cuda.synchronize()
        for r, bs in enumerate(self.bufs):
            for i, (b, s) in enumerate(zip(bs, self.sz)):
                raw = b.view(torch.int32)
                kept = int(raw[0]) == PAT and bool((raw[1 + s:1 + s + GUARD] == PAT).all()) and bool((b[-SENTINEL:] == 1000.0 + r).all())
                assert kept, f"{what}: role {r}, tensor {i} (size {s}): the floats around it changed"


def wd_tensor(mode):
    return None if mode == "none" else torch.tensor(WDS, device="cuda")


def bit_equal(a, b):
    return torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


def within(what, seen, bound, d32):
    print(f"  {what}: d32 {d32:.2e} bound {bound:.2e} kernel {seen:.2e}")
    assert seen <= bound, f"{what}: distance {seen:.3e}, bound {bound:.3e} (d32 {d32:.3e})"


# ------------------------------------------------------------------------------------------------ SGD
@gpu
@pytest.mark.parametrize("mu,nesterov,first", SGD_STATES, ids=str)
@pytest.mark.parametrize("ce", CES)
def test_mt_sgd(hip, ce, mu, nesterov, first):
    D = inputs(ce)
    plain = None
    for mode in ("none", "mixed"):
        R = sgd_ref(ce, mode, mu, nesterov, first)
        what = f"mt_sgd ce {ce} mu {mu:.3f} nesterov {nesterov} first {first} wd {mode}"
        T = Table(ce, [D.p, D.g, NAN if first else PAT if mu == 0 else D.buf])
        tabs, dims = T.args()
        hip.mt_sgd(*tabs, wd_tensor(mode), *dims, LR, mu, nesterov, first)
        T.guards_intact(what)
        p, g, buf = T.role(0), T.role(1), T.role(2)
        assert all(bit_equal(a, b) for a, b in zip(g, D.g)), what + ": the gradients changed"
        assert all(bool(torch.isfinite(t).all()) for t in p), what + ": parameters not finite"
        within(what + " p", worst(rel, p, R.p), R.bound_p, R.d32_p)
        if mu == 0:
            assert all(bool((v.view(torch.int32) == PAT).all()) for v in T.views[2]), what + ": buf written"
        else:
            within(what + " buf", worst(scaled, buf, R.buf), R.bound_s, R.d32_s)
        for i in range(T.n):
            if first and wd_of(mode, i) == 0:
                assert bit_equal(buf[i], D.g[i]), what + f": buf != d on the first step, tensor {i}"
            if mode == "mixed" and WDS[i] == 0:          # wd[t] == 0 is the wd = NULL arithmetic
                assert bit_equal(p[i], plain[0][i]) and bit_equal(buf[i], plain[1][i]), what + f": tensor {i} differs from wd NULL"
        if mode == "none":
            plain = (p, buf)


# ------------------------------------------------------------------------------------------------ Adam
@gpu
@pytest.mark.parametrize("step", ADAM_STEPS)
@pytest.mark.parametrize("ce", CES)
def test_mt_adam(hip, ce, step):
    D = inputs(ce)
    plain = None
    for mode in ("none", "mixed"):
        R = adam_ref(ce, mode, step)
        what = f"mt_adam ce {ce} step {step} wd {mode}"
        T = Table(ce, [D.p, D.g, D.m, D.v])
        tabs, dims = T.args()
        hip.mt_adam(*tabs, wd_tensor(mode), *dims, LR, B1, B2, EPS, step)
        T.guards_intact(what)
        p, g, m, v = (T.role(r) for r in range(4))
        assert all(bit_equal(a, b) for a, b in zip(g, D.g)), what + ": the gradients changed"
        within(what + " p", worst(rel, p, R.p), R.bound_p, R.d32_p)
        within(what + " exp_avg", worst(scaled, m, R.m), R.bound_s, R.d32_s)
        within(what + " exp_avg_sq", worst(scaled, v, R.v), R.bound_s, R.d32_s)
        if mode == "none":
            plain = (p, m, v)
        else:
            for i in range(T.n):
                if WDS[i] == 0:
                    same = all(bit_equal(a[i], b[i]) for a, b in zip((p, m, v), plain))
                    assert same, what + f": tensor {i} differs from wd = NULL"


# ------------------------------------------------------------------------------------------------ EMA, copy
@gpu
@pytest.mark.parametrize("d", EMA_DECAYS)
@pytest.mark.parametrize("ce", CES)
def test_mt_ema(hip, ce, d):
    D = inputs(ce)
    R = ema_ref(ce, d)
    what = f"mt_ema ce {ce} d {d}"
    T = Table(ce, [D.e, D.mod])
    tabs, dims = T.args()
    hip.mt_ema(*tabs, *dims, d)
    T.guards_intact(what)
    e, mod = T.role(0), T.role(1)
    assert all(bit_equal(a, b) for a, b in zip(mod, D.mod)), what + ": the model changed"
    within(what, worst(scaled, e, R.e), R.bound_s, R.d32_s)
    if d == 0.0:
        assert all(bit_equal(a, b) for a, b in zip(e, D.mod)), what + ": e != model"
    if d == 1.0:
        assert all(bit_equal(a, b) for a, b in zip(e, D.e)), what + ": e changed"


@gpu
@pytest.mark.parametrize("ce", CES)
def test_mt_copy(hip, ce):
    D = inputs(ce)
    T = Table(ce, [PAT, D.p])
    tabs, dims = T.args()
    hip.mt_copy(*tabs, *dims)
    T.guards_intact(f"mt_copy ce {ce}")
    assert all(bit_equal(a, b) for a, b in zip(T.role(0), D.p)) and all(bit_equal(a, b) for a, b in zip(T.role(1), D.p))


# ------------------------------------------------------------------------------------------------ nothing to do, refusals
def calls(hip, T, **kw):
    """(entry point, call) of the four kernels on the table T (four roles: enough for Adam), dimensions overridden by kw."""
    tabs, dims = T.args(**kw)
    wd = wd_tensor("mixed")
    return [("mt_sgd", lambda: hip.mt_sgd(*tabs, wd, *dims, LR, MU, 1, 0)),
            ("mt_adam", lambda: hip.mt_adam(*tabs, wd, *dims, LR, B1, B2, EPS, 1)),
            ("mt_ema", lambda: hip.mt_ema(*tabs, *dims, 0.5)),
            ("mt_copy", lambda: hip.mt_copy(*tabs, *dims))]


@gpu
def test_no_chunks_is_no_work(hip):
    D = inputs(256)
    T = Table(256, [D.p, D.g, D.m, D.v])
    before = [b.view(torch.int32).clone() for b in T.all_buffers()]
    for _, call in calls(hip, T, n_chunks=0):
        call()
    torch.cuda.synchronize()
    assert all(torch.equal(b.view(torch.int32), b0) for b, b0 in zip(T.all_buffers(), before))


@gpu
def test_refusals(hip):
    D = inputs(256)
    T = Table(256, [D.p, D.g, D.m, D.v])
    bufs = T.all_buffers()
    for kw in (dict(ce=0), dict(ce=255), dict(ce=384), dict(n=0)):
        for name, call in calls(hip, T, **kw):
            refused(name + ": bad tensor table", call, *bufs)
    tabs, dims = T.args()
    refused("mt_sgd: nesterov needs momentum", lambda: hip.mt_sgd(*tabs, None, *dims, LR, 0.0, 1, 0), *bufs)
    refused("mt_adam: step counts from 1", lambda: hip.mt_adam(*tabs, None, *dims, LR, B1, B2, EPS, 0), *bufs)
