"""The strided-row entry points on channel slices of wider buffers and on the arguments that send them to a fallback kernel.

The program hands almost every kernel a row stride beside the channel count (ASPP's five branches in one 5C-wide buffer, the
ClusterBlocks' f | v in one 2 E D buffer, Act.ld everywhere); the launchers pick a 16-byte kernel or a scalar one per call, or
refuse.  Every op below is called in three layouts of each strided operand:

  A  an aligned slice of a wider row (lead % 4 == 0, ld % 4 == 0, ld > C): what the program does -- the 16-byte kernel;
  B  the same row width, the base address off by one float (lead = 5): vr_aligned16 fails;
  C  a ragged row stride (lead 0, ld = C + 5): ld % 4 fails.

B and C take the scalar kernel or are refused (RuntimeError naming the entry point, outputs untouched); which of the two is
written down at each test, from the launcher's source.  With several strided operands every operand has its own lead / ld in
layout A (an index built with another operand's stride shows), and one operand at a time is B or C (each term of the launcher's
predicate separately).  A 16-byte access to a dword-aligned address does not fault on this hardware and gives the right values,
so for the ops without a kernel-family counter (all but conv and the fused Mlp) a B / C case holds the result and the guard
columns, not the kernel choice: that B and C reach the scalar kernel there rests on the launcher's source, quoted at each test.

Checks of every call: the result against the reference of the existing test of that op (fp64 or ATen; for the cluster core
the CPU oracle on the fp32 inputs, as test_cluster_core), at that test's tolerance, on the logical tensors; inputs sit in NaN (a guard column that reaches a result poisons it; at least four guard columns behind
every slice, so that a quad read or written past column C stays inside the allocation and is seen); outputs sit in a fixed bit
pattern, and the guard columns must keep it bit for bit."""
import functools
import types

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests.test_hip_ops import TOL, close, nchw, nhwc, pack, rnd

pytestmark = pytest.mark.gpu

NAN = float("nan")
PAT = 0x7FD5A5A5                 # the outputs' pre-fill: a quiet NaN with a payload, so an unwritten element shows too
A_LAYS = [(4, 8), (8, 8), (12, 12), (16, 4), (4, 16)]      # (lead, trail) of layout A, one per operand: ld = C + 12, 16, 24, 20, 20


@pytest.fixture(scope="module")
def hip():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    import asy_vrnet_amd.hip as h
    return h


# ------------------------------------------------------------------------------------------------ helpers
def lay(kind, i=0):
    return {"A": A_LAYS[i], "B": (5, 7), "C": (0, 5)}[kind]


def embed(t, lead, trail, fill):
    """A (rows..., lead + C + trail) device buffer filled with `fill` (a float, or the int PAT: that bit pattern) with the
    (rows..., C) tensor t in columns [lead, lead + C) -- t may be a shape: the slice keeps the fill.  -> (buffer, slice, ld)."""
    assert trail >= 4
    shape = tuple(t) if isinstance(t, (tuple, torch.Size)) else tuple(t.shape)
    C = shape[-1]
    ld = lead + C + trail
    buf = torch.empty(shape[:-1] + (ld,), device="cuda")
    if isinstance(fill, int):
        buf.view(torch.int32).fill_(fill)
    else:
        buf.fill_(fill)
    view = buf[..., lead:lead + C]
    if isinstance(t, torch.Tensor):
        view.copy_(t)
    assert view.stride(-2) == ld and view.data_ptr() % 16 == (4 * lead) % 16
    return buf, view, ld


def pat(*shape):
    """A contiguous output pre-filled with PAT."""
    t = torch.empty(*shape, device="cuda")
    t.view(torch.int32).fill_(PAT)
    return t


def inp(t, kind, i=0):
    """An input in layout `kind`, NaN all around."""
    return embed(t, *lay(kind, i), NAN)[1]


def outp(t, kind, i=0):
    """An output (a shape; or a tensor for the accumulating forms) in layout `kind`, PAT all around -> (buffer, slice)."""
    return embed(t, *lay(kind, i), PAT)[:2]


def ld(v):
    return v.stride(-2)


def guards_intact(buf, view):
    lead, C = view.storage_offset(), view.shape[-1]
    raw = buf.view(torch.int32)
    return bool((raw[..., :lead] == PAT).all()) and bool((raw[..., lead + C:] == PAT).all())


def check(got, ref, buf, what, tol=TOL, floor=1e-6):
    """got: an output slice of buf.  No NaN from an input guard or an unwritten element, the reference at tol, guards intact."""
    assert not bool(torch.isnan(got).any()), what + ": NaN in the result"
    close(got, ref, tol, what, floor)
    assert guards_intact(buf, got), what + ": guard columns of the output changed"


def refused(name, call, *bufs):
    """The wrapper raises with the entry point's name; the output buffers keep every bit."""
    before = [b.view(torch.int32).clone() if b.dtype == torch.float32 else b.clone() for b in bufs]
    with pytest.raises(RuntimeError, match=name):
        call()
    torch.cuda.synchronize()
    for b, b0 in zip(bufs, before):
        assert torch.equal(b.view(torch.int32) if b.dtype == torch.float32 else b, b0), name + ": a refused call wrote"


def scenarios(n):
    """All operands in layout A; then one operand at a time in B, in C."""
    return [("A",) * n] + [tuple(k if j == i else "A" for j in range(n)) for i in range(n) for k in "BC"]


def sid(s):
    return s if isinstance(s, str) else "".join(s)


def dev(*ts):
    return [t.detach().float().contiguous().cuda() for t in ts]


# ------------------------------------------------------------------------------------------------ 1. moments
# moments_launch (stream_ops.hip): moments_kernel<4> iff C % 4 == 0 and x, x2 (if given), mask (if given) each have ld % 4 == 0
# and a 16-byte aligned base; anything else -> moments_kernel<1> with the chunk plan of width 1 (TPR = 64 at C = 64, 256 at
# C = 256).  Nothing is refused here (ldx >= C holds).  So: A -> <4>; B or C in any one operand -> <1>.
MOM_SHAPES = [(2, 5, 7, 64), (2, 32, 32, 64), (2, 8, 8, 256)]      # ragged; several chunks per sample in both plans; a wide row


@functools.lru_cache(maxsize=None)
def mom_case(shape):
    B, H, W, C = shape
    x, x2, m = rnd(B, H, W, C, seed=1) + 3.0, rnd(B, H, W, C, seed=2), rnd(B, H, W, C, seed=3)
    xd, x2d = x.double().reshape(B, -1, C), x2.double().reshape(B, -1, C)
    xm = torch.where(m.reshape(B, -1, C) > 0, xd, torch.zeros_like(xd))
    refs = ((xd.sum(1), (xd * xd).sum(1)), (xd.sum(1), (xd * x2d).sum(1)), (xm.sum(1), (xm * x2d).sum(1)))
    return x, x2, m, refs


@pytest.mark.parametrize("s", scenarios(3), ids=sid)          # x, x2, mask
@pytest.mark.parametrize("shape", MOM_SHAPES, ids=str)
def test_moments(hip, shape, s):
    B, H, W, C = shape
    x, x2, m, refs = mom_case(shape)
    xv, x2v, mv = inp(x, s[0], 0), inp(x2, s[1], 1), inp(m, s[2], 2)
    assert s != ("A",) * 3 or len({ld(xv), ld(x2v), ld(mv)}) == 3
    forms = ((None, 0, None, 0), (x2v, ld(x2v), None, 0), (x2v, ld(x2v), mv, ld(mv)))
    for (a2, l2, mk, lm), (r1, r2), name in zip(forms, refs, ("x", "x, x2", "x, x2, mask")):
        mom = hip.moments(xv, ld(xv), B, H * W, C, x2=a2, ldx2=l2, mask=mk, ldm=lm)
        assert not bool(torch.isnan(mom).any()), name
        close(mom[..., 0], r1, 1e-6, f"moments({name}) sum")
        close(mom[..., 1], r2, 1e-6, f"moments({name}) second sum")


# ------------------------------------------------------------------------------------------------ 2. affine
# affine_impl (stream_ops.hip): affine_kernel<4> iff C % 4 == 0, bstride % 4 == 0, 16-byte coefficient vectors and, for out and
# every operand that is read (x1, x2, masky only when pre == 2, add -- accumulate makes add = out), ld % 4 == 0 and a 16-byte
# base; else affine_kernel<1> (the flat kernel needs C % 4 != 0: not here).  A -> <4>; B / C in one operand -> <1>.  Row strides
# below C are refused.
@functools.lru_cache(maxsize=None)
def affine_case(shape):
    B, H, W, C = shape
    x1, x2, m, add = (rnd(B, H, W, C, seed=k) for k in (1, 2, 3, 4))
    x1 = x1 + 3.0
    co = [rnd(B, C, seed=10 + k) for k in range(6)]          # A, D1, S1, E, D2, S2
    d = lambda t: t.double()
    bc = lambda t: d(t)[:, None, None, :]
    A, D1, S1, E, D2, S2 = co
    pre0 = bc(A) * (d(x1) - bc(S1)) + bc(D1)
    tail = bc(E) * (d(x2) - bc(S2)) + bc(D2) + d(add)
    refs = [pre0 + tail, torch.relu(pre0) + tail, torch.where(m > 0, pre0, torch.zeros_like(pre0)) + tail]
    acc = d(add) + d(A[0])[None, None, None, :] * d(x1)
    bcast = bc(D2).expand(B, H, W, C)
    return x1, x2, m, add, co, refs, acc, bcast


@pytest.mark.parametrize("s", scenarios(5), ids=sid)          # out, x1, x2, masky, add
@pytest.mark.parametrize("shape", [(2, 5, 7, 64), (2, 16, 16, 64)], ids=str)
def test_affine(hip, shape, s):
    B, H, W, C = shape
    HW = H * W
    x1, x2, m, add, co, refs, acc_ref, bcast_ref = affine_case(shape)
    x1v, x2v, mv, addv = inp(x1, s[1], 1), inp(x2, s[2], 2), inp(m, s[3], 3), inp(add, s[4], 4)
    A, D1, S1, E, D2, S2 = dev(*co)
    for pre in (0, 1, 2):          # per-sample coefficients, out-of-place addend
        buf, out = outp(shape, s[0], 0)
        hip.affine(out, ld(out), B, HW, C, x1=x1v, ld1=ld(x1v), A=A, D1=D1, S1=S1, pre=pre, masky=mv, ldm=ld(mv), x2=x2v,
                   ld2=ld(x2v), E=E, D2=D2, S2=S2, bstride=C, add=addv, ldadd=ld(addv))
        check(out, refs[pre], buf, f"affine pre={pre}")
    buf, out = outp(add.cuda(), s[0], 0)          # in place, coefficients shared by the samples
    hip.affine(out, ld(out), B, HW, C, x1=x1v, ld1=ld(x1v), A=A[0].contiguous(), bstride=0, accumulate=1)
    check(out, acc_ref, buf, "affine accumulate, bstride 0")
    # the constant of ASPP's pooling branch into cat[..., 4 C:] (here with guard columns behind the last branch)
    lead, trail = (4 * C, 4) if s[0] == "A" else lay(s[0])
    buf, out, ldo = embed(shape, lead, trail, PAT)
    hip.affine(out, ldo, B, HW, C, D2=D2, bstride=C)
    check(out, bcast_ref, buf, "affine broadcast")


def test_affine_and_depthwise_refuse_rows_shorter_than_the_channel_count(hip):
    B, H, W, C = 1, 3, 3, 8
    x, out = torch.zeros(B, H, W, C, device="cuda"), embed((B, H, W, C), 0, 4, PAT)[0]
    refused("affine", lambda: hip.affine(out, C + 4, B, H * W, C, x1=x, ld1=C - 4), out)
    refused("affine", lambda: hip.affine(out, C - 4, B, H * W, C, x1=x, ld1=C), out)
    w = torch.zeros(C, 1, 3, 3, device="cuda")
    refused("dwconv3x3", lambda: hip.dwconv3x3(x, C - 4, w, out, C + 4, B, H, W, C), out)
    refused("dwconv3x3", lambda: hip.dwconv3x3(x, C, w, out, C - 4, B, H, W, C), out)


# ------------------------------------------------------------------------------------------------ 3. BatchNorm + ReLU, ASPP's way
# Forward: bn_stats_fwd on a strided z (moments_launch: A -> <4>, B / C -> <1>), affine(pre = 1) into a branch slice of the
# 5 C-wide cat buffer.  Backward: dy = dcat[..., k C:] and the mask = cat[..., k C:], ld = 5 C: bn_stats_bwd (moments over dy, z,
# mask), bn_stats_bwd_zmask (dy, z), bn_apply_bwd_zmask and affine(pre = 2) (affine_impl).  All of them fall to the scalar
# kernels when one operand is B or C; none refuses.
@functools.lru_cache(maxsize=None)
def bn_case(C):
    B, H, W = 3, 10, 12
    z = (rnd(B, H, W, C, seed=1) * 1.5 + 40.0).double().requires_grad_(True)          # |mean| >> std
    gam, bet = (rnd(C, seed=2) * 0.3 + 1).double().requires_grad_(True), (rnd(C, seed=3) * 0.5).double().requires_grad_(True)
    rm, rv = (rnd(C, seed=4) * 0.1).double(), (rnd(C, seed=5, kind="uniform") + 0.5).double()
    rm0, rv0 = rm.clone(), rv.clone()
    y = torch.relu(F.batch_norm(z.permute(0, 3, 1, 2), rm, rv, gam, bet, True, 0.03, 1e-3)).permute(0, 2, 3, 1)
    g = rnd(B, H, W, C, seed=6)
    y.backward(g.double())
    return types.SimpleNamespace(z=z.detach().float(), gam=gam.detach().float(), bet=bet.detach().float(), rm0=rm0.float(),
                                 rv0=rv0.float(), rm=rm, rv=rv, y=y.detach(), g=g, dz=z.grad, dgam=gam.grad, dbet=bet.grad)


@pytest.mark.parametrize("s", scenarios(4), ids=sid)          # z, cat (y and the mask), dcat (dy), dz
@pytest.mark.parametrize("C", [24, 64])
def test_batch_norm_relu_chain_in_branch_slices(hip, C, s):
    B, H, W = 3, 10, 12
    HW, shape = H * W, (3, 10, 12, C)
    r = bn_case(C)
    branch = lambda kind: {"A": (2 * C, 2 * C), "B": (2 * C + 1, 2 * C - 1), "C": (0, 5)}[kind]      # A, B: ld = 5 C
    z = inp(r.z, s[0], 0)
    gam, bet, rm, rv = dev(r.gam, r.bet, r.rm0, r.rv0)
    nbt = torch.zeros((), dtype=torch.int64, device="cuda")
    A, D, S = (torch.empty(C, device="cuda") for _ in range(3))
    ms = torch.empty(C, 2, device="cuda")
    hip.bn_stats_fwd(z, ld(z), gam, bet, 1e-3, 0.03, rm, rv, nbt, B, HW, C, A, D, S, ms)
    ybuf, y, ldy = embed(shape, *branch(s[1]), PAT)
    hip.affine(y, ldy, B, HW, C, x1=z, ld1=ld(z), A=A, D1=D, S1=S, pre=1)
    check(y, r.y, ybuf, "bn + relu forward")
    close(rm, r.rm, what="running_mean")
    close(rv, r.rv, what="running_var")
    assert int(nbt.item()) == 1
    _, dy, lddy = embed(r.g, *branch(s[2]), NAN)
    assert s[1] != "A" or s[2] != "A" or ldy == lddy == 5 * C
    co4 = [torch.empty(C, device="cuda") for _ in range(4)]
    dg4, db4 = torch.full((C,), 3.0, device="cuda"), torch.full((C,), 3.0, device="cuda")
    hip.bn_stats_bwd(dy, lddy, z, ld(z), y, ldy, ms, gam, True, B, HW, C, *co4, dg4, db4, 1)
    close(dg4, r.dgam + 3, what="bn_stats_bwd dgamma")
    close(db4, r.dbet + 3, what="bn_stats_bwd dbeta")
    co5 = [torch.empty(C, device="cuda") for _ in range(4)]
    dg5, db5 = torch.full((C,), 3.0, device="cuda"), torch.full((C,), 3.0, device="cuda")
    hip.bn_stats_bwd_zmask(dy, lddy, z, ld(z), (A, D, S), ms, gam, True, B, HW, C, *co5, dg5, db5, 1)
    close(dg5, r.dgam + 3, what="bn_stats_bwd_zmask dgamma")
    close(db5, r.dbet + 3, what="bn_stats_bwd_zmask dbeta")
    if s[1] == "A":          # the mask operand does not change the kernel: the recomputed mask gives the stored mask's bits
        for a_, b_ in zip(co5 + [dg5, db5], co4 + [dg4, db4]):
            assert torch.equal(a_, b_), "bn_stats_bwd_zmask against bn_stats_bwd"
    dzbuf, dz = outp(shape, s[3], 3)
    hip.bn_apply_bwd_zmask(dy, lddy, z, ld(z), (A, D, S), *co5, dz, ld(dz), B, HW, C)
    check(dz, r.dz, dzbuf, "bn_apply_bwd_zmask")
    dzbuf, dz = outp(shape, s[3], 3)
    hip.affine(dz, ld(dz), B, HW, C, x1=dy, ld1=lddy, A=co4[0], pre=2, masky=y, ldm=ldy, x2=z, ld2=ld(z), E=co4[1], D2=co4[2],
               S2=co4[3])
    check(dz, r.dz, dzbuf, "affine pre=2 with the mask slice")


# ------------------------------------------------------------------------------------------------ 4. GroupNorm
# gn_stats_fwd: moments_launch in its total_only form (A -> <4>, B / C -> <1>), never refused.
# gn_apply_fwd / gn_apply_bwd have 16-byte kernels only: VR_CHECK_ARG refuses C % 4, ld % 4 (layout C: hip.gn_apply_ok says so
# too) and unaligned bases (layout B: the predicate does not see addresses) with "gn_apply_fwd: ..." / "gn_apply_bwd: ...".
@functools.lru_cache(maxsize=None)
def gn_case():
    B, H, W, C = 2, 16, 16, 64
    x = rnd(B, H, W, C, seed=1) * 1.5 + 10.0
    gam, bet = rnd(C, seed=2) * 0.3 + 1, rnd(C, seed=3) * 0.5
    g, addend = rnd(B, H, W, C, seed=4), rnd(B, H, W, C, seed=5)
    xd = x.double().requires_grad_(True)
    gd, bd = gam.double().requires_grad_(True), bet.double().requires_grad_(True)
    ref = F.group_norm(xd.permute(0, 3, 1, 2), 1, gd, bd, 1e-5).permute(0, 2, 3, 1)
    ref.backward(g.double())
    nb = (C + 31) // 32          # tile pairs as a conv epilogue leaves them: (sum, sumsq) per 32 rows x 32 channels, fp64
    t = x.double().view(B, H * W // 32, 32, C)
    pairs = torch.zeros(B, H * W // 32, nb, 2, dtype=torch.float64)
    for j in range(nb):
        blk = t[..., 32 * j:32 * (j + 1)]
        pairs[:, :, j, 0], pairs[:, :, j, 1] = blk.sum((2, 3)), (blk * blk).sum((2, 3))
    mean = x.double().mean((1, 2, 3))
    rstd = 1 / torch.sqrt(x.double().var((1, 2, 3), unbiased=False) + 1e-5)
    return types.SimpleNamespace(x=x, gam=gam, bet=bet, g=g, add=addend, y=ref.detach(), dx=xd.grad, dgam=gd.grad, dbet=bd.grad,
                                 pairs=pairs, per=(H * W // 32) * nb, mean=mean, rstd=rstd)


@pytest.mark.parametrize("kind", "ABC")
def test_group_norm_statistics(hip, kind):
    B, H, W, C = 2, 16, 16, 64
    r = gn_case()
    x = inp(r.x, kind)
    gam, bet = dev(r.gam, r.bet)
    A, D, S = (torch.empty(B, C, device="cuda") for _ in range(3))
    ms = torch.empty(B, 2, device="cuda")
    hip.gn_stats_fwd(x, ld(x), gam, bet, 1e-5, B, H * W, C, A, D, S, ms)
    close(ms[:, 0], r.mean, 1e-6, "mean")
    close(ms[:, 1], r.rstd, 1e-5, "rstd")
    bc = lambda t: t.double().cpu()[:, None, None, :]
    close(bc(A) * (r.x.double() - bc(S)) + bc(D), r.y, what="A (x - S) + D of gn_stats_fwd")


@pytest.mark.parametrize("s", scenarios(2), ids=sid)          # x, y
def test_group_norm_apply_forward(hip, s):
    B, H, W, C = 2, 16, 16, 64
    r = gn_case()
    x = inp(r.x, s[0], 0)
    buf, y = outp(r.x.shape, s[1], 1)
    gam, bet = dev(r.gam, r.bet)
    ms = pat(B, 2)
    call = lambda: hip.gn_apply_fwd(x, ld(x), r.pairs.cuda(), r.per, gam, bet, 1e-5, B, H * W, C, y, ld(y), ms)
    assert hip.gn_apply_ok(C, ld(x), ld(y)) == ("C" not in s)
    if s != ("A", "A"):
        refused("gn_apply_fwd", call, buf, ms)
        return
    call()
    check(y, r.y, buf, "gn_apply_fwd", 2e-5)
    close(ms[:, 0], r.mean, 1e-6, "mean")
    close(ms[:, 1], r.rstd, 1e-5, "rstd")


@pytest.mark.parametrize("s", scenarios(4), ids=sid)          # dy, x, out, add
def test_group_norm_apply_backward(hip, s):
    B, H, W, C = 2, 16, 16, 64
    r = gn_case()
    dy, x, add = inp(r.g, s[0], 0), inp(r.x, s[1], 1), inp(r.add, s[3], 3)
    buf, out = outp(r.x.shape, s[2], 2)
    gam, = dev(r.gam)
    ms = torch.stack([r.mean, r.rstd], 1).float().cuda()
    dg, db = torch.full((C,), 2.0, device="cuda"), torch.full((C,), 2.0, device="cuda")
    call = lambda: hip.gn_apply_bwd(dy, ld(dy), x, ld(x), ms, gam, B, H * W, C, out, ld(out), dg, db, 1, add=add, ldadd=ld(add))
    assert hip.gn_apply_ok(C, ld(dy), ld(x), ld(out), ld(add)) == ("C" not in s)
    if s != ("A",) * 4:
        refused("gn_apply_bwd", call, buf, dg, db)
        return
    call()
    check(out, r.dx + r.add.double(), buf, "gn_apply_bwd dx + add", 5e-5)
    close(dg, r.dgam + 2, 5e-5, "dgamma (accumulated)")
    close(db, r.dbet + 2, 5e-5, "dbeta (accumulated)")


# ------------------------------------------------------------------------------------------------ 5. spatial
# vrnet_dwconv3x3_f32: 16-byte kernels iff C % 4 == 0, 256 % (C / 4) == 0, ldx % 4 == ldy % 4 == 0 and 16-byte x, y, w --
# dwconv3x3_slide_kernel<8> when W % 8 == 0 (W = 8), dwconv3x3_vec_kernel otherwise (W = 9); B / C in x or y -> dwconv3x3_kernel.
@functools.lru_cache(maxsize=None)
def dw_case(shape):
    B, H, W, C = shape
    x = rnd(B, C, H, W, seed=1).double().requires_grad_(True)
    w = rnd(C, 1, 3, 3, seed=2).double().requires_grad_(True)
    y = F.conv2d(x, w, None, 1, 1, 1, C)
    g = rnd(B, C, H, W, seed=3)
    y.backward(g.double())
    p = lambda t: t.detach().permute(0, 2, 3, 1).contiguous()
    return types.SimpleNamespace(x=p(x).float(), g=p(g), w=w.detach().float(), y=p(y), dx=p(x.grad), dw=w.grad, y0=rnd(B, H, W, C, seed=4))


@pytest.mark.parametrize("s", scenarios(2), ids=sid)          # x, y
@pytest.mark.parametrize("W", [8, 9])
def test_depthwise(hip, W, s):
    B, H, C = 2, 9, 64
    r = dw_case((B, H, W, C))
    w, = dev(r.w)
    for flip, src, ref, what in ((0, r.x, r.y, "dw fwd"), (1, r.g, r.dx, "dw dgrad")):
        xv = inp(src, s[0], 0)
        buf, out = outp(src.shape, s[1], 1)
        hip.dwconv3x3(xv, ld(xv), w, out, ld(out), B, H, W, C, flip=flip)
        check(out, ref, buf, what)
        buf, out = outp(r.y0.cuda(), s[1], 1)
        hip.dwconv3x3(xv, ld(xv), w, out, ld(out), B, H, W, C, flip=flip, accumulate=1)
        check(out, ref + r.y0.double(), buf, what + ", accumulate")


# vrnet_dwconv3x3_wgrad_f32: dwconv3x3_wgrad_slide_kernel iff dw_wgrad_slide_ok (W % 16 == 0, C % 4 == 0, ldx % 4 == lddy % 4
# == 0, 16-byte x and dy, ...): (2, 16, 16, 64) in layout A; dwconv3x3_wgrad_kernel (scalar loads, any stride) for B / C there and
# for every layout of (2, 9, 8, 64).  Tolerances: 2e-5 where the sliding-window kernel runs (its test's), 1e-4 for the generic one.
@pytest.mark.parametrize("s", scenarios(2), ids=sid)          # x, dy
@pytest.mark.parametrize("shape", [(2, 16, 16, 64), (2, 9, 8, 64)], ids=str)
def test_depthwise_wgrad(hip, shape, s):
    B, H, W, C = shape
    r = dw_case(shape)
    xv, gv = inp(r.x, s[0], 0), inp(r.g, s[1], 1)
    tol = 2e-5 if (W % 16 == 0 and s == ("A", "A")) else TOL
    dw = torch.full((C, 1, 3, 3), NAN, device="cuda")
    hip.dwconv3x3_wgrad(xv, ld(xv), gv, ld(gv), dw, B, H, W, C)
    close(dw, r.dw, tol, what="dw wgrad")
    dw2 = torch.full((C, 1, 3, 3), 2.0, device="cuda")
    hip.dwconv3x3_wgrad(xv, ld(xv), gv, ld(gv), dw2, B, H, W, C, accumulate=1)
    close(dw2, r.dw + 2.0, tol, what="dw wgrad, accumulate")


# upsample_launch (spatial.hip): NHWC output -> upsample_vec_kernel iff C % 4 == 0, ldx % 4 == ldy % 4 == 0, 16-byte x and y, else
# upsample_kernel.  NCHW output -> upsample_nchw4_kernel iff OW % 4 == 0 and y is 16-byte aligned (scale 4: OW = 20), else
# upsample_kernel (scale 2: OW = 10); both read x one float at a time, so ldx and x's base are rightly not in that predicate.
# upsample_bwd_launch: upsample_bwd_vec_kernel iff NHWC dy, C % 4 == 0, lddy % 4 == lddx % 4 == 0, 16-byte dy and dx; else
# upsample_bwd_kernel.  Nothing is refused.
@functools.lru_cache(maxsize=None)
def up_case(scale):
    B, H, W, C = 2, 6, 5, 64
    x = rnd(B, C, H, W, seed=1).double().requires_grad_(True)
    y = F.interpolate(x, scale_factor=scale, mode="bilinear", align_corners=True)
    g = rnd(*y.shape, seed=2)
    y.backward(g.double())
    A, D, S = rnd(C, seed=3), rnd(C, seed=4), rnd(C, seed=5)
    bc = lambda t: t.double()[None, :, None, None]
    lo = torch.relu(bc(A) * (x.detach() - bc(S)) + bc(D))
    ybn = F.interpolate(lo, scale_factor=scale, mode="bilinear", align_corners=True)
    p = lambda t: t.detach().permute(0, 2, 3, 1).contiguous()
    return types.SimpleNamespace(x=p(x).float(), y=y.detach(), ybn=ybn, g=g, dx=p(x.grad), coef=(A, D, S), dx0=rnd(B, H, W, C, seed=6))


@pytest.mark.parametrize("s", scenarios(2), ids=sid)          # x, y
@pytest.mark.parametrize("scale", [2, 4])
def test_upsample_nhwc(hip, scale, s):
    B, H, W, C = 2, 6, 5, 64
    r = up_case(scale)
    xv = inp(r.x, s[0], 0)
    A, D, S = dev(*r.coef)
    shape = (B, H * scale, W * scale, C)
    buf, out = outp(shape, s[1], 1)
    hip.upsample(xv, ld(xv), out, ld(out), B, H, W, C, scale)
    check(out, r.y.permute(0, 2, 3, 1), buf, "up fwd")
    buf, out = outp(shape, s[1], 1)
    hip.bn_relu_upsample(xv, ld(xv), A, D, S, out, ld(out), B, H, W, C, scale)
    check(out, r.ybn.permute(0, 2, 3, 1), buf, "bn + relu + up fwd")


@pytest.mark.parametrize("kind", "ABC")                       # x (the NCHW output is contiguous)
@pytest.mark.parametrize("scale", [2, 4])
def test_upsample_nchw(hip, scale, kind):
    B, H, W, C = 2, 6, 5, 64
    r = up_case(scale)
    xv = inp(r.x, kind)
    A, D, S = dev(*r.coef)
    out = torch.full((B, C, H * scale, W * scale), NAN, device="cuda")
    hip.upsample(xv, ld(xv), out, 0, B, H, W, C, scale, out_nchw=1)
    close(out, r.y, what="up fwd nchw")
    out.fill_(NAN)
    hip.bn_relu_upsample(xv, ld(xv), A, D, S, out, 0, B, H, W, C, scale, out_nchw=1)
    close(out, r.ybn, what="bn + relu + up fwd nchw")


@pytest.mark.parametrize("s", scenarios(2) + [("N", "A"), ("N", "B"), ("N", "C")], ids=sid)          # dy (N: NCHW, contiguous), dx
@pytest.mark.parametrize("scale", [2, 4])
def test_upsample_adjoint(hip, scale, s):
    B, H, W, C = 2, 6, 5, 64
    r = up_case(scale)
    if s[0] == "N":
        dy, lddy, nchw_in = r.g.cuda(), 0, 1
    else:
        dy = inp(r.g.permute(0, 2, 3, 1).contiguous(), s[0], 0)
        lddy, nchw_in = ld(dy), 0
    buf, dx = outp(r.x.shape, s[1], 1)
    hip.upsample_bwd(dy, lddy, nchw_in, dx, ld(dx), B, H, W, C, scale)
    check(dx, r.dx, buf, "up bwd")
    buf, dx = outp(r.dx0.cuda(), s[1], 1)
    hip.upsample_bwd(dy, lddy, nchw_in, dx, ld(dx), B, H, W, C, scale, accumulate=1)
    check(dx, r.dx + r.dx0.double(), buf, "up bwd, accumulate")


# ------------------------------------------------------------------------------------------------ 6. cluster core
# cluster_check / cluster_fwd_impl / cluster_bwd_impl (cluster.hip) have 16-byte kernels only: ld, ldo, lddo, lddf % 4 and the
# bases of f, v, out, dout, df, dv must be 16-byte aligned, else "cluster_fwd: rows must be 16-byte aligned" /
# "cluster_bwd: rows must be 16-byte aligned".  Layout A is the program's f | v in one buffer (v = fv[..., E D:]) and df | dv
# likewise, here with guard columns around the 2 E D columns; out and dout are slices of wider buffers.
CLUSTER = [(2, 4, 24, 16, 16, 2), (1, 2, 32, 36, 30, 2), (2, 4, 32, 4, 4, 2)]      # register kernel; smallest streaming case; N = 4


@functools.lru_cache(maxsize=None)
def cluster_inputs(case):
    B, E, D, H, W, fold = case
    return rnd(B, H, W, E * D, seed=1), rnd(B, H, W, E * D, seed=2), rnd(B, H, W, E * D, seed=3)


def cluster_buffers(case, kinds):
    """kinds: layouts of (f | v, out, dout, df | dv)."""
    B, E, D, H, W, fold = case
    ED = E * D
    f, v, g = cluster_inputs(case)
    n = types.SimpleNamespace()
    _, fv, n.ld = embed(torch.cat([f, v], -1), *lay(kinds[0], 0), NAN)
    n.f, n.v = fv[..., :ED], fv[..., ED:]
    n.obuf, n.out = outp((B, H, W, ED), kinds[1], 1)
    n.dout = inp(g, kinds[2], 2)
    n.dbuf, dfv = outp((B, H, W, 2 * ED), kinds[3], 3)
    n.df, n.dv, n.lddf = dfv[..., :ED], dfv[..., ED:], ld(dfv)
    n.idx = torch.zeros(B, H, W, E, dtype=torch.uint8, device="cuda")
    n.wgt = torch.empty(B, H, W, E, device="cuda")
    n.alpha, n.beta = torch.tensor([1.3], device="cuda"), torch.tensor([-0.2], device="cuda")
    n.dab = torch.zeros(2, device="cuda")
    return n


def cluster_calls(hip, case, n):
    B, E, D, H, W, fold = case
    fwd = lambda: hip.cluster_fwd(n.f, n.v, n.ld, n.alpha, n.beta, n.out, ld(n.out), n.idx, n.wgt, B, H, W, E, D, fold)
    bwd = lambda: hip.cluster_bwd(n.f, n.v, n.ld, n.alpha, n.beta, n.idx, n.dout, ld(n.dout), n.df, n.dv, n.lddf, n.dab[0:1],
                                  n.dab[1:2], 0, B, H, W, E, D, fold)
    return fwd, bwd


@pytest.mark.parametrize("case", CLUSTER, ids=str)
def test_cluster_core_on_slices(hip, case):
    from oracle import vrnet_oracle as O
    B, E, D, H, W, fold = case
    n = cluster_buffers(case, "AAAA")
    assert (n.ld, n.lddf) == (2 * E * D + 12, 2 * E * D + 20) and n.v.data_ptr() - n.f.data_ptr() == 4 * E * D
    fwd, bwd = cluster_calls(hip, case, n)
    fwd()
    fc, vc, gc = (t.permute(0, 3, 1, 2).contiguous().requires_grad_(True) for t in cluster_inputs(case))
    alpha, beta = torch.tensor([1.3], requires_grad=True), torch.tensor([-0.2], requires_grad=True)
    rep = {}
    ref, _ = O.cluster_core(fc, vc, alpha, beta, E, fold, forced_idx=n.idx.permute(0, 3, 1, 2).contiguous().cpu().long(), report=rep)
    assert rep["mismatch"] <= max(2, rep["points"] // 5000), rep          # as test_cluster_core: only numerical near-ties
    assert rep["max_gap"] < 1e-5, rep
    check(n.out, ref.permute(0, 2, 3, 1), n.obuf, "cluster fwd")
    ref.backward(gc.detach())
    bwd()
    assert guards_intact(n.dbuf, n.dbuf[..., lay("A", 3)[0]:lay("A", 3)[0] + 2 * E * D]), "guard columns of df | dv changed"
    for got, want, tol, floor, what in ((n.dv, vc.grad, TOL, 1e-6, "cluster dv"), (n.df, fc.grad, 5e-4, 1e-2, "cluster df")):
        assert not bool(torch.isnan(got).any()), what
        close(nchw(got), want, tol, what, floor)
    close(n.dab[0:1], alpha.grad, 5e-4, what="dalpha", floor=1e-2)
    close(n.dab[1:2], beta.grad, 5e-4, what="dbeta", floor=1e-2)


@pytest.mark.parametrize("kind", "BC")
@pytest.mark.parametrize("operand", range(4), ids=["fv", "out", "dout", "dfdv"])
def test_cluster_core_refuses_unaligned_rows(hip, operand, kind):
    case = CLUSTER[2]
    n = cluster_buffers(case, "".join(kind if j == operand else "A" for j in range(4)))
    fwd, bwd = cluster_calls(hip, case, n)
    if operand in (0, 1):
        refused("cluster_fwd: rows must be 16-byte aligned", fwd, n.obuf, n.idx)
    if operand in (0, 2, 3):
        refused("cluster_bwd: rows must be 16-byte aligned", bwd, n.dbuf, n.dab)


# ------------------------------------------------------------------------------------------------ 7. fused Mlp, precision 2
# vrnet_mlp_{fwd,bwd,bwd_rc}_f32 (mlp_fused.hip) have 16-byte kernels only: mlp_vec_ok wants every tensor 16-byte aligned with
# ld % 4 == 0, else "<entry point>: tensors must be 16-byte aligned with row strides that are multiples of 4".  Layout A runs
# the x6 kernels (family 7); B and C are refused for every strided operand.
MLP = [(1, 8, 12, 64, 128), (3, 8, 8, 128, 96)]


@functools.lru_cache(maxsize=None)
def mlp_case(case):
    B, H, W, C, hid = case
    M = B * H * W
    x, res = rnd(M, C, seed=1), rnd(M, C, seed=2)
    w1, b1 = rnd(hid, C, seed=3) / np.sqrt(C), rnd(hid, seed=4)
    w2, b2 = rnd(C, hid, seed=5) / np.sqrt(hid), rnd(C, seed=6)
    ls, dy = rnd(C, seed=7), rnd(M, C, seed=8)
    d = lambda t: t.double()
    u = d(x) @ d(w1).T + d(b1)
    y = d(res) + d(ls) * (F.gelu(u) @ d(w2).T + d(b2))
    return types.SimpleNamespace(M=M, x=x, res=res, w1=w1, b1=b1, w2=w2, b2=b2, ls=ls, dy=dy, u=u, y=y)


def mlp_buffers(hip, case, fk, bk):
    """fk: layouts of the forward's (x, res, y, u); bk: of the backward's (dy, h, du, dx)."""
    B, H, W, C, hid = case
    r = mlp_case(case)
    n = types.SimpleNamespace(r=r)
    n.x, n.res = inp(r.x, fk[0], 0), inp(r.res, fk[1], 1)
    n.ybuf, n.y = outp((r.M, C), fk[2], 2)
    n.ubuf, n.u = outp((r.M, hid), fk[3], 3)
    n.dy = inp(r.dy, bk[0], 4)
    n.hbuf, n.h = outp((r.M, hid), bk[1], 0)
    n.dubuf, n.du = outp((r.M, hid), bk[2], 1)
    n.dxbuf, n.dx = outp((r.M, C), bk[3], 2)
    n.w1, n.w2, n.b1, n.b2, n.ls = dev(r.w1, r.w2, r.b1, r.b2, r.ls)
    return n


@pytest.mark.parametrize("case", MLP, ids=str)
def test_fused_mlp_on_slices(hip, case):
    B, H, W, C, hid = case
    n = mlp_buffers(hip, case, "AAAA", "AAAA")
    r, M = n.r, n.r.M
    fwd, bwd = hip.mlp_pack(n.w1, n.w2, C, hid, 2)
    hip.mlp_fwd(n.x, ld(n.x), fwd, n.b1, n.b2, n.res, ld(n.res), n.ls, n.y, ld(n.y), n.u, ld(n.u), None, M, C, hid, 2)
    assert hip.last_kernel() == 7
    check(n.u, r.u, n.ubuf, "u", 2e-5)
    check(n.y, r.y, n.ybuf, "y", 2e-5)
    # backward from the stored u, as test_fused_mlp_against_fp64
    d = lambda t: t.double()
    uu = n.u.double().cpu()
    cdf = 0.5 * (1 + torch.erf(uu / np.sqrt(2.0)))
    gp = cdf + uu * torch.exp(-0.5 * uu * uu) / np.sqrt(2 * np.pi)
    du_ref = (d(r.dy * r.ls) @ d(r.w2)) * gp
    dx_ref = d(du_ref.float()) @ d(r.w1)
    hip.mlp_bwd(n.dy, ld(n.dy), n.ls, bwd, n.u, ld(n.u), n.h, ld(n.h), n.du, ld(n.du), n.dx, ld(n.dx), M, C, hid, 2)
    assert hip.last_kernel() == 7
    check(n.h, uu * cdf, n.hbuf, "recomputed h", 2e-6)
    check(n.du, du_ref, n.dubuf, "du", 2e-5)
    check(n.dx, dx_ref, n.dxbuf, "dx", 2e-5)
    # the backward that recomputes u from the strided x: the stored-u kernel's bits
    assert hip.mlp_rc_ok(C, hid)
    m = mlp_buffers(hip, case, "AAAA", "AAAA")
    rc = hip.mlp_pack_rc(n.w1, n.w2, C, hid, 2)
    hip.mlp_bwd_rc(m.dy, ld(m.dy), m.ls, rc, m.x, ld(m.x), m.b1, m.h, ld(m.h), m.du, ld(m.du), m.dx, ld(m.dx), M, C, hid, 2)
    assert hip.last_kernel() == 7
    check(m.h, uu * cdf, m.hbuf, "rc: recomputed h", 2e-6)
    check(m.du, du_ref, m.dubuf, "rc: du", 2e-5)
    check(m.dx, dx_ref, m.dxbuf, "rc: dx", 2e-5)
    assert torch.equal(m.h, n.h) and torch.equal(m.du, n.du) and torch.equal(m.dx, n.dx)


@pytest.mark.parametrize("kind", "BC")
@pytest.mark.parametrize("operand", range(8), ids=["x", "res", "y", "u", "dy", "h", "du", "dx"])
def test_fused_mlp_refuses_unaligned_rows(hip, operand, kind):
    case = MLP[0]
    B, H, W, C, hid = case
    kinds = "".join(kind if j == operand else "A" for j in range(8))
    n = mlp_buffers(hip, case, kinds[:4], kinds[4:])
    M = n.r.M
    fwd, bwd = hip.mlp_pack(n.w1, n.w2, C, hid, 2)
    rc = hip.mlp_pack_rc(n.w1, n.w2, C, hid, 2)
    outs = (n.hbuf, n.dubuf, n.dxbuf)
    if operand < 4:
        refused("mlp_fwd: tensors must be 16-byte aligned",
                lambda: hip.mlp_fwd(n.x, ld(n.x), fwd, n.b1, n.b2, n.res, ld(n.res), n.ls, n.y, ld(n.y), n.u, ld(n.u), None, M, C,
                                    hid, 2), n.ybuf, n.ubuf)
    if operand >= 3:          # u is the stored pre-activation the backward reads
        refused("mlp_bwd: tensors must be 16-byte aligned",
                lambda: hip.mlp_bwd(n.dy, ld(n.dy), n.ls, bwd, n.u, ld(n.u), n.h, ld(n.h), n.du, ld(n.du), n.dx, ld(n.dx), M, C,
                                    hid, 2), *outs)
    if operand == 0 or operand >= 4:
        refused("mlp_bwd_rc: tensors must be 16-byte aligned",
                lambda: hip.mlp_bwd_rc(n.dy, ld(n.dy), n.ls, rc, n.x, ld(n.x), n.b1, n.h, ld(n.h), n.du, ld(n.du), n.dx, ld(n.dx),
                                       M, C, hid, 2), *outs)


# ------------------------------------------------------------------------------------------------ 8. attention, cat2
# vrnet_sa_apply_f32 / vrnet_sa_bwd_f32 (spatial.hip): one float per access everywhere, no 16-byte form: every layout is served
# by the same kernels (sa_apply_kernel; sa_bwd_reduce_kernel + sa_bwd_apply_kernel).
@functools.lru_cache(maxsize=None)
def sa_case():
    from oracle import vrnet_oracle as O
    B, H, W, C, G = 2, 6, 7, 64, 8
    cp = C // (2 * G)
    d = lambda t: t.double().requires_grad_(True)
    x = d(rnd(B, C, H, W, seed=1) + 8.0)
    names = ["cweight", "cbias", "sweight", "sbias"]
    P = {"m." + n: d(rnd(1, cp, 1, 1, seed=10 + i)) for i, n in enumerate(names)}
    P["m.gn.weight"], P["m.gn.bias"] = d(rnd(cp, seed=20) * 0.3 + 1), d(rnd(cp, seed=21))
    y = O.shuffle_attention(P, "m", x, G)
    g = rnd(B, C, H, W, seed=3)
    y.backward(g.double())
    order = ["m.cweight", "m.cbias", "m.sweight", "m.sbias", "m.gn.weight", "m.gn.bias"]
    rad = rnd(B, H, W, C, seed=4)
    cat = O.shuffle2(torch.cat([y.detach(), rad.double().permute(0, 3, 1, 2)], 1)).permute(0, 2, 3, 1)
    p = lambda t: t.detach().permute(0, 2, 3, 1).contiguous()
    return types.SimpleNamespace(x=p(x).float(), g=p(g), y=p(y), dx=p(x.grad), params=[P[k].detach().float().reshape(-1) for k in order],
                                 pgrads=[P[k].grad.reshape(-1) for k in order], rad=rad, cat=cat, dx0=rnd(B, H, W, C, seed=5))


def sa_coefs(hip, r, B, HW, C, G):
    """The gate's coefficients from the contiguous x (moments + sa_coef_fwd: inputs of the kernels under test)."""
    xc = r.x.cuda()
    mom = hip.moments(xc, C, B, HW, C)
    Pq, Qq, Mn = (torch.empty(B, C, device="cuda") for _ in range(3))
    params = dev(*r.params)
    hip.sa_coef_fwd(mom, *params, B, HW, C, G, Pq, Qq, Mn)
    return mom, params, Pq, Qq, Mn


@pytest.mark.parametrize("s", scenarios(2), ids=sid)          # x, y
def test_shuffle_attention_apply(hip, s):
    B, H, W, C, G = 2, 6, 7, 64, 8
    r = sa_case()
    _, _, Pq, Qq, Mn = sa_coefs(hip, r, B, H * W, C, G)
    xv = inp(r.x, s[0], 0)
    buf, out = outp(r.x.shape, s[1], 1)
    hip.sa_apply(xv, ld(xv), Pq, Qq, Mn, out, ld(out), B, H * W, C)
    check(out, r.y, buf, "sa fwd")


@pytest.mark.parametrize("s", scenarios(3), ids=sid)          # dy, x, dx
def test_shuffle_attention_backward(hip, s):
    B, H, W, C, G = 2, 6, 7, 64, 8
    r = sa_case()
    mom, params, Pq, Qq, Mn = sa_coefs(hip, r, B, H * W, C, G)
    gv, xv = inp(r.g, s[0], 0), inp(r.x, s[1], 1)
    EF = torch.empty(2, B, C, device="cuda")
    buf, dx = outp(r.x.shape, s[2], 2)
    grads = [torch.zeros(C // (2 * G), device="cuda") for _ in range(6)]
    hip.sa_bwd(gv, ld(gv), xv, ld(xv), Pq, Qq, Mn, mom, params, dx, ld(dx), grads, EF, B, H * W, C, G, 0, 0)
    check(dx, r.dx, buf, "sa dx")
    for gk, want in zip(grads, r.pgrads):
        close(gk, want, 2e-4, what="sa parameter gradient")
    buf, dx = outp(r.dx0.cuda(), s[2], 2)
    hip.sa_bwd(gv, ld(gv), xv, ld(xv), Pq, Qq, Mn, mom, params, dx, ld(dx), grads, EF, B, H * W, C, G, 1, 1)
    check(dx, r.dx + r.dx0.double(), buf, "sa dx, accumulate")
    for gk, want in zip(grads, r.pgrads):
        close(gk, 2 * want, 2e-4, what="sa parameter gradient, accumulate")


# vrnet_sa_cat_sums_f32 (stream_ops.hip): one kernel -- x one float at a time (every layout served), the radar map r as 8-byte
# pairs (ldr % 2 == 0 and an 8-byte base: B and C refused), cat as 16-byte stores (ldc % 4 == 0, 16-byte base: B and C
# refused) -- "sa_cat_sums: needs ...".
@pytest.mark.parametrize("s", scenarios(3), ids=sid)          # x, r, cat
def test_shuffle_attention_cat_sums(hip, s):
    B, H, W, C, G = 2, 6, 7, 64, 8
    HW = H * W
    r = sa_case()
    _, _, Pq, Qq, Mn = sa_coefs(hip, r, B, HW, C, G)
    xv, rv = inp(r.x, s[0], 0), inp(r.rad, s[1], 1)
    buf, cat = outp((B, H, W, 2 * C), s[2], 2)
    call = lambda: hip.sa_cat_sums(xv, ld(xv), Pq, Qq, Mn, rv, ld(rv), cat, ld(cat), B, HW, C)
    if s[1] != "A" or s[2] != "A":
        refused("sa_cat_sums", call, buf)
        return
    mom = call()
    check(cat, r.cat, buf, "sa + cat + shuffle")
    assert torch.equal(cat[..., 1::2].cpu(), r.rad), "the radar lanes of cat are copies"
    close(mom[..., 0], cat.double().reshape(B, HW, 2 * C).sum(1), 1e-6, "channel sums of cat")


# vrnet_cat2_f32 (stream_ops.hip): cat2_vec_kernel iff Ca % 4 == Cb % 4 == 0, ldc % 4 == 0, 16-byte cat and, for each source
# given, ld % 4 == 0 and a 16-byte base; else cat2_kernel (one float per thread; the 3 + 4 row kernel is not reached here).
# Copies: results are exact.
@pytest.mark.parametrize("s", scenarios(3), ids=sid)          # a, b, cat
@pytest.mark.parametrize("case", [(37, 8, 8, False), (37, 8, 8, True), (200, 12, 20, False)], ids=str)      # the shuffle needs Ca == Cb
def test_cat2_both_directions(hip, case, s):
    rows, Ca, Cb, interleave = case
    a, b, g = rnd(rows, Ca, seed=1), rnd(rows, Cb, seed=2), rnd(rows, Ca + Cb, seed=3)
    a0, b0 = rnd(rows, Ca, seed=4), rnd(rows, Cb, seed=5)
    av, bv = inp(a, s[0], 0), inp(b, s[1], 1)
    buf, cat = outp((rows, Ca + Cb), s[2], 2)
    hip.cat2(av, ld(av), Ca, bv, ld(bv), Cb, cat, ld(cat), rows, interleave)
    ref = torch.cat([a, b], 1)
    if interleave:
        ref = ref.view(rows, 2, Ca).transpose(1, 2).reshape(rows, 2 * Ca)
    assert torch.equal(cat.cpu(), ref) and guards_intact(buf, cat), "cat2"
    # the adjoint: a accumulates, b is overwritten; then b alone, accumulating
    gv = inp(g, s[2], 2)
    abuf, ga = outp(a0.cuda(), s[0], 0)
    bbuf, gb = outp((rows, Cb), s[1], 1)
    hip.cat2(ga, ld(ga), Ca, gb, ld(gb), Cb, gv, ld(gv), rows, interleave, dir=1, accumulate_a=1, accumulate_b=0)
    ra, rb = (g[:, 0::2], g[:, 1::2]) if interleave else (g[:, :Ca], g[:, Ca:])
    assert torch.equal(ga.cpu(), a0 + ra) and torch.equal(gb.cpu(), rb), "cat2 adjoint"
    assert guards_intact(abuf, ga) and guards_intact(bbuf, gb), "cat2 adjoint: guard columns changed"
    bbuf, gb = outp(b0.cuda(), s[1], 1)
    hip.cat2(None, Ca, Ca, gb, ld(gb), Cb, gv, ld(gv), rows, interleave, dir=1, accumulate_b=1)
    assert torch.equal(gb.cpu(), b0 + rb) and guards_intact(bbuf, gb), "cat2 adjoint, b alone"


# ------------------------------------------------------------------------------------------------ 9. dense conv, strided input
# vrnet_conv2d_f32 (igemm.hip): a_vec = CK % 4 == 0 && lda % 4 == 0 && 16-byte a; the LDS-DMA kernels (families 2, 6) need
# a_vec && b_vec, so layouts B and C of the input leave them for the register-staged igemm_kernel<.., vec = false> (family 1),
# which loads one float at a time.  precision 1 has no scalar form: "conv2d: the bf16 path needs 16-byte aligned rows ...".
# vrnet_conv2d_wgrad_f32: vec_all (both operands) gates the x6 tiles (family 6) and the 16-byte loads of wgrad_kernel /
# wgrad_dma_kernel; B or C in x or dy -> wgrad_kernel<.., vec = false> (family 1) at precision 0, and precision 2 falls back to
# it.  Layout A must reach the family written beside each case below (read from the dispatch), which is also the family of the
# contiguous call: forward / data gradient -- 2 (LDS-DMA ring, fp32) for maps of <= 8192 rows, 1 (register-staged
# igemm_kernel<.., vec = true>: 16-byte loads along lda) for a larger map with a short contraction, 6 (x6 tiles) at precision 2
# when vr_dma_tile finds >= 256 tiles; weight gradient -- 1 at precision 0, 6 at precision 2 (wgrad_plan: Cin, Cout > 32, one > 64).
# Tolerances: 1e-4 (test_conv_forward_dgrad_wgrad) on the fp32 kernels, 2e-5 (test_x6_conv_against_fp64_aten) where an x6 kernel
# (family 6) ran; the reference is fp64 ATen throughout.
CONV = [
    # case, precision, family of: forward / data gradient, weight gradient (layout A)
    ((2, 12, 10, 64, 128, 1, 1, 0, 1), 0, 2, 1),
    ((2, 32, 32, 64, 96, 3, 2, 1, 1), 0, 2, 1),
    ((2, 12, 10, 64, 128, 1, 1, 0, 1), 2, 2, 6),      # 240 rows: no x6 forward tile, the fp32 ring serves it; the weight gradient has one
    ((4, 64, 64, 128, 96, 1, 1, 0, 1), 2, 6, 6),      # the smallest map of the x6 tests
    ((4, 64, 64, 128, 96, 1, 1, 0, 1), 0, 1, 1),      # 16 384 rows, contraction 128 / 96: the register-staged vector kernel
]


@functools.lru_cache(maxsize=None)
def conv_case(case):
    B, H, W, Ci, Co, k, s, p, d = case
    x = rnd(B, Ci, H, W, seed=1).double().requires_grad_(True)
    w = (rnd(Co, Ci, k, k, seed=2) / np.sqrt(Ci * k * k)).double().requires_grad_(True)
    b = rnd(Co, seed=3).double().requires_grad_(True)
    y = F.conv2d(x, w, b, s, p, d)
    g = rnd(*y.shape, seed=4)
    y.backward(g.double())
    return types.SimpleNamespace(x=x.detach().float(), w=w.detach().float(), b=b.detach().float(), g=g, y=y.detach(), dx=x.grad,
                                 dw=w.grad, db=b.grad)


def conv_tol(fam):
    return 2e-5 if fam == 6 else TOL


@pytest.mark.parametrize("kind", "ABC")
@pytest.mark.parametrize("case,precision,want,want_w", CONV, ids=str)
def test_conv_with_a_strided_input(hip, case, precision, want, want_w, kind):
    B, H, W, Ci, Co, k, s, p, d = case
    r = conv_case(case)
    OH, OW = r.y.shape[2:]
    geo = (B, H, W, Ci, OH, OW, Co, k, k, s, p, d)
    xg, gg, wp, bg = nhwc(r.x), nhwc(r.g), pack(hip, r.w), r.b.cuda()
    y = torch.full((B, OH, OW, Co), NAN, device="cuda")
    dx = torch.full((B, H, W, Ci), NAN, device="cuda")
    hip.conv2d(xg, Ci, wp, bg, y, Co, *geo, precision=precision)          # the contiguous calls: for their kernel families only
    fam_f = hip.last_kernel()
    hip.conv2d(gg, Co, wp, None, dx, Ci, *geo, mode=1, precision=precision)
    fam_d = hip.last_kernel()
    assert (fam_f, fam_d) == (want, want), (fam_f, fam_d)
    xv, gv = inp(xg, kind, 0), inp(gg, kind, 1)
    y.fill_(NAN)
    hip.conv2d(xv, ld(xv), wp, bg, y, Co, *geo, precision=precision)
    fam = hip.last_kernel()
    assert fam == (want if kind == "A" else 1), fam
    close(nchw(y), r.y, conv_tol(fam), what=f"fwd, family {fam}")
    dx.fill_(NAN)
    hip.conv2d(gv, ld(gv), wp, None, dx, Ci, *geo, mode=1, precision=precision)
    fam = hip.last_kernel()
    assert fam == (want if kind == "A" else 1), fam
    close(nchw(dx), r.dx, conv_tol(fam), what=f"dgrad, family {fam}")


@pytest.mark.parametrize("s", scenarios(2), ids=sid)          # x, dy
@pytest.mark.parametrize("case,precision,want,want_w", CONV, ids=str)
def test_conv_wgrad_with_strided_operands(hip, case, precision, want, want_w, s):
    B, H, W, Ci, Co, k, st, p, d = case
    r = conv_case(case)
    OH, OW = r.y.shape[2:]
    geo = (B, H, W, Ci, OH, OW, Co, k, k, st, p, d)
    xg, gg = nhwc(r.x), nhwc(r.g)
    dw, db = torch.full((Co, Ci, k, k), NAN, device="cuda"), torch.full((Co,), NAN, device="cuda")
    hip.conv2d_wgrad(xg, Ci, gg, Co, dw, db, None, *geo, precision=precision)          # contiguous: for the kernel family only
    assert hip.last_kernel() == want_w, hip.last_kernel()
    xv, gv = inp(xg, s[0], 0), inp(gg, s[1], 1)
    dw.fill_(NAN)
    db.fill_(NAN)
    hip.conv2d_wgrad(xv, ld(xv), gv, ld(gv), dw, db, None, *geo, precision=precision)
    fam = hip.last_kernel()
    assert fam == (want_w if s == ("A", "A") else 1), fam
    close(dw, r.dw, conv_tol(fam), what=f"wgrad, family {fam}")
    close(db, r.db, conv_tol(fam), what=f"bgrad, family {fam}")
    rs = rnd(Co, seed=5)
    hip.conv2d_wgrad(xv, ld(xv), gv, ld(gv), dw, db, rs.cuda(), *geo, accumulate=1, precision=precision)
    close(dw, r.dw * (1 + rs.double()[:, None, None, None]), conv_tol(fam), what="wgrad, accumulate + row scale")
    close(db, r.db * (1 + rs.double()), conv_tol(fam), what="bgrad, accumulate + row scale")


@pytest.mark.parametrize("kind", "ABC")
def test_conv_bf16_operands_with_a_strided_input(hip, kind):
    """precision 1 (family 3), first case of test_conv_bf16_operands, its reference (the conv of the bf16-rounded tensors) and
    its tolerance.  The bf16 kernels stage 16-byte rows only: layouts B and C are refused."""
    B, H, W, Ci, Co, k, s, p, d = 2, 16, 16, 64, 96, 1, 1, 0, 1
    x, w = rnd(B, Ci, H, W, seed=1), rnd(Co, Ci, k, k, seed=2) * (1.0 / (Ci * k * k) ** 0.5)
    bias, g, ks = rnd(Co, seed=3), rnd(B, Co, H, W, seed=4), rnd(Co, seed=5) * 0.3 + 1
    rb = lambda t: t.bfloat16().double()
    xr = rb(x).requires_grad_(True)
    yref = F.conv2d(rb(x), rb(w), bias.double(), s, p, d)
    F.conv2d(xr, rb(w * ks.view(-1, 1, 1, 1)), None, s, p, d).backward(rb(g))
    geo = (B, H, W, Ci, H, W, Co, k, k, s, p, d)
    wt = torch.empty(k * k, Ci, Co, device="cuda")
    hip.pack_weight_t(w.contiguous().cuda(), ks.cuda(), wt, Co, Ci, k, k)
    xv, gv = inp(nhwc(x), kind, 0), inp(nhwc(g), kind, 1)
    assert hip.bf16_conv_ok(ld(xv), Ci, Co, 0) == hip.bf16_conv_ok(ld(gv), Ci, Co, 1) == (kind != "C")
    ybuf, y = outp((B, H, W, Co), "A", 2)
    dbuf, dx = outp((B, H, W, Ci), "A", 3)
    fwd = lambda: hip.conv2d(xv, ld(xv), pack(hip, w), bias.cuda(), y, ld(y), *geo, mode=0, precision=1)
    bwd = lambda: hip.conv2d(gv, ld(gv), wt, None, dx, ld(dx), *geo, mode=1, precision=1)
    if kind != "A":
        refused("conv2d: the bf16 path", fwd, ybuf)
        refused("conv2d: the bf16 path", bwd, dbuf)
        return
    fwd()
    assert hip.last_kernel() == 3
    check(y, yref.permute(0, 2, 3, 1), ybuf, "bf16 conv fwd", 2e-5)
    bwd()
    assert hip.last_kernel() == 3
    check(dx, xr.grad.permute(0, 2, 3, 1), dbuf, "bf16 conv dgrad", 2e-5)
