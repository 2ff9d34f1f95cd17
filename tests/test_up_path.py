"""The neck's up-path as one gather (csrc/spatial.hip, round 7): vrnet_bn_relu_upsample_cat_f32 against the launches it replaces,
its statistics against a moments pass over the stored tensor, the adjoint that reads the concatenation's gradient in place, the
re-indexed gathers of the family against their own expression, and the program with model.fused_up_cat on and off.

Shapes are the smallest at which the index maps (rows that are no multiple of the chunk, one-row maps, scale 4), the chunk
meeting (several chunks per sample) and the channel maps (both orders, shuffle, unequal halves, strides) can go wrong."""
import pytest
import torch
import torch.nn.functional as F

from tests.test_hip_ops import close, nchw, nhwc, rnd

pytestmark = pytest.mark.gpu

B = 2
SPATIAL = [(3, 5, 2), (4, 4, 4), (1, 7, 2)]                     # H, W, scale
# C, Cs, interleave, up_first: the shuffle with the interpolated half first and second; unequal halves, the skip map first
CHANNELS = [(8, 8, True, True), (8, 8, True, False), (8, 12, False, False)]


@pytest.fixture(scope="module")
def hip():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    import asy_vrnet_amd.hip as h
    return h


def strided(t, ld):
    """The (.., C) tensor t as a view of rows `ld` floats apart (the padding holds NaN: nobody may read it)."""
    buf = torch.full(t.shape[:-1] + (ld,), float("nan"), device=t.device)
    buf[..., :t.shape[-1]] = t
    return buf[..., :t.shape[-1]]


def inputs(H, W, s, C, Cs, ldz=None, lds=None, batch=B, seed=0):
    z = rnd(batch, H, W, C, seed=seed + 1).cuda()
    skip = rnd(batch, H * s, W * s, Cs, seed=seed + 2).cuda()
    A, D, S = rnd(C, seed=seed + 3).cuda(), rnd(C, seed=seed + 4).cuda(), rnd(C, seed=seed + 5).cuda()
    if ldz:
        z = strided(z, ldz)
    if lds:
        skip = strided(skip, lds)
    return z, skip, (A, D, S)


def two_launches(hip, z, skip, coef, H, W, s, C, Cs, il, up_first, batch=B):
    """hip.bn_relu_upsample (hip.upsample without coefficients) + hip.cat2: what the fused kernel replaces."""
    hi = torch.empty(batch, H * s, W * s, C, device="cuda")
    if coef is None:
        hip.upsample(z, z.stride(2), hi, C, batch, H, W, C, s)
    else:
        hip.bn_relu_upsample(z, z.stride(2), *coef, hi, C, batch, H, W, C, s)
    cat = torch.empty(batch, H * s, W * s, C + Cs, device="cuda")
    rows = batch * H * s * W * s
    if up_first:
        hip.cat2(hi, C, C, skip, skip.stride(2), Cs, cat, C + Cs, rows, il)
    else:
        hip.cat2(skip, skip.stride(2), Cs, hi, C, C, cat, C + Cs, rows, il)
    return cat


def fused(hip, z, skip, coef, H, W, s, C, Cs, il, up_first, stats=0, batch=B):
    cat = torch.full((batch, H * s, W * s, C + Cs), float("nan"), device="cuda")
    A, D, S = coef if coef is not None else (None, None, None)
    res = hip.bn_relu_upsample_cat(z, z.stride(2), A, D, S, skip, skip.stride(2), cat, C + Cs, batch, H, W, C, Cs, s, up_first, il,
                                   stats)
    return cat, res


# ------------------------------------------------------------------------------------------------ tensor bits
@pytest.mark.parametrize("C,Cs,il,up_first", CHANNELS)
@pytest.mark.parametrize("H,W,s", SPATIAL)
def test_cat_has_the_bits_of_upsample_then_cat2(hip, H, W, s, C, Cs, il, up_first):
    z, skip, coef = inputs(H, W, s, C, Cs)
    cat, _ = fused(hip, z, skip, coef, H, W, s, C, Cs, il, up_first)
    assert torch.equal(cat, two_launches(hip, z, skip, coef, H, W, s, C, Cs, il, up_first))


@pytest.mark.parametrize("C,Cs,il,up_first", CHANNELS)
def test_cat_from_strided_inputs(hip, C, Cs, il, up_first):
    H, W, s = 3, 5, 2
    z, skip, coef = inputs(H, W, s, C, Cs, ldz=C + 4, lds=Cs + 8)
    assert z.stride(2) == C + 4 and skip.stride(2) == Cs + 8
    cat, _ = fused(hip, z, skip, coef, H, W, s, C, Cs, il, up_first)
    assert torch.equal(cat, two_launches(hip, z, skip, coef, H, W, s, C, Cs, il, up_first))


@pytest.mark.parametrize("C,Cs,il,up_first", CHANNELS)
def test_cat_without_batchnorm_coefficients(hip, C, Cs, il, up_first):
    H, W, s = 4, 4, 4
    z, skip, _ = inputs(H, W, s, C, Cs)
    cat, _ = fused(hip, z, skip, None, H, W, s, C, Cs, il, up_first)
    assert torch.equal(cat, two_launches(hip, z, skip, None, H, W, s, C, Cs, il, up_first))


# ------------------------------------------------------------------------------------------------ statistics
@pytest.mark.parametrize("C,Cs,il,up_first", CHANNELS)
@pytest.mark.parametrize("H,W,s,batch", [(h, w, s, B) for h, w, s in SPATIAL] + [(16, 16, 4, 1)])      # the last: several chunks
def test_statistics_of_the_written_tensor(hip, H, W, s, batch, C, Cs, il, up_first):
    z, skip, coef = inputs(H, W, s, C, Cs, batch=batch)
    Ct, HW = C + Cs, H * s * W * s
    if batch == 1:
        assert hip._lib.vrnet_up_cat_pairs(batch, HW, Ct) > 1
    cat, mom = fused(hip, z, skip, coef, H, W, s, C, Cs, il, up_first, stats=hip.UP_CAT_SA_SUMS, batch=batch)
    cat2_, (pairs, per) = fused(hip, z, skip, coef, H, W, s, C, Cs, il, up_first, stats=hip.UP_CAT_GN_PAIRS, batch=batch)
    assert torch.equal(cat, cat2_)
    v = cat.double().reshape(batch, HW, Ct)
    # sa_sums: the kernel follows moments_plan and the moments kernel's order, so equality with hip.moments is expected and
    # asserted; against the fp64 torch sum, the bound of two fp64 summation orders
    ref = hip.moments(cat, Ct, batch, HW, Ct)
    assert torch.equal(mom, ref)
    for k, terms in enumerate((v, v * v)):
        lim = HW * 2.0 ** -52 * terms.abs().sum(1)
        d = (mom[..., k] - ref[..., k]).abs()
        print("sa_sums", k, "max |delta|", d.max().item(), "bound", lim.min().item())
        assert (d <= lim).all()
        assert ((mom[..., k] - terms.sum(1)).abs() <= lim).all()
    # gn_pairs: per-sample totals against an fp64 torch sum of the stored tensor
    assert pairs.shape == (batch, per, 2)
    tot = pairs.sum(1)
    for k, terms in enumerate((v, v * v)):
        lim = HW * Ct * 2.0 ** -52 * terms.abs().sum((1, 2))
        d = (tot[:, k] - terms.sum((1, 2))).abs()
        print("gn_pairs", k, "max |delta|", d.max().item(), "bound", lim.min().item())
        assert (d <= lim).all()


# ------------------------------------------------------------------------------------------------ fallback
def test_widths_the_kernel_does_not_take_run_the_old_launches(hip):
    """C = 6 is no multiple of 4: the library refuses it (no quiet scalar path), the predicate says so and program.up_cat runs
    bn_relu_upsample + cat2 as before -- with the same result whichever way model.fused_up_cat is set."""
    import asy_vrnet_amd as A
    import asy_vrnet_amd.modules as M
    import asy_vrnet_amd.program as program
    H, W, s, C, Cs = 3, 5, 2, 6, 6
    z, skip, coef = inputs(H, W, s, C, Cs)
    assert not hip.up_cat_ok(C, Cs, C, Cs, C + Cs, True, z, skip)
    with pytest.raises(RuntimeError, match="bn_relu_upsample_cat"):
        fused(hip, z, skip, coef, H, W, s, C, Cs, True, True)
    dev = torch.device("cuda", torch.cuda.current_device())
    outs = []
    for cout, flag in ((6, True), (6, False), (8, True), (8, False)):
        mod = M.CoCUpsample(8, cout, s)
        A.randomize_state_dict(mod.state_dict(), seed=3)
        mod = mod.cuda().train()
        rt = program.RT(dev, True, True)
        rt.fused_up_cat = flag
        x = program.Act(rnd(B, H, W, 8, seed=7).cuda())
        sk = program.Act(rnd(B, H * s, W * s, cout, seed=8).cuda())
        ran = []
        orig = hip.bn_relu_upsample_cat
        hip.bn_relu_upsample_cat = lambda *a, **k: (ran.append(1), orig(*a, **k))[1]
        try:
            cat, res = program.up_cat(rt, x, mod, sk, True, True, hip.UP_CAT_SA_SUMS)
        finally:
            hip.bn_relu_upsample_cat = orig
        assert bool(ran) == (flag and cout == 8) and (res is not None) == bool(ran)
        g = rnd(*cat.t.shape, seed=9).cuda()
        rt.give_grad(cat, g)
        program.backward_begin(rt, (None, None, None), None)
        program.backward_range(rt, 0, len(rt.tape))
        program.backward_cut(rt)
        torch.cuda.synchronize()
        outs.append([cat.t, x.grad, sk.grad] + [rt.pgrads[p] for p in mod.parameters() if p in rt.pgrads])
    # C = 8: the fused level has the bits of the unfused one, gradients too
    assert len(outs[2]) == len(outs[3]) and all(torch.equal(u, v) for u, v in zip(outs[2], outs[3]))
    # C = 6: both runs took the old launches; their concatenation against hip.cat2 called directly on CoCUpsample's output
    mod = M.CoCUpsample(8, 6, s)
    A.randomize_state_dict(mod.state_dict(), seed=3)
    rt = program.RT(dev, True, False)
    up = program.coc_upsample(rt, program.Act(rnd(B, H, W, 8, seed=7).cuda()), mod.cuda().train())
    want = torch.empty(B, H * s, W * s, 12, device="cuda")
    hip.cat2(up.t, 6, 6, rnd(B, H * s, W * s, 6, seed=8).cuda(), 6, 6, want, 12, B * H * s * W * s, True)
    assert torch.equal(outs[0][0], want) and torch.equal(outs[1][0], want)


# ------------------------------------------------------------------------------------------------ adjoint in place
@pytest.mark.parametrize("accumulate", [0, 1])
@pytest.mark.parametrize("C,Cs,il,up_first", CHANNELS + [(8, 12, False, True)])
@pytest.mark.parametrize("H,W,s", [(3, 5, 2), (4, 4, 4)])
def test_adjoint_reads_the_concatenation_gradient_in_place(hip, H, W, s, C, Cs, il, up_first, accumulate):
    Ct, rows = C + Cs, B * H * s * W * s
    g = rnd(B, H * s, W * s, Ct, seed=11).cuda()
    # the parent's form: cat2's adjoint writes both halves, upsample_bwd gathers from the copied half
    dhi = torch.empty(B, H * s, W * s, C, device="cuda")
    dsk0 = rnd(B, H * s, W * s, Cs, seed=12).cuda()
    dsk = dsk0.clone()
    if up_first:
        hip.cat2(dhi, C, C, dsk, Cs, Cs, g, Ct, rows, il, dir=1, accumulate_b=accumulate)
    else:
        hip.cat2(dsk, Cs, Cs, dhi, C, C, g, Ct, rows, il, dir=1, accumulate_a=accumulate)
    dlo = torch.empty(B, H, W, C, device="cuda")
    hip.upsample_bwd(dhi, C, 0, dlo, C, B, H, W, C, s)
    # in place
    coff, cs = ((0 if up_first else 1), 2) if il else ((0 if up_first else Cs), 1)
    dlo2 = torch.full((B, H, W, C), float("nan"), device="cuda")
    hip.upsample_bwd_cat(g, Ct, coff, cs, dlo2, C, B, H, W, C, s)
    assert torch.equal(dlo2, dlo)
    dsk2 = dsk0.clone()
    if up_first:
        hip.cat2(None, C, C, dsk2, Cs, Cs, g, Ct, rows, il, dir=1, accumulate_b=accumulate)
    else:
        hip.cat2(dsk2, Cs, Cs, None, C, C, g, Ct, rows, il, dir=1, accumulate_a=accumulate)
    assert torch.equal(dsk2, dsk)
    if accumulate:
        assert not torch.equal(dsk, dsk0)
        dlo3 = dlo2.clone()
        hip.upsample_bwd_cat(g, Ct, coff, cs, dlo3, C, B, H, W, C, s, accumulate=1)
        assert torch.equal(dlo3, dlo2 + dlo2)


# ------------------------------------------------------------------------------------------------ the re-indexed gathers
@pytest.mark.parametrize("H,W,s,C", [(4, 4, 4, 9), (2, 3, 4, 9), (4, 4, 4, 8)])      # W = 3: OW = 12, a multiple of 4
def test_nchw_gather_agrees_with_the_other_layouts(hip, H, W, s, C):
    """The 16-byte NCHW kernel (shared taps from scale 2 on), the 16-byte NHWC kernel (C = 8) and the scalar kernel (C = 9,
    NHWC) evaluate one expression: equal bits; and they meet torch's bilinear upsampling to the tolerance of test_hip_ops."""
    x = rnd(B, C, H, W, seed=1)
    y = F.interpolate(x, scale_factor=s, mode="bilinear", align_corners=True)
    xg = nhwc(x)
    OH, OW = H * s, W * s
    assert OW % 4 == 0
    out_nchw = torch.full((B, C, OH, OW), float("nan"), device="cuda")
    hip.upsample(xg, C, out_nchw, 0, B, H, W, C, s, out_nchw=1)
    out_nhwc = torch.full((B, OH, OW, C), float("nan"), device="cuda")
    hip.upsample(xg, C, out_nhwc, C, B, H, W, C, s)
    close(out_nchw.cpu(), y, what="up fwd nchw")
    assert torch.equal(out_nchw, out_nhwc.permute(0, 3, 1, 2))
    A, D, S = rnd(C, seed=3).cuda(), rnd(C, seed=4).cuda(), rnd(C, seed=5).cuda()
    hip.bn_relu_upsample(xg, C, A, D, S, out_nchw, 0, B, H, W, C, s, out_nchw=1)
    hip.bn_relu_upsample(xg, C, A, D, S, out_nhwc, C, B, H, W, C, s)
    assert torch.equal(out_nchw, out_nhwc.permute(0, 3, 1, 2))
    lo = torch.empty(B, H, W, C, device="cuda")
    hip.affine(lo, C, B, H * W, C, x1=xg, ld1=C, A=A, D1=D, S1=S, pre=1)
    hip.upsample(lo, C, out_nhwc, C, B, H, W, C, s)
    assert torch.equal(out_nchw, out_nhwc.permute(0, 3, 1, 2))


def fma32(a, b, c):
    """The correctly rounded fp32 fma(a, b, c) of fp32 tensors: the product is exact in fp64; the fp64 sum is brought to
    round-to-odd with its exact residual (TwoSum), after which the second rounding, to fp32, cannot go wrong."""
    p, c = a.double() * b.double(), c.double() + torch.zeros_like(a.double() * b.double())
    s = p + c
    bb = s - p
    e = (p - (s - bb)) + (c - bb)
    even = (s.view(torch.int64) & 1) == 0
    toward = torch.where(e > 0, torch.full_like(s, float("inf")), torch.full_like(s, float("-inf")))
    s = torch.where((e != 0) & even, torch.nextafter(s, toward), s)
    return s.to(torch.float32)


def adjoint_restated(g, H, W, s, dx0, fused_l):
    """The adjoint kernels' expression (the parent commit's, unchanged), restated on the CPU: g (B, C, OH, OW), dx0 (B, C, H, W).
    For every input pixel, over oy ascending and inside it ox ascending, s = fma(wy * wx, g, s) for the pairs whose weights
    are both non-zero, with wy, wx and their product in fp32; then dx = dx0 + s.  The interpolation weight is
    the single rounding l = fma(ratio, o, -i0) (fused_l).  That form is not in the parent's source, which says
    `r - (float)a`: it was read from the compiler's output for the parent's two adjoint kernels (a fused multiply-add with a
    negated addend) and from the parent's results on the GPU, and is now written out in csrc/spatial.hip; this test cannot
    verify it against the parent, only hold the kernels to it.  (The forward gathers round twice, l = fl(ratio * o) - i0.)"""
    f32 = torch.float32

    def weights(n_in, n_out):
        r = (torch.tensor(float(n_in - 1), dtype=f32) / torch.tensor(float(n_out - 1), dtype=f32)) if n_out > 1 else torch.zeros((), dtype=f32)
        o = torch.arange(n_out)
        pos = r * o.to(f32)
        i0 = pos.to(torch.int64).clamp(max=n_in - 1)
        i1 = i0 + (i0 < n_in - 1)
        l1 = fma32(r.expand(n_out), o.to(f32), -i0.to(f32)) if fused_l else pos - i0.to(f32)
        i = torch.arange(n_in)[None, :]
        z = torch.zeros((), dtype=f32)
        return torch.where(i0[:, None] == i, (1 - l1)[:, None], z) + torch.where(i1[:, None] == i, l1[:, None], z)      # [out][in]
    OH, OW = H * s, W * s
    wy, wx = weights(H, OH), weights(W, OW)
    acc = torch.zeros_like(dx0)
    for oy in range(OH):
        for ox in range(OW):
            w = wy[oy][:, None] * wx[ox][None, :]                                  # (H, W), fp32 product
            live = (wy[oy][:, None] != 0) & (wx[ox][None, :] != 0)
            t = fma32(w.expand_as(acc), g[:, :, oy, ox][:, :, None, None].expand_as(acc), acc)
            acc = torch.where(live, t, acc)
    return dx0 + acc


@pytest.mark.parametrize("kind,C", [("nchw", 9), ("nhwc", 9), ("nhwc", 8)])      # scalar kernel in both layouts, 16-byte kernel
@pytest.mark.parametrize("H,W,s", [(4, 4, 4), (2, 3, 4), (3, 5, 2)])
def test_adjoints_accumulate_in_the_parent_order(hip, kind, C, H, W, s):
    g = rnd(B, C, H * s, W * s, seed=21)
    dx0 = rnd(B, C, H, W, seed=22)
    want = adjoint_restated(g, H, W, s, dx0, fused_l=True)
    dx = nhwc(dx0)
    if kind == "nchw":
        hip.upsample_bwd(g.cuda(), 0, 1, dx, C, B, H, W, C, s, accumulate=1)
    else:
        hip.upsample_bwd(nhwc(g), C, 0, dx, C, B, H, W, C, s, accumulate=1)
    assert torch.equal(nchw(dx), want)
    x = rnd(B, C, H, W, seed=23).requires_grad_(True)
    F.interpolate(x, scale_factor=s, mode="bilinear", align_corners=True).backward(g)
    close(nchw(dx), x.grad + dx0, what="up bwd, accumulate")


# ------------------------------------------------------------------------------------------------ program level
def test_step_with_the_fused_up_path_agrees_and_captures(hip):
    """phi = nano, 64 px, batch 2, one training step with model.fused_up_cat on and off.  The seg branch's tensors and channel
    sums have the bits of the unfused launches; the det branch's GroupNorm takes its statistics as per-workgroup pairs (one
    launch) instead of per-sample coefficients (two), which reassociates a sum: outputs and gradients agree to the
    tolerances tests/test_net_parity.py holds two forms of one program to (test_round5_schedule_and_fused_passes_agree_with_
    the_round4_forms: 2e-5 of the largest output, 2e-3 of a gradient's norm; they are literals inside that test, there is no
    constant to import).  With the flag on, the step captured as a graph equals the eager step bit for bit."""
    import asy_vrnet_amd as A
    from asy_vrnet_amd.graph import GraphedStep
    from tests.test_net_parity import build

    def loss_of(det, seg):
        return sum((d * d).mean() for d in det) + (seg * seg).mean()
    x, r = A.synthetic_inputs(2, 64, 9)
    x, r = x.cuda(), r.cuda()

    def run(flag):
        m = build(A, "nano", 64, 13, True)
        m.fused_up_cat = flag
        det, seg = m(x, r)
        loss = loss_of(det, seg)
        loss.backward()
        torch.cuda.synchronize()
        return [d.detach() for d in det] + [seg.detach()], {k: p.grad for k, p in m.named_parameters() if p.grad is not None}, loss.detach()
    launches = []
    orig = hip.bn_relu_upsample_cat
    hip.bn_relu_upsample_cat = lambda *a, **k: (launches.append(1), orig(*a, **k))[1]
    try:
        new = run(True)
        assert len(launches) == 5, launches          # three seg levels, two det levels
        old = run(False)
        assert len(launches) == 5
    finally:
        hip.bn_relu_upsample_cat = orig
    for a, b in zip(new[0], old[0]):
        err = ((a - b).abs().max() / b.abs().max()).item()
        print("output: rel max", err)
        assert err < 2e-5
    assert new[1].keys() == old[1].keys()
    worst = max(((new[1][k] - old[1][k]).norm() / old[1][k].norm().clamp_min(1e-20)).item() for k in old[1])
    print("gradients: worst rel norm", worst)
    assert worst < 2e-3, worst
    ref = build(A, "nano", 64, 13, True)
    sd0 = {k: v.clone() for k, v in ref.state_dict().items()}
    m = build(A, "nano", 64, 13, True)
    assert getattr(m, "fused_up_cat", True)
    gs = GraphedStep(m, loss_of, 2, 64, x.device, warmup=2)
    m.load_state_dict(sd0)
    loss = gs(x, r)
    torch.cuda.synchronize()
    assert torch.equal(loss, new[2])
    for k, p in m.named_parameters():
        if p.numel() and k in new[1]:
            assert torch.equal(p.grad, new[1][k]), k
