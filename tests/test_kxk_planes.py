"""k x k convolutions at precision 2 on pre-split weights: igemm_planes_kernel<1, 3, true> (kernel family 9) behind vrnet_conv2d_f32's
`w_planes`, forward (mode 0) and data gradient (mode 1), and the per-tap pack image it reads.

The pack of a [Cout][Cin][kh][kw] weight is kh * kw images of the 1x1 pack in one buffer, one table entry of
vrnet_conv_planes_pack_f32 per tap (pack_kxk below builds the table as program.py's X6WeightPlanes does); image() restates the
byte layout in torch on the CPU -- [tap][k16 step][64-column block][plane][lane half][column][8], planes split by truncation exactly
as vr_split3 of csrc/x6.h splits a fragment (bit 32 of a table entry's J), or round-to-nearest-even as the 1x1 entries are -- and
test_pack_image_is_the_restated_layout compares the two bit for bit, per mode and split.

Which calls reach the kernel is restated too (eligible(): contraction % 16 == 0, 2 .. 32 taps, vector loaders, not the 128 x 128
tile) and compared with vrnet_conv2d_plan, without a GPU; a call that is not eligible must have the plan it has without planes.
The GPU tests assert hip.last_kernel() from the plan after every call.  A call that reaches the kernel is handed the OIHW tensor
as `w`: the kernel must read the pack alone.

Cases: the smallest shapes at which the gather can still go wrong (CASES, each with its reason), both modes, operands in NaN-guarded
pitched buffers as in tests/test_conv_plan.py, whose operands, references and bounds are used as they are:

  exact    integer operands: every output equals the fp64 result bit for bit (integers have empty middle and low planes).  Forward
           with bias and column statistics (the bn_stats partials) and data gradient with kscale and aux must in addition equal,
           bit for bit, what the same call gives without planes -- partials included -- and the partials the fp64 sums.
  rounded  the precision-2 bound of tests/test_conv_plan.py, element by element.

The split case runs on a workspace of exactly the plan's bytes, NaN-poisoned, guard behind it; with one byte less the plan names
the unsplit launch, which must run and hold.

test_error_is_no_larger_than_the_in_kernel_splits: the kernel that splits both operands itself (igemm_dma_kernel<*, 3, 2, 1, 6>,
family 6) only runs where the tile rule gives it >= 256 tiles, so the comparison is made at the smallest such shape (32 761 rows),
not at the shapes of CASES, where the call without planes is the fp32 ring.  The pack splits a k x k weight into the very planes
that kernel makes of its weight fragments, and both kernels add the same products in the same order, so the result on planes must
equal the in-kernel split's BIT FOR BIT on random operands -- which is what keeps the training step's outputs what they were; the
error against fp64 (root mean square over all outputs, and the maximum; both printed for both kernels) is then no larger because it
is the same (measured on an MI355X: rms 3.169e-7 forward, 4.231e-7 data gradient, both kernels).  Over CASES the largest share of its
element's precision-2 bound that any output used is 0.124."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests.test_conv_plan import NAN, data, dma_tile, gemm_of, held, workspace, ws_guard_intact
from tests.test_direct_conv import cdiv, g12, out_hw
from tests.test_hip_ops import nchw, nhwc, pack, rnd
from tests.test_strided_rows import guards_intact, inp, ld, outp

gpu = pytest.mark.gpu
KINDS = ["exact", "rounded"]

# (B, H, W, Cin, Cout, k, stride, pad, dil)
CASES = [
    ((1, 9, 13, 16, 64, 3, 1, 1, 1), "one K16 step per tap, one ragged row tile"),
    ((3, 9, 13, 48, 72, 3, 1, 1, 1), "row tiles straddle samples, ragged last column tile; dgrad contracts over 72: falls back"),
    ((2, 15, 20, 32, 64, 3, 2, 1, 1), "the reducer form on an odd map"),
    ((1, 8, 8, 32, 64, 3, 1, 6, 6), "whole taps in the padding: k_live"),
    ((1, 8, 8, 512, 64, 3, 1, 1, 1), "fwd: split 8 ways on the plan's exact workspace"),
    ((1, 9, 13, 40, 64, 3, 1, 1, 1), "fwd: Cin = 40 is no multiple of 16: falls back"),
    ((3, 9, 13, 80, 48, 3, 1, 1, 1), "dgrad: ragged last column tile, row tiles straddle samples; fwd contracts over 80"),
    ((2, 16, 16, 64, 64, 3, 2, 1, 1), "dgrad of the reducer form under perm2: parity-major rows, 4 of 9 taps live per tile at most"),
]
GEOS = [g for g, _ in CASES]
BIG = (1, 181, 181, 48, 64, 3, 1, 1, 1)          # 32 761 rows: 256 row tiles, the least the x6 tile rule takes at <= 64 columns


@pytest.fixture(scope="module")
def hip():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    import asy_vrnet_amd.hip as h
    return h


@pytest.fixture(scope="module")
def lib():
    try:
        import asy_vrnet_amd.hip as h
    except ImportError:                    # not built yet
        import __graft_entry__ as g
        g.build()
        import asy_vrnet_amd.hip as h
    return h


# ================================================================================================ the rule and the plan
def eligible(geo, mode):
    """igemm.hip, conv_choose: a k x k call at precision 2 that brings planes runs on igemm_planes_kernel<1, 3, true> (aligned bases and
    row strides % 4 == 0, as every call of this file has them)."""
    B, H, W, Ci, Co, k, s, p, d = geo
    M, MH, MW, SH, SW, CK, CN = gemm_of(geo, mode)
    return CK % 16 == 0 and Ci % 4 == 0 and 1 < k * k <= 32 and dma_tile(M, CN) != 22


def plan(h, geo, mode, form, planes, ws):
    M, MH, MW, SH, SW, CK, CN = gemm_of(geo, mode)
    return h.conv2d_plan(*g12(geo), mode=mode, precision=2, lda=CK + 12, ldy=CN + 16, kscale=form == "c" and mode == 1,
                         plain=form == "a", w_planes=planes, workspace_bytes=ws)


def default_ws(h, geo, mode):
    """What hip.conv2d hands a precision-2 call that is given no workspace of its own."""
    M, MH, MW, SH, SW, CK, CN = gemm_of(geo, mode)
    return h.conv2d_splitk_workspace(M, CN, CK * geo[5] ** 2)


def test_plan_with_planes(lib):
    """Eligible calls: family 9, kernel 4, the 128 x 64 tile, grid and split from the row and column tiles.  All others: the plan
    they have without planes, bit for bit.  Without planes nothing changes by definition of the second rule, asserted anyway."""
    seen = set()
    for geo in GEOS + [BIG]:
        for mode in (0, 1):
            M, MH, MW, SH, SW, CK, CN = gemm_of(geo, mode)
            for form in "ac":
                for ws in (0, default_ws(lib, geo, mode), 1 << 40):
                    got, bare = plan(lib, geo, mode, form, True, ws), plan(lib, geo, mode, form, False, ws)
                    seen.add(eligible(geo, mode))
                    if not eligible(geo, mode):
                        assert got == bare and got[0] != 9, (geo, mode, form, ws)
                        continue
                    gt = 8 * cdiv(cdiv(M, 128), 8) * cdiv(CN, 64)
                    S = got[3]
                    assert got[:3] == (9, 4, 21) and got[5:9] == bare[5:9] and got[9:] == (gt * S, 1, gt if S > 1 else 0), (geo, mode, got)
                    assert S == 1 or S * gt * 32768 <= ws
    assert seen == {True, False}
    assert [eligible(g, 0) for g in GEOS] == [True, True, True, True, True, False, True, True]
    assert [eligible(g, 1) for g in GEOS] == [True, False, True, True, True, True, True, True]
    assert eligible(BIG, 0) and eligible(BIG, 1) and plan(lib, BIG, 0, "a", False, 0)[:3] == plan(lib, BIG, 1, "a", False, 0)[:3] == (6, 2, 21)
    # more than 32 taps, and the shapes of the 128 x 128 tile, keep the kernel that splits both operands
    assert plan(lib, (1, 14, 14, 16, 64, 6, 2, 2, 1), 0, "a", True, 0) == plan(lib, (1, 14, 14, 16, 64, 6, 2, 2, 1), 0, "a", False, 0)
    g22 = (1, 256, 256, 16, 128, 3, 1, 1, 1)
    assert dma_tile(256 * 256, 128) == 22 and plan(lib, g22, 0, "a", True, 0) == plan(lib, g22, 0, "a", False, 0) and plan(lib, g22, 0, "a", True, 0)[:3] == (6, 2, 22)


# ================================================================================================ the pack
def chop(v):
    """The top 16 bits of fp32 values as bf16."""
    return (v.contiguous().view(torch.int32) & -65536).view(torch.float32).bfloat16()


def split3(v, trunc=False):
    """Planes of fp32 values, v = p0 + p1 + p2 exactly (csrc/igemm.hip, planes_pack_kernel): round-to-nearest-even, or by truncation
    as vr_split3 of csrc/x6.h."""
    top = chop if trunc else (lambda t: t.bfloat16())
    p0 = top(v)
    r1 = v - p0.float()
    p1 = top(r1)
    p2 = top(r1 - p1.float())
    return p0, p1, p2


def test_split3_is_exact():
    v = torch.cat([rnd(4096, seed=3), rnd(4096, seed=4) * 1e-3, torch.tensor([1.0 + 2.0 ** -8, 1.0 + 3 * 2.0 ** -8, 0.0, -7.0])])
    for trunc in (False, True):
        p0, p1, p2 = split3(v, trunc)
        assert torch.equal(p0.float() + p1.float() + p2.float(), v) and torch.equal((p0.float() + p1.float()) + p2.float(), v)
        assert float(p1.float().abs().max()) > 0 and float(p2.float().abs().max()) > 0
        # truncated planes all carry the value's sign; rounded ones do not
        assert bool((p1.float() * v >= 0).all()) == trunc


def image(w, mode, ks=None, trunc=True):
    """The pack of an OIHW weight as int16 bf16 bit patterns, restated: mode 0 columns j = Cout, contraction k = Cin; mode 1 columns
    Cin, contraction Cout with ks[Cout] folded in (one fp32 product, then the split); [tap][k / 16][j / 64, padded to whole 128-column
    tiles][plane][(k % 16) / 8][j % 64][k % 8], zeros (times the scale) in the padding."""
    Co, Ci, kh, kw = w.shape
    T = kh * kw
    m = w.reshape(Co, Ci, T).permute(2, 0, 1)          # [t][Cout][Cin]
    if mode == 1:
        m = m.transpose(1, 2)                           # [t][j = Cin][k = Cout]
    J, K = m.shape[1:]
    JB = 2 * cdiv(J, 128)
    padded = torch.zeros(T, JB * 64, K)
    padded[:, :J] = m
    if mode == 1 and ks is not None:
        padded = padded * ks[None, None, :]             # the padding too: a zero under a negative scale is -0 in plane 0
    planes = torch.stack(split3(padded, trunc), 0)                                   # [plane][t][j][k]
    v = planes.reshape(3, T, JB, 64, K // 16, 2, 8)                            # [plane][t][jb][col][kb][hh][i]
    return v.permute(1, 4, 2, 0, 5, 3, 6).contiguous().view(torch.int16).reshape(-1)


def pack_kxk(hip, w, mode, ks=None, trunc=True):
    """One table entry per tap: source w + t, destination + t images, 2^32 in the J field for the truncating split
    (include/vrnet_hip.h)."""
    Co, Ci, kh, kw = w.shape
    T = kh * kw
    J, K, sj, sk = (Co, Ci, Ci * T, T) if mode == 0 else (Ci, Co, T, Ci * T)
    per, nb = hip.conv_planes_bytes(J, K), (K // 16) * 2 * cdiv(J, 128)
    assert hip.conv_planes_bytes(J, T * K) == T * per == T * nb * 6144
    buf = torch.empty((T * per,), dtype=torch.uint8, device="cuda")
    rows = []
    for t in range(T):
        rows += [w.data_ptr() + 4 * t, J | trunc << 32, K, sj, sk, 0 if ks is None else ks.data_ptr(), buf.data_ptr() + t * per, t * nb]
    hip.conv_planes_pack(torch.tensor(rows, dtype=torch.int64, device="cuda"), T, T * nb)
    return buf


@gpu
@pytest.mark.parametrize("trunc", [True, False], ids=["trunc", "rne"])
@pytest.mark.parametrize("mode", [0, 1])
def test_pack_image_is_the_restated_layout(hip, mode, trunc):
    w = rnd(80, 48, 3, 3, seed=7)          # 80 / 48 columns: a second block of 16 resp. a first one of 48, zeros up to 128
    w[0, 0, 0, 0], w[1, 0, 0, 0] = 1.0 + 2.0 ** -8, 1.0 + 3 * 2.0 ** -8          # ties: to even, down and up
    # kscale: signed powers of two, one per contraction index -- w * ks is then exact, so the image does not depend on whether the
    # compiler contracts that multiplication into the first subtraction of the split
    ks = torch.sign(rnd(80, seed=8)) * 2.0 ** torch.from_numpy(np.random.default_rng(9).integers(-2, 3, 80).astype(np.float32)) if mode == 1 else None
    got = pack_kxk(hip, w.cuda(), mode, None if ks is None else ks.cuda(), trunc).view(torch.int16).cpu()
    want = image(w, mode, ks, trunc)
    assert got.shape == want.shape
    bad = got != want
    assert not bool(bad.any()), f"{int(bad.sum())} of {want.numel()} bf16 values differ, first at {int(bad.nonzero()[0])}"


# ================================================================================================ the calls
def operands(hip, D):
    if "woihw" not in D.dev:
        D.dev.update({("a", 0): inp(nhwc(D.x), "A", 0), ("a", 1): inp(nhwc(D.g), "A", 0), "w": pack(hip, D.w), "woihw": D.w.contiguous().cuda(),
                      ("bias", 0): D.b.cuda(), ("bias", 1): D.b1.cuda(), "rs": D.rs.cuda(), "ks": D.ks.cuda()})
    return D.dev


def call(hip, D, mode, form, planes, ws=None, colstats=False, aux=None):
    """Forms of tests/test_conv_plan.py: (a) bias; (c) forward res + res_scale, act = 1 and ypre, data gradient kscale.
    ws: bytes of an exact NaN-poisoned workspace (None: the wrapper's own).  -> ({name: NCHW result}, column partials or None)."""
    geo = D.geo
    B, H, W, Ci, Co, k, s, p, d = geo
    M, MH, MW, SH, SW, CK, CN = gemm_of(geo, mode)
    dv = operands(hip, D)
    want = plan(hip, geo, mode, form, planes, default_ws(hip, geo, mode) if ws is None else ws)
    assert (want[0] == 9) == (planes and eligible(geo, mode)), (geo, mode, form, planes, want)
    ks = dv["ks"] if (form == "c" and mode == 1) else None
    kw = dict(mode=mode, precision=2)
    if planes:          # (a contraction that is no multiple of 16 has no pack: the call falls back and must not read what it is handed)
        kw["w_planes"] = pack_kxk(hip, dv["woihw"], mode, ks) if CK % 16 == 0 else torch.zeros(16, dtype=torch.uint8, device="cuda")
    wbuf, ws4 = None, 0
    if ws is not None:          # exactly ws bytes of a NaN-poisoned buffer, the guard pattern behind it
        ws4 = cdiv(ws, 4) * 4
        wbuf, full = workspace(ws4, NAN)
        kw["workspace"] = full[:ws]
    if colstats:
        part = torch.full((cdiv(M, 32), CN, 2), NAN, dtype=torch.float64, device="cuda")
        kw["colstats"] = (part, None, 0, None, None)
    if aux is not None:
        kw.update(aux=aux, ldaux=ld(aux))
    a = dv["a", mode]
    oshape = (B, MH, MW, CN)
    buf, y = outp(oshape, "A", 1)
    outs = {}
    if form == "c" and mode == 0:
        pbuf, ypre = outp(oshape, "A", 2)
        res = inp(nhwc(D.res), "A", 3)
        kw.update(act=1, ypre=ypre, ldypre=ld(ypre), res=res, ldres=ld(res), res_scale=dv["rs"])
    if form == "c" and mode == 1:
        kw.update(kscale=ks)
    bias = None if (form == "c" and mode == 1) else dv["bias", mode]
    # a call that reaches the planes kernel gets the OIHW tensor: nothing but the pack may be read
    hip.conv2d(a, ld(a), dv["woihw"] if want[0] == 9 else dv["w"], bias, y, ld(y), *g12(geo), **kw)
    assert hip.last_kernel() == want[0], (geo, mode, form, planes, hip.last_kernel(), want)
    assert guards_intact(buf, y), f"{geo} ({form}): guard columns of the output changed"
    assert wbuf is None or ws_guard_intact(wbuf, ws4), f"{geo}: the guard behind the workspace changed"
    outs["y"] = nchw(y)
    if form == "c" and mode == 0:
        assert guards_intact(pbuf, ypre), f"{geo} (c): guard columns of ypre changed"
        outs["ypre"] = nchw(ypre)
    return outs, (kw["colstats"][0].cpu() if colstats else None)


def same_bits(a, b):
    return torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


@gpu
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("geo", GEOS, ids=str)
def test_kxk_conv_on_planes(hip, geo, kind):
    D = data(geo, kind)
    for mode in (0, 1):
        M, MH, MW, SH, SW, CK, CN = gemm_of(geo, mode)
        for form in "ac":
            what = f"mode {mode} ({form}, planes)"
            outs, _ = call(hip, D, mode, form, True)
            for name, got in outs.items():
                held(D, 2, (mode, form, name), got, f"{what} {name}")
            if kind == "rounded":          # for the record: the same call without planes (here the fp32 ring or igemm_kernel)
                bare, _ = call(hip, D, mode, form, False)
                ref = D.ref[2][mode, form, "y"]
                e = lambda t: float((t.double() - ref).pow(2).mean().sqrt())
                print(f"  {geo} {what}: rms error {e(outs['y']):.3e}, without planes (family {hip.last_kernel()}) {e(bare['y']):.3e}")
        if kind != "exact" or not eligible(geo, mode):
            continue
        if mode == 0 and CN > 32:
            # forward with bias and the bn_stats column partials: the bits of the call without planes, and the fp64 sums
            (o1, p1), (o0, p0) = call(hip, D, 0, "a", True, colstats=True), call(hip, D, 0, "a", False, colstats=True)
            assert same_bits(o1["y"], o0["y"]) and torch.equal(p1.view(torch.int64), p0.view(torch.int64)), f"{geo}: column partials differ"
            v = D.ref[2][0, "a", "y"].permute(0, 2, 3, 1).reshape(M, CN)
            v = torch.cat([v, torch.zeros(cdiv(M, 32) * 32 - M, CN, dtype=v.dtype)]).reshape(-1, 32, CN)
            assert torch.equal(p1[..., 0], v.sum(1)) and torch.equal(p1[..., 1], (v * v).sum(1)), f"{geo}: column partials are not the sums"
        if mode == 1:
            aux = inp(rnd(geo[0], MH, MW, CN, seed=31).cuda(), "A", 4)
            (o1, _), (o0, _) = call(hip, D, 1, "c", True, aux=aux), call(hip, D, 1, "c", False, aux=aux)
            assert not bool(torch.isnan(o1["y"]).any()) and same_bits(o1["y"], o0["y"]), f"{geo}: kscale + aux differs from the call without planes"


@gpu
@pytest.mark.parametrize("kind", KINDS)
def test_split_on_the_exact_workspace(hip, kind):
    geo = GEOS[4]
    D = data(geo, kind)
    M, MH, MW, SH, SW, CK, CN = gemm_of(geo, 0)
    S, fin = plan(hip, geo, 0, "a", True, 1 << 40)[3], plan(hip, geo, 0, "a", True, 1 << 40)[11]
    need = S * fin * 32768
    assert S == 8 and fin == 8 and plan(hip, geo, 0, "a", True, need)[3] == S
    for form in "ac":
        outs, _ = call(hip, D, 0, form, True, ws=need)
        for name, got in outs.items():
            held(D, 2, (0, form, name), got, f"split {S} ({form}) {name}")
    # one byte less: the plan names the unsplit launch of the same kernel
    short = plan(hip, geo, 0, "a", True, need - 1)
    assert short[:4] == (9, 4, 21, 1) and short[11] == 0
    outs, _ = call(hip, D, 0, "a", True, ws=need - 1)
    held(D, 2, (0, "a", "y"), outs["y"], "short workspace")
    # the data gradient of the case contracts over 64 x 9: too short to split
    assert plan(hip, geo, 1, "a", True, 1 << 40)[3] == 1


@gpu
def test_error_is_no_larger_than_the_in_kernel_splits(hip):
    geo = BIG
    B, H, W, Ci, Co, k, s, p, d = geo
    OH, OW = out_hw(geo)
    x, g = rnd(B, Ci, H, W, seed=41), rnd(B, Co, OH, OW, seed=42)
    w = (rnd(Co, Ci, k, k, seed=43) / np.sqrt(Ci * k * k)).float()
    ref = {0: F.conv2d(x.double(), w.double(), None, s, p, d),
           1: torch.nn.grad.conv2d_input((B, Ci, H, W), w.double(), g.double(), s, p, d)}
    wo, wp = w.contiguous().cuda(), pack(hip, w)
    for mode in (0, 1):
        M, MH, MW, SH, SW, CK, CN = gemm_of(geo, mode)
        a = inp(nhwc(x if mode == 0 else g), "A", 0)
        err, out = {}, {}
        for planes in (True, False):
            buf, y = outp((B, MH, MW, CN), "A", 1)
            kw = dict(w_planes=pack_kxk(hip, wo, mode)) if planes else {}
            hip.conv2d(a, ld(a), wo if planes else wp, None, y, ld(y), *g12(geo), mode=mode, precision=2, **kw)
            assert hip.last_kernel() == (9 if planes else 6) and guards_intact(buf, y)
            out[planes] = nchw(y)
            e = out[planes].double() - ref[mode]
            assert not bool(torch.isnan(e).any())
            err[planes] = (float(e.pow(2).mean().sqrt()), float(e.abs().max()))
        print(f"KXK-PLANES {geo} mode {mode}: rms error {err[True][0]:.4e} on planes, {err[False][0]:.4e} split in the kernel; "
              f"max {err[True][1]:.3e}, {err[False][1]:.3e}")
        assert err[True][0] <= err[False][0], (mode, err)
        assert same_bits(out[True], out[False]), f"mode {mode}: {int((out[True] != out[False]).sum())} outputs differ from the in-kernel split's"


# shapes of the training step where the kernel that splits both operands runs (family 6), no fp64 reference needed
SAME_BITS = [
    ((2, 128, 128, 48, 64, 3, 2, 1, 1), 1, "data gradient of the reducer form under perm2, 256 row tiles"),
    ((8, 16, 16, 512, 512, 3, 1, 6, 6), 0, "the dilated ASPP form: split contraction, row tiles with different live taps"),
    ((8, 16, 16, 512, 512, 3, 1, 6, 6), 1, "its data gradient"),
]


@gpu
@pytest.mark.parametrize("geo,mode,why", SAME_BITS, ids=lambda v: str(v) if not isinstance(v, str) else "")
def test_same_bits_as_the_in_kernel_split(hip, geo, mode, why):
    """Random operands, bias, the wrapper's own split workspace: with planes family 9, without family 6, the same bits."""
    B, H, W, Ci, Co, k, s, p, d = geo
    OH, OW = out_hw(geo)
    M, MH, MW, SH, SW, CK, CN = gemm_of(geo, mode)
    w = (rnd(Co, Ci, k, k, seed=53) / np.sqrt(Ci * k * k)).float()
    a = inp(nhwc(rnd(B, Ci, H, W, seed=51) if mode == 0 else rnd(B, Co, OH, OW, seed=52)), "A", 0)
    bias = rnd(CN, seed=54).cuda()
    wo, wp = w.contiguous().cuda(), pack(hip, w)
    out = {}
    for planes in (True, False):
        buf, y = outp((B, MH, MW, CN), "A", 1)
        kw = dict(w_planes=pack_kxk(hip, wo, mode)) if planes else {}
        hip.conv2d(a, ld(a), wo if planes else wp, bias, y, ld(y), *g12(geo), mode=mode, precision=2, **kw)
        assert hip.last_kernel() == (9 if planes else 6), (geo, mode, planes, hip.last_kernel())
        assert guards_intact(buf, y)
        out[planes] = y.clone()
    assert not bool(torch.isnan(out[True]).any())
    assert same_bits(out[True], out[False]), f"{geo} mode {mode}: {int((out[True] != out[False]).sum())} of {out[True].numel()} outputs differ"
