"""The dense (MFMA) weight gradient, vrnet_conv2d_wgrad_f32 past its tiny / narrow early exits, at every edge of its plan: the 12
wgrad_kernel, 2 wgrad_dma_kernel and 12 wgrad_x6_kernel instantiations and the bf16 kernel of igemm_bf16.hip, each on the row
split of wgrad_plan (S, rows_per_split, a ragged last split, the 48 MB slab cap, the XCD-grouped launch order) and followed by
one of the reductions (wgrad_reduce_kernel<VEC, SL>, wgrad_reduce_rows_kernel<SL>, wgrad_rowdot_kernel).

Which variant a case reaches is not taken on trust.  The tests without a gpu mark restate wgrad_plan, the launcher's kernel
choice, xcd_group, the reduce choice and vrnet_conv2d_wgrad_workspace in Python and require, for every case, precision and
argument form, that the restatement equals the library's own host-side answer (hip.conv2d_wgrad_plan, the query the launcher
itself dispatches on, and vrnet_conv2d_wgrad_workspace); the union over the table must be the complete list of variants.  The
GPU tests assert hip.last_kernel() from the same plan.

The call goes past the wrapper's cached arena: a workspace of exactly vrnet_conv2d_wgrad_workspace bytes, poisoned, followed by
a 4 KB guard pattern.  The first poison is NaN -- a slab element read before it was written shows in an output -- the second a
finite number, and both runs must give the same bits (the summation order is fixed).  One byte less is refused.

Forms per case: (a) dw, db and row_scale into NaN-filled outputs, twice; (b) dw alone, accumulated onto old values; (c) 1 x 1
convs: the layer-scale gradient dls with w and bias, plain and accumulated -- which is what selects wgrad_reduce_rows_kernel or
wgrad_rowdot_kernel.  Two kinds of operands, as in tests/test_direct_conv.py, whose helpers this file imports:

  exact    integers (x, dy in {-2..2}; row scale, w, bias, old values in {-3..3}): every partial sum is an integer below 2^24
           (test_exact_cases_stay_below_2_24, from conv(|x|, |dy|), the row scale, the old values and the dls dot), small
           integers are exact in bf16 -- the x6 split has zero middle and low planes, the bf16-rounded kernels round nothing --
           so at all three precisions every output must equal the fp64 result bit for bit.  dls too: fp32 quad dots of
           integers, fp64 sums, one conversion.
  rounded  rnd(...) operands redrawn until the fp64 reference is well conditioned (COND_LIMIT; no case needs a redraw).
           Precisions 0 and 1: bound = 4 * max(d32, ULP_FLOOR) in the metric of dist(), d32 = fp32 CPU ATen against fp64 ATen
           on the same operands (precision 1: both on the operands rounded with .bfloat16(), db from the unrounded dy).
           Precision 2, element by element: that bound times max |ref| plus 2^-20 * A[e], A = the same gradient of |x| and
           |dy| -- 2^-20 |ab| per product is the bias csrc/x6.h derives for the plane products the scheme drops.  dls is held to
           what these bounds allow dw_raw and db_raw, propagated through the dot, plus the dot's own rounding (dls_allowance),
           and to the suite's TOL.

           Measured on an MI355X (the tests print every figure), over the 39 cases (16 have an x6 kernel, 22 a kernel at
           precision 1): d32 1.4e-7 .. 2.2e-6, bounds 3.8e-6 .. 8.6e-6; the kernels' largest distance per case 1.6e-7 .. 9.8e-7
           at precision 0 (at most 0.26 of the case's bound), 9.8e-8 .. 6.1e-7 at precision 1 (0.13), 2.7e-7 .. 9.2e-7 at
           precision 2, where the largest share of its element's bound that any element of any case used is 0.144 (the
           840-channel case); dls used at most 0.017 of its allowance."""
import functools
import types

import numpy as np
import pytest
import torch

from tests.test_direct_conv import COND_LIMIT, EXACT_LIMIT, MAX_DRAWS, ULP_FLOOR, agree, aten, cdiv, conditioning, dist, out_hw
from tests.test_hip_ops import TOL, nhwc, rnd
from tests.test_strided_rows import NAN, PAT

gpu = pytest.mark.gpu
U = 2.0 ** -24

@pytest.fixture(scope="module")
def hip():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    import asy_vrnet_amd.hip as h
    return h


@pytest.fixture(scope="module")
def lib():
    """The library for the host-only queries: it loads without a GPU (tests/test_abi_surface.py)."""
    try:
        import asy_vrnet_amd.hip as h
    except ImportError:                    # not built yet
        import __graft_entry__ as g
        g.build()
        import asy_vrnet_amd.hip as h
    return h


# ================================================================================================ the launcher's integer rules
Plan = types.SimpleNamespace
SLAB_CAP = 48 << 20


def wgrad_plan(M, Cin, Cout, T, bf16=0, cap=SLAB_CAP):
    """igemm.hip: wgrad_plan -> cfg, bn, nt, ct, S, rows (None: bf16 == 2 and no x6 kernel for the shape).  cap: the bytes of
    slabs allowed (the 48 MB of the source; a larger value shows what the plan wanted)."""
    wsz = T * Cout * Cin
    sbytes = cap // (wsz * 4)
    if bf16 == 2:
        if Cout <= 32 or Cin <= 32:
            return None
        tn, tc = (2 if Cout > 64 else 1), (2 if Cin > 64 else 1)
        if tn == 1 and tc == 1:
            return None
        nt, ct = cdiv(Cout, 64 * tn), cdiv(Cin, 64 * tc)
        tiles = nt * ct * T
        s, smax = cdiv(768, tiles), cdiv(M, 256)
        if tiles <= 96:
            g = max(8 * (32 // tiles), 8)
            while g > 8 and (g > smax or g > sbytes):
                g -= 8
            if g <= smax and g <= sbytes:
                s = g
        s = max(min(s, smax, sbytes), 1)
        r = cdiv(cdiv(M, s), 16) * 16
        return Plan(cfg=10 * tn + tc, bn=64 * tc, nt=nt, ct=ct, S=cdiv(M, r), rows=r)

    def splits(tiles):
        smax = max(cdiv(M, 512), min(cdiv(M, 128), 64))
        return max(min(cdiv(1024, tiles), smax, sbytes), 1)

    bn128 = 128 if Cin > 64 else 64 if Cin > 32 else 32
    tiles128 = cdiv(Cout, 128) * cdiv(Cin, bn128) * T
    small_ok = Cin > 32 and Cout > 32
    if bf16 or (tiles128 < 64 and small_ok):
        nt, ct = cdiv(Cout, 64), cdiv(Cin, 64)
        q = 64 if bf16 else 32
        r = cdiv(cdiv(M, splits(nt * ct * T)), q) * q
        return Plan(cfg=1 if small_ok else 0, bn=64, nt=nt, ct=ct, S=cdiv(M, r), rows=r)
    r = cdiv(cdiv(M, splits(tiles128)), 16) * 16
    return Plan(cfg=0, bn=bn128, nt=cdiv(Cout, 128), ct=cdiv(Cin, bn128), S=cdiv(M, r), rows=r)


def wgrad_choose(M, Cin, Cout, T, vec, precision, cap=SLAB_CAP):
    """igemm.hip: wgrad_choose (the kernel choice of vrnet_conv2d_wgrad_f32) -> kind, tile, S, rows, xcd_group, tiles, and
    the precision the kernel runs at; None: precision 1 is refused.  kind: 0 wgrad_kernel, 1 wgrad_dma_kernel, 2
    wgrad_x6_kernel, 3 the bf16 kernel."""
    x6 = wgrad_plan(M, Cin, Cout, T, 2, cap) if precision in (1, 2) and vec else None
    if x6 is None and precision == 2:
        precision = 0
    p = x6 or wgrad_plan(M, Cin, Cout, T, 1 if precision == 1 else 0, cap)
    c = Plan(S=p.S, rows=p.rows, tiles=p.nt * p.ct * T, xcd_group=0, precision=precision)
    if x6:
        c.kind, c.tile = 2, x6.cfg
        c.xcd_group = 1 if x6.S % 8 == 0 and c.tiles * (x6.S // 8) <= 96 else 0          # the launcher's xcd_group
    elif precision == 1:
        if not (vec and p.cfg == 1 and p.rows % 64 == 0):
            return None
        c.kind, c.tile = 3, 64064
    elif p.cfg == 1 and vec and c.tiles <= 4:
        c.kind, c.tile = 1, 64064
    else:
        c.kind, c.tile = 0, 64064 if p.cfg == 1 else {128: 128128, 64: 128064, 32: 128032}[p.bn]
    return c


def reduce_choose(S, T, Cout, Cin, has_bias, has_dls):
    """igemm.hip: wgrad_reduce_choose (the choice of vr_wgrad_reduce_launch; dw and w 16-byte aligned) -> (kind, VEC, SL):
    kind 0 wgrad_reduce_kernel, 1 wgrad_reduce_rows_kernel."""
    rvec = Cin % 4 == 0
    if has_dls and T == 1 and rvec:
        sl = 1
        while sl < 16 and sl * 2 * (Cin // 4) <= 256:
            sl *= 2
        return 1, 4, sl
    total = T * Cout * Cin // (4 if rvec else 1) + (Cout if has_bias else 0)
    return 0, 4 if rvec else 1, 1 if total >= 65536 or S <= 2 else 4 if total >= 16384 or S <= 8 else 16


def workspace(geo):
    """igemm.hip: vrnet_conv2d_wgrad_workspace (pair = 0).  No case of this file is a tiny (Cin, Cout <= 8) or narrow
    (Cout <= 16) shape, whose kernels have workspace rules of their own."""
    B, H, W, Ci, Co, k, s, p, d = geo
    assert not (Ci <= 8 and Co <= 8) and Co > 16
    M, T = rows_of(geo), k * k
    plans = [wgrad_plan(M, Ci, Co, T, 0), wgrad_plan(M, Ci, Co, T, 1), wgrad_plan(M, Ci, Co, T, 2)]
    return max((q.S * T * Co * Ci + q.S * Co) * 4 + 256 for q in plans if q) + (Co * Ci + Co) * 4


def rows_of(geo):
    OH, OW = out_hw(geo)
    return geo[0] * OH * OW


def is_ident(geo):
    return geo[5:8] == (1, 1, 0)


def is_vec(geo):
    return geo[3] % 4 == 0 and geo[4] % 4 == 0          # contiguous operands: ldx = Cin, lddy = Cout, aligned bases


def choice(geo, precision, cap=SLAB_CAP):
    return wgrad_choose(rows_of(geo), geo[3], geo[4], geo[5] ** 2, is_vec(geo), precision, cap)


def forms(geo):
    """(has_bias, has_dls) of the calls a case makes: (a), (b), and (c) for a 1 x 1 conv."""
    return [(True, False), (False, False)] + ([(True, True)] if geo[5] == 1 else [])


def last_split(c, M):
    return M - (c.S - 1) * c.rows


# ================================================================================================ the cases
# (B, H, W, Cin, Cout, k, stride, pad, dil); the comment: the fp32 plan | the x6 or bf16 plan
CASES = [
    (1, 9, 7, 36, 44, 1, 1, 0, 1),        # dma<ident>, S1, rows 64, last split 63 rows (a 32-row stage of 31) | bf16 kernel S1, 63 of 64
    (1, 16, 16, 48, 48, 1, 1, 0, 1),      # dma<ident>, S2 | bf16 kernel S2
    (1, 9, 9, 40, 40, 1, 2, 0, 1),        # dma<gather>: 1x1 stride 2, 25 rows of 32
    (1, 8, 8, 40, 40, 2, 2, 0, 1),        # dma<gather>: 4 taps = 4 tiles, the last count the ring takes
    (1, 8, 8, 72, 72, 1, 1, 0, 1),        # dma<ident>, 4 tiles | x6 22 ident, S1, 64 rows
    (1, 16, 16, 72, 136, 1, 1, 0, 1),     # mfma 64x64 ident: 6 tiles, the first count off the ring; S2 | x6 22 S1
    (1, 16, 16, 72, 140, 1, 1, 0, 1),     # as above with ragged 64- and 128-wide Cout tiles
    (1, 20, 13, 72, 136, 1, 1, 0, 1),     # S3, rows 96, last 68; reduce (4,4) | x6 S2, rows 144, last 116 (a 16-row stage of 4)
    (1, 50, 41, 72, 136, 1, 1, 0, 1),     # S17, last split 2 rows; reduce (4,16) | x6 S8, rows 272, last 146, xcd 1
    (8, 32, 32, 72, 136, 1, 1, 0, 1),     # S64 = the cap of the small-map rule | x6 S32, xcd 1
    (2, 8, 8, 40, 40, 3, 1, 1, 1),        # mfma 64x64 gather,vec
    (1, 16, 16, 40, 40, 3, 1, 18, 18),    # only the centre tap reaches the image: eight taps' slabs must be written as zeros
    (1, 8, 8, 37, 41, 1, 1, 0, 1),        # mfma 64x64 scalar; reduce (1,1); dls -> rowdot
    (2, 16, 16, 37, 41, 1, 1, 0, 1),      # S4: reduce (1,4)
    (2, 24, 24, 37, 41, 1, 1, 0, 1),      # S9: reduce (1,16)
    (1, 9, 9, 37, 41, 3, 2, 1, 1),        # scalar gather, stride 2, 25 rows
    (1, 8, 8, 100, 24, 3, 1, 1, 1),       # mfma 128x128 gather (Cout <= 32)
    (1, 8, 8, 101, 22, 3, 1, 1, 1),       # mfma 128x128 scalar
    (1, 8, 8, 392, 136, 3, 1, 1, 1),      # mfma 128x128 because the 128-wide tiling has 72 >= 64 tiles | x6 22 gather, 72 tiles, S1
    (1, 8, 8, 48, 24, 3, 1, 1, 1),        # mfma 128x64 gather
    (1, 8, 8, 48, 20, 1, 1, 0, 1),        # mfma 128x64 ident
    (1, 8, 8, 50, 22, 3, 1, 1, 1),        # mfma 128x64 scalar
    (1, 8, 8, 20, 24, 3, 1, 1, 1),        # mfma 128x32 gather
    (1, 8, 8, 24, 100, 1, 1, 0, 1),       # mfma 128x32 ident; dls: rows SL16
    (1, 8, 8, 21, 100, 1, 1, 0, 1),       # mfma 128x32 scalar
    (1, 8, 8, 100, 20, 1, 1, 0, 1),       # dls: rows SL8     (Cout 20: above the narrow kernels' 16)
    (1, 8, 8, 132, 20, 1, 1, 0, 1),       # dls: rows SL4
    (1, 8, 8, 260, 20, 1, 1, 0, 1),       # dls: rows SL2
    (1, 8, 8, 1028, 20, 1, 1, 0, 1),      # dls: rows SL1, 257 quads = two passes
    (2, 32, 32, 72, 136, 1, 1, 0, 1),     # S16, reduce (4,16) | x6 22 ident S8 xcd 1, 2 tiles
    (2, 32, 32, 72, 48, 1, 1, 0, 1),      # dma<ident> S16 | x6 12 ident, xcd 1, 1 tile
    (2, 32, 32, 48, 72, 1, 1, 0, 1),      # dma<ident> S16 | x6 21 ident, xcd 1
    (4, 32, 32, 72, 48, 3, 2, 1, 1),      # x6 12 gather
    (4, 32, 32, 48, 72, 3, 2, 1, 1),      # S8, reduce (4,4) | x6 21 gather, S4, xcd 0
    (2, 32, 32, 72, 136, 3, 1, 1, 1),     # x6 22 gather, 18 tiles, S8, xcd 1
    (2, 16, 16, 392, 264, 3, 1, 1, 1),    # x6 108 > 96 tiles: the workgroup-target branch, S2
    (2, 32, 32, 392, 264, 3, 1, 1, 1),    # fp32 S10, rows 208, last 176 | x6 S8 with 108 tiles: S % 8 == 0 and xcd 0
    (2, 16, 16, 840, 840, 3, 1, 1, 1),    # 25.4 MB of dW: the 48 MB slab cap leaves S1 where the plan wanted 3 (fp32) / 2 (x6)
    (1, 8, 8, 516, 20, 1, 1, 0, 1),       # dls: rows SL1, 129 quads = one pass (beside the two passes of 1028 channels)
]
KINDS = ["exact", "rounded"]
PRECISIONS = [0, 2, 1]
TILES = (64064, 128128, 128064, 128032)


def variants(geo):
    """What the calls of a case reach, as names."""
    M, T, Ci, Co = rows_of(geo), geo[5] ** 2, geo[3], geo[4]
    mode = "scalar" if not is_vec(geo) else "ident" if is_ident(geo) else "gather"
    out = set()
    for prec in PRECISIONS:
        c = choice(geo, prec)
        if c is None:
            continue
        if c.kind == 0:
            out.add(("wgrad_kernel", c.tile, mode))
        elif c.kind == 1:
            out.add(("wgrad_dma_kernel", mode))
        elif c.kind == 2:
            out.add(("wgrad_x6_kernel", c.tile, mode, c.precision))
            if c.xcd_group and c.tiles in (1, 18):
                out.add(("xcd_group 1", c.tiles))
            if not c.xcd_group and c.S % 8 == 0:
                out.add(("xcd_group 0 with S % 8 == 0",))
        else:
            out.add(("bf16 kernel", "S = 1" if c.S == 1 else "S > 1"))
        if c.S == 1 and choice(geo, prec, cap=1 << 40).S > 1:
            out.add(("slab cap", "x6" if c.kind == 2 else "fp32"))
        for has_bias, has_dls in forms(geo):
            kind, vec, sl = reduce_choose(c.S, T, Co, Ci, has_bias, has_dls)
            if kind == 1:
                out.add(("wgrad_reduce_rows_kernel", sl, "two passes" if Ci // 4 > 256 // sl else "one pass"))
            else:
                out.add(("wgrad_reduce_kernel", vec, sl))
                if has_dls:
                    out.add(("wgrad_rowdot_kernel",))
    return out


ALL_VARIANTS = (
    {("wgrad_kernel", t, m) for t in TILES for m in ("ident", "gather", "scalar")} |
    {("wgrad_dma_kernel", m) for m in ("ident", "gather")} |
    {("wgrad_x6_kernel", t, m, p) for t in (22, 21, 12) for m in ("ident", "gather") for p in (2, 1)} |
    {("bf16 kernel", "S = 1"), ("bf16 kernel", "S > 1")} |
    {("wgrad_reduce_kernel", v, sl) for v in (4, 1) for sl in (1, 4, 16)} |
    {("wgrad_reduce_rows_kernel", sl, "one pass") for sl in (16, 8, 4, 2, 1)} | {("wgrad_reduce_rows_kernel", 1, "two passes")} |
    {("wgrad_rowdot_kernel",), ("xcd_group 1", 1), ("xcd_group 1", 18), ("xcd_group 0 with S % 8 == 0",), ("slab cap", "fp32"),
     ("slab cap", "x6")})


# ================================================================================================ operands and references
def bf(t):
    return t.bfloat16().float()


def build(geo, kind):
    """kind: "exact", "exact1" ({-1, 0, 1}: a case whose sums would pass 2^24) or "rounded".  dw, db: the fp64 gradients before
    the row scale; A_dw, A_db: the same of |x| and |dy|; dw1: the fp64 weight gradient of the operands rounded to bf16."""
    B, H, W, Ci, Co, k, s, p, d = geo
    OH, OW = out_hw(geo)
    shapes = dict(x=(B, Ci, H, W), w=(Co, Ci, k, k), b=(Co,), g=(B, Co, OH, OW), dw0=(Co, Ci, k, k), db0=(Co,), rs=(Co,),
                  dls0=(Co,))
    D = types.SimpleNamespace(kind=kind, geo=geo)
    if kind != "rounded":
        rng = np.random.default_rng(list(geo))
        for name, sh in shapes.items():
            m = 1 if kind == "exact1" else 2 if name in ("x", "g") else 3
            setattr(D, name, torch.from_numpy(rng.integers(-m, m + 1, sh).astype(np.float32)))
        D.y, D.dx, D.dw, D.db = aten(D.x, D.w, D.b, D.g, geo, torch.float64)
    for D.draw in range(MAX_DRAWS if kind == "rounded" else 0):          # the first draw whose reference is well conditioned
        for i, (name, sh) in enumerate(shapes.items()):
            setattr(D, name, rnd(*sh, seed=100 * D.draw + i + 1))
        D.w = (D.w / np.sqrt(Ci * k * k)).float()
        D.y, D.dx, D.dw, D.db = aten(D.x, D.w, D.b, D.g, geo, torch.float64)
        D.cond = conditioning(D)
        if D.cond <= COND_LIMIT:
            break
    a = lambda t: t.double().abs()
    D.A_dw, D.A_db = aten(a(D.x), a(D.w), a(D.b), a(D.g), geo, torch.float64)[2:]
    D.dw1 = D.dw
    D.at = {}
    if kind == "rounded":
        D.dw1 = aten(bf(D.x), D.w, D.b, bf(D.g), geo, torch.float64)[2]
        d32 = {0: max(dist(r32, r) for r32, r in zip(aten(D.x, D.w, D.b, D.g, geo, torch.float32)[2:], (D.dw, D.db)))}
        d32[1] = max(dist(aten(bf(D.x), D.w, D.b, bf(D.g), geo, torch.float32)[2], D.dw1), d32[0])
        d32[2] = d32[0]
        for prec, e in d32.items():          # what agree() reads: the bound of the precision, the largest distance seen
            D.at[prec] = types.SimpleNamespace(kind=kind, geo=geo, d32=e, bound=4 * max(e, ULP_FLOOR), seen=0.0, share=0.0)
    return D


@functools.lru_cache(maxsize=None)
def data(geo, kind):
    D = build(geo, kind)
    if kind == "exact" and abs_bound(D) >= EXACT_LIMIT:
        D = build(geo, "exact1")
    return D


def dls_of(D, dw, db):
    return (D.w.double() * dw).sum((1, 2, 3)) + D.b.double() * db


def abs_bound(D):
    """The largest |partial sum| any order of summation can meet in any output of the case: the raw gradients, the scaled ones on
    top of the old values, and the dot of the layer-scale gradient on top of its old value."""
    a = lambda t: t.double().abs()
    rs = a(D.rs).clamp(min=1.0)
    dls = (a(D.w) * D.A_dw).sum((1, 2, 3)) + a(D.b) * D.A_db + a(D.dls0)
    return max((rs[:, None, None, None] * D.A_dw + a(D.dw0)).max().item(), (rs * D.A_db + a(D.db0)).max().item(), dls.max().item())


# ================================================================================================ tests that need no GPU
def test_restatement_is_the_librarys_plan(lib):
    """Every case, precision and form: the Python restatement == vrnet_conv2d_wgrad_plan, and the workspace size."""
    for geo in CASES:
        B, H, W, Ci, Co, k, s, p, d = geo
        M, T = rows_of(geo), k * k
        OH, OW = out_hw(geo)
        assert workspace(geo) == lib._lib.vrnet_conv2d_wgrad_workspace(B, OH, OW, Ci, Co, k, k, 0), geo
        for prec in PRECISIONS:
            c = choice(geo, prec)
            for has_bias, has_dls in forms(geo):
                args = (M, Ci, Co, T, is_ident(geo), is_vec(geo), prec, has_bias, has_dls)
                if c is None:
                    with pytest.raises(RuntimeError, match="bf16 path"):
                        lib.conv2d_wgrad_plan(*args)
                    continue
                want = (c.kind, c.tile, c.S, c.rows, c.xcd_group) + reduce_choose(c.S, T, Co, Ci, has_bias, has_dls)
                assert lib.conv2d_wgrad_plan(*args) == want, (geo, prec, has_bias, has_dls)


def test_plan_query_refuses_what_the_launcher_refuses(lib):
    with pytest.raises(RuntimeError, match="precision 0"):
        lib.conv2d_wgrad_plan(64, 72, 72, 1, True, True, 3)
    with pytest.raises(RuntimeError, match="bf16 path"):
        lib.conv2d_wgrad_plan(64, 72, 72, 1, True, False, 1)          # rows that are not 16-byte rows
    with pytest.raises(RuntimeError, match="bad arguments"):
        lib.conv2d_wgrad_plan(0, 72, 72, 1, True, True, 0)


def test_cases_reach_the_variants_they_are_named_after():
    assert len(CASES) == len(set(CASES)) == 39
    reached = set().union(*(variants(g) for g in CASES))
    assert reached == ALL_VARIANTS, (sorted(map(str, ALL_VARIANTS - reached)), sorted(map(str, reached - ALL_VARIANTS)))


def test_split_edges_of_the_case_table():
    """The comments of CASES, asserted: (kind, tile, S, rows per split, rows of the last split) and what else a comment names."""
    def plan(geo, prec):
        c = choice(geo, prec)
        return c.kind, c.tile, c.S, c.rows, last_split(c, rows_of(geo))

    red = lambda geo, prec, form: reduce_choose(choice(geo, prec).S, geo[5] ** 2, geo[4], geo[3], *form)
    A, Bf, C = (True, False), (False, False), (True, True)
    g = iter(CASES)
    geo = next(g); assert plan(geo, 0) == (1, 64064, 1, 64, 63) and 63 % 32 == 31 and plan(geo, 1) == (3, 64064, 1, 64, 63)
    geo = next(g); assert plan(geo, 0) == (1, 64064, 2, 128, 128) and plan(geo, 1) == (3, 64064, 2, 128, 128)
    geo = next(g); assert plan(geo, 0) == (1, 64064, 1, 32, 25) and not is_ident(geo)
    geo = next(g); assert plan(geo, 0)[:2] == (1, 64064) and choice(geo, 0).tiles == 4 and rows_of(geo) == 16
    geo = next(g); assert plan(geo, 0)[:2] == (1, 64064) and choice(geo, 0).tiles == 4 and plan(geo, 2) == (2, 22, 1, 64, 64)
    geo = next(g); assert plan(geo, 0)[:3] == (0, 64064, 2) and choice(geo, 0).tiles == 6 and plan(geo, 2)[:3] == (2, 22, 1)
    geo = next(g); assert plan(geo, 0)[:3] == (0, 64064, 2) and geo[4] % 64 == 12 and plan(geo, 2)[:3] == (2, 22, 1)
    geo = next(g); assert plan(geo, 0) == (0, 64064, 3, 96, 68) and red(geo, 0, A) == (0, 4, 4)
    assert plan(geo, 2) == (2, 22, 2, 144, 116) and 116 % 16 == 4
    geo = next(g); assert plan(geo, 0)[2:] == (17, 128, 2) and red(geo, 0, A) == (0, 4, 16)
    assert plan(geo, 2) == (2, 22, 8, 272, 146) and choice(geo, 2).xcd_group == 1
    geo = next(g); assert plan(geo, 0)[2] == 64 == min(cdiv(rows_of(geo), 128), 64) and plan(geo, 2)[2] == 32 and choice(geo, 2).xcd_group == 1
    geo = next(g); assert plan(geo, 0)[:2] == (0, 64064) and is_vec(geo) and not is_ident(geo)
    geo = next(g); assert plan(geo, 0)[:2] == (0, 64064) and geo[7] == geo[8] == 18 > geo[1]          # a tap 18 rows away is outside
    geo = next(g); assert plan(geo, 0)[:2] == (0, 64064) and not is_vec(geo) and red(geo, 0, A) == (0, 1, 1) == red(geo, 0, C)
    geo = next(g); assert plan(geo, 0)[2] == 4 and red(geo, 0, A) == (0, 1, 4)
    geo = next(g); assert plan(geo, 0)[2] == 9 and red(geo, 0, A) == (0, 1, 16)
    geo = next(g); assert plan(geo, 0)[:2] == (0, 64064) and not is_vec(geo) and rows_of(geo) == 25
    geo = next(g); assert plan(geo, 0)[:2] == (0, 128128) and is_vec(geo)
    geo = next(g); assert plan(geo, 0)[:2] == (0, 128128) and not is_vec(geo)
    geo = next(g); assert plan(geo, 0)[:2] == (0, 128128) and choice(geo, 0).tiles == 72 and plan(geo, 2)[:3] == (2, 22, 1) and choice(geo, 2).tiles == 72
    geo = next(g); assert plan(geo, 0)[:2] == (0, 128064) and is_vec(geo) and not is_ident(geo)
    geo = next(g); assert plan(geo, 0)[:2] == (0, 128064) and is_vec(geo) and is_ident(geo)
    geo = next(g); assert plan(geo, 0)[:2] == (0, 128064) and not is_vec(geo)
    geo = next(g); assert plan(geo, 0)[:2] == (0, 128032) and is_vec(geo) and not is_ident(geo)
    geo = next(g); assert plan(geo, 0)[:2] == (0, 128032) and is_vec(geo) and is_ident(geo) and red(geo, 0, C) == (1, 4, 16)
    geo = next(g); assert plan(geo, 0)[:2] == (0, 128032) and not is_vec(geo)
    for sl in (8, 4, 2, 1):
        geo = next(g); assert red(geo, 0, C) == (1, 4, sl) and geo[4] == 20 > 16
    assert geo[3] // 4 == 257 > 256
    geo = next(g); assert plan(geo, 0)[2] == 16 and red(geo, 0, A) == (0, 4, 16) and plan(geo, 2)[:3] == (2, 22, 8)
    assert choice(geo, 2).xcd_group == 1 and choice(geo, 2).tiles == 2
    geo = next(g); assert plan(geo, 0)[:3] == (1, 64064, 16) and plan(geo, 2)[:2] == (2, 12) and choice(geo, 2).xcd_group == 1 and choice(geo, 2).tiles == 1
    geo = next(g); assert plan(geo, 0)[:3] == (1, 64064, 16) and plan(geo, 2)[:2] == (2, 21) and choice(geo, 2).xcd_group == 1
    geo = next(g); assert plan(geo, 2)[:2] == (2, 12) and not is_ident(geo)
    geo = next(g); assert plan(geo, 0)[2] == 8 and red(geo, 0, A) == (0, 4, 4) and plan(geo, 2)[:3] == (2, 21, 4) and choice(geo, 2).xcd_group == 0
    geo = next(g); assert plan(geo, 2)[:3] == (2, 22, 8) and choice(geo, 2).tiles == 18 and choice(geo, 2).xcd_group == 1
    geo = next(g); assert choice(geo, 2).tiles == 108 > 96 and plan(geo, 2)[:3] == (2, 22, 2)
    geo = next(g); assert plan(geo, 0)[2:] == (10, 208, 176) and plan(geo, 2)[2] == 8 and choice(geo, 2).tiles == 108 and choice(geo, 2).xcd_group == 0
    geo = next(g); assert plan(geo, 0)[2] == 1 == plan(geo, 2)[2] and choice(geo, 0, 1 << 40).S == 3 and choice(geo, 2, 1 << 40).S == 2
    assert 25e6 < geo[3] * geo[4] * 9 * 4 < 26e6
    geo = next(g); assert red(geo, 0, C) == (1, 4, 1) and 128 < geo[3] // 4 <= 256
    assert next(g, None) is None


def test_exact_cases_stay_below_2_24():
    for geo in CASES:
        D = data(geo, "exact")
        assert abs_bound(D) < EXACT_LIMIT, (geo, D.kind)


def test_rounded_bounds_stay_below_the_suite_tolerance():
    for geo in CASES:
        D = data(geo, "rounded")
        assert D.cond <= COND_LIMIT, (geo, D.cond)          # a draw was found
        for prec in (0, 1):
            assert ULP_FLOOR * 4 <= D.at[prec].bound <= TOL, (geo, prec, D.at[prec].d32)


# ================================================================================================ running a case on the GPU
GUARD = 1024          # ints of PAT behind the workspace: 4 KB
FINITE = 12345.0      # the second poison


def launch(hip, D, prec, dw, db=None, rs=None, accumulate=0, w=None, bias=None, dls=None, poison=NAN, short=0):
    """vrnet_conv2d_wgrad_f32 on a workspace of exactly the required bytes (minus `short`), poisoned, with a guard behind it."""
    B, H, W, Ci, Co, k, s, p, d = D.geo
    OH, OW = out_hw(D.geo)
    need = hip._lib.vrnet_conv2d_wgrad_workspace(B, OH, OW, Ci, Co, k, k, 0)
    assert need % 4 == 0
    ws = torch.full((need // 4 + GUARD,), poison, device="cuda")
    ws.view(torch.int32)[need // 4:] = PAT
    assert ws.data_ptr() % 16 == 0
    ptr = hip.ptr
    hip._check(hip._lib.vrnet_conv2d_wgrad_f32(ptr(D.xg), Ci, ptr(D.gg), Co, ptr(dw), ptr(db), ptr(rs), B, H, W, Ci, OH, OW, Co, k, k,
                                               s, p, d, accumulate, prec, None, None, None, ptr(w), ptr(bias), ptr(dls), None,
                                               None, None, ptr(ws), need - short, hip.stream()), "conv2d_wgrad")
    assert bool((ws.view(torch.int32)[need // 4:] == PAT).all()), f"{D.geo}: the guard behind the workspace changed"


def family(c):
    return 1 if c.precision == 0 else 6 if c.precision == 2 else 3


def held(D, prec, got, ref, what, allow=None):
    """No NaN; then bit for bit (exact), within the precision's bound in the metric of dist() (rounded, precisions 0 and 1), or
    within `allow` element by element (rounded: precision 2 and dls)."""
    assert not bool(torch.isnan(got).any()), f"{what} {D.geo}: NaN in the result -- a slab element read before it was written"
    if D.kind != "rounded" or allow is None:
        return agree(D if D.kind != "rounded" else D.at[prec], got, ref, f"{what} p{prec}")
    R = D.at[prec]
    err = (got.detach().double().cpu() - ref).abs()
    share = (err / allow).max().item()
    print(f"  {D.geo} {what} p{prec}: {dist(got, ref):.2e}, {share:.3f} of its bound")
    R.seen, R.share = max(R.seen, dist(got, ref)), max(R.share, share)
    assert share <= 1.0, f"{what} {D.geo} p{prec}: {share:.3f} of the element's bound, distance {dist(got, ref):.3e}"


def x6_allowance(D, ref, A):
    """Precision 2, per element: the fp32 bound times max |ref| plus 2^-20 A (csrc/x6.h: the bias of the dropped plane products)."""
    return D.at[2].bound * ref.abs().max().item() + 2.0 ** -20 * A


def dls_allowance(D, prec, dw, db, ref):
    """What the case's bounds allow dw_raw and db_raw (E_dw, E_db), through dls[n] = sum_c w dw_raw + b db_raw, plus the dot
    itself -- fp32 dots of four products (4 u of their magnitude), fp64 sums, a conversion and, accumulating, an fp32 sum (2 u of
    the result); never more than TOL in the metric of dist()."""
    a = lambda t: t.double().abs()
    Bd = D.at[prec].bound
    E_dw = Bd * a(dw).max().item() + (2.0 ** -20 * D.A_dw if prec == 2 else 0.0)
    E_db = Bd * a(db).max().item()
    E = (a(D.w) * E_dw).sum((1, 2, 3)) + a(D.b) * E_db + 4 * U * ((a(D.w) * a(dw)).sum((1, 2, 3)) + a(D.b) * a(db)) + 2 * U * a(ref)
    return E.clamp(max=TOL * a(ref).max().item())


def run_case(hip, geo, kind, prec):
    D = data(geo, kind)
    B, H, W, Ci, Co, k, s, p, d = geo
    M, T = rows_of(geo), k * k
    c = choice(geo, prec)
    if not hasattr(D, "xg"):
        D.xg, D.gg = nhwc(D.x), nhwc(D.g)
    nan = lambda *sh: torch.full(sh, NAN, device="cuda")
    if c is None:                          # precision 1 without a kernel for the shape
        dw, db = nan(Co, Ci, k, k), nan(Co)
        with pytest.raises(RuntimeError, match="bf16 path"):
            launch(hip, D, prec, dw, db)
        with pytest.raises(RuntimeError, match="bf16 path"):
            hip.conv2d_wgrad_plan(M, Ci, Co, T, is_ident(geo), is_vec(geo), prec)
        assert bool(torch.isnan(dw).all()) and bool(torch.isnan(db).all()), "a refused call wrote"
        return
    assert hip.conv2d_wgrad_plan(M, Ci, Co, T, is_ident(geo), is_vec(geo), prec)[:5] == (c.kind, c.tile, c.S, c.rows, c.xcd_group)
    if c.precision != prec:
        pytest.skip(f"no tile kernel for this shape: precision {prec} runs the fp32 path, which the precision 0 test holds")
    rounded = kind == "rounded"
    dw_ref, db_ref = (D.dw1 if prec == 1 else D.dw), D.db          # raw
    rs = D.rs.double()
    # (a) dw, db, row_scale into NaN-filled outputs; twice, the second time on another poison: the same bits
    runs = []
    for poison in (NAN, FINITE):
        dw, db = nan(Co, Ci, k, k), nan(Co)
        launch(hip, D, prec, dw, db, D.rs.cuda(), poison=poison)
        assert hip.last_kernel() == family(c), (hip.last_kernel(), family(c))
        runs.append((dw, db))
    ref = rs[:, None, None, None] * dw_ref
    held(D, prec, runs[0][0], ref, "dw, row_scale", x6_allowance(D, ref, rs.abs()[:, None, None, None] * D.A_dw) if rounded and prec == 2 else None)
    held(D, prec, runs[0][1], rs * db_ref, "db, row_scale")
    assert torch.equal(runs[0][0].view(torch.int32), runs[1][0].view(torch.int32)), f"{geo}: two weight gradients differ"
    assert torch.equal(runs[0][1].view(torch.int32), runs[1][1].view(torch.int32)), f"{geo}: two bias gradients differ"
    # (b) dw alone, accumulated onto old values
    dw = D.dw0.cuda()
    launch(hip, D, prec, dw, accumulate=1)
    assert hip.last_kernel() == family(c)
    ref = D.dw0.double() + dw_ref
    held(D, prec, dw, ref, "dw, accumulate", x6_allowance(D, ref, D.A_dw) if rounded and prec == 2 else None)
    # (c) 1 x 1: the layer-scale gradient, plain and accumulated
    if k == 1:
        wg, bg = D.w.cuda(), D.b.cuda()
        dls_ref = dls_of(D, dw_ref, db_ref)
        for acc in (0, 1):
            dw, db, dls = (D.dw0.cuda(), D.db0.cuda(), D.dls0.cuda()) if acc else (nan(Co, Ci, k, k), nan(Co), nan(Co))
            launch(hip, D, prec, dw, db, None, acc, wg, bg, dls)
            assert hip.last_kernel() == family(c)
            what = "dls form, accumulate" if acc else "dls form"
            ref = D.dw0.double() + dw_ref if acc else dw_ref
            held(D, prec, dw, ref, "dw, " + what, x6_allowance(D, ref, D.A_dw) if rounded and prec == 2 else None)
            held(D, prec, db, D.db0.double() + db_ref if acc else db_ref, "db, " + what)
            ref = D.dls0.double() + dls_ref if acc else dls_ref
            held(D, prec, dls, ref, "dls, " + what, dls_allowance(D, prec, dw_ref, db_ref, ref) if rounded else None)
    # one byte less than the required workspace is refused
    dw = nan(Co, Ci, k, k)
    with pytest.raises(RuntimeError, match="conv2d_wgrad: workspace"):
        launch(hip, D, prec, dw, short=1)
    assert bool(torch.isnan(dw).all()), "a refused call wrote"
    if rounded:
        R = D.at[prec]
        print(f"WGRAD-PLAN {geo} p{prec}: draw {D.draw} cond {D.cond:.1f} d32 {R.d32:.2e} bound {R.bound:.2e} kernel {R.seen:.2e} "
              f"share {R.share:.3f}")


@gpu
@pytest.mark.parametrize("prec", PRECISIONS, ids=lambda p: f"p{p}")
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("geo", CASES, ids=str)
def test_wgrad_at_plan_edge(hip, geo, kind, prec):
    run_case(hip, geo, kind, prec)
