"""The dense forward and data-gradient convolution, vrnet_conv2d_f32 past its tiny / narrow / patch early exits, at every edge of
its dispatch: the 12 igemm_kernel instantiations, the fp32 LDS-DMA ring, the x6 and bf16-rounded tile kernels (tile 22 = 128 x 128,
21 = 128 x 64), the split contraction with its finish kernel, the three kernels on pre-split weights and igemm_bf16_kernel.

Which variant a call reaches is not taken on trust.  The tests without a gpu mark restate conv_choose of igemm.hip in Python
(vr_dma_tile, vr_dma_plan with its workspace cap, the live-tap count k_live, dma_ok, dma_shape, the bf16 rules of precision 1 and 3,
the 128 x 32 / 128 x 64 / 64 x 64 rule, perm2, the *_vec flags, the grids, vrnet_conv2d_splitk_workspace) and require, for every
case, mode, precision and argument form, that the restatement equals the library's own host-side answer (hip.conv2d_plan, the
function the launcher itself dispatches on); the union over the table must be the complete list of variants, with both values
of perm2 and of e_vec wherever a kernel can have both.  Three rules cannot be reached with the default tuning values, and a test
says so for each: the third rule of vr_dma_tile (tile 22 at >= 256 tiles: the second rule always takes those shapes), and
igemm_kernel<128, 64, ..., vec = false> in both modes (the 128 x 64 rule asks for vector loaders).  The GPU tests assert
hip.last_kernel() from the same plan after each call.

Every case runs forward (mode 0) and data gradient (mode 1) at precisions 0, 2, 1 and 3.  The activation operand and the NHWC
output sit in pitched buffers (layout A of tests/test_strided_rows.py): inputs in NaN, outputs in a fixed bit pattern whose
guard columns must keep every bit.  Forms per call: (a) bias into a pattern-filled output, twice with equal bits; (b)
accumulate = 1 onto old values; (c) forward: res + res_scale, act = 1 and ypre -- data gradient: kscale; (d) the scalar
epilogue: out_nchw into a channel range of a wider tensor, the channels beside it untouched; (p) where the case qualifies, (a),
(c) and (d) on pre-split weights (family 9).  Split cases (S > 1) get a workspace of exactly the plan's bytes, poisoned with NaN on
the first run of (a) and with a finite value on the second, with a 4 KB guard behind it; with one byte less the plan names the
unsplit kernel, last_kernel() agrees and the result still holds.  Where precision 2 has neither tile nor split the fp32 path runs,
held to the same checks.

Two kinds of operands, as in tests/test_wgrad_plan.py:

  exact    integers (x, g in {-2..2}; w, bias, scales, old values, residual in {-3..3}): every partial sum is an integer below 2^24
           (test_exact_cases_stay_below_2_24, from conv(|x|, |w|), the bias, the residual, the scales and the old values), small
           integers are exact in bf16 and have empty middle and low x6 planes, so at all four precisions every output must equal
           the fp64 result bit for bit.
  rounded  rnd(...) operands redrawn until the fp64 reference is well conditioned (COND_LIMIT).  Precisions 0, 1, 3: bound =
           4 * max(d32, ULP_FLOOR) in the metric of dist(), d32 = fp32 CPU ATen against fp64 ATen on the same operands (1 and 3:
           both on the operands rounded with .bfloat16(); kscale is then a signed power of two, which commutes with that rounding
           wherever the kernel applies it).  Precision 2, element by element: that bound times max |ref| plus 2^-20 * A[e], A =
           the same convolution of |x| and |w| (times |res_scale| resp. with |kscale| inside) -- 2^-20 |ab| per product is the
           bias csrc/x6.h derives for the plane products the scheme drops.  No bound exceeds the suite's TOL.

           Measured on an MI355X (the tests print every figure), over the 39 cases, none of which needs a redraw: d32 2.2e-7 ..
           1.2e-6, bounds 3.8e-6 .. 4.9e-6; the kernels' largest distance per case 2.3e-7 .. 3.1e-6 at precision 0 (at most 0.81
           of the case's bound: the 4608-long contraction of the 3 x 3, 512 -> 512 case on the fp32 ring), 5.4e-8 .. 1.0e-6 at
           precision 1 (32 cases have a kernel; 0.27), 9.0e-8 .. 3.6e-7 at precision 3 (9 cases; 0.09), 2.3e-7 .. 1.2e-6 at
           precision 2, where the largest share of its element's bound that any element of any case used is 0.160."""
import functools
import types

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests.test_direct_conv import COND_LIMIT, EXACT_LIMIT, MAX_DRAWS, ULP_FLOOR, cdiv, dist, g12, out_hw
from tests.test_hip_ops import TOL, nchw, nhwc, pack, rnd
from tests.test_strided_rows import NAN, PAT, guards_intact, inp, ld, outp, pat

gpu = pytest.mark.gpu
Plan = types.SimpleNamespace
IGEMM, RING, X6, BF16_TILE, PLANES, BF16 = range(6)          # the kernel codes of vrnet_conv2d_plan
PRECISIONS = [0, 2, 1, 3]
KINDS = ["exact", "rounded"]
FORMS, PLANE_FORMS = "abcd", "acd"
BF16_PATH, PREC3 = "the bf16 path needs", "precision 3 .* has no kernel"          # the launcher's refusals


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
MIN_N, MIN_TILES, SPLIT_TARGET, SPLIT_MIN_STEPS = 96, 256, 512, 32          # the default tuning values of igemm.hip


def dma_tile(M, CN, rule=False):
    """igemm.hip: vr_dma_tile -> 22, 21 or 0 (rule: which of its three rules answered, 0 for none)."""
    mt, nt22, nt21 = cdiv(M, 128), cdiv(CN, 128), cdiv(CN, 64)
    waste22 = nt22 * 128 - CN > 16 * nt22
    if CN >= MIN_N and mt * nt22 >= 2 * MIN_TILES and not waste22:
        r = (22, 1)
    elif CN > 32 and mt * nt21 >= MIN_TILES:
        r = (21, 2)
    elif CN >= MIN_N and mt * nt22 >= MIN_TILES:
        r = (22, 3)
    else:
        r = (0, 0)
    return r[1] if rule else r[0]


def dma_plan(M, CN, ktot, ws_bytes):
    """igemm.hip: vr_dma_plan -> (tile, S)."""
    tile = dma_tile(M, CN)
    if tile or CN <= 32 or ws_bytes <= 0:
        return tile, 1
    mt, nt21 = cdiv(M, 128), cdiv(CN, 64)
    tiles, steps = mt * nt21, ktot // 16
    S = min(cdiv(SPLIT_TARGET, tiles), steps // SPLIT_MIN_STEPS, 8)
    if S < 2 or tiles * S < 192 or S * (8 * cdiv(mt, 8) * nt21) * 8192 * 4 > ws_bytes:
        return 0, 1
    return 21, S


def splitk_workspace(M, CN, ktot):
    """igemm.hip: vrnet_conv2d_splitk_workspace."""
    tile, S = dma_plan(M, CN, ktot, 1 << 40)
    return S * (8 * cdiv(cdiv(M, 128), 8) * cdiv(CN, 64)) * 8192 * 4 if tile and S > 1 else 0


def gemm_of(geo, mode):
    """(M, MH, MW, SH, SW, CK, CN) of the GEMM: rows = output pixels (mode 0) or input pixels (mode 1)."""
    B, H, W, Ci, Co, k, s, p, d = geo
    OH, OW = out_hw(geo)
    return (B * OH * OW, OH, OW, H, W, Ci, Co) if mode == 0 else (B * H * W, H, W, OH, OW, Co, Ci)


def tap_live(geo, mode, o, t, n_s):
    """Whether tap t of one axis reaches the source axis of n_s pixels from the GEMM-side coordinate(s) o (src_of in the kernels)."""
    k, s, p, d = geo[5:]
    if mode == 0:
        src = o * s - p + t * d
        return (src >= 0) & (src < n_s)
    tt = o + p - t * d
    return (tt >= 0) & (tt % s == 0) & (tt // s < n_s)


def k_live_of(geo, mode):
    """The launcher's contraction length that counts for the split: CK times the taps that reach the image for at least one row."""
    M, MH, MW, SH, SW, CK, CN = gemm_of(geo, mode)
    k = geo[5]
    if k == 1:
        return CK
    live = lambda n_m, n_s: sum(bool(tap_live(geo, mode, np.arange(n_m), t, n_s).any()) for t in range(k))
    return CK * live(MH, SH) * live(MW, SW)


def perm2_of(geo, mode):
    M, MH, MW = gemm_of(geo, mode)[:3]
    return int(mode == 1 and geo[6] == 2 and MH % 2 == 0 and MW % 2 == 0 and (M // 4) % 128 == 0)


def has_kscale(mode, prec, form):
    """Form (c) of a data gradient passes kscale -- but at precision 1, where the transposed weight pack has it folded in."""
    return form == "c" and mode == 1 and prec != 1


class Refused(Exception):
    pass


def conv_choose(geo, mode, prec, form="a", planes=False, ws=0):
    """igemm.hip: conv_choose for a call of this file -- aligned bases, row strides lda = CK + 12 and ldy = CN + 16 (% 4 as the
    channel counts), form (c) of a data gradient with kscale, form (d) with out_nchw.  -> the twelve values of vrnet_conv2d_plan,
    or Refused(pattern of the launcher's message)."""
    B, H, W, Ci, Co, k, s, p, d = geo
    M, MH, MW, SH, SW, CK, CN = gemm_of(geo, mode)
    kscale, out_nchw = has_kscale(mode, prec, form), form == "d"
    perm2 = perm2_of(geo, mode)
    a_vec, b_vec = int(CK % 4 == 0), int(Ci % 4 == 0)
    e_vec = int(not out_nchw and CN % 4 == 0)
    ktot = CK * k * k
    P = Plan(S=1, k_live=ktot, perm2=perm2, a_vec=a_vec, b_vec=b_vec, e_vec=e_vec, fin=0)
    vec = a_vec and b_vec
    if prec == 1 and not (mode == 0 and vec and CN > 32 and dma_tile(M, CN)):
        if not (a_vec and CN > 32 and not kscale):
            raise Refused(BF16_PATH)
        P.family, P.kernel, P.tile, P.perm2, P.gx, P.gy = 3, BF16, 64064, 0, cdiv(M, 64), cdiv(CN, 64)
        return P
    dma_ok = vec and CN > 32 and (not kscale or CK <= 1024)
    dma_shape = M <= 8192 or (M <= 32768 and ktot >= 1024)
    if prec in (1, 2, 3) and dma_ok:
        P.k_live = k_live_of(geo, mode)
        tile, S = dma_plan(M, CN, P.k_live, ws) if prec == 2 else (dma_tile(M, CN), 1)
        if tile:
            mt, nt = cdiv(M, 128), cdiv(CN, 128 if tile == 22 else 64)
            P.tile, P.S, P.gx, P.gy = tile, S, 8 * cdiv(mt, 8) * nt * S, 1
            P.fin = 8 * cdiv(mt, 8) * nt if S > 1 else 0
            if prec == 2 and planes and (k, s, p) == (1, 1, 0) and CK % 16 == 0:
                P.family, P.kernel = 9, PLANES
            else:
                P.family, P.kernel = (6, X6) if prec == 2 else (3, BF16_TILE)
            return P
    if prec == 3:
        raise Refused(PREC3)
    if dma_ok and dma_shape:
        P.family, P.kernel, P.tile, P.gx, P.gy = 2, RING, 64064, 8 * cdiv(cdiv(M, 64), 8) * cdiv(CN, 64), 1
    elif CN <= 32:
        P.family, P.kernel, P.tile, P.gx, P.gy = 1, IGEMM, 128032, cdiv(M, 128), 1
    elif vec and CN <= 192 and ktot >= 512:
        P.family, P.kernel, P.tile, P.gx, P.gy = 1, IGEMM, 128064, cdiv(M, 128), cdiv(CN, 64)
    else:
        P.family, P.kernel, P.tile, P.gx, P.gy = 1, IGEMM, 64064, cdiv(M, 64), cdiv(CN, 64)
    return P


def choice(geo, mode, prec, form="a", planes=False, ws=0):
    """conv_choose, or None where the call is refused."""
    try:
        return conv_choose(geo, mode, prec, form, planes, ws)
    except Refused:
        return None


def as_tuple(P):
    return (P.family, P.kernel, P.tile, P.S, P.k_live, P.perm2, P.a_vec, P.b_vec, P.e_vec, P.gx, P.gy, P.fin)


def library_plan(h, geo, mode, prec, form="a", planes=False, ws=0):
    M, MH, MW, SH, SW, CK, CN = gemm_of(geo, mode)
    return h.conv2d_plan(*g12(geo), mode=mode, precision=prec, lda=CK + 12, ldy=CN + 16, kscale=has_kscale(mode, prec, form),
                         plain=form != "c" or (mode == 1 and prec == 1), out_nchw=form == "d", w_planes=planes, workspace_bytes=ws)


def ws_of(geo, mode):
    """The bytes the wrapper's own rule gives a precision-2 call: vrnet_conv2d_splitk_workspace on the full contraction."""
    M, MH, MW, SH, SW, CK, CN = gemm_of(geo, mode)
    return splitk_workspace(M, CN, CK * geo[5] ** 2)


def planes_ok(geo, mode):
    """Whether the case runs on pre-split weights at precision 2: 1 x 1, contraction a multiple of 16, a tile."""
    c = choice(geo, mode, 2, "a", True, ws_of(geo, mode))
    return c is not None and c.kernel == PLANES


def row_pixels(geo, mode):
    """(y, x) of every GEMM row in the kernels' order (igemm_row_to_pixel: parity-major under perm2)."""
    M, MH, MW = gemm_of(geo, mode)[:3]
    m = np.arange(M)
    if not perm2_of(geo, mode):
        return (m // MW) % MH, m % MW
    per, Hh, Wh = M // 4, MH // 2, MW // 2
    ph, r = m // per, m % per
    return 2 * ((r // Wh) % Hh) + (ph >> 1), 2 * (r % Wh) + (ph & 1)


def tile_taps(geo, mode, BM):
    """Taps that reach the image from at least one row, for every tile of BM GEMM rows."""
    M, MH, MW, SH, SW = gemm_of(geo, mode)[:5]
    k = geo[5]
    y, x = row_pixels(geo, mode)
    ly = np.stack([tap_live(geo, mode, y, t, SH) for t in range(k)])          # (k, M)
    lx = np.stack([tap_live(geo, mode, x, t, SW) for t in range(k)])
    live = (ly[:, None, :] & lx[None, :, :]).reshape(k * k, M)
    pad = cdiv(M, BM) * BM - M
    live = np.concatenate([live, np.zeros((k * k, pad), dtype=bool)], 1).reshape(k * k, -1, BM).any(2)
    return live.sum(0)


def kernel_taps(geo, mode, BM):
    """Taps a workgroup walks: the block-uniform list of its live taps where 1 < k * k <= 32, every tap otherwise."""
    n, kk = tile_taps(geo, mode, BM), geo[5] ** 2
    return n if 1 < kk <= 32 else np.full_like(n, kk)


def split_ranges(geo, mode, S):
    """(first step, steps) of every (row tile, split) of a split launch: steps [split, split + 1) * n / S of the tile's n = live
    taps * ceil(CK / 16) (the column tiles of a row tile share them)."""
    CK = gemm_of(geo, mode)[5]
    n = kernel_taps(geo, mode, 128) * cdiv(CK, 16)
    return [[(sp * t // S, (sp + 1) * t // S - sp * t // S) for sp in range(S)] for t in n.tolist()]


# ================================================================================================ the cases
# (B, H, W, Cin, Cout, k, stride, pad, dil) and the property the case is in the table for; every comment is asserted by
# test_cases_have_the_properties_they_are_named_after.  fwd / dgrad: mode 0 / 1; p0 .. p3: the precision.
CASES = [
    ((1, 13, 11, 64, 24, 3, 1, 1, 1), "fwd p0: 128x32 with vector loaders, 143 rows = a ragged second row tile"),
    ((2, 9, 9, 10, 7, 3, 1, 1, 1), "p0: 128x32 scalar in both modes, 7 resp. 10 columns of 32"),
    ((2, 9, 9, 10, 8, 3, 1, 1, 1), "fwd p0: 128x32 scalar with the vector epilogue"),
    ((2, 9, 9, 8, 10, 3, 1, 1, 1), "dgrad p0: 128x32 scalar with the vector epilogue"),
    ((2, 9, 9, 50, 70, 1, 1, 0, 1), "p0: 64x64 scalar in both modes"),
    ((2, 9, 9, 50, 72, 1, 1, 0, 1), "fwd p0: 64x64 scalar with the vector epilogue"),
    ((2, 9, 9, 52, 70, 1, 1, 0, 1), "dgrad p0: 64x64 scalar with the vector epilogue"),
    ((1, 65, 127, 64, 80, 1, 1, 0, 1), "p0: 64x64 vector in both modes, M = 8255, ktot = 64; p2 without tile or split falls back to it"),
    ((1, 65, 127, 64, 96, 3, 1, 1, 1), "p0: 128x64 in both modes, with taps"),
    ((1, 65, 127, 512, 96, 1, 1, 0, 1), "p0: 128x64 forward, 64x64 data gradient (ktot = 96 < 512)"),
    ((1, 64, 128, 64, 48, 1, 1, 0, 1), "p0: M = 8192, the last row count of dma_shape: family 2"),
    ((1, 64, 128, 64, 48, 1, 1, 1, 1), "fwd p0: the same map padded by a pixel, M = 8580 at ktot < 1024: family 1; dgrad: M = 8192, family 2"),
    ((1, 1, 8193, 64, 48, 1, 1, 0, 1), "p0: M = 8193 at ktot < 1024: family 1 in both modes"),
    ((1, 65, 127, 1024, 48, 1, 1, 0, 1), "fwd p0: family 2 above 8192 rows through ktot >= 1024"),
    ((1, 13, 11, 72, 100, 1, 1, 0, 1), "p0: the ring with ragged M, N and K; 3 row tiles padded to 8, five idle"),
    ((1, 8, 8, 64, 1024, 1, 1, 0, 1), "dgrad p0 with kscale: the 1024-float copy filled exactly, family 2"),
    ((1, 8, 8, 64, 1028, 1, 1, 0, 1), "dgrad p0 with kscale: 1028 > 1024 -> 128x64 of family 1; without kscale family 2"),
    ((1, 67, 64, 40, 16, 3, 4, 0, 1), "dgrad p0: ring; the 64-row tile of y = 3 has no live tap"),
    ((1, 67, 64, 40, 10, 3, 4, 0, 1), "dgrad p0: 64x64 scalar; the 64-row tile of y = 3 has no live tap"),
    ((1, 14, 14, 12, 40, 6, 2, 2, 1), "36 taps > 32: no tap list"),
    ((1, 16, 16, 24, 40, 3, 1, 18, 18), "only the centre tap is live"),
    ((2, 16, 16, 48, 96, 3, 2, 1, 1), "dgrad p0: the ring under perm2"),
    ((1, 18, 14, 48, 96, 3, 2, 1, 1), "dgrad p0: stride 2 without perm2, M = 252 is no multiple of 512"),
    ((1, 128, 128, 64, 64, 1, 2, 0, 1), "dgrad p0: 1x1 stride 2, three pixels in four have no tap; 64x64 vector under perm2"),
    ((2, 16, 16, 50, 70, 3, 2, 1, 1), "dgrad p0: 64x64 scalar under perm2"),
    ((2, 16, 16, 24, 40, 3, 2, 1, 1), "dgrad p0: 128x32 vector under perm2"),
    ((2, 16, 16, 10, 7, 3, 2, 1, 1), "dgrad p0: 128x32 scalar under perm2"),
    ((1, 128, 96, 48, 64, 3, 2, 1, 1), "dgrad p0: 128x64 under perm2"),
    ((1, 127, 129, 72, 72, 1, 1, 0, 1), "fwd and dgrad p2 / p1 / p3: tile 21 unsplit, ragged rows (M = 16383), columns and contraction"),
    ((1, 90, 90, 64, 1000, 1, 1, 0, 1), "fwd: tile 22 with a ragged last column tile, 64 x 8 = 512 tiles; dgrad: family 2"),
    ((1, 150, 218, 64, 220, 1, 1, 0, 1), "fwd: waste22 turns tile 22 into tile 21; dgrad: tile 21 at 64 columns"),
    ((1, 128, 128, 128, 40, 3, 2, 1, 1), "dgrad: tile 21 under perm2, contraction of 40"),
    ((1, 256, 256, 128, 48, 1, 1, 0, 1), "dgrad: tile 22 (512 row tiles x 1), pre-split weights on <2, 2> in mode 1; fwd tile 21"),
    ((1, 256, 256, 128, 40, 1, 2, 0, 1), "dgrad: tile 22 under perm2"),
    ((1, 15, 20, 4096, 512, 1, 1, 0, 1), "fwd p2: S = 8, M = 300: 3 row tiles x 8 = 24 tiles"),
    ((8, 16, 16, 2048, 512, 1, 1, 0, 1), "fwd p2: S = 4"),
    ((1, 15, 20, 512, 512, 3, 1, 1, 1), "p2: 3x3 split 8 ways, splits start inside a tap"),
    ((1, 15, 20, 512, 512, 3, 1, 8, 8), "p2: k_live is the full 4608 but the first row tile has six live taps"),
    ((1, 15, 20, 512, 512, 3, 1, 20, 20), "p2: only the centre tap reaches the 15 x 20 map (at 16 the columns 16..19 still do): k_live = 512 turns the split off that ktot = 4608 would have made: family 2"),
]
GEOS = [g for g, _ in CASES]


def variants(geo):
    """What the calls of a case reach: (kernel name, tile, mode, loaders, e_vec), ("perm2", ...) and the finish kernels."""
    out = set()
    for mode in (0, 1):
        for prec in PRECISIONS:
            calls = [(f, False) for f in FORMS] + ([(f, True) for f in PLANE_FORMS] if prec == 2 and planes_ok(geo, mode) else [])
            for form, pl in calls:
                c = choice(geo, mode, prec, form, pl, ws_of(geo, mode) if prec == 2 else 0)
                if c is None:
                    continue
                name = ["igemm_kernel", "igemm_dma_kernel<3,1,1>", "x6 tile", "bf16 tile", "igemm_planes_kernel", "igemm_bf16_kernel"][c.kernel]
                key = (name, c.tile, mode, "vec" if (c.a_vec and c.b_vec) or c.kernel == BF16 else "scalar")          # (the bf16 kernel has one loader)
                out.add(key + (c.e_vec,))
                if mode == 1 and c.kernel not in (PLANES, BF16):
                    out.add(("perm2",) + key + (c.perm2,))
                if c.S > 1:
                    out.add(("igemm_splitk_finish_kernel", "<1,2,4,1>" if c.kernel == PLANES else "<2,1,2,2>"))
    return out


KERNELS = ([("igemm_kernel", t, m, v) for t in (128032, 128064, 64064) for m in (0, 1) for v in ("vec", "scalar")] +          # 12
           [("igemm_dma_kernel<3,1,1>", 64064, m, "vec") for m in (0, 1)] +                                                # 2
           [(n, t, m, "vec") for n in ("x6 tile", "bf16 tile") for t in (22, 21) for m in (0, 1)] +                         # 4 + 4
           [("igemm_planes_kernel", 22, m, "vec") for m in (0, 1)] + [("igemm_planes_kernel", 21, m, "vec") for m in (0, 1)] +   # <2,2,false>, <1,3,false>
           [("igemm_bf16_kernel", 64064, m, "vec") for m in (0, 1)])                                                       # 2
FINISH = {("igemm_splitk_finish_kernel", "<2,1,2,2>"), ("igemm_splitk_finish_kernel", "<1,2,4,1>")}
# instantiated by the launcher's macro, out of reach of its rule: 128 x 64 asks for vector loaders
UNREACHABLE = {("igemm_kernel", 128064, 0, "scalar"), ("igemm_kernel", 128064, 1, "scalar")}
ALL_VARIANTS = ({k + (e,) for k in KERNELS if k not in UNREACHABLE for e in (0, 1)} | FINISH |
                {("perm2",) + k + (v,) for k in KERNELS if k not in UNREACHABLE and k[2] == 1
                 and k[0] not in ("igemm_planes_kernel", "igemm_bf16_kernel") for v in (0, 1)})


# ================================================================================================ operands and references
def bf(t):
    return t.bfloat16().float()


def conv(x, w, geo):
    return F.conv2d(x, w, None, *geo[6:])


def conv_t(g, w, geo):
    B, H, W, Ci = geo[:4]
    return torch.nn.grad.conv2d_input((B, Ci, H, W), w, g, *geo[6:])


def bc(t):
    return t[None, :, None, None]


def refs(D, x, w, g, ks, dtype):
    """The outputs of every form in `dtype`, on the fp32 operands x, w, g (as given: rounded to bf16 or not) -> dict by (mode, form, name)."""
    t = lambda v: v.to(dtype)
    Y, DX, DXK = conv(t(x), t(w), D.geo), conv_t(t(g), t(w), D.geo), conv_t(t(g) * bc(t(ks)), t(w), D.geo)
    ypre = Y + bc(t(D.b))
    return {(0, "a", "y"): ypre, (0, "b", "y"): t(D.y0) + ypre, (0, "c", "ypre"): ypre,
            (0, "c", "y"): t(D.res) + bc(t(D.rs)) * torch.relu(ypre), (0, "d", "y"): ypre,
            (1, "a", "y"): DX + bc(t(D.b1)), (1, "b", "y"): t(D.dx0) + DX + bc(t(D.b1)), (1, "c", "y"): DXK, (1, "d", "y"): DX + bc(t(D.b1))}


def magnitudes(D, ks):
    """A of every output: the same convolution of the absolute operands, through the form's scale (the x6 allowance), and the
    largest |partial sum| any order of summation can meet (the 2^24 proof)."""
    a = lambda v: v.double().abs()
    AY, ADX, ADXK = conv(a(D.x), a(D.w), D.geo), conv_t(a(D.g), a(D.w), D.geo), conv_t(a(D.g) * bc(a(ks)), a(D.w), D.geo)
    A = {(0, "a", "y"): AY, (0, "b", "y"): AY, (0, "c", "ypre"): AY, (0, "c", "y"): bc(a(D.rs)) * AY, (0, "d", "y"): AY,
         (1, "a", "y"): ADX, (1, "b", "y"): ADX, (1, "c", "y"): ADXK, (1, "d", "y"): ADX}
    top = max((AY + bc(a(D.b)) + a(D.y0)).max().item(), (a(D.res) + bc(a(D.rs)) * (AY + bc(a(D.b)))).max().item(),
              (ADX + bc(a(D.b1)) + a(D.dx0)).max().item(), ADXK.max().item())
    return A, top


def build(geo, kind):
    """kind: "exact", "exact1" ({-1, 0, 1}: a case whose sums would pass 2^24) or "rounded"."""
    B, H, W, Ci, Co, k, s, p, d = geo
    OH, OW = out_hw(geo)
    shapes = dict(x=(B, Ci, H, W), w=(Co, Ci, k, k), b=(Co,), b1=(Ci,), g=(B, Co, OH, OW), y0=(B, Co, OH, OW), dx0=(B, Ci, H, W),
                  res=(B, Co, OH, OW), rs=(Co,), ks=(Co,))
    D = types.SimpleNamespace(kind=kind, geo=geo, at={}, dev={})
    if kind != "rounded":
        rng = np.random.default_rng(list(geo))
        for name, sh in shapes.items():
            m = 1 if kind == "exact1" else 2 if name in ("x", "g") else 3
            setattr(D, name, torch.from_numpy(rng.integers(-m, m + 1, sh).astype(np.float32)))
        D.ks2 = D.ks
        r64 = refs(D, D.x, D.w, D.g, D.ks, torch.float64)
        D.ref = {prec: r64 for prec in PRECISIONS}
        D.A, D.top = magnitudes(D, D.ks)
        return D
    for D.draw in range(MAX_DRAWS):          # the first draw whose reference is well conditioned
        for i, (name, sh) in enumerate(shapes.items()):
            setattr(D, name, rnd(*sh, seed=100 * D.draw + i + 1))
        D.w = (D.w / np.sqrt(Ci * k * k)).float()
        r64 = refs(D, D.x, D.w, D.g, D.ks, torch.float64)
        D.A, D.top = magnitudes(D, D.ks)
        # the metric of dist() divides by an output's largest element: sum |terms| / |sum| of THAT element (tests/test_direct_conv.py)
        D.cond = max((D.A[key].flatten()[r64[key].abs().argmax()] / r64[key].abs().max()).item() for key in ((0, "c", "ypre"), (1, "a", "y"), (1, "c", "y")))
        if D.cond <= COND_LIMIT:
            break
    # precisions 1 and 3: the operands rounded to bf16; kscale a signed power of two there, so that scaling commutes with the rounding
    D.ks2 = torch.sign(D.ks) * 2.0 ** torch.round(D.ks.abs().clamp(0.5, 2.0).log2())
    D.ks2[D.ks2 == 0] = 1.0
    r64b = refs(D, bf(D.x), bf(D.w), bf(D.g), D.ks2, torch.float64)
    r32 = refs(D, D.x, D.w, D.g, D.ks, torch.float32)
    r32b = refs(D, bf(D.x), bf(D.w), bf(D.g), D.ks2, torch.float32)
    d32 = max(dist(r32[key], r64[key]) for key in r64)
    d32b = max(max(dist(r32b[key], r64b[key]) for key in r64), d32)
    D.ref = {0: r64, 2: r64, 1: r64b, 3: r64b}
    for prec, e in ((0, d32), (2, d32), (1, d32b), (3, d32b)):
        D.at[prec] = types.SimpleNamespace(d32=e, bound=4 * max(e, ULP_FLOOR), seen=0.0, share=0.0)
    return D


@functools.lru_cache(maxsize=None)
def data(geo, kind):
    D = build(geo, kind)
    if kind == "exact" and D.top >= EXACT_LIMIT:
        D = build(geo, "exact1")
    return D


# ================================================================================================ tests that need no GPU
def every_call(geo):
    """(mode, precision, form, planes, workspace bytes) of every call the GPU test makes for a case, the short workspace included."""
    for mode in (0, 1):
        for prec in PRECISIONS:
            ws = ws_of(geo, mode) if prec == 2 else 0
            for form in FORMS:
                yield mode, prec, form, False, ws
                if ws:
                    yield mode, prec, form, False, ws - 1
                    yield mode, prec, form, False, 0
            if prec == 2 and planes_ok(geo, mode):
                for form in PLANE_FORMS:
                    yield mode, prec, form, True, ws
                    if ws:
                        yield mode, prec, form, True, ws - 1


def test_restatement_is_the_librarys_plan(lib):
    """Every case, mode, precision and form: the Python restatement == vrnet_conv2d_plan, refusals and the workspace size included."""
    n = 0
    for geo in GEOS:
        for mode in (0, 1):
            M, MH, MW, SH, SW, CK, CN = gemm_of(geo, mode)
            assert ws_of(geo, mode) == lib._lib.vrnet_conv2d_splitk_workspace(M, CN, CK * geo[5] ** 2), (geo, mode)
            assert dma_tile(M, CN) == lib.conv2d_dma_tile(M, CN)
            assert dma_plan(M, CN, CK * geo[5] ** 2, 1 << 40) == lib.conv2d_dma_plan(M, CN, CK * geo[5] ** 2)
        for mode, prec, form, planes, ws in every_call(geo):
            n += 1
            try:
                want = as_tuple(conv_choose(geo, mode, prec, form, planes, ws))
            except Refused as r:
                with pytest.raises(RuntimeError, match=str(r)):
                    library_plan(lib, geo, mode, prec, form, planes, ws)
                continue
            assert library_plan(lib, geo, mode, prec, form, planes, ws) == want, (geo, mode, prec, form, planes, ws)
    assert n > 1000


def test_plan_query_refuses_what_the_launcher_refuses(lib):
    geo = GEOS[0]
    with pytest.raises(RuntimeError, match="conv2d: precision 0"):
        lib.conv2d_plan(*g12(geo), precision=4)
    with pytest.raises(RuntimeError, match="row stride smaller than channel count"):
        lib.conv2d_plan(*g12(geo), lda=geo[3] - 1)
    with pytest.raises(RuntimeError, match="inconsistent with input"):
        lib.conv2d_plan(1, 13, 11, 64, 13, 12, 24, 3, 3, 1, 1, 1)
    with pytest.raises(RuntimeError, match="output statistics need"):
        lib.conv2d_plan(*g12(geo), stats=True)                                        # 24 <= 32 output channels
    with pytest.raises(RuntimeError, match=BF16_PATH):
        lib.conv2d_plan(*g12((1, 65, 127, 64, 80, 1, 1, 0, 1)), precision=1, misaligned=("a",))
    with pytest.raises(RuntimeError, match=PREC3):
        lib.conv2d_plan(*g12((1, 127, 129, 72, 72, 1, 1, 0, 1)), precision=3, misaligned=("w",))
    # the early exits, which tests/test_direct_conv.py holds: tiny (plain calls only), narrow, patch data gradient
    assert lib.conv2d_plan(*g12((2, 17, 19, 4, 4, 1, 1, 0, 1)), plain=True)[:2] == (4, 6)
    assert lib.conv2d_plan(*g12((2, 17, 19, 4, 4, 1, 1, 0, 1)))[0] == 1
    assert lib.conv2d_plan(*g12((2, 5, 7, 100, 9, 1, 1, 0, 1)), plain=True)[:2] == (5, 7)
    assert lib.conv2d_plan(*g12((2, 5, 7, 100, 9, 1, 1, 0, 1)), plain=True, misaligned=("a",))[0] == 1
    assert lib.conv2d_plan(*g12((2, 12, 20, 5, 64, 4, 4, 0, 1)), mode=1, plain=True)[:2] == (4, 8)
    # each alignment flag on its own: the vector epilogue goes, the kernel stays
    geo = (1, 13, 11, 72, 100, 1, 1, 0, 1)
    assert lib.conv2d_plan(*g12(geo))[8] == 1
    for name in ("y", "bias", "ypre", "res", "res_scale", "aux"):
        got = lib.conv2d_plan(*g12(geo), misaligned=(name,))
        assert got[8] == 0 and got[:2] == (2, 1), name
    assert lib.conv2d_plan(*g12(geo), misaligned=("a",))[6:8] == (0, 1) and lib.conv2d_plan(*g12(geo), misaligned=("w",))[6:8] == (1, 0)
    assert lib.conv2d_plan(*g12(geo), ldy=101)[8] == 0 and lib.conv2d_plan(*g12(geo), lda=73)[6] == 0


def test_cases_reach_every_variant():
    assert len(GEOS) == len(set(GEOS))
    # the 28 instantiations the launcher names (igemm_planes_kernel<2, 2, false> and <1, 3, false> serve both modes: mode is an argument there)
    assert len({k[:2] if k[0] == "igemm_planes_kernel" else k for k in KERNELS}) + len(FINISH) == 28 and UNREACHABLE < set(KERNELS)
    reached = set().union(*(variants(g) for g in GEOS))
    assert reached == ALL_VARIANTS, (sorted(map(str, ALL_VARIANTS - reached)), sorted(map(str, reached - ALL_VARIANTS)))


def test_rules_that_no_shape_reaches():
    """With the default tuning values: the third rule of vr_dma_tile never answers (nt21 >= nt22, so the second rule takes every
    shape it would), and the 128 x 64 register-staged tile never runs with scalar loaders (its rule asks for `vec`).  The code
    stays: VRNET_X6_MIN_TILES / VRNET_X6_MIN_N and VRNET_IGEMM_NARROW of the diagnostic build can still reach it."""
    for CN in range(33, 600):
        nt22, nt21 = cdiv(CN, 128), cdiv(CN, 64)
        assert nt21 >= nt22
        for mt in sorted({cdiv(MIN_TILES, nt22) + e for e in (-1, 0, 1)} | {cdiv(MIN_TILES, nt21) + e for e in (-1, 0, 1)} |
                         {cdiv(2 * MIN_TILES, nt22) + e for e in (-1, 0, 1)} | {1, 547}):
            assert dma_tile(128 * mt, CN, rule=True) != 3 and dma_tile(128 * mt - 127, CN, rule=True) != 3, (mt, CN)
    rng = np.random.default_rng(0)
    for _ in range(20000):
        geo = tuple(int(v) for v in (rng.integers(1, 3), rng.integers(1, 40), rng.integers(1, 40), rng.integers(9, 300), rng.integers(17, 300),
                                     rng.integers(1, 4), rng.integers(1, 3), rng.integers(0, 3), 1))
        if min(out_hw(geo)) < 1:
            continue
        for mode in (0, 1):
            c = choice(geo, mode, 0)
            assert not (c.kernel == IGEMM and c.tile == 128064 and not (c.a_vec and c.b_vec)), (geo, mode)


def test_cases_have_the_properties_they_are_named_after():
    """The comments of CASES, asserted, in the table's order."""
    def K(geo, mode, prec, form="a", planes=False, ws=None):
        c = choice(geo, mode, prec, form, planes, ws_of(geo, mode) if ws is None else ws)
        return None if c is None else (c.family, c.kernel, c.tile, "vec" if c.a_vec and c.b_vec else "scalar")

    C = lambda geo, mode, prec, form="a", planes=False: choice(geo, mode, prec, form, planes, ws_of(geo, mode))
    M = lambda geo, mode: gemm_of(geo, mode)[0]
    it = iter(GEOS)
    g = next(it); assert K(g, 0, 0) == (1, IGEMM, 128032, "vec") and M(g, 0) == 143 and C(g, 0, 0).gx == 2
    g = next(it); assert K(g, 0, 0) == K(g, 1, 0) == (1, IGEMM, 128032, "scalar") and C(g, 0, 0).e_vec == C(g, 1, 0).e_vec == 0
    g = next(it); assert K(g, 0, 0) == (1, IGEMM, 128032, "scalar") and C(g, 0, 0).e_vec == 1
    g = next(it); assert K(g, 1, 0) == (1, IGEMM, 128032, "scalar") and C(g, 1, 0).e_vec == 1
    g = next(it); assert K(g, 0, 0) == K(g, 1, 0) == (1, IGEMM, 64064, "scalar") and C(g, 0, 0).e_vec == C(g, 1, 0).e_vec == 0
    g = next(it); assert K(g, 0, 0) == (1, IGEMM, 64064, "scalar") and C(g, 0, 0).e_vec == 1
    g = next(it); assert K(g, 1, 0) == (1, IGEMM, 64064, "scalar") and C(g, 1, 0).e_vec == 1
    g = next(it); assert K(g, 0, 0) == K(g, 1, 0) == (1, IGEMM, 64064, "vec") and M(g, 0) == 8255 and K(g, 0, 2) == K(g, 1, 2) == K(g, 0, 0)
    assert ws_of(g, 0) == 0 and dma_tile(8255, 80) == 0 and K(g, 0, 3) is None and K(g, 0, 1) == (3, BF16, 64064, "vec")
    g = next(it); assert K(g, 0, 0) == K(g, 1, 0) == (1, IGEMM, 128064, "vec") and g[5] == 3
    g = next(it); assert K(g, 0, 0) == (1, IGEMM, 128064, "vec") and K(g, 1, 0) == (1, IGEMM, 64064, "vec") and g[4] < 512 <= g[3]
    g = next(it); assert M(g, 0) == M(g, 1) == 8192 and K(g, 0, 0) == K(g, 1, 0) == (2, RING, 64064, "vec")
    g = next(it); assert M(g, 0) == 8580 and K(g, 0, 0) == (1, IGEMM, 64064, "vec") and K(g, 1, 0)[0] == 2 and g[:7] == GEOS[10][:7]
    g = next(it); assert M(g, 0) == M(g, 1) == 8193 and K(g, 0, 0) == K(g, 1, 0) == (1, IGEMM, 64064, "vec") and g[3:] == GEOS[10][3:]
    g = next(it); assert M(g, 0) == 8255 and K(g, 0, 0) == (2, RING, 64064, "vec") and g[3] == 1024
    g = next(it); assert K(g, 0, 0) == K(g, 1, 0) == (2, RING, 64064, "vec") and M(g, 0) == 143 and (72 % 16, 100 % 64, 143 % 64) == (8, 36, 15)
    assert C(g, 0, 0).gx == 8 * 2 and cdiv(143, 64) == 3
    g = next(it); assert K(g, 1, 0, "c") == K(g, 1, 0, "a") == (2, RING, 64064, "vec") and g[4] == 1024
    g = next(it); assert K(g, 1, 0, "c") == (1, IGEMM, 128064, "vec") and K(g, 1, 0, "a") == (2, RING, 64064, "vec") and g[4] == 1028
    g = next(it); assert K(g, 1, 0) == (2, RING, 64064, "vec") and tile_taps(g, 1, 64)[3] == 0 and tile_taps(g, 1, 64)[2] > 0 and g[2] == 64
    g = next(it); assert K(g, 1, 0) == (1, IGEMM, 64064, "scalar") and tile_taps(g, 1, 64)[3] == 0
    g = next(it); assert g[5] ** 2 == 36 > 32 and K(g, 0, 0)[0] == 2 and K(g, 1, 0)[:3] == (1, IGEMM, 128032)
    g = next(it); assert k_live_of(g, 0) == g[3] and k_live_of(g, 1) == g[4] and set(tile_taps(g, 0, 64).tolist()) == {1}
    g = next(it); assert K(g, 1, 0) == (2, RING, 64064, "vec") and C(g, 1, 0).perm2 == 1
    g = next(it); assert K(g, 1, 0) == (2, RING, 64064, "vec") and C(g, 1, 0).perm2 == 0 and M(g, 1) == 252
    g = next(it); assert K(g, 1, 0) == (1, IGEMM, 64064, "vec") and C(g, 1, 0).perm2 == 1 and g[5:7] == (1, 2)
    y, x = row_pixels(g, 1)
    assert (tap_live(g, 1, y, 0, 64) & tap_live(g, 1, x, 0, 64)).mean() == 0.25 and (tile_taps(g, 1, 64) == 0).mean() == 0.75
    g = next(it); assert K(g, 1, 0) == (1, IGEMM, 64064, "scalar") and C(g, 1, 0).perm2 == 1
    g = next(it); assert K(g, 1, 0) == (1, IGEMM, 128032, "vec") and C(g, 1, 0).perm2 == 1
    g = next(it); assert K(g, 1, 0) == (1, IGEMM, 128032, "scalar") and C(g, 1, 0).perm2 == 1
    g = next(it); assert K(g, 1, 0) == (1, IGEMM, 128064, "vec") and C(g, 1, 0).perm2 == 1
    g = next(it); assert M(g, 0) == 16383 and [K(g, m, p)[:3] for m in (0, 1) for p in (2, 3)] == [(6, X6, 21), (3, BF16_TILE, 21)] * 2
    assert K(g, 0, 1)[:3] == (3, BF16_TILE, 21) and K(g, 1, 1)[:2] == (3, BF16) and (16383 % 128, 72 % 64, 72 % 16) == (127, 8, 8)
    g = next(it); assert K(g, 0, 2)[:3] == (6, X6, 22) and C(g, 0, 2).gx == 64 * 8 and 1000 % 128 == 104 and K(g, 1, 2)[0] == 2 and K(g, 1, 3) is None
    g = next(it); assert K(g, 0, 2)[:3] == (6, X6, 21) and cdiv(32700, 128) * 2 >= 512 and 2 * 128 - 220 > 32 and K(g, 1, 2)[:3] == (6, X6, 21)
    g = next(it); assert K(g, 1, 2)[:3] == (6, X6, 21) and C(g, 1, 2).perm2 == 1 and g[4] == 40 and K(g, 1, 3)[:3] == (3, BF16_TILE, 21)
    g = next(it); assert K(g, 1, 2)[:3] == (6, X6, 22) and K(g, 1, 2, "a", True)[:3] == (9, PLANES, 22) and K(g, 0, 2)[:3] == (6, X6, 21)
    assert K(g, 0, 2, "a", True)[:3] == (9, PLANES, 21) and C(g, 1, 2).gx == 512
    g = next(it); assert K(g, 1, 2)[:3] == (6, X6, 22) and C(g, 1, 2).perm2 == 1 and K(g, 1, 3)[:3] == (3, BF16_TILE, 22)
    g = next(it); assert K(g, 0, 2)[:3] == (6, X6, 21) and C(g, 0, 2).S == 8 and M(g, 0) == 300 and C(g, 0, 2).fin == 8 * 8 and 3 * 8 == 24
    assert K(g, 0, 2, "a", True)[:2] == (9, PLANES) and C(g, 0, 2, "a", True).S == 8
    g = next(it); assert K(g, 0, 2)[:3] == (6, X6, 21) and C(g, 0, 2).S == 4
    g = next(it); assert C(g, 0, 2).S == 8 == C(g, 1, 2).S and any(b % 32 for tile in split_ranges(g, 0, 8) for b, n in tile)
    g = next(it); assert C(g, 0, 2).S == 8 and C(g, 0, 2).k_live == 4608 and tile_taps(g, 0, 128).tolist() == [6, 9, 6]
    g = next(it); assert C(g, 0, 2).k_live == 512 and K(g, 0, 2) == (2, RING, 64064, "vec") and ws_of(g, 0) > 0 and dma_plan(300, 512, 4608, 1 << 40) == (21, 8)
    assert next(it, None) is None
    # no split of the table has a workgroup with an empty step range; the fall-back of every split case is family 2
    for geo in GEOS:
        for mode in (0, 1):
            c = C(geo, mode, 2)
            if c.S > 1:
                assert all(n > 0 for tile in split_ranges(geo, mode, c.S) for b, n in tile), (geo, mode)
                assert K(geo, mode, 2, ws=ws_of(geo, mode) - 1) == (2, RING, 64064, "vec") == K(geo, mode, 2, ws=0), (geo, mode)


def test_exact_cases_stay_below_2_24():
    for geo in GEOS:
        D = data(geo, "exact")
        assert D.top < EXACT_LIMIT, (geo, D.kind)


def test_rounded_bounds_stay_below_the_suite_tolerance():
    for geo in GEOS:
        D = data(geo, "rounded")
        assert D.cond <= COND_LIMIT, (geo, D.cond)          # a draw was found
        for prec in PRECISIONS:
            assert ULP_FLOOR * 4 <= D.at[prec].bound <= TOL, (geo, prec, D.at[prec].d32)


# ================================================================================================ running a case on the GPU
GUARD = 4096          # bytes of PAT behind the workspace
FINITE = 12345.0      # the second poison
CTOT_EXTRA, COFF = 5, 2          # form (d): the output is channels [2, 2 + CN) of a tensor of CN + 5


def workspace(nbytes, poison):
    """A workspace of exactly nbytes, poisoned, with the guard pattern behind it -> (buffer, the workspace view)."""
    assert nbytes % 4 == 0
    buf = torch.full((nbytes // 4 + GUARD // 4,), poison, device="cuda")
    buf.view(torch.int32)[nbytes // 4:] = PAT
    assert buf.data_ptr() % 16 == 0
    return buf, buf.view(torch.uint8)[:nbytes]


def ws_guard_intact(buf, nbytes):
    return bool((buf.view(torch.int32)[nbytes // 4:] == PAT).all())


def held(D, prec, key, got, what):
    """No NaN; then bit for bit (exact), within the precision's bound in the metric of dist() (rounded, precisions 0, 1, 3), or
    within bound * max |ref| + 2^-20 A element by element (rounded, precision 2)."""
    ref = D.ref[prec][key]
    got = got.detach().double().cpu()
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    assert not bool(torch.isnan(got).any()), f"{what} {D.geo}: NaN in the result (a guard column or an unwritten slab element was read)"
    if D.kind != "rounded":
        bad = got != ref
        assert not bool(bad.any()), f"{what} {D.geo}: {int(bad.sum())} of {ref.numel()} values differ from the exact result, first at " \
                                    f"{tuple(bad.nonzero()[0].tolist())}: {got[bad][0].item()} for {ref[bad][0].item()}"
        return
    R = D.at[prec]
    e = dist(got, ref)
    R.seen = max(R.seen, e)
    if prec == 2:
        allow = R.bound * ref.abs().max().item() + 2.0 ** -20 * D.A[key]
        share = ((got - ref).abs() / allow).max().item()
        R.share = max(R.share, share)
        print(f"  {D.geo} {what}: {e:.2e}, {share:.3f} of its bound")
        assert share <= 1.0, f"{what} {D.geo}: {share:.3f} of the element's bound, distance {e:.3e}"
    else:
        print(f"  {D.geo} {what}: {e:.2e}")
        assert e <= R.bound, f"{what} {D.geo}: distance {e:.3e}, bound {R.bound:.3e} (d32 {R.d32:.3e})"


def planes_pack(hip, D, mode, ks):
    """Pre-split weights as tests/test_hip_ops.py::test_x6_conv_with_presplit_weights packs them: forward w[Cout][Cin], data
    gradient the transposed weights with kscale folded in."""
    from tests.test_hip_ops import _planes
    Ci, Co = D.geo[3:5]
    w = D.dev["w1x1"]
    return _planes(hip, w, Co, Ci, Ci, 1) if mode == 0 else _planes(hip, w, Ci, Co, 1, Ci, kscale=ks)


def call(hip, D, mode, prec, form, planes=False, ws=None, want=None):
    """One call of form `form`; -> {name: NCHW result on the CPU}.  Guards of the pitched output checked, last_kernel() asserted."""
    geo = D.geo
    B, H, W, Ci, Co, k, s, p, d = geo
    OH, OW = out_hw(geo)
    M, MH, MW, SH, SW, CK, CN = gemm_of(geo, mode)
    dv = D.dev
    ks = (D.ks2 if prec in (1, 3) else D.ks) if (form == "c" and mode == 1) else None
    ksg = None if ks is None else ks.cuda()
    w = dv["w"]
    kw = dict(mode=mode, precision=prec)
    if prec == 1 and mode == 1:          # the transposed pack, kscale folded in
        w = torch.empty(k * k, Ci, Co, device="cuda")
        hip.pack_weight_t(D.w.contiguous().cuda(), ksg, w, Co, Ci, k, k)
        ksg = None
    if planes:
        kw["w_planes"] = planes_pack(hip, D, mode, ksg)
    if ws is not None:
        kw["workspace"] = ws
    a = dv["a", mode]
    oshape = (B, MH, MW, CN)
    outs = {}
    if form == "d":
        y = pat(B, CN + CTOT_EXTRA, MH, MW)
        hip.conv2d(a, ld(a), w, dv["bias", mode], y, CN, *g12(geo), out_nchw=1, out_ctot=CN + CTOT_EXTRA, out_coff=COFF, **kw)
        raw = y.view(torch.int32)
        assert bool((raw[:, :COFF] == PAT).all()) and bool((raw[:, COFF + CN:] == PAT).all()), f"{geo} (d): channels beside the range changed"
        outs["y"] = y[:, COFF:COFF + CN].cpu()
    else:
        old = {0: D.y0, 1: D.dx0}[mode]
        buf, y = outp(nhwc(old) if form == "b" else oshape, "A", 1)
        extra = {}
        if form == "b":
            extra = dict(accumulate=1)
        if form == "c" and mode == 0:
            pbuf, ypre = outp(oshape, "A", 2)
            res = inp(nhwc(D.res), "A", 3)
            extra = dict(act=1, ypre=ypre, ldypre=ld(ypre), res=res, ldres=ld(res), res_scale=dv["rs"])
        if form == "c" and mode == 1:
            extra = dict(kscale=ksg)
        bias = None if (form == "c" and mode == 1) else dv["bias", mode]
        hip.conv2d(a, ld(a), w, bias, y, ld(y), *g12(geo), **extra, **kw)
        assert guards_intact(buf, y), f"{geo} ({form}): guard columns of the output changed"
        outs["y"] = nchw(y)
        if form == "c" and mode == 0:
            assert guards_intact(pbuf, ypre), f"{geo} (c): guard columns of ypre changed"
            outs["ypre"] = nchw(ypre)
    assert hip.last_kernel() == want.family, (geo, mode, prec, form, hip.last_kernel(), want.family)
    return outs


def run_case(hip, geo, kind, prec):
    D = data(geo, kind)
    B, H, W, Ci, Co, k, s, p, d = geo
    if not D.dev:
        D.dev.update({("a", 0): inp(nhwc(D.x), "A", 0), ("a", 1): inp(nhwc(D.g), "A", 0), "w": pack(hip, D.w), "w1x1": D.w.contiguous().cuda(),
                      ("bias", 0): D.b.cuda(), ("bias", 1): D.b1.cuda(), "rs": D.rs.cuda()})
    ran = 0
    for mode in (0, 1):
        need = ws_of(geo, mode) if prec == 2 else 0
        M, MH, MW, SH, SW, CK, CN = gemm_of(geo, mode)
        assert ws_of(geo, mode) == hip._lib.vrnet_conv2d_splitk_workspace(M, CN, CK * k * k)
        for planes in ((False, True) if prec == 2 and planes_ok(geo, mode) else (False,)):
            for form in (PLANE_FORMS if planes else FORMS):
                want = choice(geo, mode, prec, form, planes, need)
                what = f"mode {mode} p{prec} ({form}{', planes' if planes else ''})"
                if want is None:          # precision 1 / 3 without a kernel for the shape
                    msg = BF16_PATH if prec == 1 else PREC3
                    with pytest.raises(RuntimeError, match=msg):
                        library_plan(hip, geo, mode, prec, form, planes, need)
                    with pytest.raises(RuntimeError, match=msg):
                        call(hip, D, mode, prec, form, planes, None, want)
                    continue
                assert library_plan(hip, geo, mode, prec, form, planes, need) == as_tuple(want), what
                ran += 1
                runs = []
                for poison in ((NAN, FINITE) if form == "a" else (NAN,)):          # (a) twice: the same bits, whatever the slabs held
                    buf, ws = workspace(need, poison) if need else (None, None)
                    runs.append(call(hip, D, mode, prec, form, planes, ws, want))
                    assert buf is None or ws_guard_intact(buf, need), f"{geo} {what}: the guard behind the workspace changed"
                for name, got in runs[0].items():
                    held(D, prec, (mode, form, name), got, f"{what} {name}")
                    if len(runs) > 1:
                        assert torch.equal(got.view(torch.int32), runs[1][name].view(torch.int32)), f"{geo} {what}: two runs differ"
                if want.S > 1 and form == "a":          # one byte less: the unsplit fall-back the plan names
                    short = choice(geo, mode, prec, form, planes, need - 1)
                    assert library_plan(hip, geo, mode, prec, form, planes, need - 1) == as_tuple(short) and short.S == 1 and short.family == 2
                    buf, ws = workspace(need, NAN)
                    got = call(hip, D, mode, prec, form, planes, ws[:need - 1], short)
                    assert ws_guard_intact(buf, need)
                    if kind == "exact":
                        held(D, 0, (mode, form, "y"), got["y"], f"{what}, short workspace")
                    else:
                        assert dist(got["y"], D.ref[0][mode, form, "y"]) <= D.at[0].bound
    if kind == "rounded" and ran:
        R = D.at[prec]
        print(f"CONV-PLAN {geo} p{prec}: draw {D.draw} cond {D.cond:.1f} d32 {R.d32:.2e} bound {R.bound:.2e} kernel {R.seen:.2e} share {R.share:.3f}")


@gpu
@pytest.mark.parametrize("prec", PRECISIONS, ids=lambda p: f"p{p}")
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("geo", GEOS, ids=str)
def test_conv_at_plan_edge(hip, geo, kind, prec):
    run_case(hip, geo, kind, prec)
