"""The direct (no MFMA) convolution kernels at their dispatch edges: csrc/tinyconv.hip (kernel family 4: Cin, Cout <= 8 at full
resolution, and the data gradient of the patch embeddings) and csrc/narrowconv.hip (family 5: 1 x 1 convs with <= 12 / 16 output
channels over wide rows), through vrnet_conv2d_f32 / vrnet_conv2d_wgrad_f32, forward (mode 0), data gradient (mode 1) and weight
gradient of every case, with hip.last_kernel() asserted after each call.

Two references per case, both fp64 ATen on the fp32 operands:

  exact    integer-valued operands (activations and gradients in {-2..2}, weights, bias and row scale in {-3..3}; {-1, 0, 1} on the
           big maps).  Every partial sum, in any order, is an integer below 2^24 (test_exact_cases_stay_below_2_24 proves it per
           case from conv(|x|, |w|)), so fp32 arithmetic is exact whatever the order and the kernel must give the fp64 result bit
           for bit: an indexing, masking or split error has no tolerance to hide in.
  rounded  rnd(...) operands, weights scaled by 1 / sqrt(fan_in).  The bound comes from the reference, never from the kernel:
           d32 = the largest distance (metric of close(): max |a - b| / max |b|) of fp32 CPU ATen from the fp64 result over the
           case's four outputs, bound = 4 * max(d32, 16 * 2^-24) -- the 4 x of tests/test_loss_edges.py for an fp32 sum in another
           order, the floor so that a case where ATen is nearly exact does not ask for bit equality.  No bound may exceed the
           suite's TOL = 1e-4 (test_rounded_bounds_stay_below_the_suite_tolerance).

           Operands are redrawn until the reference is well conditioned (COND_LIMIT below; 7 of the 123 cases need a redraw).
           Measured on an MI355X (the tests print every figure): d32 5e-8 .. 3.5e-6, the kernels' largest distance per case
           5e-8 .. 5.2e-7, at most 0.14 of the case's bound.

A pass that does NOT run on a direct kernel (the cases that leave a family, the forward and weight gradient of the patch
embeddings) is held to the exact reference as well -- fp32 MFMA products and sums of small integers are exact too -- and, on
rounded operands, to TOL, the bound of those kernels' own tests.

The tests without a gpu mark restate the launchers' integer rules (tiny_shape, vr_narrow_conv_ok, vr_narrow_wgrad_ok, the patch
rule, tiny_wgrad_plan, narrow::plan, narrow_wgrad_plan) in Python and assert for each case the property it was chosen for; the
GPU tests' last_kernel() asserts use the same functions, so the table and the library check each other."""
import functools
import types

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests.test_hip_ops import TOL, nchw, nhwc, pack, rnd
from tests.test_strided_rows import NAN, PAT, guards_intact, inp, ld, outp, pat, refused, scenarios, sid

gpu = pytest.mark.gpu
EXACT_LIMIT = float(1 << 24)
ULP_FLOOR = 16 * 2.0 ** -24
# A rounded case's bound is at least 64 u relative to an output's largest element (u = 2^-24).  Rounding one partial sum as large
# as sum |terms| moves that element by u * conditioning relative to itself (conditioning = sum |terms| / |sum|, of that
# element).  Where the largest element is itself a badly cancelling sum -- the weight gradient of 1 -> 1 is a single element, a
# bias gradient is a sum of zero-mean values over all pixels -- and ATen's sum happens to land close, the floor would ask the
# kernel for better than one such rounding: the figure would measure the draw, not the kernel.  So the operands of a rounded
# case are the first draw of rnd(...) seeds whose fp64 reference has conditioning <= 64: an error of a whole u * sum |terms|
# still fits the floor.  A property of the reference alone; the kernel's result has no part in it.
COND_LIMIT, MAX_DRAWS = 64.0, 12


@pytest.fixture(scope="module")
def hip():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    import asy_vrnet_amd.hip as h
    return h


# ================================================================================================ the launchers' integer rules
def cdiv(a, b):
    return -(-a // b)


def out_hw(geo):
    B, H, W, Ci, Co, k, s, p, d = geo
    return (H + 2 * p - d * (k - 1) - 1) // s + 1, (W + 2 * p - d * (k - 1) - 1) // s + 1


def tiny_shape(geo):                    # igemm.hip: tiny_shape
    B, H, W, Ci, Co, k, s, p, d = geo
    return Ci <= 8 and Co <= 8 and s == 1 and k in (1, 3) and out_hw(geo) == (H, W)


def narrow_conv_ok(geo):                # narrowconv.hip: vr_narrow_conv_ok
    B, H, W, Ci, Co, k, s, p, d = geo
    return k == 1 and s == 1 and p == 0 and Co <= 12 and Ci % 4 == 0 and 16 <= Ci <= 256


def narrow_wgrad_ok(geo):               # narrowconv.hip: vr_narrow_wgrad_ok
    B, H, W, Ci, Co, k, s, p, d = geo
    return k == 1 and s == 1 and p == 0 and Co <= 16 and Ci % 4 == 0 and 16 <= Ci <= 1024


def patch_lds(geo):
    B, H, W, Ci, Co, k, s, p, d = geo
    return k * k * Co * Ci * 4


def patch_ok(geo):                      # vrnet_conv2d_f32: the patch data gradient (plain, mode 1)
    B, H, W, Ci, Co, k, s, p, d = geo
    OH, OW = out_hw(geo)
    return Ci <= 8 and k == s and p == 0 and d == 1 and H == OH * k and W == OW * k and patch_lds(geo) <= 60000


def families(geo, plain=True, aligned=True, dls=False):
    """(forward, data gradient, weight gradient): 4, 5 or 0 (an MFMA kernel), in the order the launchers test -- tiny, narrow,
    patch.  aligned: the operand the narrow dispatch tests has 16-byte rows."""
    tiny = tiny_shape(geo)
    nar = narrow_conv_ok(geo) and not tiny and aligned
    fwd = 4 if plain and tiny else 5 if nar else 0
    dgr = 4 if plain and tiny else 5 if nar else 4 if plain and patch_ok(geo) else 0
    wgr = 4 if tiny else 5 if (not dls and narrow_wgrad_ok(geo) and aligned) else 0
    return fwd, dgr, wgr


def tiny_blocks(npix):                  # vr_tiny_conv / vr_patch_dgrad: workgroups of 256 pixels, at most 16384
    return min(cdiv(npix, 256), 16384)


def tiny_wgrad_plan(npix):              # tinyconv.hip: tiny_wgrad_plan -> (nblk, pix_per_block)
    nb = max(1, min(cdiv(npix, 1024), 2048))
    ppb = cdiv(npix, nb)
    return cdiv(npix, ppb), ppb


TINY_FIXED = [(3, 3, 1), (4, 4, 1), (7, 4, 1), (4, 3, 3)]          # (Cin, Cout, k): conv_fixed_kernel and wgrad_all_kernel


def tiny_wgrad_kernel(Ci, Co, k):       # vr_tiny_wgrad: "all" or wgrad_kernel<CP, KS>
    return "all" if (Ci, Co, k) in TINY_FIXED else (4 if Ci <= 4 else 8, k)


def narrow_plan(K):                     # narrowconv.hip: narrow::plan -> (QP, RL)
    qp = 1
    while qp < K // 4:
        qp <<= 1
    return qp, 256 // qp


def narrow_blocks(M, K):                # vr_narrow_conv
    return max(1, min(cdiv(M, narrow_plan(K)[1] * 8), 2048))


def narrow_wgrad_plan(M):               # narrowconv.hip: narrow_wgrad_plan -> (rows per split, S)
    r = max(cdiv(M, 1024), 32)
    return r, cdiv(M, r)


def narrow_wgrad_lds(K, N):
    qp, rl = narrow_plan(K)
    return rl * N * 4 * qp * 4


# ================================================================================================ the cases
TINY_GENERIC = [(1, 1, 1), (2, 7, 1), (4, 3, 1), (8, 8, 1), (3, 3, 3), (4, 4, 3), (5, 2, 3), (8, 8, 3)]
TINY_MAPS = [(3, 1, 1), (2, 1, 9), (2, 9, 1), (2, 5, 7), (2, 17, 19), (1, 40, 41), (2, 33, 35)]
BIG_MAP = (1, 2049, 2048)


def tiny_geo(shape, m, dil=1):
    (Ci, Co, k), (B, H, W) = shape, m
    return (B, H, W, Ci, Co, k, 1, dil * (k - 1) // 2, dil)


TINY_CASES = ([tiny_geo(s, m) for s in TINY_FIXED for m in TINY_MAPS] +
              [tiny_geo(s, m) for s in TINY_GENERIC for m in ((2, 5, 7), (2, 17, 19))] +
              [tiny_geo(s, (2, 5, 7), dil) for s in TINY_FIXED + TINY_GENERIC if s[2] == 3 for dil in (2, 3, 6)])
TINY_BIG = [tiny_geo((4, 4, 1), BIG_MAP), tiny_geo((4, 3, 3), BIG_MAP)]
TINY_ARGS = [tiny_geo(s, (2, 17, 19)) for s in TINY_FIXED + [(2, 7, 1), (5, 2, 3)]]
TINY_STRIDED = [tiny_geo(s, (2, 17, 19)) for s in [(4, 4, 1), (4, 3, 3), (7, 4, 1), (5, 2, 3)]]

PATCH_SHAPES = [(5, 64, 4), (6, 64, 4), (3, 16, 2), (8, 24, 2), (1, 8, 4), (4, 64, 1)]


def patch_geo(shape):
    Ci, Co, k = shape
    return (2, 3 * k, 5 * k, Ci, Co, k, k, 0, 1)


PATCH_CASES = [patch_geo(s) for s in PATCH_SHAPES]
COUT9_1X1 = (2, 5, 7, 4, 9, 1, 1, 0, 1)          # beside (4, 8, 1) of TINY_LEAVING: forward and weight gradient leave, the data gradient is a patch gradient
PATCH_LDS = [patch_geo((6, 156, 4)), patch_geo((6, 157, 4))]          # 59 904 bytes: family 4; 60 288 bytes: not

# (in the family, its neighbour outside): Cin = 9, Cout = 9, stride 2, k = 3 without padding.  Cout = 9 at k = 3: the data gradient
# of a 1 x 1 conv with Cin <= 8 is a patch data gradient with k = stride = 1 (family 4 again: (4, 64, 1) of PATCH_SHAPES)
TINY_LEAVING = [((2, 5, 7, 8, 4, 1, 1, 0, 1), (2, 5, 7, 9, 4, 1, 1, 0, 1)),
                ((2, 5, 7, 4, 8, 3, 1, 1, 1), (2, 5, 7, 4, 9, 3, 1, 1, 1)),
                ((2, 6, 8, 4, 4, 3, 1, 1, 1), (2, 6, 8, 4, 4, 3, 2, 1, 1)),
                ((2, 5, 7, 4, 3, 3, 1, 1, 1), (2, 5, 7, 4, 3, 3, 1, 0, 1))]

NARROW_SHAPES = [(16, 1), (20, 3), (36, 12), (100, 9), (252, 5), (256, 12)]          # (K, N): all three passes
NARROW_WGRAD_SHAPES = [(260, 4), (516, 7), (1020, 13), (1024, 16)]                   # the weight gradient only
ROWS = {1: (1, 1, 1), 3: (3, 1, 1), 7: (1, 7, 1), 9: (1, 3, 3), 70: (2, 5, 7), 31: (1, 31, 1), 32: (2, 4, 4), 33: (1, 3, 11),
        33124: (1, 182, 182), 66049: (1, 257, 257)}


def narrow_geo(shape, M):
    (K, N), (B, H, W) = shape, ROWS[M]
    return (B, H, W, K, N, 1, 1, 0, 1)


NARROW_CASES = ([narrow_geo(s, M) for s in NARROW_SHAPES + NARROW_WGRAD_SHAPES for M in (3, 33)] +
                [narrow_geo(s, M) for s in ((100, 9), (256, 12)) for M in (1, 7, 9, 70, 31, 32, 33124)])
NARROW_BIG = [narrow_geo((256, 3), 66049)]
NARROW_ARGS = [narrow_geo(s, 70) for s in ((100, 9), (256, 12), (1024, 16))]
NARROW_STRIDED = narrow_geo((100, 9), 70)
# (in the family, its neighbour outside, the passes that leave): N = 13, N = 17, K = 260, K = 1028, K = 12, K = 18
NARROW_LEAVING = [(narrow_geo((100, 12), 70), narrow_geo((100, 13), 70)), (narrow_geo((100, 16), 70), narrow_geo((100, 17), 70)),
                  (narrow_geo((256, 4), 70), narrow_geo((260, 4), 70)), (narrow_geo((1024, 4), 70), narrow_geo((1028, 4), 70)),
                  (narrow_geo((16, 9), 70), narrow_geo((12, 9), 70)), (narrow_geo((20, 9), 70), narrow_geo((18, 9), 70))]

SMALL = sorted(set(TINY_CASES + TINY_ARGS + TINY_STRIDED + PATCH_CASES + PATCH_LDS + NARROW_CASES + NARROW_ARGS +
                   [NARROW_STRIDED] + [g for pair in TINY_LEAVING + NARROW_LEAVING for g in pair] +
                   [tiny_geo((3, 3, 1), (2, 17, 19)), tiny_geo((4, 4, 1), (2, 5, 7)), COUT9_1X1, (2, 5, 7, 4, 8, 1, 1, 0, 1)]))
BIG = TINY_BIG + NARROW_BIG
KINDS = ["exact", "rounded"]


# ================================================================================================ operands and references
def aten(x, w, b, g, geo, dtype):
    """(y, dx, dw, db) of F.conv2d in `dtype` on the fp32 operands."""
    s, p, d = geo[6:]
    x, w, b = (t.to(dtype, copy=True).requires_grad_(True) for t in (x, w, b))
    y = F.conv2d(x, w, b, s, p, d)
    y.backward(g.to(dtype))
    return y.detach(), x.grad, w.grad, b.grad


def dist(a, b):
    """The metric of close() in tests/test_hip_ops.py."""
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    assert a.shape == b.shape, (a.shape, b.shape)
    return ((a - b).abs().max() / max(b.abs().max().item(), 1e-6)).item()


def conditioning(D):
    """The metric of dist() divides by an output's largest element.  sum |terms| / |sum| of THAT element, the largest over the four
    outputs: how many times the rounding of one partial sum of full magnitude is magnified in the metric."""
    a = lambda t: t.double().abs()
    outs = (D.y, D.dx, D.dw, D.db)
    mags = aten(a(D.x), a(D.w), a(D.b), a(D.g), D.geo, torch.float64)
    return max((m.flatten()[o.abs().argmax()] / o.abs().max()).item() for o, m in zip(outs, mags))


def build(geo, kind):
    """kind: "exact" (integers, see the module docstring), "exact1" ({-1, 0, 1}: the big maps; no old values) or "rounded"."""
    B, H, W, Ci, Co, k, s, p, d = geo
    OH, OW = out_hw(geo)
    shapes = dict(x=(B, Ci, H, W), w=(Co, Ci, k, k), b=(Co,), g=(B, Co, OH, OW), y0=(B, Co, OH, OW), dx0=(B, Ci, H, W),
                  dw0=(Co, Ci, k, k), db0=(Co,), rs=(Co,))
    if kind == "exact1":
        for name in ("y0", "dx0", "dw0", "db0", "rs"):
            del shapes[name]
    D = types.SimpleNamespace(kind=kind, geo=geo)
    if kind != "rounded":
        rng = np.random.default_rng(list(geo))
        for name, sh in shapes.items():
            m = 1 if kind == "exact1" else 3 if name in ("w", "b", "rs") else 2
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
    if kind == "rounded":
        D.d32 = max(dist(a, r) for a, r in zip(aten(D.x, D.w, D.b, D.g, geo, torch.float32), (D.y, D.dx, D.dw, D.db)))
        D.bound = 4 * max(D.d32, ULP_FLOOR)
    D.seen = 0.0
    return D


data = functools.lru_cache(maxsize=None)(build)          # the small cases; the big maps are built where they are used


def abs_bound(D):
    """The largest |partial sum| any order of summation can meet in any output of the case, accumulating forms included."""
    a = lambda t: t.double().abs()
    y, dx, dw, db = aten(a(D.x), a(D.w), a(D.b), a(D.g), D.geo, torch.float64)
    if D.kind == "exact1":
        return max(t.max().item() for t in (y, dx, dw, db))
    rs = max(1.0, a(D.rs).max().item())
    return max((y + a(D.y0)).max().item(), (dx + a(D.dx0)).max().item(), (rs * dw + a(D.dw0)).max().item(),
               (rs * db + a(D.db0)).max().item())


# ================================================================================================ tests that need no GPU
def test_exact_cases_stay_below_2_24():
    for geo in SMALL:
        assert abs_bound(data(geo, "exact")) < EXACT_LIMIT, geo


@pytest.mark.parametrize("geo", BIG, ids=str)
def test_exact_big_maps_stay_below_2_24(geo):
    assert abs_bound(build(geo, "exact1")) < EXACT_LIMIT


def test_rounded_bounds_stay_below_the_suite_tolerance():
    for geo in SMALL:
        D = data(geo, "rounded")
        assert D.cond <= COND_LIMIT, (geo, D.cond)          # a draw was found (see COND_LIMIT)
        assert ULP_FLOOR * 4 <= D.bound <= TOL, (geo, D.d32)


def test_tiny_cases_reach_the_paths_they_are_named_after():
    npix = lambda g: g[0] * g[1] * g[2]
    for geo in TINY_CASES + TINY_BIG + TINY_ARGS + TINY_STRIDED:
        assert families(geo) == (4, 4, 4), geo
        assert geo[7] == geo[8] * (geo[5] - 1) // 2
    reached = {tiny_wgrad_kernel(*g[3:6]) for g in TINY_CASES}
    assert reached == {"all", (4, 1), (8, 1), (4, 3), (8, 3)}
    assert {g[3:6] for g in TINY_CASES if tiny_wgrad_kernel(*g[3:6]) == "all"} == set(TINY_FIXED)
    for shape in TINY_FIXED:                    # the fixed shapes on every map, every shape on the two maps
        assert {g[:3] for g in TINY_CASES if g[3:6] == shape and g[8] == 1} == set(TINY_MAPS)
    for shape in TINY_GENERIC:
        assert {g[:3] for g in TINY_CASES if g[3:6] == shape and g[8] == 1} == {(2, 5, 7), (2, 17, 19)}
    assert all(m[0] >= 2 for m in TINY_MAPS if m != (1, 40, 41))
    assert 2 * 5 * 7 < 256                                                                        # fewer pixels than a workgroup
    assert tiny_blocks(2 * 17 * 19) == 3 and 2 * 17 * 19 % 256 != 0 and tiny_wgrad_plan(2 * 17 * 19) == (1, 646)
    assert tiny_wgrad_plan(40 * 41) == (2, 820)
    assert tiny_wgrad_plan(2 * 33 * 35)[0] == 3
    big = npix(TINY_BIG[0])
    assert big == 4196352 > 16384 * 256 and tiny_blocks(big) == 16384 and big < 2 ** 31          # the grid-stride loop
    assert big > 2048 * 1024 and tiny_wgrad_plan(big) == (2048, 2049)                             # the nblk cap, 2049 pixels per block
    assert {g[3:6] for g in TINY_BIG} == {(4, 4, 1), (4, 3, 3)}
    # dilation: (pad, dil) = (1, 1), (2, 2), (3, 3), (6, 6) on 5 x 7; at 6 all but the centre row of taps is outside the image
    for shape in TINY_FIXED + TINY_GENERIC:
        if shape[2] == 3:
            assert {(g[7], g[8]) for g in TINY_CASES if g[3:6] == shape and g[:3] == (2, 5, 7)} == {(1, 1), (2, 2), (3, 3), (6, 6)}
    # (a tap 6 rows away is outside for every y: 6 > H - 1 = 4; 6 columns away it is inside for x = 0 and x = 6 alone: 6 = W - 1)
    for inside, outside in TINY_LEAVING:
        assert families(inside) == (4, 4, 4) and 4 not in families(outside), (inside, outside)
    assert families(tiny_geo((4, 4, 1), (2, 5, 7)), plain=False)[:2] == (0, 0)                     # act = 1 is not "plain"


def test_patch_cases_reach_the_paths_they_are_named_after():
    for geo in PATCH_CASES:
        assert families(geo) == (0, 4, 0) and not tiny_shape(geo), geo
    assert {g[5] for g in PATCH_CASES} == {1, 2, 4}
    assert [patch_lds(g) for g in PATCH_LDS] == [59904, 60288]
    assert families(PATCH_LDS[0])[1] == 4 and families(PATCH_LDS[1])[1] == 0
    assert families(COUT9_1X1) == (0, 4, 0) and families((2, 5, 7, 4, 8, 1, 1, 0, 1)) == (4, 4, 4)


def test_narrow_cases_reach_the_paths_they_are_named_after():
    rows = lambda g: g[0] * g[1] * g[2]
    for geo in NARROW_CASES + NARROW_BIG + NARROW_ARGS + [NARROW_STRIDED]:
        want = (5, 5, 5) if (geo[3], geo[4]) not in NARROW_WGRAD_SHAPES else (0, 0, 5)
        assert families(geo) == want, geo
    # live quads below QP: 5 of 8, 9 of 16, 25 of 32, 63 of 64 lanes of a row group; 16 and 256 fill theirs
    assert [(K // 4,) + narrow_plan(K) for K, _ in NARROW_SHAPES] == [(4, 4, 64), (5, 8, 32), (9, 16, 16), (25, 32, 8), (63, 64, 4),
                                                                      (64, 64, 4)]
    assert [(K // 4,) + narrow_plan(K) for K, _ in NARROW_WGRAD_SHAPES] == [(65, 128, 2), (129, 256, 1), (255, 256, 1), (256, 256, 1)]
    assert narrow_wgrad_lds(1024, 16) == 65536 == narrow_wgrad_lds(16, 16)
    assert all(narrow_wgrad_lds(K, N) <= 65536 for K, N in NARROW_SHAPES + NARROW_WGRAD_SHAPES)
    for s in ((100, 9), (256, 12)):
        assert {rows(g) for g in NARROW_CASES if g[3:5] == s} == {1, 3, 7, 9, 70, 31, 32, 33, 33124}
    assert narrow_plan(100)[1] == 8                                  # 7, 9, 70 rows: around RL and RL * 8 + 6
    assert [narrow_wgrad_plan(M) for M in (31, 32, 33)] == [(32, 1), (32, 1), (32, 2)] and 33 - 32 == 1
    assert narrow_wgrad_plan(33124) == (33, 1004) and 33124 - 1003 * 33 == 25
    # rows r, r + RL, ... of a 33-row and of the 25-row split at RL = 8 (K = 100): 5 / 4 and 4 / 3 rows per thread -- the
    # two-rows-per-trip loop is left with and without a row for the single-row loop
    assert {len(range(r, n, 8)) % 2 for r in range(8) for n in (33,)} == {0, 1} == {len(range(r, 25, 8)) % 2 for r in range(8)}
    big = NARROW_BIG[0]
    assert rows(big) == 66049 > 2048 * narrow_plan(256)[1] * 8 and narrow_blocks(rows(big), 256) == 2048      # the grid-stride loop
    for inside, outside in NARROW_LEAVING:
        assert 5 in families(inside) and families(inside) != families(outside), (inside, outside)
    fams = [families(o) for _, o in NARROW_LEAVING]
    assert fams == [(0, 0, 5), (0, 0, 0), (0, 0, 5), (0, 0, 0), (0, 0, 0), (0, 0, 0)]
    assert families(NARROW_STRIDED, dls=True) == (5, 5, 0) and families(NARROW_STRIDED, aligned=False) == (0, 0, 0)


# ================================================================================================ running a case on the GPU
def family_is(hip, want, what):
    """want: a family (4, 5), -f for "any but f", None for an MFMA kernel whichever it is: neither 4 nor 5."""
    got = hip.last_kernel()
    if want is None:
        assert got not in (4, 5) and got > 0, f"{what}: kernel family {got}, expected an MFMA kernel"
    else:
        assert got == want if want > 0 else got != -want, f"{what}: kernel family {got}, expected {want}"


def agree(D, got, ref, what, direct=True):
    """Bit for bit on the exact operands; within the case's bound (TOL off the direct kernels) on the rounded ones."""
    got = got.detach().double().cpu()
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    if D.kind != "rounded":
        bad = got != ref
        assert not bool(bad.any()), f"{what} {D.geo}: {int(bad.sum())} of {ref.numel()} values differ from the exact result, first at " \
                                    f"{tuple(bad.nonzero()[0].tolist())}: {got[bad][0].item()} for {ref[bad][0].item()}"
        return
    e = dist(got, ref)
    print(f"  {D.geo} {what}: {e:.2e}")
    if direct:
        D.seen = max(D.seen, e)
    assert e <= (D.bound if direct else TOL), f"{what} {D.geo}: distance {e:.3e}, bound {D.bound:.3e} (d32 {D.d32:.3e})"


def want_of(geo, **kw):
    return tuple(f if f else None for f in families(geo, **kw))


def report(D):
    if D.kind == "rounded":
        print(f"DIRECT-CONV {D.geo}: draw {D.draw} cond {D.cond:.1f} d32 {D.d32:.2e} bound {D.bound:.2e} kernel {D.seen:.2e}")


def g12(geo):
    B, H, W, Ci, Co, k, s, p, d = geo
    OH, OW = out_hw(geo)
    return (B, H, W, Ci, OH, OW, Co, k, k, s, p, d)


def three_passes(hip, D, want, passes="fdw"):
    """Forward, data gradient and weight gradient on contiguous tensors, outputs pre-filled with PAT (an unwritten value shows)."""
    B, H, W, Ci, Co, k, s, p, d = D.geo
    OH, OW = out_hw(D.geo)
    xg, gg, wp, bg = nhwc(D.x), nhwc(D.g), pack(hip, D.w), D.b.cuda()
    if "f" in passes:
        y = pat(B, OH, OW, Co)
        hip.conv2d(xg, Ci, wp, bg, y, Co, *g12(D.geo))
        family_is(hip, want[0], "forward")
        agree(D, nchw(y), D.y, "forward", want[0] is not None and want[0] > 0)
    if "d" in passes:
        dx = pat(B, H, W, Ci)
        hip.conv2d(gg, Co, wp, None, dx, Ci, *g12(D.geo), mode=1)
        family_is(hip, want[1], "data gradient")
        agree(D, nchw(dx), D.dx, "data gradient", want[1] is not None and want[1] > 0)
    if "w" in passes:
        dw, db = pat(Co, Ci, k, k), pat(Co)
        hip.conv2d_wgrad(xg, Ci, gg, Co, dw, db, None, *g12(D.geo))
        family_is(hip, want[2], "weight gradient")
        direct = want[2] is not None and want[2] > 0
        agree(D, dw, D.dw, "weight gradient", direct)
        agree(D, db, D.db, "bias gradient", direct)
    report(D)


def argument_forms(hip, D, want, passes="fdw", y_slice=False):
    """bias = None; accumulate on the forward and on the data gradient; the weight gradient without dbias, with row_scale and
    accumulate, and twice with the same bits (its reduction order is fixed)."""
    B, H, W, Ci, Co, k, s, p, d = D.geo
    OH, OW = out_hw(D.geo)
    xg, gg, wp, bg = nhwc(D.x), nhwc(D.g), pack(hip, D.w), D.b.cuda()
    bc = lambda t: t.double()[None, :, None, None]
    if "f" in passes:
        y = pat(B, OH, OW, Co)
        hip.conv2d(xg, Ci, wp, None, y, Co, *g12(D.geo))
        family_is(hip, want[0], "forward")
        agree(D, nchw(y), D.y - bc(D.b), "forward, bias = None")
        ybuf, y = outp(nhwc(D.y0), "A") if y_slice else (None, nhwc(D.y0))
        hip.conv2d(xg, Ci, wp, bg, y, ld(y), *g12(D.geo), accumulate=1)
        family_is(hip, want[0], "forward")
        agree(D, nchw(y), D.y0.double() + D.y, "forward, accumulate")
        assert ybuf is None or guards_intact(ybuf, y), "forward, accumulate: guard columns of the output changed"
    if "d" in passes:
        dx = nhwc(D.dx0)
        hip.conv2d(gg, Co, wp, None, dx, Ci, *g12(D.geo), mode=1, accumulate=1)
        family_is(hip, want[1], "data gradient")
        agree(D, nchw(dx), D.dx0.double() + D.dx, "data gradient, accumulate")
    dw = pat(Co, Ci, k, k)
    hip.conv2d_wgrad(xg, Ci, gg, Co, dw, None, None, *g12(D.geo))
    family_is(hip, want[2], "weight gradient")
    agree(D, dw, D.dw, "weight gradient, dbias = None")
    dw, db = D.dw0.cuda(), D.db0.cuda()
    hip.conv2d_wgrad(xg, Ci, gg, Co, dw, db, D.rs.cuda(), *g12(D.geo), accumulate=1)
    family_is(hip, want[2], "weight gradient")
    agree(D, dw, D.dw0.double() + D.rs.double()[:, None, None, None] * D.dw, "weight gradient, row_scale + accumulate")
    agree(D, db, D.db0.double() + D.rs.double() * D.db, "bias gradient, row_scale + accumulate")
    twice = []
    for _ in range(2):
        dw, db = pat(Co, Ci, k, k), pat(Co)
        hip.conv2d_wgrad(xg, Ci, gg, Co, dw, db, None, *g12(D.geo))
        twice.append((dw, db))
    assert torch.equal(twice[0][0], twice[1][0]) and torch.equal(twice[0][1], twice[1][1]), "two weight gradients differ"
    report(D)


def strided_passes(hip, D, s, want):
    """The three passes with each pass's two strided operands in layouts s (tests/test_strided_rows.py: A an aligned slice of
    a wider row, B the base off by one float, C a ragged row stride): (a, y) of forward and data gradient, (x, dy) of the weight
    gradient.  Inputs sit in NaN, outputs in PAT with the guard columns checked.  want: a function of (pass, s)."""
    B, H, W, Ci, Co, k, st, p, d = D.geo
    OH, OW = out_hw(D.geo)
    wp, bg = pack(hip, D.w), D.b.cuda()
    xa = inp(nhwc(D.x), s[0], 0)
    buf, y = outp((B, OH, OW, Co), s[1], 1)
    hip.conv2d(xa, ld(xa), wp, bg, y, ld(y), *g12(D.geo))
    family_is(hip, want("f", s), f"forward {s}")
    agree(D, nchw(y), D.y, f"forward {s}", want("f", s) > 0)
    assert guards_intact(buf, y), f"forward {s}: guard columns of the output changed"
    ga = inp(nhwc(D.g), s[0], 0)
    buf, dx = outp((B, H, W, Ci), s[1], 1)
    hip.conv2d(ga, ld(ga), wp, None, dx, ld(dx), *g12(D.geo), mode=1)
    family_is(hip, want("d", s), f"data gradient {s}")
    agree(D, nchw(dx), D.dx, f"data gradient {s}", want("d", s) > 0)
    assert guards_intact(buf, dx), f"data gradient {s}: guard columns of the output changed"
    xv, gv = inp(nhwc(D.x), s[0], 0), inp(nhwc(D.g), s[1], 1)
    dw, db = pat(Co, Ci, k, k), pat(Co)
    hip.conv2d_wgrad(xv, ld(xv), gv, ld(gv), dw, db, None, *g12(D.geo))
    family_is(hip, want("w", s), f"weight gradient {s}")
    agree(D, dw, D.dw, f"weight gradient {s}", want("w", s) > 0)
    agree(D, db, D.db, f"bias gradient {s}", want("w", s) > 0)
    report(D)


# ================================================================================================ tiny family (4)
@gpu
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("geo", TINY_CASES, ids=str)
def test_tiny_conv(hip, geo, kind):
    three_passes(hip, data(geo, kind), (4, 4, 4))


@gpu
@pytest.mark.parametrize("geo", TINY_BIG, ids=str)
def test_tiny_conv_big_map(hip, geo):
    """4 196 352 pixels: the grid-stride loop of the forward / data-gradient kernels (16384 workgroups of 256), the weight
    gradient's cap of 2048 blocks with 2049 pixels each."""
    three_passes(hip, build(geo, "exact1"), (4, 4, 4))


@gpu
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("geo", TINY_ARGS, ids=str)
def test_tiny_conv_arguments(hip, geo, kind):
    argument_forms(hip, data(geo, kind), (4, 4, 4))


# vr_tiny_conv (tinyconv.hip):
#   const bool al = (lda != 4 || vr_aligned16(a)) && (ldy != 4 || vr_aligned16(y)) && (long)B * H * W < (1L << 31);
#   if (al && mode == 0) { ... conv_fixed_kernel<0, CK, CN, KS> for the four shapes ... } else if (al) { ... <1, ...> ... }
#   ... else conv_kernel<mode> (the generic one).
# and inside conv_fixed_kernel "if (CK == 4 && p.lda == 4)" / "if (CN == 4 && p.ldy == 4)" choose the 16-byte load / store.  So a
# fixed shape stays on conv_fixed_kernel in layouts A, B and C alike (lda, ldy = C + 12 ... C + 24 != 4), with scalar access;
# only a row stride of exactly 4 on a misaligned base reaches the generic kernel: test_tiny_conv_rows_of_four_off_alignment.
# vr_tiny_wgrad:
#   const int vec4 = Cin == 4 && ldx % 4 == 0 && vr_aligned16(x);
# layout A of x (ldx = 16, aligned) keeps the 16-byte load of wgrad_all_kernel<4, ..> / wgrad_kernel<4, ..>, B (base off by one
# float) and C (ldx = Cin + 5) clear vec4; dy is read one float at a time in every layout.  The family is 4 throughout.
@gpu
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("s", scenarios(2), ids=sid)
@pytest.mark.parametrize("geo", TINY_STRIDED, ids=str)
def test_tiny_conv_on_channel_slices(hip, geo, s, kind):
    strided_passes(hip, data(geo, kind), s, lambda which, s: 4)


def flat_view(t, fill):
    """t (B, H, W, C), or that shape (the view keeps the fill), as a view with row stride C whose base is one float past a
    16-byte boundary -> (buffer, view)."""
    shape = tuple(t) if isinstance(t, (tuple, torch.Size)) else tuple(t.shape)
    n = int(np.prod(shape))
    buf = torch.empty(n + 8, device="cuda")
    if isinstance(fill, int):
        buf.view(torch.int32).fill_(fill)
    else:
        buf.fill_(fill)
    v = buf[1:1 + n].view(shape)
    if isinstance(t, torch.Tensor):
        v.copy_(t)
    assert v.data_ptr() % 16 == 4 and v.stride(-2) == shape[-1]
    return buf, v


def flat_guards(buf, n):
    raw = buf.view(torch.int32)
    return bool((raw[:1] == PAT).all()) and bool((raw[1 + n:] == PAT).all())


@gpu
@pytest.mark.parametrize("kind", KINDS)
def test_tiny_conv_rows_of_four_off_alignment(hip, kind):
    """lda == 4 or ldy == 4 on a base that is not 16-byte aligned: `al` fails (source quoted above) and the generic kernel
    serves the fixed shapes.  4 -> 4 on contiguous rows one float off alignment, one operand at a time; 3 -> 3 on channels
    1..3 of a 4-wide buffer (lda = ldy = 4, base off by one float), channel 0 a guard."""
    D = data(tiny_geo((4, 4, 1), (2, 17, 19)), kind)
    B, H, W, Ci, Co, k, s, p, d = D.geo
    wp, bg = pack(hip, D.w), D.b.cuda()
    for off_a, off_y in ((True, False), (False, True)):
        for mode, src, ref, what in ((0, D.x, D.y, "forward"), (1, D.g, D.dx, "data gradient")):
            a = flat_view(nhwc(src), NAN)[1] if off_a else nhwc(src)
            buf, y = flat_view((B, H, W, 4), PAT) if off_y else (None, pat(B, H, W, 4))
            hip.conv2d(a, 4, wp, bg if mode == 0 else None, y, 4, *g12(D.geo), mode=mode)
            family_is(hip, 4, what)
            agree(D, nchw(y), ref, f"{what}, a off {off_a}, y off {off_y}")
            assert buf is None or flat_guards(buf, y.numel()), what + ": wrote outside the output"
    xv = flat_view(nhwc(D.x), NAN)[1]                      # weight gradient: ldx = 4, misaligned -> vec4 = 0
    dw, db = pat(Co, Ci, 1, 1), pat(Co)
    hip.conv2d_wgrad(xv, 4, nhwc(D.g), 4, dw, db, None, *g12(D.geo))
    family_is(hip, 4, "weight gradient")
    agree(D, dw, D.dw, "weight gradient, x off alignment")
    agree(D, db, D.db, "bias gradient, x off alignment")
    report(D)
    D = data(tiny_geo((3, 3, 1), (2, 17, 19)), kind)
    wp, bg = pack(hip, D.w), D.b.cuda()
    for mode, src, ref, what in ((0, D.x, D.y, "forward"), (1, D.g, D.dx, "data gradient")):
        a4 = torch.full((B, H, W, 4), NAN, device="cuda")
        a4[..., 1:] = nhwc(src)
        y4 = pat(B, H, W, 4)
        hip.conv2d(a4[..., 1:], 4, wp, bg if mode == 0 else None, y4[..., 1:], 4, *g12(D.geo), mode=mode)
        family_is(hip, 4, what)
        agree(D, nchw(y4[..., 1:]), ref, what + ", channels 1..3 of 4")
        assert bool((y4.view(torch.int32)[..., 0] == PAT).all()), what + ": channel 0 of the output changed"
    x4 = torch.full((B, H, W, 4), NAN, device="cuda")
    x4[..., 1:] = nhwc(D.x)
    dw, db = pat(3, 3, 1, 1), pat(3)
    hip.conv2d_wgrad(x4[..., 1:], 4, nhwc(D.g), 3, dw, db, None, *g12(D.geo))
    family_is(hip, 4, "weight gradient")
    agree(D, dw, D.dw, "weight gradient, channels 1..3 of 4")
    agree(D, db, D.db, "bias gradient, channels 1..3 of 4")
    report(D)


# ------------------------------------------------------------------------------------------------ patch data gradient
@gpu
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("geo", PATCH_CASES + PATCH_LDS, ids=str)
def test_patch_data_gradient(hip, geo, kind):
    """k == stride, pad 0, Cin <= 8 -> patch_dgrad_kernel (family 4) while its weights fit 60 000 bytes of LDS; forward and
    weight gradient of these shapes run on the MFMA kernels."""
    three_passes(hip, data(geo, kind), want_of(geo))


@gpu
@pytest.mark.parametrize("kind", KINDS)
def test_nine_outputs_at_1x1_leave_the_tiny_family_but_for_the_data_gradient(hip, kind):
    """4 -> 8 (1 x 1) is tiny in all three passes; 4 -> 9 runs forward and weight gradient on MFMA kernels, and its data
    gradient, k == stride == 1 with Cin <= 8, on patch_dgrad_kernel: family 4 again."""
    three_passes(hip, data((2, 5, 7, 4, 8, 1, 1, 0, 1), kind), (4, 4, 4))
    three_passes(hip, data(COUT9_1X1, kind), (None, 4, None))


# vr_patch_dgrad / patch_dgrad_kernel read dy and write dx one float at a time: every layout is served by the one kernel.
@gpu
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("geo", PATCH_CASES, ids=str)
def test_patch_data_gradient_accumulate_and_channel_slices(hip, geo, kind):
    D = data(geo, kind)
    B, H, W, Ci, Co, k, st, p, d = geo
    wp = pack(hip, D.w)
    for s in scenarios(2):                      # dy, dx
        gv = inp(nhwc(D.g), s[0], 0)
        for old, ref, what in ((None, D.dx, "patch data gradient"), (D.dx0, D.dx0.double() + D.dx, "patch data gradient, accumulate")):
            buf, dx = outp((B, H, W, Ci) if old is None else nhwc(old), s[1], 1)
            hip.conv2d(gv, ld(gv), wp, None, dx, ld(dx), *g12(geo), mode=1, accumulate=0 if old is None else 1)
            family_is(hip, 4, what)
            agree(D, nchw(dx), ref, f"{what} {s}")
            assert guards_intact(buf, dx), f"{what} {s}: guard columns of the output changed"
    report(D)


# ------------------------------------------------------------------------------------------------ leaving the tiny family
@gpu
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("inside,outside", TINY_LEAVING, ids=str)
def test_neighbours_of_the_tiny_family(hip, inside, outside, kind):
    three_passes(hip, data(inside, kind), (4, 4, 4))
    three_passes(hip, data(outside, kind), want_of(outside))


@gpu
@pytest.mark.parametrize("kind", KINDS)
def test_an_activation_leaves_the_tiny_family(hip, kind):
    """act = 1 (ReLU in the epilogue) is not "plain": 4 -> 4 1 x 1 runs on an MFMA kernel, with the plain call beside it."""
    D = data(tiny_geo((4, 4, 1), (2, 5, 7)), kind)
    B, H, W, Ci, Co, k, s, p, d = D.geo
    xg, wp, bg = nhwc(D.x), pack(hip, D.w), D.b.cuda()
    y = pat(B, H, W, Co)
    hip.conv2d(xg, Ci, wp, bg, y, Co, *g12(D.geo))
    family_is(hip, 4, "plain")
    agree(D, nchw(y), D.y, "plain")
    y = pat(B, H, W, Co)
    hip.conv2d(xg, Ci, wp, bg, y, Co, *g12(D.geo), act=1)
    family_is(hip, -4, "act = 1")
    agree(D, nchw(y), torch.relu(D.y), "act = 1", direct=False)


# ================================================================================================ narrow family (5)
@gpu
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("geo", NARROW_CASES, ids=str)
def test_narrow_conv(hip, geo, kind):
    want = families(geo)
    three_passes(hip, data(geo, kind), want_of(geo), "fdw" if want[0] == 5 else "w")


@gpu
@pytest.mark.parametrize("geo", NARROW_BIG, ids=str)
def test_narrow_conv_big_map(hip, geo):
    """66 049 rows of 256 channels: more than 2048 workgroups x RL = 4 rows x 8 passes, the forward / data-gradient grid-stride
    loop runs."""
    three_passes(hip, build(geo, "exact1"), (5, 5, 5))


@gpu
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("geo", NARROW_ARGS, ids=str)
def test_narrow_conv_arguments(hip, geo, kind):
    """The forward accumulates into a channel slice of a wider NHWC buffer (the NCHW store: test_narrow_conv_head_layout)."""
    want = families(geo)
    argument_forms(hip, data(geo, kind), want_of(geo), "fdw" if want[0] == 5 else "w", y_slice=True)


# vrnet_conv2d_f32 (igemm.hip): the narrow kernels need
#   ... vr_narrow_conv_ok(...) && ... && vr_aligned16(w) &&
#   (mode == 0 ? (lda % 4 == 0 && vr_aligned16(a)) : (!out_nchw && ldy % 4 == 0 && vr_aligned16(y)))
# -- the operand they move as float4: a in the forward, y (= dx) in the data gradient.  vrnet_conv2d_wgrad_f32:
#   ... && vr_narrow_wgrad_ok(...) && ldx % 4 == 0 && vr_aligned16(x)
# Layout A of that operand stays family 5; B (base off by one float) and C (ld = K + 5) leave for an MFMA kernel.  The other
# operand (the forward's y, dy of both gradients) is read or written one float at a time: any layout, family 5.
def narrow_want(which, s):
    return 5 if s[{"f": 0, "d": 1, "w": 0}[which]] == "A" else -5


@gpu
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("s", scenarios(2), ids=sid)
def test_narrow_conv_on_channel_slices(hip, s, kind):
    strided_passes(hip, data(NARROW_STRIDED, kind), s, narrow_want)


@gpu
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("inside,outside", NARROW_LEAVING, ids=str)
def test_neighbours_of_the_narrow_family(hip, inside, outside, kind):
    for geo in (inside, outside):
        three_passes(hip, data(geo, kind), want_of(geo))


@gpu
@pytest.mark.parametrize("kind", KINDS)
def test_a_layer_scale_gradient_leaves_the_narrow_family(hip, kind):
    """dls given: the weight gradient runs on the MFMA kernel whose slabs the layer-scale dot reads; without it, family 5.
    dls[n] = sum_c w[n][c] dw[n][c] + bias[n] db[n] (include/vrnet_hip.h)."""
    D = data(NARROW_STRIDED, kind)
    B, H, W, Ci, Co, k, s, p, d = D.geo
    xg, gg = nhwc(D.x), nhwc(D.g)
    for with_dls in (False, True):
        dw, db, dls = pat(Co, Ci, 1, 1), pat(Co), pat(Co)
        kw = dict(w=D.w.cuda(), bias=D.b.cuda(), dls=dls) if with_dls else {}
        hip.conv2d_wgrad(xg, Ci, gg, Co, dw, db, None, *g12(D.geo), **kw)
        family_is(hip, -5 if with_dls else 5, f"weight gradient, dls {with_dls}")
        agree(D, dw, D.dw, "weight gradient", not with_dls)
        agree(D, db, D.db, "bias gradient", not with_dls)
    agree(D, dls, (D.w.double() * D.dw).sum((1, 2, 3)) + D.b.double() * D.db, "layer-scale gradient", direct=False)


# ================================================================================================ refusals
@gpu
def test_conv_refuses_rows_shorter_than_the_channel_count(hip):
    """A row stride below the channel count makes the last row reach past a buffer of rows x ld floats: refused on the host for
    every kernel family (RuntimeError naming the entry point, nothing launched, outputs untouched)."""
    def fwd_like(geo, mode, short_a, short_y):
        B, H, W, Ci, Co, k, s, p, d = geo
        OH, OW = out_hw(geo)
        ca, cy, ra, ry = (Ci, Co, (B, H, W), (B, OH, OW)) if mode == 0 else (Co, Ci, (B, OH, OW), (B, H, W))
        a, y, w = torch.zeros(*ra, ca, device="cuda"), pat(*ry, cy + 4), torch.zeros(k * k, Co, Ci, device="cuda")
        refused("conv2d: row stride smaller than channel count", lambda: hip.conv2d(a, short_a, w, None, y, cy + 4, *g12(geo), mode=mode), y)
        refused("conv2d: row stride smaller than channel count", lambda: hip.conv2d(a, ca, w, None, y, short_y, *g12(geo), mode=mode), y)

    def wgrad(geo, short_x, short_dy):
        B, H, W, Ci, Co, k, s, p, d = geo
        OH, OW = out_hw(geo)
        x, dy = torch.zeros(B, H, W, Ci, device="cuda"), torch.zeros(B, OH, OW, Co, device="cuda")
        dw, db = pat(Co, Ci, k, k), pat(Co)
        refused("conv2d_wgrad: row stride smaller than channel count", lambda: hip.conv2d_wgrad(x, short_x, dy, Co, dw, db, None, *g12(geo)), dw, db)
        refused("conv2d_wgrad: row stride smaller than channel count", lambda: hip.conv2d_wgrad(x, Ci, dy, short_dy, dw, db, None, *g12(geo)), dw, db)

    tiny, patch = tiny_geo((4, 4, 1), (2, 5, 7)), patch_geo((5, 64, 4))
    narrow, mfma = narrow_geo((100, 9), 70), (2, 5, 7, 64, 48, 1, 1, 0, 1)
    assert families(tiny) == (4, 4, 4) and families(patch)[1] == 4 and families(narrow)[2] == 5 and families(mfma) == (0, 0, 0)
    fwd_like(tiny, 0, 3, 3)                     # tiny forward and data gradient
    fwd_like(tiny, 1, 3, 3)
    fwd_like(patch, 1, 60, 4)                   # patch data gradient: a = dy (64 channels), y = dx (5)
    fwd_like(narrow, 0, 96, 8)                  # the narrow and MFMA paths refused before: still do
    fwd_like(mfma, 0, 60, 44)
    wgrad(tiny, 3, 3)
    wgrad(narrow, 96, 8)
    wgrad(mfma, 60, 44)
