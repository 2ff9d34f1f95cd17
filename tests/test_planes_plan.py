"""The plane kernels of csrc/pgemm.hip at every edge of their plans: pgemm_kernel<3> / <1> (vrnet_gemm_planes_f32, kernel families 10
and 11), pwgrad_kernel<3> / <1> (vrnet_wgrad_planes_f32, families 12 and 13) and the two split kernels.  tests/test_planes_gemm.py
stays the suite at workload shapes; this file is about the loop shapes, masks, tile maps and plane pairs.

Which plan a case reaches is not taken on trust.  The tests without a gpu mark restate the launchers' integer rules in Python
(pwgrad_plan, the workgroup -> (split, tile) and workgroup -> (row tile, column tile) maps, the three loops over the 32-deep
stages, the workspace size, the two _ok queries, the split kernels' block count) and require, for every case of the tables
and both np, that the restatement equals the library's own host-side answer (hip.wgrad_planes_plan, the query over the
function the launcher plans with; vrnet_wgrad_planes_workspace; the _ok queries).  Each case records its coverage facts, and
the union over a table must hold the complete list of edges (REQUIRED_*): a later plan change that moves a case off its edge
fails there, on the CPU.

Two kinds of operands:

  exact    ("plane-exact") the operand PLANES are written directly, not through a split: each of the np planes of either
           operand is an independent draw of integers in {-2..2} (exact in bf16) -- the kernels do not need the planes to be a
           valid split of anything.  Expected: the sum over the six plane pairs with i + j <= 2 (np = 1: the one product) of
           A_i B_j^T, evaluated in fp64, where every partial sum is an integer far below 2^53, i.e. the int64 result.  Bias, res,
           res_scale, old y / dw, row_scale, w come from {-3..3}.  Every partial sum a kernel can form, in any order, is an
           integer below 2^24 (test_exact_operands_stay_below_2_24: 6 * 4 * K plus the epilogue's integers; 6 * 4 * M times the
           row scale), so every output must equal the expectation bit for bit.  A dropped plane product, a1b2 for a1b1, or a
           plane read at a wrong stride changes integers here; on a split fp32 tensor it would change the 2^-14 .. 2^-16 part
           of the result.  The nine-pair tests pin the scheme itself: with only plane i of one operand and plane j of the other
           non-zero the result is that one product if i + j <= 2 and exactly zero otherwise.
  rounded  rnd(...) operands put on planes by hip.planes_from_f32, redrawn until the fp64 reference is well conditioned
           (COND_LIMIT / MAX_DRAWS of tests/test_direct_conv.py; no case needs a redraw).  Reference: fp64 ATen on the CPU;
           d32 = fp32 CPU ATen against it on the same operands (np = 1: both on the operands rounded with .bfloat16()).
           np = 3, element by element: 4 * max(d32, ULP_FLOOR) * max |ref| + 2^-20 * (|A| |B|^T)[e], the second term the bias
           csrc/x6.h derives for the dropped plane products; np = 1: 4 * max(d32, ULP_FLOOR) in the metric of dist().  The
           weight gradient takes the data, the bounds and the dls allowance of tests/test_wgrad_plan.py at precision 2 (np = 3)
           and 1 (np = 1).  An epilogue behind the product (ReLU, res + res_scale * v, accumulate) scales that allowance by
           |res_scale| and adds 2 u of every magnitude it adds or multiplies (one rounding each, doubled).  GELU and aux
           (x gelu') outputs, whose fp32 evaluation of erf is not part of that budget, are held to the suite's 2e-5 in the metric
           of dist(); the pre-activation beside them to the element bound.  The kernels' own output never sets a bound.

Guards on every call: operand planes lie 16 bytes into their allocations with bf16 NaN in every pad column (ld > K), in 128
rows behind the last row and in the slack between planes; outputs lie 16 bytes into allocations pre-filled with NaN and, in a
second run, with PAT: both runs must give the same bits, every pad column and every row at or beyond M must keep the pre-fill,
and so must the statistics pairs of row blocks at or beyond M.  The weight gradient's workspace is exactly
vrnet_wgrad_planes_workspace bytes, poisoned with NaN and then with a finite number (same bits), followed by a 4 KB guard; one
byte less is refused.

The 48 MB slab bound of pwgrad_plan: it never binds for channel counts up to 2048 on either side (the network's largest layer
is 2048 x 512), whatever M (test_slab_bound_sweep).  Beyond that it CAN bind, at np = 1 only: the plan asks for
ceil(512 / tiles) = 2 splits at 257 .. 511 tiles, the bound allows floor(12.58M / (Cout Cin)) = 1 once Cout * Cin > 6.29M
(more than 24 MB of dW), e.g. 2560 x 2560 -- S = 1 where the plan wanted 2.  At np = 3 (256 workgroups) it cannot: two splits
need <= 255 tiles, at most 4.2M elements.  No GPU case is made for it: 26 MB of weight gradient is not an edge of this network.

Measured on an MI355X (the tests print every figure); every exact case, both nine-pair tests and every guard hold bit for bit:
  GEMM, 30 shapes x the forms they run: d32 1.1e-7 .. 7.8e-7 (np = 3) and 7.0e-8 .. 3.8e-7 (np = 1), so the bound is its floor,
        3.8e-6, everywhere; the kernels' largest distance per case 6.7e-8 .. 2.6e-7 (np = 3) and 5.9e-8 .. 1.3e-7 (np = 1); the
        largest share of its bound that any element used: 0.222 (np = 3) and 0.218 (np = 1), both in the res + res_scale form
        of (1025, 260, 160); GELU and aux outputs 9.6e-8 .. 2.7e-7 against their 2e-5.
  wgrad, 11 shapes: d32 2.9e-7 .. 4.3e-6, bounds 3.8e-6 .. 1.7e-5; the kernels' largest distance per case 1.4e-7 .. 3.1e-7
        (np = 3) and 9.4e-8 .. 2.4e-7 (np = 1), at most 0.056 / 0.034 of the case's bound; the largest share of its element's
        bound at np = 3: 0.025 (the 300-row case); dls used at most 0.004 of its allowance.
  With a1b2 in place of a1b1 in the kernels' six products every exact np = 3 case and both nine-pair tests fail, while the
  rounded cases and tests/test_planes_gemm.py still pass: that product is below what any tolerance on split fp32 data sees.
  With every statistics pair stored at the neighbouring column block every case with statistics fails, exact and rounded,
  while the grand totals of tests/test_planes_gemm.py still pass."""
import functools
import types

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests.test_direct_conv import COND_LIMIT, EXACT_LIMIT, MAX_DRAWS, ULP_FLOOR, agree, aten, cdiv, conditioning, dist
from tests.test_hip_ops import nhwc, rnd
from tests.test_strided_rows import NAN, PAT
from tests.test_wgrad_plan import bf, build as wgrad_build, dls_allowance, dls_of, held, x6_allowance

gpu = pytest.mark.gpu
U = 2.0 ** -24
Plan = types.SimpleNamespace
D64 = lambda t: t.detach().double().cpu()


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


# ================================================================================================ the launchers' integer rules
SLAB_CAP = 48 << 20
NST = 3                                  # PG_NST: stages of the LDS ring


def pwgrad_plan(M, Cin, Cout, np_, cap=SLAB_CAP):
    """pgemm.hip: pwgrad_plan -> nt, ct, S, rows, grid; wanted: the splits before the slab bound."""
    nt, ct = cdiv(Cout, 128), cdiv(Cin, 128)
    tiles = nt * ct
    target = 512 if np_ == 1 else 256                      # workgroups: two per CU at np = 1, one at np = 3
    s = 8 * (target // (8 * tiles))                        # multiples of 8: a split's tiles share an XCD
    if s < 8:
        s = cdiv(target, tiles)
    wanted = min(s, cdiv(M, 128))
    s = max(min(wanted, cap // (Cout * Cin * 4)), 1)
    rows = cdiv(cdiv(M, s), 32) * 32
    S = cdiv(M, rows)
    return Plan(nt=nt, ct=ct, S=S, rows=rows, grid=8 * cdiv(S, 8) * tiles, wanted=wanted)


def pwgrad_map(p):
    """pwgrad_kernel: workgroup L -> (split, n-tile, c-tile), or None for the workgroups that pad the splits to eights."""
    tiles, out = p.nt * p.ct, []
    for L in range(p.grid):
        j = L >> 3
        split, tile = (j // tiles) * 8 + (L & 7), j % tiles
        out.append(None if split >= p.S else (split, tile // p.ct, tile % p.ct))
    return out


def workspace(M, Cin, Cout):
    """pgemm.hip: vrnet_wgrad_planes_workspace (the np = 1 plan has the most splits)."""
    S = pwgrad_plan(M, Cin, Cout, 1).S
    return (S * (Cout * Cin + Cout) + Cout * Cin + Cout) * 4 + 256


def wgrad_ok(M, Cin, Cout):
    return M >= 256 and Cin >= 64 and Cout >= 64 and Cin % 8 == 0 and Cout % 8 == 0


def gemm_ok(rows, cols, K):
    return K % 32 == 0 and K >= 32 and cols >= 96 and cols % 4 == 0 and cdiv(rows, 128) * cdiv(cols, 128) >= 96


def split_blocks(R, K):
    return cdiv(R, 32) * cdiv(K, 64)


def pgemm_map(M, N):
    """pgemm_kernel: GT and workgroup L -> (row tile, column tile), or None where the row tiles are padded to eights."""
    MT, NT = cdiv(M, 128), cdiv(N, 128)
    GT, out = 8 * cdiv(MT, 8) * NT, []
    for L in range(GT):
        nt, mt = (L >> 3) % NT, ((L >> 3) // NT) * 8 + (L & 7)
        out.append(None if mt >= MT else (mt, nt))
    return MT, NT, GT, out


def loop_shape(nsteps):
    """The np = 3 loops over the stages (both kernels): (step_main pairs, step_tail pairs, an odd last step_tail)."""
    s = main = tail = 0
    while s + 2 + NST <= nsteps:
        main, s = main + 1, s + 2
    while s + 1 < nsteps:
        tail, s = tail + 1, s + 2
    return main, tail, int(s < nsteps)


def wgrad_facts(case, np_):
    M, Ci, Co = case
    p = pwgrad_plan(M, Ci, Co, np_)
    last = M - (p.S - 1) * p.rows
    return Plan(S=p.S, stages=p.rows // 32 if p.S > 1 else cdiv(last, 32), last_rows=last, last_stages=cdiv(last, 32),
                live=last - 32 * (cdiv(last, 32) - 1), nt=p.nt, ct=p.ct, n_live=Co - 128 * (p.nt - 1), c_live=Ci - 128 * (p.ct - 1),
                idle=p.grid - p.S * p.nt * p.ct)


def gemm_facts(case):
    M, N, K = case
    MT, NT, GT, tiles = pgemm_map(M, N)
    return Plan(stages=K // 32, loops=loop_shape(K // 32), MT=MT, NT=NT, idle=GT - MT * NT, m_live=M - 128 * (MT - 1), n_live=N - 128 * (NT - 1))


# ================================================================================================ the cases
# ---- vrnet_gemm_planes_f32: (M, N, K)
GEMM_STAGES = [(200, 132, 32 * k) for k in range(1, 10)]
# 1 .. 9 stages on two row tiles (the second: 72 live rows, its wm = 1 waves hold 8) and two column tiles (the second: 4 live
# columns): prologue only (1), tail pairs (2, 4), tail pair + odd step (3), main then tail (6, 8), main, tail, odd step (5, 7, 9)
GEMM_ROWS = [(M, 132, 96) for M in (1, 31, 32, 33, 127, 128, 129, 1023, 1025)]
# one row; a row block short of / at / past 32 and 128; MT = 8 (1023: 127 live rows in the last) and MT = 9 (1025: one live
# row in the ninth tile, the grid padded to 16 row tiles: seven idle workgroups per column tile)
GEMM_COLS = [(200, N, 64) for N in (4, 28, 32, 36, 60, 64, 68, 124, 128, 132, 260)]
# one column quad; around the 32- and 64-column blocks of a wave; a 4-column tail behind 128 and 256; NT = 1, 2, 3
GEMM_EDGES = list(dict.fromkeys(GEMM_STAGES + GEMM_ROWS + GEMM_COLS))
GEMM_FORM_SHAPES = [(224, 132, 96), (1025, 260, 160)]          # the first on tight rows (ld == the width, as the program calls)
GEMM_ALL = list(dict.fromkeys(GEMM_EDGES + GEMM_FORM_SHAPES))
PAIR_GEMM = (200, 132, 96)

REQUIRED_GEMM = dict(
    loops={(0, 0, 1), (0, 1, 0), (0, 1, 1), (0, 2, 0), (1, 1, 1), (1, 2, 0), (2, 1, 1), (2, 2, 0), (3, 1, 1)},
    MT={1, 2, 8, 9}, NT={1, 2, 3},
    m_live={1, 31, 32, 33, 72, 127, 128}, n_live={4, 28, 32, 36, 60, 64, 68, 124, 128})

# ---- vrnet_wgrad_planes_f32: (M, Cin, Cout); the comment: the np = 3 plan | the np = 1 plan where it differs
WGRAD_CASES = [
    (256, 64, 64),            # the smallest accepted shape: S 2 x 4 stages
    (257, 64, 72),            # S 3 x 3 stages, last split ONE row; 72 channels = one unit into the second 64-channel half
    (300, 136, 104),          # ct 2 with 8 live channels in the second c-tile; S 3, last split 44 rows = 2 stages, 12 live rows
    (8193, 128, 128),         # S 65: the grid padded to 72 (seven idle workgroups), last split ONE row
    (1000, 264, 136),         # nt 2, ct 3 (8 live channels in the last of each), S 8; the bias gradient only from ct = 0
    (40000, 64, 64),          # S 250 x 5 stages: main loop + odd tail, S % 8 = 2 | S 313 x 4 stages, last split 64 rows
    (28672, 136, 64),         # S 128 x 7 stages | S 224 x 4
    (12288, 136, 136),        # S 64 x 6 stages | S 96 x 4
    (2000, 1280, 320),        # S 8 x 8 stages, last split 208 rows = 7 stages (16 live rows) | S 16 x 4, last 80 rows = 3 stages
    (3000, 640, 640),         # S 8 x 12 stages, last split 312 rows = 10 stages | S 16 x 6 stages, last 120 rows = 4 stages
    (20000, 128, 264),        # nt 3, S 79 x 8 stages, last split 32 rows = one full stage | S 157 x 4
]
PAIR_WGRAD = (300, 136, 104)

REQUIRED_WGRAD = {
    3: dict(stages={3, 4, 5, 6, 7, 8, 12}, last_stages={1, 2, 3, 4, 5, 6, 7, 10}, live={1, 12, 16, 24, 32}),
    1: dict(stages={3, 4, 6}, last_stages={1, 2, 3, 4}, live={1, 12, 16, 24, 32}),
}


# ================================================================================================ tests that need no GPU
def test_restatement_is_the_librarys_plan(lib):
    """Every case, both np: the restated plan == vrnet_wgrad_planes_plan, the workspace and the two _ok queries."""
    for case in WGRAD_CASES + [PAIR_WGRAD, (288, 96, 128)]:
        M, Ci, Co = case
        for np_ in (3, 1):
            p = pwgrad_plan(M, Ci, Co, np_)
            assert lib.wgrad_planes_plan(M, Ci, Co, np_) == (p.nt, p.ct, p.S, p.rows), (case, np_)
            assert p.rows % 32 == 0 and (p.S - 1) * p.rows < M <= p.S * p.rows
            live = [w for w in pwgrad_map(p) if w is not None]
            assert sorted(live) == [(s, n, c) for s in range(p.S) for n in range(p.nt) for c in range(p.ct)], (case, np_)
            assert p.S == pwgrad_plan(M, Ci, Co, np_, cap=1 << 60).S           # (the slab bound does not bind)
        assert pwgrad_plan(M, Ci, Co, 1).S >= pwgrad_plan(M, Ci, Co, 3).S                                 # what the workspace relies on
        assert lib.wgrad_planes_workspace(M, Ci, Co) == workspace(M, Ci, Co), case
        assert lib.wgrad_planes_ok(M, Ci, Co) and wgrad_ok(M, Ci, Co), case
    for case in GEMM_ALL:
        assert lib.gemm_planes_ok(*case) == gemm_ok(*case), case
        MT, NT, GT, tiles = pgemm_map(case[0], case[1])
        assert sorted(t for t in tiles if t is not None) == [(m, n) for m in range(MT) for n in range(NT)], case
    # the stale comment of tests/test_planes_gemm.py beside (288, 96, 128): three splits of 96 rows, three stages each
    assert lib.wgrad_planes_plan(288, 96, 128, 3) == (1, 1, 3, 96)
    with pytest.raises(RuntimeError, match="wgrad_planes_plan: bad arguments"):
        lib.wgrad_planes_plan(256, 64, 64, 2)
    with pytest.raises(RuntimeError, match="wgrad_planes_plan: bad arguments"):
        lib.wgrad_planes_plan(0, 64, 64, 3)


def test_ok_queries_at_their_thresholds(lib):
    G = [(95 * 128, 128, 64, False), (95 * 128 + 1, 128, 64, True), (96 * 128, 128, 64, True),          # 95 and 96 tiles
         (48 * 128, 132, 64, True), (48 * 128 - 1, 132, 64, True), (47 * 128, 256, 64, False),           # ... over two column tiles
         (1 << 20, 92, 64, False), (1 << 20, 96, 64, True), (1 << 20, 98, 64, False), (1 << 20, 100, 64, True),      # cols 92 / 96, % 4
         (1 << 20, 128, 32, True), (1 << 20, 128, 48, False), (1 << 20, 128, 0, False), (1 << 20, 128, 96, True)]   # K % 32
    for rows, cols, K, want in G:
        assert gemm_ok(rows, cols, K) == want == lib.gemm_planes_ok(rows, cols, K), (rows, cols, K)
    Wg = [(255, 64, 64, False), (256, 64, 64, True), (256, 56, 64, False), (256, 64, 56, False), (256, 64, 68, False),
          (256, 68, 64, False), (256, 72, 64, True), (256, 64, 72, True), (1 << 20, 60, 60, False)]
    for M, Ci, Co, want in Wg:
        assert wgrad_ok(M, Ci, Co) == want == lib.wgrad_planes_ok(M, Ci, Co), (M, Ci, Co)
    for R, K in ((1, 1), (32, 64), (33, 64), (32, 65), (37, 12), (320, 96), (70, 130)):
        assert split_blocks(R, K) == lib.planes_split_blocks(R, K)


def test_wgrad_cases_reach_the_edges_they_are_named_after():
    """The comments of WGRAD_CASES, asserted, and the union the table must keep."""
    f = {(c, n): wgrad_facts(c, n) for c in WGRAD_CASES for n in (3, 1)}
    key = lambda c, n: (f[c, n].S, f[c, n].stages, f[c, n].last_rows, f[c, n].last_stages, f[c, n].live)
    g = iter(WGRAD_CASES)
    c = next(g); assert key(c, 3) == key(c, 1) == (2, 4, 128, 4, 32)
    c = next(g); assert key(c, 3) == key(c, 1) == (3, 3, 65, 3, 1) and f[c, 3].n_live == 72
    c = next(g); assert key(c, 3) == key(c, 1) == (3, 4, 44, 2, 12) and (f[c, 3].nt, f[c, 3].ct, f[c, 3].c_live, f[c, 3].n_live) == (1, 2, 8, 104)
    c = next(g); assert key(c, 3) == key(c, 1) == (65, 4, 1, 1, 1) and f[c, 3].idle == 7
    c = next(g); assert key(c, 3) == key(c, 1) == (8, 4, 104, 4, 8) and (f[c, 3].nt, f[c, 3].ct, f[c, 3].n_live, f[c, 3].c_live) == (2, 3, 8, 8)
    c = next(g); assert key(c, 3) == (250, 5, 160, 5, 32) and loop_shape(5) == (1, 1, 1) and key(c, 1) == (313, 4, 64, 2, 32)
    assert f[c, 3].S % 8 == 2 and f[c, 1].S % 8 == 1
    c = next(g); assert key(c, 3) == (128, 7, 224, 7, 32) and loop_shape(7) == (2, 1, 1) and key(c, 1)[:2] == (224, 4)
    c = next(g); assert key(c, 3) == (64, 6, 192, 6, 32) and loop_shape(6) == (1, 2, 0) and key(c, 1)[:2] == (96, 4)
    c = next(g); assert key(c, 3) == (8, 8, 208, 7, 16) and key(c, 1) == (16, 4, 80, 3, 16) and (f[c, 3].nt, f[c, 3].ct) == (3, 10)
    c = next(g); assert key(c, 3) == (8, 12, 312, 10, 24) and key(c, 1) == (16, 6, 120, 4, 24) and (f[c, 3].nt, f[c, 3].ct) == (5, 5)
    c = next(g); assert key(c, 3) == (79, 8, 32, 1, 32) and key(c, 1)[:2] == (157, 4) and (f[c, 3].nt, f[c, 3].n_live) == (3, 8)
    assert next(g, None) is None and len(set(WGRAD_CASES)) == len(WGRAD_CASES)
    for n in (3, 1):
        got = lambda name: {getattr(f[c, n], name) for c in WGRAD_CASES}
        for name, want in REQUIRED_WGRAD[n].items():
            assert got(name) >= want, (n, name, sorted(want - got(name)))
        assert max(got("stages")) >= 9 or n == 1                          # np = 3: a split of nine or more stages
        assert {1, 2, 3} <= got("last_stages") and max(got("last_stages")) >= 4
        assert {1, 32} <= got("live") and any(1 < v < 32 for v in got("live"))
        assert {s % 8 == 0 for s in got("S")} == {True, False} and min(got("S")) < 8 and got("idle") >= {0, 7}
        assert got("nt") == {1, 2, 3, 5} and {1, 2, 3} <= got("ct")
        assert 8 in got("n_live") and 8 in got("c_live")


def test_gemm_cases_reach_the_edges_they_are_named_after():
    facts = [gemm_facts(c) for c in GEMM_EDGES]
    assert [gemm_facts(c).loops for c in GEMM_STAGES] == [(0, 0, 1), (0, 1, 0), (0, 1, 1), (0, 2, 0), (1, 1, 1), (1, 2, 0), (2, 1, 1),
                                                         (2, 2, 0), (3, 1, 1)]
    assert all((f.MT, f.NT, f.m_live, f.n_live) == (2, 2, 72, 4) for f in map(gemm_facts, GEMM_STAGES))
    assert [(gemm_facts(c).MT, gemm_facts(c).m_live) for c in GEMM_ROWS] == [(1, 1), (1, 31), (1, 32), (1, 33), (1, 127), (1, 128), (2, 1),
                                                                             (8, 127), (9, 1)]
    assert gemm_facts((1025, 132, 96)).idle == 14 and gemm_facts((1025, 260, 160)).idle == 21          # 7 per column tile
    assert [(gemm_facts(c).NT, gemm_facts(c).n_live) for c in GEMM_COLS] == [(1, 4), (1, 28), (1, 32), (1, 36), (1, 60), (1, 64), (1, 68),
                                                                             (1, 124), (1, 128), (2, 4), (3, 4)]
    for name, want in REQUIRED_GEMM.items():
        got = {getattr(f, name) for f in facts + [gemm_facts(c) for c in GEMM_FORM_SHAPES]}
        assert got >= want, (name, sorted(want - got))
    assert all(M <= 1100 and N <= 260 and K <= 288 for M, N, K in GEMM_ALL)


def test_slab_bound_sweep():
    """Where the 48 MB slab bound of pwgrad_plan binds (module docstring): nowhere up to 2048 channels a side, whatever M; the
    np = 1 plan never has fewer splits than the np = 3 plan (the workspace query sizes both from the np = 1 plan)."""
    c = np.arange(64, 2049, 8, dtype=np.int64)
    Co, Ci = np.meshgrid(c, c, indexing="ij")
    tiles = -(-Co // 128) * -(-Ci // 128)
    sbytes = SLAB_CAP // (Co * Ci * 4)
    want = {}
    for np_, target in ((3, 256), (1, 512)):
        s = 8 * (target // (8 * tiles))
        want[np_] = np.where(s < 8, -(-target // tiles), s)          # smax of an unbounded M: the most the plan can ask for
        assert (want[np_] <= sbytes).all(), (np_, int((want[np_] > sbytes).sum()))
    assert (want[1] >= want[3]).all()
    for case in [(256, 64, 64), (100000, 2048, 2048), (1 << 30, 2048, 512), (1 << 30, 64, 64), (5000, 1024, 2048)]:          # the scalar form agrees
        for np_ in (3, 1):
            assert pwgrad_plan(*case, np_).S == pwgrad_plan(*case, np_, cap=1 << 60).S, (case, np_)
    # beyond: np = 1 wants two splits of 400 tiles, the bound allows one; np = 3 wants one
    assert (pwgrad_plan(4096, 2560, 2560, 1).wanted, pwgrad_plan(4096, 2560, 2560, 1).S, pwgrad_plan(4096, 2560, 2560, 3).wanted) == (2, 1, 1)
    assert 2560 * 2560 * 4 * 2 > SLAB_CAP > 2560 * 2560 * 4


def test_exact_operands_stay_below_2_24():
    """Plane-exact operands: every plane product is at most 4 in magnitude, six per contraction index."""
    for M, N, K in GEMM_ALL:
        z = 6 * K * 4                                # |z|
        v = 3 + 3 * (z + 3) + 3                      # res + res_scale * (z + bias), accumulated onto an old value
        assert v < EXACT_LIMIT and 1024 * v * v < 2 ** 53          # ... and a tile's fp64 sum of squares is exact too
    for M, Ci, Co in WGRAD_CASES + [PAIR_WGRAD]:
        dw, db = 6 * M * 4, 3 * M * 2                # |dw_raw|, |db_raw| (all three dy planes times ones)
        assert 3 * dw + 3 < EXACT_LIMIT and 3 * db + 3 < EXACT_LIMIT          # row scale, old values
        assert 4 * 3 * dw < EXACT_LIMIT              # dls: fp32 dots of four products w * dw_raw, then fp64 sums and ONE
        # conversion: exact when the result is below 2^24, which the GPU test asserts of the reference before it compares


# ================================================================================================ operands and references
def gelu_grad(u):
    return 0.5 * (1 + torch.erf(u / np.sqrt(2.0))) + u * torch.exp(-0.5 * u * u) / np.sqrt(2 * np.pi)


def ints(rng, m, *shape):
    return torch.from_numpy(rng.integers(-m, m + 1, shape).astype(np.float32))


def six_pairs(a, b):
    """sum over i + j <= 2 of a_i b_j^T, planes (3, R, K) fp64."""
    return a[0] @ (b[0] + b[1] + b[2]).t() + a[1] @ (b[0] + b[1]).t() + a[2] @ b[0].t()


@functools.lru_cache(maxsize=None)
def gemm_data(case, kind):
    M, N, K = case
    geo = (1, M, 1, K, N, 1, 1, 0, 1)                  # the GEMM as the 1 x 1 conv it is: aten() and conditioning() apply
    D = Plan(kind=kind, geo=geo, case=case, dev={})
    if kind == "exact":
        rng = np.random.default_rng([M, N, K])
        D.ap, D.bp = ints(rng, 2, 3, M, K), ints(rng, 2, 3, N, K)
        D.b, D.res, D.ls, D.y0 = ints(rng, 3, N), ints(rng, 3, M, N), ints(rng, 3, N), ints(rng, 3, M, N)
        a, b = D.ap.double(), D.bp.double()
        D.z = {3: six_pairs(a, b), 1: a[0] @ b[0].t()}
        assert max(t.abs().max().item() for t in D.z.values()) <= 6 * K * 4
        return D
    for D.draw in range(MAX_DRAWS):                    # the first draw whose reference is well conditioned
        s = 100 * D.draw
        D.x, D.w, D.b, D.g = rnd(1, K, M, 1, seed=s + 1), (rnd(N, K, 1, 1, seed=s + 2) / np.sqrt(K)).float(), rnd(N, seed=s + 3), rnd(1, N, M, 1, seed=s + 4)
        D.y, D.dx, D.dw, D.db = aten(D.x, D.w, D.b, D.g, geo, torch.float64)
        D.cond = conditioning(D)
        if D.cond <= COND_LIMIT:
            break
    mat = lambda y: y[0, :, :, 0].t().contiguous()      # (1, N, M, 1) -> (M, N)
    D.a, D.wm = mat(D.x), D.w.view(N, K)
    D.res, D.ls, D.y0, D.aux = rnd(M, N, seed=5), rnd(N, seed=6, kind="uniform"), rnd(M, N, seed=7), rnd(M, N, seed=8)
    b64 = D.b.double()
    y1 = aten(bf(D.x), bf(D.w), D.b, D.g, geo, torch.float64)[0]
    D.z = {3: mat(D.y) - b64, 1: mat(y1) - b64}         # (the bias goes back on in expected(): forms without one exist)
    D.zb = {3: mat(D.y), 1: mat(y1)}
    D.A = D.a.double().abs() @ D.wm.double().abs().t()
    d32 = {3: dist(aten(D.x, D.w, D.b, D.g, geo, torch.float32)[0], D.y),
           1: dist(aten(bf(D.x), bf(D.w), D.b, D.g, geo, torch.float32)[0], y1)}
    D.at = {n: Plan(d32=e, bound=4 * max(e, ULP_FLOOR), seen=0.0, share=0.0) for n, e in d32.items()}
    return D


def test_rounded_gemm_operands_are_well_conditioned():
    for case in GEMM_ALL:
        D = gemm_data(case, "rounded")
        assert D.cond <= COND_LIMIT, (case, D.cond)
        for n in (3, 1):
            assert 4 * ULP_FLOOR <= D.at[n].bound <= 2e-5, (case, n, D.at[n].d32)


@functools.lru_cache(maxsize=None)
def wgrad_data(case, kind):
    M, Ci, Co = case
    geo = (1, M, 1, Ci, Co, 1, 1, 0, 1)
    if kind == "rounded":
        D = wgrad_build(geo, "rounded")                # tests/test_wgrad_plan.py: operands, fp64 references, d32 and bounds
        D.case, D.dev = case, {}
        g1 = bf(D.g).double()
        D.dwr, D.dbr = {3: D.dw, 1: D.dw1}, {3: D.db, 1: g1.sum((0, 2, 3))}          # np = 1 sums the ROUNDED dy: plane 0 times ones
        return D
    D = Plan(kind=kind, geo=geo, case=case, dev={})
    rng = np.random.default_rng([M, Ci, Co])
    D.xp, D.gp = ints(rng, 2, 3, M, Ci), ints(rng, 2, 3, M, Co)
    D.rs, D.w, D.b = ints(rng, 3, Co), ints(rng, 3, Co, Ci, 1, 1), ints(rng, 3, Co)
    D.dw0, D.db0, D.dls0 = ints(rng, 3, Co, Ci, 1, 1), ints(rng, 3, Co), ints(rng, 3, Co)
    x, g = D.xp.double(), D.gp.double()
    gt = g.transpose(1, 2).contiguous()
    sh = lambda t: t.view(Co, Ci, 1, 1)
    D.dwr = {3: sh(six_pairs(gt, x.transpose(1, 2))), 1: sh(gt[0] @ x[0])}
    D.dbr = {3: g.sum((0, 1)), 1: g[0].sum(0)}         # every dy plane times ones
    return D


# ================================================================================================ buffers with guards
BITS = {torch.float32: torch.int32, torch.bfloat16: torch.int16, torch.float64: torch.int64}


def prefilled(n, dtype, fill):
    size = torch.empty((), dtype=dtype).element_size()
    n += (-n * size % 4) // size                     # whole 32-bit words
    buf = torch.empty(n, dtype=dtype, device="cuda")
    if fill != fill:
        buf.fill_(NAN)
    else:
        buf.view(torch.int32).fill_(fill)
    return buf


class Out:
    """An M x N output (np_: that many planes of it) inside a pre-filled allocation: 16 bytes in front of it, ld - N pad columns,
    32 rows behind row M and, with planes, slack behind each."""
    def __init__(self, M, N, ld, dtype, fill, np_=0, old=None):
        lead = 16 // torch.empty((), dtype=dtype).element_size()
        self.ld, self.plane = ld, (M + 32) * ld + (64 if np_ else 0)
        self.buf = prefilled(lead + max(np_, 1) * self.plane, dtype, fill)
        self.geom = (((np_,) if np_ else ()) + (M, N), ((self.plane,) if np_ else ()) + (ld, 1), lead)
        self.t = torch.as_strided(self.buf, *self.geom)
        if old is not None:
            self.t.copy_(old)
        self.before = self.buf.clone()

    def bits(self):
        return self.t.contiguous().view(BITS[self.t.dtype])

    def untouched(self, what):
        inside = torch.zeros(self.buf.shape, dtype=torch.bool, device="cuda")
        torch.as_strided(inside, *self.geom).fill_(True)
        b = BITS[self.buf.dtype]
        assert torch.equal(self.buf.view(b)[~inside], self.before.view(b)[~inside]), f"{what}: a pad column, a row at or beyond M or the slack changed"


def guarded(vals, ld, tight=False):
    """An fp32 / bf16 input matrix 16 bytes into a NaN-filled allocation, NaN in the pad columns and in 32 rows behind it."""
    R, C = vals.shape
    if tight:
        return vals.cuda().contiguous()
    lead = 16 // vals.element_size()
    buf = torch.full((lead + (R + 32) * ld,), NAN, dtype=vals.dtype, device="cuda")
    t = torch.as_strided(buf, (R, C), (ld, 1), lead)
    t.copy_(vals)
    return t


def plane_operand(hip, vals, np_, pad, tight=False):
    """Planes of an (R, K) operand: `vals` (3, R, K) integers written as they are (the first np_ of them), or an (R, K) fp32
    matrix through hip.planes_from_f32.  ld = K + pad, the planes 16 bytes into their allocation, 128 rows and a slack of 72
    elements behind each, NaN everywhere outside the R x K images.  tight: ld = K, no lead (the NaN rows stay)."""
    R, K = vals.shape[-2:]
    ld, lead = (K, 0) if tight else (K + pad, 8)
    plane = (R + 128) * ld + (0 if tight else 72)
    buf = torch.full((lead + np_ * plane,), NAN, dtype=torch.bfloat16, device="cuda")
    P = hip.Planes(torch.as_strided(buf, (np_, R, K), (plane, ld, 1), lead), ld=ld, plane=plane)
    if vals.dim() == 3:
        P.t.copy_(vals[:np_])
    else:
        src = vals.cuda().contiguous()
        hip.planes_from_f32(src, K, R, K, P)
    assert P.t.data_ptr() % 16 == 0 and (tight or P.t.data_ptr() % 32 == 16)
    return P


# ================================================================================================ vrnet_gemm_planes_f32 on the GPU
# act "A": ReLU on the exact operands, GELU on the rounded ones.  yp: yp_np.  noy: the form runs a second time without the fp32
# output and must write the same planes.  The first seven are the forms the program issues (program.py, the ClusterBlock).
FORMS = dict(
    plain=dict(),
    bias=dict(bias=1),
    fc2=dict(bias=1, res=1, ls=1, stats=1),
    fc1=dict(bias=1, act="A", ypre=1, yp=3, noy=1),
    fc1_bf16=dict(bias=1, act="A", ypre=1, yp=1, noy=1),
    aux=dict(aux=1, yp=3, noy=1),
    aux_bf16=dict(aux=1, yp=1, noy=1),
    acc=dict(bias=1, acc=1),
    relu=dict(bias=1, act=1),
    res=dict(res=1),
    full=dict(bias=1, ypre=1, act=1, res=1, ls=1, stats=1, yp=3),
)
EXACT_FORMS = [f for f in FORMS if not f.startswith("aux")]


def expected(D, np_, f):
    """fp64: (pre-activation, result, allowance of the pre-activation, allowance of the result); the allowances None on the
    exact operands, the result's None too behind a GELU or an aux (module docstring)."""
    rounded = D.kind == "rounded"
    d = lambda t: t.double()
    v = D.z[np_] + (d(D.b) if f.get("bias") else 0.0)
    allow = None
    if rounded:
        allow = D.at[np_].bound * v.abs().max().item() + (2.0 ** -20 * D.A if np_ == 3 else 0.0)
        allow = allow + torch.zeros_like(v)
    if f.get("aux"):
        v, allow = v * gelu_grad(d(D.aux_used)), None
    pre, pre_allow = v, allow
    act = f.get("act", 0)
    act = (2 if rounded else 1) if act == "A" else act
    if act == 1:
        v = v.clamp(min=0.0)
    elif act == 2:
        v, allow = F.gelu(v), None
    if f.get("res"):
        s = d(D.ls) if f.get("ls") else 1.0
        if allow is not None:
            allow = allow * (s.abs() if f.get("ls") else 1.0) + 2 * U * ((s * v).abs() + d(D.res).abs() + (d(D.res) + s * v).abs())
        v = d(D.res) + s * v
    if f.get("acc"):
        if allow is not None:
            allow = allow + 2 * U * (v.abs() + d(D.y0).abs())
        v = v + d(D.y0)
    return pre, v, pre_allow, allow


def tile_sums(v, M, N):
    """fp64 (sum, sum of squares) per 32 x 32 tile of an M x N matrix -> (ceil(M / 32), ceil(N / 32), 2)."""
    mb, nb = cdiv(M, 32), cdiv(N, 32)
    p = torch.zeros(mb * 32, nb * 32, dtype=torch.float64)
    p[:M, :N] = v
    t = p.view(mb, 32, nb, 32)
    return torch.stack([t.sum((1, 3)), (t * t).sum((1, 3))], -1)


def gemm_launch(hip, D, np_, f, fill, tight, with_y=True, half=False):
    M, N, K = D.case
    key = (np_, tight)
    if key not in D.dev:
        if D.kind == "exact":
            D.dev[key] = plane_operand(hip, D.ap, np_, 8, tight), plane_operand(hip, D.bp, np_, 16, tight)
        else:
            D.dev[key] = plane_operand(hip, D.a, np_, 8, tight), plane_operand(hip, D.wm, np_, 16, tight)
    A, B = D.dev[key]
    pad = (lambda p: 0) if tight else (lambda p: p)
    act = f.get("act", 0)
    act = (1 if D.kind == "exact" else 2) if act == "A" else act
    o = Plan(y=None, yp=None, ypre=None, stats=None)
    kw = dict(act=act, accumulate=f.get("acc", 0))
    if with_y:
        o.y = Out(M, N, N + pad(4), torch.float32, fill, old=D.y0 if f.get("acc") else None)
        kw.update(y=o.y.t, ldy=o.y.ld)
    if f.get("bias"):
        kw["bias"] = D.b.cuda()
    if f.get("res"):
        r = guarded(D.res, N + 8, tight)               # its own row stride, not ldy
        kw.update(res=r, ldres=r.stride(0), res_scale=D.ls.cuda() if f.get("ls") else None)
    if f.get("aux"):
        a = guarded(D.aux_used.bfloat16() if half else D.aux_used, N + 12, tight)
        kw.update(aux=a, ldaux=a.stride(0))
    if f.get("ypre"):
        o.ypre = Out(M, N, N + pad(8), torch.bfloat16 if half else torch.float32, fill)
        kw.update(ypre=o.ypre.t, ldypre=o.ypre.ld)
    if f.get("yp"):
        o.yp = Out(M, N, N + pad(12), torch.bfloat16, fill, np_=f["yp"])
        kw["yp"] = hip.Planes(o.yp.t, ld=o.yp.ld, plane=o.yp.plane)
    if f.get("stats") and N > 32:
        o.stats = Out(cdiv(M, 32), 2 * cdiv(N, 32), 2 * cdiv(N, 32), torch.float64, fill)
        kw.update(stats=o.stats.t, stats_hw=32)
    hip.gemm_planes(A, B, M, N, K, **kw)
    assert hip.last_kernel() == (10 if np_ == 3 else 11)
    for name in ("y", "yp", "ypre", "stats"):
        if getattr(o, name) is not None:
            getattr(o, name).untouched(f"{D.case} np {np_} {name}")
    return o


def within(D, np_, got, ref, allow, what):
    """Rounded operands: no NaN, then |got - ref| <= allow element by element."""
    R = D.at[np_]
    got = D64(got)
    assert got.shape == ref.shape and not bool(torch.isnan(got).any()), f"{what} {D.case}: NaN in the result -- an element was not written, or a guard was read"
    share, e = ((got - ref).abs() / allow).max().item(), dist(got, ref)
    R.seen, R.share = max(R.seen, e), max(R.share, share)
    print(f"  {D.case} np {np_} {what}: {e:.2e}, {share:.3f} of its bound")
    assert share <= 1.0, f"{what} {D.case} np {np_}: {share:.3f} of the element's bound, distance {e:.3e} (d32 {R.d32:.2e})"


def run_gemm(hip, case, np_, kind, form, tight=False):
    D = gemm_data(case, kind)
    M, N, K = case
    f = FORMS[form]
    if f.get("aux"):
        D.aux_used = bf(D.aux) if form == "aux_bf16" else D.aux          # (the bf16 form reads the same values from a bf16 tensor)
    half = form.endswith("bf16")
    runs = [gemm_launch(hip, D, np_, f, fill, tight) for fill in (NAN, PAT)]
    o = runs[0]
    for name in ("y", "yp", "ypre", "stats"):
        if getattr(o, name) is not None:
            assert torch.equal(getattr(o, name).bits(), getattr(runs[1], name).bits()), f"{case} np {np_} {form}: two runs differ in {name}"
    pre, ref, pre_allow, allow = expected(D, np_, f)
    y = o.y.t
    if kind == "exact":
        assert ref.abs().max().item() < EXACT_LIMIT
        agree(D, y, ref, f"y {form} np {np_}")
        if o.ypre is not None:
            agree(D, o.ypre.t, pre, f"ypre {form} np {np_}")
    else:
        if allow is not None:
            within(D, np_, y, ref, allow, f"y {form}")
        else:                                            # behind a GELU or an aux: the suite's 2e-5
            e = dist(y, ref)
            print(f"  {case} np {np_} y {form}: {e:.2e} (held to 2e-5)")
            assert not bool(torch.isnan(y).any()) and e < 2e-5, (case, np_, form, e)
        if o.ypre is not None:
            within(D, np_, o.ypre.t, pre, pre_allow, f"ypre {form}")
    # the plane output is what was stored: its planes add up to y bit for bit (yp_np = 3), its bf16 rounding (yp_np = 1)
    if o.yp is not None:
        P = hip.Planes(o.yp.t, ld=o.yp.ld, plane=o.yp.plane)
        if f["yp"] == 3:
            assert torch.equal(P.float(), y), f"{case} np {np_} {form}: planes != y"
        else:
            assert torch.equal(o.yp.t[0], y.bfloat16()), f"{case} np {np_} {form}: bf16 plane != rounded y"
    # statistics: one fp64 pair per 32 x 32 tile of exactly what was stored, at (row block, column block)
    if o.stats is not None:
        got = D64(o.stats.t).view(cdiv(M, 32), cdiv(N, 32), 2)
        if kind == "exact":
            assert torch.equal(got, tile_sums(ref, M, N)), f"{case} np {np_} {form}: statistics pairs differ from the exact tile sums"
        else:
            want, mag = tile_sums(D64(y), M, N), tile_sums(D64(y).abs(), M, N)
            assert bool(((got - want).abs() <= 2.0 ** -40 * mag).all()), f"{case} np {np_} {form}: statistics pairs are not the sums of the stored tiles"
    # without the fp32 output: the same planes, the same pre-activation
    if f.get("noy"):
        n = gemm_launch(hip, D, np_, f, NAN, tight, with_y=False)
        assert torch.equal(n.yp.bits(), o.yp.bits()), f"{case} np {np_} {form}: planes differ without y"
        if o.ypre is not None:
            assert torch.equal(n.ypre.bits(), o.ypre.bits())
    # bf16 side tensors (half_side): the pre-activation stored rounded once, the GELU' argument read from a bf16 tensor; all
    # else as with the fp32 tensors of the same values, bit for bit
    if half:
        h = gemm_launch(hip, D, np_, f, NAN, tight, half=True)
        assert torch.equal(h.y.bits(), o.y.bits()) and torch.equal(h.yp.bits(), o.yp.bits()), f"{case} np {np_} {form}: bf16 side tensor"
        if o.ypre is not None:
            assert torch.equal(h.ypre.t, o.ypre.t.bfloat16()), f"{case} np {np_} {form}: bf16 pre-activation != rounded fp32 one"
    if kind == "rounded":
        R = D.at[np_]
        print(f"PLANES-PLAN gemm {case} np {np_} {form}: draw {D.draw} cond {D.cond:.1f} d32 {R.d32:.2e} bound {R.bound:.2e} kernel {R.seen:.2e} "
              f"share {R.share:.3f}")


KINDS = ["exact", "rounded"]
NPS = [3, 1]


@gpu
@pytest.mark.parametrize("np_", NPS, ids=lambda n: f"np{n}")
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("case", GEMM_EDGES, ids=str)
def test_gemm_at_plan_edge(hip, case, kind, np_):
    """Every output of one launch (bias, pre-activation, ReLU, res + res_scale, statistics, planes) on padded rows."""
    run_gemm(hip, case, np_, kind, "full")


@gpu
@pytest.mark.parametrize("np_", NPS, ids=lambda n: f"np{n}")
@pytest.mark.parametrize("form,kind", [(f, "exact") for f in EXACT_FORMS] + [(f, "rounded") for f in FORMS])
@pytest.mark.parametrize("case", GEMM_FORM_SHAPES, ids=str)
def test_gemm_epilogue_forms(hip, case, form, kind, np_):
    """(gelu' is not an integer: the aux forms run on the rounded operands only)"""
    run_gemm(hip, case, np_, kind, form, tight=case == GEMM_FORM_SHAPES[0])


def one_pair(vals, q):
    out = torch.zeros_like(vals)
    out[q] = vals[q]
    return out


@gpu
def test_gemm_multiplies_the_six_plane_pairs_with_i_plus_j_at_most_2(hip):
    M, N, K = PAIR_GEMM
    D = gemm_data(PAIR_GEMM, "exact")
    for i in range(3):
        for j in range(3):
            A, B = plane_operand(hip, one_pair(D.ap, i), 3, 8), plane_operand(hip, one_pair(D.bp, j), 3, 16)
            y = Out(M, N, N + 4, torch.float32, NAN)
            hip.gemm_planes(A, B, M, N, K, y=y.t, ldy=y.ld)
            want = D.ap[i].double() @ D.bp[j].double().t() if i + j <= 2 else torch.zeros(M, N, dtype=torch.float64)
            agree(D, y.t, want, f"A plane {i} x B plane {j}")
            y.untouched(f"pair ({i}, {j})")


# ================================================================================================ vrnet_wgrad_planes_f32 on the GPU
GUARD = 1024          # ints of PAT behind the workspace: 4 KB
FINITE = 12345.0      # the second poison


def wgrad_launch(hip, D, X, DY, dw, db=None, rs=None, accumulate=0, w=None, bias=None, dls=None, poison=NAN, short=0):
    """vrnet_wgrad_planes_f32 on a workspace of exactly the required bytes (minus `short`), poisoned, with a guard behind it."""
    M, Ci, Co = D.case
    need = hip.wgrad_planes_workspace(M, Ci, Co)
    assert need % 4 == 0
    ws = torch.full((need // 4 + GUARD,), poison, device="cuda")
    ws.view(torch.int32)[need // 4:] = PAT
    assert ws.data_ptr() % 16 == 0
    hip.wgrad_planes(X, DY, M, Ci, Co, dw, db, rs, accumulate, w, bias, dls, ws=ws, ws_bytes=need - short)
    assert bool((ws.view(torch.int32)[need // 4:] == PAT).all()), f"{D.case}: the guard behind the workspace changed"


def run_wgrad(hip, case, np_, kind):
    D = wgrad_data(case, kind)
    M, Ci, Co = case
    prec, fam = (2, 12) if np_ == 3 else (1, 13)
    p = pwgrad_plan(M, Ci, Co, np_)
    assert hip.wgrad_planes_plan(M, Ci, Co, np_) == (p.nt, p.ct, p.S, p.rows)
    rounded = kind == "rounded"
    if np_ not in D.dev:
        if rounded:
            D.dev[np_] = plane_operand(hip, nhwc(D.x).view(M, Ci).cpu(), np_, 8), plane_operand(hip, nhwc(D.g).view(M, Co).cpu(), np_, 16)
        else:
            D.dev[np_] = plane_operand(hip, D.xp, np_, 8), plane_operand(hip, D.gp, np_, 16)
    X, DY = D.dev[np_]
    nan = lambda *sh: torch.full(sh, NAN, device="cuda")
    dw_ref, db_ref, rs = D.dwr[np_], D.dbr[np_], D.rs.double()
    x6 = rounded and np_ == 3
    # (a) dw, db, row_scale into NaN-filled outputs; twice, the second time on another poison: the same bits
    runs = []
    for poison in (NAN, FINITE):
        dw, db = nan(Co, Ci, 1, 1), nan(Co)
        wgrad_launch(hip, D, X, DY, dw, db, D.rs.cuda(), poison=poison)
        assert hip.last_kernel() == fam
        runs.append((dw, db))
    ref = rs[:, None, None, None] * dw_ref
    held(D, prec, runs[0][0], ref, "dw, row_scale", x6_allowance(D, ref, rs.abs()[:, None, None, None] * D.A_dw) if x6 else None)
    held(D, prec, runs[0][1], rs * db_ref, "db, row_scale")
    assert torch.equal(runs[0][0].view(torch.int32), runs[1][0].view(torch.int32)), f"{case}: two weight gradients differ"
    assert torch.equal(runs[0][1].view(torch.int32), runs[1][1].view(torch.int32)), f"{case}: two bias gradients differ"
    # (b) dw alone, accumulated onto old values
    dw = D.dw0.cuda()
    wgrad_launch(hip, D, X, DY, dw, accumulate=1)
    ref = D.dw0.double() + dw_ref
    held(D, prec, dw, ref, "dw, accumulate", x6_allowance(D, ref, D.A_dw) if x6 else None)
    # (c) the layer-scale gradient with w and bias, plain and accumulated
    wg, bg = D.w.cuda(), D.b.cuda()
    dls_ref = dls_of(D, dw_ref, db_ref)
    assert rounded or (dls_ref.abs() + D.dls0.abs()).max().item() < EXACT_LIMIT
    for acc in (0, 1):
        dw, db, dls = (D.dw0.cuda(), D.db0.cuda(), D.dls0.cuda()) if acc else (nan(Co, Ci, 1, 1), nan(Co), nan(Co))
        wgrad_launch(hip, D, X, DY, dw, db, None, acc, wg, bg, dls)
        assert hip.last_kernel() == fam
        what = "dls form, accumulate" if acc else "dls form"
        ref = D.dw0.double() + dw_ref if acc else dw_ref
        held(D, prec, dw, ref, "dw, " + what, x6_allowance(D, ref, D.A_dw) if x6 else None)
        held(D, prec, db, D.db0.double() + db_ref if acc else db_ref, "db, " + what)
        ref = D.dls0.double() + dls_ref if acc else dls_ref
        held(D, prec, dls, ref, "dls, " + what, dls_allowance(D, prec, dw_ref, db_ref, ref) if rounded else None)
    # one byte less than the required workspace is refused
    dw = nan(Co, Ci, 1, 1)
    with pytest.raises(RuntimeError, match="wgrad_planes: workspace"):
        wgrad_launch(hip, D, X, DY, dw, short=1)
    assert bool(torch.isnan(dw).all()), "a refused call wrote"
    if rounded:
        R = D.at[prec]
        print(f"PLANES-PLAN wgrad {case} np {np_}: draw {D.draw} cond {D.cond:.1f} d32 {R.d32:.2e} bound {R.bound:.2e} kernel {R.seen:.2e} "
              f"share {R.share:.3f}")


@gpu
@pytest.mark.parametrize("np_", NPS, ids=lambda n: f"np{n}")
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("case", WGRAD_CASES, ids=str)
def test_wgrad_planes_at_plan_edge(hip, case, kind, np_):
    run_wgrad(hip, case, np_, kind)


@gpu
def test_wgrad_multiplies_the_six_plane_pairs_with_i_plus_j_at_most_2(hip):
    """... and the bias gradient sums EVERY dy plane (each is multiplied by a fragment of ones)."""
    M, Ci, Co = PAIR_WGRAD
    D = wgrad_data(PAIR_WGRAD, "exact")
    for i in range(3):
        for j in range(3):
            X, DY = plane_operand(hip, one_pair(D.xp, j), 3, 8), plane_operand(hip, one_pair(D.gp, i), 3, 16)
            dw, db = torch.full((Co, Ci), NAN, device="cuda"), torch.full((Co,), NAN, device="cuda")
            wgrad_launch(hip, D, X, DY, dw, db)
            want = D.gp[i].double().t() @ D.xp[j].double() if i + j <= 2 else torch.zeros(Co, Ci, dtype=torch.float64)
            agree(D, dw, want, f"dy plane {i} x x plane {j}")
            agree(D, db, D.gp[i].double().sum(0), f"column sums of dy plane {i}")


# ================================================================================================ the split kernels on the GPU
SENTINEL = 7.0


def split_dest(np_, R, K, ld):
    """Destination planes with 64 sentinels behind every plane and sentinels in the pad columns."""
    plane = R * ld + 64
    buf = torch.full((np_ * plane,), SENTINEL, dtype=torch.bfloat16, device="cuda")
    return buf, torch.as_strided(buf, (np_, R, K), (plane, ld, 1), 0), plane


def check_split(hip, buf, t, ld, plane, want, np_, what):
    P = hip.Planes(t, ld=ld, plane=plane)
    if np_ == 3:
        assert torch.equal(P.float(), want), f"{what}: the planes do not add up to the source"
    assert torch.equal(t[0], want.bfloat16()), f"{what}: plane 0 is not the bf16 rounding"
    inside = torch.zeros(buf.shape, dtype=torch.bool, device="cuda")
    torch.as_strided(inside, t.shape, t.stride(), 0).fill_(True)
    assert bool((buf[~inside] == SENTINEL).all()), f"{what}: wrote outside the planes"


def entry(src, R, K, sr, sk, ksc, dst, ld, plane, first):
    return [src.data_ptr(), R, K, sr, sk, ksc.data_ptr() if ksc is not None else 0, dst.data_ptr(), ld, plane, first]


@gpu
@pytest.mark.parametrize("np_", NPS, ids=lambda n: f"np{n}")
def test_split_tables(hip, np_):
    """planes_split_kernel's search over the first blocks: one entry; five entries, the first and the last a single block (every
    block of those is an entry's first AND last, at both ends of the grid), one transposed with a scale."""
    shapes = [(20, 40, 40, False), (70, 132, 136, False), (33, 64, 64, False), (64, 200, 200, True), (32, 64, 68, False)]
    assert [split_blocks(R, K) for R, K, _, _ in shapes] == [1, 9, 2, 8, 1]
    for chosen in ([shapes[1]], shapes):
        table, checks, first = [], [], 0
        for e, (R, K, ld, transposed) in enumerate(chosen):
            buf, t, plane = split_dest(np_, R, K, ld)
            if transposed:                               # source (K, R) row-major: rows at element stride 1, k at stride R
                src, ksc = (rnd(K, R, seed=40 + e) * 0.05).cuda(), rnd(K, seed=50 + e, kind="uniform").cuda()
                table += entry(src, R, K, 1, R, ksc, t, ld, plane, first)
                want = (src * ksc[:, None]).t().contiguous()
            else:
                src = (rnd(R, K, seed=40 + e) * 0.05).cuda()
                table += entry(src, R, K, K, 1, None, t, ld, plane, first)
                want = src
            checks.append((buf, t, ld, plane, want, src))
            first += hip.planes_split_blocks(R, K)
        hip.planes_split(torch.tensor(table, dtype=torch.int64, device="cuda"), len(chosen), first, np_)
        for e, (buf, t, ld, plane, want, _) in enumerate(checks):
            check_split(hip, buf, t, ld, plane, want, np_, f"entry {e} of {len(chosen)}")


@gpu
@pytest.mark.parametrize("np_", NPS, ids=lambda n: f"np{n}")
@pytest.mark.parametrize("shape", [(37, 12), (5, 4), (70, 68), (33, 100)], ids=str)
def test_split_transposed_with_scale(hip, shape, np_):
    """The data-gradient form (k stride = R of the source, a scale per k): K % 8 == 4 on a tight destination (the thread at
    K - 4 owns four columns only), R no multiple of 32, K no multiple of 64."""
    R, K = shape
    src, ksc = rnd(K, R, seed=60).cuda(), rnd(K, seed=61, kind="uniform").cuda()
    buf, t, plane = split_dest(np_, R, K, K)
    hip.planes_split(torch.tensor(entry(src, R, K, 1, R, ksc, t, K, plane, 0), dtype=torch.int64, device="cuda"), 1, hip.planes_split_blocks(R, K), np_)
    check_split(hip, buf, t, K, plane, (src * ksc[:, None]).t().contiguous(), np_, f"transposed {shape}")


@gpu
@pytest.mark.parametrize("np_", NPS, ids=lambda n: f"np{n}")
@pytest.mark.parametrize("scaled", [False, True])
def test_split_row_major_source_off_16_byte_alignment(hip, scaled, np_):
    """A row-major source whose rows start 4 bytes past a 16-byte boundary: the scalar loads, whole eights included."""
    R, K = 37, 72
    src = rnd(R * K + 1, seed=62).cuda()[1:].view(R, K)
    assert src.data_ptr() % 16 == 4 and (K * 4) % 16 == 0
    ksc = rnd(K, seed=63, kind="uniform").cuda() if scaled else None
    buf, t, plane = split_dest(np_, R, K, K + 4)
    hip.planes_split(torch.tensor(entry(src, R, K, K, 1, ksc, t, K + 4, plane, 0), dtype=torch.int64, device="cuda"), 1, hip.planes_split_blocks(R, K), np_)
    check_split(hip, buf, t, K + 4, plane, src * ksc if scaled else src, np_, "misaligned source")
