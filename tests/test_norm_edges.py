"""The statistics and normalisation kernels of csrc/stream_ops.hip at the edges of their launch plans: the moments pass in all its
forms, moments_reduce, the three affine kernels, GroupNorm(1, C) and BatchNorm in every form, and the ECA, layer-scale and
moments_to_float coefficient kernels -- in the manner of tests/test_spatial_edges.py, whose helpers this file imports.

Which branch a case reaches is not taken on trust.  The tests without a gpu mark restate moments_plan (TPR, RP, ncb, nc and the
clamp that set it, rows, nchunks, the last chunk, the live threads of the last channel block), the vec / flat / scalar choice of
affine_impl with its grid, the bx rules of the GroupNorm apply launchers and the grids of the coefficient launchers in Python;
assert each case's claimed branch from the restatement; require that the restated plans reproduce the library's host-only
queries vrnet_moments_workspace and vrnet_gn_bwd_workspace; sweep the two sizes those formulas rely on (nchunks * ncb <= 2048
pairs of gtot, nchunks * ncb <= nchunks * C pairs of partial); and require that the union over the case tables is the complete
list ALL_BRANCHES.  A case whose removal would leave the union whole is listed in DUPLICATES with the reason it is kept
(test_every_case_is_needed_or_a_named_duplicate).  The clamp `nc < 1` of moments_plan is dead for HW, C > 0 (cdiv of a positive
number): "nc floor 1" names the plans that cdiv(HW C, 4096) itself leaves at one chunk.

Operands and bounds, four classes:

  exact    the moments kernels convert to fp64 before they multiply and add, affine only multiplies and adds small integers:
           x, x2 in {-3..3}, mask, z and the coefficients in {-2..2}.  Every form of moments (x | x, x2 | x, x2, mask | x, x2 with
           the mask recomputed from z | total_only | gtot) and every form of affine in its three kernels must equal the integer
           reference bit for bit (test_exact_cases_stay_in_range: below 2^24 in fp32, below 2^53 in fp64).  The total_only pairs
           and the gtot pairs are read back from the caller's workspace and added on the host: integers, so any order is exact.
           (gtot comes from vrnet_gn_apply_bwd, which takes 16-byte rows only: the cases of the scalar kernel run the other five.)
  fp64 sum one case per moments form at x = 40 +- 1.5 against numpy.longdouble: |error| <= n 2^-53 sum |terms| per output, the
           worst case of n roundings in any order (n - 1 additions and, for gtot, the one product by gamma).
  coef     the coefficient kernels evaluate in fp64 and round once: given moments / partials / pairs / mean_rstd, the reference
           evaluates the kernel's documented formula in numpy.longdouble and rounds to fp32; bound = one fp32 ulp of that value
           + 4 d64, d64 = the same formula in fp64 against longdouble, per output.  Operands are redrawn (at most MAX_DRAWS
           times) until d64 < ulp / 16 on every output -- a condition on the reference alone.  running_mean, running_var and
           num_batches_tracked (exactly + 1, however many workgroups) fall under the same rule.  No case took a second draw.
  apply    gn_apply_fwd / gn_apply_bwd / gn_apply_bwd_from_partials / bn_apply_bwd_zmask and the chains moments -> gn_coef_fwd ->
           affine, gn_stats_fwd -> affine, pairs -> gn_apply_fwd -> gn_apply_bwd, bn_stats_fwd -> affine(pre 1) -> bn_stats_bwd /
           bn_stats_bwd_zmask -> bn_apply_bwd_zmask against F.group_norm / F.batch_norm + ReLU in fp64 with autograd:
           bound = 4 * max(d32, ULP_FLOOR) in the metric of dist(), d32 = ATen in fp32 against fp64 on the same operands.  dy is
           drawn correlated with the normalised input so that the parameter gradients do not cancel (conditioning <= COND_LIMIT
           on the first draw everywhere); the BatchNorm operands are redrawn while a pre-activation lies within 2e-6 of the ReLU's
           kink (never).  zmask against the stored mask, affine(pre 3) against affine(pre 2) and the in-place accumulate against
           the out-of-place add are bit for bit (torch.equal).

Outputs sit in the PAT bit pattern inside buffers with guard elements in front and behind and four guard columns behind every
NHWC row (none where the flat kernel needs ld == C, five where a case forces the scalar kernel at C % 4 == 0), all of which must
keep it; inputs are surrounded by NaN.  The entry points with a caller's workspace (vrnet_moments_f32, vrnet_gn_stats_fwd,
vrnet_gn_apply_bwd, vrnet_bn_stats_bwd_zmask) get exactly the queried bytes in front of a 4 KB guard, run on a NaN and on a finite
poison for equal bits, and are refused with one byte less, outputs untouched.

The sensitivity tests (no GPU) plant in the reference the errors these kernels could make -- the short last chunk skipped, channel
block 1 aliased onto block 0, the one live thread of the last block dropped, pair 256 / 512 or partial 64 / 256 skipped, the flat
kernel's channel counter not wrapped, per-sample coefficients read with bstride 0, the elements behind 4096 blocks x 2 trips left
unwritten, num_batches_tracked raised per block, the mean rounded to fp32 before the variance -- and require that the comparison
the GPU tests use rejects each.

Measured on an MI355X (the tests print every figure):

  moments, 17 exact cases, 5 to 7 read-backs   equal to the integer reference bit for bit; NaN and finite poison give equal bits
  moments at x = 40 +- 1.5, (2, 70, 48)        per-channel sums (n = 70): bounds 7.8e-12 .. 8.9e-10, every kernel error 0 (the sums
                                               agree with longdouble to the last bit); total_only (n = 3360): bounds 5.0e-8 ..
                                               2.0e-6, kernel 3.5e-10; gtot: bounds 3.9e-8 .. 1.6e-6, kernel 1.4e-10
  affine, 24 cases x 5 or 6 forms, 3 caps      equal bit for bit; accumulate == add, pre 3 == pre 2
  coefficient kernels, 113 cases               d64 / ulp at most 1.7e-5 (bn_coef_bwd_from_chunks; gn 1.0e-6, bn 2.7e-6 / 8.9e-6 from
                                               chunks, eca 1.8e-6): every first draw passes 1/16.  Every output of every kernel
                                               EQUALS the longdouble reference rounded to fp32: distance 0 of a bound of one ulp
  gn_apply_fwd y at the 7 pair counts          d32 8.4e-8 .. 5.5e-7, every bound the floor 3.8e-6, kernel 8.6e-8 .. 5.4e-7 (0.14)
  GroupNorm chains, 10 cases                   d32 2.6e-8 .. 7.9e-6, bounds 3.8e-6 .. 3.2e-5, kernels at most 6.1e-7: 0.026 .. 0.16 of
                                               their bounds, the largest share at HW = 1, B = 1, C = 4
  BatchNorm chains, 8 cases                    d32 2.5e-8 .. 4.4e-6, bounds 3.8e-6 .. 1.75e-5, kernels at most 4.1e-6: 0.20 .. 0.26 of
                                               their bounds.  The kernels' distance equals d32 to three digits where one fp32
                                               rounding both sides share dominates: z - mean at |mean| >> std (y, dz) and the
                                               final addition onto the old parameter gradient (dgamma, dbeta)
  the whole file                               185 tests in 6 s, the slowest (1025, 1120, 8) at 1.3 s

No kernel error was found: the paths read correct and measure correct.  (The one failure on the way was a shape mistake in
f_gn_fwd, a reference of this file.)"""
import functools
import types
import zlib

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests.test_direct_conv import COND_LIMIT, EXACT_LIMIT, MAX_DRAWS, ULP_FLOOR, dist
from tests.test_hip_ops import TOL, nchw, nhwc, rnd
from tests.test_spatial_edges import (FINITE, GUARD, VR_ERR_WORKSPACE, Buf, bound_of, cdiv, ints, out_vec, rejected, same, same_bits,
                                      vec, within)
from tests.test_strided_rows import NAN, PAT

gpu = pytest.mark.gpu
NS = types.SimpleNamespace
LD, F64, F32 = np.longdouble, np.float64, np.float32
U53 = 2.0 ** -53


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
def moments_plan(B, HW, C, v):
    """moments_plan of csrc/stream_ops.hip for moments_kernel<v>."""
    CV = C // v
    t = 1
    while t < CV and t < 256:
        t <<= 1
    ncb = cdiv(CV, t)
    nc = cdiv(HW * C, 4096)
    why = "HW C / 4096" if nc > 1 else "floor 1"
    if nc > 512:
        nc, why = 512, "cap 512"
    by_grid = cdiv(1024, B * ncb)
    if nc > by_grid:
        nc, why = by_grid, "by_grid"
    if nc > HW:
        nc, why = HW, "HW"
    rows = cdiv(HW, nc)
    nchunks = cdiv(HW, rows)
    return NS(v=v, CV=CV, TPR=t, RP=256 // t, ncb=ncb, nc=nc, why=why, rows=rows, nchunks=nchunks, last=HW - (nchunks - 1) * rows,
              live=CV - (ncb - 1) * t, gper=nchunks * ncb)


def moments_workspace(B, HW, C):
    n = moments_plan(B, HW, C, 1).nchunks
    if C % 4 == 0:
        n = max(n, moments_plan(B, HW, C, 4).nchunks)
    return B * n * C * 2 * 8 + 256


def gn_bwd_workspace(B, HW, C):
    return moments_workspace(B, HW, C) + B * 512 * 4 * 2 * 8 + 256


def gtot_offset(B, HW, C):
    """Bytes from the workspace of vrnet_gn_apply_bwd to its gtot pairs."""
    return cdiv(moments_workspace(B, HW, C), 256) * 256


def affine_plan(HW, C, bstride, padc):
    """affine_impl on 16-byte aligned buffers whose rows are C + padc floats apart."""
    ld = C + padc
    vec_ = C % 4 == 0 and ld % 4 == 0 and bstride % 4 == 0
    flat = not vec_ and C % 4 != 0 and C <= 16 and (HW * C) % 4 == 0 and ld == C
    why = None if vec_ or flat else "C > 16" if C % 4 and C > 16 else "ld % 4" if C % 4 == 0 else "strided" if ld != C else "HW C % 4"
    n = HW * C // 4 if vec_ or flat else HW * C
    blocks = min(max(cdiv(n, 1024), 1), 4096)
    stride = blocks * 256
    trips, e = 0, 0                            # thread 0 of block 0, the thread that makes the most trips
    while e + stride < n:
        trips, e = trips + 1, e + 2 * stride
    return NS(kernel="<4>" if vec_ else "flat" if flat else "<1>", why=why, n=n, blocks=blocks, stride=stride, trips=trips,
              tail=e < n, capped=cdiv(n, 1024) > 4096)


def gn_fwd_bx(B, HW, C):
    bx, cap = cdiv(HW * (C // 4), 1024), cdiv(2048, B)
    return NS(bx=max(min(bx, cap), 1), rule="capped" if bx > cap else "bx 1" if bx <= 1 else "free")


def gn_bwd_bx(B, HW, C):
    """gn_apply_bwd_impl and vrnet_gn_apply_bwd_from_partials."""
    bx, cap, need = cdiv(HW * (C // 4), 1024), cdiv(2048, B), cdiv(C, 4)
    capped = bx > cap
    bx = min(bx, cap)
    return NS(bx=max(bx, need), rule="raised to need" if bx < need else "capped" if capped else "free")


def coef_grid(kernel, B=1, C=1, k=1, n=1):
    """(workgroups, threads) of the coefficient launchers."""
    return {"gn_coef_fwd": (B, 256), "gn_coef_from_pairs": (B, 256), "gn_coef_bwd": (B + cdiv(C, 256), 256),
            "bn_coef_fwd": (cdiv(C, 128), 128), "bn_coef_bwd": (cdiv(C, 128), 128), "bn_partial": (cdiv(C, 4), 256),
            "eca_coef": (cdiv(B * C, 256), 256), "eca_dwk": (k, 256), "ls_coef_bwd": (cdiv(C, 128), 128),
            "moments_to_float": (cdiv(n, 256), 256), "moments_reduce": (cdiv(B * C * 2, 16), 256)}[kernel]


# ================================================================================================ the cases
MOM_CASES = [                              # (B, HW, C, v): v = 1 at C % 4 == 0 is forced by rows of C + 5 floats
    (1, 1, 4, 4),                          # the smallest legal map of the 16-byte kernel: one quad
    (2, 33, 64, 4),                        # TPR == CV = 16
    (1, 128, 20, 4),                       # TPR = 8 > CV = 5: three idle lanes per row; rows == 4 RP: the unrolled trip alone
    (1, 129, 20, 4),                       # rows == 4 RP + 1: ... and one row of the tail loop
    (2, 1, 1024, 4),                       # HW = 1 at TPR = 256, RP = 1: the LDS reduction has no trips
    (1, 64, 1028, 4),                      # nc = 17 but nchunks = 16; the second channel block holds one live thread
    (1, 64, 2048, 4),                      # two full channel blocks, 32 chunks
    (8, 128, 2052, 4),                     # by_grid: 43 chunks of 3 rows, the last of 2; three channel blocks, one live thread
    (1, 8200, 256, 4),                     # the cap 512: 483 chunks of 17 rows, the last of 6
    (1, 3, 4100, 4),                       # nc clamped by HW; five channel blocks
    (3, 7, 5, 1),                          # B C 2 = 30: the last workgroup of moments_reduce is ragged
    (1, 256, 3, 1),                        # the scalar kernel's rows == 4 RP
    (1, 257, 3, 1),                        # ... + 1
    (1, 20, 257, 1),                       # the scalar kernel with one live thread in its second channel block
    (2, 16, 256, 1),                       # the scalar kernel at C % 4 == 0 (unaligned rows): TPR == CV = 256
    (8, 128, 1028, 1),                     # ... with five channel blocks, the last ragged (4 threads); by_grid: 26 chunks
    (4, 300, 2, 1),                        # the scalar kernel at TPR == CV = 2
]
SHORT_CHUNK = [(8, 128, 2052, 4), (1, 8200, 256, 4), (8, 128, 1028, 1)]          # where the sensitivity tests plant their errors
CHANNEL_BLOCKS = [(1, 64, 1028, 4), (1, 64, 2048, 4), (8, 128, 2052, 4), (1, 3, 4100, 4), (1, 20, 257, 1), (8, 128, 1028, 1)]
MOM_FORMS = ["x", "x x2", "x x2 mask", "x x2 mA", "total_only", "gtot"]
MOM_REAL = (2, 70, 48, 4)
PAIR_COUNTS = [1, 255, 256, 257, 512, 513, 769]
BN_TOTALS = [1, 64, 65, 256, 257, 449]
BN_CHUNK_C = [4, 5, 7]                     # C % 4 = 0, 1, 3: no, three and one dead wave in the last workgroup
GN_COEF = [(2, 5, 48), (3, 7, 260)]        # (B, HW, C): C < 256; C > 256 and no multiple of it
BN_COEF = [(2, 5, 7), (3, 7, 131)]         # C < 128; two workgroups, the second ragged
ECA_K = [1, 3, 5, 7]
ECA_BC = [(2, 1), (2, 2), (3, 100)]        # C < k; B C = 300: two workgroups
LS_CASE, M2F_N = (3, 129), 300

GN_CASES = [                               # (B, HW, C): the chains; the moments-plan edge each one sits on in the comment
    (1, 1, 4),                             # HW = 1, B = 1, C = 4
    (2, 1, 1024),                          # HW = 1: the backward's bx raised from 1 to need = 256
    (2, 70, 48),                           # idle lanes
    (2, 5, 260),                           # TPR = 128 > CV = 65
    (1, 64, 1028),                         # nchunks < nc, one live thread
    (8, 128, 2052),                        # by_grid
    (1, 8200, 256),                        # cap 512: gper = 483 > 256, parameter row over 483 > 64 partials
    (1025, 1120, 8),                       # bx capped by cdiv(2048, B) = 2 in both directions; by_grid = 1
]
GN_PARTIALS = [(2, 64, 48), (1, 4128, 40), (1025, 1120, 8)]      # HW % 32 == 0; C % 32 != 0
BN_CASES = [(2, 2, 4), (3, 1, 48), (2, 70, 48), (2, 5, 260), (1, 64, 1028), (1, 40, 2052), (3, 7, 5), (2, 8, 7)]

FLAT_C = [1, 2, 3, 5, 6, 7, 9, 15]
AFF_CASES = ([(2, 5, 8, 1, 4), (1, 75, 16, 0, 4), (2, 150, 16, 1, 4)] +          # (B, HW, C, per-sample coefficients, padc)
             [(2, 8, C, ps, 0) for C in FLAT_C if C != 3 for ps in (0, 1)] + [(1, 400, 3, 0, 0), (2, 800, 3, 1, 0)] +
             [(2, 4, 17, 1, 0), (2, 5, 3, 1, 0), (2, 8, 8, 0, 5), (1, 100, 3, 0, 4), (2, 200, 3, 1, 4)])
AFF_CAPS = [(1, 4194304 + 1030, 4, 0, 4), (1, 5593000, 3, 0, 0), (1, 1398443, 3, 0, 0)]          # <4>, flat, <1>
AFF_FORMS = ["A S1 D1", "full pre 1 add", "bare pre 2", "no x1 accumulate", "A only", "pre 3"]


def rows_class(p):
    """Where several rows share a workgroup's trip (RP > 1): how rows_per_chunk sits against the four-rows-per-trip loop."""
    if p.RP == 1:
        return None
    return {p.RP * 4: "rows == 4 RP", p.RP * 4 + 1: "rows == 4 RP + 1"}.get(p.rows, "rows < RP" if p.rows < p.RP else None)


def reduce_class(n):
    return "nchunks < 16" if n < 16 else "nchunks == 16" if n == 16 else "nchunks > 16, % 16" if n % 16 else "nchunks % 16 == 0"


def mom_branches(case):
    B, HW, C, v = case
    p = moments_plan(B, HW, C, v)
    k = f"moments<{v}>"
    one = "ncb 1, TPR 256, RP 1" if p.TPR == 256 else "ncb 1, TPR == CV" if p.TPR == p.CV else "ncb 1, TPR > CV"
    out = {(k,), (k, one if p.ncb == 1 else "ncb >1 full" if p.live == p.TPR else "ncb >1 one live thread" if p.live == 1 else "ncb >1 ragged"),
           ("moments", "nc " + p.why), ("moments", "nchunks == nc" if p.nchunks == p.nc else "nchunks < nc"),
           ("moments", "last chunk full" if p.last == p.rows else "last chunk short"), ("moments_reduce", reduce_class(p.nchunks))}
    if rows_class(p):
        out.add((k, rows_class(p)))
    if (B * C * 2) % 16:
        out.add(("moments_reduce", "B C 2 % 16"))
    return out


def aff_branches(case):
    B, HW, C, ps, padc = case
    p = affine_plan(HW, C, C if ps else 0, padc)
    k = "affine " + p.kernel
    out = {(k,), (k, "bstride C" if ps else "bstride 0"),
           (k, "capped" if p.capped else "loop not taken" if p.trips == 0 else "loop with tail" if p.tail else "loop once")}
    if p.why:
        out.add((k, p.why))
    if p.kernel == "flat":
        out.add((k, f"C {C} bstride {C if ps else 0}"))
    if p.blocks == 1:
        out.add((k, "one block"))
    return out


def gn_branches(case, partials=False):
    B, HW, C = case
    k = "gn from_partials" if partials else "gn bwd"
    nch, gper = (HW // 32, HW // 32 * cdiv(C, 32)) if partials else (lambda p: (p.nchunks, p.gper))(moments_plan(B, HW, C, 4))
    out = {(k, gn_bwd_bx(B, HW, C).rule), (k, "B nchunks < 64" if B * nch < 64 else "B nchunks > 64")}
    if gper > 256:
        out.add((k, "gper > 256"))
    if partials and C % 32:
        out.add((k, "C % 32"))
    if not partials:
        out.add(("gn fwd", gn_fwd_bx(B, HW, C).rule))
    return out


def chunk_loop_class(total):
    """bn_channel_sums of lanes 0 and 63: trips of the four-per-trip loop, then of the tail loop."""
    out = []
    for j in (0, 63):
        trips = 0
        while j + 192 < total:
            j, trips = j + 256, trips + 1
        out.append(f"{trips}+{len(range(j, total, 64))}")
    return " | ".join(out)


def pair_loop_class(per):
    """The two-per-trip loop of threads 0 and 255: trips, then whether the single tail pair is taken."""
    out = []
    for i in (0, 255):
        trips = 0
        while i + 256 < per:
            i, trips = i + 512, trips + 1
        out.append(f"{trips}+{int(i < per)}")
    return " | ".join(out)


CASE_TABLES = [("mom", MOM_CASES, mom_branches), ("aff", AFF_CASES + AFF_CAPS, aff_branches), ("gn", GN_CASES, gn_branches),
               ("gnp", GN_PARTIALS, lambda c: gn_branches(c, True)),
               ("pairs", PAIR_COUNTS, lambda n: {("pairs", pair_loop_class(n))}),
               ("chunks", BN_TOTALS, lambda n: {("bn_channel_sums", chunk_loop_class(n))}),
               ("chunkC", BN_CHUNK_C, lambda C: {("bn partial", f"C % 4 == {C % 4}")}),
               ("gncoef", GN_COEF, lambda c: {("gn_coef", "C < 256" if c[2] < 256 else "C > 256, % 256")}),
               ("bncoef", BN_COEF, lambda c: {("bn_coef", "C < 128" if c[2] < 128 else "C > 128, % 128")}),
               ("ecak", ECA_K, lambda k: {("eca", f"k {k}")}),
               ("ecabc", ECA_BC, lambda c: {("eca", "C < k" if c[1] < 3 else "B C % 256"), ("eca", f"C {c[1]}")})]


def branches(skip=None):
    out = set()
    for name, table, fn in CASE_TABLES:
        for case in table:
            if (name, case) != skip:
                out |= fn(case)
    return out


ALL_BRANCHES = (
    {("moments<4>",), ("moments<1>",)} |
    {(k, t) for k in ("moments<4>", "moments<1>") for t in ("ncb 1, TPR == CV", "ncb 1, TPR > CV", "ncb 1, TPR 256, RP 1",
                                                            "ncb >1 one live thread", "rows < RP", "rows == 4 RP", "rows == 4 RP + 1")} |
    {("moments<4>", "ncb >1 full"), ("moments<1>", "ncb >1 ragged")} |
    {("moments", "nc " + w) for w in ("HW C / 4096", "floor 1", "cap 512", "by_grid", "HW")} |
    {("moments", t) for t in ("nchunks == nc", "nchunks < nc", "last chunk full", "last chunk short")} |
    {("moments_reduce", t) for t in ("nchunks < 16", "nchunks == 16", "nchunks > 16, % 16", "nchunks % 16 == 0", "B C 2 % 16")} |
    {("pairs", t) for t in ("0+1 | 0+0", "0+1 | 0+1", "1+0 | 0+1", "1+0 | 1+0", "1+1 | 1+0", "2+0 | 1+1")} |          # threads 0 | 255
    {("bn_channel_sums", t) for t in ("0+1 | 0+0", "0+1 | 0+1", "0+2 | 0+1", "1+0 | 1+0", "1+1 | 1+0", "2+0 | 1+3")} |      # lanes 0 | 63
    {("bn partial", f"C % 4 == {r}") for r in (0, 1, 3)} |
    {("gn fwd", r) for r in ("bx 1", "free", "capped")} |
    {(k, r) for k in ("gn bwd", "gn from_partials") for r in ("raised to need", "free", "capped", "B nchunks < 64", "B nchunks > 64",
                                                              "gper > 256")} |
    {("gn from_partials", "C % 32")} |
    {("gn_coef", "C < 256"), ("gn_coef", "C > 256, % 256"), ("bn_coef", "C < 128"), ("bn_coef", "C > 128, % 128")} |
    {("eca", f"k {k}") for k in ECA_K} | {("eca", t) for t in ("C < k", "B C % 256", "C 1", "C 2", "C 100")} |
    {("affine " + k,) for k in ("<4>", "flat", "<1>")} |
    {("affine " + k, t) for k in ("<4>", "flat", "<1>") for t in ("bstride 0", "bstride C", "one block", "loop not taken", "loop once",
                                                                  "loop with tail", "capped")} |
    {("affine <1>", w) for w in ("C > 16", "HW C % 4", "strided", "ld % 4")} | {("affine flat", f"C {C} bstride {b}") for C in FLAT_C for b in (0, C)})

# cases that reach no branch of their own, and why they stay
DUPLICATES = {
    ("mom", (8, 128, 2052, 4)): "(8, 128, 2052): by_grid in the 16-byte kernel, three channel blocks; C = 2052 of the issue's list",
    ("mom", (2, 33, 64, 4)): "TPR == CV = 16, a whole row of live lanes; (1, 1, 4) reaches the branch with a single one",
    ("mom", (1, 129, 20, 4)): "rows == 4 RP + 1 in a single chunk: the tail row is the sample's last; (1, 8200, 256) has it in 482 chunks",
    ("pairs", 1): "one pair: the smallest count", ("pairs", 255): "255 pairs: the last count with an idle thread",
    ("gn", (1, 1, 4)): "HW = 1, B = 1, C = 4: the degenerate shape the issue names",
    ("gn", (2, 1, 1024)): "HW = 1 at C = 1024: need = 256 workgroups for two rows, the issue's example",
    ("gn", (2, 70, 48)): "C = 48 of the issue's list", ("gn", (2, 5, 260)): "C = 260 of the issue's list", ("gn", (1, 64, 1028)): "C = 1028 of the issue's list",
    ("gn", (8, 128, 2052)): "C = 2052 of the issue's list",
    ("aff", (2, 5, 3, 1, 0)): "(2, 5, 3): HW C % 4 != 0 at a size where every form runs; the other such case is the 4.2 M-float cap",
}


# ================================================================================================ operands and references
def rows_of(t):
    """(B, C, HW, 1) on the CPU -> what nhwc() puts on the device, as the (B, HW, C) rows a Buf takes."""
    return nhwc(t).view(t.shape[0], t.shape[2], t.shape[1])


def maps_of(v):
    """(B, HW, C) on the device -> (B, C, HW, 1) on the CPU."""
    return nchw(v.unsqueeze(2))


def padc_of(case):
    B, HW, C, v = case
    return 5 if v == 1 and C % 4 == 0 else 4


def relu_mask_from_z(fa, z, fs, fd):
    """[bn_pre(fa, z, fs, fd) > 0]: z - fs rounds to fp32, the multiply-add's sign is that of the exact value."""
    return (fa.double() * (z - fs).double() + fd.double()) > 0


@functools.lru_cache(maxsize=None)
def mom_data(case, kind="exact"):
    """Operands (B, HW, C) and, per form, the reference: fp64 tensors (exact) or longdouble arrays with their bounds (real)."""
    B, HW, C, v = case
    D = NS(kind=kind, case=case, plan=moments_plan(B, HW, C, v))
    if kind == "exact":
        rng = np.random.default_rng([5, B, HW, C])
        D.x, D.x2, D.mask = ints(rng, 3, B, HW, C), ints(rng, 3, B, HW, C), ints(rng, 2, B, HW, C)
        D.gamma, D.fa, D.fd, D.fs = (ints(rng, 2, C) for _ in range(4))
    else:
        D.x, D.x2, D.mask = rnd(B, HW, C, seed=1) * 1.5 + 40.0, rnd(B, HW, C, seed=2) * 1.5 + 40.0, rnd(B, HW, C, seed=3)
        D.gamma, D.fa, D.fd, D.fs = rnd(C, seed=4), rnd(C, seed=5), rnd(C, seed=6), rnd(C, seed=7) + 40.0
    keep = {"x": None, "x x2": None, "x x2 mask": D.mask > 0, "x x2 mA": relu_mask_from_z(D.fa, D.x2, D.fs, D.fd)}
    T = (lambda t: t.double()) if kind == "exact" else (lambda t: t.numpy().astype(LD))
    absv = torch.abs if kind == "exact" else np.abs
    stack = (lambda a, b: torch.stack([a, b], -1)) if kind == "exact" else (lambda a, b: np.stack([a, b], -1))
    D.ref, D.mag = {}, {}
    for form, m in keep.items():
        a = T(D.x if m is None else D.x * m)
        w = a if form == "x" else T(D.x2)
        D.ref[form], D.mag[form] = stack(a.sum(1), (a * w).sum(1)), stack(absv(a).sum(1), absv(a * w).sum(1))
    D.ref["total_only"], D.mag["total_only"] = D.ref["x"].sum(1), D.mag["x"].sum(1)
    g = T(D.gamma)[None, :, None]
    D.ref["gtot"], D.mag["gtot"] = (g * D.ref["x x2"]).sum(1), (absv(g) * D.mag["x x2"]).sum(1)
    D.terms = {f: HW for f in keep} | {"total_only": HW * C, "gtot": HW * C}          # roundings: n - 1 additions (+ 1 product)
    return D


def mom_check(D, form, got, what):
    """got: a (B, C, 2) / (B, 2) fp64 CPU tensor of sums, or the pairs / partials of a workspace still to be added over dim 1."""
    if D.kind == "exact":
        same(got if got.dim() == D.ref[form].dim() else got.sum(1), D.ref[form], what)
        return
    got = got.numpy().astype(LD)
    got = got if got.ndim == D.ref[form].ndim else got.sum(1)
    assert not np.isnan(got).any(), f"{what}: NaN"
    err, bound = np.abs(got - D.ref[form]), D.terms[form] * U53 * D.mag[form]
    share = np.divide(err, bound, out=np.zeros_like(err), where=bound > 0)
    print(f"  {what}: n {D.terms[form]} bound {float(bound.min()):.2e} .. {float(bound.max()):.2e} kernel {float(err.max()):.2e} "
          f"share {float(share.max()):.3f}")
    assert (err <= bound).all(), f"{what}: error {float(err.max()):.3e} above n 2^-53 sum |terms|"


# ---- affine
def aff_coef(rng, Bc, C):
    return ints(rng, 2, Bc, C)


@functools.lru_cache(maxsize=None)
def aff_data(case):
    B, HW, C, ps, padc = case
    rng = np.random.default_rng([6] + list(case))
    Bc = B if ps else 1
    D = NS(case=case, plan=affine_plan(HW, C, C if ps else 0, padc), Bc=Bc)
    D.x1, D.x2, D.mask, D.old = ints(rng, 3, B, HW, C), ints(rng, 3, B, HW, C), ints(rng, 2, B, HW, C), ints(rng, 3, B, HW, C)
    D.A, D.D1, D.S1, D.E, D.D2, D.S2 = (aff_coef(rng, Bc, C) for _ in range(6))
    D.mA, D.mD, D.mS = (ints(rng, 2, C) for _ in range(3))
    return D


def aff_args(D, form):
    """The operands of a form: name -> CPU tensor; pre."""
    g = lambda *names: {n: getattr(D, n) for n in names}
    return {"A S1 D1": (g("x1", "A", "S1", "D1"), 0),
            "full pre 1 add": (g("x1", "A", "S1", "D1", "x2", "E", "S2", "D2") | {"add": D.old}, 1),
            "bare pre 2": (g("x1", "x2") | {"masky": D.mask}, 2),
            "no x1 accumulate": (g("D1", "x2", "E", "D2") | {"add": D.old}, 0),
            "A only": (g("x1", "A"), 0),
            "pre 3": (g("x1", "A", "x2", "E", "D2", "S2", "mA", "mD", "mS"), 3)}[form]


def affine_ref(a, pre, dt, plant=None):
    """out = pre(A (x1 - S1) + D1) + E (x2 - S2) + D2 + add, the subtractions first, in dt.  Coefficients are (Bc, C).
    plant "bstride 0": every sample reads sample 0's coefficients; "no wrap": the flat kernel's channel counter runs on."""
    get = lambda n: None if a.get(n) is None else a[n].to(dt)
    x1, x2, add = get("x1"), get("x2"), get("add")
    B, HW, C = (x1 if x1 is not None else x2).shape

    def co(n, default):
        t = get(n)
        if t is None:
            return default
        if plant == "bstride 0":
            t = t[:1]
        if plant == "no wrap":              # element i of a sample reads entry cb + (4 (i // 4)) % C + i % 4 of the (Bc, C) table
            i = torch.arange(HW * C)
            c = (4 * (i // 4)) % C + i % 4
            flat = torch.cat([t.reshape(-1), torch.full((4,), NAN, dtype=dt)])          # behind the table: anything
            idx = (torch.arange(t.shape[0]) * C)[:, None] + c[None, :]
            return flat[idx].view(t.shape[0], HW, C)
        return t[:, None, :]
    v = co("D1", 0.0)
    if x1 is not None:
        v = co("A", 1.0) * (x1 - co("S1", 0.0)) + v
    if pre == 1:
        v = torch.relu(v)
    elif pre == 2:
        v = v * (a["masky"] > 0)
    elif pre == 3:
        v = v * relu_mask_from_z(a["mA"], a["x2"], a["mS"], a["mD"])
    if x2 is not None:
        v = v + co("E", 1.0) * (x2 - co("S2", 0.0))
    if a.get("D2") is not None:
        v = v + co("D2", 0.0)
    if add is not None:
        v = v + add
    return v.expand(B, HW, C)


def aff_magnitude(D, form):
    a, pre = aff_args(D, form)
    return affine_ref({n: (t.abs() if n not in ("masky", "mA", "mD", "mS") else t) for n, t in a.items()} |
                      ({"S1": -a["S1"].abs()} if "S1" in a else {}) | ({"S2": -a["S2"].abs()} if "S2" in a else {}),
                      0 if pre == 3 else pre, torch.float64).max().item()


@functools.lru_cache(maxsize=None)
def cap_data(case):
    B, HW, C, ps, padc = case
    rng = np.random.default_rng([7] + list(case))
    D = NS(case=case, plan=affine_plan(HW, C, 0, padc))
    D.x1 = torch.from_numpy(rng.integers(-3, 4, (B, HW, C)).astype(np.float32))
    D.A, D.S1, D.D1 = (ints(rng, 2, 1, C) for _ in range(3))
    D.A[D.A == 0] = 1.0
    D.ref = D.A[:, None] * (D.x1 - D.S1[:, None]) + D.D1[:, None]          # integers below 2^24: fp32 is exact
    return D


# ---- the coefficient kernels: their formulas in a floating type T (numpy.float64 or numpy.longdouble)
def np_of(t):
    return t.detach().cpu().numpy()


def norm_coefs(s1, s2, n, eps, gamma, beta, T, plant=None):
    mean = s1 / n
    m = mean.astype(F32).astype(T) if plant == "mean in fp32" else mean
    var = np.maximum(s2 / n - m * m, T(0))
    rstd = 1 / np.sqrt(var + T(F32(eps)))
    return mean, var, rstd


def f_gn_fwd(I, T, plant=None):
    """gn_coef_fwd_kernel (I.mom: (B, C, 2)) and gn_coef_fwd_partial_kernel / gn_apply_fwd_kernel (I.mom: (B, pairs, 2))."""
    m = I.mom.astype(T)
    if plant is not None and plant != "mean in fp32":
        m = np.delete(m, plant, 1)           # a pair skipped
    mean, _, rstd = norm_coefs(m[..., 0].sum(1), m[..., 1].sum(1), T(I.HW) * T(I.C), I.eps, None, None, T, plant)
    one = np.ones((m.shape[0], I.C), T)
    return {"A": rstd[:, None] * I.gamma.astype(T)[None], "D": one * I.beta.astype(T)[None], "S": mean[:, None] * one,
            "mean_rstd": np.stack([mean, rstd], 1)}


def acc32(old, v):
    """(accumulate ? old : 0) + (float)v in fp32."""
    v = v.astype(F32)
    return v if old is None else (old.astype(F32) + v).astype(F32)


def f_gn_bwd(I, T):
    m, g = I.mom.astype(T), I.gamma.astype(T)[None]
    mu, r = I.ms[:, :1].astype(T), I.ms[:, 1:].astype(T)
    s1, s2 = m[..., 0], m[..., 1]
    n = T(I.HW) * T(I.C)
    t1, t2 = (g * s1).sum(1, keepdims=True), (g * (s2 - mu * s1)).sum(1, keepdims=True)
    m1, m2 = t1 / n, r * t2 / n
    one = np.ones_like(s1)
    return {"A": r * g, "E": -r * r * m2 * one, "D": -r * m1 * one, "S": mu * one,
            "dgamma": acc32(I.old.get("dgamma"), (r * (s2 - mu * s1)).sum(0)), "dbeta": acc32(I.old.get("dbeta"), s1.sum(0))}


def f_bn_fwd(I, T, plant=None):
    """bn_coef_fwd_kernel (I.mom: (B, C, 2), n = B HW) and bn_coef_fwd_partial_kernel (I.mom: (chunks, C, 2), n = count)."""
    m = I.mom.astype(T)
    if plant is not None:
        m = np.delete(m, plant, 0)
    g, mom = I.gamma.astype(T), T(F32(I.momentum))
    out = {}
    if I.training:
        n = T(I.n)
        mean, var, _ = norm_coefs(m[..., 0].sum(0), m[..., 1].sum(0), n, I.eps, None, None, T)
        out["running_mean"] = (T(1) - mom) * I.rm.astype(T) + mom * mean
        out["running_var"] = (T(1) - mom) * I.rv.astype(T) + mom * var * (n / (n - T(1)))
    else:
        mean, var = I.rm.astype(T), I.rv.astype(T)
    rstd = 1 / np.sqrt(var + T(F32(I.eps)))
    return out | {"A": rstd * g, "D": I.beta.astype(T), "S": mean, "mean_rstd": np.stack([mean, rstd], 1)}


def f_bn_bwd(I, T, plant=None):
    m = I.mom.astype(T)
    if plant is not None:
        m = np.delete(m, plant, 0)
    s1, s2 = m[..., 0].sum(0), m[..., 1].sum(0)
    mu, r, g, n = I.ms[:, 0].astype(T), I.ms[:, 1].astype(T), I.gamma.astype(T), T(I.n)
    dxh = r * (s2 - mu * s1)
    z = np.zeros_like(s1)
    return {"A": g * r, "E": -g * r * r * (dxh / n) if I.training else z, "D": -g * r * (s1 / n) if I.training else z, "S": mu,
            "dgamma": acc32(I.old.get("dgamma"), dxh), "dbeta": acc32(I.old.get("dbeta"), s1)}


def eca_taps(k, C):
    pad = (k - 1) // 2
    return [(j, c, c + j - pad) for j in range(k) for c in range(C) if 0 <= c + j - pad < C]


def f_eca_fwd(I, T):
    mean = I.mom[..., 0].astype(T) / T(I.HW)
    z = np.zeros((I.B, I.C), T)
    for j, c, cc in eca_taps(I.k, I.C):
        z[:, c] += I.wk.astype(T)[j] * mean[:, cc]
    return {"gate": 1 / (1 + np.exp(-z))}


def f_eca_bwd(I, T):
    g, wk = I.gate.astype(T), I.wk.astype(T)
    q = I.mom2[..., 1].astype(T) * g * (1 - g)                 # d loss / d z
    mean = I.mom[..., 0].astype(T) / T(I.HW)
    dm, dwk = np.zeros((I.B, I.C), T), np.zeros(I.k, T)
    for j, c, cc in eca_taps(I.k, I.C):                         # z[b][c] reads mean[b][cc] through tap j
        dm[:, cc] += wk[j] * q[:, c]
        dwk[j] += (q[:, c] * mean[:, cc]).sum()
    return {"F": dm / T(I.HW), "dwk": acc32(I.old.get("dwk"), dwk)}


def f_ls(I, T):
    s1, s2 = I.mom[..., 0].astype(T).sum(0), I.mom[..., 1].astype(T).sum(0)
    out = {}
    if I.want_dls:
        out["dls"] = acc32(I.old.get("dls"), s2)
    if I.want_dbias:
        out["dbias"] = acc32(I.old.get("dbias"), (I.ls.astype(T) if I.ls is not None else T(1)) * s1)
    return out


def f_m2f(I, T):
    return {"out": I.mom.reshape(-1, 2)[:I.n, I.which].astype(T) * T(I.scale)}


FORMULAS = dict(gn_fwd=f_gn_fwd, gn_bwd=f_gn_bwd, bn_fwd=f_bn_fwd, bn_bwd=f_bn_bwd, eca_fwd=f_eca_fwd, eca_bwd=f_eca_bwd, ls=f_ls,
                m2f=f_m2f)


def coef_reference(I, plant=None):
    """Per output: the longdouble value rounded to fp32, one ulp of it, d64 and the bound ulp + 4 d64."""
    f = FORMULAS[I.formula]
    r64, rld = f(I, F64), (f(I, LD) if plant is None else f(I, LD, plant))
    R = {}
    for name in rld:
        ref32 = rld[name].astype(F32)
        ulp = np.spacing(np.abs(ref32)).astype(LD)
        d64 = np.abs(r64[name].astype(LD) - rld[name].astype(LD)) if plant is None else np.zeros_like(ulp)
        R[name] = NS(ref32=ref32, ulp=ulp, d64=d64, bound=ulp + 4 * d64)
    return R


def stat_moments(rng, lead, C, n_each, mean=40.0, std=1.5):
    """(lead, C, 2) fp64 sums of n_each values per entry around `mean`: consistent (every entry's variance > 0), |mean| >> std."""
    m = mean + std * rng.standard_normal((lead, C))
    v = std * std * (0.5 + rng.random((lead, C)))
    return np.stack([n_each * m, n_each * (m * m + v)], -1)


def grad_moments(rng, lead, C, n_each):
    """(sum dy, sum dy x) per entry: dy of mean 0.5, correlated with x so that neither parameter gradient cancels."""
    s1 = n_each * (0.5 + 0.3 * rng.standard_normal((lead, C)))
    return np.stack([s1, 40.0 * s1 + n_each * (0.8 + 0.3 * rng.standard_normal((lead, C)))], -1)


def f32s(rng, *shape, scale=1.0, shift=0.0):
    return (shift + scale * rng.standard_normal(shape)).astype(F32)


def coef_inputs(key, draw):
    """The given inputs of a coefficient case.  key: (formula tag, parameters...)."""
    kind = key[0]
    rng = np.random.default_rng([11, draw] + [zlib.crc32(str(k).encode()) % 9973 for k in key])
    I = NS(key=key, old={})
    if kind in ("gn_coef_fwd", "gn_pairs"):
        B, HW, C, per = key[1:5]
        I.__dict__.update(formula="gn_fwd", B=B, HW=HW, C=C, eps=1e-5, gamma=f32s(rng, C, scale=0.3, shift=1.0), beta=f32s(rng, C, scale=0.5))
        I.mom = stat_moments(rng, B, per, HW * C / per)
        if kind == "gn_pairs":
            I.x = torch.from_numpy(f32s(rng, B, HW, C, scale=1.5, shift=40.0))
    elif kind == "gn_coef_bwd":
        B, HW, C, acc = key[1:5]
        I.__dict__.update(formula="gn_bwd", B=B, HW=HW, C=C, gamma=f32s(rng, C, scale=0.3, shift=1.0), mom=grad_moments(rng, B, C, HW),
                          ms=np.stack([f32s(rng, B, shift=40.0), f32s(rng, B, scale=0.05, shift=0.7)], 1))
        if acc:
            I.old = dict(dgamma=f32s(rng, C, shift=3.0), dbeta=f32s(rng, C, shift=3.0))
    elif kind in ("bn_coef_fwd", "bn_chunks_fwd"):
        lead, n, C, training = key[1:5]          # lead: B or the number of chunk partials; n: values per channel
        I.__dict__.update(formula="bn_fwd", lead=lead, n=n, C=C, training=training, eps=1e-3, momentum=0.03,
                          gamma=f32s(rng, C, scale=0.3, shift=1.0), beta=f32s(rng, C, scale=0.5), rm=f32s(rng, C, shift=39.0),
                          rv=(0.5 + rng.random(C)).astype(F32), mom=stat_moments(rng, lead, C, n / lead))
    elif kind in ("bn_coef_bwd", "bn_chunks_bwd"):
        lead, n, C, training, acc = key[1:6]
        I.__dict__.update(formula="bn_bwd", lead=lead, n=n, C=C, training=training, gamma=f32s(rng, C, scale=0.3, shift=1.0),
                          mom=grad_moments(rng, lead, C, n / lead),
                          ms=np.stack([f32s(rng, C, shift=40.0), f32s(rng, C, scale=0.05, shift=0.7)], 1))
        if acc:
            I.old = dict(dgamma=f32s(rng, C, shift=3.0), dbeta=f32s(rng, C, shift=3.0))
    elif kind == "eca":
        k, B, C, acc = key[1:5]
        HW = 37
        I.__dict__.update(formula="eca_bwd", fwd="eca_fwd", k=k, B=B, C=C, HW=HW, wk=f32s(rng, k, scale=0.7),
                          mom=stat_moments(rng, B, C, HW, mean=0.4, std=1.0), mom2=grad_moments(rng, B, C, HW),
                          gate=(0.1 + 0.8 * rng.random((B, C))).astype(F32))
        if acc:
            I.old = dict(dwk=f32s(rng, k, shift=3.0))
    elif kind == "ls":
        B, C, has_ls, want_dls, want_dbias, acc = key[1:7]
        I.__dict__.update(formula="ls", B=B, C=C, ls=f32s(rng, C, scale=0.2, shift=0.5) if has_ls else None, want_dls=want_dls,
                          want_dbias=want_dbias, mom=grad_moments(rng, B, C, 50))
        if acc:
            I.old = dict(dls=f32s(rng, C, shift=3.0), dbias=f32s(rng, C, shift=3.0))
    elif kind == "m2f":
        n, which = key[1:3]
        I.__dict__.update(formula="m2f", n=n, which=which, scale=1.0 / 49, mom=stat_moments(rng, 1, n, 49)[0])
    return I


@functools.lru_cache(maxsize=None)
def coef_case(key):
    """Inputs redrawn until d64 < ulp / 16 on every output of the reference."""
    for draw in range(MAX_DRAWS):
        I = coef_inputs(key, draw)
        formulas = [I.formula] + ([I.fwd] if hasattr(I, "fwd") else [])
        R = {}
        for f in formulas:
            I.formula = f
            R |= coef_reference(I)
        I.formula = formulas[0]
        if all(bool((r.d64 < r.ulp / 16).all()) for r in R.values()):
            break
    I.draw, I.R = draw, R
    I.well = all(bool((r.d64 < r.ulp / 16).all()) for r in R.values())
    return I


def coef_close(what, R, got):
    """got: name -> fp32 values (numpy or tensor).  |got - ref32| <= ulp + 4 d64 per output."""
    for name, r in R.items():
        g = np_of(got[name]).astype(F32).reshape(r.ref32.shape) if torch.is_tensor(got[name]) else got[name].reshape(r.ref32.shape)
        assert not np.isnan(g).any(), f"{what} {name}: NaN"
        err = np.abs(g.astype(LD) - r.ref32.astype(LD))
        print(f"  {what} {name}: d64 / ulp {float((r.d64 / r.ulp).max()):.2e} kernel / bound {float((err / r.bound).max()):.3f}")
        assert (err <= r.bound).all(), f"{what} {name}: {float((err / r.bound).max()):.3f} of the bound (one ulp + 4 d64)"


def nbt_check(before, after, what):
    assert after == before + 1, f"{what}: num_batches_tracked went from {before} to {after}"


COEF_KEYS = ([("gn_coef_fwd", B, HW, C, C) for B, HW, C in GN_COEF] + [("gn_pairs", 2, 3, 8, per) for per in PAIR_COUNTS] +
             [("gn_coef_bwd", B, HW, C, acc) for B, HW, C in GN_COEF for acc in (0, 1)] +
             [("bn_coef_fwd", B, B * HW, C, tr) for B, HW, C in BN_COEF for tr in (1, 0)] +
             [("bn_coef_bwd", B, B * HW, C, tr, acc) for B, HW, C in BN_COEF for tr, acc in ((1, 0), (0, 1))] +
             [("bn_chunks_fwd", t, 16 * t + 3, C, 1) for t in BN_TOTALS for C in BN_CHUNK_C] +
             [("bn_chunks_bwd", t, 16 * t + 3, C, tr, acc) for t in BN_TOTALS for C in BN_CHUNK_C for tr, acc in ((1, 0), (0, 1))] +
             [("eca", k, B, C, acc) for k in ECA_K for B, C in ECA_BC for acc in (0, 1)] +
             [("ls", *LS_CASE, *f) for f in ((1, 1, 1, 0), (0, 1, 1, 1), (1, 0, 1, 0), (1, 1, 0, 1))] +
             [("m2f", M2F_N, w) for w in (0, 1)])


# ---- GroupNorm and BatchNorm chains
def gn_ref(x, gam, bet, g, dt):
    xs, gs, bs = (t.detach().to(dt, copy=True).requires_grad_(True) for t in (x, gam, bet))
    y = F.group_norm(xs, 1, gs, bs, 1e-5)
    y.backward(g.to(dt))
    return y.detach(), xs.grad, gs.grad, bs.grad


def grad_cond(terms):
    """sum |terms| / |sum| of the largest element of a parameter gradient; terms: (C, n)."""
    s = terms.sum(1)
    return (terms.abs().sum(1)[s.abs().argmax()] / s.abs().max()).item()


@functools.lru_cache(maxsize=None)
def gn_data(case):
    B, HW, C = case
    D = NS(kind="rounded", case=case)
    for D.draw in range(MAX_DRAWS):
        s = 100 * D.draw
        n = rnd(B, C, HW, 1, seed=s + 1)
        D.x, D.g = n * 1.5 + 10.0, rnd(B, C, HW, 1, seed=s + 4) + 1.0 + 0.5 * n
        D.gam, D.bet, D.add = rnd(C, seed=s + 2) * 0.3 + 1, rnd(C, seed=s + 3) * 0.5, rnd(B, C, HW, 1, seed=s + 5)
        D.y, D.dx, D.dgam, D.dbet = gn_ref(D.x, D.gam, D.bet, D.g, torch.float64)
        xd = D.x.double()
        mu = xd.mean((1, 2, 3), keepdim=True)
        D.rstd = torch.rsqrt(((xd - mu) ** 2).mean((1, 2, 3), keepdim=True) + 1e-5)
        D.mean = mu
        xhat = (xd - mu) * D.rstd
        per_c = lambda t: t.permute(1, 0, 2, 3).reshape(C, -1)
        D.cond = max(grad_cond(per_c(D.g.double() * xhat)), grad_cond(per_c(D.g.double())))
        if D.cond <= COND_LIMIT:
            break
    y32, dx32, dg32, db32 = gn_ref(D.x, D.gam, D.bet, D.g, torch.float32)
    D.old_g, D.old_b = rnd(C, seed=31) + 3, rnd(C, seed=32) + 3
    D.R = dict(y=bound_of(y32, D.y), dx=bound_of(D.add + dx32, D.add.double() + D.dx), dgam=bound_of(D.old_g + dg32, D.old_g.double() + D.dgam),
               dbet=bound_of(D.old_b + db32, D.old_b.double() + D.dbet))
    return D


def gn_pairs(D, per):
    """`per` (sum, sum of squares) pairs per sample, fp64: rows r with r % per == i make pair i (an empty one is (0, 0))."""
    B, HW, C = D.case
    xd = D.x.double().squeeze(3)                 # (B, C, HW)
    pairs = torch.zeros(B, per, 2, dtype=torch.float64)
    for i in range(per):
        blk = xd[:, :, i::per]
        pairs[:, i, 0], pairs[:, i, 1] = blk.sum((1, 2)), (blk * blk).sum((1, 2))
    return pairs


def gn_tile_partials(D):
    """What a producing conv leaves for gn_apply_bwd_from_partials: partial [B HW / 32][C][2] of (dy, dy x), tile_totals
    [B HW / 32][ceil(C / 32)][2] weighted by gamma."""
    B, HW, C = D.case
    g, x = D.g.double().squeeze(3).permute(0, 2, 1), D.x.double().squeeze(3).permute(0, 2, 1)          # (B, HW, C)
    t = torch.stack([g, g * x], -1).view(B * HW // 32, 32, C, 2).sum(1)
    w = t * D.gam.double()[None, :, None]
    nb = cdiv(C, 32)
    tot = torch.stack([w[:, 32 * j:32 * (j + 1)].sum(1) for j in range(nb)], 1)
    return t.contiguous(), tot.contiguous()


def bn_ref(z, gam, bet, rm, rv, g, dt):
    zs, gs, bs = (t.detach().to(dt, copy=True).requires_grad_(True) for t in (z, gam, bet))
    rm, rv = rm.to(dt, copy=True), rv.to(dt, copy=True)
    pre = F.batch_norm(zs, rm, rv, gs, bs, True, 0.03, 1e-3)
    y = torch.relu(pre)
    y.backward(g.to(dt))
    return NS(y=y.detach(), pre=pre.detach(), dz=zs.grad, dgam=gs.grad, dbet=bs.grad, rm=rm, rv=rv)


@functools.lru_cache(maxsize=None)
def bn_data(case):
    B, HW, C = case
    D = NS(kind="rounded", case=case)
    for D.draw in range(MAX_DRAWS):
        s = 100 * D.draw
        n = rnd(B, C, HW, 1, seed=s + 1)
        D.z, D.g = n * 1.5 + 40.0, rnd(B, C, HW, 1, seed=s + 6) + 1.0 + 0.5 * n
        D.gam, D.bet = rnd(C, seed=s + 2) * 0.3 + 1, rnd(C, seed=s + 3) * 0.5
        D.rm0, D.rv0 = rnd(C, seed=s + 4) * 0.1, rnd(C, seed=s + 5, kind="uniform") + 0.5
        D.r = bn_ref(D.z, D.gam, D.bet, D.rm0, D.rv0, D.g, torch.float64)
        live = (D.r.pre > 0).double()
        zd = D.z.double()
        mu = zd.mean((0, 2, 3), keepdim=True)
        xhat = (zd - mu) * torch.rsqrt(((zd - mu) ** 2).mean((0, 2, 3), keepdim=True) + 1e-3)
        per_c = lambda t: t.permute(1, 0, 2, 3).reshape(C, -1)
        D.cond = max(grad_cond(per_c(D.g.double() * live * xhat)), grad_cond(per_c(D.g.double() * live)))
        D.margin = D.r.pre.abs().min().item()
        if D.cond <= COND_LIMIT and D.margin >= 2e-6:
            break
    r32 = bn_ref(D.z, D.gam, D.bet, D.rm0, D.rv0, D.g, torch.float32)
    D.old_g, D.old_b = rnd(C, seed=31) + 3, rnd(C, seed=32) + 3
    D.R = dict(y=bound_of(r32.y, D.r.y), dz=bound_of(r32.dz, D.r.dz), rm=bound_of(r32.rm, D.r.rm), rv=bound_of(r32.rv, D.r.rv),
               dgam=bound_of(D.old_g + r32.dgam, D.old_g.double() + D.r.dgam), dbet=bound_of(D.old_b + r32.dbet, D.old_b.double() + D.r.dbet))
    return D


# ================================================================================================ tests that need no GPU
def test_cases_reach_the_branches_they_are_named_after():
    reached = branches()
    assert reached == ALL_BRANCHES, (sorted(map(str, ALL_BRANCHES - reached)), sorted(map(str, reached - ALL_BRANCHES)))


def test_every_case_is_needed_or_a_named_duplicate():
    spare = {(name, case) for name, table, _ in CASE_TABLES for case in table if branches(skip=(name, case)) == ALL_BRANCHES}
    assert spare == set(DUPLICATES), (sorted(spare - set(DUPLICATES)), sorted(set(DUPLICATES) - spare))


def test_moments_plans_of_the_case_table():
    plan = lambda c: moments_plan(*c)
    assert all(c[3] == 1 or c[2] % 4 == 0 for c in MOM_CASES) and len(set(MOM_CASES)) == len(MOM_CASES)
    p = plan((1, 128, 20, 4)); assert (p.TPR, p.CV, p.why, p.rows, p.RP) == (8, 5, "floor 1", 128, 32) and plan((1, 129, 20, 4)).rows == 129
    p = plan((2, 1, 1024, 4)); assert (p.TPR, p.RP, p.ncb, p.rows) == (256, 1, 1, 1)
    p = plan((1, 64, 1028, 4)); assert (p.nc, p.nchunks, p.rows, p.last, p.ncb, p.live) == (17, 16, 4, 4, 2, 1)          # the issue's example
    p = plan((1, 64, 2048, 4)); assert (p.ncb, p.live, p.nchunks) == (2, 256, 32)
    p = plan((8, 128, 2052, 4)); assert (p.why, p.nc, p.nchunks, p.rows, p.last, p.ncb, p.live) == ("by_grid", 43, 43, 3, 2, 3, 1)
    p = plan((1, 8200, 256, 4)); assert (p.why, p.nc, p.nchunks, p.rows, p.last) == ("cap 512", 512, 483, 17, 6)
    p = plan((1, 3, 4100, 4)); assert (p.why, p.nc, p.ncb, p.live) == ("HW", 3, 5, 1)
    p = plan((1, 20, 257, 1)); assert (p.ncb, p.live) == (2, 1)
    p = plan((8, 128, 1028, 1)); assert (p.why, p.nchunks, p.ncb, p.live, p.last) == ("by_grid", 26, 5, 4, 3)
    p = plan(MOM_REAL); assert p.TPR == 16 > p.CV == 12
    assert all(c in MOM_CASES for c in SHORT_CHUNK + CHANNEL_BLOCKS)


def test_restated_plans_are_the_librarys(lib):
    shapes = {c[:3] for c in MOM_CASES} | set(GN_CASES) | set(GN_PARTIALS) | set(BN_CASES) | {MOM_REAL[:3]}
    for B, HW, C in sorted(shapes):
        assert moments_workspace(B, HW, C) == lib._lib.vrnet_moments_workspace(B, HW, C), (B, HW, C)
        assert gn_bwd_workspace(B, HW, C) == lib._lib.vrnet_gn_bwd_workspace(B, HW, C), (B, HW, C)
        assert moments_workspace(B, HW, C) % 8 == 0 and gtot_offset(B, HW, C) + B * 2048 * 16 <= gn_bwd_workspace(B, HW, C)


SWEEP_B, SWEEP_HW = [1, 2, 3, 8, 64, 1025], list(range(1, 71)) + [1024, 4104, 16384]
SWEEP_C = list(range(1, 41)) + [48, 96, 240, 256, 260, 384, 1024, 1028, 2052, 4096, 4100]


def test_the_two_sizes_the_workspace_formulas_rely_on(lib):
    shapes = [(B, HW, C) for B in SWEEP_B for HW in SWEEP_HW for C in SWEEP_C] + [c[:3] for c in MOM_CASES] + GN_CASES + BN_CASES
    for n, (B, HW, C) in enumerate(shapes):
        for v in (1, 4) if C % 4 == 0 else (1,):
            p = moments_plan(B, HW, C, v)
            assert p.nchunks * p.ncb <= 2048, (B, HW, C, v)                            # gtot: B * 512 * 4 pairs
            assert p.nchunks * p.ncb * 2 <= p.nchunks * C * 2, (B, HW, C, v)           # total_only pairs inside partial
            assert 1 <= p.nchunks <= p.nc <= 512 and 1 <= p.last <= p.rows and 1 <= p.live <= p.TPR
            assert B * p.nchunks * C * 16 + 256 <= moments_workspace(B, HW, C)
        if n % 97 == 0:
            assert moments_workspace(B, HW, C) == lib._lib.vrnet_moments_workspace(B, HW, C), (B, HW, C)


def test_affine_plans_of_the_case_table():
    plan = lambda c: affine_plan(c[1], c[2], c[2] if c[3] else 0, c[4])
    assert [plan(c).kernel for c in AFF_CASES[:3]] == ["<4>"] * 3
    assert [(plan(c).trips, plan(c).tail, plan(c).blocks) for c in AFF_CASES[:3]] == [(0, True, 1), (1, False, 1), (1, True, 1)]
    assert all(plan(c).kernel == "flat" for c in AFF_CASES[3:19]) and len(AFF_CASES[3:19]) == 2 * len(FLAT_C)
    assert [(plan(c).trips, plan(c).tail) for c in AFF_CASES[17:19]] == [(1, False), (1, True)]
    assert [plan(c).why for c in AFF_CASES[19:]] == ["C > 16", "HW C % 4", "ld % 4", "strided", "strided"]
    assert [(plan(c).trips, plan(c).tail) for c in AFF_CASES[22:]] == [(1, False), (1, True)]
    for c, kernel, floats in zip(AFF_CAPS, ("<4>", "flat", "<1>"), (16.8e6, 16.8e6, 4.2e6)):
        p = plan(c)
        assert p.kernel == kernel and p.capped and p.blocks == 4096 and p.trips == 2 and p.tail and c[1] * c[2] < floats * 1.001
        assert p.n > 4 * p.stride          # the elements behind 4096 blocks x 2 trips x 2 exist
    assert not any(plan(c).capped for c in AFF_CASES)


def test_groupnorm_grids_of_the_case_table():
    assert [gn_fwd_bx(*c).rule for c in GN_CASES] == ["bx 1"] * 4 + ["free"] * 3 + ["capped"]
    assert [gn_bwd_bx(*c).rule for c in GN_CASES] == ["free"] + ["raised to need"] * 5 + ["free", "capped"]
    assert gn_bwd_bx(1, 1, 4).bx == 1 and gn_bwd_bx(1, 8200, 256).bx == cdiv(8200 * 64, 1024) > 64
    assert gn_bwd_bx(2, 1, 1024).bx == 256 and gn_bwd_bx(1025, 1120, 8).bx == 2 == gn_fwd_bx(1025, 1120, 8).bx
    assert [gn_bwd_bx(*c).rule for c in GN_PARTIALS] == ["raised to need", "free", "capped"]
    assert all(c[1] % 32 == 0 and c[2] % 4 == 0 for c in GN_PARTIALS) and all(c[2] % 4 == 0 for c in GN_CASES)
    assert moments_plan(1, 8200, 256, 4).gper == 483 and 4128 // 32 * cdiv(40, 32) == 258
    assert coef_grid("bn_partial", C=5) == (2, 256) and coef_grid("bn_partial", C=7)[0] * 4 - 7 == 1
    assert coef_grid("gn_coef_bwd", B=3, C=260)[0] == 5 and coef_grid("bn_coef_fwd", C=131)[0] == 2
    assert coef_grid("eca_coef", B=3, C=100)[0] == 2 and coef_grid("ls_coef_bwd", C=129)[0] == 2
    assert coef_grid("moments_to_float", n=M2F_N)[0] == 2 and coef_grid("moments_reduce", B=3, C=5)[0] == 2 and 30 % 16


def test_exact_cases_stay_in_range():
    for case in MOM_CASES:
        D = mom_data(case)
        assert max(m.max().item() for m in D.mag.values()) < 2.0 ** 53, case
    for case in AFF_CASES:
        D = aff_data(case)
        for form in AFF_FORMS:
            assert aff_magnitude(D, form) < EXACT_LIMIT, (case, form)
    for case in AFF_CAPS:
        assert cap_data(case).ref.abs().max().item() < EXACT_LIMIT


def test_coefficient_references_are_well_conditioned():
    """d64 < ulp / 16 on every output; which cases took a second draw."""
    redrawn = [I.key for I in map(coef_case, COEF_KEYS) if I.draw]
    assert all(coef_case(k).well for k in COEF_KEYS)
    print("cases that took a second draw:", redrawn)
    assert redrawn == []                    # the docstring says so


def test_chain_references_are_conditioned_and_below_the_suite_tolerance():
    for D in [gn_data(c) for c in GN_CASES[:6] + GN_PARTIALS[:1]] + [bn_data(c) for c in BN_CASES]:
        assert D.cond <= COND_LIMIT and D.draw == 0, (D.case, D.cond, D.draw)
        for name, R in D.R.items():
            assert 4 * ULP_FLOOR <= R.bound <= TOL, (D.case, name, R)
    assert all(bn_data(c).margin >= 2e-6 for c in BN_CASES)


def test_formulas_agree_with_autograd():
    """f_gn_fwd / f_gn_bwd / f_bn_fwd / f_bn_bwd, which the sensitivity tests plant errors in, against ATen in fp64."""
    D = gn_data((2, 70, 48))
    B, HW, C = D.case
    xd, gd = D.x.double().squeeze(3), D.g.double().squeeze(3)          # (B, C, HW)
    I = NS(formula="gn_fwd", B=B, HW=HW, C=C, eps=1e-5, gamma=np_of(D.gam), beta=np_of(D.bet), mom=np_of(torch.stack([xd.sum(2), (xd * xd).sum(2)], -1)))
    r = f_gn_fwd(I, F64)
    y = torch.from_numpy(r["A"])[:, :, None] * (xd - torch.from_numpy(r["S"])[:, :, None]) + torch.from_numpy(r["D"])[:, :, None]
    assert dist(y, D.y.squeeze(3)) < 1e-12
    I = NS(formula="gn_bwd", B=B, HW=HW, C=C, gamma=np_of(D.gam), ms=r["mean_rstd"], old={}, mom=np_of(torch.stack([gd.sum(2), (gd * xd).sum(2)], -1)))
    q = f_gn_bwd(I, F64)
    t = lambda n: torch.from_numpy(q[n].astype(F64))
    dx = t("A")[:, :, None] * gd + t("E")[:, :, None] * (xd - t("S")[:, :, None]) + t("D")[:, :, None]
    assert dist(dx, D.dx.squeeze(3)) < 1e-6 and dist(t("dgamma"), D.dgam) < 1e-6 and dist(t("dbeta"), D.dbet) < 1e-6
    D = bn_data((2, 70, 48))
    zd, gd = D.z.double().squeeze(3), (D.g.double() * (D.r.pre > 0)).squeeze(3)
    I = NS(formula="bn_fwd", n=2 * 70, C=48, training=1, eps=1e-3, momentum=0.03, gamma=np_of(D.gam), beta=np_of(D.bet), rm=np_of(D.rm0),
           rv=np_of(D.rv0), mom=np_of(torch.stack([zd.sum(2), (zd * zd).sum(2)], -1)))
    r = f_bn_fwd(I, F64)
    assert dist(torch.from_numpy(r["running_mean"]), D.r.rm) < 1e-6 and dist(torch.from_numpy(r["running_var"]), D.r.rv) < 1e-6
    I = NS(formula="bn_bwd", n=2 * 70, C=48, training=1, gamma=np_of(D.gam), ms=r["mean_rstd"], old={}, mom=np_of(torch.stack([gd.sum(2), (gd * zd).sum(2)], -1)))
    q = f_bn_bwd(I, F64)
    t = lambda n: torch.from_numpy(q[n].astype(F64))
    dz = t("A")[None, :, None] * gd + t("E")[None, :, None] * (zd - t("S")[None, :, None]) + t("D")[None, :, None]
    assert dist(dz, D.r.dz.squeeze(3)) < 1e-6 and dist(t("dgamma"), D.r.dgam) < 1e-6 and dist(t("dbeta"), D.r.dbet) < 1e-6


# ---- sensitivity: errors planted in the reference must be rejected by the comparisons the GPU tests use
def test_sensitivity_moments_chunks_and_channel_blocks():
    """The short last chunk skipped; channel block 1 aliased onto block 0; the one live thread of the last block dropped."""
    for case in SHORT_CHUNK:
        B, HW, C, v = case
        D, p = mom_data(case), moments_plan(*case)
        assert p.last < p.rows
        head = (p.nchunks - 1) * p.rows
        for form in ("x", "x x2"):
            a = D.x[:, :head].double()
            wrong = torch.stack([a.sum(1), (a * (a if form == "x" else D.x2[:, :head].double())).sum(1)], -1)
            rejected(lambda: mom_check(D, form, wrong, "last chunk skipped"))
            mom_check(D, form, D.ref[form].clone(), "the reference itself")
        rejected(lambda: mom_check(D, "total_only", wrong.sum(1), "last chunk skipped"))
    for case in CHANNEL_BLOCKS:
        D, p = mom_data(case), moments_plan(*case)
        per = p.TPR * p.v
        assert p.ncb > 1
        wrong = D.ref["x x2"].clone()
        wrong[:, per:2 * per] = D.ref["x x2"][:, :wrong[:, per:2 * per].shape[1]]
        rejected(lambda: mom_check(D, "x x2", wrong, "channel block aliased"))
        if p.live == 1:
            wrong = D.ref["x x2"].clone()
            wrong[:, -p.v:] = 0.0
            rejected(lambda: mom_check(D, "x x2", wrong, "live thread dropped"))
            g = D.gamma.double()[None, :, None]
            rejected(lambda: mom_check(D, "gtot", (g * wrong).sum(1), "live thread dropped from gtot"))
            rejected(lambda: mom_check(D, "total_only", D.ref["total_only"] - D.ref["x"][:, -p.v:].sum(1), "live thread dropped from the totals"))
    R = mom_data(MOM_REAL, "real")
    for form in MOM_FORMS:
        mom_check(R, form, torch.from_numpy(R.ref[form].astype(F64)), "the reference rounded to fp64")
        rejected(lambda: mom_check(R, form, torch.from_numpy(R.ref[form].astype(F32).astype(F64)), "sums kept in fp32"))


def test_sensitivity_pair_and_partial_loops():
    """The pair at index 256 or 512 skipped in the two-per-trip loop; the partial at index 64 or 256 in bn_channel_sums."""
    for per, skip in ((257, 256), (513, 256), (513, 512), (769, 512), (769, 256)):
        I = coef_case(("gn_pairs", 2, 3, 8, per))
        wrong = {n: r.ref32 for n, r in coef_reference(I, plant=skip).items()}
        coef_close("the reference itself", I.R, {n: r.ref32 for n, r in I.R.items()})
        rejected(lambda: coef_close("pair skipped", {n: I.R[n] for n in ("A", "S", "mean_rstd")}, wrong))
    for t, skip in ((65, 64), (257, 64), (257, 256), (449, 256)):
        for key in (("bn_chunks_fwd", t, 16 * t + 3, 5, 1), ("bn_chunks_bwd", t, 16 * t + 3, 5, 1, 0)):
            I = coef_case(key)
            wrong = {n: r.ref32 for n, r in coef_reference(I, plant=skip).items()}
            for name in ("S", "running_mean") if key[0] == "bn_chunks_fwd" else ("dgamma", "dbeta", "D"):
                rejected(lambda: coef_close("partial skipped", {name: I.R[name]}, wrong))


def test_sensitivity_mean_rounded_before_the_variance():
    """var = s2 / n - fl32(mean)^2 at |mean| >> std."""
    for key in [k for k in COEF_KEYS if k[0] in ("gn_coef_fwd", "gn_pairs")]:
        I = coef_case(key)
        wrong = {n: r.ref32 for n, r in coef_reference(I, plant="mean in fp32").items()}
        rejected(lambda: coef_close("mean in fp32", {"A": I.R["A"]}, wrong))
        rejected(lambda: coef_close("mean in fp32", {"mean_rstd": I.R["mean_rstd"]}, wrong))


def test_sensitivity_num_batches_tracked():
    for C in (5, 7, 131):
        blocks = max(coef_grid("bn_partial", C=C)[0], coef_grid("bn_coef_fwd", C=C)[0])
        assert blocks > 1
        nbt_check(4, 5, "once")
        rejected(lambda: nbt_check(4, 4 + blocks, "once per block"))


def test_sensitivity_affine():
    """The flat kernel's channel counter not wrapped; per-sample coefficients read with bstride 0; the elements behind
    4096 blocks x 2 trips left unwritten."""
    for case in [(1, 400, 3, 0, 0), (2, 800, 3, 1, 0)]:
        D = aff_data(case)
        assert case in AFF_CASES
        for form in ("A S1 D1", "full pre 1 add", "no x1 accumulate", "A only"):
            a, pre = aff_args(D, form)
            ref = affine_ref(a, pre, torch.float64)
            same(ref.float(), ref, "the reference itself")
            rejected(lambda: same(affine_ref(a, pre, torch.float64, "no wrap").float(), ref, "counter not wrapped"))
            if case[3]:
                rejected(lambda: same(affine_ref(a, pre, torch.float64, "bstride 0").float(), ref, "bstride 0"))
    D = cap_data(AFF_CAPS[2])
    wrong = D.ref.clone()
    wrong.view(-1)[2 * 2 * D.plan.stride:] = NAN
    assert D.plan.n > 4 * D.plan.stride
    rejected(lambda: same(wrong, D.ref, "tail unwritten"))


# ================================================================================================ running a case on the GPU
def dbuf(n, fill=PAT, data=None):
    """n doubles inside guards (a Buf of 2 n floats); .d is the fp64 view."""
    b = Buf((2 * n,), fill, padc=0)
    b.d = b.v.view(torch.float64)
    if data is not None:
        b.d.copy_(data.reshape(-1))
    return b


def workspace(need, poison):
    assert need % 8 == 0
    ws = torch.full((need // 4 + GUARD,), poison, device="cuda")
    ws.view(torch.int32)[need // 4:] = PAT
    return ws


def ws_doubles(ws, byte_offset, n):
    return ws[byte_offset // 4:byte_offset // 4 + 2 * n].view(torch.float64).cpu()


def guard_ok(ws, need):
    return bool((ws.view(torch.int32)[need // 4:] == PAT).all())


def untouched(*bufs):
    torch.cuda.synchronize()
    return all(bool((b.flat.view(torch.int32) == PAT).all()) for b in bufs)


def run_moments(hip, D, poison, short=0):
    """Every form of the moments pass on the caller's workspace.  -> form -> fp64 CPU tensor, or the return codes when short."""
    B, HW, C, v = D.case
    p, L, ptr, st = D.plan, hip._lib, hip.ptr, hip.stream()
    padc = padc_of(D.case)
    xb, x2b, mb = (Buf((B, HW, C), NAN, t.cuda(), padc=padc) for t in (D.x, D.x2, D.mask))
    gam, fa, fd, fs = (vec(t) for t in (D.gamma, D.fa, D.fd, D.fs))
    need, need_gn = L.vrnet_moments_workspace(B, HW, C), L.vrnet_gn_bwd_workspace(B, HW, C)
    got, rcs, outs = {}, [], []
    for form in ("x", "x x2", "x x2 mask"):
        ws, ob = workspace(need, poison), dbuf(B * C * 2)
        rcs.append(L.vrnet_moments_f32(ptr(xb.v), xb.ld, ptr(x2b.v) if form != "x" else None, x2b.ld, ptr(mb.v) if "mask" in form else None,
                                       mb.ld, B, HW, C, ptr(ob.d), ptr(ws), need - short, st))
        assert guard_ok(ws, need) and ob.intact(), f"{D.case} {form}: a guard changed"
        got[form] = ob.d.cpu().view(B, C, 2)
        outs.append(ob)
    ms = vec(torch.tensor([0.0, 1.0]).repeat(max(B, C)))
    co = [out_vec(C) for _ in range(6)]
    ws = workspace(need, poison)
    rcs.append(L.vrnet_bn_stats_bwd_zmask(ptr(xb.v), xb.ld, ptr(x2b.v), x2b.ld, ptr(fa.v), ptr(fd.v), ptr(fs.v), ptr(ms.v), ptr(gam.v), 1, B, HW,
                                          C, *[ptr(c.v) for c in co], 0, ptr(ws), need - short, st))
    assert guard_ok(ws, need) and all(c.intact() for c in co)
    got["x x2 mA"] = ws_doubles(ws, 0, B * p.nchunks * C * 2).view(B, p.nchunks, C, 2)
    outs += co
    co = [out_vec(B * C) for _ in range(3)] + [out_vec(2 * B)]
    ws = workspace(need, poison)
    rcs.append(L.vrnet_gn_stats_fwd(ptr(xb.v), xb.ld, ptr(gam.v), ptr(fd.v), 1e-5, B, HW, C, *[ptr(c.v) for c in co], None, None, ptr(ws),
                                    need - short, st))
    assert guard_ok(ws, need) and all(c.intact() for c in co)
    got["total_only"] = ws_doubles(ws, 0, B * p.gper * 2).view(B, p.gper, 2)
    outs += co
    if v == 4:
        dxb, dg, db = Buf((B, HW, C), PAT), out_vec(C), out_vec(C)
        ws = workspace(need_gn, poison)
        rcs.append(L.vrnet_gn_apply_bwd(ptr(xb.v), xb.ld, ptr(x2b.v), x2b.ld, ptr(ms.v), ptr(gam.v), B, HW, C, None, 0, ptr(dxb.v), dxb.ld,
                                        ptr(dg.v), ptr(db.v), 0, ptr(ws), need_gn - short, st))
        assert guard_ok(ws, need_gn) and dxb.intact() and dg.intact() and db.intact()
        got["gtot"] = ws_doubles(ws, gtot_offset(B, HW, C), B * p.gper * 2).view(B, p.gper, 2)
        got["gtot partial"] = ws_doubles(ws, 0, B * p.nchunks * C * 2).view(B, p.nchunks, C, 2)
        outs += [dxb, dg, db]
    if short:
        assert all(rc == VR_ERR_WORKSPACE for rc in rcs), rcs
        assert untouched(*outs), f"{D.case}: a call refused for its workspace wrote"
        return None
    assert all(rc == 0 for rc in rcs), (rcs, L.vrnet_last_error())
    return got


def check_moments(hip, D):
    runs = [run_moments(hip, D, poison) for poison in (NAN, FINITE)]
    for form, got in runs[0].items():
        assert not bool(torch.isnan(got).any()), f"moments {D.case} {form}: NaN -- a slot of the workspace read before it was written"
        assert same_bits(got, runs[1][form]), f"moments {D.case} {form}: the two poisons give different bits"
        mom_check(D, "x x2" if form == "gtot partial" else form, got, f"moments {D.case} {form}")
    run_moments(hip, D, NAN, short=1)


@gpu
@pytest.mark.parametrize("case", MOM_CASES, ids=str)
def test_moments_exact(hip, case):
    check_moments(hip, mom_data(case))


@gpu
def test_moments_fp64_sums_of_real_data(hip):
    check_moments(hip, mom_data(MOM_REAL, "real"))


# ---- affine
def run_affine(hip, D, form):
    B, HW, C, ps, padc = D.case
    a, pre = aff_args(D, form)
    ref = affine_ref(a, pre, torch.float64)
    rows = lambda t, fill=NAN: Buf((B, HW, C), fill, t.cuda(), padc=padc)
    dev = {n: (rows(t) if t.dim() == 3 else vec(t)) for n, t in a.items()}
    v = lambda n: dev[n].v if n in dev else None
    ld = lambda n: dev[n].ld if n in dev else 0
    ob = Buf((B, HW, C), PAT, padc=padc)
    if pre == 3:
        hip.bn_apply_bwd_zmask(v("x1"), ld("x1"), v("x2"), ld("x2"), (v("mA"), v("mD"), v("mS")), v("A"), v("E"), v("D2"), v("S2"), ob.v, ob.ld,
                               B, HW, C)
    else:
        kw = dict(x1=v("x1"), ld1=ld("x1"), A=v("A"), D1=v("D1"), S1=v("S1"), pre=pre, masky=v("masky"), ldm=ld("masky"), x2=v("x2"), ld2=ld("x2"),
                  E=v("E"), D2=v("D2"), S2=v("S2"), bstride=C if ps else 0)
        hip.affine(ob.v, ob.ld, B, HW, C, add=v("add"), ldadd=ld("add"), **kw)
        if "add" in a:                      # in place: add == out
            ib = Buf((B, HW, C), PAT, D.old.cuda(), padc=padc)
            hip.affine(ib.v, ib.ld, B, HW, C, accumulate=1, **kw)
            assert torch.equal(ib.v, ob.v) and ib.intact(), f"affine {D.case} {form}: accumulate differs from the out-of-place add"
    same(ob.v, ref, f"affine {D.case} {D.plan.kernel} {form}")
    assert ob.intact(), f"affine {D.case} {form}: a guard element of the output changed"


@gpu
@pytest.mark.parametrize("case", AFF_CASES, ids=str)
def test_affine_exact(hip, case):
    D = aff_data(case)
    for form in AFF_FORMS:
        if form != "pre 3" or not case[3]:          # the recomputed mask comes with per-channel coefficients only
            run_affine(hip, D, form)


@gpu
@pytest.mark.parametrize("case", AFF_CAPS, ids=str)
def test_affine_grid_cap_exact(hip, case):
    B, HW, C, ps, padc = case
    D = cap_data(case)
    xb, ob = Buf((B, HW, C), NAN, D.x1.cuda(), padc=padc), Buf((B, HW, C), PAT, padc=padc)
    A, S1, D1 = vec(D.A), vec(D.S1), vec(D.D1)
    hip.affine(ob.v, ob.ld, B, HW, C, x1=xb.v, ld1=xb.ld, A=A.v, D1=D1.v, S1=S1.v)
    same(ob.v, D.ref, f"affine {case} {D.plan.kernel} at the 4096-block cap")
    assert ob.intact()


# ---- the coefficient kernels
def dev_f32(a):
    return None if a is None else vec(torch.from_numpy(np.ascontiguousarray(a, dtype=F32)))


def dev_f64(a):
    return dbuf(a.size, NAN, torch.from_numpy(np.ascontiguousarray(a, dtype=F64)).cuda())


def outs_for(I, names_sizes):
    """name -> out_vec, pre-filled with the old value where the case accumulates."""
    return {n: out_vec(size, torch.from_numpy(I.old[n]) if n in I.old else None) for n, size in names_sizes}


def finish(what, I, outs, names=None):
    torch.cuda.synchronize()
    assert all(o.intact() for o in outs.values()), f"{what}: a guard element changed"
    coef_close(what, {n: I.R[n] for n in (names or outs)}, {n: o.v.cpu() for n, o in outs.items()})
    print(f"NORM-EDGES coef {I.key}: draw {I.draw}")


@gpu
@pytest.mark.parametrize("key", [k for k in COEF_KEYS if k[0] in ("gn_coef_fwd", "gn_pairs", "gn_coef_bwd")], ids=str)
def test_groupnorm_coefficients(hip, key):
    I = coef_case(key)
    B, HW, C = I.B, I.HW, I.C
    mom, gam = dev_f64(I.mom), dev_f32(I.gamma)
    if key[0] == "gn_coef_bwd":
        ms = dev_f32(I.ms)
        outs = outs_for(I, [(n, B * C) for n in "AEDS"] + [("dgamma", C), ("dbeta", C)])
        hip.gn_coef_bwd(mom.d, ms.v, gam.v, B, HW, C, *[outs[n].v for n in ("A", "E", "D", "S", "dgamma", "dbeta")], key[4])
        finish(f"gn_coef_bwd {key}", I, outs)
        return
    bet = dev_f32(I.beta)
    outs = outs_for(I, [(n, B * C) for n in "ADS"] + [("mean_rstd", 2 * B)])
    args = (gam.v, bet.v, I.eps, B, HW, C, *[outs[n].v for n in ("A", "D", "S", "mean_rstd")])
    if key[0] == "gn_coef_fwd":
        hip.gn_coef_fwd(mom.d, *args)
        finish(f"gn_coef_fwd {key}", I, outs)
        return
    per = key[4]
    hip.gn_coef_from_pairs(mom.d, per, *args)
    finish(f"gn_coef_from_pairs {key}", I, outs)
    # gn_apply_fwd from the same pairs: mean_rstd under the coefficient rule, y under the apply rule
    xb, yb, ms = Buf((B, HW, C), NAN, I.x.cuda()), Buf((B, HW, C), PAT), out_vec(2 * B)
    hip.gn_apply_fwd(xb.v, xb.ld, mom.d, per, gam.v, bet.v, I.eps, B, HW, C, yb.v, yb.ld, ms.v)
    finish(f"gn_apply_fwd {key}", I, {"mean_rstd": ms})
    rld = f_gn_fwd(I, LD)
    t = lambda a, dt: torch.from_numpy(a.astype(F32 if dt == torch.float32 else F64)).to(dt)[:, None, :]
    ev = lambda dt: t(rld["A"], dt) * (I.x.to(dt) - t(rld["S"], dt)) + t(rld["D"], dt)
    R = bound_of(ev(torch.float32), ev(torch.float64))
    within(R, yb.v.cpu(), ev(torch.float64), f"gn_apply_fwd {key} y")
    assert yb.intact()


@gpu
@pytest.mark.parametrize("key", [k for k in COEF_KEYS if k[0].startswith("bn_")], ids=str)
def test_batchnorm_coefficients(hip, key):
    I = coef_case(key)
    C, chunks, bwd = I.C, "chunks" in key[0], key[0].endswith("bwd")
    mom, gam = dev_f64(I.mom), dev_f32(I.gamma)
    if bwd:
        ms = dev_f32(I.ms)
        outs = outs_for(I, [(n, C) for n in ("A", "E", "D", "S", "dgamma", "dbeta")])
        o = [outs[n].v for n in ("A", "E", "D", "S", "dgamma", "dbeta")]
        if chunks:
            hip.bn_coef_bwd_from_chunks(mom.d, I.lead, I.n, ms.v, gam.v, I.training, C, *o, key[5])
        else:
            hip.bn_coef_bwd(mom.d, ms.v, gam.v, I.training, I.lead, I.n // I.lead, C, *o, key[5])
        finish(f"{key}", I, outs)
        return
    bet = dev_f32(I.beta)
    run = out_vec(C, torch.from_numpy(I.rm)), out_vec(C, torch.from_numpy(I.rv))
    nbt = torch.full((3,), 7, dtype=torch.int64, device="cuda")
    outs = outs_for(I, [("A", C), ("D", C), ("S", C), ("mean_rstd", 2 * C)])
    o = [outs[n].v for n in ("A", "D", "S", "mean_rstd")]
    if chunks:
        hip.bn_coef_fwd_from_chunks(mom.d, I.lead, I.n, gam.v, bet.v, I.eps, I.momentum, run[0].v, run[1].v, nbt[1:2], C, *o)
    else:
        hip.bn_coef_fwd(mom.d, gam.v, bet.v, I.eps, I.momentum, run[0].v, run[1].v, nbt[1:2], I.training, I.lead, I.n // I.lead, C, *o)
    if I.training:
        outs |= {"running_mean": run[0], "running_var": run[1]}
        nbt_check(7, int(nbt[1].item()), f"{key}")
    else:
        assert torch.equal(run[0].v.cpu(), torch.from_numpy(I.rm)) and torch.equal(run[1].v.cpu(), torch.from_numpy(I.rv)) and int(nbt[1].item()) == 7
        assert run[0].intact() and run[1].intact()
    assert nbt[0].item() == 7 and nbt[2].item() == 7
    finish(f"{key}", I, outs)


@gpu
@pytest.mark.parametrize("key", [k for k in COEF_KEYS if k[0] in ("eca", "ls", "m2f")], ids=str)
def test_eca_layer_scale_and_pooling_coefficients(hip, key):
    I = coef_case(key)
    if key[0] == "eca":
        k, B, C, acc = key[1:5]
        mom, mom2, wk, gate = dev_f64(I.mom), dev_f64(I.mom2), dev_f32(I.wk), dev_f32(I.gate)
        go = out_vec(B * C)
        hip.eca_coef_fwd(mom.d, wk.v, k, B, I.HW, C, go.v)
        finish(f"eca_coef_fwd {key}", I, {"gate": go})
        for want in (("F", "dwk"), ("F",), ("dwk",)):
            outs = outs_for(I, [("F", B * C), ("dwk", k)])
            hip.eca_coef_bwd(mom2.d, mom.d, gate.v, wk.v, k, B, I.HW, C, outs["F"].v if "F" in want else None,
                             outs["dwk"].v if "dwk" in want else None, acc)
            skipped = [n for n in ("F", "dwk") if n not in want]
            expect = torch.from_numpy(I.old["dwk"]) if acc else None
            for n in skipped:               # the half that was not asked for stays as it was
                b = outs.pop(n)
                assert b.intact() and (untouched(b) if n == "F" or not acc else torch.equal(b.v.cpu(), expect)), f"eca {key}: {n} written"
            finish(f"eca_coef_bwd {key} {want}", I, outs)
    elif key[0] == "ls":
        B, C, has_ls, want_dls, want_dbias, acc = key[1:7]
        mom, ls = dev_f64(I.mom), dev_f32(I.ls)
        outs = outs_for(I, [("dls", C), ("dbias", C)])
        hip.ls_coef_bwd(mom.d, ls.v if has_ls else None, B, C, outs["dls"].v if want_dls else None, outs["dbias"].v if want_dbias else None, acc)
        for n, want in (("dls", want_dls), ("dbias", want_dbias)):
            if not want:
                b = outs.pop(n)
                assert b.intact() and (torch.equal(b.v.cpu(), torch.from_numpy(I.old[n])) if acc else untouched(b)), f"ls {key}: {n} written"
        finish(f"ls_coef_bwd {key}", I, outs)
    else:
        n, which = key[1:3]
        mom, ob = dev_f64(I.mom), out_vec(n)
        hip.moments_to_float(mom.d, ob.v, n, I.scale, which)
        finish(f"moments_to_float {key}", I, {"out": ob})


# ---- the chains
def report(tag, D):
    Rs = list(D.R.values())
    print(f"NORM-EDGES {tag} {D.case}: draw {D.draw} cond {D.cond:.1f} d32 {min(R.d32 for R in Rs):.2e} .. {max(R.d32 for R in Rs):.2e} bound "
          f"{min(R.bound for R in Rs):.2e} .. {max(R.bound for R in Rs):.2e} kernel {max(R.seen for R in Rs):.2e} "
          f"share {max(R.seen / R.bound for R in Rs):.3f}")


@gpu
@pytest.mark.parametrize("case", GN_CASES + GN_PARTIALS[:2], ids=str)
def test_groupnorm_chains_against_fp64(hip, case):
    B, HW, C = case
    D = gn_data(case)
    xb, gb, ab = (Buf((B, HW, C), NAN, rows_of(t)) for t in (D.x, D.g, D.add))
    gam, bet = vec(D.gam), vec(D.bet)
    coefs = lambda: ([out_vec(B * C) for _ in range(3)], out_vec(2 * B))
    # moments -> gn_coef_fwd -> affine
    mom = hip.moments(xb.v, xb.ld, B, HW, C)
    (A, Dc, S), ms1 = coefs()
    hip.gn_coef_fwd(mom, gam.v, bet.v, 1e-5, B, HW, C, A.v, Dc.v, S.v, ms1.v)
    yb = Buf((B, HW, C), PAT)
    hip.affine(yb.v, yb.ld, B, HW, C, x1=xb.v, ld1=xb.ld, A=A.v, D1=Dc.v, S1=S.v, bstride=C)
    within(D.R["y"], maps_of(yb.v), D.y, f"gn {case} moments -> gn_coef_fwd -> affine")
    assert yb.intact() and all(t.intact() for t in (A, Dc, S, ms1))
    # gn_stats_fwd -> affine
    (A, Dc, S), ms2 = coefs()
    hip.gn_stats_fwd(xb.v, xb.ld, gam.v, bet.v, 1e-5, B, HW, C, A.v, Dc.v, S.v, ms2.v)
    yb = Buf((B, HW, C), PAT)
    hip.affine(yb.v, yb.ld, B, HW, C, x1=xb.v, ld1=xb.ld, A=A.v, D1=Dc.v, S1=S.v, bstride=C)
    within(D.R["y"], maps_of(yb.v), D.y, f"gn {case} gn_stats_fwd -> affine")
    assert yb.intact() and all(t.intact() for t in (A, Dc, S, ms2))
    # tile pairs -> gn_apply_fwd -> gn_apply_bwd
    per = min(HW, 3)
    pairs = dbuf(B * per * 2, NAN, gn_pairs(D, per).cuda())
    yb, ms3 = Buf((B, HW, C), PAT), out_vec(2 * B)
    hip.gn_apply_fwd(xb.v, xb.ld, pairs.d, per, gam.v, bet.v, 1e-5, B, HW, C, yb.v, yb.ld, ms3.v)
    within(D.R["y"], maps_of(yb.v), D.y, f"gn {case} gn_apply_fwd")
    assert yb.intact() and ms3.intact()
    stats = torch.stack([D.mean.flatten(), D.rstd.flatten()], 1)
    Rs = NS(d32=0.0, bound=4 * ULP_FLOOR, seen=0.0)
    for ms, name in ((ms1, "gn_coef_fwd"), (ms2, "gn_stats_fwd"), (ms3, "gn_apply_fwd")):
        within(Rs, ms.v.view(B, 2).cpu()[:, 0], stats[:, 0], f"gn {case} mean of {name}")
        within(Rs, ms.v.view(B, 2).cpu()[:, 1], stats[:, 1], f"gn {case} rstd of {name}")

    def backward(call, what):
        dxb, dg, db = Buf((B, HW, C), PAT), out_vec(C, D.old_g), out_vec(C, D.old_b)
        call(dxb, dg, db)
        within(D.R["dx"], maps_of(dxb.v), D.add.double() + D.dx, f"gn {case} {what} dx + add")
        within(D.R["dgam"], dg.v.cpu(), D.old_g.double() + D.dgam, f"gn {case} {what} dgamma (accumulated)")
        within(D.R["dbet"], db.v.cpu(), D.old_b.double() + D.dbet, f"gn {case} {what} dbeta (accumulated)")
        assert dxb.intact() and dg.intact() and db.intact(), f"gn {case} {what}: a guard element changed"
    backward(lambda dxb, dg, db: hip.gn_apply_bwd(gb.v, gb.ld, xb.v, xb.ld, ms3.v, gam.v, B, HW, C, dxb.v, dxb.ld, dg.v, db.v, 1, add=ab.v,
                                                  ldadd=ab.ld), "gn_apply_bwd")
    if case in GN_PARTIALS:
        part, tot = gn_tile_partials(D)
        pb, tb = dbuf(part.numel(), NAN, part.cuda()), dbuf(tot.numel(), NAN, tot.cuda())
        backward(lambda dxb, dg, db: hip.gn_apply_bwd_from_partials(gb.v, gb.ld, xb.v, xb.ld, pb.d, tb.d, ms3.v, gam.v, B, HW, C, dxb.v, dxb.ld,
                                                                    dg.v, db.v, 1, add=ab.v, ldadd=ab.ld), "gn_apply_bwd_from_partials")
    report("gn", D)


@gpu
@pytest.mark.parametrize("case", BN_CASES, ids=str)
def test_batchnorm_relu_chain_against_fp64(hip, case):
    B, HW, C = case
    D = bn_data(case)
    padc = 0 if C % 4 and (HW * C) % 4 == 0 else 4          # (2, 8, 7): contiguous, the flat kernel
    zb, gb = (Buf((B, HW, C), NAN, rows_of(t), padc=padc) for t in (D.z, D.g))
    gam, bet = vec(D.gam), vec(D.bet)
    rm, rv = out_vec(C, D.rm0), out_vec(C, D.rv0)
    nbt = torch.zeros((), dtype=torch.int64, device="cuda")
    A, Dc, S, ms = out_vec(C), out_vec(C), out_vec(C), out_vec(2 * C)
    hip.bn_stats_fwd(zb.v, zb.ld, gam.v, bet.v, 1e-3, 0.03, rm.v, rv.v, nbt, B, HW, C, A.v, Dc.v, S.v, ms.v)
    yb = Buf((B, HW, C), PAT, padc=padc)
    hip.affine(yb.v, yb.ld, B, HW, C, x1=zb.v, ld1=zb.ld, A=A.v, D1=Dc.v, S1=S.v, pre=1)
    within(D.R["y"], maps_of(yb.v), D.r.y, f"bn {case} bn_stats_fwd -> affine(pre 1)")
    within(D.R["rm"], rm.v.cpu(), D.r.rm, f"bn {case} running_mean")
    within(D.R["rv"], rv.v.cpu(), D.r.rv, f"bn {case} running_var")
    nbt_check(0, int(nbt.item()), f"bn {case}")
    assert all(t.intact() for t in (yb, rm, rv, A, Dc, S, ms))
    co = {}
    for route in ("mask", "zmask"):
        c4, dg, db = [out_vec(C) for _ in range(4)], out_vec(C, D.old_g), out_vec(C, D.old_b)
        o = [t.v for t in c4] + [dg.v, db.v, 1]
        if route == "mask":
            hip.bn_stats_bwd(gb.v, gb.ld, zb.v, zb.ld, yb.v, yb.ld, ms.v, gam.v, True, B, HW, C, *o)
        else:
            hip.bn_stats_bwd_zmask(gb.v, gb.ld, zb.v, zb.ld, (A.v, Dc.v, S.v), ms.v, gam.v, True, B, HW, C, *o)
        within(D.R["dgam"], dg.v.cpu(), D.old_g.double() + D.r.dgam, f"bn {case} {route} dgamma (accumulated)")
        within(D.R["dbet"], db.v.cpu(), D.old_b.double() + D.r.dbet, f"bn {case} {route} dbeta (accumulated)")
        assert all(t.intact() for t in c4 + [dg, db])
        co[route] = c4 + [dg, db]
    for a_, b_ in zip(co["mask"], co["zmask"]):
        assert torch.equal(a_.v, b_.v), f"bn {case}: bn_stats_bwd_zmask against bn_stats_bwd"
    c4 = [t.v for t in co["zmask"][:4]]
    dz3, dz2 = Buf((B, HW, C), PAT, padc=padc), Buf((B, HW, C), PAT, padc=padc)
    hip.bn_apply_bwd_zmask(gb.v, gb.ld, zb.v, zb.ld, (A.v, Dc.v, S.v), *c4, dz3.v, dz3.ld, B, HW, C)
    hip.affine(dz2.v, dz2.ld, B, HW, C, x1=gb.v, ld1=gb.ld, A=c4[0], pre=2, masky=yb.v, ldm=yb.ld, x2=zb.v, ld2=zb.ld, E=c4[1], D2=c4[2], S2=c4[3])
    within(D.R["dz"], maps_of(dz3.v), D.r.dz, f"bn {case} bn_apply_bwd_zmask")
    assert torch.equal(dz3.v, dz2.v) and dz3.intact() and dz2.intact(), f"bn {case}: the recomputed mask against the stored one"
    report("bn", D)


# ---- refusals, each with its outputs untouched
@gpu
def test_refusals_leave_the_outputs_untouched(hip):
    def refused(what, call, *bufs):
        with pytest.raises(RuntimeError):
            call()
        assert untouched(*bufs), f"{what}: a refused call wrote"
    C = 8
    x = Buf((1, 1, C), NAN, torch.ones(1, 1, C).cuda())
    gam, bet = vec(torch.ones(C)), vec(torch.zeros(C))
    o = [out_vec(C) for _ in range(5)] + [out_vec(2 * C)]          # rm, rv, A, D, S, mean_rstd
    ov = [t.v for t in o]
    nbt = torch.zeros((), dtype=torch.int64, device="cuda")
    mom = torch.ones(1, C, 2, dtype=torch.float64, device="cuda")
    refused("bn_stats_fwd at B HW = 1", lambda: hip.bn_stats_fwd(x.v, x.ld, gam.v, bet.v, 1e-3, 0.03, ov[0], ov[1], nbt, 1, 1, C, *ov[2:]), *o)
    refused("bn_coef_fwd at B HW = 1", lambda: hip.bn_coef_fwd(mom, gam.v, bet.v, 1e-3, 0.03, ov[0], ov[1], nbt, True, 1, 1, C, *ov[2:]), *o)
    refused("bn_coef_fwd_from_chunks at count = 1",
            lambda: hip.bn_coef_fwd_from_chunks(mom, 1, 1, gam.v, bet.v, 1e-3, 0.03, ov[0], ov[1], nbt, C, *ov[2:]), *o)
    part = torch.ones(4, C, 2, dtype=torch.float64, device="cuda")
    refused("bn_coef_fwd_from_partials at HW % 32",
            lambda: hip.bn_coef_fwd_from_partials(part, gam.v, bet.v, 1e-3, 0.03, ov[0], ov[1], nbt, 2, 33, C, *ov[2:]), *o)
    refused("bn_coef_fwd_from_partials at B HW = 1",
            lambda: hip.bn_coef_fwd_from_partials(part, gam.v, bet.v, 1e-3, 0.03, ov[0], ov[1], nbt, 1, 1, C, *ov[2:]), *o)
    assert int(nbt.item()) == 0
    B, HW = 2, 33
    xb, yb = Buf((B, HW, C), NAN, torch.ones(B, HW, C).cuda()), Buf((B, HW, C), PAT)
    dg, db, ms = out_vec(C), out_vec(C), vec(torch.ones(2 * B))
    refused("gn_apply_bwd_from_partials at HW % 32",
            lambda: hip.gn_apply_bwd_from_partials(xb.v, xb.ld, xb.v, xb.ld, part, part, ms.v, gam.v, B, HW, C, yb.v, yb.ld, dg.v, db.v, 0), yb, dg, db)
    wk, gate = vec(torch.ones(4)), out_vec(C)
    refused("eca_coef_fwd with even k", lambda: hip.eca_coef_fwd(mom, wk.v, 4, 1, 9, C, gate.v), gate)
    C6 = 6
    x6, y6 = Buf((B, HW, C6), NAN, torch.ones(B, HW, C6).cuda(), padc=2), Buf((B, HW, C6), PAT, padc=2)
    ms6 = out_vec(2 * B)
    refused("gn_apply_fwd at C % 4", lambda: hip.gn_apply_fwd(x6.v, x6.ld, part, 1, gam.v, bet.v, 1e-5, B, HW, C6, y6.v, y6.ld, ms6.v), y6, ms6)
    refused("gn_apply_bwd at C % 4", lambda: hip.gn_apply_bwd(x6.v, x6.ld, x6.v, x6.ld, ms.v, gam.v, B, HW, C6, y6.v, y6.ld, dg.v, db.v, 0), y6, dg, db)
    for pre in (-1, 3):
        refused(f"affine with pre {pre}", lambda: hip.affine(yb.v, yb.ld, B, HW, C, x1=xb.v, ld1=xb.ld, pre=pre, masky=xb.v, ldm=xb.ld), yb)
    refused("affine with accumulate and add", lambda: hip.affine(yb.v, yb.ld, B, HW, C, x1=xb.v, ld1=xb.ld, accumulate=1, add=xb.v, ldadd=xb.ld), yb)
