"""The kernels of csrc/spatial.hip at the edges of their launch plans: the depthwise 3 x 3 convolution (forward / data gradient
and weight gradient), the bilinear resize with its adjoints, the unfused min / max and image gain, and ShuffleAttention -- every
branch of the launchers, in the manner of tests/test_wgrad_plan.py and tests/test_direct_conv.py, whose helpers this file imports.

Which branch a case reaches is not taken on trust: the spatial launchers note no kernel family, so the tests without a gpu mark
restate dw_wgrad_plan, dw_wgrad_slide_ok, the forward depthwise choice with its ppb loop, up_grid / segs, up_bwd_window (in
float32, as the kernels evaluate it), sa_plan and the grid_for caps of the min / max family in Python, assert each case's claimed
branch from the restatement, require that the restated plans reproduce the library's host-only workspace queries, and that the
union over the case tables is the complete list ALL_BRANCHES.

Operands, as in tests/test_direct_conv.py:

  exact    wherever a kernel only multiplies and adds (all depthwise kernels, the resize at scale 1, min / max): small integers
           (x, w, old values in {-3..3}; x, dy in {-2..2} for the weight gradient), every partial sum an integer below 2^24 in
           any order (test_exact_cases_stay_below_2_24, from the same operation on |x| and |dy|): the result must equal the fp64
           reference bit for bit.
  rounded  everywhere else: bound = 4 * max(d32, ULP_FLOOR) in the metric of dist(), d32 = the fp32 CPU result (ATen, the oracle,
           or the formula of ref_gain in fp32) against the fp64 one on the same operands, per output.  The ShuffleAttention
           operands are redrawn while a parameter gradient of the fp64 reference cancels worse than COND_LIMIT (the 1089-row case
           takes the second draw), the resize operands while the adjoint's largest element does (never).  The gain's dt and x are positive, so that the sums behind the gradient of min p and max p do not cancel, and
           dp is held on the tied elements (which carry those sums, n times larger) and on the others separately.

Outputs sit in the PAT bit pattern inside buffers with guard elements in front and behind and four guard columns behind every
NHWC row, all of which must keep it; inputs are surrounded by NaN in the same way (min / max: by +-3e38, fminf skips a NaN).  The
two entry points with a caller-supplied workspace (vrnet_dwconv3x3_wgrad_f32, vrnet_sa_bwd_f32) get exactly the queried bytes,
poisoned, in front of a 4 KB guard; they run twice, on a NaN and on a finite poison, for equal bits; one byte less is refused with
the outputs untouched.

The sensitivity tests (no GPU) plant in the reference the errors a kernel could make -- a halo column zeroed between two runs, the
last row chunk skipped, a window term of the adjoint dropped, the last workgroup's partial of a reduction ignored, channel block
1 aliased onto block 0 -- and require that the comparison the GPU tests use rejects each.

Measured on an MI355X (the tests print every figure; d32, the bound and the kernel's distance are per output):

  depthwise, 3 rounded cases x 4 forms   d32 4.1e-8 .. 1.2e-7, every bound the floor 3.8e-6, kernels 4.1e-8 .. 8.3e-8 (0.022 of it)
  resize, the 25 cases above scale 1     d32 0 .. 2.3e-6, bounds 3.8e-6 .. 9.0e-6; forward and adjoint 4.4e-8 .. 2.3e-6, at most 0.25
                                         of their bounds.  The conservation of mass is the tight one: 3.4e-6 and 3.7e-6 at
                                         (2, 1, 32), where an element of dx is an fp32 sum of 2 048 positive terms -- 0.90 and 0.98
                                         of the bound 3.8e-6 (elsewhere at most 0.49)
  gain, n = 5, 2049, 524 295             d32 1.2e-9 .. 3.2e-7, every bound the floor, kernels at most 2.1e-7 (0.055)
  ShuffleAttention, 6 cases x 2 forms    d32 0 .. 1.7e-6 and bounds 3.8e-6 .. 6.7e-6 but for dx at HW = 1 (d32 1.4e-5 / 7.0e-6
                                         accumulating: autograd adds the gate term to two cancelling terms 316 times its size);
                                         kernels 8.2e-8 .. 6.8e-7, at most 0.16 of their bounds

The HW = 1 case found an error: before this file sa_bwd_apply_kernel left 1.13e-4 (5.9e-5 accumulating) in dx there, twice the bound
and above the suite's TOL -- it rounded P dz and F = -P mean(dz), each 1 / sqrt(eps) = 316 times the size of their sum, to fp32 one by
one.  The kernel now subtracts the mean of dz from dz before it scales by P (csrc/spatial.hip: sa_dz, sa_bwd_apply_kernel): 4.9e-8."""
import functools
import math
import types

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests.test_direct_conv import COND_LIMIT, EXACT_LIMIT, MAX_DRAWS, ULP_FLOOR, dist
from tests.test_fusion_kernels import ref_gain, ref_gain_bwd
from tests.test_hip_ops import TOL, nchw, nhwc, rnd
from tests.test_strided_rows import NAN, PAT

gpu = pytest.mark.gpu
NS = types.SimpleNamespace
VR_ERR_WORKSPACE = 3          # csrc/common.h


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
def cdiv(a, b):
    return -(-a // b)


def grid_for(n, per_block=1024, cap=8192):
    return min(max(cdiv(n, per_block), 1), cap)


def dw_fwd_plan(shape):
    """vrnet_dwconv3x3_f32 on 16-byte aligned rows with ld % 4 == 0."""
    B, H, W, C = shape
    vec = C % 4 == 0 and C <= 1024 and 256 % (C // 4) == 0
    if vec and W % 8 == 0:
        items = B * H * (W // 8) * (C // 4)
        return NS(kernel="slide", blocks=cdiv(items, 256), items=items, runs=W // 8, CQ=C // 4)
    if vec:
        npix, pp = B * H * W, 256 // (C // 4)
        ppb, doublings = pp * 8, 0
        while cdiv(npix, ppb) > 4096:
            ppb, doublings = ppb * 2, doublings + 1
        return NS(kernel="vec", blocks=cdiv(npix, ppb), ppb=ppb, doublings=doublings, PP=pp, CQ=C // 4, npix=npix)
    total = B * H * W * C
    blocks = grid_for(total)
    return NS(kernel="scalar", blocks=blocks, capped=cdiv(total, 1024) > 8192, trips=cdiv(total, blocks * 256), total=total)


def dw_wgrad_plan(nrows, W, C):
    """-> (chunks, rows per chunk)"""
    nc = min(max(cdiv(nrows * W * C, 16384), 1), 512, nrows)
    rpc = cdiv(nrows, nc)
    return cdiv(nrows, rpc), rpc


def dw_wgrad_refusal(W, C):
    """dw_wgrad_slide_ok on aligned rows: None if the sliding-window kernel takes the map, else the reason it does not."""
    if W % 16 or C % 4:
        return "W % 16 or C % 4"
    if W > 512:
        return "W > 512"
    q, nseg = C // 4, W // 16
    if q > 64:
        return None if q % 64 == 0 and (4 % nseg == 0 if nseg <= 4 else nseg % 4 == 0) else "wide C"
    if 256 % q:
        return "256 % (C/4)"
    groups = 256 // q
    if nseg <= groups:
        return None if groups % nseg == 0 else "groups % nseg"
    return None if nseg % groups == 0 else "nseg % groups"


def dw_wgrad_launch(shape):
    B, H, W, C = shape
    chunks, rpc = dw_wgrad_plan(B * H, W, C)
    p = NS(chunks=chunks, rpc=rpc, last=B * H - (chunks - 1) * rpc, capped=cdiv(B * H * W * C, 16384) > 512 and B * H > 512,
           refusal=dw_wgrad_refusal(W, C), workspace=chunks * C * 9 * 4 + 256)
    if p.refusal is None:
        p.kernel, p.quads = "slide", min(C // 4, 64)
        p.groups, p.nseg = 256 // p.quads, W // 16
        p.nsegp = min(p.nseg, p.groups)
        p.rpar, p.grid_y, p.lds = p.groups // p.nsegp, (C // 4) // p.quads, (p.groups - 1) * p.quads * 9 * 16
    else:
        p.kernel, p.TPR = "scalar", 32 if C <= 32 else 64
        p.grid_y, p.RP = cdiv(C, p.TPR), 256 // p.TPR
    return p


def up_grid(lines, per):
    segs = cdiv(per, 256)
    assert per < 2 ** 31 and lines * segs < 2 ** 31
    return segs, lines * segs


def up_fwd_plan(B, H, W, C, scale, out_nchw):
    OH, OW = H * scale, W * scale
    if not out_nchw and C % 4 == 0:
        return NS(kernel="vec", segs=up_grid(B * OH, OW * (C // 4))[0])
    if out_nchw and OW % 4 == 0:
        return NS(kernel=f"nchw4 near {1 if scale >= 2 else 0}", segs=up_grid(B * C, OH * (OW // 4))[0])
    return NS(kernel="scalar", segs=None, layout="nchw" if out_nchw else "nhwc")


def up_bwd_plan(B, H, W, C, scale, dy_nchw, cs=1, coff=0):
    if not dy_nchw and C % 4 == 0 and (cs == 2 or coff % 4 == 0):
        return NS(kernel="vec", segs=up_grid(B * H, W * (C // 4))[0])
    return NS(kernel="scalar", segs=up_grid(B * C, H * W)[0] if dy_nchw else up_grid(B * H, W * C)[0],
              layout="nchw" if dy_nchw else "nhwc")


UP_MAXR = 16


def up_windows(n_in, scale):
    """up_bwd_window in float32 for every input index of an axis: the widths hi - lo + 1."""
    n_out = n_in * scale
    r = np.float32(n_in - 1) / np.float32(n_out - 1) if n_out > 1 else np.float32(0)
    i = np.arange(n_in)
    if not r > 0:
        return np.full(n_in, n_out)
    lo = np.maximum(0, np.floor((i - 1).astype(np.float32) / r).astype(np.int64) - 1)
    hi = np.minimum(n_out - 1, np.ceil((i + 1).astype(np.float32) / r).astype(np.int64) + 1)
    return hi - lo + 1


def sa_plan(HW, C):
    t = 1
    while t < C and t < 256:
        t <<= 1
    nc = min(max(cdiv(HW * C, 8192), 1), 1024, HW)
    rows = cdiv(HW, nc)
    return NS(TPR=t, ncb=cdiv(C, t), chunks=cdiv(HW, rows), rows=rows)


def sa_workspace(B, HW, C):
    return (B * sa_plan(HW, C).chunks * C * 2 + B * C * 2) * 8 + 256


MINMAX_GRID, FWD_GRID, BWD_GRID = (2048, 2048), (2048, 512), (2048, 256)          # (elements per block, cap) of grid_for


def reduce_class(n, grid):
    nb = grid_for(n, *grid)
    return "one block" if nb == 1 else "capped" if cdiv(n, grid[0]) > grid[1] else "several blocks"


def owner(e, n, grid):
    """The workgroup whose grid-stride loop reads element e."""
    return (e // 256) % grid_for(n, *grid)


# ================================================================================================ the cases
DW_FWD = [                                 # kernel, (B, H, W, C)
    ("slide", (2, 3, 16, 8)),              # two runs per row: both halo columns are real data; the image boundary between rows
    ("slide", (1, 2, 24, 4)),              # three runs, CQ = 1
    ("slide", (2, 5, 32, 64)),             # 640 items: 3 workgroups, ragged last
    ("slide", (1, 1, 8, 1024)),            # H = 1: both outer rows null; CQ = 256
    ("vec", (2, 3, 9, 8)),                 # W % 8 != 0
    ("vec", (1, 1, 1, 4)),                 # a single pixel
    ("vec", (2, 7, 5, 1024)),              # PP = 1, 9 workgroups
    ("vec", (1, 33, 31, 16)),              # 2 workgroups, ragged
    ("scalar", (2, 3, 5, 6)),              # C % 4 != 0
    ("scalar", (1, 4, 8, 12)),             # C % 4 == 0, 256 % 3 != 0; one workgroup, two trips of the grid-stride loop
    ("scalar", (1, 2, 2, 1028)),           # C > 1024
    ("scalar", (1, 65, 64, 2050)),         # 8 528 000 elements: the 8 192-workgroup cap, grid-stride
]
DW_FWD_BIG = ("vec", (1, 129, 255, 1024))  # 32 895 px: the ppb *= 2 loop runs once (2 056 workgroups); 135 MB per tensor
DW_FWD_ROUNDED = [DW_FWD[0], DW_FWD[4], DW_FWD[8]]
DW_FORMS = [(0, 0), (1, 0), (0, 1), (1, 1)]          # (flip, accumulate)
DW_FORMS_BIG = [(0, 0), (1, 1)]

DW_WGRAD = [
    ("scalar", (1, 1, 1, 1)),              # one element; TPR = 32
    ("scalar", (2, 3, 3, 33)),             # TPR = 64 with 31 dead channel lanes
    ("scalar", (1, 5, 7, 32)),             # TPR = 32, W < RP = 8
    ("scalar", (4, 41, 24, 70)),           # plan (17, 10): ragged last chunk of 4 rows, 2 channel blocks, the reduction's second k step
    ("scalar", (1, 4, 48, 64)),            # nseg = 3 does not divide groups = 16
    ("scalar", (1, 2, 528, 4)),            # W > 512
    ("scalar", (1, 6, 80, 256)),           # nseg = 5, groups = 4
    ("scalar", (1, 4, 16, 12)),            # 256 % 3 != 0
    ("slide", (2, 5, 16, 4)),              # quads = 1, groups = 256, rpar = 256 > 10 rows, 36 720 B of LDS
    ("slide", (3, 7, 16, 64)),             # plan (2, 11): H odd, ragged chunk, chunk boundary inside an image
    ("slide", (1, 3, 32, 8)),              # quads = 2, two segments side by side
    ("slide", (1, 4, 512, 4)),             # the widest row taken, nseg = 32
    ("slide", (2, 1, 16, 8)),              # H = 1: the ok[ky] rows
    ("slide", (1, 2, 16, 8)),              # H = 2
    ("slide", (2, 300, 16, 1024)),         # 9.8 M elements: the 512-chunk cap (plan (300, 2)), C/4 = 256: gridDim.y = 4
]

# (B, H, W, C, scale, nchw)
UP_GEOS = [(1, 1, 4), (1, 5, 2), (5, 1, 4), (6, 5, 1), (4, 5, 3), (3, 3, 8), (2, 1, 32)]          # (H, W, scale), run at C = 8, 9, NCHW
UP_CASES = [(2, H, W, C, s, n) for H, W, s in UP_GEOS for C, n in ((8, 0), (9, 0), (9, 1))] + [
    (2, 3, 4, 3, 1, 1),                    # identity into NCHW rows of whole quads: nchw4 with near = 0
    (1, 33, 32, 3, 1, 1),                  # ... 264 quads per plane: segs = 2
    (2, 9, 8, 3, 4, 1),                    # 288 positions per plane: segs = 2 in upsample_nchw4_kernel, ragged, near = 1
    (2, 17, 16, 3, 2, 1),                  # segs = 2 in the NCHW adjoint
    (2, 2, 5, 256, 2, 0),                  # segs = 2 in upsample_bwd_vec_kernel (3 in the forward)
    (2, 2, 3, 512, 2, 0),                  # segs = 3 in upsample_vec_kernel (2 in the adjoint)
    (2, 2, 30, 9, 2, 0),                   # segs = 2 in the scalar NHWC adjoint
    (1, 31, 33, 4, 4, 0),                  # a map large enough for index rounding to matter
    (1, 31, 33, 3, 4, 1),
]
CAT_FORMS = [(2, 0), (2, 1), (1, 4), (1, 2)]          # (cs, coff)

MINMAX_N = [1, 255, 2049, 4095, 2048 * 2048 + 3]      # 4095: both extremes in the LAST workgroup's elements
GAIN_N = [5, 2049, 524288 + 7]
SA_CASES = [                               # (B, HW, C, G)
    (2, 63, 512, 8),                       # ncb = 2
    (2, 63, 480, 8),                       # ncb = 2, ragged channel block
    (2, 1089, 128, 8),                     # 18 chunks of 61 rows, ragged: the second step of sa_reduce_chunks_kernel
    (33, 4, 16, 8),                        # B * G = 264 > 256, cp = 1
    (2, 1, 16, 4),                         # HW = 1: variance exactly 0
    (1, 9, 2, 1),                          # the smallest legal map
]


def up_branches(case):
    B, H, W, C, scale, n = case
    out = set()
    f = up_fwd_plan(B, H, W, C, scale, n)
    out.add(("up", "scalar", f.layout) if f.kernel == "scalar" else ("up", f.kernel, "segs 1" if f.segs == 1 else "segs >1"))
    forms = [(1, 0)] if n else [(1, 0)] + CAT_FORMS
    wide = bool((up_windows(W, scale) > UP_MAXR).any())
    narrow = bool((up_windows(W, scale) <= UP_MAXR).any())
    for cs, coff in forms:
        b = up_bwd_plan(B, H, W, C, scale, n, cs, coff)
        out.add(("up bwd", b.kernel, f"cs {cs}"))
        if wide:
            out.add(("up bwd", b.kernel, "generic window"))
        if narrow:
            out.add(("up bwd", b.kernel, "register window"))
        if H == 1 or W == 1:
            out.add(("up bwd", b.kernel, "r == 0"))
        if b.segs > 1:
            out.add(("up bwd", b.kernel if b.kernel == "vec" else "scalar " + b.layout, "segs >1"))
    return out


def chunk_class(n):
    return "chunks 1" if n == 1 else "chunks >16" if n > 16 else "chunks >1"


def branches():
    out = set()
    for _, shape in DW_FWD + [DW_FWD_BIG]:
        p = dw_fwd_plan(shape)
        out.add(("dw", p.kernel))
        if p.kernel == "vec" and p.doublings:
            out.add(("dw", "vec ppb doubled"))
        if p.kernel == "scalar" and p.capped:
            out.add(("dw", "scalar grid cap"))
    for _, shape in DW_WGRAD:
        p = dw_wgrad_launch(shape)
        out.add(("dw wgrad", p.kernel, chunk_class(p.chunks)))
        if p.capped:
            out.add(("dw wgrad", "512-chunk cap"))
        if p.grid_y > 1:
            out.add(("dw wgrad", p.kernel, "gridDim.y > 1"))
        if p.refusal:
            out.add(("dw wgrad refused", p.refusal))
    for case in UP_CASES:
        out |= up_branches(case)
    out |= {("minmax", reduce_class(n, MINMAX_GRID)) for n in MINMAX_N}
    out |= {("gain bwd", reduce_class(n, BWD_GRID)) for n in GAIN_N}
    for B, HW, C, G in SA_CASES:
        p = sa_plan(HW, C)
        out |= {("sa", f"ncb {p.ncb}"), ("sa", chunk_class(p.chunks)), ("sa", "B * G > 256" if B * G > 256 else "B * G <= 256")}
    return out


ALL_BRANCHES = (
    {("dw", k) for k in ("slide", "vec", "scalar", "vec ppb doubled", "scalar grid cap")} |
    {("dw wgrad", k, c) for k in ("scalar", "slide") for c in ("chunks 1", "chunks >1", "chunks >16", "gridDim.y > 1")} |
    {("dw wgrad", "512-chunk cap")} |
    {("dw wgrad refused", r) for r in ("W % 16 or C % 4", "W > 512", "groups % nseg", "nseg % groups", "256 % (C/4)")} |
    {("up", k, s) for k in ("vec", "nchw4 near 0", "nchw4 near 1") for s in ("segs 1", "segs >1")} |
    {("up", "scalar", "nhwc"), ("up", "scalar", "nchw")} |
    {("up bwd", k, w) for k in ("vec", "scalar") for w in ("register window", "generic window", "r == 0", "cs 1", "cs 2")} |
    {("up bwd", k, "segs >1") for k in ("vec", "scalar nhwc", "scalar nchw")} |
    {(f, c) for f in ("minmax", "gain bwd") for c in ("one block", "several blocks", "capped")} |
    {("sa", c) for c in ("ncb 1", "ncb 2", "chunks 1", "chunks >1", "chunks >16", "B * G <= 256", "B * G > 256")})


# ================================================================================================ operands and references
def ints(rng, m, *shape):
    return torch.from_numpy(rng.integers(-m, m + 1, shape).astype(np.float32))


def bound_of(r32, r64):
    d32 = dist(r32, r64)
    return NS(d32=d32, bound=4 * max(d32, ULP_FLOOR), seen=0.0)


def cond_of(out, mag):
    """sum |terms| / |sum| of the output's largest element (tests/test_direct_conv.py: conditioning)."""
    top = out.abs().max().item()
    return 0.0 if top == 0.0 else (mag.flatten()[out.abs().argmax()] / top).item()


def same(got, ref, what):
    """Bit for bit (an exact case): no tolerance; a NaN or an unwritten PAT element differs too."""
    got = got.detach().cpu()
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    bad = ~(got == ref.to(got.dtype))
    assert not bool(bad.any()), f"{what}: {int(bad.sum())} of {ref.numel()} values differ from the exact result, first at " \
                                f"{tuple(bad.nonzero()[0].tolist())}: {got[bad][0].item()} for {ref[bad][0].item()}"


def within(R, got, ref, what):
    """No NaN, and within the bound of R (from the reference's own fp32 error) in the metric of dist()."""
    assert not bool(torch.isnan(got).any()), f"{what}: NaN in the result"
    e = dist(got, ref)
    R.seen = max(R.seen, e)
    print(f"  {what}: d32 {R.d32:.2e} bound {R.bound:.2e} kernel {e:.2e}")
    assert e <= R.bound, f"{what}: distance {e:.3e}, bound {R.bound:.3e} (d32 {R.d32:.3e})"


def check(D, R, got, ref, what):
    same(got, ref, what) if D.kind == "exact" else within(R, got, ref, what)


def same_bits(a, b):
    return torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


# ---- depthwise
def dw_ref(x, w, flip, dtype=torch.float64):
    w = w.flip(2, 3) if flip else w
    return F.conv2d(x.to(dtype), w.to(dtype), None, 1, 1, 1, x.shape[1])


@functools.lru_cache(maxsize=None)
def dw_data(shape, kind):
    """x, w, old (NCHW / (C, 1, 3, 3)); ref[flip]: fp64 (stored as fp32 where exact); R[flip]: the bound of a rounded case."""
    B, H, W, C = shape
    D = NS(kind=kind, shape=shape, R={0: None, 1: None}, draw=0)
    if kind == "exact":
        rng = np.random.default_rng([1] + list(shape))
        D.x, D.w, D.old = ints(rng, 3, B, C, H, W), ints(rng, 3, C, 1, 3, 3), ints(rng, 3, B, C, H, W)
        D.ref = {f: dw_ref(D.x, D.w, f).float() for f in (0, 1)}
        return D
    D.x, D.w, D.old = rnd(B, C, H, W, seed=1), (rnd(C, 1, 3, 3, seed=2) / 3).float(), rnd(B, C, H, W, seed=3)
    D.ref = {f: dw_ref(D.x, D.w, f) for f in (0, 1)}
    D.R = {f: bound_of(dw_ref(D.x, D.w, f, torch.float32), D.ref[f]) for f in (0, 1)}
    return D


def dw_abs_bound(D):
    return max(dw_ref(D.x.abs(), D.w.abs(), f).max().item() for f in (0, 1)) + D.old.abs().max().item()


def dw_wgrad_ref(x, g, rows=None):
    """dw[c, ky, kx] = sum dy[b, y, x, c] x[b, y + ky - 1, x + kx - 1, c] in fp64; rows: a (B * H) mask of the rows of dy that count."""
    B, C, H, W = x.shape
    x, g = x.double(), g.double()
    if rows is not None:
        g = g * rows.view(B, 1, H, 1).double()
    xp = F.pad(x, (1, 1, 1, 1))
    out = torch.empty(C, 1, 3, 3, dtype=torch.float64)
    for ky in range(3):
        for kx in range(3):
            out[:, 0, ky, kx] = (g * xp[:, :, ky:ky + H, kx:kx + W]).sum((0, 2, 3))
    return out


@functools.lru_cache(maxsize=None)
def dw_wgrad_data(shape):
    B, H, W, C = shape
    rng = np.random.default_rng([2] + list(shape))
    D = NS(kind="exact", shape=shape, x=ints(rng, 2, B, C, H, W), g=ints(rng, 2, B, C, H, W), old=ints(rng, 3, C, 1, 3, 3))
    D.ref = dw_wgrad_ref(D.x, D.g)
    return D


def dw_wgrad_abs_bound(D):
    return dw_wgrad_ref(D.x.abs(), D.g.abs()).max().item() + D.old.abs().max().item()


# ---- resize
def interp(x, scale):
    return F.interpolate(x, scale_factor=scale, mode="bilinear", align_corners=True)


def up_ref(x, g, scale, dtype):
    x = x.detach().to(dtype, copy=True).requires_grad_(True)
    y = interp(x, scale)
    y.backward(g.to(dtype))
    return y.detach(), x.grad


def lerp_matrix(n_in, n_out):
    """The (n_out, n_in) matrix of one axis of the align_corners=True resize, fp64."""
    A = torch.zeros(n_out, n_in, dtype=torch.float64)
    r = (n_in - 1) / (n_out - 1) if n_out > 1 else 0.0
    for o in range(n_out):
        i0 = min(int(r * o), n_in - 1)
        i1 = min(i0 + 1, n_in - 1)
        l = r * o - i0
        A[o, i0] += 1.0 - l
        A[o, i1] += l
    return A


def up_adjoint(g, Ay, Ax):
    return torch.einsum("oh,bcop,pw->bchw", Ay, g.double(), Ax)


@functools.lru_cache(maxsize=None)
def up_data(case):
    """Scale 1: integers (the resize is the identity: exact).  Else rounded, redrawn while the adjoint's largest element cancels."""
    B, H, W, C, scale, n = case
    OH, OW = H * scale, W * scale
    D = NS(kind="exact" if scale == 1 else "rounded", case=case, draw=0, cond=0.0)
    if scale == 1:
        rng = np.random.default_rng([3] + list(case))
        D.x, D.g, D.old = ints(rng, 3, B, C, H, W), ints(rng, 3, B, C, OH, OW), ints(rng, 3, B, C, H, W)
        D.y, D.dx = up_ref(D.x, D.g, scale, torch.float64)
        D.Ry = D.Rdx = None
    for D.draw in range(MAX_DRAWS if scale > 1 else 0):
        s = 100 * D.draw
        D.x, D.g, D.old = rnd(B, C, H, W, seed=s + 1), rnd(B, C, OH, OW, seed=s + 2), rnd(B, C, H, W, seed=s + 3)
        D.y, D.dx = up_ref(D.x, D.g, scale, torch.float64)
        D.cond = cond_of(D.dx, up_ref(D.x, D.g.abs(), scale, torch.float64)[1])
        if D.cond <= COND_LIMIT:
            break
    if scale > 1:
        y32, dx32 = up_ref(D.x, D.g, scale, torch.float32)
        D.Ry, D.Rdx = bound_of(y32, D.y), bound_of(dx32, D.dx)
    rng = np.random.default_rng([4] + list(case))
    D.gpos = torch.from_numpy(rng.integers(1, 4, (B, C, OH, OW)).astype(np.float32))          # for the conservation of mass
    D.A, D.Dc, D.S = rnd(C, seed=7), rnd(C, seed=8), rnd(C, seed=9)
    return D


# ---- gain
TIE_MIN, TIE_MAX = -4.5, 5.25


def gain_ties(n):
    """Where the minimum and the maximum of p sit: three elements each, in different workgroups of the backward's partial kernel,
    one of them the LAST workgroup's and one in the ragged tail (n = 5: one workgroup, two each)."""
    if n == 5:
        return [0, 3], [1, 4]
    nb = grid_for(n, *BWD_GRID)
    last = 256 * (nb - 1)                              # the first element of the last workgroup
    return [1, last + 5, n - 1], [2, last + 70, n - 2]


@functools.lru_cache(maxsize=None)
def gain_data(n):
    D = NS(kind="rounded", n=n)
    D.p = rnd(n, seed=1).clamp(-4.0, 4.0)
    D.imin, D.imax = gain_ties(n)
    D.p[D.imin], D.p[D.imax] = TIE_MIN, TIE_MAX
    D.x, D.dt, D.old = rnd(n, seed=2).abs() + 0.5, rnd(n, seed=3).abs() + 0.5, rnd(n, seed=4)
    D.tied = torch.zeros(n, dtype=torch.bool)
    D.tied[D.imin + D.imax] = True
    D.out = ref_gain(D.p, D.x)
    D.dx, D.dp = ref_gain_bwd(D.dt, D.x, D.p)
    out32, dx32, dp32 = gain_fp32(D.p, D.x, D.dt)
    D.R = dict(out=bound_of(out32, D.out), dx=bound_of(dx32, D.dx), dx_acc=bound_of(D.old + dx32, D.old.double() + D.dx),
               dp_tied=bound_of(dp32[D.tied], D.dp[D.tied]), dp_rest=bound_of(dp32[~D.tied], D.dp[~D.tied]))
    return D


def gain_fp32(p, x, dt, skip=None):
    """ref_gain and ref_gain_bwd evaluated in fp32.  skip: a mask of elements the backward's sums ignore (a planted error)."""
    p, x, dt = p.float(), x.float(), dt.float()
    mn, mx = p.min(), p.max()
    d = mx - mn
    out = (1.0 + (p - mn) / d) * x
    dn = dt * x
    keep = torch.ones_like(p, dtype=torch.bool) if skip is None else ~skip
    at_mn, at_mx = p == mn, p == mx
    s0, s1 = dn[keep].sum(), (dn * (p - mn))[keep].sum()
    g_mn = (-s0 / d + s1 / d ** 2) / (at_mn & keep).sum()
    g_mx = (-s1 / d ** 2) / (at_mx & keep).sum()
    return out, dt * (1.0 + (p - mn) / d), dn / d + at_mn * g_mn + at_mx * g_mx


def minmax_data(n):
    p = rnd(n, seed=5).clamp(-6.0, 6.0)
    if n == 1:
        p[0] = -1.5
        return p
    where = {255: (100, 200), 2049: (2048, 0), 4095: (4094, 256), 2048 * 2048 + 3: (n - 1, n - 3)}[n]          # (min, max)
    p[where[0]], p[where[1]] = -7.5, 9.25
    return p


# ---- ShuffleAttention
SA_NAMES = ["m.cweight", "m.cbias", "m.sweight", "m.sbias", "m.gn.weight", "m.gn.bias"]
SA_OUT = ["dcw", "dcb", "dsw", "dsb", "dgnw", "dgnb"]


def sa_oracle(x, prm, g, G, dtype):
    """(y, dx, the six parameter gradients) of oracle.vrnet_oracle.shuffle_attention in `dtype`."""
    from oracle import vrnet_oracle as O
    xs = x.detach().to(dtype, copy=True).requires_grad_(True)
    ps = [p.detach().to(dtype, copy=True).requires_grad_(True) for p in prm]
    y = O.shuffle_attention(dict(zip(SA_NAMES, ps)), "m", xs, G)
    y.backward(g.to(dtype))
    return y.detach(), xs.grad, [p.grad.reshape(-1) for p in ps]


def sa_conditioning(x, prm, g, G, grads):
    """sum |terms| / |sum| of the largest element of each parameter gradient.  A term is g x sigmoid' times a factor; x > 0, so
    with |g| the terms of dcw (times a mean > 0), dcb, dsb and dgnb (times sweight) all have one sign; those of dsw carry the
    normalised value gn(x) and those of dgnw xhat, whose signs go into g."""
    from oracle import vrnet_oracle as O
    B, C, H, W = x.shape
    cp = C // (2 * G)
    assert bool((x > 0).all())
    x1 = x.double().reshape(B * G, C // G, H, W)[:, cp:]
    mu = x1.mean((2, 3), keepdim=True)
    xhat = (x1 - mu) * torch.rsqrt(((x1 - mu) ** 2).mean((2, 3), keepdim=True) + 1e-5)
    xn = xhat * prm[4].double()[None, :, None, None] + prm[5].double()[None, :, None, None]
    worst = 0.0
    for names, sign in ((("dcw", "dcb", "dsb", "dgnb"), None), (("dsw",), xn), (("dgnw",), xhat)):
        s = torch.ones(B * G, C // G, H, W, dtype=torch.float64)
        if sign is not None:
            s[:, cp:] = torch.sign(sign)
        mags = sa_oracle(x, prm, g.double().abs() * O.shuffle2(s.reshape(B, C, H, W)), G, torch.float64)[2]
        for nm in names:
            k = SA_OUT.index(nm)
            worst = max(worst, cond_of(grads[k], mags[k].abs()))
    return worst


@functools.lru_cache(maxsize=None)
def sa_data(case):
    B, HW, C, G = case
    cp = C // (2 * G)
    D = NS(kind="rounded", case=case)
    for D.draw in range(MAX_DRAWS):
        s = 100 * D.draw
        D.x, D.g = rnd(B, C, HW, 1, seed=s + 1) + 8.0, rnd(B, C, HW, 1, seed=s + 3)
        D.prm = [rnd(1, cp, 1, 1, seed=s + 10 + i) for i in range(4)] + [rnd(cp, seed=s + 20) * 0.3 + 1, rnd(cp, seed=s + 21)]
        D.y, D.dx, D.grads = sa_oracle(D.x, D.prm, D.g, G, torch.float64)
        D.cond = sa_conditioning(D.x, D.prm, D.g, G, D.grads)
        if D.cond <= COND_LIMIT:
            break
    D.old_dx, D.old = rnd(B, C, HW, 1, seed=30), [rnd(cp, seed=31 + k) for k in range(6)]
    y32, dx32, g32 = sa_oracle(D.x, D.prm, D.g, G, torch.float32)
    D.R = {"y": bound_of(y32, D.y), ("dx", 0): bound_of(dx32, D.dx), ("dx", 1): bound_of(D.old_dx + dx32, D.old_dx.double() + D.dx)}
    for k, nm in enumerate(SA_OUT):
        D.R[(nm, 0)] = bound_of(g32[k], D.grads[k])
        D.R[(nm, 1)] = bound_of(D.old[k] + g32[k], D.old[k].double() + D.grads[k])
    return D


# ================================================================================================ tests that need no GPU
def test_cases_reach_the_branches_they_are_named_after():
    reached = branches()
    assert reached == ALL_BRANCHES, (sorted(map(str, ALL_BRANCHES - reached)), sorted(map(str, reached - ALL_BRANCHES)))


def test_depthwise_forward_plans_of_the_case_table():
    for kernel, shape in DW_FWD + [DW_FWD_BIG]:
        assert dw_fwd_plan(shape).kernel == kernel, shape
        assert math.prod(shape) < 2 ** 31
    plan = lambda i: dw_fwd_plan(DW_FWD[i][1])
    assert plan(0).runs == 2 and plan(1).runs == 3 and plan(1).CQ == 1
    assert (plan(2).items, plan(2).blocks) == (640, 3) and 640 % 256 != 0
    assert plan(3).CQ == 256 and DW_FWD[3][1][1] == 1
    assert DW_FWD[4][1][2] % 8 != 0 and plan(5).npix == 1
    assert (plan(6).PP, plan(6).blocks) == (1, 9) and (plan(7).blocks, plan(7).npix % plan(7).ppb != 0) == (2, True)
    assert DW_FWD[8][1][3] % 4 != 0
    assert DW_FWD[9][1][3] % 4 == 0 and 256 % (DW_FWD[9][1][3] // 4) != 0 and (plan(9).blocks, plan(9).trips) == (1, 2)
    assert DW_FWD[10][1][3] > 1024 and DW_FWD[10][1][3] % 4 == 0
    assert plan(11).total == 8528000 and plan(11).capped and plan(11).blocks == 8192 and plan(11).trips == 5
    big = dw_fwd_plan(DW_FWD_BIG[1])
    assert (big.npix, big.doublings, big.ppb, big.blocks) == (32895, 1, 16, 2056) and cdiv(32895, 8) > 4096
    assert all(dw_fwd_plan(s).doublings == 0 for k, s in DW_FWD if k == "vec")


def test_depthwise_weight_gradient_plans_are_the_librarys(lib):
    for kernel, shape in DW_WGRAD:
        p = dw_wgrad_launch(shape)
        assert p.kernel == kernel, (shape, p.refusal)
        assert p.workspace == lib._lib.vrnet_dwconv3x3_wgrad_workspace(*shape), shape
        assert math.prod(shape) < 2 ** 31 and p.chunks <= 512
    plan = lambda i: dw_wgrad_launch(DW_WGRAD[i][1])
    assert plan(0).TPR == 32 and plan(1).TPR == 64 and 2 * 64 - 33 - 64 == 31 and plan(1).grid_y == 1
    assert plan(2).TPR == 32 and DW_WGRAD[2][1][2] < plan(2).RP == 8
    assert (plan(3).chunks, plan(3).rpc, plan(3).last, plan(3).grid_y) == (17, 10, 4, 2)
    assert [plan(i).refusal for i in range(8)] == ["W % 16 or C % 4"] * 4 + ["groups % nseg", "W > 512", "nseg % groups", "256 % (C/4)"]
    assert plan(6).chunks == 6 and plan(6).grid_y == 4
    p = plan(8); assert (p.quads, p.groups, p.rpar, p.lds, p.chunks, p.rpc) == (1, 256, 256, 36720, 1, 10) and p.rpar > p.rpc
    p = plan(9); assert (p.chunks, p.rpc, p.last) == (2, 11, 10) and 11 % 7 != 0
    p = plan(10); assert (p.quads, p.nseg, p.nsegp) == (2, 2, 2)
    p = plan(11); assert (p.nseg, p.nsegp, p.rpar) == (32, 32, 8) and DW_WGRAD[11][1][2] == 512
    assert DW_WGRAD[12][1][1] == 1 and DW_WGRAD[13][1][1] == 2
    p = plan(14); assert (p.chunks, p.rpc, p.capped, p.grid_y, p.quads) == (300, 2, True, 4, 64) and p.lds <= 65536
    assert all(dw_wgrad_launch(s).lds <= 65536 for k, s in DW_WGRAD if k == "slide")


def test_resize_plans_of_the_case_table():
    def fwd(c): return up_fwd_plan(*c)
    def bwd(c, cs=1, coff=0): return up_bwd_plan(*c, cs, coff)
    for H, W, s in UP_GEOS:
        assert fwd((2, H, W, 8, s, 0)).kernel == "vec" and fwd((2, H, W, 9, s, 0)).kernel == "scalar"
        assert bwd((2, H, W, 8, s, 0)).kernel == "vec" and bwd((2, H, W, 9, s, 0)).kernel == "scalar"
        assert bwd((2, H, W, 8, s, 0), 2, 1).kernel == "vec" and bwd((2, H, W, 8, s, 0), 1, 4).kernel == "vec"
        assert bwd((2, H, W, 8, s, 0), 1, 2).kernel == "scalar"
    assert fwd((2, 4, 5, 9, 3, 1)).kernel == "scalar" and 15 % 4 != 0
    extra = UP_CASES[3 * len(UP_GEOS):]
    assert (fwd(extra[0]).kernel, fwd(extra[0]).segs) == ("nchw4 near 0", 1) and (fwd(extra[1]).kernel, fwd(extra[1]).segs) == ("nchw4 near 0", 2)
    assert (fwd(extra[2]).kernel, fwd(extra[2]).segs) == ("nchw4 near 1", 2) and 36 * 8 == 288
    assert (bwd(extra[3]).kernel, bwd(extra[3]).layout, bwd(extra[3]).segs) == ("scalar", "nchw", 2)
    assert (bwd(extra[4]).kernel, bwd(extra[4]).segs, fwd(extra[4]).segs) == ("vec", 2, 3)
    assert (fwd(extra[5]).kernel, fwd(extra[5]).segs, bwd(extra[5]).segs) == ("vec", 3, 2)
    assert (bwd(extra[6]).kernel, bwd(extra[6]).layout, bwd(extra[6]).segs) == ("scalar", "nhwc", 2)
    assert len(UP_CASES) == len(set(UP_CASES))


def test_adjoint_windows_pass_the_register_window_only_above_scale_4():
    """The generic loop of both adjoint kernels (more than UP_MAXR output columns reach an input column) is what (3, 3, 8) and
    (2, 1, 32) are for; no scale <= 4 reaches it at any width up to 1000."""
    assert up_windows(3, 8).max() == 24 and up_windows(3, 8).min() <= UP_MAXR          # both loops in one launch
    assert up_windows(1, 32).max() == 32
    assert max(up_windows(W, s).max() for s in (1, 2, 3, 4) for W in range(1, 1001)) <= 14 < UP_MAXR


def test_shuffle_attention_plans_are_the_librarys(lib):
    for B, HW, C, G in SA_CASES:
        assert sa_workspace(B, HW, C) == lib._lib.vrnet_sa_bwd_workspace(B, HW, C), (B, HW, C)
        assert C % (2 * G) == 0
    plan = lambda i: sa_plan(*SA_CASES[i][1:3])
    assert (plan(0).TPR, plan(0).ncb, plan(0).chunks) == (256, 2, 4) and plan(1).ncb == 2 and 480 % 256 != 0
    assert (plan(2).chunks, plan(2).rows, 1089 - 17 * 61) == (18, 61, 52)
    assert SA_CASES[3][0] * SA_CASES[3][3] == 264 and SA_CASES[3][2] // (2 * SA_CASES[3][3]) == 1
    assert all(plan(i).chunks == 1 and plan(i).ncb == 1 for i in (3, 4, 5))


def test_reduction_grids_fit_the_librarys_workspace(lib):
    need = lib._lib.vrnet_reduce_workspace()
    assert need == 8192 * 4 * 8 + 256
    assert max(MINMAX_GRID[1] * 2 * 4, FWD_GRID[1] * 2 * 4, BWD_GRID[1] * 4 * 8) <= need - 256
    assert [reduce_class(n, MINMAX_GRID) for n in MINMAX_N] == ["one block", "one block", "several blocks", "several blocks", "capped"]
    assert [reduce_class(n, BWD_GRID) for n in GAIN_N] == ["one block", "several blocks", "capped"]
    assert [reduce_class(n, FWD_GRID) for n in GAIN_N] == ["one block", "several blocks", "several blocks"]
    assert grid_for(2049, *MINMAX_GRID) == 2 and owner(4094, 4095, MINMAX_GRID) == owner(256, 4095, MINMAX_GRID) == 1
    for n in GAIN_N[1:]:          # the ties sit in different workgroups, the last one and the tail among them
        nb = grid_for(n, *BWD_GRID)
        imin, imax = gain_ties(n)
        assert [owner(e, n, BWD_GRID) for e in imin] == [0, nb - 1, owner(n - 1, n, BWD_GRID)] and imin[2] >= n - n % 256
        assert [owner(e, n, BWD_GRID) for e in imax][:2] == [0, nb - 1]
        assert n % 256 != 0
    for n in GAIN_N:
        D = gain_data(n)
        assert int((D.p == D.p.min()).sum()) == len(D.imin) and int((D.p == D.p.max()).sum()) == len(D.imax) and D.p.min() < 0
    for n in MINMAX_N:
        assert minmax_data(n).min() < 0


def test_exact_cases_stay_below_2_24():
    for _, shape in DW_FWD:
        assert dw_abs_bound(dw_data(shape, "exact")) < EXACT_LIMIT, shape
    for _, shape in DW_WGRAD:
        assert dw_wgrad_abs_bound(dw_wgrad_data(shape)) < EXACT_LIMIT, shape
    for case in UP_CASES:
        if case[4] == 1:
            D = up_data(case)
            mags = up_ref(D.x.abs(), D.g.abs(), 1, torch.float64)
            assert max(mags[0].max().item(), mags[1].max().item() + D.old.abs().max().item()) < EXACT_LIMIT


def test_exact_big_depthwise_map_stays_below_2_24():
    assert dw_abs_bound(dw_data(DW_FWD_BIG[1], "exact")) < EXACT_LIMIT


def test_rounded_bounds_stay_below_the_suite_tolerance():
    bounds = [R for _, s in DW_FWD_ROUNDED for R in dw_data(s, "rounded").R.values()]
    for case in UP_CASES:
        D = up_data(case)
        if D.kind == "rounded":
            assert D.cond <= COND_LIMIT, (case, D.cond)
            bounds += [D.Ry, D.Rdx]
    for n in GAIN_N:
        bounds += list(gain_data(n).R.values())
    for case in SA_CASES:
        D = sa_data(case)
        assert D.cond <= COND_LIMIT, (case, D.cond)
        bounds += list(D.R.values())
    for R in bounds:
        assert ULP_FLOOR * 4 <= R.bound <= TOL, R


def test_references_agree_with_autograd():
    """dw_wgrad_ref, lerp_matrix / up_adjoint and gain_fp32 are what the sensitivity tests plant errors in."""
    x, g = rnd(2, 5, 4, 6, seed=1).double(), rnd(2, 5, 4, 6, seed=2).double()
    w = rnd(5, 1, 3, 3, seed=3).double().requires_grad_(True)
    F.conv2d(x, w, None, 1, 1, 1, 5).backward(g)
    assert torch.allclose(dw_wgrad_ref(x, g), w.grad, rtol=0, atol=1e-12)
    for H, W, s in UP_GEOS + [(31, 33, 4)]:
        x, g = rnd(1, 2, H, W, seed=1), rnd(1, 2, H * s, W * s, seed=2)
        y, dx = up_ref(x, g, s, torch.float64)
        Ay, Ax = lerp_matrix(H, H * s), lerp_matrix(W, W * s)
        assert torch.allclose(torch.einsum("oh,bchw,pw->bcop", Ay, x.double(), Ax), y, rtol=0, atol=1e-12)
        assert torch.allclose(up_adjoint(g, Ay, Ax), dx, rtol=0, atol=1e-12)
    D = gain_data(2049)
    out32, dx32, dp32 = gain_fp32(D.p, D.x, D.dt)
    assert dist(out32, D.out) < 1e-6 and dist(dx32, D.dx) < 1e-6 and dist(dp32, D.dp) < 1e-5


# ---- sensitivity: errors planted in the reference must be rejected by the comparisons the GPU tests use
def rejected(call):
    with pytest.raises(AssertionError):
        call()


def test_sensitivity_depthwise_forward():
    """A sliding-window kernel that read zeros for the halo column between two runs of a row."""
    for kind in ("exact", "rounded"):
        D = dw_data((2, 3, 16, 8), kind)
        for flip in (0, 1):
            w = D.w.flip(2, 3) if flip else D.w
            wrong = D.ref[flip].double().clone()
            # outputs x = 8 (the first of run 1) lose column 7, outputs x = 7 (the last of run 0) lose column 8
            xp = F.pad(D.x.double(), (1, 1, 1, 1))
            for ky in range(3):
                wrong[:, :, :, 8] -= w[None, :, 0, ky, 0].double()[:, :, None] * xp[:, :, ky:ky + 3, 8]
                wrong[:, :, :, 7] -= w[None, :, 0, ky, 2].double()[:, :, None] * xp[:, :, ky:ky + 3, 9]
            check(D, D.R[flip], D.ref[flip].float(), D.ref[flip], "the reference itself")
            rejected(lambda: check(D, D.R[flip], wrong.float(), D.ref[flip], "halo zeroed"))


def test_sensitivity_depthwise_weight_gradient():
    """The last row chunk skipped; channel block 1 computed from the channels of block 0."""
    for i in (3, 9, 14):
        shape = DW_WGRAD[i][1]
        D, p = dw_wgrad_data(shape), dw_wgrad_launch(shape)
        rows = torch.arange(shape[0] * shape[1]) < (p.chunks - 1) * p.rpc
        rejected(lambda: same(dw_wgrad_ref(D.x, D.g, rows).float(), D.ref, "last chunk skipped"))
        per = p.TPR if p.kernel == "scalar" else 4 * p.quads
        assert p.grid_y > 1 or i == 9
        if p.grid_y > 1:
            wrong = D.ref.clone()
            wrong[per:2 * per] = D.ref[:per][:wrong[per:2 * per].shape[0]]
            rejected(lambda: same(wrong.float(), D.ref, "channel block aliased"))
        same(D.ref.float(), D.ref, "the reference itself")


def test_sensitivity_resize_adjoint():
    """One term of the window dropped: the last output column that reaches each input column."""
    for case in UP_CASES:
        B, H, W, C, s, n = case
        D = up_data(case)
        Ay, Ax = lerp_matrix(H, H * s), lerp_matrix(W, W * s)
        for drop_x in (True, False):
            A = (Ax if drop_x else Ay).clone()
            for i in range(A.shape[1]):
                A[A[:, i].nonzero().max(), i] = 0.0
            wrong = up_adjoint(D.g, Ay, A) if drop_x else up_adjoint(D.g, A, Ax)
            rejected(lambda: check(D, D.Rdx, wrong.float(), D.dx, "window term dropped"))
        check(D, D.Rdx, up_adjoint(D.g, Ay, Ax).float(), D.dx, "the reference itself")


def test_sensitivity_minmax_and_gain():
    """The last workgroup's partial ignored by the final step."""
    n = 4095
    p = minmax_data(n)
    seen = p[owner(torch.arange(n), n, MINMAX_GRID) != grid_for(n, *MINMAX_GRID) - 1]
    rejected(lambda: same(torch.stack([seen.min(), seen.max()]), torch.stack([p.min(), p.max()]), "last block ignored"))
    for n in GAIN_N[1:]:
        D = gain_data(n)
        skip = owner(torch.arange(n), n, BWD_GRID) == grid_for(n, *BWD_GRID) - 1
        dp = gain_fp32(D.p, D.x, D.dt, skip)[2]
        rejected(lambda: within(D.R["dp_tied"], dp[D.tied], D.dp[D.tied], "last block ignored"))
        tail = torch.arange(n) >= n - n % 256          # ... or the ragged tail
        dp = gain_fp32(D.p, D.x, D.dt, tail)[2]
        rejected(lambda: within(D.R["dp_tied"], dp[D.tied], D.dp[D.tied], "tail ignored"))
        rest = gain_fp32(D.p, D.x, D.dt)[2][~D.tied]
        within(D.R["dp_rest"], rest, D.dp[~D.tied], "the reference itself")
        rejected(lambda: within(D.R["dp_rest"], rest * (1 + 1e-5), D.dp[~D.tied], "dp off by 1e-5"))


def test_sensitivity_shuffle_attention():
    """Channel block 1 aliased onto block 0; the last row chunk of the backward's sums skipped."""
    for case in SA_CASES[:3]:
        B, HW, C, G = case
        D, p = sa_data(case), sa_plan(HW, C)
        if p.ncb > 1:
            for ref, R in ((D.y, D.R["y"]), (D.dx, D.R[("dx", 0)])):
                wrong = ref.clone()
                wrong[:, 256:] = ref[:, :C - 256]
                rejected(lambda: within(R, wrong.float(), ref, "channel block aliased"))
        g = D.g.clone()
        g[:, :, (p.chunks - 1) * p.rows:] = 0.0          # what the sums lose; dx itself still reads the rows
        grads = sa_oracle(D.x, D.prm, g, G, torch.float64)[2]
        for k, nm in enumerate(SA_OUT):
            rejected(lambda: within(D.R[(nm, 0)], grads[k].float(), D.grads[k], nm + ": last chunk skipped"))


# ================================================================================================ running a case on the GPU
LEAD = TAIL = 64      # guard elements in front of and behind every buffer (256 bytes: the payload stays 16-byte aligned)
PADC = 4              # guard columns behind every NHWC row
GUARD = 1024          # ints of PAT behind a workspace: 4 KB
FINITE = 12345.0      # the second poison


class Buf:
    """A flat device buffer: LEAD guard elements | rows of C + padc elements | TAIL guard elements, filled with `fill` (a float, or
    the int PAT: that bit pattern).  .v is the (..., C) view that a kernel is given, .ld its row stride."""

    def __init__(self, shape, fill, data=None, padc=PADC):
        *dims, C = shape
        self.ld, self.dims, self.C = C + padc, dims, C
        self.n = math.prod(dims) * self.ld
        self.flat = torch.empty(LEAD + self.n + TAIL, device="cuda")
        if isinstance(fill, int):
            self.flat.view(torch.int32).fill_(fill)
        else:
            self.flat.fill_(fill)
        self.v = self.flat[LEAD:LEAD + self.n].view(*dims, self.ld)[..., :C]
        if data is not None:
            self.v.copy_(data.reshape(self.v.shape))
        assert self.v.data_ptr() % 16 == 0

    def intact(self):
        """Every element outside .v still holds PAT."""
        raw = self.flat.view(torch.int32).clone()
        raw[LEAD:LEAD + self.n].view(*self.dims, self.ld)[..., :self.C] = PAT
        return bool((raw == PAT).all())


def vec(t, fill=NAN):
    """A contiguous tensor (any shape, flattened) inside guards."""
    return Buf((t.numel(),), fill, t.cuda(), padc=0)


def out_vec(n, old=None):
    return Buf((n,), PAT, None if old is None else old.cuda(), padc=0)


def report(tag, case, D, Rs):
    if D.kind == "rounded":
        Rs = [R for R in Rs if R is not None]
        print(f"{tag} {case}: draw {getattr(D, 'draw', 0)} d32 {min(R.d32 for R in Rs):.2e} .. {max(R.d32 for R in Rs):.2e} bound "
              f"{min(R.bound for R in Rs):.2e} .. {max(R.bound for R in Rs):.2e} kernel {max(R.seen for R in Rs):.2e} "
              f"share {max(R.seen / R.bound for R in Rs):.3f}")


# ---- 1. depthwise forward / data gradient
def run_dw_fwd(hip, shape, kind, forms):
    B, H, W, C = shape
    D = dw_data(shape, kind)
    xb, wb = Buf((B, H, W, C), NAN, nhwc(D.x)), vec(D.w)
    for flip, acc in forms:
        yb = Buf((B, H, W, C), PAT, nhwc(D.old) if acc else None)
        hip.dwconv3x3(xb.v, xb.ld, wb.v, yb.v, yb.ld, B, H, W, C, flip=flip, accumulate=acc)
        ref = D.ref[flip] + D.old.to(D.ref[flip].dtype) if acc else D.ref[flip]
        R = D.R[flip]
        if acc and kind == "rounded":
            R = bound_of(D.old + dw_ref(D.x, D.w, flip, torch.float32), ref)
        check(D, R, nchw(yb.v), ref, f"dw {shape} flip {flip} accumulate {acc}")
        assert yb.intact(), f"dw {shape} flip {flip} accumulate {acc}: a guard element of the output changed"
        if kind == "rounded":
            report("SPATIAL-EDGES dw", (shape, flip, acc), D, [R])


@gpu
@pytest.mark.parametrize("kernel,shape", DW_FWD, ids=str)
def test_depthwise_forward_exact(hip, kernel, shape):
    run_dw_fwd(hip, shape, "exact", DW_FORMS)


@gpu
def test_depthwise_forward_exact_big_map(hip):
    run_dw_fwd(hip, DW_FWD_BIG[1], "exact", DW_FORMS_BIG)


@gpu
@pytest.mark.parametrize("kernel,shape", DW_FWD_ROUNDED, ids=str)
def test_depthwise_forward_rounded(hip, kernel, shape):
    run_dw_fwd(hip, shape, "rounded", DW_FORMS)


# ---- 2. depthwise weight gradient
def launch_dw_wgrad(hip, xb, gb, dwb, shape, acc, poison, short=0):
    """vrnet_dwconv3x3_wgrad_f32 on a workspace of exactly the queried bytes (minus `short`), poisoned, a guard behind it."""
    need = hip._lib.vrnet_dwconv3x3_wgrad_workspace(*shape)
    assert need % 4 == 0
    ws = torch.full((need // 4 + GUARD,), poison, device="cuda")
    ws.view(torch.int32)[need // 4:] = PAT
    rc = hip._lib.vrnet_dwconv3x3_wgrad_f32(hip.ptr(xb.v), xb.ld, hip.ptr(gb.v), gb.ld, hip.ptr(dwb.v), *shape, acc, hip.ptr(ws),
                                            need - short, hip.stream())
    assert bool((ws.view(torch.int32)[need // 4:] == PAT).all()), f"{shape}: the guard behind the workspace changed"
    return rc


@gpu
@pytest.mark.parametrize("kernel,shape", DW_WGRAD, ids=str)
def test_depthwise_weight_gradient_exact(hip, kernel, shape):
    B, H, W, C = shape
    D = dw_wgrad_data(shape)
    xb, gb = Buf((B, H, W, C), NAN, nhwc(D.x)), Buf((B, H, W, C), NAN, nhwc(D.g))
    for acc in (0, 1):
        runs = []
        for poison in (NAN, FINITE):
            dwb = out_vec(C * 9, D.old if acc else None)
            assert launch_dw_wgrad(hip, xb, gb, dwb, shape, acc, poison) == 0
            same(dwb.v.view(C, 1, 3, 3), D.ref + D.old.double() if acc else D.ref, f"dw wgrad {shape} accumulate {acc}")
            assert dwb.intact(), f"dw wgrad {shape}: a guard element of dw changed"
            runs.append(dwb.v.clone())
        assert same_bits(*runs), f"dw wgrad {shape}: two runs differ"
    dwb = out_vec(C * 9)
    assert launch_dw_wgrad(hip, xb, gb, dwb, shape, 0, NAN, short=1) == VR_ERR_WORKSPACE
    torch.cuda.synchronize()
    assert bool((dwb.flat.view(torch.int32) == PAT).all()), "a refused call wrote"


# ---- 3. bilinear resize
def to_layout(t, n):
    """A CPU NCHW tensor as the device tensor a kernel reads: NHWC in guard columns, or contiguous NCHW."""
    B, C, H, W = t.shape
    return vec(t) if n else Buf((B, H, W, C), NAN, nhwc(t))


def from_layout(buf, shape, n):
    B, C, H, W = shape
    return buf.v.view(B, C, H, W).cpu() if n else nchw(buf.v)


def out_layout(shape, n, old=None):
    B, C, H, W = shape
    return out_vec(B * C * H * W, old) if n else Buf((B, H, W, C), PAT, None if old is None else nhwc(old))


@gpu
@pytest.mark.parametrize("case", UP_CASES, ids=str)
def test_resize_forward_and_adjoint(hip, case):
    B, H, W, C, scale, n = case
    OH, OW = H * scale, W * scale
    D = up_data(case)
    xb = Buf((B, H, W, C), NAN, nhwc(D.x))
    # the forward gather
    yb = out_layout(D.y.shape, n)
    hip.upsample(xb.v, xb.ld, yb.v, 0 if n else yb.ld, B, H, W, C, scale, out_nchw=n)
    check(D, D.Ry, from_layout(yb, D.y.shape, n), D.y, f"up {case} fwd")
    assert yb.intact(), f"up {case}: a guard element of y changed"
    if scale == 1:
        assert same_bits(from_layout(yb, D.y.shape, n), D.x), "the identity changed bits"
    # BatchNorm + ReLU on the taps: the bits of affine(pre = 1) + upsample
    A, Dc, S = vec(D.A), vec(D.Dc), vec(D.S)
    act = Buf((B, H, W, C), PAT)
    hip.affine(act.v, act.ld, B, H * W, C, x1=xb.v, ld1=xb.ld, A=A.v, D1=Dc.v, S1=S.v, pre=1)
    y1, y2 = out_layout(D.y.shape, n), out_layout(D.y.shape, n)
    hip.upsample(act.v, act.ld, y1.v, 0 if n else y1.ld, B, H, W, C, scale, out_nchw=n)
    hip.bn_relu_upsample(xb.v, xb.ld, A.v, Dc.v, S.v, y2.v, 0 if n else y2.ld, B, H, W, C, scale, out_nchw=n)
    assert not bool(torch.isnan(y2.v).any()) and same_bits(y1.v, y2.v), f"up {case}: fused BN + ReLU taps differ from affine + upsample"
    assert y2.intact() and bool((y2.v > 0).any())
    # the adjoint, plain and accumulated
    gb = to_layout(D.g, n)
    plain = None
    for acc in (0, 1):
        dxb = Buf((B, H, W, C), PAT, nhwc(D.old) if acc else None)
        hip.upsample_bwd(gb.v, 0 if n else gb.ld, n, dxb.v, dxb.ld, B, H, W, C, scale, accumulate=acc)
        ref = D.old.double() + D.dx if acc else D.dx
        R = D.Rdx if not acc or scale == 1 else bound_of(D.old + up_ref(D.x, D.g, scale, torch.float32)[1], ref)
        check(D, R, nchw(dxb.v), ref, f"up {case} bwd accumulate {acc}")
        assert dxb.intact(), f"up {case}: a guard element of dx changed"
        if not acc:
            plain = dxb.v.clone()
            if scale == 1:
                assert same_bits(nchw(dxb.v), D.g), "the identity's adjoint changed bits"
    # mass: every output's four weights sum to one
    gpb, dxb = to_layout(D.gpos, n), Buf((B, H, W, C), PAT)
    hip.upsample_bwd(gpb.v, 0 if n else gpb.ld, n, dxb.v, dxb.ld, B, H, W, C, scale)
    Rm = D.Rdx or NS(d32=0.0, bound=4 * ULP_FLOOR, seen=0.0)
    within(Rm, nchw(dxb.v).double().sum((2, 3)), D.gpos.double().sum((2, 3)), f"up {case} mass")
    report("SPATIAL-EDGES up", case, D, [D.Ry, D.Rdx])
    if n:
        return
    # the adjoint read in place from a concatenation's gradient: the bits of upsample_bwd on the half copied out
    for cs, coff in CAT_FORMS:
        width = cdiv(coff + cs * C, 4) * 4
        wide = Buf((B, OH, OW, width), NAN, nhwc(rnd(B, width, OH, OW, seed=11)))
        half = Buf((B, OH, OW, C), NAN, wide.v[..., coff:coff + cs * C:cs])
        for acc in (0, 1):
            d1, d2 = (Buf((B, H, W, C), PAT, nhwc(D.old) if acc else None) for _ in range(2))
            hip.upsample_bwd(half.v, half.ld, 0, d1.v, d1.ld, B, H, W, C, scale, accumulate=acc)
            hip.upsample_bwd_cat(wide.v, wide.ld, coff, cs, d2.v, d2.ld, B, H, W, C, scale, accumulate=acc)
            assert not bool(torch.isnan(d2.v).any()), f"up {case} cat cs {cs} coff {coff}: NaN: a column outside the half was read"
            assert same_bits(d1.v, d2.v), f"up {case} cat cs {cs} coff {coff} accumulate {acc}: differs from the half copied out"
            assert d2.intact()


# ---- 4. min / max and the image gain
def p_buf(p):
    """p between +-3e38 instead of NaN: fminf and fmaxf skip a NaN, a guard element that was read would not show."""
    b = vec(p)
    fence = torch.tensor([-3e38, 3e38, -3e38, 3e38], device="cuda")
    b.flat[LEAD - 4:LEAD], b.flat[LEAD + b.n:LEAD + b.n + 4] = fence, fence
    return b


@gpu
@pytest.mark.parametrize("n", MINMAX_N)
def test_minmax_exact(hip, n):
    p = minmax_data(n)
    pb, mm = p_buf(p), out_vec(2)
    hip.minmax(pb.v, n, mm.v)
    same(mm.v, torch.stack([p.min(), p.max()]), f"minmax n = {n}")
    assert mm.intact() and mm.v[0].item() < 0


@gpu
@pytest.mark.parametrize("n", GAIN_N)
def test_gain_against_fp64(hip, n):
    D = gain_data(n)
    pb, xb, gb = p_buf(D.p), vec(D.x), vec(D.dt)
    mm = out_vec(2)
    hip.minmax(pb.v, n, mm.v)
    same(mm.v, torch.tensor([TIE_MIN, TIE_MAX]), "minmax")
    ob = out_vec(n)
    hip.enhance_mul(pb.v, xb.v, mm.v, ob.v, n)
    within(D.R["out"], ob.v.cpu(), D.out, f"gain n = {n}: enhance_mul")
    mm2, ob2 = out_vec(2), out_vec(n)
    hip.enhance_fwd(pb.v, xb.v, mm2.v, ob2.v, n)
    same(mm2.v, torch.tensor([TIE_MIN, TIE_MAX]), "enhance_fwd: mm")
    within(D.R["out"], ob2.v.cpu(), D.out, f"gain n = {n}: enhance_fwd")
    assert ob.intact() and ob2.intact() and mm.intact() and mm2.intact()
    for acc in (0, 1):
        dxb, dpb = out_vec(n, D.old if acc else None), out_vec(n)
        hip.enhance_bwd(gb.v, xb.v, pb.v, mm.v, dxb.v, dpb.v, n, accumulate_dx=acc)
        within(D.R["dx_acc" if acc else "dx"], dxb.v.cpu(), D.old.double() + D.dx if acc else D.dx, f"gain n = {n}: dx accumulate {acc}")
        dp = dpb.v.cpu()
        within(D.R["dp_tied"], dp[D.tied], D.dp[D.tied], f"gain n = {n}: dp on the tied elements")
        within(D.R["dp_rest"], dp[~D.tied], D.dp[~D.tied], f"gain n = {n}: dp elsewhere")
        assert dxb.intact() and dpb.intact()
    report("SPATIAL-EDGES gain", n, D, D.R.values())


@gpu
def test_gain_of_a_constant_map_is_nan_where_the_fp32_formula_is(hip):
    n = 37
    p, x, dt = torch.full((n,), 1.5), rnd(n, seed=2).abs() + 0.5, rnd(n, seed=3).abs() + 0.5
    out32, dx32, dp32 = gain_fp32(p, x, dt)
    assert bool(torch.isnan(out32).all())          # 0 / 0 in every element
    pb, xb, gb = p_buf(p), vec(x), vec(dt)
    mm = out_vec(2)
    hip.minmax(pb.v, n, mm.v)
    same(mm.v, torch.tensor([1.5, 1.5]), "minmax")
    for fused in (0, 1):
        ob, mm2 = out_vec(n), out_vec(2)
        hip.enhance_fwd(pb.v, xb.v, mm2.v, ob.v, n) if fused else hip.enhance_mul(pb.v, xb.v, mm.v, ob.v, n)
        assert torch.equal(torch.isnan(ob.v).cpu(), torch.isnan(out32)) and ob.intact()
    dxb, dpb = out_vec(n), out_vec(n)
    hip.enhance_bwd(gb.v, xb.v, pb.v, mm.v, dxb.v, dpb.v, n)
    assert torch.equal(torch.isnan(dxb.v).cpu(), torch.isnan(dx32)) and torch.equal(torch.isnan(dpb.v).cpu(), torch.isnan(dp32))
    assert dxb.intact() and dpb.intact()


# ---- 5. ShuffleAttention
def launch_sa_bwd(hip, case, acc, gb, xb, coef, mom, params, dxb, grads, EF, poison, short=0):
    """vrnet_sa_bwd_f32 on a workspace of exactly the queried bytes (minus `short`), poisoned, a guard behind it."""
    B, HW, C, G = case
    need = hip._lib.vrnet_sa_bwd_workspace(B, HW, C)
    assert need % 8 == 0
    ws = torch.full((need // 4 + GUARD,), poison, device="cuda")
    ws.view(torch.int32)[need // 4:] = PAT
    ptr = hip.ptr
    rc = hip._lib.vrnet_sa_bwd_f32(ptr(gb.v), gb.ld, ptr(xb.v), xb.ld, *[ptr(c.v) for c in coef], ptr(mom), *[ptr(p.v) for p in params],
                                   ptr(dxb.v), dxb.ld, *[ptr(t.v) for t in grads], ptr(EF.v), B, HW, C, G, acc, acc, ptr(ws),
                                   need - short, hip.stream())
    assert bool((ws.view(torch.int32)[need // 4:] == PAT).all()), f"{case}: the guard behind the workspace changed"
    hip._check(rc, "sa_bwd")


def rows_of(t):
    """(B, C, HW, 1) on the CPU -> (B, HW, C) on the device."""
    return t.squeeze(3).permute(0, 2, 1).contiguous().cuda()


def maps_of(v):
    return v.permute(0, 2, 1).unsqueeze(3).contiguous().cpu()


@gpu
@pytest.mark.parametrize("acc", [0, 1])
@pytest.mark.parametrize("case", SA_CASES, ids=str)
def test_shuffle_attention_against_fp64(hip, case, acc):
    B, HW, C, G = case
    cp = C // (2 * G)
    D = sa_data(case)
    xb, gb = Buf((B, HW, C), NAN, rows_of(D.x)), Buf((B, HW, C), NAN, rows_of(D.g))
    params = [vec(p) for p in D.prm]
    mom = hip.moments(xb.v, xb.ld, B, HW, C)
    coef = [out_vec(B * C) for _ in range(3)]
    hip.sa_coef_fwd(mom, *[p.v for p in params], B, HW, C, G, *[c.v for c in coef])
    yb = Buf((B, HW, C), PAT)
    hip.sa_apply(xb.v, xb.ld, *[c.v for c in coef], yb.v, yb.ld, B, HW, C)
    within(D.R["y"], maps_of(yb.v), D.y, f"sa {case} y")
    assert yb.intact() and all(c.intact() for c in coef)
    fresh = lambda: (Buf((B, HW, C), PAT, rows_of(D.old_dx) if acc else None), [out_vec(cp, D.old[k] if acc else None) for k in range(6)],
                     out_vec(2 * B * C))
    runs = []
    for poison in (NAN, FINITE):
        dxb, grads, EF = fresh()
        launch_sa_bwd(hip, case, acc, gb, xb, coef, mom, params, dxb, grads, EF, poison)
        runs.append([dxb.v.clone()] + [t.v.clone() for t in grads])
        assert dxb.intact() and EF.intact() and all(t.intact() for t in grads), f"sa {case}: a guard element changed"
    within(D.R[("dx", acc)], maps_of(runs[0][0]), D.old_dx.double() + D.dx if acc else D.dx, f"sa {case} dx accumulate {acc}")
    for k, nm in enumerate(SA_OUT):
        within(D.R[(nm, acc)], runs[0][1 + k].cpu(), D.old[k].double() + D.grads[k] if acc else D.grads[k], f"sa {case} {nm} accumulate {acc}")
    assert all(same_bits(a, b) for a, b in zip(*runs)), f"sa {case}: two runs differ"
    dxb, grads, EF = fresh()
    before = [t.flat.clone() for t in [dxb] + grads]
    with pytest.raises(RuntimeError, match="workspace"):
        launch_sa_bwd(hip, case, acc, gb, xb, coef, mom, params, dxb, grads, EF, NAN, short=1)
    torch.cuda.synchronize()
    assert all(same_bits(t.flat, b) for t, b in zip([dxb] + grads, before)), "a refused call wrote"
    print(f"SPATIAL-EDGES sa {case} accumulate {acc}: draw {D.draw} cond {D.cond:.1f}")
    report("SPATIAL-EDGES sa", (case, acc), D, [R for key, R in D.R.items() if key == "y" or key[1] == acc])
