"""The two halves of a ClusterBlock at the edges of their launch plans: the Cluster core (csrc/cluster.hip) in every instantiation
cluster_kernel<NPT, BWD, MAXT> that cluster_plan can choose, the streaming kernel at its chunk edges, and the fused Mlp
(csrc/mlp_fused.hip) at its hidden-width limits -- in the manner of tests/test_norm_edges.py and tests/test_spatial_edges.py, whose
helpers this file imports.

Which kernel a case reaches is not taken on trust: the tests without a gpu mark restate cluster_plan in Python, require that the
restatement equals the library's host-only query vrnet_cluster_plan (hip.cluster_plan: the function the launchers call) for every
N in 1..300 at 1, 256, 257 and 4096 workgroups in both directions, that the state and workspace queries agree with it, that every
case reaches the class it is listed under, and that the union over the case table is the complete list ALL_BRANCHES: every
(T, NPT, direction) class, the live-slot counts np = 1..8 and the region geometries (h = 1, w = 1, odd sides with overlapping
pooling windows, even sides) inside it, and the streaming kernel's chunk edges.  The refusal np > 8 of cluster_plan is
unreachable for N <= 256 (asserted over the sweep, recorded in the list).

Operands: f, v = rnd(seed 1 / 2); the upstream gradient is drawn CORRELATED with the output, g = out / std(out) + 0.5 noise, so
that the sums behind d alpha and d beta do not cancel (conditioning = sum |terms| / |sum| from the reference with alpha, beta as
per-point leaves, required <= COND_LIMIT).  A case whose fp64 reference has more than 1 / 2000 of its points within GAP = 1e-5
of a tie between two DISTINCT centres (twin centres of h = 1 or w = 1 regions tie exactly and go to the lower index on both
sides) is redrawn with the next seeds.  Both are properties of the reference alone.

Comparisons: where the fp64 reference's top-two gap is >= GAP the kernel's idx must be the reference's own arg-max, elsewhere
its choice must lie within GAP of the best; the reference is then teacher-forced with the kernel's idx, and out, wgt, df, dv,
d alpha, d beta must lie within bound_of(reference in fp32, reference in fp64) = 4 max(d32, ULP_FLOOR) in the metric of dist().
The reference cl_ref is the oracle's cluster_core restated so that it also returns the similarity map and takes planted errors;
test_reference_is_the_oracles pins it to oracle.vrnet_oracle.cluster_core.  f, v, g sit in NaN-surrounded buffers, every output
in a PAT-filled Buf (idx: a byte pattern) with guards that must survive; the backward runs through hip._lib on exactly the
queried workspace bytes in front of a 4 KB guard, on a NaN and on a finite poison for equal bits, and is refused one byte short.

The fused Mlp keeps the references and tolerances of test_fused_mlp_against_fp64 / test_fused_mlp_bf16_hidden_tensors
(tests/test_hip_ops.py) at the shapes those tests leave out.

The sensitivity tests (no GPU) plant in the reference the errors these kernels could make -- see test_sensitivity_* -- and require
that the comparisons the GPU tests use reject each.

Measured on an MI355X (the tests print every figure; d32, the bound and the kernel's distance are per output and case):

  every bound of the 30 cases is the floor 4 * ULP_FLOOR = 3.8e-6: d32 of no output exceeds 4.9e-7
  class (T, NPT) forward / backward          d32                  kernel               largest share of a bound
  (64, 1)                    2 cases         1.2e-8 .. 2.6e-7     1.2e-8 .. 2.1e-7     0.056 (dv)
  (64, 2)                    2 cases         2.3e-13 .. 2.3e-7    2.3e-13 .. 2.0e-7    0.052 (df)
  (64, 4)                    3 cases         1.7e-9 .. 2.6e-7     1.7e-9 .. 1.6e-7     0.043 (out)
  (256, 2)                   1 case          6.2e-8 .. 1.6e-7     3.3e-9 .. 1.7e-7     0.045 (dv)
  (512, 2)                   2 cases         1.4e-9 .. 2.9e-7     5.2e-9 .. 2.3e-7     0.059 (df)
  (768, 2)                   2 cases         1.0e-8 .. 3.5e-7     2.2e-8 .. 2.9e-7     0.077 (df)
  (1024, 2)                  2 cases         5.1e-8 .. 4.9e-7     3.3e-8 .. 4.3e-7     0.112 (df)
  (64, 8)                    4 cases         8.1e-10 .. 2.8e-7    8.1e-10 .. 2.1e-7    0.056 (out)
  (128, 8)                   3 cases         6.0e-9 .. 2.9e-7     6.0e-9 .. 2.5e-7     0.066 (df)
  (192, 8)                   3 cases         1.3e-8 .. 3.9e-7     1.1e-8 .. 2.5e-7     0.066 (out)
  (512, 4) / (256, 8)        2 cases         4.4e-9 .. 4.3e-7     4.4e-9 .. 5.2e-7     0.137 (df at 13 x 15; 16 x 16: 0.068)
  streaming                  4 cases         2.2e-8 .. 4.1e-7     2.2e-8 .. 3.4e-7     0.089 (df)
  per output, all classes: out 1.0e-7 .. 3.9e-7, wgt 3.9e-8 .. 1.6e-7 (the fast __expf of vr_sigmoid costs nothing that shows: at
  most 0.041 of the bound), df 8.8e-8 .. 5.2e-7, dv 9.7e-8 .. 2.6e-7, d alpha 8.1e-10 .. 3.5e-7, d beta 2.3e-13 .. 1.0e-7; the
  rotated assignment 5.9e-8 .. 3.0e-7.  No bound had to be widened.
  near-tie shares: 0 for every case of at most 12 workgroups but (2, 1, 16, 24, 32, 2), whose first draw has 6.5e-4 and was redrawn
  (second seeds: 0); 5.3e-5 .. 2.1e-4 at 289 / 294 / 578 workgroups.  Conditioning of d alpha, d beta: 1.00 .. 2.28.
  degenerate operands, 3 shapes x 7 kinds: at most 0.077 of a bound, the 1e12-scaled rows of df 5.8e-8 .. 2.0e-7 of their own
  magnitude (0.051), but for two kinds whose reference leaves the kernel nothing to miss: f constant over a region has df = 0 in
  exact arithmetic (4e-16 in fp64, 1e-7 in fp32: d32 0.12 .. 0.27 of the metric's floor 1e-6, kernels 0.06 .. 0.17), and at
  beta = 30 both fp32 sides round dz to 0 where fp64 keeps 1e-13, so the kernels' d alpha, d beta ARE the fp32 reference's
  (distance = d32 = 8.2e-6 .. 3.3e-3, 0.25 of the bound).  wgt at beta = -30, relative to itself: 2.7e-6.
  fused Mlp, 7 shapes: precision 2: u 1.5e-7 .. 2.4e-7, y 1.4e-7 .. 6.4e-7, dx 2.2e-7 .. 1.6e-6 (d32 of fp32 ATen 2.1e-7 .. 4.1e-7,
  2.1e-7 .. 3.8e-7, 1.6e-7 .. 3.8e-7) of the 2e-5 allowed; precision 1: y at most 3.6e-4, dx at most 7.8e-4 of 2e-3; the recompute
  backward equals the stored-u kernel bit for bit at precision 2 and leaves h 2.8e-3, du 3.0e-3, dx 2.4e-5 at precision 4 (6e-3, 6e-3,
  4e-3 allowed); absent operands: y and dx at most 2.6e-7 at precision 2, 8.5e-4 at precision 1
  the whole file                             111 tests in 6.3 s (3.8 s from the first GPU test), the slowest GPU test 0.6 s

No kernel error was found: every instantiation, the streaming kernel and the fused Mlp read correct and measure correct.  (The two
failures on the way were in this file: a reference leaf that was a view of the cached operands, and zero-centre shapes whose
window size is no power of two, where the reference's averaged sum of a zero window is 1e-17, not zero.)"""
import functools
import math
import time
import types

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests.test_direct_conv import COND_LIMIT, MAX_DRAWS, ULP_FLOOR, dist
from tests.test_hip_ops import _bf16r, close, nhwc, rnd
from tests.test_spatial_edges import FINITE, GUARD, VR_ERR_WORKSPACE, Buf, bound_of, cdiv, ints, rejected, same_bits, vec, within
from tests.test_strided_rows import NAN, PAT

gpu = pytest.mark.gpu
NS = types.SimpleNamespace
GAP = 1e-5                    # the project's own figure: the max_gap assertion of test_cluster_core
TIE_CAP = 1 / 2000
TOL_CEILING = 1e-4            # tests/test_hip_ops.py: TOL, the tolerance of test_cluster_core
ALPHA, BETA = 1.3, -0.2
CL_STATE = 264                # csrc/cluster.hip: floats of forward state per region-head
T0 = time.time()


@pytest.fixture(scope="module")
def hip():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    import asy_vrnet_amd.hip as h
    yield h
    print(f"CLUSTER-EDGES the whole file: {time.time() - T0:.1f} s")


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


# ================================================================================================ cluster_plan, restated
def cluster_plan(N, blocks, bwd):
    """(T, NPT) of csrc/cluster.hip: cluster_plan with VRNET_CLUSTER_T unset; (0, 0): the streaming kernel; None: refused."""
    if N > 256:
        return 0, 0
    t = max(64, cdiv(N, 64) * 64)
    if blocks <= 256 and N > 4 * (t // 8):
        t *= 4
    if not bwd and blocks > 256 and t == 256 and N > 128:
        t = 512
    t = min(t, 1024)
    np_ = cdiv(N, t // 8)
    if np_ > 8:
        return None
    return t, 1 if np_ <= 1 else 2 if np_ <= 2 else 4 if np_ <= 4 else 8


def bwd_workspace(B, E, fold):
    return B * E * fold * fold * 2 * 4 + 256


def bwd_workspace2(B, H, W, E, fold):
    return (B * E * fold * fold * 2 + B * H * W * E) * 4 + 512


def geometry(case):
    B, E, D, H, W, fold = case
    h, w = H // fold, W // fold
    return NS(B=B, E=E, D=D, H=H, W=W, fold=fold, h=h, w=w, N=h * w, blocks=B * E * fold * fold, C=E * D)


def reg(h, w, D, form):
    B, E, fold = form
    return (B, E, D, h * fold, w * fold, fold)


F1, F2, F4 = (1, 2, 1), (2, 1, 2), (1, 3, 2)          # (B, E, fold): 2, 8 and 12 workgroups
M17, M7 = (1, 1, 17), (2, 3, 7)                       # 289 and 294 workgroups; M7: E and fold no powers of two, two samples
STREAM = (0, 0)
CL_CASES = [                                          # ((B, E, D, H, W, fold), forward (T, NPT), backward (T, NPT))
    # few workgroups, T = 64
    (reg(1, 5, 4, F1), (64, 1), (64, 1)),             # h = 1: the centres are pairwise identical
    (reg(2, 4, 8, F4), (64, 1), (64, 1)),
    (reg(3, 3, 12, F1), (64, 2), (64, 2)),            # one point in slot 1
    (reg(4, 4, 16, F2), (64, 2), (64, 2)),
    (reg(3, 7, 20, F1), (64, 4), (64, 4)),            # np 3
    (reg(5, 5, 24, F2), (64, 4), (64, 4)),            # np 4, odd windows
    (reg(4, 8, 28, F1), (64, 4), (64, 4)),
    # few workgroups, four times the threads
    (reg(3, 11, 32, F1), (256, 2), (256, 2)),
    (reg(5, 13, 4, F2), (512, 2), (512, 2)),
    (reg(8, 16, 8, F1), (512, 2), (512, 2)),
    (reg(3, 43, 12, F1), (768, 2), (768, 2)),
    (reg(12, 16, 16, F2), (768, 2), (768, 2)),
    (reg(1, 193, 20, F1), (1024, 2), (1024, 2)),
    (reg(13, 15, 24, F2), (1024, 2), (1024, 2)),
    # many workgroups
    (reg(3, 11, 28, M17), (64, 8), (64, 8)),          # np 5
    (reg(5, 9, 32, M7), (64, 8), (64, 8)),            # np 6
    (reg(7, 7, 4, M17), (64, 8), (64, 8)),            # np 7
    (reg(8, 8, 8, M7), (64, 8), (64, 8)),
    (reg(5, 13, 12, M17), (128, 8), (128, 8)),        # np 5
    (reg(7, 15, 16, M7), (128, 8), (128, 8)),         # np 7
    (reg(8, 16, 20, M17), (128, 8), (128, 8)),
    (reg(3, 43, 24, M7), (192, 8), (192, 8)),         # np 6
    (reg(11, 13, 28, M17), (192, 8), (192, 8)),
    (reg(12, 16, 32, M7), (192, 8), (192, 8)),
    (reg(13, 15, 8, M17), (512, 4), (256, 8)),        # backward np 7
    (reg(16, 16, 32, M7), (512, 4), (256, 8)),        # the production shape: stage 0 at 512 px, batch >= 2
    # streaming
    (reg(1, 257, 4, F1), STREAM, STREAM),             # one live point in the fifth chunk
    (reg(16, 20, 28, F2), STREAM, STREAM),            # 320: exactly five chunks
    (reg(16, 32, 16, F1), STREAM, STREAM),            # 512: eight chunks
    (reg(257, 1, 32, (2, 1, 1)), STREAM, STREAM),     # w = 1
]
CASES = [c[0] for c in CL_CASES]
# once per class: bf16 inputs with plane outputs; one many-workgroup two-stream launch
CLASS_CASES = [CASES[i] for i in (0, 2, 5, 7, 8, 10, 12, 15, 19, 21, 24, 27)]
PAIR_CASE = reg(7, 7, 8, (2, 1, 17))                  # 578 workgroups, 289 per stream: each half is a many-workgroup launch too
# degenerate operands: window sizes |Q| that are powers of two (16, 16, 128), so that a window of integers that sums to zero is an
# exactly zero centre in the reference too, which averages with 1 / |Q| before it sums
DEGENERATE_CASES = [reg(7, 7, 8, F2), reg(7, 7, 8, M17), reg(16, 32, 8, F2)]


def tag_of(G):
    return "h 1" if G.h == 1 else "w 1" if G.w == 1 else "odd" if (G.h % 2 or G.w % 2) else "even"


def cl_branches(case):
    G = geometry(case)
    out, tag = set(), tag_of(G)
    for d, bwd in (("fwd", 0), ("bwd", 1)):
        T, npt = cluster_plan(G.N, G.blocks, bwd)
        out.add(("stream", d, tag) if T == 0 else ("register", T, npt, d, f"np {cdiv(G.N, T // 8)}", tag))
    if T == 0:
        chunks = cdiv(G.N, 64)
        out |= {("stream", "chunks % 4 == 0" if chunks % 4 == 0 else "chunks % 4 != 0"), ("stream", "forward with state"),
                ("stream", "backward from saved state")}
        if G.N % 64 == 1:
            out.add(("stream", "one live point in the last chunk"))
    return out


SWEEP = [(N, blocks, bwd) for N in range(1, 301) for blocks in (1, 256, 257, 4096) for bwd in (0, 1)]


def branches(skip=None):
    out = set()
    for case in CASES:
        if case != skip:
            out |= cl_branches(case)
    if all(cluster_plan(N, blocks, bwd) is not None for N, blocks, bwd in SWEEP):
        out.add(("refusal np > 8", "unreachable for N <= 256"))
    return out


REGISTER_CLASSES = [                                  # T, NPT, directions, (live slots np, geometry)
    (64, 1, "fwd bwd", [(1, "h 1"), (1, "even")]),
    (64, 2, "fwd bwd", [(2, "odd"), (2, "even")]),
    (64, 4, "fwd bwd", [(3, "odd"), (4, "odd"), (4, "even")]),
    (256, 2, "fwd bwd", [(2, "odd")]),
    (512, 2, "fwd bwd", [(2, "odd"), (2, "even")]),
    (768, 2, "fwd bwd", [(2, "odd"), (2, "even")]),
    (1024, 2, "fwd bwd", [(2, "h 1"), (2, "odd")]),
    (64, 8, "fwd bwd", [(5, "odd"), (6, "odd"), (7, "odd"), (8, "even")]),
    (128, 8, "fwd bwd", [(5, "odd"), (7, "odd"), (8, "even")]),
    (192, 8, "fwd bwd", [(6, "odd"), (8, "even")]),
    (256, 8, "bwd", [(7, "odd"), (8, "even")]),
    (512, 4, "fwd", [(4, "odd"), (4, "even")]),
]
ALL_BRANCHES = (
    {("register", T, npt, d, f"np {n}", tag) for T, npt, dirs, forms in REGISTER_CLASSES for d in dirs.split() for n, tag in forms} |
    {("stream", d, tag) for d in ("fwd", "bwd") for tag in ("h 1", "even", "w 1")} |
    {("stream", e) for e in ("one live point in the last chunk", "chunks % 4 == 0", "chunks % 4 != 0", "forward with state",
                             "backward from saved state")} |
    {("refusal np > 8", "unreachable for N <= 256")})

# cases that reach no branch of their own, and why they stay
DUPLICATES = {
    # (these two cover each other: np 6 at T = 192 with odd sides needs one of them, the test below requires that too)
    reg(3, 43, 24, M7): "N = 129, three rows, the first size of T = 192: 11 x 13 reaches the branch with two nearly equal sides",
    reg(11, 13, 28, M17): "N = 143, both sides odd and nearly equal: 3 x 43 reaches the branch with three rows only",
    reg(16, 20, 28, F2): "320 points: exactly five chunks, the last one full; both 257-point cases leave one live point in it",
}


# ================================================================================================ the reference
def regions(t, E, fold):
    """(B, E D, H, W) -> (R, N, D): R = (b, e, f1, f2), n = i w + j (oracle.vrnet_oracle.cluster_core: to_regions)."""
    B, ED, H, W = t.shape
    h, w = H // fold, W // fold
    return t.reshape(B, E, ED // E, fold, h, fold, w).permute(0, 1, 3, 5, 4, 6, 2).reshape(B * E * fold * fold, h * w, ED // E)


def region_rows(m, fold):
    """(B, E, H, W) -> (R, N)."""
    B, E, H, W = m.shape
    h, w = H // fold, W // fold
    return m.reshape(B, E, fold, h, fold, w).permute(0, 1, 2, 4, 3, 5).reshape(-1, h * w)


def region_maps(r, G):
    """(R, N, ...) -> (B, E, H, W, ...)."""
    rest = r.shape[2:]
    k = len(rest)
    t = r.reshape(G.B, G.E, G.fold, G.fold, G.h, G.w, *rest).permute(0, 1, 2, 4, 3, 5, *range(6, 6 + k))
    return t.reshape(G.B, G.E, G.H, G.W, *rest)


def windows(n, once=False):
    lo, hi = (0, (n + 1) // 2), (n // 2, n)
    if once and n % 2:
        hi = ((n + 1) // 2, n)
    return lo, hi


def centre_matrix(h, w, dtype, plant=None):
    """The (4, N) averaging matrix of the 2 x 2 adaptive average pooling; planted: the middle row / column of an odd side
    counted in the first window only ("middle once"), 1 / |Q| taken as 1 / (h/2 w/2) ("floor")."""
    q = torch.zeros(4, h, w, dtype=dtype)
    for i, (r0, r1) in enumerate(windows(h, plant == "middle once")):
        for j, (c0, c1) in enumerate(windows(w, plant == "middle once")):
            q[2 * i + j, r0:r1, c0:c1] = 1.0
    size = max(h // 2, 1) * max(w // 2, 1) if plant == "floor" else ((h + 1) // 2) * ((w + 1) // 2)
    return q.reshape(4, h * w) / size


def distinct_centres(h, w):
    """One index per distinct pooling window: windows coincide along a side of one point."""
    return [m for m in range(4) if not (m & 1 and w == 1) and not (m & 2 and h == 1)]


def cl_ref(f, v, alpha, beta, E, fold, idx=None, plant=None, arg=None):
    """oracle.vrnet_oracle.cluster_core, restated: returns out (B, E D, H, W), wgt, idx, gap (B, E, H, W) and sim (B, E, H, W, 4).
    alpha, beta: floats, one-element tensors or (R, 1, N) per-point leaves.  idx given: teacher-forced.  plant (arg): an error."""
    B, ED, H, W = f.shape
    G = geometry((B, E, ED // E, H, W, fold))
    fr, vr = regions(f, E, fold), regions(v, E, fold)
    keep = torch.ones(G.N, dtype=f.dtype)
    if plant == "last skipped":                       # arg: the first point of the last slot or chunk
        keep[arg:] = 0.0
    Q = centre_matrix(G.h, G.w, f.dtype, plant) * keep
    c, vc = torch.einsum("mn,rnd->rmd", Q, fr), torch.einsum("mn,rnd->rmd", Q, vr)
    fx, cx = fr, c
    if plant == "dims":                               # lanes 4 sub >= D hold the next head's first four channels instead of zeros
        ph = torch.roll(fr[..., :4], -fold * fold, 0)
        fx, cx = torch.cat([fr, ph], -1), torch.cat([c, torch.einsum("mn,rnd->rmd", Q, ph)], -1)
    fn = fx / fx.norm(dim=-1, keepdim=True).clamp_min(1e-12)
    cn = cx / cx.norm(dim=-1, keepdim=True).clamp_min(1e-12)
    sim = torch.sigmoid(beta + alpha * torch.einsum("rmd,rnd->rmn", cn, fn))          # (R, 4, N)
    with torch.no_grad():
        dis = distinct_centres(G.h, G.w)
        sd = sim[:, dis]
        own = torch.tensor(dis)[sd.argmax(1)]
        if plant == "tie high":                       # a tie goes to the higher centre index
            own = 3 - sim.flip(1).argmax(1)
        top = sd.topk(2, dim=1).values if len(dis) > 1 else None
        gap = top[:, 0] - top[:, 1] if top is not None else torch.full_like(sd[:, 0], float("inf"))
    k = own if idx is None else region_rows(idx, fold)
    wgt = sim.gather(1, k[:, None, :]).squeeze(1)
    onehot = F.one_hot(k, 4).to(f.dtype) * keep[None, :, None]
    cnt = onehot.sum(1)
    if plant == "pad counted":                        # arg: padded points of the lane groups, all of them at centre 0
        cnt = cnt + torch.tensor([float(arg), 0.0, 0.0, 0.0], dtype=f.dtype)
    agg = torch.einsum("rnm,rnd->rmd", onehot * wgt[:, :, None], vr)
    a = (agg + vc) / (cnt[:, :, None] + (0.0 if plant == "no +1" else 1.0))
    out = wgt[:, :, None] * a.gather(1, k[:, :, None].expand(-1, -1, G.D))
    out = out.view(B, E, fold, fold, G.h, G.w, G.D).permute(0, 1, 6, 2, 4, 3, 5).reshape(B, ED, H, W)
    return NS(out=out, wgt=region_maps(wgt, G), idx=region_maps(k, G), gap=region_maps(gap, G),
              sim=region_maps(sim.detach().permute(0, 2, 1), G), a=a.detach(), vc=vc.detach(), cnt=cnt.detach(), c=c.detach())


def f32_of(x):
    return float(np.float32(x))


def cl_grads(f, v, g, alpha, beta, E, fold, idx, dtype, plant=None, arg=None):
    """out, wgt and the six gradients of the teacher-forced reference in `dtype`.  float64: alpha and beta (the fp32 values the
    kernel is given) are per-point leaves, so that the terms of d alpha and d beta are at hand: their conditioning, and the
    per-region partial sums."""
    fs, vs = (t.detach().to(dtype, copy=True).requires_grad_(True) for t in (f, v))
    R, N = f.shape[0] * E * fold * fold, (f.shape[2] // fold) * (f.shape[3] // fold)
    shape = (R, 1, N) if dtype == torch.float64 else (1,)
    al = torch.full(shape, f32_of(alpha), dtype=dtype, requires_grad=True)
    be = torch.full(shape, f32_of(beta), dtype=dtype, requires_grad=True)
    r = cl_ref(fs, vs, al, be, E, fold, idx=idx, plant=plant, arg=arg)
    r.out.backward(g.to(dtype))
    o = NS(out=r.out.detach(), wgt=r.wgt.detach(), df=fs.grad, dv=vs.grad, ref=r)
    if dtype == torch.float64:
        o.da_terms, o.db_terms = al.grad.reshape(R, N), be.grad.reshape(R, N)
        o.da, o.db = o.da_terms.sum().reshape(1), o.db_terms.sum().reshape(1)
        o.cond = max((t.abs().sum() / t.sum().abs().clamp_min(1e-300)).item() for t in (o.da_terms, o.db_terms))
    else:
        o.da, o.db = al.grad, be.grad
    return o


NAMES = ("out", "wgt", "df", "dv", "da", "db")


def cl_bounds(g32, g64):
    return {nm: bound_of(getattr(g32, nm), getattr(g64, nm)) for nm in NAMES}


def draw_operands(case, draw, kind="normal"):
    G = geometry(case)
    s = 10 * draw
    shape = (G.B, G.C, G.H, G.W)
    if kind == "ints":
        rng = np.random.default_rng([draw, 7] + list(case))
        return ints(rng, 3, *shape), ints(rng, 3, *shape), ints(rng, 3, *shape)
    return rnd(*shape, seed=s + 1), rnd(*shape, seed=s + 2), rnd(*shape, seed=s + 3)


def upstream(out, noise):
    """g = out / std(out) + 0.5 noise: correlated with the output, so that the sums behind d alpha, d beta do not cancel."""
    return (out.double() / out.double().std() + 0.5 * noise.double()).float()


@functools.lru_cache(maxsize=None)
def cl_data(case, alpha=ALPHA, beta=BETA):
    """The operands of a case (the first draw whose fp64 reference passes the near-tie cap and the conditioning limit) with the
    reference teacher-forced by its own arg-max in both precisions."""
    G = geometry(case)
    D = NS(case=case, G=G, alpha=alpha, beta=beta, redrawn=[])
    for D.draw in range(MAX_DRAWS):
        D.f, D.v, noise = draw_operands(case, D.draw)
        with torch.no_grad():
            own = cl_ref(D.f.double(), D.v.double(), f32_of(alpha), f32_of(beta), G.E, G.fold)
        D.share = (own.gap < GAP).double().mean().item()
        D.g = upstream(own.out, noise)
        D.own = own.idx
        D.g64 = cl_grads(D.f, D.v, D.g, alpha, beta, G.E, G.fold, own.idx, torch.float64)
        D.cond = D.g64.cond
        if D.share <= TIE_CAP and D.cond <= COND_LIMIT:
            break
        D.redrawn.append((D.draw, D.share, D.cond))
    else:
        raise AssertionError(f"{case}: no draw of {MAX_DRAWS} passes the near-tie cap and the conditioning limit: {D.redrawn}")
    D.g32 = cl_grads(D.f, D.v, D.g, alpha, beta, G.E, G.fold, own.idx, torch.float32)
    D.R = cl_bounds(D.g32, D.g64)
    return D


def forced(D, idx):
    """(fp32, fp64, bounds) of the reference teacher-forced with the kernel's assignment."""
    if torch.equal(idx, D.own):
        return D.g32, D.g64, D.R
    G = D.G
    g64 = cl_grads(D.f, D.v, D.g, D.alpha, D.beta, G.E, G.fold, idx, torch.float64)
    g32 = cl_grads(D.f, D.v, D.g, D.alpha, D.beta, G.E, G.fold, idx, torch.float32)
    return g32, g64, cl_bounds(g32, g64)


def check_assignment(D, idx, what):
    """Where the fp64 reference's top-two gap is >= GAP the assignment is the reference's; elsewhere it lies within GAP of the best."""
    ref = D.g64.ref
    clear = ref.gap >= GAP
    assert torch.equal(idx[clear], D.own[clear]), f"{what}: {int((idx != D.own)[clear].sum())} points away from a tie differ from the arg-max"
    assert int(idx.min()) >= 0 and int(idx.max()) <= 3, what
    lost = ref.sim.max(-1).values - ref.sim.gather(-1, idx[..., None]).squeeze(-1)
    assert float(lost.max()) <= GAP, f"{what}: an assigned centre is {float(lost.max()):.3e} below the best"


def compare(R, got, ref, what):
    for nm in NAMES:
        if nm in got:
            within(R[nm], got[nm], getattr(ref, nm), f"{what} {nm}")


# ================================================================================================ tests that need no GPU
def test_cases_reach_the_branches_they_are_named_after():
    reached = branches()
    assert reached == ALL_BRANCHES, (sorted(map(str, ALL_BRANCHES - reached)), sorted(map(str, reached - ALL_BRANCHES)))
    for case, fwd, bwd in CL_CASES:
        G = geometry(case)
        assert (cluster_plan(G.N, G.blocks, 0), cluster_plan(G.N, G.blocks, 1)) == (fwd, bwd), case
        assert (G.blocks <= 256) == ((G.B, G.E, G.fold) in (F1, F2, F4, (2, 1, 1))) and (G.blocks > 256) == ((G.B, G.E, G.fold) in (M17, M7)), case
    assert {c[2] for c in CASES if cluster_plan(geometry(c).N, geometry(c).blocks, 0)[0]} == {4, 8, 12, 16, 20, 24, 28, 32}
    assert {c[2] for c in CASES if not cluster_plan(geometry(c).N, geometry(c).blocks, 0)[0]} >= {4, 28}
    for case in CLASS_CASES + DEGENERATE_CASES + [PAIR_CASE]:
        assert cluster_plan(geometry(case).N, geometry(case).blocks, 0) is not None
    assert {cluster_plan(geometry(c).N, geometry(c).blocks, 1) for c in CLASS_CASES} | {(512, 4)} == \
        {(T, npt) for T, npt, _, _ in REGISTER_CLASSES} | {STREAM}
    assert geometry(PAIR_CASE).blocks == 2 * 289 and cluster_plan(49, 289, 0) == cluster_plan(49, 578, 0) == (64, 8)
    assert [cluster_plan(geometry(c).N, geometry(c).blocks, 1) for c in DEGENERATE_CASES] == [(256, 2), (64, 8), STREAM]
    for c in DEGENERATE_CASES:
        q = ((geometry(c).h + 1) // 2) * ((geometry(c).w + 1) // 2)
        assert q & (q - 1) == 0, c


def test_every_case_is_needed_or_a_named_duplicate():
    spare = {case for case in CASES if branches(skip=case) == ALL_BRANCHES}
    assert spare == set(DUPLICATES), (sorted(spare - set(DUPLICATES)), sorted(set(DUPLICATES) - spare))
    both = set()
    for case in CASES:
        if case not in (reg(3, 43, 24, M7), reg(11, 13, 28, M17)):
            both |= cl_branches(case)
    assert ("register", 192, 8, "bwd", "np 6", "odd") not in both


def test_restated_plan_is_the_librarys(lib):
    """Every N in 1..300 at 1, 256, 257 and 4096 workgroups, both directions; the refusal np > 8 is never reached."""
    for N, blocks, bwd in SWEEP:
        mine = cluster_plan(N, blocks, bwd)
        assert mine is not None, (N, blocks, bwd)
        assert lib.cluster_plan(N, blocks, bwd) == mine, (N, blocks, bwd, lib.cluster_plan(N, blocks, bwd), mine)
        T, npt = mine
        assert T == 0 or (T % 64 == 0 and 64 <= T <= 1024 and npt * (T // 8) >= N and cdiv(N, T // 8) <= npt)
    with pytest.raises(RuntimeError, match="bad shape"):
        lib.cluster_plan(0, 1, 0)
    with pytest.raises(RuntimeError, match="bad shape"):
        lib.cluster_plan(5, 0, 1)


def test_state_and_workspace_queries_agree_with_the_plan(lib):
    L = lib._lib
    for case in CASES + DEGENERATE_CASES + [PAIR_CASE, (2, 4, 32, 32, 32, 2), (1, 4, 24, 64, 64, 2)]:
        G = geometry(case)
        T = lib.cluster_plan(G.N, G.blocks, 1)[0]
        floats = L.vrnet_cluster_state_floats(G.B, G.H, G.W, G.E, G.fold)
        assert (floats > 0) == (T == 0) and floats == (G.blocks * CL_STATE if T == 0 else 0), case
        assert L.vrnet_cluster_bwd_workspace(G.B, G.E, G.fold) == bwd_workspace(G.B, G.E, G.fold), case
        assert L.vrnet_cluster_bwd_workspace2(G.B, G.H, G.W, G.E, G.fold) == bwd_workspace2(G.B, G.H, G.W, G.E, G.fold), case
        # what the kernels index: 2 floats per workgroup; streaming: one float per point and head behind them, 64-float aligned
        assert bwd_workspace(G.B, G.E, G.fold) >= 8 * G.blocks
        assert bwd_workspace2(G.B, G.H, G.W, G.E, G.fold) >= 4 * (cdiv(2 * G.blocks, 64) * 64 + G.B * G.H * G.W * G.E)


def test_reference_is_the_oracles():
    """cl_ref is oracle.vrnet_oracle.cluster_core: output, assignment and all four gradients, free and teacher-forced."""
    from oracle import vrnet_oracle as O
    for h, w in ((1, 5), (5, 5), (4, 8), (3, 1)):
        assert torch.equal(centre_matrix(h, w, torch.float64), O.center_matrix(h, w, torch.float64))
    for case in (reg(5, 5, 24, F2), reg(3, 7, 20, F1), reg(4, 4, 8, (2, 3, 3))):
        G = geometry(case)
        f, v, g = (t.double() for t in draw_operands(case, 0))
        for forced_idx in (None, torch.from_numpy(np.random.default_rng(5).integers(0, 4, (G.B, G.E, G.H, G.W)))):
            leaves = [[t.clone().requires_grad_(True) for t in (f, v, torch.tensor([1.3], dtype=torch.float64),
                                                                torch.tensor([-0.2], dtype=torch.float64))] for _ in range(2)]
            mine = cl_ref(*leaves[0], G.E, G.fold, idx=forced_idx)
            theirs, their_idx = O.cluster_core(*leaves[1], G.E, G.fold, forced_idx=forced_idx)
            assert torch.equal(mine.idx, their_idx)
            assert dist(mine.out, theirs) < 1e-14
            mine.out.backward(g)
            theirs.backward(g)
            for a, b in zip(*leaves):
                assert dist(a.grad, b.grad) < 1e-12


def test_near_ties_and_conditioning_of_every_case():
    """Properties of the fp64 reference alone: at most 1 / 2000 of the points within GAP of a tie; d alpha, d beta conditioned."""
    for case in CASES + [PAIR_CASE]:
        D = cl_data(case)
        print(f"CLUSTER-EDGES {case}: draw {D.draw} near-tie share {D.share:.2e} conditioning {D.cond:.2f} redrawn {D.redrawn}")
        assert D.share <= TIE_CAP and D.cond <= COND_LIMIT, (case, D.share, D.cond)
        assert all(bool(torch.isfinite(getattr(D.g64, nm)).all()) for nm in NAMES), case
        assert all(4 * ULP_FLOOR <= r.bound <= TOL_CEILING for r in D.R.values()), case          # never wider than test_cluster_core's TOL


def test_degenerate_references_stay_finite():
    for case in DEGENERATE_CASES:
        for kind in DEGENERATE_KINDS:
            D = degenerate_data(case, kind)
            for g in (D.g32, D.g64):
                assert all(bool(torch.isfinite(getattr(g, nm)).all()) for nm in NAMES), (case, kind)


def padded(case, bwd=0):
    G = geometry(case)
    T, npt = cluster_plan(G.N, G.blocks, bwd)
    return (64 * cdiv(G.N, 64) if T == 0 else npt * (T // 8)) - G.N


def last_start(case, bwd=0):
    G = geometry(case)
    T, npt = cluster_plan(G.N, G.blocks, bwd)
    pp = 64 if T == 0 else T // 8
    return (cdiv(G.N, pp) - 1) * pp


SENS_CASES = [reg(3, 3, 12, F1), reg(5, 5, 24, F2), reg(7, 15, 16, M7), reg(13, 15, 8, M17), reg(1, 257, 4, F1), reg(16, 20, 28, F2)]


def test_sensitivity_sums_and_windows():
    """A padded slot counted in cnt; the +1 of the denominator dropped; the last ragged slot or chunk skipped; the middle row or
    column of an odd window counted once; 1 / |Q| taken as 1 / (h/2 w/2); dims >= D of a lane group read as non-zero."""
    for case in SENS_CASES:
        D, G = cl_data(case), geometry(case)
        plants = [("no +1", None), ("last skipped", last_start(case))]
        if padded(case):
            plants.append(("pad counted", padded(case)))
        if G.h % 2 and G.h > 1 or G.w % 2 and G.w > 1:
            plants += [("middle once", None), ("floor", None)]
        if G.D < 32:
            plants.append(("dims", None))
        for plant, arg in plants:
            wrong = cl_grads(D.f, D.v, D.g, D.alpha, D.beta, G.E, G.fold, D.own, torch.float64, plant, arg)
            rejected(lambda: within(D.R["out"], wrong.out.float(), D.g64.out, f"{case} {plant}: out"))
            if plant != "no +1":          # (an empty cluster divides by zero there: NaN, refused as such)
                rejected(lambda: within(D.R["dv"], wrong.dv.float(), D.g64.dv, f"{case} {plant}: dv"))
            if plant == "dims":
                rejected(lambda: within(D.R["wgt"], wrong.wgt.float(), D.g64.wgt, f"{case} {plant}: wgt"))
                rejected(lambda: within(D.R["df"], wrong.df.float(), D.g64.df, f"{case} {plant}: df"))
        compare(D.R, {nm: getattr(D.g64, nm).float() for nm in NAMES}, D.g64, f"{case} the reference itself")


def test_sensitivity_ties_and_region_ids():
    """A tie going to the higher centre index; head e or fold cell (f1, f2) transposed in the region id."""
    for case in (reg(1, 5, 4, F1), reg(1, 257, 4, F1), reg(257, 1, 32, (2, 1, 1))):          # twin centres: every point ties
        D, G = cl_data(case), geometry(case)
        with torch.no_grad():
            wrong = cl_ref(D.f.double(), D.v.double(), f32_of(ALPHA), f32_of(BETA), G.E, G.fold, plant="tie high")
        rejected(lambda: check_assignment(D, wrong.idx, f"{case} tie high"))
        check_assignment(D, D.own, f"{case} the reference itself")
    for case in (reg(5, 5, 24, F2), reg(7, 15, 16, M7), reg(16, 20, 28, F2)):
        D, G = cl_data(case), geometry(case)
        for nm in ("out", "df", "dv"):
            ref = getattr(D.g64, nm)
            heads = ref.reshape(G.B, G.E, G.D, G.H, G.W).flip(1).reshape(ref.shape)
            blocks = ref.reshape(G.B, G.C, G.fold, G.h, G.fold, G.w).permute(0, 1, 4, 3, 2, 5).reshape(ref.shape)
            for wrong in (heads if G.E > 1 else None, blocks):
                if wrong is not None:
                    rejected(lambda: within(D.R[nm], wrong.float(), ref, f"{case} {nm}: region id transposed"))
        idx_t = D.own.reshape(G.B, G.E, G.fold, G.h, G.fold, G.w).permute(0, 1, 4, 3, 2, 5).reshape(D.own.shape)
        rejected(lambda: check_assignment(D, idx_t, f"{case}: fold cells transposed"))


def test_sensitivity_clamp_and_last_workgroup():
    """The clamp's projection applied to a zero vector (0 / 0: NaN); d alpha, d beta reduced without the last workgroup."""
    for case in DEGENERATE_CASES:
        for kind in ("zero point", "zero centre"):
            D = degenerate_data(case, kind)
            wrong = D.g64.df.clone()
            hot = D.hot.nonzero()
            assert len(hot), (case, kind)
            wrong[tuple(hot[0])] = float("nan")       # (dh - c_hat (c_hat . dh)) / |c| at |c| = 0
            rejected(lambda: compare_rows(D, D.R, wrong.float(), D.g64.df, D.hot, f"{case} {kind}: projection on a zero vector"))
            compare_rows(D, D.R, D.g64.df.float(), D.g64.df, D.hot, f"{case} {kind}: the reference itself")
    for case in SENS_CASES + [reg(16, 16, 32, M7)]:
        D = cl_data(case)
        for nm, terms in (("da", D.g64.da_terms), ("db", D.g64.db_terms)):
            rejected(lambda: within(D.R[nm], terms[:-1].sum().reshape(1).float(), getattr(D.g64, nm), f"{case} {nm} without the last workgroup"))


# ---- degenerate operands: small integers, so that fp32 and fp64 agree on what is exactly zero
DEGENERATE_KINDS = ("zero point", "zero centre", "alpha 0", "f constant", "alpha -1.3", "beta 30", "beta -30")


@functools.lru_cache(maxsize=None)
def degenerate_data(case, kind):
    G = geometry(case)
    alpha = {"alpha 0": 0.0, "alpha -1.3": -1.3}.get(kind, ALPHA)
    beta = {"beta 30": 30.0, "beta -30": -30.0}.get(kind, BETA)
    D = NS(case=case, G=G, alpha=alpha, beta=beta, kind=kind, draw=0, redrawn=[])
    D.f, D.v, noise = draw_operands(case, 0, "ints")
    fr = D.f.reshape(G.B, G.C, G.fold, G.h, G.fold, G.w)          # a view: edits land in D.f
    if kind == "zero point":
        fr[:, :, :, 1, :, 2] = 0.0                                # point (1, 2) of every region, all heads
    if kind == "zero centre":                                     # window 0 of every region sums to zero, in every channel
        hh, wh = (G.h + 1) // 2, (G.w + 1) // 2
        fr[:, :, :, hh - 1, :, wh - 1] = 0.0
        fr[:, :, :, hh - 1, :, wh - 1] = -fr[:, :, :, :hh, :, :wh].sum((3, 5))
    if kind == "f constant":
        fr[:] = fr[:, :, :, :1, :, :1].clone()
    with torch.no_grad():
        own = cl_ref(D.f.double(), D.v.double(), f32_of(alpha), f32_of(beta), G.E, G.fold)
    D.own = own.idx
    if kind in ("alpha 0", "f constant"):                         # every point ties: centre 0
        D.own = torch.zeros_like(own.idx)
    D.g = upstream(own.out, noise) if float(own.out.double().std()) > 1e-9 else noise
    D.g64 = cl_grads(D.f, D.v, D.g, alpha, beta, G.E, G.fold, D.own, torch.float64)
    D.g32 = cl_grads(D.f, D.v, D.g, alpha, beta, G.E, G.fold, D.own, torch.float32)
    D.R = cl_bounds(D.g32, D.g64)
    # rows of df that carry the 1e12 of a clamped norm: compared relative to their own magnitude, the others as usual
    rows = D.g64.df.reshape(G.B, G.E, G.D, G.H, G.W).abs().amax(2)
    D.hot = (rows > 1e6)[:, :, None].expand(G.B, G.E, G.D, G.H, G.W).reshape(D.g64.df.shape)
    if bool(D.hot.any()):
        D.R["df hot"] = bound_of(D.g32.df[D.hot], D.g64.df[D.hot])
        D.R["df"] = bound_of(D.g32.df[~D.hot], D.g64.df[~D.hot])
    return D


def compare_rows(D, R, got, ref, hot, what):
    if bool(hot.any()):
        within(R["df hot"], got[hot], ref[hot], what + " (the 1e12-scaled rows)")
        within(R["df"], got[~hot], ref[~hot], what + " (the other rows)")
    else:
        within(R["df"], got, ref, what)


# ================================================================================================ running a case on the GPU
class Raw:
    """A device buffer of any type: 256 guard bytes | rows of C + padc elements | 256 guard bytes, every byte 0xA5.  .v is the
    (..., C) view a kernel is given, .ld its row stride in elements."""

    def __init__(self, shape, dtype, padc=0, data=None):
        *dims, C = shape
        self.es = torch.empty((), dtype=dtype).element_size()
        self.ld, self.dims, self.C = C + padc, dims, C
        self.nb = math.prod(dims) * self.ld * self.es
        self.raw = torch.full((256 + self.nb + 256,), 0xA5, dtype=torch.uint8, device="cuda")
        self.v = self.raw[256:256 + self.nb].view(dtype).view(*dims, self.ld)[..., :C]
        if data is not None:
            self.v.copy_(data.reshape(self.v.shape))
        assert self.v.data_ptr() % 16 == 0

    def intact(self):
        """Every byte outside .v still holds 0xA5."""
        mask = torch.ones_like(self.raw, dtype=torch.bool)
        mask[256:256 + self.nb].view(*self.dims, self.ld, self.es)[..., :self.C, :] = False
        return bool((self.raw[mask] == 0xA5).all())


def to_rows(t):
    """(B, C, H, W) on the CPU -> (B, H, W, C) on the device."""
    return nhwc(t)


def to_maps(t):
    """(B, H, W, C) on the device -> (B, C, H, W) on the CPU."""
    return t.permute(0, 3, 1, 2).contiguous().cpu()


class Launch:
    """The device side of one case: inputs in NaN-surrounded buffers, fresh PAT-filled outputs per call."""

    def __init__(self, hip, D):
        G = self.G = D.G
        self.hip, self.D = hip, D
        self.shape, self.eshape = (G.B, G.H, G.W, G.C), (G.B, G.H, G.W, G.E)
        self.f, self.v, self.g = (Buf(self.shape, NAN, to_rows(t)) for t in (D.f, D.v, D.g))
        self.al, self.be = vec(torch.tensor([D.alpha])), vec(torch.tensor([D.beta]))
        self.T = hip.cluster_plan(G.N, G.blocks, 1)[0]
        self.dims = (G.B, G.H, G.W, G.E, G.D, G.fold)

    def fwd(self, idx=None, wgt=True, **kw):
        out, wg = Buf(self.shape, PAT), Buf(self.eshape, PAT, padc=0)
        ix = Raw(self.eshape, torch.uint8, data=idx)
        self.hip.cluster_fwd(self.f.v, self.v.v, self.f.ld, self.al.v, self.be.v, out.v, out.ld, ix.v, wg.v if wgt else None, *self.dims,
                             forced=idx is not None, **kw)
        assert out.intact() and wg.intact() and ix.intact(), f"{self.D.case}: the forward changed a guard element"
        return out, ix, wg

    def bwd(self, ix, poison=NAN, short=0, acc=0, preset=None):
        """vrnet_cluster_bwd_f32 on a workspace of exactly the queried bytes (minus `short`), poisoned, a guard behind it."""
        G, hip, L = self.G, self.hip, self.hip._lib
        need = L.vrnet_cluster_bwd_workspace2(G.B, G.H, G.W, G.E, G.fold) if self.T == 0 else L.vrnet_cluster_bwd_workspace(G.B, G.E, G.fold)
        assert need % 4 == 0
        ws = torch.full((need // 4 + GUARD,), poison, device="cuda")
        ws.view(torch.int32)[need // 4:] = PAT
        df, dv = Buf(self.shape, PAT), Buf(self.shape, PAT)
        dab = Buf((2,), PAT, None if preset is None else preset.cuda(), padc=0)
        before = [t.flat.clone() for t in (df, dv, dab)]
        p = hip.ptr
        rc = L.vrnet_cluster_bwd_f32(p(self.f.v), p(self.v.v), self.f.ld, p(self.al.v), p(self.be.v), p(ix.v), p(self.g.v), self.g.ld,
                                     p(df.v), p(dv.v), df.ld, p(dab.v[0:1]), p(dab.v[1:2]), acc, *self.dims, None, None, None, None,
                                     p(ws), need - short, hip.stream())
        torch.cuda.synchronize()
        assert bool((ws.view(torch.int32)[need // 4:] == PAT).all()), f"{self.D.case}: the guard behind the workspace changed"
        assert df.intact() and dv.intact() and dab.intact(), f"{self.D.case}: the backward changed a guard element"
        if short:
            assert rc == VR_ERR_WORKSPACE, rc
            assert all(same_bits(t.flat, b) for t, b in zip((df, dv, dab), before)), "a refused call wrote"
            return None
        hip._check(rc, "cluster_bwd")
        return df, dv, dab


def results(out, wg, bw):
    df, dv, dab = bw
    return dict(out=to_maps(out.v), wgt=to_maps(wg.v), df=to_maps(df.v), dv=to_maps(dv.v), da=dab.v[0:1].cpu(), db=dab.v[1:2].cpu())


def report(tag, case, D, R):
    for nm in NAMES + ("df hot",):
        if nm in R:
            print(f"{tag} {case} {nm}: d32 {R[nm].d32:.2e} bound {R[nm].bound:.2e} kernel {R[nm].seen:.2e} share {R[nm].seen / R[nm].bound:.3f}")
    print(f"{tag} {case}: draw {D.draw} redrawn {D.redrawn} worst share {max(r.seen / r.bound for r in R.values()):.3f}")


def fresh(R):
    return {k: NS(d32=r.d32, bound=r.bound, seen=0.0) for k, r in R.items()}


@gpu
@pytest.mark.parametrize("case", CASES, ids=str)
def test_cluster_core_at_plan_edges(hip, case):
    D = cl_data(case)
    G, fwd_class, bwd_class = D.G, *[c[1:] for c in CL_CASES if c[0] == case][0]
    assert (hip.cluster_plan(G.N, G.blocks, 0), hip.cluster_plan(G.N, G.blocks, 1)) == (fwd_class, bwd_class)
    X = Launch(hip, D)
    stream = X.T == 0
    out, ix, wg = X.fwd()
    idx = to_maps(ix.v).long()
    check_assignment(D, idx, f"{case} idx")
    g32, g64, R = forced(D, idx)
    R = fresh(R)
    runs = [X.bwd(ix, poison) for poison in (NAN, FINITE)]
    got = results(out, wg, runs[0])
    compare(R, got, g64, f"{case}")
    assert all(same_bits(a.v, b.v) for a, b in zip(*runs)), f"{case}: the backward differs between a NaN and a finite workspace"
    assert X.bwd(ix, short=1) is None
    # ---- equal bits: a second run; the teacher-forced form with the kernel's own assignment
    out2, ix2, wg2 = X.fwd()
    assert same_bits(out2.v, out.v) and torch.equal(ix2.v, ix.v) and same_bits(wg2.v, wg.v), f"{case}: two forward runs differ"
    out3, ix3, _ = X.fwd(idx=ix.v)
    assert same_bits(out3.v, out.v) and torch.equal(ix3.v, ix.v), f"{case}: forced with the kernel's own assignment"
    # ---- the rotated assignment: what the reference computes for it; idx is read, not written
    rot = ((ix.v.long() + 1) % 4).to(torch.uint8)
    out4, ix4, _ = X.fwd(idx=rot)
    assert torch.equal(ix4.v, rot), f"{case}: the forced forward wrote idx"
    with torch.no_grad():
        rot_idx = to_maps(rot).long()
        r64 = cl_ref(D.f.double(), D.v.double(), f32_of(D.alpha), f32_of(D.beta), G.E, G.fold, idx=rot_idx).out
        r32 = cl_ref(D.f, D.v, torch.tensor([D.alpha]), torch.tensor([D.beta]), G.E, G.fold, idx=rot_idx).out
    R["out rotated"] = bound_of(r32, r64)
    within(R["out rotated"], to_maps(out4.v), r64, f"{case} out, rotated assignment")
    # ---- wgt = None: accepted iff the region kernel runs
    if stream:
        with pytest.raises(RuntimeError, match="similarity map"):
            X.fwd(wgt=False)
    else:
        out5, ix5, _ = X.fwd(wgt=False)
        assert same_bits(out5.v, out.v) and torch.equal(ix5.v, ix.v)
    # ---- streaming: forward with state + backward from the saved state = the four-pass backward, bit for bit
    p = (X.f.v, X.v.v, X.f.ld, X.al.v, X.be.v)
    if stream:
        state = torch.full((hip.cluster_state_floats(G.B, G.H, G.W, G.E, G.fold) + GUARD,), NAN, device="cuda")
        state.view(torch.int32)[-GUARD:] = PAT
        out6, ix6, wg6 = X.fwd(state=state)
        assert same_bits(out6.v, out.v) and torch.equal(ix6.v, ix.v) and same_bits(wg6.v, wg.v)
        assert bool((state.view(torch.int32)[-GUARD:] == PAT).all())
        st = state[:-GUARD].view(-1, CL_STATE)
        assert not bool(torch.isnan(st[:, :260]).any()) and bool(torch.isnan(st[:, 260:]).all())
        df6, dv6, dab6 = Buf(X.shape, PAT), Buf(X.shape, PAT), Buf((2,), PAT, padc=0)
        hip.cluster_bwd(*p, ix6.v, X.g.v, X.g.ld, df6.v, dv6.v, df6.ld, dab6.v[0:1], dab6.v[1:2], 0, *X.dims, saved=(wg6.v, state))
        assert all(same_bits(a.v, b.v) for a, b in zip((df6, dv6, dab6), runs[0])), f"{case}: backward from the saved state"
        assert df6.intact() and dv6.intact() and dab6.intact()
    # ---- deferred d alpha, d beta; accumulate_ab onto a preset value
    df7, dv7, dab7 = Buf(X.shape, PAT), Buf(X.shape, PAT), Buf((2,), PAT, padc=0)
    ws = hip.cluster_bwd(*p, ix.v, X.g.v, X.g.ld, df7.v, dv7.v, df7.ld, None, None, 0, *X.dims)
    hip.cluster_ab_reduce_multi([(ws, G.blocks, dab7.v[0:1], dab7.v[1:2], 0)])
    assert all(same_bits(a.v, b.v) for a, b in zip((df7, dv7, dab7), runs[0])), f"{case}: the deferred d alpha, d beta"
    assert dab7.intact()
    preset = torch.tensor([0.75, -1.5])
    acc = X.bwd(ix, acc=1, preset=preset)
    assert same_bits(acc[2].v, preset.cuda() + runs[0][2].v), f"{case}: accumulate_ab"
    report("CLUSTER-EDGES", case, D, R)


@gpu
@pytest.mark.parametrize("case", CLASS_CASES, ids=str)
def test_cluster_bf16_inputs_and_planes(hip, case):
    """bf16 f, v, g with plane outputs = the fp32 run on the widened inputs, bit for bit; the planes are the split of what was
    stored (tests/test_planes_gemm.py: test_producers_write_the_planes_of_what_they_store)."""
    D = cl_data(case)
    G = D.G
    dims, C = (G.B, G.H, G.W, G.E, G.D, G.fold), G.C
    al, be = torch.tensor([D.alpha], device="cuda"), torch.tensor([D.beta], device="cuda")
    half = [to_rows(t).to(torch.bfloat16) for t in (D.f, D.v, D.g)]
    wide = [t.float() for t in half]
    for np_ in (3, 1):
        res = []
        for f, v, g in (half, wide):
            out, dfv = Buf((G.B, G.H, G.W, C), PAT), Buf((G.B, G.H, G.W, 2 * C), PAT)
            ix, wg = Raw((G.B, G.H, G.W, G.E), torch.uint8), Buf((G.B, G.H, G.W, G.E), PAT, padc=0)
            op, dp = hip.Planes.empty(np_, (G.B, G.H, G.W, C), "cuda"), hip.Planes.empty(np_, (G.B, G.H, G.W, 2 * C), "cuda")
            dab = Buf((2,), PAT, padc=0)
            hip.cluster_fwd(f, v, C, al, be, out.v, out.ld, ix.v, wg.v, *dims, planes=op)
            hip.cluster_bwd(f, v, C, al, be, ix.v, g, C, dfv.v[..., :C], dfv.v[..., C:], dfv.ld, dab.v[0:1], dab.v[1:2], 0, *dims, planes=dp)
            assert out.intact() and dfv.intact() and ix.intact() and wg.intact() and dab.intact(), f"{case}: a guard element changed"
            for planes, stored, what in ((op, out.v, "out"), (dp, dfv.v, "[df | dv]")):
                if np_ == 3:
                    assert torch.equal(planes.float(), stored), f"{case} {what}: the three planes do not add up to what was stored"
                else:
                    assert torch.equal(planes.t[0], stored.to(torch.bfloat16)), f"{case} {what}: the plane is not the bf16 rounding"
            res.append((out.v, dfv.v, ix.v, wg.v, dab.v, op.t, dp.t))
        for a, b, what in zip(*res, ("out", "df | dv", "idx", "wgt", "d alpha, d beta", "planes of out", "planes of df | dv")):
            assert torch.equal(a, b), f"{case} np {np_} {what}: bf16 inputs differ from the widened fp32 inputs"


@gpu
def test_cluster_two_stream_many_workgroups(hip):
    """One two-stream launch over more than 256 workgroups per stream-pair = two single-stream launches of its halves."""
    case = PAIR_CASE
    D = cl_data(case)
    G = D.G
    Bh, C = G.B // 2, G.C
    f, v, g = (to_rows(t) for t in (D.f, D.v, D.g))
    al = [torch.tensor([1.3], device="cuda"), torch.tensor([0.7], device="cuda")]
    be = [torch.tensor([-0.2], device="cuda"), torch.tensor([0.3], device="cuda")]
    assert hip.cluster_plan(G.N, G.blocks, 0) == hip.cluster_plan(G.N, G.blocks // 2, 0) == (64, 8)

    def run(sl, B, a, b, **kw):
        out, df, dv = (Buf((B, G.H, G.W, C), PAT) for _ in range(3))
        ix, wg = Raw((B, G.H, G.W, G.E), torch.uint8), Buf((B, G.H, G.W, G.E), PAT, padc=0)
        dab = Buf((4,), PAT, padc=0)
        two = dict(alpha2=kw["alpha2"], beta2=kw["beta2"]) if kw else {}
        hip.cluster_fwd(f[sl], v[sl], C, a, b, out.v, out.ld, ix.v, wg.v, B, G.H, G.W, G.E, G.D, G.fold, **two)
        if kw:
            two.update(dalpha2=dab.v[2:3], dbeta2=dab.v[3:4])
        hip.cluster_bwd(f[sl], v[sl], C, a, b, ix.v, g[sl], C, df.v, dv.v, df.ld, dab.v[0:1], dab.v[1:2], 0, B, G.H, G.W, G.E, G.D, G.fold, **two)
        assert all(t.intact() for t in (out, df, dv, ix, wg)), "a guard element changed"
        return out.v, ix.v, wg.v, df.v, dv.v, dab.v

    both = run(slice(0, G.B), G.B, al[0], be[0], alpha2=al[1], beta2=be[1])
    for i in range(2):
        sl = slice(i * Bh, (i + 1) * Bh)
        one = run(sl, Bh, al[i], be[i])
        for a, b, what in zip(both[:5], one[:5], ("out", "idx", "wgt", "df", "dv")):
            assert torch.equal(a[sl], b), f"stream {i}: {what}"
        assert same_bits(both[5][2 * i:2 * i + 2], one[5][0:2]), f"stream {i}: d alpha, d beta"


@gpu
@pytest.mark.parametrize("kind", DEGENERATE_KINDS)
@pytest.mark.parametrize("case", DEGENERATE_CASES, ids=str)
def test_cluster_degenerate_operands(hip, case, kind):
    D = degenerate_data(case, kind)
    G = D.G
    X = Launch(hip, D)
    state = None
    if X.T == 0:
        state = torch.full((hip.cluster_state_floats(G.B, G.H, G.W, G.E, G.fold),), NAN, device="cuda")
    out, ix, wg = X.fwd(**({} if state is None else dict(state=state)))
    idx = to_maps(ix.v).long()
    check_assignment(D, idx, f"{case} {kind} idx")
    if kind in ("alpha 0", "f constant"):
        assert int(idx.max()) == 0, f"{case} {kind}: every point ties, so every point belongs to centre 0"
    if kind == "zero point":
        assert int(idx.reshape(G.B, G.E, G.fold, G.h, G.fold, G.w)[:, :, :, 1, :, 2].max()) == 0, "a zero point ties: centre 0"
    assert torch.equal(idx, D.own) or kind not in ("alpha 0", "f constant")
    g32, g64, R = forced(D, idx) if not torch.equal(idx, D.own) else (D.g32, D.g64, D.R)
    if "df hot" in D.R and "df hot" not in R:
        R["df hot"], R["df"] = bound_of(g32.df[D.hot], g64.df[D.hot]), bound_of(g32.df[~D.hot], g64.df[~D.hot])
    R = fresh(R)
    bw = X.bwd(ix)
    got = results(out, wg, bw)
    df = got.pop("df")
    compare(R, got, g64, f"{case} {kind}")
    compare_rows(D, R, df, g64.df, D.hot, f"{case} {kind} df")
    if kind == "alpha 0" and state is not None:                   # counts (N, 0, 0, 0); the empty clusters give a_m = vc_m
        st = state.view(-1, CL_STATE).cpu()
        assert torch.equal(st[:, 256:260], torch.tensor([float(G.N), 0.0, 0.0, 0.0]).expand(G.blocks, 4))
        a = st[:, 128:256].reshape(-1, 4, 32)[:, :, :G.D]
        within(bound_of(g32.ref.a, g64.ref.a), a, g64.ref.a, f"{case} {kind} a_m")
        within(bound_of(g32.ref.vc[:, 1:], g64.ref.vc[:, 1:]), a[:, 1:], g64.ref.vc[:, 1:], f"{case} {kind} a_m = vc_m of the empty clusters")
    if kind.startswith("beta"):
        rel = ((got["wgt"].double() - g64.wgt).abs() / g64.wgt.abs()).max().item()
        print(f"CLUSTER-EDGES {case} {kind}: wgt relative to itself {rel:.2e}; max |dz| share: df max {float(df.abs().max()):.2e}")
    report("CLUSTER-EDGES degenerate " + kind, case, D, R)


# ================================================================================================ the fused Mlp
MLP_SHAPES = [                                        # (C, hid, M)
    (128, 32, 32),                                    # a single chunk at C = 128, one live wave
    (64, 64, 160),                                    # two chunks: both LDS stages once; the second workgroup has one live wave
    (128, 96, 288),
    (64, 2560, 128), (128, 2560, 32),                 # the maximum hidden width: the whole bias copy in LDS
    (64, 1024, 64), (128, 1536, 64),                  # the recompute backward at its limits
]
MLP_OPERANDS = ("b1", "b2", "res", "res_scale", "dy_scale")


@functools.lru_cache(maxsize=None)
def mlp_data(shape):
    C, hid, M = shape
    return NS(x=rnd(M, C, seed=1), res=rnd(M, C, seed=2), w1=rnd(hid, C, seed=3) / np.sqrt(C), b1=rnd(hid, seed=4),
              w2=rnd(C, hid, seed=5) / np.sqrt(hid), b2=rnd(C, seed=6), ls=rnd(C, seed=7), dy=rnd(M, C, seed=8))


def gelu_grad(u):
    cdf = 0.5 * (1 + torch.erf(u / np.sqrt(2.0)))
    return cdf, cdf + u * torch.exp(-0.5 * u * u) / np.sqrt(2 * np.pi)


def mlp_forward_ref(I, rd, absent=(), dt=torch.float64):
    """test_fused_mlp_against_fp64's reference, with the formula of each absent operand.  res_scale without res: ignored."""
    d = lambda t: t.to(dt)
    u = d(rd(I.x)) @ d(rd(I.w1)).T + (0 if "b1" in absent else d(I.b1))
    t = d(rd(F.gelu(u).float())) @ d(rd(I.w2)).T + (0 if "b2" in absent else d(I.b2))
    if "res" in absent:
        return u, t
    return u, d(I.res) + (t if "res_scale" in absent else d(I.ls) * t)


def mlp_backward_ref(I, rd, uu, absent=()):
    d = lambda t: t.double()
    dh = d(rd(I.dy if "dy_scale" in absent else I.dy * I.ls)) @ d(rd(I.w2))
    cdf, gp = gelu_grad(uu)
    du = dh * gp
    return uu * cdf, du, d(rd(du.float())) @ d(rd(I.w1)), dh


class MlpRun:
    """One forward + backward of the fused Mlp at `precision` in guarded buffers with padded rows."""

    def __init__(self, hip, shape, precision, absent=(), u_from=None):
        C, hid, M = shape
        I = mlp_data(shape)
        hdt = torch.bfloat16 if precision == 4 else torch.float32
        opt = lambda name, t: None if name in absent else vec(t).v
        self.x, self.res, self.dy = (Buf((M, C), NAN, t.cuda()) for t in (I.x, I.res, I.dy))
        w1, w2 = I.w1.cuda(), I.w2.cuda()
        self.fwd_pack, self.bwd_pack = hip.mlp_pack(w1, w2, C, hid, precision)
        self.y, self.dx = Buf((M, C), PAT), Buf((M, C), PAT)
        self.u, self.h, self.du = (Raw((M, hid), hdt, padc=8) for _ in range(3))
        self.tiles, nb = cdiv(M, 128) * 4, C // 32
        self.stats = Raw((self.tiles * nb * 2,), torch.float64)
        res = None if "res" in absent else self.res
        hip.mlp_fwd(self.x.v, self.x.ld, self.fwd_pack, opt("b1", I.b1), opt("b2", I.b2), None if res is None else res.v, 0 if res is None else res.ld,
                    opt("res_scale", I.ls), self.y.v, self.y.ld, self.u.v, self.u.ld, self.stats.v, M, C, hid, precision)
        self.kernel = hip.last_kernel()
        u_in = self.u if u_from is None else u_from
        hip.mlp_bwd(self.dy.v, self.dy.ld, opt("dy_scale", I.ls), self.bwd_pack, u_in.v, u_in.ld, self.h.v, self.h.ld, self.du.v, self.du.ld,
                    self.dx.v, self.dx.ld, M, C, hid, precision)
        torch.cuda.synchronize()
        assert all(t.intact() for t in (self.y, self.dx, self.u, self.h, self.du, self.stats)), f"mlp {shape}: a guard element changed"
        # the pairs of live 32-row tiles are the fp64 sums of the stored y; those of dead tiles keep their bytes
        pairs = self.stats.v.view(self.tiles, nb, 2)
        yd = self.y.v.double().reshape(M // 32, 32, nb, 32)
        close(pairs[:M // 32, :, 0], yd.sum((1, 3)), 1e-9, what="tile sums")
        close(pairs[:M // 32, :, 1], (yd * yd).sum((1, 3)), 1e-9, what="tile sums of squares")
        assert bool((pairs[M // 32:].contiguous().view(torch.uint8) == 0xA5).all()), f"mlp {shape}: the pairs of a dead tile changed"


def mlp_report(shape, precision, what, got, ref, ref32):
    print(f"MLP-EDGES {shape} precision {precision} {what}: kernel {dist(got, ref):.2e} d32 {dist(ref32, ref):.2e}")


@gpu
@pytest.mark.parametrize("precision", [2, 1, 4])
@pytest.mark.parametrize("shape", MLP_SHAPES, ids=str)
def test_fused_mlp_at_plan_edges(hip, shape, precision):
    C, hid, M = shape
    I = mlp_data(shape)
    assert hip.mlp_fused_ok(C, hid, M)
    if precision == 4:
        # test_fused_mlp_bf16_hidden_tensors: the kernels of precision 1 with u, h, du stored as bf16
        one, four = MlpRun(hip, shape, 1), MlpRun(hip, shape, 4)
        assert four.kernel == 8
        assert torch.equal(four.y.v, one.y.v) and torch.equal(four.u.v, one.u.v.to(torch.bfloat16))
        ub = Raw((M, hid), torch.float32, padc=8, data=four.u.v.float())
        again = MlpRun(hip, shape, 1, u_from=ub)      # precision 1 fed the SAME rounded u
        assert torch.equal(four.dx.v, again.dx.v)
        assert torch.equal(four.h.v, again.h.v.to(torch.bfloat16)) and torch.equal(four.du.v, again.du.v.to(torch.bfloat16))
    else:
        rd = _bf16r if precision == 1 else (lambda t: t)
        X = MlpRun(hip, shape, precision)
        assert X.kernel == (7 if precision == 2 else 8)
        tol = 2e-5 if precision == 2 else 2e-3
        u_ref, y_ref = mlp_forward_ref(I, rd)
        u32, y32 = mlp_forward_ref(I, rd, dt=torch.float32)
        close(X.u.v, u_ref, 2e-5, what="u")
        close(X.y.v, y_ref, tol, what="y")
        uu = X.u.v.double().cpu()
        h_ref, du_ref, dx_ref, dh = mlp_backward_ref(I, rd, uu)
        close(X.h.v, h_ref, 2e-6, what="recomputed h")
        close(X.du.v, du_ref, 2e-5, what="du")
        close(X.dx.v, dx_ref, tol, what="dx")
        dx32 = (rd((dh.float() * gelu_grad(uu.float())[1])) @ rd(I.w1))
        for what, got, ref, r32 in (("u", X.u.v, u_ref, u32), ("y", X.y.v, y_ref, y32), ("dx", X.dx.v, dx_ref, dx32)):
            mlp_report(shape, precision, what, got, ref, r32)
        # without the pre-activation output and without statistics
        y2 = Buf((M, C), PAT)
        hip.mlp_fwd(X.x.v, X.x.ld, X.fwd_pack, I.b1.cuda(), I.b2.cuda(), X.res.v, X.res.ld, I.ls.cuda(), y2.v, y2.ld, None, 0, None, M, C, hid, precision)
        assert same_bits(y2.v, X.y.v) and y2.intact()
    # ---- the backward that recomputes u from x: precision 2 = the stored-u kernel's bits; precision 4 held to the existing bounds
    if not hip.mlp_rc_ok(C, hid) or precision == 1:
        return
    rc = hip.mlp_pack_rc(I.w1.cuda(), I.w2.cuda(), C, hid, precision)
    hdt = torch.bfloat16 if precision == 4 else torch.float32
    h2, du2, dx2 = Raw((M, hid), hdt, padc=8), Raw((M, hid), hdt, padc=8), Buf((M, C), PAT)
    Y = X if precision == 2 else four
    hip.mlp_bwd_rc(Y.dy.v, Y.dy.ld, I.ls.cuda(), rc, Y.x.v, Y.x.ld, I.b1.cuda(), h2.v, h2.ld, du2.v, du2.ld, dx2.v, dx2.ld, M, C, hid, precision)
    assert h2.intact() and du2.intact() and dx2.intact()
    if precision == 2:
        assert hip.last_kernel() == 7
        assert torch.equal(h2.v, X.h.v) and torch.equal(du2.v, X.du.v) and same_bits(dx2.v, X.dx.v), f"mlp {shape}: recomputed u"
    else:
        ue = mlp_forward_ref(I, _bf16r)[0]
        h_e, du_e, dx_e, _ = mlp_backward_ref(I, _bf16r, ue)
        close(h2.v.float(), h_e, 6e-3, what="rc h (bf16)")
        close(du2.v.float(), du_e, 6e-3, what="rc du (bf16)")
        close(dx2.v, dx_e, 4e-3, what="rc dx")
        print(f"MLP-EDGES {shape} precision 4 recompute: h {dist(h2.v.float(), h_e):.2e} du {dist(du2.v.float(), du_e):.2e} dx {dist(dx2.v, dx_e):.2e}")


def test_recompute_limits_of_the_fused_mlp(lib):
    L = lib._lib
    for C, top in ((64, 1024), (128, 1536)):
        assert L.vrnet_mlp_rc_ok(C, top, 32) and not L.vrnet_mlp_rc_ok(C, top + 32, 32) and L.vrnet_mlp_fused_ok(C, top + 32, 32)
    assert L.vrnet_mlp_fused_ok(64, 2560, 32) and not L.vrnet_mlp_fused_ok(64, 2592, 32) and not L.vrnet_mlp_fused_ok(128, 2592, 32)
    assert {s[:2] for s in MLP_SHAPES} >= {(64, 1024), (128, 1536), (64, 2560), (128, 2560)}
    for C, hid, M in MLP_SHAPES:
        assert M % 32 == 0 and L.vrnet_mlp_fused_ok(C, hid, M)
    assert 160 % 128 == 32 and 288 % 128 == 32          # a last workgroup with one live wave


@gpu
@pytest.mark.parametrize("precision", [2, 1])
@pytest.mark.parametrize("absent", [(nm,) for nm in MLP_OPERANDS] + [("res_scale", "res"), MLP_OPERANDS], ids=str)
def test_fused_mlp_absent_operands(hip, absent, precision):
    """Each optional operand taken away, then all of them, against the reference of that formula.  res_scale given without res
    is ignored by the kernel (the case ("res",) gives res_scale alone): pinned here."""
    shape = (64, 64, 160)
    C, hid, M = shape
    I = mlp_data(shape)
    rd = _bf16r if precision == 1 else (lambda t: t)
    tol = 2e-5 if precision == 2 else 2e-3
    X = MlpRun(hip, shape, precision, absent)
    u_ref, y_ref = mlp_forward_ref(I, rd, absent)
    close(X.u.v, u_ref, 2e-5, what=f"u without {absent}")
    close(X.y.v, y_ref, tol, what=f"y without {absent}")
    _, du_ref, dx_ref, _ = mlp_backward_ref(I, rd, X.u.v.double().cpu(), absent)
    close(X.du.v, du_ref, 2e-5, what=f"du without {absent}")
    close(X.dx.v, dx_ref, tol, what=f"dx without {absent}")
    if absent == ("res",):
        both = MlpRun(hip, shape, precision, ("res", "res_scale"))
        assert same_bits(both.y.v, X.y.v), "res_scale without res is ignored"
    print(f"MLP-EDGES absent {absent} precision {precision}: y {dist(X.y.v, y_ref):.2e} dx {dist(X.dx.v, dx_ref):.2e}")


@gpu
def test_fused_mlp_refusals_leave_the_outputs_untouched(hip):
    C, hid, M = 64, 64, 64
    I = mlp_data((C, hid, M))
    fwd, bwd = hip.mlp_pack(I.w1.cuda(), I.w2.cuda(), C, hid, 2)
    x, dy = Buf((M, C), NAN, I.x.cuda()), Buf((M, C), NAN, I.dy.cuda())
    y, u, h, du, dx = Buf((M, C), PAT), Buf((M, hid), PAT), Buf((M, hid), PAT), Buf((M, hid), PAT), Buf((M, C), PAT)
    b1 = torch.zeros(hid + 4, device="cuda")
    before = [t.flat.clone() for t in (y, u, h, du, dx)]
    f = lambda **k: hip.mlp_fwd(x.v, x.ld, fwd, k.get("b1"), None, None, 0, None, y.v, y.ld, u.v, k.get("ldu", u.ld), None, k.get("M", M), C,
                                k.get("hid", hid), 2)
    b = lambda **k: hip.mlp_bwd(dy.v, dy.ld, None, bwd, u.v, k.get("ldu", u.ld), h.v, h.ld, du.v, du.ld, dx.v, dx.ld, k.get("M", M), C,
                                k.get("hid", hid), 2)
    for call in (f, b):
        with pytest.raises(RuntimeError, match="no fused Mlp kernel"):
            call(hid=2592)
        with pytest.raises(RuntimeError, match="no fused Mlp kernel"):
            call(M=48)
        with pytest.raises(RuntimeError, match="row stride smaller than width"):
            call(ldu=hid - 4)
    with pytest.raises(RuntimeError, match="16-byte aligned"):
        f(b1=b1[1:hid + 1])
    for top, C2 in ((1056, 64), (1568, 128)):
        assert not hip.mlp_rc_ok(C2, top) and hip.mlp_fused_ok(C2, top, 32)
        w1, w2 = torch.zeros(top, C2, device="cuda"), torch.zeros(C2, top, device="cuda")
        with pytest.raises(RuntimeError, match="no recompute kernel"):
            hip.mlp_pack_rc(w1, w2, C2, top, 2)
        z = torch.zeros(32, top, device="cuda")
        with pytest.raises(RuntimeError, match="no recompute kernel"):
            hip.mlp_bwd_rc(z, top, None, z, z, top, None, z, top, z, top, z, top, 32, C2, top, 2)
    torch.cuda.synchronize()
    assert all(same_bits(t.flat, b0) for t, b0 in zip((y, u, h, du, dx), before)), "a refused call wrote"
