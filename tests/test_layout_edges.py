"""The layout, copy and patch kernels at their edges, bit for bit.

stream_ops.hip: nchw_to_nhwc (the one-thread-per-pixel kernel of the network's 3- and 4-channel inputs and the 32 x 33 tile
kernel), nhwc_to_nchw, copy_channels, add, fill; spatial.hip: patch_gather, patch_scatter, weight_ohwi.  All of them move data,
so every comparison is torch.equal on int32 views -- no tolerance anywhere; the accumulating forms are one IEEE fp32 add per
element, which the CPU reproduces exactly.

Every operand is a strided view of a flat buffer (lead floats in front, TAIL behind the last row, ld - C between the rows:
embed() of tests/test_strided_rows.py with the contiguous layout ld == C added, which that helper's trailing columns rule out).
Inputs sit in NaN, so a read outside the logical tensor poisons a result; outputs sit in PAT, and every element outside the
logical result -- lead, row padding, the floats behind the last row -- must keep it.  An output that is overwritten starts as PAT
too: an element the kernel skips shows.  Copied values carry -0.0, +-inf and NaNs with payloads; the accumulating forms are
fed -0.0 and +inf but no NaN (the payload a NaN sum keeps is not part of the contract).

There is no kernel-family counter for these ops: which kernel a case reaches is read from the launchers' source and written
down at each test."""
import functools

import pytest
import torch

from tests.test_hip_ops import rnd
from tests.test_strided_rows import NAN, PAT, hip, refused      # noqa: F401  (hip: the fixture)

pytestmark = pytest.mark.gpu

TAIL = 4          # floats behind the last row of every buffer
I32 = torch.int32


# ------------------------------------------------------------------------------------------------ helpers
def bits(t):
    return t.contiguous().view(I32)


def same(got, ref, what):
    got, ref = got.detach().cpu().contiguous(), ref.detach().cpu().contiguous()
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    bad = bits(got) != bits(ref)
    assert not bool(bad.any()), f"{what}: {int(bad.sum())} of {ref.numel()} elements differ in bits, first at " \
                                f"{tuple(bad.nonzero()[0].tolist())}"


def payload(*shape, seed, nan=True):
    """Random normal values with a few -0.0, +-inf (and NaNs with payloads) planted: a copy must carry bits."""
    t = rnd(*shape, seed=seed).contiguous()
    flat, n = t.view(-1), t.numel()
    specials = [-0.0, float("inf")] + ([float("-inf")] if nan else [])
    for j, v in enumerate(specials):
        flat[(7 * j + 3) % n] = v
    if nan:
        raw = flat.view(I32)
        raw[(n // 2 + 1) % n] = 0x7FC12345
        raw[(n - 1) - (n // 3)] = -0x3AB3FF           # 0xFFC54C01: a negative quiet NaN with a payload
    return t


def strided(rows, C, ld, lead, fill, data=None):
    """A flat device buffer of lead + rows * ld + TAIL floats filled with `fill` (a float, or the int PAT: that bit pattern)
    and its (rows, C) view with row stride ld at float offset lead; `data` (rows, C) is copied into the view."""
    assert ld >= C and rows > 0
    buf = torch.empty(lead + rows * ld + TAIL, device="cuda")
    if isinstance(fill, int):
        buf.view(I32).fill_(fill)
    else:
        buf.fill_(fill)
    view = buf.as_strided((rows, C), (ld, 1), lead)
    if data is not None:
        view.copy_(data.reshape(rows, C))
    assert view.data_ptr() == buf.data_ptr() + 4 * lead and buf.data_ptr() % 16 == 0
    return buf, view


def outside(buf, view):
    """True for the floats of buf that are not part of view."""
    m = torch.ones(buf.numel(), dtype=torch.bool, device=buf.device)
    m.as_strided(view.shape, view.stride(), view.storage_offset()).fill_(False)
    return m


def intact(buf, view, what):
    raw = buf.view(I32)[outside(buf, view)]
    assert bool((raw == PAT).all()), f"{what}: {int((raw != PAT).sum())} floats outside the result changed"


def source(t, lead=4):
    """A contiguous input in NaN: lead floats in front, TAIL behind."""
    return strided(1, t.numel(), t.numel(), lead, NAN, t.reshape(1, -1))[1].view(t.shape)


def dest(shape, lead=4, old=None):
    """A contiguous output of `shape` in PAT (holding `old` for an accumulating call) -> (buffer, view of that shape, the same
    as one row: what intact() takes)."""
    n = 1
    for s in shape:
        n *= s
    buf, v = strided(1, n, n, lead, PAT, None if old is None else old.reshape(1, -1))
    return buf, v.view(shape), v


# ------------------------------------------------------------------------------------------------ 1. nchw_to_nhwc, small kernel
# vrnet_nchw_to_nhwc_f32: (C == 3 || C == 4) && HW >= 4096 -> nchw_to_nhwc_small_kernel<C>, one thread per pixel, a grid of
# min(ceil(HW / 256), 4096) x B with a grid-stride loop; anything else -> the 32 x 33 tile kernel.  So of the cases below C = 5
# and HW = 4095 take the tile kernel, the others the small one (from the launcher's source: these ops have no kernel-family
# counter).  C == 4 stores 16 bytes per pixel iff ldd % 4 == 0 && vr_aligned16(dst), else four floats; C == 3 always three.
SMALL_LAYOUTS = {          # C: (ldd, lead) ...
    3: [(3, 0), (3, 4), (7, 0), (7, 4)],          # contiguous; row 3 of the 3 + 4 input-fusion buffer (its radar half at lead 4)
    4: [(4, 0), (8, 4), (8, 5), (7, 0)],          # 16-byte store; the same in a wider row; base off by one float; ldd % 4 fails
    5: [(5, 0), (9, 4), (10, 0)],
}


@functools.lru_cache(maxsize=None)
def planes(B, C, HW):
    x = payload(B, C, HW, seed=B + C)
    return x, x.permute(0, 2, 1).contiguous()


def run_nchw_to_nhwc(hip, B, C, HW, ldd, lead):
    x, ref = planes(B, C, HW)
    buf, out = strided(B * HW, C, ldd, lead, PAT)
    hip.nchw_to_nhwc(source(x), out, ldd, B, C, HW)
    what = f"nchw_to_nhwc B {B} C {C} HW {HW} ldd {ldd} lead {lead}"
    same(out, ref.view(B * HW, C), what)
    intact(buf, out, what)
    return out


@pytest.mark.parametrize("HW", [4095, 4096, 4096 + 37])
@pytest.mark.parametrize("C", [3, 4, 5])
def test_nchw_to_nhwc_at_the_small_kernel_edge(hip, C, HW):
    for ldd, lead in SMALL_LAYOUTS[C]:
        run_nchw_to_nhwc(hip, 2, C, HW, ldd, lead)


def test_nchw_to_nhwc_small_kernel_past_its_grid_cap(hip):
    """ceil(HW / 256) = 4098 > 4096 blocks: the last 257 pixels come from the second pass of the grid-stride loop."""
    run_nchw_to_nhwc(hip, 1, 3, 4096 * 256 + 257, 3, 0)


# ------------------------------------------------------------------------------------------------ 2. the tile kernels
# nchw_to_nhwc_kernel / nhwc_to_nchw_kernel: 32 pixels x 32 channels per workgroup through a 32 x 33 LDS tile.  C and HW of 1
# (one lane live), 31 / 33 (a tail of one on either side of a full tile), 32 (full tiles only), 65 and 97 (full tiles next to a
# tail tile, three and four tiles in a row); 97 = H x W with H != W would be e.g. 1 x 97 -- the kernels only see HW.
TILE_C = [1, 31, 32, 33, 65]
TILE_HW = [1, 31, 32, 33, 97]


def tile_layouts(C):
    return [(C, 0), (C + 4, 4), (C + 5, 0)]          # contiguous; an aligned slice of a wider row; a ragged row stride


@pytest.mark.parametrize("HW", TILE_HW)
@pytest.mark.parametrize("C", TILE_C)
def test_nchw_to_nhwc_tile_kernel(hip, C, HW):
    for ldd, lead in tile_layouts(C):
        run_nchw_to_nhwc(hip, 2, C, HW, ldd, lead)


@pytest.mark.parametrize("HW", TILE_HW)
@pytest.mark.parametrize("C", TILE_C)
def test_nhwc_to_nchw(hip, C, HW):
    B = 2
    ref, x = planes(B, C, HW)          # x: (B, HW, C) with NaNs and infinities; ref: (B, C, HW)
    xa = payload(B, HW, C, seed=9, nan=False)
    old = rnd(B, C, HW, seed=10)
    for lds, lead in tile_layouts(C):
        what = f"nhwc_to_nchw B {B} C {C} HW {HW} lds {lds} lead {lead}"
        src = strided(B * HW, C, lds, lead, NAN, x)[1]
        buf, out, flat = dest((B, C, HW))
        hip.nhwc_to_nchw(src, lds, out, B, C, HW)
        same(out, ref, what)
        intact(buf, flat, what)
        src = strided(B * HW, C, lds, lead, NAN, xa)[1]
        buf, out, flat = dest((B, C, HW), old=old)
        hip.nhwc_to_nchw(src, lds, out, B, C, HW, accumulate=1)
        same(out, old + xa.permute(0, 2, 1), what + ", accumulate")
        intact(buf, flat, what + ", accumulate")


def test_transposes_round_trip(hip):
    B, C, HW = 2, 33, 97
    x, _ = planes(B, C, HW)
    mid = run_nchw_to_nhwc(hip, B, C, HW, C + 4, 4)
    buf, out, flat = dest((B, C, HW))
    hip.nhwc_to_nchw(mid, C + 4, out, B, C, HW)
    same(out, x, "nhwc_to_nchw(nchw_to_nhwc(x))")
    intact(buf, flat, "round trip")


def test_transposes_and_moments_to_float_refuse_empty_and_oversized_shapes(hip):
    """B, C, HW <= 0 would launch an empty grid, B >= 65536 one past gridDim's limit: refused before any launch."""
    B, C, HW = 2, 5, 7
    x = source(rnd(B, C, HW, seed=1))
    buf, out = strided(B * HW, C, C, 4, PAT)
    for b, c, hw in ((0, C, HW), (-1, C, HW), (65536, C, HW), (B, 0, HW), (B, -3, HW), (B, C, 0), (B, C, -7)):
        refused("nchw_to_nhwc", lambda: hip.nchw_to_nhwc(x, out, C, b, c, hw), buf)
        refused("nhwc_to_nchw", lambda: hip.nhwc_to_nchw(x, C, out, b, c, hw), buf)
        refused("nhwc_to_nchw", lambda: hip.nhwc_to_nchw(x, C, out, b, c, hw, accumulate=1), buf)
    refused("nchw_to_nhwc", lambda: hip.nchw_to_nhwc(x, out, C - 1, B, C, HW), buf)
    refused("nhwc_to_nchw", lambda: hip.nhwc_to_nchw(x, C - 1, out, B, C, HW), buf)
    refused("nchw_to_nhwc", lambda: hip.nchw_to_nhwc(x, out, 3, 65536, 3, 4096), buf)          # the small kernel's branch
    mom = torch.ones(4, 2, dtype=torch.float64, device="cuda")
    for n in (0, -1):
        refused("moments_to_float", lambda: hip.moments_to_float(mom, out, n, 1.0), buf)
    hip.moments_to_float(mom, out, 4, 0.5, 1)
    assert out.reshape(-1)[:4].tolist() == [0.5] * 4
    intact(buf, out.reshape(-1)[:4], "moments_to_float")


# ------------------------------------------------------------------------------------------------ 3. copy_channels
# copy_channels_kernel: dst[r * ldd + c * dcs] (+)= src[r * lds + c * scs], one element per thread in a grid-stride loop over
# min(ceil(rows * C / 1024), 8192) workgroups of 256.
def run_copy_channels(hip, rows, C, scs, dcs, lds, ldd, accumulate):
    what = f"copy_channels rows {rows} C {C} scs {scs} dcs {dcs} lds {lds} ldd {ldd} accumulate {accumulate}"
    v = payload(rows, C, seed=3, nan=not accumulate)
    old = rnd(rows, C, seed=4)
    sbuf = torch.full((rows * lds + TAIL,), NAN, device="cuda")
    src = sbuf[:rows * lds].view(rows, lds)
    src[:, 0:C * scs:scs] = v.cuda()          # the interleaved positions the copy skips hold NaN
    dbuf = torch.empty(rows * ldd + TAIL, device="cuda")
    dbuf.view(I32).fill_(PAT)
    dst = dbuf[:rows * ldd].view(rows, ldd)
    if accumulate:
        dst[:, 0:C * dcs:dcs] = old.cuda()
    want = dbuf.cpu()
    want[:rows * ldd].view(rows, ldd)[:, 0:C * dcs:dcs] = old + v if accumulate else v
    hip.copy_channels(src, lds, scs, dst, ldd, dcs, rows, C, accumulate)
    same(dbuf, want, what)          # the whole buffer: the skipped positions, the row padding and the tail keep PAT


@pytest.mark.parametrize("accumulate", [0, 1])
@pytest.mark.parametrize("C", [1, 5, 8])
@pytest.mark.parametrize("scs,dcs", [(1, 1), (1, 2), (2, 1), (3, 2)])
def test_copy_channels_element_strides(hip, scs, dcs, C, accumulate):
    run_copy_channels(hip, 37, C, scs, dcs, C * scs + 3, C * dcs + 5, accumulate)


# rows * C = 8192 * 256 + 1000 elements: 2049 workgroups whose threads each take four or five turns of the loop;
# 8192 * 1024 + 1000: ceil(rows * C / 1024) = 8193 > 8192, the cap itself, where the loop's stride is the capped grid.
@pytest.mark.parametrize("rows", [(8192 * 256 + 1000) // 8, (8192 * 1024 + 1000) // 8], ids=["2M", "8M"])
def test_copy_channels_long_grid_stride_loop(hip, rows):
    run_copy_channels(hip, rows, 8, 1, 1, 9, 12, 1)


# ------------------------------------------------------------------------------------------------ 4. add_, fill_
# add_kernel / fill_kernel: grid-stride loops over min(ceil(n / 1024), 8192) workgroups; the last n exceeds the cap by one
# workgroup and a ragged tail.  n = 0 returns before the launch.
FLAT_N = [1, 255, 1024, 1025, 8192 * 1024 + 1029]


@pytest.mark.parametrize("n", FLAT_N)
def test_add(hip, n):
    a, b = payload(n, seed=1, nan=False), rnd(n, seed=2)
    buf, dst = strided(1, n, n, 4, PAT, a)
    src = source(b)
    hip.add_(dst.view(-1), src)
    same(dst.view(-1), a + b, f"add n {n}")
    intact(buf, dst, f"add n {n}")
    same(src, b, "add: the source")


@pytest.mark.parametrize("n", FLAT_N)
def test_fill(hip, n):
    for value in (-0.0, float("inf"), 0.3):
        buf, dst = strided(1, n, n, 4, PAT)
        hip.fill_(dst.view(-1), value)
        same(dst.view(-1), torch.full((n,), value), f"fill n {n} value {value}")
        intact(buf, dst, f"fill n {n} value {value}")


def test_add_and_fill_of_nothing(hip):
    buf, dst = strided(1, 8, 8, 4, PAT)
    before = buf.view(I32).clone()
    empty = dst.view(-1)[:0]
    hip.fill_(empty, 1.0)
    hip.add_(empty, torch.ones(8, device="cuda")[:0])
    torch.cuda.synchronize()
    assert torch.equal(buf.view(I32), before)


# ------------------------------------------------------------------------------------------------ 5. patch_gather, patch_scatter
# P[b, oy, ox, (ky k + kx) CT + c] = cat(x, pos)[b, oy k + ky, ox k + kx, c], CT = C + CP; pos is (H, W, CP), shared by the
# samples; CP == 0 takes pos = NULL.  Non-square maps and k = 1 .. 4, so that a swapped pair of indices shows in the bits.
PATCH = [(3, 2, 4, 8, 12), (4, 0, 2, 6, 10), (5, 2, 3, 9, 6), (4, 1, 1, 5, 7)]          # C, CP, k, H, W
PB = 3


def patches(t, k):
    """(B, H, W, CT) -> (B, OH, OW, k k CT)."""
    B, H, W, CT = t.shape
    return t.reshape(B, H // k, k, W // k, k, CT).permute(0, 1, 3, 2, 4, 5).reshape(B, H // k, W // k, k * k * CT)


def unpatches(p, k, CT):
    """The inverse: (B, OH, OW, k k CT) -> (B, H, W, CT)."""
    B, OH, OW, _ = p.shape
    return p.reshape(B, OH, OW, k, k, CT).permute(0, 1, 3, 2, 4, 5).reshape(B, OH * k, OW * k, CT)


@pytest.mark.parametrize("pad", [0, 5], ids=["ld=C", "ld=C+5"])
@pytest.mark.parametrize("case", PATCH, ids=str)
def test_patch_gather(hip, case, pad):
    C, CP, k, H, W = case
    x = payload(PB, H, W, C, seed=1)
    pos = payload(H, W, CP, seed=2) if CP else None
    ref = patches(torch.cat([x, pos.expand(PB, H, W, CP)], -1) if CP else x, k)
    xv = strided(PB * H * W, C, C + pad, 0, NAN, x)[1]
    buf, out, flat = dest(tuple(ref.shape))
    hip.patch_gather(xv, C + pad, None if pos is None else source(pos), out, PB, H, W, C, CP, k)
    same(out, ref, f"patch_gather {case}")
    intact(buf, flat, f"patch_gather {case}")


@pytest.mark.parametrize("pad", [0, 5], ids=["ld=C", "ld=C+5"])
@pytest.mark.parametrize("case", PATCH, ids=str)
def test_patch_scatter(hip, case, pad):
    C, CP, k, H, W = case
    CT = C + CP
    dp = payload(PB, H // k, W // k, k * k * CT, seed=3, nan=False)
    dp.view(PB, H // k, W // k, k * k, CT)[..., C:] = NAN          # the pos columns have no adjoint: they must not reach dx
    ref = unpatches(dp, k, CT)[..., :C]
    assert not bool(torch.isnan(ref).any())
    old = rnd(PB, H, W, C, seed=4)
    for accumulate in (0, 1):
        buf, dx = strided(PB * H * W, C, C + pad, 0, PAT, old if accumulate else None)
        hip.patch_scatter(source(dp), dx, C + pad, PB, H, W, C, CP, k, accumulate)
        what = f"patch_scatter {case} accumulate {accumulate}"
        same(dx, (old + ref if accumulate else ref).reshape(-1, C), what)
        intact(buf, dx, what)


def test_patch_ops_refuse_bad_shapes(hip):
    C, CP, k, H, W = 3, 2, 4, 8, 12
    x, pos = torch.zeros(PB, H, W, C, device="cuda"), torch.zeros(H, W, CP, device="cuda")
    out = dest((PB, H // k, W // k, k * k * (C + CP)))[0]
    refused("patch_gather", lambda: hip.patch_gather(x, C, pos, out, PB, H - 1, W, C, CP, k), out)
    refused("patch_gather", lambda: hip.patch_gather(x, C, pos, out, PB, H, W - 2, C, CP, k), out)
    refused("patch_gather", lambda: hip.patch_gather(x, C - 1, pos, out, PB, H, W, C, CP, k), out)
    refused("patch_gather", lambda: hip.patch_gather(x, C, None, out, PB, H, W, C, CP, k), out)
    dp = torch.zeros(PB, H // k, W // k, k * k * (C + CP), device="cuda")
    dx = dest((PB, H, W, C))[0]
    refused("patch_scatter", lambda: hip.patch_scatter(dp, dx, C, PB, H - 1, W, C, CP, k), dx)
    refused("patch_scatter", lambda: hip.patch_scatter(dp, dx, C - 1, PB, H, W, C, CP, k), dx)


# ------------------------------------------------------------------------------------------------ 6. weight_ohwi
# ohwi_kernel: OIHW [n][c][t] -> OHWI [n][t][c] with t = ky kw + kx (dir 0) and the gradient back, (+)= (dir 1): one thread per
# element, ceil(Cout Cin kh kw / 256) workgroups.  1 x 3 and 3 x 1 taps tell kh from kw; (24, 7, 4, 4) is more than one workgroup.
@pytest.mark.parametrize("case", [(3, 5, 1, 3), (7, 6, 3, 1), (24, 7, 4, 4), (1, 1, 1, 1)], ids=str)
def test_weight_ohwi(hip, case):
    Cout, Cin, kh, kw = case
    w = payload(Cout, Cin, kh, kw, seed=1)
    buf, out, flat = dest((Cout, kh, kw, Cin), lead=0)
    hip.weight_ohwi(source(w), out, Cout, Cin, kh, kw, 0)
    same(out, w.permute(0, 2, 3, 1), f"weight_ohwi {case} dir 0")
    intact(buf, flat, f"weight_ohwi {case} dir 0")
    g = payload(Cout, kh, kw, Cin, seed=2, nan=False)
    old = rnd(Cout, Cin, kh, kw, seed=3)
    back = g.permute(0, 3, 1, 2)
    for accumulate, want in ((0, 0.0 + back), (1, old + back)):          # 0 + src: a -0.0 comes out as +0.0, as in the kernel
        buf, out, flat = dest((Cout, Cin, kh, kw), lead=0, old=old if accumulate else None)
        hip.weight_ohwi(source(g), out, Cout, Cin, kh, kw, 1, accumulate)
        same(out, want, f"weight_ohwi {case} dir 1 accumulate {accumulate}")
        intact(buf, flat, f"weight_ohwi {case} dir 1 accumulate {accumulate}")
