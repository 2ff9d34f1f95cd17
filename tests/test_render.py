"""Device-side result rendering (csrc/render.hip, asy-vrnet_amd/render.py): a numpy restatement of the rules -- Pillow's
ImagingBlend per byte in float32 with one rounding per operation, the palette lookup, the background mask, the pixel counts,
and the `thickness` nested rectangle outlines drawn row after row -- pinned byte for byte on Pillow's own results
(tests/golden/render_small.npz, tools/make_golden_render.py) and, where Pillow is installed, on Pillow itself; then the HIP
path against the goldens and the restatement.  Every comparison is exact: no tolerance appears in this file."""
import os

import numpy as np
import pytest
import torch

from asy_vrnet_amd import render

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "render_small.npz")


# ---- the restatement ------------------------------------------------------------------------------------------------

def blend_restated(a, b, alpha):
    """Blend.c ImagingBlend on uint8 arrays: (uint8)((float)a + alpha * (float)((int)b - (int)a)) with alpha a C float;
    numpy float32 arithmetic rounds after the product and after the sum."""
    d = (b.astype(np.int32) - a.astype(np.int32)).astype(np.float32)
    t = np.float32(alpha) * d
    return (a.astype(np.float32) + t).astype(np.int32).astype(np.uint8)


def blend_contracted(a, b, alpha):
    """The same expression with the product and the sum rounded ONCE (what a fused multiply-add gives): the operands are
    small integers and a 24-bit alpha, so the double-precision value is exact and float32() is its single rounding."""
    exact = a.astype(np.float64) + np.float64(np.float32(alpha)) * (b.astype(np.float64) - a.astype(np.float64))
    return exact.astype(np.float32).astype(np.int32).astype(np.uint8)


def paint_ring(img, left, top, right, bottom, colour):
    """The perimeter of the inclusive rectangle, clipped to the image."""
    ih, iw = img.shape[:2]
    if left > right or top > bottom or right < 0 or bottom < 0:      # empty, or wholly outside (a negative slice end would wrap)
        return
    xs = slice(max(left, 0), min(right, iw - 1) + 1)
    ys = slice(max(top, 0), min(bottom, ih - 1) + 1)
    for y in (top, bottom):
        if 0 <= y < ih:
            img[y, xs] = colour
    for x in (left, right):
        if 0 <= x < iw:
            img[ys, x] = colour


def boxes_restated(img, rows, thickness, box_palette):
    """yolo.py:221-222 in drawing order on one (ih, iw, 3) image, in place."""
    for left, top, right, bottom, c in np.asarray(rows).reshape(-1, 5):
        for i in range(thickness):
            paint_ring(img, left + i, top + i, right - i, bottom - i, box_palette[c])


def render_restated(frames, cmap=None, palette=None, mix_type=0, alpha=0.7, rows=None, offsets=None, box_palette=None,
                    thickness=1):
    """(out (B, ih, iw, 3), counts (B, n) or None)."""
    counts = None
    if cmap is None:
        out = frames.copy()
    else:
        assert mix_type == 2 or cmap.max() < len(palette)
        if mix_type == 1:
            out = palette[cmap]
        elif mix_type == 2:
            out = np.where((cmap != 0)[..., None], frames, 0).astype(np.uint8)
        else:
            out = blend_restated(frames, palette[cmap], alpha)
        if palette is not None:
            counts = np.stack([np.bincount(m.reshape(-1), minlength=len(palette))[:len(palette)] for m in cmap]).astype(np.int64)
    if rows is not None:
        for b in range(len(frames)):
            boxes_restated(out[b], rows[offsets[b]:offsets[b + 1]], thickness, box_palette)
    return out, counts


def class_map(rng, B, ih, iw, n):
    """Blocks of one class plus single-pixel noise: regions (a whole wave agrees) and edges (it does not)."""
    bh, bw = max(ih // 5, 1), max(iw // 7, 1)
    blocks = rng.integers(0, n, (B, (ih + bh - 1) // bh, (iw + bw - 1) // bw), dtype=np.uint8)
    m = np.repeat(np.repeat(blocks, bh, axis=1), bw, axis=2)[:, :ih, :iw].copy()
    noise = rng.random((B, ih, iw)) < 0.05
    m[noise] = rng.integers(0, n, int(noise.sum()), dtype=np.uint8)
    return m


def random_rows(rng, B, ih, iw, n_per_image, n_colours, min_rows=1):
    """Rows reaching outside the image, inverted ones (nothing painted) included; offsets."""
    rows, offsets = [], [0]
    for b in range(B):
        n = n_per_image[b]
        left = rng.integers(-6, iw + 2, n)
        top = rng.integers(-6, ih + 2, n)
        right = left + rng.integers(-2 if min_rows < 1 else 0, iw // 2 + 3, n)
        bottom = top + rng.integers(-2 if min_rows < 1 else min_rows, ih // 2 + 3, n)
        rows.append(np.stack([left, top, right, bottom, rng.integers(0, n_colours, n)], axis=1))
        offsets.append(offsets[-1] + n)
    return np.concatenate(rows).astype(np.int32), np.array(offsets, np.int32)


@pytest.fixture(scope="module")
def golden():
    return np.load(GOLDEN)


def box_cases(g):
    for name in g["box_names"]:
        name = str(name)
        yield name, g[f"box_{name}_rows"], int(g[f"box_{name}_thickness"]), g[f"box_{name}_out"]


GREY = np.repeat(np.arange(256, dtype=np.uint8)[:, None], 3, axis=1)


def blend_table_inputs():
    """The frame whose byte is the row index and the class map whose class is the column index, with the grey palette."""
    a = np.repeat(np.arange(256, dtype=np.uint8)[:, None], 256, axis=1)
    return np.repeat(a[..., None], 3, axis=2), a.T.copy()


# ---- the restatement pinned on Pillow's results ---------------------------------------------------------------------

def test_restated_blend_equals_the_golden_tables_and_they_tell_contraction_apart(golden):
    frame, cmap = blend_table_inputs()
    alphas, sensitive = golden["blend_alphas"], golden["blend_contract_sensitive"]
    assert {0.7, 0.3, 0.5, 0.0, 1.0} <= set(alphas.tolist()) and int(sensitive.sum()) >= 3
    for alpha, sens, table in zip(alphas, sensitive, golden["blend_tables"]):
        got = blend_restated(frame[..., 0], GREY[cmap][..., 0], alpha)
        contracted = int((blend_contracted(frame[..., 0], GREY[cmap][..., 0], alpha) != table).sum())
        print(f"alpha {alpha}: {int((got != table).sum())} bytes differ from Pillow; a contracted evaluation differs on {contracted}")
        assert np.array_equal(got, table)
        if sens:
            assert contracted > 0


def test_restatement_reproduces_the_golden_mix_types_and_counts(golden):
    frame, cmap, pal = golden["mix_frame"][None], golden["mix_class_map"][None], golden["seg_palette_9"]
    assert frame.shape == (1, 37, 53, 3) and (cmap == 0).any() and cmap.max() == 8
    for mix in (0, 1, 2):
        out, counts = render_restated(frame, cmap, pal, mix, 0.7)
        assert np.array_equal(out[0], golden[f"mix{mix}"]), mix
        assert np.array_equal(counts[0], golden["mix_counts"]) and counts.sum() == 37 * 53


def test_restatement_reproduces_the_golden_box_cases(golden):
    names = [n for n, *_ in box_cases(golden)]
    assert len(names) >= 9 and {int(golden[f"box_{n}_thickness"]) for n in names} == {1, 5}
    ih, iw = golden["box_frame"].shape[:2]
    assert any((golden[f"box_{n}_rows"][:, 2] == iw).any() and (golden[f"box_{n}_rows"][:, 3] == ih).any() for n in names)
    assert any((golden[f"box_{n}_rows"][:, :2] < 0).any() for n in names)
    for name, rows, thickness, want in box_cases(golden):
        img = golden["box_frame"].copy()
        boxes_restated(img, rows, thickness, golden["det_palette_4"])
        print(f"{name}: {int((img != want).any(axis=-1).sum())} pixels differ from Pillow")
        assert np.array_equal(img, want), name
        assert not np.array_equal(img, golden["box_frame"])
    a, b = golden["box_overlap_a_then_b_t5_out"], golden["box_overlap_b_then_a_t5_out"]
    assert not np.array_equal(a, b)                                 # the order of two overlapping boxes shows


def test_restatement_equals_live_pillow():
    Image = pytest.importorskip("PIL.Image")
    ImageDraw = pytest.importorskip("PIL.ImageDraw")
    rng = np.random.default_rng(31)
    ih, iw = 61, 83
    frames = rng.integers(0, 256, (2, ih, iw, 3), dtype=np.uint8)
    cmap = class_map(rng, 2, ih, iw, 22)
    pal = render.seg_palette(21)
    for alpha in (0.7, 0.6, 0.123):
        out, _ = render_restated(frames, cmap, pal, 0, alpha)
        for b in range(2):
            want = np.array(Image.blend(Image.fromarray(frames[b]), Image.fromarray(pal[cmap[b]]), alpha))
            assert np.array_equal(out[b], want)
    rows, offsets = random_rows(rng, 2, ih, iw, [60, 60], 4, min_rows=6)   # thickness 3: every drawn ring has >= 2 rows
    bpal = render.det_palette(4)
    out, _ = render_restated(frames, rows=rows, offsets=offsets, box_palette=bpal, thickness=3)
    drawn = 0
    for b in range(2):
        image = Image.fromarray(frames[b].copy())
        d = ImageDraw.Draw(image)
        for left, top, right, bottom, c in rows[offsets[b]:offsets[b + 1]].tolist():
            for i in range(3):
                if left + i <= right - i:                              # Pillow raises ValueError otherwise
                    assert bottom - i > top + i
                    d.rectangle([left + i, top + i, right - i, bottom - i], outline=tuple(int(v) for v in bpal[c]))
                    drawn += 1
        assert np.array_equal(out[b], np.array(image))
    assert drawn > 300


# ---- the host interface: what needs no GPU ---------------------------------------------------------------------------

def test_palettes_equal_the_reference_lists(golden):
    assert np.array_equal(render.seg_palette(9), golden["seg_palette_9"])
    assert np.array_equal(render.seg_palette(21), golden["seg_palette_21"])
    assert np.array_equal(render.seg_palette(30), golden["seg_palette_30"])
    assert np.array_equal(render.det_palette(4), golden["det_palette_4"])
    for p in (render.seg_palette(9), render.seg_palette(30), render.det_palette(4)):
        assert p.dtype == np.uint8 and p.ndim == 2 and p.shape[1] == 3
    assert render.seg_palette(21).shape == (22, 3) and tuple(render.seg_palette(21)[21]) == (128, 64, 12)


def test_box_rows_against_hand_computed_rows():
    results = [
        np.array([[10.7, 20.2, 30.9, 40.5, 0.9, 0.8, 2.0],            # top, left, bottom, right, obj, conf, class
                  [-5.5, -0.5, 1090.0, 1925.3, 0.5, 0.5, 0.0],        # beyond every edge
                  [1079.9, 1919.9, 1080.0, 1920.0, 0.5, 0.5, 2.0]], np.float32),
        None,
        np.zeros((0, 7), np.float32),
        np.array([[0.0, 0.0, 5.0, 5.0, 0.3, 0.3, 3.0]], np.float32),
    ]
    rows, offsets, thickness, counts = render.box_rows(results, (1080, 1920), 4, (512, 512))
    assert rows.dtype == np.int32 and offsets.dtype == np.int32 and counts.dtype == np.int64
    assert rows.tolist() == [[20, 10, 40, 30, 2], [0, 0, 1920, 1080, 0], [1919, 1079, 1920, 1080, 2], [0, 0, 5, 5, 3]]
    assert offsets.tolist() == [0, 3, 3, 3, 4]
    assert thickness == 5                                            # (1920 + 1080) // 512
    assert counts.tolist() == [[1, 0, 2, 0], [0, 0, 0, 0], [0, 0, 0, 0], [0, 0, 0, 1]]
    assert render.box_rows(results, (1080, 1920), ["a", "b", "c", "d"])[2:][0] is None
    assert render.box_rows([None], (30, 40), 4, (512, 512))[2] == 1   # max(70 // 512, 1)
    assert render.box_rows([], (30, 40), 4)[0].shape == (0, 5)


def test_exports():
    import asy_vrnet_amd.hip as hip
    assert "vrnet_render_u8" in hip.EXPORTED and callable(hip.render)
    import asy_vrnet_amd.ops  # noqa: F401
    assert hasattr(torch.ops.vrnet, "render")
    for name in ("seg_palette", "det_palette", "seg_render", "box_rows", "draw_boxes", "render_frame"):
        assert callable(getattr(render, name))


def test_argument_errors():
    img = np.zeros((2, 20, 30, 3), np.uint8)
    cmap = np.zeros((2, 20, 30), np.uint8)
    with pytest.raises(RuntimeError, match="uint8"):
        render.seg_render(img.astype(np.float32), cmap)
    with pytest.raises(RuntimeError, match="uint8"):
        render.seg_render(img, cmap.astype(np.int64))
    with pytest.raises(RuntimeError, match="shape"):
        render.seg_render(np.zeros((2, 20, 30, 4), np.uint8), cmap)
    with pytest.raises(RuntimeError, match="class map"):
        render.seg_render(img, np.zeros((2, 20, 31), np.uint8))
    with pytest.raises(RuntimeError, match="class map"):
        render.seg_render(img, np.zeros((1, 20, 30), np.uint8))
    for alpha in (-0.01, 1.5, float("nan")):
        with pytest.raises(RuntimeError, match="alpha"):
            render.seg_render(img, cmap, alpha=alpha)
    with pytest.raises(RuntimeError, match="mix_type"):
        render.seg_render(img, cmap, mix_type=3)
    with pytest.raises(RuntimeError, match="palette"):
        render.seg_render(img, cmap, palette=np.zeros((257, 3), np.uint8))
    with pytest.raises(RuntimeError, match="palette"):
        render.seg_render(img, cmap, palette=np.zeros((9, 3), np.int32))
    with pytest.raises(RuntimeError, match="palette"):
        render.seg_render(img, cmap, palette=np.zeros((9, 4), np.uint8))
    frames = torch.zeros(2, 20, 30, 3, dtype=torch.uint8)
    with pytest.raises(RuntimeError, match="alias"):
        render.seg_render(frames, torch.from_numpy(cmap), out=frames)
    with pytest.raises(RuntimeError, match="out must be"):
        render.seg_render(frames, torch.from_numpy(cmap), out=torch.zeros(2, 20, 31, 3, dtype=torch.uint8))
    with pytest.raises(RuntimeError, match="count"):
        render.render_frame(img, None, count=True)
    with pytest.raises(RuntimeError, match="result entries"):
        render.draw_boxes(img, [None], (64, 64))
    with pytest.raises(RuntimeError, match="thickness"):
        render.draw_boxes(img, [None, None], (64, 64), thickness=0)
    with pytest.raises(RuntimeError, match="boxes in one image"):
        render.draw_boxes(img, [np.zeros((render.MAX_BOXES + 1, 7), np.float32), None], (64, 64))


def test_fake_kernel_gives_the_output_shapes():
    import asy_vrnet_amd.ops  # noqa: F401
    from torch._subclasses.fake_tensor import FakeTensorMode
    with FakeTensorMode():
        img = torch.empty((3, 40, 70, 3), dtype=torch.uint8)
        out, counts = torch.ops.vrnet.render(img, torch.empty((3, 40, 70), dtype=torch.uint8), torch.empty((9, 3), dtype=torch.uint8),
                                             0, 0.7, torch.empty((5, 5), dtype=torch.int32), torch.empty(4, dtype=torch.int32),
                                             torch.empty((4, 3), dtype=torch.uint8), 2)
    assert tuple(out.shape) == (3, 40, 70, 3) and out.dtype == torch.uint8
    assert tuple(counts.shape) == (3, 9) and counts.dtype == torch.int64


# ---- the HIP path against the goldens and the restatement ------------------------------------------------------------

def cuda(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).cuda()


def check_device(frames, cmap=None, palette=None, mix_type=0, alpha=0.7, rows=None, offsets=None, box_palette=None, thickness=1,
                 want=None):
    """render_frame against `want` (default: the restatement) with array_equal, counts included; the flag word stays 0."""
    if want is None:
        want = render_restated(frames, cmap, palette, mix_type, alpha, rows, offsets, box_palette, thickness)
    src = cuda(frames)
    before = src.clone()
    flag = torch.zeros(1, dtype=torch.int32, device="cuda")
    res = render.render_frame(src, cuda(cmap), None if rows is None else (cuda(rows), cuda(offsets)), None, palette, mix_type, alpha,
                              count=cmap is not None, box_palette=box_palette, thickness=thickness, flag=flag)
    out, counts = res if cmap is not None else (res, None)
    assert torch.equal(src, before), "the frames were modified"
    assert out.is_cuda and out.dtype == torch.uint8 and tuple(out.shape) == frames.shape
    bad = int((out.cpu().numpy() != want[0]).sum())
    print(f"render {frames.shape} mix {mix_type} alpha {alpha} colours {None if palette is None else len(palette)} "
          f"rows {None if rows is None else len(rows)}: {bad} bytes differ")
    assert np.array_equal(out.cpu().numpy(), want[0])
    if cmap is not None and want[1] is not None:
        assert counts.dtype == torch.int64 and np.array_equal(counts.cpu().numpy(), want[1])
        assert (counts.sum(dim=1) == frames.shape[1] * frames.shape[2]).all()
    assert int(flag) == 0
    return out, counts


@pytest.mark.gpu
def test_device_blend_equals_every_golden_table(golden):
    frame, cmap = blend_table_inputs()
    for alpha, table in zip(golden["blend_alphas"], golden["blend_tables"]):
        want = np.repeat(table[None, ..., None], 3, axis=3)
        check_device(frame[None], cmap[None], GREY, 0, float(alpha), want=(want, None))
        check_device(frame[None], cmap[None], GREY, 0, float(alpha))


@pytest.mark.gpu
def test_device_mix_types_equal_the_golden_and_the_restatement(golden):
    frame, cmap, pal = golden["mix_frame"][None], golden["mix_class_map"][None], golden["seg_palette_9"]
    for mix in (0, 1, 2):
        check_device(frame, cmap, pal, mix, 0.7, want=(golden[f"mix{mix}"][None], golden["mix_counts"][None]))
    # a single (ih, iw, 3) frame counts as B = 1; numpy inputs
    out = render.seg_render(frame[0], cmap[0], pal)
    assert tuple(out.shape) == (1, 37, 53, 3) and np.array_equal(out.cpu().numpy()[0], golden["mix0"])


# B = 2 of 37 x 53: 3 922 pixels, % 4 == 2 (the tail path), the second image starts at pixel 1 961, no multiple of 4;
# 1 x 1 and 1 x 7: fewer pixels than one thread's four, plus a tail; 3 of 270 x 480: 127 workgroup-iterations per image and a
# half, so several workgroups add to one image's counts and one iteration straddles each image boundary
@pytest.mark.gpu
@pytest.mark.parametrize("B,ih,iw", [(2, 37, 53), (1, 1, 1), (1, 1, 7), (3, 1, 7), (3, 270, 480)])
@pytest.mark.parametrize("n_colors", [9, 22, 256])
def test_device_equals_the_restatement(B, ih, iw, n_colors):
    rng = np.random.default_rng(B * 1000 + iw + n_colors)
    frames = rng.integers(0, 256, (B, ih, iw, 3), dtype=np.uint8)
    cmap = class_map(rng, B, ih, iw, n_colors)
    pal = render.seg_palette(21)[:n_colors] if n_colors <= 22 else rng.integers(0, 256, (256, 3), dtype=np.uint8)
    for mix in (0, 1, 2):
        out, counts = check_device(frames, cmap, pal, mix, 0.7)
    again = render.seg_render(frames, cmap, pal, 2, count=True)
    assert torch.equal(again[0], out) and torch.equal(again[1], counts)          # identical on two runs
    want = np.stack([np.bincount(m.reshape(-1), minlength=n_colors) for m in cmap])
    assert np.array_equal(counts.cpu().numpy(), want) and int(counts.sum()) == B * ih * iw


@pytest.mark.gpu
def test_device_boxes_equal_every_golden_case(golden):
    frame, bpal = golden["box_frame"][None], golden["det_palette_4"]
    for name, rows, thickness, want in box_cases(golden):
        print(name)
        offsets = np.array([0, len(rows)], np.int32)
        check_device(frame, rows=rows, offsets=offsets, box_palette=bpal, thickness=thickness, want=(want[None], None))


@pytest.mark.gpu
def test_device_random_boxes_offsets_and_in_place():
    rng = np.random.default_rng(41)
    ih, iw = 37, 53
    bpal = render.det_palette(7)
    frames = rng.integers(0, 256, (2, ih, iw, 3), dtype=np.uint8)
    for thickness in (1, 2, 5):
        rows, offsets = random_rows(rng, 2, ih, iw, [100, 100], 7, min_rows=0)      # one-row and inverted rings included
        check_device(frames, rows=rows, offsets=offsets, box_palette=bpal, thickness=thickness)
    # an image without boxes between two with boxes; more pixels than one workgroup-iteration
    frames = rng.integers(0, 256, (3, 45, 80, 3), dtype=np.uint8)
    rows, offsets = random_rows(rng, 3, 45, 80, [7, 0, 9], 7)
    assert offsets.tolist() == [0, 7, 7, 16]
    out, _ = check_device(frames, rows=rows, offsets=offsets, box_palette=bpal, thickness=3)
    assert np.array_equal(out[1].cpu().numpy(), frames[1])
    # in place: out is the frames tensor
    src = cuda(frames)
    got = render.render_frame(src, None, (cuda(rows), cuda(offsets)), box_palette=bpal, thickness=3, out=src)
    assert got is src and torch.equal(src, out)
    # the host list of non_max_suppression gives the same picture as its packed rows
    results = [np.array([[4.5, 3.2, 30.9, 50.1, 0.9, 0.9, 1.0], [-3.0, 20.0, 44.2, 90.0, 0.8, 0.9, 6.0]], np.float32), None,
               np.array([[10.0, 10.0, 20.0, 30.0, 0.9, 0.9, 0.0]], np.float32)]
    r2, o2, t2, _ = render.box_rows(results, (45, 80), 7, (16, 16))
    assert t2 == 7
    want, _ = render_restated(frames, rows=r2, offsets=o2, box_palette=bpal, thickness=t2)
    got = render.draw_boxes(frames, results, (16, 16), palette=7)
    assert np.array_equal(got.cpu().numpy(), want)


@pytest.mark.gpu
def test_render_frame_equals_seg_render_then_draw_boxes_and_leaves_the_surroundings_alone():
    rng = np.random.default_rng(42)
    B, ih, iw = 2, 37, 53
    frames = rng.integers(0, 256, (B, ih, iw, 3), dtype=np.uint8)
    cmap = class_map(rng, B, ih, iw, 9)
    rows, offsets = random_rows(rng, B, ih, iw, [12, 5], 4)
    dev_rows = (cuda(rows), cuda(offsets))
    pal, bpal = render.seg_palette(9), render.det_palette(4)
    want, want_counts = render_restated(frames, cmap, pal, 0, 0.7, rows, offsets, bpal, 2)
    for pad in (512, 513, 514, 515):                 # dword-aligned and the three misaligned starts of `out`
        big = torch.full((pad + B * ih * iw * 3 + 512,), 0xA5, dtype=torch.uint8, device="cuda")
        out = big[pad:pad + B * ih * iw * 3].view(B, ih, iw, 3)
        got, counts = render.render_frame(frames, cmap, dev_rows, palette=pal, box_palette=bpal, thickness=2, count=True, out=out)
        assert got is out and np.array_equal(out.cpu().numpy(), want) and np.array_equal(counts.cpu().numpy(), want_counts)
        assert bool((big[:pad] == 0xA5).all()) and bool((big[pad + B * ih * iw * 3:] == 0xA5).all())
    two = render.seg_render(frames, cmap, pal)
    render.render_frame(two, None, dev_rows, box_palette=bpal, thickness=2, out=two)
    assert np.array_equal(two.cpu().numpy(), want)
    # frames and class map at the matching misalignment take the head path: frames + 3 h and map + h on dword boundaries
    fbuf = torch.zeros(B * ih * iw * 3 + 16, dtype=torch.uint8, device="cuda")
    cbuf = torch.zeros(B * ih * iw + 16, dtype=torch.uint8, device="cuda")
    for h in (1, 2, 3):
        f = fbuf[h:h + B * ih * iw * 3].view(B, ih, iw, 3).copy_(cuda(frames))
        c = cbuf[4 - h:4 - h + B * ih * iw].view(B, ih, iw).copy_(cuda(cmap))
        big = torch.full((h + B * ih * iw * 3 + 64,), 0xA5, dtype=torch.uint8, device="cuda")
        out = big[h:h + B * ih * iw * 3].view(B, ih, iw, 3)
        render.render_frame(f, c, dev_rows, palette=pal, box_palette=bpal, thickness=2, out=out)
        assert np.array_equal(out.cpu().numpy(), want)
        assert bool((big[:h] == 0xA5).all()) and bool((big[h + B * ih * iw * 3:] == 0xA5).all())


@pytest.mark.gpu
def test_data_errors_set_the_flag_and_are_clamped():
    rng = np.random.default_rng(43)
    frames = rng.integers(0, 256, (1, 20, 30, 3), dtype=np.uint8)
    cmap = class_map(rng, 1, 20, 30, 9)
    cmap[0, 3, 4] = 200
    pal = render.seg_palette(9)[:9]
    flag = torch.zeros(1, dtype=torch.int32, device="cuda")
    out, counts = render.seg_render(frames, cmap, pal, 1, count=True, flag=flag)
    assert int(flag) == render.FLAG_CLASS
    clamped = np.minimum(cmap, 8)
    assert np.array_equal(out.cpu().numpy(), pal[clamped])                      # the last colour
    assert int(counts.sum()) == 20 * 30 - 1                                     # and not counted
    flag.zero_()
    rows, offsets = np.array([[2, 2, 12, 12, 9]], np.int32), np.array([0, 1], np.int32)
    got = render.render_frame(frames, None, (cuda(rows), cuda(offsets)), box_palette=4, thickness=1, flag=flag)
    rows[0, 4] = 3
    assert int(flag) == render.FLAG_BOX_COLOUR
    assert np.array_equal(got.cpu().numpy(), render_restated(frames, rows=rows, offsets=offsets, box_palette=render.det_palette(4))[0])


@pytest.mark.gpu
def test_render_in_a_captured_graph():
    rng = np.random.default_rng(44)
    B, ih, iw = 2, 90, 160
    pal, bpal = render.seg_palette(9), render.det_palette(4)
    first = (rng.integers(0, 256, (B, ih, iw, 3), dtype=np.uint8), class_map(rng, B, ih, iw, 9)) + random_rows(rng, B, ih, iw, [20, 20], 4)
    second = (rng.integers(0, 256, (B, ih, iw, 3), dtype=np.uint8), class_map(rng, B, ih, iw, 9)) + random_rows(rng, B, ih, iw, [20, 20], 4)
    src, cm, rows, offsets = (cuda(a) for a in first)
    call = lambda: render.render_frame(src, cm, (rows, offsets), palette=pal, box_palette=bpal, thickness=2, count=True)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        call()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        out, counts = call()
    for t, a in zip((src, cm, rows, offsets), second):
        t.copy_(torch.from_numpy(a))
    g.replay()
    torch.cuda.synchronize()
    want, want_counts = render_restated(second[0], second[1], pal, 0, 0.7, second[2], second[3], bpal, 2)
    assert np.array_equal(out.cpu().numpy(), want) and np.array_equal(counts.cpu().numpy(), want_counts)
    eager, eager_counts = call()
    assert torch.equal(eager, out) and torch.equal(eager_counts, counts)
    assert not np.array_equal(want, render_restated(first[0], first[1], pal, 0, 0.7, first[2], first[3], bpal, 2)[0])


@pytest.mark.gpu
def test_render_does_not_sync_and_op_matches():
    import asy_vrnet_amd.ops  # noqa: F401
    rng = np.random.default_rng(45)
    B, ih, iw = 2, 90, 160
    frames, cmap = rng.integers(0, 256, (B, ih, iw, 3), dtype=np.uint8), class_map(rng, B, ih, iw, 9)
    rows, offsets = random_rows(rng, B, ih, iw, [10, 30], 4)
    src, cm, rg, og = cuda(frames), cuda(cmap), cuda(rows), cuda(offsets)
    pal, bpal = cuda(render.seg_palette(9)), cuda(render.det_palette(4))
    results = [np.array([[4.5, 3.2, 30.9, 50.1, 0.9, 0.9, 1.0]], np.float32), None]
    call = lambda: (render.render_frame(src, cm, (rg, og), palette=pal, box_palette=bpal, thickness=3, count=True),
                    render.draw_boxes(src, results, (64, 64), palette=bpal))
    call()
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        (out, counts), drawn = call()
    finally:
        torch.cuda.set_sync_debug_mode("default")
    oo, oc = torch.ops.vrnet.render(src, cm, pal, 0, 0.7, rg, og, bpal, 3)
    assert torch.equal(oo, out) and torch.equal(oc, counts)
    want, want_counts = render_restated(frames, cmap, render.seg_palette(9), 0, 0.7, rows, offsets, render.det_palette(4), 3)
    assert np.array_equal(out.cpu().numpy(), want) and np.array_equal(counts.cpu().numpy(), want_counts)
    r2, o2, t2, _ = render.box_rows(results, (ih, iw), 4, (64, 64))
    assert np.array_equal(drawn.cpu().numpy(), render_restated(frames, rows=r2, offsets=o2, box_palette=render.det_palette(4), thickness=t2)[0])


@pytest.mark.gpu
def test_end_to_end_nano():
    import asy_vrnet_amd as A
    from asy_vrnet_amd import data, decode
    rng = np.random.default_rng(46)
    B, ih, iw, S = 2, 45, 80, 64
    raw = rng.integers(0, 256, (B, ih, iw, 3), dtype=np.uint8)
    model = A.EfficientVRNet(4, 9, "nano", img_size=S).cuda().eval()
    A.randomize_state_dict(model.state_dict(), seed=2)
    frames = cuda(raw)
    images, _ = data.device_letterbox(frames, (S, S))
    radar = A.synthetic_inputs(B, S, 1, "cuda")[1]
    with torch.no_grad():
        det, seg = model(images, radar)
    results = decode.non_max_suppression(decode.decode_outputs(det, (S, S)), 4, (S, S), (ih, iw), True, conf_thres=0.01, nms_thres=0.5)
    n_boxes = [0 if r is None else len(r) for r in results]
    print("boxes per image", n_boxes)
    assert sum(n_boxes) > 0
    results = [None if r is None else r[:render.MAX_BOXES] for r in results]
    pred = decode.seg_predict(seg, (S, S), (ih, iw))
    out, counts = render.render_frame(frames, pred, results, (S, S), palette=render.seg_palette(9), box_palette=4, count=True)
    rows, offsets, thickness, _ = render.box_rows(results, (ih, iw), 4, (S, S))
    assert thickness == (ih + iw) // S
    want, want_counts = render_restated(raw, pred.cpu().numpy(), render.seg_palette(9), 0, 0.7, rows, offsets, render.det_palette(4),
                                        thickness)
    assert np.array_equal(out.cpu().numpy(), want) and np.array_equal(counts.cpu().numpy(), want_counts)
