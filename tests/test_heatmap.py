"""Detection heat maps (csrc/heatmap.hip, render.heatmap*): a float64 numpy restatement of yolo.py:288-351 `detect_heatmap`
-- per level sigmoid(class).max * sigmoid(objectness), OpenCV's INTER_LINEAR resize of the whole level map, times 255
truncated to a byte, the max over the levels, then matplotlib's default normalisation, its colour index and the jet bytes
-- pinned on hand-built cases, on matplotlib's own results (tests/golden/heatmap_jet.npz, tools/make_golden_heatmap.py)
and, where they are installed, on cv2 and matplotlib; then the HIP path against it.

The mask is compared under a near-integer rule.  A float32 numpy evaluation of score * 255 differs from the float64 one by
at most 4.5e-5 for these shapes and logits 2 N(0, 1); NEAR is 20 times that, which leaves room for contracted
multiply-adds.  A pixel may differ from the restatement, by 1, only where the float64 value of score * 255 of some level
lies within NEAR of an integer (the truncation may then fall either way); 0.18-0.22 % of the pixels do, and MAX_NEAR is 5
times that.  Everything after the mask -- min / max, colour index, blend -- is compared exactly."""
import functools
import os

import numpy as np
import pytest
import torch

from asy_vrnet_amd import data, decode, render

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "heatmap_jet.npz")
F32 = np.float32
NEAR = 1e-3              # distance of score * 255 from an integer below which a mask byte may differ by 1
MAX_NEAR = 1e-2          # ... and the largest fraction of a case's pixels that may be such pixels


@pytest.fixture(scope="module")
def golden():
    return np.load(GOLDEN)


# ---- the restatement ------------------------------------------------------------------------------------------------

def linear_coords(src, dst):
    """OpenCV INTER_LINEAR source taps along one axis: scale = src / dst, f = (d + 0.5) * scale - 0.5 in float32,
    s = floor(f), f -= s; s < 0 -> (0, 0); s >= src - 1 -> (src - 1, 0).  Returns (s0, s1, f).  (tests/test_segpost.py)"""
    scale = F32(src) / F32(dst)
    f = (np.arange(dst, dtype=F32) + F32(0.5)) * scale - F32(0.5)
    fl = np.floor(f)
    f = f - fl
    s = fl.astype(np.int64)
    low = s < 0
    s[low], f[low] = 0, 0
    high = s >= src - 1
    s[high], f[high] = src - 1, 0
    assert f.dtype == F32
    return s, np.minimum(s + 1, src - 1), f.astype(np.float64)


def window_coords(src, dst, off, n, canvas):
    """The aligned form along one axis: output index d of dst pixels, through the window [off, off + n) of a canvas of
    `canvas` pixels, into a level of src cells: f = ((off + ((d + 0.5) * n) / dst) * src) / canvas - 0.5 in float64, the same
    floor and clamps, the fraction rounded to float32."""
    d = np.arange(dst, dtype=np.float64)
    f = ((off + ((d + 0.5) * n) / dst) * src) / canvas - 0.5
    fl = np.floor(f)
    f = (f - fl).astype(F32)
    s = fl.astype(np.int64)
    low = s < 0
    s[low], f[low] = 0, 0
    high = s >= src - 1
    s[high], f[high] = src - 1, 0
    return s, np.minimum(s + 1, src - 1), f.astype(np.float64)


def resize_plane(plane, ycoords, xcoords):
    """(h, w) float64 -> (oh, ow): the horizontal taps blended first, then the vertical ones."""
    (y0, y1, fy), (x0, x1, fx) = ycoords, xcoords
    top = plane[y0][:, x0] * (1 - fx) + plane[y0][:, x1] * fx
    bot = plane[y1][:, x0] * (1 - fx) + plane[y1][:, x1] * fx
    return top * (1 - fy)[:, None] + bot * fy[:, None]


def sigmoid64(x):
    return 1.0 / (1.0 + np.exp(-np.asarray(x, np.float64)))


def scores_restated(level):
    """yolo.py:339 on one (B, 5 + nc, h, w) map: (B, h, w) float64."""
    return sigmoid64(level[:, 5:]).max(axis=1) * sigmoid64(level[:, 4])


def mask_restated(levels, image_shape, input_shape=None, window=None):
    """Steps :336-342 for a batch: (mask (B, ih, iw) uint8, near (B, ih, iw) bool: score * 255 of some level lies within NEAR
    of an integer).  window = (dx, dy, nw, nh) selects the aligned form."""
    ih, iw = image_shape
    B = levels[0].shape[0]
    mask = np.zeros((B, ih, iw), np.uint8)
    near = np.zeros((B, ih, iw), bool)
    for level in levels:
        score = scores_restated(np.asarray(level))
        h, w = score.shape[1:]
        if window is None:
            yc, xc = linear_coords(h, ih), linear_coords(w, iw)
        else:
            dx, dy, nw, nh = window
            yc, xc = window_coords(h, ih, dy, nh, input_shape[0]), window_coords(w, iw, dx, nw, input_shape[1])
        for b in range(B):
            v = resize_plane(score[b], yc, xc) * 255.0
            near[b] |= np.abs(v - np.rint(v)) < NEAR
            mask[b] = np.maximum(mask[b], v.astype(np.uint8))
    return mask, near


def colour_index(m, vmin, vmax):
    """matplotlib's Normalize(vmin, vmax) followed by Colormap.__call__ on integers m in [vmin, vmax]: float64, one
    rounding per operation."""
    m = np.asarray(m, np.float64)
    if vmax == vmin:
        return np.zeros(m.shape, np.int64)
    idx = np.trunc(((m - vmin) / (vmax - vmin)) * 256.0).astype(np.int64)
    idx[idx == 256] = 255
    return idx


def blend_restated(a, b, alpha):
    """Blend.c ImagingBlend on uint8 arrays, numpy float32 arithmetic: one rounding per operation (tests/test_render.py)."""
    d = (b.astype(np.int32) - a.astype(np.int32)).astype(np.float32)
    t = np.float32(alpha) * d
    return (a.astype(np.float32) + t).astype(np.int32).astype(np.uint8)


def picture_restated(frames, mask, minmax, jet, alpha, sizes=None):
    """The blend of jet[index(mask)] over the frames, image by image; sizes: the images' own (ih, iw) inside padded slots,
    everything outside them 0."""
    out = np.zeros(frames.shape, np.uint8)
    for b in range(len(frames)):
        ih, iw = frames.shape[1:3] if sizes is None else sizes[b]
        colour = jet[colour_index(mask[b, :ih, :iw], int(minmax[b, 0]), int(minmax[b, 1]))]
        out[b, :ih, :iw] = blend_restated(frames[b, :ih, :iw], colour, alpha)
    return out


def make_levels(seed, B, nc, input_shape, value=None):
    """The three raw maps (B, 5 + nc, H/8, W/8) .. (.., H/32, W/32): logits 2 N(0, 1), or all `value`."""
    rng = np.random.default_rng(seed)
    H, W = input_shape
    shapes = [(B, 5 + nc, H // s, W // s) for s in (8, 16, 32)]
    if value is not None:
        return [np.full(s, value, F32) for s in shapes]
    return [(2.0 * rng.standard_normal(s)).astype(F32) for s in shapes]


def make_frames(seed, B, image_shape):
    return np.random.default_rng(seed + 1000).integers(0, 256, (B,) + tuple(image_shape) + (3,), dtype=np.uint8)


# ---- CPU: the restatement on hand-built cases -----------------------------------------------------------------------

def quiet(levels, keep):
    """All levels but `keep` silenced: logits -30 give a score below 1e-25."""
    return [lv if k == keep else np.full_like(lv, -30.0) for k, lv in enumerate(levels)]


def test_restatement_identity_size():
    levels = quiet(make_levels(1, 2, 3, (64, 64)), 0)
    mask, _ = mask_restated(levels, (8, 8))
    assert np.array_equal(mask, (scores_restated(levels[0]) * 255.0).astype(np.uint8))
    assert mask.max() > 30 and mask.min() < mask.max()


def test_restatement_row_upscale_with_both_clamps():
    s0, s1, f = linear_coords(2, 4)
    assert s0.tolist() == [0, 0, 0, 1] and s1.tolist() == [1, 1, 1, 1] and f.tolist() == [0.0, 0.25, 0.75, 0.0]
    row = resize_plane(np.array([[0.0, 0.8]]), linear_coords(1, 1), (s0, s1, f))
    assert np.allclose(row, [[0.0, 0.2, 0.6, 0.8]], rtol=0, atol=1e-15)
    # the same through the mask: a 1 x 2 level whose scores are 0.25 and 0.75 (objectness +30: sigmoid = 1 in float64 to 1e-13)
    levels = make_levels(0, 1, 1, (32, 64), value=-30.0)
    logit = lambda p: np.log(p / (1 - p))
    levels[2][0, 4] = 30.0
    levels[2][0, 5, 0] = [logit(0.25), logit(0.75)]
    mask, _ = mask_restated(levels, (3, 4))
    want = (np.array([0.25, 0.375, 0.625, 0.75]) * 255.0 - 1e-6).astype(np.uint8)      # 63, 95, 159, 191
    assert want.tolist() == [63, 95, 159, 191]
    assert np.array_equal(mask[0], np.tile(want, (3, 1)))


def test_restatement_one_pixel_wide_level():
    """Input 32 x 64: the coarsest level is 1 x 2, so every output row takes the one source row with weight 1."""
    levels = quiet(make_levels(2, 1, 3, (32, 64)), 2)
    assert levels[2].shape[2:] == (1, 2)
    y0, y1, fy = linear_coords(1, 45)
    assert not y0.any() and not y1.any() and not fy.any()
    mask, _ = mask_restated(levels, (45, 80))
    assert (mask == mask[:, :1]).all()                                   # all rows alike
    s = scores_restated(levels[2])[0, 0]
    x0, x1, fx = linear_coords(2, 80)
    assert np.array_equal(mask[0, 0], ((s[x0] * (1 - fx) + s[x1] * fx) * 255.0).astype(np.uint8))
    assert mask[0, 0, 0] != mask[0, 0, -1]


def test_restatement_against_cv2():
    cv2 = pytest.importorskip("cv2")
    rng = np.random.default_rng(3)
    for (h, w), (oh, ow) in (((8, 8), (37, 53)), ((4, 12), (150, 70)), ((1, 2), (45, 80)), ((8, 12), (8, 12)), ((8, 8), (5, 3))):
        score = rng.random((h, w)).astype(F32)
        want = cv2.resize(score, (ow, oh))
        got = resize_plane(score.astype(np.float64), linear_coords(h, oh), linear_coords(w, ow))
        assert want.dtype == F32 and np.abs(got - want).max() <= 2e-7, ((h, w), (oh, ow))


def test_window_of_the_whole_canvas_is_the_whole_map_rule():
    for src, dst, canvas in ((8, 37, 64), (12, 96, 96), (2, 150, 64), (1, 45, 32)):
        a, b = linear_coords(src, dst), window_coords(src, dst, 0, canvas, canvas)
        pos = lambda c: c[0] + c[2]                                      # continuous where a floor falls to the other side
        assert np.abs(pos(a) - pos(b)).max() <= 1e-5


# ---- CPU: the colour rule, the jet table, the interface -------------------------------------------------------------

def test_jet_lut_equals_the_fixture_and_matplotlib(golden):
    lut = render.jet_lut()
    assert lut.dtype == np.uint8 and lut.shape == (256, 3)
    assert np.array_equal(lut, golden["jet"])
    assert lut[0].tolist() == [0, 0, 127] and lut[255].tolist() == [127, 0, 0]
    matplotlib = pytest.importorskip("matplotlib")
    assert np.array_equal(lut, matplotlib.colormaps["jet"](np.arange(256), bytes=True)[:, :3])


def test_index_rule_equals_matplotlib(golden):
    pairs = [tuple(int(v) for v in p) for p in golden["pairs"]]
    assert len(pairs) >= 40 and {(0, 255), (0, 1), (254, 255), (0, 0), (255, 255)} <= set(pairs)
    for (lo, hi), row in zip(pairs, golden["indices"]):
        got = colour_index(np.arange(lo, hi + 1), lo, hi)
        assert np.array_equal(got, row[lo:hi + 1]), (lo, hi)
        assert got[0] == 0 and (hi == lo or got[-1] == 255)


def test_exports():
    import asy_vrnet_amd.hip as hip
    assert {"vrnet_heatmap_workspace", "vrnet_heatmap_f32", "vrnet_heatmap_ragged_workspace",
            "vrnet_heatmap_ragged_f32"} <= set(hip.EXPORTED)
    assert hip.ABI_VERSION == 11
    for name in ("heatmap_workspace_bytes", "heatmap", "heatmap_ragged_workspace_bytes", "heatmap_ragged"):
        assert callable(getattr(hip, name))
    for name in ("jet_lut", "heatmap_mask", "heatmap", "heatmap_ragged"):
        assert callable(getattr(render, name))
    assert hip.heatmap_workspace_bytes(2, 512, 512) == 2 * 5376 * 4 == hip.heatmap_ragged_workspace_bytes(2, 512, 512)
    import asy_vrnet_amd as A
    from asy_vrnet_amd import infer
    res = infer.FrameResult(1, 2, 3, 4, 5, 6, 7)
    assert (res.rows, res.flag, res.sizes, res.heat_mask, res.heat_picture, res.heat_range) == (1, 7, None, None, None, None)
    model = A.EfficientVRNet(4, 9, "nano", img_size=64).eval()
    with pytest.raises(RuntimeError, match="heat_alpha"):
        A.FramePipeline(model, (40, 56), (64, 64), heatmap=True, heat_alpha=1.5)


def test_argument_errors():
    S = (64, 64)
    lv = [torch.from_numpy(a) for a in make_levels(4, 2, 3, S)]
    frames = torch.zeros(2, 20, 30, 3, dtype=torch.uint8)
    geom = torch.zeros(2, 80, dtype=torch.uint8)
    calls = (lambda o, **kw: render.heatmap(frames, o, kw.pop("input_shape", S), **kw),
             lambda o, **kw: render.heatmap_ragged(frames, o, geom, kw.pop("input_shape", S), **kw))
    for call in calls:
        with pytest.raises(RuntimeError, match="three detection maps"):
            call(lv[:2])
        with pytest.raises(RuntimeError, match="three detection maps"):
            call(lv[0])
        with pytest.raises(RuntimeError, match="channels"):
            call([t[:, :5] for t in lv])
        with pytest.raises(RuntimeError, match="stride 16"):
            call([lv[0], lv[2], lv[2]])
        with pytest.raises(RuntimeError, match="stride 8"):
            call(lv, input_shape=(64, 96))
        with pytest.raises(RuntimeError, match="multiples of 32"):
            call(lv, input_shape=(64, 72))
        with pytest.raises(RuntimeError, match="dtype"):
            call([t.double() for t in lv])
        with pytest.raises(RuntimeError, match="uint8 frames"):
            (render.heatmap if call is calls[0] else lambda f, o, s: render.heatmap_ragged(f, o, geom, s))(frames.float(), lv, S)
        for alpha in (-0.01, 1.5, float("nan")):
            with pytest.raises(RuntimeError, match="alpha"):
                call(lv, alpha=alpha)
        with pytest.raises(RuntimeError, match="cmap"):
            call(lv, cmap=np.zeros((255, 3), np.uint8))
        with pytest.raises(RuntimeError, match="cmap"):
            call(lv, cmap=torch.zeros(256, 3))
        with pytest.raises(RuntimeError, match="alias"):
            call(lv, out=frames)
        with pytest.raises(RuntimeError, match="out must be"):
            call(lv, out=torch.zeros(2, 20, 31, 3, dtype=torch.uint8))
        with pytest.raises(RuntimeError, match="GPU"):                    # valid arguments, but no device: there is no fallback
            call(lv)
    with pytest.raises(RuntimeError, match="frames for outputs"):
        render.heatmap(frames[:1], lv, S)
    with pytest.raises(RuntimeError, match="image_shape"):
        render.heatmap_mask(lv, (0, 30), S)
    with pytest.raises(RuntimeError, match="GPU"):
        render.heatmap_mask(lv, (20, 30), S)


# ---- the HIP path ---------------------------------------------------------------------------------------------------

def cuda(a):
    return torch.from_numpy(np.array(a)).cuda()                          # a copy: the shared references are read-only


# (B, nc, input (H, W), frames (ih, iw)): an odd width (byte stores), a frame smaller than the input, frame == input; the
# 1 x 2 level of the 32 x 64 input only with B = 3 (one of its columns alone is more than MAX_NEAR of a single frame)
CASES = [(1, 1, (64, 64), (37, 53)), (3, 3, (64, 64), (150, 70)), (3, 1, (32, 64), (45, 80)), (1, 3, (64, 96), (64, 96)),
         (3, 3, (64, 96), (37, 53)), (3, 3, (32, 64), (150, 70))]


def case_seed(B, nc, input_shape, image_shape):
    return B * 1000 + nc * 100 + input_shape[1] + image_shape[0]


@functools.lru_cache(maxsize=None)
def reference(B, nc, input_shape, image_shape, aligned):
    """(levels, frames, restated mask, near) of a case, computed once and shared; the arrays are read-only."""
    seed = case_seed(B, nc, input_shape, image_shape)
    levels, frames = make_levels(seed, B, nc, input_shape), make_frames(seed, B, image_shape)
    window = None
    if aligned:
        top, left, nh, nw = decode.seg_window(input_shape, image_shape)
        window = (left, top, nw, nh)
    mask, near = mask_restated(levels, image_shape, input_shape, window)
    for a in levels + [frames, mask, near]:
        a.setflags(write=False)
    return levels, frames, mask, near


def check_mask(got, want, near, what):
    diff = got.astype(np.int64) - want.astype(np.int64)
    wrong = (diff != 0) & ~near
    print(f"heatmap {what}: {int(near.sum())} of {near.size} pixels near an integer, {int((diff != 0).sum())} differ, "
          f"largest difference {int(np.abs(diff).max())}, {int(wrong.sum())} differ outside the near set; mask range "
          f"{int(want.min())}..{int(want.max())}")
    assert not wrong.any()
    assert np.abs(diff).max() <= 1
    assert near.sum() <= MAX_NEAR * near.size


@pytest.mark.parametrize("aligned", [False, True])
@pytest.mark.parametrize("B,nc,input_shape,image_shape", CASES)
def test_reference_cases_are_not_degenerate(B, nc, input_shape, image_shape, aligned):
    """No GPU: the share of near-integer pixels of every case, from the restatement alone, and masks that use the range."""
    _, _, mask, near = reference(B, nc, input_shape, image_shape, aligned)
    assert near.sum() <= MAX_NEAR * near.size
    assert mask.max() - mask.min() > 60


@pytest.mark.gpu
@pytest.mark.parametrize("B,nc,input_shape,image_shape", CASES)
def test_mask_and_minmax_match_restatement(B, nc, input_shape, image_shape):
    levels, frames, want, near = reference(B, nc, input_shape, image_shape, False)
    lv = [cuda(a) for a in levels]
    before = [t.clone() for t in lv]
    picture, mask, minmax = render.heatmap(cuda(frames), lv, input_shape)
    assert all(torch.equal(a, b) for a, b in zip(lv, before)), "the maps were modified"
    assert mask.is_cuda and mask.dtype == torch.uint8 and tuple(mask.shape) == (B,) + image_shape
    assert minmax.dtype == torch.int32 and tuple(minmax.shape) == (B, 2)
    assert picture.dtype == torch.uint8 and tuple(picture.shape) == (B,) + image_shape + (3,)
    got = mask.cpu().numpy()
    check_mask(got, want, near, f"B {B} nc {nc} {input_shape} -> {image_shape}")
    mm = minmax.cpu().numpy()
    assert np.array_equal(mm[:, 0], got.reshape(B, -1).min(axis=1)) and np.array_equal(mm[:, 1], got.reshape(B, -1).max(axis=1))
    assert torch.equal(render.heatmap_mask(lv, image_shape, input_shape), mask)


@pytest.mark.gpu
@pytest.mark.parametrize("alpha", [0.5, 0.3, 0.6, 1.0])
def test_picture_matches_restatement_exactly(golden, alpha):
    jet = golden["jet"]
    for B, nc, input_shape, image_shape in CASES[:5]:
        levels, frames, _, _ = reference(B, nc, input_shape, image_shape, False)
        picture, mask, minmax = render.heatmap(cuda(frames), [cuda(a) for a in levels], input_shape, alpha=alpha)
        want = picture_restated(frames, mask.cpu().numpy(), minmax.cpu().numpy(), jet, alpha)
        got = picture.cpu().numpy()
        print(f"heatmap picture alpha {alpha} {image_shape}: {int((got != want).sum())} bytes differ")
        assert np.array_equal(got, want)
    # constant masks: vmax == vmin, every pixel takes colour 0
    frames = make_frames(7, 2, (37, 53))
    for value, level in ((-30.0, 0), (30.0, 255)):
        lv = [cuda(a) for a in make_levels(0, 2, 3, (64, 64), value=value)]
        picture, mask, minmax = render.heatmap(cuda(frames), lv, (64, 64), alpha=alpha)
        assert (mask == level).all() and (minmax == level).all()
        want = picture_restated(frames, mask.cpu().numpy(), minmax.cpu().numpy(), jet, alpha)
        assert np.array_equal(picture.cpu().numpy(), want)
        assert np.array_equal(want, blend_restated(frames, np.broadcast_to(jet[0], frames.shape), alpha))


@pytest.mark.gpu
def test_custom_cmap_and_out(golden):
    B, nc, input_shape, image_shape = CASES[1]
    levels, frames, _, _ = reference(B, nc, input_shape, image_shape, False)
    cmap = np.random.default_rng(5).integers(0, 256, (256, 3), dtype=np.uint8)
    out = torch.full((B,) + image_shape + (3,), 9, dtype=torch.uint8, device="cuda")
    frames = np.array(frames)
    picture, mask, minmax = render.heatmap(frames, [cuda(a) for a in levels], input_shape, alpha=0.4, cmap=cmap, out=out)
    assert picture is out
    assert np.array_equal(out.cpu().numpy(), picture_restated(frames, mask.cpu().numpy(), minmax.cpu().numpy(), cmap, 0.4))
    again = render.heatmap(frames[0], [cuda(a[:1]) for a in levels], input_shape, alpha=0.4, cmap=torch.from_numpy(cmap))
    assert torch.equal(again[1], mask[:1])                                # a single (ih, iw, 3) frame counts as B = 1


@pytest.mark.gpu
@pytest.mark.parametrize("B,nc,input_shape,image_shape", CASES)
def test_aligned_form_matches_its_restatement(B, nc, input_shape, image_shape):
    levels, frames, want, near = reference(B, nc, input_shape, image_shape, True)
    lv = [cuda(a) for a in levels]
    _, mask, minmax = render.heatmap(cuda(frames), lv, input_shape, letterbox_image=True)
    got = mask.cpu().numpy()
    check_mask(got, want, near, f"aligned, B {B} nc {nc} {input_shape} -> {image_shape}")
    mm = minmax.cpu().numpy()
    assert np.array_equal(mm[:, 0], got.reshape(B, -1).min(axis=1)) and np.array_equal(mm[:, 1], got.reshape(B, -1).max(axis=1))


@pytest.mark.gpu
@pytest.mark.parametrize("B,nc,input_shape,image_shape", CASES[:4])
def test_window_of_the_whole_canvas_agrees_with_the_whole_map_form(B, nc, input_shape, image_shape):
    import asy_vrnet_amd.hip as hip
    levels, _, want, near = reference(B, nc, input_shape, image_shape, False)
    lv = [cuda(a) for a in levels]
    H, W = input_shape
    masks = []
    for window in ((0, 0, 0, 0, 0), (1, 0, 0, W, H)):
        mask = torch.empty((B,) + image_shape, dtype=torch.uint8, device="cuda")
        minmax = torch.empty((B, 2), dtype=torch.int32, device="cuda")
        ws = torch.empty(hip.heatmap_workspace_bytes(B, H, W), dtype=torch.uint8, device="cuda")
        hip.heatmap(lv, H, W, mask, minmax, ws, *window)
        masks.append(mask.cpu().numpy())
    differ = masks[0] != masks[1]
    print(f"whole-canvas window {image_shape}: {int(differ.sum())} pixels differ from the whole-map form, "
          f"{int((differ & ~near).sum())} of them outside the near set")
    assert not (differ & ~near).any()
    check_mask(masks[1], want, near, "whole-canvas window")


RAGGED_S, RAGGED_CAP, RAGGED_SIZES = (64, 64), (64, 96), [(37, 53), (45, 80), (64, 96)]


def padded(images, cap, fill=0):
    out = np.full((len(images),) + tuple(cap) + images[0].shape[2:], fill, np.uint8)
    for b, im in enumerate(images):
        out[b, :im.shape[0], :im.shape[1]] = im
    return out


def geom_tensor(table):
    return data.geometry_bytes(table).cuda()


@pytest.mark.gpu
@pytest.mark.parametrize("window", [True, False])
def test_ragged_equals_the_fixed_call_per_image(window):
    import asy_vrnet_amd.hip as hip
    S, cap, sizes = RAGGED_S, RAGGED_CAP, RAGGED_SIZES
    lv = [cuda(a) for a in make_levels(21, 3, 3, S)]
    images = [make_frames(30 + b, 1, s)[0] for b, s in enumerate(sizes)]
    geom = geom_tensor(data.frame_geometry(sizes, S, True, cap))
    flag = torch.zeros(1, dtype=torch.int32, device="cuda")
    picture, mask, minmax = render.heatmap_ragged(cuda(padded(images, cap)), lv, geom, S, window=window, alpha=0.6, flag=flag)
    assert tuple(picture.shape) == (3,) + cap + (3,) and tuple(mask.shape) == (3,) + cap and tuple(minmax.shape) == (3, 2)
    poisoned = render.heatmap_ragged(cuda(padded(images, cap, 0xA5)), lv, geom, S, window=window, alpha=0.6, flag=flag)
    assert all(torch.equal(a, b) for a, b in zip((picture, mask, minmax), poisoned))
    assert int(flag) == 0
    inside = np.zeros((3,) + cap, bool)
    for b, (ih, iw) in enumerate(sizes):
        one = render.heatmap(images[b], [t[b:b + 1] for t in lv], S, letterbox_image=window, alpha=0.6)
        assert torch.equal(picture[b, :ih, :iw], one[0][0]) and torch.equal(mask[b, :ih, :iw], one[1][0]), b
        assert torch.equal(minmax[b], one[2][0]), b
        inside[b, :ih, :iw] = True
    assert not mask.cpu().numpy()[~inside].any() and not picture.cpu().numpy()[~inside].any()
    assert (minmax[:, 0] < minmax[:, 1]).all()
    # a record that claims more rows than its slot has, and a window that reaches past the canvas: clamped and flagged,
    # the other images as before
    good = data.frame_geometry(sizes, S, True, cap)
    tall, wide, empty = good.copy(), good.copy(), good.copy()
    tall["ih"][1] = cap[0] + 1
    wide["dx"][1] = S[1] - wide["nw"][1] + 5
    empty["iw"][1] = 0
    for table in (tall, wide, empty):
        flag.zero_()
        got = render.heatmap_ragged(cuda(padded(images, cap)), lv, geom_tensor(table), S, window=window, alpha=0.6, flag=flag)
        torch.cuda.synchronize()
        assert int(flag) == hip.FLAG_GEOMETRY
        for b in (0, 2):
            assert all(torch.equal(a[b], w[b]) for a, w in zip(got, (picture, mask, minmax))), b
    assert not got[1][1].any() and not got[0][1].any() and got[2][1].tolist() == [255, 0]      # an image without pixels


@pytest.mark.gpu
@pytest.mark.parametrize("image_shape", [(37, 53), (150, 70)])
def test_workspace_is_all_the_call_writes(image_shape):
    """A workspace of exactly heatmap_workspace_bytes, carved from the front of a larger 0xA5 tensor: the bytes behind it
    stay 0xA5, and the results are those of the public call."""
    import asy_vrnet_amd.hip as hip
    B, nc, S = 3, 3, (64, 96)
    lv = [cuda(a) for a in make_levels(41, B, nc, S)]
    frames = cuda(make_frames(41, B, image_shape))
    need = hip.heatmap_workspace_bytes(B, *S)
    assert need == B * (8 * 12 + 4 * 6 + 2 * 3) * 4
    big = torch.full((need + (1 << 20),), 0xA5, dtype=torch.uint8, device="cuda")
    mask = torch.full((B,) + image_shape, 77, dtype=torch.uint8, device="cuda")
    out = torch.full((B,) + image_shape + (3,), 77, dtype=torch.uint8, device="cuda")
    minmax = torch.full((B, 2), 77, dtype=torch.int32, device="cuda")
    hip.heatmap(lv, S[0], S[1], mask, minmax, big[:need], frames=frames, cmap=cuda(render.jet_lut()), alpha=0.5, out=out)
    touched = int((big[need:] != 0xA5).sum())
    scores = big[:need].view(torch.float32).cpu().numpy().reshape(B, -1)
    print(f"heatmap -> {image_shape}: workspace {need} bytes, {touched} bytes behind it written")
    assert touched == 0
    assert np.isfinite(scores).all() and scores.min() > 0 and scores.max() < 1            # all of it is score planes
    want = render.heatmap(frames, lv, S)
    assert torch.equal(out, want[0]) and torch.equal(mask, want[1]) and torch.equal(minmax, want[2])
    with pytest.raises(RuntimeError, match="workspace"):
        hip.heatmap(lv, S[0], S[1], mask, minmax, big[:need - 4])


@pytest.mark.gpu
def test_heatmap_is_deterministic_capturable_and_does_not_sync():
    B, nc, S, image_shape = 3, 3, (64, 64), (150, 70)
    lv = [cuda(a) for a in make_levels(51, B, nc, S)]
    frames = cuda(make_frames(51, B, image_shape))
    keep = [t.clone() for t in lv + [frames]]
    render.heatmap(frames, lv, S)                                          # the colour table reaches the device once
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        a = render.heatmap(frames, lv, S, letterbox_image=True)
        b = render.heatmap(frames, lv, S, letterbox_image=True)
        m = render.heatmap_mask(lv, image_shape, S, letterbox_image=True)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    assert all(torch.equal(x, y) for x, y in zip(a, b)) and torch.equal(m, a[1])
    assert all(torch.equal(x, y) for x, y in zip(keep, lv + [frames])), "the inputs were modified"
    stream = torch.cuda.Stream()
    stream.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(stream):
        render.heatmap(frames, lv, S, letterbox_image=True)
    torch.cuda.current_stream().wait_stream(stream)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=stream):
        got = render.heatmap(frames, lv, S, letterbox_image=True)
    for t in got:
        t.zero_()
    graph.replay()
    torch.cuda.synchronize()
    assert all(torch.equal(x, y) for x, y in zip(got, a))


# ---- the pipeline ---------------------------------------------------------------------------------------------------
NC, NSEG, PIPE_S, PIPE_F = 4, 9, (64, 64), (40, 56)


@pytest.fixture(scope="module")
def model():
    import asy_vrnet_amd as A
    net = A.EfficientVRNet(NC, NSEG, "nano", img_size=PIPE_S[0]).cuda().eval()
    A.randomize_state_dict(net.state_dict(), seed=4)
    return net


def pipe_inputs(seed, sizes):
    rng = np.random.default_rng(seed)
    frames = [rng.integers(0, 256, tuple(s) + (3,), dtype=np.uint8) for s in sizes]
    radar = (rng.standard_normal((len(sizes), 4) + PIPE_S) * 2.0 + 1.0).astype(np.float32)
    return frames, radar


@pytest.mark.gpu
@pytest.mark.parametrize("graph", [False, True])
def test_pipeline_heat_fields_equal_the_public_call(model, graph):
    import asy_vrnet_amd as A
    frames, radar = pipe_inputs(61, [PIPE_F] * 2)
    frames = np.stack(frames)
    pipe = A.FramePipeline(model, PIPE_F, PIPE_S, batch=2, conf_thres=0.3, graph=graph, heatmap=True, heat_alpha=0.6)
    res = pipe.run(frames, radar)
    images, _ = data.device_letterbox(cuda(frames), PIPE_S)
    with torch.no_grad():
        det, _ = model(images, cuda(radar))
    want = render.heatmap(cuda(frames), det, PIPE_S, letterbox_image=True, alpha=0.6)
    assert torch.equal(res.heat_picture, want[0]) and torch.equal(res.heat_mask, want[1]) and torch.equal(res.heat_range, want[2])
    assert (res.heat_range[:, 0] < res.heat_range[:, 1]).all() and int(res.flag) == 0
    # without the option: the other fields are those of this pipeline, and the heat fields are None
    plain = A.FramePipeline(model, PIPE_F, PIPE_S, batch=2, conf_thres=0.3, graph=graph).run(frames, radar)
    assert plain.heat_mask is None and plain.heat_picture is None and plain.heat_range is None
    for k in ("rows", "kept", "det_counts", "class_map", "seg_counts", "rendered", "flag"):
        assert torch.equal(getattr(plain, k), getattr(res, k)), k


@pytest.mark.gpu
def test_ragged_pipeline_heat_fields_equal_the_public_call(model, tmp_path):
    import asy_vrnet_amd as A
    import asy_vrnet_amd.hip as hip
    cap, sizes = (48, 68), [(40, 56), (48, 68), (23, 41)]
    frames, radar = pipe_inputs(62, sizes)
    pipe = A.FramePipeline(model, cap, PIPE_S, batch=3, conf_thres=0.3, ragged=True, heatmap=True)
    res = pipe.run(frames, radar)
    slots = cuda(padded(frames, cap))
    geom = geom_tensor(data.frame_geometry(sizes, PIPE_S, True, cap))
    images = torch.empty((3, 3) + PIPE_S, device="cuda")
    hip.letterbox_ragged(slots, None, geom, PIPE_S[0], PIPE_S[1], pipe.max_taps, images=images)
    with torch.no_grad():
        det, _ = model(images, cuda(radar))
    want = render.heatmap_ragged(slots, det, geom, PIPE_S, window=True, alpha=0.5)
    assert torch.equal(res.heat_picture, want[0]) and torch.equal(res.heat_mask, want[1]) and torch.equal(res.heat_range, want[2])
    assert int(res.flag) == 0 and res.heat_mask[2, :23, :41].any() and not res.heat_mask[2, 23:].any()
    plain = A.FramePipeline(model, cap, PIPE_S, batch=3, conf_thres=0.3, ragged=True).run(frames, radar)
    assert plain.heat_mask is None and plain.heat_picture is None and plain.heat_range is None
    for k in ("rows", "kept", "det_counts", "class_map", "seg_counts", "rendered", "flag"):
        assert torch.equal(getattr(plain, k), getattr(res, k)), k
    # predict_dir saves <stem>_heat.png beside the rendered picture
    from PIL import Image
    from asy_vrnet_amd import infer
    src, radar_root, dst = tmp_path / "in", tmp_path / "radar", tmp_path / "out"
    src.mkdir()
    radar_root.mkdir()
    names = [f"{1600000000 + b}.{b:05d}.png" for b in range(3)]
    for b, n in enumerate(names):
        Image.fromarray(frames[b]).save(src / n)
        np.savez(radar_root / (data.frame_id(n) + ".npz"), radar[b])
    infer.predict_dir(pipe, str(src), str(radar_root), str(dst))
    for b, n in enumerate(names):
        ih, iw = sizes[b]
        assert np.array_equal(np.array(Image.open(dst / (n[:-4] + "_heat.png"))), want[0][b, :ih, :iw].cpu().numpy()), n
        assert (dst / n).exists()
