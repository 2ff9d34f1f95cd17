"""The training augmentation on the host (data.augment_params, augment_sample, augment_boxes, augment_radar, hsv_jitter): the
recipe of utils/dataloader.py:187-247 restated, held to an independent draw written out here, to the numpy expressions of
the colour tables, to pinned values of the two colour conversions, and to the letterbox functions it must reduce to.  No
GPU: these functions are the truth the kernels of csrc/augment.hip are held to (tests/test_augment.py)."""
import numpy as np
import pytest
from PIL import Image

from asy_vrnet_amd import data

S = (64, 64)
CAP = (96, 112)
SIZES = [(48, 80), (90, 60), (64, 64), (37, 111), (96, 112)]


def reference_draw(rs, ih, iw, h, w, jitter=.3, hue=.1, sat=.7, val=.4):
    """utils/dataloader.py:187-217, draw by draw, on a RandomState of its own."""
    def rand(a=0, b=1):
        return rs.rand() * (b - a) + a
    new_ar = iw / ih * rand(1 - jitter, 1 + jitter) / rand(1 - jitter, 1 + jitter)
    scale = rand(.25, 2)
    if new_ar < 1:
        nh = int(scale * h)
        nw = int(nh * new_ar)
    else:
        nw = int(scale * w)
        nh = int(nw / new_ar)
    dx = int(rand(0, w - nw))
    dy = int(rand(0, h - nh))
    flip = rand() < .5
    r = rs.uniform(-1, 1, 3) * [hue, sat, val] + 1
    return new_ar, (nw, nh, dx, dy, int(flip)), r


def test_augment_params_draws_in_the_reference_order():
    sizes = SIZES * 8                                      # 40 draws from one stream
    tab = data.augment_params(sizes, S, 7, capacity=CAP, max_taps=data.default_aug_max_taps(CAP, S))
    rs = np.random.RandomState(7)
    below, above, negative, flips = 0, 0, 0, 0
    for b, (ih, iw) in enumerate(sizes):
        new_ar, want, r = reference_draw(rs, ih, iw, *S)
        got = tuple(int(tab[b][k]) for k in ("nw", "nh", "dx", "dy", "flip"))
        assert got == want, (b, got, want)
        assert (int(tab[b]["ih"]), int(tab[b]["iw"]), int(tab[b]["color"])) == (ih, iw, 1)
        assert tuple(int(tab[b][k]) for k in ("lb_nw", "lb_nh", "lb_dx", "lb_dy")) == data.letterbox_geometry(iw, ih, S[1], S[0])
        # the three tables: the reference's numpy expressions (:226-229)
        x = np.arange(0, 256, dtype=r.dtype)
        assert np.array_equal(tab[b]["lut"][0], ((x * r[0]) % 180).astype(np.uint8))
        assert np.array_equal(tab[b]["lut"][1], np.clip(x * r[1], 0, 255).astype(np.uint8))
        assert np.array_equal(tab[b]["lut"][2], np.clip(x * r[2], 0, 255).astype(np.uint8))
        below += new_ar < 1
        above += new_ar >= 1
        negative += want[0] > S[1] and want[2] < 0
        flips += want[4]
    assert below > 3 and above > 3 and negative > 0 and 0 < flips < len(sizes)          # both branches, a window wider than the canvas
    # a RandomState is taken as it is and advanced; a seed starts a fresh one
    rs = np.random.RandomState(7)
    first = data.augment_params(sizes[:5], S, rs)
    second = data.augment_params(sizes[5:10], S, rs)
    assert first.tobytes() == tab[:5].tobytes() and second.tobytes() == tab[5:10].tobytes()
    assert data.AUG_DTYPE.itemsize == 816 and data.augment_bytes(tab).shape == (40, 816)
    # color=False leaves the stream where it was
    plain = data.augment_params(sizes, S, 7, color=False)
    assert all(int(p["color"]) == 0 for p in plain)
    assert all(tuple(p)[:7] == tuple(t)[:7] for p, t in zip(plain, tab))


def test_hsv_check_values():
    rgb = np.array([(10, 200, 30), (200, 100, 50), (1, 2, 3), (0, 0, 255), (128, 128, 128)], np.uint8)
    hsv = np.array([(63, 242, 200), (10, 191, 200), (105, 170, 3), (120, 255, 255), (0, 0, 128)], np.uint8)
    back = np.array([(10, 200, 29), (200, 100, 50), (1, 2, 3), (0, 0, 255), (128, 128, 128)], np.uint8)
    assert np.array_equal(data.rgb_to_hsv_u8(rgb), hsv)
    assert np.array_equal(data.hsv_to_rgb_u8(hsv), back)
    assert np.array_equal(data.hsv_jitter(rgb, data.aug_luts((1, 1, 1))), back)          # identity gains: the round trip alone
    # the round trip is NOT the identity: up to 5 levels on random bytes
    x = np.random.default_rng(0).integers(0, 256, (200000, 3), dtype=np.uint8)
    err = np.abs(data.hsv_jitter(x, data.aug_luts((1, 1, 1))).astype(int) - x).max()
    assert 1 <= err <= 5, err
    assert data.rgb_to_hsv_u8(x)[:, 0].max() < 180


def test_grey_stays_grey_under_any_gains():
    grey = np.repeat(np.arange(256, dtype=np.uint8)[:, None], 3, 1)
    rs = np.random.RandomState(1)
    for _ in range(20):
        gains = rs.uniform(-1, 1, 3) * [.1, .7, .4] + 1
        out = data.hsv_jitter(grey, data.aug_luts(gains))
        assert np.array_equal(out[:, 0], out[:, 1]) and np.array_equal(out[:, 1], out[:, 2])
    out = data.hsv_jitter(grey, data.aug_luts((1.3, 5.0, 0.2)))          # gains outside the sampler's range too
    assert np.array_equal(out[:, 0], out[:, 1]) and np.array_equal(out[:, 1], out[:, 2])


BOX = np.array([[3, 5, 41, 33, 0], [10, 0, 12, 40, 1], [10, 0, 13, 40, 2], [50, 20, 200, 100, 3], [0, 10, 79, 11, 1],
                [0, 10, 79, 12, 2], [-20, -30, 30, 30, 0], [70, 40, 75, 47, 3]])


def test_augment_boxes_with_the_letterbox_window_equals_adjust_boxes():
    for ih, iw in SIZES:
        for (h, w) in (S, (40, 63)):
            rec = data.aug_record((ih, iw), (h, w), *data.letterbox_geometry(iw, ih, w, h))
            got, want = data.augment_boxes(BOX, iw, ih, w, h, rec), data.adjust_boxes(BOX, iw, ih, w, h)
            assert got.dtype == want.dtype and np.array_equal(got, want), (ih, iw, h, w)
    assert data.augment_boxes(np.zeros((0, 5)), 80, 48, 64, 64, rec).shape == (0, 5)


def test_augment_boxes_by_hand():
    # a 100 x 100 image into a 50 x 50 window at (10, 20) of a 64 x 64 canvas: x / 2 + 10, y / 2 + 20
    rec = data.aug_record((100, 100), S, 50, 50, 10, 20)
    box = np.array([[10, 10, 31, 41, 2]])
    assert data.augment_boxes(box, 100, 100, 64, 64, rec).tolist() == [[15, 25, 25, 40, 2]]          # 25.5 -> 25, 40.5 -> 40
    flipped = data.aug_record((100, 100), S, 50, 50, 10, 20, flip=True)
    assert data.augment_boxes(box, 100, 100, 64, 64, flipped).tolist() == [[64 - 25, 25, 64 - 15, 40, 2]]
    # a 160 x 160 window at (-40, -50): x * 1.6 - 40, y * 1.6 - 50; one box per canvas edge
    rec = data.aug_record((100, 100), S, 160, 160, -40, -50)
    box = np.array([[10, 40, 40, 60, 0],           # x1 = -24 -> 0; x2 = 24
                    [40, 10, 60, 40, 1],           # y1 = -34 -> 0; y2 = 14
                    [50, 40, 90, 60, 2],           # x2 = 104 -> 64
                    [40, 50, 60, 95, 3]])          # y2 = 102 -> 64
    assert data.augment_boxes(box, 100, 100, 64, 64, rec).tolist() == [
        [0, 14, 24, 46, 0], [24, 0, 56, 14, 1], [40, 14, 64, 46, 2], [24, 30, 56, 64, 3]]
    flipped = data.aug_record((100, 100), S, 160, 160, -40, -50, flip=True)
    assert data.augment_boxes(box, 100, 100, 64, 64, flipped).tolist() == [
        [40, 14, 64, 46, 0], [8, 0, 40, 14, 1], [0, 14, 24, 46, 2], [8, 30, 40, 64, 3]]          # -40 -> 0 AFTER the flip: 64 - 104
    # thinned to exactly 1 px by the clip and dropped, between two kept rows; exactly 2 px is kept (x * 1.6 - 41, x2 -> 64)
    rec = data.aug_record((100, 100), S, 160, 160, -41, -50)
    box = np.array([[50, 40, 90, 60, 0],           # x1 = 39
                    [65, 40, 90, 60, 1],           # x1 = 63: 63 .. 64, dropped
                    [64, 40, 90, 60, 2],           # x1 = 61.4 -> 61
                    [40, 69, 60, 95, 3]])          # y1 = 60.4 -> 60, y2 = 102 -> 64: kept
    assert data.augment_boxes(box, 100, 100, 64, 64, rec).tolist() == [
        [39, 14, 64, 46, 0], [61, 14, 64, 46, 2], [23, 60, 55, 64, 3]]
    rec = data.aug_record((100, 100), S, 160, 160, -40, -50)
    box = np.array([[64, 40, 90, 60, 1], [65, 40, 90, 60, 2]])          # x1 = 62.4 -> 62: exactly 2 px, kept; x1 = 64: empty
    assert data.augment_boxes(box, 100, 100, 64, 64, rec).tolist() == [[62, 14, 64, 46, 1]]


def raw(seed, ih, iw):
    rng = np.random.default_rng(seed)
    return rng.integers(0, 256, (ih, iw, 3), dtype=np.uint8), rng.integers(0, 6, (ih, iw), dtype=np.uint8)


def letterboxed_radar(seed, size, input_shape):
    """A stored radar map: values inside the letterbox window of its frame, 0 outside (nothing is measured there)."""
    (ih, iw), (H, W) = size, input_shape
    nw, nh, dx, dy = data.letterbox_geometry(iw, ih, W, H)
    radar = np.zeros((4, H, W), np.float32)
    radar[:, dy:dy + nh, dx:dx + nw] = np.random.default_rng(seed).standard_normal((4, nh, nw)).astype(np.float32)
    return radar


@pytest.mark.parametrize("input_shape", [S, (40, 63)])
def test_augment_sample_with_the_letterbox_window_equals_letterbox_sample(input_shape):
    H, W = input_shape
    for k, (ih, iw) in enumerate(SIZES):
        frame, label = raw(k, ih, iw)
        radar = letterboxed_radar(k, (ih, iw), input_shape)
        rec = data.aug_record((ih, iw), input_shape, *data.letterbox_geometry(iw, ih, W, H))
        image, box, lab, rad = data.augment_sample(Image.fromarray(frame), Image.fromarray(label), BOX, radar, input_shape, rec)
        want_image, want_box, want_lab = data.letterbox_sample(Image.fromarray(frame), Image.fromarray(label), BOX, input_shape)
        assert image.tobytes() == want_image.tobytes() and lab.tobytes() == want_lab.tobytes() and image.size == (W, H)
        assert np.array_equal(box, want_box)
        assert rad.dtype == radar.dtype and rad.tobytes() == radar.tobytes()          # bit for bit


def test_augment_radar_flip_and_rescale():
    H, W = 40, 63
    radar = np.random.default_rng(3).standard_normal((4, H, W)).astype(np.float32)
    # a frame whose letterbox window is the whole canvas, pasted over the whole canvas and flipped
    rec = data.aug_record((80, 126), (H, W), W, H, 0, 0, flip=True)
    assert (int(rec["lb_nw"]), int(rec["lb_nh"]), int(rec["lb_dx"]), int(rec["lb_dy"])) == (W, H, 0, 0)
    assert np.array_equal(data.augment_radar(radar, (H, W), rec), radar[..., ::-1])
    # twice the size at (-10, -20): canvas (x, y) shows window (x + 10, y + 20), stored pixel ((x + 10) // 2, (y + 20) // 2)
    rec = data.aug_record((80, 126), (H, W), 2 * W, 2 * H, -10, -20)
    got = data.augment_radar(radar, (H, W), rec)
    ys, xs = (np.arange(H) + 20) // 2, (np.arange(W) + 10) // 2
    assert np.array_equal(got, radar[:, ys[:, None], xs[None, :]])
    # a third of the size at (5, 7): window pixel w shows stored pixel 3 w + 1, the rest is 0
    rec = data.aug_record((80, 126), (H, W), 21, 13, 5, 7)
    got = data.augment_radar(radar, (H, W), rec)
    want = np.zeros_like(radar)
    want[:, 7:20, 5:26] = radar[:, ((2 * np.arange(13) + 1) * H // 26)[:, None], ((2 * np.arange(21) + 1) * W // 42)[None, :]]
    assert np.array_equal(got, want) and ((2 * 4 + 1) * W) // 42 == 13


def test_augment_sample_crops_flips_and_colours():
    """A window larger than the canvas at negative offsets: Pillow's own crop of the resized frame is the expectation."""
    frame, label = raw(9, 48, 80)
    radar = letterboxed_radar(9, (48, 80), S)
    rec = data.aug_record((48, 80), S, 120, 100, -30, -20, flip=True, color=True, gains=(1.05, 1.4, 0.8))
    image, box, lab, rad = data.augment_sample(Image.fromarray(frame), Image.fromarray(label), BOX, radar, S, rec)
    crop = np.array(Image.fromarray(frame).resize((120, 100), Image.BICUBIC))[20:84, 30:94][:, ::-1]
    assert np.array_equal(np.array(image), data.hsv_jitter(crop, rec["lut"]))
    assert np.array_equal(np.array(lab), np.array(Image.fromarray(label).resize((120, 100), Image.NEAREST))[20:84, 30:94][:, ::-1])


def test_errors_name_the_image():
    with pytest.raises(RuntimeError, match="image 1.*capacity"):
        data.augment_params([(48, 80), (97, 60)], S, 0, capacity=CAP)
    with pytest.raises(RuntimeError, match="image 0.*empty window"):
        data.augment_params([(2, 111)], S, 0, scale=(.01, .02), capacity=CAP)          # nh = int(nw / new_ar) = 0
    with pytest.raises(RuntimeError, match="image 0.*taps"):
        data.augment_params([(48, 80)], S, 0, scale=(.25, .25), capacity=CAP, max_taps=5)          # 80 -> 16 columns: 21 taps
    with pytest.raises(RuntimeError, match="image 0.*taps"):
        data.check_aug_table(np.stack([data.aug_record((96, 112), S, 3, 40, 0, 0)]), S, CAP, data.default_aug_max_taps(CAP, S))
    with pytest.raises(RuntimeError, match="image 0.*empty window"):
        data.check_aug_table(np.stack([data.aug_record((96, 112), S, 0, 40, 0, 0)]), S, CAP)
    with pytest.raises(RuntimeError, match="image 0.*out of range"):
        data.check_aug_table(np.stack([data.aug_record((96, 112), S, 200, 40, 0, 0)]), S, CAP)
    # the default tap capacity serves the sampler's draws for frames up to the capacity
    taps = data.default_aug_max_taps(CAP, S)
    assert taps == 55
    data.augment_params([CAP, (96, 20), (20, 112)] * 30, S, 11, capacity=CAP, max_taps=taps)


def test_augment_without_from_frames_raises():
    from asy_vrnet_amd.graph import TrainStep

    class Uniform:
        def _uniform(self, key):
            return 0.1
    with pytest.raises(RuntimeError, match="augment needs from_frames"):
        TrainStep(None, None, Uniform(), None, 2, 64, 9, augment=True)
    with pytest.raises(RuntimeError, match="augment needs from_frames"):
        TrainStep(None, None, Uniform(), None, 2, 64, 9, from_bytes=True, augment={"flip": 0.0})
