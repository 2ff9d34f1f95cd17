"""The host statement of the fixed-size detection chips (render.chip_boxes_host, render.chip_geometry) against the
reference's rule written out here with live Pillow -- the clamp, `crop`, and the two branches of resize_image,
utils/utils.py:19-32 -- and the arithmetic the kernels run (render.chip_resample_host) against Pillow's resize, byte for
byte.  No GPU: the kernels of csrc/chips.hip are compared with these functions in tests/test_chips.py."""
import numpy as np
import pytest

from asy_vrnet_amd import render

IH, IW = 37, 53
SIZES = [(8, 8), (5, 7), (16, 12)]
# tests/test_crops.py's EDGE_ROWS
EDGE_ROWS = np.array([[7, 9, 8, 10, 0],               # 1 x 1
                      [5, 6, 5, 20, 0],               # empty: w == 0
                      [4, 3, 5, 10, 1],               # 1 x 7
                      [10, 2, 12, 5, 1],              # 2 x 3
                      [30, 6, 20, 9, 2],              # inverted
                      [11, 20, 14, 25, 2],            # 3 x 5
                      [0, 0, IW, IH, 3],              # the whole frame
                      [5, 6, 20, 6, 0],               # empty: h == 0
                      [48, 30, 53, 35, 3],            # 5 x 5 in the corner
                      [0, 33, IW, 36, 0],             # 53 x 3: whole rows
                      [-9, -9, 2, 3, 1],              # hostile: 2 x 3 after the clamp
                      [50, 35, 99, 99, 1]], np.int32)  # hostile: 3 x 2 after the clamp


@pytest.fixture(scope="module")
def frame():
    return np.random.default_rng(190).integers(0, 256, (IH, IW, 3), dtype=np.uint8)


@pytest.fixture(scope="module")
def big():
    return np.random.default_rng(191).integers(0, 256, (300, 400, 3), dtype=np.uint8)


def reference_chip(frame, row, size, letterbox):
    """The reference's rule for one row: the clamp of the crops, image.crop, then resize_image(crop, (sw, sh), letterbox)
    written out, with nw, nh >= 1."""
    from PIL import Image
    ih, iw = frame.shape[:2]
    sh, sw = size
    l, t, r, b = max(int(row[0]), 0), max(int(row[1]), 0), min(int(row[2]), iw), min(int(row[3]), ih)
    if r - l <= 0 or b - t <= 0:
        return np.full((sh, sw, 3), 128, np.uint8)
    image = Image.fromarray(frame).crop((l, t, r, b))
    cw, ch = image.size
    w, h = sw, sh
    if letterbox:
        scale = min(w / cw, h / ch)
        nw, nh = max(int(cw * scale), 1), max(int(ch * scale), 1)
        image = image.resize((nw, nh), Image.BICUBIC)
        new_image = Image.new("RGB", (w, h), (128, 128, 128))
        new_image.paste(image, ((w - nw) // 2, (h - nh) // 2))
    else:
        new_image = image.resize((w, h), Image.BICUBIC)
    return np.array(new_image)


@pytest.mark.parametrize("letterbox", [False, True])
@pytest.mark.parametrize("size", SIZES)
def test_edge_rows_equal_the_reference_rule(frame, size, letterbox):
    got = render.chip_boxes_host(frame, EDGE_ROWS, size, letterbox)
    assert len(got) == len(EDGE_ROWS)
    for n, row in enumerate(EDGE_ROWS):
        want = reference_chip(frame, row, size, letterbox)
        assert got[n].dtype == np.uint8 and got[n].shape == size + (3,) and np.array_equal(got[n], want), n
    for n in (1, 4, 7):                               # the empty and the inverted rows: all grey
        assert (got[n] == 128).all()
    if letterbox:                                     # the whole frame keeps its aspect ratio: grey above and below
        nw, nh, dx, dy = render.chip_geometry(IW, IH, size, True)
        assert (nw == size[1] or nh == size[0]) and (got[6][:dy] == 128).all() and (got[6][:, :dx] == 128).all()


def test_crop_then_resize_is_not_resize_with_a_box(frame):
    """The taps stop at the crop's edge: resize(box=...) reads the frame beyond it and gives other bytes."""
    from PIL import Image
    row = np.array([[11, 10, 31, 30, 0]], np.int32)
    got = render.chip_boxes_host(frame, row, (8, 8))[0]
    boxed = np.array(Image.fromarray(frame).resize((8, 8), Image.BICUBIC, box=(11, 10, 31, 30)))
    assert np.array_equal(got, reference_chip(frame, row[0], (8, 8), False)) and not np.array_equal(got, boxed)


def test_big_frame_rows(big):
    rows = np.array([[0, 0, 400, 300, 0], [0, 100, 400, 102, 1], [200, 3, 208, 298, 2], [100, 100, 108, 108, 3]], np.int32)
    for size in ((8, 8), (5, 7)):
        for letterbox in (False, True):
            got = render.chip_boxes_host(big, rows, size, letterbox)
            for n, row in enumerate(rows):
                assert np.array_equal(got[n], reference_chip(big, row, size, letterbox)), (size, letterbox, n)
    # the 400 x 2 strip into 8 x 8 with a letterbox: nh = int(2 * 0.02) = 0 in the reference, one row here
    assert render.chip_geometry(400, 2, (8, 8), True) == (8, 1, 0, 3)
    strip = render.chip_boxes_host(big, rows[1:2], (8, 8), True)[0]
    assert (strip[:3] == 128).all() and (strip[4:] == 128).all() and not (strip[3] == 128).all()
    # an 8 x 8 crop into 8 x 8: both passes are skipped
    assert np.array_equal(render.chip_boxes_host(big, rows[3:], (8, 8))[0], big[100:108, 100:108])


def test_chip_geometry():
    g = render.chip_geometry
    assert g(1000, 3, (64, 64), True) == (64, 1, 0, 31)                    # nh = int(3 * 0.064) = 0 -> 1
    assert g(3, 1000, (64, 64), True) == (1, 64, 31, 0)
    assert g(0, 5, (8, 8), True) == (0, 0, 0, 0) == g(5, 0, (8, 8), False) == g(-3, 5, (8, 8), False)     # empty
    assert g(53, 37, (8, 8), False) == (8, 8, 0, 0) and g(1, 1, (5, 7), False) == (7, 5, 0, 0)
    assert g(53, 37, (8, 8), True) == (8, 5, 0, 1)                         # int(37 * 8 / 53) = 5
    assert g(53, 37, (16, 12), True) == (12, 8, 0, 4)
    assert g(3, 5, (256, 256), True) == (153, 256, 51, 0)
    assert g(7, 7, (1, 1), True) == (1, 1, 0, 0)
    for w, h, size in ((200, 300, (64, 64)), (17, 3, (5, 7)), (1, 1, (16, 12))):                 # resize_image's own integers
        sh, sw = size
        scale = min(sw / w, sh / h)
        nw, nh = int(w * scale), int(h * scale)
        assert nw >= 1 and nh >= 1 and g(w, h, size, True) == (nw, nh, (sw - nw) // 2, (sh - nh) // 2)
    for bad in ((0, 8), (8, 257), (8,), "ab", (8.0, 8), (True, 8)):
        with pytest.raises(RuntimeError, match="size is"):
            g(5, 5, bad, False)


def resample_cases(frame, big):
    """(crop, nh, nw): every non-empty edge row into every size in both modes, the big frame's rows, the largest and the
    smallest chip, and 400 -> 7."""
    cases = []
    for row in EDGE_ROWS:
        crop = render.crop_boxes_host(frame, row[None])[0]
        if crop.size:
            for size in SIZES:
                for letterbox in (False, True):
                    nw, nh = render.chip_geometry(crop.shape[1], crop.shape[0], size, letterbox)[:2]
                    cases.append((crop, nh, nw))
    for crop in (big, big[100:102], big[3:298, 200:208], big[100:108, 100:108]):
        for size in ((8, 8), (5, 7)):
            for letterbox in (False, True):
                nw, nh = render.chip_geometry(crop.shape[1], crop.shape[0], size, letterbox)[:2]
                cases.append((crop, nh, nw))
    cases += [(frame[20:25, 11:14], 256, 256), (frame, 1, 1), (big[:1], 1, 7), (frame[:5, :7], 5, 7), (frame[:5, :9], 5, 7),
              (frame[:9, :7], 5, 7)]
    return cases


def test_chip_resample_host_is_pillow_byte_for_byte(frame, big):
    from PIL import Image
    cases = resample_cases(frame, big)
    seen = set()
    for crop, nh, nw in cases:
        key = (crop.shape, crop.tobytes()[:64], nh, nw)
        if key in seen:
            continue
        seen.add(key)
        want = np.array(Image.fromarray(np.ascontiguousarray(crop)).resize((nw, nh), Image.BICUBIC))
        got = render.chip_resample_host(crop, nh, nw)
        assert got.dtype == np.uint8 and got.shape == want.shape and np.array_equal(got, want), (crop.shape, nh, nw)
    assert len(seen) >= 30
    shapes = {c.shape[:2] for c, _, _ in cases}
    assert {(1, 1), (7, 1), (3, 2), (300, 400), (2, 400), (295, 8)} <= shapes
    # 400 -> 5 columns: scale 80, 321 taps an output index; 3 -> 256: an upscale of 85
    assert max(n for _, n, _, _ in render._chip_axis(400, 5)) > 300 and max(n for _, n, _, _ in render._chip_axis(3, 256)) <= 5


def test_an_unchanged_axis_is_the_identity(frame):
    """in == out: the weights are exactly (0, 1, 0, 0) in 22 bits, so the pass Pillow skips may run."""
    for xmin, n, ww, k in render._chip_axis(9, 9):
        assert ww == 1.0 and int(k.sum()) == 1 << 22 and sorted(k.tolist())[:-1] == [0] * (n - 1)
    assert np.array_equal(render.chip_resample_host(frame, IH, IW), frame)


def test_argument_checks(frame):
    with pytest.raises(RuntimeError, match="int32 rows"):
        render.chip_boxes_host(frame, EDGE_ROWS.astype(np.int64), (8, 8))
    with pytest.raises(RuntimeError, match="uint8 frame"):
        render.chip_boxes_host(frame.astype(np.float32), EDGE_ROWS, (8, 8))
    with pytest.raises(RuntimeError, match="size is"):
        render.chip_boxes_host(frame, EDGE_ROWS, (0, 8))
    with pytest.raises(RuntimeError, match="non-empty uint8 crop"):
        render.chip_resample_host(frame[:0], 4, 4)
    with pytest.raises(RuntimeError, match="at least 1 x 1"):
        render.chip_resample_host(frame, 0, 4)


def test_chip_table_follows_each_image_size():
    rows = np.array([[0, 0, 50, 50, 0], [0, 0, 50, 50, 0], [3, 4, 2, 9, 1]], np.int32)
    offsets = np.array([0, 1, 3], np.int32)
    table, N = render.chip_table(rows, offsets, np.array([[20, 31], [37, 53]]), (8, 8), True)
    assert N == 3 and table.dtype == render.CHIP_RECORD and table.dtype.itemsize == 32
    assert table.tolist() == [(0, 31, 20, 8, 5, 0, 1, 1), (1, 50, 37, 8, 5, 0, 1, 1), (1, 0, 0, 0, 0, 0, 0, 2)]
    table, N = render.chip_table(rows, np.array([5, -3, 99], np.int32), (37, 53), (5, 7))
    assert N == 3 and table["image"].tolist() == [0, 0, 0] and table["nw"].tolist() == [7, 7, 0]
    assert render.chip_table(rows, np.array([0, 2, -7], np.int32), (37, 53), (5, 7))[1] == 0
