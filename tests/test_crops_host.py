"""The host statement of the detection crops (render.crop_boxes_host, render.crop_layout) against live Pillow `image.crop`
and against its own layout rule.  No GPU: the kernels of csrc/crops.hip are compared with these functions in
tests/test_crops.py."""
import numpy as np
import pytest

from asy_vrnet_amd import render

IH, IW = 37, 53


@pytest.fixture(scope="module")
def frame():
    return np.random.default_rng(90).integers(0, 256, (IH, IW, 3), dtype=np.uint8)


def pillow_crop(frame, row):
    from PIL import Image
    return np.array(Image.fromarray(frame).crop([int(v) for v in row[:4]]))


def random_detections(n, seed):
    """(n, 7) float32 rows top, left, bottom, right, obj, conf, class, sticking out of the frame on every side."""
    rng = np.random.default_rng(seed)
    det = np.zeros((n, 7), np.float32)
    top, left = rng.uniform(-12, IH + 4, n), rng.uniform(-12, IW + 4, n)
    det[:, 0], det[:, 1] = top, left
    det[:, 2], det[:, 3] = top + rng.uniform(0.0, 30, n), left + rng.uniform(0.0, 40, n)
    det[:, 4:6] = 0.9
    det[:, 6] = rng.integers(0, 4, n)
    return det


def test_random_box_rows_equal_pillow(frame):
    det = random_detections(400, 91)
    rows = render.box_rows([det], (IH, IW), 4)[0]
    assert (det[:, 0] < 0).any() and (det[:, 1] < 0).any() and (det[:, 2] > IH).any() and (det[:, 3] > IW).any()
    got = render.crop_boxes_host(frame, rows)
    assert len(got) == 400
    nonempty = 0
    for n, row in enumerate(rows):
        l, t, r, b = (int(v) for v in row[:4])
        if r < l or b < t:                            # box_rows can leave an inverted row for a box wholly outside
            assert got[n].shape == (0, 0, 3), n
            continue
        want = pillow_crop(frame, row)
        if want.size == 0:                            # Pillow: (h, 0, 3) or (0, w, 3); here the one empty shape
            assert got[n].shape == (0, 0, 3) and (r == l or b == t), n
            continue
        nonempty += 1
        assert got[n].dtype == np.uint8 and got[n].shape == want.shape and np.array_equal(got[n], want), n
    assert nonempty > 200


def test_special_rows(frame):
    from PIL import Image
    rows = np.array([[7, 9, 8, 10, 0],                # 1 x 1
                     [0, 0, IW, IH, 1],               # the whole frame
                     [5, 6, 5, 20, 0],                # w == 0
                     [5, 6, 20, 6, 0],                # h == 0
                     [20, 6, 5, 30, 2],               # right < left: Pillow raises
                     [5, 30, 20, 6, 2],               # bottom < top
                     [-4, -2, 10, 12, 3],             # hostile: negative left and top
                     [40, 30, IW + 9, IH + 5, 3],     # hostile: beyond the right and lower edge
                     [-100, -100, 1000, 1000, 0],     # hostile on every side: the whole frame
                     [IW + 3, 2, IW + 9, 8, 0],       # wholly outside
                     [-2 ** 31, -2 ** 31, 2 ** 31 - 1, 2 ** 31 - 1, 0]], np.int32)
    got = render.crop_boxes_host(frame, rows)
    assert got[0].shape == (1, 1, 3) and np.array_equal(got[0], pillow_crop(frame, rows[0])) and np.array_equal(got[0][0, 0], frame[9, 7])
    assert np.array_equal(got[1], frame) and np.array_equal(got[1], pillow_crop(frame, rows[1]))
    assert pillow_crop(frame, rows[2]).shape[1] == 0 and pillow_crop(frame, rows[3]).shape[0] == 0        # Pillow's zero sizes
    assert got[2].shape == (0, 0, 3) and got[3].shape == (0, 0, 3)
    with pytest.raises(ValueError):
        Image.fromarray(frame).crop([int(v) for v in rows[4, :4]])
    assert got[4].shape == (0, 0, 3) and got[5].shape == (0, 0, 3)
    assert np.array_equal(got[6], frame[0:12, 0:10])
    assert np.array_equal(got[7], frame[30:IH, 40:IW])
    assert np.array_equal(got[8], frame) and np.array_equal(got[10], frame)
    assert got[9].shape == (0, 0, 3)
    assert all(g.dtype == np.uint8 for g in got)
    with pytest.raises(RuntimeError, match="int32 rows"):
        render.crop_boxes_host(frame, rows.astype(np.int64))
    with pytest.raises(RuntimeError, match="uint8 frame"):
        render.crop_boxes_host(frame.astype(np.float32), rows)


def layout_rows():
    det = [random_detections(0, 1), random_detections(60, 92), random_detections(45, 93)]
    rows, offsets = render.box_rows(det, (IH, IW), 4)[:2]
    return rows, offsets


def check_layout(rows, offsets, sizes, capacity):
    table, (N, used), flag = render.crop_layout(rows, offsets, sizes, capacity)
    assert N == len(rows) == len(table) and table.dtype == render.CROP_RECORD and table.dtype.itemsize == 16
    a = (table["w"].astype(np.int64) * table["h"] + 3) // 4 * 4
    nonempty = a > 0
    dropped = table["offset"] < 0
    assert not (dropped & ~nonempty).any() and (table["offset"][~nonempty] == 0).all()
    assert ((table["w"] == 0) == (table["h"] == 0)).all()
    assert (table["offset"][~dropped] % 4 == 0).all()
    # the offset of a kept row is the sum over ALL earlier rows, and it fits
    want = np.cumsum(a) - a
    kept = nonempty & ~dropped
    assert np.array_equal(table["offset"][kept], want[kept]) and (want[kept] + a[kept] <= capacity).all()
    assert (want[dropped] + a[dropped] > capacity).all()
    # the prefix rule: behind the first dropped row no non-empty row is kept
    if dropped.any():
        first = int(np.flatnonzero(dropped)[0])
        assert not kept[first:].any()
    assert used == int(a[kept].sum()) and flag == (render.FLAG_CROP_ARENA if dropped.any() else 0)
    for b in range(len(offsets) - 1):
        assert (table["image"][offsets[b]:offsets[b + 1]] == b).all()
    return table, used, flag


def test_layout_offsets_prefix_used_and_flag():
    rows, offsets = layout_rows()
    table, used, flag = check_layout(rows, offsets, (IH, IW), 1 << 20)
    assert flag == 0 and (table["w"] > 0).sum() > 50 and (table["w"] == 0).sum() > 0
    need = used
    # a capacity exactly equal to the need drops nothing; one pixel less drops the last non-empty row, and only that one
    exact, used_exact, flag_exact = check_layout(rows, offsets, (IH, IW), need)
    assert flag_exact == 0 and used_exact == need and np.array_equal(exact, table)
    less, used_less, flag_less = check_layout(rows, offsets, (IH, IW), need - 1)
    last = int(np.flatnonzero(table["w"] > 0)[-1])
    assert flag_less == render.FLAG_CROP_ARENA and less["offset"][last] == -1 and (less["offset"] < 0).sum() == 1
    assert (less["w"][last], less["h"][last]) == (table["w"][last], table["h"][last])
    assert used_less == need - (int(table["w"][last]) * int(table["h"][last]) + 3) // 4 * 4
    # a capacity in the middle: a prefix is kept
    mid, used_mid, flag_mid = check_layout(rows, offsets, (IH, IW), need // 2)
    assert flag_mid and 0 < used_mid <= need // 2 and (mid["offset"] < 0).sum() > 1
    # one pixel: everything non-empty is dropped
    none, used_none, _ = check_layout(rows, offsets, (IH, IW), 1)
    assert used_none == 0 and ((none["offset"] < 0) == (table["w"] > 0)).all()


def test_layout_follows_each_image_size():
    rows = np.array([[0, 0, 50, 50, 0], [0, 0, 50, 50, 0], [3, 4, 2, 9, 1]], np.int32)
    offsets = np.array([0, 1, 3], np.int32)
    table, used, flag = check_layout(rows, offsets, np.array([[20, 31], [37, 53]]), 1 << 20)
    assert table.tolist() == [(0, 31, 20, 0), (620, 50, 37, 1), (0, 0, 0, 1)] and used == 620 + 1852 and flag == 0
    # hostile offsets are made monotone and never index outside the rows
    table, (N, used), _ = render.crop_layout(rows, np.array([5, -3, 99], np.int32), (37, 53), 1 << 20)
    assert N == 3 and table["image"].tolist() == [0, 0, 0]
    table, (N, used), _ = render.crop_layout(rows, np.array([0, 2, -7], np.int32), (37, 53), 1 << 20)
    assert N == 0 and len(table) == 0 and used == 0
