"""Mosaic on the host (data.mosaic_params, mosaic_sample, mosaic_boxes, merge_boxes, check_mosaic_table): the recipe of
utils/dataloader.py:251-426 restated.  `merge_boxes` is pinned to the reference's own `merge_bboxes` through
tests/golden/mosaic_merge.npz (tools/make_golden_mosaic.py), the draw to an independent restatement written out here, the
sample to Pillow and to `augment_sample`, which it must reduce to.  No GPU: these functions are the truth the kernels of
csrc/mosaic.hip are held to (tests/test_mosaic.py)."""
import os

import numpy as np
import pytest
from PIL import Image

from asy_vrnet_amd import data

S = (64, 64)
CAP = (96, 112)
SIZES = [(48, 80), (90, 60), (64, 64), (37, 111), (96, 112), (20, 30), (96, 40), (50, 112)]
BOX = np.array([[3, 5, 41, 33, 0], [10, 0, 12, 40, 1], [10, 0, 13, 40, 2], [50, 20, 200, 100, 3], [0, 10, 79, 11, 1],
                [0, 10, 79, 12, 2], [-20, -30, 30, 30, 0], [70, 40, 75, 47, 3]])
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "mosaic_merge.npz")


def test_merge_boxes_equals_the_reference_merge_bboxes():
    z = np.load(GOLDEN)
    assert len(z["cuts"]) == 3
    for k, (cutx, cuty) in enumerate(z["cuts"].tolist()):
        lists = [z[f"boxes_{k}_{i}"] for i in range(4)]
        got, want = data.merge_boxes(lists, cutx, cuty), z[f"merged_{k}"]
        assert got.dtype == want.dtype and got.shape == want.shape and np.array_equal(got, want), k
        assert 0 < len(want) < sum(len(b) for b in lists)              # some were skipped, some kept
    assert data.merge_boxes([np.zeros((0, 5))] * 4, 10, 10).shape == (0, 5)


def reference_draw(rs, sizes, h, w, jitter=.3, hue=.1, sat=.7, val=.4):
    """utils/dataloader.py:299-360 and :404, draw by draw, on a RandomState of its own: (cutx, cuty), four (nw, nh, dx, dy,
    flip), the gains."""
    def rand(a=0, b=1):
        return rs.rand() * (b - a) + a
    min_offset_x = rand(0.3, 0.7)
    min_offset_y = rand(0.3, 0.7)
    tiles = []
    for index, (ih, iw) in enumerate(sizes):
        flip = rand() < .5
        new_ar = iw / ih * rand(1 - jitter, 1 + jitter) / rand(1 - jitter, 1 + jitter)
        scale = rand(.4, 1)
        if new_ar < 1:
            nh = int(scale * h)
            nw = int(nh * new_ar)
        else:
            nw = int(scale * w)
            nh = int(nw / new_ar)
        if index == 0:
            dx = int(w * min_offset_x) - nw
            dy = int(h * min_offset_y) - nh
        elif index == 1:
            dx = int(w * min_offset_x) - nw
            dy = int(h * min_offset_y)
        elif index == 2:
            dx = int(w * min_offset_x)
            dy = int(h * min_offset_y)
        elif index == 3:
            dx = int(w * min_offset_x)
            dy = int(h * min_offset_y) - nh
        tiles.append((nw, nh, dx, dy, int(flip)))
    cut = int(w * min_offset_x), int(h * min_offset_y)
    r = rs.uniform(-1, 1, 3) * [hue, sat, val] + 1
    return cut, tiles, r


def check_mosaic_record(rec, b, sizes, want, input_shape):
    cut, tiles, r = want
    assert (int(rec["cutx"]), int(rec["cuty"]), int(rec["color"])) == cut + (1,), b
    for t, tile in enumerate(rec["tile"]):
        ih, iw = sizes[4 * b + t]
        assert (int(tile["src"]), int(tile["ih"]), int(tile["iw"])) == (4 * b + t, ih, iw), (b, t)
        assert tuple(int(tile[k]) for k in ("nw", "nh", "dx", "dy", "flip")) == tiles[t], (b, t)
        assert tuple(int(tile[k]) for k in ("lb_nw", "lb_nh", "lb_dx", "lb_dy")) == data.letterbox_geometry(iw, ih, input_shape[1], input_shape[0])
    assert np.array_equal(rec["lut"], data.aug_luts(r))


def check_plain_record(rec, b, sizes, a, input_shape):
    """A record that is not mosaicked against the `augment_params` record a of source 4 b."""
    H, W = input_shape
    assert (int(rec["cutx"]), int(rec["cuty"]), int(rec["color"])) == (W, H, int(a["color"])), b
    assert [int(s) for s in rec["tile"]["src"]] == [4 * b, -1, -1, -1]
    tile = rec["tile"][0]
    assert all(int(tile[k]) == int(a[k]) for k in ("ih", "iw", "nw", "nh", "dy", "flip", "lb_nw", "lb_nh", "lb_dx", "lb_dy"))
    assert int(tile["dx"]) == (W - int(a["dx"]) - int(a["nw"]) if int(a["flip"]) else int(a["dx"]))
    assert np.array_equal(rec["lut"], a["lut"])


@pytest.mark.parametrize("input_shape", [S, (40, 63)])
def test_mosaic_params_draws_in_the_reference_order(input_shape):
    H, W = input_shape
    sizes = SIZES * 5                                      # ten output images from one stream
    taps = data.default_mosaic_max_taps(CAP, input_shape, prob=0.5)
    tab = data.mosaic_params(sizes, input_shape, 7, 10, capacity=CAP, max_taps=taps)
    assert tab.dtype == data.MOSAIC_DTYPE and data.MOSAIC_DTYPE.itemsize == 976 and data.mosaic_bytes(tab).shape == (10, 976)
    rs = np.random.RandomState(7)
    flips = 0
    for b in range(10):
        assert rs.rand() < 1.0                             # the mosaic draw itself
        want = reference_draw(rs, sizes[4 * b:4 * b + 4], H, W)
        check_mosaic_record(tab[b], b, sizes, want, input_shape)
        flips += sum(t[4] for t in want[1])
        assert .3 * W - 1 <= want[0][0] <= .7 * W and .3 * H - 1 <= want[0][1] <= .7 * H
    assert 0 < flips < 40
    # prob = 0: one rand(), then the single-image draw of source 4 b with the keywords of plain
    plain = {"scale": (.5, 1.5), "jitter": .2}
    tab0 = data.mosaic_params(sizes, input_shape, 7, 10, prob=0.0, plain=plain, capacity=CAP, max_taps=taps)
    rs = np.random.RandomState(7)
    for b in range(10):
        rs.rand()
        check_plain_record(tab0[b], b, sizes, data.augment_params([sizes[4 * b]], input_shape, rs, **plain)[0], input_shape)
    # prob = .5: the same single rand() decides, image by image
    tab5 = data.mosaic_params(sizes, input_shape, 7, 10, prob=0.5, plain=plain, capacity=CAP, max_taps=taps)
    rs = np.random.RandomState(7)
    kinds = []
    for b in range(10):
        kinds.append(rs.rand() < 0.5)
        if kinds[-1]:
            check_mosaic_record(tab5[b], b, sizes, reference_draw(rs, sizes[4 * b:4 * b + 4], H, W), input_shape)
        else:
            check_plain_record(tab5[b], b, sizes, data.augment_params([sizes[4 * b]], input_shape, rs, **plain)[0], input_shape)
    assert 0 < sum(kinds) < 10
    # a RandomState is taken as it is and advanced
    rs = np.random.RandomState(7)
    first, second = data.mosaic_params(sizes[:8], input_shape, rs, 2), data.mosaic_params(sizes[8:16], input_shape, rs, 2)
    assert first.tobytes()[:976] == tab[0].tobytes() and second[1]["lut"].tobytes() == tab[3]["lut"].tobytes()


def test_the_stream_does_not_depend_on_prob():
    """The first image's mosaic draw consumes the same numbers whatever prob says about the others: image 0 is mosaicked at
    every prob above its rand(), and its record is then the same; color=False leaves the stream where it was, too."""
    sizes = SIZES
    first = np.random.RandomState(11).rand()
    a = data.mosaic_params(sizes, S, 11, 2, prob=1.0)
    b = data.mosaic_params(sizes, S, 11, 2, prob=first + 1e-9)
    assert a[0].tobytes() == b[0].tobytes()
    c = data.mosaic_params(sizes, S, 11, 2, color=False)
    assert all(int(r["color"]) == 0 for r in c) and c["tile"].tobytes() == a["tile"].tobytes()
    # and the generator ends where the draws say: 1 + 2 + 4 * 4 + 3 numbers per mosaicked image
    rs, ref = np.random.RandomState(11), np.random.RandomState(11)
    data.mosaic_params(sizes, S, rs, 2)
    ref.rand(2 * 22)
    assert rs.rand() == ref.rand()


# ---- the sample ---------------------------------------------------------------------------------------------------------
def raw(seed, ih, iw):
    rng = np.random.default_rng(seed)
    return rng.integers(0, 256, (ih, iw, 3), dtype=np.uint8), rng.integers(0, 6, (ih, iw), dtype=np.uint8)


def stored_radar(seed, size, input_shape):
    (ih, iw), (H, W) = size, input_shape
    nw, nh, dx, dy = data.letterbox_geometry(iw, ih, W, H)
    radar = np.zeros((4, H, W), np.float32)
    radar[:, dy:dy + nh, dx:dx + nw] = np.random.default_rng(seed).standard_normal((4, nh, nw)).astype(np.float32)
    return radar


def sources(input_shape, sizes=SIZES[:4]):
    frames, labels = zip(*(raw(k, ih, iw) for k, (ih, iw) in enumerate(sizes)))
    images = [Image.fromarray(f) for f in frames]
    radars = [stored_radar(k, s, input_shape) for k, s in enumerate(sizes)]
    boxes = [BOX, BOX[:3], None, BOX[3:]]
    return frames, labels, images, radars, boxes


def same(got, want):
    return (np.array_equal(np.array(got[0]), np.array(want[0])) and np.array_equal(got[1], want[1])
            and np.array_equal(np.array(got[2]), np.array(want[2])) and got[3].tobytes() == want[3].tobytes())


@pytest.mark.parametrize("input_shape", [S, (40, 63)])
def test_one_unflipped_tile_at_the_full_cut_equals_augment_sample(input_shape):
    H, W = input_shape
    frames, labels, images, radars, boxes = sources(input_shape)
    rows = [(30, 22, 20, 11, False), (2 * W - 3, 2 * H - 1, -(W // 2) - 3, -(H // 2), True), (64, 64, 5, -7, False),
            (W + 20, 30, -15, 4, True)]
    for src, (nw, nh, dx, dy, color) in enumerate(rows):
        gains = (1.07, 1.5, .75)
        rec = data.mosaic_record(input_shape, (W, H), [(src, SIZES[src], nw, nh, dx, dy), None, None, None], color, gains)
        aug = data.aug_record(SIZES[src], input_shape, nw, nh, dx, dy, False, color, gains)
        got = data.mosaic_sample(images, labels, boxes, radars, input_shape, rec)
        want = data.augment_sample(images[src], Image.fromarray(labels[src]), boxes[src] if boxes[src] is not None else np.zeros((0, 5)),
                                   radars[src], input_shape, aug)
        assert same(got, want), src


def test_the_four_corner_cuts_show_exactly_one_tile():
    H, W = S
    frames, labels, images, radars, boxes = sources(S)
    tiles = [(t, SIZES[t], 50 + t, 40 + 2 * t, 3 * t - 4, 5 - 2 * t, t % 2) for t in range(4)]
    for t, cut in enumerate([(W, H), (W, 0), (0, 0), (0, H)]):
        rec = data.mosaic_record(S, cut, tiles)
        alone = data.mosaic_record(S, cut, [tile if k == t else None for k, tile in enumerate(tiles)])
        got, want = data.mosaic_sample(images, labels, boxes, radars, S, rec), data.mosaic_sample(images, labels, boxes, radars, S, alone)
        assert np.array_equal(np.array(got[0]), np.array(want[0])) and np.array_equal(np.array(got[2]), np.array(want[2]))
        assert got[3].tobytes() == want[3].tobytes()
        # ... and it is that tile's own Pillow resize, pasted
        src = images[t].transpose(Image.FLIP_LEFT_RIGHT) if t % 2 else images[t]
        whole = Image.new("RGB", (W, H), (128, 128, 128))
        whole.paste(src.resize((50 + t, 40 + 2 * t), Image.BICUBIC), (3 * t - 4, 5 - 2 * t))
        assert np.array_equal(np.array(got[0]), np.array(whole))


@pytest.mark.parametrize("input_shape", [S, (40, 63)])
def test_a_flipped_tile_equals_an_unflipped_tile_on_the_preflipped_source(input_shape):
    H, W = input_shape
    frames, labels, images, radars, boxes = sources(input_shape)
    cut = (W // 2 - 3, H // 2 + 2)
    tiles = [(0, SIZES[0], 40, 30, cut[0] - 40, cut[1] - 30, 1), (1, SIZES[1], 25, 33, cut[0] - 25, cut[1], 1),
             (2, SIZES[2], 47, 41, cut[0], cut[1], 1), (3, SIZES[3], 60, 20, cut[0], cut[1] - 20, 1)]
    got = data.mosaic_sample(images, labels, boxes, radars, input_shape, data.mosaic_record(input_shape, cut, tiles, True, (.95, 1.3, .8)))
    # the mirrored sources: pixels, labels, boxes (x1, x2 = iw - x2, iw - x1) and the stored radar inside its letterbox window
    pre_images = [im.transpose(Image.FLIP_LEFT_RIGHT) for im in images]
    pre_labels = [l[:, ::-1] for l in labels]
    pre_boxes, pre_radars = [], []
    for (ih, iw), bx, rad in zip(SIZES, boxes, radars):
        if bx is not None:
            bx = bx.copy()
            bx[:, [0, 2]] = iw - bx[:, [2, 0]]
        pre_boxes.append(bx)
        nw, nh, dx, dy = data.letterbox_geometry(iw, ih, W, H)
        flipped = rad.copy()
        flipped[:, dy:dy + nh, dx:dx + nw] = rad[:, dy:dy + nh, dx:dx + nw][..., ::-1]
        pre_radars.append(flipped)
    plain = data.mosaic_record(input_shape, cut, [t[:6] + (0,) for t in tiles], True, (.95, 1.3, .8))
    want = data.mosaic_sample(pre_images, pre_labels, pre_boxes, pre_radars, input_shape, plain)
    assert np.array_equal(np.array(got[0]), np.array(want[0])) and np.array_equal(np.array(got[2]), np.array(want[2]))
    assert np.array_equal(got[1], want[1]) and len(got[1]) > 0
    # the radar gather mirrors the WINDOW index, the pre-flipped map mirrors the letterbox window: floor((2 (nw - 1 - wx) + 1)
    # lb_nw / (2 nw)) is lb_nw - 1 - floor((2 wx + 1) lb_nw / (2 nw)) wherever that quotient is no integer: in all those columns
    # the maps agree bit for bit (a pixel centre that falls exactly between two stored pixels goes left either way)
    for rows, pair in ((slice(0, cut[1]), (0, 3)), (slice(cut[1], H), (1, 2))):          # the top and the bottom half
        exact = np.ones(W, bool)
        for t in pair:
            src, _, nw, _, dx, _, _ = tiles[t]
            lb_nw = data.letterbox_geometry(SIZES[src][1], SIZES[src][0], W, H)[0]
            xs = np.arange(cut[0], W) if t >= 2 else np.arange(0, cut[0])
            exact[xs] = ((2 * (xs - dx) + 1) * lb_nw) % (2 * nw) != 0
        assert exact.mean() > .75 and np.array_equal(got[3][:, rows][..., exact], want[3][:, rows][..., exact]), pair
        assert got[3][:, rows].any()


def test_mosaic_boxes_by_hand():
    # 100 x 100 sources into 50 x 50 windows around the cut (32, 32) of a 64 x 64 canvas: x / 2 + dx, y / 2 + dy
    cut = (32, 32)
    tiles = [(0, (100, 100), 50, 50, -18, -18), (1, (100, 100), 50, 50, -18, 32), (2, (100, 100), 50, 50, 32, 32),
             (3, (100, 100), 50, 50, 32, -18, 1)]
    rec = data.mosaic_record(S, cut, tiles)
    sizes = [(100, 100)] * 4
    boxes = [np.array([[40, 40, 80, 80, 0],            # tile 0: (2, 2, 22, 22): untouched
                       [60, 60, 120, 120, 1],          #         (12, 12, 42, 42) -> clipped to the cut: (12, 12, 32, 32)
                       [98, 60, 130, 90, 2]]),         #         (31, 12, 47, 27) -> x2 = 32: one pixel wide, dropped by the second test
             np.array([[40, 10, 80, 60, 3]]),          # tile 1: (2, 37, 22, 62)
             None,
             np.array([[10, 40, 50, 120, 1]])]         # tile 3, flipped: x 50..90 -> (57, 2, 64, 42) -> y2 = 32
    got = data.mosaic_boxes(boxes, sizes, S, rec)
    assert got.tolist() == [[2, 2, 22, 22, 0], [12, 12, 32, 32, 1], [2, 37, 22, 62, 3], [57, 2, 64, 32, 1]]


def test_check_mosaic_table_names_the_image_and_the_tile():
    taps = data.default_mosaic_max_taps(CAP, S, prob=0.0)
    good = data.mosaic_params(SIZES, S, 5, 2, capacity=CAP, max_taps=taps)

    def bad(b, t, field, value):
        tab = good.copy()
        if t is None:
            tab[b][field] = value
        else:
            tab[b]["tile"][t][field] = value
        return tab
    assert data.check_mosaic_table(good, S, SIZES, CAP, taps) is not None
    for field, value in (("cutx", -1), ("cutx", 65), ("cuty", 65)):
        with pytest.raises(RuntimeError, match="image 1: the cut"):
            data.check_mosaic_table(bad(1, None, field, value), S, SIZES, CAP, taps)
    for field, value, what in (("src", 8, "source 8 of 8"), ("src", -2, "source -2"), ("ih", 47, "the record is for"),
                               ("src", 0, "the record is for"), ("nw", 0, "empty window"), ("nw", 129, "out of range"),
                               ("dx", 65, "out of range"), ("nh", 2, "taps"), ("lb_nw", 63, "letterbox window")):
        with pytest.raises(RuntimeError, match=f"image 1, tile 2: .*{what}"):
            data.check_mosaic_table(bad(1, 2, field, value), S, SIZES, CAP, taps)
    with pytest.raises(RuntimeError, match="image 0, tile 3: .*capacity"):
        data.check_mosaic_table(good, S, SIZES, (96, 110), taps)
    # a tile with src = -1 is no tile: the rest of its head is not looked at
    absent = bad(0, 1, "src", -1)
    absent[0]["tile"][1]["nw"] = -5
    data.check_mosaic_table(absent, S, SIZES, CAP, taps)
    with pytest.raises(RuntimeError, match="MOSAIC_DTYPE"):
        data.check_mosaic_table(np.zeros(2, data.AUG_DTYPE), S, SIZES)
    with pytest.raises(RuntimeError, match="image 1, tile 1: .*capacity"):
        data.mosaic_params(SIZES[:5] + [(97, 30)] + SIZES[6:], S, 0, 2, capacity=CAP)
    # the default tap capacity serves the sampler's draws for sources up to the capacity
    assert taps == data.default_aug_max_taps(CAP, S) >= data.default_mosaic_max_taps(CAP, S)
    data.mosaic_params([CAP, (96, 40), (40, 112), CAP] * 30, S, 11, 30, capacity=CAP, max_taps=data.default_mosaic_max_taps(CAP, S))
