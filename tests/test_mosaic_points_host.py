"""Radar points under Mosaic, the host statement: `data.mosaic_radar_map` against `data.radar_map` (the pinned rule it is defined
through) composed per tile by this file's own masks, the footprint at the cut, and the packing of the source table.  No GPU.
Every comparison is bit for bit, as uint32."""
import numpy as np
import pytest
import torch

from asy_vrnet_amd import data
from tests import mosaic_points_cases as C

H, W = C.CANVAS
IDENTITY = np.array([[1, 0, 0, 0], [0, 1, 0, 0], [0, 0, 1, 0]], np.float32)      # z = 1: (x, y) are the continuous pixel coordinates


def composed(points, P, rec, radius, min_depth=0.1):
    """The rule, written out with boolean masks: per tile `radar_map` under the (shifted when flipped) window, kept where the
    pixel belongs to the tile's quadrant."""
    x, y = np.arange(W)[None, :], np.arange(H)[:, None]
    cutx, cuty = int(rec["cutx"]), int(rec["cuty"])
    quadrant = [(x < cutx) & (y < cuty), (x < cutx) & (y >= cuty), (x >= cutx) & (y >= cuty), (x >= cutx) & (y < cuty)]
    out = np.zeros((4, H, W), np.uint32)
    for t, tile in enumerate(rec["tile"]):
        src = int(tile["src"])
        if src < 0:
            continue
        nw, nh, dx, dy, flip = (int(tile[k]) for k in ("nw", "nh", "dx", "dy", "flip"))
        pts = points[src] if points[src] is not None else np.zeros((0, 7), np.float32)
        m = data.radar_map(pts, P[src], (int(tile["ih"]), int(tile["iw"])), (H, W), (nw, nh, W - dx - nw if flip else dx, dy), bool(flip),
                           radius, min_depth)
        out = np.where(quadrant[t][None], C.bits(m), out)
    return out


def one_tile(size, nw, nh, dx, dy, flip):
    """A non-mosaicked record: the cut at (W, H), tile 0 alone."""
    return data.mosaic_record((H, W), (W, H), [(0, size, nw, nh, dx, dy, flip), None, None, None])


@pytest.mark.parametrize("flip", [0, 1])
@pytest.mark.parametrize("radius", [0, 2])
@pytest.mark.parametrize("window", [(40, 24, 7, 9), (70, 50, -3, -5), (30, 60, 40, -11)])
def test_a_non_mosaicked_record_is_radar_map_under_tile_0s_window(flip, radius, window):
    nw, nh, dx, dy = window
    pts = C.point_sets(3)[:1]
    P = C.calib()[0]
    got = data.mosaic_radar_map(pts, P, C.SIZES[:1], (H, W), one_tile(C.SIZES[0], nw, nh, dx, dy, flip), radius)
    want = data.radar_map(pts[0], P, C.SIZES[0], (H, W), (nw, nh, W - dx - nw if flip else dx, dy), bool(flip), radius)
    assert got.dtype == np.float32 and got.shape == (4, H, W)
    assert np.array_equal(C.bits(got), C.bits(want))
    assert C.nonzero_pixels(got, (0, W, 0, H)) >= 20


@pytest.mark.parametrize("radius", [0, 2])
def test_a_flipped_tile_mirrors_the_source_inside_the_window_not_the_canvas(radius):
    """With the window inside the canvas the flipped tile is the unflipped one mirrored about the WINDOW's centre: window
    column wx goes to nw - 1 - wx and the window stays at [dx, dx + nw - 1]."""
    nw, nh, dx, dy = 33, 21, 6, 8                 # not centred: a mirror of the canvas would move it to [17, 49]
    pts = C.point_sets(4)[:1]
    P = C.calib()[0]
    plain = data.mosaic_radar_map(pts, P, C.SIZES[:1], (H, W), one_tile(C.SIZES[0], nw, nh, dx, dy, 0), radius)
    flipped = data.mosaic_radar_map(pts, P, C.SIZES[:1], (H, W), one_tile(C.SIZES[0], nw, nh, dx, dy, 1), radius)
    want = np.zeros_like(plain)
    want[:, :, dx:dx + nw] = plain[:, :, dx:dx + nw][:, :, ::-1]
    assert np.array_equal(C.bits(flipped), C.bits(want))
    assert not C.bits(flipped)[:, :, dx + nw:].any() and not C.bits(flipped)[:, :, :dx].any()
    assert C.nonzero_pixels(flipped, (dx, dx + nw, dy, dy + nh)) >= 20


@pytest.mark.parametrize("name", C.NAMES)
@pytest.mark.parametrize("radius", [0, 1, 3])
def test_every_quadrant_is_the_cut_of_its_tiles_radar_map(name, radius):
    """interior cuts; cut (0, 0), where only tile 2 shows; cut (W, H); tiles with src = -1; windows larger than the canvas at
    negative offsets (C.tables).  A quadrant that shows enough of its window to expect 50 of the source's 300 points holds at
    least 20 non-zero pixels (19 of the 26 present tiles; the others show slivers, or a sixteenth of a window)."""
    pts, P = C.point_sets(7), C.calib()
    for rec in C.tables()[name]:
        got = data.mosaic_radar_map(pts, P, C.SIZES, (H, W), rec, radius)
        assert np.array_equal(C.bits(got), composed(pts, P, rec, radius))
        covered = np.zeros((H, W), bool)
        for t in range(4):
            box = C.shown(rec, t)
            if box is None:
                continue
            covered[box[2]:box[3], box[0]:box[1]] = True
            if C.expected_points(rec, t) >= C.MIN_EXPECTED:
                assert C.nonzero_pixels(got, box) >= 20, (name, t)
        assert not C.bits(got)[:, ~covered].any()            # nothing outside what the tiles show


def test_counts_zero_and_one_and_absent_point_sets():
    counts = [C.MAX_POINTS, 0, 1, C.MAX_POINTS, 0, 1, C.MAX_POINTS, C.MAX_POINTS]
    pts, P = C.point_sets(8, counts), C.calib()
    assert pts[1] is None and len(pts[2]) == 1
    empty = list(pts)
    empty[4] = np.zeros((0, 7), np.float32)
    for rec in C.tables()["interior"]:
        got = data.mosaic_radar_map(pts, P, C.SIZES, (H, W), rec, 1)
        assert np.array_equal(C.bits(got), composed(pts, P, rec, 1))
        assert np.array_equal(C.bits(got), C.bits(data.mosaic_radar_map(empty, P, C.SIZES, (H, W), rec, 1)))
        for t in range(4):
            if counts[int(rec["tile"][t]["src"])] == 0:
                assert C.nonzero_pixels(got, C.shown(rec, t)) == 0


def crossing_record(cutx, cuty):
    """Tile 0: a 30 x 20 source shown 1:1 at (0, 0), so its window crosses a cut at cutx < 30; tile 3: another source, right of it."""
    return data.mosaic_record((H, W), (cutx, cuty), [(0, (20, 30), 30, 20, 0, 0, 0), None, None, (1, (20, 30), 30, 20, cutx, 0, 0)])


def at_pixel(ix, iy, value):
    """One point that lands on window pixel (ix, iy) of a 1:1 window under IDENTITY."""
    return np.array([[ix + 0.5, iy + 0.5, 1.0, value, value + 1, value + 2, value + 3]], np.float32)


def test_the_footprint_stops_at_the_cut_and_reaches_back_over_it():
    cutx, cuty = 12, 18
    rec = crossing_record(cutx, cuty)
    sizes = [(20, 30), (20, 30)]
    # centred on the last column of its quadrant: nothing at x >= cutx, although the window goes on to column 29
    got = data.mosaic_radar_map([at_pixel(cutx - 1, 5, 1.0), None], IDENTITY, sizes, (H, W), rec, radius=2)
    assert not got[:, :, cutx:].any()
    assert (got[0, 3:8, cutx - 3:cutx] == 1.0).all() and C.nonzero_pixels(got, (0, W, 0, H)) == 15
    # centred outside its quadrant, on column cutx + 1 of the window: it still covers column cutx - 1, and only that one
    got = data.mosaic_radar_map([at_pixel(cutx + 1, 5, 2.0), None], IDENTITY, sizes, (H, W), rec, radius=2)
    assert (got[0, 3:8, cutx - 1] == 2.0).all() and C.nonzero_pixels(got, (0, W, 0, H)) == 5
    assert not got[:, :, cutx:].any() and not got[:, :, :cutx - 1].any()
    # the same across the horizontal cut, and a point beyond reach writes nothing
    got = data.mosaic_radar_map([at_pixel(4, cuty + 1, 3.0), None], IDENTITY, sizes, (H, W), rec, radius=2)
    assert (got[0, cuty - 1, 2:7] == 3.0).all() and C.nonzero_pixels(got, (0, W, 0, H)) == 5
    got = data.mosaic_radar_map([at_pixel(cutx + 3, 5, 4.0), None], IDENTITY, sizes, (H, W), rec, radius=2)
    assert not got.any()
    # each pixel hears one source only: a nearer point of tile 3's source does not win a pixel of tile 0's quadrant
    near = at_pixel(0, 5, 9.0)                     # window pixel 0 of tile 3 = canvas column cutx
    near[0, 2] = 0.5
    near[0, :2] *= 0.5
    got = data.mosaic_radar_map([at_pixel(cutx - 1, 5, 1.0), near], IDENTITY, sizes, (H, W), rec, radius=2)
    assert (got[0, 3:8, cutx - 3:cutx] == 1.0).all() and (got[0, 3:8, cutx:cutx + 3] == 9.0).all()
    assert C.nonzero_pixels(got, (0, W, 0, H)) == 30


def test_the_winner_is_the_nearest_then_the_lowest_index_within_the_source():
    rec = crossing_record(12, 18)
    pts = np.concatenate([at_pixel(3, 3, 5.0), at_pixel(3, 3, 6.0), at_pixel(3, 3, 7.0)])
    pts[2, :3] *= 0.5                              # the same pixel from half the depth
    got = data.mosaic_radar_map([pts, None], IDENTITY, [(20, 30)] * 2, (H, W), rec)
    assert got[0, 3, 3] == 7.0
    got = data.mosaic_radar_map([pts[:2], None], IDENTITY, [(20, 30)] * 2, (H, W), rec)
    assert got[0, 3, 3] == 5.0


def test_radar_sources_packs_56_bytes_per_record():
    from asy_vrnet_amd import hip
    assert data.RADAR_SOURCE_DTYPE.itemsize == hip.RADAR_SOURCE_BYTES == 56
    P = C.calib()
    counts = np.array([5, 0, 300, 1, 2, 3, 4, 7], np.int32)
    tab = data.radar_sources(P, counts)
    raw = data.radar_source_bytes(tab)
    assert tab.dtype == data.RADAR_SOURCE_DTYPE and tab.shape == (8,) and tuple(raw.shape) == (8, 56) and raw.dtype == torch.uint8
    words = raw.numpy().view("<i4").reshape(8, 14)
    assert words[:, 0].tolist() == counts.tolist() and not words[:, 1].any()
    assert np.array_equal(raw.numpy().view("<f4").reshape(8, 14)[:, 2:], P.reshape(8, 12))
    one = data.radar_sources(P[3], torch.tensor([1, 2, 3]))                      # one projection for every source; a tensor of counts
    assert np.array_equal(one["P"], np.broadcast_to(P[3].reshape(12), (3, 12))) and one["count"].tolist() == [1, 2, 3]
    for bad_calib, bad_counts in ((P[:3], counts), (np.eye(4, dtype=np.float32), counts), ("calib", counts), (P, counts.astype(np.float32)),
                                  (P, counts.reshape(2, 4)), (P, np.zeros(0, np.int32))):
        with pytest.raises(RuntimeError, match="radar_sources"):
            data.radar_sources(bad_calib, bad_counts)


def test_check_calib_takes_one_projection_per_source():
    B = 2
    P = np.arange(4 * B * 12, dtype=np.float64).reshape(4 * B, 3, 4)
    got = data.check_calib(P, 4 * B, "TrainStep")
    assert got.dtype == np.float32 and got.shape == (4 * B, 3, 4) and np.array_equal(got, P.astype(np.float32))
    assert np.array_equal(data.check_calib(torch.from_numpy(P[0]), 4 * B), np.broadcast_to(P[0].astype(np.float32), (4 * B, 3, 4)))
    with pytest.raises(RuntimeError, match=r"TrainStep: calib.*\(8, 3, 4\)"):
        data.check_calib(P[:B], 4 * B, "TrainStep")                               # one per OUTPUT image is not enough


def test_exports_and_the_arguments_that_need_no_device():
    from asy_vrnet_amd import hip
    from asy_vrnet_amd.graph import TrainStep
    from asy_vrnet_amd.infer import RadarPoints
    assert hip.ABI_VERSION == 11
    assert "vrnet_mosaic_radar_points_f32" in hip.EXPORTED and "vrnet_mosaic_radar_points_workspace" in hip.EXPORTED
    assert hip.mosaic_radar_points_workspace_bytes(2, H, W) >= 2 * H * W * 8 and hip.mosaic_radar_points_workspace_bytes(0, H, W) < 0

    class Uniform:
        def _uniform(self, key):
            return 0.1
    with pytest.raises(RuntimeError, match="mosaic with radar_points needs calib= at construction"):
        TrainStep(None, None, Uniform(), None, 2, 64, 9, from_frames=True, capacity=C.CAP, mosaic=True, radar_points=64)
    with pytest.raises(RuntimeError, match=r"calib.*\(8, 3, 4\)"):                # one per source: 4 B of them
        TrainStep(None, None, Uniform(), None, 2, 64, 9, from_frames=True, capacity=C.CAP, mosaic=True, radar_points=64,
                  calib=np.zeros((2, 3, 4)))
    rp = RadarPoints(8, calib=np.eye(3, 4), batch=8, fn="TrainStep", per_image=4)
    sets = [np.zeros((3, 7), np.float32)] * 8
    with pytest.raises(RuntimeError, match="image 1, tile 2 has 9 points"):
        rp.validate(sets[:6] + [np.zeros((9, 7), np.float32)] + sets[7:], None)
    with pytest.raises(RuntimeError, match="image 0, tile 3: points are float32"):
        rp.validate(sets[:3] + [np.zeros((3, 7))] + sets[4:], None)
    with pytest.raises(RuntimeError, match="not finished maps"):
        rp.validate(np.zeros((8, 4, H, W), np.float32), None)
    with pytest.raises(RuntimeError, match="2 point sets for a batch of 8"):
        rp.validate(sets[:2], None)
    packed, (P, counts) = rp.validate(sets, None, np.zeros((8, 3, 4)))
    assert tuple(packed.shape) == (8, 8, 7) and P.shape == (8, 3, 4) and counts.tolist() == [3] * 8
    with pytest.raises(RuntimeError, match="image 1 has 9 points"):              # a plain batch names its images as before
        RadarPoints(8, calib=np.eye(3, 4), batch=2).validate([sets[0], np.zeros((9, 7), np.float32)], None)
