"""The radar map from radar points on the host (data.radar_map, radar_project, radar_views, pack_points): this project's own
definition -- the reference describes the step and ships no code for it -- held to a plain per-point, per-pixel loop written
out here, to the same rule in float64, and to cases computed by hand.  No GPU: `data.radar_map` is the truth the kernels of
csrc/radarmap.hip are held to (tests/test_radar_map.py)."""
import numpy as np
import pytest
import torch

from asy_vrnet_amd import data

F = np.float32
CANVAS = (64, 96)                                          # (H, W)
FRAMES = [(48, 100), (120, 60), (64, 96)]                  # (ih, iw): a window cut in y, one cut in x, the whole canvas


def camera(size, f=0.9, t=(0.3, -0.2, 0.5)):
    """A pinhole (3, 4) projection for a frame of size (ih, iw): focal length f * iw, the principal point in the middle."""
    ih, iw = size
    K = np.array([[f * iw, 0, iw / 2], [0, f * iw, ih / 2], [0, 0, 1]])
    return (K @ np.concatenate([np.eye(3), np.array(t, float)[:, None]], 1)).astype(F)


def cloud(seed, n, spread=1.0):
    """n points in front of (and a few behind) the camera, features drawn at random."""
    rs = np.random.RandomState(seed)
    z = rs.uniform(-2, 40, n)
    xy = rs.uniform(-0.8, 0.8, (n, 2)) * spread * np.abs(z)[:, None]
    return np.concatenate([xy, z[:, None], rs.randn(n, 4)], 1).astype(F)


def loop_radar_map(points, P, size, input_shape, window, flip, radius, min_depth):
    """The definition, one point and one pixel at a time, in numpy float32 scalars."""
    (H, W), (ih, iw), (nw, nh, dx, dy) = input_shape, size, window
    out = np.zeros((4, H, W), F)
    best = {}
    for i, (x, y, z) in enumerate(points[:, :3]):
        with np.errstate(all="ignore"):
            hu = ((P[0, 0] * x + P[0, 1] * y) + P[0, 2] * z) + P[0, 3]
            hv = ((P[1, 0] * x + P[1, 1] * y) + P[1, 2] * z) + P[1, 3]
            hw = ((P[2, 0] * x + P[2, 1] * y) + P[2, 2] * z) + P[2, 3]
            if not (hw >= F(min_depth) and np.isfinite(hw) and np.isfinite(hu) and np.isfinite(hv)):
                continue
            fx = ((hu / hw) * F(nw)) / F(iw)
            fy = ((hv / hw) * F(nh)) / F(ih)
        assert type(fx) is F and type(fy) is F
        if not (0 <= fx < nw and 0 <= fy < nh):
            continue
        ix, iy = int(np.floor(fx)), int(np.floor(fy))
        X, Y = (W - 1 - dx - ix if flip else dx + ix), dy + iy
        for oy in range(-radius, radius + 1):
            for ox in range(-radius, radius + 1):
                px, py = X + ox, Y + oy
                ux = W - 1 - px if flip else px            # the column before the mirror: the window's extent is [dx, dx + nw)
                if not (0 <= px < W and 0 <= py < H and dx <= ux < dx + nw and dy <= py < dy + nh):
                    continue
                if (py, px) not in best or (hw, i) < best[(py, px)]:
                    best[(py, px)] = (hw, i)
    for (py, px), (_, i) in best.items():
        out[:, py, px] = points[i, 3:7]
    return out


def same_bits(a, b):
    return a.shape == b.shape and a.dtype == b.dtype == F and np.array_equal(a.view(np.int32), b.view(np.int32))


@pytest.mark.parametrize("size", FRAMES)
@pytest.mark.parametrize("radius", [0, 2])
def test_radar_map_equals_the_plain_loop(size, radius):
    H, W = CANVAS
    P = camera(size)
    pts = cloud(3, 400)
    pts[7, 0] = np.nan
    pts[9, 2] = np.inf
    lb = data.letterbox_geometry(size[1], size[0], W, H)
    covered = 0
    for window, flip in ((lb, False), (lb, True), ((2 * W, 2 * H, -W // 2, -H // 3), True), ((W, H, 0, 0), False)):
        got = data.radar_map(pts, P, size, CANVAS, window, flip, radius, 0.1)
        want = loop_radar_map(pts, P, size, CANVAS, window, flip, radius, 0.1)
        assert same_bits(got, want), (size, window, flip)
        nw, nh, dx, dy = window
        inside = np.zeros((H, W), bool)
        inside[max(dy, 0):max(dy + nh, 0), max(dx, 0):max(dx + nw, 0)] = True
        inside = inside[:, ::-1] if flip else inside
        assert not got[:, ~inside].any()                   # nothing outside the window
        covered += int((got != 0).any(0).sum())
    assert covered > 100                                   # the case is not empty


def project64(points, P, size, window, min_depth):
    """`data.radar_project`'s rule in float64."""
    (ih, iw), (nw, nh) = size, window[:2]
    p, P = points[:, :3].astype(np.float64), P.astype(np.float64)
    hu, hv, hw = (((P[r, 0] * p[:, 0] + P[r, 1] * p[:, 1]) + P[r, 2] * p[:, 2]) + P[r, 3] for r in range(3))
    ok = hw >= np.float64(F(min_depth))
    den = np.where(ok, hw, 1.0)
    fx, fy = ((hu / den) * nw) / iw, ((hv / den) * nh) / ih
    ok &= (fx >= 0) & (fx < nw) & (fy >= 0) & (fy < nh)
    return ok, np.where(ok, np.floor(fx), 0).astype(np.int64), np.where(ok, np.floor(fy), 0).astype(np.int64)


def test_float32_rule_agrees_with_float64_on_all_but_1e_4_of_the_points_in_view():
    rs = np.random.RandomState(2024)
    in_view = differ = 0
    for k in range(200):
        size = (int(rs.randint(32, 720)), int(rs.randint(32, 1280)))
        S = int(rs.choice([64, 256, 512]))
        window = data.letterbox_geometry(size[1], size[0], S, S) if k % 2 else \
            (int(rs.randint(S // 4, 2 * S)), int(rs.randint(S // 4, 2 * S)), 0, 0)
        P = camera(size, f=rs.uniform(0.5, 1.5), t=rs.uniform(-1, 1, 3))
        pts = cloud(1000 + k, 4096, spread=rs.uniform(0.3, 1.2))
        ok32, ix32, iy32, _ = data.radar_project(pts, P, size, window, 0.1)
        ok64, ix64, iy64 = project64(pts, P, size, window, 0.1)
        in_view += int((ok32 | ok64).sum())
        differ += int(((ok32 != ok64) | (ix32 != ix64) | (iy32 != iy64)).sum())
    print(f"float32 against float64: {differ} of {in_view} points in view differ")
    assert in_view > 200000
    assert differ <= 1e-4 * in_view                        # measured with this seed: 4 of 369 873 (1.1e-5)


EYE = np.array([[1, 0, 0, 0], [0, 1, 0, 0], [0, 0, 1, 0]], F)          # hu = x, hv = y, hw = z


def rows(*xyz):
    """Points (x, y, z) with the features (k + 1, 10 (k + 1), 100 (k + 1), 1000 (k + 1)) for point k."""
    out = np.zeros((len(xyz), 7), F)
    for k, p in enumerate(xyz):
        out[k] = tuple(p) + tuple((k + 1) * m for m in (1, 10, 100, 1000))
    return out


def lit(m):
    """{(y, x): f0} of the pixels a map sets, after checking that the four channels are f0 times 1, 10, 100, 1000."""
    ys, xs = np.nonzero(m[0])
    assert np.array_equal(np.nonzero(m.any(0)), (ys, xs))
    for c, mult in enumerate((1, 10, 100, 1000)):
        assert np.array_equal(m[c], m[0] * mult)
    return {(int(y), int(x)): int(m[0, y, x]) for y, x in zip(ys, xs)}


def test_hand_computed_cases():
    S8 = (8, 8)
    whole = (8, 8, 0, 0)
    # a pixel boundary belongs to the pixel it starts; u == iw is outside; so is anything negative; -0.0 is 0
    pts = rows((3.0, 2.0, 1.0), (8.0, 2.0, 1.0), (np.nextafter(F(8), F(0)), 0.0, 1.0), (-1e-6, 1.0, 1.0), (-0.0, 7.5, 1.0))
    assert lit(data.radar_map(pts, EYE, S8, S8, whole)) == {(2, 3): 1, (0, 7): 3, (7, 0): 5}
    # hw == min_depth is kept, the float32 below it is not: x = 2 hw, so u = 2 exactly
    md = F(0.1)
    below = np.nextafter(md, F(0))
    pts = rows((2 * md, 4 * md, md), (2 * below, below, below))
    assert lit(data.radar_map(pts, EYE, S8, S8, whole, min_depth=0.1)) == {(4, 2): 1}
    assert lit(data.radar_map(pts, EYE, S8, S8, whole, min_depth=float(below))) == {(4, 2): 1, (1, 2): 2}
    # the nearer point wins whatever the order; equal depth: the lower index
    pts = rows((4.5, 4.5, 1.0), (2.25, 2.25, 0.5), (9.0, 9.0, 2.0), (1.5, 1.5, 1.0), (3.0, 3.0, 2.0), (1.75, 1.75, 1.0))
    assert lit(data.radar_map(pts, EYE, S8, S8, whole)) == {(4, 4): 2, (1, 1): 4}
    # flip mirrors the canvas: column 3 -> W - 1 - 3
    pts = rows((3.0, 2.0, 1.0))
    assert lit(data.radar_map(pts, EYE, S8, S8, whole, flip=True)) == {(2, 4): 1}
    # a window twice the canvas at (-4, -4): u = 4 of 8 -> fx = 8 -> canvas column 4; u = 1 -> fx = 2 -> column -2, cropped
    big = (16, 16, -4, -4)
    pts = rows((4.0, 5.0, 1.0), (1.0, 5.0, 1.0), (7.9, 2.0, 1.0))
    assert lit(data.radar_map(pts, EYE, S8, S8, big)) == {(6, 4): 1}
    assert lit(data.radar_map(pts, EYE, S8, S8, big, flip=True)) == {(6, 3): 1}
    # ... but its footprint reaches the canvas: centre column -2, radius 2 -> column 0 alone
    assert lit(data.radar_map(pts[1:2], EYE, S8, S8, big, radius=2)) == {(y, 0): 2 for y in range(4, 8)}
    # radius 1 at the corner of a 4 x 4 window at (2, 2): cut by the window, not by the canvas
    small = (4, 4, 2, 2)
    pts = rows((0.5, 0.5, 1.0))
    assert lit(data.radar_map(pts, EYE, (4, 4), S8, small, radius=1)) == {(2, 2): 1, (2, 3): 1, (3, 2): 1, (3, 3): 1}
    assert lit(data.radar_map(pts, EYE, (4, 4), S8, small, flip=True, radius=1)) == {(2, 5): 1, (2, 4): 1, (3, 5): 1, (3, 4): 1}
    # a frame twice the window: u = 5 of 8 -> fx = 2.5 of 4
    pts = rows((5.0, 7.0, 1.0))
    assert lit(data.radar_map(pts, EYE, S8, S8, small)) == {(5, 4): 1}
    # NaN features are copied bit for bit; a NaN coordinate rejects; no points: zeros
    pts = rows((1.0, 1.0, 1.0), (np.nan, 1.0, 1.0), (2.0, 2.0, np.inf))
    pts[0, 3:7].view(np.uint32)[:] = (0x7FC01234, 0xFFC00001, 0x7F800000, 0x80000000)
    m = data.radar_map(pts, EYE, S8, S8, whole)
    assert m[:, 1, 1].view(np.uint32).tolist() == [0x7FC01234, 0xFFC00001, 0x7F800000, 0x80000000]
    assert np.count_nonzero(m.view(np.uint32)) == 4
    assert not data.radar_map(np.zeros((0, 7), F), EYE, S8, S8, whole).any()
    # the argument checks
    for bad in (dict(radius=9), dict(radius=-1), dict(radius=1.0), dict(min_depth=0.0), dict(min_depth=float("nan"))):
        with pytest.raises(RuntimeError, match="radius|min_depth"):
            data.radar_map(pts, EYE, S8, S8, whole, **bad)
    with pytest.raises(RuntimeError, match="float32"):
        data.radar_map(pts.astype(np.float64), EYE, S8, S8, whole)
    with pytest.raises(RuntimeError, match=r"\(3, 4\)"):
        data.radar_map(pts, np.eye(4, dtype=F), S8, S8, whole)


def test_radar_views_packs_80_bytes_from_both_table_kinds():
    from asy_vrnet_amd import hip
    assert data.RADAR_VIEW_DTYPE.itemsize == hip.RADAR_VIEW_BYTES == 80
    sizes = [(48, 100), (120, 60)]
    P = np.stack([camera(s) for s in sizes])
    geom = data.frame_geometry(sizes, CANVAS)
    v = data.radar_views(geom, P, [5, 0])
    raw = data.radar_view_bytes(v)
    assert raw.dtype == torch.uint8 and tuple(raw.shape) == (2, 80)
    ints = raw.numpy().view("<i4").reshape(2, 20)
    for b, (ih, iw) in enumerate(sizes):
        assert ints[b, :8].tolist() == [ih, iw, *data.letterbox_geometry(iw, ih, CANVAS[1], CANVAS[0]), 0, (5, 0)[b]]
        assert np.array_equal(raw.numpy()[b, 32:].view("<f4"), P[b].reshape(12))
    aug = np.stack([data.aug_record(sizes[0], CANVAS, 192, 128, -48, -21, flip=True),
                    data.aug_record(sizes[1], CANVAS, 30, 40, 7, 9)])
    v = data.radar_views(aug, P[0], np.array([3, 4], np.int32))          # one projection for all
    ints = data.radar_view_bytes(v).numpy().view("<i4").reshape(2, 20)
    assert ints[0, :8].tolist() == [48, 100, 192, 128, -48, -21, 1, 3] and ints[1, :8].tolist() == [120, 60, 30, 40, 7, 9, 0, 4]
    assert np.array_equal(v["P"][1], P[0].reshape(12))
    with pytest.raises(RuntimeError, match="calib"):
        data.radar_views(geom, np.eye(3), [0, 0])
    with pytest.raises(RuntimeError, match="counts"):
        data.radar_views(geom, P, [0])
    with pytest.raises(RuntimeError, match="GEOM_DTYPE"):
        data.radar_views(np.zeros(2), P, [0, 0])


def test_pack_points_packs_and_its_errors_name_the_image():
    a, b = cloud(1, 3), cloud(2, 5)
    packed, counts = data.pack_points([a, None, b, np.zeros((0, 7), F)], 6)
    assert tuple(packed.shape) == (4, 6, 7) and packed.dtype == torch.float32 and counts.tolist() == [3, 0, 5, 0]
    assert np.array_equal(packed[0, :3].numpy(), a) and np.array_equal(packed[2, :5].numpy(), b)
    assert not packed[0, 3:].any() and not packed[1].any() and not packed[3].any()
    padded = np.zeros((2, 5, 7), F)
    padded[0, :3], padded[1] = a, b
    again, counts = data.pack_points((padded, np.array([3, 5])), 6)
    assert counts.tolist() == [3, 5] and np.array_equal(again[0].numpy(), packed[0].numpy())
    assert np.array_equal(again[1].numpy(), packed[2].numpy())
    with pytest.raises(RuntimeError, match="image 1 has 5 points, above max_points = 4"):
        data.pack_points([a, b], 4)
    with pytest.raises(RuntimeError, match="image 1: points are float32"):
        data.pack_points([a, b.astype(np.float64)], 8)
    with pytest.raises(RuntimeError, match=r"image 0: expected \(n, 7\)"):
        data.pack_points([a[:, :6], b], 8)
    with pytest.raises(RuntimeError, match="image 1: counts says 6 points"):
        data.pack_points((padded, np.array([3, 6])), 8)
    with pytest.raises(RuntimeError, match="expected a list"):
        data.pack_points(a, 8)


def test_exports_exist_and_the_abi_stays_11():
    from asy_vrnet_amd import hip
    assert hip.ABI_VERSION == 11
    assert "vrnet_radar_map_f32" in hip.EXPORTED and "vrnet_radar_map_workspace" in hip.EXPORTED
    assert hip.FLAG_POINT_COUNT == 1024 and hip.FLAG_POINT_COUNT not in (hip.FLAG_GEOMETRY, hip.FLAG_BOX_COUNT)
    assert hip.radar_map_workspace_bytes(3, 64, 96) >= 3 * 64 * 96 * 8
    for name in ("radar_map", "radar_project", "radar_views", "radar_view_bytes", "pack_points", "device_radar_map"):
        assert callable(getattr(data, name))


def test_pipeline_arguments_that_need_no_device():
    from asy_vrnet_amd.graph import TrainStep
    from asy_vrnet_amd.infer import FramePipeline, RadarPoints

    class Uniform:
        def _uniform(self, key):
            return 0.1
    with pytest.raises(RuntimeError, match="radar_points needs from_frames"):
        TrainStep(None, None, Uniform(), None, 2, 64, 9, radar_points=100)
    with pytest.raises(RuntimeError, match="belong to radar_points"):
        TrainStep(None, None, Uniform(), None, 2, 64, 9, from_frames=True, capacity=(64, 64), radar_radius=1)
    with pytest.raises(RuntimeError, match="radius"):
        TrainStep(None, None, Uniform(), None, 2, 64, 9, from_frames=True, capacity=(64, 64), radar_points=10, radar_radius=9)

    class Eval:
        training = False
    for kw, match in ((dict(radar_points=0), "radar_points"), (dict(radar_points=10, radar_radius=9), "radius"),
                      (dict(radar_points=10, radar_min_depth=0.0), "min_depth"), (dict(calib=np.eye(3, 4)), "belong to radar_points"),
                      (dict(radar_points=10, calib=np.eye(3)), "calib"),
                      (dict(radar_points=10, radar_dtype=torch.float64, normalise_radar=True), "float32")):
        with pytest.raises(RuntimeError, match=match):
            FramePipeline(Eval(), (48, 64), (64, 64), batch=2, **kw)
    # what a call brings: points, not maps; a projection from somewhere; one set per image; within the capacity
    table = data.frame_geometry([(48, 64)] * 2, (64, 64))
    rp = RadarPoints(8, batch=2)
    with pytest.raises(RuntimeError, match="not finished maps"):
        rp.validate(np.zeros((2, 4, 64, 64), F), table, np.eye(3, 4))
    with pytest.raises(RuntimeError, match="need a projection"):
        rp.validate([cloud(1, 3)] * 2, table)
    with pytest.raises(RuntimeError, match="1 point sets for a batch of 2"):
        rp.validate([cloud(1, 3)], table, np.eye(3, 4))
    with pytest.raises(RuntimeError, match="image 1 has 9 points"):
        rp.validate([cloud(1, 3), cloud(1, 9)], table, np.eye(3, 4))
    packed, views = rp.validate([cloud(1, 3), cloud(1, 8)], table, np.eye(3, 4))
    assert tuple(packed.shape) == (2, 8, 7) and tuple(views.shape) == (2, 80)
    assert views.numpy().view("<i4").reshape(2, 20)[:, 7].tolist() == [3, 8]
