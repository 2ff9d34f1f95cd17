"""The radar map from points under the rotation of the post stage, on the host: `data.radar_map(..., post=)` -- this project's
own definition -- held to a per-point, per-pixel restatement in plain Python floats written out here (the forward matrix
included), and to cases placed by hand.  No GPU: the function is the truth vrnet_radar_map_post_f32 is held to
(tests/test_radar_post.py)."""
import math

import numpy as np
import pytest

from asy_vrnet_amd import data

F = np.float32
CANVASES = [(40, 63), (64, 96)]                            # (H, W)
ANGLES = [1, -1, 10, -10, 45]
FRAMES = [(48, 100), (120, 60), (64, 96)]                  # the layouts of tests/test_radar_map_host.py
EYE = np.array([[1, 0, 0, 0], [0, 1, 0, 0], [0, 0, 1, 0]], F)          # hu = x, hv = y, hw = z: x / z is the pixel column


def camera(size, f=0.9, t=(0.3, -0.2, 0.5)):
    ih, iw = size
    K = np.array([[f * iw, 0, iw / 2], [0, f * iw, ih / 2], [0, 0, 1]])
    return (K @ np.concatenate([np.eye(3), np.array(t, float)[:, None]], 1)).astype(F)


def cloud(seed, n, spread=1.0):
    rs = np.random.RandomState(seed)
    z = rs.uniform(-2, 40, n)
    xy = rs.uniform(-0.8, 0.8, (n, 2)) * spread * np.abs(z)[:, None]
    return np.concatenate([xy, z[:, None], rs.randn(n, 4)], 1).astype(F)


def forward(canvas, angle):
    """The reference's rotation by `angle` about (W // 2, H // 2) as cv2.getRotationMatrix2D(-angle) writes it, restated."""
    H, W = canvas
    cx, cy = float(W // 2), float(H // 2)
    a = -angle * math.pi / 180
    alpha, beta = math.cos(a), math.sin(a)
    return [alpha, beta, (1 - alpha) * cx - beta * cy, -beta, alpha, beta * cx + (1 - alpha) * cy]


def rotated(canvas, angle, X, Y):
    """The rule for one centre, in plain Python floats: (X', Y'), or None when it leaves the canvas."""
    H, W = canvas
    m = forward(canvas, angle)
    rx = (m[0] * float(X) + m[1] * float(Y)) + m[2]
    ry = (m[3] * float(X) + m[4] * float(Y)) + m[5]
    Xr, Yr = math.floor(rx + 0.5), math.floor(ry + 0.5)
    return (Xr, Yr) if 0 <= Xr < W and 0 <= Yr < H else None


def loop_radar_map(points, P, size, canvas, window, flip, radius, min_depth, angle=0):
    """The definition, one point and one pixel at a time: the pixels a point covers without the rotation, each moved by the
    displacement of the centre."""
    (H, W), (ih, iw), (nw, nh, dx, dy) = canvas, size, window
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
        if not (0 <= fx < nw and 0 <= fy < nh):
            continue
        ix, iy = int(np.floor(fx)), int(np.floor(fy))
        X, Y = (W - 1 - dx - ix if flip else dx + ix), dy + iy
        tx = ty = 0
        if angle:
            to = rotated(canvas, angle, X, Y)
            if to is None:
                continue
            tx, ty = to[0] - X, to[1] - Y
        for oy in range(-radius, radius + 1):
            for ox in range(-radius, radius + 1):
                px, py = X + ox, Y + oy
                ux = W - 1 - px if flip else px            # the column before the mirror: the window's extent is [dx, dx + nw)
                if not (0 <= px < W and 0 <= py < H and dx <= ux < dx + nw and dy <= py < dy + nh):
                    continue
                px, py = px + tx, py + ty
                if not (0 <= px < W and 0 <= py < H):
                    continue
                if (py, px) not in best or (hw, i) < best[(py, px)]:
                    best[(py, px)] = (hw, i)
    for (py, px), (_, i) in best.items():
        out[:, py, px] = points[i, 3:7]
    return out


def same_bits(a, b):
    return a.shape == b.shape and a.dtype == b.dtype == F and np.array_equal(a.view(np.int32), b.view(np.int32))


def at_pixels(cells, z=1.0):
    """Points under EYE whose window pixel is (X, Y) for every cell (the window being the whole frame): feature 0 = index + 1."""
    pts = np.zeros((len(cells), 7), F)
    for i, (X, Y) in enumerate(cells):
        pts[i] = ((X + 0.5) * z, (Y + 0.5) * z, z, i + 1, -(i + 1), 0.5, 2.0)
    return pts


def whole(canvas):
    return (canvas[1], canvas[0], 0, 0)


@pytest.mark.parametrize("size", FRAMES)
@pytest.mark.parametrize("radius", [0, 2])
def test_no_rotation_is_the_map_of_before(size, radius):
    canvas = H, W = 64, 96
    P, pts = camera(size), cloud(3, 400)
    pts[7, 0], pts[9, 2] = np.nan, np.inf
    lb = data.letterbox_geometry(size[1], size[0], W, H)
    off = data.aug_post_record(canvas, True, 0)                        # blurs, does not rotate
    kept = data.aug_post_record(canvas, False, 10)
    kept["rotate"] = 0                                                 # a matrix that is not looked at
    lit = 0
    for window, flip in ((lb, False), (lb, True), ((2 * W, 2 * H, -W // 2, -H // 3), True), ((W, H, 0, 0), False)):
        want = loop_radar_map(pts, P, size, canvas, window, flip, radius, 0.1)
        assert same_bits(data.radar_map(pts, P, size, canvas, window, flip, radius, 0.1), want)
        for post in (None, off, kept):
            assert same_bits(data.radar_map(pts, P, size, canvas, window, flip, radius, 0.1, post=post), want), (window, flip)
        lit += int((want != 0).any(0).sum())
    assert lit > 100


@pytest.mark.parametrize("canvas", CANVASES)
@pytest.mark.parametrize("angle", ANGLES)
def test_single_points_land_where_the_rule_says(canvas, angle):
    H, W = canvas
    post = data.aug_post_record(canvas, False, angle)
    assert [float(v) for v in post["fwd"]] == forward(canvas, angle)
    cells = [(W // 2, H // 2), (0, 0), (W - 1, 0), (0, H - 1), (W - 1, H - 1), (W // 2, 0), (3, H // 2), (W - 5, H - 7), (W // 3, H // 4),
             (W // 2 + 1, H // 2), (W // 2, H // 2 - 1)]
    gone = 0
    for X, Y in cells:
        pts = at_pixels([(X, Y)])
        plain = data.radar_map(pts, EYE, canvas, canvas, whole(canvas))
        assert np.argwhere(plain[0] != 0).tolist() == [[Y, X]]
        got = data.radar_map(pts, EYE, canvas, canvas, whole(canvas), post=post)
        to = rotated(canvas, angle, X, Y)
        if to is None:
            gone += 1
            assert not got.view(np.uint32).any(), (X, Y)
        else:
            assert np.argwhere(got[0] != 0).tolist() == [[to[1], to[0]]], (X, Y)
            assert same_bits(got[:, to[1], to[0]], pts[0, 3:7])
    assert rotated(canvas, angle, W // 2, H // 2) == (W // 2, H // 2)              # the centre stays where it is
    assert gone >= (2 if abs(angle) >= 10 else 0)                                  # corners leave the canvas and vanish
    if angle == 45:
        assert rotated(canvas, angle, 0, 0) is None


def grid_cloud(seed, canvas, share=0.35):
    """Isolated points: a random share of the cells (4 i + 1, 4 j + 1), so every pair is at least 4 pixels apart."""
    H, W = canvas
    rs = np.random.RandomState(seed)
    cells = [(x, y) for y in range(1, H, 4) for x in range(1, W, 4) if rs.rand() < share]
    return cells, at_pixels(cells)


ONCE_SEED = 5          # chosen on the CPU so that the last assertion below holds in all four cases (seeds 0 .. 4 miss one each)


@pytest.mark.parametrize("canvas", CANVASES)
@pytest.mark.parametrize("angle", [10, -10])
def test_every_point_is_placed_exactly_once_and_the_gather_of_a_finished_map_does_not(canvas, angle):
    cells, pts = grid_cloud(ONCE_SEED, canvas)
    assert len(cells) > 40 and min(max(abs(a[0] - b[0]), abs(a[1] - b[1])) for k, a in enumerate(cells) for b in cells[:k]) > 3
    post = data.aug_post_record(canvas, False, angle)
    plain = data.radar_map(pts, EYE, canvas, canvas, whole(canvas))
    assert np.count_nonzero(plain[0]) == len(cells)
    got = data.radar_map(pts, EYE, canvas, canvas, whole(canvas), post=post)
    inside = [c for c in cells if rotated(canvas, angle, *c) is not None]
    assert len(inside) < len(cells)
    assert np.count_nonzero(got[0]) == len(inside)
    assert sorted(got[0][got[0] != 0].tolist()) == [float(cells.index(c) + 1) for c in inside]     # each of them, once
    # the nearest gather of the finished map drops some of these one-pixel points and doubles others: why this path exists
    gathered = data.rotate_nearest(plain[0], post["inv"], 0.0)
    assert np.count_nonzero(gathered) != len(inside)


def test_points_that_meet_only_after_the_rotation_the_lower_index_wins():
    canvas = H, W = 64, 96
    angle = 10
    pair = None
    for Y in range(4, H - 4):
        for X in range(4, W - 5):
            a, b = rotated(canvas, angle, X, Y), rotated(canvas, angle, X + 1, Y)
            if a is not None and a == b:
                pair = ((X, Y), (X + 1, Y), a)
                break
        if pair:
            break
    assert pair is not None
    first, second, to = pair
    post = data.aug_post_record(canvas, False, angle)
    for cells in ((first, second), (second, first)):
        pts = at_pixels(cells, z=2.0)
        pts[:, 3:] = [[7, 1, 2, 3], [9, 4, 5, 6]]
        assert np.count_nonzero(data.radar_map(pts, EYE, canvas, canvas, whole(canvas))[0]) == 2
        got = data.radar_map(pts, EYE, canvas, canvas, whole(canvas), post=post)
        assert np.argwhere(got[0] != 0).tolist() == [[to[1], to[0]]]
        assert got[:, to[1], to[0]].tolist() == [7, 1, 2, 3]           # index 0, whichever pixel it came from
        far = pts.copy()
        far[0, :3] *= 2                                                # the same pixel, twice the depth: the nearer one wins
        assert data.radar_map(far, EYE, canvas, canvas, whole(canvas), post=post)[:, to[1], to[0]].tolist() == [9, 4, 5, 6]


def rect_mask(canvas, x0, x1, y0, y1):
    m = np.zeros(canvas, bool)
    if x0 <= x1 and y0 <= y1:
        m[y0:y1 + 1, x0:x1 + 1] = True
    return m


@pytest.mark.parametrize("radius", [2, 8])
@pytest.mark.parametrize("angle", [10, -7])
@pytest.mark.parametrize("flip", [False, True])
def test_the_footprint_is_the_cut_rectangle_moved_with_its_centre(radius, angle, flip):
    canvas = H, W = 64, 96
    post = data.aug_post_record(canvas, False, angle)
    seen = 0
    # a window inside the canvas, the point next to each of its borders; the whole canvas, the point next to each edge
    for window, cells in (((40, 30, 30, 20), [(0, 0), (39, 29), (1, 15), (20, 28)]), ((W, H, 0, 0), [(1, 1), (W - 2, H // 2), (W // 2, H - 1)])):
        nw, nh, dx, dy = window
        for ix, iy in cells:
            size = (nh, nw)                                            # the frame fills the window: window pixel = frame pixel
            pts = at_pixels([(ix, iy)])
            cx, cy = dx + ix, dy + iy
            x0, x1 = max(cx - radius, 0, dx), min(cx + radius, W - 1, dx + nw - 1)
            y0, y1 = max(cy - radius, 0, dy), min(cy + radius, H - 1, dy + nh - 1)
            assert (x1 - x0 + 1) * (y1 - y0 + 1) < (2 * radius + 1) ** 2           # the window or the canvas cuts it
            if flip:
                x0, x1, cx = W - 1 - x1, W - 1 - x0, W - 1 - cx
            plain = data.radar_map(pts, EYE, size, canvas, window, flip, radius)
            assert np.array_equal(plain[0] != 0, rect_mask(canvas, x0, x1, y0, y1))
            to = rotated(canvas, angle, cx, cy)
            want = np.zeros(canvas, bool)
            if to is not None:
                tx, ty = to[0] - cx, to[1] - cy
                want = rect_mask(canvas, max(x0 + tx, 0), min(x1 + tx, W - 1), max(y0 + ty, 0), min(y1 + ty, H - 1))
            got = data.radar_map(pts, EYE, size, canvas, window, flip, radius, post=post)
            assert np.array_equal(got[0] != 0, want), (window, ix, iy)
            assert same_bits(got, loop_radar_map(pts, EYE, size, canvas, window, flip, radius, 0.1, angle))
            seen += int(want.sum())
    assert seen > 50                                       # the case is not empty


@pytest.mark.parametrize("canvas", CANVASES)
@pytest.mark.parametrize("radius", [0, 2, 8])
def test_rotated_map_equals_the_plain_loop(canvas, radius):
    H, W = canvas
    size = FRAMES[0]
    P, pts = camera(size), cloud(3, 300)
    pts[7, 0], pts[9, 2] = np.nan, np.inf
    lb = data.letterbox_geometry(size[1], size[0], W, H)
    lit = 0
    for k, (window, flip) in enumerate(((lb, False), (lb, True), ((2 * W, 2 * H, -W // 2, -H // 3), True), ((30, 20, 5, 9), False))):
        angle = (10, -10, 1, -7)[k]
        got = data.radar_map(pts, P, size, canvas, window, flip, radius, 0.1, post=data.aug_post_record(canvas, k % 2, angle))
        assert same_bits(got, loop_radar_map(pts, P, size, canvas, window, flip, radius, 0.1, angle)), (window, flip, angle)
        lit += int((got != 0).any(0).sum())
    assert lit > 100


def test_a_matrix_that_sends_every_point_nowhere_drops_it():
    canvas = (40, 63)
    pts = at_pixels([(5, 5), (30, 20)])
    post = data.aug_post_record(canvas, False, 10)
    for value in (np.inf, np.nan, 1e300):
        post["fwd"][2] = value
        assert not data.radar_map(pts, EYE, canvas, canvas, whole(canvas), post=post).view(np.uint32).any()
