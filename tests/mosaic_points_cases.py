"""What tests/test_mosaic_points_host.py and tests/test_mosaic_points.py share: a 40 x 56 canvas, eight sources of mixed sizes
inside 96 x 112 slots, hand-written Mosaic tables that between them hold every branch, and point clouds built to land in
every window.  No GPU and no test in here."""
import numpy as np

from asy_vrnet_amd import data

CANVAS = (40, 56)                                # (H, W): not square, W no multiple of a wave
CAP = (96, 112)
SIZES = [(48, 80), (90, 60), (64, 64), (37, 111), (96, 112), (20, 30), (96, 40), (50, 112)]
MAX_POINTS = 300
NAMES = ("interior", "edge", "gaps", "corners_a", "corners_b")
NAN_PAYLOAD = 0x7FC12345                         # a quiet NaN with a payload: features are copied as bits
MIN_EXPECTED = 50                                # a shown rectangle expected to receive this many points must hold 20 non-zero pixels


def tables(input_shape=CANVAS):
    """name -> a table of two records (the layout of tests/test_mosaic.py's tables on this canvas).
    interior   cuts inside the canvas, every tile against the cut as the sampler places it, two tiles of each image flipped
    edge       image 0: one-pixel quadrants (cutx = 1, cuty = H - 1), windows wider than the canvas; image 1: a window about twice
               the canvas at negative offsets, one source in two tiles
    gaps       a window smaller than its quadrant, one wholly outside its quadrant, one wholly outside the canvas, one that
               straddles the cut, absent tiles (src = -1)
    corners_a  cuts (W, H) and (W, 0): tile 0 / tile 1 alone -- the first is the non-mosaicked record, flipped
    corners_b  cuts (0, 0) and (0, H): tile 2 / tile 3 alone"""
    H, W = input_shape
    s = SIZES

    def rec(cut, tiles):
        return data.mosaic_record(input_shape, cut, tiles)
    cx, cy = W // 2 - 5, H // 2 + 3
    interior = [rec((cx, cy), [(0, s[0], 40, 24, cx - 40, cy - 24, 0), (1, s[1], 20, 30, cx - 20, cy, 1), (2, s[2], 45, 45, cx, cy, 0),
                               (3, s[3], 50, 17, cx, cy - 17, 1)]),
                rec((W // 3, H // 2), [(4, s[4], 30, 26, W // 3 - 30, H // 2 - 26, 1), (5, s[5], 27, 18, W // 3 - 27, H // 2, 0),
                                       (6, s[6], 16, 38, W // 3, H // 2, 1), (7, s[7], 48, 21, W // 3, H // 2 - 21, 0)])]
    edge = [rec((1, H - 1), [(0, s[0], 80, 60, -79, H - 61, 1), (1, s[1], 30, 40, -29, H - 1, 0), (2, s[2], 64, 64, 1, H - 1, 0),
                             (3, s[3], W + 20, 37, 1, H - 38, 0)]),
            rec((W // 2, H // 2), [(4, s[4], 2 * W - 3, 2 * H - 1, -(W // 2) - 3, -(H // 2), 0), (4, s[4], 60, 50, W // 2 - 60, H // 2 - 10, 1),
                                   (5, s[5], 30, 40, W // 2, H // 2, 0), (6, s[6], 33, 96, W // 2 + 2, -50, 1)])]
    gaps = [rec((W // 2, H // 2), [(0, s[0], 20, 12, 3, 2, 1), (1, s[1], 20, 15, 0, 0, 0), (2, s[2], 20, 20, W - 10, H - 10, 0), None]),
            rec((W // 2, H // 2), [(7, s[7], 30, 20, W, 0, 0), None, (6, s[6], 10, 24, W // 2 + 5, H // 2 + 3, 1),
                                   (5, s[5], 25, 15, W // 2 - 10, 2, 0)])]
    corners_a = [rec((W, H), [(0, s[0], 70, 50, -3, -5, 1), None, None, None]),
                 rec((W, 0), [None, (5, s[5], 45, 30, 4, 3, 0), None, None])]
    corners_b = [rec((0, 0), [None, None, (2, s[2], 64, 64, 0, 0, 1), None]),
                 rec((0, H), [None, None, None, (7, s[7], 56, 25, 5, 9, 0)])]
    return {n: data.check_mosaic_table(np.stack(t), input_shape, SIZES, CAP) for n, t in zip(NAMES, (interior, edge, gaps, corners_a, corners_b))}


def calib():
    """(S, 3, 4): a pinhole per source, the principal point in the middle of its own frame."""
    P = np.zeros((len(SIZES), 3, 4), np.float32)
    for k, (ih, iw) in enumerate(SIZES):
        P[k] = [[40.0 + k, 0, iw / 2, 0.25], [0, 38.0 - k, ih / 2, -0.5], [0, 0, 1, 0]]
    return P


def cloud(rng, size, P, n):
    """n rows whose projections spread over the frame and a margin around it, at depths 1 .. 60."""
    ih, iw = size
    u, v = rng.uniform(-4, iw + 4, n), rng.uniform(-4, ih + 4, n)
    z = rng.uniform(1, 60, n)
    pts = np.zeros((n, 7), np.float32)
    pts[:, 0] = (u - P[0, 2]) * z / P[0, 0]
    pts[:, 1] = (v - P[1, 2]) * z / P[1, 1]
    pts[:, 2] = z
    pts[:, 3:] = rng.standard_normal((n, 4))
    return pts


def point_sets(seed, counts=None):
    """One cloud per source (MAX_POINTS rows unless counts says otherwise; 0: None).  In every cloud of more than 40 rows:
    rows 10..14 repeat the position of row 5 (equal depths on one pixel: row 5 must win), rows 15 and 16 have a NaN and an
    Inf coordinate, rows 17 and 18 lie behind min_depth (z = 0.05 and z < 0), and rows 20..24 carry NaN payloads as features."""
    rng = np.random.default_rng(seed)
    P = calib()
    out = []
    for k, size in enumerate(SIZES):
        n = MAX_POINTS if counts is None else counts[k]
        if n == 0:
            out.append(None)
            continue
        pts = cloud(rng, size, P[k], n)
        if n > 40:
            pts[10:15, :3] = pts[5, :3]
            pts[15, 0], pts[16, 1] = np.nan, np.inf
            pts[17, 2], pts[18, 2] = 0.05, -3.0
            pts[20:25, 3:].view(np.uint32)[:] = NAN_PAYLOAD + np.arange(20, dtype=np.uint32).reshape(5, 4)
        out.append(pts)
    return out


def shown(rec, t, input_shape=CANVAS):
    """(x0, x1, y0, y1), half open: the canvas pixels tile t of the record shows -- its window cut by its quadrant; None: none."""
    H, W = input_shape
    tile = rec["tile"][t]
    if int(tile["src"]) < 0:
        return None
    cutx, cuty = int(rec["cutx"]), int(rec["cuty"])
    qx = (cutx, W) if t in (2, 3) else (0, cutx)
    qy = (cuty, H) if t in (1, 2) else (0, cuty)
    x0, x1 = max(qx[0], int(tile["dx"])), min(qx[1], int(tile["dx"]) + int(tile["nw"]))
    y0, y1 = max(qy[0], int(tile["dy"])), min(qy[1], int(tile["dy"]) + int(tile["nh"]))
    return (x0, x1, y0, y1) if x0 < x1 and y0 < y1 else None


def expected_points(rec, t, n=MAX_POINTS, input_shape=CANVAS):
    """How many of n points spread evenly over the source land in what tile t shows: n * shown area / window area."""
    box = shown(rec, t, input_shape)
    if box is None:
        return 0.0
    tile = rec["tile"][t]
    return n * (box[1] - box[0]) * (box[3] - box[2]) / (int(tile["nw"]) * int(tile["nh"]))


def nonzero_pixels(m, box):
    x0, x1, y0, y1 = box
    return int((np.ascontiguousarray(m[:, y0:y1, x0:x1]).view(np.uint32) != 0).any(axis=0).sum())


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)
