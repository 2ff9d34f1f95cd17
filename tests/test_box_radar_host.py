"""The radar readout of the detections on the host (data.box_radar): this project's own definition -- the reference has no code
for it -- held to a plain loop over boxes and points written out here (`sorted` on (depth bits, index)), to cases computed by
hand, and to the same rule in float64.  No GPU: `data.box_radar` is the truth the kernels of csrc/boxradar.hip are held to
(tests/test_box_radar.py).  Also here: `FrameResult.radar_readout` and the text of `predict_dir` on a result made by hand."""
import numpy as np
import pytest
import torch

from asy_vrnet_amd import data, infer

F = np.float32
EYE = np.array([[1, 0, 0, 0], [0, 1, 0, 0], [0, 0, 1, 0]], F)          # hu = x, hv = y, hw = z: u = x / z, v = y / z
SIZE = (8, 16)                                                         # (ih, iw) of the hand-built cases


def camera(size, f=0.9, t=(0.3, -0.2, 0.5)):
    """tests/test_radar_map_host.py: a pinhole (3, 4) projection for a frame of size (ih, iw)."""
    ih, iw = size
    K = np.array([[f * iw, 0, iw / 2], [0, f * iw, ih / 2], [0, 0, 1]])
    return (K @ np.concatenate([np.eye(3), np.array(t, float)[:, None]], 1)).astype(F)


def cloud(seed, n, spread=1.0):
    """tests/test_radar_map_host.py: n points in front of (and a few behind) the camera, features drawn at random."""
    rs = np.random.RandomState(seed)
    z = rs.uniform(-2, 40, n)
    xy = rs.uniform(-0.8, 0.8, (n, 2)) * spread * np.abs(z)[:, None]
    return np.concatenate([xy, z[:, None], rs.randn(n, 4)], 1).astype(F)


def uvz(*pts):
    """Points under EYE written as (pixel column u, pixel row v, depth z) -> (u z, v z, z), with the features
    (k + 1) * (1, 10, 100, 1000) for point k.  With z a power of two u and v come back exactly."""
    out = np.zeros((len(pts), 7), F)
    for k, (u, v, z) in enumerate(pts):
        out[k] = (F(u) * F(z), F(v) * F(z), z) + tuple((k + 1) * m for m in (1, 10, 100, 1000))
    return out


def boxes(*tlbr):
    """Rows as FrameResult.rows has them: top, left, bottom, right, then obj, class_conf, class."""
    out = np.zeros((len(tlbr), 7), F)
    for k, b in enumerate(tlbr):
        out[k] = tuple(b) + (0.9, 0.8, 1)
    return out


def loop_box_radar(points, P, size, rows, min_depth=0.1, shrink=1.0):
    """The definition, one box and one point at a time, in numpy float32 scalars; the order by `sorted`."""
    ih, iw = size
    half, md, s = F(0.5), F(min_depth), F(shrink)
    proj = []
    with np.errstate(all="ignore"):
        for i, (x, y, z) in enumerate(points[:, :3]):
            hu = ((P[0, 0] * x + P[0, 1] * y) + P[0, 2] * z) + P[0, 3]
            hv = ((P[1, 0] * x + P[1, 1] * y) + P[1, 2] * z) + P[1, 3]
            hw = ((P[2, 0] * x + P[2, 1] * y) + P[2, 2] * z) + P[2, 3]
            if not (hw >= md and np.isfinite(hw) and np.isfinite(hu) and np.isfinite(hv)):
                continue
            u, v = hu / hw, hv / hw
            assert type(u) is F and type(v) is F and type(hw) is F
            if 0 <= u < F(iw) and 0 <= v < F(ih):
                proj.append((i, u, v, hw))
        count = np.zeros(len(rows), np.int32)
        readout = np.zeros((len(rows), 2, 5), np.uint32)
        for r, (t, l, b, rt) in enumerate(rows[:, :4]):
            if s == 1:
                y0, y1, x0, x1 = t, b, l, rt
            else:
                cy, cx = (t + b) * half, (l + rt) * half
                hy, hx = ((b - t) * half) * s, ((rt - l) * half) * s
                y0, y1, x0, x1 = cy - hy, cy + hy, cx - hx, cx + hx
            assert type(y0) is F and type(x1) is F
            cand = sorted((int(np.array(hw).view(np.uint32)), i) for i, u, v, hw in proj if x0 <= u < x1 and y0 <= v < y1)
            count[r] = len(cand)
            if cand:
                for k, (depth, i) in enumerate((cand[0], cand[(len(cand) - 1) // 2])):
                    readout[r, k, 0] = depth
                    readout[r, k, 1:] = points[i, 3:7].view(np.uint32)
    return count, readout.view(F)


def same(got, want):
    (gc, gr), (wc, wr) = got, want
    return gc.dtype == wc.dtype == np.int32 and gr.dtype == wr.dtype == F and gc.shape == wc.shape and gr.shape == wr.shape and \
        np.array_equal(gc, wc) and np.array_equal(gr.view(np.int32), wr.view(np.int32))


def both(points, P, size, rows, **kw):
    """data.box_radar, after checking it against the plain loop."""
    got = data.box_radar(points, P, size, rows, **kw)
    assert same(got, loop_box_radar(points, P, size, rows, **kw)), kw
    return got


def who(readout):
    """(f0 of the nearest, f0 of the median) per box: the 1-based point number under `uvz`, 0 without a candidate; after
    checking that every feature row is that number times 1, 10, 100, 1000."""
    for c, mult in enumerate((1, 10, 100, 1000)):
        assert np.array_equal(readout[:, :, 1 + c], readout[:, :, 1] * mult)
    return [tuple(int(v) for v in row) for row in readout[:, :, 1]]


def test_hand_computed_edges_of_box_and_frame():
    last_u, last_v = np.nextafter(F(10), F(0)), np.nextafter(F(6), F(0))
    # left and top inclusive, right and bottom exclusive
    pts = uvz((4, 2, 1), (10, 3, 1), (5, 6, 1), (last_u, last_v, 1), (np.nextafter(F(4), F(0)), 3, 1), (5, np.nextafter(F(2), F(0)), 1))
    count, ro = both(pts, EYE, SIZE, boxes((2, 4, 6, 10)))
    assert count.tolist() == [2] and who(ro) == [(1, 1)]                  # points 1 and 4, equal depth: the lower index twice
    # the frame: u == iw is not in view, the float32 below it is; a box the NMS did not clip still sees the frame only
    edge = np.nextafter(F(16), F(0))
    pts = uvz((16, 1, 1), (edge, 1, 2), (18, 1, 1), (-1, 1, 1), (3, 8, 1), (3, -0.0, 4), (3, np.nextafter(F(8), F(0)), 8))
    count, ro = both(pts, EYE, SIZE, boxes((-4, -4, 12, 20), (0, 0, 8, 16)))
    assert count.tolist() == [3, 3] and who(ro) == [(2, 6), (2, 6)] and ro[0, :, 0].tolist() == [2.0, 4.0]
    # hw below, at and above min_depth (x = 2 hw: u = 2 exactly)
    md = F(0.1)
    below, above = np.nextafter(md, F(0)), np.nextafter(md, F(1))
    pts = uvz((2, 1, below), (2, 1, md), (2, 1, above))
    count, ro = both(pts, EYE, SIZE, boxes((0, 0, 8, 16)), min_depth=0.1)
    assert count.tolist() == [2] and who(ro) == [(2, 2)] and ro[0, 0, 0] == md
    count, ro = both(pts, EYE, SIZE, boxes((0, 0, 8, 16)), min_depth=float(below))
    assert count.tolist() == [3] and who(ro) == [(1, 2)]
    count, ro = both(pts, EYE, SIZE, boxes((0, 0, 8, 16)), min_depth=0.5)
    assert count.tolist() == [0] and not ro.view(np.uint32).any()


def test_hand_computed_rejections():
    whole = boxes((0, 0, 8, 16))
    pts = uvz((3, 3, 1), (3, 3, 2), (3, 3, 4), (3, 3, 8), (3, 3, 16), (3, 3, 32), (3, 3, 0.5))
    pts[0, 0], pts[1, 1], pts[2, 2] = np.nan, np.nan, np.nan
    pts[3, 0], pts[4, 1], pts[5, 2] = np.inf, -np.inf, np.inf
    count, ro = both(pts, EYE, SIZE, whole)
    assert count.tolist() == [1] and who(ro) == [(7, 7)]
    good = uvz((3, 3, 1), (4, 4, 2))
    for r, c, bad in ((0, 3, np.nan), (1, 0, np.nan), (2, 2, np.nan), (0, 3, np.inf), (2, 3, np.inf), (1, 3, -np.inf)):
        P = EYE.copy()
        P[r, c] = bad
        count, ro = both(good, P, SIZE, whole)
        assert count.tolist() == [0] and not ro.view(np.uint32).any(), (r, c, bad)
    # a NaN edge contains nothing, whichever edge; a degenerate box neither; the box beside them is not disturbed
    rows = boxes((np.nan, 0, 8, 16), (0, np.nan, 8, 16), (0, 0, np.nan, 16), (0, 0, 8, np.nan), (5, 0, 5, 16), (6, 0, 2, 16),
                 (0, 9, 8, 3), (0, 0, 8, 16))
    for shrink in (1.0, 0.5):
        count, ro = both(uvz((8, 4, 1), (8.5, 4.5, 2)), EYE, SIZE, rows, shrink=shrink)
        assert count.tolist() == [0] * 7 + [2] and not ro[:7].view(np.uint32).any() and who(ro[7:]) == [(1, 1)]
    # an image without pixels, no points, no boxes
    assert not data.box_radar(good, EYE, (0, 16), whole)[0].any()
    count, ro = both(np.zeros((0, 7), F), EYE, SIZE, whole)
    assert count.tolist() == [0] and ro.shape == (1, 2, 5) and not ro.view(np.uint32).any()
    count, ro = both(good, EYE, SIZE, np.zeros((0, 7), F))
    assert count.shape == (0,) and ro.shape == (0, 2, 5)


def test_hand_computed_nearest_and_lower_median():
    whole = boxes((0, 0, 8, 16))
    depths = (16, 1, 4, 2, 8)                                             # ascending: points 2, 4, 3, 5, 1
    want = {0: (0, 0), 1: (1, 1), 2: (2, 2), 3: (2, 3), 4: (2, 4), 5: (2, 3)}
    #        count 2: rank 0, the median IS the nearest; 3: (2, 3, 1) -> 3; 4: (2, 4, 3, 1) -> 4, the LOWER median; 5: -> 3
    for n in range(6):
        count, ro = both(uvz(*[(3, 3, z) for z in depths[:n]]), EYE, SIZE, whole)
        assert count.tolist() == [n] and who(ro) == [want[n]], n
        if n:
            assert ro[0, :, 0].tolist() == [float(depths[want[n][0] - 1]), float(depths[want[n][1] - 1])]
    # equal depths go to the lower index: (2, 2, 2, 1, 2) in key order is points 4, 1, 2, 3, 5
    count, ro = both(uvz((3, 3, 2), (4, 4, 2), (5, 5, 2), (6, 6, 1), (7, 7, 2)), EYE, SIZE, whole)
    assert count.tolist() == [5] and who(ro) == [(4, 2)]
    count, ro = both(uvz((3, 3, 2), (4, 4, 2), (5, 5, 2)), EYE, SIZE, whole)
    assert count.tolist() == [3] and who(ro) == [(1, 2)]
    # a point inside two overlapping boxes is a candidate of each
    pts = uvz((2, 2, 4), (6, 3, 2), (12, 5, 1))
    count, ro = both(pts, EYE, SIZE, boxes((0, 0, 4, 8), (1, 4, 7, 14), (0, 0, 1, 1)))
    assert count.tolist() == [2, 2, 0] and who(ro) == [(2, 2), (3, 3), (0, 0)]
    # feature bits are copied: NaN payloads, infinities, -0.0, a denormal
    pts = uvz((3, 3, 1), (3, 3, 2), (3, 3, 4))
    pts[0, 3:7].view(np.uint32)[:] = (0x7FC01234, 0xFFC00001, 0x7F800000, 0x80000000)
    pts[1, 3:7].view(np.uint32)[:] = (0x7FC0BEEF, 0xFFFFFFFF, 0xFF800000, 0x00000001)
    count, ro = data.box_radar(pts, EYE, SIZE, whole)
    assert same((count, ro), loop_box_radar(pts, EYE, SIZE, whole)) and count.tolist() == [3]
    assert ro[0, 0].view(np.uint32).tolist() == [0x3F800000, 0x7FC01234, 0xFFC00001, 0x7F800000, 0x80000000]
    assert ro[0, 1].view(np.uint32).tolist() == [0x40000000, 0x7FC0BEEF, 0xFFFFFFFF, 0xFF800000, 0x00000001]


def test_hand_computed_shrink():
    # shrink = 1 uses the row's own numbers: the centre form would round this top edge, 1 + 2^-23, to (8) 0.5 - (6) 0.5 = 1
    t, b = F(1) + F(2) ** -23, F(7)
    assert (t + b) * F(0.5) - ((b - t) * F(0.5)) * F(1) == F(1) and t > F(1)
    pts = uvz((8, t, 1), (8, 1, 1))
    count, _ = both(pts, EYE, SIZE, boxes((t, 0, b, 16)), shrink=1.0)
    assert count.tolist() == [1]                                          # v = 1 is above the top edge as the row has it
    # shrink = 0.5 keeps the centre: (0, 0, 8, 16) -> [2, 6) x [4, 12)
    pts = uvz((4, 2, 1), (12, 3, 2), (8, 6, 2), (np.nextafter(F(12), F(0)), np.nextafter(F(6), F(0)), 4), (3.5, 4, 1), (8, 1.5, 1))
    count, ro = both(pts, EYE, SIZE, boxes((0, 0, 8, 16)), shrink=0.5)
    assert count.tolist() == [2] and who(ro) == [(1, 1)]
    count, ro = both(pts, EYE, SIZE, boxes((0, 0, 8, 16)), shrink=1.0)
    assert count.tolist() == [6] and who(ro) == [(1, 6)]                  # depths 1, 1, 1, 2, 2, 4 by index: rank 2 is point 6
    # shrink = 0.25 of an odd box, every step rounded on its own: the loop is the witness
    both(cloud(5, 300), camera((48, 100)), (48, 100), boxes((3.3, 7.7, 40.1, 90.9), (10, 10, 11, 11)), shrink=0.25)


def test_random_rigs_equal_the_plain_loop():
    rs = np.random.RandomState(7)
    members = 0
    for k, size in enumerate([(48, 100), (120, 60), (64, 96)]):
        ih, iw = size
        pts = cloud(20 + k, 500)
        pts[::50, 2] = pts[1::50, 2][:len(pts[::50])]                     # pairs of equal depth
        tl = rs.uniform(-0.2, 0.7, (8, 2)) * (ih, iw)
        br = tl + rs.uniform(0.1, 0.8, (8, 2)) * (ih, iw)
        rows = boxes(*np.concatenate([tl, br], 1).astype(F))
        for shrink, md in ((1.0, 0.1), (0.5, 0.1), (0.8, 0.5)):
            count, _ = both(pts, camera(size), size, rows, min_depth=md, shrink=shrink)
            members += int(count.sum())
    assert members > 1000


def test_validation_errors():
    pts, rows = uvz((3, 3, 1)), boxes((0, 0, 8, 16))
    for kw, match in ((dict(min_depth=0.0), "min_depth"), (dict(min_depth=float("nan")), "min_depth"), (dict(shrink=0.0), "shrink"),
                      (dict(shrink=1.5), "shrink"), (dict(shrink=float("nan")), "shrink"), (dict(shrink=-0.5), "shrink"),
                      (dict(shrink=None), "shrink"), (dict(shrink=True), "shrink")):
        with pytest.raises(RuntimeError, match=match):
            data.box_radar(pts, EYE, SIZE, rows, **kw)
    with pytest.raises(RuntimeError, match="float32"):
        data.box_radar(pts.astype(np.float64), EYE, SIZE, rows)
    with pytest.raises(RuntimeError, match=r"\(n, 7\)"):
        data.box_radar(pts[:, :6], EYE, SIZE, rows)
    with pytest.raises(RuntimeError, match=r"\(3, 4\)"):
        data.box_radar(pts, np.eye(4, dtype=F), SIZE, rows)
    with pytest.raises(RuntimeError, match=r"\(3, 4\)"):
        data.box_radar(pts, EYE.astype(np.float64), SIZE, rows)
    with pytest.raises(RuntimeError, match="rows are"):
        data.box_radar(pts, EYE, SIZE, rows[:, :3])
    with pytest.raises(RuntimeError, match="rows are"):
        data.box_radar(pts, EYE, SIZE, rows.astype(np.float64))
    with pytest.raises(RuntimeError, match="rows are"):
        data.box_radar(pts, EYE, SIZE, rows[0])


def membership(points, P, size, rows, min_depth, shrink, dt):
    """The rule's (box, point) membership matrix, every number and operation in `dt`."""
    ih, iw = size
    p, P, rows = points[:, :3].astype(dt), P.astype(dt), rows[:, :4].astype(dt)
    with np.errstate(all="ignore"):
        hu, hv, hw = (((P[r, 0] * p[:, 0] + P[r, 1] * p[:, 1]) + P[r, 2] * p[:, 2]) + P[r, 3] for r in range(3))
        ok = (hw >= dt(F(min_depth))) & np.isfinite(hw) & np.isfinite(hu) & np.isfinite(hv)
        den = np.where(ok, hw, dt(1))
        u, v = hu / den, hv / den
        assert u.dtype == dt
        ok &= (u >= 0) & (u < dt(iw)) & (v >= 0) & (v < dt(ih))
        t, l, b, rt = (rows[:, k, None] for k in range(4))
        if F(shrink) != 1:
            s, half = dt(F(shrink)), dt(0.5)
            cy, cx, hy, hx = (t + b) * half, (l + rt) * half, ((b - t) * half) * s, ((rt - l) * half) * s
            t, b, l, rt = cy - hy, cy + hy, cx - hx, cx + hx
        return ok[None] & (l <= u) & (u < rt) & (t <= v) & (v < b)


def test_float32_rule_agrees_with_float64_on_all_but_1e_4_of_the_member_pairs():
    rs = np.random.RandomState(2025)
    members = differ = 0
    for k in range(200):
        size = ih, iw = (int(rs.randint(32, 720)), int(rs.randint(32, 1280)))
        P = camera(size, f=rs.uniform(0.5, 1.5), t=rs.uniform(-1, 1, 3))
        pts = cloud(3000 + k, 4096, spread=rs.uniform(0.3, 1.2))
        tl = rs.uniform(-0.1, 0.6, (8, 2)) * (ih, iw)
        br = tl + rs.uniform(0.2, 0.9, (8, 2)) * (ih, iw)
        rows = boxes(*np.concatenate([tl, br], 1).astype(F))
        shrink = 1.0 if k % 2 else float(rs.uniform(0.3, 1.0))
        m32 = membership(pts, P, size, rows, 0.1, shrink, F)
        m64 = membership(pts, P, size, rows, 0.1, shrink, np.float64)
        count, _ = data.box_radar(pts, P, size, rows, 0.1, shrink)
        assert np.array_equal(count, m32.sum(1))                          # the matrix is the rule's
        members += int((m32 | m64).sum())
        differ += int((m32 != m64).sum())
    print(f"float32 against float64: {differ} of {members} member pairs differ")
    assert members > 100000
    assert differ < 1e-4 * members                                        # measured with this seed: see DESIGN 3.13a


class Stub:
    """What `predict_dir` and `radar_readout` read of a result, on the host."""


def test_radar_readout_and_the_text_of_predict_dir():
    B, cap = 2, 3
    rows = torch.zeros((B, cap, 7))
    rows[0, 0] = torch.tensor([10.5, 20.25, 30.0, 40.0, 0.9, 0.5, 2.0])
    rows[1, 0] = torch.tensor([1.0, 2.0, 3.0, 4.0, 1.0, 0.25, 0.0])
    rows[1, 1] = torch.tensor([5.0, 6.0, 7.0, 8.0, 0.5, 0.5, 3.0])
    kept = torch.tensor([1, 2], dtype=torch.int32)
    points = torch.tensor([[7, 0, 0], [0, 16777216, 0]], dtype=torch.int32)
    readout = torch.zeros((B, cap, 2, 5))
    readout[0, 0] = torch.tensor([[12.5, 1, 2, 3, 4], [0.1, -1, -2, -3, -4]])
    readout[1, 1] = torch.tensor([[3.0, 0.5, 0.25, 0.125, 1e-3], [4.0, 5, 6, 7, 8]])
    readout[0, 0, 0, 1:].view(torch.int32)[0] = 0x7FC01234                  # a NaN payload travels
    res = infer.FrameResult(rows, kept, None, None, None, None, torch.zeros(1, dtype=torch.int32), box_points=points, box_radar=readout)
    got = res.radar_readout()
    assert [g.shape for g in got] == [(1, 11), (2, 11)] and all(g.dtype == F for g in got)
    assert got[0][0, 0] == 7 and got[1][:, 0].tolist() == [0.0, 16777216.0]
    assert got[0][0, 1:].view(np.int32).tolist() == readout[0, 0].reshape(-1).view(torch.int32).tolist()
    assert np.array_equal(got[1][:, 1:], readout[1, :2].reshape(2, 10).numpy())
    dets = res.detections()
    text = infer.radar_text(dets[1], got[1])
    assert text == ("0 0.25 2 1 4 3 0 0 0 0 0 0 0 0 0 0 0\n"
                    "3 0.25 6 5 8 7 16777216 3 0.5 0.25 0.125 0.00100000005 4 5 6 7 8\n")
    line = infer.radar_text(dets[0], got[0]).split()
    assert line[:8] == ["2", "0.449999988", "20.25", "10.5", "40", "30", "7", "12.5"] and line[8] == "nan" and len(line) == 17
    assert [F(v) for v in line[9:]] == [2, 3, 4, F(0.1), -1, -2, -3, -4]
    assert infer.radar_text(np.zeros((0, 7), F), np.zeros((0, 11), F)) == ""
    with pytest.raises(RuntimeError, match="radar_text"):
        infer.radar_text(dets[1], got[0])
    plain = infer.FrameResult(rows, kept, None, None, None, None, None)
    assert plain.box_points is None and plain.box_radar is None
    with pytest.raises(RuntimeError, match="not built with box_radar"):
        plain.radar_readout()


def test_pipeline_arguments_that_need_no_device():
    class Eval:
        training = False
    for kw, match in ((dict(box_radar=True), "box_radar reads the radar POINTS"), (dict(box_shrink=0.5), "box_shrink belongs to box_radar"),
                      (dict(radar_points=10, box_shrink=0.5), "box_shrink belongs to box_radar"),
                      (dict(radar_points=10, box_radar=True, box_shrink=0.0), "shrink"),
                      (dict(radar_points=10, box_radar=True, box_shrink=1.5), "shrink"),
                      (dict(radar_points=10, box_radar=True, box_shrink=float("nan")), "shrink")):
        with pytest.raises(RuntimeError, match=match):
            infer.FramePipeline(Eval(), (48, 64), (64, 64), batch=2, **kw)


def test_exports_exist_and_the_abi_stays_11():
    from asy_vrnet_amd import hip
    assert hip.ABI_VERSION == 11
    assert "vrnet_box_radar_f32" in hip.EXPORTED and "vrnet_box_radar_workspace" in hip.EXPORTED
    assert hip.box_radar_workspace_bytes(3, 300) >= 3 * 300 * 12 and hip.box_radar_workspace_bytes(1, (1 << 24) + 1) == -1
    assert hip.box_radar_workspace_bytes(0, 10) == -1
    for name in ("box_radar", "device_box_radar", "check_box_shrink"):
        assert callable(getattr(data, name))
