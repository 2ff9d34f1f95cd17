"""The radar map from radar points on the GPU: vrnet_radar_map_f32 (csrc/radarmap.hip) against the host statement
`data.radar_map`, and the pipelines built with radar_points against the same pipelines fed the host's maps.  Both sides do the
same float32 operations without contraction and copy feature bits, so every comparison is bit for bit, on int32 views: NaN
features count.  Shapes: a 64 x 96 canvas (W no multiple of a wave), 300 points (two workgroups of the point pass, the second
partial); 4096 points on 16 pixels for the contention; pipelines and steps: nano, 64 x 64, B = 2."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

F = np.float32
H, W = CANVAS = (64, 96)
FRAMES = [(48, 100), (120, 60), (64, 96)]                  # (ih, iw): a window cut in y, one cut in x, the whole canvas
MAXP = 300
COUNTS = (0, 1, 300)
EYE = np.array([[1, 0, 0, 0], [0, 1, 0, 0], [0, 0, 1, 0]], F)          # hu = x, hv = y, hw = z: x / z is the pixel column


@pytest.fixture(scope="module")
def A():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    import asy_vrnet_amd
    from asy_vrnet_amd import data, hip  # noqa: F401  (A.data, A.hip below)
    return asy_vrnet_amd


def cuda(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def bits(a):
    a = a.detach().cpu().numpy() if torch.is_tensor(a) else np.asarray(a)
    assert a.dtype == np.float32
    return np.ascontiguousarray(a).view(np.int32)


def camera(size, f=0.9, t=(0.3, -0.2, 0.5)):
    ih, iw = size
    K = np.array([[f * iw, 0, iw / 2], [0, f * iw, ih / 2], [0, 0, 1]])
    return (K @ np.concatenate([np.eye(3), np.array(t, float)[:, None]], 1)).astype(F)


def cloud(seed, n, spread=1.0):
    rs = np.random.RandomState(seed)
    z = rs.uniform(-2, 40, n)
    xy = rs.uniform(-0.8, 0.8, (n, 2)) * spread * np.abs(z)[:, None]
    return np.concatenate([xy, z[:, None], rs.randn(n, 4)], 1).astype(F)


def pixel_points(seed, n, size):
    """n points under EYE for a frame of size (ih, iw), written as (pixel column u, pixel row v, depth z) -> (u z, v z, z):
    a random part that overshoots the frame on every side, and the special cases of the module docstring in front."""
    ih, iw = size
    rs = np.random.RandomState(seed)
    uvz = [
        (3.0, 2.0, 1.0), (0.0, 0.0, 2.0), (float(iw), 5.0, 1.0), (5.0, float(ih), 1.0),          # pixel and frame boundaries
        (np.nextafter(F(iw), F(0)), np.nextafter(F(ih), F(0)), 1.0), (-0.0, 3.0, 1.0), (iw / 2, ih / 2, 0.1875),
        (10.5, 7.5, 2.0), (10.5, 7.5, 0.5), (10.5, 7.5, 8.0),                                    # far, near, farther on one pixel
        (20.5, 9.5, 0.5), (20.5, 9.5, 4.0), (20.25, 9.25, 0.5), (20.75, 9.75, 0.5),              # near first; then equal depths
        (30.5, 11.5, -1.0), (30.5, 11.5, 0.0), (30.5, 11.5, 0.0625), (31.5, 11.5, 0.125),        # behind, at 0, below and above min_depth
        (0.5, 0.5, 1.0), (iw - 0.5, ih - 0.5, 1.0), (0.5, ih - 0.5, 3.0), (iw - 0.5, 0.5, 3.0),  # footprints over the window's corners
    ]
    pts = np.zeros((n, 7), F)
    k = len(uvz)
    for i, (u, v, z) in enumerate(uvz):
        pts[i, :3] = F(u) * F(z), F(v) * F(z), z
    z = np.where(rs.rand(n - k) < 0.1, -1.0, rs.choice([0.25, 0.5, 1.0, 2.0, 4.0, 16.0], n - k) * rs.choice([1.0, 1.0, 1.37], n - k))
    u, v = rs.uniform(-0.1 * iw, 1.1 * iw, n - k), rs.uniform(-0.1 * ih, 1.1 * ih, n - k)
    pts[k:, 0], pts[k:, 1], pts[k:, 2] = u * z, v * z, z
    pts[:, 3:] = rs.randn(n, 4)
    pts[k + 0, 0], pts[k + 1, 1], pts[k + 2, 2] = np.nan, np.inf, np.nan                          # rejected, each of them
    pts[k + 3, 2], pts[k + 4, 0] = np.inf, -np.inf
    feat = pts[:, 3:].view(np.uint32)
    feat[7] = (0x7FC01234, 0xFFC00001, 0x7F800000, 0x80000000)                                   # loses its pixel
    feat[8] = (0x7FC0BEEF, 0xFFFFFFFF, 0xFF800000, 0x00000001)                                   # wins it: NaN payloads, -Inf, a denormal
    feat[18] = (0xFFC00002, 0x7FA00000, 0x80000000, 0x7F7FFFFF)
    feat[6] = (0x7FC00006, 0xFFC00006, 0x7F800001, 0xFF800001)                                   # the nearest of all, mid-frame
    return pts


def view_table(A, windows, P, counts):
    """windows: per image (size, (nw, nh, dx, dy), flip)."""
    v = np.zeros(len(windows), A.data.RADAR_VIEW_DTYPE)
    for b, (size, win, flip) in enumerate(windows):
        v[b] = (size[0], size[1]) + tuple(win) + (int(flip), counts[b], np.asarray(P[b], F).reshape(12))
    return v


def host_maps(A, pts, views, radius, min_depth, counts=None):
    out = []
    for b, v in enumerate(views):
        n = int(v["count"]) if counts is None else counts[b]
        win = tuple(int(v[k]) for k in ("nw", "nh", "dx", "dy"))
        out.append(A.data.radar_map(pts[b, :n], v["P"].reshape(3, 4), (int(v["ih"]), int(v["iw"])), CANVAS, win, bool(v["flip"]),
                                    radius, min_depth))
    return np.stack(out)


_POINTS = {}


def batch_points(layout):
    """(3, MAXP, 7): image 0 brings nothing, image 1 one point, image 2 all 300, made for the frame size it has in this layout;
    the rows past each count are filled with values that would land, so that a read past the count shows."""
    if layout not in _POINTS:
        pts = np.stack([pixel_points(5, MAXP, (64, 96)), cloud(6, MAXP), pixel_points(7 + layout, MAXP, FRAMES[layout % 3])])
        pts[1, 0] = (0.1, 0.1, 5.0, 1.5, -2.5, 3.5, -4.5)
        _POINTS[layout] = pts
    return _POINTS[layout]


def layouts(A):
    """Four view tables: the letterbox windows of FRAMES rotated through the images, and an augmentation-like one (twice the
    canvas at negative offsets, flipped; a small window inside the canvas, flipped; a window over the right and bottom edges)."""
    data = A.data
    out = []
    for r in range(3):
        sizes = [FRAMES[(b + r + 1) % 3] for b in range(3)]             # image 2 has FRAMES[r]
        wins = [(s, data.letterbox_geometry(s[1], s[0], W, H), False) for s in sizes]
        out.append((wins, [camera(sizes[0]), camera(sizes[1]), EYE]))
    sizes = [FRAMES[0], FRAMES[1], FRAMES[0]]
    wins = [(sizes[0], (40, 30, 50, 20), True), (sizes[1], (70, 50, 40, 30), False), (sizes[2], (2 * W, 2 * H, -W // 2, -H // 3), True)]
    out.append((wins, [camera(sizes[0]), camera(sizes[1]), EYE]))
    return out


@pytest.mark.parametrize("radius", [0, 1, 3])
def test_kernel_equals_the_host_statement(A, radius):
    hip = A.hip
    flag = torch.zeros(1, dtype=torch.int32, device="cuda")
    ws = torch.empty(hip.radar_map_workspace_bytes(3, H, W), dtype=torch.uint8, device="cuda")
    out = torch.full((3, 4, H, W), 7.0, device="cuda")
    for k, (wins, P) in enumerate(layouts(A)):
        pts = batch_points(k)
        views = view_table(A, wins, P, COUNTS)
        got = hip.radar_map(cuda(pts), cuda(A.data.radar_view_bytes(views).numpy()), H, W, radius, 0.1, out, flag=flag, ws=ws)
        want = host_maps(A, pts, views, radius, 0.1)
        assert got is out and np.array_equal(bits(got), bits(want)), (k, radius)
        assert not want[0].any() and np.count_nonzero(want[1].any(0)) == (2 * radius + 1) ** 2
        lit = want[2].view(np.uint32).any(0)
        assert lit.sum() > 30 and np.isnan(want[2]).any()                  # the case is not empty, and a NaN feature won a pixel
        # the footprint reaches the window's edge and stops there
        nw, nh, dx, dy = wins[2][1]
        inside = np.zeros((H, W), bool)
        inside[max(dy, 0):max(dy + nh, 0), max(dx, 0):max(dx + nw, 0)] = True
        inside = inside[:, ::-1] if wins[2][2] else inside
        assert not lit[~inside].any() and (lit & inside)[max(dy, 0)].any()
    assert int(flag.item()) == 0
    # data.device_radar_map: the same through the packing helpers, under the letterbox windows
    sizes = [w[0] for w in layouts(A)[0][0]]
    pts = batch_points(0)
    items = [pts[b, :n] for b, n in enumerate(COUNTS)]
    got = A.data.device_radar_map(items, sizes, CANVAS, np.stack(layouts(A)[0][1]), radius=radius, max_points=MAXP, flag=flag)
    assert np.array_equal(bits(got), bits(host_maps(A, pts, view_table(A, *layouts(A)[0], COUNTS), radius, 0.1)))
    assert int(flag.item()) == 0


def test_contention_and_no_state_between_calls(A):
    """4096 points of one image on 16 pixels (sixteen workgroups of the point pass on the same keys, depths from a set of
    eight, so most comparisons are ties that the index decides); then other points on the same workspace; then the first."""
    hip, data = A.hip, A.data
    rs = np.random.RandomState(11)
    n = 4096
    z = rs.choice([0.5, 0.75, 1.0, 1.5, 2.0, 3.0, 4.0, 8.0], n)
    u, v = 40 + rs.randint(0, 4, n) + rs.uniform(0.05, 0.95, n), 20 + rs.randint(0, 4, n) + rs.uniform(0.05, 0.95, n)
    first = np.concatenate([np.stack([u * z, v * z, z], 1), rs.randn(n, 4)], 1).astype(F)[None]
    other = np.zeros((1, n, 7), F)
    other[0, :50] = pixel_points(12, 50, CANVAS)
    other[0, 50:] = first[0, 50:]                              # past the count: never read
    ws = torch.empty(hip.radar_map_workspace_bytes(1, H, W), dtype=torch.uint8, device="cuda")
    whole = [(CANVAS, (W, H, 0, 0), False)]
    outs = []
    for pts, count in ((first, n), (other, 50), (first, n)):
        views = view_table(A, whole, [EYE], [count])
        out = torch.empty((1, 4, H, W), device="cuda")
        hip.radar_map(cuda(pts), cuda(data.radar_view_bytes(views).numpy()), H, W, 0, 0.1, out, ws=ws)
        want = host_maps(A, pts, views, 0, 0.1)
        assert np.array_equal(bits(out), bits(want))
        outs.append(bits(out))
    assert np.count_nonzero(outs[0].any(1)) == 16 and np.count_nonzero(outs[1].any(1)) > 16
    assert not (outs[1].any(1) & outs[0].any(1)).all() and np.array_equal(outs[0], outs[2])


def test_counts_are_clamped_and_bad_records_give_zero_maps(A):
    hip, data = A.hip, A.data
    wins, P = layouts(A)[2]
    pts = batch_points(2)
    flag = torch.zeros(1, dtype=torch.int32, device="cuda")

    def run(views):
        flag.zero_()
        out = torch.full((3, 4, H, W), 7.0, device="cuda")
        hip.radar_map(cuda(pts), cuda(data.radar_view_bytes(views).numpy()), H, W, 1, 0.1, out, flag=flag)
        return bits(out), int(flag.item())
    views = view_table(A, wins, P, (-1, 1, MAXP + 5))
    got, f = run(views)
    assert f == hip.FLAG_POINT_COUNT
    assert np.array_equal(got, bits(host_maps(A, pts, views, 1, 0.1, counts=(0, 1, MAXP))))
    # a zeroed record, and one without a window: zero maps, the other image as it was
    views = view_table(A, wins, P, (MAXP, 1, MAXP))
    good = bits(host_maps(A, pts, views, 1, 0.1))
    views[0] = np.zeros((), data.RADAR_VIEW_DTYPE)
    views[2]["nh"] = 0
    got, f = run(views)
    assert f == hip.FLAG_GEOMETRY and not got[0].any() and not got[2].any() and np.array_equal(got[1], good[1]) and good[0].any()
    views[0]["count"] = MAXP + 1
    assert run(views)[1] == hip.FLAG_GEOMETRY | hip.FLAG_POINT_COUNT
    # flag may be absent; the argument checks of the wrapper and the library
    out = torch.empty((3, 4, H, W), device="cuda")
    hip.radar_map(cuda(pts), cuda(data.radar_view_bytes(views).numpy()), H, W, 0, 0.1, out)
    good_views = cuda(data.radar_view_bytes(view_table(A, wins, P, COUNTS)).numpy())
    for kw, match in ((dict(radius=9), "radius"), (dict(min_depth=0.0), "min_depth"), (dict(min_depth=float("inf")), "min_depth")):
        args = dict(radius=0, min_depth=0.1)
        args.update(kw)
        with pytest.raises(RuntimeError, match=match):
            hip.radar_map(cuda(pts), good_views, H, W, args["radius"], args["min_depth"], out)
    with pytest.raises(RuntimeError, match="view table"):
        hip.radar_map(cuda(pts), good_views[:2], H, W, 0, 0.1, out)
    with pytest.raises(RuntimeError, match="workspace"):
        hip.radar_map(cuda(pts), good_views, H, W, 0, 0.1, out, ws=torch.empty(64, dtype=torch.uint8, device="cuda"))


# ---- the pipelines ------------------------------------------------------------------------------------------------------
NC, NS, S, B, K = 4, 9, 64, 2, 200
CAP = (80, 112)
RUN_SIZES = [[(40, 56), (80, 112)], [(61, 33), (48, 80)]]


def frame_points(seed, sizes):
    """Per image K / 2 .. K points spread over its frame under its own pinhole camera."""
    rs = np.random.RandomState(seed)
    return [cloud(seed + 10 * b, int(rs.randint(K // 2, K + 1)), 0.9) for b in range(len(sizes))], np.stack([camera(s) for s in sizes])


def frames_of(seed, sizes):
    rng = np.random.default_rng(seed)
    return [rng.integers(0, 256, (ih, iw, 3), dtype=np.uint8) for ih, iw in sizes]


def letterbox_maps(A, points, P, sizes, radius=0, letterbox_image=True):
    wins = [A.data.letterbox_geometry(iw, ih, S, S) if letterbox_image else (S, S, 0, 0) for ih, iw in sizes]
    return np.stack([A.data.radar_map(p, P[b], sizes[b], (S, S), wins[b], False, radius, 0.1) for b, p in enumerate(points)])


def test_frame_pipeline_with_points_equals_the_pipeline_fed_the_host_maps(A):
    model = A.EfficientVRNet(NC, NS, "nano", img_size=S).cuda().eval()
    A.randomize_state_dict(model.state_dict(), seed=4)
    kw = dict(batch=B, conf_thres=0.05, nms_thres=0.4, max_candidates=64, graph=True, ragged=True)
    maps = A.FramePipeline(model, CAP, (S, S), **kw)
    points = A.FramePipeline(model, CAP, (S, S), radar_points=K, radar_radius=1, **kw)
    assert points.graph is not None and tuple(points.points.shape) == (B, K, 7) and tuple(points.views.shape) == (B, 80)
    seen = []
    for k, sizes in enumerate(RUN_SIZES):
        frames = frames_of(40 + k, sizes)
        pts, P = frame_points(50 + k, sizes)
        host = letterbox_maps(A, pts, P, sizes, radius=1)
        assert np.count_nonzero(host) > 500
        want = maps.run(frames, host)
        want = [t.clone() for t in (want.rows, want.kept, want.det_counts, want.class_map, want.seg_counts, want.flag)]
        got = points.run(frames, pts, calib=P)
        assert np.array_equal(bits(points.radar), bits(host)), k
        for g, w in zip((got.rows, got.kept, got.det_counts, got.class_map, got.seg_counts, got.flag), want):
            assert g.dtype == w.dtype and torch.equal(g, w), k
        assert int(got.kept.max()) > 0 and np.asarray(got.sizes).tolist() == [list(s) for s in sizes]
        seen.append(bits(points.radar).copy())
    assert not np.array_equal(seen[0], seen[1])
    # a run enqueues and returns: no host synchronisation
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        got = points.run(frames, pts, calib=P)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    assert np.array_equal(bits(points.radar), seen[1]) and torch.equal(got.rows, want[0])
    # validated on the host before anything is enqueued: the static buffers stay as they are
    before = points.points.clone(), points.views.clone()
    with pytest.raises(RuntimeError, match="image 1 has"):
        points.run(frames, [pts[0], cloud(1, K + 1)], calib=P)
    with pytest.raises(RuntimeError, match="need a projection"):
        points.run(frames, pts)
    with pytest.raises(RuntimeError, match="calib belongs"):
        maps.run(frames, host, calib=P)
    torch.cuda.synchronize()
    assert torch.equal(before[0], points.points) and torch.equal(before[1], points.views)


def trainer(A, seed=5):
    from asy_vrnet_amd import losses, optim
    m = A.EfficientVRNet(NC, NS, "nano", img_size=(S, S)).cuda().train()
    A.randomize_state_dict(m.state_dict(), seed=seed)
    return m, losses.YOLOLoss(NC).cuda(), optim.build_optimizer(m, "sgd", 1e-2, 0.937, 5e-4), optim.ModelEMA(m)


STEP_BOXES = [np.array([[5, 4, 30, 30, 1], [10, 10, 50, 35, 3]]), np.array([[4, 8, 30, 40, 0], [20, 20, 22, 44, 1], [10, 5, 30, 33, 2]])]


def labels_of(seed, sizes):
    rng = np.random.default_rng(seed)
    return [rng.integers(0, NS + 3, (ih, iw), dtype=np.uint8) for ih, iw in sizes]


def test_train_step_with_points_equals_the_step_fed_the_host_maps(A):
    from asy_vrnet_amd.graph import TrainStep
    tm, tp = trainer(A), trainer(A)
    step_m = TrainStep(tm[0], tm[1], tm[2], tm[3], B, S, NS, max_gt=8, from_frames=True, capacity=CAP)
    step_p = TrainStep(tp[0], tp[1], tp[2], tp[3], B, S, NS, max_gt=8, from_frames=True, capacity=CAP, radar_points=K)
    assert not hasattr(step_p, "radar_in")
    for k, sizes in enumerate(RUN_SIZES):
        frames, labels = frames_of(60 + k, sizes), labels_of(70 + k, sizes)
        pts, P = frame_points(80 + k, sizes)
        host = letterbox_maps(A, pts, P, sizes)
        rm = step_m(frames, host, STEP_BOXES, labels)
        rp = step_p(frames, pts, STEP_BOXES, labels, calib=P)
        assert np.array_equal(bits(step_p.r), bits(host)) and np.count_nonzero(host) > 100, k
        assert rm.keys() == rp.keys() == {"total", "loss_det", "loss_seg"}
        assert all(torch.isfinite(rm[n]) and torch.equal(rm[n], rp[n]) for n in rm), (k, rm, rp)
    st = step_p.stats()
    assert st["steps"] == 2 and st["flag"] == 0
    with pytest.raises(RuntimeError, match="image 0 has"):
        step_p(frames, [cloud(1, K + 1), pts[1]], STEP_BOXES, labels, calib=P)
    with pytest.raises(RuntimeError, match="calib belongs"):
        step_m(frames, host, STEP_BOXES, labels, calib=P)


def test_augmenting_train_step_projects_the_points_into_each_record_s_window(A, monkeypatch):
    from asy_vrnet_amd import data, graph
    from asy_vrnet_amd.graph import TrainStep
    calls = []
    for name in ("augment_radar", "radar_map"):
        def counted(*a, _f=getattr(graph.hip, name), _n=name, **k):
            calls.append(_n)
            return _f(*a, **k)
        monkeypatch.setattr(graph.hip, name, counted)
    t = trainer(A)
    step = TrainStep(t[0], t[1], t[2], t[3], B, S, NS, max_gt=8, from_frames=True, capacity=CAP, augment=True, aug_seed=3,
                     radar_points=K, radar_radius=2, radar_min_depth=0.5)
    assert calls == ["radar_map"] * 3 and not hasattr(step, "radar_in")         # two warm-up passes and the capture
    records = [[((40, 56), 100, 70, -20, -3, True), ((80, 112), 30, 44, 10, 8, False)],
               [((61, 33), 128, 128, -32, -64, False), ((48, 80), 60, 20, 2, 40, True)]]
    for k, rows in enumerate(records):
        sizes = [r[0] for r in rows]
        table = np.stack([data.aug_record(size, (S, S), nw, nh, dx, dy, flip) for size, nw, nh, dx, dy, flip in rows])
        pts, P = frame_points(90 + k, sizes)
        res = step(frames_of(91 + k, sizes), pts, STEP_BOXES, labels_of(92 + k, sizes), aug=table, calib=P)
        want = np.stack([data.radar_map(pts[b], P[b], sizes[b], (S, S), rows[b][1:5], rows[b][5], 2, 0.5) for b in range(B)])
        assert np.array_equal(bits(step.r), bits(want)) and all(np.count_nonzero(w) > 100 for w in want), k
        assert torch.isfinite(res["total"])
    assert step.stats()["flag"] == 0


def test_eval_pipeline_with_points_equals_the_pipeline_fed_the_host_maps(A):
    model = A.EfficientVRNet(NC, NS, "nano", img_size=S).cuda().eval()
    A.randomize_state_dict(model.state_dict(), seed=4)
    names = [f"c{k}" for k in range(NC)]
    kw = dict(batch=B, capacity=4, max_boxes=4, max_gt=4, conf_thres=0.05, nms_thres=0.4, max_candidates=64, ragged=True)
    maps = A.EvalPipeline(model, CAP, (S, S), names, NS, **kw)
    points = A.EvalPipeline(model, CAP, (S, S), names, NS, radar_points=K, **kw)
    rng = np.random.default_rng(7)
    for k, sizes in enumerate(RUN_SIZES):
        frames = frames_of(40 + k, sizes)
        pts, P = frame_points(50 + k, sizes)
        labels = [rng.integers(0, NS, s, dtype=np.uint8) for s in sizes]
        gts = []
        for ih, iw in sizes:
            x1, y1 = rng.integers(0, iw - 12, 2), rng.integers(0, ih - 12, 2)
            gts.append(np.stack([x1, y1, x1 + rng.integers(4, 12, 2), y1 + rng.integers(4, 12, 2), rng.integers(0, NC, 2)], axis=1))
        ids = [f"{k}_{b}" for b in range(B)]
        maps.add(ids, frames, letterbox_maps(A, pts, P, sizes), labels, gts)
        points.add(ids, frames, pts, labels, gts, calib=P)
    want, got = maps.compute(strict=False), points.compute(strict=False)
    assert got.images == want.images == 4 and got.flag == want.flag
    assert int(want.det["n_det"].sum()) > 0
    for key in ("map", "ap", "f1", "recall", "precision", "lamr", "n_gt", "n_det", "n_tp"):
        g, w = got.det[key].cpu().numpy(), want.det[key].cpu().numpy()
        assert g.dtype == w.dtype and np.array_equal(g, w, equal_nan=g.dtype.kind == "f"), key
    assert np.array_equal(np.asarray(got.hist), np.asarray(want.hist)) and int(np.asarray(want.hist).sum()) > 0
    assert np.array_equal(got.miou, want.miou, equal_nan=True)
