"""Radar points under Mosaic on the GPU: vrnet_mosaic_radar_points_f32 against `data.mosaic_radar_map` (the host statement,
itself held to `data.radar_map` by tests/test_mosaic_points_host.py), `data.device_mosaic_radar_map`, and
`graph.TrainStep(from_frames=True, mosaic=..., radar_points=..., calib=...)`.  Both sides are the same float32 operations
without contraction and an order-independent integer minimum, so every comparison is bit for bit, as uint32.
Shapes: a 40 x 56 canvas, two output images, eight sources of mixed sizes in 96 x 112 slots, 300 points per source (two
workgroups of points per tile, the second partly filled); the step: nano, 64 x 64, B = 2."""
import numpy as np
import pytest
import torch

from tests import mosaic_points_cases as C

pytestmark = pytest.mark.gpu

H, W = C.CANVAS
NSRC = len(C.SIZES)
IDENTITY = np.array([[1, 0, 0, 0], [0, 1, 0, 0], [0, 0, 1, 0]], np.float32)


@pytest.fixture(scope="module")
def A():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    import asy_vrnet_amd
    return asy_vrnet_amd


def cuda(a):
    return (a if torch.is_tensor(a) else torch.from_numpy(np.ascontiguousarray(a))).cuda()


def new_flag():
    return torch.zeros(1, dtype=torch.int32, device="cuda")


def launch(points, P, table, radius, input_shape=C.CANVAS, counts=None, max_points=C.MAX_POINTS, min_depth=0.1, **kw):
    """hip.mosaic_radar_points on packed points; counts: what the source table says instead of the points' own counts.
    Returns (out (B, 4, H, W) on the host as uint32, flag word)."""
    from asy_vrnet_amd import data, hip
    packed, own = data.pack_points(points, max_points)
    sources = data.radar_sources(P, own.numpy() if counts is None else np.asarray(counts, np.int32))
    h, w = input_shape
    out = kw.pop("out", None)
    if out is None:
        out = torch.full((len(table), 4, h, w), 7.0, dtype=torch.float32, device="cuda")
    flag = new_flag()
    hip.mosaic_radar_points(cuda(packed), cuda(data.radar_source_bytes(sources)), cuda(data.mosaic_bytes(np.ascontiguousarray(table))), C.CAP,
                            h, w, radius, min_depth, out, flag=flag, **kw)
    return C.bits(out.cpu().numpy()), int(flag.item())


_HOST = {}


def host(points, P, table, radius, key, sizes=C.SIZES, input_shape=C.CANVAS):
    """`data.mosaic_radar_map` per record, computed once per key and shared, as uint32."""
    from asy_vrnet_amd import data
    if key not in _HOST:
        _HOST[key] = np.stack([C.bits(data.mosaic_radar_map(points, P, sizes, input_shape, rec, radius)) for rec in table])
        _HOST[key].setflags(write=False)
    return _HOST[key]


# ---- 1. the kernel against the host statement -------------------------------------------------------------------------------
@pytest.mark.parametrize("radius", [0, 1, 3])
@pytest.mark.parametrize("name", C.NAMES)
def test_kernel_equals_mosaic_radar_map(A, name, radius):
    """Every record of C.tables; clouds with NaN and Inf coordinates, points behind min_depth, equal depths on one pixel and
    NaN payloads (C.point_sets).  A quadrant expected to receive 50 points holds at least 20 non-zero pixels: an all-zero map
    cannot pass."""
    pts, P, table = C.point_sets(7), C.calib(), C.tables()[name]
    want = host(pts, P, table, radius, ("full", name, radius))
    got, flag = launch(pts, P, table, radius)
    assert flag == 0
    assert np.array_equal(got, want), (name, radius, int((got != want).sum()))
    for b, rec in enumerate(table):
        for t in range(4):
            if C.expected_points(rec, t) >= C.MIN_EXPECTED:
                assert C.nonzero_pixels(got[b].view(np.float32), C.shown(rec, t)) >= 20, (name, b, t)
    payload = (want >= C.NAN_PAYLOAD) & (want < C.NAN_PAYLOAD + 20)
    if name == "interior" and radius == 3:
        assert payload.any()                                     # a NaN payload reached the map, bit for bit


@pytest.mark.parametrize("radius", [0, 2])
def test_counts_zero_one_and_max_points(A, radius):
    counts = [C.MAX_POINTS, 0, 1, C.MAX_POINTS, 0, 1, C.MAX_POINTS, C.MAX_POINTS]
    pts, P = C.point_sets(8, counts), C.calib()
    for name in ("interior", "edge"):
        table = C.tables()[name]
        got, flag = launch(pts, P, table, radius)
        assert flag == 0 and np.array_equal(got, host(pts, P, table, radius, ("counts", name, radius)))
        for b, rec in enumerate(table):
            for t in range(4):
                if counts[int(rec["tile"][t]["src"])] == 0 and C.shown(rec, t):
                    assert C.nonzero_pixels(got[b].view(np.float32), C.shown(rec, t)) == 0


def test_the_lowest_index_wins_equal_depths(A):
    """Rows 10..14 of a cloud repeat row 5's position with other features: wherever row 5 wins on the host, the kernel shows
    row 5's features, never a copy's."""
    from asy_vrnet_amd import data
    pts, P = C.point_sets(7), C.calib()
    rec = data.mosaic_record(C.CANVAS, (W, H), [(2, C.SIZES[2], 56, 40, 0, 0, 0), None, None, None])
    only = [np.concatenate([pts[2][5:6], pts[2][10:15]]) if k == 2 else None for k in range(NSRC)]
    got, flag = launch(only, P, np.stack([rec]), 1)
    assert flag == 0 and np.array_equal(got, host(only, P, np.stack([rec]), 1, "ties"))
    seen = np.unique(got[0, 0][got[0, 0] != 0])
    assert seen.tolist() == [int(C.bits(pts[2][5, 3:4])[0])]


# ---- 2. contention and statelessness ---------------------------------------------------------------------------------------
def pile(rng, ix, iy, n=256):
    """n points on window pixel (ix, iy) of a 1:1 window under IDENTITY, at shuffled depths with ties."""
    z = rng.permutation(np.repeat(np.linspace(1.0, 9.0, n // 4, dtype=np.float32), 4))
    pts = np.zeros((n, 7), np.float32)
    pts[:, 0], pts[:, 1], pts[:, 2] = (ix + 0.5) * z, (iy + 0.5) * z, z
    pts[:, 3:] = rng.standard_normal((n, 4))
    return pts


def four_tiles():
    """Four 20 x 30 sources shown 1:1, one per quadrant of a cut at (26, 19)."""
    from asy_vrnet_amd import data
    size = (20, 30)
    rec = data.mosaic_record(C.CANVAS, (26, 19), [(0, size, 30, 20, 0, 0, 0), (1, size, 30, 20, 0, 19, 1), (2, size, 30, 20, 26, 19, 0),
                                                  (3, size, 30, 20, 26, 0, 1)])
    return np.stack([rec, rec]), [size] * 4


def test_256_points_on_one_pixel_per_quadrant_twice_and_then_other_points(A):
    from asy_vrnet_amd import hip
    table, sizes = four_tiles()
    rng = np.random.default_rng(11)
    first = [pile(rng, 8 + k, 4 + k) for k in range(4)]
    second = [pile(rng, 15 - k, 9 + k) for k in range(4)]
    ws = torch.empty(hip.mosaic_radar_points_workspace_bytes(2, H, W), dtype=torch.uint8, device="cuda")
    want = host(first, IDENTITY, table, 2, "pile 1", sizes)
    a, fa = launch(first, IDENTITY, table, 2, max_points=256, ws=ws)
    b, fb = launch(first, IDENTITY, table, 2, max_points=256, ws=ws)
    assert fa == fb == 0 and np.array_equal(a, want) and np.array_equal(a, b)
    for t in range(4):                                           # 25 pixels per pile, all inside the quadrant
        assert C.nonzero_pixels(a[0].view(np.float32), C.shown(table[0], t)) == 25
    c, fc = launch(second, IDENTITY, table, 2, max_points=256, ws=ws)
    want2 = host(second, IDENTITY, table, 2, "pile 2", sizes)
    assert fc == 0 and np.array_equal(c, want2) and not np.array_equal(want, want2)


# ---- 3. bad records, bad counts, bad arguments --------------------------------------------------------------------------------
def test_bad_source_and_counts_set_their_bits_and_zero_what_is_theirs(A):
    """A src outside [-1, S) makes the record one that mos_load calls bad: as in every Mosaic kernel the WHOLE output image of
    that record is what an empty record gives (zero) and FLAG_GEOMETRY is set; the other image is untouched.  A count above
    max_points is clamped (the buffer's rows all count), a negative one is 0 and empties only the quadrants of the tiles
    that name that source; both set FLAG_POINT_COUNT and nothing else."""
    from asy_vrnet_amd import hip
    pts, P = C.point_sets(7), C.calib()
    table = C.tables()["interior"]
    want = host(pts, P, table, 1, ("full", "interior", 1))
    bad = table.copy()
    bad[0]["tile"][1]["src"] = NSRC
    got, flag = launch(pts, P, bad, 1)
    assert flag == hip.FLAG_GEOMETRY
    assert not got[0].any() and np.array_equal(got[1], want[1])
    bad[0]["tile"][1]["src"] = -2
    got, flag = launch(pts, P, bad, 1)
    assert flag == hip.FLAG_GEOMETRY and not got[0].any() and np.array_equal(got[1], want[1])
    counts = [C.MAX_POINTS] * NSRC
    counts[2] = C.MAX_POINTS + 1000
    got, flag = launch(pts, P, table, 1, counts=counts)
    assert flag == hip.FLAG_POINT_COUNT and np.array_equal(got, want)
    counts[2], counts[5] = C.MAX_POINTS, -4
    got, flag = launch(pts, P, table, 1, counts=counts)
    assert flag == hip.FLAG_POINT_COUNT
    x0, x1, y0, y1 = C.shown(table[1], 1)                        # source 5 is tile 1 of image 1
    assert not got[1][:, y0:y1, x0:x1].any() and want[1][:, y0:y1, x0:x1].any()
    rest = want.copy()
    rest[1][:, y0:y1, x0:x1] = 0
    assert np.array_equal(got, rest)
    counts[5], counts[6] = C.MAX_POINTS, 2 ** 31 - 1
    bad = table.copy()
    bad[0]["cutx"] = W + 1
    got, flag = launch(pts, P, bad, 1, counts=counts)
    assert flag == hip.FLAG_GEOMETRY | hip.FLAG_POINT_COUNT and not got[0].any() and np.array_equal(got[1], want[1])


def test_argument_errors_come_before_any_launch(A):
    from asy_vrnet_amd import hip
    pts, P, table = C.point_sets(7), C.calib(), C.tables()["interior"]
    need = hip.mosaic_radar_points_workspace_bytes(2, H, W)
    assert need >= 2 * H * W * 8 and need % 8 == 0
    out = torch.full((2, 4, H, W), 7.0, dtype=torch.float32, device="cuda")
    big = torch.empty(need + 16, dtype=torch.uint8, device="cuda")
    for kw, match in ((dict(ws=big[:need - 8]), "workspace"), (dict(ws=big[1:need + 1]), "8-byte aligned"), (dict(radius=9), "radius"),
                      (dict(min_depth=0.0), "min_depth"), (dict(min_depth=float("inf")), "min_depth")):
        args = dict(radius=1, out=out)
        args.update(kw)
        with pytest.raises(RuntimeError, match="mosaic_radar_points.*" + match):
            launch(pts, P, table, **args)
    torch.cuda.synchronize()
    assert (out == 7.0).all()
    with pytest.raises(RuntimeError, match="source table"):
        from asy_vrnet_amd import data
        hip.mosaic_radar_points(torch.zeros((NSRC, 8, 7), device="cuda"), torch.zeros((NSRC - 1, 56), dtype=torch.uint8, device="cuda"),
                                cuda(data.mosaic_bytes(table)), C.CAP, H, W, 0, 0.1, out)
    with pytest.raises(RuntimeError, match="Mosaic table"):
        hip.mosaic_radar_points(torch.zeros((NSRC, 8, 7), device="cuda"), torch.zeros((NSRC, 56), dtype=torch.uint8, device="cuda"),
                                torch.zeros((2, 80), dtype=torch.uint8, device="cuda"), C.CAP, H, W, 0, 0.1, out)


# ---- 4. the stand-alone batch call ---------------------------------------------------------------------------------------------
def test_device_mosaic_radar_map_equals_the_host_statement(A):
    from asy_vrnet_amd import data
    pts, P = C.point_sets(7), C.calib()
    for name in ("interior", "gaps"):
        table = C.tables()[name]
        flag = new_flag()
        got = data.device_mosaic_radar_map(pts, C.SIZES, C.CANVAS, P, table, radius=1, flag=flag)
        assert got.dtype == torch.float32 and tuple(got.shape) == (2, 4, H, W)
        assert np.array_equal(C.bits(got.cpu().numpy()), host(pts, P, table, 1, ("full", name, 1))) and int(flag.item()) == 0
    wrong = C.tables()["interior"].copy()
    wrong[1]["tile"][2]["src"] = NSRC
    with pytest.raises(RuntimeError, match="device_mosaic_radar_map: image 1, tile 2: source 8"):
        data.device_mosaic_radar_map(pts, C.SIZES, C.CANVAS, P, wrong)
    with pytest.raises(RuntimeError, match="image 0 has 300 points"):
        data.device_mosaic_radar_map(pts, C.SIZES, C.CANVAS, P, table, max_points=299)


# ---- 5. the captured step ------------------------------------------------------------------------------------------------------
B, S, NC, NS = 2, 64, 4, 9
MAX_GT = 8
BOXES = [
    np.array([[3, 5, 41, 33, 0], [50, 20, 200, 100, 3]]),
    np.array([[4, 8, 50, 70, 0], [10, 40, 55, 88, 2]]),
    np.zeros((0, 5), np.int64),
    np.array([[0, 0, 111, 37, 1], [20, 5, 24, 9, 2]]),
    np.array([[0, 0, 112, 96, 3], [13, 17, 59, 61, 1], [30, 20, 33, 90, 0]]),
    np.array([[2, 3, 25, 18, 1]]),
    np.array([[5, 10, 35, 90, 2], [0, 0, 40, 96, 0]]),
    None,
]


def trainer(A, seed=5):
    from asy_vrnet_amd import losses, optim
    m = A.EfficientVRNet(NC, NS, "nano", img_size=(S, S)).cuda().train()
    A.randomize_state_dict(m.state_dict(), seed=seed)
    return m, losses.YOLOLoss(NC).cuda(), optim.build_optimizer(m, "sgd", 1e-2, 0.937, 5e-4), optim.ModelEMA(m)


def raw_batch(seed):
    rng = np.random.default_rng(seed)
    frames = [rng.integers(0, 256, (ih, iw, 3), dtype=np.uint8) for ih, iw in C.SIZES]
    labels = [rng.integers(0, NS, (ih, iw), dtype=np.uint8) for ih, iw in C.SIZES]
    return frames, labels


@pytest.fixture(scope="module")
def step(A):
    from asy_vrnet_amd.graph import TrainStep
    t = trainer(A)
    return TrainStep(t[0], t[1], t[2], t[3], B, S, NS, max_gt=MAX_GT, from_frames=True, capacity=C.CAP, mosaic=True, aug_seed=3,
                     radar_points=C.MAX_POINTS, radar_radius=1, calib=C.calib())


def step_radar(step):
    return C.bits(step.r.cpu().numpy())


def test_step_buffers_are_points_and_a_source_table(A, step):
    from asy_vrnet_amd import hip
    assert tuple(step.points.shape) == (4 * B, C.MAX_POINTS, 7) and tuple(step.views.shape) == (4 * B, hip.RADAR_SOURCE_BYTES)
    assert not hasattr(step, "radar_in") and step.sources == 4 * B
    assert step._radar_ws.numel() == hip.mosaic_radar_points_workspace_bytes(B, S, S)


def test_step_radar_equals_the_host_statement_over_explicit_tables(A, step):
    graphs = [id(g) for g in step.graphs]
    P = C.calib()
    for it, name in enumerate(("interior", "gaps")):
        table = C.tables((S, S))[name]
        frames, labels = raw_batch(40 + it)
        pts = C.point_sets(50 + it)
        res = step(frames, pts, BOXES, labels, aug=table)
        assert all(bool(torch.isfinite(v)) for v in res.values())
        want = host(pts, P, table, 1, ("step", name), input_shape=(S, S))
        assert np.array_equal(step_radar(step), want) and want.any()
        assert step.aug_table.tobytes() == table.tobytes()
    assert [id(g) for g in step.graphs] == graphs                # no new capture
    st = step.stats()
    assert st["flag"] == 0 and np.isfinite(st["total"])


def test_step_radar_under_drawn_tables_and_a_per_call_projection(A, step):
    from asy_vrnet_amd import data
    frames, labels = raw_batch(42)
    pts = C.point_sets(52)
    P = C.calib()
    for prob in (1.0, 0.0):
        step.mosaic_prob = prob
        step(frames, pts, BOXES, labels)
        table = step.aug_table.copy()
        assert ((table["tile"]["src"][:, 1:] == -1).all()) == (prob == 0.0)
        want = np.stack([C.bits(data.mosaic_radar_map(pts, P, C.SIZES, (S, S), rec, 1)) for rec in table])
        assert np.array_equal(step_radar(step), want) and want.any()
    step.mosaic_prob = 1.0
    other = P.copy()                                             # (4 B, 3, 4), one per source: a shifted principal point
    other[:, 0, 2] += 3.0
    other[:, 1, 2] -= 2.0
    table = C.tables((S, S))["interior"]
    step(frames, pts, BOXES, labels, aug=table, calib=other)
    want = np.stack([C.bits(data.mosaic_radar_map(pts, other, C.SIZES, (S, S), rec, 1)) for rec in table])
    assert np.array_equal(step_radar(step), want)
    assert not np.array_equal(want, host(pts, P, table, 1, ("step", "other"), input_shape=(S, S)))
    step(frames, pts, BOXES, labels, aug=table)                  # and the constructor's projection is back
    assert np.array_equal(step_radar(step), host(pts, P, table, 1, ("step", "other"), input_shape=(S, S)))
    assert step.stats()["flag"] == 0


def test_step_errors_name_the_source_and_leave_the_step_alone(A, step):
    frames, labels = raw_batch(43)
    pts = C.point_sets(53)
    before = step.points.clone(), step.views.clone(), step.stats()["steps"]
    many = list(pts)
    many[6] = np.zeros((C.MAX_POINTS + 1, 7), np.float32)
    with pytest.raises(RuntimeError, match="image 1, tile 2 has 301 points"):
        step(frames, many, BOXES, labels)
    with pytest.raises(RuntimeError, match="not finished maps"):
        step(frames, np.zeros((4 * B, 4, S, S), np.float32), BOXES, labels)
    with pytest.raises(RuntimeError, match="2 point sets for a batch of 8"):
        step(frames, pts[:2], BOXES, labels)
    with pytest.raises(RuntimeError, match=r"calib.*\(8, 3, 4\)"):
        step(frames, pts, BOXES, labels, calib=C.calib()[:B])
    torch.cuda.synchronize()
    assert torch.equal(before[0].view(torch.int32), step.points.view(torch.int32))       # as bits: the clouds hold NaNs
    assert torch.equal(before[1], step.views) and step.stats()["steps"] == before[2]


def test_the_prologue_launches_the_points_call_and_not_the_map_gather(A, step, monkeypatch):
    from asy_vrnet_amd import graph
    calls = []
    names = ("letterbox_ragged", "seg_targets_ragged", "box_targets_ragged", "batch_formats", "augment_frames", "augment_seg_targets",
             "augment_box_targets", "augment_radar", "mosaic_frames", "mosaic_seg_targets", "mosaic_box_targets", "mosaic_radar", "radar_map",
             "mosaic_radar_points")
    for name in names:
        def counted(*a, _f=getattr(graph.hip, name), _n=name, **k):
            calls.append(_n)
            return _f(*a, **k)
        monkeypatch.setattr(graph.hip, name, counted)
    step._prologue()
    torch.cuda.synchronize()
    assert calls == ["mosaic_frames", "mosaic_seg_targets", "mosaic_box_targets", "mosaic_radar_points"]


def test_the_constructor_asks_for_the_projection(A):
    from asy_vrnet_amd.graph import TrainStep
    t = trainer(A)
    with pytest.raises(RuntimeError, match="mosaic with radar_points needs calib= at construction"):
        TrainStep(t[0], t[1], t[2], t[3], B, S, NS, from_frames=True, capacity=C.CAP, mosaic=True, radar_points=64)
