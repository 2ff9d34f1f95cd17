"""The radar readout of the detections on the GPU: vrnet_box_radar_f32 (csrc/boxradar.hip) against the host statement
`data.box_radar`, and the pipelines built with box_radar against the same pipelines without it.  Both sides do the same float32
operations without contraction and copy feature bits, so every comparison is bit for bit, on int32 views: NaN features count.
Shapes: 300 points (two workgroups of the point pass, the second partial; more than one point a thread in the selection), 8
rows; 20 000 points in one box for the selection (the kernel keeps no list of candidates, so there is no capacity to pass:
the radix select alone answers); pipelines: nano, 64 x 64, B = 2."""
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

F = np.float32
FRAMES = [(48, 100), (120, 60), (64, 96)]                  # (ih, iw) of the three images: ragged
MAXP, COUNTS = 300, (0, 1, 300)
CAPR, KEPT = 8, (0, 3, 8)
EYE = np.array([[1, 0, 0, 0], [0, 1, 0, 0], [0, 0, 1, 0]], F)          # hu = x, hv = y, hw = z: x / z is the pixel column


@pytest.fixture(scope="module")
def A():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    import asy_vrnet_amd
    from asy_vrnet_amd import data, hip, infer  # noqa: F401  (A.data, A.hip, A.infer below)
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


def from_uvz(uvz, n, seed, size, exact):
    """n points under EYE: the (u, v, z) given in front, then random ones.  exact: every depth a power of two and every pixel
    inside the frame, so that ALL n are kept and in view at min_depth 0.1; otherwise the random part overshoots the frame on
    every side, lies partly behind the camera and has depths that round u and v."""
    ih, iw = size
    rs = np.random.RandomState(seed)
    pts = np.zeros((n, 7), F)
    k = len(uvz)
    for i, (u, v, z) in enumerate(uvz):
        pts[i, :3] = F(u) * F(z), F(v) * F(z), z
    m = n - k
    if exact:
        z = rs.choice([0.25, 0.5, 1.0, 2.0, 4.0, 16.0], m)
        u = np.minimum(rs.uniform(0, iw, m).astype(F), np.nextafter(F(iw), F(0)))
        v = np.minimum(rs.uniform(0, ih, m).astype(F), np.nextafter(F(ih), F(0)))
    else:
        z = np.where(rs.rand(m) < 0.1, -1.0, rs.choice([0.25, 0.5, 1.0, 2.0, 4.0, 16.0], m) * rs.choice([1.0, 1.0, 1.37], m))
        u, v = rs.uniform(-0.1 * iw, 1.1 * iw, m).astype(F), rs.uniform(-0.1 * ih, 1.1 * ih, m).astype(F)
    pts[k:, 0], pts[k:, 1], pts[k:, 2] = u * z.astype(F), v * z.astype(F), z
    pts[:, 3:] = rs.randn(n, 4)
    feat = pts[:, 3:].view(np.uint32)
    feat[5] = (0x7FC01234, 0xFFC00001, 0x7F800000, 0x80000000)           # the nearest of the whole frame (depth 0.125 below)
    feat[11] = (0x7FC0BEEF, 0xFFFFFFFF, 0xFF800000, 0x00000001)          # the median of the one-pixel box: third of the equal three
    return pts


S2 = FRAMES[2]
LAST_U, LAST_V = np.nextafter(F(48), F(0)), np.nextafter(F(24), F(0))
EDGES = [                                                                 # against box 2 = (8, 16, 24, 48) and the (64, 96) frame
    (16, 8, 1), (48, 10, 1), (20, 24, 1), (LAST_U, LAST_V, 2), (np.nextafter(F(96), F(0)), np.nextafter(F(64), F(0)), 1),
    (0, 0, 0.125), (-0.0, 3, 1),
    (24.5, 16.5, 4), (24.25, 16.25, 2), (24.75, 16.5, 2), (24.5, 16.75, 8), (24.5, 16.5, 2),     # the one-pixel box: 2, 2, 2, 4, 8
    (60.5, 40.5, 0.5), (60.5, 40.5, 0.25), (60.5, 40.5, 0.5),            # at, below and at min_depth 0.5; an equal-depth pair
]
REJECTED = [                                                              # layout 1: none of these is a candidate of any box
    (96, 5, 1), (5, 64, 1), (98, 30, 1), (-1, 30, 1), (30, -2, 1), (30, 30, -1.0), (30, 30, 0.0), (30, 30, 0.0625),
]


def layout_points(layout):
    """(3, MAXP, 7): image 0 brings nothing, image 1 one point, image 2 all 300; the rows past each count are filled with
    points that would land in boxes.  Image 2: layout 0 all 300 kept and in view under EYE, layout 1 with rejected points
    (outside the frame, behind it, NaN, Inf) under EYE, layout 2 a cloud under a pinhole camera."""
    img2 = (from_uvz(EDGES, MAXP, 7, S2, True), from_uvz(REJECTED + EDGES, MAXP, 8, S2, False), cloud(9, MAXP, 0.9))[layout]
    if layout == 1:
        k = len(REJECTED) + len(EDGES)
        img2[k + 0, 0], img2[k + 1, 1], img2[k + 2, 2] = np.nan, np.inf, np.nan
        img2[k + 3, 2], img2[k + 4, 0] = np.inf, -np.inf
    pts = np.stack([from_uvz(EDGES, MAXP, 5, FRAMES[0], True), cloud(6, MAXP, 0.5), img2])
    pts[1, 0] = (0.1, 0.1, 5.0, 1.5, -2.5, 3.5, -4.5)
    return pts


def layout_rows():
    """(3, CAPR, 7) rows; those past KEPT hold boxes that do contain points and must come back zero."""
    rows = np.zeros((3, CAPR, 7), F)
    rows[:, :, 4:] = (0.9, 0.8, 1.0)
    rows[0, :, :4] = (0, 0, 48, 100)
    rows[1, :, :4] = (0, 0, 120, 60)                                      # the one point of image 1 is in all eight
    rows[1, 1, :4] = (100, 50, 119, 59)                                   # ... but for this one
    rows[2, :, :4] = [(0, 0, 64, 96), (70, 100, 90, 120), (8, 16, 24, 48), (8, 32, 40, 80), (np.nan, 0, 64, 96), (30, 10, 30, 50),
                      (-5, -5, 70, 101), (16, 24, 17, 25)]
    return rows


def view_table(A, P, counts, sizes=FRAMES):
    v = np.zeros(len(sizes), A.data.RADAR_VIEW_DTYPE)
    for b, size in enumerate(sizes):
        v[b] = (size[0], size[1], 64, 64, 0, 0, 0, counts[b], np.asarray(P[b], F).reshape(12))
    return v


def host(A, pts, views, rows, kept, min_depth, shrink, counts=None):
    """data.box_radar per image on rows[:kept], zeros behind: what the kernel has to write, element for element."""
    B, cap = rows.shape[:2]
    want_c, want_r = np.zeros((B, cap), np.int32), np.zeros((B, cap, 2, 5), F)
    for b, v in enumerate(views):
        n = int(v["count"]) if counts is None else counts[b]
        c, r = A.data.box_radar(pts[b, :n], v["P"].reshape(3, 4), (int(v["ih"]), int(v["iw"])), rows[b, :kept[b]], min_depth, shrink)
        want_c[b, :kept[b]], want_r[b, :kept[b]] = c, r
    return want_c, want_r


def device(A, pts, views, rows, kept, min_depth, shrink, flag=None, ws=None, out=None):
    hip = A.hip
    B, cap = rows.shape[:2]
    counts = torch.full((B, cap), -7, dtype=torch.int32, device="cuda") if out is None else out[0]
    readout = torch.full((B, cap, 2, 5), 7.0, device="cuda") if out is None else out[1]
    hip.box_radar(cuda(pts), cuda(A.data.radar_view_bytes(views).numpy()), cuda(rows), cuda(np.asarray(kept, np.int32)), min_depth,
                  shrink, counts, readout, flag=flag, ws=ws)
    return counts.cpu().numpy(), readout.cpu().numpy()


def equal(got, want):
    return got[0].dtype == want[0].dtype == np.int32 and np.array_equal(got[0], want[0]) and np.array_equal(bits(got[1]), bits(want[1]))


def cameras(layout):
    return [EYE, camera(FRAMES[1]), camera(S2) if layout == 2 else EYE]


@pytest.mark.parametrize("shrink", [1.0, 0.5])
@pytest.mark.parametrize("min_depth", [0.1, 0.5])
def test_kernel_equals_the_host_statement(A, shrink, min_depth):
    flag = torch.zeros(1, dtype=torch.int32, device="cuda")
    rows = layout_rows()
    for layout in range(3):
        pts = layout_points(layout)
        views = view_table(A, cameras(layout), COUNTS)
        got = device(A, pts, views, rows, KEPT, min_depth, shrink, flag=flag)
        want = host(A, pts, views, rows, KEPT, min_depth, shrink)
        assert equal(got, want), (layout, np.argwhere(got[0] != want[0]).tolist())
        assert not got[0][0].any() and not got[0][1, 3:].any() and not bits(got[1][0]).any() and not bits(got[1][1, 3:]).any()
        c2 = want[0][2]
        assert c2[1] == c2[4] == c2[5] == 0 and c2[0] > 20                # outside the frame, a NaN edge, a degenerate box
        if shrink == 1.0:
            assert want[0][1].tolist() == [1, 0, 1, 0, 0, 0, 0, 0] and c2[0] == c2[6] > 50
            if layout < 2:
                assert c2[7] == 5 and c2[2] >= 2
        if layout == 0 and shrink == 1.0 and min_depth == 0.1:
            assert c2[0] == MAXP                                          # one box holds all 300 points
            assert want[1][2, 7, :, 0].tolist() == [2.0, 2.0] and bits(want[1][2, 7, 1, 1:]).tolist()[0] == 0x7FC0BEEF
            assert want[1][2, 0, 0, 0] == F(0.125) and bits(want[1][2, 0, 0, 1:]).tolist()[0] == 0x7FC01234
    assert int(flag.item()) == 0
    # data.device_box_radar: the same through the eager helper
    pts, views = layout_points(2), view_table(A, cameras(2), COUNTS)
    c, r = A.data.device_box_radar(cuda(pts), cuda(A.data.radar_view_bytes(views).numpy()), cuda(rows), cuda(np.asarray(KEPT, np.int32)),
                                   min_depth, shrink, flag=flag)
    assert tuple(c.shape) == (3, CAPR) and tuple(r.shape) == (3, CAPR, 2, 5)
    assert equal((c.cpu().numpy(), r.cpu().numpy()), host(A, pts, views, rows, KEPT, min_depth, shrink)) and int(flag.item()) == 0


def test_no_state_between_calls(A):
    """The same call twice on one workspace and one pair of outputs, both scribbled over in between, and another call between
    them: equal bytes."""
    hip = A.hip
    rows = layout_rows()
    ws = torch.empty(hip.box_radar_workspace_bytes(3, MAXP), dtype=torch.uint8, device="cuda")
    out = torch.empty((3, CAPR), dtype=torch.int32, device="cuda"), torch.empty((3, CAPR, 2, 5), device="cuda")
    seen = []
    for layout in (1, 2, 1):
        ws.fill_(0x7F)
        out[0].fill_(-1)
        out[1].fill_(float("nan"))
        pts, views = layout_points(layout), view_table(A, cameras(layout), COUNTS)
        got = device(A, pts, views, rows, KEPT, 0.1, 0.5, ws=ws, out=out)
        assert equal(got, host(A, pts, views, rows, KEPT, 0.1, 0.5)), layout
        seen.append((got[0].copy(), bits(got[1]).copy()))
    assert np.array_equal(seen[0][0], seen[2][0]) and np.array_equal(seen[0][1], seen[2][1])
    assert not np.array_equal(seen[0][1], seen[1][1])


def test_selection_beyond_any_on_chip_list(A):
    """20 000 points of one image, every one inside box 0 and exactly half inside box 1; the depths are a seeded permutation of
    distinct values with a run of 500 equal ones across the median rank, so the index decides the median.  The kernel has no
    LDS list of candidates (capacity 0): the radix select over the workspace planes is the only path, 79 points a thread."""
    n, size = 20000, (480, 640)
    rs = np.random.RandomState(31)
    depth = F(1) + np.arange(n, dtype=F) * F(2) ** -10                     # ascending and exact in float32
    depth[9750:10250] = depth[9750]
    z = depth[rs.permutation(n)]
    left = np.zeros(n, bool)
    left[rs.permutation(n)[:n // 2]] = True
    u = np.where(left, rs.uniform(50, 300, n), rs.uniform(340, 600, n)).astype(F)
    v = rs.uniform(20, 460, n).astype(F)
    pts = np.concatenate([np.stack([u * z, v * z, z], 1), rs.randn(n, 4).astype(F)], 1).astype(F)[None]
    rows = np.zeros((1, 3, 7), F)
    rows[0, :, :4] = [(0, 0, 480, 640), (0, 0, 480, 320), (0, 320, 480, 640)]
    views = view_table(A, [EYE], [n], [size])
    want = host(A, pts, views, rows, [3], 0.1, 1.0)
    assert want[0].tolist() == [[n, n // 2, n // 2]]
    assert want[1][0, 0, 1, 0] == depth[9750] and want[1][0, 1, 1, 0] == depth[9750] and want[1][0, 0, 0, 0] == F(1)
    flag = torch.zeros(1, dtype=torch.int32, device="cuda")
    got = device(A, pts, views, rows, [3], 0.1, 1.0, flag=flag)
    assert equal(got, want) and int(flag.item()) == 0


def test_clamps_flags_and_argument_errors(A):
    hip, data = A.hip, A.data
    rows, pts, P = layout_rows(), layout_points(2), cameras(2)
    flag = torch.zeros(1, dtype=torch.int32, device="cuda")

    def run(views, kept):
        flag.zero_()
        return device(A, pts, views, rows, kept, 0.1, 1.0, flag=flag), int(flag.item())
    good = host(A, pts, view_table(A, P, COUNTS), rows, KEPT, 0.1, 1.0)
    # a point count outside [0, max_points] is clamped
    views = view_table(A, P, (-1, 1, MAXP + 5))
    got, f = run(views, KEPT)
    assert f == hip.FLAG_POINT_COUNT and equal(got, good)
    # kept outside [0, cap] is clamped
    got, f = run(view_table(A, P, COUNTS), (CAPR + 3, -2, 8))
    assert f == hip.FLAG_BOX_COUNT
    assert equal(got, host(A, pts, view_table(A, P, COUNTS), rows, (CAPR, 0, 8), 0.1, 1.0))
    # an image without pixels gives zero rows; the others are as they were
    views = view_table(A, P, (MAXP, MAXP, MAXP))
    full = host(A, pts, views, rows, (8, 8, 8), 0.1, 1.0)
    assert full[0][0].any() and full[0][1].any()
    views[1]["ih"] = 0
    got, f = run(views, (8, 8, 8))
    assert f == hip.FLAG_GEOMETRY and not got[0][1].any() and not bits(got[1][1]).any()
    full[0][1], full[1][1] = 0, 0
    assert equal(got, full)
    views[1]["count"], views[0]["iw"] = MAXP + 1, -3
    assert run(views, (8, 9, 8))[1] == hip.FLAG_GEOMETRY | hip.FLAG_POINT_COUNT | hip.FLAG_BOX_COUNT
    # flag may be absent; the argument checks of the wrapper and the library
    device(A, pts, views, rows, KEPT, 0.1, 1.0)
    vw = cuda(data.radar_view_bytes(view_table(A, P, COUNTS)).numpy())
    dp, dr, dk = cuda(pts), cuda(rows), cuda(np.asarray(KEPT, np.int32))
    c, r = torch.empty((3, CAPR), dtype=torch.int32, device="cuda"), torch.empty((3, CAPR, 2, 5), device="cuda")
    for kw, match in ((dict(shrink=0.0), "shrink"), (dict(shrink=1.5), "shrink"), (dict(min_depth=0.0), "min_depth"),
                      (dict(min_depth=float("inf")), "min_depth")):
        args = dict(min_depth=0.1, shrink=1.0)
        args.update(kw)
        with pytest.raises(RuntimeError, match=match):
            hip.box_radar(dp, vw, dr, dk, args["min_depth"], args["shrink"], c, r)
    with pytest.raises(RuntimeError, match="torch.float32"):
        hip.box_radar(dp, vw, dr.double(), dk, 0.1, 1.0, c, r)
    with pytest.raises(RuntimeError, match="torch.int32"):
        hip.box_radar(dp, vw, dr, dk.long(), 0.1, 1.0, c, r)
    with pytest.raises(RuntimeError, match="torch.int32"):
        hip.box_radar(dp, vw, dr, dk, 0.1, 1.0, c.float(), r)
    with pytest.raises(RuntimeError, match="expected rows"):
        hip.box_radar(dp, vw, dr[:2], dk, 0.1, 1.0, c, r)
    with pytest.raises(RuntimeError, match="view table"):
        hip.box_radar(dp, vw[:2], dr, dk, 0.1, 1.0, c, r)
    with pytest.raises(RuntimeError, match="workspace"):
        hip.box_radar(dp, vw, dr, dk, 0.1, 1.0, c, r, ws=torch.empty(64, dtype=torch.uint8, device="cuda"))
    with pytest.raises(RuntimeError, match="workspace"):
        hip.box_radar(dp, vw, dr, dk, 0.1, 1.0, c, r, ws=torch.empty(4096, dtype=torch.float32, device="cuda"))


# ---- the pipelines ------------------------------------------------------------------------------------------------------
NC, NS, S, B, K = 4, 9, 64, 2, 200
CAP = (80, 112)
RUN_SIZES = {True: [[(40, 56), (80, 112)], [(61, 33), (48, 80)]], False: [[CAP, CAP], [CAP, CAP]]}
_MODEL = []


def model_of(A):
    if not _MODEL:
        m = A.EfficientVRNet(NC, NS, "nano", img_size=S).cuda().eval()
        A.randomize_state_dict(m.state_dict(), seed=4)
        _MODEL.append(m)
    return _MODEL[0]


def frame_points(seed, sizes):
    rs = np.random.RandomState(seed)
    return [cloud(seed + 10 * b, int(rs.randint(K // 2, K + 1)), 0.9) for b in range(len(sizes))], np.stack([camera(s) for s in sizes])


def frames_of(seed, sizes, ragged):
    rng = np.random.default_rng(seed)
    frames = [rng.integers(0, 256, (ih, iw, 3), dtype=np.uint8) for ih, iw in sizes]
    return frames if ragged else np.stack(frames)


def check_readout(A, got, pts, P, sizes, min_depth, shrink):
    """box_points / box_radar of a result against data.box_radar on the result's own rows; returns the points counted."""
    rows, kept = got.rows.cpu().numpy(), got.kept.cpu().numpy()
    views = view_table(A, P, [len(p) for p in pts], sizes)
    packed = np.zeros((B, K, 7), F)
    for b, p in enumerate(pts):
        packed[b, :len(p)] = p
    want = host(A, packed, views, rows, kept, min_depth, shrink)
    assert tuple(got.box_points.shape) == rows.shape[:2] and tuple(got.box_radar.shape) == rows.shape[:2] + (2, 5)
    assert equal((got.box_points.cpu().numpy(), got.box_radar.cpu().numpy()), want)
    return int(want[0].sum())


@pytest.mark.parametrize("ragged", [True, False])
@pytest.mark.parametrize("graph", [True, False])
def test_frame_pipeline_with_the_stage_equals_the_pipeline_without(A, ragged, graph):
    model = model_of(A)
    shrink, md = (0.5, 0.5) if ragged == graph else (1.0, 0.1)
    kw = dict(batch=B, conf_thres=0.05, nms_thres=0.4, max_candidates=64, graph=graph, ragged=ragged, radar_points=K, radar_radius=1,
              radar_min_depth=md, letterbox_image=ragged or graph)
    plain = A.FramePipeline(model, CAP, (S, S), **kw)
    stage = A.FramePipeline(model, CAP, (S, S), box_radar=True, box_shrink=shrink, **kw)
    assert (stage.graph is not None) == graph and (plain.graph is not None) == graph
    names = ("rows", "kept", "det_counts", "class_map", "seg_counts", "rendered", "flag")
    inside = 0
    for k, sizes in enumerate(RUN_SIZES[ragged]):
        frames = frames_of(40 + k, sizes, ragged)
        pts, P = frame_points(50 + k, sizes)
        want = plain.run(frames, pts, calib=P)
        assert want.box_points is None and want.box_radar is None
        want = [getattr(want, n).clone() for n in names]
        got = stage.run(frames, pts, calib=P)
        for n, w in zip(names, want):
            g = getattr(got, n)
            assert g.dtype == w.dtype and torch.equal(g, w), (k, n)
        assert int(got.kept.max()) > 0 and int(got.flag.item()) & ~A.infer.FLAG_CANDIDATES == 0
        inside += check_readout(A, got, pts, P, sizes, md, shrink)
        readout = got.radar_readout()
        dets = got.detections()
        assert [r.shape for r in readout] == [(len(d), 11) for d in dets]
        for b in range(B):
            assert np.array_equal(readout[b][:, 0], got.box_points[b, :len(dets[b])].cpu().numpy().astype(F))
            assert np.array_equal(bits(readout[b][:, 1:]), bits(got.box_radar[b, :len(dets[b])].reshape(-1, 10)))
    assert inside > 0                                                       # at least one box has points in it
    # a run enqueues and returns: no host synchronisation
    torch.cuda.synchronize()
    before = got.box_radar.clone()
    torch.cuda.set_sync_debug_mode("error")
    try:
        got = stage.run(frames, pts, calib=P)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    assert torch.equal(got.rows, want[0]) and np.array_equal(bits(got.box_radar), bits(before))


def test_construction_errors(A):
    model = model_of(A)
    kw = dict(batch=B, max_candidates=64, graph=False)
    with pytest.raises(RuntimeError, match="box_radar reads the radar POINTS"):
        A.FramePipeline(model, CAP, (S, S), box_radar=True, **kw)
    with pytest.raises(RuntimeError, match="box_shrink belongs to box_radar"):
        A.FramePipeline(model, CAP, (S, S), box_shrink=0.5, radar_points=K, **kw)
    for bad in (0.0, 1.25, -1.0, float("nan")):
        with pytest.raises(RuntimeError, match="shrink"):
            A.FramePipeline(model, CAP, (S, S), box_radar=True, box_shrink=bad, radar_points=K, **kw)


def test_predict_dir_writes_the_readout_beside_each_picture(A, tmp_path):
    from PIL import Image
    model = model_of(A)
    sizes = [(61, 33), (48, 80)]
    stems = ["1234567890.00001", "1234567890.00002"]
    src, radar_root, dst = tmp_path / "in", tmp_path / "radar", tmp_path / "out"
    src.mkdir()
    radar_root.mkdir()
    P = camera(CAP)
    pts = [cloud(70 + b, K, 0.9) for b in range(B)]
    for b, (stem, frame) in enumerate(zip(stems, frames_of(60, sizes, True))):
        Image.fromarray(frame).save(src / (stem + ".png"))
        np.savez(radar_root / (stem + ".npz"), pts[b])
    pipe = A.FramePipeline(model, CAP, (S, S), batch=B, conf_thres=0.05, nms_thres=0.4, max_candidates=64, graph=False, ragged=True,
                           radar_points=K, calib=P, box_radar=True)
    out = A.infer.predict_dir(pipe, str(src), str(radar_root), str(dst))
    assert [n for n, _ in out] == [s + ".png" for s in stems] and sum(len(d) for _, d in out) > 0
    for b, (name, dets) in enumerate(out):
        text = open(os.path.join(dst, stems[b] + "_radar.txt")).read()
        lines = text.splitlines()
        assert len(lines) == len(dets) and all(len(line.split()) == 17 for line in lines)
        count, readout = A.data.box_radar(pts[b], P, sizes[b], dets)
        want = np.concatenate([count[:, None].astype(F), readout.reshape(-1, 10)], 1)
        assert text == A.infer.radar_text(dets, want)
    # a picture named like another's readout: refused before anything runs
    Image.fromarray(np.zeros((20, 20, 3), np.uint8)).save(src / (stems[0] + "_radar.png"))
    with pytest.raises(RuntimeError, match="would both be saved"):
        A.infer.predict_dir(pipe, str(src), str(radar_root), str(dst))
