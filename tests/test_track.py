"""The tracker on the GPU: vrnet_track_update_f32 (csrc/track.hip) against the host statement `data.track_update`, and the
pipelines built with track against the same pipelines without it.  Both sides do the same float32 operations without
contraction, so every comparison is bit for bit, on int32 views of table, header and ids, after EVERY call of a sequence of
six on one persistent device table.  B = 3 streams with different histories, the last with kept = 0 throughout.
Shapes: T = 4 against 6 valid rows (the table fills, the flag is raised, a freed slot is re-taken in the same call); T = 64
with cap = 300 and 300 kept rows (more than one row a thread in every sweep, the last sweep partial); T = 256 (every thread
owns a slot); a chain of 32 tracks and 32 rows that takes the mutually-best matching through 32 rounds; pipelines: nano,
64 x 64, B = 2."""
import os

import numpy as np
import pytest
import torch

from tests.test_track_host import candidates, greedy_mutual

pytestmark = pytest.mark.gpu

F = np.float32
NB = 3


@pytest.fixture(scope="module")
def A():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    import asy_vrnet_amd
    from asy_vrnet_amd import data, hip, infer, evaluate  # noqa: F401  (A.data, A.hip, A.infer, A.evaluate below)
    return asy_vrnet_amd


def cuda(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def words(a):
    """Any array of 4-byte items (TRACK_DTYPE records included) as int32 words."""
    a = a.detach().cpu().numpy() if torch.is_tensor(a) else np.asarray(a)
    return np.frombuffer(np.ascontiguousarray(a).tobytes(), np.int32)


def run_sequence(A, calls, T, params=None, radar=False):
    """calls: a list of (rows (NB, cap, 7), kept (NB)[, box_points, box_radar]).  One device table through all of them; after
    every call table, head, ids and flag against data.track_update on the same inputs and the state before.  Returns the
    host's (table, head) at the end and the OR of the flags."""
    params = A.data.check_track_params(dict(max_tracks=T, **(params or {})))
    cap = calls[0][0].shape[1]
    table, head = np.zeros((NB, T), A.data.TRACK_DTYPE), np.zeros((NB, 4), np.int32)
    d_table = torch.zeros((NB, T, 16), dtype=torch.int32, device="cuda")
    d_head = torch.zeros((NB, 4), dtype=torch.int32, device="cuda")
    d_ids = torch.full((NB, cap), -7, dtype=torch.int32, device="cuda")          # every element must be written
    d_flag = torch.zeros(1, dtype=torch.int32, device="cuda")
    flags = 0
    for k, call in enumerate(calls):
        rows, kept = call[0], call[1]
        bp, br = (call[2], call[3]) if radar else (None, None)
        table, head, ids, flag = A.data.track_update(table, head, rows, kept, bp, br, params)
        d_flag.zero_()
        d_ids.fill_(-7)
        A.hip.track_update(cuda(rows), cuda(kept), d_table, d_head, d_ids, params, box_points=None if bp is None else cuda(bp),
                           box_radar=None if br is None else cuda(br), flag=d_flag)
        assert int(d_flag.item()) == flag, (k, int(d_flag.item()), flag)
        assert np.array_equal(words(d_head), words(head)), (k, d_head.cpu().numpy(), head)
        assert np.array_equal(words(d_ids), words(ids)), (k, np.flatnonzero(words(d_ids) != words(ids))[:8])
        bad = np.flatnonzero(words(d_table) != words(table))
        assert not len(bad), (k, bad[:8] // 16, bad[:8] % 16)
        flags |= flag
    return table, head, flags


def moving_scene(seed, cap, kept, calls=6, classes=3, radar=False, span=2000.0):
    """Objects that move at constant rates over a span x span field, jittered detections of them in shuffled order, some
    missing in a call, some spurious; stream 1 sees other objects than stream 0, stream 2 nothing."""
    rs = np.random.RandomState(seed)
    out = []
    objs = []
    for b in range(NB):
        m = kept[b]
        c = rs.uniform(0, span, (m, 2))
        size = rs.uniform(20, 80, (m, 2))
        objs.append((c, size, rs.uniform(-6, 6, (m, 2)), rs.randint(0, classes, m)))
    for k in range(calls):
        rows, n = np.zeros((NB, cap, 7), F), np.zeros(NB, np.int32)
        bp, br = np.zeros((NB, cap), np.int32), np.zeros((NB, cap, 2, 5), F)
        for b in range(NB):
            c, size, vel, cls = objs[b]
            m = kept[b]
            if not m:
                continue
            centre = c + k * vel + rs.normal(0, 1.5, (m, 2))
            half = size / 2 + rs.normal(0, 1.0, (m, 2))
            box = np.concatenate([centre - half, centre + half], 1)[:, [0, 1, 2, 3]]
            gone = rs.rand(m) < 0.15                                             # a missing detection: a spurious one instead
            box[gone] = np.concatenate([rs.uniform(0, span, (gone.sum(), 2))] * 2, 1) + [0, 0, 30, 30]
            order = rs.permutation(m)
            rows[b, :m, :4] = box[order]
            rows[b, :m, 4:6] = rs.uniform(0.3, 1, (m, 2))
            rows[b, :m, 6] = cls[order]
            n[b] = m
            bp[b, :m] = rs.randint(0, 4, m)
            br[b, :m, :, 0] = rs.uniform(5, 200, (m, 2))
            br[b, :m, :, 1:] = rs.randn(m, 2, 4)
        out.append((rows, n, bp, br) if radar else (rows, n))
    return out


def test_a_small_table_fills_frees_and_is_retaken(A):
    """T = 4 against 6 valid rows, max_age 0: every call the unmatched tracks are freed and their slots re-taken in the same
    call by rows that found no match; rows beyond the free slots get id 0 and FLAG_TRACK_FULL."""
    cap = 8
    grid = [(40.0 * i, 10.0, 40.0 * i + 30, 50.0) for i in range(12)]
    picks = [[(0, 1, 2, 3, 4, 5), (6, 7, 8, 9, 10, 11)], [(0, 1, 6, 7, 8, 9), (6, 7)], [(5, 4, 3, 2, 1, 0), ()],
             [(0, 1, 2), (0, 1, 2, 3, 4, 5)], [(10, 11, 0, 1, 2, 3), (5, 3, 1, 0, 2, 4)], [(), (0, 1, 2, 3, 4, 5)]]
    calls = []
    for pick in picks:
        rows, kept = np.zeros((NB, cap, 7), F), np.zeros(NB, np.int32)
        for b, idx in enumerate(pick):
            for i, g in enumerate(idx):
                rows[b, i, :4], rows[b, i, 6] = grid[g], g % 2
            kept[b] = len(idx)
        calls.append((rows, kept))
    table, head, flags = run_sequence(A, calls, 4, dict(max_age=0))
    assert flags == A.data.FLAG_TRACK_FULL and head[:, 2].tolist() == [6, 6, 6] and head[2].tolist() == [0, 0, 6, 0]
    assert head[0, 0] > 8 and (table["id"][1] != 0).all()                        # ids went on while slots were re-used


@pytest.mark.parametrize("radar", [False, True])
def test_sixty_four_tracks_against_three_hundred_rows(A, radar):
    calls = moving_scene(5 + radar, 300, (300, 120, 0), radar=radar)
    table, head, flags = run_sequence(A, calls, 64, radar=radar)
    assert flags == A.data.FLAG_TRACK_FULL and head[:, 1].tolist() == [64, 64, 0]
    assert table["hits"][0].max() >= 5                                          # tracks do persist through the six calls
    if radar:
        assert (table["range_age"] >= 0).sum() > 40 and (table["range_age"][table["id"] != 0] < 0).any()


def test_a_table_of_two_hundred_and_fifty_six(A):
    calls = moving_scene(9, 320, (250, 320, 0), radar=True, span=4000.0)
    table, head, flags = run_sequence(A, calls, 256, dict(iou=0.2, max_age=2, gain=(0.75, 0.5), range_gain=(1.0, 0.125)), radar=True)
    assert head[0, 1] > 200 and head[1, 1] == 256 and flags & A.data.FLAG_TRACK_FULL
    assert table["hits"][0].max() >= 5 and table["hits"][1].max() >= 5


def chain(k):
    """Track k at column P_k and row k at Q_k, P_k < Q_k < P_(k+1), width 64: d_k = Q_k - P_k = 32 - k / 2 and e_k = P_(k+1) -
    Q_k = 31.75 - k / 2, so the overlaps 64 - d_0 < 64 - e_0 < 64 - d_1 < ... rise along the chain, every one an IoU of 1 / 3
    or more, and rows two tracks away stay below 0.14.  All multiples of a quarter: exact in float32."""
    P = sum((32 - j / 2) + (31.75 - j / 2) for j in range(k))
    return P, P + 32 - k / 2


def test_a_chain_takes_the_mutually_best_matching_through_many_rounds(A):
    """Row k prefers track k + 1, which prefers row k + 1: only the last pair is mutually best, and the chain unzips one pair
    a round.  The plain greedy loop and the rounds must agree -- the host rule is the former, the kernel does the latter."""
    cap = 32
    at_p, at_q = np.zeros((NB, cap, 7), F), np.zeros((NB, cap, 7), F)
    for k in range(32):
        P, Q = chain(k)
        at_p[:2, k, :4], at_q[:2, k, :4] = (0, P, 10, P + 64), (0, Q, 10, Q + 64)
    at_q[1, :, :4] = at_q[1, ::-1, :4].copy()                                    # stream 1: the same rows in reverse order
    kept = np.array([32, 32, 0], np.int32)
    params = A.data.check_track_params(dict(max_tracks=32))
    born = A.data.track_update(np.zeros((NB, 32), A.data.TRACK_DTYPE), np.zeros((NB, 4), np.int32), at_p, kept, params=params)
    pairs, rounds = greedy_mutual(candidates(born[0], at_q, params["iou"]), 32, 32)
    assert rounds == 32 and pairs == list(range(32))                            # the input does what it is built for
    table, head, flags = run_sequence(A, [(at_p, kept), (at_q, kept), (at_p, kept), (at_q, kept), (at_q, kept), (at_p, kept)], 32)
    assert head[:, 1].tolist() == [32, 32, 0] and table["hits"][:2].min() >= 5     # the 32 tracks live through the sequence


def test_ties_threshold_class_gate_bad_rows_and_a_kept_outside_the_buffer(A):
    cap = 12
    nan, inf = float("nan"), float("inf")
    box = (10, 10, 30, 30)
    thr = float(A.data.track_iou(np.array([[0, 0, 4, 4]], F), np.array([[0, 2, 4, 6]], F))[0, 0])

    def call(per_stream, kept=None, depth=None, points=None):
        rows = np.zeros((NB, cap, 7), F)
        bp, br = np.zeros((NB, cap), np.int32), np.zeros((NB, cap, 2, 5), F)
        n = np.zeros(NB, np.int32)
        for b, boxes in enumerate(per_stream):
            for i, bx in enumerate(boxes):
                rows[b, i, :4], rows[b, i, 6] = bx[:4], bx[4] if len(bx) > 4 else 0
            n[b] = len(boxes)
            bp[b, :len(boxes)] = 2 if points is None else points[b]
            br[b, :len(boxes), 1, 0] = 10.0 + b if depth is None else depth[b]
        return rows, (n if kept is None else np.array(kept, np.int32)), bp, br

    bad = [(10, 10, nan, 30), (10, 10, 10, 30), (30, 10, 10, 30), (10, -inf, 30, inf), (nan, nan, nan, nan), box]
    s0 = [[box, box, (100, 100, 104, 104)],                                      # two tracks on one box; one for the threshold
          [(40, 40, 50, 50), box, box, (100, 102, 104, 106)],                    # the tie: slot 0 takes row 1; iou == thr matches
          bad,                                                                   # NaN / Inf / inverted rows
          [box + (1,), (12, 12, 32, 32, 0), (200, 200, 220, 220, nan), (200, 200, 220, 220, 3e9)],      # the class gate
          [box, (200, 200, 220, 220, nan)],
          [box]]
    s1 = [[(0, 0, 20, 20, 2)], [(0, 0, 20, 20, 2)], [(1, 1, 21, 21, 2)], [(2, 2, 22, 22, 2)], [(3, 3, 23, 23, 2)], [(4, 4, 24, 24, 2)]]
    depths = [(10, 20, 0), (nan, 24, 0), (12, inf, 0), (13, 26, 0), (14, 28, 0), (15, 30, 0)]
    points = [(2, 1, 0), (2, 1, 0), (2, 1, 0), (0, 0, 0), (2, 1, 0), (2, 1, 0)]
    calls = [call([a, c, []], depth=d, points=p) for a, c, d, p in zip(s0, s1, depths, points)]
    for radar in (False, True):
        table, head, flags = run_sequence(A, calls, 8, dict(iou=thr), radar=radar)
        assert flags == 0 and head[0, 0] >= 6
        t = table[1][0]
        assert t["hits"] == 6 and (t["range_age"], t["x"][4] > 0) == ((0, True) if radar else (-1, False))
    # kept outside [0, cap]: clamped and flagged, on stream 0 above the buffer and on stream 1 below zero
    calls = [call([[box] * 3, [box], []], kept=k) for k in ([3, 1, 0], [cap + 5, -3, 0], [2, 1, 0], [cap, 0, -1], [0, 0, 0], [1, 1, 0])]
    table, head, flags = run_sequence(A, calls, 8, radar=True)
    assert flags == 512


def test_argument_errors(A):
    p = A.data.check_track_params(True)
    rows, kept = torch.zeros((2, 8, 7), device="cuda"), torch.zeros(2, dtype=torch.int32, device="cuda")
    i32 = dict(dtype=torch.int32, device="cuda")
    table, head, ids = torch.zeros((2, 4, 16), **i32), torch.zeros((2, 4), **i32), torch.zeros((2, 8), **i32)
    A.hip.track_update(rows, kept, table, head, ids, p)
    assert head.cpu().tolist() == [[0, 0, 1, 0]] * 2
    for bad in (dict(table=torch.zeros((2, 4, 15), **i32)), dict(table=torch.zeros((2, 257, 16), **i32)), dict(head=torch.zeros((2, 3), **i32)),
                dict(ids=torch.zeros((2, 7), **i32)), dict(kept=kept.long()), dict(box_points=torch.zeros((2, 8), **i32)),
                dict(rows=torch.zeros((2, 1025, 7), device="cuda"), ids=torch.zeros((2, 1025), **i32)), dict(params=dict(p, iou=0.0)),
                dict(params=dict(p, gain=(0.5, 2.5))), dict(params=None), dict(table=table.cpu())):
        kw = dict(dict(rows=rows, kept=kept, table=table, head=head, ids=ids, params=p), **bad)
        with pytest.raises(RuntimeError):
            A.hip.track_update(**kw)


# ---- the pipelines (the setup of tests/test_box_radar.py) -----------------------------------------------------------------
from tests.test_box_radar import B, CAP, K, S, camera, cloud, frame_points, frames_of, model_of  # noqa: E402

RUN_SIZES = {True: [[(40, 56), (80, 112)], [(61, 33), (48, 80)]], False: [[CAP, CAP], [CAP, CAP]]}
TRACK = dict(max_tracks=256, iou=0.2)                       # three runs of at most 64 rows never fill 256 slots


def host_step(A, state, got, params):
    """data.track_update on what the caller of a pipeline reads back: detections() and, with box_radar, radar_readout()."""
    dets = got.detections()
    cap = got.rows.shape[1]
    rows, kept = np.zeros((B, cap, 7), F), np.array([len(d) for d in dets], np.int32)
    bp = br = None
    if got.box_radar is not None:
        bp, br = np.zeros((B, cap), np.int32), np.zeros((B, cap, 2, 5), F)
    for b, d in enumerate(dets):
        rows[b, :len(d)] = d
        if bp is not None:
            r = got.radar_readout()[b]
            bp[b, :len(d)], br[b, :len(d)] = r[:, 0].astype(np.int32), r[:, 1:].reshape(-1, 2, 5)
    return A.data.track_update(state[0], state[1], rows, kept, bp, br, params)


@pytest.mark.parametrize("box_radar", [False, True])
@pytest.mark.parametrize("ragged", [False, True])
def test_frame_pipeline_with_tracking(A, ragged, box_radar):
    model = model_of(A)
    kw = dict(batch=B, conf_thres=0.05, nms_thres=0.4, max_candidates=64, ragged=ragged, radar_points=K, radar_radius=1,
              letterbox_image=True, box_radar=True if box_radar else None)
    plain = A.FramePipeline(model, CAP, (S, S), **kw)
    stage = A.FramePipeline(model, CAP, (S, S), track=TRACK, **kw)
    eager = A.FramePipeline(model, CAP, (S, S), track=TRACK, graph=False, **kw)
    assert stage.graph is not None and eager.graph is None and plain.track is None
    params = A.data.check_track_params(TRACK)
    # the warm-up and the capture ran the chain, and left no trace in the state
    for pipe in (stage, eager):
        for t in (pipe._track_table, pipe._track_head, pipe._track_ids):
            assert not t.any().item()
    names = ("rows", "kept", "det_counts", "class_map", "seg_counts", "rendered", "flag")
    state = (np.zeros((B, 256), A.data.TRACK_DTYPE), np.zeros((B, 4), np.int32))
    first, second = RUN_SIZES[ragged]
    matched = 0
    for k, (seed, sizes) in enumerate([(40, first), (40, first), (41, second)]):          # the second frame repeats the first
        frames = frames_of(seed, sizes, ragged)
        pts, P = frame_points(seed + 10, sizes)
        want = plain.run(frames, pts, calib=P)
        assert want.track_ids is None and want.track_table is None and want.track_head is None
        want = [getattr(want, n).clone() for n in names]
        got = stage.run(frames, pts, calib=P)
        for n, w in zip(names, want):
            g = getattr(got, n)
            assert g.dtype == w.dtype and torch.equal(g, w), (k, n)
        assert int(got.kept.max()) > 0 and int(got.flag.item()) & ~A.infer.FLAG_CANDIDATES == 0
        table, head, ids, flag = host_step(A, state, got, params)
        state = (table, head)
        assert flag == 0
        assert np.array_equal(words(got.track_table), words(table)) and np.array_equal(words(got.track_head), words(head)), k
        assert np.array_equal(words(got.track_ids), words(ids)), k
        other = eager.run(frames, pts, calib=P)                                            # captured equals graph=False
        for n in ("track_table", "track_head", "track_ids", "rows"):
            assert torch.equal(getattr(other, n), getattr(got, n)), (k, n)
        tracks = got.tracks()
        for b in range(B):
            live, row_ids = tracks[b]
            assert live.dtype == A.data.TRACK_DTYPE and np.array_equal(words(live), words(table[b][table[b]["id"] != 0]))
            assert np.array_equal(row_ids, ids[b, :int(got.kept[b])])
        if k == 1:                                                                         # the same frame again: every row matches
            matched = int((table["hits"] == 2).sum())
            assert head[:, 3].tolist() == [0, 0] and matched == int((ids != 0).sum()) > 0
            if box_radar:
                assert ((table["range_age"] == 0) & (table["id"] != 0)).any()
    # a run enqueues and returns: no host synchronisation
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        stage.run(frames, pts, calib=P)
        stage.reset_tracks([1])
    finally:
        torch.cuda.set_sync_debug_mode("default")
    # reset_tracks([1]) clears stream 1 only
    assert stage._track_table[0].any().item() and stage._track_head[0].any().item()
    assert not stage._track_table[1].any().item() and not stage._track_head[1].any().item() and not stage._track_ids[1].any().item()
    stage.reset_tracks()
    assert not stage._track_table.any().item() and not stage._track_head.any().item()
    with pytest.raises(RuntimeError, match="batch slots"):
        stage.reset_tracks([B])
    with pytest.raises(RuntimeError, match="not built with track"):
        plain.reset_tracks()
    with pytest.raises(RuntimeError, match="not built with track"):
        plain.result.tracks()


def test_construction_errors_and_eval_pipeline(A):
    model = model_of(A)
    kw = dict(batch=B, max_candidates=64, graph=False)
    for bad in (dict(max_tracks=0), dict(iou=2.0), dict(velocity=1), 5):
        with pytest.raises(RuntimeError, match="FramePipeline"):
            A.FramePipeline(model, CAP, (S, S), track=bad, **kw)
    with pytest.raises(TypeError, match="track"):
        A.evaluate.EvalPipeline(model, CAP, (S, S), ["a", "b", "c", "d"], 9, track=True, **kw)


def test_predict_dir_tracks_a_folder_as_one_sequence(A, tmp_path):
    from PIL import Image
    model = model_of(A)
    sizes = [(61, 33), (61, 33), (48, 80)]
    stems = ["1234567890.00001", "1234567890.00002", "1234567890.00003"]
    src, radar_root, dst = tmp_path / "in", tmp_path / "radar", tmp_path / "out"
    src.mkdir()
    radar_root.mkdir()
    P = camera(CAP)
    frames = frames_of(60, sizes, True)
    frames[1] = frames[0]                                                          # the second picture repeats the first
    pts = [cloud(70, K, 0.9), cloud(70, K, 0.9), cloud(72, K, 0.9)]
    for stem, frame, p in zip(stems, frames, pts):
        Image.fromarray(frame).save(src / (stem + ".png"))
        np.savez(radar_root / (stem + ".npz"), p)
    kw = dict(conf_thres=0.05, nms_thres=0.4, max_candidates=64, graph=False, ragged=True, radar_points=K, calib=P, box_radar=True,
              track=TRACK)
    two = A.FramePipeline(model, CAP, (S, S), batch=2, **kw)
    with pytest.raises(RuntimeError, match="needs batch 1"):
        A.infer.predict_dir(two, str(src), str(radar_root), str(dst))
    assert not os.path.exists(dst) and not two._track_head.any().item()            # before anything was enqueued
    one = A.FramePipeline(model, CAP, (S, S), batch=1, **kw)
    out = A.infer.predict_dir(one, str(src), str(radar_root), str(dst))
    assert [n for n, _ in out] == [s + ".png" for s in stems] and len(out[0][1]) > 0
    texts = [open(os.path.join(dst, s + "_tracks.txt")).read() for s in stems]
    first, second = ([line.split() for line in t.splitlines()] for t in texts[:2])
    assert 0 < len(first) <= len(out[0][1]) and all(len(f) == 10 and f[2:4] == ["1", "0"] for f in first)
    assert [f[0] for f in second] == [f[0] for f in first] and all(f[2:4] == ["2", "0"] for f in second)
    assert texts[2] == A.data.track_text(one.result.tracks()[0][0])
    Image.fromarray(np.zeros((20, 20, 3), np.uint8)).save(src / (stems[0] + "_tracks.png"))
    with pytest.raises(RuntimeError, match="would both be saved"):
        A.infer.predict_dir(one, str(src), str(radar_root), str(dst))
