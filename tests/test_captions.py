"""The caption kernels (csrc/captions.hip) against their host statements, byte for byte: vrnet_caption_text_f32 against
render.caption_strings (code for code, through render.caption_records), the two draw kernels against
render.draw_captions_host, and a FramePipeline built with captions against the same pipeline without them plus the host
rule.  tests/test_captions_host.py pins those statements to Python's format and to live Pillow.  The atlas is built with
Pillow when it imports, otherwise it is the committed fixture of the same face."""
import numpy as np
import pytest
import torch

from asy_vrnet_amd import data, render
from tests import captions_cases as CC
from tests import labels_cases as LC

pytestmark = pytest.mark.gpu
PAL = render.det_palette(4)
I32 = dict(dtype=torch.int32, device="cuda")


@pytest.fixture(scope="module")
def hip():
    import asy_vrnet_amd.hip as hip
    return hip


def cuda(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def new_flag():
    return torch.zeros(1, **I32)


def table_words(table):
    return cuda(np.frombuffer(np.ascontiguousarray(table).tobytes(), np.int32).reshape(table.shape + (16,)).copy())


def text_on_device(hip, kept, offsets, n_out, ids=None, table=None, points=None, readout=None, rate_scale=0.0):
    out, flag = torch.full((n_out, 12), -7, **I32), new_flag()
    got = hip.caption_text(cuda(np.asarray(kept, np.int32)), cuda(np.asarray(offsets, np.int32)), out,
                           ids=None if ids is None else cuda(ids), table=None if table is None else table_words(table),
                           box_points=None if points is None else cuda(points), box_radar=None if readout is None else cuda(readout),
                           rate_scale=rate_scale, flag=flag)
    assert got is out
    return out.cpu().numpy(), int(flag)


def check_text(hip, kept, cap, **kw):
    """One launch against caption_strings: the records of the kept rows code for code, nothing else written, the flag."""
    kept = np.asarray(kept, np.int32)
    n = np.clip(kept, 0, cap)
    offsets = np.concatenate([[0], np.cumsum(n)]).astype(np.int32)
    total = int(offsets[-1])
    got, flag = text_on_device(hip, kept, offsets, total + 5, **kw)
    host = dict(table=kw.get("table"), box_points=kw.get("points"), box_radar=kw.get("readout"), rate_scale=kw.get("rate_scale", 0.0))
    strings, bits = render.caption_strings(kw.get("ids"), kept, **host)
    assert [len(s) for s in strings] == n.tolist()
    want = render.caption_records(strings)
    bad = np.flatnonzero((got[:total] != want).any(axis=1))
    print(f"caption_text B {len(kept)} cap {cap} rows {total}: {len(bad)} records differ, flag {flag} (host {bits})")
    assert not len(bad), (bad[:5], render.caption_decode(got[bad[:5]]), render.caption_decode(want[bad[:5]]))
    assert (got[total:] == -7).all() and flag == bits
    assert render.caption_decode(got[:total]) == [s for image in strings for s in image]
    return strings, flag


def test_text_kernel_without_a_tracker_formats_every_tie(hip):
    B, cap = 489, 1024
    ties = CC.tie_sweep()
    extra = np.array([np.inf, -np.inf, np.nan, -1.0, -0.0, -0.04, 9999.95, 9999.94, 0.0, 0.04, 0.05, 1e-45, 3e38, 100000.0], np.float32)
    depth = np.ones(B * cap, np.float32)
    depth[:len(ties)] = ties
    depth[len(ties):len(ties) + len(extra)] = extra
    assert len(ties) + len(extra) <= B * cap
    readout = np.zeros((B, cap, 2, 5), np.float32)
    readout[:, :, 0, 0] = -5.0                                # the nearest point: never what is drawn
    readout[:, :, 1, 0] = depth.reshape(B, cap)
    points = np.ones((B, cap), np.int32)
    points[-1, -40:] = (0, -1) * 20                           # rows without points: the empty caption, no flag
    strings, flag = check_text(hip, [cap] * B, cap, points=points, readout=readout)
    assert flag == render.FLAG_CAPTION
    flat = [s for image in strings for s in image]
    drawn = render.fixed_tenths(ties)[0] <= 99999            # the last ties round up to 10000.0: left out
    assert drawn.sum() >= len(ties) - 3
    assert flat[:len(ties)] == [t + "m" if ok else "" for t, ok in zip(CC.tenths_text(ties), drawn.tolist())]
    assert flat[len(ties):len(ties) + len(extra)] == ["", "", "", "", "", "", "", "9999.9m", "0.0m", "0.0m", "0.1m", "0.0m", "", ""]
    assert flat[-40:] == [""] * 40
    # the same values without the bad ones raise no flag; with ids beside the readout the id stands in front
    ids = np.arange(1, B * cap + 1, dtype=np.int32).reshape(B, cap)[:2]
    strings, flag = check_text(hip, [cap, 7], cap, ids=ids, points=points[:2], readout=readout[:2])
    assert flag == 0 and strings[0][3] == "#4 " + flat[3] and len(strings[1]) == 7


def track_case(rng, B, cap, T, kept):
    """A table as the tracker leaves it -- live slots name distinct kept rows or none -- with ids 1, 9, 10, 2^31 - 1 among them,
    ranges and rates of both signs, coasting and unborn ranges, and a few corrupt slots the rule still defines an answer for."""
    table, ids = np.zeros((B, T), data.TRACK_DTYPE), np.zeros((B, cap), np.int32)
    special = [1, 9, 10, 2 ** 31 - 1]
    for b in range(B):
        n = int(np.clip(kept[b], 0, cap))
        rows = rng.permutation(cap)[:T]
        for s in range(T):
            if rng.random() < 0.2:
                continue                                      # a free slot
            t = table[b, s]
            t["id"] = special[s] if s < len(special) else int(rng.integers(11, 5000))
            t["row"] = int(rows[s]) if rows[s] < n and rng.random() < 0.9 else -1
            t["range_age"] = int(rng.integers(-1, 4))
            t["x"][4] = np.float32(rng.random() * 10 ** int(rng.integers(0, 5)))
            t["v"][4] = np.float32((rng.random() - 0.5) * 10 ** int(rng.integers(-2, 2)))
            if t["row"] >= 0:
                ids[b, t["row"]] = t["id"]
        live = [s for s in range(T) if table[b, s]["id"] != 0 and table[b, s]["row"] >= 0]
        if len(live) >= 4:
            a, c, d, e = live[:4]
            table[b, c]["row"] = table[b, a]["row"]           # two slots name one row: only the one that carries its id counts
            table[b, d]["x"][4], table[b, d]["range_age"] = np.nan, 0
            table[b, e]["v"][4], table[b, e]["range_age"] = np.inf, 0
    return table, ids


@pytest.mark.parametrize("B,cap,T", [(2, 8, 4), (1, 1024, 256)])
def test_text_kernel_with_a_track_table(hip, B, cap, T):
    rng = np.random.default_rng(cap + T)
    seen = 0
    for kept in ([cap] * B, [0] * B, [cap + 3] * B, [cap // 2] + [cap] * (B - 1)):
        table, ids = track_case(rng, B, cap, T, kept)
        for rate_scale in (0.0, 25.0):
            strings, flag = check_text(hip, kept, cap, ids=ids, table=table, rate_scale=rate_scale)
            assert bool(flag & render.FLAG_BOX_COUNT) == (kept[0] > cap)
            flat = [s for image in strings for s in image]
            assert not any("m/s" in s for s in flat) or rate_scale > 0
            seen += sum("m/s" in s for s in flat)
        # ids alone: no table, no readout
        strings, _ = check_text(hip, kept, cap, ids=ids)
        assert all(s == "" or s.startswith("#") and " " not in s for image in strings for s in image)
    assert seen > 0
    # the named ids, each with a range and a rate of either sign
    table, ids = np.zeros((B, T), data.TRACK_DTYPE), np.zeros((B, cap), np.int32)
    for s, (tid, rng_m, rate) in enumerate([(1, 42.46, -0.048), (9, 0.25, 0.032), (10, 9999.9, -39.996), (2 ** 31 - 1, 0.75, 0.0)]):
        t = table[0, s]
        t["id"], t["row"], t["range_age"], t["x"][4], t["v"][4] = tid, s + 1, s, rng_m, rate
        ids[0, s + 1] = tid
    strings, flag = check_text(hip, [6] + [0] * (B - 1), cap, ids=ids, table=table, rate_scale=25.0)
    assert strings[0] == ["", "#1 42.5m -1.2m/s", "#9 0.2m +0.8m/s", "#10 9999.9m -999.9m/s", "#2147483647 0.8m +0.0m/s", ""] and flag == 0


def drawn_on_device(frames, cases, font_size, want_flag=0, records=None):
    """render.draw_captions on device pairs against the host statement per image; returns the device picture."""
    atlas = CC.atlas()
    rows, offsets, packed = CC.pack(cases)
    packed = packed if records is None else records
    strings = render.caption_decode(packed)
    src, flag = cuda(frames), new_flag()
    got = render.draw_captions(src, (cuda(rows), cuda(offsets)), cuda(packed), atlas, font_size=font_size, box_palette=PAL, flag=flag)
    assert got is src
    want = np.stack([render.draw_captions_host(frames[b], rows[offsets[b]:offsets[b + 1]], strings[offsets[b]:offsets[b + 1]], atlas,
                                               font_size, PAL) for b in range(len(frames))])
    bad = int((got.cpu().numpy() != want).any(axis=3).sum())
    print(f"captions {frames.shape} font {font_size} rows {np.diff(offsets).tolist()}: {bad} pixels differ, flag {int(flag)}")
    assert np.array_equal(got.cpu().numpy(), want) and int(flag) == want_flag
    return got, want


@pytest.mark.parametrize("B,ih,iw,font_size", [(2, 64, 96, 10), (1, 33, 47, 8), (1, 17, 17, None), (3, 270, 480, None)])
def test_draw_kernel_equals_the_host_statement(B, ih, iw, font_size):
    assert render.label_font_size(270) == 8 and render.label_font_size(17) == 1
    rng = np.random.default_rng(100 * ih + B)
    frames = rng.integers(0, 256, (B, ih, iw, 3), dtype=np.uint8)
    counts = {1: ([40], [1], [0]), 2: ([40, 1], [0, 40], [0, 0]), 3: ([40, 0, 1], [1, 40, 0])}[B]
    changed = 0
    for per_image in counts:
        cases = [CC.random_case(rng, ih, iw, n) for n in per_image]
        for rows, strings in cases:                          # every image that has rows has one caption in full view
            if len(rows):
                rows[0, 0], rows[0, 3], strings[0] = 0, ih // 3, "#7 1.5m"
        got, want = drawn_on_device(frames, cases, font_size)
        changed += int((want != frames).any())
        assert (want != frames).any() == (sum(per_image) > 0)        # not vacuous: the captions changed the picture
        # host strings go the same way: packed on the host, one copy
        again = render.draw_captions(cuda(frames), (cuda(CC.pack(cases)[0]), cuda(CC.pack(cases)[1])), [s for _, s in cases], CC.atlas(),
                                     font_size=font_size, box_palette=PAL)
        assert torch.equal(again, got)
    assert changed >= 2
    assert torch.equal(render.draw_captions(cuda(frames), (cuda(CC.pack(cases)[0]), cuda(CC.pack(cases)[1])), [s for _, s in cases],
                                            CC.atlas(), font_size=0, box_palette=PAL), cuda(frames))       # size 0 draws nothing


def test_more_than_1024_rows_are_flagged_and_the_first_1024_drawn():
    rng = np.random.default_rng(5)
    frames = rng.integers(0, 256, (2, 64, 96, 3), dtype=np.uint8)
    cases = [CC.random_case(rng, 64, 96, 3), CC.random_case(rng, 64, 96, 1030)]
    cases[1][0][-1] = (0, 10, 90, 30, 2)                     # a row that is dropped would put a long tag across the picture
    cases[1][1][-1] = "#2147483647 9999.9m -999.9m/s"
    _, want = drawn_on_device(frames, cases, 10, want_flag=render.FLAG_BOX_ROWS)
    kept = [cases[0], (cases[1][0][:render.MAX_BOXES], cases[1][1][:render.MAX_BOXES])]
    _, first = drawn_on_device(frames, kept, 10)
    assert np.array_equal(want, first)


def test_corrupt_records_are_clamped():
    """A count of 40 and a code of 200 draw as 32 glyphs with a space: the answer caption_decode states, never a read past the
    record, the glyph table or the blob.  A class outside the palette takes the clamped colour."""
    rng = np.random.default_rng(6)
    frames = rng.integers(0, 256, (1, 64, 96, 3), dtype=np.uint8)
    rows, strings = CC.random_case(rng, 64, 96, 4)
    rows[:, 0], rows[:, 3], rows[:, 4] = (0, 3, -2, 50), (8, 20, 34, 48), (0, 3, 7, -4)
    strings[:] = ["0123456789.-+#m/s 0123456789.-+#", "#1 2.0m", "", "-3.5m/s"]
    records = render.caption_records(strings)
    records[0, 8] = 40
    records.view(np.uint8).reshape(4, 48)[0, 5] = 200
    records[2, 8] = -9                                        # a negative count: the empty caption
    records[3, 9:] = -1                                       # the spare words are not read
    assert render.caption_decode(records) == ["01234 6789.-+#m/s 0123456789.-+#", "#1 2.0m", "", "-3.5m/s"]
    _, want = drawn_on_device(frames, [(rows, strings)], 10, records=records)
    assert (want != frames).any()


def geom_tensor(table):
    return cuda(table.view(np.uint8).reshape(len(table), -1))


def test_ragged_equals_the_fixed_call_per_image_and_writes_nothing_outside():
    atlas, S, cap = CC.atlas(), (64, 64), (320, 100)
    sizes = [(40, 60), (270, 100), (12, 50), (320, 90)]
    table = data.frame_geometry(sizes, S)
    size_tab = atlas.size_table([h for h, _ in sizes])
    assert size_tab.tolist() == [0, 1, -1, 2]
    rng = np.random.default_rng(9)
    cases = [CC.random_case(rng, h, w, n) for (h, w), n in zip(sizes, (12, 40, 5, 30))]
    for (h, w), (rows, strings) in zip(sizes, cases):
        rows[0, 0], rows[0, 3], strings[0] = w - 20, h + 2, "#3 12.0m +0.5m/s"     # reaches for the padding right of and below the image
    rows, offsets, records = CC.pack(cases)
    slots = rng.integers(0, 256, (len(sizes),) + cap + (3,), dtype=np.uint8)     # the padding holds bytes that must stay
    flag = new_flag()
    got = render.draw_captions(cuda(slots), (cuda(rows), cuda(offsets)), cuda(records), atlas, font_size=cuda(size_tab),
                               box_palette=PAL, geom=geom_tensor(table), flag=flag).cpu().numpy()
    assert int(flag) == 0
    for b, (ih, iw) in enumerate(sizes):
        one = (cuda(rows[offsets[b]:offsets[b + 1]]), cuda(np.array([0, len(cases[b][0])], np.int32)))
        fixed = render.draw_captions(cuda(slots[b:b + 1, :ih, :iw]), one, cuda(records[offsets[b]:offsets[b + 1]]), atlas, box_palette=PAL)
        assert np.array_equal(got[b, :ih, :iw], fixed.cpu().numpy()[0]), b
        assert np.array_equal(got[b, :ih, :iw], render.draw_captions_host(slots[b, :ih, :iw], *cases[b], atlas, None, PAL)), b
        outside, before = got[b].copy(), slots[b].copy()
        outside[:ih, :iw] = before[:ih, :iw] = 0
        assert np.array_equal(outside, before), b
    assert np.array_equal(got[2], slots[2]) and not np.array_equal(got[1], slots[1])        # size index -1: nothing is drawn
    with pytest.raises(RuntimeError, match="size_table"):
        render.draw_captions(cuda(slots), (cuda(rows), cuda(offsets)), cuda(records), atlas, geom=geom_tensor(table))


def test_captions_in_a_captured_graph_and_without_a_sync(hip):
    rng = np.random.default_rng(12)
    B, ih, iw, cap, T, atlas = 2, 90, 160, 16, 8, CC.atlas()
    blob, glyphs = atlas.on("cuda")
    bpal = cuda(PAL)

    def inputs():
        frames = rng.integers(0, 256, (B, ih, iw, 3), dtype=np.uint8)
        kept = np.array([cap, 5], np.int32)
        rows, offsets, _ = CC.pack([CC.random_case(rng, ih, iw, int(n)) for n in kept])
        table, ids = track_case(rng, B, cap, T, kept)
        return frames, rows, offsets, kept, ids, np.frombuffer(table.tobytes(), np.int32).reshape(B, T, 16).copy(), table

    first, second = inputs(), inputs()
    frames, rows, offsets, kept, ids, words = (cuda(a) for a in first[:6])
    pic, records, flag = torch.zeros_like(frames), torch.zeros((B * cap, 12), **I32), new_flag()

    def call():
        pic.copy_(frames)
        hip.caption_text(kept, offsets, records, ids=ids, table=words, rate_scale=25.0, flag=flag)
        hip.render_captions(pic, rows, offsets, bpal, records[:rows.shape[0]], blob, glyphs, atlas.size_index(10), flag=flag)
        return pic

    def host(inp):
        strings, _ = render.caption_strings(inp[4], inp[3], inp[6], rate_scale=25.0)
        return np.stack([render.draw_captions_host(inp[0][b], inp[1][inp[2][b]:inp[2][b + 1]], strings[b], atlas, 10, PAL)
                         for b in range(B)])

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        call()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        out = call()
    g.replay()
    torch.cuda.synchronize()
    replayed = out.clone()
    assert np.array_equal(replayed.cpu().numpy(), host(first)) and torch.equal(call(), replayed)
    for t, a in zip((frames, rows, offsets, kept, ids, words), second[:6]):
        t.copy_(torch.from_numpy(np.ascontiguousarray(a)))
    g.replay()
    torch.cuda.synchronize()
    want = host(second)
    assert np.array_equal(out.cpu().numpy(), want) and not np.array_equal(want, host(first))
    # an eager call enqueues and returns: no host synchronisation (the atlas went to this device with the first call)
    render.draw_captions(pic, (rows, offsets), records[:rows.shape[0]], atlas, font_size=10, box_palette=bpal, flag=flag)
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        call()
        render.draw_captions(pic, (rows, offsets), records[:rows.shape[0]], atlas, font_size=10, box_palette=bpal, flag=flag)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    assert np.array_equal(pic.cpu().numpy(), want)


# ---- the pipelines (the setup of tests/test_box_radar.py) -----------------------------------------------------------------
from tests.test_box_radar import B, K, S, frame_points, frames_of, model_of  # noqa: E402

CAP = (48, 64)
RUN_SIZES = {True: [[(40, 56), (48, 64)], [(34, 33), (48, 60)]], False: [[CAP, CAP], [CAP, CAP]]}
FPS = 25
TRACK = dict(max_tracks=256, iou=0.2)                       # three runs of at most 64 rows never fill 256 slots


@pytest.fixture(scope="module")
def A():
    import asy_vrnet_amd
    from asy_vrnet_amd import infer  # noqa: F401
    return asy_vrnet_amd


def label_kw():
    return dict(labels=True, class_names=LC.CLASS_NAMES) if LC.have_pillow() else dict(labels=LC.atlas())


def caption_kw(**kw):
    return kw if CC.have_pillow() else dict(kw, atlas=CC.atlas())


def check_run(A, plain, stage, frames, pts, P, sizes, fps):
    """One run of both pipelines: the captioned picture is the host rule on the picture of the pipeline without captions,
    with the strings the host rule composes from the result's own ids, table and readout."""
    base = plain.run(frames, pts, calib=P).rendered.cpu().numpy()
    res = stage.run(frames, pts, calib=P)
    kept = res.kept.cpu().numpy()
    table = None if res.track_table is None else np.frombuffer(res.track_table.cpu().numpy().tobytes(), data.TRACK_DTYPE).reshape(B, -1)
    strings, bits = render.caption_strings(
        None if res.track_ids is None else res.track_ids.cpu().numpy(), kept, table,
        None if res.box_points is None else res.box_points.cpu().numpy(), None if res.box_radar is None else res.box_radar.cpu().numpy(),
        rate_scale=fps)
    assert res.caption_strings() == strings and int(res.flag) & ~A.infer.FLAG_CANDIDATES == bits
    rows, offsets = stage._draw_rows.cpu().numpy(), stage._offsets.cpu().numpy()
    assert np.array_equal(np.diff(offsets), kept) and kept.max() > 0
    got = res.rendered.cpu().numpy()
    atlas = stage.captions
    for b, (ih, iw) in enumerate(sizes):
        want = render.draw_captions_host(base[b, :ih, :iw], rows[offsets[b]:offsets[b + 1]], strings[b], atlas, None,
                                         stage.box_palette.cpu().numpy())
        assert np.array_equal(got[b, :ih, :iw], want), b
        outside, before = got[b].copy(), base[b].copy()
        outside[:ih, :iw] = before[:ih, :iw] = 0
        assert np.array_equal(outside, before), b
    return strings, not np.array_equal(got, base)


@pytest.mark.parametrize("ragged", [False, True])
def test_frame_pipeline_with_captions(A, ragged):
    model = model_of(A)
    assert render.label_font_size(CAP[0]) == 1
    kw = dict(batch=B, conf_thres=0.05, nms_thres=0.4, max_candidates=64, ragged=ragged, radar_points=K, radar_radius=1,
              track=TRACK, box_radar=True, **label_kw())
    plain = A.FramePipeline(model, CAP, (S, S), **kw)
    stage = A.FramePipeline(model, CAP, (S, S), captions=caption_kw(fps=FPS), **kw)
    assert plain.captions is None and plain.result.captions is None and stage.graph is not None and stage.caption_fps == FPS
    assert stage.captions.sizes == ((1,) if CC.have_pillow() else CC.FIXTURE_SIZES)
    with pytest.raises(RuntimeError, match="not built with captions"):
        plain.result.caption_strings()
    first, second = RUN_SIZES[ragged]
    changed, everything = False, []
    for seed, sizes in [(40, first), (40, first), (41, second)]:          # the second frame repeats the first: every track matches
        frames, (pts, P) = frames_of(seed, sizes, ragged), frame_points(seed + 10, sizes)
        strings, moved = check_run(A, plain, stage, frames, pts, P, sizes, FPS)
        changed |= moved
        everything += [s for image in strings for s in image]
    print(len(everything), "captions in the three runs, the last ones:", everything[-6:])
    assert changed and any("m/s" in s for s in everything) and all(s.startswith("#") for s in everything if s)
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")                    # a run enqueues and returns
    try:
        stage.run(frames, pts, calib=P)
    finally:
        torch.cuda.set_sync_debug_mode("default")


@pytest.mark.parametrize("how", ["no_labels", "no_tracker", "no_readout"])
def test_captions_without_labels_without_a_tracker_and_without_the_readout(A, how):
    model = model_of(A)
    kw = dict(batch=B, conf_thres=0.05, nms_thres=0.4, max_candidates=64, radar_points=K, radar_radius=1, graph=False)
    kw.update(dict(no_labels=dict(track=TRACK, box_radar=True), no_tracker=dict(box_radar=True, **label_kw()),
                   no_readout=dict(track=TRACK))[how])
    fps = FPS if how == "no_labels" else 0
    plain = A.FramePipeline(model, CAP, (S, S), **kw)
    stage = A.FramePipeline(model, CAP, (S, S), captions=caption_kw(fps=fps) if fps else (True if CC.have_pillow() else CC.atlas()), **kw)
    sizes, changed, everything = [CAP, CAP], False, []
    for seed in (40, 40):
        frames, (pts, P) = frames_of(seed, sizes, False), frame_points(seed + 10, sizes)
        strings, moved = check_run(A, plain, stage, frames, pts, P, sizes, fps)
        changed |= moved
        everything += [s for image in strings for s in image]
    assert changed and any(everything)
    if how == "no_tracker":
        assert all(s == "" or s.endswith("m") and "#" not in s for s in everything)
    if how == "no_readout":
        assert all(s.startswith("#") and " " not in s for s in everything if s)


def test_construction_errors(A):
    model = model_of(A)
    kw = dict(batch=B, max_candidates=64, graph=False, radar_points=K)
    for bad, match in ((dict(captions=True, track=True, render=False), "render=True"),
                       (dict(captions=True), "track= or box_radar=True"),
                       (dict(captions={"fps": 25}, track=True), "lacks box_radar=True"),
                       (dict(captions={"fps": 25}, box_radar=True), "lacks track="),
                       (dict(captions={"fps": -1}, track=True, box_radar=True), "fps"),
                       (dict(captions={"colour": 1}, track=True), "captions is None, True"),
                       (dict(captions={"sizes": (1, 2)}, track=True), "ragged"),
                       (dict(captions={"atlas": CC.atlas(), "sizes": (1,)}, track=True), "brings its own"),
                       (dict(captions=5, track=True), "captions is None, True")):
        before = torch.cuda.memory_allocated()
        with pytest.raises(RuntimeError, match=match):
            A.FramePipeline(model, CAP, (S, S), **dict(kw, **bad))
        assert torch.cuda.memory_allocated() == before      # raised before anything was allocated or enqueued
    # a ragged frame whose font size was not built raises in the host validation of run, before anything is enqueued
    atlas = render.GlyphAtlas.from_arrays((1,), CC.atlas().blob, CC.atlas().records[:1])
    pipe = A.FramePipeline(model, (120, 64), (S, S), ragged=True, track=True, captions=atlas, **kw)
    frames = frames_of(3, [(48, 64), (100, 64)], True)
    pts, P = frame_points(13, [(48, 64), (100, 64)])
    before = pipe.frames_u8.clone()
    with pytest.raises(RuntimeError, match="image 1 of 100 rows needs font size 3"):
        pipe.run(frames, pts, calib=P)
    assert torch.equal(pipe.frames_u8, before)


def test_argument_errors(hip):
    B, cap, T, n = 2, 8, 4, 6
    good = dict(kept=torch.zeros(B, **I32), offsets=torch.zeros(B + 1, **I32), captions=torch.zeros((n, 12), **I32),
                ids=torch.zeros((B, cap), **I32), table=torch.zeros((B, T, 16), **I32), box_points=torch.zeros((B, cap), **I32),
                box_radar=torch.zeros((B, cap, 2, 5), device="cuda"), rate_scale=25.0, flag=new_flag())
    hip.caption_text(**good)
    for bad in (dict(kept=None), dict(offsets=None), dict(captions=None), dict(ids=None), dict(ids=None, table=None, box_points=None, box_radar=None),
                dict(box_radar=None), dict(table=torch.zeros((B, T, 15), **I32)), dict(table=torch.zeros((B, 257, 16), **I32)),
                dict(captions=torch.zeros((n, 11), **I32)), dict(kept=good["kept"].long()), dict(offsets=torch.zeros(B, **I32)),
                dict(ids=torch.zeros((B, 1025), **I32), box_points=None, box_radar=None, table=None), dict(rate_scale=-1.0),
                dict(rate_scale=float("nan")), dict(ids=good["ids"].cpu())):
        with pytest.raises(RuntimeError):
            hip.caption_text(**dict(good, **bad))
    assert hip._lib.vrnet_caption_text_f32(None, None, None, B, cap, None, 0, None, None, 0.0, None, n, None, None) != 0
    atlas = CC.atlas()
    blob, glyphs = atlas.on("cuda")
    good = dict(picture=torch.zeros((B, 32, 48, 3), dtype=torch.uint8, device="cuda"), boxes=torch.zeros((n, 5), **I32),
                box_offsets=torch.zeros(B + 1, **I32), box_palette=cuda(PAL), captions=torch.zeros((n, 12), **I32), blob=blob,
                records=glyphs, size_index=0, flag=new_flag())
    hip.render_captions(**good)
    tab, geom = torch.zeros(B, **I32), geom_tensor(data.frame_geometry([(32, 48)] * B, (64, 64)))
    hip.render_captions(**dict(good, size_index=tab, geom=geom))
    for bad in (dict(picture=None), dict(boxes=None), dict(box_offsets=None), dict(box_palette=None), dict(captions=None), dict(blob=None),
                dict(records=None), dict(size_index=-1), dict(size_index=len(atlas.sizes)), dict(records=glyphs[:, :17]),
                dict(captions=torch.zeros((n, 8), **I32)), dict(captions=torch.zeros((n + 1, 12), **I32)),
                dict(box_palette=torch.zeros((257, 3), dtype=torch.uint8, device="cuda")), dict(picture=good["picture"].cpu()),
                dict(size_index=tab), dict(geom=geom), dict(geom=geom, size_index=None), dict(geom=geom[:1], size_index=tab)):
        with pytest.raises(RuntimeError):
            hip.render_captions(**dict(good, **bad))
    assert not good["picture"].any().item() and int(good["flag"]) == 0
