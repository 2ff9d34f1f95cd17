"""The fixed-size detection chips on the device (csrc/chips.hip: vrnet_chip_boxes_u8) against their host statement,
render.chip_boxes_host (Pillow itself) and render.chip_table, bit for bit: the chips, the float chips, the table and the
summary; every buffer is pre-filled with 0xAB and must still hold that behind the last row.  Then the surface above the
kernels: render.chip_boxes, FramePipeline(chips=...) fixed-size and ragged, and infer.predict_dir."""
import inspect
import os

import numpy as np
import pytest
import torch

from asy_vrnet_amd import data, decode, infer, render

pytestmark = pytest.mark.gpu
IH, IW = 37, 53
FILL = 0xAB
MEAN, SD = np.array([0.485, 0.456, 0.406]), np.array([0.229, 0.224, 0.225])
# tests/test_crops.py's EDGE_ROWS
EDGE_ROWS = np.array([[7, 9, 8, 10, 0],               # 1 x 1
                      [5, 6, 5, 20, 0],               # empty: w == 0
                      [4, 3, 5, 10, 1],               # 1 x 7
                      [10, 2, 12, 5, 1],              # 2 x 3
                      [30, 6, 20, 9, 2],              # inverted
                      [11, 20, 14, 25, 2],            # 3 x 5
                      [0, 0, IW, IH, 3],              # the whole frame
                      [5, 6, 20, 6, 0],               # empty: h == 0
                      [48, 30, 53, 35, 3],            # 5 x 5 in the corner
                      [0, 33, IW, 36, 0],             # 53 x 3: whole rows
                      [-9, -9, 2, 3, 1],              # hostile: 2 x 3 after the clamp
                      [50, 35, 99, 99, 1]], np.int32)  # hostile: 3 x 2 after the clamp


def cuda(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def frames_of(seed, B, ih=IH, iw=IW, high=256):
    return np.random.default_rng(seed).integers(0, high, (B, ih, iw, 3), dtype=np.uint8)


def normalised(chip):
    """batch_formats_kernel's arithmetic in numpy doubles, rounded once: (sh, sw, 3) uint8 -> (3, sh, sw) float32."""
    return (((chip.astype(np.float64) / 255.0) - MEAN) / SD).astype(np.float32).transpose(2, 0, 1)


def launch(frames, rows, offsets, size, letterbox, extra=5, geom=None, f32=True):
    """One hip.chip_boxes call on n_cap = len(rows) + extra rows (the rows behind N hold a box that would be a crop) ->
    (chips, float chips as bytes, table (n_cap) records, summary, flag)."""
    import asy_vrnet_amd.hip as hip
    n_cap, (sh, sw) = len(rows) + extra, size
    padded = np.concatenate([rows, np.tile(np.array([[0, 0, 5, 5, 0]], np.int32), (extra, 1))]).astype(np.int32)
    chips = torch.full((n_cap, sh, sw, 3), FILL, dtype=torch.uint8, device="cuda")
    raw = torch.full((n_cap * 3 * sh * sw * 4,), FILL, dtype=torch.uint8, device="cuda")
    table = torch.full((n_cap, 8), -7, dtype=torch.int32, device="cuda")
    summary = torch.full((1,), -7, dtype=torch.int32, device="cuda")
    flag = torch.zeros(1, dtype=torch.int32, device="cuda")
    ws = torch.full((hip.chip_workspace_bytes(n_cap, sh, sw),), FILL, dtype=torch.uint8, device="cuda")
    hip.chip_boxes(cuda(frames), cuda(padded), cuda(offsets), chips, table, summary, ws, letterbox=letterbox,
                   chips_f32=raw.view(torch.float32).view(n_cap, 3, sh, sw) if f32 else None, geom=geom, flag=flag)
    torch.cuda.synchronize()
    return (chips.cpu().numpy(), raw.cpu().numpy().reshape(n_cap, -1), table.cpu().numpy().reshape(-1).view(render.CHIP_RECORD),
            summary.cpu().numpy().tolist(), int(flag))


def check(frames, rows, offsets, size, letterbox, sizes=None, geom=None, extra=5, want_flag=0):
    """The kernels against the host rule on one call; images: each picture at its own size.  Returns the table."""
    B = len(frames)
    sizes = [(frames.shape[1], frames.shape[2])] * B if sizes is None else sizes
    images = [frames[b, :sizes[b][0], :sizes[b][1]] for b in range(B)]
    want_table, N = render.chip_table(rows, offsets, np.array(sizes), size, letterbox)
    chips, raw, table, summary, flag = launch(frames, rows, offsets, size, letterbox, extra, geom)
    assert summary == [N] and flag == want_flag
    assert np.array_equal(table[:N], want_table), (table[:N], want_table)
    assert table[N:].tolist() == [(-1, 0, 0, 0, 0, 0, 0, 0)] * (len(table) - N)       # behind N, whatever the rows hold
    for n in range(N):
        want = render.chip_boxes_host(images[want_table["image"][n]], rows[n:n + 1], size, letterbox)[0]
        assert np.array_equal(chips[n], want), (n, want_table[n], np.argwhere(chips[n] != want)[:4].tolist())
        assert np.array_equal(raw[n].view(np.float32), normalised(want).reshape(-1)), n
    assert (chips[N:] == FILL).all() and (raw[N:] == FILL).all()         # nothing is written behind the last row
    # without the float form the bytes are the same
    assert np.array_equal(launch(frames, rows, offsets, size, letterbox, extra, geom, f32=False)[0], chips)
    return want_table


@pytest.mark.parametrize("letterbox", [False, True])
@pytest.mark.parametrize("size", [(8, 8), (5, 7), (16, 12)])
def test_every_edge_in_one_call(size, letterbox):
    frames = frames_of(1, 2)
    offsets = np.array([0, 0, len(EDGE_ROWS)], np.int32)                   # image 0 has no rows
    table = check(frames, EDGE_ROWS, offsets, size, letterbox)
    assert (table["state"] == 2).sum() == 3 and (table["image"] == 1).all()
    shapes = set(zip(table["w"].tolist(), table["h"].tolist()))
    assert {(1, 1), (1, 7), (2, 3), (3, 5), (IW, IH), (53, 3)} <= shapes   # upscales and downscales in the same call


@pytest.mark.parametrize("letterbox", [False, True])
def test_the_skipped_passes(letterbox):
    rows = np.array([[3, 3, 11, 20, 0],               # 8 x 17: the width is sw
                     [3, 3, 20, 11, 1],               # 17 x 8: the height is sh
                     [3, 3, 11, 11, 2]], np.int32)    # 8 x 8: the chip is the crop
    frames = frames_of(2, 1)
    check(frames, rows, np.array([0, 3], np.int32), (8, 8), letterbox)
    assert np.array_equal(launch(frames, rows, np.array([0, 3], np.int32), (8, 8), letterbox)[0][2], frames[0, 3:11, 3:11])


@pytest.mark.parametrize("letterbox", [False, True])
@pytest.mark.parametrize("size", [(8, 8), (5, 7)])
def test_a_300_by_400_frame(size, letterbox):
    """Scale 57 with 229 taps, many chunks of source rows per band, and the letterbox's max(.., 1)."""
    rows = np.array([[0, 0, 400, 300, 0], [0, 100, 400, 102, 1], [200, 3, 208, 298, 2], [100, 100, 108, 108, 3]], np.int32)
    table = check(frames_of(3, 1, 300, 400), rows, np.array([0, 4], np.int32), size, letterbox)
    if letterbox:
        assert table["nh"][1] == 1 and table["nw"][2] == 1


@pytest.mark.parametrize("width", [1000, 1100])
def test_both_sides_of_the_weight_cache(width):
    """8 columns from 1000 and 995 (501 and 499 taps an index, 4008 and 3992 weights: kept in LDS) and from 1100 and 1095 (551
    and 549 taps, 4408 and 4392 weights, above the 4096 the kernel keeps: recomputed per tap).  The same bytes either way."""
    frames = frames_of(5, 1, 4, width)
    rows = np.array([[0, 0, width, 4, 0], [3, 1, width - 2, 3, 1]], np.int32)
    for letterbox in (False, True):
        check(frames, rows, np.array([0, 2], np.int32), (8, 8), letterbox, extra=1)


@pytest.mark.parametrize("letterbox", [False, True])
def test_the_largest_and_the_smallest_chip(letterbox):
    frames = frames_of(4, 1)
    rows = np.array([[11, 20, 14, 25, 2]], np.int32)                       # 3 x 5
    check(frames, rows, np.array([0, 1], np.int32), (256, 256), letterbox, extra=1)
    check(frames, EDGE_ROWS, np.array([0, len(EDGE_ROWS)], np.int32), (1, 1), letterbox)


def test_ragged_chips_hold_no_padding_and_a_clamped_record_sets_the_flag():
    cap, sizes = (40, 56), [(20, 31), (37, 53)]
    frames = np.full((2,) + cap + (3,), 255, np.uint8)                      # the padding is 255, no picture byte is
    for b, (ih, iw) in enumerate(sizes):
        frames[b, :ih, :iw] = frames_of(8 + b, 1, ih, iw, high=200)[0]
    rows = np.array([[25, 10, 31, 20, 0],             # reaches the image's right and lower edge, not the slot's
                     [0, 0, 56, 40, 1],               # hostile: the whole slot -> the whole image
                     [30, 19, 100, 100, 2],           # hostile: one pixel stays
                     [31, 0, 56, 40, 2],              # wholly in the padding: empty
                     [0, 0, 53, 37, 0],               # image 1: its whole picture
                     [50, 30, 56, 40, 1],             # hostile: beyond image 1, inside the slot
                     [-5, -5, 3, 3, 3]], np.int32)
    offsets = np.array([0, 4, 7], np.int32)
    geom = data.geometry_bytes(data.frame_geometry(sizes, (64, 64), True, cap)).cuda()
    for letterbox in (False, True):
        table = check(frames, rows, offsets, (8, 8), letterbox, sizes, geom)
        assert table["w"].tolist() == [6, 31, 1, 0, 53, 3, 3] and table["state"][3] == 2
        both = launch(frames, rows, offsets, (8, 8), letterbox, geom=geom)[0]
        assert (both[[0, 1, 4, 5, 6]] != 255).all()                         # not stretched: no padding byte in a chip
        # each image alone, at its own size, gives the same chips
        for b, (lo, hi) in enumerate(((0, 4), (4, 7))):
            alone = np.ascontiguousarray(frames[b:b + 1, :sizes[b][0], :sizes[b][1]])
            one = launch(alone, rows[lo:hi], np.array([0, hi - lo], np.int32), (8, 8), letterbox)[0]
            assert np.array_equal(one[:hi - lo], both[lo:hi]), b
    # a record larger than its slot is clamped to the slot and reported
    hostile = geom.clone()
    hostile.view(torch.int32).view(2, -1)[0, 0] = cap[0] + 9
    check(frames, rows, offsets, (8, 8), False, [(cap[0], 31), sizes[1]], hostile, want_flag=256)


def test_a_record_above_its_slot_and_an_empty_one():
    """Image 1's record is no image.  ih = 25 in a slot of 16 rows is clamped to the slot, so its rows are cut as in a 16 x 20
    image; ih = 0 leaves it no pixel, so both its rows are empty crops: grey chips.  Either way FLAG_GEOMETRY, and image 0 as
    ever."""
    import asy_vrnet_amd.hip as hip
    cap, good = (16, 24), (11, 17)
    frames = frames_of(20, 2, *cap)
    rows = np.array([[2, 1, 9, 8, 0],                 # image 0: 7 x 7
                     [10, 5, 30, 30, 1],              # hostile: 7 x 6 after the clamp to 17 x 11
                     [3, 2, 8, 14, 2],                # image 1: 5 x 12
                     [0, 10, 24, 40, 3]], np.int32)   # 20 x 6 of 16 x 20
    offsets = np.array([0, 2, 4], np.int32)
    geom = data.geometry_bytes(data.frame_geometry([good, (16, 20)], (64, 64), True, cap)).cuda()
    images = [frames[0, :11, :17], frames[1, :16, :20]]
    for ih, records in ((25, [(1, 5, 12, 8, 8, 0, 0, 1), (1, 20, 6, 8, 8, 0, 0, 1)]), (0, [(1, 0, 0, 0, 0, 0, 0, 2)] * 2)):
        hostile = geom.clone()
        hostile.view(torch.int32).view(2, -1)[1, 0] = ih
        chips, raw, table, summary, flag = launch(frames, rows, offsets, (8, 8), False, geom=hostile)
        assert flag == hip.FLAG_GEOMETRY == 256 and summary == [4]
        assert table[:4].tolist() == [(0, 7, 7, 8, 8, 0, 0, 1), (0, 7, 6, 8, 8, 0, 0, 1)] + records
        for n in range(4):
            want = render.chip_boxes_host(images[n // 2], rows[n:n + 1], (8, 8), False)[0] if ih or n < 2 else np.full((8, 8, 3), 128)
            assert np.array_equal(chips[n], want) and np.array_equal(raw[n].view(np.float32), normalised(want).reshape(-1)), n


def test_argument_checks():
    import asy_vrnet_amd.hip as hip
    frames, rows, offsets = cuda(frames_of(12, 2)), cuda(EDGE_ROWS), cuda(np.array([0, 0, len(EDGE_ROWS)], np.int32))
    n = len(EDGE_ROWS)
    chips = torch.zeros((n, 8, 8, 3), dtype=torch.uint8, device="cuda")
    table, summary = torch.zeros((n, 8), dtype=torch.int32, device="cuda"), torch.zeros(1, dtype=torch.int32, device="cuda")
    ws = torch.zeros(hip.chip_workspace_bytes(n, 8, 8), dtype=torch.uint8, device="cuda")
    assert hip.chip_workspace_bytes(n, 8, 8) == n * 16 * 16
    with pytest.raises(RuntimeError, match="sides in 1..256"):
        hip.chip_boxes(frames, rows, offsets, torch.zeros((n, 8, 257, 3), dtype=torch.uint8, device="cuda"), table, summary, ws)
    with pytest.raises(RuntimeError, match="sides in 1..256"):
        hip.chip_workspace_bytes(n, 0, 8)
    with pytest.raises(RuntimeError, match="workspace must be"):
        hip.chip_boxes(frames, rows, offsets, chips, table, summary, ws[:-1])
    with pytest.raises(RuntimeError, match="shape \\(3,\\)"):
        hip.chip_boxes(frames, rows, offsets[:2], chips, table, summary, ws)
    with pytest.raises(RuntimeError, match=f"shape \\({n}, 8\\)"):
        hip.chip_boxes(frames, rows, offsets, chips, table[:3], summary, ws)
    with pytest.raises(RuntimeError, match=f"shape \\({n}, 3, 8, 8\\)"):
        hip.chip_boxes(frames, rows, offsets, chips, table, summary, ws, chips_f32=torch.zeros((n, 8, 8, 3), device="cuda"))
    with pytest.raises(RuntimeError, match="size is"):
        render.chip_boxes(frames, (rows, offsets), (8, 300))
    torch.cuda.synchronize()


def test_chip_boxes_takes_the_list_of_non_max_suppression():
    frames = frames_of(13, 3)
    rng = np.random.default_rng(14)
    results = []
    for n in (4, 0, 7):
        top, left = rng.uniform(-5, IH, n), rng.uniform(-5, IW, n)
        det = np.stack([top, left, top + rng.uniform(0, 25, n), left + rng.uniform(0, 25, n), np.full(n, .9), np.full(n, .9),
                        rng.integers(0, 4, n)], 1).astype(np.float32)
        results.append(det if n else None)
    for letterbox in (False, True):
        chips = render.chip_boxes(frames, results, (16, 12), letterbox=letterbox, normalised=True)
        got = chips.images()
        assert int(chips.flag) == 0 and [len(g) for g in got] == [4, 0, 7] and chips.summary.tolist() == [11]
        f32 = chips.chips_f32.cpu().numpy()
        n = 0
        for b in range(3):
            rows = render.box_rows([results[b]], (IH, IW), 4)[0]
            want = render.chip_boxes_host(frames[b], rows, (16, 12), letterbox)
            for g, w in zip(got[b], want):
                assert g.shape == (16, 12, 3) and np.array_equal(g, w) and np.array_equal(f32[n], normalised(w)), (b, n)
                n += 1
    # the device pair gives the same, and a single frame counts as B = 1
    rows, offsets = render.box_rows(results, (IH, IW), 4)[:2]
    pair = render.chip_boxes(cuda(frames), (cuda(rows), cuda(offsets)), (16, 12), letterbox=True)
    assert pair.chips_f32 is None and all(np.array_equal(x, y) for b in range(3) for x, y in zip(pair.images()[b], got[b]))
    one = render.chip_boxes(frames[2], results[2:], (5, 7)).images()
    assert len(one) == 1 and len(one[0]) == 7 and one[0][0].shape == (5, 7, 3)
    assert render.chip_boxes(frames[:1], [None], (5, 7)).images() == [[]]


# ---- the pipeline: the sizes and the threshold of tests/test_crops.py ------------------------------------------------------
NC, S, F, CAP, NMS_THRES = 4, (64, 64), (40, 56), 64, 0.4
RAGGED_CAP, RAGGED_SIZES = (48, 68), [(40, 56), (23, 41)]
FIXED_CHIPS = dict(size=(16, 12), letterbox=True, normalised=True)
RAGGED_CHIPS = (8, 8)


def inputs(seed, sizes):
    rng = np.random.default_rng(seed)
    frames = [rng.integers(0, 256, tuple(s) + (3,), dtype=np.uint8) for s in sizes]
    return frames, (rng.standard_normal((len(sizes), 4) + S) * 2.0 + 1.0).astype(np.float32)


@pytest.fixture(scope="module")
def model():
    import asy_vrnet_amd as A
    net = A.EfficientVRNet(NC, 9, "nano", img_size=S[0]).cuda().eval()
    A.randomize_state_dict(net.state_dict(), seed=4)
    return net


def twelfth_score(model, images, radar):
    """The 12th-largest score of the batch, the threshold tests/test_infer.py uses."""
    with torch.no_grad():
        det, _ = model(images, cuda(radar))
    pred = decode.decode_outputs(det, S)
    return float((pred[..., 4] * pred[..., 5:5 + NC].amax(-1)).flatten().sort(descending=True).values[11])


@pytest.fixture(scope="module")
def fixed(model):
    import asy_vrnet_amd as A
    first, second = inputs(74, [F] * 2), inputs(75, [F] * 2)
    first, second = (np.stack(first[0]), first[1]), (np.stack(second[0]), second[1])
    conf = twelfth_score(model, data.device_letterbox(cuda(first[0]), S)[0], first[1])
    kw = dict(batch=2, conf_thres=conf, nms_thres=NMS_THRES, max_candidates=CAP)
    return dict(first=first, second=second, kw=kw, chips=A.FramePipeline(model, F, S, chips=FIXED_CHIPS, **kw))


@pytest.fixture(scope="module")
def ragged(model):
    import asy_vrnet_amd as A
    import asy_vrnet_amd.hip as hip
    first, second = inputs(76, RAGGED_SIZES), inputs(77, RAGGED_SIZES[::-1])
    kw = dict(batch=2, nms_thres=NMS_THRES, max_candidates=CAP, ragged=True)
    slots = np.zeros((2,) + RAGGED_CAP + (3,), np.uint8)
    for b, f in enumerate(first[0]):
        slots[b, :f.shape[0], :f.shape[1]] = f
    geom = data.geometry_bytes(data.frame_geometry(RAGGED_SIZES, S, True, RAGGED_CAP)).cuda()
    images = torch.empty((2, 3) + S, device="cuda")
    hip.letterbox_ragged(cuda(slots), None, geom, S[0], S[1], data.default_max_taps(RAGGED_CAP, S), images=images)
    kw["conf_thres"] = twelfth_score(model, images, first[1])
    # with the crops in front: the chip launches sit behind the crop launches
    return dict(first=first, second=second, kw=kw, chips=A.FramePipeline(model, RAGGED_CAP, S, chips=RAGGED_CHIPS, crops=True, **kw))


def host_chips(frames, detections, size, letterbox):
    return [render.chip_boxes_host(f, render.box_rows([d], f.shape[:2], NC)[0], size, letterbox) for f, d in zip(frames, detections)]


def same_chips(got, want):
    assert len(got) == len(want)
    for g, w in zip(got, want):
        assert len(g) == len(w)
        assert all(x.dtype == np.uint8 and x.shape == y.shape and np.array_equal(x, y) for x, y in zip(g, w))


@pytest.mark.parametrize("kind", ["fixed", "ragged"])
def test_pipeline_chips_are_the_host_chips(kind, request):
    setup = request.getfixturevalue(kind)
    pipe = setup["chips"]
    cfg = infer.chip_config(FIXED_CHIPS if kind == "fixed" else RAGGED_CHIPS)
    assert pipe.graph is not None and pipe.chips == cfg
    res = pipe.run(*setup["first"])
    dets = res.detections()
    print(kind, "conf_thres", setup["kw"]["conf_thres"], "kept per image", [len(d) for d in dets])
    assert max(len(d) for d in dets) >= 2                                  # not vacuous: an image with two or more detections
    assert res.chips is pipe.result.chips and res.chips.chips.shape == (2 * pipe.cap,) + cfg["size"] + (3,)
    first = res.chips.images()
    want = host_chips(setup["first"][0], dets, cfg["size"], cfg["letterbox"])
    same_chips(first, want)
    N = sum(len(d) for d in dets)
    assert int(res.flag) == 0 and res.chips.summary.tolist() == [N]
    table = res.chips.table.cpu().numpy().reshape(-1).view(render.CHIP_RECORD)
    assert (table["state"][:N] >= 1).all() and (table["image"][N:] == -1).all() and (table["state"][N:] == 0).all()
    if cfg["normalised"]:
        f32 = res.chips.chips_f32[:N].cpu().numpy()
        assert np.array_equal(f32, np.stack([normalised(c) for g in want for c in g]))
    else:
        assert res.chips.chips_f32 is None
    if kind == "ragged":                                                    # the crops in front of the chips are what they were
        crops = res.crops.images()
        assert [len(g) for g in crops] == [len(g) for g in first]
    # a second replay on the same frames gives the same bytes
    packed = res.chips._packed.clone()
    res = pipe.run(*setup["first"])
    assert torch.equal(res.chips._packed, packed)
    # a replay on other frames gives the chips of those frames
    res = pipe.run(*setup["second"])
    second = res.chips.images()
    same_chips(second, host_chips(setup["second"][0], res.detections(), cfg["size"], cfg["letterbox"]))
    assert int(res.flag) == 0 and sum(len(g) for g in second) > 0
    assert any(len(a) != len(b) or any(not np.array_equal(x, y) for x, y in zip(a, b)) for a, b in zip(first, second))


def test_chips_keyword_checks(model, fixed):
    import asy_vrnet_amd as A
    for bad in ((0, 8), (8, 8, 8), {"letterbox": True}, {"size": (8, 8), "filter": "nearest"}, True):
        with pytest.raises(RuntimeError, match="chips"):
            A.FramePipeline(model, F, S, chips=bad, **fixed["kw"])
    assert infer.chip_config(None) is None
    assert infer.chip_config((5, 7)) == dict(size=(5, 7), letterbox=False, normalised=False)


def recorded_calls(monkeypatch):
    """A list that every public wrapper of hip.py appends its name to when it is called, in call order."""
    import asy_vrnet_amd.hip as hip
    calls = []
    quiet = ("ptr", "stream", "empty", "tuning_build", "kernel_launches", "last_kernel")
    for name, f in inspect.getmembers(hip, inspect.isfunction):
        if f.__module__ != hip.__name__ or name.startswith("_") or name in quiet or name.endswith("_bytes") or name.endswith("_ok"):
            continue

        def counted(*a, _f=f, _n=name, **k):
            calls.append(_n)
            return _f(*a, **k)
        monkeypatch.setattr(hip, name, counted)
    return calls


def test_without_chips_the_chain_issues_the_calls_it_issued_before(model, fixed, monkeypatch):
    """Every wrapper of hip.py the chain calls, in order: chips=None never reaches chip_boxes and issues the calls of a
    pipeline built without the keyword, and chips=(8, 8) adds exactly that one call, right behind detect_finish (behind
    crop_boxes with crops)."""
    import asy_vrnet_amd as A
    calls = recorded_calls(monkeypatch)

    def chain(**extra):
        pipe = A.FramePipeline(model, F, S, graph=False, **extra, **fixed["kw"])
        del calls[:]
        with torch.no_grad():
            pipe._chain()
        torch.cuda.synchronize()
        return list(calls)
    without, none, chips = chain(), chain(chips=None), chain(chips=(8, 8))
    assert none == without and "chip_boxes" not in without and without.count("detect_finish") == 1
    at = chips.index("chip_boxes")
    assert chips[at - 1] == "detect_finish" and chips[:at] + chips[at + 1:] == without
    both, crops = chain(chips=(8, 8), crops=True), chain(crops=True)
    at = both.index("chip_boxes")
    assert both[at - 1] == "crop_boxes" and both[at - 2] == "detect_finish" and both[:at] + both[at + 1:] == crops


ALL_STAGES = dict(dehaze=True, ace=True, crops=True, chips=(8, 8), radar_points=16, calib=np.array(
    [[40.0, 0, 28, 0], [0, 40.0, 20, 0], [0, 0, 1, 0]], np.float32), box_radar=True, track=True, captions=dict(fps=25.0),
    regions=True, labels=True, class_names=("a", "b", "c", "d"), heatmap=True, graph=False)
# recorded on the commit in front of the stage objects, where `_chain` named every stage in an `if` of its own
ALL_STAGES_CALLS = {
    "fixed": ["dehaze", "ace", "letterbox", "radar_map", ("forward", 677), "decode_outputs", "detect_select", "nms_capped",
              "detect_finish", "crop_boxes", "chip_boxes", "box_radar", "track_update", "caption_text", "seg_predict",
              "seg_regions", "label_index", "render", "render_labels", "render_captions", "heatmap"],
    "ragged": ["dehaze", "ace", "letterbox", "radar_map", ("forward", 677), "decode_outputs", "detect_select", "nms_capped",
               "detect_finish", "crop_boxes", "chip_boxes", "box_radar", "track_update", "caption_text", "seg_predict",
               "seg_regions", "label_index", "render", "render_labels", "render_captions", "heatmap"]}


@pytest.mark.parametrize("kind", ["fixed", "ragged"])
def test_with_every_stage_on_the_chain_issues_the_calls_it_issued_before(kind, model, request, monkeypatch):
    """The launch order of the ten optional stages, pinned: one pass of the chain with all of them on issues exactly the
    calls, in the order, that it issued when every stage was a block of `_chain`.  The several hundred calls of the model's
    forward, which the chain issues as one, stand in the list as ("forward", their number)."""
    import asy_vrnet_amd as A
    kw = request.getfixturevalue(kind)["kw"]
    pipe = A.FramePipeline(model, (48, 64) if kind == "fixed" else RAGGED_CAP, S, **ALL_STAGES, **kw)
    calls, forward = recorded_calls(monkeypatch), []
    hooks = [model.register_forward_pre_hook(lambda *a: forward.append(len(calls))),
             model.register_forward_hook(lambda *a: forward.append(len(calls)))]
    with torch.no_grad():
        pipe._chain()
    torch.cuda.synchronize()
    for h in hooks:
        h.remove()
    start, end = forward
    calls = calls[:start] + [("forward", end - start)] + calls[end:]
    print(kind, calls)
    assert calls == ALL_STAGES_CALLS[kind]


def test_predict_dir_saves_the_chips_of_every_picture(ragged, tmp_path):
    from PIL import Image
    sizes = [(40, 56), (48, 68), (23, 41)]
    frames, radar = inputs(78, sizes)
    src, radar_root, dst = tmp_path / "in", tmp_path / "radar", tmp_path / "out"
    src.mkdir()
    radar_root.mkdir()
    names = [f"{1600000000 + b}.{b:05d}.png" for b in range(3)]
    for b, n in enumerate(names):
        Image.fromarray(frames[b]).save(src / n)
        np.savez(radar_root / (data.frame_id(n) + ".npz"), radar[b])
    out = infer.predict_dir(ragged["chips"], str(src), str(radar_root), str(dst))      # batch 2: the last call repeats picture 2
    assert [n for n, _ in out] == names
    want = {}
    for (n, det), frame in zip(out, frames):
        for i, chip in enumerate(host_chips([frame], [det], RAGGED_CHIPS, False)[0]):
            want[f"{n[:-4]}_chip_{i}.png"] = chip
    print("detections per picture", [len(d) for _, d in out], "chips saved", len(want))
    assert len(want) >= 2 and sorted(os.listdir(dst / "img_chip")) == sorted(want)
    for name, chip in want.items():
        assert np.array_equal(np.array(Image.open(dst / "img_chip" / name)), chip), name
    assert "img_chip" in os.listdir(dst) and "img_crop" in os.listdir(dst)
