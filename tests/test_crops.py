"""The detection crops on the device (csrc/crops.hip: vrnet_crop_boxes_u8) against their host statement, render.crop_boxes_host
and render.crop_layout, bit for bit: the table, the summary, the flag and the used prefix of the arena, whose pad pixels are
zero; the arena is pre-filled with 0xAB and everything from 3 * used on must still be 0xAB.  Then the surface above the
kernels: render.crop_boxes, FramePipeline(crops=...) fixed-size and ragged, and infer.predict_dir."""
import inspect
import os

import numpy as np
import pytest
import torch

from asy_vrnet_amd import data, decode, infer, render

pytestmark = pytest.mark.gpu
IH, IW = 37, 53                       # a frame row of 159 bytes: no multiple of 4
FILL = 0xAB


def cuda(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def frames_of(seed, B, ih=IH, iw=IW, high=256):
    return np.random.default_rng(seed).integers(0, high, (B, ih, iw, 3), dtype=np.uint8)


def launch(frames, rows, offsets, capacity, extra=5, geom=None):
    """One hip.crop_boxes call on n_cap = len(rows) + extra rows (the rows behind N hold a box that would be a crop) ->
    (arena bytes, table (n_cap) records, summary, flag)."""
    import asy_vrnet_amd.hip as hip
    n_cap = len(rows) + extra
    padded = np.concatenate([rows, np.tile(np.array([[0, 0, 5, 5, 0]], np.int32), (extra, 1))]).astype(np.int32)
    arena = torch.full((3 * capacity,), FILL, dtype=torch.uint8, device="cuda")
    table = torch.full((n_cap, 4), -7, dtype=torch.int32, device="cuda")
    summary = torch.full((2,), -7, dtype=torch.int32, device="cuda")
    flag = torch.zeros(1, dtype=torch.int32, device="cuda")
    hip.crop_boxes(cuda(frames), cuda(padded), cuda(offsets), arena, table, summary, geom=geom, flag=flag)
    torch.cuda.synchronize()
    return arena.cpu().numpy(), table.cpu().numpy().reshape(-1).view(render.CROP_RECORD), summary.cpu().numpy().tolist(), int(flag)


def expected_arena(images, rows, table, used):
    """The used prefix of the arena by the host rule: the crops of `crop_boxes_host` at their offsets, zero in between."""
    want = np.zeros(3 * used, np.uint8)
    for n, (off, w, h, b) in enumerate(table.tolist()):
        if off >= 0 and w > 0:
            crop = render.crop_boxes_host(images[b], rows[n:n + 1])[0]
            assert crop.shape == (h, w, 3)
            want[3 * off:3 * (off + w * h)] = crop.reshape(-1)
    return want


def check(frames, rows, offsets, capacity, sizes=None, geom=None, extra=5):
    """The kernel against the host rule on one call; images: each picture at its own size.  Returns (table, used, flag)."""
    B = len(frames)
    sizes = [(frames.shape[1], frames.shape[2])] * B if sizes is None else sizes
    images = [frames[b, :sizes[b][0], :sizes[b][1]] for b in range(B)]
    want_table, (N, used), want_flag = render.crop_layout(rows, offsets, np.array(sizes), capacity)
    arena, table, summary, flag = launch(frames, rows, offsets, capacity, extra, geom)
    assert summary == [N, used] and flag == want_flag
    assert np.array_equal(table[:N], want_table), (table[:N], want_table)
    assert table[N:].tolist() == [(0, 0, 0, -1)] * extra                   # behind N: empty, whatever the rows hold
    assert np.array_equal(arena[:3 * used], expected_arena(images, rows, want_table, used))
    assert (arena[3 * used:] == FILL).all()                                 # nothing is written beyond the used prefix
    return want_table, used, flag


# w x h of image 1's crops: w * h * 3 % 4 is 3, 2, 1 for w * h % 4 = 1, 2, 3; widths 1, 2, 3, 5 and the whole row of 53
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


def test_every_edge_in_one_call():
    frames = frames_of(1, 2)
    offsets = np.array([0, 0, len(EDGE_ROWS)], np.int32)                   # image 0 has no rows
    table, used, flag = check(frames, EDGE_ROWS, offsets, 4096)
    sizes = table["w"].astype(int) * table["h"]
    assert {int(s) * 3 % 4 for s in sizes if s} == {1, 2, 3} and {1, 2, 3, 5, 53} <= set(table["w"].tolist())
    assert (sizes == 0).sum() == 3 and flag == 0 and (table["image"] == 1).all()
    assert (sizes[sizes > 0] % 4 != 0).any()                               # pad pixels exist, and check() saw them as zeros


def tiny_rows(n, seed, ih=IH, iw=IW):
    rng = np.random.default_rng(seed)
    l, t = rng.integers(-2, iw, n), rng.integers(-2, ih, n)
    return np.stack([l, t, l + rng.integers(0, 5, n), t + rng.integers(0, 5, n), rng.integers(0, 4, n)], 1).astype(np.int32)


def test_300_rows_cross_the_chunk_and_the_running_base():
    rows = tiny_rows(300, 2)
    offsets = np.array([0, 130, 130, 300], np.int32)
    table, used, flag = check(frames_of(3, 3), rows, offsets, 8192)
    assert flag == 0 and (table["w"] > 0).sum() > 150 and (table["w"] == 0).sum() > 20
    assert table["offset"][299] > table["offset"][255] > 0 and set(table["image"].tolist()) == {0, 2}


def test_more_images_than_one_chunk_of_the_layout():
    """300 images (the layout kernel walks the images in chunks of 256 too), most of them without rows."""
    B = 300
    counts = np.zeros(B, np.int64)
    counts[[0, 7, 254, 255, 256, 257, 299]] = [3, 1, 2, 4, 1, 5, 2]
    offsets = np.concatenate([[0], np.cumsum(counts)]).astype(np.int32)
    table, used, flag = check(frames_of(5, B, 9, 11), tiny_rows(int(counts.sum()), 4, 9, 11), offsets, 2048)
    assert table["image"].tolist() == np.repeat(np.arange(B), counts).tolist() and (table["w"] > 0).sum() > 9


def test_the_first_dropped_row_in_the_middle():
    rows = tiny_rows(40, 6)
    offsets = np.array([0, 25, 40], np.int32)
    full, (_, need), _ = render.crop_layout(rows, offsets, (IH, IW), 1 << 20)
    nonempty = np.flatnonzero(full["w"] > 0)
    k = int(nonempty[len(nonempty) // 2])
    a_k = (int(full["w"][k]) * int(full["h"][k]) + 3) // 4 * 4
    capacity = int(full["offset"][k]) + a_k - 1                            # row k misses the arena by one pixel
    table, used_k, flag = check(frames_of(7, 2), rows, offsets, capacity)
    assert flag == render.FLAG_CROP_ARENA and used_k == int(full["offset"][k])
    assert (table["offset"][nonempty[nonempty >= k]] == -1).all() and (table["offset"][nonempty[nonempty < k]] >= 0).all()
    assert np.array_equal(table["w"], full["w"]) and np.array_equal(table["h"], full["h"])     # a dropped row keeps its size
    # exactly enough: nothing is dropped
    assert check(frames_of(7, 2), rows, offsets, need)[1:] == (need, 0)


def test_ragged_crops_hold_no_padding():
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
    table, used, flag = check(frames, rows, offsets, 8192, sizes, geom)
    assert table.tolist()[:4] == [(0, 6, 10, 0), (60, 31, 20, 0), (680, 1, 1, 0), (0, 0, 0, 0)] and flag == 0
    assert (table["w"][4], table["h"][4], table["w"][5], table["h"][5]) == (53, 37, 3, 7)
    arena = launch(frames, rows, offsets, 8192, geom=geom)[0]
    assert (arena[:3 * used] != 255).all()


def test_a_record_above_its_slot_and_an_empty_one():
    """Image 1's record is no image.  ih = 25 in a slot of 16 rows is clamped to the slot, so its rows are cut as in a 16 x 20
    image; ih = 0 leaves it no pixel, so both its rows are empty records.  Either way FLAG_GEOMETRY, and image 0 as ever."""
    import asy_vrnet_amd.hip as hip
    cap, good = (16, 24), (11, 17)
    frames = frames_of(20, 2, *cap)
    rows = np.array([[2, 1, 9, 8, 0],                 # image 0: 7 x 7, 52 pixels of the arena
                     [10, 5, 30, 30, 1],              # hostile: 7 x 6 after the clamp to 17 x 11, 44 pixels
                     [3, 2, 8, 14, 2],                # image 1: 5 x 12
                     [0, 10, 24, 40, 3]], np.int32)   # 20 x 6 of 16 x 20
    offsets = np.array([0, 2, 4], np.int32)
    geom = data.geometry_bytes(data.frame_geometry([good, (16, 20)], (64, 64), True, cap)).cuda()
    for ih, records, used in ((25, [(96, 5, 12, 1), (156, 20, 6, 1)], 276), (0, [(0, 0, 0, 1), (0, 0, 0, 1)], 96)):
        hostile = geom.clone()
        hostile.view(torch.int32).view(2, -1)[1, 0] = ih
        arena, table, summary, flag = launch(frames, rows, offsets, 2048, geom=hostile)
        assert flag == hip.FLAG_GEOMETRY == 256 and summary == [4, used]
        assert table[:4].tolist() == [(0, 7, 7, 0), (52, 7, 6, 0)] + records
        want = expected_arena([frames[0, :11, :17], frames[1, :16, :20]], rows, table[:4], used)
        assert np.array_equal(arena[:3 * used], want) and (arena[3 * used:] == FILL).all()


def test_the_same_call_twice_gives_the_same_bytes():
    frames, rows = frames_of(10, 3), tiny_rows(300, 11)
    offsets = np.array([0, 100, 180, 300], np.int32)
    a, b = launch(frames, rows, offsets, 800), launch(frames, rows, offsets, 800)
    assert a[3] == render.FLAG_CROP_ARENA == b[3] and a[2] == b[2]
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])


def test_argument_checks():
    import asy_vrnet_amd.hip as hip
    frames, rows, offsets = cuda(frames_of(12, 2)), cuda(EDGE_ROWS), cuda(np.array([0, 0, len(EDGE_ROWS)], np.int32))
    n = len(EDGE_ROWS)
    arena = torch.zeros(3 * 64 + 3, dtype=torch.uint8, device="cuda")
    table, summary = torch.zeros((n, 4), dtype=torch.int32, device="cuda"), torch.zeros(2, dtype=torch.int32, device="cuda")
    with pytest.raises(RuntimeError, match="4-byte aligned"):
        hip.crop_boxes(frames, rows, offsets, arena[3:], table, summary)
    with pytest.raises(RuntimeError, match="3 \\* capacity"):
        hip.crop_boxes(frames, rows, offsets, arena[:64], table, summary)
    with pytest.raises(RuntimeError, match="shape \\(3,\\)"):
        hip.crop_boxes(frames, rows, offsets[:2], arena, table, summary)
    with pytest.raises(RuntimeError, match=f"shape \\({n}, 4\\)"):
        hip.crop_boxes(frames, rows, offsets, arena, table[:3], summary)
    with pytest.raises(RuntimeError, match="capacity must lie"):
        render.crop_boxes(frames, (rows, offsets), capacity=0)
    torch.cuda.synchronize()


def test_crop_boxes_takes_the_list_of_non_max_suppression():
    frames = frames_of(13, 3)
    rng = np.random.default_rng(14)
    results = []
    for n in (4, 0, 7):
        top, left = rng.uniform(-5, IH, n), rng.uniform(-5, IW, n)
        det = np.stack([top, left, top + rng.uniform(0, 25, n), left + rng.uniform(0, 25, n), np.full(n, .9), np.full(n, .9),
                        rng.integers(0, 4, n)], 1).astype(np.float32)
        results.append(det if n else None)
    crops = render.crop_boxes(frames, results)
    got = crops.images()
    assert crops.arena.numel() == 3 * 2 * 3 * IH * IW and int(crops.flag) == 0 and [len(g) for g in got] == [4, 0, 7]
    for b in range(3):
        rows = render.box_rows([results[b]], (IH, IW), 4)[0]
        want = render.crop_boxes_host(frames[b], rows)
        assert all(g.shape == w.shape and np.array_equal(g, w) for g, w in zip(got[b], want)), b
    # the device pair gives the same, and a single frame counts as B = 1; an arena that is too small gives None
    rows, offsets = render.box_rows(results, (IH, IW), 4)[:2]
    pair = render.crop_boxes(cuda(frames), (cuda(rows), cuda(offsets))).images()
    assert all(np.array_equal(x, y) for b in range(3) for x, y in zip(pair[b], got[b]))
    one = render.crop_boxes(frames[2], results[2:], capacity=8)
    assert [c is None or c.size <= 3 * 8 for c in one.images()[0]] == [True] * 7 and int(one.flag) == render.FLAG_CROP_ARENA
    assert render.crop_boxes(frames[:1], [None]).images() == [[]]


# ---- the pipeline: the sizes and the threshold of tests/test_infer.py ------------------------------------------------------
NC, S, F, CAP, NMS_THRES = 4, (64, 64), (40, 56), 64, 0.4
RAGGED_CAP, RAGGED_SIZES = (48, 68), [(40, 56), (23, 41)]


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
    return dict(first=first, second=second, kw=kw, plain=A.FramePipeline(model, F, S, **kw),
                crops=A.FramePipeline(model, F, S, crops=True, **kw))


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
    return dict(first=first, second=second, kw=kw, plain=A.FramePipeline(model, RAGGED_CAP, S, **kw),
                crops=A.FramePipeline(model, RAGGED_CAP, S, crops=True, **kw))


def host_crops(frames, detections):
    return [render.crop_boxes_host(f, render.box_rows([d], f.shape[:2], NC)[0]) for f, d in zip(frames, detections)]


def same_crops(got, want):
    assert len(got) == len(want)
    for g, w in zip(got, want):
        assert len(g) == len(w)
        assert all(x is not None and x.dtype == np.uint8 and x.shape == y.shape and np.array_equal(x, y) for x, y in zip(g, w))


@pytest.mark.parametrize("kind", ["fixed", "ragged"])
def test_pipeline_crops_are_the_host_crops(kind, request):
    setup = request.getfixturevalue(kind)
    pipe, plain = setup["crops"], setup["plain"]
    assert pipe.graph is not None and plain.crop_capacity is None
    shape = RAGGED_CAP if kind == "ragged" else F
    assert pipe.crop_capacity == 2 * 2 * shape[0] * shape[1] == pipe.result.crops.arena.numel() // 3
    res = pipe.run(*setup["first"])
    dets = res.detections()
    print(kind, "conf_thres", setup["kw"]["conf_thres"], "kept per image", [len(d) for d in dets])
    assert max(len(d) for d in dets) >= 2                                  # not vacuous: an image with two or more detections
    first = res.crops.images()
    same_crops(first, host_crops(setup["first"][0], dets))
    assert sum(c.size > 0 for g in first for c in g) >= 2 and int(res.flag) == 0
    # the rest of the result is that of the same pipeline without crops, bit for bit
    base = plain.run(*setup["first"])
    assert base.crops is None and res.crops is pipe.result.crops
    for k in ("rows", "kept", "det_counts", "rendered", "class_map", "seg_counts", "flag"):
        assert torch.equal(getattr(base, k), getattr(res, k)), k
    # a replay on other frames gives the crops of those frames
    res = pipe.run(*setup["second"])
    second = res.crops.images()
    same_crops(second, host_crops(setup["second"][0], res.detections()))
    assert int(res.flag) == 0 and sum(len(g) for g in second) > 0
    assert any(len(a) != len(b) or any(x.shape != y.shape or not np.array_equal(x, y) for x, y in zip(a, b))
               for a, b in zip(first, second))


def test_pipeline_with_an_arena_of_a_few_pixels(model, fixed):
    import asy_vrnet_amd as A
    pipe = A.FramePipeline(model, F, S, crops=24, **fixed["kw"])
    res = pipe.run(*fixed["first"])
    dets = res.detections()
    rows, offsets = render.box_rows(dets, F, NC)[:2]
    table, (N, used), flag = render.crop_layout(rows, offsets, F, 24)
    assert flag == render.FLAG_CROP_ARENA == int(res.flag) and res.crops.summary.tolist() == [N, used] and used <= 24
    got = res.crops.table.cpu().numpy().reshape(-1).view(render.CROP_RECORD)
    assert np.array_equal(got[:N], table) and (got[N:]["image"] == -1).all()
    want = host_crops(fixed["first"][0], dets)
    flat = [c for g in res.crops.images() for c in g]
    assert len(flat) == N and any(c is None for c in flat)
    for c, w, off in zip(flat, [c for g in want for c in g], table["offset"]):
        assert (c is None) if off < 0 else np.array_equal(c, w)
    with pytest.raises(RuntimeError, match="crops is None, True or the capacity"):
        A.FramePipeline(model, F, S, crops=0, **fixed["kw"])


def test_without_crops_the_chain_issues_the_calls_it_issued_before(model, fixed, monkeypatch):
    """Every wrapper of hip.py the chain calls, in order: crops=None never reaches crop_boxes, and crops=True adds exactly
    that one call, right behind detect_finish."""
    import asy_vrnet_amd as A
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
    plain = A.FramePipeline(model, F, S, graph=False, **fixed["kw"])
    crops = A.FramePipeline(model, F, S, graph=False, crops=True, **fixed["kw"])
    del calls[:]
    with torch.no_grad():
        plain._chain()
    without = [c for c in calls]
    del calls[:]
    with torch.no_grad():
        crops._chain()
    torch.cuda.synchronize()
    assert "crop_boxes" not in without and without.count("detect_finish") == 1 and "render" in without
    at = calls.index("crop_boxes")
    assert calls[at - 1] == "detect_finish" and calls[:at] + calls[at + 1:] == without
    tail = [c for c in without if c in ("detect_select", "nms_capped", "detect_finish", "seg_predict", "render")]
    assert tail == ["detect_select", "nms_capped", "detect_finish", "seg_predict", "render"]


def test_predict_dir_saves_the_crops_of_every_picture(ragged, tmp_path):
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
    out = infer.predict_dir(ragged["crops"], str(src), str(radar_root), str(dst))      # batch 2: the last call repeats picture 2
    assert [n for n, _ in out] == names
    want = {}
    for (n, det), frame in zip(out, frames):
        for i, crop in enumerate(host_crops([frame], [det])[0]):
            if crop.size:
                want[f"{n[:-4]}_crop_{i}.png"] = crop
    print("detections per picture", [len(d) for _, d in out], "crops saved", len(want))
    assert len(want) >= 2 and sorted(os.listdir(dst / "img_crop")) == sorted(want)
    for name, crop in want.items():
        assert np.array_equal(np.array(Image.open(dst / "img_crop" / name)), crop), name
    assert sorted(os.listdir(dst)) == sorted([n for n in names] + ["img_crop"])
