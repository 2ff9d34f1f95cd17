"""The captured validation pass (asy-vrnet_amd/evaluate.py) and the append kernel under it (vrnet_eval_append_f32).  Both are
specified as exact restatements of host functions of this package -- metrics.format_detections, DetectionEvaluator,
fast_hist -- so every comparison is equality: integers, and float64 values made by the same operations in the same order."""
import os

import numpy as np
import pytest
import torch

import asy_vrnet_amd as A
from asy_vrnet_amd import data, decode, evaluate, infer, metrics

NC, NSEG = 4, 9
NAMES = ["boat", "buoy", "pier", "ship"]
S, F, NMS_THRES = (64, 64), (40, 56), 0.5
MAX_BOXES, MAX_GT = 4, 4


def cuda(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def f32_neighbours(v):
    v = np.asarray(v, dtype=np.float32)
    return np.nextafter(v, np.float32(-1)), np.nextafter(v, np.float32(2))


# ---------------------------------------------------------------------------------------------- 1. score6 (no GPU)
def test_score6_equals_the_six_characters_python_reads_back():
    """score6(x) == float(str(np.float32(x))[:6]) on 200 000 uniform samples of [1e-4, 1], on every k / 1e4 (k = 1..10 000)
    with its two float32 neighbours, on 1.0 and on 1e-4.  The rule is stated for float32(1e-4) <= x: the lower neighbour of
    float32(1e-4), which numpy prints as 9.999999e-05, lies outside it (conf_thres >= 1e-4 keeps it out of a pipeline) and is
    the one value left out; the upper neighbour of 1.0 stays in."""
    rng = np.random.default_rng(90)
    grid = (np.arange(1, 10001) / 1e4).astype(np.float32)
    below, above = f32_neighbours(grid)
    x = np.concatenate([rng.uniform(1e-4, 1.0, 200000).astype(np.float32), grid, below, above,
                        np.float32([1.0, 1e-4])])
    x = x[x >= np.float32(1e-4)]
    assert len(x) == 200000 + 30000 + 2 - 1
    want = np.array([float(str(v)[:6]) for v in x], dtype=np.float64)
    got = evaluate.score6(x)
    assert got.dtype == np.float64 and got.shape == x.shape
    bad = np.flatnonzero(got != want)
    assert bad.size == 0, (x[bad][:5], got[bad][:5], want[bad][:5])
    assert evaluate.score6(np.float32(1.0)) == 1.0 and evaluate.score6(np.float32(1e-4)) == 1e-4


# ---------------------------------------------------------------------------------------------- 2. argument errors (no GPU)
def make_inputs(seed):
    rng = np.random.default_rng(seed)
    frames = rng.integers(0, 256, (2,) + F + (3,), dtype=np.uint8)
    radar = (rng.standard_normal((2, 4) + S) * 2.0 + 1.0).astype(np.float32)
    labels = rng.choice(np.array(list(range(10)) + [255], dtype=np.uint8), (2,) + F)
    return frames, radar, labels


def test_eval_pipeline_argument_errors():
    model = A.EfficientVRNet(NC, NSEG, "nano", img_size=S[0])
    with pytest.raises(RuntimeError, match="eval mode"):
        A.EvalPipeline(model, F, S, NAMES, NSEG)
    model.eval()
    with pytest.raises(RuntimeError, match="conf_thres"):
        A.EvalPipeline(model, F, S, NAMES, NSEG, conf_thres=5e-5)
    for kw in ({"max_boxes": 0}, {"max_gt": 0}, {"capacity": 0}, {"max_boxes": -3}, {"max_gt": 2.5}):
        with pytest.raises(RuntimeError, match=next(iter(kw))):
            A.EvalPipeline(model, F, S, NAMES, NSEG, **kw)
    with pytest.raises(RuntimeError, match="multiple of batch"):
        A.EvalPipeline(model, F, S, NAMES, NSEG, batch=2, capacity=5)
    with pytest.raises(RuntimeError, match="HIP device"):                      # every argument is fine: only the device is missing
        A.EvalPipeline(model, F, S, NAMES, NSEG, batch=2, capacity=6)
    assert evaluate.validate_eval_config(NAMES, NSEG, 3, None, 100, 64, 0.05)[2] == 4098

    labels = make_inputs(91)[2]
    gts = [np.array([[1, 2, 30, 20, 3]]), np.zeros((0, 5), dtype=np.int64)]
    check = lambda ids=("a", "b"), seen=(), lab=labels, gt=gts: evaluate.validate_add(list(ids), set(seen), lab, gt, 2, F, NC, MAX_GT)
    ids, lab, packed = check()
    assert ids == ["a", "b"] and lab.dtype == torch.uint8 and tuple(lab.shape) == (2,) + F
    assert packed.dtype == np.int32 and packed[-2:].tolist() == [1, 0]
    assert packed[:5].tolist() == [1, 2, 30, 20, 3] and not packed[5:-2].any()
    with pytest.raises(RuntimeError, match="added twice"):
        check(seen=("b",))
    with pytest.raises(RuntimeError, match="added twice"):
        check(ids=("a", "a"))
    with pytest.raises(RuntimeError, match="exactly batch"):
        check(ids=("a",))
    with pytest.raises(RuntimeError, match="exactly batch"):
        check(ids=("a", "b", "c"))
    with pytest.raises(RuntimeError, match="label maps of shape"):
        check(lab=labels[:, :-1])
    with pytest.raises(RuntimeError, match="label maps of shape"):
        check(lab=labels[:1])
    with pytest.raises(RuntimeError, match="uint8 label maps"):
        check(lab=labels.astype(np.int64))
    for bad in (NC, -1):
        with pytest.raises(RuntimeError, match="class outside"):
            check(gt=[np.array([[1, 2, 30, 20, bad]]), gts[1]])
    with pytest.raises(RuntimeError, match="max_gt"):
        check(gt=[np.tile(gts[0], (MAX_GT + 1, 1)), gts[1]])
    with pytest.raises(RuntimeError, match="exactly batch"):
        check(gt=gts[:1])


# ---------------------------------------------------------------------------------------------- 3. evaluate_lines (no GPU)
class StubPipeline:
    def __init__(self, batch, frame_shape):
        self.batch, self.frame_shape, self.calls, self.resets = batch, frame_shape, [], 0

    def reset(self):
        self.resets += 1

    def add(self, *args):
        self.calls.append(args)

    def compute(self):
        return "computed"


def test_evaluate_lines_ids_paths_and_batches(tmp_path):
    from PIL import Image
    rng = np.random.default_rng(92)
    radar_root, seg_root = tmp_path / "radar", tmp_path / "VOC2007"
    os.makedirs(radar_root)
    os.makedirs(seg_root / "SegmentationClass")
    os.makedirs(tmp_path / "JPEGImages")
    fids, ih, iw = ["1665000001.12345", "1665000000.54321"], 5, 7
    rgb = rng.integers(0, 256, (ih, iw, 3), dtype=np.uint8)
    grey = rng.integers(0, 256, (ih, iw), dtype=np.uint8)
    Image.fromarray(rgb).save(tmp_path / "JPEGImages" / (fids[0] + ".png"))
    Image.fromarray(grey, mode="L").save(tmp_path / "JPEGImages" / (fids[1] + ".png"))
    labels = rng.integers(0, NSEG, (2, ih, iw), dtype=np.uint8)
    radars = rng.standard_normal((2, 4, 8, 8))
    for k, fid in enumerate(fids):
        Image.fromarray(labels[k], mode="L").save(seg_root / "SegmentationClass" / (fid + ".png"))
        np.savez(radar_root / (fid + ".npz"), radars[k])
    lines = [f"{tmp_path}/JPEGImages/{fids[0]}.png 1,2,3,4,0 0,1,6,4,2\n", f"{tmp_path}/JPEGImages/{fids[1]}.png\n"]

    pipe = StubPipeline(2, (ih, iw))
    assert evaluate.evaluate_lines(pipe, lines, str(radar_root), str(seg_root)) == "computed"
    assert pipe.resets == 1 and len(pipe.calls) == 1
    ids, frames, radar, label_maps, gts = pipe.calls[0]
    assert ids == ["1665000001", "1665000000"]                                   # os.path.basename(path).split('.')[0]
    assert frames.dtype == np.uint8 and np.array_equal(frames[0], rgb)
    assert np.array_equal(frames[1], np.repeat(grey[:, :, None], 3, axis=2))     # an L frame becomes RGB
    assert radar.dtype == np.float32 and np.array_equal(radar, radars.astype(np.float32))
    assert label_maps.dtype == np.uint8 and np.array_equal(label_maps, labels)
    assert np.array_equal(gts[0], [[1, 2, 3, 4, 0], [0, 1, 6, 4, 2]]) and gts[1].shape == (0, 5)

    single = StubPipeline(1, (ih, iw))
    evaluate.evaluate_lines(single, lines, str(radar_root), str(seg_root))
    assert [c[0] for c in single.calls] == [["1665000001"], ["1665000000"]]
    assert all(c[1].shape == (1, ih, iw, 3) for c in single.calls)

    with pytest.raises(RuntimeError, match="multiple of the pipeline's batch"):
        evaluate.evaluate_lines(StubPipeline(2, (ih, iw)), lines + lines[:1], str(radar_root), str(seg_root))
    Image.fromarray(rgb[:-1]).save(tmp_path / "JPEGImages" / (fids[1] + ".png"))
    with pytest.raises(RuntimeError, match=fids[1].replace(".", r"\.") + r"\.png"):
        evaluate.evaluate_lines(StubPipeline(2, (ih, iw)), lines, str(radar_root), str(seg_root))


# ---------------------------------------------------------------------------------------------- 4. the append kernel
ARENA_FILL = -7


def filled_arena(capacity, max_boxes, max_gt):
    arena = evaluate.new_arena(capacity, max_boxes, max_gt, "cuda")
    for t in arena.values():
        t.fill_(ARENA_FILL)
    return arena


def synthetic_rows(seed):
    """(3, 8, 7) rows in descending score order, kept = [0, 3, 8]: scores exactly at k / 1e4, one ulp either side, 1.0 and
    products that round in float32; coordinates in (-1, 0), below -1, with fractions and near 1e6."""
    rng = np.random.default_rng(seed)
    rows = np.zeros((3, 8, 7), np.float32)
    g = np.float32(0.7301)
    lo, hi = f32_neighbours(g)
    # (obj, class_conf): the score is their float32 product
    pairs = {1: [(0.9, 0.97), (1.0, np.float32(0.1234)), (1.0, f32_neighbours(np.float32(0.1234))[0])],
             2: [(1.0, 1.0), (hi, 1.0), (1.0, g), (1.0, lo), (0.9, 0.7), (0.61, 0.5), (0.3, 0.4), (0.0123, 0.9)]}
    for b, pl in pairs.items():
        rows[b, :len(pl), 4:6] = np.float32(pl)
    rows[..., 0:4] = rng.uniform(0.0, 900.0, (3, 8, 4))
    rows[1, 0, 0:4] = [-0.5, -0.999, 12.75, 999999.9]
    rows[1, 1, 0:4] = [-1.5, -3.99, 1e6 - 0.0625, 1e6 + 0.9375]
    rows[2, 0, 0:4] = [-0.25, 17.5, 39.99, -2.0]
    rows[2, 4, 0:4] = [0.0, -0.0, 999998.5, 55.999]
    rows[..., 6] = rng.integers(0, NC, (3, 8))
    if seed % 2:                                      # the second launch: other numbers at the same special places
        rows[..., 6] = (rows[..., 6] + 1) % NC
    return rows, [0, 3, 8]


def synthetic_gt(max_gt, counts, seed):
    rng = np.random.default_rng(seed)
    gt = rng.integers(-5, 2000, (len(counts), max_gt, 5)).astype(np.int32)
    return gt, np.array(counts, dtype=np.int32)


def append(rows, kept, gt, gt_count, cursor, arena, flag):
    import asy_vrnet_amd.hip as hip
    hip.eval_append(cuda(rows), torch.tensor(kept, dtype=torch.int32, device="cuda"), cuda(gt), cuda(gt_count), cursor, arena, flag)


def host(arena):
    return {k: v.cpu().numpy() for k, v in arena.items()}


def assert_slots(got, first, rows, kept, gt, gt_count, max_boxes, max_gt):
    """Slots first .. first + B - 1 hold format_detections of every image bit for bit, and nothing beyond the counts."""
    for b in range(len(kept)):
        s = first + b
        label, score, box = metrics.format_detections(rows[b, :kept[b]], max_boxes)
        n = len(label)
        assert n == min(kept[b], max_boxes) and got["det_count"][s] == n
        assert np.array_equal(got["det_label"][s, :n], label)
        assert np.array_equal(got["det_score"][s, :n].view(np.int64), score.view(np.int64)), (b, got["det_score"][s, :n], score)
        assert np.array_equal(got["det_box"][s, :n].view(np.int64), box.view(np.int64)), (b, got["det_box"][s, :n], box)
        assert (got["det_label"][s, n:] == ARENA_FILL).all() and (got["det_score"][s, n:] == ARENA_FILL).all()
        assert (got["det_box"][s, n:] == ARENA_FILL).all()
        g = min(int(gt_count[b]), max_gt)
        assert got["gt_n"][s] == g
        assert np.array_equal(got["gt_label"][s, :g], gt[b, :g, 4])
        assert np.array_equal(got["gt_box"][s, :g], gt[b, :g, :4].astype(np.float64))
        assert (got["gt_label"][s, g:] == ARENA_FILL).all() and (got["gt_box"][s, g:] == ARENA_FILL).all()


@pytest.mark.gpu
def test_append_equals_format_detections():
    max_boxes, max_gt = 5, 3
    rows, kept = synthetic_rows(94)
    for b in range(3):
        score = rows[b, :kept[b], 4] * rows[b, :kept[b], 5]
        assert (np.diff(score) < 0).all(), b                                   # descending and pairwise distinct
    assert (rows[..., :4] < -1).any() and ((rows[..., :4] > -1) & (rows[..., :4] < 0)).any() and (rows[..., :4] > 999990).any()
    gt, gt_count = synthetic_gt(max_gt, [0, 2, max_gt], 95)
    arena = filled_arena(6, max_boxes, max_gt)
    cursor, flag = torch.zeros(1, dtype=torch.int32, device="cuda"), torch.zeros(1, dtype=torch.int32, device="cuda")
    append(rows, kept, gt, gt_count, cursor, arena, flag)
    first = host(arena)
    assert int(cursor) == 3 and int(flag) == 0
    assert_slots(first, 0, rows, kept, gt, gt_count, max_boxes, max_gt)
    assert all((v[3:] == ARENA_FILL).all() for v in first.values())           # the slots behind the cursor are untouched
    # the quantised scores are the six characters, not the float32 values
    assert first["det_score"][2, :4].tolist() == [1.0, 0.7301, 0.7301, 0.73]
    assert first["det_box"][1, 0].tolist() == [0.0, 0.0, 999999.0, 12.0] and first["det_box"][1, 1, :2].tolist() == [-3.0, -1.0]
    # a second launch lands in slots 3 .. 5 and leaves 0 .. 2 alone
    rows2, kept2 = synthetic_rows(95)
    kept2 = kept2[::-1]
    rows2 = rows2[::-1].copy()
    gt2, gt_count2 = synthetic_gt(max_gt, [max_gt, 1, 0], 96)
    append(rows2, kept2, gt2, gt_count2, cursor, arena, flag)
    second = host(arena)
    assert int(cursor) == 6 and int(flag) == 0
    assert all(np.array_equal(second[k][:3], first[k][:3]) for k in first)
    assert_slots(second, 3, rows2, kept2, gt2, gt_count2, max_boxes, max_gt)


@pytest.mark.gpu
def test_append_flags():
    max_boxes, max_gt = 5, 3
    rows, kept = synthetic_rows(94)
    gt, gt_count = synthetic_gt(max_gt, [0, 2, max_gt], 95)
    zeros = lambda: torch.zeros(1, dtype=torch.int32, device="cuda")
    # capacity 4: the second launch of 3 finds no room, writes nothing and leaves the cursor
    arena, cursor, flag = filled_arena(4, max_boxes, max_gt), zeros(), zeros()
    append(rows, kept, gt, gt_count, cursor, arena, flag)
    before = host(arena)
    assert int(cursor) == 3 and int(flag) == 0
    append(rows, kept, gt, gt_count, cursor, arena, flag)
    assert int(cursor) == 3 and int(flag) == evaluate.FLAG_EVAL_CAPACITY
    after = host(arena)
    assert all(np.array_equal(after[k], before[k]) for k in before)
    # more ground truths than max_gt: the first max_gt are kept
    arena, cursor, flag = filled_arena(3, max_boxes, max_gt), zeros(), zeros()
    append(rows, kept, gt, np.array([0, 2, max_gt + 2], dtype=np.int32), cursor, arena, flag)
    assert int(flag) == evaluate.FLAG_EVAL_GT and int(cursor) == 3
    assert_slots(host(arena), 0, rows, kept, gt, [0, 2, max_gt], max_boxes, max_gt)
    # a NaN coordinate is written as 0; so are an infinite one and one outside int32
    bad = rows.copy()
    bad[1, 1, 2], bad[2, 0, 0], bad[2, 1, 3] = np.nan, np.inf, 3e9
    arena, cursor, flag = filled_arena(3, max_boxes, max_gt), zeros(), zeros()
    append(bad, kept, gt, gt_count, cursor, arena, flag)
    got = host(arena)
    assert int(flag) == evaluate.FLAG_EVAL_BOX
    assert got["det_box"][1, 1, 3] == 0.0 and got["det_box"][2, 0, 1] == 0.0 and got["det_box"][2, 1, 2] == 0.0      # box = l, t, r, b
    mended = np.nan_to_num(bad, nan=0.0, posinf=0.0)
    mended[2, 1, 3] = 0.0
    assert_slots(got, 0, mended, kept, gt, gt_count, max_boxes, max_gt)


@pytest.mark.gpu
def test_format_detections_device():
    rows, kept = synthetic_rows(94)
    label, score, box, count = evaluate.format_detections_device(cuda(rows), torch.tensor(kept, dtype=torch.int32), 5)
    assert (label.dtype, score.dtype, box.dtype, count.dtype) == (torch.int32, torch.float64, torch.float64, torch.int32)
    for b in range(3):
        want = metrics.format_detections(rows[b, :kept[b]], 5)
        n = int(count[b])
        assert n == len(want[0]) and np.array_equal(label[b, :n].cpu().numpy(), want[0])
        assert np.array_equal(score[b, :n].cpu().numpy(), want[1]) and np.array_equal(box[b, :n].cpu().numpy(), want[2])
        assert not label[b, n:].any() and not score[b, n:].any() and not box[b, n:].any()


# ---------------------------------------------------------------------------------------------- 5-7. the pipeline
IDS = [["img_e", "img_b"], ["img_f", "img_a"], ["img_d", "img_c"]]              # not in sorted order across the batches


def eager(model, frames, radar, conf):
    """The eager composition of the public calls for one batch: (list of (N_b, 7) rows, class map (2, ih, iw), pred)."""
    images, _ = data.device_letterbox(cuda(frames), S)
    with torch.no_grad():
        det, seg = model(images, cuda(radar))
    pred = decode.decode_outputs(det, S)
    results = decode.non_max_suppression(pred, NC, S, F, True, conf_thres=conf, nms_thres=NMS_THRES)
    return [np.zeros((0, 7), np.float32) if r is None else np.asarray(r, dtype=np.float32) for r in results], \
        decode.seg_predict(seg, S, F), pred


def seg_numbers(hist):
    """IoU, recall, precision per class, accuracy and mIoU of a confusion matrix (rows = labels), denominators at least 1."""
    h = np.asarray(hist)
    diag = np.diag(h)
    iou = diag / np.maximum(h.sum(1) + h.sum(0) - diag, 1)
    return dict(iou=iou, pa_recall=diag / np.maximum(h.sum(1), 1), precision=diag / np.maximum(h.sum(0), 1),
                accuracy=np.sum(diag) / np.maximum(np.sum(h), 1), miou=np.nanmean(iou))


DET_KEYS = ("map", "ap", "f1", "recall", "precision", "lamr", "n_gt", "n_det", "n_tp")


def expectation(images):
    """DetectionEvaluator + fast_hist over `images` (the per-image records of the fixture), image by image."""
    ev = metrics.DetectionEvaluator(NAMES, max_boxes=MAX_BOXES)
    hist = torch.zeros((NSEG, NSEG), dtype=torch.int64, device="cuda")
    for im in images:
        ev.add(im["id"], im["rows"], im["gt"])
        metrics.fast_hist(cuda(im["label"]), im["class_map"], NSEG, out=hist)
    det = ev.compute()
    want = {"det." + k: det[k].cpu().numpy() for k in DET_KEYS}
    want["hist"] = hist.cpu().numpy()
    want.update(seg_numbers(want["hist"]))
    return want


def snapshot(res):
    got = {"det." + k: res.det[k].cpu().numpy() for k in DET_KEYS}
    got.update(hist=res.hist, iou=res.iou, pa_recall=res.pa_recall, precision=res.precision, accuracy=res.accuracy,
               miou=res.miou)
    return got


def assert_same(got, want):
    assert set(got) == set(want)
    for k in want:
        g, w = np.asarray(got[k]), np.asarray(want[k])
        assert g.dtype == w.dtype and g.shape == w.shape, (k, g.dtype, w.dtype, g.shape, w.shape)
        assert np.array_equal(g, w, equal_nan=g.dtype.kind == "f"), (k, g, w)


def add_args(setup, k, device=False):
    frames, radar, labels = setup["batches"][k]
    if device:
        frames, radar, labels = cuda(frames), cuda(radar), cuda(labels)
    return IDS[k], frames, radar, labels, [im["gt"] for im in setup["images"][2 * k:2 * k + 2]]


def add_batch(pipe, setup, k):
    return pipe.add(*add_args(setup, k))


@pytest.fixture(scope="module")
def setup():
    model = A.EfficientVRNet(NC, NSEG, "nano", img_size=S[0]).cuda().eval()
    A.randomize_state_dict(model.state_dict(), seed=4)
    batches = [make_inputs(seed) for seed in (97, 98, 99)]
    pred = eager(model, batches[0][0], batches[0][1], 0.5)[2]
    score = (pred[..., 4] * pred[..., 5:5 + NC].amax(-1)).flatten().sort(descending=True).values
    conf = float(score[39])                                   # the 40th-largest score of the first batch
    assert conf >= evaluate.MIN_CONF
    rng = np.random.default_rng(100)
    images, candidates = [], []
    for k, (frames, radar, labels) in enumerate(batches):
        rows, class_map, pred = eager(model, frames, radar, conf)
        candidates += ((pred[..., 4] * pred[..., 5:5 + NC].amax(-1)) >= conf).sum(1).tolist()
        for b in range(2):
            s = rows[b][:, 4] * rows[b][:, 5]
            assert len(np.unique(s)) == len(s), "equal scores in one image: the tie rule, not the code, would decide"
            label, _, box = metrics.format_detections(rows[b], MAX_BOXES)
            own = np.concatenate([box[:2], label[:2, None]], axis=1).astype(np.int64).reshape(-1, 5)
            x1, y1 = rng.integers(0, F[1] - 8, 2), rng.integers(0, F[0] - 8, 2)
            rand = np.stack([x1, y1, x1 + rng.integers(4, 8, 2), y1 + rng.integers(4, 8, 2), rng.integers(0, NC, 2)], axis=1)
            images.append(dict(id=IDS[k][b], rows=rows[b], gt=np.concatenate([own, rand]), label=labels[b],
                               class_map=class_map[b].clone()))
    print("conf_thres", conf, "candidates per image", candidates, "kept per image", [len(im["rows"]) for im in images])
    assert max(len(im["rows"]) for im in images) > MAX_BOXES                    # the max_boxes cut engages
    buffers = [b.detach().clone() for b in model.buffers()]
    pipes = {g: A.EvalPipeline(model, F, S, NAMES, NSEG, batch=2, capacity=6, max_boxes=MAX_BOXES, max_gt=MAX_GT,
                               conf_thres=conf, nms_thres=NMS_THRES, graph=g) for g in (False, True)}
    fresh = {g: (int(p.cursor), int(p.hist.abs().sum()), int(p.eval_flag), int(p.arena["det_count"].abs().sum()))
             for g, p in pipes.items()}
    untouched = all(torch.equal(a, b) for a, b in zip(buffers, model.buffers()))
    return dict(model=model, conf=conf, batches=batches, images=images, pipes=pipes, fresh=fresh, untouched=untouched,
                candidates=candidates, want=expectation(images))


@pytest.mark.gpu
@pytest.mark.parametrize("graph", [False, True])
def test_pipeline_equals_the_composition(setup, graph):
    want = setup["want"]
    print("map", want["det.map"], "n_tp", want["det.n_tp"], "n_det", want["det.n_det"], "miou", want["miou"])
    assert 0.0 < float(want["det.map"]) < 1.0 and want["det.n_tp"].sum() > 0 and want["hist"].sum() > 0      # not vacuous
    pipe = setup["pipes"][graph]
    assert (pipe.graph is not None) == graph
    pipe.reset()
    for k in range(3):
        add_batch(pipe, setup, k)
    res = pipe.compute()
    assert res.flag == 0 and res.images == 6 and pipe.image_ids == sum(IDS, [])
    assert_same(snapshot(res), want)


@pytest.mark.gpu
@pytest.mark.parametrize("graph", [False, True])
def test_add_does_not_synchronise(setup, graph):
    pipe = setup["pipes"][graph]
    pipe.reset()
    first, second = add_args(setup, 0, device=True), add_args(setup, 1, device=True)
    pipe.add(*first)
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        pipe.add(*second)              # frames, radar and label maps on the device; the ground truths come from the host
    finally:
        torch.cuda.set_sync_debug_mode("default")
    assert_same(snapshot(pipe.compute()), expectation(setup["images"][:4]))


@pytest.mark.gpu
def test_pipeline_state(setup):
    assert setup["untouched"]                                                    # the warm-up left the model's buffers alone
    assert setup["fresh"] == {False: (0, 0, 0, 0), True: (0, 0, 0, 0)}           # and cursor, hist, flag, counts at zero
    pipe = setup["pipes"][True]
    pipe.reset()
    empty = pipe.compute()                                                       # nothing added: no error
    assert float(empty.det.map) == 0.0 and not empty.hist.any() and empty.hist.shape == (NSEG, NSEG) and empty.images == 0
    assert empty.miou == 0.0 and empty.flag == 0
    for k in range(3):
        add_batch(pipe, setup, k)
    first, again = snapshot(pipe.compute()), snapshot(pipe.compute())
    assert_same(again, first)
    with pytest.raises(RuntimeError, match="added twice"):
        add_batch(pipe, setup, 1)
    pipe.reset()
    assert int(pipe.cursor) == 0 and pipe.image_ids == [] and not pipe.hist.any()
    for k in range(3):
        add_batch(pipe, setup, k)
    assert_same(snapshot(pipe.compute()), first)
    assert_same(first, setup["want"])
    with pytest.raises(RuntimeError, match="full"):                              # capacity 6 is used up
        pipe.add(["x", "y"], *setup["batches"][0], [np.zeros((0, 5), np.int64)] * 2)


@pytest.mark.gpu
def test_strict_raises_on_a_capped_candidate_set(setup):
    cap = 8
    assert max(setup["candidates"][:2]) > cap
    pipe = A.EvalPipeline(setup["model"], F, S, NAMES, NSEG, batch=2, capacity=2, max_boxes=MAX_BOXES, max_gt=MAX_GT,
                          conf_thres=setup["conf"], nms_thres=NMS_THRES, max_candidates=cap, graph=True)
    add_batch(pipe, setup, 0)
    with pytest.raises(RuntimeError, match="FLAG_CANDIDATES"):
        pipe.compute()
    res = pipe.compute(strict=False)
    assert res.flag == infer.FLAG_CANDIDATES and res.images == 2 and int(res.det.n_det.sum()) > 0
