"""Training from raw frames on the GPU: the two target kernels of csrc/traintargets.hip against Pillow and the host
functions of data.py, `data.device_train_batch_ragged`, and `graph.TrainStep(from_frames=True)` against
`TrainStep(from_bytes=True)` fed with the host-side letterbox of the same frames.  Both sides of every comparison are
integers or the same fp64 arithmetic rounded once, so every comparison is bit for bit (torch.equal / np.array_equal).
Kernel shapes: input 64 x 64, ns = 3, five frames of mixed sizes in slots of 96 x 112 -- plus one input of 40 x 63 with
ns = 4, where W (ns + 1) is no multiple of 4 and the one-hot rows take the 4-byte store path, and H no multiple of the 16
rows of a workgroup.  Steps: nano, 64 x 64, B = 2."""
import os

import numpy as np
import pytest
import torch
from PIL import Image

pytestmark = pytest.mark.gpu

CAP = (96, 112)
SIZES = [(48, 80), (90, 60), (64, 64), (37, 111), (96, 112)]      # wider, taller, both passes skipped, odd, the capacity
MAX_GT = 8
# x1, y1, x2, y2, cls in pixels of the original image.  Image 0 (48 x 80 -> window 64 x 38 at (0, 13): x * 0.8, y * 38 / 48 +
# 13) carries exactly MAX_GT rows, one per case; image 2 has none.
BOXES = [
    np.array([[3, 5, 41, 33, 0],            # 2.4, 16.96, 32.8, 39.1: truncation
              [10, 0, 12, 40, 1],           # 8 .. 9: exactly 1 px wide, dropped BETWEEN two kept rows
              [10, 0, 13, 40, 2],           # 8 .. 10: exactly 2 px wide, kept
              [50, 20, 200, 100, 3],        # past the right and the bottom edge: clipped to W, H
              [0, 10, 79, 11, 1],           # 20 .. 21: exactly 1 px high, dropped
              [0, 10, 79, 12, 2],           # 20 .. 22: exactly 2 px high, kept
              [-20, -30, 30, 30, 0],        # negative: -10.75 truncates toward zero, then clips to 0
              [70, 40, 75, 47, 3]]),
    np.array([[4, 8, 50, 70, 0], [20, 20, 22, 60, 1], [10, 40, 55, 88, 2]]),
    np.zeros((0, 5), np.int64),
    np.array([[0, 0, 111, 37, 1], [7, 3, 100, 30, 0]]),
    np.array([[0, 0, 112, 96, 3], [111, 95, 112, 96, 2], [13, 17, 59, 61, 1]]),
]


@pytest.fixture(scope="module")
def A():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    import asy_vrnet_amd
    return asy_vrnet_amd


def cuda(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def geom_tensor(table):
    return cuda(table.view(np.uint8).reshape(len(table), -1))


def padded(items, capacity, fill):
    buf = np.full((len(items),) + tuple(capacity) + items[0].shape[2:], fill, np.uint8)
    for b, a in enumerate(items):
        buf[b, :a.shape[0], :a.shape[1]] = a
    return buf


def raw_batch(seed, sizes=SIZES, top=6):
    rng = np.random.default_rng(seed)
    frames = [rng.integers(0, 256, (ih, iw, 3), dtype=np.uint8) for ih, iw in sizes]
    labels = [rng.integers(0, top, (ih, iw), dtype=np.uint8) for ih, iw in sizes]          # above ns: the clamp fires
    return frames, labels


def pillow_label_canvas(label, input_shape):
    """The label half of data.letterbox_sample (dataloader.py:144-146)."""
    from asy_vrnet_amd import data
    H, W = input_shape
    nw, nh, dx, dy = data.letterbox_geometry(label.shape[1], label.shape[0], W, H)
    canvas = Image.new("L", [W, H], 0)
    canvas.paste(Image.fromarray(label).resize((nw, nh), Image.NEAREST), (dx, dy))
    return np.array(canvas)


def host_targets(boxes, size, input_shape):
    from asy_vrnet_amd import data
    (ih, iw), (H, W) = size, input_shape
    return data.boxes_xyxy_to_cxcywh(data.adjust_boxes(boxes, iw, ih, W, H)).astype(np.float32)


# ---- 1. the segmentation targets --------------------------------------------------------------------------------------
@pytest.mark.parametrize("input_shape,ns", [((64, 64), 3), ((40, 63), 4)])
def test_seg_targets_ragged_equals_pillow_nearest_and_seg_targets(A, input_shape, ns):
    from asy_vrnet_amd import data, hip
    H, W = input_shape
    _, labels = raw_batch(1)
    B = len(labels)
    taps = data.default_max_taps(CAP, input_shape)
    geom = geom_tensor(data.frame_geometry(SIZES, input_shape, True, CAP, taps))
    slots = cuda(padded(labels, CAP, 255))                      # the slot padding must not appear in a result
    png = torch.full((B, H, W), -77, dtype=torch.int64, device="cuda")          # guards: every element is written
    onehot = torch.full((B, H, W, ns + 1), 7.5, dtype=torch.float32, device="cuda")
    flag = torch.zeros(1, dtype=torch.int32, device="cuda")
    hip.seg_targets_ragged(slots, geom, H, W, ns, png_out=png, onehot=onehot, flag=flag)
    assert int(flag) == 0
    clamped = 0
    for b, lab in enumerate(labels):
        want_png, want_onehot = data.seg_targets(pillow_label_canvas(lab, input_shape), ns)
        clamped += int((want_png == ns).sum())
        assert np.array_equal(png[b].cpu().numpy(), want_png.astype(np.int64)), b
        assert np.array_equal(onehot[b].cpu().numpy(), want_onehot.astype(np.float32)), b
    assert clamped > 0 and int(png.max()) == ns and int(png.min()) == 0


# ---- 2. the box targets -----------------------------------------------------------------------------------------------
def run_box_targets(boxes, sizes, input_shape, capacity, max_gt, counts=None):
    from asy_vrnet_amd import data, hip
    H, W = input_shape
    B = len(sizes)
    geom = geom_tensor(data.frame_geometry(sizes, input_shape, True, capacity, None))
    packed, cnt = data.pack_boxes(boxes, max_gt)
    if counts is not None:
        cnt = torch.tensor(counts, dtype=torch.int32)
    targets = torch.full((B, max_gt, 5), -7.0, dtype=torch.float32, device="cuda")          # guard
    counts_out = torch.full((B,), -1, dtype=torch.int32, device="cuda")
    flag = torch.zeros(1, dtype=torch.int32, device="cuda")
    hip.box_targets_ragged(packed.cuda(), cnt.cuda(), geom, capacity, H, W, targets=targets, counts_out=counts_out, flag=flag)
    return targets.cpu().numpy(), counts_out.cpu().numpy(), int(flag)


def test_box_targets_ragged_equals_adjust_boxes_and_cxcywh(A):
    S = (64, 64)
    got, counts, flag = run_box_targets(BOXES, SIZES, S, CAP, MAX_GT)
    assert flag == 0 and len(BOXES[0]) == MAX_GT and len(BOXES[2]) == 0
    for b, (boxes, size) in enumerate(zip(BOXES, SIZES)):
        want = host_targets(boxes, size, S)
        assert counts[b] == len(want), (b, counts[b], len(want))
        assert np.array_equal(got[b, :len(want)], want), (b, got[b], want)              # kept rows in input order
        assert np.array_equal(got[b, len(want):], np.zeros((MAX_GT - len(want), 5), np.float32)), b       # the guard is gone
    # the table does cover its cases: the reference itself truncates, clips, drops at 1 px and keeps at 2 px
    want0 = host_targets(BOXES[0], SIZES[0], S)
    assert want0[:, 4].tolist() == [0, 2, 3, 2, 0, 3]                                 # rows 1 and 4 dropped, order kept
    assert want0[0].tolist() == [17.0, 27.5, 30.0, 23.0, 0.0]                         # 2.4 -> 2, 16.96 -> 16, 32.8 -> 32, 39.1 -> 39
    assert want0[1, 2] == 2.0 and want0[3, 3] == 2.0                                  # the `> 1` boundary from above
    assert want0[2].tolist() == [52.0, 46.0, 24.0, 36.0, 3.0]                         # x2 -> W = 64, y2 -> H = 64
    assert counts[2] == 0 and counts[0] == 6


def test_box_targets_ragged_equals_the_reference_dataset_rows(A):
    """tests/golden/dataset_small.npz is the reference's own YoloDataset output; it carries the annotation lines and the
    frames, so the original boxes and sizes are there.  The reference shuffles the rows in place, so the comparison is up
    to row order, as in tests/test_data.py."""
    from asy_vrnet_amd import data
    z = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "dataset_small.npz"))
    S = tuple(int(v) for v in z["input_shape"])
    tails = [str(t) for t in z["line_tails"]]
    boxes = [data.parse_annotation_line("x " + t)[1] for t in tails]
    sizes = [z[f"img{i}"].shape[:2] for i in range(len(tails))]
    cap = (max(s[0] for s in sizes), max(s[1] for s in sizes))
    max_gt = max(max(len(b) for b in boxes), 1)
    got, counts, flag = run_box_targets(boxes, sizes, S, cap, max_gt)
    order = lambda a: a[np.lexsort(a.T[::-1])]
    assert flag == 0 and sum(len(b) for b in boxes) > 0
    for i in range(len(tails)):
        want = z[f"boxes_out{i}"].reshape(-1, 5).astype(np.float32)
        assert counts[i] == len(want), i
        assert np.array_equal(order(got[i, :counts[i]]), order(want)), (i, got[i], want)


def test_box_targets_ragged_clamps_a_count_above_max_gt(A):
    """The device-side backstop behind `pack_boxes`: a count of max_gt + 3 is clamped (every index stays inside the
    buffers), reported in the flag word, and at most max_gt rows are written."""
    from asy_vrnet_amd import hip
    S = (64, 64)
    counts = [MAX_GT + 3, 3, -2, 2, 3]
    got, counts_out, flag = run_box_targets(BOXES, SIZES, S, CAP, MAX_GT, counts=counts)
    assert flag == hip.FLAG_BOX_COUNT == 512
    want0 = host_targets(BOXES[0], SIZES[0], S)
    assert counts_out[0] == len(want0) <= MAX_GT and np.array_equal(got[0, :len(want0)], want0)
    assert counts_out[2] == 0 and not got[2].any()
    assert counts_out.tolist() == [len(host_targets(b, s, S)) for b, s in zip(BOXES, SIZES)]


# ---- 3. the stand-alone batch ------------------------------------------------------------------------------------------
def test_device_train_batch_ragged_equals_its_parts(A):
    from asy_vrnet_amd import data
    S, ns = (64, 64), 3
    frames, labels = raw_batch(2)
    flag = torch.zeros(1, dtype=torch.int32, device="cuda")
    images, png, onehot, targets, counts = data.device_train_batch_ragged(
        padded(frames, CAP, 255), SIZES, S, padded(labels, CAP, 255), BOXES, ns, max_gt=MAX_GT, flag=flag)
    want_images, _ = data.device_letterbox_ragged(frames, None, S, normalise=True, capacity=CAP)
    assert torch.equal(images, want_images)                                  # the same kernel on the same bytes
    assert images.dtype == torch.float32 and png.dtype == torch.int64 and tuple(onehot.shape) == (len(SIZES), 64, 64, ns + 1)
    assert tuple(targets.shape) == (len(SIZES), MAX_GT, 5) and counts.dtype == torch.int32 and int(flag) == 0
    for b, lab in enumerate(labels):
        want_png, want_onehot = data.seg_targets(pillow_label_canvas(lab, S), ns)
        assert np.array_equal(png[b].cpu().numpy(), want_png.astype(np.int64))
        assert np.array_equal(onehot[b].cpu().numpy(), want_onehot.astype(np.float32))
        want = host_targets(BOXES[b], SIZES[b], S)
        assert int(counts[b]) == len(want) and np.array_equal(targets[b, :len(want)].cpu().numpy(), want)


# ---- 4. - 6. the captured step ------------------------------------------------------------------------------------------
B, S, NC, NS = 2, 64, 4, 9
STEP_CAP = (96, 208)              # wide enough for the 2 x 200 and 5 x 200 slivers to pass the capacity check
STEP_SIZES = [(48, 80), (90, 60)]
STEP_BOXES = [np.array([[5, 4, 60, 40, 1], [30, 10, 75, 45, 3]]),
              np.array([[4, 8, 50, 70, 0], [20, 20, 22, 60, 1], [10, 40, 55, 88, 2]])]      # the middle row is dropped


def trainer(A, seed=5):
    from asy_vrnet_amd import losses, optim
    m = A.EfficientVRNet(NC, NS, "nano", img_size=(S, S)).cuda().train()
    A.randomize_state_dict(m.state_dict(), seed=seed)
    return m, losses.YOLOLoss(NC).cuda(), optim.build_optimizer(m, "sgd", 1e-2, 0.937, 5e-4), optim.ModelEMA(m)


def tensors_equal(a, b):
    return a.keys() == b.keys() and all(torch.equal(a[k], b[k]) if torch.is_tensor(a[k]) else a[k] == b[k] for k in a)


def trainers_equal(t1, t2, what):
    (m1, _, o1, e1), (m2, _, o2, e2) = t1, t2
    for (k, p), (_, q) in zip(m1.named_parameters(), m2.named_parameters()):
        assert torch.equal(p, q), (what, k)
    for (k, p), (_, q) in zip(m1.named_buffers(), m2.named_buffers()):
        assert torch.equal(p, q), (what, k)
    s1, s2 = o1.state_dict()["state"], o2.state_dict()["state"]
    assert s1.keys() == s2.keys() and len(s1) > 100, what
    assert all(tensors_equal(s1[i], s2[i]) for i in s1), what
    assert e1.updates == e2.updates and tensors_equal(e1.ema.state_dict(), e2.ema.state_dict()), what


@pytest.fixture(scope="module")
def steps(A):
    """Identical trainers (one seed) under a TrainStep each: letterboxed bytes, raw frames, and a second raw-frames step
    that stays fresh until the leak test."""
    from asy_vrnet_amd.graph import TrainStep
    out = []
    for kw in (dict(from_bytes=True), dict(from_frames=True, capacity=STEP_CAP), dict(from_frames=True, capacity=STEP_CAP)):
        t = trainer(A)
        out.append((t, TrainStep(t[0], t[1], t[2], t[3], B, S, NS, max_gt=MAX_GT, **kw)))
    return out


def host_batch(frames, labels, boxes):
    """What a host loader hands `TrainStep(from_bytes=True)`: data.letterbox_sample and boxes_xyxy_to_cxcywh per image."""
    from asy_vrnet_amd import data
    imgs, labs, targets = [], [], []
    for f, l, bx in zip(frames, labels, boxes):
        image, box, label = data.letterbox_sample(Image.fromarray(f), Image.fromarray(l), bx, (S, S))
        imgs.append(np.array(image))
        labs.append(np.array(label))
        targets.append(torch.from_numpy(data.boxes_xyxy_to_cxcywh(box).astype(np.float32)))
    return np.stack(imgs), np.stack(labs), targets


def both(A, steps, seed, sizes, boxes, it):
    """One step of the from_bytes and the from_frames twin on the same raw batch; they must stay equal."""
    (tb, step_b), (tf, step_f) = steps[:2]
    frames, labels = raw_batch(seed, sizes, top=NS + 3)
    _, r = A.synthetic_inputs(B, S, seed, "cuda")
    img, lab, targets = host_batch(frames, labels, boxes)
    rb = step_b(img, r, targets, lab)
    rf = step_f(frames, r, boxes, labels)
    assert rb.keys() == rf.keys() == {"total", "loss_det", "loss_seg"}
    assert all(torch.isfinite(rb[k]) and torch.equal(rb[k], rf[k]) for k in rb), (it, rb, rf)
    # the prologue wrote the buffers the forward pass and the losses read
    assert torch.equal(step_f.x, step_b.x) and torch.equal(step_f.png, step_b.png) and torch.equal(step_f.onehot, step_b.onehot)
    assert torch.equal(step_f.labels, step_b.labels) and torch.equal(step_f.counts, step_b.counts)
    trainers_equal(tb, tf, f"step {it}")
    assert step_f.stats()["flag"] == 0
    return frames, r, labels


def test_from_frames_equals_from_bytes_on_the_host_letterbox(A, steps):
    p0 = steps[1][0][0].head.stems[0].conv.weight.detach().clone()
    for it in range(2):
        both(A, steps, 20 + it, STEP_SIZES, STEP_BOXES, it)
    st = steps[1][1].stats()
    assert st["steps"] == 2 and set(st) == {"steps", "total", "loss_det", "loss_seg", "flag"}
    assert set(steps[0][1].stats()) == {"steps", "total", "loss_det", "loss_seg"}            # the other modes: unchanged
    assert int(steps[1][1].counts.sum()) == 4 and not torch.equal(steps[1][0][0].head.stems[0].conv.weight, p0)


def test_a_second_call_with_other_sizes_leaves_no_trace_of_the_first(A, steps):
    """The size pairs swap between the slots -- slot 0 gets a taller, slot 1 a frame that is smaller than its predecessor in
    both directions -- with other boxes and fewer of them in slot 1.  The used step's prologue must write what a FRESH step
    writes for that batch (the model states differ by now, the inputs of the forward pass and the losses may not), and the
    step must still equal its from_bytes twin, which has no table, counts or slots to leak from."""
    both(A, steps, 30, STEP_SIZES, STEP_BOXES, 0)
    sizes = [(90, 60), (40, 50)]
    boxes = [np.array([[4, 8, 50, 70, 0], [10, 40, 55, 88, 2], [1, 1, 30, 30, 3]]), np.array([[3, 3, 44, 33, 2]])]
    frames, r, labels = both(A, steps, 31, sizes, boxes, 1)
    used, fresh = steps[1][1], steps[2][1]
    fresh(frames, r, boxes, labels)
    for name in ("x", "r", "png", "onehot", "labels", "counts"):
        assert torch.equal(getattr(used, name), getattr(fresh, name)), name
    assert fresh.stats()["flag"] == 0 and used.counts.tolist() == [3, 1]


def test_host_validation_raises_before_any_launch(A, steps):
    from asy_vrnet_amd.graph import TrainStep
    (tb, step_b), (tf, step_f) = steps[:2]
    frames, labels = raw_batch(40, STEP_SIZES, top=NS + 3)
    _, r = A.synthetic_inputs(B, S, 40, "cuda")

    def snapshot(t):
        m, _, opt, ema = t
        return ([p.detach().clone() for p in m.parameters()] + [b.clone() for b in m.buffers()] +
                [v.clone() for st in opt.state_dict()["state"].values() for v in st.values() if torch.is_tensor(v)] +
                [v.clone() for v in ema.ema.state_dict().values()], ema.updates)
    before, steps_before = snapshot(tf), step_f.stats()["steps"]
    inputs = [t.clone() for t in (step_f.x, step_f.png, step_f.labels, step_f.counts, step_f.geom, step_f.boxes)]

    def sliver(ih, iw):
        return [np.zeros((ih, iw, 3), np.uint8), frames[1]], [np.zeros((ih, iw), np.uint8), labels[1]]
    with pytest.raises(RuntimeError, match="image 0.*capacity"):
        step_f(sliver(97, 50)[0], r, STEP_BOXES, sliver(97, 50)[1])                     # a frame above the capacity
    with pytest.raises(RuntimeError, match="image 0.*empty window"):
        step_f(sliver(2, 200)[0], r, STEP_BOXES, sliver(2, 200)[1])
    with pytest.raises(RuntimeError, match="image 0.*taps"):
        step_f(sliver(5, 200)[0], r, STEP_BOXES, sliver(5, 200)[1])                     # the default tap capacity
    with pytest.raises(RuntimeError, match="image 1.*max_gt"):
        step_f(frames, r, [STEP_BOXES[0], np.ones((MAX_GT + 1, 5), np.int64)], labels)
    with pytest.raises(RuntimeError, match="image 0.*integer"):
        step_f(frames, r, [STEP_BOXES[0].astype(np.float32), STEP_BOXES[1]], labels)    # float boxes
    with pytest.raises(RuntimeError, match="synchronise"):
        step_f(frames, r, STEP_BOXES, labels, sizes=torch.tensor(STEP_SIZES).cuda())    # a device tensor for sizes
    with pytest.raises(RuntimeError, match="from_bytes"):
        TrainStep(tf[0], tf[1], tf[2], tf[3], B, S, NS, from_frames=True, from_bytes=True, capacity=STEP_CAP)
    with pytest.raises(RuntimeError, match="capacity"):
        TrainStep(tf[0], tf[1], tf[2], tf[3], B, S, NS, from_frames=True)
    torch.cuda.synchronize()
    after = snapshot(tf)
    assert before[1] == after[1] and all(torch.equal(p, q) for p, q in zip(before[0], after[0]))
    assert step_f.stats()["steps"] == steps_before
    for was, t in zip(inputs, (step_f.x, step_f.png, step_f.labels, step_f.counts, step_f.geom, step_f.boxes)):
        assert torch.equal(was, t)                                                       # nothing was enqueued
    both(A, steps, 41, STEP_SIZES, STEP_BOXES, "after the errors")                       # the next valid call
