"""The training augmentation on the GPU: the four entry points of csrc/augment.hip against the host functions of data.py
(`augment_sample`, `augment_boxes`, `augment_radar`, `hsv_jitter`, `seg_targets`), `data.device_augment_batch_ragged`
against `device_train_batch_ragged`, and `graph.TrainStep(from_frames=True, augment=...)` against `TrainStep(from_bytes=True)`
fed with the host-side augmentation of the same frames.  Both sides of every comparison are integers, the same fp64
arithmetic rounded once, or the same float32 operations without contraction, so every comparison is bit for bit.
Shapes: canvases 64 x 64 (ns = 3) and 40 x 63 (ns = 4: odd width for the flip, W (ns + 1) no multiple of 4, H no multiple
of a workgroup's 16 rows), five frames of mixed sizes in slots of 96 x 112, one explicit record each, which between them
hold every branch (RECORDS).  Steps: nano, 64 x 64, B = 2."""
import numpy as np
import pytest
import torch
from PIL import Image

pytestmark = pytest.mark.gpu

CAP = (96, 112)
SIZES = [(48, 80), (90, 60), (64, 64), (37, 111), (96, 112)]      # those of tests/test_train_frames.py
MAX_GT = 8
CANVASES = [((64, 64), 3), ((40, 63), 4)]
BOXES = [
    np.array([[3, 5, 41, 33, 0], [10, 0, 12, 40, 1], [10, 0, 13, 40, 2], [50, 20, 200, 100, 3], [0, 10, 79, 11, 1],
              [0, 10, 79, 12, 2], [-20, -30, 30, 30, 0], [70, 40, 75, 47, 3]]),          # exactly MAX_GT rows
    np.array([[4, 8, 50, 70, 0], [20, 20, 22, 60, 1], [10, 40, 55, 88, 2], [0, 0, 60, 90, 3], [30, 45, 31, 46, 1]]),
    np.zeros((0, 5), np.int64),
    np.array([[0, 0, 111, 37, 1], [7, 3, 100, 30, 0], [20, 5, 24, 9, 2]]),
    np.array([[0, 0, 112, 96, 3], [111, 95, 112, 96, 2], [13, 17, 59, 61, 1], [30, 20, 33, 90, 0]]),
]


def RECORDS(input_shape, color=None):
    """One record per frame of SIZES; together: (a) a small window well inside the canvas (scale .25; 21 taps per axis), (b) a
    window about twice the canvas at dx < 0, dy < 0, (c) nw == iw and nh == ih at a non-zero offset (both passes skipped), (d)
    dx < 0 <= dy, and a window with nw == iw only (the horizontal pass skipped, the vertical one not) that leaves the canvas
    on the left and, on the 40-row canvas, at the bottom; (e) flip on and off; (f) colour on and off (color: override)."""
    from asy_vrnet_amd import data
    H, W = input_shape
    rows = [((48, 80), W // 4, H // 4 - 6, 20, 17, True, True, (1.07, 1.5, 0.75)),
            ((90, 60), 2 * W - 3, 2 * H - 1, -(W // 2) - 3, -(H // 2), False, True, (0.93, 0.4, 1.35)),
            ((64, 64), 64, 64, 5, -7, True, False, (1, 1, 1)),
            ((37, 111), W + 20, 30, -15, 4, False, False, (1, 1, 1)),
            ((96, 112), 112, 48, -30, 10, True, True, (1.0, 1.69, 1.4))]
    return np.stack([data.aug_record(size, input_shape, nw, nh, dx, dy, flip, c if color is None else color, gains)
                     for size, nw, nh, dx, dy, flip, c, gains in rows])


@pytest.fixture(scope="module")
def A():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    import asy_vrnet_amd
    return asy_vrnet_amd


def cuda(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def aug_tensor(table):
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


def stored_radar(seed, sizes, input_shape):
    """(B, 4, H, W) float32 as the dataset stores it: aligned with the letterbox window of each frame, 0 outside."""
    from asy_vrnet_amd import data
    H, W = input_shape
    out = np.zeros((len(sizes), 4, H, W), np.float32)
    rng = np.random.default_rng(seed)
    for b, (ih, iw) in enumerate(sizes):
        nw, nh, dx, dy = data.letterbox_geometry(iw, ih, W, H)
        out[b, :, dy:dy + nh, dx:dx + nw] = rng.standard_normal((4, nh, nw)).astype(np.float32)
    return out


_HOST = {}


def host_items(seed, input_shape, table, sizes=SIZES, boxes=BOXES, top=6):
    """data.augment_sample per image, computed once per (seed, canvas, table) and shared: (frames, labels, radar, canvases
    (B,H,W,3) u8, label canvases (B,H,W) u8, box lists, radar (B,4,H,W))."""
    from asy_vrnet_amd import data
    key = (seed, input_shape, table.tobytes(), tuple(sizes))
    if key not in _HOST:
        frames, labels = raw_batch(seed, sizes, top)
        radar = stored_radar(seed, sizes, input_shape)
        items = [data.augment_sample(Image.fromarray(f), Image.fromarray(l), bx, r, input_shape, rec)
                 for f, l, bx, r, rec in zip(frames, labels, boxes, radar, table)]
        _HOST[key] = (frames, labels, radar, np.stack([np.array(i[0]) for i in items]), np.stack([np.array(i[2]) for i in items]),
                      [i[1] for i in items], np.stack([i[3] for i in items]))
    return _HOST[key]


def taps(input_shape):
    from asy_vrnet_amd import data
    return data.default_aug_max_taps(CAP, input_shape)


# ---- 1. the frames ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("color", [None, False])
@pytest.mark.parametrize("input_shape,ns", CANVASES)
def test_canvas_and_images_equal_augment_sample(A, input_shape, ns, color):
    from asy_vrnet_amd import data, hip
    H, W = input_shape
    table = data.check_aug_table(RECORDS(input_shape, color), input_shape, CAP, taps(input_shape))
    frames, _, _, want, _, _, _ = host_items(1, input_shape, table)
    B = len(frames)
    canvas = torch.full((B, H, W, 3), 77, dtype=torch.uint8, device="cuda")            # guards: every element is written
    images = torch.full((B, 3, H, W), 7.5, dtype=torch.float32, device="cuda")
    flag = torch.zeros(1, dtype=torch.int32, device="cuda")
    hip.augment_frames(cuda(padded(frames, CAP, 255)), aug_tensor(table), H, W, taps(input_shape), canvas=canvas, images=images,
                       flag=flag)
    assert int(flag) == 0
    got = canvas.cpu().numpy()
    for b in range(B):
        assert np.array_equal(got[b], want[b]), (b, int((got[b] != want[b]).sum()))
    assert torch.equal(images, data.device_batch(want, None, ns)[0])                  # the normalisation of those bytes
    if color is None:                  # the colour stage did something, and it also recoloured the padding of image 0
        plain = host_items(1, input_shape, RECORDS(input_shape, False))[3]
        assert (plain[0] != want[0]).any() and tuple(want[0, 0, 0]) != (128, 128, 128) and tuple(plain[0, 0, 0]) == (128, 128, 128)
        assert np.array_equal(plain[2], want[2])                                       # image 2's record has the stage off


# ---- 2. the segmentation targets ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("input_shape,ns", CANVASES)
def test_seg_targets_equal_seg_targets_of_the_host_label_canvas(A, input_shape, ns):
    from asy_vrnet_amd import data, hip
    H, W = input_shape
    table = RECORDS(input_shape)
    _, labels, _, _, want_labels, _, _ = host_items(1, input_shape, table)
    B = len(labels)
    png = torch.full((B, H, W), -77, dtype=torch.int64, device="cuda")
    onehot = torch.full((B, H, W, ns + 1), 7.5, dtype=torch.float32, device="cuda")
    flag = torch.zeros(1, dtype=torch.int32, device="cuda")
    hip.augment_seg_targets(cuda(padded(labels, CAP, 255)), aug_tensor(table), H, W, ns, png_out=png, onehot=onehot, flag=flag)
    assert int(flag) == 0
    for b in range(B):
        want_png, want_onehot = data.seg_targets(want_labels[b], ns)
        assert np.array_equal(png[b].cpu().numpy(), want_png.astype(np.int64)), b
        assert np.array_equal(onehot[b].cpu().numpy(), want_onehot.astype(np.float32)), b
    assert int(png.max()) == ns and int(png.min()) == 0


# ---- 3. the box targets -------------------------------------------------------------------------------------------------
def run_boxes(table, input_shape, counts=None):
    from asy_vrnet_amd import data, hip
    H, W = input_shape
    packed, cnt = data.pack_boxes(BOXES, MAX_GT)
    if counts is not None:
        cnt = torch.tensor(counts, dtype=torch.int32)
    targets = torch.full((len(SIZES), MAX_GT, 5), -7.0, dtype=torch.float32, device="cuda")
    counts_out = torch.full((len(SIZES),), -1, dtype=torch.int32, device="cuda")
    flag = torch.zeros(1, dtype=torch.int32, device="cuda")
    hip.augment_box_targets(packed.cuda(), cnt.cuda(), aug_tensor(table), CAP, H, W, targets=targets, counts_out=counts_out,
                            flag=flag)
    return targets.cpu().numpy(), counts_out.cpu().numpy(), int(flag)


def host_targets(table, input_shape):
    from asy_vrnet_amd import data
    H, W = input_shape
    return [data.boxes_xyxy_to_cxcywh(data.augment_boxes(bx, iw, ih, W, H, rec)).astype(np.float32)
            for bx, (ih, iw), rec in zip(BOXES, SIZES, table)]


@pytest.mark.parametrize("input_shape,ns", CANVASES)
def test_box_targets_equal_augment_boxes_and_cxcywh(A, input_shape, ns):
    from asy_vrnet_amd import hip
    table = RECORDS(input_shape)
    want = host_targets(table, input_shape)
    got, counts, flag = run_boxes(table, input_shape)
    assert flag == 0
    for b, w in enumerate(want):
        assert counts[b] == len(w), (b, counts[b], len(w))
        assert np.array_equal(got[b, :len(w)], w), (b, got[b], w)
        assert not got[b, len(w):].any(), b                                            # rows behind the count are zero
    assert sum(len(w) for w in want) < sum(len(b) for b in BOXES) and counts[2] == 0   # some rows were dropped
    # the count clamp of the existing box kernel: above max_gt and below 0 are clamped and reported
    got, counts, flag = run_boxes(table, input_shape, counts=[MAX_GT + 3, 3, -2, 2, 3])
    assert flag == hip.FLAG_BOX_COUNT
    assert counts[0] == len(want[0]) and np.array_equal(got[0, :len(want[0])], want[0]) and counts[2] == 0 and not got[2].any()


# ---- 4. the radar -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("input_shape,ns", CANVASES)
def test_radar_equals_the_host_gather(A, input_shape, ns):
    from asy_vrnet_amd import data, hip
    H, W = input_shape
    table = RECORDS(input_shape)
    _, _, radar, _, _, _, want = host_items(1, input_shape, table)
    out = torch.full(radar.shape, 7.5, dtype=torch.float32, device="cuda")
    flag = torch.zeros(1, dtype=torch.int32, device="cuda")
    hip.augment_radar(cuda(radar), aug_tensor(table), CAP, out=out, flag=flag)
    assert int(flag) == 0 and np.array_equal(out.cpu().numpy(), want)
    assert (want[1] != 0).sum() > (radar[1] != 0).sum()                                # the enlarged window duplicates points
    # the identity record -- the letterbox window, no flip -- returns the input bit for bit
    ident = np.stack([data.aug_record(s, input_shape, *data.letterbox_geometry(s[1], s[0], W, H)) for s in SIZES])
    out = hip.augment_radar(cuda(radar), aug_tensor(ident), CAP)
    assert out.cpu().numpy().tobytes() == radar.tobytes()


# ---- 5. the stand-alone batch ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("input_shape,ns", CANVASES)
def test_device_augment_batch_ragged_equals_the_host_items(A, input_shape, ns):
    from asy_vrnet_amd import data
    table = RECORDS(input_shape)
    frames, labels, radar, canvases, label_canvases, _, want_radar = host_items(2, input_shape, table)
    flag = torch.zeros(1, dtype=torch.int32, device="cuda")
    images, png, onehot, targets, counts, rad = data.device_augment_batch_ragged(
        padded(frames, CAP, 255), SIZES, input_shape, padded(labels, CAP, 255), BOXES, radar, ns, table, max_gt=MAX_GT, flag=flag)
    want_images, want_png, want_onehot = data.device_batch(canvases, label_canvases, ns)
    assert int(flag) == 0 and torch.equal(images, want_images) and torch.equal(png, want_png) and torch.equal(onehot, want_onehot)
    for b, w in enumerate(host_targets(table, input_shape)):
        assert int(counts[b]) == len(w) and np.array_equal(targets[b, :len(w)].cpu().numpy(), w)
    assert np.array_equal(rad.cpu().numpy(), want_radar)
    with pytest.raises(RuntimeError, match="image 3.*record is for"):
        data.device_augment_batch_ragged(frames, None, input_shape, labels, BOXES, radar, ns, table[[0, 1, 2, 4, 3]], max_gt=MAX_GT)


@pytest.mark.parametrize("input_shape,ns", CANVASES)
def test_letterbox_records_equal_device_train_batch_ragged(A, input_shape, ns):
    """With letterbox windows, no flip and color=False the augmented path is the frame path: all six outputs, bit for bit."""
    from asy_vrnet_amd import data
    H, W = input_shape
    frames, labels = raw_batch(3)
    radar = stored_radar(3, SIZES, input_shape)
    table = np.stack([data.aug_record(s, input_shape, *data.letterbox_geometry(s[1], s[0], W, H)) for s in SIZES])
    got = data.device_augment_batch_ragged(frames, None, input_shape, labels, BOXES, radar, ns, table, max_gt=MAX_GT, capacity=CAP)
    want = data.device_train_batch_ragged(frames, None, input_shape, labels, BOXES, ns, max_gt=MAX_GT, capacity=CAP)
    for g, w, name in zip(got, want, ("images", "png", "onehot", "targets", "counts")):
        assert g.dtype == w.dtype and torch.equal(g, w), name
    assert torch.equal(got[5], data.device_radar(radar, normalise=False))


# ---- 6. a bad record, and a second call ------------------------------------------------------------------------------------
def run_all(frames, labels, radar, table, input_shape, ns, out=None, boxes=BOXES, counts=None):
    """The four entry points on one table; out: the buffers (and workspace) of an earlier call, to be written again."""
    from asy_vrnet_amd import data, hip
    H, W = input_shape
    B = len(table)
    if out is None:
        out = dict(canvas=torch.full((B, H, W, 3), 77, dtype=torch.uint8, device="cuda"),
                   images=torch.full((B, 3, H, W), 7.5, dtype=torch.float32, device="cuda"),
                   png=torch.full((B, H, W), -77, dtype=torch.int64, device="cuda"),
                   onehot=torch.full((B, H, W, ns + 1), 7.5, dtype=torch.float32, device="cuda"),
                   targets=torch.full((B, MAX_GT, 5), -7.0, dtype=torch.float32, device="cuda"),
                   counts=torch.full((B,), -1, dtype=torch.int32, device="cuda"),
                   radar=torch.full((B, 4, H, W), 7.5, dtype=torch.float32, device="cuda"),
                   flag=torch.zeros(1, dtype=torch.int32, device="cuda"),
                   ws=torch.full((hip.letterbox_ragged_workspace_bytes(B, CAP[0], CAP[1], H, W, taps(input_shape)),), 0x5A,
                                 dtype=torch.uint8, device="cuda"),
                   slots=torch.full((B,) + CAP + (3,), 255, dtype=torch.uint8, device="cuda"),
                   label_slots=torch.full((B,) + CAP, 255, dtype=torch.uint8, device="cuda"))
    sizes = [f.shape[:2] for f in frames]
    data.fill_slots(out["slots"], [torch.from_numpy(f) for f in frames], sizes)
    data.fill_slots(out["label_slots"], [torch.from_numpy(l) for l in labels], sizes)
    aug = aug_tensor(table)
    packed, cnt = data.pack_boxes(boxes, MAX_GT)
    hip.augment_frames(out["slots"], aug, H, W, taps(input_shape), canvas=out["canvas"], images=out["images"], flag=out["flag"],
                       ws=out["ws"])
    hip.augment_seg_targets(out["label_slots"], aug, H, W, ns, png_out=out["png"], onehot=out["onehot"], flag=out["flag"])
    hip.augment_box_targets(packed.cuda(), cnt.cuda(), aug, CAP, H, W, targets=out["targets"], counts_out=out["counts"],
                            flag=out["flag"])
    hip.augment_radar(cuda(radar), aug, CAP, out=out["radar"], flag=out["flag"])
    return out


OUTPUTS = ("canvas", "images", "png", "onehot", "targets", "counts", "radar")


def test_a_record_above_the_capacity_is_flagged_and_its_image_is_padding(A):
    """The device-side backstop behind `check_aug_table`: the host would have raised for this table."""
    from asy_vrnet_amd import data, hip
    input_shape, ns = (40, 63), 4
    table = RECORDS(input_shape)
    frames, labels, radar = host_items(1, input_shape, table)[:3]
    good = run_all(frames, labels, radar, table, input_shape, ns)
    assert int(good["flag"]) == 0
    bad = table.copy()
    bad[1]["ih"] = CAP[0] + 5
    with pytest.raises(RuntimeError, match="image 1.*capacity"):
        data.check_aug_table(bad, input_shape, CAP, taps(input_shape))
    got = run_all(frames, labels, radar, bad, input_shape, ns)
    assert int(got["flag"]) == hip.FLAG_GEOMETRY == 256
    others = [0, 2, 3, 4]
    for name in OUTPUTS:
        assert torch.equal(got[name][others], good[name][others]), name               # the other images are unaffected
    assert (got["canvas"][1] == 128).all() and torch.equal(got["images"][1:2], data.device_batch(got["canvas"][1:2].cpu(), None, ns)[0])
    assert not got["png"][1].any() and (got["onehot"][1, ..., 0] == 1).all() and not got["onehot"][1, ..., 1:].any()
    assert int(got["counts"][1]) == 0 and not got["targets"][1].any() and not got["radar"][1].any()
    # a window beyond twice the canvas, and taps beyond the capacity, are reported as well
    for field, value in (("nw", 2 * 63 + 1), ("dx", 64), ("lb_nw", 64)):
        bad = table.copy()
        bad[3][field] = value
        assert int(run_all(frames, labels, radar, bad, input_shape, ns)["flag"]) == 256, field
    thin = table.copy()
    thin[4]["nh"] = 2                                                                  # 96 rows -> 2: 193 taps
    assert data.resample_ksize(96, 2) > taps(input_shape)
    got = run_all(frames, labels, radar, thin, input_shape, ns)
    assert int(got["flag"]) == 256
    for name in OUTPUTS:
        assert torch.equal(got[name][:4], good[name][:4]), name


def test_a_second_call_with_other_sizes_and_records_leaves_no_trace_of_the_first(A):
    from asy_vrnet_amd import data
    input_shape, ns = (40, 63), 4
    H, W = input_shape
    first = RECORDS(input_shape)
    frames, labels, radar = host_items(1, input_shape, first)[:3]
    used = run_all(frames, labels, radar, first, input_shape, ns)
    # the sizes rotate through the slots; every image gets a record of another kind than its slot saw before
    sizes = SIZES[2:] + SIZES[:2]
    boxes = BOXES[2:] + BOXES[:2]
    rows = [(20, 20, 1, 2, False, True), (W, 13, 0, 30, True, False), (2 * W, 70, -W, -31, False, False), (30, 48, 40, -9, True, True),
            (60, 90, -5, -50, True, True)]
    second = np.stack([data.aug_record(s, input_shape, nw, nh, dx, dy, flip, color, (0.95, 1.2, 1.1))
                       for s, (nw, nh, dx, dy, flip, color) in zip(sizes, rows)])
    data.check_aug_table(second, input_shape, CAP, taps(input_shape))
    frames2, labels2 = raw_batch(5, sizes)
    radar2 = stored_radar(5, sizes, input_shape)
    fresh = run_all(frames2, labels2, radar2, second, input_shape, ns, boxes=boxes)
    again = run_all(frames2, labels2, radar2, second, input_shape, ns, out=used, boxes=boxes)
    assert int(again["flag"]) == 0
    for name in OUTPUTS:
        assert torch.equal(again[name], fresh[name]), name
    want = host_items(5, input_shape, second, sizes, boxes)
    assert np.array_equal(again["canvas"].cpu().numpy(), want[3]) and np.array_equal(again["radar"].cpu().numpy(), want[6])


# ---- 7. the captured step --------------------------------------------------------------------------------------------------
B, S, NC, NS = 2, 64, 4, 9
STEP_CAP = (96, 112)
STEP_SIZES = [(48, 80), (90, 60)]
STEP_BOXES = [np.array([[5, 4, 60, 40, 1], [30, 10, 75, 45, 3]]),
              np.array([[4, 8, 50, 70, 0], [20, 20, 22, 60, 1], [10, 40, 55, 88, 2]])]


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
    """Identical trainers (one seed) under a TrainStep each: host-augmented bytes, and two augmenting steps of one seed."""
    from asy_vrnet_amd.graph import TrainStep
    out = []
    for kw in (dict(from_bytes=True), dict(from_frames=True, capacity=STEP_CAP, augment=True, aug_seed=3),
               dict(from_frames=True, capacity=STEP_CAP, augment={"jitter": .3}, aug_seed=3)):
        t = trainer(A)
        out.append((t, TrainStep(t[0], t[1], t[2], t[3], B, S, NS, max_gt=MAX_GT, **kw)))
    return out


STEP_RECORDS = [
    [((48, 80), 100, 70, -20, -3, True, True, (1.05, 1.3, 0.8)), ((90, 60), 30, 44, 10, 8, False, False, (1, 1, 1))],
    [((90, 60), 60, 57, 3, -11, False, True, (0.92, 0.5, 1.3)), ((40, 50), 128, 100, -64, -30, True, True, (1.1, 1.0, 1.0))],
]
STEP_BOXES2 = [np.array([[4, 8, 50, 70, 0], [10, 40, 55, 88, 2], [1, 1, 30, 30, 3]]), np.array([[3, 3, 44, 33, 2]])]


def test_augmenting_step_equals_from_bytes_on_the_host_augmentation(A, steps):
    from asy_vrnet_amd import data
    (tb, step_b), (ta, step_a) = steps[:2]
    p0 = ta[0].head.stems[0].conv.weight.detach().clone()
    for it, (rows, boxes) in enumerate(zip(STEP_RECORDS, (STEP_BOXES, STEP_BOXES2))):
        sizes = [r[0] for r in rows]
        table = np.stack([data.aug_record(size, (S, S), nw, nh, dx, dy, flip, color, gains)
                          for size, nw, nh, dx, dy, flip, color, gains in rows])
        frames, labels, radar, canvases, label_canvases, host_boxes, host_radar = host_items(20 + it, (S, S), table, sizes, boxes, NS + 3)
        targets = [torch.from_numpy(data.boxes_xyxy_to_cxcywh(bx).astype(np.float32)) for bx in host_boxes]
        rb = step_b(canvases, host_radar, targets, label_canvases)
        ra = step_a(frames, radar, boxes, labels, aug=table)
        assert rb.keys() == ra.keys() == {"total", "loss_det", "loss_seg"}
        assert all(torch.isfinite(rb[k]) and torch.equal(rb[k], ra[k]) for k in rb), (it, rb, ra)
        for name in ("x", "r", "png", "onehot", "labels", "counts"):                  # what the forward pass and the losses read
            assert torch.equal(getattr(step_a, name), getattr(step_b, name)), (it, name)
        trainers_equal(tb, ta, f"step {it}")
        assert step_a.aug_table.tobytes() == table.tobytes()
    st = step_a.stats()
    assert st["steps"] == 2 and st["flag"] == 0 and set(st) == {"steps", "total", "loss_det", "loss_seg", "flag"}
    assert int(step_a.counts.sum()) > 0 and not torch.equal(ta[0].head.stems[0].conv.weight, p0)


def test_two_steps_of_one_seed_draw_the_same_tables_and_validation_comes_first(A, steps):
    from asy_vrnet_amd import data
    step_1, step_2 = steps[1][1], steps[2][1]
    frames, labels = raw_batch(30, STEP_SIZES, top=NS + 3)
    radar = stored_radar(30, STEP_SIZES, (S, S))
    assert step_1.max_taps == step_2.max_taps == data.default_aug_max_taps(STEP_CAP, (S, S))
    # an explicit table for other frames, and a frame above the capacity: raised before anything is enqueued or drawn
    before = step_1.aug.clone(), step_1.x.clone(), step_1.stats()["steps"]
    wrong = np.stack([data.aug_record((48, 81), (S, S), 30, 30, 0, 0), data.aug_record((90, 60), (S, S), 30, 30, 0, 0)])
    with pytest.raises(RuntimeError, match="image 0.*record is for"):
        step_1(frames, radar, STEP_BOXES, labels, aug=wrong)
    tall = [np.zeros((97, 50, 3), np.uint8), frames[1]], [np.zeros((97, 50), np.uint8), labels[1]]
    with pytest.raises(RuntimeError, match="image 0.*capacity"):
        step_1(tall[0], radar, STEP_BOXES, tall[1])
    with pytest.raises(RuntimeError, match="image 0.*capacity"):
        step_2(tall[0], radar, STEP_BOXES, tall[1])
    with pytest.raises(RuntimeError, match="image 1.*max_gt"):                         # step_1 alone: it must not draw for it
        step_1(frames, radar, [STEP_BOXES[0], np.ones((MAX_GT + 1, 5), np.int64)], labels)
    torch.cuda.synchronize()
    assert torch.equal(before[0], step_1.aug) and torch.equal(before[1], step_1.x) and step_1.stats()["steps"] == before[2]
    tables = []
    for it in range(2):
        step_1(frames, radar, STEP_BOXES, labels)
        step_2(frames, radar, STEP_BOXES, labels)
        assert step_1.aug_table.tobytes() == step_2.aug_table.tobytes()               # compared on the host
        assert step_1.aug.cpu().numpy().tobytes() == step_1.aug_table.tobytes()       # ... and it is what the device holds
        tables.append(step_1.aug_table.tobytes())
    assert tables[0] != tables[1]
    rs = np.random.RandomState(3)
    assert tables[0] == data.augment_params(STEP_SIZES, (S, S), rs).tobytes()          # the explicit tables drew nothing
    assert step_1.stats()["flag"] == 0 and step_2.stats()["flag"] == 0


def test_the_prologues_launch_what_they_say(A, steps, monkeypatch):
    """augment=None runs the three entry points it ran before this feature (three, one and one launches) and none of the
    new ones; augment runs the four new entry points (three, one, one and one launches: six nodes) and none of the old."""
    from asy_vrnet_amd import graph
    from asy_vrnet_amd.graph import TrainStep
    calls = []
    names = ("letterbox_ragged", "seg_targets_ragged", "box_targets_ragged", "batch_formats", "augment_frames", "augment_seg_targets",
             "augment_box_targets", "augment_radar")
    for name in names:
        def counted(*a, _f=getattr(graph.hip, name), _n=name, **k):
            calls.append(_n)
            return _f(*a, **k)
        monkeypatch.setattr(graph.hip, name, counted)
    steps[1][1]._prologue()
    assert calls == ["augment_frames", "augment_seg_targets", "augment_box_targets", "augment_radar"]
    del calls[:]
    t = trainer(A)
    plain = TrainStep(t[0], t[1], t[2], t[3], B, S, NS, max_gt=MAX_GT, from_frames=True, capacity=STEP_CAP, warmup=2)
    per_pass = ["letterbox_ragged", "seg_targets_ragged", "box_targets_ragged"]
    assert calls == per_pass * 3                                                       # two warm-up passes and the capture
    assert plain.augment is None and not hasattr(plain, "aug") and not hasattr(plain, "radar_in")
    torch.cuda.synchronize()
