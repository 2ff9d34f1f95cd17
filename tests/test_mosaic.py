"""Mosaic on the GPU: the four entry points of csrc/mosaic.hip against the host functions of data.py (`mosaic_sample`,
`mosaic_boxes`, `seg_targets`), `data.device_mosaic_batch_ragged` against `device_augment_batch_ragged` where the two must
agree, and `graph.TrainStep(from_frames=True, mosaic=...)` against `TrainStep(from_bytes=True)` fed with the host-made
mosaics of the same sources.  Both sides of every comparison are integers, the same fp64 arithmetic rounded once, or the
same float32 operations without contraction, so every comparison is bit for bit.
Shapes: canvases 64 x 64 (ns = 3) and 40 x 63 (ns = 4: odd width, W (ns + 1) no multiple of 4, H no multiple of a workgroup's
16 rows, so a block of rows straddles the cut), eight sources of mixed sizes in slots of 96 x 112, two output images, tables
written by hand which between them hold every branch (TABLES).  Steps: nano, 64 x 64, B = 2."""
import numpy as np
import pytest
import torch
from PIL import Image

pytestmark = pytest.mark.gpu

CAP = (96, 112)
SIZES = [(48, 80), (90, 60), (64, 64), (37, 111), (96, 112), (20, 30), (96, 40), (50, 112)]
MAX_GT = 8
CANVASES = [((64, 64), 3), ((40, 63), 4)]
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
NAMES = ("interior", "edge", "gaps", "corners_a", "corners_b")


def TABLES(input_shape):
    """name -> a table of two records.
    interior   cuts inside the canvas, every tile placed against the cut as the sampler places it (dx = cutx - nw or cutx, dy =
               cuty - nh or cuty), two tiles of each image flipped, colour on (image 0) and off (image 1); an enlarged source
    edge       image 0: one-pixel quadrants (cutx = 1, cuty = H - 1), a flipped tile with nw == iw, a tile with both sizes
               unchanged, a tile with nh == ih; image 1: a window about twice the canvas at negative offsets, one source in
               two tiles, nw == iw and nh == ih again
    gaps       a window smaller than its quadrant that does not touch the cut (grey and 0 show), a window wholly outside its
               quadrant, a window wholly outside the canvas, a window that straddles the cut, absent tiles
    corners_a  cuts (W, H) and (W, 0): tile 0 / tile 1 alone, src = -1 elsewhere
    corners_b  cuts (0, 0) and (0, H): tile 2 / tile 3 alone"""
    from asy_vrnet_amd import data
    H, W = input_shape
    s = SIZES

    def rec(cut, tiles, color=False, gains=(1, 1, 1)):
        return data.mosaic_record(input_shape, cut, tiles, color, gains)
    cx, cy = W // 2 - 5, H // 2 + 3
    interior = [rec((cx, cy), [(0, s[0], 40, 24, cx - 40, cy - 24, 0), (1, s[1], 20, 30, cx - 20, cy, 1), (2, s[2], 45, 45, cx, cy, 0),
                               (3, s[3], 50, 17, cx, cy - 17, 1)], True, (1.07, 1.5, 0.75)),
                rec((W // 3, H // 2), [(4, s[4], 30, 26, W // 3 - 30, H // 2 - 26, 1), (5, s[5], 27, 18, W // 3 - 27, H // 2, 0),
                                       (6, s[6], 16, 38, W // 3, H // 2, 1), (7, s[7], 48, 21, W // 3, H // 2 - 21, 0)])]
    edge = [rec((1, H - 1), [(0, s[0], 80, 60, -79, H - 61, 1), (1, s[1], 30, 40, -29, H - 1, 0), (2, s[2], 64, 64, 1, H - 1, 0),
                             (3, s[3], W + 20, 37, 1, H - 38, 0)], True, (0.93, 0.4, 1.35)),
            rec((W // 2, H // 2), [(4, s[4], 2 * W - 3, 2 * H - 1, -(W // 2) - 3, -(H // 2), 0), (4, s[4], 60, 50, W // 2 - 60, H // 2 - 10, 1),
                                   (5, s[5], 30, 40, W // 2, H // 2, 0), (6, s[6], 33, 96, W // 2 + 2, -50, 1)])]
    gaps = [rec((W // 2, H // 2), [(0, s[0], 20, 12, 3, 2, 1), (1, s[1], 20, 15, 0, 0, 0), (2, s[2], 20, 20, W - 10, H - 10, 0), None],
                True, (1.0, 1.69, 1.4)),
            rec((W // 2, H // 2), [(7, s[7], 30, 20, W, 0, 0), None, (6, s[6], 10, 24, W // 2 + 5, H // 2 + 3, 1),
                                   (5, s[5], 25, 15, W // 2 - 10, 2, 0)])]
    corners_a = [rec((W, H), [(0, s[0], 70, 50, -3, -5, 1), None, None, None], True, (1.05, 1.3, 0.8)),
                 rec((W, 0), [None, (5, s[5], 45, 30, 4, 3, 0), None, None])]
    corners_b = [rec((0, 0), [None, None, (2, s[2], 64, 64, 0, 0, 1), None]),
                 rec((0, H), [None, None, None, (7, s[7], 56, 25, 5, 9, 0)], True, (0.95, 1.2, 1.1))]
    return {n: np.stack(t) for n, t in zip(NAMES, (interior, edge, gaps, corners_a, corners_b))}


@pytest.fixture(scope="module")
def A():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    import asy_vrnet_amd
    return asy_vrnet_amd


def cuda(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def mos_tensor(table):
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
    """(S, 4, H, W) float32 as the dataset stores it: aligned with the letterbox window of each source, 0 outside."""
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
    """data.mosaic_sample per output image, computed once per (seed, canvas, table) and shared: (frames, labels, radar (S, 4, H,
    W), canvases (B, H, W, 3) u8, label canvases (B, H, W) u8, box lists, radar (B, 4, H, W))."""
    from asy_vrnet_amd import data
    key = (seed, input_shape, table.tobytes(), tuple(sizes), top)
    if key not in _HOST:
        frames, labels = raw_batch(seed, sizes, top)
        radar = stored_radar(seed, sizes, input_shape)
        images = [Image.fromarray(f) for f in frames]
        items = [data.mosaic_sample(images, labels, boxes, radar, input_shape, rec) for rec in table]
        _HOST[key] = (frames, labels, radar, np.stack([np.array(i[0]) for i in items]), np.stack([np.array(i[2]) for i in items]),
                      [i[1] for i in items], np.stack([i[3] for i in items]))
    return _HOST[key]


def taps(input_shape):
    from asy_vrnet_amd import data
    return data.default_mosaic_max_taps(CAP, input_shape, prob=0.0)


def checked(name, input_shape):
    from asy_vrnet_amd import data
    return data.check_mosaic_table(TABLES(input_shape)[name], input_shape, SIZES, CAP, taps(input_shape))


# ---- 1. the frames ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", NAMES)
@pytest.mark.parametrize("input_shape,ns", CANVASES)
def test_canvas_and_images_equal_mosaic_sample(A, input_shape, ns, name):
    from asy_vrnet_amd import data, hip
    H, W = input_shape
    table = checked(name, input_shape)
    frames, _, _, want, _, _, _ = host_items(1, input_shape, table)
    B = len(table)
    canvas = torch.full((B, H, W, 3), 77, dtype=torch.uint8, device="cuda")            # guards: every element is written
    images = torch.full((B, 3, H, W), 7.5, dtype=torch.float32, device="cuda")
    flag = torch.zeros(1, dtype=torch.int32, device="cuda")
    hip.mosaic_frames(cuda(padded(frames, CAP, 255)), mos_tensor(table), H, W, taps(input_shape), canvas=canvas, images=images,
                      flag=flag)
    assert int(flag) == 0
    got = canvas.cpu().numpy()
    for b in range(B):
        assert np.array_equal(got[b], want[b]), (b, int((got[b] != want[b]).sum()))
    assert torch.equal(images, data.device_batch(want, None, ns)[0])                  # the normalisation of those bytes
    if name == "gaps":                 # grey shows: recoloured in image 0 (colour on), plain in image 1
        assert tuple(want[1, H - 1, 0]) == (128, 128, 128) and tuple(want[0, H - 1, 0]) != (128, 128, 128)
        assert len(np.unique(want[0, :, :W // 2][H // 2:].reshape(-1, 3), axis=0)) == 1          # tile 1 shows nothing


# ---- 2. the segmentation targets ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", NAMES)
@pytest.mark.parametrize("input_shape,ns", CANVASES)
def test_seg_targets_equal_seg_targets_of_the_host_label_canvas(A, input_shape, ns, name):
    from asy_vrnet_amd import data, hip
    H, W = input_shape
    table = checked(name, input_shape)
    _, labels, _, _, want_labels, _, _ = host_items(1, input_shape, table)
    B = len(table)
    png = torch.full((B, H, W), -77, dtype=torch.int64, device="cuda")
    onehot = torch.full((B, H, W, ns + 1), 7.5, dtype=torch.float32, device="cuda")
    flag = torch.zeros(1, dtype=torch.int32, device="cuda")
    hip.mosaic_seg_targets(cuda(padded(labels, CAP, 255)), mos_tensor(table), H, W, ns, png_out=png, onehot=onehot, flag=flag)
    assert int(flag) == 0
    for b in range(B):
        want_png, want_onehot = data.seg_targets(want_labels[b], ns)
        assert np.array_equal(png[b].cpu().numpy(), want_png.astype(np.int64)), (b, int((png[b].cpu().numpy() != want_png).sum()))
        assert np.array_equal(onehot[b].cpu().numpy(), want_onehot.astype(np.float32)), b
    assert int(png.max()) == ns and int(png.min()) == 0


# ---- 3. the box targets -------------------------------------------------------------------------------------------------
def run_boxes(table, input_shape, boxes=BOXES, counts=None):
    from asy_vrnet_amd import data, hip
    H, W = input_shape
    packed, cnt = data.pack_boxes(boxes, MAX_GT)
    if counts is not None:
        cnt = torch.tensor(counts, dtype=torch.int32)
    targets = torch.full((len(table), MAX_GT, 5), -7.0, dtype=torch.float32, device="cuda")
    counts_out = torch.full((len(table),), -1, dtype=torch.int32, device="cuda")
    flag = torch.zeros(1, dtype=torch.int32, device="cuda")
    hip.mosaic_box_targets(packed.cuda(), cnt.cuda(), mos_tensor(table), CAP, H, W, targets=targets, counts_out=counts_out, flag=flag)
    return targets.cpu().numpy(), counts_out.cpu().numpy(), int(flag)


def host_targets(table, input_shape, boxes=BOXES):
    from asy_vrnet_amd import data
    return [data.boxes_xyxy_to_cxcywh(data.mosaic_boxes(boxes, SIZES, input_shape, rec)).astype(np.float32) for rec in table]


@pytest.mark.parametrize("input_shape,ns", CANVASES)
def test_box_targets_equal_mosaic_boxes_and_cxcywh(A, input_shape, ns):
    from asy_vrnet_amd import hip
    kept = given = 0
    for name in NAMES:
        table = checked(name, input_shape)
        want = host_targets(table, input_shape)
        got, counts, flag = run_boxes(table, input_shape)
        assert flag == 0, name
        for b, w in enumerate(want):
            assert len(w) <= MAX_GT and counts[b] == len(w), (name, b, counts[b], len(w))
            assert np.array_equal(got[b, :len(w)], w), (name, b, got[b], w)
            assert not got[b, len(w):].any(), (name, b)                                # rows behind the count are zero
            kept += len(w)
            given += sum(len(BOXES[s]) for s in table[b]["tile"]["src"] if s >= 0 and BOXES[s] is not None)
    assert 0 < kept < given                                                            # some rows were dropped or cut away
    # a source count above max_gt or below 0 is clamped and reported
    table = checked("interior", input_shape)
    counts_in = [len(b) if b is not None else 0 for b in BOXES]
    counts_in[1], counts_in[2] = MAX_GT + 3, -2
    got, counts, flag = run_boxes(table, input_shape, counts=counts_in)
    assert flag == hip.FLAG_BOX_COUNT
    want = host_targets(table, input_shape)
    assert counts[1] == len(want[1]) and np.array_equal(got[1, :len(want[1])], want[1])          # image 1 names neither source


def test_more_than_max_gt_surviving_boxes_keep_the_first_and_set_the_flag(A):
    """Through the low-level call, which has no host validation: four sources of five boxes each, all of which survive."""
    from asy_vrnet_amd import hip
    input_shape = (64, 64)
    table = checked("interior", input_shape)
    box = np.array([[8, 6, 30, 30, 0], [12, 10, 40, 34, 1], [5, 5, 36, 30, 2], [10, 8, 20, 28, 3], [14, 4, 28, 20, 1]])
    boxes = [box + [k, k, k, k, 0] for k in range(8)]
    want = host_targets(table, input_shape, boxes)
    assert len(want[0]) > MAX_GT and len(want[1]) > MAX_GT
    got, counts, flag = run_boxes(table, input_shape, boxes)
    assert flag == hip.FLAG_BOX_COUNT == 512
    for b in range(2):
        assert counts[b] == MAX_GT and np.array_equal(got[b], want[b][:MAX_GT]), b


# ---- 4. the radar -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", NAMES)
@pytest.mark.parametrize("input_shape,ns", CANVASES)
def test_radar_equals_the_host_gather(A, input_shape, ns, name):
    from asy_vrnet_amd import hip
    H, W = input_shape
    table = checked(name, input_shape)
    _, _, radar, _, _, _, want = host_items(1, input_shape, table)
    out = torch.full((len(table), 4, H, W), 7.5, dtype=torch.float32, device="cuda")
    flag = torch.zeros(1, dtype=torch.int32, device="cuda")
    hip.mosaic_radar(cuda(radar), mos_tensor(table), CAP, out=out, flag=flag)
    assert int(flag) == 0 and out.cpu().numpy().tobytes() == want.tobytes()
    assert want.any()


# ---- 5. the stand-alone batch ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ("interior", "edge"))
@pytest.mark.parametrize("input_shape,ns", CANVASES)
def test_device_mosaic_batch_ragged_equals_the_host_items(A, input_shape, ns, name):
    from asy_vrnet_amd import data
    table = TABLES(input_shape)[name]
    frames, labels, radar, canvases, label_canvases, _, want_radar = host_items(2, input_shape, table)
    flag = torch.zeros(1, dtype=torch.int32, device="cuda")
    images, png, onehot, targets, counts, rad = data.device_mosaic_batch_ragged(
        padded(frames, CAP, 255), SIZES, input_shape, padded(labels, CAP, 255), BOXES, radar, ns, table, max_gt=MAX_GT, flag=flag)
    want_images, want_png, want_onehot = data.device_batch(canvases, label_canvases, ns)
    assert int(flag) == 0 and torch.equal(images, want_images) and torch.equal(png, want_png) and torch.equal(onehot, want_onehot)
    for b, w in enumerate(host_targets(table, input_shape)):
        assert int(counts[b]) == len(w) and np.array_equal(targets[b, :len(w)].cpu().numpy(), w)
    assert np.array_equal(rad.cpu().numpy(), want_radar)
    swapped = table.copy()
    swapped[1]["tile"][2]["src"] = 0
    with pytest.raises(RuntimeError, match="image 1, tile 2.*record is for"):
        data.device_mosaic_batch_ragged(frames, None, input_shape, labels, BOXES, radar, ns, swapped, max_gt=MAX_GT)


@pytest.mark.parametrize("input_shape,ns", CANVASES)
def test_one_tile_unflipped_records_equal_device_augment_batch_ragged(A, input_shape, ns):
    """One record per source with cut = (W, H) and tile 0 alone, unflipped: the Mosaic path is the augmentation path, all six
    outputs bit for bit, colour included."""
    from asy_vrnet_amd import data
    H, W = input_shape
    frames, labels = raw_batch(3)
    radar = stored_radar(3, SIZES, input_shape)
    rows = [(W // 4, H // 4 - 6, 20, 17, True, (1.07, 1.5, 0.75)), (2 * W - 3, 2 * H - 1, -(W // 2) - 3, -(H // 2), True, (0.93, 0.4, 1.35)),
            (64, 64, 5, -7, False, (1, 1, 1)), (W + 20, 30, -15, 4, False, (1, 1, 1)), (112, 48, -30, 10, True, (1.0, 1.69, 1.4)),
            (30, 20, 7, 9, True, (1.1, 1.0, 0.9)), (25, 60, W - 30, -8, False, (1, 1, 1)), (90, 40, -11, H - 35, True, (0.9, 1.2, 1.1))]
    aug = np.stack([data.aug_record(s, input_shape, nw, nh, dx, dy, False, color, gains)
                    for s, (nw, nh, dx, dy, color, gains) in zip(SIZES, rows)])
    mos = np.stack([data.mosaic_record(input_shape, (W, H), [(k, s, nw, nh, dx, dy), None, None, None], color, gains)
                    for k, (s, (nw, nh, dx, dy, color, gains)) in enumerate(zip(SIZES, rows))])
    t = data.default_aug_max_taps(CAP, input_shape)
    got = data.device_mosaic_batch_ragged(frames, None, input_shape, labels, BOXES, radar, ns, mos, max_gt=MAX_GT, capacity=CAP, max_taps=t)
    want = data.device_augment_batch_ragged(frames, None, input_shape, labels, BOXES, radar, ns, aug, max_gt=MAX_GT, capacity=CAP,
                                            max_taps=t)
    for g, w, name in zip(got, want, ("images", "png", "onehot", "targets", "counts", "radar")):
        assert g.dtype == w.dtype and torch.equal(g, w), name
    assert int(got[4].sum()) > 0


# ---- 6. a bad record, and a second call ------------------------------------------------------------------------------------
def run_all(frames, labels, radar, table, input_shape, ns, out=None, boxes=BOXES):
    """The four entry points on one table; out: the buffers (and workspace) of an earlier call, to be written again."""
    from asy_vrnet_amd import data, hip
    H, W = input_shape
    B, S = len(table), len(frames)
    if out is None:
        out = dict(canvas=torch.full((B, H, W, 3), 77, dtype=torch.uint8, device="cuda"),
                   images=torch.full((B, 3, H, W), 7.5, dtype=torch.float32, device="cuda"),
                   png=torch.full((B, H, W), -77, dtype=torch.int64, device="cuda"),
                   onehot=torch.full((B, H, W, ns + 1), 7.5, dtype=torch.float32, device="cuda"),
                   targets=torch.full((B, MAX_GT, 5), -7.0, dtype=torch.float32, device="cuda"),
                   counts=torch.full((B,), -1, dtype=torch.int32, device="cuda"),
                   radar=torch.full((B, 4, H, W), 7.5, dtype=torch.float32, device="cuda"),
                   flag=torch.zeros(1, dtype=torch.int32, device="cuda"),
                   ws=torch.full((hip.mosaic_workspace_bytes(B, CAP[0], CAP[1], H, W, taps(input_shape)),), 0x5A, dtype=torch.uint8,
                                 device="cuda"),
                   slots=torch.full((S,) + CAP + (3,), 255, dtype=torch.uint8, device="cuda"),
                   label_slots=torch.full((S,) + CAP, 255, dtype=torch.uint8, device="cuda"))
    sizes = [f.shape[:2] for f in frames]
    data.fill_slots(out["slots"], [torch.from_numpy(f) for f in frames], sizes)
    data.fill_slots(out["label_slots"], [torch.from_numpy(l) for l in labels], sizes)
    mos = mos_tensor(table)
    packed, cnt = data.pack_boxes(boxes, MAX_GT)
    hip.mosaic_frames(out["slots"], mos, H, W, taps(input_shape), canvas=out["canvas"], images=out["images"], flag=out["flag"],
                      ws=out["ws"])
    hip.mosaic_seg_targets(out["label_slots"], mos, H, W, ns, png_out=out["png"], onehot=out["onehot"], flag=out["flag"])
    hip.mosaic_box_targets(packed.cuda(), cnt.cuda(), mos, CAP, H, W, targets=out["targets"], counts_out=out["counts"], flag=out["flag"])
    hip.mosaic_radar(cuda(radar), mos, CAP, out=out["radar"], flag=out["flag"])
    return out


OUTPUTS = ("canvas", "images", "png", "onehot", "targets", "counts", "radar")


def test_a_tile_above_the_capacity_is_flagged_and_its_image_is_padding(A):
    """The device-side backstop behind `check_mosaic_table`: the host would have raised for these tables.  ONE bad tile
    empties its whole output image; the other image is untouched."""
    from asy_vrnet_amd import data, hip
    input_shape, ns = (40, 63), 4
    table = TABLES(input_shape)["interior"]
    frames, labels, radar = host_items(1, input_shape, table)[:3]
    good = run_all(frames, labels, radar, table, input_shape, ns)
    assert int(good["flag"]) == 0 and int(good["counts"][1]) > 0
    bad = table.copy()
    bad[1]["tile"][2]["ih"] = CAP[0] + 5
    with pytest.raises(RuntimeError, match="image 1, tile 2"):
        data.check_mosaic_table(bad, input_shape, SIZES, CAP, taps(input_shape))
    got = run_all(frames, labels, radar, bad, input_shape, ns)
    assert int(got["flag"]) == hip.FLAG_GEOMETRY == 256
    for name in OUTPUTS:
        assert torch.equal(got[name][0], good[name][0]), name                          # the other image is unaffected
    assert (got["canvas"][1] == 128).all() and torch.equal(got["images"][1:2], data.device_batch(got["canvas"][1:2].cpu(), None, ns)[0])
    assert not got["png"][1].any() and (got["onehot"][1, ..., 0] == 1).all() and not got["onehot"][1, ..., 1:].any()
    assert int(got["counts"][1]) == 0 and not got["targets"][1].any() and not got["radar"][1].any()
    # a source outside the slots, a cut outside the canvas, a window beyond twice the canvas, a stale letterbox window
    for where, field, value in ((0, "src", len(SIZES)), (3, "src", -2), (None, "cutx", 64), (None, "cuty", -1), (1, "nw", 2 * 63 + 1),
                                (2, "dx", 64), (0, "lb_nw", 64), (3, "nh", 0)):
        bad = table.copy()
        if where is None:
            bad[0][field] = value
        else:
            bad[0]["tile"][where][field] = value
        got = run_all(frames, labels, radar, bad, input_shape, ns)
        assert int(got["flag"]) == 256, (where, field)
        assert (got["canvas"][0] == 128).all() and int(got["counts"][0]) == 0 and not got["radar"][0].any(), (where, field)
        for name in OUTPUTS:
            assert torch.equal(got[name][1], good[name][1]), (name, where, field)
    # taps beyond the capacity are reported as well; the other image is as it was
    thin = table.copy()
    thin[1]["tile"][0]["nh"] = 2                                                       # 96 rows -> 2: 193 taps
    assert data.resample_ksize(96, 2) > taps(input_shape)
    got = run_all(frames, labels, radar, thin, input_shape, ns)
    assert int(got["flag"]) == 256
    for name in OUTPUTS:
        assert torch.equal(got[name][0], good[name][0]), name


def test_a_second_call_with_other_sizes_and_records_leaves_no_trace_of_the_first(A):
    from asy_vrnet_amd import data
    input_shape, ns = (40, 63), 4
    first = TABLES(input_shape)["edge"]
    frames, labels, radar = host_items(1, input_shape, first)[:3]
    used = run_all(frames, labels, radar, first, input_shape, ns)
    # the sizes rotate through the slots, and the records are of another kind than their images saw before
    sizes = SIZES[3:] + SIZES[:3]
    boxes = BOXES[3:] + BOXES[:3]
    src = lambda k: (k, sizes[k])
    second = np.stack([
        data.mosaic_record(input_shape, (40, 12), [src(0) + (30, 10, 5, 1, 0), src(1) + (50, 40, -20, 12, 1), src(2) + (20, 30, 41, 15, 0),
                                                   src(3) + (22, 11, 40, 0, 1)]),
        data.mosaic_record(input_shape, (20, 30), [src(4) + (64, 64, -44, -34, 1), None, src(6) + (60, 60, 20, 30, 0),
                                                   src(7) + (45, 28, 22, 3, 1)], True, (0.95, 1.2, 1.1))])
    data.check_mosaic_table(second, input_shape, sizes, CAP, taps(input_shape))
    frames2, labels2 = raw_batch(5, sizes)
    radar2 = stored_radar(5, sizes, input_shape)
    fresh = run_all(frames2, labels2, radar2, second, input_shape, ns, boxes=boxes)
    again = run_all(frames2, labels2, radar2, second, input_shape, ns, out=used, boxes=boxes)
    assert int(again["flag"]) == 0
    for name in OUTPUTS:
        assert torch.equal(again[name], fresh[name]), name
    want = host_items(5, input_shape, second, sizes, boxes)
    assert np.array_equal(again["canvas"].cpu().numpy(), want[3]) and np.array_equal(again["radar"].cpu().numpy(), want[6])
    assert np.array_equal(again["png"].cpu().numpy(), np.minimum(want[4], ns))


# ---- 7. the captured step --------------------------------------------------------------------------------------------------
B, S, NC, NS = 2, 64, 4, 9


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
    """Identical trainers (one seed) under a TrainStep each: host-made mosaics as bytes, and two Mosaic steps of one seed."""
    from asy_vrnet_amd.graph import TrainStep
    out = []
    for kw in (dict(from_bytes=True), dict(from_frames=True, capacity=CAP, mosaic=True, aug_seed=3),
               dict(from_frames=True, capacity=CAP, mosaic={"jitter": .3}, augment={"flip": .5}, aug_seed=3)):
        t = trainer(A)
        out.append((t, TrainStep(t[0], t[1], t[2], t[3], B, S, NS, max_gt=MAX_GT, **kw)))
    return out


def test_mosaic_step_equals_from_bytes_on_the_host_mosaics(A, steps):
    from asy_vrnet_amd import data
    (tb, step_b), (ta, step_a) = steps[:2]
    p0 = ta[0].head.stems[0].conv.weight.detach().clone()
    for it, name in enumerate(("interior", "gaps")):
        table = TABLES((S, S))[name]
        frames, labels, radar, canvases, label_canvases, host_boxes, host_radar = host_items(20 + it, (S, S), table, top=NS + 3)
        targets = [torch.from_numpy(data.boxes_xyxy_to_cxcywh(bx).astype(np.float32)) for bx in host_boxes]
        rb = step_b(canvases, host_radar, targets, label_canvases)
        ra = step_a(frames, radar, BOXES, labels, aug=table)
        assert rb.keys() == ra.keys() == {"total", "loss_det", "loss_seg"}
        assert all(torch.isfinite(rb[k]) and torch.equal(rb[k], ra[k]) for k in rb), (it, rb, ra)
        for attr in ("x", "r", "png", "onehot", "labels", "counts"):                  # what the forward pass and the losses read
            assert torch.equal(getattr(step_a, attr), getattr(step_b, attr)), (it, attr)
        trainers_equal(tb, ta, f"step {it}")
        assert step_a.aug_table.tobytes() == table.tobytes()
        assert int(step_a.counts.sum()) > 0
    st = step_a.stats()
    assert st["steps"] == 2 and st["flag"] == 0 and set(st) == {"steps", "total", "loss_det", "loss_seg", "flag"}
    assert not torch.equal(ta[0].head.stems[0].conv.weight, p0)


def test_two_steps_of_one_seed_draw_the_same_tables_and_validation_comes_first(A, steps):
    from asy_vrnet_amd import data
    step_1, step_2 = steps[1][1], steps[2][1]
    frames, labels = raw_batch(30, top=NS + 3)
    radar = stored_radar(30, SIZES, (S, S))
    assert step_1.max_taps == step_2.max_taps == data.default_mosaic_max_taps(CAP, (S, S), prob=0.0)
    # an explicit table for other sources, a frame above the capacity, too many boxes: raised before anything is enqueued
    # or drawn
    before = step_1.aug.clone(), step_1.x.clone(), step_1.stats()["steps"]
    wrong = TABLES((S, S))["interior"].copy()
    wrong[0]["tile"][1]["iw"] = 61
    with pytest.raises(RuntimeError, match="image 0, tile 1.*record is for"):
        step_1(frames, radar, BOXES, labels, aug=wrong)
    with pytest.raises(RuntimeError, match="MOSAIC_DTYPE"):
        step_1(frames, radar, BOXES, labels, aug=TABLES((S, S))["interior"][:1])
    tall = [np.zeros((97, 50, 3), np.uint8)] + frames[1:], [np.zeros((97, 50), np.uint8)] + labels[1:]
    with pytest.raises(RuntimeError, match="image 0.*capacity"):
        step_1(tall[0], radar, BOXES, tall[1])
    with pytest.raises(RuntimeError, match="image 0.*capacity"):
        step_2(tall[0], radar, BOXES, tall[1])
    with pytest.raises(RuntimeError, match="8 frames for a batch of 2|2 frames for a batch of 8"):
        step_1(frames[:2], radar[:2], BOXES[:2], labels[:2])
    many = BOXES[:4] + [np.ones((3, 5), np.int64)] * 3 + [None]                        # image 1: 9 boxes from sources of 3
    with pytest.raises(RuntimeError, match="image 1.*9 boxes together.*max_gt"):       # step_1 alone: it must not draw for it
        step_1(frames, radar, many, labels)
    with pytest.raises(RuntimeError, match="image 5.*max_gt"):
        step_1(frames, radar, BOXES[:5] + [np.ones((MAX_GT + 1, 5), np.int64)] + BOXES[6:], labels)
    torch.cuda.synchronize()
    assert torch.equal(before[0], step_1.aug) and torch.equal(before[1], step_1.x) and step_1.stats()["steps"] == before[2]
    tables = []
    for it in range(2):
        step_1(frames, radar, BOXES, labels)
        step_2(frames, radar, BOXES, labels)
        assert step_1.aug_table.tobytes() == step_2.aug_table.tobytes()               # compared on the host
        assert step_1.aug.cpu().numpy().tobytes() == step_1.aug_table.tobytes()       # ... and it is what the device holds
        tables.append(step_1.aug_table.tobytes())
    assert tables[0] != tables[1]
    rs = np.random.RandomState(3)
    assert tables[0] == data.mosaic_params(SIZES, (S, S), rs, B).tobytes()             # the explicit tables drew nothing
    # mosaic_prob is read at every call: one assignment, no new capture
    step_1.mosaic_prob = 0.0
    step_1(frames, radar, BOXES, labels)
    assert [int(v) for v in step_1.aug_table["cutx"]] == [S, S] and (step_1.aug_table["tile"]["src"][:, 1:] == -1).all()
    data.mosaic_params(SIZES, (S, S), rs, B)
    assert step_1.aug_table.tobytes() == data.mosaic_params(SIZES, (S, S), rs, B, prob=0.0).tobytes()
    step_1.mosaic_prob = 1.0
    assert step_1.stats()["flag"] == 0 and step_2.stats()["flag"] == 0


def test_the_prologues_launch_what_they_say(A, steps, monkeypatch):
    """mosaic=None steps, plain and augmenting, run the entry points they ran before this feature and none of the new ones;
    the Mosaic step runs the four new entry points (three, one, one and one launches: six nodes) and none of the old."""
    from asy_vrnet_amd import graph
    from asy_vrnet_amd.graph import TrainStep
    calls = []
    names = ("letterbox_ragged", "seg_targets_ragged", "box_targets_ragged", "batch_formats", "augment_frames", "augment_seg_targets",
             "augment_box_targets", "augment_radar", "mosaic_frames", "mosaic_seg_targets", "mosaic_box_targets", "mosaic_radar", "radar_map")
    for name in names:
        def counted(*a, _f=getattr(graph.hip, name), _n=name, **k):
            calls.append(_n)
            return _f(*a, **k)
        monkeypatch.setattr(graph.hip, name, counted)
    steps[1][1]._prologue()
    steps[2][1]._prologue()                                                            # with augment as the plain draw's keywords
    assert calls == ["mosaic_frames", "mosaic_seg_targets", "mosaic_box_targets", "mosaic_radar"] * 2
    del calls[:]
    steps[0][1]._prologue()
    assert calls == ["batch_formats"]
    del calls[:]
    t = trainer(A)
    plain = TrainStep(t[0], t[1], t[2], t[3], B, S, NS, max_gt=MAX_GT, from_frames=True, capacity=CAP, warmup=2)
    assert calls == ["letterbox_ragged", "seg_targets_ragged", "box_targets_ragged"] * 3          # two warm-up passes and the capture
    assert plain.augment is None and plain.mosaic is None and not hasattr(plain, "aug") and not hasattr(plain, "radar_in")
    assert plain.frames_u8.shape[0] == B and not hasattr(plain, "mosaic_prob")
    del calls[:]
    t = trainer(A)
    aug = TrainStep(t[0], t[1], t[2], t[3], B, S, NS, max_gt=MAX_GT, from_frames=True, capacity=CAP, augment=True, warmup=2)
    assert calls == ["augment_frames", "augment_seg_targets", "augment_box_targets", "augment_radar"] * 3
    assert aug.mosaic is None and aug.aug.shape == (B, 816) and aug.radar_in.shape[0] == B and aug.frames_u8.shape[0] == B
    torch.cuda.synchronize()


def test_the_three_constructor_errors(A):
    from asy_vrnet_amd.graph import TrainStep
    t = trainer(A)
    with pytest.raises(RuntimeError, match="mosaic needs from_frames"):
        TrainStep(t[0], t[1], t[2], t[3], B, S, NS, mosaic=True)
    with pytest.raises(RuntimeError, match="mosaic with radar_points"):
        TrainStep(t[0], t[1], t[2], t[3], B, S, NS, from_frames=True, capacity=CAP, mosaic=True, radar_points=64)
    with pytest.raises(RuntimeError, match="mosaic places the tiles itself"):
        TrainStep(t[0], t[1], t[2], t[3], B, S, NS, from_frames=True, capacity=CAP, mosaic=True, letterbox_image=False)
