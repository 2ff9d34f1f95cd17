"""Detection NMS (csrc/nms.hip): a float32 numpy restatement of utils/utils_bbox.py:86-135 -- per-class greedy NMS in the
form of the reference's own commented loop (:161-172) with torchvision's CPU IoU expression -- pinned on hand-built cases,
then the HIP path (decode.non_max_suppression, decode.batched_nms, torch.ops.vrnet.batched_nms) against it."""
import numpy as np
import pytest
import torch

import asy_vrnet_amd.ops  # noqa: F401  (registers torch.ops.vrnet.*)
from asy_vrnet_amd import decode
from asy_vrnet_amd.decode import batched_nms, non_max_suppression

F32 = np.float32


# ---- the restatement -----------------------------------------------------------------------------------------------

def suppressed(bi, bj, thr):
    """IoU(bi, rows of bj) > thr, evaluated as torchvision's CPU kernel does: fp32, one rounding per operation,
    std::max / std::min operand order, the comparison in double.  Two zero-area boxes give 0/0 = NaN: not suppressed."""
    bi, bj = bi.astype(F32), bj.astype(F32)
    area_i = (bi[2] - bi[0]) * (bi[3] - bi[1])
    area_j = (bj[:, 2] - bj[:, 0]) * (bj[:, 3] - bj[:, 1])
    xx1 = np.where(bi[0] < bj[:, 0], bj[:, 0], bi[0])
    yy1 = np.where(bi[1] < bj[:, 1], bj[:, 1], bi[1])
    xx2 = np.where(bj[:, 2] < bi[2], bj[:, 2], bi[2])
    yy2 = np.where(bj[:, 3] < bi[3], bj[:, 3], bi[3])
    w, h = xx2 - xx1, yy2 - yy1
    w = np.where(F32(0) < w, w, F32(0))
    h = np.where(F32(0) < h, h, F32(0))
    inter = w * h
    with np.errstate(invalid="ignore", divide="ignore"):
        iou = inter / (area_i + area_j - inter)
    assert iou.dtype == F32
    return iou.astype(np.float64) > thr


def greedy_nms(boxes, scores, classes, ids, thr):
    """Indices of the kept rows by (score descending, id ascending): per class, take the best remaining box and drop the
    rest of its class that it suppresses (utils_bbox.py:161-172 with the IoU rule above)."""
    keep = []
    for c in np.unique(classes):
        order = np.nonzero(classes == c)[0]
        order = order[np.lexsort((ids[order], -scores[order]))]
        while len(order):
            keep.append(order[0])
            rest = order[1:]
            order = rest[~suppressed(boxes[order[0]], boxes[rest], thr)]
    keep = np.asarray(keep, dtype=np.int64)
    return keep[np.lexsort((ids[keep], -scores[keep]))]


def correct_boxes(det, input_shape, image_shape, letterbox):
    """(x1, y1, x2, y2) normalised to the network input -> (top, left, bottom, right) pixels of the original image."""
    centre = ((det[:, 0:2] + det[:, 2:4]) / 2)[:, ::-1].astype(np.float64)
    size = (det[:, 2:4] - det[:, 0:2])[:, ::-1].astype(np.float64)
    net, img = np.array(input_shape, np.float64), np.array(image_shape, np.float64)
    if letterbox:
        inner = np.round(img * np.min(net / img))
        centre = (centre - (net - inner) / 2.0 / net) * (net / inner)
        size = size * (net / inner)
    return np.concatenate([centre - size / 2.0, centre + size / 2.0], axis=1) * np.concatenate([img, img])


def nms_restated(prediction, num_classes, input_shape, image_shape, letterbox, conf_thres, nms_thres):
    out = []
    for p in np.asarray(prediction, dtype=F32):
        cls = p[:, 5:5 + num_classes]
        class_conf, class_pred = cls.max(axis=1), cls.argmax(axis=1)
        score = p[:, 4] * class_conf
        with np.errstate(invalid="ignore"):
            passed = np.nonzero(score >= F32(conf_thres))[0]
        half_w, half_h = p[:, 2] / F32(2), p[:, 3] / F32(2)
        det = np.stack([p[:, 0] - half_w, p[:, 1] - half_h, p[:, 0] + half_w, p[:, 1] + half_h, p[:, 4], class_conf,
                        class_pred.astype(F32)], axis=1)[passed]
        det = det[greedy_nms(det[:, :4], score[passed], class_pred[passed], passed, nms_thres)]
        if len(det):
            det[:, :4] = correct_boxes(det, input_shape, image_shape, letterbox)
        out.append(det.astype(F32))
    return out


def row(cx, cy, w, h, obj, *cls):
    return [cx, cy, w, h, obj, *cls]


def run_restated(rows, num_classes=2, conf=0.1, nms=0.5, letterbox=False, image_shape=(1, 1)):
    pred = np.asarray([rows], dtype=F32)
    return nms_restated(pred, num_classes, (1, 1), image_shape, letterbox, conf, nms)[0]


# ---- the restatement pinned on hand-built cases ---------------------------------------------------------------------

def test_restated_same_class_overlap_drops_lower_score():
    det = run_restated([row(.5, .5, .4, .4, .9, .9, .1), row(.52, .5, .4, .4, .8, .9, .1)])
    assert det.shape == (1, 7) and det[0, 4] == F32(.9)


def test_restated_other_class_keeps_both():
    det = run_restated([row(.5, .5, .4, .4, .9, .9, .1), row(.52, .5, .4, .4, .8, .1, .9)])
    assert det.shape == (2, 7) and list(det[:, 6]) == [0, 1]


def test_restated_iou_equal_to_threshold_is_kept():
    # corners (0, 0, 2, 1) and (0, 0, 1, 1): IoU = 1 / (2 + 1 - 1) = 0.5 exactly; 0.5 > 0.5 is false
    boxes = np.array([[0, 0, 2, 1], [0, 0, 1, 1]], F32)
    assert not suppressed(boxes[0], boxes[1:], 0.5)[0]
    assert suppressed(boxes[0], boxes[1:], 0.49)[0]
    det = run_restated([row(1, .5, 2, 1, .9, .9, 0), row(.5, .5, 1, 1, .8, .9, 0)], nms=0.5)
    assert det.shape == (2, 7)
    assert run_restated([row(1, .5, 2, 1, .9, .9, 0), row(.5, .5, 1, 1, .8, .9, 0)], nms=0.49).shape == (1, 7)


def test_restated_score_at_threshold_is_kept():
    # 0.5 * 0.5 = 0.25 exactly
    det = run_restated([row(.2, .2, .1, .1, .5, .5, 0), row(.7, .7, .1, .1, .5, .4999, 0)], conf=0.25)
    assert det.shape == (1, 7) and det[0, 5] == F32(.5)


def test_restated_reads_num_classes_channels_only():
    # channel 7 (a third class channel) is larger but not read with num_classes = 2
    det = run_restated([row(.5, .5, .2, .2, .9, .3, .6, 1.0)], num_classes=2)
    assert det.shape == (1, 7) and det[0, 5] == F32(.6) and det[0, 6] == 1
    det = run_restated([row(.5, .5, .2, .2, .9, .3, .6, 1.0)], num_classes=3)
    assert det[0, 5] == 1 and det[0, 6] == 2


def test_restated_equal_scores_lower_anchor_first():
    det = run_restated([row(.8, .8, .1, .1, .5, .5, 0), row(.2, .2, .1, .1, .5, .5, 0), row(.5, .5, .1, .1, .5, .5, 0)])
    assert det.shape == (3, 7)
    assert np.allclose((det[:, 0] + det[:, 2]) / 2, [.8, .2, .5])        # anchor order 0, 1, 2
    # coincident boxes, equal scores: only the lowest anchor survives
    det = run_restated([row(.3, .3, .2, .2, .5, .5, 0)] * 3 + [row(.31, .3, .2, .2, .5, .5, 0)])
    assert det.shape == (1, 7)


def test_restated_zero_area_boxes_are_kept():
    det = run_restated([row(.5, .5, 0, 0, .9, .9, 0), row(.5, .5, 0, 0, .8, .9, 0), row(.5, .5, 0, .2, .7, .9, 0)])
    assert det.shape == (3, 7)


def test_restated_nothing_passes_gives_empty_float32():
    det = run_restated([row(.5, .5, .2, .2, .1, .1, .1)], conf=0.5)
    assert det.shape == (0, 7) and det.dtype == F32


def test_restated_letterbox_on_and_off():
    # a 360 x 640 image letterboxed into 512 x 512: scale 0.8 -> 288 x 512, 112 px of padding above and below
    pred = np.asarray([[row(.5, .5, .2, .4, .9, .9, 0)]], F32)
    on = nms_restated(pred, 2, (512, 512), (360, 640), True, 0.1, 0.5)[0]
    off = nms_restated(pred, 2, (512, 512), (360, 640), False, 0.1, 0.5)[0]
    assert np.allclose(on[0, :4], [180 - 128, 320 - 64, 180 + 128, 320 + 64], atol=1e-4)
    assert np.allclose(off[0, :4], [180 - 72, 320 - 64, 180 + 72, 320 + 64], atol=1e-4)
    # the product's host un-map agrees
    det = np.array([[.4, .3, .6, .7]], F32)
    xy, wh = (det[:, 0:2] + det[:, 2:4]) / 2, det[:, 2:4] - det[:, 0:2]
    for lb in (False, True):
        assert np.allclose(decode.yolo_correct_boxes(xy, wh, (512, 512), (360, 640), lb),
                           correct_boxes(det, (512, 512), (360, 640), lb), atol=1e-4)


def test_non_max_suppression_rejects_cpu_input():
    with pytest.raises(RuntimeError):
        non_max_suppression(torch.zeros(1, 8, 7), 2, (64, 64), (64, 64), False)
    with pytest.raises(RuntimeError):
        batched_nms(torch.zeros(2, 4), torch.zeros(2), torch.zeros(2, dtype=torch.int64), 0.5)


def test_exports_and_fake_kernel():
    import asy_vrnet_amd.hip as hip
    from torch._subclasses.fake_tensor import FakeTensorMode
    from torch.fx.experimental.symbolic_shapes import ShapeEnv
    assert hip.ABI_VERSION == 11
    assert {"vrnet_detect_select_f32", "vrnet_nms_workspace_bytes", "vrnet_nms_segmented_f32"} <= set(hip.EXPORTED)
    # mask of 100 boxes: 100 rows of 2 words, plus the ordered copies
    assert hip.nms_workspace_bytes(1, 100) >= 100 * 2 * 8 + 100 * (16 + 8 + 4)
    with FakeTensorMode(shape_env=ShapeEnv()):
        out = torch.ops.vrnet.batched_nms(torch.empty(10, 4, device="cuda"), torch.empty(10, device="cuda"),
                                          torch.empty(10, dtype=torch.int64, device="cuda"), 0.5)
    assert out.dtype == torch.int64 and out.dim() == 1 and isinstance(out.shape[0], torch.SymInt)


# ---- the HIP path against the restatement ---------------------------------------------------------------------------

def random_prediction(B, A, nc, seed, C=None):
    """Decoded-looking predictions: normalised centres in [0, 1], sizes in [0.01, 0.3], sigmoid-range confidences."""
    rng = np.random.default_rng(seed)
    C = C or 5 + nc
    p = np.empty((B, A, C), F32)
    p[..., 0:2] = rng.random((B, A, 2), dtype=F32)
    p[..., 2:4] = F32(0.01) + F32(0.29) * rng.random((B, A, 2), dtype=F32)
    p[..., 4:] = rng.random((B, A, C - 4), dtype=F32)
    return torch.from_numpy(p)


def check(pred, nc, conf, nms, image_shape=(360, 640), letterbox=True, input_shape=(512, 512)):
    before = pred.clone()
    got = non_max_suppression(pred, nc, input_shape, image_shape, letterbox, conf_thres=conf, nms_thres=nms)
    want = nms_restated(pred.cpu().numpy(), nc, input_shape, image_shape, letterbox, conf, nms)
    assert torch.equal(pred, before), "prediction was modified"
    assert len(got) == len(want) == pred.shape[0]
    for g, w in zip(got, want):
        assert isinstance(g, np.ndarray) and g.dtype == F32 and g.shape == w.shape, (g.shape, w.shape)
        assert np.array_equal(g[:, 4:].view(np.uint32), w[:, 4:].view(np.uint32))
        assert np.abs(g[:, :4].astype(np.float64) - w[:, :4]).max(initial=0) <= 1e-3
    return got


CASES = [  # (B, A, nc, conf, nms): every value of each axis appears, both anchor counts with every class count
    (1, 5376, 1, 0.001, 0.5), (3, 5376, 4, 0.3, 0.4), (1, 5376, 20, 0.5, 0.65), (3, 5376, 20, 0.001, 0.4),
    (3, 5376, 1, 0.3, 0.65), (1, 5376, 4, 0.001, 0.65),
    (1, 21504, 1, 0.3, 0.5), (3, 21504, 4, 0.001, 0.5), (1, 21504, 20, 0.001, 0.65), (3, 21504, 20, 0.3, 0.4),
    (1, 21504, 4, 0.5, 0.4), (3, 21504, 1, 0.5, 0.65),
]


@pytest.mark.gpu
@pytest.mark.parametrize("B,A,nc,conf,nms", CASES)
def test_nms_matches_restatement(B, A, nc, conf, nms):
    check(random_prediction(B, A, nc, seed=A + 7 * nc + B).cuda(), nc, conf, nms)


@pytest.mark.gpu
def test_nms_extra_class_channels_and_no_letterbox():
    pred = random_prediction(2, 5376, 6, seed=3).cuda()
    check(pred, 4, 0.05, 0.5, letterbox=False)


@pytest.mark.gpu
def test_nms_all_anchors_one_class():
    # 21 504 candidates of one class: the largest mask (21 504 x 336 words)
    got = check(random_prediction(1, 21504, 1, seed=11).cuda(), 1, 0.0, 0.5)
    assert len(got[0]) > 0


@pytest.mark.gpu
def test_nms_coincident_boxes_equal_scores():
    rng = np.random.default_rng(4)
    p = random_prediction(2, 5376, 3, seed=5).numpy()
    p[..., 0:4] = p[0, rng.integers(0, 12, size=5376), 0:4]           # 12 distinct boxes
    p[..., 4] = F32(0.75)
    p[..., 5:] = np.array([0.5, 0.25, 0.125], F32)[rng.integers(0, 3, size=(2, 5376, 3))]
    got = check(torch.from_numpy(p).cuda(), 3, 0.01, 0.5)
    assert all(len(g) > 0 for g in got)


@pytest.mark.gpu
def test_nms_counts_not_multiple_of_64_and_empty_image():
    p = random_prediction(3, 1000, 2, seed=9).numpy()
    p[1, :, 4] = 0                                                   # image 1: no candidate at conf > 0
    got = check(torch.from_numpy(p).cuda(), 2, 1e-6, 0.45)
    assert got[1].shape == (0, 7) and len(got[0]) and len(got[2])
    # 1000 candidates exactly (conf 0), and an odd count from a random threshold
    check(torch.from_numpy(p).cuda(), 2, 0.0, 0.5)
    check(torch.from_numpy(p[:1]).cuda(), 2, 0.377, 0.5)
    # nothing passes anywhere
    assert [g.shape for g in check(torch.from_numpy(p).cuda(), 2, 1.5, 0.5)] == [(0, 7)] * 3


@pytest.mark.gpu
def test_nms_deterministic_and_input_unchanged():
    pred = random_prediction(3, 5376, 4, seed=21).cuda()
    before = pred.clone()
    a = non_max_suppression(pred, 4, (512, 512), (512, 512), False, conf_thres=0.01, nms_thres=0.5)
    b = non_max_suppression(pred, 4, (512, 512), (512, 512), False, conf_thres=0.01, nms_thres=0.5)
    assert torch.equal(pred, before)
    assert all(np.array_equal(x.view(np.uint32), y.view(np.uint32)) for x, y in zip(a, b))


@pytest.mark.gpu
def test_batched_nms_pixel_boxes_large_class_ids():
    rng = np.random.default_rng(8)
    n = 3000
    xy = rng.random((n, 2), dtype=F32) * F32(1000)
    wh = F32(5) + rng.random((n, 2), dtype=F32) * F32(200)
    boxes = np.concatenate([xy, xy + wh], axis=1).astype(F32)
    scores = rng.random(n, dtype=F32)
    scores[::7] = scores[0]                                          # ties: the lower index first
    classes = np.array([0, 7, 2 ** 40, 2 ** 40 + 1, -3], np.int64)[rng.integers(0, 5, size=n)]
    want = greedy_nms(boxes, scores, classes, np.arange(n), 0.5)
    args = [torch.from_numpy(t).cuda() for t in (boxes, scores, classes)]
    for fn in (batched_nms, torch.ops.vrnet.batched_nms):
        got = fn(*args, 0.5)
        assert got.is_cuda and got.dtype == torch.int64
        assert np.array_equal(got.cpu().numpy(), want)
    empty = batched_nms(torch.empty(0, 4).cuda(), torch.empty(0).cuda(), torch.empty(0, dtype=torch.int64).cuda(), 0.5)
    assert empty.shape == (0,) and empty.dtype == torch.int64 and empty.is_cuda
    empty = torch.ops.vrnet.batched_nms(torch.empty(0, 4).cuda(), torch.empty(0).cuda(),
                                        torch.empty(0, dtype=torch.int64).cuda(), 0.5)
    assert empty.shape == (0,)


@pytest.mark.gpu
def test_end_to_end_nano():
    import asy_vrnet_amd as A
    model = A.EfficientVRNet(4, 9, "nano", img_size=128).cuda().eval()
    A.randomize_state_dict(model.state_dict(), seed=2)
    x, r = A.synthetic_inputs(2, 128, 1, "cuda")
    with torch.no_grad():
        det, _ = model(x, r)
        pred = decode.decode_outputs(det, (128, 128))
    for conf in (0.001, 0.3):
        check(pred, 4, conf, 0.5, image_shape=(360, 640), input_shape=(128, 128))
