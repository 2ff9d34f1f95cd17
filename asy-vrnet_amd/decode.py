"""Box decode and NMS of the det maps, mirroring utils/utils_bbox.py: `decode_outputs` runs as one HIP
kernel (no concat / grid / stride tensors); `non_max_suppression` as the HIP select + NMS kernels of csrc/nms.hip, in
place of the torchvision `batched_nms` the reference calls (utils_bbox.py:124); `yolo_correct_boxes` is the reference's
host-side letterbox un-map (numpy, on the handful of boxes that survive NMS).  `seg_predict` is the class map of the seg
logits (utils_seg/callbacks.py:113-160, deeplab.py:141-167) as the two HIP kernels of csrc/segpost.hip."""
import numpy as np
import torch

from . import hip
from .metrics import MAX_CLASSES as SEG_MAX_CLASSES


def decode_outputs(outputs, input_shape, local_rank=None):
    """outputs: list of (B, 5+nc, h, w) raw head maps on the GPU (P3, P4, P5); input_shape = (H, W).
    Returns (B, sum h*w, 5+nc): normalised cx, cy, w, h, then sigmoid(obj), sigmoid(cls...).  utils_bbox.py:32-84
    (`local_rank` is accepted for signature parity; the result lives on the inputs' device)."""
    outs = [o.detach().contiguous().float() for o in outputs]
    if not outs or not all(o.is_cuda and o.dim() == 4 and o.shape[:2] == outs[0].shape[:2] for o in outs):
        raise RuntimeError("decode_outputs: expects a list of (B, 5+nc, h, w) GPU tensors of one batch")
    B, C = outs[0].shape[:2]
    A = sum(o.shape[2] * o.shape[3] for o in outs)
    out = torch.empty((B, A, C), dtype=torch.float32, device=outs[0].device)
    hip.decode_outputs(outs, input_shape[0], input_shape[1], out)
    return out


def yolo_correct_boxes(box_xy, box_wh, input_shape, image_shape, letterbox_image):
    """Normalised (cx, cy), (w, h) of the network input -> (y1, x1, y2, x2) in pixels of the original image, undoing
    the letterbox when there was one (interface of utils/utils_bbox.py:5-30; host side, on the few boxes NMS keeps).
    input_shape / image_shape are (H, W)."""
    net_hw = np.asarray(input_shape, dtype=np.float64)
    img_hw = np.asarray(image_shape, dtype=np.float64)
    centre = np.asarray(box_xy, dtype=np.float64)[..., ::-1]          # (cy, cx)
    size = np.asarray(box_wh, dtype=np.float64)[..., ::-1]            # (h, w)
    if letterbox_image:
        # the image occupies a centred `inner` window of the network input: map window coordinates to [0, 1]
        inner = np.round(img_hw * (net_hw / img_hw).min())
        centre = (centre - 0.5 * (net_hw - inner) / net_hw) * (net_hw / inner)
        size = size * (net_hw / inner)
    top_left, bottom_right = centre - 0.5 * size, centre + 0.5 * size
    return np.concatenate([top_left * img_hw, bottom_right * img_hw], axis=-1)


def _nms_workspace(segments, n_max, device):
    return torch.empty(hip.nms_workspace_bytes(segments, n_max), dtype=torch.uint8, device=device)


def non_max_suppression(prediction, num_classes, input_shape, image_shape, letterbox_image, conf_thres=0.5, nms_thres=0.4):
    """utils_bbox.py:86-135 on the (B, A, 5+nc) GPU tensor `decode_outputs` returns.  A list of B float32 numpy arrays
    (N_b, 7): (top, left, bottom, right) in pixels of the original image, obj, class_conf, class_pred, rows in
    descending score = obj * class_conf order (ties: lower anchor first); (0, 7) when no anchor passes conf_thres.
    Only channels 5 .. 5+num_classes-1 are read.  Unlike the reference, `prediction` is left unchanged (it overwrites
    prediction[..., :4] with corner boxes), and boxes of one class are compared as they are rather than after
    batched_nms' per-class coordinate offset (which only perturbs the rounding of the IoU).

    One device -> host read of the B candidate counts sizes the suppression mask from the largest of them (rather than
    from A: 21 504 anchors at 1024 px would need 58 MB per image); the kept rows come back in a second copy."""
    if not (torch.is_tensor(prediction) and prediction.is_cuda and prediction.dim() == 3):
        raise RuntimeError("non_max_suppression: expects the (B, A, 5+nc) GPU tensor of decode_outputs")
    B, A, C = prediction.shape
    if A == 0:
        return [None] * B                    # the reference skips an image without anchors (utils_bbox.py:112-113)
    pred = prediction.detach().float().contiguous()
    dev = pred.device
    rows = torch.empty((B, A, 7), dtype=torch.float32, device=dev)
    scores = torch.empty((B, A), dtype=torch.float32, device=dev)
    cls = torch.empty((B, A), dtype=torch.int64, device=dev)
    ids = torch.empty((B, A), dtype=torch.int32, device=dev)
    counts = torch.empty(B, dtype=torch.int32, device=dev)
    hip.detect_select(pred, num_classes, conf_thres, rows, scores, cls, ids, counts)
    n_max = int(counts.max())
    out = [np.zeros((0, 7), dtype=np.float32) for _ in range(B)]
    if n_max == 0:
        return out
    keep = torch.empty((B, n_max), dtype=torch.int32, device=dev)
    kept = torch.empty(B, dtype=torch.int32, device=dev)
    rows_out = torch.empty((B, n_max, 7), dtype=torch.float32, device=dev)
    hip.nms_segmented(rows, scores, cls, ids, counts, B, A, n_max, nms_thres, _nms_workspace(B, n_max, dev), keep, kept,
                      rows_out)
    kept = kept.cpu().numpy()
    host = rows_out[:, :int(kept.max())].cpu().numpy()
    for b in range(B):
        det = host[b, :kept[b]].copy()
        if len(det):
            box_xy, box_wh = (det[:, 0:2] + det[:, 2:4]) / 2, det[:, 2:4] - det[:, 0:2]
            det[:, :4] = yolo_correct_boxes(box_xy, box_wh, input_shape, image_shape, letterbox_image)
        out[b] = det
    return out


def batched_nms(boxes, scores, idxs, iou_threshold):
    """torchvision.ops.boxes.batched_nms on the GPU: boxes (N, 4) as (x1, y1, x2, y2), scores (N,), idxs (N,) class ids.
    Returns the int64 indices of the kept boxes on the boxes' device, by decreasing score (ties: lower index first).
    Boxes of different classes never suppress each other; boxes and scores are computed in fp32."""
    if not (torch.is_tensor(boxes) and boxes.is_cuda and boxes.dim() == 2 and boxes.shape[1] == 4):
        raise RuntimeError("batched_nms: expects (N, 4) boxes on a GPU")
    n = boxes.shape[0]
    if scores.shape != (n,) or idxs.shape != (n,):
        raise RuntimeError(f"batched_nms: scores / idxs must be ({n},), got {tuple(scores.shape)} / {tuple(idxs.shape)}")
    if n == 0:
        return torch.empty(0, dtype=torch.int64, device=boxes.device)
    dev = boxes.device
    keep = torch.empty(n, dtype=torch.int32, device=dev)
    kept = torch.empty(1, dtype=torch.int32, device=dev)
    hip.nms_segmented(boxes.detach().float().contiguous(), scores.detach().float().contiguous(),
                      idxs.detach().to(dev, torch.int64).contiguous(), None, None, 1, n, n, iou_threshold,
                      _nms_workspace(1, n, dev), keep, kept)
    return keep[:int(kept)].long()


def seg_window(input_shape, image_shape):
    """The letterbox window (top, left, nh, nw) that utils_seg/utils.py:19-31 `resize_image` pastes an image of
    image_shape = (ih, iw) into, in a network input of input_shape = (H, W).  nw / nh truncate (int(), not the np.round of
    yolo_correct_boxes: the reference's two letterboxes differ)."""
    H, W = int(input_shape[0]), int(input_shape[1])
    ih, iw = int(image_shape[0]), int(image_shape[1])
    scale = min(W / iw, H / ih)
    nw, nh = int(iw * scale), int(ih * scale)
    return (H - nh) // 2, (W - nw) // 2, nh, nw


def seg_predict(outputs_seg, input_shape, image_shape=None, geom=None, capacity=None, flag=None, fn="seg_predict"):
    """get_miou_png / detect_image (utils_seg/callbacks.py:140-157, deeplab.py:141-167) for a batch of images of one
    original size: outputs_seg (B, C, H, W) seg logits of a letterboxed input of input_shape = (H, W), image_shape =
    (ih, iw).  Returns the (B, ih, iw) uint8 class map on the logits' device: per output pixel the arg-max over classes of
    the OpenCV INTER_LINEAR resize of the letterbox window's softmax (softmax, crop, resize, arg-max: the reference's
    order), equal values going to the lower class as numpy argmax.  No host synchronisation; fp16 / bf16 logits are
    computed in fp32.
    geom: the (B, hip.GEOM_BYTES) device table of `data.frame_geometry` for a batch of images of their own sizes
    (vrnet_seg_predict_ragged_f32), with capacity = (ihm, iwm) in place of image_shape.  The class map is then the padded
    (B, ihm, iwm): image b is `[b, :ih_b, :iw_b]`, equal to the call without a table on that image alone, and every pixel
    outside it is 0.  flag: an int32 device word for hip.FLAG_GEOMETRY, or None."""
    table = hip._table_call(fn, geom, (("image_shape", image_shape, None),), (("capacity", capacity, None),))
    if not (torch.is_tensor(outputs_seg) and outputs_seg.dim() == 4):
        raise RuntimeError(f"{fn}: expects (B, C, H, W) seg logits")
    B, C, H, W = outputs_seg.shape
    if not 0 < C <= SEG_MAX_CLASSES:
        raise RuntimeError(f"{fn}: {C} classes (1..{SEG_MAX_CLASSES} supported)")
    if input_shape is not None and (H, W) != (int(input_shape[0]), int(input_shape[1])):
        raise RuntimeError(f"{fn}: logits are {H} x {W}, input_shape is {tuple(input_shape)}")
    if table:
        oh, ow = int(capacity[0]), int(capacity[1])
        if not outputs_seg.is_cuda:
            raise RuntimeError(f"{fn}: the logits must be on a GPU (there is no CPU fallback)")
        if oh <= 0 or ow <= 0 or B == 0:
            raise RuntimeError(f"{fn}: bad capacity {tuple(capacity)} or an empty batch")
    else:
        oh, ow = int(image_shape[0]), int(image_shape[1])
        if oh <= 0 or ow <= 0:
            raise RuntimeError(f"{fn}: bad image_shape {tuple(image_shape)}")
        top, left, nh, nw = seg_window(input_shape, image_shape)
        if nh <= 0 or nw <= 0:
            raise RuntimeError(f"{fn}: image {oh} x {ow} leaves an empty window in {H} x {W}")
        if not outputs_seg.is_cuda:
            raise RuntimeError(f"{fn}: the logits must be on a GPU (there is no CPU fallback)")
    x = outputs_seg.detach()
    x = x if (x.is_contiguous() and x.dtype == torch.float32) else x.contiguous().float()
    with torch.cuda.device(x.device):
        out = torch.empty((B, oh, ow), dtype=torch.uint8, device=x.device)
        if table:
            ws = torch.empty(hip.seg_predict_ragged_workspace_bytes(B, C, H, W), dtype=torch.uint8, device=x.device)
            hip.seg_predict(x, None, None, None, None, out, ws, geom=geom, flag=flag, fn=fn)
        elif B:
            ws = torch.empty(hip.seg_predict_workspace_bytes(B, C, nh, nw), dtype=torch.uint8, device=x.device)
            hip.seg_predict(x, top, left, nh, nw, out, ws)
    return out


def seg_predict_ragged(outputs_seg, geom, capacity, flag=None):
    """`seg_predict` with a geometry table, under its earlier name."""
    return seg_predict(outputs_seg, None, None, geom, capacity, flag, "seg_predict_ragged")
