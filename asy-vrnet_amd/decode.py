"""Box decode and NMS of the det maps, mirroring utils/utils_bbox.py: `decode_outputs` runs as one HIP
kernel (no concat / grid / stride tensors); `non_max_suppression` as the HIP select + NMS kernels of csrc/nms.hip, in
place of the torchvision `batched_nms` the reference calls (utils_bbox.py:124); `yolo_correct_boxes` is the reference's
host-side letterbox un-map (numpy, on the handful of boxes that survive NMS).  `seg_predict` is the class map of the seg
logits (utils_seg/callbacks.py:113-160, deeplab.py:141-167) as the two HIP kernels of csrc/segpost.hip.  `seg_regions` is
the step the reference does not take: the connected regions of that class map, linked with the detection rows
(csrc/regions.hip; `seg_regions_host` states the rule in numpy)."""
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


# ---- connected regions of the class map: host statement of csrc/regions.hip --------------------------------------------------
# vrnet_region of include/vrnet_hip.h: one region, 48 bytes = 12 int32 words, the two sums as int64 at bytes 32 and 40
REGION_DTYPE = np.dtype([("cls", "<i4"), ("area", "<i4"), ("left", "<i4"), ("top", "<i4"), ("right", "<i4"), ("bottom", "<i4"),
                         ("first", "<i4"), ("det", "<i4"), ("sum_x", "<i8"), ("sum_y", "<i8")])
assert REGION_DTYPE.itemsize == 48
REGION_HEAD = 4                      # per image, int32: regions, records in the table, pixels kept, pixels dropped by min_area
REGION_MAX_REGIONS, REGION_MAX_CLASSES = 4096, 256
FLAG_REGIONS = 131072                # VR_FLAG_REGIONS of csrc/common.h: more regions than max_regions; labels and head are complete
_REGION_DEFAULTS = dict(connectivity=8, background=0, min_area=1, max_regions=1024, det_to_seg=None)


def check_region_params(spec=True, fn="seg_regions", num_classes=None):
    """The parameters of the region rule from True / None (the defaults) or a dict that overrides some of connectivity = 8 (4
    or 8), background = 0 (the class that is not labelled, -1: none; -1..255), min_area = 1 (>= 1), max_regions = 1024 (the
    records of the table, 1..4096) and det_to_seg = None (one seg class in 0..255 per detection class, 1..256 of them; with
    num_classes exactly that many) -> a dict with all five, det_to_seg as a tuple or None.  Anything else raises RuntimeError
    naming fn."""
    if spec is None or spec is True:
        spec = {}
    if not isinstance(spec, dict):
        raise RuntimeError(f"{fn}: regions is None, True or a dict of parameters, got {type(spec).__name__}")
    unknown = sorted(set(spec) - set(_REGION_DEFAULTS))
    if unknown:
        raise RuntimeError(f"{fn}: unknown region parameters {unknown}; known: {sorted(_REGION_DEFAULTS)}")
    p = dict(_REGION_DEFAULTS, **spec)

    def whole(name, v, lo, hi):
        if isinstance(v, (bool, np.bool_)) or not isinstance(v, (int, np.integer)) or not lo <= int(v) <= hi:
            raise RuntimeError(f"{fn}: {name} must be an integer in [{lo}, {hi}], got {v!r}")
        return int(v)

    if isinstance(p["connectivity"], (bool, np.bool_)) or p["connectivity"] not in (4, 8):
        raise RuntimeError(f"{fn}: connectivity must be 4 or 8, got {p['connectivity']!r}")
    out = dict(connectivity=int(p["connectivity"]), background=whole("background", p["background"], -1, 255),
               min_area=whole("min_area", p["min_area"], 1, 2 ** 31 - 1),
               max_regions=whole("max_regions", p["max_regions"], 1, REGION_MAX_REGIONS), det_to_seg=None)
    if p["det_to_seg"] is not None:
        try:
            gate = tuple(np.asarray(p["det_to_seg"]).tolist()) if np.asarray(p["det_to_seg"]).ndim == 1 else None
        except (TypeError, ValueError):
            gate = None
        want = f"{int(num_classes)}" if num_classes is not None else f"1..{REGION_MAX_CLASSES}"
        if gate is None or not 1 <= len(gate) <= REGION_MAX_CLASSES or (num_classes is not None and len(gate) != int(num_classes)):
            raise RuntimeError(f"{fn}: det_to_seg holds one seg class per detection class ({want} of them), got {p['det_to_seg']!r}")
        out["det_to_seg"] = tuple(whole("det_to_seg", v, 0, 255) for v in gate)
    return out


def _region_runs(cm, connectivity, background):
    """The runs of equal non-background class of every row of cm, in raster order, and the root run of each: (row, x0, x1,
    cls, root) as int64 arrays, x1 exclusive.  Runs of neighbouring rows that touch (8: also at a corner) and share a class
    are united; the root of a set is its first run."""
    ih, iw = cm.shape
    reach = 1 if connectivity == 8 else 0
    rows, x0s, x1s, classes = [], [], [], []
    parent = []

    def find(a):
        while parent[a] != a:
            parent[a] = parent[parent[a]]
            a = parent[a]
        return a

    prev = (np.zeros(0, np.int64),) * 3 + (0,)          # starts, ends, classes of the row above and its first run's number
    for y in range(ih):
        line = cm[y]
        cut = np.flatnonzero(line[1:] != line[:-1]) + 1
        s, e = np.concatenate(([0], cut)), np.concatenate((cut, [iw]))
        c = line[s].astype(np.int64)
        keep = c != background
        s, e, c = s[keep].astype(np.int64), e[keep].astype(np.int64), c[keep]
        base = len(parent)
        parent.extend(range(base, base + len(s)))
        ps, pe, pc, pbase = prev
        if len(s) and len(ps):
            lo = np.searchsorted(pe, s - reach, side="right")       # the first run above that ends behind s - reach
            hi = np.searchsorted(ps, e + reach, side="left")        # the first run above that begins at e + reach or later
            for j in np.flatnonzero(hi > lo).tolist():
                for k in range(int(lo[j]), int(hi[j])):
                    if pc[k] == c[j]:
                        a, b = find(pbase + k), find(base + j)
                        if a != b:
                            parent[max(a, b)] = min(a, b)
        rows.append(np.full(len(s), y, np.int64)); x0s.append(s); x1s.append(e); classes.append(c)
        prev = (s, e, c, base)
    root = np.array([find(a) for a in range(len(parent))], np.int64)
    cat = lambda parts: np.concatenate(parts) if parts else np.zeros(0, np.int64)
    return cat(rows), cat(x0s), cat(x1s), cat(classes), root


def _region_link(boxes, others, gate):
    """The best partner of every box among `others` ((n, 4) int64 left, top, right, bottom each, right and bottom exclusive):
    the largest I / U compared as I1 U2 against I2 U1, I > 0, ties to the lowest index; gate (n, m) bool: the pairs that may
    link.  Returns (n) int64 indices, -1 for none."""
    best = np.full(len(boxes), -1, np.int64)
    for i, (l, t, r, b) in enumerate(boxes.tolist()):
        if r <= l or b <= t or not len(others):
            continue
        w = np.minimum(r, others[:, 2]) - np.maximum(l, others[:, 0])
        h = np.minimum(b, others[:, 3]) - np.maximum(t, others[:, 1])
        ok = (w > 0) & (h > 0) & (others[:, 2] > others[:, 0]) & (others[:, 3] > others[:, 1]) & gate[i]
        inter = np.where(ok, w * h, 0)
        union = (r - l) * (b - t) + (others[:, 2] - others[:, 0]) * (others[:, 3] - others[:, 1]) - inter
        bi, bu = 0, 1
        for k in np.flatnonzero(ok).tolist():
            if best[i] < 0 or int(inter[k]) * bu > bi * int(union[k]):
                best[i], bi, bu = k, int(inter[k]), int(union[k])
    return best


def seg_regions_host(class_map, rows=None, connectivity=8, background=0, min_area=1, max_regions=1024, det_to_seg=None):
    """The connected regions of ONE class map in numpy, the statement the kernels of csrc/regions.hip are tested against.
    class_map (ih, iw) uint8; rows (n, 5) int32 = left, top, right, bottom, class as `render.box_rows` / `detect_finish` leave
    them, None: no boxes.  The rule:
      1. pixels of class `background` are unlabelled; background = -1 labels every class;
      2. a region is a maximal set of pixels of one class connected under `connectivity`, 4 or 8;
      3. a region of fewer than min_area pixels is dropped, its pixels get label 0;
      4. the remaining n regions get the ids 1..n in the order of their first pixel in raster order, the smallest y * iw + x;
      5. labels (ih, iw) int32: the id of every kept region, ids beyond max_regions included;
      6. table (max_regions) of REGION_DTYPE: the records of the ids 1..min(n, max_regions), zeros behind -- cls, area, the
         bounding box left, top, right, bottom (right and bottom exclusive), first = y * iw + x of the first pixel, det, and
         the exact integer sums sum_x, sum_y of the pixel coordinates; n > max_regions gives FLAG_REGIONS;
      7. head (4) int32 = n, min(n, max_regions), the pixels in kept regions, the non-background pixels dropped by min_area;
      8. the link, over the records of the table: a row is clamped to the image (left and right to [0, iw], top and bottom to
         [0, ih]: nothing changes for the rows `box_rows` makes) and is empty with right <= left or bottom <= top; a row and a
         region's bounding box have the integer intersection I and union U, and the best partner is the one with the largest
         I / U, compared as I1 * U2 against I2 * U1 in int64, I > 0 required, ties to the lowest index.  det of a record: its
         best row or -1; box_regions (n) int32: the id of a row's best region or 0; an empty row links to nothing.  det_to_seg:
         one seg class per detection class -- a row of class c then links only with regions of class det_to_seg[c], regions of
         other classes ignore it, and a class outside the list links to nothing.
    Returns (labels, table, head, box_regions, flag)."""
    fn = "seg_regions_host"
    p = check_region_params(dict(connectivity=connectivity, background=background, min_area=min_area, max_regions=max_regions,
                                 det_to_seg=det_to_seg), fn)
    cm = np.asarray(class_map)
    if cm.dtype != np.uint8 or cm.ndim != 2 or cm.shape[0] < 1 or cm.shape[1] < 1 or cm.size >= 2 ** 31:
        raise RuntimeError(f"{fn}: expected a uint8 class map (ih, iw) of fewer than 2^31 pixels, got {cm.dtype} {cm.shape}")
    rows = np.zeros((0, 5), np.int32) if rows is None else np.asarray(rows)
    if rows.dtype != np.int32 or rows.ndim != 2 or rows.shape[1] != 5:
        raise RuntimeError(f"{fn}: expected int32 rows (n, 5) = left, top, right, bottom, class, got {rows.dtype} {rows.shape}")
    ih, iw = cm.shape
    R = p["max_regions"]
    row, x0, x1, cls, root = _region_runs(cm, p["connectivity"], p["background"])
    length = x1 - x0
    nruns = len(row)
    area = np.bincount(root, weights=None if not nruns else length, minlength=nruns).astype(np.int64)
    is_root = root == np.arange(nruns)
    kept_root = is_root & (area >= p["min_area"])
    ident = np.zeros(nruns, np.int64)
    ident[kept_root] = np.arange(1, int(kept_root.sum()) + 1)      # runs are in raster order: so are the first pixels
    n = int(kept_root.sum())
    run_id = ident[root] if nruns else ident
    labels = np.zeros(ih * iw, np.int32)
    if nruns:
        begin = np.cumsum(length) - length
        pixel = np.repeat(row * iw + x0 - begin, length) + np.arange(int(length.sum()))
        labels[pixel] = np.repeat(run_id, length)
    labels = labels.reshape(ih, iw)
    nrec = min(n, R)
    table = np.zeros(R, REGION_DTYPE)
    if nrec:
        inside = (run_id >= 1) & (run_id <= nrec)
        k = run_id[inside] - 1
        big = np.iinfo(np.int64).max
        left, top = np.full(nrec, big), np.full(nrec, big)
        right, bottom = np.zeros(nrec, np.int64), np.zeros(nrec, np.int64)
        np.minimum.at(left, k, x0[inside]); np.minimum.at(top, k, row[inside])
        np.maximum.at(right, k, x1[inside]); np.maximum.at(bottom, k, row[inside] + 1)
        sum_x, sum_y, count = np.zeros(nrec, np.int64), np.zeros(nrec, np.int64), np.zeros(nrec, np.int64)
        np.add.at(count, k, length[inside])
        np.add.at(sum_x, k, length[inside] * (x0[inside] + x1[inside] - 1) // 2)
        np.add.at(sum_y, k, length[inside] * row[inside])
        heads = np.flatnonzero(kept_root)[:nrec]                    # the root run of id k + 1
        table["cls"][:nrec], table["area"][:nrec] = cls[heads], count
        table["left"][:nrec], table["top"][:nrec], table["right"][:nrec], table["bottom"][:nrec] = left, top, right, bottom
        table["first"][:nrec] = row[heads] * iw + x0[heads]
        table["sum_x"][:nrec], table["sum_y"][:nrec] = sum_x, sum_y
    kept_px = int(area[kept_root].sum())
    head = np.array([n, nrec, kept_px, int(area[is_root].sum()) - kept_px], np.int32)
    boxes = rows[:, :4].astype(np.int64)
    boxes[:, 0::2] = np.clip(boxes[:, 0::2], 0, iw)
    boxes[:, 1::2] = np.clip(boxes[:, 1::2], 0, ih)
    regions = np.stack([table[f][:nrec].astype(np.int64) for f in ("left", "top", "right", "bottom")], axis=1)
    gate = np.ones((len(rows), nrec), bool)
    if p["det_to_seg"] is not None:
        m = np.array(p["det_to_seg"], np.int64)
        c = rows[:, 4].astype(np.int64)
        known = (c >= 0) & (c < len(m))
        want = np.where(known, m[np.clip(c, 0, len(m) - 1)], -1)
        gate = known[:, None] & (want[:, None] == table["cls"][:nrec].astype(np.int64)[None, :])
    table["det"][:nrec] = _region_link(regions, boxes, gate.T)
    box_regions = (_region_link(boxes, regions, gate) + 1).astype(np.int32)
    return labels, table, head, box_regions, FLAG_REGIONS if n > R else 0


def region_text(table_rows):
    """One line per record of a REGION_DTYPE array, `id cls area left top right bottom cx cy det`, the id being the record's
    place + 1 and cx, cy the centroid sum / area with one decimal: what `infer.predict_dir` saves as <stem>_regions.txt."""
    out = []
    for k, r in enumerate(np.asarray(table_rows, REGION_DTYPE).reshape(-1)):
        a = max(int(r["area"]), 1)
        out.append(f"{k + 1} {int(r['cls'])} {int(r['area'])} {int(r['left'])} {int(r['top'])} {int(r['right'])} {int(r['bottom'])} "
                   f"{'{:.1f}'.format(int(r['sum_x']) / a)} {'{:.1f}'.format(int(r['sum_y']) / a)} {int(r['det'])}\n")
    return "".join(out)


def seg_regions(class_map, results=None, connectivity=8, background=0, min_area=1, max_regions=1024, det_to_seg=None, geom=None,
                flag=None, cap=None, device="cuda"):
    """`seg_regions_host` on the device for a batch (vrnet_seg_regions_u8, seven launches, no host synchronisation): class_map
    (B, ih, iw) uint8, numpy or tensor (a single (ih, iw) map counts as B = 1).  results: None (no boxes), the list
    `non_max_suppression` returns -- packed by `render.box_rows` and sent in one pinned non-blocking copy -- or a pair (rows
    (n_cap, 5) int32, offsets (B + 1) int32) of device tensors, as `render.crop_boxes` takes them.  geom: the (B,
    hip.GEOM_BYTES) device table of `data.frame_geometry` for padded ragged maps (image b in the top-left corner of slot b);
    nothing outside an image is labelled or connected.  cap: the rows an image can have, the width of box_regions (default:
    the largest count of the list, or n_cap of a device pair).  flag: a zeroed int32 device tensor of one element (a fresh
    one by default) that receives FLAG_REGIONS and hip.FLAG_GEOMETRY.  Returns (labels (B, ih, iw) int32, table (B,
    max_regions, 12) int32 -- the records of REGION_DTYPE as words --, head (B, 4) int32, box_regions (B, cap) int32, flag),
    per image what the host rule gives, bit for bit."""
    from . import render
    fn = "seg_regions"
    p = check_region_params(dict(connectivity=connectivity, background=background, min_area=min_area, max_regions=max_regions,
                                 det_to_seg=det_to_seg), fn)
    cm = class_map if torch.is_tensor(class_map) else torch.from_numpy(np.ascontiguousarray(class_map))
    cm = cm[None] if cm.dim() == 2 else cm
    if cm.dtype != torch.uint8 or cm.dim() != 3 or min(cm.shape) <= 0:
        raise RuntimeError(f"{fn}: expected a uint8 class map (B, ih, iw) or (ih, iw), got {cm.dtype} {tuple(cm.shape)}")
    B, ih, iw = cm.shape
    host = None
    if results is None:
        host = (np.zeros((0, 5), np.int32), np.zeros(B + 1, np.int32))
    elif isinstance(results, tuple) and len(results) == 2 and all(torch.is_tensor(t) for t in results):
        rows, offsets = results
    else:
        if len(results) != B:
            raise RuntimeError(f"{fn}: {len(results)} result entries for {B} class maps")
        host = render.box_rows(results, (ih, iw), render.MAX_COLORS)[:2]
    cm = cm.to(device, non_blocking=True).contiguous()
    dev = cm.device
    i32 = dict(dtype=torch.int32, device=dev)
    with torch.cuda.device(dev):
        if host is not None:                  # offsets and rows in one pinned buffer; at least one row, so it has an address
            n = max(len(host[0]), 1)
            packed = torch.zeros(B + 1 + 5 * n, dtype=torch.int32).pin_memory()
            packed[:B + 1] = torch.from_numpy(host[1])
            packed[B + 1:B + 1 + host[0].size] = torch.from_numpy(host[0].reshape(-1))
            packed = packed.to(dev, non_blocking=True)
            offsets, rows = packed[:B + 1], packed[B + 1:].view(n, 5)
            width = max(int(np.diff(host[1]).max()), 1)
        else:
            rows, offsets = rows.to(dev).contiguous(), offsets.to(dev).contiguous()
            width = max(rows.shape[0], 1)
        cap = width if cap is None else int(cap)
        if cap < 1:
            raise RuntimeError(f"{fn}: cap must be at least 1, got {cap}")
        if flag is None:
            flag = torch.zeros(1, **i32)
        gate = None if p["det_to_seg"] is None else torch.tensor(p["det_to_seg"], **i32)
        labels = torch.empty((B, ih, iw), **i32)
        table = torch.empty((B, p["max_regions"], hip.REGION_WORDS), **i32)
        head, box_regions = torch.empty((B, REGION_HEAD), **i32), torch.empty((B, cap), **i32)
        ws = torch.empty(hip.seg_regions_workspace_bytes(B, ih, iw), dtype=torch.uint8, device=dev)
        hip.seg_regions(cm, rows, offsets, labels, table, head, box_regions, ws, p["connectivity"], p["background"], p["min_area"],
                        det_to_seg=gate, geom=geom, flag=flag)
    return labels, table, head, box_regions, flag
