"""A validation pass as graph replays and ONE read-back: the two EvalCallbacks of the reference (detection,
utils/callbacks.py:114-248; segmentation, utils_seg/callbacks.py:113-192 with utils_seg/utils_metrics.py:47-133) run the
network twice per validation image at batch 1, write a text file and a PNG per image and read them back in `get_map` and
`compute_mIoU`.  `EvalPipeline` runs `infer.FramePipeline`'s chain once per batch -- one forward serves both metrics --
and appends to buffers on the device: the rows `get_map_txt` would write go into a record arena (csrc/evalacc.hip), the
class map into the confusion matrix (`metrics.fast_hist(..., out=hist)`).  `compute()` reads back once and returns the
`metrics.voc_map` result next to the per-class IoU / recall / precision, the accuracy and the mIoU.

The arena (N = capacity images): det_label (N, max_boxes) int32, det_score (N, max_boxes) float64, det_box (N, max_boxes, 4)
float64 = left, top, right, bottom, det_count (N) int32, gt_label (N, max_gt) int32, gt_box (N, max_gt, 4) float64, gt_n (N)
int32, and a device cursor = images appended so far.  Image slots are filled in the order of the `add` calls; `compute`
renumbers them by sorted image id, the order in which the reference reads its files.

The score of a detection is the one `metrics.format_detections` computes, float(str(np.float32(obj * class_conf))[:6]),
restated without printing (`score6`); the rule holds for 1e-4 <= score <= 1 (below 1e-4 numpy prints in scientific
notation), which is why conf_thres >= 1e-4 is required.

Tie rule: among equal float32 scores of one image the reference's `np.argsort(...)[::-1]` order is unspecified (its sort
is not stable); here the order is the pipeline's, score descending then anchor index ascending.

Flag bits, beside those of `infer` (FLAG_CANDIDATES matters here: a capped candidate set changes the mAP, so `compute`
raises on any bit unless strict=False): FLAG_EVAL_CAPACITY -- an append found no room and wrote nothing; FLAG_EVAL_GT -- an
image had more ground truths than max_gt; FLAG_EVAL_BOX -- a coordinate or class that int() cannot take (non-finite, or
outside int32), written as 0."""
import os

import numpy as np
import torch

from . import data, infer

FLAG_EVAL_CAPACITY, FLAG_EVAL_GT, FLAG_EVAL_BOX = 32, 64, 128     # EVAL_FLAG_* of csrc/evalacc.hip, above infer.FLAG_*
MIN_CONF = 1e-4
_FLAG_NAMES = {1: "render.FLAG_CLASS", 2: "render.FLAG_BOX_COLOUR", 4: "render.FLAG_BOX_ROWS", 8: "FLAG_CANDIDATES",
               16: "FLAG_DET_CLASS", 32: "FLAG_EVAL_CAPACITY", 64: "FLAG_EVAL_GT", 128: "FLAG_EVAL_BOX", 8192: "FLAG_DEHAZE",
               16384: "FLAG_ACE"}


def score6(x):
    """float(str(np.float32(x))[:6]) for 1e-4 <= x <= 1, elementwise, as float64 (host only; the device restates it in
    csrc/evalacc.hip).  s = float32(x); y = float64(s) * 1e4 is exact (24 x 14 bits); q = rint(y) / 1e4; if q rounds to s
    as a float32, the shortest representation of s has at most four decimals and is q; otherwise the six characters cut
    the digits after the fourth decimal: floor(y) / 1e4."""
    s = np.asarray(x, dtype=np.float32)
    y = s.astype(np.float64) * 1e4
    q = np.rint(y) / 1e4
    return np.where(q.astype(np.float32) == s, q, np.floor(y) / 1e4)


def new_arena(capacity, max_boxes, max_gt, device):
    """The zeroed record arena of the module docstring, as a dict of device tensors."""
    i32, f64 = dict(dtype=torch.int32, device=device), dict(dtype=torch.float64, device=device)
    return dict(det_label=torch.zeros((capacity, max_boxes), **i32), det_score=torch.zeros((capacity, max_boxes), **f64),
                det_box=torch.zeros((capacity, max_boxes, 4), **f64), det_count=torch.zeros(capacity, **i32),
                gt_label=torch.zeros((capacity, max_gt), **i32), gt_box=torch.zeros((capacity, max_gt, 4), **f64),
                gt_n=torch.zeros(capacity, **i32))


def format_detections_device(rows, kept, max_boxes=100):
    """`metrics.format_detections` for one batch on the device, without a pipeline: rows (B, cap, 7) float32 in descending
    score order and kept (B) int32, as `FrameResult.rows` / `FrameResult.kept` -> (label (B, max_boxes) int32, score
    (B, max_boxes) float64, box (B, max_boxes, 4) float64 = left, top, right, bottom, count (B) int32) on the rows' device;
    image b holds count[b] = min(kept[b], max_boxes) entries, the rest is zero.  No host synchronisation.  A coordinate
    that int() cannot take is written as 0; `hip.eval_append` reports it in its flag word."""
    from . import hip
    if not (torch.is_tensor(rows) and rows.is_cuda and rows.dim() == 3 and rows.shape[-1] == 7 and int(max_boxes) >= 1):
        raise RuntimeError("format_detections_device: expects (B, cap, 7) rows on a GPU (there is no CPU fallback) and max_boxes >= 1")
    dev, B = rows.device, rows.shape[0]
    i32 = dict(dtype=torch.int32, device=dev)
    arena = new_arena(B, int(max_boxes), 1, dev)
    with torch.cuda.device(dev):
        hip.eval_append(rows.detach().float().contiguous(), kept.to(dev, torch.int32).contiguous(), torch.zeros((B, 1, 5), **i32),
                        torch.zeros(B, **i32), torch.zeros(1, **i32), arena, torch.zeros(1, **i32))
    return arena["det_label"], arena["det_score"], arena["det_box"], arena["det_count"]


def validate_eval_config(class_names, num_seg_classes, batch, capacity, max_boxes, max_gt, conf_thres):
    """The constructor's own checks, which need no device; returns (class_names, num_seg_classes, capacity, max_boxes,
    max_gt) with capacity=None resolved to the multiple of `batch` at or above 4096."""
    names = list(class_names)
    if not names:
        raise RuntimeError("EvalPipeline: class_names is empty")
    if not float(conf_thres) >= MIN_CONF:
        raise RuntimeError(f"EvalPipeline: conf_thres must be >= {MIN_CONF} (below it numpy prints a score in scientific "
                           f"notation and the six-character rule no longer holds), got {conf_thres!r}")
    batch = int(batch)
    capacity = -(-4096 // batch) * batch if capacity is None else capacity
    for name, v in (("max_boxes", max_boxes), ("max_gt", max_gt), ("capacity", capacity)):
        if isinstance(v, bool) or int(v) != v or int(v) < 1:
            raise RuntimeError(f"EvalPipeline: {name} must be an integer >= 1, got {v!r}")
    if int(capacity) % batch:
        raise RuntimeError(f"EvalPipeline: capacity ({capacity}) must be a multiple of batch ({batch}): every add appends "
                           "exactly `batch` images")
    return names, int(num_seg_classes), int(capacity), int(max_boxes), int(max_gt)


def validate_add(image_ids, seen, label_maps, gt_boxes, batch, frame_shape, num_classes, max_gt, sizes=None):
    """The host checks of `EvalPipeline.add` beside `infer.validate_inputs`: B distinct new ids, label maps (B, ih, iw)
    uint8, B integer (n, 5) ground-truth arrays with n <= max_gt and classes in [0, num_classes).  Returns (ids, labels as a
    tensor, the ground truths packed as one int32 array: (B, max_gt, 5) rows x1, y1, x2, y2, class, then the B counts).
    sizes (B, 2), from a ragged pipeline: the label maps come as the frames do (`data.ragged_items`: a list of maps of
    their images' sizes, or a padded buffer) and are returned in that form."""
    if isinstance(image_ids, str) or len(image_ids) != batch:
        raise RuntimeError(f"EvalPipeline: add takes exactly batch = {batch} image ids, got {image_ids!r}")
    ids = [str(i) for i in image_ids]
    for k, i in enumerate(ids):
        if i in seen or i in ids[:k]:
            raise RuntimeError(f"EvalPipeline: image {i!r} was added twice")
    if sizes is not None:
        lab = data.ragged_items(label_maps, sizes, batch, (), "label maps", "EvalPipeline")[0]
    else:
        lab = label_maps if torch.is_tensor(label_maps) else torch.from_numpy(np.ascontiguousarray(label_maps))
        if lab.dtype != torch.uint8:
            raise RuntimeError(f"EvalPipeline: expected uint8 label maps, got {lab.dtype}")
        lab = lab[None] if batch == 1 and lab.dim() == 2 else lab
        if tuple(lab.shape) != (batch,) + tuple(frame_shape):
            raise RuntimeError(f"EvalPipeline: built for label maps of shape {(batch,) + tuple(frame_shape)} (the frames' size), "
                               f"got {tuple(lab.shape)}")
    if len(gt_boxes) != batch:
        raise RuntimeError(f"EvalPipeline: add takes exactly batch = {batch} ground-truth arrays, got {len(gt_boxes)}")
    packed = np.zeros(batch * max_gt * 5 + batch, dtype=np.int32)
    rows = packed[:batch * max_gt * 5].reshape(batch, max_gt, 5)
    for b, g in enumerate(gt_boxes):
        g = np.asarray(g.detach().cpu() if torch.is_tensor(g) else g)
        if g.size and not np.issubdtype(g.dtype, np.integer):
            raise RuntimeError(f"EvalPipeline: ground truths are integer (n, 5) arrays (data.parse_annotation_line), got {g.dtype}")
        g = g.reshape(-1, 5).astype(np.int64)
        if len(g) > max_gt:
            raise RuntimeError(f"EvalPipeline: image {ids[b]!r} has {len(g)} ground truths, max_gt is {max_gt}")
        if len(g) and (g[:, 4].min() < 0 or g[:, 4].max() >= num_classes):
            raise RuntimeError(f"EvalPipeline: image {ids[b]!r} has a ground-truth class outside [0, {num_classes})")
        if len(g) and np.abs(g).max() >= 2 ** 31:
            raise RuntimeError(f"EvalPipeline: image {ids[b]!r} has a ground-truth coordinate outside int32")
        rows[b, :len(g)] = g
        packed[batch * max_gt * 5 + b] = len(g)
    return ids, lab, packed


class EvalResult:
    """What `EvalPipeline.compute` returns.  det: the `metrics.DetMapResult` of the detections (device tensors: map, ap, f1,
    recall, precision, lamr, n_gt, n_det, n_tp); coco: the `metrics.CocoMapResult` of the same detections with
    compute(coco=True), else None; hist (n, n) int64, rows = labels, columns = predictions; iou, pa_recall,
    precision (n,) float64 and accuracy, miou floats: per_class_iu, per_class_PA_Recall, per_class_Precision, per_Accuracy
    and nanmean(iou) of utils_seg/utils_metrics.py:47-60,131 on that matrix (numpy, on the host); flag: the int word of
    the module docstring; images: the number of images evaluated."""

    def __init__(self, **kw):
        self.__dict__.update(kw)


class EvalPipeline(infer.FramePipeline):
    """add(image_ids, frames_u8, radar, label_maps, gt_boxes) per batch of validation images, compute() once at the end.

    model, frame_shape, input_shape, batch, nms_thres, letterbox_image, max_candidates, normalise_radar, graph: as
    `infer.FramePipeline`, whose chain runs here with render=False; the defaults conf_thres 0.05, nms_thres 0.5,
    max_boxes 100 are EvalCallback's (utils/callbacks.py:84-86), and the radar maps are fed raw, as both callbacks do.
    class_names: the detection classes (ground-truth class ids index it); num_seg_classes: the size of the confusion
    matrix.  capacity: images the arena holds, a multiple of batch (None: the multiple at or above 4096); max_boxes:
    detections kept per image, the best-scored first; max_gt: ground truths per image.  conf_thres >= 1e-4.

    The tail of the chain -- `hip.eval_append` of the kept rows and the static `gt` / `gt_count`, then
    `metrics.fast_hist(labels_u8, class_map, num_seg_classes, out=hist)` -- is part of the ONE captured graph (graph=True).
    Static inputs beside frames_u8 / radar: labels_u8 (B, ih, iw) uint8, the ground-truth class maps at frame size (255
    "void" and values >= num_seg_classes are skipped, as the reference does); gt (B, max_gt, 5) int32 rows x1, y1, x2, y2,
    class and gt_count (B) int32.  The constructor's warm-up passes leave cursor, arena, hist and the model's buffers as
    they were.

    `add` takes exactly `batch` images: for a validation set whose length is no multiple of batch, evaluate the rest with
    a second pipeline of batch 1 (or build this one with batch=1).

    ragged=True (with max_taps, as `infer.FramePipeline`): frame_shape is the capacity, every image has its own size, and
    `add` takes frames and label maps as lists of arrays (or padded buffers with sizes).  labels_u8 is filled with 255
    outside each image, which the confusion matrix skips, so only an image's own pixels are counted.

    radar_points / radar_radius / radar_min_depth / calib: as `infer.FramePipeline`; `add` then takes radar points.
    crops: forwarded to `infer.FramePipeline` (the crops of the last batch are `self.result.crops`); nothing here reads them.
    dehaze: forwarded to `infer.FramePipeline`: the validation pass then scores the network on the dehazed frames.
    ace: forwarded likewise: the validation pass scores the network on the ACE-enhanced frames."""

    def __init__(self, model, frame_shape, input_shape, class_names, num_seg_classes, batch=1, capacity=None, max_boxes=100,
                 max_gt=64, conf_thres=0.05, nms_thres=0.5, letterbox_image=True, max_candidates=1024, normalise_radar=False,
                 graph=True, ragged=False, max_taps=None, radar_points=None, radar_radius=0, radar_min_depth=0.1, calib=None,
                 crops=None, dehaze=None, ace=None):
        infer.validate_config(model, frame_shape, input_shape, batch, max_candidates)
        self.class_names, self.num_seg_classes, self.capacity, self.max_boxes, self.max_gt = validate_eval_config(
            class_names, num_seg_classes, batch, capacity, max_boxes, max_gt, conf_thres)
        if len(self.class_names) != int(model.num_classes):
            raise RuntimeError(f"EvalPipeline: {len(self.class_names)} class names for a model of {int(model.num_classes)} classes")
        p = next(model.parameters(), None)
        if p is None or not p.is_cuda:
            raise RuntimeError("EvalPipeline: the model must be on a HIP device (there is no CPU fallback)")
        dev, B = p.device, int(batch)
        i32 = dict(dtype=torch.int32, device=dev)
        self.image_ids = []
        self.labels_u8 = torch.zeros((B,) + tuple(int(v) for v in frame_shape), dtype=torch.uint8, device=dev)
        self._gt_packed = torch.zeros(B * self.max_gt * 5 + B, **i32)              # one copy per add fills both views
        self.gt = self._gt_packed[:B * self.max_gt * 5].view(B, self.max_gt, 5)
        self.gt_count = self._gt_packed[B * self.max_gt * 5:]
        self.cursor, self.eval_flag = torch.zeros(1, **i32), torch.zeros(1, **i32)
        self.arena = new_arena(self.capacity, self.max_boxes, self.max_gt, dev)
        self.hist = torch.zeros((self.num_seg_classes, self.num_seg_classes), dtype=torch.int64, device=dev)
        super().__init__(model, frame_shape, input_shape, batch=batch, conf_thres=conf_thres, nms_thres=nms_thres,
                         letterbox_image=letterbox_image, max_candidates=max_candidates, normalise_radar=normalise_radar,
                         render=False, graph=graph, ragged=ragged, max_taps=max_taps, radar_points=radar_points,
                         radar_radius=radar_radius, radar_min_depth=radar_min_depth, calib=calib, crops=crops,
                         dehaze=dehaze, ace=ace)

    def _tail(self, result):
        from . import hip, metrics
        hip.eval_append(result.rows, result.kept, self.gt, self.gt_count, self.cursor, self.arena, self.eval_flag)
        self.eval_flag.bitwise_or_(result.flag)         # `flag` is zeroed by every run; the pass accumulates its bits here
        metrics.fast_hist(self.labels_u8, result.class_map, self.num_seg_classes, out=self.hist)

    def _warm_up(self, passes, stream=None):
        super()._warm_up(passes, stream)
        with torch.cuda.device(self.device):            # the zero-input passes appended `passes` batches: undo them
            for t in self.arena.values():
                t.zero_()
            self.reset()
            torch.cuda.synchronize(self.device)

    def reset(self):
        """Forgets every image added: zeroes cursor, det_count, gt_n, hist, flag and the id list."""
        for t in (self.cursor, self.arena["det_count"], self.arena["gt_n"], self.hist, self.eval_flag):
            t.zero_()
        self.image_ids = []

    def add(self, image_ids, frames_u8, radar, label_maps, gt_boxes, sizes=None, calib=None):
        """One batch: image_ids, a list of B strings (a duplicate raises); frames_u8 (B, ih, iw, 3) uint8 RGB and radar
        (B, 4, H, W), as `FramePipeline.run`; label_maps (B, ih, iw) uint8; gt_boxes, a list of B integer (n, 5) arrays x1,
        y1, x2, y2, class as `data.parse_annotation_line` returns.  Validates on the host, copies into the static buffers
        (non_blocking) and replays the graph (graph=False: runs the chain); no host synchronisation.  Returns the
        `infer.FrameResult` of the batch.  A ragged pipeline takes frames_u8 and label_maps as `FramePipeline.run` takes its
        frames (lists of arrays of their own sizes, or padded buffers with sizes).  A pipeline built with radar_points takes
        radar POINTS and calib as `FramePipeline.run` does."""
        table = None
        if calib is not None and self.radar_points is None:
            raise RuntimeError("EvalPipeline: calib belongs to a pipeline built with radar_points")
        if self.ragged:
            f, r, sizes, table = infer.validate_ragged_inputs(frames_u8, radar, sizes, self.batch, self.frame_shape,
                                                              self.input_shape, self.letterbox_image, self.max_taps,
                                                              self.radar_points, calib)
        else:
            if sizes is not None:
                raise RuntimeError("EvalPipeline: sizes belong to a ragged pipeline (ragged=True)")
            f, r = infer.validate_inputs(frames_u8, radar, self.batch, self.frame_shape, self.input_shape, self.radar_points,
                                         calib, self.letterbox_image)
        ids, labels, packed = validate_add(image_ids, set(self.image_ids), label_maps, gt_boxes, self.batch, self.frame_shape,
                                           len(self.class_names), self.max_gt, sizes)
        if len(self.image_ids) + self.batch > self.capacity:
            raise RuntimeError(f"EvalPipeline: the arena holds {self.capacity} images and is full (capacity=...)")
        with torch.cuda.device(self.device):
            if self.ragged:
                self.labels_u8.fill_(255)
                data.fill_slots(self.labels_u8, labels, sizes, corners_only=True)     # a padded buffer's own padding stays out
            else:
                self.labels_u8.copy_(labels, non_blocking=True)
            self._gt_packed.copy_(torch.from_numpy(packed), non_blocking=True)
        result = self._launch(f, r, sizes, table)
        self.image_ids.extend(ids)
        return result

    def compute(self, min_overlap=0.5, score_threhold=0.5, strict=True, coco=False):
        """The one read-back of a validation pass (`voc_map` then makes its own range check) -> `EvalResult`.  strict: raise
        if any flag bit is set -- FLAG_CANDIDATES included, since a capped candidate set changes the mAP; strict=False
        returns the result with the bits in `flag`.  coco=True: `coco` of the result is the `metrics.CocoMapResult` of the
        same arrays (no ground truth is a crowd, annotation ids from 1), at the price of `coco_map`'s own range check.  May
        be called repeatedly: the same bits every time."""
        from . import metrics
        n, N, dev = self.num_seg_classes, len(self.image_ids), self.device
        with torch.cuda.device(dev), torch.no_grad():
            hist = self.hist
            diag = torch.diagonal(hist)
            # utils_metrics.py:47-60, integer sums first, one fp64 division each
            per_class = torch.stack([
                diag.double() / torch.clamp(hist.sum(1) + hist.sum(0) - diag, min=1).double(),
                diag.double() / torch.clamp(hist.sum(1), min=1).double(),
                diag.double() / torch.clamp(hist.sum(0), min=1).double()])
            accuracy = diag.sum().double() / torch.clamp(hist.sum(), min=1).double()
            words = torch.cat([self.eval_flag, self.cursor]).view(torch.float64)
            host = torch.cat([hist.reshape(-1).view(torch.float64), per_class.reshape(-1), accuracy.reshape(1), words]).cpu().numpy()
        flag, cursor = (int(v) for v in host[-1:].view(np.int32))
        if cursor != N:
            raise RuntimeError(f"EvalPipeline: {N} images were added but the device cursor is {cursor} (flag {flag})")
        if flag and strict:
            bits = ", ".join(name for bit, name in _FLAG_NAMES.items() if flag & bit)
            raise RuntimeError(f"EvalPipeline: flag {flag} ({bits}) is set; the numbers would differ from the reference's "
                               "(strict=False returns them all the same)")
        iou, pa_recall, precision = host[n * n:n * n + 3 * n].reshape(3, n).copy()
        a = self.arena
        with torch.cuda.device(dev), torch.no_grad():
            # image slots in sorted-id order (a gather: the order inside an image stays), then the valid entries of each
            perm = torch.tensor(sorted(range(N), key=self.image_ids.__getitem__), dtype=torch.int64, device=dev)
            image = torch.arange(N, device=dev)[:, None]
            dmask = torch.arange(self.max_boxes, device=dev)[None, :] < a["det_count"][perm][:, None]
            gmask = torch.arange(self.max_gt, device=dev)[None, :] < a["gt_n"][perm][:, None]
            arrays = (image.expand(N, self.max_boxes)[dmask], a["det_label"][perm][dmask], a["det_score"][perm][dmask],
                      a["det_box"][perm][dmask], image.expand(N, self.max_gt)[gmask], a["gt_label"][perm][gmask],
                      a["gt_box"][perm][gmask])
            det = metrics.voc_map(*arrays, num_classes=len(self.class_names), min_overlap=min_overlap,
                                  score_threhold=score_threhold, device=dev)
            coco_res = metrics.coco_map(*arrays, num_classes=len(self.class_names), device=dev) if coco else None
        return EvalResult(det=det, coco=coco_res, hist=host[:n * n].view(np.int64).reshape(n, n).copy(), iou=iou, pa_recall=pa_recall,
                          precision=precision, accuracy=float(host[n * n + 3 * n]), miou=float(np.nanmean(iou)), flag=flag,
                          images=N)


def cvt_color(image):
    """utils/utils.py `cvtColor`: an RGB image as it is, every other mode converted to RGB."""
    return image if len(np.shape(image)) == 3 and np.shape(image)[2] == 3 else image.convert("RGB")


def load_line(line, radar_root, seg_root):
    """What both `on_epoch_end`s read for one annotation line -> (image id, frame (ih, iw, 3) uint8, radar (4, H, W) float32,
    label map (ih, iw) uint8, ground truths (n, 5)).  The image id is os.path.basename(path).split('.')[0]
    (utils/callbacks.py:199); the radar file radar_root/<frame id>.npz and the label map seg_root/SegmentationClass/<frame
    id>.png are named by `data.frame_id`."""
    from PIL import Image
    path, boxes = data.parse_annotation_line(line)
    fid = data.frame_id(line)
    frame = np.array(cvt_color(Image.open(path)), dtype=np.uint8)
    label = np.array(Image.open(os.path.join(seg_root, "SegmentationClass", fid + ".png")))
    radar = np.asarray(data.load_radar(radar_root, fid), dtype=np.float32)
    return os.path.basename(path).split('.')[0], frame, radar, label, boxes


def evaluate_lines(pipeline, val_lines, radar_root, seg_root, batch_loader=None):
    """The host loop of the two `on_epoch_end`s (utils/callbacks.py:185-226, utils_seg/callbacks.py:172-193) in one place:
    resets `pipeline`, adds the annotation lines `val_lines` in batches of pipeline.batch and returns pipeline.compute().
    batch_loader(line, radar_root, seg_root) -> (image id, frame, radar, label map, ground truths), default `load_line`.
    len(val_lines) must be a multiple of pipeline.batch (see `EvalPipeline`); a frame or label map whose size differs from
    the pipeline's raises with the file's name.  A ragged pipeline accepts mixed sizes up to its capacity (a label map
    must still have its frame's size)."""
    load = load_line if batch_loader is None else batch_loader
    lines = [l for l in val_lines if l.strip()]
    B, (ih, iw) = pipeline.batch, pipeline.frame_shape
    if len(lines) % B:
        raise RuntimeError(f"evaluate_lines: {len(lines)} lines are no multiple of the pipeline's batch {B}: evaluate the rest "
                           "with a pipeline of batch 1")
    pipeline.reset()
    for k in range(0, len(lines), B):
        items = [load(l, radar_root, seg_root) for l in lines[k:k + B]]
        if getattr(pipeline, "ragged", False):
            for l, (_, frame, _, label, _) in zip(lines[k:k + B], items):
                if np.ndim(frame) != 3 or tuple(np.shape(label)) != tuple(np.shape(frame)[:2]) or np.asarray(label).dtype != np.uint8:
                    raise RuntimeError(f"evaluate_lines: {l.split()[0]}: frame {tuple(np.shape(frame))}, but its label map is "
                                       f"{tuple(np.shape(label))} {np.asarray(label).dtype} (a uint8 map of the frame's size is needed)")
            pipeline.add([i[0] for i in items], [np.asarray(i[1], dtype=np.uint8) for i in items], np.stack([i[2] for i in items]),
                         [np.asarray(i[3]) for i in items], [i[4] for i in items])
            continue
        for l, (_, frame, _, label, _) in zip(lines[k:k + B], items):
            if tuple(np.shape(frame)) != (ih, iw, 3) or tuple(np.shape(label)) != (ih, iw):
                raise RuntimeError(f"evaluate_lines: {l.split()[0]}: frame {tuple(np.shape(frame))} / label map "
                                   f"{tuple(np.shape(label))}, but the pipeline was built for {ih} x {iw} frames")
        pipeline.add([i[0] for i in items], np.stack([i[1] for i in items]), np.stack([i[2] for i in items]),
                     np.stack([i[3] for i in items]).astype(np.uint8), [i[4] for i in items])
    return pipeline.compute()
