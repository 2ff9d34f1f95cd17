"""Segmentation metrics on the device, with the interfaces of utils_seg/utils_metrics.py: `f_score` (:12-31, called on
every training and validation step, utils/utils_fit.py:78,109,177) and `fast_hist` (:35-44, the per-image confusion
matrix of compute_mIoU, :102).  Each is one or two HIP launches with no host synchronisation; the result stays on the
device until the caller reads it.  per_class_iu, per_class_PA_Recall, per_class_Precision and per_Accuracy (:47-60) work
unchanged on `hist.cpu().numpy()`.  No CPU fallback.

The detection metric of utils/utils_map.py (`get_map`, :276-798: VOC AP matching, voc_ap, log-average miss rate) is
`voc_map` on flat arrays, `DetectionEvaluator` for an evaluation loop that feeds it image by image in place of the two
text files per image of utils/callbacks.py:175-248, and `read_map_dir` / `get_map` for directories in the reference's
format.  Matching, flags, curves and AP are HIP kernels (csrc/detmap.hip); the global sort and the grouping of the ground
truths by (image, class) are torch ops on the device.

The COCO numbers the same callback logs where pycocotools is installed (`get_coco_map`, utils_map.py:894-923, called at
utils/callbacks.py:224) are `coco_map` on the same flat arrays, `DetectionEvaluator.compute_coco`, and `get_coco_map` for
directories: COCOeval's bbox evaluation restated in csrc/cocomap.hip, without pycocotools."""
import glob
import os

import numpy as np
import torch

from . import hip

MAX_CLASSES = 32              # the seg loss's class cap (SMAXC in csrc/loss.hip)


def f_score(inputs, target, beta=1, smooth=1e-5, threhold=0.5):
    """utils_metrics.py:12-31 (the keyword keeps the reference's spelling): inputs (B, C, H, W) logits, target (B, H, W,
    C+1) one-hot labels.  Per class c < C over all pixels tp = sum t_c [p_c > threhold], fp, fn as the reference;
    returns the mean over c of ((1+b^2) tp + smooth) / ((1+b^2) tp + b^2 fn + fp + smooth) as a 0-d fp32 tensor on the
    logits' device.  The logits must already be at the target's size: the reference's bilinear resize branch (:15-16)
    never runs on this net, whose seg head outputs full resolution."""
    if not (torch.is_tensor(inputs) and inputs.dim() == 4 and torch.is_tensor(target) and target.dim() == 4):
        raise RuntimeError("f_score: expects (B, C, H, W) logits and a (B, H, W, C+1) one-hot target")
    B, C, H, W = inputs.shape
    if not 0 < C <= MAX_CLASSES:
        raise RuntimeError(f"f_score: {C} classes (1..{MAX_CLASSES} supported)")
    if tuple(target.shape) != (B, H, W, C + 1):
        raise RuntimeError(f"f_score: target must be (B, H, W, C+1) = {(B, H, W, C + 1)} for logits {tuple(inputs.shape)} "
                           "(the reference's resize branch, utils_metrics.py:15-16, never runs on this net)")
    if not inputs.is_cuda:
        raise RuntimeError("f_score: the logits must be on a GPU (there is no CPU fallback)")
    x = inputs.detach()
    x = x if (x.is_contiguous() and x.dtype == torch.float32) else x.contiguous().float()
    t = target.detach().to(x.device, torch.float32).contiguous()
    out = torch.empty(1, dtype=torch.float32, device=x.device)
    hip.seg_fscore(x, t, beta, smooth, threhold, out)
    return out.reshape(())


_LABEL_DTYPES = (torch.uint8, torch.int64)


def fast_hist(a, b, n, out=None):
    """utils_metrics.py:35-44: a = labels, b = predictions, tensors of one number of elements (any shape, uint8 or int64)
    on the GPU.  Returns the (n, n) int64 confusion matrix on that device, rows = labels, columns = predictions; with
    `out` ((n, n) int64, contiguous) the counts are added to it in place and `out` is returned, so a whole validation set
    needs one read-back.  Pairs whose label is outside [0, n) are skipped, as the reference does (255 "void" pixels, the
    ignore class n); so are pairs whose prediction is outside [0, n), which the reference would count in another bin."""
    n = int(n)
    if not 0 < n <= MAX_CLASSES:
        raise RuntimeError(f"fast_hist: n = {n} (1..{MAX_CLASSES} supported)")
    if not (torch.is_tensor(a) and torch.is_tensor(b)):
        raise RuntimeError("fast_hist: expects label and prediction tensors")
    if a.dtype not in _LABEL_DTYPES or b.dtype not in _LABEL_DTYPES:
        raise RuntimeError(f"fast_hist: labels and predictions must be uint8 or int64, got {a.dtype} / {b.dtype}")
    if a.numel() != b.numel():
        raise RuntimeError(f"fast_hist: {a.numel()} labels but {b.numel()} predictions")
    if out is not None and (tuple(out.shape) != (n, n) or out.dtype != torch.int64 or not out.is_contiguous()):
        raise RuntimeError(f"fast_hist: out must be a contiguous ({n}, {n}) int64 tensor")
    if not (a.is_cuda and b.is_cuda and a.device == b.device and (out is None or out.device == a.device)):
        raise RuntimeError("fast_hist: the tensors must be on one GPU (there is no CPU fallback)")
    if out is None:
        out = torch.zeros((n, n), dtype=torch.int64, device=a.device)
    hip.confusion_hist(a.detach().contiguous().reshape(-1), b.detach().contiguous().reshape(-1), n, out)
    return out


# ---- detection mAP (utils/utils_map.py) -------------------------------------------------------------------------------

MAX_THRESHOLDS = 16
MAX_BOXES = 1 << 24           # detections / ground truths of one call (DM_MAX_N in csrc/detmap.hip)
MAX_MAP_CLASSES = 65535
MAX_GROUPS = 1 << 27          # images x classes


class DetMapResult:
    """What `voc_map` returns: device tensors, read back only when the caller asks (`.cpu()`, `.item()`, `float(r.map)`).
    With a scalar min_overlap the shapes are as listed; with a sequence of T thresholds every tensor but `score` and
    `offsets` gains a leading T axis.
      map        ()   mean of `ap` over the classes with a non-difficult ground truth, 0 if there is none
      ap, f1, recall, precision, lamr   (num_classes,) fp64; NaN for a class without a non-difficult ground truth (the
                 reference does not evaluate such a class and it does not enter `map`), 0 for an evaluated class without
                 detections; f1 / recall / precision are read at the last rank whose score >= score_threhold
      n_gt       (num_classes,) int32 non-difficult ground truths;  n_det (num_classes,) int32 detections
      n_tp       (num_classes,) int32 true positives (0 for a class without ground truth, utils_map.py:688-690)
    and, with return_curves=True, flat arrays in rank order (classes ascending, inside a class score descending with ties
    in input order), class c at offsets[c] .. offsets[c + 1] - 1:
      offsets (num_classes + 1,) int32; order (D,) int64 index into the input detections; score (D,) fp64;
      tp, fp (D,) uint8 (both 0: matched to a difficult ground truth); rec, prec (D,) fp64."""

    def __init__(self, **kw):
        self.__dict__.update(kw)

    def keys(self):
        return self.__dict__.keys()

    def __getitem__(self, k):
        return self.__dict__[k]


def _flat(x, dtype, dev, cols=None):
    t = torch.as_tensor(x).detach()
    t = t.reshape(-1, cols) if cols else t.reshape(-1)
    return t.to(dev, dtype).contiguous()


def voc_map(det_image, det_label, det_score, det_box, gt_image, gt_label, gt_box, gt_difficult=None, num_classes=None,
            min_overlap=0.5, score_threhold=0.5, return_curves=False, device="cuda"):
    """utils_map.py:276-798 `get_map` on flat arrays (numpy arrays or tensors, moved to `device`, which must be a GPU: there
    is no CPU fallback).  Detections: det_image (D,) image index, det_label (D,) class id, det_score (D,), det_box (D, 4)
    = left, top, right, bottom; ground truths: gt_image (G,), gt_label (G,), gt_box (G, 4), gt_difficult (G,) or None
    (none difficult).  The input order of the detections is the reference's reading order (images by sorted file name,
    then lines): equal scores keep it.  Image indices are 0 .. n_images - 1 with n_images taken from the data; class ids
    lie in [0, num_classes) (None: the largest id + 1).  D = 0 and G = 0 are valid.  min_overlap: a float, or a sequence
    of up to 16 floats evaluated in the same launches (VOC matching at each; not COCO's interpolated AP).
    score_threhold keeps the reference's spelling.  Returns a `DetMapResult`.  All arithmetic is fp64 in the reference's
    operand order; the result is bitwise the same on every run.  One host synchronisation (the range check)."""
    dev = torch.device(device)
    if dev.type != "cuda":
        raise RuntimeError("voc_map: the device must be a GPU (there is no CPU fallback)")
    single = not isinstance(min_overlap, (list, tuple, np.ndarray, torch.Tensor))
    thr = [float(min_overlap)] if single else [float(v) for v in min_overlap]
    T = len(thr)
    if not 1 <= T <= MAX_THRESHOLDS:
        raise RuntimeError(f"voc_map: {T} thresholds (1..{MAX_THRESHOLDS} supported)")
    d_img, d_lab = _flat(det_image, torch.int64, dev), _flat(det_label, torch.int64, dev)
    d_score = _flat(det_score, torch.float64, dev) + 0.0            # -0.0 -> +0.0: one key for the sort, as float compares
    d_box = _flat(det_box, torch.float64, dev, 4)
    g_img, g_lab = _flat(gt_image, torch.int64, dev), _flat(gt_label, torch.int64, dev)
    g_box = _flat(gt_box, torch.float64, dev, 4)
    D, G = d_score.numel(), g_img.numel()
    g_diff = torch.zeros(G, dtype=torch.uint8, device=dev) if gt_difficult is None else \
        (_flat(gt_difficult, torch.int64, dev) != 0).to(torch.uint8)
    if not (d_img.numel() == d_lab.numel() == d_box.shape[0] == D and g_lab.numel() == g_box.shape[0] == g_diff.numel() == G):
        raise RuntimeError("voc_map: the detection arrays (and the ground-truth arrays) must have one length each")
    if D > MAX_BOXES or G > MAX_BOXES:
        raise RuntimeError(f"voc_map: {D} detections, {G} ground truths (0..{MAX_BOXES} each supported)")
    # ranges, in one read-back: [min image, max image, min label, max label, NaN scores]
    img_all, lab_all = torch.cat([d_img, g_img]), torch.cat([d_lab, g_lab])
    if D + G:
        lo_i, hi_i, lo_l, hi_l, bad = torch.stack([img_all.min(), img_all.max(), lab_all.min(), lab_all.max(),
                                                   torch.isnan(d_score).sum()]).tolist()
    else:
        lo_i, hi_i, lo_l, hi_l, bad = 0, -1, 0, -1, 0
    if bad:
        raise RuntimeError("voc_map: NaN scores cannot be ranked")
    C = hi_l + 1 if num_classes is None else int(num_classes)
    C = max(C, 1) if num_classes is None else C
    n_images = hi_i + 1
    if not 1 <= C <= MAX_MAP_CLASSES:
        raise RuntimeError(f"voc_map: {C} classes (1..{MAX_MAP_CLASSES} supported)")
    if lo_i < 0 or lo_l < 0 or hi_l >= C:
        raise RuntimeError(f"voc_map: image indices must be >= 0 and class ids in [0, {C}) "
                           f"(got images {lo_i}..{hi_i}, classes {lo_l}..{hi_l})")
    if n_images * C > MAX_GROUPS:
        raise RuntimeError(f"voc_map: {n_images} images x {C} classes (at most {MAX_GROUPS} (image, class) pairs supported)")
    # rank order: a stable sort by score descending, then a stable sort by class
    by_score = torch.sort(d_score, descending=True, stable=True).indices
    order = by_score[torch.sort(d_lab[by_score], stable=True).indices]
    det_off = torch.zeros(C + 1, dtype=torch.int32, device=dev)
    det_off[1:] = torch.cumsum(torch.bincount(d_lab, minlength=C), 0)
    # ground truths grouped by (image, class), input order inside a group
    key = g_img * C + g_lab
    gt_perm = torch.sort(key, stable=True).indices.to(torch.int32)
    gt_off = torch.zeros(n_images * C + 1, dtype=torch.int32, device=dev)
    if n_images:
        gt_off[1:] = torch.cumsum(torch.bincount(key, minlength=n_images * C), 0)
    i32, f64 = dict(dtype=torch.int32, device=dev), dict(dtype=torch.float64, device=dev)
    out = {"match": torch.empty(D, **i32), "ovmax": torch.empty(D, **f64),
           "tp": torch.empty((T, D), dtype=torch.uint8, device=dev), "fp": torch.empty((T, D), dtype=torch.uint8, device=dev),
           "rec": torch.empty((T, D), **f64) if return_curves else None,
           "prec": torch.empty((T, D), **f64) if return_curves else None,
           "n_gt": torch.empty(C, **i32), "n_img": torch.empty(C, **i32), "n_tp": torch.empty((T, C), **i32),
           "map": torch.empty(T, **f64)}
    for k in ("ap", "f1", "recall", "precision", "lamr"):
        out[k] = torch.empty((T, C), **f64)
    # (an empty result of an indexing op may carry a zero stride, which hip.ptr refuses: hand over fresh empty tensors)
    arg = lambda t, dt=None: (t.to(dt) if dt else t).contiguous() if t.numel() else \
        torch.empty(t.shape, dtype=dt or t.dtype, device=dev)
    with torch.cuda.device(dev):
        hip.det_map(arg(d_img, torch.int32), arg(d_lab, torch.int32), arg(d_score), arg(d_box), arg(order, torch.int32),
                    det_off, arg(g_box), arg(g_diff), arg(gt_perm), gt_off, n_images, C, thr, score_threhold, out)
    n_gt, n_det = out["n_gt"], det_off[1:] - det_off[:-1]
    res = {k: out[k] for k in ("map", "ap", "f1", "recall", "precision", "lamr", "n_tp")}
    res.update(n_gt=n_gt.expand(T, C), n_det=n_det.expand(T, C))
    if return_curves:
        res.update(order=order.expand(T, D), tp=out["tp"], fp=out["fp"], rec=out["rec"], prec=out["prec"])
    if single:
        res = {k: v[0] for k, v in res.items()}
    if return_curves:
        res.update(score=d_score[order], offsets=det_off)
    return DetMapResult(**res)


def format_detections(nms_rows, max_boxes=100):
    """What utils/callbacks.py:151-170 `get_map_txt` writes for one image and `get_map` parses back, without the file:
    nms_rows (N, 7) = top, left, bottom, right, obj, class_conf, class_pred as `decode.non_max_suppression` returns them.
    Returns (label (n,) int64, score (n,) float64, box (n, 4) float64 = left, top, right, bottom), n = min(N, max_boxes):
    score = obj * class_conf in float32, rows taken by np.argsort(score)[::-1][:max_boxes], the score quantised to
    float(str(score)[:6]) (the six characters the reference writes), coordinates truncated with int()."""
    rows = np.asarray(nms_rows.detach().cpu() if torch.is_tensor(nms_rows) else nms_rows, dtype=np.float32).reshape(-1, 7)
    top_label = np.array(rows[:, 6], dtype="int32")
    top_conf = rows[:, 4] * rows[:, 5]
    top = np.argsort(top_conf)[::-1][:max_boxes]
    label = top_label[top].astype(np.int64)
    score = np.array([float(str(c)[:6]) for c in top_conf[top]], dtype=np.float64)
    box = np.array([[int(l), int(t), int(r), int(b)] for t, l, b, r in rows[top, :4]], dtype=np.float64).reshape(-1, 4)
    return label, score, box


class DetectionEvaluator:
    """The detection half of EvalCallback.on_epoch_end (utils/callbacks.py:175-248) without its text files: `add` per
    validation image in place of the two `open(...).write` blocks, `compute().map` in place of `get_map`.

    add(image_id, nms_rows, gt_boxes): nms_rows = one image's (N, 7) rows from `decode.non_max_suppression` (None or
    empty: no detections), formatted by `format_detections` exactly as get_map_txt writes and get_map parses them (first
    max_boxes rows by score, six-character score, int() coordinates); gt_boxes = the (n, 5) integer array x1, y1, x2, y2,
    cls of `data.parse_annotation_line` (never difficult).  Among equal float32 scores the order is the one
    `non_max_suppression` produced put through np.argsort(...)[::-1]; the reference leaves that tie order unspecified too
    (its argsort is not stable), so which of two equal-score rows survives the max_boxes cut may differ from a given run
    of the reference.  Images are evaluated in sorted image_id order, as the reference's sorted file lists."""

    def __init__(self, class_names, max_boxes=100):
        self.class_names = list(class_names)
        self.max_boxes = int(max_boxes)
        self.reset()

    def reset(self):
        self._images = {}

    def add(self, image_id, nms_rows, gt_boxes):
        image_id = str(image_id)
        if image_id in self._images:
            raise RuntimeError(f"DetectionEvaluator: image {image_id!r} was added twice")
        n = len(self.class_names)
        if nms_rows is None:
            nms_rows = np.zeros((0, 7), dtype=np.float32)
        label, score, box = format_detections(nms_rows, self.max_boxes)
        gt = np.asarray(gt_boxes.detach().cpu() if torch.is_tensor(gt_boxes) else gt_boxes).reshape(-1, 5)
        if not np.issubdtype(gt.dtype, np.integer):
            gt = gt.astype(np.int64)                               # parse_annotation_line: integers
        if (len(label) and (label.min() < 0 or label.max() >= n)) or (len(gt) and (gt[:, 4].min() < 0 or gt[:, 4].max() >= n)):
            raise RuntimeError(f"DetectionEvaluator: class id outside [0, {n})")
        self._images[image_id] = (label, score, box, gt[:, 4].astype(np.int64), gt[:, :4].astype(np.float64))

    def arrays(self):
        """The flat arrays `voc_map` takes, images numbered by sorted image_id."""
        ids = sorted(self._images)
        parts = [self._images[i] for i in ids]
        cat = lambda k, shape, dt: np.concatenate([p[k] for p in parts]) if parts else np.zeros(shape, dtype=dt)
        rep = lambda k: np.concatenate([np.full(len(p[k]), i, dtype=np.int64) for i, p in enumerate(parts)]) \
            if parts else np.zeros(0, dtype=np.int64)
        return dict(det_image=rep(0), det_label=cat(0, 0, np.int64), det_score=cat(1, 0, np.float64),
                    det_box=cat(2, (0, 4), np.float64), gt_image=rep(3), gt_label=cat(3, 0, np.int64),
                    gt_box=cat(4, (0, 4), np.float64))

    def compute(self, min_overlap=0.5, score_threhold=0.5, return_curves=False, device="cuda"):
        """One upload and one `voc_map` call over everything added since the last reset."""
        return voc_map(**self.arrays(), num_classes=len(self.class_names), min_overlap=min_overlap,
                       score_threhold=score_threhold, return_curves=return_curves, device=device)

    def compute_coco(self, device="cuda"):
        """One upload and one `coco_map` call over everything added since the last reset (annotation ids from 1)."""
        return coco_map(**self.arrays(), num_classes=len(self.class_names), device=device)


def _map_line(line, n_numbers):
    tok = line.split()
    return " ".join(tok[:-n_numbers]), [float(v) for v in tok[-n_numbers:]]


def read_map_dir(path):
    """Parses a directory in the reference's format (utils_map.py:310-416) on the host: path/ground-truth/<id>.txt with
    lines `class left top right bottom [difficult]` and path/detection-results/<id>.txt with lines `class confidence left
    top right bottom`; the numbers are the last 4 (5 with a trailing `difficult` token; 5 for a detection) tokens of a
    line, so class names may contain spaces.  Images are numbered by sorted file name, classes by sorted name over both
    directories.  Returns a dict: the arrays `voc_map` takes plus class_names and image_ids.  A detection file without a
    ground-truth file, or the reverse, raises RuntimeError (the reference calls sys.exit there)."""
    gt_files = sorted(glob.glob(os.path.join(path, "ground-truth", "*.txt")))
    dr_files = sorted(glob.glob(os.path.join(path, "detection-results", "*.txt")))
    if not gt_files:
        raise RuntimeError(f"read_map_dir: no ground-truth files under {path}")
    ident = lambda f: os.path.basename(f)[:-len(".txt")]
    ids = [ident(f) for f in gt_files]
    if ids != [ident(f) for f in dr_files]:
        odd = sorted(set(ids) ^ set(ident(f) for f in dr_files))
        raise RuntimeError(f"read_map_dir: ground-truth and detection-results files do not pair up: {odd[:5]}")
    gts, dets = [], []
    for i, (gf, df) in enumerate(zip(gt_files, dr_files)):
        for line in open(gf):
            line = line.strip()
            if not line:
                continue
            diff = line.split()[-1] == "difficult"
            name, box = _map_line(line.rsplit(None, 1)[0] if diff else line, 4)
            gts.append((i, name, box, diff))
        for line in open(df):
            line = line.strip()
            if not line:
                continue
            name, num = _map_line(line, 5)
            dets.append((i, name, num[0], num[1:]))
    names = sorted({g[1] for g in gts} | {d[1] for d in dets})
    cid = {n: k for k, n in enumerate(names)}
    return dict(det_image=np.array([d[0] for d in dets], dtype=np.int64),
                det_label=np.array([cid[d[1]] for d in dets], dtype=np.int64),
                det_score=np.array([d[2] for d in dets], dtype=np.float64),
                det_box=np.array([d[3] for d in dets], dtype=np.float64).reshape(-1, 4),
                gt_image=np.array([g[0] for g in gts], dtype=np.int64),
                gt_label=np.array([cid[g[1]] for g in gts], dtype=np.int64),
                gt_box=np.array([g[2] for g in gts], dtype=np.float64).reshape(-1, 4),
                gt_difficult=np.array([g[3] for g in gts], dtype=np.uint8),
                class_names=names, image_ids=ids)


def get_map(MINOVERLAP, draw_plot, score_threhold=0.5, path='./map_out'):
    """utils_map.py:276-798 with the reference's signature: the VOC mAP at IoU threshold MINOVERLAP of the directory
    `path` (format: `read_map_dir`), as a Python float.  Only the return value is reproduced -- the one thing the training
    loop uses (utils/callbacks.py:226): nothing is written or deleted (no results/ directory, no .temp_files/), nothing
    is printed, and draw_plot=True raises RuntimeError because there are no plots here."""
    if draw_plot:
        raise RuntimeError("get_map: draw_plot is not supported (no plots are produced)")
    data = read_map_dir(path)
    names = data.pop("class_names")
    data.pop("image_ids")
    return float(voc_map(**data, num_classes=len(names), min_overlap=float(MINOVERLAP), score_threhold=score_threhold).map)


# ---- COCO detection metrics (utils/utils_map.py:800-923, COCOeval) ------------------------------------------------------

COCO_IOU_THRS = np.linspace(.5, 0.95, int(np.round((0.95 - .5) / .05)) + 1, endpoint=True)      # cocoeval.py Params.setDetParams
COCO_REC_THRS = np.linspace(.0, 1.00, int(np.round((1.00 - .0) / .01)) + 1, endpoint=True)
COCO_MAX_DETS = (1, 10, 100)
COCO_AREA_RNG = ((0.0, 1e10), (0.0, 1024.0), (1024.0, 9216.0), (9216.0, 1e10))                  # all, small, medium, large
COCO_LDS_BYTES = 65536        # a group's IoUs and state stay in LDS up to here (CM_LDS in csrc/cocomap.hip)
_coco_consts = {}


class CocoMapResult:
    """What `coco_map` returns: device tensors, read back only when the caller asks.  K = num_classes; the axes are
    COCOeval's: T = 10 IoU thresholds, R = 101 recall points, A = 4 area ranges (all, small, medium, large), M = 3 caps on
    the detections per image (1, 10, 100).
      stats      (12,) fp64   COCOeval.stats: AP, AP50, AP75, AP small / medium / large, AR at 1 / 10 / 100 detections, AR
                              small / medium / large; -1 where no class has a ground truth that counts
      precision  (10, 101, K, 4, 3) fp64;  recall (10, K, 4, 3) fp64: -1 for a class without a counted ground truth
      n_gt       (K, 4) int32 ground truths that are neither crowd nor outside the area range
    and, with return_matches=True, in the detections' input order:
      dt_match   (10, 4, D) int32 the input index of the matched ground truth, -1 for none
      dt_ignore  (10, 4, D) uint8 the detection is ignored at that threshold and range
      kept       (D,) uint8       0: cut by the 100 detections per (image, class); such a detection has dt_match -1"""

    def __init__(self, **kw):
        self.__dict__.update(kw)

    def keys(self):
        return self.__dict__.keys()

    def __getitem__(self, k):
        return self.__dict__[k]


def coco_map(det_image, det_label, det_score, det_box, gt_image, gt_label, gt_box, gt_difficult=None, num_classes=None,
             gt_area=None, zero_id_gt=None, return_matches=False, device="cuda"):
    """COCOeval(cocoGt, cocoDt, 'bbox') with evaluate(), accumulate(), summarize() -- what utils_map.py:894-923
    `get_coco_map` runs -- on the flat arrays `voc_map` takes (same conventions and checks: numpy arrays or tensors, moved
    to `device`, which must be a GPU; boxes left, top, right, bottom; D = 0 and G = 0 valid; NaN scores refused).  A box
    becomes x, y, w, h = l, t, r - l, b - t; gt_difficult is COCO's iscrowd (and ignore); gt_area (G,) defaults to the
    reference's w * h - 10.0 (utils_map.py:842).  Images are evaluated in index order, so equal scores order by image
    index and then by input order.  zero_id_gt: the index of the ground truth carrying annotation id 0, which COCOeval
    cannot tell from "unmatched" (the reference numbers from 0, :865); None: ids from 1, the COCO convention.  The
    parameters are COCOeval's defaults and fixed.  Returns a `CocoMapResult`.  All arithmetic is fp64 in COCOeval's
    operand order; the result is bitwise the same on every run.  One read-back (the range check, which also fetches the
    number of (image, class) groups and the workspace size)."""
    dev = torch.device(device)
    if dev.type != "cuda":
        raise RuntimeError("coco_map: the device must be a GPU (there is no CPU fallback)")
    d_img, d_lab = _flat(det_image, torch.int64, dev), _flat(det_label, torch.int64, dev)
    d_score = _flat(det_score, torch.float64, dev) + 0.0
    d_box = _flat(det_box, torch.float64, dev, 4)
    g_img, g_lab = _flat(gt_image, torch.int64, dev), _flat(gt_label, torch.int64, dev)
    g_box = _flat(gt_box, torch.float64, dev, 4)
    D, G = d_score.numel(), g_img.numel()
    g_crowd = torch.zeros(G, dtype=torch.uint8, device=dev) if gt_difficult is None else \
        (_flat(gt_difficult, torch.int64, dev) != 0).to(torch.uint8)
    g_area = (g_box[:, 2] - g_box[:, 0]) * (g_box[:, 3] - g_box[:, 1]) - 10.0 if gt_area is None else \
        _flat(gt_area, torch.float64, dev)
    if not (d_img.numel() == d_lab.numel() == d_box.shape[0] == D and
            g_lab.numel() == g_box.shape[0] == g_crowd.numel() == g_area.numel() == G):
        raise RuntimeError("coco_map: the detection arrays (and the ground-truth arrays) must have one length each")
    if D > MAX_BOXES or G > MAX_BOXES:
        raise RuntimeError(f"coco_map: {D} detections, {G} ground truths (0..{MAX_BOXES} each supported)")
    zero_id = -1 if zero_id_gt is None else int(zero_id_gt)
    if zero_id_gt is not None and not 0 <= zero_id < G:
        raise RuntimeError(f"coco_map: zero_id_gt = {zero_id} is no index into the {G} ground truths")
    i64 = dict(dtype=torch.int64, device=dev)
    with torch.cuda.device(dev):
        img_all, lab_all = torch.cat([d_img, g_img]), torch.cat([d_lab, g_lab])
        zero = torch.zeros((), **i64)
        # the (image, class) key: with num_classes=None the multiplier is the largest id + 1, still on the device
        if num_classes is not None:
            mult = int(num_classes)
        else:
            mult = lab_all.max().clamp(min=0) + 1 if D + G else 1
        dkey, gkey = d_img * mult + d_lab, g_img * mult + g_lab
        # slots: grouped by (image, class), score descending inside a group, ties in input order
        by_score = torch.sort(d_score, descending=True, stable=True).indices
        order = by_score[torch.sort(dkey[by_score], stable=True).indices]
        skey = dkey[order]
        is_start = torch.ones(D, dtype=torch.bool, device=dev)
        is_start[1:] = skey[1:] != skey[:-1]
        gid = torch.cumsum(is_start, 0) - 1
        # at most D groups: the tables have D rows, of which the first n_groups are used
        grp_cnt = torch.zeros(D, **i64).scatter_add_(0, gid, torch.ones(D, **i64))
        grp_start = torch.zeros(D + 1, **i64)
        grp_start[1:] = torch.cumsum(grp_cnt, 0)
        rank = torch.arange(D, **i64) - grp_start[gid]
        g_sorted = torch.sort(gkey, stable=True)
        gt_perm = g_sorted.indices
        gk = skey[grp_start[:D].clamp(max=max(D - 1, 0))]
        glo = torch.searchsorted(g_sorted.values, gk)
        ghi = torch.searchsorted(g_sorted.values, gk, right=True)
        n_g = ghi - glo
        need = 8 * grp_cnt.clamp(max=COCO_MAX_DETS[-1]) * n_g + 160 * ((n_g + 31) // 32) + (n_g + 7) // 8 * 8
        used = grp_cnt > 0
        big = used & (need > COCO_LDS_BYTES)
        slice_need = torch.where(big, need, zero)
        grp_ws = torch.cumsum(slice_need, 0) - slice_need
        lds_need = torch.where(used & ~big, need, zero)
        # ranges, in one read-back: [min image, max image, min label, max label, NaN scores, groups, slice bytes, LDS bytes]
        if D + G:
            words = [img_all.min(), img_all.max(), lab_all.min(), lab_all.max(), torch.isnan(d_score).sum()]
            words += [is_start.sum(), slice_need.sum(), lds_need.max()] if D else [zero, zero, zero]
            lo_i, hi_i, lo_l, hi_l, bad, NG, slice_bytes, lds_bytes = torch.stack(words).tolist()
        else:
            lo_i, hi_i, lo_l, hi_l, bad, NG, slice_bytes, lds_bytes = 0, -1, 0, -1, 0, 0, 0, 0
    if bad:
        raise RuntimeError("coco_map: NaN scores cannot be ranked")
    C = max(hi_l + 1, 1) if num_classes is None else int(num_classes)
    if not 1 <= C <= MAX_MAP_CLASSES:
        raise RuntimeError(f"coco_map: {C} classes (1..{MAX_MAP_CLASSES} supported)")
    if lo_i < 0 or lo_l < 0 or hi_l >= C:
        raise RuntimeError(f"coco_map: image indices must be >= 0 and class ids in [0, {C}) "
                           f"(got images {lo_i}..{hi_i}, classes {lo_l}..{hi_l})")
    i32, f64 = dict(dtype=torch.int32, device=dev), dict(dtype=torch.float64, device=dev)
    with torch.cuda.device(dev):
        # class order -> slot: classes ascending, score descending, ties by image index, then by input order -- two stable
        # sorts of the slot sequence, which already runs by image, then by rank inside a group
        by_score = torch.sort(d_score[order], descending=True, stable=True).indices
        class_slot = by_score[torch.sort(d_lab[order][by_score], stable=True).indices]
        det_off = torch.zeros(C + 1, **i32)
        det_off[1:] = torch.cumsum(torch.bincount(d_lab, minlength=C), 0)
        if dev not in _coco_consts:
            _coco_consts[dev] = (torch.from_numpy(COCO_IOU_THRS).to(dev), torch.from_numpy(COCO_REC_THRS).to(dev))
        iou_thrs, rec_thrs = _coco_consts[dev]
        T, R, A, M = len(COCO_IOU_THRS), len(COCO_REC_THRS), len(COCO_AREA_RNG), len(COCO_MAX_DETS)
        out = {"dt_match": torch.empty((T * A, D), **i32), "dt_code": torch.empty((T * A, D), dtype=torch.uint8, device=dev),
               "n_gt": torch.empty((C, A), **i32), "precision": torch.empty((T, R, C, A, M), **f64),
               "recall": torch.empty((T, C, A, M), **f64), "stats": torch.empty(12, **f64)}
        arg = lambda t, dt=None: (t.to(dt) if dt else t).contiguous() if t.numel() else \
            torch.empty(t.shape, dtype=dt or t.dtype, device=dev)
        hip.coco_map(arg(d_box), arg(order, torch.int32), arg(rank, torch.int32), arg(class_slot, torch.int32), det_off,
                     arg(grp_start[:NG + 1], torch.int32), arg(torch.stack([glo, ghi], 1)[:NG], torch.int32), arg(grp_ws[:NG]),
                     lds_bytes, slice_bytes, arg(g_box), arg(g_area), arg(g_crowd), arg(g_lab, torch.int32),
                     arg(gt_perm, torch.int32), C, zero_id, iou_thrs, rec_thrs, out)
        res = {k: out[k] for k in ("stats", "precision", "recall", "n_gt")}
        if return_matches:
            dt_match = torch.empty((T * A, D), **i32)
            dt_ignore = torch.empty((T * A, D), dtype=torch.uint8, device=dev)
            kept = torch.empty(D, dtype=torch.uint8, device=dev)
            dt_match[:, order] = out["dt_match"]
            dt_ignore[:, order] = (out["dt_code"] == 2).to(torch.uint8)
            kept[order] = (rank < COCO_MAX_DETS[-1]).to(torch.uint8)
            res.update(dt_match=dt_match.view(T, A, D), dt_ignore=dt_ignore.view(T, A, D), kept=kept)
    return CocoMapResult(**res)


def get_coco_map(class_names, path):
    """utils_map.py:894-923 with the reference's signature: COCOeval.stats, the 12 COCO summary numbers, of the directory
    `path` (format: `read_map_dir`) as a numpy array; utils/callbacks.py:224 logs element 1, the AP at IoU 0.5.  The two
    directories are parsed on the host as preprocess_gt / preprocess_dr do (:800-892): a line whose class is not in
    class_names is dropped, a ground-truth line containing `difficult` is a crowd, the area of a ground truth is w * h -
    10.0.  Images are numbered by sorted file stem (COCOeval sorts the image ids).  The reference numbers its annotations
    from 0 in os.listdir order of ground-truth/, and COCOeval cannot tell annotation id 0 from "unmatched": the first kept
    box in that order is handed to `coco_map` as zero_id_gt.  Without any kept detection the result is twelve zeros
    (:912-914).  A detection file without a ground-truth file raises RuntimeError: pycocotools asserts there ("Results do
    not correspond to current coco set") and the callback's `except` then falls back to `get_map`.  Only the return value is
    reproduced: nothing is written (no coco_eval/ directory), nothing is printed."""
    class_names = list(class_names)
    gt_path, dr_path = os.path.join(path, "ground-truth"), os.path.join(path, "detection-results")
    stem = lambda f: os.path.splitext(f)[0]
    gt_files, dr_files = os.listdir(gt_path), os.listdir(dr_path)
    index = {s: i for i, s in enumerate(sorted({stem(f) for f in gt_files}))}
    odd = sorted({stem(f) for f in dr_files} - set(index))
    if odd:
        raise RuntimeError(f"get_coco_map: detection-results files without a ground-truth file: {odd[:5]}")
    lines = lambda f: [l.strip() for l in open(f).read().splitlines() if l.strip()]
    gts, dets = [], []
    for f in gt_files:                                               # os.listdir order: the first kept box gets id 0
        for line in lines(os.path.join(gt_path, f)):
            diff = "difficult" in line
            tok = line.split()
            name, box = " ".join(tok[:-5] if diff else tok[:-4]), [float(v) for v in (tok[-5:-1] if diff else tok[-4:])]
            if name in class_names:
                gts.append((index[stem(f)], class_names.index(name), box, diff))
    for f in dr_files:
        for line in lines(os.path.join(dr_path, f)):
            tok = line.split()
            name, num = " ".join(tok[:-5]), [float(v) for v in tok[-5:]]
            if name in class_names:
                dets.append((index[stem(f)], class_names.index(name), num[0], num[1:]))
    if not dets:
        return np.zeros(12, dtype=np.float64)
    res = coco_map(np.array([d[0] for d in dets], dtype=np.int64), np.array([d[1] for d in dets], dtype=np.int64),
                   np.array([d[2] for d in dets], dtype=np.float64), np.array([d[3] for d in dets], dtype=np.float64).reshape(-1, 4),
                   np.array([g[0] for g in gts], dtype=np.int64), np.array([g[1] for g in gts], dtype=np.int64),
                   np.array([g[2] for g in gts], dtype=np.float64).reshape(-1, 4), np.array([g[3] for g in gts], dtype=np.uint8),
                   num_classes=max(len(class_names), 1), zero_id_gt=0 if gts else None)
    return res.stats.cpu().numpy()
