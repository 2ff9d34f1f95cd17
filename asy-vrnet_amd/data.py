"""Input formats of the training pipeline, restated from the reference's dataloader (utils/dataloader.py is
not importable here: cv2 / albumentations).  The deterministic evaluation path (`random=False`) and the format
conversions came first; the random resize / placement / flip / HSV jitter of :187-247 followed (`augment_params`,
`augment_sample`, `device_augment_batch_ragged`; csrc/augment.hip); mosaic and mixup (:251-437) stay out.
Host side (numpy / PIL): parsing, box mapping, and the PIL letterbox (`letterbox_sample`,
`resize_image`) kept as the restated reference.  Device side: `device_letterbox` (csrc/letterbox.hip) -- the letterbox
itself from RAW frame bytes, Pillow's bicubic / nearest resize reproduced bit for bit, with the paste, the padding and
the normalisation in the same call -- and `device_batch` (csrc/formats.hip): the per-pixel conversions of a letterboxed
batch -- image normalisation + CHW, label clamp, one-hot -- from bytes.  Pins: the functions the reference keeps in importable modules (`preprocess_input`, `preprocess_input_radar`,
`resize_image`) produced tests/golden/formats_small.npz (tools/make_golden_formats.py); round 5: the reference's own
`YoloDataset.__getitem__` (train=False) + `yolo_dataset_collate`, importable once cv2 / albumentations are stubbed (the
evaluation path touches neither), produced tests/golden/dataset_small.npz (tools/make_golden_dataset.py) -- parsing,
letterbox, box mapping, clamp, one-hot and collate are held to it bit for bit (tests/test_data.py)."""
import math
import os
import re

import numpy as np
import torch

MEAN = np.array([0.485, 0.456, 0.406])
STD = np.array([0.229, 0.224, 0.225])
_FRAME = re.compile(r"\d{10}.\d{5}")            # utils/dataloader.py:76-79: the frame id (timestamp) inside the path


def parse_annotation_line(line):
    """`path x1,y1,x2,y2,cls x1,y1,x2,y2,cls ...` (README.md:21-26; dataloader.py:119,133) -> (path, (n,5) int array)."""
    parts = line.split()
    if not parts:
        raise ValueError("empty annotation line")
    boxes = np.array([np.array(list(map(int, b.split(",")))) for b in parts[1:]])
    if boxes.size and boxes.shape[1] != 5:
        raise ValueError(f"annotation boxes need 5 comma-separated integers: {line!r}")
    return parts[0], boxes.reshape(-1, 5)


def frame_id(line):
    """Last `\\d{10}.\\d{5}` match of the line: names the radar .npz and the segmentation .png (dataloader.py:76-84)."""
    m = _FRAME.findall(line)
    if not m:
        raise ValueError(f"no frame id (\\d{{10}}.\\d{{5}}) in {line!r}")
    return m[-1]


def load_radar(radar_root, fid):
    """radar_root/<frame id>.npz, array `arr_0` of shape (4, H, W) (dataloader.py:111-112)."""
    return np.load(os.path.join(radar_root, fid + ".npz"))["arr_0"]


def preprocess_input(image):
    """utils_seg/utils.py:43-47 (HWC, RGB, 0..255 -> normalised); works on a float copy."""
    image = np.array(image, dtype=np.float64)
    image /= 255.0
    image -= MEAN
    image /= STD
    return image


def preprocess_input_radar(data):
    """utils/utils.py:50-53 (min-max to [0,1] + 1e-13)."""
    lo = np.min(data)
    return (data - lo) / (np.max(data) - lo) + 0.0000000000001


def letterbox_geometry(iw, ih, w, h):
    """dataloader.py:131-135: (nw, nh, dx, dy) of the aspect-preserving resize pasted into a w x h canvas."""
    scale = min(w / iw, h / ih)
    nw, nh = int(iw * scale), int(ih * scale)
    return nw, nh, (w - nw) // 2, (h - nh) // 2


def adjust_boxes(box, iw, ih, w, h):
    """Boxes (x1, y1, x2, y2, cls) of an iw x ih image -> the letterboxed w x h canvas: scaled and shifted like the
    pixels, clipped to the canvas, and boxes thinner than 2 px dropped (dataloader.py:170-180, minus its in-place
    shuffle).  The reference parses the annotation into an INTEGER array (:133) and assigns the scaled coordinates back
    into it, so every mapped coordinate is truncated towards zero before clipping -- reproduced here (pinned by
    tests/golden/dataset_small.npz, the reference's own output)."""
    nw, nh, dx, dy = letterbox_geometry(iw, ih, w, h)
    out = np.array(box, dtype=np.int64).reshape(-1, 5)
    if out.shape[0] == 0:
        return out.astype(np.float64)
    out[:, [0, 2]] = out[:, [0, 2]] * nw / iw + dx            # float result -> int64 storage: truncation, as the reference
    out[:, [1, 3]] = out[:, [1, 3]] * nh / ih + dy
    out[:, 0:2][out[:, 0:2] < 0] = 0
    out[:, 2][out[:, 2] > w] = w
    out[:, 3][out[:, 3] > h] = h
    keep = ((out[:, 2] - out[:, 0]) > 1) & ((out[:, 3] - out[:, 1]) > 1)
    return out[keep].astype(np.float64)


def boxes_xyxy_to_cxcywh(box):
    """dataloader.py:91-94: the [cx, cy, w, h, cls] rows YOLOLoss consumes."""
    box = np.array(box, dtype=np.float64).reshape(-1, 5)
    if len(box) != 0:
        box[:, 2:4] = box[:, 2:4] - box[:, 0:2]
        box[:, 0:2] = box[:, 0:2] + box[:, 2:4] / 2
    return box


def seg_targets(png, num_classes_seg):
    """dataloader.py:96-105: labels >= num_classes_seg become the ignore class; one-hot with the extra channel."""
    png = np.array(png)
    png[png >= num_classes_seg] = num_classes_seg
    seg_labels = np.eye(num_classes_seg + 1)[png.reshape([-1])].reshape(png.shape + (num_classes_seg + 1,))
    return png, seg_labels


def letterbox_sample(image, seg_label, box, input_shape):
    """The `random=False` branch of get_random_data (dataloader.py:137-183) on PIL images: bicubic resize onto a grey
    (128) canvas, nearest resize of the label onto a 0 canvas, boxes mapped alongside."""
    from PIL import Image
    iw, ih = image.size
    h, w = input_shape
    nw, nh, dx, dy = letterbox_geometry(iw, ih, w, h)
    new_image = Image.new("RGB", [w, h], (128, 128, 128))
    new_image.paste(image.convert("RGB").resize((nw, nh), Image.BICUBIC), (dx, dy))
    new_label = Image.new("L", [w, h], (0))
    new_label.paste(Image.fromarray(np.array(seg_label)).resize((nw, nh), Image.NEAREST), (dx, dy))
    return new_image, adjust_boxes(box, iw, ih, w, h), new_label


def resize_image(image, size):
    """utils_seg/utils.py:20-31 (the letterbox of the prediction scripts): bicubic resize onto a grey canvas.
    Returns (canvas, nw, nh)."""
    from PIL import Image
    iw, ih = image.size
    w, h = size
    nw, nh, dx, dy = letterbox_geometry(iw, ih, w, h)
    canvas = Image.new("RGB", size, (128, 128, 128))
    canvas.paste(image.resize((nw, nh), Image.BICUBIC), (dx, dy))
    return canvas, nw, nh


def device_batch(images_u8, pngs_u8, num_classes_seg, device="cuda"):
    """The tensors `yolo_dataset_collate` ships for a letterboxed batch, made ON THE DEVICE from bytes
    (vrnet_batch_formats_u8): images_u8 (B,H,W,3) uint8 RGB -> images (B,3,H,W) float32 normalised as preprocess_input does
    (bit-identical); pngs_u8 (B,H,W) uint8 -> png (B,H,W) int64 with the ignore class, seg_labels (B,H,W,nc+1) float32.
    numpy arrays or tensors; either input may be None.  4 B per pixel cross PCIe instead of 12 + 8 + 4 (nc + 1)."""
    from . import hip

    def dev(a):
        if a is None:
            return None
        t = a if torch.is_tensor(a) else torch.from_numpy(np.ascontiguousarray(a))
        if t.dtype != torch.uint8:
            raise RuntimeError(f"device_batch: expected uint8 bytes, got {t.dtype}")
        return t.to(device, non_blocking=True).contiguous()
    return hip.batch_formats(dev(images_u8), dev(pngs_u8), num_classes_seg)


def device_letterbox(images_u8, input_shape, labels_u8=None, letterbox_image=True, normalise=True, device="cuda"):
    """`resize_image` (utils/utils.py:19-32, utils_seg/utils.py:19-31) and the image / label half of `letterbox_sample`, ON
    THE DEVICE from raw bytes (vrnet_letterbox_u8): images_u8 (B,ih,iw,3) uint8 RGB frames of ONE original size (a single
    (ih,iw,3) frame counts as B = 1), labels_u8 (B,ih,iw) uint8 or None; input_shape = (H, W).  Returns (images, labels):
    images (B,3,H,W) float32, normalised as `device_batch` does it, or the uint8 (B,H,W,3) canvas when normalise=False;
    labels (B,H,W) uint8 -- what `device_batch(None, labels, ns)` takes -- or None.  The bytes are Pillow's BICUBIC /
    NEAREST bytes, bit for bit.  letterbox_image=False stretches to the whole canvas (utils/utils.py:30-31).  numpy arrays
    or tensors.  The boxes stay with `adjust_boxes`, on the host."""
    from . import hip

    def host(a, what, batched):
        t = a if torch.is_tensor(a) else torch.from_numpy(np.ascontiguousarray(a))
        if t.dtype != torch.uint8:
            raise RuntimeError(f"device_letterbox: expected uint8 {what}, got {t.dtype}")
        return t[None] if t.dim() == batched - 1 else t
    img = host(images_u8, "frames", 4)
    if img.dim() != 4 or img.shape[-1] != 3:
        raise RuntimeError(f"device_letterbox: expected frames of shape (B, ih, iw, 3) or (ih, iw, 3), got {tuple(img.shape)}")
    B, ih, iw = img.shape[:3]
    lab = None if labels_u8 is None else host(labels_u8, "labels", 3)
    if lab is not None and tuple(lab.shape) != (B, ih, iw):
        raise RuntimeError(f"device_letterbox: the labels {tuple(lab.shape)} do not match the frames {(B, ih, iw)}")
    H, W = (int(v) for v in input_shape)
    nw, nh, dx, dy = letterbox_geometry(max(iw, 1), max(ih, 1), W, H) if letterbox_image else (W, H, 0, 0)
    if min(B, ih, iw) <= 0 or nw <= 0 or nh <= 0:
        raise RuntimeError(f"device_letterbox: {B} frames of {ih} x {iw} leave an empty window ({nh} x {nw}) in a {H} x {W} input")
    img = img.to(device, non_blocking=True).contiguous()
    lab = None if lab is None else lab.to(device, non_blocking=True).contiguous()
    with torch.cuda.device(img.device):
        canvas = None if normalise else torch.empty((B, H, W, 3), dtype=torch.uint8, device=img.device)
        images = torch.empty((B, 3, H, W), dtype=torch.float32, device=img.device) if normalise else None
        labels = None if lab is None else torch.empty((B, H, W), dtype=torch.uint8, device=img.device)
        hip.letterbox(img, lab, H, W, nw, nh, dx, dy, canvas=canvas, images=images, label_out=labels)
    return (images if normalise else canvas), labels


# ---- ragged batches: frames of their own sizes in the corners of padded (B, ihm, iwm[, 3]) slots ------------------------
# vrnet_frame_geom of include/vrnet_hip.h, one record per image (80 bytes)
GEOM_DTYPE = np.dtype([(n, "<i4") for n in ("ih", "iw", "nw", "nh", "dx", "dy", "seg_top", "seg_left", "seg_nh", "seg_nw",
                                            "thickness", "reserved")] +
                      [(n, "<f8") for n in ("offset_y", "offset_x", "scale_y", "scale_x")])


def resample_ksize(n_in, n_out):
    """Pillow's Resample.c precompute_coeffs: the taps one output index of an axis resized n_in -> n_out can take."""
    return int(np.ceil(2.0 * max(n_in / n_out, 1.0))) * 2 + 1


def default_max_taps(capacity, input_shape):
    """The tap capacity a ragged pipeline reserves per table entry.  Both axes of a letterboxed frame share one scale s, and
    1 / s <= R = max(iwm / W, ihm / H, 1) for a frame inside the capacity; an axis in -> out = int(in * s) has
    in / out = (1 / s) * (1 + f / out) with 0 <= f < 1 the part int() cut off, so its support 2 * in / out exceeds 2 / s by less
    than 2 / (s * out) <= 1 once out >= 2 R: ceil() then grows by at most one and ksize by at most two.  Hence
    ksize(R) + 2 = 2 * ceil(2 R) + 3 serves every frame whose window is at least 2 R pixels on both axes; only thinner
    slivers can need more, and `frame_geometry` rejects those."""
    (ihm, iwm), (H, W) = capacity, input_shape
    return int(np.ceil(2.0 * max(iwm / W, ihm / H, 1.0))) * 2 + 3


def frame_sizes(sizes, batch=None, fn="frame_geometry"):
    """sizes as a (B, 2) int64 array of (ih, iw) rows.  Sizes are HOST integers (a list, an array or a CPU tensor): they
    size the copies and are validated before anything is launched, so a device tensor, whose read-back would synchronise,
    is rejected."""
    if torch.is_tensor(sizes) and sizes.is_cuda:
        raise RuntimeError(f"{fn}: sizes are host integers, got a tensor on {sizes.device} (reading it back would synchronise)")
    try:
        arr = np.asarray(sizes)
        ok = arr.ndim == 2 and arr.shape[1] == 2 and np.array_equal(arr, arr.astype(np.int64))
    except (TypeError, ValueError):
        ok = False
    if not ok:
        raise RuntimeError(f"{fn}: sizes are B integer (height, width) pairs, got {sizes!r}")
    if batch is not None and len(arr) != batch:
        raise RuntimeError(f"{fn}: {len(arr)} sizes for a batch of {batch} frames")
    return arr.astype(np.int64)


def frame_geometry(sizes, input_shape, letterbox_image=True, capacity=None, max_taps=None, fn="frame_geometry"):
    """The packed per-image table of the ragged entry points: sizes (B, 2) = (ih, iw) per image -> a (B,) GEOM_DTYPE array
    (`geometry_bytes` of it is what the device takes).  Every value is what the fixed-size path computes for that
    image alone: `letterbox_geometry`, `decode.seg_window`, `infer.unmap_scalars` and the thickness of yolo.py:164; with
    letterbox_image=False the window is the whole input.  Host only.  Raises RuntimeError naming the image index for a
    size that is not positive or above capacity = (ihm, iwm), for an empty window, and for a frame whose resize needs more
    taps than max_taps (see `default_max_taps`)."""
    from . import decode, infer
    arr = frame_sizes(sizes, fn=fn)
    H, W = (int(v) for v in input_shape)
    tab = np.zeros(len(arr), GEOM_DTYPE)
    for b, (ih, iw) in enumerate(arr.tolist()):
        if ih <= 0 or iw <= 0:
            raise RuntimeError(f"{fn}: image {b}: bad size {ih} x {iw}")
        if capacity is not None and (ih > capacity[0] or iw > capacity[1]):
            raise RuntimeError(f"{fn}: image {b}: {ih} x {iw} is above the capacity {capacity[0]} x {capacity[1]}")
        if letterbox_image:
            nw, nh, dx, dy = letterbox_geometry(iw, ih, W, H)
            top, left, snh, snw = decode.seg_window((H, W), (ih, iw))
        else:
            (nw, nh, dx, dy), (top, left, snh, snw) = (W, H, 0, 0), (0, 0, H, W)
        if min(nw, nh, snw, snh) <= 0:
            raise RuntimeError(f"{fn}: image {b}: {ih} x {iw} leaves an empty window ({nh} x {nw}) in a {H} x {W} input")
        need = max(resample_ksize(iw, nw) if nw != iw else 0, resample_ksize(ih, nh) if nh != ih else 0)
        if max_taps is not None and need > max_taps:
            raise RuntimeError(f"{fn}: image {b}: resizing {ih} x {iw} to {nh} x {nw} takes {need} taps, above the tap capacity "
                               f"{max_taps} (a sliver: raise max_taps)")
        offset, scale = infer.unmap_scalars((H, W), (ih, iw), letterbox_image)
        tab[b] = (ih, iw, nw, nh, dx, dy, top, left, snh, snw, int(max((iw + ih) // np.mean((H, W)), 1)), 0,
                  offset[0], offset[1], scale[0], scale[1])
    return tab


def geometry_bytes(table):
    """A `frame_geometry` table as the (B, hip.GEOM_BYTES) uint8 host tensor the device takes; it shares the table's memory."""
    return torch.from_numpy(table.view(np.uint8).reshape(len(table), -1))


def ragged_items(items, sizes, batch, trailing, what, fn):
    """The two forms a ragged batch comes in -> (list of B uint8 tensors or one padded uint8 tensor, sizes (B, 2) int64):
    a list of B arrays (ih_b, iw_b) + trailing of their own sizes (sizes optional, checked when given), or a padded buffer
    (B, ihp, iwp) + trailing with the images in the top-left corners, which needs sizes.  batch=None: B follows the input."""
    def u8(a, k):
        t = a if torch.is_tensor(a) else torch.from_numpy(np.ascontiguousarray(a))
        if t.dtype != torch.uint8:
            raise RuntimeError(f"{fn}: expected uint8 {what}, got {t.dtype}" + ("" if k is None else f" for image {k}"))
        return t
    if isinstance(items, (list, tuple)):
        if batch is not None and len(items) != batch:
            raise RuntimeError(f"{fn}: {len(items)} {what} for a batch of {batch}")
        ts = [u8(a, k) for k, a in enumerate(items)]
        for k, t in enumerate(ts):
            if t.dim() != 2 + len(trailing) or tuple(t.shape[2:]) != trailing:
                raise RuntimeError(f"{fn}: image {k}: expected {what} of shape (ih, iw{''.join(', %d' % v for v in trailing)}), "
                                   f"got {tuple(t.shape)}")
        own = np.array([t.shape[:2] for t in ts], np.int64).reshape(-1, 2)
        if sizes is not None:
            given = frame_sizes(sizes, len(ts), fn)
            for k in range(len(ts)):
                if tuple(given[k]) != tuple(own[k]):
                    raise RuntimeError(f"{fn}: image {k}: sizes says {tuple(given[k].tolist())}, the array is "
                                       f"{tuple(own[k].tolist())}")
        return ts, own
    t = u8(items, None)
    if t.dim() != 3 + len(trailing) or tuple(t.shape[3:]) != trailing:
        raise RuntimeError(f"{fn}: expected a list of {what} or a padded buffer (B, ihm, iwm{''.join(', %d' % v for v in trailing)}), "
                           f"got {tuple(t.shape)}")
    if batch is not None and t.shape[0] != batch:
        raise RuntimeError(f"{fn}: {t.shape[0]} {what} for a batch of {batch}")
    if sizes is None:
        raise RuntimeError(f"{fn}: a padded buffer of {what} needs sizes, the (height, width) of every image in it")
    given = frame_sizes(sizes, t.shape[0], fn)
    for k, (ih, iw) in enumerate(given.tolist()):
        if ih > t.shape[1] or iw > t.shape[2]:
            raise RuntimeError(f"{fn}: image {k}: sizes says {ih} x {iw}, the padded buffer is {t.shape[1]} x {t.shape[2]}")
    return t, given


def fill_slots(dst, items, sizes, corners_only=False):
    """Copies a ragged batch (`ragged_items`) into the corners of the slots of the device buffer dst (B, ihm, iwm, ...), all
    non_blocking.  A padded buffer is copied whole, its padding included: the ragged kernels read no input padding into a
    result.  corners_only=True copies only the `[:ih_b, :iw_b]` corner of every slot of a padded buffer too and leaves the
    rest of dst as it is -- for a buffer whose padding means something, as the 255 of `EvalPipeline.labels_u8`."""
    if torch.is_tensor(items) and not corners_only:
        dst[:, :items.shape[1], :items.shape[2]].copy_(items, non_blocking=True)
    else:
        for b, t in enumerate(items):
            ih, iw = int(sizes[b][0]), int(sizes[b][1])
            dst[b, :ih, :iw].copy_(t[:ih, :iw], non_blocking=True)


def device_letterbox_ragged(frames, sizes, input_shape, labels=None, letterbox_image=True, normalise=True, capacity=None,
                            max_taps=None, flag=None, device="cuda"):
    """`device_letterbox` for frames of DIFFERENT original sizes in one call (vrnet_letterbox_ragged_u8).  frames: a list of
    B uint8 arrays (ih_b, iw_b, 3) (sizes may be None), or a padded (B, ihm, iwm, 3) buffer with image b in its top-left
    corner and sizes (B, 2) = (ih_b, iw_b); labels: the same two forms of (ih_b, iw_b) maps, or None.  capacity = (ihm, iwm)
    of the device slots (default: the padded buffer's, or the largest frame's); max_taps: `default_max_taps`.  Returns
    (images, labels) exactly as `device_letterbox` would for every frame alone: the same Pillow bytes.  flag: an int32
    device word that receives hip.FLAG_GEOMETRY (never, for a table this function built).  numpy arrays or tensors."""
    from . import hip
    fn = "device_letterbox_ragged"
    items, own = ragged_items(frames, sizes, None, (3,), "frames", fn)
    B = len(own)
    labs = None if labels is None else ragged_items(labels, own, B, (), "label maps", fn)[0]
    if capacity is None:
        capacity = tuple(items.shape[1:3]) if torch.is_tensor(items) else (int(own[:, 0].max()), int(own[:, 1].max()))
    ihm, iwm = (int(v) for v in capacity)
    for t in (items, labs):
        if torch.is_tensor(t) and (t.shape[1] > ihm or t.shape[2] > iwm):
            raise RuntimeError(f"{fn}: the padded buffer {tuple(t.shape[1:3])} is above the capacity {(ihm, iwm)}")
    H, W = (int(v) for v in input_shape)
    max_taps = default_max_taps((ihm, iwm), (H, W)) if max_taps is None else int(max_taps)
    tab = frame_geometry(own, (H, W), letterbox_image, (ihm, iwm), max_taps, fn)
    dev = torch.device(device)
    with torch.cuda.device(dev):
        geom = geometry_bytes(tab).to(dev, non_blocking=True)
        img = torch.zeros((B, ihm, iwm, 3), dtype=torch.uint8, device=dev)
        fill_slots(img, items, own)
        lab = None
        if labs is not None:
            lab = torch.zeros((B, ihm, iwm), dtype=torch.uint8, device=dev)
            fill_slots(lab, labs, own)
        canvas = None if normalise else torch.empty((B, H, W, 3), dtype=torch.uint8, device=dev)
        images = torch.empty((B, 3, H, W), dtype=torch.float32, device=dev) if normalise else None
        out_lab = None if lab is None else torch.empty((B, H, W), dtype=torch.uint8, device=dev)
        hip.letterbox_ragged(img, lab, geom, H, W, max_taps, canvas=canvas, images=images, label_out=out_lab, flag=flag)
    return (images if normalise else canvas), out_lab


def pack_boxes(boxes, max_gt):
    """B arrays of (n_i, 5) INTEGER rows x1, y1, x2, y2, cls in pixels of the original image (`parse_annotation_line`'s;
    None or empty: no boxes) -> the pinned host pair (B, max_gt, 5) int32 and (B,) int32 that `hip.box_targets_ragged` takes
    after one non-blocking copy each, as `losses.pack_targets` packs float targets; unused rows are zero.  Raises
    RuntimeError naming the image for more than max_gt rows, for values that are not integers (the reference parses the
    annotation with int()) or outside int32, and for a wrong shape -- before anything is written."""
    B, max_gt = len(boxes), int(max_gt)
    rows = []
    for b, a in enumerate(boxes):
        if a is None:
            rows.append(None)
            continue
        a = a.detach().cpu().numpy() if torch.is_tensor(a) else np.asarray(a)
        if a.size == 0:
            rows.append(None)
            continue
        if a.dtype == np.bool_ or not np.issubdtype(a.dtype, np.integer):
            raise RuntimeError(f"pack_boxes: image {b}: boxes are integer pixel rows x1, y1, x2, y2, cls, got {a.dtype}")
        if a.ndim != 2 or a.shape[1] != 5:
            raise RuntimeError(f"pack_boxes: image {b}: expected (n, 5) rows x1, y1, x2, y2, cls, got {a.shape}")
        if a.shape[0] > max_gt:
            raise RuntimeError(f"pack_boxes: image {b} has {a.shape[0]} boxes, above max_gt = {max_gt}")
        if a.min() < -2 ** 31 or a.max() >= 2 ** 31:
            raise RuntimeError(f"pack_boxes: image {b}: a value outside int32")
        rows.append(a.astype(np.int32))
    out = torch.zeros((B, max(max_gt, 1), 5), dtype=torch.int32)
    counts = torch.zeros(B, dtype=torch.int32)
    if torch.cuda.is_available():
        out, counts = out.pin_memory(), counts.pin_memory()
    for b, a in enumerate(rows):
        if a is not None:
            out[b, :len(a)] = torch.from_numpy(a)
            counts[b] = len(a)
    return out, counts


def _device_batch_ragged(fn, frames, sizes, input_shape, labels, boxes, radar, num_classes_seg, max_gt, capacity, max_taps, flag,
                         device, default_taps, table, ops, per="a batch of {}"):
    """What `device_train_batch_ragged`, `device_augment_batch_ragged` and `device_mosaic_batch_ragged` share; fn is the
    caller's name in the messages.  default_taps(capacity, input_shape): its tap capacity; table(sizes, input_shape, capacity,
    max_taps): its validated table as the bytes the device takes, one record per output image; ops: its hip functions for
    the frames, the segmentation targets, the boxes and the radar maps (None: no radar, and none is returned)."""
    frames_op, seg_op, box_op, radar_op = ops
    items, own = ragged_items(frames, sizes, None, (3,), "frames", fn)
    n = len(own)
    if labels is None:
        raise RuntimeError(f"{fn}: the label maps are required")
    labs = ragged_items(labels, own, n, (), "label maps", fn)[0]
    if len(boxes) != n:
        raise RuntimeError(f"{fn}: {len(boxes)} box lists for {per.format(n)}")
    if capacity is None:
        capacity = tuple(items.shape[1:3]) if torch.is_tensor(items) else (int(own[:, 0].max()), int(own[:, 1].max()))
    ihm, iwm = (int(v) for v in capacity)
    for t in (items, labs):
        if torch.is_tensor(t) and (t.shape[1] > ihm or t.shape[2] > iwm):
            raise RuntimeError(f"{fn}: the padded buffer {tuple(t.shape[1:3])} is above the capacity {(ihm, iwm)}")
    H, W = (int(v) for v in input_shape)
    ns = int(num_classes_seg)
    max_taps = default_taps((ihm, iwm), (H, W)) if max_taps is None else int(max_taps)
    tab = table(own, (H, W), (ihm, iwm), max_taps)
    if radar_op is not None:
        rad = radar if torch.is_tensor(radar) else torch.from_numpy(np.ascontiguousarray(radar))
        if tuple(rad.shape) != (n, 4, H, W) or rad.dtype != torch.float32:
            raise RuntimeError(f"{fn}: radar must be torch.float32 of shape {(n, 4, H, W)}, got {rad.dtype} {tuple(rad.shape)}")
    packed, counts = pack_boxes(boxes, max_gt)
    dev = torch.device(device)
    with torch.cuda.device(dev):
        tab = tab.to(dev, non_blocking=True)
        img = torch.zeros((n, ihm, iwm, 3), dtype=torch.uint8, device=dev)
        fill_slots(img, items, own)
        lab = torch.zeros((n, ihm, iwm), dtype=torch.uint8, device=dev)
        fill_slots(lab, labs, own)
        images = torch.empty((len(tab), 3, H, W), dtype=torch.float32, device=dev)
        frames_op(img, tab, H, W, max_taps, images=images, flag=flag)
        png, onehot = seg_op(lab, tab, H, W, ns, flag=flag)
        targets, counts_out = box_op(packed.to(dev, non_blocking=True), counts.to(dev, non_blocking=True), tab, (ihm, iwm), H, W,
                                     flag=flag)
        out = (images, png, onehot, targets, counts_out)
        if radar_op is not None:
            out += (radar_op(rad.to(dev, non_blocking=True).contiguous(), tab, (ihm, iwm), flag=flag),)
    return out


def device_train_batch_ragged(frames, sizes, input_shape, labels, boxes, num_classes_seg, max_gt=64, letterbox_image=True,
                              capacity=None, max_taps=None, flag=None, device="cuda"):
    """The dataset item of the reference's training path (`random=False`: `letterbox_sample`, `boxes_xyxy_to_cxcywh`,
    `seg_targets`, the image half of `make_sample`) for a batch of RAW frames of different sizes, ON THE DEVICE: one call of
    vrnet_letterbox_ragged_u8 (the float images), one of vrnet_seg_targets_ragged_u8 and one of
    vrnet_box_targets_ragged_f32.  frames / labels / sizes / capacity / max_taps: as `device_letterbox_ragged` takes them
    (labels are required); boxes: B arrays of (n_i, 5) integer rows in original pixels (`pack_boxes`).  Returns (images
    (B,3,H,W) f32, png (B,H,W) int64, onehot (B,H,W,ns+1) f32, targets (B,max_gt,5) f32 rows [cx, cy, w, h, cls], counts (B)
    int32): what `losses.training_loss_packed` reads, bit for bit what the host functions give per image."""
    from . import hip
    fn = "device_train_batch_ragged"
    return _device_batch_ragged(
        fn, frames, sizes, input_shape, labels, boxes, None, num_classes_seg, max_gt, capacity, max_taps, flag, device, default_max_taps,
        lambda own, shape, cap, taps: geometry_bytes(frame_geometry(own, shape, letterbox_image, cap, taps, fn)),
        (lambda img, *a, **k: hip.letterbox_ragged(img, None, *a, **k), hip.seg_targets_ragged, hip.box_targets_ragged, None))


# ---- the random training augmentation (utils/dataloader.py:187-247, utils_seg/dataloader.py:79-111), host side ----------
# The host functions below are the truth the kernels of csrc/augment.hip are held to, as `letterbox_sample`, `adjust_boxes`
# and `seg_targets` are for the frame path.  The reference's joint loader returns before its augmentation (:182) and never
# moves the radar map; here one record per image drives the frame, the label map, the boxes and the radar map alike.
# vrnet_aug_rec of include/vrnet_hip.h, one record per image (816 bytes)
AUG_DTYPE = np.dtype([(n, "<i4") for n in ("ih", "iw", "nw", "nh", "dx", "dy", "flip", "color", "lb_nw", "lb_nh", "lb_dx",
                                           "lb_dy")] + [("lut", "u1", (3, 256))])


def default_aug_max_taps(capacity, input_shape, jitter=.3, scale=(.25, 2)):
    """The tap capacity an augmented pipeline reserves per table entry.  The sampler fixes one axis of the window first --
    nw = int(s W) when new_ar >= 1, nh = int(s H) otherwise, s >= scale[0] -- so that axis has in / out <= R0 =
    max(iwm / int(scale[0] W), ihm / int(scale[0] H)) for a frame inside the capacity.  The other axis follows through
    new_ar = iw / ih * u / v with u, v in [1 - jitter, 1 + jitter]: its in / out is the first axis's times v / u or u / v, at
    most J = (1 + jitter) / (1 - jitter), times (1 + f / out) with 0 <= f < 1 the part int() cut off.  With R = max(R0 J, 1) the
    support 2 in / out then exceeds 2 R by less than 2 R / out <= 1 once out >= 2 R, so ceil() grows by at most one and ksize
    by at most two, as in `default_max_taps`: 2 * ceil(2 R) + 3 serves every window of at least 2 R pixels on both axes.
    Only thinner slivers can need more, and `augment_params` rejects those by name."""
    (ihm, iwm), (H, W) = capacity, input_shape
    lo = max(int(scale[0] * W), 1), max(int(scale[0] * H), 1)
    R = max(max(iwm / lo[0], ihm / lo[1]) * (1 + jitter) / (1 - jitter), 1.0)
    return int(np.ceil(2.0 * R)) * 2 + 3


def aug_luts(r):
    """The three 256-byte tables of the colour stage from the gains r = (hue, sat, val) (dataloader.py:226-229)."""
    r = np.asarray(r, np.float64)
    x = np.arange(0, 256, dtype=r.dtype)
    return np.stack([((x * r[0]) % 180).astype(np.uint8), np.clip(x * r[1], 0, 255).astype(np.uint8),
                     np.clip(x * r[2], 0, 255).astype(np.uint8)])


def aug_record(size, input_shape, nw, nh, dx, dy, flip=False, color=False, gains=(1.0, 1.0, 1.0)):
    """One AUG_DTYPE record for an image of size = (ih, iw) written out by hand: the window, the flip, and the tables of
    `aug_luts(gains)`; the letterbox window of the image is filled in.  Not validated: `check_aug_table` does that."""
    H, W = (int(v) for v in input_shape)
    ih, iw = (int(v) for v in size)
    rec = np.zeros((), AUG_DTYPE)
    lb = letterbox_geometry(max(iw, 1), max(ih, 1), W, H)
    for k, v in zip(AUG_DTYPE.names[:12], (ih, iw, nw, nh, dx, dy, int(bool(flip)), int(bool(color))) + lb):
        rec[k] = v
    rec["lut"] = aug_luts(gains)
    return rec


def check_aug_table(table, input_shape, capacity=None, max_taps=None, fn="augment_params"):
    """Raises RuntimeError naming the image index for a record the kernels would have to clamp: a size that is not positive
    or above capacity = (ihm, iwm), an empty window or one above twice the canvas's larger side, a stale letterbox window,
    and a resize that needs more taps than max_taps.  Host only.  Returns the table."""
    H, W = (int(v) for v in input_shape)
    table = np.asarray(table)
    if table.dtype != AUG_DTYPE or table.ndim != 1:
        raise RuntimeError(f"{fn}: the augmentation table is a (B,) array of data.AUG_DTYPE records")
    for b, t in enumerate(table):
        check_window(t, (H, W), capacity, max_taps, f"image {b}", fn)
    return table


def check_window(t, input_shape, capacity, max_taps, where, fn):
    """`check_aug_table`'s checks for one record or one Mosaic tile t (fields ih, iw, nw, nh, dx, dy, lb_*); where names it."""
    H, W = input_shape
    ih, iw, nw, nh, dx, dy = (int(t[k]) for k in ("ih", "iw", "nw", "nh", "dx", "dy"))
    if ih <= 0 or iw <= 0:
        raise RuntimeError(f"{fn}: {where}: bad size {ih} x {iw}")
    if capacity is not None and (ih > capacity[0] or iw > capacity[1]):
        raise RuntimeError(f"{fn}: {where}: {ih} x {iw} is above the capacity {capacity[0]} x {capacity[1]}")
    if nw <= 0 or nh <= 0:
        raise RuntimeError(f"{fn}: {where}: the draw leaves an empty window ({nh} x {nw}) for {ih} x {iw} in a {H} x {W} input")
    if max(nw, nh) > 2 * max(W, H) or not (-nw <= dx <= W and -nh <= dy <= H):
        raise RuntimeError(f"{fn}: {where}: the window {nh} x {nw} at ({dy}, {dx}) is out of range for a {H} x {W} input "
                           f"(at most {2 * max(W, H)} pixels, touching the canvas)")
    if tuple(int(t[k]) for k in ("lb_nw", "lb_nh", "lb_dx", "lb_dy")) != letterbox_geometry(iw, ih, W, H) or \
            min(int(t["lb_nw"]), int(t["lb_nh"])) <= 0:
        raise RuntimeError(f"{fn}: {where}: the record's letterbox window is not that of {ih} x {iw} in a {H} x {W} input")
    need = max(resample_ksize(iw, nw) if nw != iw else 0, resample_ksize(ih, nh) if nh != ih else 0)
    if max_taps is not None and need > max_taps:
        raise RuntimeError(f"{fn}: {where}: resizing {ih} x {iw} to {nh} x {nw} takes {need} taps, above the tap capacity "
                           f"{max_taps} (a sliver: raise max_taps)")


def augment_params(sizes, input_shape, rng, jitter=.3, hue=.1, sat=.7, val=.4, scale=(.25, 2), flip=.5, color=True,
                   capacity=None, max_taps=None, fn="augment_params"):
    """The random draw of the training augmentation, one AUG_DTYPE record per image (`augment_bytes` of the table is what
    the device takes): sizes (B, 2) = (ih, iw) per image, rng a numpy.random.RandomState or a seed.  Per image, in the order
    of utils/dataloader.py:187-217: two rand() for new_ar = iw / ih * rand(1 - jitter, 1 + jitter) / rand(1 - jitter, 1 + jitter),
    one for scale, then nh = int(scale * h), nw = int(nh * new_ar) when new_ar < 1, else nw = int(scale * w), nh =
    int(nw / new_ar); one rand() each for dx = int(rand(0, w - nw)) and dy (negative when the window is larger than the
    canvas; int() truncates toward zero); one for the flip (rand() < flip); uniform(-1, 1, 3) * [hue, sat, val] + 1 for the
    gains, from which `aug_luts` builds the three tables (drawn with color=False too, so the stream does not depend on it).
    The record also carries the image's letterbox window, which the stored radar map is aligned with.  Host only.  Raises
    RuntimeError naming the image index (`check_aug_table`) for an empty window, a size above capacity = (ihm, iwm) and a
    resize that needs more taps than max_taps (see `default_aug_max_taps`)."""
    arr = frame_sizes(sizes, fn=fn)
    H, W = (int(v) for v in input_shape)
    rs = rng if isinstance(rng, np.random.RandomState) else np.random.RandomState(rng)

    def rand(a=0.0, b=1.0):
        return rs.rand() * (b - a) + a
    tab = np.zeros(len(arr), AUG_DTYPE)
    for b, (ih, iw) in enumerate(arr.tolist()):            # what no draw can mend is raised before the generator moves
        if ih <= 0 or iw <= 0:
            raise RuntimeError(f"{fn}: image {b}: bad size {ih} x {iw}")
        if capacity is not None and (ih > capacity[0] or iw > capacity[1]):
            raise RuntimeError(f"{fn}: image {b}: {ih} x {iw} is above the capacity {capacity[0]} x {capacity[1]}")
    for b, (ih, iw) in enumerate(arr.tolist()):
        new_ar = iw / ih * rand(1 - jitter, 1 + jitter) / rand(1 - jitter, 1 + jitter)
        sc = rand(scale[0], scale[1])
        if new_ar < 1:
            nh = int(sc * H)
            nw = int(nh * new_ar)
        else:
            nw = int(sc * W)
            nh = int(nw / new_ar)
        dx = int(rand(0, W - nw))
        dy = int(rand(0, H - nh))
        flipped = rand() < flip
        gains = rs.uniform(-1, 1, 3) * [hue, sat, val] + 1
        tab[b] = aug_record((ih, iw), (H, W), nw, nh, dx, dy, flipped, color, gains)
    return check_aug_table(tab, (H, W), capacity, max_taps, fn)


def augment_bytes(table):
    """An AUG_DTYPE table as the (B, hip.AUG_BYTES) uint8 host tensor the device takes; it shares the table's memory."""
    return torch.from_numpy(table.view(np.uint8).reshape(len(table), -1))


def rgb_to_hsv_u8(rgb):
    """OpenCV's 8-bit COLOR_RGB2HSV restated, integers only: (..., 3) uint8 -> (..., 3) uint8 with h in [0, 180).
    v = max, d = max - min; s = (d * sdiv[v] + 2048) >> 12 with sdiv[i] = rint((255 << 12) / i); h0 = g - b if v == r, else
    b - r + 2 d if v == g, else r - g + 4 d; h = (h0 * hdiv[d] + 2048) >> 12 (arithmetic shift) with hdiv[i] =
    rint((180 << 12) / (6 i)), plus 180 when negative; both tables are 0 at i = 0."""
    a = np.asarray(rgb).astype(np.int64)
    r, g, b = a[..., 0], a[..., 1], a[..., 2]
    i = np.arange(1, 256, dtype=np.float64)
    sdiv = np.concatenate([[0], np.rint((255 << 12) / i)]).astype(np.int64)
    hdiv = np.concatenate([[0], np.rint((180 << 12) / (6 * i))]).astype(np.int64)
    v = np.maximum(np.maximum(r, g), b)
    d = v - np.minimum(np.minimum(r, g), b)
    s = (d * sdiv[v] + 2048) >> 12
    h0 = np.where(v == r, g - b, np.where(v == g, b - r + 2 * d, r - g + 4 * d))
    h = (h0 * hdiv[d] + 2048) >> 12
    h = np.where(h < 0, h + 180, h)
    return np.stack([h, np.minimum(s, 255), v], -1).astype(np.uint8)


def hsv_to_rgb_u8(hsv):
    """OpenCV's COLOR_HSV2RGB for 8-bit input restated in float32, one rounding per operation: s, v times 1 / 255f, h times
    6f / 180 (minus 6 when a hue byte of 180 or more brings it to 6 or above); sector = floor(h), f = h - sector; tab = {v,
    v (1 - s), v (1 - s f), v (1 - s (1 - f))}; (b, g, r) = tab[{1,3,0},{1,0,2},{3,0,1},{0,2,1},{0,1,3},{2,1,0}][sector]; s == 0
    gives v in all three; each channel times 255f, rounded half to even, clipped to a byte."""
    f32 = np.float32
    a = np.asarray(hsv)
    h, s, v = (a[..., k].astype(f32) for k in range(3))
    s = s * (f32(1) / f32(255))
    v = v * (f32(1) / f32(255))
    h = h * (f32(6) / f32(180))
    h = np.where(h >= f32(6), h - f32(6), h).astype(f32)
    fl = np.floor(h)
    sector = fl.astype(np.int64)
    f = h - fl
    one = f32(1)
    tab = np.stack([v, v * (one - s), v * (one - s * f), v * (one - s * (one - f))], -1)
    assert tab.dtype == np.float32
    pick = np.array([[1, 3, 0], [1, 0, 2], [3, 0, 1], [0, 2, 1], [0, 1, 3], [2, 1, 0]])[sector]          # (..., 3): b, g, r
    bgr = np.take_along_axis(tab, pick, -1)
    bgr = np.where((a[..., 1] == 0)[..., None], v[..., None], bgr).astype(f32)
    out = np.clip(np.rint(bgr * f32(255)), 0, 255).astype(np.uint8)
    return out[..., ::-1]


def hsv_jitter(canvas_u8, luts):
    """The colour stage (dataloader.py:221-232) on a (..., 3) uint8 RGB array: `rgb_to_hsv_u8`, the three table lookups
    (luts (3, 256) uint8: hue, sat, val), `hsv_to_rgb_u8`.  The conversions restate OpenCV's 8-bit paths from its public
    sources; cv2 is not a dependency of this project and agreement with cv2's own bytes is UNMEASURED.  The round trip alone
    moves a byte by up to 5 levels on random input, so identity gains are not the identity; `color=False` skips the stage."""
    luts = np.asarray(luts, np.uint8).reshape(3, 256)
    hsv = rgb_to_hsv_u8(canvas_u8)
    return hsv_to_rgb_u8(np.stack([luts[k][hsv[..., k]] for k in range(3)], -1))


# ---- the blur and the rotation behind the paste (utils_seg/dataloader.py:113-131), host side ---------------------------------
# The segmentation loader blurs (cv2.GaussianBlur(image, (5, 5), 0)) and rotates (cv2.warpAffine about the canvas centre by a
# whole angle in [-10, 10]: INTER_CUBIC and a grey border for the image, INTER_NEAREST and a 0 border for the label map) each
# item with probability 0.25 each, between the flip and the colour stage.  The functions below restate OpenCV's 8-bit
# fixed-point paths from its public sources and are the truth the vrnet_augment_post_* kernels of csrc/augment.hip are held
# to, bit for bit; cv2 is not a dependency of this project and agreement with cv2's own bytes is UNMEASURED.
# vrnet_aug_post_rec of include/vrnet_hip.h, one record per image (112 bytes)
AUG_POST_DTYPE = np.dtype([(n, "<i4") for n in ("blur", "rotate", "angle", "reserved")] + [("inv", "<f8", (6,)), ("fwd", "<f8", (6,))])
AUG_POST_MIN_SIDE = 8                            # the smallest canvas side the entry points of the post stage take
AUG_POST_MAX_ANGLE = 45                          # the largest max_angle they take


def reflect_101(i, n):
    """OpenCV's BORDER_REFLECT_101 for indices -n < i < 2 n - 1 of an axis of n: -1 -> 1, -2 -> 2, n -> n - 2, n + 1 -> n - 3."""
    i = np.asarray(i)
    i = np.where(i < 0, -i, i)
    return np.where(i >= n, 2 * n - 2 - i, i)


def gaussian_blur5_u8(canvas):
    """cv2.GaussianBlur(canvas, (5, 5), 0) on (H, W, 3) uint8 restated, integers only: with w = [1, 4, 6, 4, 1] on both axes
    and BORDER_REFLECT_101, S = sum_j sum_i w[j] w[i] p[y + j - 2, x + i - 2]; the output is (S + 128) >> 8.  That is what
    OpenCV's 8-bit fixed-point path gives for the ksize = 5, sigma = 0 kernel {1, 4, 6, 4, 1} / 16: every weight is exact in
    8.8 fixed point, and its final rounding is this one.  Restated from OpenCV's published behaviour; agreement with cv2's own
    bytes is UNMEASURED.  H, W >= 3 (the reflection); the device entry points ask for 8."""
    a = np.asarray(canvas)
    if a.ndim != 3 or a.dtype != np.uint8 or min(a.shape[:2]) < 3:
        raise RuntimeError(f"gaussian_blur5_u8: expected (H, W, C) uint8 with H, W >= 3, got {a.dtype} {a.shape}")
    a = a.astype(np.int64)
    H, W = a.shape[:2]
    w = (1, 4, 6, 4, 1)
    ix, iy = reflect_101(np.arange(-2, W + 2), W), reflect_101(np.arange(-2, H + 2), H)
    h = sum(w[i] * a[:, ix[i:i + W]] for i in range(5))
    s = sum(w[j] * h[iy[j:j + H]] for j in range(5))
    return ((s + 128) >> 8).astype(np.uint8)


def rotation_matrices(input_shape, angle):
    """(fwd, inv), six float64 each, of the reference's rotation by `angle` (its `rotation`, an int; it passes -rotation to
    cv2.getRotationMatrix2D) about c = (W // 2, H // 2): a = -angle * pi / 180, alpha = cos a, beta = sin a, fwd = [[alpha, beta,
    (1 - alpha) cx - beta cy], [-beta, alpha, beta cx + (1 - alpha) cy]]; inv is its inverse by warpAffine's own sequence: D =
    1 / (m0 m4 - m1 m3), A11 = m4 D, A22 = m0 D, m1 *= -D, m3 *= -D, b1 = -A11 m2 - m1 m5, b2 = -m3 m2 - A22 m5.  Host only:
    the device receives the twelve doubles."""
    H, W = (int(v) for v in input_shape)
    cx, cy = float(W // 2), float(H // 2)
    a = -int(angle) * math.pi / 180
    alpha, beta = math.cos(a), math.sin(a)
    m = [alpha, beta, (1 - alpha) * cx - beta * cy, -beta, alpha, beta * cx + (1 - alpha) * cy]
    fwd = np.array(m, np.float64)
    D = m[0] * m[4] - m[1] * m[3]
    D = 1.0 / D if D != 0 else 0.0
    A11, A22 = m[4] * D, m[0] * D
    m[0], m[4] = A11, A22
    m[1] *= -D
    m[3] *= -D
    b1 = -m[0] * m[2] - m[1] * m[5]
    b2 = -m[3] * m[2] - m[4] * m[5]
    m[2], m[5] = b1, b2
    return fwd, np.array(m, np.float64)


def _sat_i32(v):
    return np.clip(np.rint(v), -2.0 ** 31, 2.0 ** 31 - 1).astype(np.int64)


def _wrap_i32(v):
    return ((v + 2 ** 31) % 2 ** 32) - 2 ** 31


def warp_coords(inv, H, W, nearest):
    """warpAffine's fixed-point coordinate walk (AB_BITS = 10) for the (H, W) output under the inverse map inv: adelta[x] =
    rint(inv[0] x 1024), bdelta[x] = rint(inv[3] x 1024); per row X0 = rint((inv[1] y + inv[2]) 1024) + rd, Y0 = rint((inv[4] y +
    inv[5]) 1024) + rd with rd = 512 for nearest and 16 otherwise; rint rounds half to even, one IEEE rounding per operation.
    nearest: returns (sx, sy) = ((X0 + adelta[x]) >> 10, (Y0 + bdelta[x]) >> 10).  Otherwise (sx, sy, ax, ay): X = (X0 +
    adelta[x]) >> 5, sx = X >> 5, ax = X & 31, the same for Y.  All shifts are arithmetic, on 32-bit integers; (H, W) int64."""
    inv = np.asarray(inv, np.float64).reshape(6)
    x, y = np.arange(W, dtype=np.float64), np.arange(H, dtype=np.float64)
    rd = 512 if nearest else 16
    adelta, bdelta = _sat_i32(inv[0] * x * 1024.0), _sat_i32(inv[3] * x * 1024.0)
    X0 = _wrap_i32(_sat_i32((inv[1] * y + inv[2]) * 1024.0) + rd)
    Y0 = _wrap_i32(_sat_i32((inv[4] * y + inv[5]) * 1024.0) + rd)
    X, Y = _wrap_i32(X0[:, None] + adelta[None, :]), _wrap_i32(Y0[:, None] + bdelta[None, :])
    if nearest:
        return X >> 10, Y >> 10
    X, Y = X >> 5, Y >> 5
    return X >> 5, Y >> 5, X & 31, Y & 31


def cubic_coeffs(a):
    """The four float32 bicubic coefficients (A = -0.75) at t = a / 32, a in 0 .. 31, one rounding per operation, evaluated left
    to right as written in `cubic_weights`; (..., 4) float32."""
    f32 = np.float32
    t = np.asarray(a).astype(f32) * f32(1 / 32)
    A, one = f32(-0.75), f32(1)
    u, v = t + one, one - t
    c0 = ((A * u - f32(5) * A) * u + f32(8) * A) * u - f32(4) * A
    c1 = ((A + f32(2)) * t - (A + f32(3))) * t * t + one
    c2 = ((A + f32(2)) * v - (A + f32(3))) * v * v + one
    c3 = one - c0 - c1 - c2
    out = np.stack([c0, c1, c2, c3], -1)
    assert out.dtype == np.float32
    return out


def cubic_weights(ay, ax):
    """The 4 x 4 fixed-point weights of warpAffine's INTER_CUBIC for the fractions ay, ax in 0 .. 31 (1 / 32 pixel): with t =
    a / 32 in float32 and A = -0.75f, c0 = ((A (t + 1) - 5 A)(t + 1) + 8 A)(t + 1) - 4 A, c1 = ((A + 2) t - (A + 3)) t t + 1, c2 =
    ((A + 2)(1 - t) - (A + 3))(1 - t)(1 - t) + 1, c3 = 1 - c0 - c1 - c2; weight [k1][k2] = rint(float32(cy[k1] cx[k2]) 32768f) as
    int32.  If the sixteen do not sum to 32768 the difference is taken from one of the four central weights (k1, k2 in {1, 2}):
    from the largest when the sum is short, from the smallest when it is long, the first in row-major order on a tie.  So
    every set sums to exactly 32768 and ay = ax = 0 is the identity.  OpenCV keeps these weights in int16; whether its bytes
    differ where a weight reaches 32768 is part of what is UNMEASURED.  Returns (..., 4, 4) int32."""
    f32 = np.float32
    cy, cx = np.broadcast_arrays(cubic_coeffs(ay), cubic_coeffs(ax))
    wt = np.rint((cy[..., :, None] * cx[..., None, :]).astype(f32) * f32(32768)).astype(np.int32)
    diff = 32768 - wt.reshape(wt.shape[:-2] + (16,)).sum(-1)
    mid = wt[..., 1:3, 1:3].reshape(wt.shape[:-2] + (4,))
    pick = np.where(diff > 0, mid.argmax(-1), mid.argmin(-1))               # argmax / argmin: the first on a tie
    add = np.zeros(mid.shape, np.int32)
    np.put_along_axis(add, pick[..., None], diff[..., None].astype(np.int32), -1)
    wt = wt.copy()
    wt[..., 1:3, 1:3] += add.reshape(add.shape[:-1] + (2, 2))
    return wt


def rotate_canvas_u8(canvas, inv):
    """cv2.warpAffine(canvas, M, (W, H), flags=INTER_CUBIC, borderValue=(128, 128, 128)) on (H, W, 3) uint8 restated, with inv the
    inverse of M (`rotation_matrices`): (sx, sy, ax, ay) = `warp_coords`, wt = `cubic_weights(ay, ax)`; each channel of output
    (x, y) is clip((sum_{k1, k2} wt[k1][k2] src[sy - 1 + k1, sx - 1 + k2] + 16384) >> 15, 0, 255); a tap outside the canvas
    reads 128.  Agreement with cv2's own bytes is UNMEASURED."""
    a = np.asarray(canvas)
    H, W = a.shape[:2]
    sx, sy, ax, ay = warp_coords(inv, H, W, False)
    wt = cubic_weights(ay, ax).astype(np.int64)
    acc = np.zeros(a.shape, np.int64)
    for k1 in range(4):
        for k2 in range(4):
            yy, xx = sy - 1 + k1, sx - 1 + k2
            ok = (yy >= 0) & (yy < H) & (xx >= 0) & (xx < W)
            v = np.where(ok[..., None], a[np.clip(yy, 0, H - 1), np.clip(xx, 0, W - 1)], 128).astype(np.int64)
            acc += wt[..., k1, k2, None] * v
    return np.clip((acc + 16384) >> 15, 0, 255).astype(np.uint8)


def rotate_nearest(plane, inv, fill):
    """cv2.warpAffine(plane, M, (W, H), flags=INTER_NEAREST, borderValue=fill) on an (H, W) array of any type: output (x, y) is
    plane[sy, sx] of the nearest walk of `warp_coords`, or fill outside.  The label canvas takes fill 0, before the
    >= num_classes clamp and the one-hot; each radar channel takes fill 0.0 -- this project's definition: the reference
    rotates no radar map."""
    a = np.asarray(plane)
    H, W = a.shape
    sx, sy = warp_coords(inv, H, W, True)
    ok = (sy >= 0) & (sy < H) & (sx >= 0) & (sx < W)
    return np.where(ok, a[np.clip(sy, 0, H - 1), np.clip(sx, 0, W - 1)], np.asarray(fill, a.dtype)).astype(a.dtype)


def rotate_boxes(box, fwd, w, h):
    """The boxes under the rotation -- this project's definition, the segmentation loader has none.  box: the int64 rows [x1,
    y1, x2, y2, cls] of `augment_boxes` before its clip, changed in place and returned: the four corners go through fwd in
    float64, x' = fwd[0] x + fwd[1] y + fwd[2], y' = fwd[3] x + fwd[4] y + fwd[5], evaluated left to right; the min and max per
    axis are stored back into the integer array, which truncates toward zero as every other box stage does.  The clip to the
    (w, h) canvas and the keep test follow in `augment_boxes`."""
    fwd = np.asarray(fwd, np.float64).reshape(6)
    if len(box):
        xs = box[:, [0, 2, 0, 2]].astype(np.float64)
        ys = box[:, [1, 1, 3, 3]].astype(np.float64)
        rx = fwd[0] * xs + fwd[1] * ys + fwd[2]
        ry = fwd[3] * xs + fwd[4] * ys + fwd[5]
        box[:, 0], box[:, 2] = rx.min(1), rx.max(1)
        box[:, 1], box[:, 3] = ry.min(1), ry.max(1)
    return box


def aug_post_record(input_shape, blur, angle):
    """One AUG_POST_DTYPE record written out by hand: blur on or off, the rotation by `angle` (the reference's `rotation`; 0:
    no rotation, the warp is then the identity and is skipped) with both matrices of `rotation_matrices`."""
    rec = np.zeros((), AUG_POST_DTYPE)
    rec["blur"], rec["rotate"], rec["angle"] = int(bool(blur)), int(int(angle) != 0), int(angle)
    rec["fwd"], rec["inv"] = rotation_matrices(input_shape, int(angle))
    return rec


def check_aug_post_table(table, input_shape, max_angle=None, batch=None, fn="augment_post_params"):
    """Raises RuntimeError naming the image index for a post record the kernels would have to clamp: a matrix entry that is
    not finite, or |angle| above max_angle, the capacity the LDS budget of vrnet_augment_post_frames_u8 was sized for.  Host
    only.  Returns the table as a contiguous array."""
    H, W = (int(v) for v in input_shape)
    table = np.ascontiguousarray(table)
    if table.dtype != AUG_POST_DTYPE or table.ndim != 1 or (batch is not None and len(table) != batch):
        raise RuntimeError(f"{fn}: the post table is a ({'B' if batch is None else batch},) array of data.AUG_POST_DTYPE records")
    if max_angle is not None and not 0 <= int(max_angle) <= AUG_POST_MAX_ANGLE:
        raise RuntimeError(f"{fn}: 0 <= max_angle <= {AUG_POST_MAX_ANGLE}, got {max_angle}")
    if min(H, W) < AUG_POST_MIN_SIDE:
        raise RuntimeError(f"{fn}: blur and rotation need a canvas of at least {AUG_POST_MIN_SIDE} x {AUG_POST_MIN_SIDE}, got {H} x {W}")
    for b, t in enumerate(table):
        if not (np.isfinite(t["inv"]).all() and np.isfinite(t["fwd"]).all()):
            raise RuntimeError(f"{fn}: image {b}: the post record's matrices are not finite")
        if max_angle is not None and abs(int(t["angle"])) > int(max_angle):
            raise RuntimeError(f"{fn}: image {b}: the angle {int(t['angle'])} is above max_angle = {int(max_angle)}")
    return table


def augment_post_params(n, input_shape, rng, blur=.25, rotate=.25, max_angle=10):
    """The random draw of the blur and the rotation, one AUG_POST_DTYPE record per image (`aug_post_bytes` of the table is what
    the device takes).  Per image, as utils_seg/dataloader.py:113-131: rand() < blur, rand() < rotate, randint(-max_angle,
    max_angle + 1); all three are always drawn, for the whole batch AFTER `augment_params` has drawn its table from the same
    RandomState -- and only when blur > 0 or rotate > 0: with both at 0 the generator is not touched, so every seeded result
    from before this stage existed stays what it was.  rotate is stored as 0 when the drawn angle is 0.  Host only."""
    rs = rng if isinstance(rng, np.random.RandomState) else np.random.RandomState(rng)
    tab = np.stack([aug_post_record(input_shape, False, 0)] * int(n)) if n else np.zeros(0, AUG_POST_DTYPE)
    if blur > 0 or rotate > 0:
        for b in range(int(n)):
            blurred, rotated = rs.rand() < blur, rs.rand() < rotate
            angle = int(rs.randint(-int(max_angle), int(max_angle) + 1))
            tab[b] = aug_post_record(input_shape, blurred, angle if rotated else 0)
    return check_aug_post_table(tab, input_shape, max_angle)


def aug_post_bytes(table):
    """An AUG_POST_DTYPE table as the (B, hip.AUG_POST_BYTES) uint8 host tensor the device takes; it shares the table's memory."""
    return torch.from_numpy(table.view(np.uint8).reshape(len(table), -1))


def augment_boxes(box, iw, ih, w, h, rec, post=None):
    """`adjust_boxes` with the window of the record instead of the letterbox's, and box[:, [0, 2]] = w - box[:, [2, 0]] when
    the record flips, before the clip (dataloader.py:237-247, minus its in-place shuffle): integer storage, so every
    mapped coordinate is truncated toward zero.  With the letterbox window and no flip it equals `adjust_boxes`.  post: an
    AUG_POST_DTYPE record; when it rotates, `rotate_boxes` runs behind the flip, and the clip follows once."""
    nw, nh, dx, dy = (int(rec[k]) for k in ("nw", "nh", "dx", "dy"))
    out = np.array(box, dtype=np.int64).reshape(-1, 5)
    if out.shape[0] == 0:
        return out.astype(np.float64)
    out[:, [0, 2]] = out[:, [0, 2]] * nw / iw + dx
    out[:, [1, 3]] = out[:, [1, 3]] * nh / ih + dy
    if int(rec["flip"]):
        out[:, [0, 2]] = w - out[:, [2, 0]]
    if post is not None and int(post["rotate"]):
        rotate_boxes(out, post["fwd"], w, h)
    out[:, 0:2][out[:, 0:2] < 0] = 0
    out[:, 2][out[:, 2] > w] = w
    out[:, 3][out[:, 3] > h] = h
    keep = ((out[:, 2] - out[:, 0]) > 1) & ((out[:, 3] - out[:, 1]) > 1)
    return out[keep].astype(np.float64)


def augment_radar(radar, input_shape, rec):
    """The radar map under an augmentation record -- this project's own definition, the reference has none.  radar (4, H, W)
    belongs to the LETTERBOXED frame (window lb_nw x lb_nh at (lb_dx, lb_dy)).  Canvas pixel (x, y): x' = W - 1 - x when the
    record flips, else x; wx = x' - dx, wy = y - dy; outside 0 <= wx < nw, 0 <= wy < nh the value is 0; inside it is
    radar[c, lb_dy + ((2 wy + 1) * lb_nh) // (2 nh), lb_dx + ((2 wx + 1) * lb_nw) // (2 nw)]: the nearest stored pixel under
    the pixel-centre map, integers only.  Values stored outside the letterbox window are never read.  With the letterbox
    window and no flip it returns the window's values bit for bit.  Nearest sampling duplicates (enlarging) or drops
    (shrinking) the sparse radar points; that is a choice, and its effect on accuracy has not been measured."""
    H, W = (int(v) for v in input_shape)
    radar = np.asarray(radar)
    nw, nh, dx, dy, lnw, lnh, ldx, ldy = (int(rec[k]) for k in ("nw", "nh", "dx", "dy", "lb_nw", "lb_nh", "lb_dx", "lb_dy"))
    x = np.arange(W, dtype=np.int64)
    wx = (W - 1 - x if int(rec["flip"]) else x) - dx
    wy = np.arange(H, dtype=np.int64) - dy
    okx, oky = (wx >= 0) & (wx < nw), (wy >= 0) & (wy < nh)
    sx = ldx + ((2 * np.where(okx, wx, 0) + 1) * lnw) // (2 * nw)
    sy = ldy + ((2 * np.where(oky, wy, 0) + 1) * lnh) // (2 * nh)
    out = radar[:, sy[:, None], sx[None, :]]
    return np.where((oky[:, None] & okx[None, :])[None], out, np.zeros((), radar.dtype)).astype(radar.dtype)


def augment_sample(image, seg_label, box, radar, input_shape, rec, post=None):
    """One dataset item under the augmentation record rec (`augment_params`), on PIL images and numpy arrays; returns
    (canvas, boxes, label canvas, radar).  Image: resize((nw, nh), BICUBIC) pasted at (dx, dy) on a grey (128) canvas --
    Pillow crops what falls outside -- then FLIP_LEFT_RIGHT of the whole canvas when the record flips, then `hsv_jitter`
    when its colour stage is on (the order of dataloader.py:195-232).  Label: resize((nw, nh), NEAREST) pasted on a 0 canvas
    and flipped with it (utils_seg/dataloader.py:91-111), no colour stage.  Boxes: `augment_boxes`.  Radar: `augment_radar`.
    post: an AUG_POST_DTYPE record (`augment_post_params`) or None.  Between the flip and the colour stage, in the order of
    utils_seg/dataloader.py:113-131: `gaussian_blur5_u8` of the canvas when it blurs; when it rotates, `rotate_canvas_u8` of
    the canvas, `rotate_nearest` of the label canvas (fill 0) and of each radar channel (fill 0.0), `rotate_boxes`."""
    from PIL import Image
    iw, ih = image.size
    h, w = input_shape
    nw, nh, dx, dy = (int(rec[k]) for k in ("nw", "nh", "dx", "dy"))
    new_image = Image.new("RGB", [w, h], (128, 128, 128))
    new_image.paste(image.convert("RGB").resize((nw, nh), Image.BICUBIC), (dx, dy))
    new_label = Image.new("L", [w, h], (0))
    new_label.paste(Image.fromarray(np.array(seg_label)).resize((nw, nh), Image.NEAREST), (dx, dy))
    if int(rec["flip"]):
        new_image = new_image.transpose(Image.FLIP_LEFT_RIGHT)
        new_label = new_label.transpose(Image.FLIP_LEFT_RIGHT)
    new_radar = augment_radar(radar, input_shape, rec)
    if post is not None:                 # utils_seg/dataloader.py:113-131: the blur, then the rotation, before the colour stage
        if int(post["blur"]):
            new_image = Image.fromarray(gaussian_blur5_u8(np.array(new_image, np.uint8)))
        if int(post["rotate"]):
            new_image = Image.fromarray(rotate_canvas_u8(np.array(new_image, np.uint8), post["inv"]))
            new_label = Image.fromarray(rotate_nearest(np.array(new_label, np.uint8), post["inv"], 0))
            new_radar = np.stack([rotate_nearest(ch, post["inv"], 0.0) for ch in new_radar])
    if int(rec["color"]):
        new_image = Image.fromarray(hsv_jitter(np.array(new_image, np.uint8), rec["lut"]))
    return new_image, augment_boxes(box, iw, ih, w, h, rec, post), new_label, new_radar


def device_augment_batch_ragged(frames, sizes, input_shape, labels, boxes, radar, num_classes_seg, params, max_gt=64,
                                capacity=None, max_taps=None, flag=None, device="cuda", post=None, max_angle=10):
    """`device_train_batch_ragged` under the training augmentation: the dataset item `augment_sample` builds per image, for a
    batch of RAW frames of different sizes, ON THE DEVICE -- vrnet_augment_frames_u8 (three launches: the float images),
    vrnet_augment_seg_targets_u8, vrnet_augment_box_targets_f32 and vrnet_augment_radar_f32.  frames / labels / sizes / boxes /
    capacity: as `device_train_batch_ragged` takes them; radar (B, 4, H, W) float32, each map aligned with the letterbox window
    of its frame; params: an AUG_DTYPE table (`augment_params`, or `aug_record`s written by hand), validated here
    (`check_aug_table`); max_taps: `default_aug_max_taps`.  Returns (images (B,3,H,W) f32, png (B,H,W) int64, onehot
    (B,H,W,ns+1) f32, targets (B,max_gt,5) f32, counts (B) int32, radar (B,4,H,W) f32), bit for bit what the host functions
    give per image.  post: an AUG_POST_DTYPE table (`augment_post_params`, or `aug_post_record`s written by hand; validated
    here, `check_aug_post_table`) adds the blur and the rotation as `augment_sample(..., post=...)` applies them: the frames
    go through vrnet_augment_frames_u8 with the colour stage off and vrnet_augment_post_frames_u8, the labels and the radar
    maps through a nearest gather behind their kernels, the boxes through vrnet_augment_post_box_targets_f32; max_angle: the
    capacity of the rotation, at least the largest |angle| of the table."""
    from . import hip
    fn = "device_augment_batch_ragged"
    ops = (hip.augment_frames, hip.augment_seg_targets, hip.augment_box_targets, hip.augment_radar)
    if post is not None:
        ops = _post_ops(check_aug_post_table(post, input_shape, max_angle, len(boxes), fn), int(max_angle), device)
    return _device_batch_ragged(
        fn, frames, sizes, input_shape, labels, boxes, radar, num_classes_seg, max_gt, capacity, max_taps, flag, device,
        default_aug_max_taps, lambda own, shape, cap, taps: augment_bytes(check_aug_params(params, own, shape, cap, taps, fn)), ops)


def aug_without_color(aug):
    """A copy of the (B, hip.AUG_BYTES) device table with the colour stage of every record off: what vrnet_augment_frames_u8
    runs on when the post stage follows, which applies the colour behind the rotation."""
    out = aug.clone()
    out[:, 28:32] = 0                    # vrnet_aug_rec.color
    return out


def _post_ops(post, max_angle, device):
    """The four eager operations of `device_augment_batch_ragged` with a post table, in the call shapes of
    `_device_batch_ragged`'s ops."""
    from . import hip
    ptab = aug_post_bytes(post).to(torch.device(device))

    def frames_op(img, tab, H, W, max_taps, images, flag):
        canvas = torch.empty((len(tab), H, W, 3), dtype=torch.uint8, device=img.device)
        hip.augment_frames(img, aug_without_color(tab), H, W, max_taps, canvas=canvas, flag=flag)
        hip.augment_post_frames(canvas, tab, ptab, tuple(img.shape[1:3]), max_angle, images=images, flag=flag)

    def seg_op(lab, tab, H, W, ns, flag):
        png, onehot = hip.augment_seg_targets(lab, tab, H, W, ns, flag=flag)
        return hip.augment_post_seg_targets(png, ptab, ns, max_angle, onehot=onehot, flag=flag)

    def box_op(packed, counts, tab, capacity, H, W, flag):
        return hip.augment_post_box_targets(packed, counts, tab, ptab, capacity, H, W, max_angle, flag=flag)

    def radar_op(rad, tab, capacity, flag):
        return hip.augment_post_radar(hip.augment_radar(rad, tab, capacity, flag=flag), ptab, max_angle, flag=flag)
    return frames_op, seg_op, box_op, radar_op


def check_aug_params(params, sizes, input_shape, capacity, max_taps, fn):
    """An explicit augmentation table against the batch it is for: B records whose (ih, iw) are the frames' own, then
    `check_aug_table`.  Returns the table as a contiguous array."""
    tab = np.ascontiguousarray(params)
    if tab.dtype != AUG_DTYPE or tab.ndim != 1 or len(tab) != len(sizes):
        raise RuntimeError(f"{fn}: the augmentation table is a ({len(sizes)},) array of data.AUG_DTYPE records")
    for b, (ih, iw) in enumerate(np.asarray(sizes).tolist()):
        if (int(tab[b]["ih"]), int(tab[b]["iw"])) != (ih, iw):
            raise RuntimeError(f"{fn}: image {b}: the record is for {int(tab[b]['ih'])} x {int(tab[b]['iw'])}, the frame is {ih} x {iw}")
    return check_aug_table(tab, input_shape, capacity, max_taps, fn)


# ---- Mosaic (utils/dataloader.py:251-426: get_random_data_with_Mosaic, merge_bboxes), host side ----------------------------
# One output image is made from up to four source frames ("tiles"), each resized and pasted as the single-image augmentation
# does and shown only inside its quadrant of the canvas, which is cut at (cutx, cuty): tile 0 x < cutx, y < cuty; tile 1
# x < cutx, y >= cuty; tile 2 x >= cutx, y >= cuty; tile 3 x >= cutx, y < cuty (:393-397).  The reference never reaches this code
# (__getitem__ does not call it) and moves neither the label map nor the radar map; here one record per output image drives
# all four parts, and the functions below are the truth the kernels of csrc/mosaic.hip are held to.  Two deliberate
# departures from the reference:
#   it flips a tile only when the tile has boxes (:329), an accident of its box code; here the flip applies to every tile,
#     because the label map and the radar map need it whether or not there are boxes
#   it keeps boxes that the cut has reduced to zero or one pixel; here a second w > 1 and h > 1 test drops them: such a
#     target costs a row of max_gt and enters SimOTA with no valid centre
# Its in-place np.random.shuffle of the boxes (:372) is left out, as in `augment_boxes`.
# vrnet_mosaic_tile / vrnet_mosaic_rec of include/vrnet_hip.h: 48 bytes per tile, one record per OUTPUT image (976 bytes)
MOSAIC_TILE_DTYPE = np.dtype([(n, "<i4") for n in ("src", "ih", "iw", "nw", "nh", "dx", "dy", "flip", "lb_nw", "lb_nh", "lb_dx",
                                                   "lb_dy")])
MOSAIC_DTYPE = np.dtype([(n, "<i4") for n in ("cutx", "cuty", "color", "reserved")] + [("tile", MOSAIC_TILE_DTYPE, (4,)),
                                                                                       ("lut", "u1", (3, 256))])


def mosaic_record(input_shape, cut, tiles, color=False, gains=(1.0, 1.0, 1.0)):
    """One MOSAIC_DTYPE record written out by hand: cut = (cutx, cuty); tiles: four entries in the reference's tile order, each
    None (no tile: src = -1) or (src, (ih, iw), nw, nh, dx, dy[, flip]) -- the source slot, that source's own size, the resized
    window and where it is pasted, and whether the SOURCE is mirrored left-right before the resize; the letterbox window of
    each source is filled in; the tables are `aug_luts(gains)`.  Not validated: `check_mosaic_table` does that."""
    H, W = (int(v) for v in input_shape)
    rec = np.zeros((), MOSAIC_DTYPE)
    rec["cutx"], rec["cuty"], rec["color"] = int(cut[0]), int(cut[1]), int(bool(color))
    rec["tile"]["src"] = -1
    if len(tiles) != 4:
        raise RuntimeError(f"mosaic_record: four tiles (None: no tile), got {len(tiles)}")
    for t, tile in enumerate(tiles):
        if tile is None:
            continue
        src, (ih, iw), nw, nh, dx, dy = tile[:6]
        lb = letterbox_geometry(max(int(iw), 1), max(int(ih), 1), W, H)
        rec["tile"][t] = (int(src), int(ih), int(iw), int(nw), int(nh), int(dx), int(dy), int(bool(tile[6])) if len(tile) > 6 else 0) + lb
    rec["lut"] = aug_luts(gains)
    return rec


def mosaic_bytes(table):
    """A MOSAIC_DTYPE table as the (B, hip.MOSAIC_BYTES) uint8 host tensor the device takes; it shares the table's memory."""
    return torch.from_numpy(table.view(np.uint8).reshape(len(table), -1))


def check_mosaic_table(table, input_shape, sizes, capacity=None, max_taps=None, fn="mosaic_params"):
    """Raises RuntimeError naming the output image, and the tile where one is at fault, for a record the kernels would have
    to clamp: a cut outside 0 <= cutx <= W, 0 <= cuty <= H, a src outside -1 .. S - 1 (sizes (S, 2) = (ih, iw) of the sources),
    a tile whose ih, iw are not its source's own, and per present tile what `check_aug_table` checks.  A tile with src = -1
    is no tile and the rest of its head is not looked at.  Host only.  Returns the table as a contiguous array."""
    H, W = (int(v) for v in input_shape)
    own = frame_sizes(sizes, fn=fn)
    table = np.ascontiguousarray(table)
    if table.dtype != MOSAIC_DTYPE or table.ndim != 1:
        raise RuntimeError(f"{fn}: the Mosaic table is a (B,) array of data.MOSAIC_DTYPE records")
    for b, rec in enumerate(table):
        cutx, cuty = int(rec["cutx"]), int(rec["cuty"])
        if not (0 <= cutx <= W and 0 <= cuty <= H):
            raise RuntimeError(f"{fn}: image {b}: the cut ({cutx}, {cuty}) is outside a {H} x {W} input")
        for t, tile in enumerate(rec["tile"]):
            src = int(tile["src"])
            if src == -1:
                continue
            where = f"image {b}, tile {t}"
            if not 0 <= src < len(own):
                raise RuntimeError(f"{fn}: {where}: source {src} of {len(own)} sources")
            if (int(tile["ih"]), int(tile["iw"])) != tuple(own[src].tolist()):
                raise RuntimeError(f"{fn}: {where}: the record is for {int(tile['ih'])} x {int(tile['iw'])}, source {src} is "
                                   f"{own[src][0]} x {own[src][1]}")
            check_window(tile, (H, W), capacity, max_taps, where, fn)
    return table


def merge_boxes(box_lists, cutx, cuty):
    """`merge_bboxes` of utils/dataloader.py:251-295 verbatim, with its asymmetric > and >= tests: box_lists, four arrays of
    rows x1, y1, x2, y2, cls on the canvas, one per tile -> the rows each tile keeps, cut at (cutx, cuty), tile by tile."""
    merged = []
    for i in range(len(box_lists)):
        for box in box_lists[i]:
            x1, y1, x2, y2 = box[0], box[1], box[2], box[3]
            if i == 0:
                if y1 > cuty or x1 > cutx:
                    continue
                if y2 >= cuty and y1 <= cuty:
                    y2 = cuty
                if x2 >= cutx and x1 <= cutx:
                    x2 = cutx
            if i == 1:
                if y2 < cuty or x1 > cutx:
                    continue
                if y2 >= cuty and y1 <= cuty:
                    y1 = cuty
                if x2 >= cutx and x1 <= cutx:
                    x2 = cutx
            if i == 2:
                if y2 < cuty or x2 < cutx:
                    continue
                if y2 >= cuty and y1 <= cuty:
                    y1 = cuty
                if x2 >= cutx and x1 <= cutx:
                    x1 = cutx
            if i == 3:
                if y1 > cuty or x2 < cutx:
                    continue
                if y2 >= cuty and y1 <= cuty:
                    y2 = cuty
                if x2 >= cutx and x1 <= cutx:
                    x1 = cutx
            merged.append([x1, y1, x2, y2, box[-1]])
    return np.array(merged, dtype=np.float64).reshape(-1, 5)


def mosaic_boxes(box_lists, sizes, input_shape, rec):
    """The boxes of one Mosaic image: box_lists and sizes are those of the S SOURCES, indexed by the tiles' src.  Tile by tile
    in order 0..3, the source's rows in their order: integer storage as `augment_boxes`; x1, x2 = iw - x2, iw - x1 when the
    tile flips (:331); x = x * nw / iw + dx, y = y * nh / ih + dy truncated toward zero; the clip to the canvas; kept when w > 1 and
    h > 1 (:371-382, minus the in-place shuffle); then `merge_boxes` at the record's cut; then a second w > 1 and h > 1 test
    (this project's: the reference keeps what the cut reduced to a line).  Returns (n, 5) float64 rows x1, y1, x2, y2, cls."""
    h, w = (int(v) for v in input_shape)
    per_tile = []
    for tile in rec["tile"]:
        src = int(tile["src"])
        out = np.zeros((0, 5), np.int64)
        if src >= 0 and box_lists[src] is not None:
            out = np.array(box_lists[src], dtype=np.int64).reshape(-1, 5)
        if out.shape[0]:
            ih, iw = (int(v) for v in sizes[src])
            nw, nh, dx, dy = (int(tile[k]) for k in ("nw", "nh", "dx", "dy"))
            if int(tile["flip"]):
                out[:, [0, 2]] = iw - out[:, [2, 0]]
            out[:, [0, 2]] = out[:, [0, 2]] * nw / iw + dx
            out[:, [1, 3]] = out[:, [1, 3]] * nh / ih + dy
            out[:, 0:2][out[:, 0:2] < 0] = 0
            out[:, 2][out[:, 2] > w] = w
            out[:, 3][out[:, 3] > h] = h
            out = out[((out[:, 2] - out[:, 0]) > 1) & ((out[:, 3] - out[:, 1]) > 1)]
        per_tile.append(out.astype(np.float64))
    merged = merge_boxes(per_tile, int(rec["cutx"]), int(rec["cuty"]))
    return merged[((merged[:, 2] - merged[:, 0]) > 1) & ((merged[:, 3] - merged[:, 1]) > 1)]


def mosaic_sample(images, labels, boxes, radars, input_shape, rec):
    """One Mosaic dataset item under the record rec (`mosaic_params`), on PIL images and numpy arrays; images, labels, boxes
    and radars are those of the S SOURCES, indexed by the tiles' src; returns (canvas, boxes, label canvas, radar).  Per
    tile, inside its quadrant: the image is (source, FLIP_LEFT_RIGHT when the tile flips).resize((nw, nh), BICUBIC) pasted
    at (dx, dy) on grey (128); the label the same with NEAREST on 0 -- flip first, then resize, the reference's order
    (:328-344), which matters: Pillow's NEAREST recurrence is not mirror-symmetric; the radar (each map (4, H, W) aligned with
    the letterbox window of its source) is `augment_radar`'s integer gather per tile, this project's definition: with wx = x -
    dx, wy = y - dy and wx' = nw - 1 - wx when the tile flips, radar[c, lb_dy + ((2 wy + 1) lb_nh) // (2 nh), lb_dx + ((2 wx' + 1)
    lb_nw) // (2 nw)] inside the window, 0 outside.  `hsv_jitter` then runs over the whole canvas when the record's colour
    stage is on (:404-419).  Boxes: `mosaic_boxes`.  Unlike the reference (:329) the flip does not depend on the tile having
    boxes."""
    from PIL import Image
    h, w = (int(v) for v in input_shape)
    cutx, cuty = int(rec["cutx"]), int(rec["cuty"])
    canvas = np.full((h, w, 3), 128, np.uint8)
    label = np.zeros((h, w), np.uint8)
    radar = np.zeros((4, h, w), np.asarray(radars[0]).dtype)
    for t, tile in enumerate(rec["tile"]):
        src = int(tile["src"])
        if src < 0:
            continue
        ys = slice(cuty, h) if t in (1, 2) else slice(0, cuty)
        xs = slice(cutx, w) if t in (2, 3) else slice(0, cutx)
        nw, nh, dx, dy, lnw, lnh, ldx, ldy = (int(tile[k]) for k in ("nw", "nh", "dx", "dy", "lb_nw", "lb_nh", "lb_dx", "lb_dy"))
        image, lab = images[src].convert("RGB"), Image.fromarray(np.array(labels[src]))
        if int(tile["flip"]):
            image, lab = image.transpose(Image.FLIP_LEFT_RIGHT), lab.transpose(Image.FLIP_LEFT_RIGHT)
        new_image = Image.new("RGB", [w, h], (128, 128, 128))
        new_image.paste(image.resize((nw, nh), Image.BICUBIC), (dx, dy))
        new_label = Image.new("L", [w, h], (0))
        new_label.paste(lab.resize((nw, nh), Image.NEAREST), (dx, dy))
        canvas[ys, xs] = np.array(new_image)[ys, xs]
        label[ys, xs] = np.array(new_label)[ys, xs]
        wx, wy = np.arange(w, dtype=np.int64) - dx, np.arange(h, dtype=np.int64) - dy
        okx, oky = (wx >= 0) & (wx < nw), (wy >= 0) & (wy < nh)
        if int(tile["flip"]):
            wx = nw - 1 - wx
        sx = ldx + ((2 * np.where(okx, wx, 0) + 1) * lnw) // (2 * nw)
        sy = ldy + ((2 * np.where(oky, wy, 0) + 1) * lnh) // (2 * nh)
        stored = np.asarray(radars[src])
        moved = np.where((oky[:, None] & okx[None, :])[None], stored[:, sy[:, None], sx[None, :]], np.zeros((), stored.dtype))
        radar[:, ys, xs] = moved[:, ys, xs]
    if int(rec["color"]):
        canvas = hsv_jitter(canvas, rec["lut"])
    sizes = [(im.size[1], im.size[0]) for im in images]
    return Image.fromarray(canvas), mosaic_boxes(boxes, sizes, input_shape, rec), Image.fromarray(label), radar


def default_mosaic_max_taps(capacity, input_shape, jitter=.3, scale=(.4, 1), prob=1.0, plain=None):
    """The tap capacity a Mosaic pipeline reserves per table entry: `default_aug_max_taps` at the Mosaic draw's scale[0] = .4
    (a tile is never enlarged, and never shrunk below .4 of the canvas on its leading axis), or with prob < 1 the larger of
    that and what the plain draw (keywords plain) needs."""
    taps = default_aug_max_taps(capacity, input_shape, jitter, scale)
    if prob < 1:
        taps = max(taps, default_aug_max_taps(capacity, input_shape, **{k: v for k, v in (plain or {}).items() if k in ("jitter", "scale")}))
    return taps


def mosaic_params(sizes, input_shape, rng, batch, prob=1.0, jitter=.3, hue=.1, sat=.7, val=.4, scale=(.4, 1), cut=(.3, .7), flip=.5,
                  color=True, plain=None, capacity=None, max_taps=None, fn="mosaic_params"):
    """The random draw of Mosaic, one MOSAIC_DTYPE record per OUTPUT image (`mosaic_bytes` of the table is what the device
    takes): sizes (4 * batch, 2) = (ih, iw) per source, output image b uses sources 4 b .. 4 b + 3; rng a numpy.random.RandomState
    or a seed.  Per output image one rand() for mosaic = rand() < prob -- always drawn, so the stream does not depend on prob
    (train.py:108-112: `mosaic_prob`; the `special_aug_ratio` policy is the caller's choice of prob per epoch).
    If mosaic, in the order of utils/dataloader.py:299-360 and :404: min_offset_x, then min_offset_y = rand(cut[0], cut[1]); per
    tile the flip (rand() < flip), the two rand() of new_ar = iw / ih * rand(1 - jitter, 1 + jitter) / rand(1 - jitter, 1 + jitter),
    then scale = rand(scale[0], scale[1]), nh = int(scale * h), nw = int(nh * new_ar) when new_ar < 1, else nw = int(scale * w), nh =
    int(nw / new_ar); with cutx = int(w * min_offset_x), cuty = int(h * min_offset_y) the placement (dx, dy) = (cutx - nw, cuty -
    nh), (cutx - nw, cuty), (cutx, cuty), (cutx, cuty - nh) for tiles 0..3; then uniform(-1, 1, 3) * [hue, sat, val] + 1 for the gains
    (drawn with color=False too).
    If not mosaic, the `augment_params` draw runs for source 4 b with the keywords in plain and is written as a record with
    cut = (w, h), tile 0 only and src = -1 for tiles 1-3; a flipping draw mirrors the SOURCE, as every Mosaic tile does, and its
    window goes to dx' = w - dx - nw, which is where a mirror of the canvas puts it.  The three unused sources of such an image
    still cost their copies into the slots: the batch layout is fixed at four sources per output image.
    Host only.  Raises RuntimeError naming the image (and tile) for what `check_mosaic_table` checks."""
    arr = frame_sizes(sizes, 4 * int(batch), fn)
    H, W = (int(v) for v in input_shape)
    rs = rng if isinstance(rng, np.random.RandomState) else np.random.RandomState(rng)

    def rand(a=0.0, b=1.0):
        return rs.rand() * (b - a) + a
    for s, (ih, iw) in enumerate(arr.tolist()):            # what no draw can mend is raised before the generator moves
        if ih <= 0 or iw <= 0:
            raise RuntimeError(f"{fn}: image {s // 4}, tile {s % 4}: bad size {ih} x {iw}")
        if capacity is not None and (ih > capacity[0] or iw > capacity[1]):
            raise RuntimeError(f"{fn}: image {s // 4}, tile {s % 4}: {ih} x {iw} is above the capacity {capacity[0]} x {capacity[1]}")
    tab = np.zeros(int(batch), MOSAIC_DTYPE)
    for b in range(int(batch)):
        if rand() < prob:
            cutx, cuty = int(W * rand(cut[0], cut[1])), int(H * rand(cut[0], cut[1]))
            tiles = []
            for t in range(4):
                ih, iw = arr[4 * b + t].tolist()
                flipped = rand() < flip
                new_ar = iw / ih * rand(1 - jitter, 1 + jitter) / rand(1 - jitter, 1 + jitter)
                sc = rand(scale[0], scale[1])
                if new_ar < 1:
                    nh = int(sc * H)
                    nw = int(nh * new_ar)
                else:
                    nw = int(sc * W)
                    nh = int(nw / new_ar)
                dx = cutx - nw if t < 2 else cutx
                dy = cuty - nh if t in (0, 3) else cuty
                tiles.append((4 * b + t, (ih, iw), nw, nh, dx, dy, flipped))
            gains = rs.uniform(-1, 1, 3) * [hue, sat, val] + 1
            tab[b] = mosaic_record((H, W), (cutx, cuty), tiles, color, gains)
        else:
            a = augment_params(arr[4 * b:4 * b + 1], (H, W), rs, capacity=capacity, max_taps=max_taps, fn=fn, **(plain or {}))[0]
            nw, dx = int(a["nw"]), int(a["dx"])
            tile = (4 * b, (int(a["ih"]), int(a["iw"])), nw, int(a["nh"]), W - dx - nw if int(a["flip"]) else dx, int(a["dy"]),
                    int(a["flip"]))
            tab[b] = mosaic_record((H, W), (W, H), [tile, None, None, None], int(a["color"]))
            tab[b]["lut"] = a["lut"]
    return check_mosaic_table(tab, (H, W), arr, capacity, max_taps, fn)


def device_mosaic_batch_ragged(frames, sizes, input_shape, labels, boxes, radar, num_classes_seg, params, max_gt=64,
                               capacity=None, max_taps=None, flag=None, device="cuda"):
    """`device_augment_batch_ragged` under Mosaic: the dataset item `mosaic_sample` builds per OUTPUT image from S raw source
    frames of different sizes, ON THE DEVICE -- vrnet_mosaic_frames_u8 (three launches: the float images),
    vrnet_mosaic_seg_targets_u8, vrnet_mosaic_box_targets_f32 and vrnet_mosaic_radar_f32.  frames / labels / sizes / boxes /
    capacity: those of the S sources, as `device_augment_batch_ragged` takes them; radar (S, 4, H, W) float32, each map aligned
    with the letterbox window of its source; params: a (B,) MOSAIC_DTYPE table (`mosaic_params`, or `mosaic_record`s written by
    hand), validated here (`check_mosaic_table`); max_taps: `default_mosaic_max_taps` with prob < 1.  Returns (images (B,3,H,W)
    f32, png (B,H,W) int64, onehot (B,H,W,ns+1) f32, targets (B,max_gt,5) f32, counts (B) int32, radar (B,4,H,W) f32), bit for
    bit what the host functions give per output image -- as long as every image keeps at most max_gt boxes; of more, the
    first max_gt stay and flag receives hip.FLAG_BOX_COUNT."""
    from . import hip
    fn = "device_mosaic_batch_ragged"
    return _device_batch_ragged(
        fn, frames, sizes, input_shape, labels, boxes, radar, num_classes_seg, max_gt, capacity, max_taps, flag, device,
        lambda cap, shape: default_mosaic_max_taps(cap, shape, prob=0.0),
        lambda own, shape, cap, taps: mosaic_bytes(check_mosaic_table(params, shape, own, cap, taps, fn)),
        (hip.mosaic_frames, hip.mosaic_seg_targets, hip.mosaic_box_targets, hip.mosaic_radar), per="{} sources")


class FrameDataset(torch.utils.data.Dataset):
    """The decode-only dataset in front of `graph.TrainStep(from_frames=True)`: item i is what YoloDataset reads from disk
    for annotation line i (dataloader.py:73-80, 111-129) and nothing more -- no resize, no box mapping, no one-hot:
    (frame (ih, iw, 3) uint8 RGB, radar (4, H, W) float32 as stored, boxes (n, 5) int64 in original pixels, label (ih, iw)
    uint8, (ih, iw)).  The JPEG is the first field of the line; its frame id (`frame_id`) names
    seg_dataset_path/VOC2007/SegmentationClass/<id>.png and radar_root/<id>.npz.  A label map of another size than its
    frame raises: the device letterbox resizes both by one geometry record."""

    def __init__(self, annotation_lines, seg_dataset_path, radar_root):
        self.annotation_lines = list(annotation_lines)
        self.seg_dataset_path, self.radar_root = seg_dataset_path, radar_root

    def __len__(self):
        return len(self.annotation_lines)

    def __getitem__(self, index):
        from PIL import Image
        line = self.annotation_lines[index % len(self.annotation_lines)]
        fid = frame_id(line)
        path, boxes = parse_annotation_line(line)
        frame = np.array(Image.open(path).convert("RGB"), dtype=np.uint8)
        label = np.array(Image.open(os.path.join(self.seg_dataset_path, "VOC2007/SegmentationClass", fid + ".png")))
        if label.ndim != 2 or label.dtype != np.uint8:
            raise RuntimeError(f"FrameDataset: {fid}.png: expected a single-channel 8-bit label map, got {label.dtype} {label.shape}")
        if label.shape != frame.shape[:2]:
            raise RuntimeError(f"FrameDataset: {fid}: the label map is {label.shape}, the frame {frame.shape[:2]}")
        radar = np.asarray(load_radar(self.radar_root, fid), dtype=np.float32)
        return frame, radar, boxes.astype(np.int64), label, frame.shape[:2]


def frames_collate(batch):
    """Items of `FrameDataset` -> the arguments of `TrainStep(from_frames=True)`'s call: (frames: list of (ih_b, iw_b, 3)
    uint8 tensors, radar (B, 4, H, W) float32, boxes: list of (n_b, 5) int64 arrays, labels: list of (ih_b, iw_b) uint8
    tensors, sizes (B, 2) int64 array).  Host only."""
    frames, radars, boxes, labels, sizes = zip(*batch)
    return ([torch.from_numpy(np.ascontiguousarray(f)) for f in frames], torch.from_numpy(np.stack(radars)).float(),
            list(boxes), [torch.from_numpy(np.ascontiguousarray(l)) for l in labels], np.array(sizes, np.int64).reshape(-1, 2))


def device_radar(radar, normalise=True, device="cuda", out=None):
    """The radar half of the prediction scripts ON THE DEVICE (vrnet_radar_normalise): radar (B, 4, H, W) float32 or
    float64 maps (a single (4, H, W) frame counts as B = 1), numpy array or tensor -> (B, 4, H, W) float32 on the device.
    normalise=True: each frame through `preprocess_input_radar` (its global min and max over all four channels, as
    yolo.py:134 calls it per frame), bit-identical to `preprocess_input_radar(frame).astype(float32)` -- the arithmetic
    runs in the maps' own type, as numpy's does; a constant frame is NaN in both.  normalise=False: the plain cast
    (deeplab.py and the dataloader feed the maps raw).  Two launches, no host synchronisation."""
    from . import hip
    t = radar if torch.is_tensor(radar) else torch.from_numpy(np.ascontiguousarray(radar))
    if t.dtype not in (torch.float32, torch.float64):
        raise RuntimeError(f"device_radar: expected float32 or float64 maps, got {t.dtype}")
    t = t[None] if t.dim() == 3 else t
    if t.dim() != 4 or t.numel() == 0:
        raise RuntimeError(f"device_radar: expected maps of shape (B, 4, H, W) or (4, H, W), got {tuple(t.shape)}")
    t = t.to(device, non_blocking=True).contiguous()
    with torch.cuda.device(t.device):
        if out is None:
            out = torch.empty(t.shape, dtype=torch.float32, device=t.device)
        hip.radar_normalise(t, out, normalise)
    return out


# ---- the radar map from 4D radar points: host statement of csrc/radarmap.hip ---------------------------------------------
# The reference's data instructions ask for "the radar map with the spatial size of images" from projected point clouds and
# ship no code for it; the rule below is this project's definition, as `augment_radar` is.  `radar_map` is the truth the
# kernels are held to, bit for bit.
# vrnet_radar_view of include/vrnet_hip.h, one record per image (80 bytes)
RADAR_VIEW_DTYPE = np.dtype([(n, "<i4") for n in ("ih", "iw", "nw", "nh", "dx", "dy", "flip", "count")] + [("P", "<f4", (12,))])
RADAR_MAX_RADIUS = 8


def check_radar_rule(radius, min_depth, fn="radar_map"):
    """radius as an int in 0..RADAR_MAX_RADIUS and min_depth as a positive finite float32, or a RuntimeError."""
    if isinstance(radius, bool) or not isinstance(radius, (int, np.integer)) or not 0 <= int(radius) <= RADAR_MAX_RADIUS:
        raise RuntimeError(f"{fn}: radius must be an integer in 0..{RADAR_MAX_RADIUS}, got {radius!r}")
    try:
        md = np.float32(min_depth)
    except (TypeError, ValueError):
        md = np.float32("nan")
    if not (md > 0 and np.isfinite(md)):
        raise RuntimeError(f"{fn}: min_depth must be a positive finite number, got {min_depth!r}")
    return int(radius), md


def check_calib(calib, batch, fn="radar_views"):
    """calib (3, 4) or (B, 3, 4), any real type -> (B, 3, 4) float32."""
    try:
        P = np.asarray(calib.detach().cpu().numpy() if torch.is_tensor(calib) else calib, dtype=np.float32)
    except (TypeError, ValueError):
        P = None
    if P is None or P.shape not in ((3, 4), (batch, 3, 4)):
        raise RuntimeError(f"{fn}: calib is a (3, 4) projection or one per image ({batch}, 3, 4), got "
                           f"{None if P is None else P.shape}")
    return np.ascontiguousarray(np.broadcast_to(P, (batch, 3, 4)))


def radar_views(table, calib, counts):
    """The packed per-image table of `hip.radar_map`: a `frame_geometry` table OR an `augment_params` table (both carry ih, iw,
    nw, nh, dx, dy; only the latter has flip), calib (3, 4) or (B, 3, 4), counts (B) points per image -> a (B,)
    RADAR_VIEW_DTYPE array (`radar_view_bytes` of it is what the device takes).  Host only."""
    table = np.asarray(table)
    if table.ndim != 1 or table.dtype not in (GEOM_DTYPE, AUG_DTYPE):
        raise RuntimeError("radar_views: the table is a (B,) array of data.GEOM_DTYPE or data.AUG_DTYPE records")
    B = len(table)
    P = check_calib(calib, B)
    counts = np.asarray(counts.cpu().numpy() if torch.is_tensor(counts) else counts)
    if counts.shape != (B,) or not np.issubdtype(counts.dtype, np.integer):
        raise RuntimeError(f"radar_views: counts are {B} integers, got {counts.dtype} {counts.shape}")
    out = np.zeros(B, RADAR_VIEW_DTYPE)
    for k in ("ih", "iw", "nw", "nh", "dx", "dy"):
        out[k] = table[k]
    if table.dtype == AUG_DTYPE:
        out["flip"] = table["flip"] != 0
    out["count"] = counts
    out["P"] = P.reshape(B, 12)
    return out


def radar_view_bytes(views):
    """A `radar_views` table as the (B, hip.RADAR_VIEW_BYTES) uint8 host tensor the device takes; it shares the table's memory."""
    return torch.from_numpy(views.view(np.uint8).reshape(len(views), -1))


def pack_points(points, max_points, where=None):
    """B arrays of (n_b, 7) float32 rows x, y, z, f0, f1, f2, f3 (None or empty: no points), or a pair (padded (B, n, 7)
    float32 array, counts (B) integers) -> the pinned host pair (B, max_points, 7) float32 and (B,) int32 that `hip.radar_map`
    takes after one non-blocking copy (the counts travel in the view table); unused rows are zero.  Raises RuntimeError naming
    the image for more than max_points rows, a type other than float32 and a wrong shape -- before anything is written.
    where: index -> the name of that point set in a message (default "image b"; the sources of a Mosaic are "image b, tile t")."""
    where = where or (lambda b: f"image {b}")
    max_points = int(max_points)
    if max_points < 1:
        raise RuntimeError(f"pack_points: max_points must be positive, got {max_points}")

    def host(a):
        return a.detach().cpu().numpy() if torch.is_tensor(a) else np.asarray(a)
    if isinstance(points, tuple) and len(points) == 2 and not isinstance(points[0], (list, tuple)) and \
            getattr(points[0], "ndim", 0) == 3:
        padded, cnt = host(points[0]), host(points[1])
        if padded.dtype != np.float32 or padded.shape[2] != 7:
            raise RuntimeError(f"pack_points: a padded buffer is float32 of shape (B, n, 7), got {padded.dtype} {padded.shape}")
        if cnt.shape != (padded.shape[0],) or not np.issubdtype(cnt.dtype, np.integer):
            raise RuntimeError(f"pack_points: counts are {padded.shape[0]} integers, got {cnt.dtype} {cnt.shape}")
        for b, n in enumerate(cnt.tolist()):
            if not 0 <= n <= padded.shape[1]:
                raise RuntimeError(f"pack_points: {where(b)}: counts says {n} points, the padded buffer holds {padded.shape[1]}")
        points = [padded[b, :n] for b, n in enumerate(cnt.tolist())]
    elif not isinstance(points, (list, tuple)):
        raise RuntimeError("pack_points: expected a list of (n, 7) float32 arrays, or a pair (padded (B, n, 7) array, counts)")
    rows = []
    for b, a in enumerate(points):
        if a is None:
            rows.append(None)
            continue
        a = host(a)
        if a.size == 0:
            rows.append(None)
            continue
        if a.dtype != np.float32:
            raise RuntimeError(f"pack_points: {where(b)}: points are float32 rows x, y, z, f0, f1, f2, f3, got {a.dtype}")
        if a.ndim != 2 or a.shape[1] != 7:
            raise RuntimeError(f"pack_points: {where(b)}: expected (n, 7) rows x, y, z, f0, f1, f2, f3, got {a.shape}")
        if a.shape[0] > max_points:
            raise RuntimeError(f"pack_points: {where(b)} has {a.shape[0]} points, above max_points = {max_points}")
        rows.append(a)
    B = len(rows)
    out = torch.zeros((B, max_points, 7), dtype=torch.float32)
    counts = torch.zeros(B, dtype=torch.int32)
    if torch.cuda.is_available():
        out, counts = out.pin_memory(), counts.pin_memory()
    for b, a in enumerate(rows):
        if a is not None:
            out[b, :len(a)] = torch.from_numpy(np.ascontiguousarray(a))
            counts[b] = len(a)
    return out, counts


def radar_project(points, P, size, window, min_depth=0.1):
    """The per-point half of `radar_map`, in float32: (kept (n) bool, ix (n) int64, iy (n) int64, hw (n) float32) -- the window
    pixel of every point and its depth; ix, iy are 0 where a point is not kept."""
    f32 = np.float32
    md = check_radar_rule(0, min_depth)[1]
    pts, P = np.asarray(points), np.asarray(P)
    if pts.ndim != 2 or pts.shape[1] != 7 or pts.dtype != np.float32:
        raise RuntimeError(f"radar_map: points are (n, 7) float32 rows x, y, z, f0, f1, f2, f3, got {pts.dtype} {pts.shape}")
    if P.shape != (3, 4) or P.dtype != np.float32:
        raise RuntimeError(f"radar_map: P is a (3, 4) float32 projection, got {P.dtype} {P.shape}")
    ih, iw = (int(v) for v in size)
    nw, nh = int(window[0]), int(window[1])
    x, y, z = pts[:, 0], pts[:, 1], pts[:, 2]
    with np.errstate(all="ignore"):
        hu, hv, hw = (((P[r, 0] * x + P[r, 1] * y) + P[r, 2] * z) + P[r, 3] for r in range(3))
        ok = (hw >= md) & np.isfinite(hw) & np.isfinite(hu) & np.isfinite(hv)
        den = np.where(ok, hw, f32(1))
        fx = ((hu / den) * f32(nw)) / f32(iw)
        fy = ((hv / den) * f32(nh)) / f32(ih)
        assert hw.dtype == f32 and fx.dtype == f32 and fy.dtype == f32
        ok &= (fx >= 0) & (fx < f32(nw)) & (fy >= 0) & (fy < f32(nh))
    ix = np.where(ok, np.floor(fx), 0).astype(np.int64)
    iy = np.where(ok, np.floor(fy), 0).astype(np.int64)
    return ok, ix, iy, hw


def radar_map(points, P, size, input_shape, window, flip=False, radius=0, min_depth=0.1, post=None):
    """The network's radar input (4, H, W) float32 of ONE image from its radar points -- this project's own definition, the
    reference has none.  points (n, 7) float32 rows x, y, z, f0, f1, f2, f3: the position in the radar's frame and the four
    features in the order of the map's channels (the reference names range, velocity, elevation and power).  P (3, 4)
    float32 maps (x, y, z, 1) to homogeneous CONTINUOUS pixel coordinates of the original frame of size = (ih, iw), source
    pixel (i, j) covering [i, i + 1) x [j, j + 1); a calibration in OpenCV's convention (pixel centres on integers) adds half
    of row 2 to rows 0 and 1 first.  window = (nw, nh, dx, dy) on the input_shape = (H, W) canvas is the one the frame went
    through: `letterbox_geometry`'s, (W, H, 0, 0) for letterbox_image=False, or the nw, nh, dx, dy and flip of an augmentation
    record (larger than the canvas and negative offsets included).  Everything in float32, every operation rounded on its
    own, in this order:
        hu = ((P00 x + P01 y) + P02 z) + P03, hv and hw likewise from rows 1 and 2
        kept when hw >= min_depth and hw, hu, hv are finite (a NaN anywhere rejects)
        u = hu / hw, v = hv / hw; fx = (u float(nw)) / float(iw), fy = (v float(nh)) / float(ih)
        kept when 0 <= fx < nw and 0 <= fy < nh; ix = floor(fx), iy = floor(fy)
        X = W - 1 - dx - ix when flip, else dx + ix; Y = dy + iy        (the whole canvas is mirrored, as `augment_radar` does)
    A kept point covers the pixels (X + ox, Y + oy), |ox|, |oy| <= radius (0..8), inside the canvas and inside the window's
    extent on the canvas (mirrored under flip): nothing is written outside the window.  Of the points covering a pixel the
    one with the smallest hw wins, the lowest index among equal hw; out[c, Y, X] = f_c of the winner, copied bit for bit, 0
    where no point lands.  The min-max normalisation of the prediction scripts stays `device_radar(normalise=True)`.
    post: one AUG_POST_DTYPE record (`augment_post_params`, `aug_post_record`) or None.  Only its rotation is looked at; None
    or rotate == 0 changes nothing above.  When it rotates, the CENTRE (X, Y) of a kept point goes through fwd in float64,
    every operation rounded on its own, left to right as `rotate_boxes` does:
        rx = (fwd[0] X + fwd[1] Y) + fwd[2], ry = (fwd[3] X + fwd[4] Y) + fwd[5]
        X' = floor(rx + 0.5), Y' = floor(ry + 0.5)      (pixel centres on integers, the rounding of `warp_coords`' nearest walk)
    A point whose (X', Y') is outside the canvas is dropped.  Otherwise the rectangle the point covers WITHOUT the rotation --
    already cut to the canvas and to the window's extent, mirrored under flip -- is translated by (X' - X, Y' - Y) and cut to
    the canvas once more.  The square is not rotated and neither is the window's border; the winner of a pixel is chosen as
    above.  Every point moves exactly once: `rotate_nearest` of a finished map drops some isolated pixels and doubles others.
    The record is taken as it is (the host check is `check_aug_post_table`, the caller's)."""
    radius = check_radar_rule(radius, min_depth)[0]
    fwd = [float(v) for v in np.asarray(post["fwd"]).reshape(6)] if post is not None and int(post["rotate"]) else None
    H, W = (int(v) for v in input_shape)
    ih, iw = (int(v) for v in size)
    nw, nh, dx, dy = (int(v) for v in window)
    pts = np.ascontiguousarray(points)
    out = np.zeros((4, H, W), np.uint32)
    if min(ih, iw, nw, nh) <= 0:
        return out.view(np.float32)
    ok, ix, iy, hw = radar_project(pts, P, (ih, iw), (nw, nh), min_depth)
    bits = np.ascontiguousarray(pts[:, 3:7]).view(np.uint32)
    depth = hw.view(np.uint32)
    best = np.full((H, W), np.iinfo(np.uint64).max, np.uint64)
    for i in np.flatnonzero(ok).tolist():
        cx, cy = dx + int(ix[i]), dy + int(iy[i])
        x0, x1 = max(cx - radius, 0, dx), min(cx + radius, W - 1, dx + nw - 1)
        y0, y1 = max(cy - radius, 0, dy), min(cy + radius, H - 1, dy + nh - 1)
        if x0 > x1 or y0 > y1:
            continue
        key = np.uint64((int(depth[i]) << 32) | i)
        if flip:                                 # the columns of the finished canvas
            x0, x1 = W - 1 - x1, W - 1 - x0
        if fwd is not None:
            X, Y = W - 1 - cx if flip else cx, cy
            rx = (fwd[0] * float(X) + fwd[1] * float(Y)) + fwd[2]
            ry = (fwd[3] * float(X) + fwd[4] * float(Y)) + fwd[5]
            fx, fy = np.floor(rx + 0.5), np.floor(ry + 0.5)
            if not (0 <= fx < W and 0 <= fy < H):        # a NaN fails here too
                continue
            tx, ty = int(fx) - X, int(fy) - Y
            x0, x1, y0, y1 = max(x0 + tx, 0), min(x1 + tx, W - 1), max(y0 + ty, 0), min(y1 + ty, H - 1)
            if x0 > x1 or y0 > y1:
                continue
        xs = slice(x0, x1 + 1)
        won = best[y0:y1 + 1, xs] > key              # hw > 0 and finite: its bits order as an integer; the index breaks ties
        best[y0:y1 + 1, xs][won] = key
        for c in range(4):
            out[c, y0:y1 + 1, xs][won] = bits[i, c]
    return out.view(np.float32)


def device_radar_map(points, sizes, input_shape, calib, letterbox_image=True, radius=0, min_depth=0.1, max_points=None,
                     views=None, device="cuda", out=None, flag=None, post=None, max_angle=10):
    """`radar_map` for a batch ON THE DEVICE (vrnet_radar_map_f32, three launches): points as `pack_points` takes them, sizes
    (B, 2) = (ih, iw) of the original frames, calib (3, 4) or (B, 3, 4) -> (B, 4, H, W) float32 on the device, bit for bit what
    `radar_map` gives per image under the letterbox window of its frame (the whole canvas with letterbox_image=False).
    max_points: the capacity of the point buffer (default: the largest count).  views: a `radar_views` table to use instead
    (an augmentation's windows; its counts are replaced by the points' own); sizes and calib are then not read.  flag: an int32
    device word that receives hip.FLAG_GEOMETRY / hip.FLAG_POINT_COUNT (never, for a table this function built).  The
    points and the table are copied non_blocking; no host synchronisation.  post: an AUG_POST_DTYPE table, one record per
    image (validated here, `check_aug_post_table`, which names the image): the rotation of `radar_map(..., post=)` inside the
    point pass (vrnet_radar_map_post_f32, the same three launches); max_angle: at least the largest |angle| of the table."""
    from . import hip
    fn = "device_radar_map"
    radius, md = check_radar_rule(radius, min_depth, fn)
    H, W = (int(v) for v in input_shape)
    if max_points is None:
        if isinstance(points, tuple) and len(points) == 2 and getattr(points[0], "ndim", 0) == 3:
            max_points = max(int(points[0].shape[1]), 1)
        else:
            max_points = max([1] + [0 if a is None else len(a) for a in points])
    packed, counts = pack_points(points, max_points)
    B = len(counts)
    if views is None:
        table = frame_geometry(frame_sizes(sizes, B, fn), (H, W), letterbox_image, fn=fn)
        views = radar_views(table, calib, counts.numpy())
    else:
        views = np.array(views, copy=True)
        if views.dtype != RADAR_VIEW_DTYPE or views.shape != (B,):
            raise RuntimeError(f"{fn}: views is a ({B},) array of data.RADAR_VIEW_DTYPE records")
        views["count"] = counts.numpy()
    if post is not None:
        post = check_aug_post_table(post, (H, W), max_angle, B, fn)
    dev = torch.device(device)
    with torch.cuda.device(dev):
        if out is None:
            out = torch.empty((B, 4, H, W), dtype=torch.float32, device=dev)
        pts, vw = packed.to(dev, non_blocking=True), radar_view_bytes(views).to(dev, non_blocking=True)
        if post is None:
            hip.radar_map(pts, vw, H, W, radius, float(md), out, flag=flag)
        else:
            hip.radar_map_post(pts, vw, aug_post_bytes(post).to(dev, non_blocking=True), H, W, radius, float(md), int(max_angle), out,
                               flag=flag)
    return out


# ---- the radar readout of the detections: host statement of csrc/boxradar.hip ---------------------------------------------------
def check_box_shrink(shrink, fn="box_radar"):
    """shrink as a float32 in (0, 1], or a RuntimeError."""
    try:
        s = np.float32(shrink)
    except (TypeError, ValueError):
        s = np.float32("nan")
    if isinstance(shrink, bool) or not (s > 0 and s <= 1):
        raise RuntimeError(f"{fn}: shrink must lie in (0, 1], got {shrink!r}")
    return s


def box_radar(points, P, size, rows, min_depth=0.1, shrink=1.0):
    """What the radar says about every detection of ONE image -- this project's own definition, the reference has none:
    (count (m) int32, readout (m, 2, 5) float32).  points (n, 7) float32 rows x, y, z, f0, f1, f2, f3 and P (3, 4) float32 as
    `radar_map` takes them, size = (ih, iw) of the original frame, rows (m, >= 4) float32 whose first four columns are top,
    left, bottom, right in pixels of that frame (`FrameResult.rows`).  Boxes and projected points both live in the original
    frame, so no window takes part.  Everything in float32, every operation rounded on its own, in this order.  Per point i
    (the first three lines are `radar_project`'s):
        hu = ((P00 x + P01 y) + P02 z) + P03, hv and hw likewise from rows 1 and 2
        kept when hw >= min_depth and hw, hu, hv are finite (a NaN anywhere rejects)
        u = hu / hw, v = hv / hw; in view when 0 <= u < float(iw) and 0 <= v < float(ih)
    Per box (t, l, b, rt) = rows[r, 0:4]:
        shrink == 1: y0 = t, y1 = b, x0 = l, x1 = rt                       (the row's own numbers, exactly)
        otherwise    cy = (t + b) * 0.5, cx = (l + rt) * 0.5, hy = ((b - t) * 0.5) * shrink, hx = ((rt - l) * 0.5) * shrink
                     y0 = cy - hy, y1 = cy + hy, x0 = cx - hx, x1 = cx + hx
        inside when x0 <= u < x1 and y0 <= v < y1                          (a NaN edge contains nothing)
    The candidates of a box are the points kept, in view and inside it -- a point inside several boxes is a candidate of each
    -- ordered by the key bits(hw) << 32 | i: hw is positive and finite, so its bits order as an unsigned integer, and equal
    depths go to the lower index.  count[r] is their number, readout[r, 0] = (hw, f0, f1, f2, f3) of the smallest key, the
    NEAREST point, readout[r, 1] the same of the candidate of rank (count - 1) // 2 in ascending order, the LOWER MEDIAN by
    depth: the value to trust when water clutter in front of a hull makes the nearest point unrepresentative.  Feature bits
    are copied (NaN payloads survive); with count == 0 all ten numbers are +0.0.  shrink in (0, 1] keeps the box's centre and
    scales its sides; min_depth as `check_radar_rule` has it.  Bad shapes or types raise RuntimeError."""
    f32 = np.float32
    md = check_radar_rule(0, min_depth, "box_radar")[1]
    s = check_box_shrink(shrink)
    pts, P, rows = np.asarray(points), np.asarray(P), np.asarray(rows)
    if pts.ndim != 2 or pts.shape[1] != 7 or pts.dtype != np.float32:
        raise RuntimeError(f"box_radar: points are (n, 7) float32 rows x, y, z, f0, f1, f2, f3, got {pts.dtype} {pts.shape}")
    if P.shape != (3, 4) or P.dtype != np.float32:
        raise RuntimeError(f"box_radar: P is a (3, 4) float32 projection, got {P.dtype} {P.shape}")
    if rows.ndim != 2 or rows.shape[1] < 4 or rows.dtype != np.float32:
        raise RuntimeError(f"box_radar: rows are (m, >= 4) float32 with top, left, bottom, right in front, got {rows.dtype} {rows.shape}")
    ih, iw = (int(v) for v in size)
    m = rows.shape[0]
    count, readout = np.zeros(m, np.int32), np.zeros((m, 2, 5), np.uint32)
    if min(ih, iw) <= 0 or not len(pts) or not m:
        return count, readout.view(f32)
    pts = np.ascontiguousarray(pts)
    x, y, z = pts[:, 0], pts[:, 1], pts[:, 2]
    with np.errstate(all="ignore"):
        hu, hv, hw = (((P[r, 0] * x + P[r, 1] * y) + P[r, 2] * z) + P[r, 3] for r in range(3))
        ok = (hw >= md) & np.isfinite(hw) & np.isfinite(hu) & np.isfinite(hv)
        den = np.where(ok, hw, f32(1))
        u, v = hu / den, hv / den
        assert hw.dtype == f32 and u.dtype == f32 and v.dtype == f32
        ok &= (u >= 0) & (u < f32(iw)) & (v >= 0) & (v < f32(ih))
        t, l, b, rt = (rows[:, k].astype(f32) for k in range(4))
        if s == 1:
            y0, y1, x0, x1 = t, b, l, rt
        else:
            cy, cx = (t + b) * f32(0.5), (l + rt) * f32(0.5)
            hy, hx = ((b - t) * f32(0.5)) * s, ((rt - l) * f32(0.5)) * s
            y0, y1, x0, x1 = cy - hy, cy + hy, cx - hx, cx + hx
        assert y0.dtype == f32 and x1.dtype == f32
        idx = np.flatnonzero(ok)
        keys = (hw[idx].view(np.uint32).astype(np.uint64) << np.uint64(32)) | idx.astype(np.uint64)
        order = np.argsort(keys, kind="stable")
        idx, uu, vv = idx[order], u[idx][order], v[idx][order]           # the candidates of any box, in ascending key order
        inside = (x0[:, None] <= uu) & (uu < x1[:, None]) & (y0[:, None] <= vv) & (vv < y1[:, None])
    bits = pts.view(np.uint32)
    depth = hw.view(np.uint32)
    for r in range(m):
        mine = idx[inside[r]]
        count[r] = len(mine)
        if len(mine):
            for k, i in enumerate((mine[0], mine[(len(mine) - 1) // 2])):
                readout[r, k, 0] = depth[i]
                readout[r, k, 1:] = bits[i, 3:7]
    return count, readout.view(f32)


def device_box_radar(points, views, rows, kept, min_depth=0.1, shrink=1.0, flag=None, ws=None):
    """`box_radar` for a batch ON THE DEVICE (vrnet_box_radar_f32, two launches), the eager call outside a pipeline: points
    (B, max_points, 7) float32 and views, the (B, hip.RADAR_VIEW_BYTES) uint8 table (`radar_view_bytes(radar_views(...))`; ih,
    iw, count and P are read), rows (B, cap, 7) float32 and kept (B) int32 as `FrameResult` holds them, all on the device ->
    (counts (B, cap) int32, readout (B, cap, 2, 5) float32) on the device: per image what `box_radar` gives on rows[:kept], bit
    for bit, zeros behind.  flag: an int32 device word that receives hip.FLAG_GEOMETRY / FLAG_POINT_COUNT / FLAG_BOX_COUNT.
    No host synchronisation."""
    from . import hip
    fn = "device_box_radar"
    md = check_radar_rule(0, min_depth, fn)[1]
    s = check_box_shrink(shrink, fn)
    if not torch.is_tensor(rows) or rows.dim() != 3 or not rows.is_cuda:
        raise RuntimeError(f"{fn}: rows is a (B, cap, 7) float32 tensor on the device")
    B, cap = rows.shape[:2]
    with torch.cuda.device(rows.device):
        counts = torch.empty((B, cap), dtype=torch.int32, device=rows.device)
        readout = torch.empty((B, cap, 2, 5), dtype=torch.float32, device=rows.device)
        return hip.box_radar(points, views, rows, kept, float(md), float(s), counts, readout, flag=flag, ws=ws)


# ---- multi-object tracking of the detections: host statement of csrc/track.hip ----------------------------------------------------
# vrnet_track of include/vrnet_hip.h: one track, 64 bytes; a free slot is all zeros, so zeroed memory is the reset state
TRACK_DTYPE = np.dtype([("id", "<i4"), ("cls", "<i4"), ("hits", "<i4"), ("misses", "<i4"), ("row", "<i4"), ("range_age", "<i4"),
                        ("x", "<f4", (5,)), ("v", "<f4", (5,))])
assert TRACK_DTYPE.itemsize == 64
TRACK_HEAD = 4                       # per stream, int32: ids handed out so far, live tracks, calls so far, births of this call
TRACK_MAX_TRACKS, TRACK_MAX_ROWS = 256, 1024
FLAG_TRACK_FULL = 32768              # VR_FLAG_TRACK_FULL of csrc/common.h: a valid row found no free slot and got id 0
_TRACK_DEFAULTS = dict(max_tracks=64, iou=0.3, max_age=5, gain=(0.5, 0.25), range_gain=(0.5, 0.25))
_INT_MAX = 2 ** 31 - 1


def check_track_params(track=True, fn="track_update"):
    """The tracker's parameters from True / None (the defaults) or a dict that overrides some of max_tracks = 64 (1..256),
    iou = 0.3 (the match threshold, in (0, 1]), max_age = 5 (a track is freed after more than that many calls in a row
    without a match; 0..2^20), gain = (0.5, 0.25) and range_gain = (0.5, 0.25) (position and rate gain of the box filter and
    of the range filter, each finite and in [0, 2]) -> a dict with all five, the floats as float32.  Anything else raises
    RuntimeError."""
    if track is None or track is True:
        track = {}
    if not isinstance(track, dict):
        raise RuntimeError(f"{fn}: track is None, True or a dict of parameters, got {type(track).__name__}")
    unknown = sorted(set(track) - set(_TRACK_DEFAULTS))
    if unknown:
        raise RuntimeError(f"{fn}: unknown track parameters {unknown}; known: {sorted(_TRACK_DEFAULTS)}")
    p = dict(_TRACK_DEFAULTS, **track)

    def whole(name, lo, hi):
        v = p[name]
        if isinstance(v, bool) or not isinstance(v, (int, np.integer)) or not lo <= int(v) <= hi:
            raise RuntimeError(f"{fn}: {name} must be an integer in [{lo}, {hi}], got {v!r}")
        return int(v)

    def real(name, v):
        try:
            f = np.float32(v)
        except (TypeError, ValueError):
            f = np.float32("nan")
        if isinstance(v, bool) or not np.isfinite(f):
            raise RuntimeError(f"{fn}: {name} must be a finite number, got {v!r}")
        return f

    out = dict(max_tracks=whole("max_tracks", 1, TRACK_MAX_TRACKS), max_age=whole("max_age", 0, 1 << 20))
    out["iou"] = real("iou", p["iou"])
    if not (out["iou"] > 0 and out["iou"] <= 1):
        raise RuntimeError(f"{fn}: iou must lie in (0, 1], got {p['iou']!r}")
    for name in ("gain", "range_gain"):
        try:
            pair = tuple(p[name])
        except TypeError:
            pair = ()
        if len(pair) != 2:
            raise RuntimeError(f"{fn}: {name} is a (position, rate) pair, got {p[name]!r}")
        out[name] = tuple(real(name, v) for v in pair)
        if not all(0 <= g <= 2 for g in out[name]):
            raise RuntimeError(f"{fn}: {name} must lie in [0, 2], got {p[name]!r}")
    return out


def track_key(iou, slot, row):
    """The 64-bit key of a candidate pair: bits(iou) << 32 | (65535 - slot) << 16 | (65535 - row).  iou is positive, so its
    bits order as an unsigned integer; the LARGEST key is the pair to take: the largest IoU, then the lowest slot, then the
    lowest row.  No two pairs share a key, and 0 is no pair.  Arrays or scalars -> uint64."""
    bits = np.asarray(iou, np.float32).view(np.uint32).astype(np.uint64)
    return (bits << np.uint64(32)) | ((np.uint64(65535) - np.asarray(slot).astype(np.uint64)) << np.uint64(16)) | \
        (np.uint64(65535) - np.asarray(row).astype(np.uint64))


def track_iou(tracks, boxes):
    """IoU of every (track box, detection box) pair, (T, 4) and (n, 4) float32 of top, left, bottom, right, all FINITE ->
    (T, n) float32, every operation rounded on its own in this order:
        ih = min(b1, b2) - max(t1, t2), iw = min(r1, r2) - max(l1, l2)           (min(a, b) = a if a < b else b; max likewise)
        ih > 0 and iw > 0: inter = ih * iw, union = ((b1 - t1) * (r1 - l1) + (b2 - t2) * (r2 - l2)) - inter, iou = inter / union
        otherwise 0
    An overflowing area can make the quotient NaN; a NaN is no candidate."""
    f32 = np.float32
    a, z = np.asarray(tracks, f32)[:, None, :], np.asarray(boxes, f32)[None, :, :]
    with np.errstate(all="ignore"):
        lo = lambda p, q: np.where(p < q, p, q)
        hi = lambda p, q: np.where(p > q, p, q)
        ih = lo(a[..., 2], z[..., 2]) - hi(a[..., 0], z[..., 0])
        iw = lo(a[..., 3], z[..., 3]) - hi(a[..., 1], z[..., 1])
        inter = ih * iw
        a1 = (a[..., 2] - a[..., 0]) * (a[..., 3] - a[..., 1])
        a2 = (z[..., 2] - z[..., 0]) * (z[..., 3] - z[..., 1])
        union = (a1 + a2) - inter
        iou = np.where((ih > 0) & (iw > 0), inter / union, f32(0))
    assert iou.dtype == f32
    return iou


def track_class(value):
    """The class of a detection row as the tracker reads it: the float32 truncated toward zero when it lies in
    [-2^31, 2^31), -1 otherwise (NaN included).  Array -> int32."""
    v = np.asarray(value, np.float32)
    ok = (v >= np.float32(-2147483648.0)) & (v < np.float32(2147483648.0))
    return np.where(ok, np.where(ok, v, 0).astype(np.int64), -1).astype(np.int32)


def _track_range(rec, depth_ok, depth, gains):
    """Step 3's range update of one record."""
    f32 = np.float32
    if not depth_ok:
        return
    if rec["range_age"] < 0:
        rec["x"][4], rec["v"][4] = depth, f32(0)
    else:
        r = f32(depth - rec["x"][4])
        rec["x"][4] = f32(rec["x"][4] + f32(gains[0] * r))
        rec["v"][4] = f32(rec["v"][4] + f32(gains[1] * r))
    rec["range_age"] = 0


def track_update(table, head, rows, kept, box_points=None, box_radar=None, params=None):
    """One call of the tracker on every stream -- this project's own definition, the reference has no tracker:
    (table, head, ids, flag), new arrays.  table (B, T) TRACK_DTYPE and head (B, 4) int32 are the state BEFORE the call (zeros:
    the reset state), rows (B, cap, >= 7) float32 and kept (B) int32 as `FrameResult` holds them (top, left, bottom, right in
    pixels of the original frame, the class in column 6), box_points (B, cap) int32 and box_radar (B, cap, 2, 5) float32 the
    radar readout of the rows (`box_radar`; both or neither), params from `check_track_params` (max_tracks is not read: T is
    the table's).  ids (B, cap) int32: the id of the track each row matched or started, 0 for an invalid row, for a row that
    found no slot and from row kept[b] on.  flag: FLAG_BOX_COUNT when a kept[b] outside [0, cap] was clamped,
    FLAG_TRACK_FULL when a valid row found no free slot.  Everything in float32, every operation rounded on its own.
    Per stream, with n = kept[b] clamped:
      1 predict  every live slot (id != 0): x[k] = x[k] + v[k], k < 4; with range_age >= 0 the same for x[4], and range_age
                 += 1 (saturating).  A slot whose predicted box is not finite is freed (all 16 words zero)
      2 match    a row is VALID when its four coordinates are finite, bottom > top and right > left.  A live slot and a valid
                 row of its class (`track_class` of column 6) are a candidate pair iff `track_iou` >= iou (equality matches).
                 Greedy: repeatedly take the candidate of the largest `track_key` among unmatched slots and unmatched rows
      3 update   a matched (slot, row i), per box component: r = z - x, x = x + g_pos r, v = v + g_vel r; hits += 1
                 (saturating), misses = 0, row = i.  Range, when box_points[b, i] > 0 and depth = box_radar[b, i, 1, 0] (the
                 lower median) is finite: range_age < 0: x[4] = depth, v[4] = 0; otherwise the same filter with range_gain;
                 then range_age = 0
      4 coast    an unmatched live slot: misses += 1, row = -1; freed when misses > max_age
      5 births   valid unmatched rows in ascending order take the free slots in ascending order, those freed in 1 and 4
                 included: id = ++head[0], cls, hits = 1, misses = 0, row = i, x[0:4] = z, v = 0, range_age = -1, then the
                 range as in 3.  Without a free slot: id 0 and FLAG_TRACK_FULL
      6 header   head[1] = live tracks, head[3] = births of this call, head[2] += 1"""
    f32, fn = np.float32, "track_update"
    p = check_track_params(params, fn)
    table, head, rows, kept = np.array(table), np.array(head), np.asarray(rows), np.asarray(kept)
    if table.dtype != TRACK_DTYPE or table.ndim != 2 or not 1 <= table.shape[1] <= TRACK_MAX_TRACKS:
        raise RuntimeError(f"{fn}: table is (B, T) TRACK_DTYPE with T in [1, {TRACK_MAX_TRACKS}], got {table.dtype} {table.shape}")
    B, T = table.shape
    if head.shape != (B, TRACK_HEAD) or head.dtype != np.int32:
        raise RuntimeError(f"{fn}: head is ({B}, {TRACK_HEAD}) int32, got {head.dtype} {head.shape}")
    if rows.ndim != 3 or rows.shape[0] != B or rows.shape[2] < 7 or rows.dtype != np.float32 or not 1 <= rows.shape[1] <= TRACK_MAX_ROWS:
        raise RuntimeError(f"{fn}: rows are ({B}, cap, >= 7) float32 with cap in [1, {TRACK_MAX_ROWS}], got {rows.dtype} {rows.shape}")
    cap = rows.shape[1]
    if kept.shape != (B,) or kept.dtype != np.int32:
        raise RuntimeError(f"{fn}: kept is ({B}) int32, got {kept.dtype} {kept.shape}")
    if (box_points is None) != (box_radar is None):
        raise RuntimeError(f"{fn}: box_points and box_radar come together or not at all")
    if box_points is not None:
        box_points, box_radar = np.asarray(box_points), np.asarray(box_radar)
        if box_points.shape != (B, cap) or box_points.dtype != np.int32 or box_radar.shape != (B, cap, 2, 5) or box_radar.dtype != f32:
            raise RuntimeError(f"{fn}: box_points is ({B}, {cap}) int32 and box_radar ({B}, {cap}, 2, 5) float32, got "
                               f"{box_points.dtype} {box_points.shape} and {box_radar.dtype} {box_radar.shape}")
    thr, max_age, (gp, gv), rg = p["iou"], p["max_age"], p["gain"], p["range_gain"]
    ids, flag = np.zeros((B, cap), np.int32), 0
    slots = np.arange(T)
    for b in range(B):
        tab, n = table[b], min(max(int(kept[b]), 0), cap)
        if n != int(kept[b]):
            flag |= 512
        with np.errstate(all="ignore"):
            # 1 predict
            live = tab["id"] != 0
            tab["x"][:, :4] = np.where(live[:, None], tab["x"][:, :4] + tab["v"][:, :4], tab["x"][:, :4])
            ranged = live & (tab["range_age"] >= 0)
            tab["x"][:, 4] = np.where(ranged, tab["x"][:, 4] + tab["v"][:, 4], tab["x"][:, 4])
            tab["range_age"] = np.where(ranged & (tab["range_age"] < _INT_MAX), tab["range_age"] + 1, tab["range_age"])
            lost = live & ~np.isfinite(tab["x"][:, :4]).all(1)
            tab[lost] = np.zeros((), TRACK_DTYPE)
            live &= ~lost
            # 2 match
            z = np.ascontiguousarray(rows[b, :n, :4])
            cls = track_class(rows[b, :n, 6])
            valid = np.isfinite(z).all(1) & (z[:, 2] > z[:, 0]) & (z[:, 3] > z[:, 1])
            iou = track_iou(np.where(live[:, None], tab["x"][:, :4], f32(0)), np.where(valid[:, None], z, f32(0)))
            cand = live[:, None] & valid[None, :] & (tab["cls"][:, None] == cls[None, :]) & (iou >= thr)
        cs, ci = np.nonzero(cand)
        keys = track_key(iou[cs, ci], cs, ci)
        slot_row, row_slot = np.full(T, -1), np.full(n, -1)
        open_ = np.ones(len(keys), bool)
        while open_.any():                   # the plain way: one pair at a time
            k = int(np.argmax(np.where(open_, keys, np.uint64(0))))
            s, i = int(cs[k]), int(ci[k])
            slot_row[s], row_slot[i] = i, s
            open_ &= (cs != s) & (ci != i)
        # 3 update, 4 coast
        for s in slots[live]:
            rec, i = tab[s], slot_row[s]
            if i < 0:
                rec["misses"] += 1
                rec["row"] = -1
                if rec["misses"] > max_age:
                    tab[s] = np.zeros((), TRACK_DTYPE)
                continue
            for k in range(4):
                r = f32(z[i, k] - rec["x"][k])
                rec["x"][k] = f32(rec["x"][k] + f32(gp * r))
                rec["v"][k] = f32(rec["v"][k] + f32(gv * r))
            rec["hits"] = min(int(rec["hits"]) + 1, _INT_MAX)
            rec["misses"], rec["row"] = 0, i
            ids[b, i] = rec["id"]
            if box_points is not None:
                depth = box_radar[b, i, 1, 0]
                _track_range(rec, box_points[b, i] > 0 and np.isfinite(depth), depth, rg)
        # 5 births
        free = [int(s) for s in slots[tab["id"] == 0]]
        births = 0
        for i in np.flatnonzero(valid & (row_slot < 0)):
            if births == len(free):
                flag |= FLAG_TRACK_FULL
                break
            rec = tab[free[births]]
            births += 1
            rec["id"] = ids[b, i] = ids_wrap(int(head[b, 0]) + births)
            rec["cls"], rec["hits"], rec["misses"], rec["row"], rec["range_age"] = cls[i], 1, 0, i, -1
            rec["x"][:4], rec["x"][4], rec["v"][:] = z[i], 0, 0
            if box_points is not None:
                depth = box_radar[b, i, 1, 0]
                _track_range(rec, box_points[b, i] > 0 and np.isfinite(depth), depth, rg)
        # 6 header
        head[b, 0] = ids_wrap(int(head[b, 0]) + births)
        head[b, 1], head[b, 3] = int((tab["id"] != 0).sum()), births
        head[b, 2] = ids_wrap(int(head[b, 2]) + 1)
    return table, head, ids, flag


def ids_wrap(v):
    """An int32 counter after 2^31 - 1: it wraps, as the device's does (2^31 births or calls of one stream are not reached)."""
    return np.int32(((int(v) + 2 ** 31) % 2 ** 32) - 2 ** 31)


def track_text(tracks):
    """The <stem>_tracks.txt of `predict_dir` for one picture: tracks, a TRACK_DTYPE array (free slots are skipped) -> one line
    per live track in slot order, space-separated: id class hits misses top left bottom right range rate -- the four integers,
    then x[0:4], and x[4], v[4] of the range filter (0 0 before the first radar update); every float as %.9g, which names a
    float32 exactly."""
    tracks = np.asarray(tracks)
    if tracks.dtype != TRACK_DTYPE or tracks.ndim != 1:
        raise RuntimeError(f"track_text: expected a one-dimensional TRACK_DTYPE array, got {tracks.dtype} {tracks.shape}")
    lines = []
    for t in tracks[tracks["id"] != 0]:
        floats = list(t["x"][:4]) + [t["x"][4], t["v"][4]]
        lines.append(" ".join([str(int(t[k])) for k in ("id", "cls", "hits", "misses")] + ["%.9g" % float(v) for v in floats]) + "\n")
    return "".join(lines)


# ---- radar points under Mosaic: host statement of the radar-points kernels of csrc/mosaic.hip ----------------------------------
# vrnet_radar_source of include/vrnet_hip.h, one record per SOURCE (56 bytes): what the kernel needs beside the Mosaic record
RADAR_SOURCE_DTYPE = np.dtype([("count", "<i4"), ("reserved", "<i4"), ("P", "<f4", (12,))])


def radar_sources(calib, counts):
    """The packed per-source table of `hip.mosaic_radar_points`: calib (3, 4) or (S, 3, 4), counts (S) points per source -> an
    (S,) RADAR_SOURCE_DTYPE array (`radar_source_bytes` of it is what the device takes).  Host only."""
    counts = np.asarray(counts.cpu().numpy() if torch.is_tensor(counts) else counts)
    if counts.ndim != 1 or len(counts) == 0 or not np.issubdtype(counts.dtype, np.integer):
        raise RuntimeError(f"radar_sources: counts are S integers, one per source, got {counts.dtype} {counts.shape}")
    S = len(counts)
    out = np.zeros(S, RADAR_SOURCE_DTYPE)
    out["count"] = counts
    out["P"] = check_calib(calib, S, "radar_sources").reshape(S, 12)
    return out


def radar_source_bytes(sources):
    """A `radar_sources` table as the (S, hip.RADAR_SOURCE_BYTES) uint8 host tensor the device takes; it shares the table's memory."""
    return torch.from_numpy(sources.view(np.uint8).reshape(len(sources), -1))


def mosaic_radar_map(points, calib, sizes, input_shape, rec, radius=0, min_depth=0.1):
    """The radar input (4, H, W) float32 of ONE Mosaic image from the radar POINTS of its sources, where `mosaic_sample` gathers
    from finished maps -- this project's own definition, stated through `radar_map` and nothing else.  points: S arrays of
    (n, 7) float32 rows, indexed by the tiles' src (None or empty: no points); calib (3, 4) or (S, 3, 4), the projection of each
    source's own frame; sizes (S, 2) = (ih, iw) of the sources; rec: one MOSAIC_DTYPE record.  For every tile t with src >= 0:
        window = (nw, nh, W - dx - nw if tile.flip else dx, dy)
        m = radar_map(points[src], P[src], (tile.ih, tile.iw), (H, W), window, flip=bool(tile.flip), radius, min_depth)
        out[:, ys, xs] = m[:, ys, xs]
    with ys, xs the tile's quadrant as in `mosaic_sample` (tile 0: x < cutx, y < cuty; 1: x < cutx, y >= cuty; 2: x >= cutx, y >=
    cuty; 3: x >= cutx, y < cuty), and 0 elsewhere.  The shifted window puts a mirrored source at X = dx + nw - 1 - ix: that is
    the tile flip of `mosaic_sample` (wx' = nw - 1 - wx, the SOURCE is mirrored), not a mirror of the canvas, and the window's
    extent stays [dx, dx + nw - 1].  What follows from the rule:
        a kept point whose centre lies outside its quadrant still covers the quadrant's pixels within radius;
        each pixel receives candidates from one source only, its quadrant's tile's;
        the winner is the smallest hw, then the lowest index within that source;
        a non-mosaicked record (cut (W, H), tile 0 only) is `radar_map` under tile 0's window.
    Every point moves exactly once, where the gather of a map rasterised under the source's letterbox window drops points of
    a shrunk tile and duplicates those of an enlarged one.  The record is taken as it is: `check_mosaic_table` validates."""
    H, W = (int(v) for v in input_shape)
    own = frame_sizes(sizes, fn="mosaic_radar_map")
    S = len(own)
    P = check_calib(calib, S, "mosaic_radar_map")
    if len(points) != S:
        raise RuntimeError(f"mosaic_radar_map: {len(points)} point sets for {S} sources")
    cutx, cuty = int(rec["cutx"]), int(rec["cuty"])
    out = np.zeros((4, H, W), np.float32)
    for t, tile in enumerate(rec["tile"]):
        src = int(tile["src"])
        if src < 0:
            continue
        ys = slice(cuty, H) if t in (1, 2) else slice(0, cuty)
        xs = slice(cutx, W) if t in (2, 3) else slice(0, cutx)
        nw, nh, dx, dy, flip = (int(tile[k]) for k in ("nw", "nh", "dx", "dy", "flip"))
        pts = points[src]
        pts = np.zeros((0, 7), np.float32) if pts is None or len(pts) == 0 else np.asarray(pts)
        m = radar_map(pts, P[src], (int(tile["ih"]), int(tile["iw"])), (H, W), (nw, nh, W - dx - nw if flip else dx, dy), bool(flip),
                      radius, min_depth)
        out[:, ys, xs] = m[:, ys, xs]
    return out


def device_mosaic_radar_map(points, sizes, input_shape, calib, params, radius=0, min_depth=0.1, max_points=None, capacity=None,
                            device="cuda", out=None, flag=None):
    """`mosaic_radar_map` for a batch ON THE DEVICE (vrnet_mosaic_radar_points_f32, three launches): points of the S sources
    as `pack_points` takes them, sizes (S, 2) = (ih, iw) of the sources, calib (3, 4) or (S, 3, 4), params a (B,) MOSAIC_DTYPE
    table (`mosaic_params`, or `mosaic_record`s written by hand), validated here (`check_mosaic_table`) -> (B, 4, H, W) float32
    on the device, bit for bit what `mosaic_radar_map` gives per output image.  max_points: the capacity of the point buffer
    (default: the largest count); capacity: (ihm, iwm) by which the records are judged (default: the largest source).  flag: an
    int32 device word that receives hip.FLAG_GEOMETRY / hip.FLAG_POINT_COUNT (never, for inputs that passed the checks here).
    The points and the tables are copied non_blocking; no host synchronisation."""
    from . import hip
    fn = "device_mosaic_radar_map"
    radius, md = check_radar_rule(radius, min_depth, fn)
    H, W = (int(v) for v in input_shape)
    if max_points is None:
        if isinstance(points, tuple) and len(points) == 2 and getattr(points[0], "ndim", 0) == 3:
            max_points = max(int(points[0].shape[1]), 1)
        else:
            max_points = max([1] + [0 if a is None else len(a) for a in points])
    packed, counts = pack_points(points, max_points)
    S = len(counts)
    own = frame_sizes(sizes, S, fn)
    if capacity is None:
        capacity = (int(own[:, 0].max()), int(own[:, 1].max()))
    table = check_mosaic_table(params, (H, W), own, capacity, None, fn)
    sources = radar_sources(check_calib(calib, S, fn), counts.numpy())
    dev = torch.device(device)
    with torch.cuda.device(dev):
        if out is None:
            out = torch.empty((len(table), 4, H, W), dtype=torch.float32, device=dev)
        hip.mosaic_radar_points(packed.to(dev, non_blocking=True), radar_source_bytes(sources).to(dev, non_blocking=True),
                                mosaic_bytes(table).to(dev, non_blocking=True), capacity, H, W, radius, float(md), out, flag=flag)
    return out


def make_sample(image, box, radar, png, num_classes_seg):
    """YoloDataset.__getitem__ after augmentation (dataloader.py:88-107): (image CHW float64, boxes cxcywh, radar,
    png, one-hot)."""
    image = np.transpose(preprocess_input(np.array(image, dtype=np.float64)), [2, 0, 1])
    png, seg_labels = seg_targets(png, num_classes_seg)
    return image, boxes_xyxy_to_cxcywh(box), np.array(radar, dtype=np.float64), png, seg_labels


def yolo_dataset_collate(batch):
    """dataloader.py:440-457."""
    images, bboxes, radars, pngs, seg_labels = zip(*batch)
    return (torch.from_numpy(np.array(images)).type(torch.FloatTensor),
            [torch.from_numpy(np.array(a, dtype=np.float64).reshape(-1, 5)).type(torch.FloatTensor) for a in bboxes],
            torch.from_numpy(np.array(radars)).type(torch.FloatTensor),
            torch.from_numpy(np.array(pngs)).long(),
            torch.from_numpy(np.array(seg_labels)).type(torch.FloatTensor))
