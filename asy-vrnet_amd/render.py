"""Result rendering on the device (csrc/render.hip): what the reference's predictors do AFTER the network ran, from the
bytes that are already there -- the frames that went into `data.device_letterbox`, the class map `decode.seg_predict`
returns and the rows `decode.non_max_suppression` keeps.

* `seg_render`: deeplab.py:169-222 -- the three `mix_type`s (0: `Image.blend(old_img, seg_img, alpha)`, Pillow's bytes bit
  for bit; 1: the palette lookup; 2: the frame where the class is not background) and the per-class pixel counts of :172-185.
* `box_rows` / `draw_boxes`: yolo.py:164-222 -- the integer box corners, `thickness`, the per-class detection counts and the
  `thickness` nested rectangle outlines per box, later boxes over earlier ones.
* `render_frame`: both in one launch, boxes over the overlay.
* `seg_palette` / `det_palette`: the colour lists of deeplab.py:75-83 and yolo.py:85-87.

The outline rule is the geometric perimeter of each ring [left+i, top+i, right-i, bottom-i], clipped to the image, drawn
while left+i <= right-i and top+i <= bottom-i.  It equals `ImageDraw.rectangle(outline=...)` of Pillow 12.2 except in two
cases: Pillow paints a ring of ONE row (y0 == y1) two rows high ([5,5,5,5] paints (5,5) and (5,6)), and it raises
ValueError for x1 < x0 where this module paints nothing.

* `heatmap_mask` / `heatmap` / `heatmap_ragged`: yolo.py:288-351 `detect_heatmap` (csrc/heatmap.hip) -- per level
  sigmoid(max class logit) * sigmoid(objectness), OpenCV's INTER_LINEAR resize to the frame, times 255 truncated to a byte,
  the max over the three levels; then matplotlib's `imshow(mask, alpha, cmap="jet")` colour rule (default normalisation:
  vmin / vmax are the mask's own min / max) blended over the frame.  Two things are NOT reproduced.  The reference saves
  matplotlib's FIGURE, a 200-dpi canvas with margins onto which both images are resampled; here the picture has the
  frame's own resolution and is `Image.blend(frame, jet[index], alpha)` per byte.  And under a letterbox the reference
  still stretches the whole level map, grey bars included, over the picture, so the heat is misaligned: letterbox_image=False
  is that faithful form (valid for any frame), letterbox_image=True maps every pixel through the letterbox window first,
  which is this project's own definition (see csrc/heatmap.hip).
* `jet_lut`: matplotlib's "jet" as 256 x 3 bytes, from its segment data; matplotlib itself is not imported.

Out of scope: the label text and its filled background (they need the reference's font file), crop saving and video I/O."""
import colorsys

import numpy as np
import torch

MAX_COLORS = 256          # RN_MAXCOL of csrc/render.hip
MAX_BOXES = 1024          # RN_MAXBOX: box rows of one image
FLAG_CLASS, FLAG_BOX_COLOUR, FLAG_BOX_ROWS = 1, 2, 4     # bits of the optional `flag` word

_device_palettes = {}


def _hsv_palette(num_classes):
    hsv_tuples = [(x / num_classes, 1., 1.) for x in range(num_classes)]
    colors = [colorsys.hsv_to_rgb(*x) for x in hsv_tuples]
    return np.array([(int(c[0] * 255), int(c[1] * 255), int(c[2] * 255)) for c in colors], np.uint8).reshape(-1, 3)


def seg_palette(num_classes):
    """The colour list of deeplab.py:75-83 as (n, 3) uint8: for num_classes <= 21 its 22 fixed entries -- the VOC colour map
    (bit i of the class id goes to bit 7 - i/3 of channel i % 3) -- otherwise the HSV wheel with int(x * 255)."""
    if num_classes > 21:
        return _hsv_palette(num_classes)
    pal = np.zeros((22, 3), np.uint8)
    for i in range(22):
        c = i
        for j in range(8):
            for ch in range(3):
                pal[i, ch] |= ((c >> ch) & 1) << (7 - j)
            c >>= 3
    pal[21] = (128, 64, 12)        # deeplab.py:79: the reference's last entry, where the VOC map has (128, 64, 128)
    return pal


def det_palette(num_classes):
    """The box colours of yolo.py:85-87 as (num_classes, 3) uint8."""
    return _hsv_palette(num_classes)


def _as_u8(a, what, batched, fn):
    t = a if torch.is_tensor(a) else torch.from_numpy(np.ascontiguousarray(a))
    if t.dtype != torch.uint8:
        raise RuntimeError(f"{fn}: expected uint8 {what}, got {t.dtype}")
    return t[None] if t.dim() == batched - 1 else t


def _palette(pal, default, fn):
    """(n, 3) uint8 numpy from None (the default), a class count or an array of colours."""
    if pal is None:
        pal = default
    if isinstance(pal, (int, np.integer)):
        pal = det_palette(int(pal))
    if torch.is_tensor(pal):
        if pal.dtype != torch.uint8:
            raise RuntimeError(f"{fn}: expected a uint8 palette, got {pal.dtype}")
        if pal.dim() != 2 or pal.shape[1] != 3 or not 1 <= pal.shape[0] <= MAX_COLORS:
            raise RuntimeError(f"{fn}: expected a palette of shape (1..{MAX_COLORS}, 3), got {tuple(pal.shape)}")
        return pal
    pal = np.asarray(pal)
    if pal.dtype != np.uint8:
        raise RuntimeError(f"{fn}: expected a uint8 palette, got {pal.dtype}")
    if pal.ndim != 2 or pal.shape[1] != 3 or not 1 <= pal.shape[0] <= MAX_COLORS:
        raise RuntimeError(f"{fn}: expected a palette of shape (1..{MAX_COLORS}, 3), got {pal.shape}")
    return pal


def _palette_on(pal, device):
    """The palette as a device tensor; host palettes are copied once per (colours, device) and kept."""
    if torch.is_tensor(pal):
        return pal.to(device).contiguous()
    key = (pal.tobytes(), str(device))
    t = _device_palettes.get(key)
    if t is None:
        t = _device_palettes[key] = torch.from_numpy(np.ascontiguousarray(pal)).to(device)
    return t


def _overlap(a, b):
    return a.device == b.device and a.data_ptr() < b.data_ptr() + b.numel() and b.data_ptr() < a.data_ptr() + a.numel()


def box_rows(results, image_shape, class_names_or_n, input_shape=None):
    """The host half of yolo.py:164-208 for the list `decode.non_max_suppression` returns (float32 (N_b, 7) rows top, left,
    bottom, right, obj, class_conf, class; None or (0, 7) for an image without detections) and image_shape = (ih, iw).
    Returns (rows, offsets, thickness, counts): rows (N, 5) int32 = left, top, right, bottom, class with top = max(0,
    floor(top)), left = max(0, floor(left)), bottom = min(ih, floor(bottom)), right = min(iw, floor(right)) (:205-208);
    offsets (B + 1) int32, the rows of image b being offsets[b] .. offsets[b + 1] - 1; thickness = int(max((iw + ih) //
    mean(input_shape), 1)) (:164; None without input_shape); counts (B, num_classes) int64, the detections of each class
    per image (:168-176)."""
    n = class_names_or_n if isinstance(class_names_or_n, (int, np.integer)) else len(class_names_or_n)
    ih, iw = int(image_shape[0]), int(image_shape[1])
    rows, offsets = [], [0]
    counts = np.zeros((len(results), n), np.int64)
    for b, det in enumerate(results):
        det = np.zeros((0, 7), np.float32) if det is None else np.asarray(det)
        if det.ndim != 2 or det.shape[1] != 7:
            raise RuntimeError(f"box_rows: expected (N, 7) rows per image, got {det.shape}")
        box = np.clip(np.floor(det[:, :4].astype(np.float64)), -2.0 ** 31, 2.0 ** 31 - 1).astype(np.int64)
        label = det[:, 6].astype(np.int32)
        r = np.empty((len(det), 5), np.int32)
        r[:, 0] = np.maximum(0, box[:, 1])
        r[:, 1] = np.maximum(0, box[:, 0])
        r[:, 2] = np.minimum(iw, box[:, 3])
        r[:, 3] = np.minimum(ih, box[:, 2])
        r[:, 4] = label
        rows.append(r)
        offsets.append(offsets[-1] + len(det))
        for i in range(n):
            counts[b, i] = np.sum(label == i)
    rows = np.concatenate(rows) if rows else np.zeros((0, 5), np.int32)
    thickness = None if input_shape is None else int(max((iw + ih) // np.mean(input_shape), 1))
    return rows, np.array(offsets, np.int32), thickness, counts


def render_frame(frames_u8, class_map=None, results=None, input_shape=None, palette=None, mix_type=0, alpha=0.7,
                 count=False, box_palette=None, thickness=None, out=None, flag=None, device="cuda"):
    """The overlay of `seg_render` and the outlines of `draw_boxes` in ONE launch (vrnet_render_u8), boxes over the
    overlay.  frames_u8 (B,ih,iw,3) uint8 RGB original frames (a single (ih,iw,3) frame counts as B = 1), class_map
    (B,ih,iw) uint8 or None, numpy arrays or tensors.  results: None, the list `non_max_suppression` returns (packed by
    `box_rows` and sent in one non-blocking copy), or a pair (rows (N,5) int32, offsets (B+1) int32) of device tensors,
    which a captured graph can re-read.  palette / box_palette: (n,3) uint8 colours, default `seg_palette(21)` /
    `det_palette(4)`; box_palette may also be the number of detection classes.  thickness: default yolo.py:164 from
    input_shape = (H, W).  out: the (B,ih,iw,3) uint8 device tensor to write; without a class map it may be the frames
    themselves (boxes drawn in place).  flag: a zeroed int32 device tensor of one element that receives the data-error
    bits (FLAG_CLASS: a class id >= len(palette), which takes the last colour and is not counted; FLAG_BOX_COLOUR: a colour
    index outside the box palette, clamped; FLAG_BOX_ROWS: more than MAX_BOXES rows in one image) -- read it when you next
    synchronise.  Returns out, or (out, counts) with counts (B, len(palette)) int64 when count=True.  No host
    synchronisation."""
    from . import hip
    fn = "render"
    img = _as_u8(frames_u8, "frames", 4, fn)
    if img.dim() != 4 or img.shape[-1] != 3:
        raise RuntimeError(f"{fn}: expected frames of shape (B, ih, iw, 3) or (ih, iw, 3), got {tuple(img.shape)}")
    B, ih, iw = img.shape[:3]
    if min(B, ih, iw) <= 0:
        raise RuntimeError(f"{fn}: empty frames {tuple(img.shape)}")
    cmap = None if class_map is None else _as_u8(class_map, "class map", 3, fn)
    if cmap is not None and tuple(cmap.shape) != (B, ih, iw):
        raise RuntimeError(f"{fn}: the class map {tuple(cmap.shape)} does not match the frames {(B, ih, iw)}")
    if mix_type not in (0, 1, 2):
        raise RuntimeError(f"{fn}: mix_type must be 0, 1 or 2, got {mix_type!r}")
    if not 0.0 <= float(alpha) <= 1.0:
        raise RuntimeError(f"{fn}: alpha must lie in [0, 1], got {alpha!r}")
    if count and cmap is None:
        raise RuntimeError(f"{fn}: count=True needs a class map")
    pal = None if cmap is None else _palette(palette, seg_palette(21), fn)
    if out is not None:
        if not torch.is_tensor(out) or out.dtype != torch.uint8 or tuple(out.shape) != tuple(img.shape) or not out.is_contiguous():
            raise RuntimeError(f"{fn}: out must be a contiguous uint8 tensor of shape {tuple(img.shape)}")
        if cmap is not None and (_overlap(out, img) or _overlap(out, cmap)):
            raise RuntimeError(f"{fn}: out must not alias the frames or the class map when a class map is given")
    rows = offsets = bpal = None
    if results is not None:
        if isinstance(results, tuple) and len(results) == 2 and all(torch.is_tensor(t) for t in results):
            rows, offsets = results
            if rows.dtype != torch.int32 or offsets.dtype != torch.int32 or rows.dim() != 2 or rows.shape[1] != 5 or \
                    tuple(offsets.shape) != (B + 1,):
                raise RuntimeError(f"{fn}: expected int32 rows (N, 5) and offsets ({B + 1},), got {tuple(rows.shape)} "
                                   f"{rows.dtype} and {tuple(offsets.shape)} {offsets.dtype}")
            host_rows = None
        else:
            if len(results) != B:
                raise RuntimeError(f"{fn}: {len(results)} result entries for {B} frames")
            host_rows, host_offsets, auto, _ = box_rows(results, (ih, iw), MAX_COLORS, input_shape)
            if int(np.diff(host_offsets).max(initial=0)) > MAX_BOXES:
                raise RuntimeError(f"{fn}: more than {MAX_BOXES} boxes in one image")
            thickness = auto if thickness is None else thickness
        if thickness is None:
            if input_shape is None:
                raise RuntimeError(f"{fn}: boxes need a thickness or the input_shape it follows from")
            thickness = int(max((iw + ih) // np.mean(input_shape), 1))
        if int(thickness) < 1:
            raise RuntimeError(f"{fn}: thickness must be at least 1, got {thickness!r}")
        bpal = _palette(box_palette, det_palette(4), fn)
    img = img.to(device, non_blocking=True).contiguous()
    dev = img.device
    cmap = None if cmap is None else cmap.to(dev, non_blocking=True).contiguous()
    with torch.cuda.device(dev):
        if results is not None and host_rows is not None:
            # offsets and rows in one pinned buffer: a single non-blocking copy
            packed = torch.empty(B + 1 + host_rows.size, dtype=torch.int32).pin_memory()
            packed[:B + 1] = torch.from_numpy(host_offsets)
            packed[B + 1:] = torch.from_numpy(host_rows.reshape(-1))
            packed = packed.to(dev, non_blocking=True)
            offsets, rows = packed[:B + 1], packed[B + 1:].view(-1, 5)
        elif results is not None:
            rows, offsets = rows.to(dev).contiguous(), offsets.to(dev).contiguous()
        if out is None:
            out = torch.empty((B, ih, iw, 3), dtype=torch.uint8, device=dev)
        counts = torch.empty((B, pal.shape[0]), dtype=torch.int64, device=dev) if count else None
        hip.render(img, cmap, out, palette=None if pal is None else _palette_on(pal, dev), mix_type=mix_type, alpha=alpha,
                   boxes=rows, box_offsets=offsets, box_palette=None if bpal is None else _palette_on(bpal, dev),
                   thickness=1 if thickness is None else int(thickness), counts=counts, flag=flag)
    return (out, counts) if count else out


def render_frame_ragged(frames_u8, geom, class_map=None, results=None, palette=None, mix_type=0, alpha=0.7, count=False,
                        box_palette=None, out=None, flag=None):
    """`render_frame` for a batch of images of their own sizes (vrnet_render_ragged_u8).  frames_u8 (B, ihm, iwm, 3) and
    class_map (B, ihm, iwm) (or None) are padded uint8 DEVICE tensors with image b in the top-left corner of slot b; geom is
    the (B, hip.GEOM_BYTES) device table of `data.frame_geometry`, which gives every image its size and its outline
    thickness.  results: None or a pair (rows (N, 5) int32, offsets (B + 1) int32) of device tensors, as
    `hip.detect_finish_ragged` leaves them.  Returns out (B, ihm, iwm, 3), or (out, counts) with count=True: image b is
    `out[b, :ih_b, :iw_b]`, equal to `render_frame` on that image alone; every pixel outside it is 0 and is not counted.
    out must not be the frames.  flag also receives hip.FLAG_GEOMETRY.  No host synchronisation."""
    from . import hip
    fn = "render_ragged"
    img = frames_u8
    if not (torch.is_tensor(img) and img.is_cuda and img.dtype == torch.uint8 and img.dim() == 4 and img.shape[-1] == 3):
        raise RuntimeError(f"{fn}: expected padded uint8 frames (B, ihm, iwm, 3) on a GPU")
    B, ih, iw = img.shape[:3]
    if class_map is not None and not (torch.is_tensor(class_map) and class_map.dtype == torch.uint8 and
                                      tuple(class_map.shape) == (B, ih, iw)):
        raise RuntimeError(f"{fn}: the class map must be a uint8 tensor of shape {(B, ih, iw)}")
    if mix_type not in (0, 1, 2) or not 0.0 <= float(alpha) <= 1.0:
        raise RuntimeError(f"{fn}: mix_type must be 0, 1 or 2 and alpha in [0, 1], got {mix_type!r}, {alpha!r}")
    if count and class_map is None:
        raise RuntimeError(f"{fn}: count=True needs a class map")
    pal = None if class_map is None else _palette(palette, seg_palette(21), fn)
    rows = offsets = bpal = None
    if results is not None:
        rows, offsets = results
        bpal = _palette(box_palette, det_palette(4), fn)
    dev = img.device
    with torch.cuda.device(dev):
        if out is None:
            out = torch.empty((B, ih, iw, 3), dtype=torch.uint8, device=dev)
        counts = torch.empty((B, pal.shape[0]), dtype=torch.int64, device=dev) if count else None
        hip.render_ragged(img.contiguous(), None if class_map is None else class_map.contiguous(), geom, out,
                          palette=None if pal is None else _palette_on(pal, dev), mix_type=mix_type, alpha=alpha, boxes=rows,
                          box_offsets=offsets, box_palette=None if bpal is None else _palette_on(bpal, dev), counts=counts,
                          flag=flag)
    return (out, counts) if count else out


# matplotlib's "jet" (_cm.py `_jet_data`): per channel the (x, y) break points of a piecewise-linear map
_JET_SEGMENTS = (
    ((0.00, 0.0), (0.35, 0.0), (0.66, 1.0), (0.89, 1.0), (1.00, 0.5)),
    ((0.000, 0.0), (0.125, 0.0), (0.375, 1.0), (0.640, 1.0), (0.910, 0.0), (1.000, 0.0)),
    ((0.00, 0.5), (0.11, 1.0), (0.34, 1.0), (0.65, 0.0), (1.00, 0.0)),
)


def jet_lut():
    """`matplotlib.colormaps["jet"](np.arange(256), bytes=True)[:, :3]` as a (256, 3) uint8 array: the lookup table
    matplotlib builds from the segment data (colors.py `_create_lookup_table`, N = 256, gamma 1), then (lut * 255)
    truncated to bytes."""
    N = 256
    lut = np.empty((N, 3), np.float64)
    xind = (N - 1) * np.linspace(0, 1, N)
    for ch, seg in enumerate(_JET_SEGMENTS):
        x, y = np.array(seg, np.float64).T
        x = x * (N - 1)
        ind = np.searchsorted(x, xind)[1:-1]
        distance = (xind[1:-1] - x[ind - 1]) / (x[ind] - x[ind - 1])
        lut[:, ch] = np.concatenate([[y[0]], distance * (y[ind] - y[ind - 1]) + y[ind - 1], [y[-1]]])
    return (np.clip(lut, 0.0, 1.0) * 255).astype(np.uint8)


def _heat_levels(outputs, input_shape, fn):
    """The checks of the three raw detection maps that need no device; returns (levels as fp32 tensors, B, (H, W))."""
    try:
        H, W = (int(v) for v in input_shape)
    except (TypeError, ValueError):
        raise RuntimeError(f"{fn}: input_shape is a (height, width) pair, got {input_shape!r}") from None
    if H <= 0 or W <= 0 or H % 32 or W % 32:
        raise RuntimeError(f"{fn}: input_shape must be positive multiples of 32, got {(H, W)}")
    if not isinstance(outputs, (list, tuple)) or len(outputs) != 3 or not all(torch.is_tensor(t) and t.dim() == 4 for t in outputs):
        raise RuntimeError(f"{fn}: outputs must be the three detection maps (B, 5 + nc, h, w) of strides 8, 16 and 32")
    B, C = outputs[0].shape[:2]
    if C < 6:
        raise RuntimeError(f"{fn}: outputs have {C} channels; 4 box values, the objectness and at least one class are needed")
    for t, s in zip(outputs, (8, 16, 32)):
        if tuple(t.shape) != (B, C, H // s, W // s):
            raise RuntimeError(f"{fn}: the outputs of stride {s} must have shape {(B, C, H // s, W // s)} for input_shape "
                               f"{(H, W)}, got {tuple(t.shape)}")
        if t.dtype not in (torch.float32, torch.float16, torch.bfloat16):
            raise RuntimeError(f"{fn}: expected float32 (or half precision) outputs, got dtype {t.dtype}")
    if B == 0:
        raise RuntimeError(f"{fn}: outputs of an empty batch")
    return B, (H, W)


def _heat_common(alpha, cmap, fn):
    if not 0.0 <= float(alpha) <= 1.0:
        raise RuntimeError(f"{fn}: alpha must lie in [0, 1], got {alpha!r}")
    if cmap is None:
        return jet_lut()
    shape, dtype = tuple(cmap.shape), (cmap.dtype if torch.is_tensor(cmap) else np.asarray(cmap).dtype)
    if shape != (256, 3) or dtype not in (torch.uint8, np.uint8):
        raise RuntimeError(f"{fn}: cmap must be a uint8 table of shape (256, 3), got {dtype} {shape}")
    return cmap if torch.is_tensor(cmap) else np.asarray(cmap)


def _heat_device(outputs, fn):
    if not all(t.is_cuda for t in outputs) or len({t.device for t in outputs}) != 1:
        raise RuntimeError(f"{fn}: the outputs must be on one GPU device (there is no CPU fallback)")
    return [t.detach() if (t.is_contiguous() and t.dtype == torch.float32) else t.detach().contiguous().float() for t in outputs]


def _heat_window(input_shape, image_shape, letterbox_image):
    """(window, dx, dy, nw, nh) of the fixed-size call."""
    if not letterbox_image:
        return 0, 0, 0, 0, 0
    from . import decode
    top, left, nh, nw = decode.seg_window(input_shape, image_shape)
    if nh <= 0 or nw <= 0:
        raise RuntimeError(f"heatmap: image {tuple(image_shape)} leaves an empty window in {tuple(input_shape)}")
    return 1, left, top, nw, nh


def heatmap_mask(outputs, image_shape, input_shape, letterbox_image=False):
    """Steps :336-342 of yolo.py `detect_heatmap` for a batch: outputs = the three raw detection maps (B, 5 + nc, H/8, W/8),
    (.., H/16, W/16), (.., H/32, W/32) of a network input of input_shape = (H, W), image_shape = (ih, iw) of the original
    frames.  Returns the (B, ih, iw) uint8 mask on the outputs' device.  letterbox_image=False: the reference's resize of the
    whole level map; True: through the window of `decode.seg_window` (module docstring).  No host synchronisation."""
    from . import hip
    fn = "heatmap"
    B, (H, W) = _heat_levels(outputs, input_shape, fn)
    ih, iw = int(image_shape[0]), int(image_shape[1])
    if ih <= 0 or iw <= 0:
        raise RuntimeError(f"{fn}: bad image_shape {tuple(image_shape)}")
    window = _heat_window((H, W), (ih, iw), letterbox_image)
    levels = _heat_device(outputs, fn)
    dev = levels[0].device
    with torch.cuda.device(dev):
        mask = torch.empty((B, ih, iw), dtype=torch.uint8, device=dev)
        minmax = torch.empty((B, 2), dtype=torch.int32, device=dev)
        ws = torch.empty(hip.heatmap_workspace_bytes(B, H, W), dtype=torch.uint8, device=dev)
        hip.heatmap(levels, H, W, mask, minmax, ws, *window)
    return mask


def _heat_frames(frames_u8, batched, out, fn):
    img = _as_u8(frames_u8, "frames", 4, fn) if batched else frames_u8
    if not torch.is_tensor(img) or img.dtype != torch.uint8 or img.dim() != 4 or img.shape[-1] != 3 or min(img.shape) <= 0:
        raise RuntimeError(f"{fn}: expected uint8 frames of shape (B, ih, iw, 3), got "
                           f"{tuple(img.shape) if torch.is_tensor(img) else type(img).__name__}")
    if out is not None:
        if not torch.is_tensor(out) or out.dtype != torch.uint8 or tuple(out.shape) != tuple(img.shape) or not out.is_contiguous():
            raise RuntimeError(f"{fn}: out must be a contiguous uint8 tensor of shape {tuple(img.shape)}")
        if _overlap(out, img):
            raise RuntimeError(f"{fn}: out must not alias the frames")
    return img


def heatmap(frames_u8, outputs, input_shape, letterbox_image=False, alpha=0.5, cmap=None, out=None):
    """yolo.py:288-351 `detect_heatmap` on the device: frames_u8 (B, ih, iw, 3) uint8 RGB original frames (numpy or tensor; a
    single (ih, iw, 3) frame counts as B = 1) and outputs as in `heatmap_mask`.  Returns (picture, mask, minmax): picture
    (B, ih, iw, 3) uint8 = Image.blend(frame, cmap[index(mask)], alpha) with matplotlib's default normalisation per image
    (module docstring), mask (B, ih, iw) uint8, minmax (B, 2) int32 = each mask's (min, max).  cmap: a (256, 3) uint8 table,
    default `jet_lut()`.  out: the device tensor to write the picture into; it must not alias the frames.  No host
    synchronisation."""
    from . import hip
    fn = "heatmap"
    B, (H, W) = _heat_levels(outputs, input_shape, fn)
    img = _heat_frames(frames_u8, True, out, fn)
    if img.shape[0] != B:
        raise RuntimeError(f"{fn}: {img.shape[0]} frames for outputs of {B} images")
    ih, iw = img.shape[1:3]
    lut = _heat_common(alpha, cmap, fn)
    window = _heat_window((H, W), (ih, iw), letterbox_image)
    levels = _heat_device(outputs, fn)
    dev = levels[0].device
    img = img.to(dev, non_blocking=True).contiguous()
    with torch.cuda.device(dev):
        picture = torch.empty((B, ih, iw, 3), dtype=torch.uint8, device=dev) if out is None else out
        mask = torch.empty((B, ih, iw), dtype=torch.uint8, device=dev)
        minmax = torch.empty((B, 2), dtype=torch.int32, device=dev)
        ws = torch.empty(hip.heatmap_workspace_bytes(B, H, W), dtype=torch.uint8, device=dev)
        hip.heatmap(levels, H, W, mask, minmax, ws, *window, frames=img, cmap=_palette_on(lut, dev), alpha=alpha, out=picture)
    return picture, mask, minmax


def heatmap_ragged(frames_u8, outputs, geom, input_shape, window=True, alpha=0.5, cmap=None, out=None, flag=None):
    """`heatmap` for a batch of images of their own sizes (vrnet_heatmap_ragged_f32): frames_u8 (B, ihm, iwm, 3) padded uint8
    DEVICE slots with image b in the top-left corner, geom the (B, hip.GEOM_BYTES) device table of `data.frame_geometry`.
    window=True maps the pixels of image b through its letterbox window (dx, dy, nw, nh) of the table (the whole input for
    a table made with letterbox_image=False); window=False is the reference's whole-map resize.  Returns (picture
    (B, ihm, iwm, 3), mask (B, ihm, iwm), minmax (B, 2)): image b is `[b, :ih_b, :iw_b]`, equal to `heatmap` on that image
    alone; every pixel outside it is 0 and minmax[b] covers the image's own pixels.  flag: an int32 device word for
    hip.FLAG_GEOMETRY, or None.  No host synchronisation."""
    from . import hip
    fn = "heatmap_ragged"
    B, (H, W) = _heat_levels(outputs, input_shape, fn)
    img = _heat_frames(frames_u8, False, out, fn)
    if img.shape[0] != B:
        raise RuntimeError(f"{fn}: {img.shape[0]} frame slots for outputs of {B} images")
    lut = _heat_common(alpha, cmap, fn)
    levels = _heat_device(outputs, fn)
    dev = levels[0].device
    if img.device != dev:
        raise RuntimeError(f"{fn}: the frames must be on the outputs' device {dev}")
    ihm, iwm = img.shape[1:3]
    with torch.cuda.device(dev):
        picture = torch.empty((B, ihm, iwm, 3), dtype=torch.uint8, device=dev) if out is None else out
        mask = torch.empty((B, ihm, iwm), dtype=torch.uint8, device=dev)
        minmax = torch.empty((B, 2), dtype=torch.int32, device=dev)
        ws = torch.empty(hip.heatmap_ragged_workspace_bytes(B, H, W), dtype=torch.uint8, device=dev)
        hip.heatmap_ragged(levels, geom, H, W, mask, minmax, ws, window=1 if window else 0, frames=img.contiguous(),
                           cmap=_palette_on(lut, dev), alpha=alpha, out=picture, flag=flag)
    return picture, mask, minmax


def seg_render(frames_u8, class_map, palette=None, mix_type=0, alpha=0.7, count=False, out=None, flag=None, device="cuda"):
    """deeplab.py:169-222 on the device: frames_u8 (B,ih,iw,3) uint8 original frames and class_map (B,ih,iw) uint8 (what
    `decode.seg_predict` returns) -> the (B,ih,iw,3) uint8 picture of mix_type 0 (Image.blend(frame, palette[class], alpha),
    Pillow's bytes), 1 (palette[class]) or 2 (the frame where class != 0, else 0); with count=True also the (B, len(palette))
    int64 pixels of each class per image (:172-185).  See `render_frame` for the arguments."""
    if class_map is None:
        raise RuntimeError("render: seg_render needs a class map")
    return render_frame(frames_u8, class_map, None, None, palette, mix_type, alpha, count, out=out, flag=flag, device=device)


def draw_boxes(frames_u8, results, input_shape, palette=None, thickness=None, out=None, flag=None, device="cuda"):
    """yolo.py:164-222 without the label text: `box_rows` of the list `non_max_suppression` returns plus the kernel --
    `thickness` nested outlines per box in palette[class] (default `det_palette(4)`), later boxes over earlier ones.
    out may be the frames tensor itself (drawn in place).  One non-blocking host-to-device copy of the packed rows."""
    if results is None:
        raise RuntimeError("render: draw_boxes needs the results of non_max_suppression")
    return render_frame(frames_u8, None, results, input_shape, box_palette=palette, thickness=thickness, out=out, flag=flag,
                        device=device)
