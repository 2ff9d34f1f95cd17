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

* `LabelAtlas` / `draw_labels` / `labels=` of `draw_boxes`, `render_frame`, `render_frame_ragged`: yolo.py:198-224, the filled
  tag in the class colour and '{} {:.2f}'.format(class name, score) in black on it (csrc/labels.hip).  A score in [0, 1] formats
  to one of 101 strings, so an atlas holds all num_classes x 101 labels of each font size, rasterised ONCE on the host by Pillow
  itself with the caller's font -- exactly the "L" mask and offset `ImageDraw.text` would paste (`font.getmask2`) -- and the
  device looks masks up and blends them: Pillow's bytes for any font, layout engine or script.  The font is the caller's: the
  reference's model_data/simhei.ttf is not shipped (pass its path to get the reference's pictures); the default is Pillow's
  built-in face, `ImageFont.load_default(size)`.  label_size is (bbox right, bbox bottom) = `font.getbbox(label)[2:4]` =
  `draw.textbbox((0, 0), label, font)[2:4]`: what the `draw.textsize` the reference calls returned in the Pillow 9 line
  (Pillow 12 has no textsize).  Memory: sum over sizes, classes and k of mask width x height, plus 32 bytes per label
  (`atlas.nbytes`; 7 classes at font size 32 are a few MB).
  The rule (`draw_labels_host` states it in numpy, the kernels equal it byte for byte): the rows of an image are drawn in
  order; row i paints (a) its rings, (b) the rectangle [ox, oy] .. [ox + size_w, oy + size_h], inclusive, clipped, in its
  colour, (ox, oy) = (left, top - size_h) if top - size_h >= 0 else (left, top + 1), (c) its mask at (ox + mask_off_x, oy +
  mask_off_y) in black, clipped: per byte v = DIV255(v * (255 - m)), DIV255(a) = ((a + 128) + ((a + 128) >> 8)) >> 8.  Font
  size `label_font_size(ih)` = floor(3e-2 ih + 0.5) (yolo.py:163); size 0 (frames lower than 17 rows) draws no labels.

* `GlyphAtlas` / `caption_strings` / `draw_captions` / `draw_captions_host`: a second tag UNDER every box with what the
  label atlas cannot hold -- '#<track id> <range>m <closing speed>m/s', e.g. '#17 42.5m -1.2m/s' -- composed on the device
  from the track table and the radar readout (csrc/captions.hip).  The reference has nothing like it: the rule is this
  project's, stated by `caption_strings` (the text; `fixed_tenths` is the integer statement of its '{:.1f}') and
  `draw_captions_host` (the pixels), and the kernels equal both byte for byte.  A caption is the atlas's glyph cells side by
  side with integer widths, NOT Pillow's layout of the whole string: kerning and fractional advances are lost, every single
  glyph is Pillow's bytes.

* `crop_boxes` / `Crops` / `crop_boxes_host` / `crop_layout`: yolo.py:180-193, the `crop` switch of detect_image -- every
  detection cut out of the ORIGINAL frame (the reference crops before it draws), all crops of a batch in one packed arena on
  the device (csrc/crops.hip).  The rule: a row left, top, right, bottom of an image (ih, iw) is clamped again, l = max(left,
  0), t = max(top, 0), r = min(right, iw), bt = min(bottom, ih), w = r - l, h = bt - t, so no read leaves the frame whatever
  the row holds; rows that `box_rows` or the finish kernel made are unchanged by it.  w <= 0 or h <= 0 is an EMPTY crop (Pillow
  gives a zero-size image for w == 0 or h == 0 and raises ValueError for right < left; the reference would crash on saving
  either, so the empty entry is this project's definition); otherwise the crop is frame[t:bt, l:r, :], bit for bit
  np.array(image.crop([left, top, right, bottom])).  The arena's layout is `crop_layout`'s.

* `jpeg_encode` / `Jpegs` / `jpeg_encode_host` / `jpeg_header` / `jpeg_tables`: the `r_image.save(..., quality=95, subsampling=0)`
  of predict.py -- every picture of a batch as a finished baseline JPEG file in a byte arena on the device (csrc/jpeg.hip),
  every byte the one Pillow (libjpeg-turbo) writes at that quality and subsampling (0: 4:4:4, 2: 4:2:0).  `jpeg_encode_host`
  states the rule in numpy, in integers from end to end, and is pinned to live Pillow without a GPU (tests/test_jpeg_host.py).

* `chip_boxes` / `Chips` / `chip_boxes_host` / `chip_geometry` / `chip_resample_host`: the same crops brought to ONE size, the
  way the reference brings any picture to a fixed size (resize_image, utils/utils.py:19-32) -- one (n, sh, sw, 3) tensor of
  equal-sized pictures, and optionally its normalised (n, 3, sh, sw) float form, for a second stage (csrc/chips.hip).
  `chip_boxes_host` states the rule with Pillow itself (crop, THEN resize with BICUBIC; letterbox: resize_image's window on
  grey 128 with nw, nh >= 1), `chip_resample_host` the integer arithmetic the kernels run; both equal Pillow byte for byte.

* `dehaze` / `dehaze_host`: He et al.'s dark-channel-prior dehazing, the reference's image_augmentation_test/dark_channel.py,
  on the raw frames (csrc/dehaze.hip).  `dehaze_host` states the rule in numpy float64, one rounding per operation; the
  kernels equal it bit for bit.

* `ace` / `ace_host`: the fast Automatic Colour Equalisation of the reference's image_augmentation_test/sharpen.py (its
  de-rain enhancement) on the raw frames (csrc/ace.hip).  `ace_host` states the rule in numpy float64, one rounding per
  operation; the kernels equal it byte for byte.

Out of scope: any resize filter but BICUBIC for the chips, image encoding and video I/O."""
import colorsys
import os

import numpy as np
import torch

MAX_COLORS = 256          # RN_MAXCOL of csrc/render.hip
MAX_BOXES = 1024          # RN_MAXBOX: box rows of one image
FLAG_CLASS, FLAG_BOX_COLOUR, FLAG_BOX_ROWS = 1, 2, 4     # bits of the optional `flag` word
FLAG_LABEL_SCORE = 2048   # LB_FLAG_SCORE of csrc/labels.hip: a label score that is NaN or outside [0, 1], clamped
LABEL_SCORES = 101        # the strings 0.00 .. 1.00 a score in [0, 1] formats to
FLAG_CROP_ARENA = 4096    # VR_FLAG_CROP_ARENA of csrc/common.h: a crop that did not fit into the arena, dropped
CROP_RECORD = np.dtype([("offset", "<i4"), ("w", "<i4"), ("h", "<i4"), ("image", "<i4")])      # vrnet_crop_rec, 16 bytes
CHIP_RECORD = np.dtype([(k, "<i4") for k in ("image", "w", "h", "nw", "nh", "dx", "dy", "state")])      # vrnet_chip_rec, 32 bytes
CHIP_MAX = 256            # CH_MAX of csrc/chips.hip: the largest side of a chip
FLAG_DEHAZE = 8192        # VR_FLAG_DEHAZE of csrc/common.h: a degenerate image, returned unchanged by `dehaze`
DEHAZE_MAX_SZ, DEHAZE_MAX_R = 31, 128
FLAG_ACE = 16384          # VR_FLAG_ACE of csrc/common.h: a degenerate image, returned unchanged by `ace`
ACE_MAX_RADIUS, ACE_MAX_BINS = 8, 4096
FLAG_BOX_COUNT = 512      # VR_FLAG_BOX_COUNT of csrc/common.h: a kept count outside [0, cap], clamped (`caption_strings`)
FLAG_CAPTION = 65536      # VR_FLAG_CAPTION of csrc/common.h: a range or a speed that cannot be drawn, left out of its caption
CAPTION_ALPHABET = "0123456789.-+#m/s "          # a glyph code is the index into it
CAPTION_GLYPHS = len(CAPTION_ALPHABET)           # 18
CAPTION_MAX, CAPTION_WORDS = 32, 12              # glyph codes and int32 words of one caption record
CAPTION_MAX_SIDE = 1 << 14                       # CP_MAXDIM of csrc/captions.hip: a cell side is clamped to this
CAPTION_SATURATED = (1 << 31) - 1                # what `fixed_tenths` gives from 2^31 - 1 on, for an infinity and for a NaN

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


def _as_frames(a, what, shapes, fn, empty_ok=False):
    """`_as_u8` of a batch of pictures, (B, ih, iw, 3) with a single picture as B = 1: `what` and `shapes` word the error."""
    img = _as_u8(a, what, 4, fn)
    if img.dim() != 4 or img.shape[-1] != 3 or (min(img.shape) <= 0 and not empty_ok):
        raise RuntimeError(f"{fn}: expected {what} of shape {shapes}, got {tuple(img.shape)}")
    return img


_FRAMES = "(B, ih, iw, 3) or (ih, iw, 3)"


def _host_sizes(sizes, geom, B, ih, iw, fn, also=None):
    """The sizes of B images in slots of (ih, iw), given on the host or in a device table, not in both: the checked (B, 2)
    array of `sizes`, or None without them.  also(b, h, w): the caller's own check of image b, behind the slot check."""
    from . import data
    if sizes is not None and geom is not None:
        raise RuntimeError(f"{fn}: give sizes or a geometry table, not both")
    if sizes is None:
        return None
    arr = data.frame_sizes(sizes, B, fn)
    for b, (h, w) in enumerate(arr.tolist()):
        if h <= 0 or w <= 0 or h > ih or w > iw:
            raise RuntimeError(f"{fn}: image {b}: bad size {h} x {w} in a slot of {ih} x {iw}")
        if also is not None:
            also(b, h, w)
    return arr


def _sizes_geom(arr, dev):
    """The device geometry table of host sizes: ih, iw and a thickness of 1, nothing else."""
    from . import data
    table = np.zeros(len(arr), data.GEOM_DTYPE)
    table["ih"], table["iw"], table["thickness"] = arr[:, 0], arr[:, 1], 1
    return data.geometry_bytes(table).pin_memory().to(dev, non_blocking=True)


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


def _results(fn, results, B, ih, iw, atlas=None, host=True):
    """The host half of handing results to a kernel: the checks, and send(dev, flag) -> (rows (N, 5), offsets (B + 1),
    label_idx (N) or None), int32 tensors on dev.  From the list `non_max_suppression` returns: the rows of `box_rows`, with
    an atlas the label indices of the float32-product scores (their FLAG_LABEL_SCORE bits OR-ed into flag), packed behind
    the offsets into one pinned buffer and sent in a single non-blocking copy.  Or from a device pair (rows, offsets) or
    triple (rows, offsets, label_idx), label_idx (N) int32 = class * 101 + k as `hip.label_index` writes it; an atlas needs
    the triple.  host=False: device tensors only."""
    if isinstance(results, tuple) and len(results) in (2, 3) and all(torch.is_tensor(t) for t in results):
        if atlas is not None and len(results) != 3:
            raise RuntimeError(f"{fn}: with labels, device results are the triple (rows, offsets, label_idx)")
        rows, offsets = results[:2]
        if rows.dtype != torch.int32 or offsets.dtype != torch.int32 or rows.dim() != 2 or rows.shape[1] != 5 or \
                tuple(offsets.shape) != (B + 1,):
            raise RuntimeError(f"{fn}: expected int32 rows (N, 5) and offsets ({B + 1},), got {tuple(rows.shape)} "
                               f"{rows.dtype} and {tuple(offsets.shape)} {offsets.dtype}")
        keep = results if atlas is not None else (rows, offsets, None)
        return lambda dev, flag: tuple(None if t is None else t.to(dev).contiguous() for t in keep)
    if not host:
        raise RuntimeError(f"{fn}: with a geometry table the results are device tensors (rows, offsets[, label_idx])")
    if results is None or len(results) != B:
        raise RuntimeError(f"{fn}: {0 if results is None else len(results)} result entries for {B} frames")
    host_rows, host_offsets, _, _ = box_rows(results, (ih, iw), MAX_COLORS)
    if int(np.diff(host_offsets).max(initial=0)) > MAX_BOXES:
        raise RuntimeError(f"{fn}: more than {MAX_BOXES} boxes in one image")
    parts, bits, n = [host_offsets, host_rows.reshape(-1)], 0, host_rows.size
    if atlas is not None:
        host_idx, bits = _host_label_idx(results, host_rows, atlas)
        parts.append(host_idx)

    def send(dev, flag):
        packed = torch.empty(sum(p.size for p in parts), dtype=torch.int32).pin_memory()
        torch.cat([torch.from_numpy(p) for p in parts], out=packed)
        packed = packed.to(dev, non_blocking=True)
        if bits and flag is not None:
            flag.bitwise_or_(bits)
        return packed[B + 1:B + 1 + n].view(-1, 5), packed[:B + 1], packed[B + 1 + n:] if atlas is not None else None
    return send


def render_frame(frames_u8, class_map=None, results=None, input_shape=None, palette=None, mix_type=0, alpha=0.7,
                 count=False, box_palette=None, thickness=None, out=None, flag=None, device="cuda", labels=None,
                 font_size=None, geom=None, label_sizes=None, fn="render"):
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
    synchronise.  labels: a `LabelAtlas` -- the class names and scores of yolo.py:210-224 are drawn over the finished
    picture by `draw_labels` (font_size: default `label_font_size(ih)`); device results are then the triple (rows, offsets,
    label_idx (N) int32 = class * 101 + k, as `hip.label_index` writes it).  With labels=None nothing about the call changes.
    Returns out, or (out, counts) with counts (B, len(palette)) int64 when count=True.  No host synchronisation.
    geom: the (B, hip.GEOM_BYTES) device table of `data.frame_geometry` for a batch of images of their own sizes
    (vrnet_render_ragged_u8).  frames_u8 (B, ihm, iwm, 3) and class_map (B, ihm, iwm) are then padded uint8 DEVICE tensors with
    image b in the top-left corner of slot b, results device tensors as `hip.detect_finish` leaves them, and the table gives
    every image its size, its outline thickness and its font size: input_shape, thickness and font_size stay away, and
    labels need label_sizes, the (B) int32 device table of `atlas.size_table` (the font size of each image as an index into
    the atlas, -1 for an image without labels).  Image b of the result is `out[b, :ih_b, :iw_b]`, equal to the call without a
    table on that image alone; every pixel outside it is 0 and is not counted.  out must not be the frames.  flag also
    receives hip.FLAG_GEOMETRY."""
    from . import hip
    table = hip._table_call(fn, geom, (("input_shape", input_shape, None), ("thickness", thickness, None),
                                      ("font_size", font_size, None)), (("label_sizes", label_sizes, None),))
    if table and not (torch.is_tensor(frames_u8) and frames_u8.is_cuda and frames_u8.dtype == torch.uint8 and frames_u8.dim() == 4):
        raise RuntimeError(f"{fn}: expected padded uint8 frames (B, ihm, iwm, 3) on a GPU")
    img = _as_frames(frames_u8, "frames", _FRAMES, fn, empty_ok=True)
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
    bpal = None
    if labels is not None:
        if results is None:
            raise RuntimeError(f"{fn}: labels need results")
        if table and label_sizes is None:
            raise RuntimeError(f"{fn}: labels need the device triple (rows, offsets, label_idx) and label_sizes")
        font_size = _label_setup(labels, 0 if table else font_size, ih, fn)
    if results is not None:
        if thickness is None and not table:
            if input_shape is None:
                raise RuntimeError(f"{fn}: boxes need a thickness or the input_shape it follows from")
            thickness = int(max((iw + ih) // np.mean(input_shape), 1))
        if not table and int(thickness) < 1:
            raise RuntimeError(f"{fn}: thickness must be at least 1, got {thickness!r}")
        bpal = _palette(box_palette, det_palette(4) if labels is None else det_palette(labels.num_classes), fn)
        if labels is not None:
            _label_palette(labels, bpal, fn)
        send = _results(fn, results, B, ih, iw, labels, host=not table)
    img = img.to(img.device if table else device, non_blocking=True).contiguous()
    dev = img.device
    cmap = None if cmap is None else cmap.to(dev, non_blocking=True).contiguous()
    with torch.cuda.device(dev):
        rows, offsets, label_idx = (None, None, None) if results is None else send(dev, flag)
        if out is None:
            out = torch.empty((B, ih, iw, 3), dtype=torch.uint8, device=dev)
        counts = torch.empty((B, pal.shape[0]), dtype=torch.int64, device=dev) if count else None
        hip.render(img, cmap, out, palette=None if pal is None else _palette_on(pal, dev), mix_type=mix_type, alpha=alpha,
                   boxes=rows, box_offsets=offsets, box_palette=None if bpal is None else _palette_on(bpal, dev),
                   thickness=1 if thickness is None else int(thickness), counts=counts, flag=flag, geom=geom, fn=fn)
        if labels is not None and (table or font_size > 0):
            blob, records = labels.on(dev)
            hip.render_labels(out, rows, offsets, _palette_on(bpal, dev), None if table else int(thickness), label_idx, blob, records,
                              label_sizes if table else labels.size_index(font_size), flag=flag, geom=geom,
                              fn=fn.replace("render", "render_labels"))
    return (out, counts) if count else out


def render_frame_ragged(frames_u8, geom, class_map=None, results=None, palette=None, mix_type=0, alpha=0.7, count=False,
                        box_palette=None, out=None, flag=None, labels=None, label_sizes=None):
    """`render_frame` with a geometry table, under its earlier name."""
    return render_frame(frames_u8, class_map, results, None, palette, mix_type, alpha, count, box_palette, out=out, flag=flag,
                        labels=labels, geom=geom, label_sizes=label_sizes, fn="render_ragged")


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
    """(window, dx, dy, nw, nh) of a call without a geometry table."""
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
    whole level map; True: through the window of `decode.seg_window` (module docstring).  No host synchronisation.  This is
    `heatmap` without the picture."""
    return heatmap(None, outputs, input_shape, letterbox_image, image_shape=image_shape)[1]


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


def heatmap(frames_u8, outputs, input_shape, letterbox_image=False, alpha=0.5, cmap=None, out=None, geom=None, window=True,
            flag=None, image_shape=None, fn="heatmap"):
    """yolo.py:288-351 `detect_heatmap` on the device: frames_u8 (B, ih, iw, 3) uint8 RGB original frames (numpy or tensor; a
    single (ih, iw, 3) frame counts as B = 1) and outputs as in `heatmap_mask`.  Returns (picture, mask, minmax): picture
    (B, ih, iw, 3) uint8 = Image.blend(frame, cmap[index(mask)], alpha) with matplotlib's default normalisation per image
    (module docstring), mask (B, ih, iw) uint8, minmax (B, 2) int32 = each mask's (min, max).  cmap: a (256, 3) uint8 table,
    default `jet_lut()`.  out: the device tensor to write the picture into; it must not alias the frames.  No host
    synchronisation.  frames_u8=None with image_shape = (ih, iw): no picture (None), the mask and its range alone.
    geom: the (B, hip.GEOM_BYTES) device table of `data.frame_geometry` for a batch of images of their own sizes
    (vrnet_heatmap_ragged_f32): frames_u8 (B, ihm, iwm, 3) are then padded uint8 DEVICE slots with image b in the top-left
    corner.  window=True maps the pixels of image b through its letterbox window (dx, dy, nw, nh) of the table (the whole
    input for a table made with letterbox_image=False), window=False is the reference's whole-map resize: window says with a
    table what letterbox_image says without one.  Image b of the results is `[b, :ih_b, :iw_b]`, equal to the call without a
    table on that image alone; every pixel outside it is 0 and minmax[b] covers the image's own pixels.  flag: an int32
    device word for hip.FLAG_GEOMETRY, or None."""
    from . import hip
    table = hip._table_call(fn, geom, (("letterbox_image", letterbox_image, False),), (("window", window, True),))
    B, (H, W) = _heat_levels(outputs, input_shape, fn)
    img = lut = None
    if frames_u8 is not None:
        img = _heat_frames(frames_u8, not table, out, fn)
        if img.shape[0] != B:
            raise RuntimeError(f"{fn}: {img.shape[0]} frame{' slot' * table}s for outputs of {B} images")
        image_shape, lut = img.shape[1:3], _heat_common(alpha, cmap, fn)
    ih, iw = int(image_shape[0]), int(image_shape[1])
    if ih <= 0 or iw <= 0:
        raise RuntimeError(f"{fn}: bad image_shape {tuple(image_shape)}")
    scalars = (1 if window else 0,) if table else _heat_window((H, W), (ih, iw), letterbox_image)
    levels = _heat_device(outputs, fn)
    dev = levels[0].device
    if table and img is not None and img.device != dev:
        raise RuntimeError(f"{fn}: the frames must be on the outputs' device {dev}")
    img = None if img is None else img.to(dev, non_blocking=True).contiguous()
    with torch.cuda.device(dev):
        picture = out if out is not None or img is None else torch.empty((B, ih, iw, 3), dtype=torch.uint8, device=dev)
        mask = torch.empty((B, ih, iw), dtype=torch.uint8, device=dev)
        minmax = torch.empty((B, 2), dtype=torch.int32, device=dev)
        need = (hip.heatmap_ragged_workspace_bytes if table else hip.heatmap_workspace_bytes)(B, H, W)
        hip.heatmap(levels, H, W, mask, minmax, torch.empty(need, dtype=torch.uint8, device=dev), *scalars, frames=img,
                    cmap=None if lut is None else _palette_on(lut, dev), alpha=alpha, out=picture, geom=geom, flag=flag, fn=fn)
    return picture, mask, minmax


def heatmap_ragged(frames_u8, outputs, geom, input_shape, window=True, alpha=0.5, cmap=None, out=None, flag=None):
    """`heatmap` with a geometry table, under its earlier name."""
    return heatmap(frames_u8, outputs, input_shape, False, alpha, cmap, out, geom, window, flag, fn="heatmap_ragged")


def seg_render(frames_u8, class_map, palette=None, mix_type=0, alpha=0.7, count=False, out=None, flag=None, device="cuda"):
    """deeplab.py:169-222 on the device: frames_u8 (B,ih,iw,3) uint8 original frames and class_map (B,ih,iw) uint8 (what
    `decode.seg_predict` returns) -> the (B,ih,iw,3) uint8 picture of mix_type 0 (Image.blend(frame, palette[class], alpha),
    Pillow's bytes), 1 (palette[class]) or 2 (the frame where class != 0, else 0); with count=True also the (B, len(palette))
    int64 pixels of each class per image (:172-185).  See `render_frame` for the arguments."""
    if class_map is None:
        raise RuntimeError("render: seg_render needs a class map")
    return render_frame(frames_u8, class_map, None, None, palette, mix_type, alpha, count, out=out, flag=flag, device=device)


def draw_boxes(frames_u8, results, input_shape, palette=None, thickness=None, out=None, flag=None, device="cuda", labels=None):
    """yolo.py:164-222: `box_rows` of the list `non_max_suppression` returns plus the kernel -- `thickness` nested outlines
    per box in palette[class] (default `det_palette(4)`), later boxes over earlier ones; with labels=a `LabelAtlas` also the
    tag and the text of every box (yolo.py:210-224), without it the outlines alone.  out may be the frames tensor itself
    (drawn in place).  One non-blocking host-to-device copy of the packed rows."""
    if results is None:
        raise RuntimeError("render: draw_boxes needs the results of non_max_suppression")
    return render_frame(frames_u8, None, results, input_shape, box_palette=palette, thickness=thickness, out=out, flag=flag,
                        device=device, labels=labels)


# ---- class names and scores (csrc/labels.hip) --------------------------------------------------------------------------------
def label_font_size(ih):
    """The font size of yolo.py:163 for a frame of ih rows: int(floor(3e-2 * ih + 0.5)); 0 below 17 rows (no labels)."""
    return int(np.floor(3e-2 * int(ih) + 0.5))


def score_index(scores, return_flag=False):
    """k = int('{:.2f}'.format(float(s)).replace('.', '')) for float32 scores in [0, 1], as an int32 array of the same shape:
    the exact value of the float32 times 100, rounded to nearest with ties to even (0.125 -> 12, 0.375 -> 38), in integer
    arithmetic on the bits -- never score * 100 in floating point.  NaN or a score outside [0, 1] is clamped into 0..100 (NaN
    and negatives to 0, above 1 to 100); return_flag=True returns (k, bits) with bits = FLAG_LABEL_SCORE if any score was."""
    s = np.asarray(scores)
    if s.dtype != np.float32:
        raise RuntimeError(f"score_index: expected float32 scores, got {s.dtype}")
    s = np.ascontiguousarray(s)
    bits = s.view(np.uint32).astype(np.uint64)
    e = (bits >> np.uint64(23)) & np.uint64(255)
    m = (bits & np.uint64(0x7FFFFF)) | np.where(e > 0, np.uint64(0x800000), np.uint64(0))
    sh = 150 - np.maximum(e.astype(np.int64), 1)                       # s = m 2^-sh; sh >= 23 for s <= 1
    shc = np.clip(sh, 1, 63).astype(np.uint64)
    N = np.uint64(100) * m
    q, rem, half = N >> shc, N & ((np.uint64(1) << shc) - np.uint64(1)), np.uint64(1) << (shc - np.uint64(1))
    k = (q + ((rem > half) | ((rem == half) & ((q & np.uint64(1)) == 1))).astype(np.uint64)).astype(np.int64)
    k = np.where(sh >= 32, 0, k)                                       # 100 m < 2^31: below half a unit
    with np.errstate(invalid="ignore"):
        bad = ~((s >= 0) & (s <= 1))
        k = np.where(bad, np.where(s > 1, 100, 0), k).astype(np.int32)
    return (k, FLAG_LABEL_SCORE if bool(bad.any()) else 0) if return_flag else k


class LabelAtlas:
    """Every label an image can show, rasterised once on the host by Pillow: for each font size in `sizes` (each >= 1), each
    class c and each k in 0..100 the label f"{name} {k / 100:.2f}" as `ImageDraw.text` would paste it -- the "L" mask and
    its offset, `font.getmask2(label, "L")` with a fractional start of 0 (origins are integers) -- and label_size =
    `font.getbbox(label)[2:4]` (module docstring).  font: the path of a TrueType file, a callable size -> PIL.ImageFont, or
    None = `ImageFont.load_default(size)`.  Pillow is imported here and only here; without it this raises.
    blob: all masks as one uint8 array; records (len(sizes), num_classes * 101, 8) int32 = blob offset, mask width, mask
    height, mask offset x, mask offset y, label_size width, label_size height, 0, indexed [size index][c * 101 + k]; both go
    to a device once (`on`) and are kept, as the palettes are.  nbytes: their size; a blob of 2 GiB or more raises."""

    def __init__(self, class_names, font=None, sizes=(32,)):
        names, sizes = self._check(class_names, sizes)
        try:
            from PIL import ImageFont
        except ImportError:
            raise RuntimeError("LabelAtlas: rasterising labels needs Pillow (pip install pillow); everything else in this "
                               "module works without it") from None
        if font is None:
            make = ImageFont.load_default
        elif callable(font):
            make = font
        else:
            make = lambda size: ImageFont.truetype(os.fspath(font), size)      # noqa: E731
        masks, total = [], 0
        records = np.zeros((len(sizes), len(names) * LABEL_SCORES, 8), np.int32)
        for si, size in enumerate(sizes):
            f = make(size)
            for c, name in enumerate(names):
                for k in range(LABEL_SCORES):
                    label = f"{name} {k / 100:.2f}"
                    mask, (mw, mh), off = _label_mask(f, label)
                    bbox = f.getbbox(label)
                    if total + mask.size >= 1 << 31:
                        raise RuntimeError("LabelAtlas: the masks need 2 GiB or more; build fewer sizes or classes")
                    records[si, c * LABEL_SCORES + k, :7] = (total, mw, mh, int(off[0]), int(off[1]), int(bbox[2]), int(bbox[3]))
                    masks.append(mask)
                    total += mask.size
        self._set(names, sizes, np.concatenate(masks) if total else np.zeros(0, np.uint8), records)

    @staticmethod
    def _check(class_names, sizes):
        names = [str(n) for n in class_names]
        if not 1 <= len(names) <= MAX_COLORS:
            raise RuntimeError(f"LabelAtlas: 1..{MAX_COLORS} class names, got {len(names)}")
        try:
            sizes = tuple(int(v) for v in sizes)
        except (TypeError, ValueError):
            raise RuntimeError(f"LabelAtlas: sizes is a sequence of font sizes, got {sizes!r}") from None
        if not sizes or min(sizes) < 1 or len(set(sizes)) != len(sizes):
            raise RuntimeError(f"LabelAtlas: sizes must be distinct font sizes >= 1, got {sizes!r}")
        return names, sizes

    def _set(self, names, sizes, blob, records):
        if blob.dtype != np.uint8 or blob.ndim != 1 or records.dtype != np.int32 or \
                records.shape != (len(sizes), len(names) * LABEL_SCORES, 8):
            raise RuntimeError("LabelAtlas: expected a 1-D uint8 blob and int32 records of shape (sizes, classes * 101, 8)")
        if blob.size >= 1 << 31:
            raise RuntimeError("LabelAtlas: the masks need 2 GiB or more; build fewer sizes or classes")
        r = records.astype(np.int64)
        if (r[..., :3] < 0).any() or (r[..., 5:7] < 0).any() or (r[..., 0] + r[..., 1] * r[..., 2] > blob.size).any():
            raise RuntimeError("LabelAtlas: a record points outside the blob")
        self.class_names, self.sizes = tuple(names), tuple(sizes)
        self.blob, self.records = np.ascontiguousarray(blob), np.ascontiguousarray(records)
        self._index = {s: i for i, s in enumerate(self.sizes)}
        self._device = {}

    @classmethod
    def from_arrays(cls, class_names, sizes, blob, records):
        """An atlas from the arrays of another one (`save` / `load`): no font and no Pillow needed."""
        self = cls.__new__(cls)
        names, sizes = cls._check(class_names, sizes)
        self._set(names, sizes, np.asarray(blob), np.asarray(records))
        return self

    def save(self, path):
        np.savez_compressed(path, class_names=np.array(self.class_names), sizes=np.array(self.sizes, np.int32), blob=self.blob,
                            records=self.records)

    @classmethod
    def load(cls, path):
        with np.load(path, allow_pickle=False) as z:
            return cls.from_arrays([str(n) for n in z["class_names"]], z["sizes"], z["blob"], z["records"])

    @property
    def num_classes(self):
        return len(self.class_names)

    @property
    def nbytes(self):
        return int(self.blob.nbytes + self.records.nbytes)

    def size_index(self, font_size):
        """The row of `records` that holds font_size; raises for a size that was not built."""
        i = self._index.get(int(font_size))
        if i is None:
            raise RuntimeError(f"LabelAtlas: font size {int(font_size)} was not built (sizes: {self.sizes})")
        return i

    def size_table(self, heights, fn="LabelAtlas"):
        """The (B) int32 table of `render_frame_ragged` for images of these heights: the size index of
        `label_font_size(ih)`, -1 where that is 0; raises, naming the image, for a size that was not built."""
        tab = np.empty(len(heights), np.int32)
        for b, ih in enumerate(heights):
            size = label_font_size(ih)
            if size > 0 and size not in self._index:
                raise RuntimeError(f"{fn}: image {b} of {int(ih)} rows needs font size {size}, which the atlas was not built "
                                   f"for (sizes: {self.sizes})")
            tab[b] = self._index[size] if size > 0 else -1
        return tab

    def record(self, font_size, c, k):
        """(mask (h, w) uint8, (mask offset x, y), (label_size w, h)) of class c at score index k."""
        off, mw, mh, mox, moy, lw, lh, _ = (int(v) for v in self.records[self.size_index(font_size), c * LABEL_SCORES + k])
        return self.blob[off:off + mw * mh].reshape(mh, mw), (mox, moy), (lw, lh)

    def on(self, device):
        """(blob, records) as tensors on the device; copied once per device and kept."""
        key = str(torch.device(device))
        t = self._device.get(key)
        if t is None:
            t = self._device[key] = (torch.from_numpy(self.blob).to(device), torch.from_numpy(self.records).to(device))
        return t


def _label_mask(font, label):
    """What `ImageDraw.text((x, y), label, font=font)` pastes on an RGB image at integer (x, y): (mask bytes, (w, h), offset)."""
    from PIL import Image
    try:
        mask, off = font.getmask2(label, "L")
    except AttributeError:                    # a bitmap font: ImageDraw.text falls back to getmask, offset 0
        mask, off = font.getmask(label, "L"), (0, 0)
    w, h = mask.size
    if w <= 0 or h <= 0:
        return np.zeros(0, np.uint8), (0, 0), off
    return np.frombuffer(Image.Image()._new(mask).tobytes(), np.uint8), (w, h), off


def _label_setup(atlas, font_size, ih, fn):
    if not isinstance(atlas, LabelAtlas):
        raise RuntimeError(f"{fn}: labels must be a render.LabelAtlas, got {type(atlas).__name__}")
    font_size = label_font_size(ih) if font_size is None else int(font_size)
    if font_size < 0:
        raise RuntimeError(f"{fn}: font_size must not be negative, got {font_size}")
    if font_size > 0:
        atlas.size_index(font_size)
    return font_size


def _label_palette(atlas, bpal, fn):
    if bpal.shape[0] != atlas.num_classes:
        raise RuntimeError(f"{fn}: the atlas has {atlas.num_classes} classes, the box palette {bpal.shape[0]} colours")


def _host_label_idx(results, host_rows, atlas):
    """class * 101 + k per packed draw row of the list `non_max_suppression` returns, and the score flag bits: the score is
    np.float32(obj) * np.float32(class_conf), one float32 multiply (yolo.py:157); the class is clamped as the colour is."""
    parts = [np.zeros((0, 7), np.float32) if d is None else np.asarray(d) for d in results]
    det = np.concatenate(parts) if parts else np.zeros((0, 7), np.float32)
    k, bits = score_index(det[:, 4].astype(np.float32) * det[:, 5].astype(np.float32), True)
    cls = np.clip(host_rows[:, 4].astype(np.int64), 0, atlas.num_classes - 1)
    return (cls * LABEL_SCORES + k).astype(np.int32), bits


def _div255(a):
    a = a + 128
    return (a + (a >> 8)) >> 8


def draw_labels_host(picture, rows, scores, atlas, font_size, thickness, box_palette=None):
    """The rule of the module docstring in numpy, for ONE image: picture (ih, iw, 3) uint8 (with or without the outlines
    already on it: they are painted again), rows (n, 5) int32 = left, top, right, bottom, class as `box_rows` gives them,
    scores (n) float32 = obj * class_conf.  The rows are drawn in order -- rings, tag, text -- as yolo.py:198-224 draws
    them; rows past MAX_BOXES are ignored.  Returns the new picture; font_size 0 draws the rings only.  This is the statement
    the kernels of csrc/labels.hip are tested against; tests/test_labels_host.py pins it to live Pillow."""
    fn = "draw_labels_host"
    pic, rows, scores = np.asarray(picture), np.asarray(rows), np.asarray(scores)
    if pic.dtype != np.uint8 or pic.ndim != 3 or pic.shape[2] != 3:
        raise RuntimeError(f"{fn}: expected a uint8 picture (ih, iw, 3), got {pic.dtype} {pic.shape}")
    if rows.dtype != np.int32 or rows.ndim != 2 or rows.shape[1] != 5:
        raise RuntimeError(f"{fn}: expected int32 rows (n, 5), got {rows.dtype} {rows.shape}")
    if scores.dtype != np.float32 or scores.shape != (len(rows),):
        raise RuntimeError(f"{fn}: expected float32 scores ({len(rows)},), got {scores.dtype} {scores.shape}")
    if int(thickness) < 1:
        raise RuntimeError(f"{fn}: thickness must be at least 1, got {thickness!r}")
    font_size = _label_setup(atlas, font_size, pic.shape[0], fn)
    pal = _palette(box_palette, det_palette(atlas.num_classes), fn)
    pal = pal.cpu().numpy() if torch.is_tensor(pal) else pal
    _label_palette(atlas, pal, fn)
    out = pic.copy()
    ih, iw = out.shape[:2]
    ks = score_index(scores)

    def fill(x0, y0, x1, y1, colour):             # the inclusive rectangle, clipped
        x0, y0, x1, y1 = max(x0, 0), max(y0, 0), min(x1, iw - 1), min(y1, ih - 1)
        if x0 <= x1 and y0 <= y1:
            out[y0:y1 + 1, x0:x1 + 1] = colour

    for (left, top, right, bottom, cls), k in zip(rows[:MAX_BOXES].tolist(), ks[:MAX_BOXES].tolist()):
        c = min(max(cls, 0), atlas.num_classes - 1)
        colour = pal[c]
        for i in range(int(thickness)):           # (a) the perimeter of each ring
            l, t, r, b = left + i, top + i, right - i, bottom - i
            if l > r or t > b:
                break
            fill(l, t, r, t, colour)
            fill(l, b, r, b, colour)
            fill(l, t, l, b, colour)
            fill(r, t, r, b, colour)
        if font_size == 0:
            continue
        mask, (mox, moy), (lw, lh) = atlas.record(font_size, c, k)
        ox, oy = (left, top - lh) if top - lh >= 0 else (left, top + 1)
        fill(ox, oy, ox + lw, oy + lh, colour)    # (b) the tag
        tx, ty = ox + mox, oy + moy               # (c) the text, black through the mask
        x0, y0, x1, y1 = max(tx, 0), max(ty, 0), min(tx + mask.shape[1], iw), min(ty + mask.shape[0], ih)
        if x0 < x1 and y0 < y1:
            m = mask[y0 - ty:y1 - ty, x0 - tx:x1 - tx].astype(np.int64)[..., None]
            out[y0:y1, x0:x1] = _div255(out[y0:y1, x0:x1].astype(np.int64) * (255 - m)).astype(np.uint8)
    return out


def draw_labels(picture, results, atlas, input_shape=None, thickness=None, font_size=None, box_palette=None, flag=None):
    """yolo.py:210-224 on the device, in place on the (B, ih, iw, 3) uint8 DEVICE picture `render_frame` / `draw_boxes`
    finished with the same results, palette and thickness (vrnet_render_labels_u8).  results: the list `non_max_suppression`
    returns -- the host packs the rows, the float32-product scores' indices and the offsets and sends them in one
    non-blocking copy -- or a device triple (rows (N, 5), offsets (B + 1), label_idx (N)) of int32 tensors.  thickness:
    default yolo.py:164 from input_shape; font_size: default `label_font_size(ih)`, 0 draws nothing; box_palette: default
    `det_palette(atlas.num_classes)`; flag: as in `render_frame`, plus FLAG_LABEL_SCORE.  Returns the picture.  No host
    synchronisation."""
    from . import hip
    fn = "draw_labels"
    if not (torch.is_tensor(picture) and picture.is_cuda and picture.dtype == torch.uint8 and picture.dim() == 4 and
            picture.shape[-1] == 3 and picture.is_contiguous()):
        raise RuntimeError(f"{fn}: expected a contiguous uint8 picture (B, ih, iw, 3) on a GPU")
    B, ih, iw = picture.shape[:3]
    font_size = _label_setup(atlas, font_size, ih, fn)
    bpal = _palette(box_palette, det_palette(atlas.num_classes), fn)
    _label_palette(atlas, bpal, fn)
    if thickness is None:
        if input_shape is None:
            raise RuntimeError(f"{fn}: labels need a thickness or the input_shape it follows from")
        thickness = int(max((iw + ih) // np.mean(input_shape), 1))
    if int(thickness) < 1:
        raise RuntimeError(f"{fn}: thickness must be at least 1, got {thickness!r}")
    send, dev = _results(fn, results, B, ih, iw, atlas), picture.device
    with torch.cuda.device(dev):
        rows, offsets, label_idx = send(dev, flag)
        if font_size > 0:
            blob, records = atlas.on(dev)
            hip.render_labels(picture, rows, offsets, _palette_on(bpal, dev), int(thickness), label_idx, blob, records,
                              atlas.size_index(font_size), flag=flag)
    return picture


# ---- track ids, radar range and closing speed under the detections (csrc/captions.hip) ---------------------------------------
def fixed_tenths(values):
    """(k, negative) of float32 values, arrays of the same shape: k int32 = the exact value of |x| times 10, rounded to nearest
    with ties to even on the exact binary value (0.25 -> 2, 0.75 -> 8), in integer arithmetic on the bits -- `score_index`
    with one decimal and no range limit -- saturated at 2^31 - 1, which is also what an infinity or a NaN gives; negative bool =
    the sign bit.  So '{:.1f}'.format(float(x)) is ('-' if negative else '') + f'{k // 10}.{k % 10}' wherever k is below
    the saturation, -0.04 -> '-0.0' included.  csrc/captions.hip mirrors this line by line."""
    s = np.asarray(values)
    if s.dtype != np.float32:
        raise RuntimeError(f"fixed_tenths: expected float32 values, got {s.dtype}")
    bits = np.ascontiguousarray(s).view(np.uint32).astype(np.uint64)
    e = ((bits >> np.uint64(23)) & np.uint64(255)).astype(np.int64)
    m = (bits & np.uint64(0x7FFFFF)) | np.where(e > 0, np.uint64(0x800000), np.uint64(0))
    sh = 150 - np.maximum(e, 1)                                        # |x| = m 2^-sh
    N = np.uint64(10) * m                                              # below 2^28
    shr = np.clip(sh, 1, 63).astype(np.uint64)
    q, rem, half = N >> shr, N & ((np.uint64(1) << shr) - np.uint64(1)), np.uint64(1) << (shr - np.uint64(1))
    down = (q + ((rem > half) | ((rem == half) & ((q & np.uint64(1)) == 1))).astype(np.uint64)).astype(np.int64)
    up = np.minimum(N << np.clip(-sh, 0, 31).astype(np.uint64), np.uint64(CAPTION_SATURATED)).astype(np.int64)
    k = np.where(sh >= 1, down, np.where(sh < -31, CAPTION_SATURATED, up))
    k = np.where(e == 255, CAPTION_SATURATED, k).astype(np.int32)
    return k.reshape(s.shape), (bits >> np.uint64(31)).astype(bool).reshape(s.shape)


class GlyphAtlas:
    """The 18 glyphs of CAPTION_ALPHABET, rasterised once on the host by Pillow, for each font size in `sizes` (each >= 1).
    font: as `LabelAtlas` takes it -- the path of a TrueType file, a callable size -> PIL.ImageFont, or None =
    `ImageFont.load_default(size)`.  Pillow is imported here and only here; without it this raises.
    A glyph's mask and offset (mox, moy) are `_label_mask(font, ch)`'s, what `ImageDraw.text` would paste, and adv =
    ceil(font.getlength(ch)).  Its CELL is the union of the advance box [0, adv) and the mask's extent [mox, mox + mw): width
    max(adv, mox + mw) - min(mox, 0), at least 1, the mask pasted into the zeroed cell at column mox - min(mox, 0), so nothing
    of a glyph is clipped (the built-in face has mox = -1 for '/', '3' and 's' at some sizes).  All cells of a size share the
    height cell_h = max(moy + mh) - min(0, min moy) over the alphabet; a mask sits at row moy - min(0, min moy).
    A caption is cells side by side with integer widths -- NOT Pillow's layout of the whole string: kerning and fractional
    advances are lost; every single glyph is Pillow's bytes.
    blob: the cells as uint8, row-major, back to back; records (len(sizes), 18, 4) int32 = blob offset, cell width, cell
    height, 0; both go to a device once (`on`) and are kept.  nbytes: their size."""

    def __init__(self, font=None, sizes=(32,)):
        sizes = self._check(sizes)
        try:
            from PIL import ImageFont
        except ImportError:
            raise RuntimeError("GlyphAtlas: rasterising glyphs needs Pillow (pip install pillow); everything else in this "
                               "module works without it") from None
        if font is None:
            make = ImageFont.load_default
        elif callable(font):
            make = font
        else:
            make = lambda size: ImageFont.truetype(os.fspath(font), size)      # noqa: E731
        cells, total = [], 0
        records = np.zeros((len(sizes), CAPTION_GLYPHS, 4), np.int32)
        for si, size in enumerate(sizes):
            f = make(size)
            glyphs = []
            for ch in CAPTION_ALPHABET:
                mask, (mw, mh), off = _label_mask(f, ch)
                glyphs.append((mask.reshape(mh, mw), int(off[0]), int(off[1]), int(np.ceil(f.getlength(ch)))))
            up = -min(0, min(moy for _, _, moy, _ in glyphs))
            cell_h = max(moy + m.shape[0] for m, _, moy, _ in glyphs) + up
            for c, (m, mox, moy, adv) in enumerate(glyphs):
                left = -min(mox, 0)
                cw = max(max(adv, mox + m.shape[1]) + left, 1)
                cell = np.zeros((cell_h, cw), np.uint8)
                cell[moy + up:moy + up + m.shape[0], mox + left:mox + left + m.shape[1]] = m
                records[si, c, :3] = (total, cw, cell_h)
                cells.append(cell.reshape(-1))
                total += cell.size
        self._set(sizes, np.concatenate(cells), records)

    @staticmethod
    def _check(sizes):
        try:
            sizes = tuple(int(v) for v in sizes)
        except (TypeError, ValueError):
            raise RuntimeError(f"GlyphAtlas: sizes is a sequence of font sizes, got {sizes!r}") from None
        if not sizes or min(sizes) < 1 or len(set(sizes)) != len(sizes):
            raise RuntimeError(f"GlyphAtlas: sizes must be distinct font sizes >= 1, got {sizes!r}")
        return sizes

    def _set(self, sizes, blob, records):
        if blob.dtype != np.uint8 or blob.ndim != 1 or records.dtype != np.int32 or records.shape != (len(sizes), CAPTION_GLYPHS, 4):
            raise RuntimeError(f"GlyphAtlas: expected a 1-D uint8 blob and int32 records of shape (sizes, {CAPTION_GLYPHS}, 4)")
        r = records.astype(np.int64)
        if blob.size >= 1 << 31 or (r[..., 0] < 0).any() or (r[..., 1] < 1).any() or (r[..., 2] < 0).any() or \
                (r[..., 1:3] > CAPTION_MAX_SIDE).any() or (r[..., 0] + r[..., 1] * r[..., 2] > blob.size).any():
            raise RuntimeError(f"GlyphAtlas: a record points outside the blob, or a cell side outside [1, {CAPTION_MAX_SIDE}]")
        if (r[..., 2] != r[:, :1, 2]).any():
            raise RuntimeError("GlyphAtlas: the cells of one font size share one height")
        self.sizes = tuple(sizes)
        self.blob, self.records = np.ascontiguousarray(blob), np.ascontiguousarray(records)
        self._index = {s: i for i, s in enumerate(self.sizes)}
        self._device = {}

    @classmethod
    def from_arrays(cls, sizes, blob, records):
        """An atlas from the arrays of another one (`save` / `load`): no font and no Pillow needed."""
        self = cls.__new__(cls)
        self._set(cls._check(sizes), np.asarray(blob), np.asarray(records))
        return self

    def save(self, path):
        np.savez_compressed(path, sizes=np.array(self.sizes, np.int32), blob=self.blob, records=self.records)

    @classmethod
    def load(cls, path):
        with np.load(path, allow_pickle=False) as z:
            return cls.from_arrays(z["sizes"], z["blob"], z["records"])

    @property
    def nbytes(self):
        return int(self.blob.nbytes + self.records.nbytes)

    def size_index(self, font_size):
        """The row of `records` that holds font_size; raises for a size that was not built."""
        i = self._index.get(int(font_size))
        if i is None:
            raise RuntimeError(f"GlyphAtlas: font size {int(font_size)} was not built (sizes: {self.sizes})")
        return i

    def size_table(self, heights, fn="GlyphAtlas"):
        """The (B) int32 table of a ragged `draw_captions` for images of these heights: the size index of
        `label_font_size(ih)`, -1 where that is 0; raises, naming the image, for a size that was not built."""
        tab = np.empty(len(heights), np.int32)
        for b, ih in enumerate(heights):
            size = label_font_size(ih)
            if size > 0 and size not in self._index:
                raise RuntimeError(f"{fn}: image {b} of {int(ih)} rows needs font size {size}, which the glyph atlas was not "
                                   f"built for (sizes: {self.sizes})")
            tab[b] = self._index[size] if size > 0 else -1
        return tab

    def cell(self, font_size, code):
        """The (cell_h, width) uint8 cell of glyph `code` at font_size."""
        off, cw, ch, _ = (int(v) for v in self.records[self.size_index(font_size), code])
        return self.blob[off:off + cw * ch].reshape(ch, cw)

    def on(self, device):
        """(blob, records) as tensors on the device; copied once per device and kept."""
        key = str(torch.device(device))
        t = self._device.get(key)
        if t is None:
            t = self._device[key] = (torch.from_numpy(self.blob).to(device), torch.from_numpy(self.records).to(device))
        return t


def caption_strings(ids, kept, table=None, box_points=None, box_radar=None, rate_scale=0.0):
    """The caption of every kept row, on the host: (strings, bits) with strings[b][r] the caption of row r < kept[b] of image b
    and bits the flag bits.  ids (B, cap) int32 track ids or None; kept (B) integers, clamped into [0, cap] with FLAG_BOX_COUNT;
    table (B, T) `data.TRACK_DTYPE` or None (needs ids); box_points (B, cap) int32 and box_radar (B, cap, 2, 5) float32, the
    radar readout, both or neither; at least one of ids and the readout.  Up to three fields joined by one space:
      '#<id>'      with ids, for ids[b][r] > 0;
      the range    '{:.1f}'.format(rng) + 'm'.  With a table: the lowest slot s with table[b][s].id == ids[b][r], id != 0 and
                   row == r; drawn when its range_age >= 0, rng = x[4], the filtered range (also while the radar coasts).
                   Without a table: box_points[b][r] > 0 and rng = box_radar[b][r][1][0], the lower median.  Valid when rng is
                   not NaN, its sign bit is clear and `fixed_tenths` gives k <= 99999; otherwise left out, with FLAG_CAPTION;
      the speed    '{:+.1f}'.format(rate) + 'm/s', only with a table, a drawn range and rate_scale > 0: rate = v[4] *
                   rate_scale, one float32 multiply (rate_scale is the caller's frame rate: the tracker's rates are per call).
                   Valid when the rate is finite and k <= 9999; otherwise left out, with FLAG_CAPTION.
    A row without a field has the empty caption.  The longest caption is '#2147483647 9999.9m -999.9m/s', 29 characters."""
    fn = "caption_strings"
    if (box_points is None) != (box_radar is None):
        raise RuntimeError(f"{fn}: box_points and box_radar come together or not at all")
    if ids is None and box_points is None:
        raise RuntimeError(f"{fn}: needs track ids or the radar readout")
    if table is not None and ids is None:
        raise RuntimeError(f"{fn}: a track table needs the track ids")
    kept = np.asarray(kept).astype(np.int64).reshape(-1)
    B = len(kept)
    ids = None if ids is None else np.asarray(ids).reshape(B, -1)
    cap = ids.shape[1] if ids is not None else np.asarray(box_points).reshape(B, -1).shape[1]
    if box_points is not None:
        box_points = np.asarray(box_points).reshape(B, cap)
        box_radar = np.asarray(box_radar, np.float32).reshape(B, cap, 2, 5)
    if table is not None:
        table = np.asarray(table).reshape(B, -1)
    scale = np.float32(rate_scale)
    if table is not None:                     # the range and the rate of every slot; the rate is one float32 multiply
        rng_of, age_of = np.ascontiguousarray(table["x"][..., 4], np.float32), table["range_age"].tolist()
        with np.errstate(invalid="ignore", over="ignore"):
            rate_of = np.ascontiguousarray(table["v"][..., 4], np.float32) * scale
        rate_ok = (np.isfinite(rate_of) & (fixed_tenths(rate_of)[0] <= 9999)).tolist()
        rate_of, slot_id, slot_row = rate_of.tolist(), table["id"].tolist(), table["row"].tolist()
    else:
        rng_of = box_radar[:, :, 1, 0] if box_points is not None else np.zeros((B, 0), np.float32)
        have = None if box_points is None else (box_points > 0).tolist()
    k, neg = fixed_tenths(np.ascontiguousarray(rng_of, np.float32))
    rng_ok, rng_of = (~np.isnan(rng_of) & ~neg & (k <= 99999)).tolist(), rng_of.tolist()
    id_of = None if ids is None else ids.tolist()
    strings, bits = [], 0
    for b in range(B):
        n = int(min(max(kept[b], 0), cap))
        if n != kept[b]:
            bits |= FLAG_BOX_COUNT
        slot_of = {}
        if table is not None:                 # the lowest slot that names a row and carries that row's id
            for s in range(table.shape[1] - 1, -1, -1):
                r = slot_row[b][s]
                if slot_id[b][s] != 0 and 0 <= r < n and id_of[b][r] == slot_id[b][s]:
                    slot_of[r] = s
        out = []
        for r in range(n):
            fields, at = [], None             # at: where this row's range stands, if it has one
            if id_of is not None and id_of[b][r] > 0:
                fields.append(f"#{id_of[b][r]}")
            if table is not None:
                s = slot_of.get(r)
                if s is not None and age_of[b][s] >= 0:
                    at = s
            elif have is not None and have[b][r]:
                at = r
            if at is not None and not rng_ok[b][at]:
                bits |= FLAG_CAPTION
            elif at is not None:
                fields.append("{:.1f}".format(rng_of[b][at]) + "m")
                if table is not None and scale > 0:
                    if rate_ok[b][at]:
                        fields.append("{:+.1f}".format(rate_of[b][at]) + "m/s")
                    else:
                        bits |= FLAG_CAPTION
            out.append(" ".join(fields))
        strings.append(out)
    return strings, bits


def caption_records(strings):
    """Host captions -> the (n, 12) int32 records of csrc/captions.hip: words 0..7 the 32 glyph codes as bytes (code i is byte
    i, little-endian), word 8 the count, words 9..11 zero.  strings: a list of strings, or of per-image lists of them (taken in
    order); every character from CAPTION_ALPHABET, at most 32 of them."""
    flat = []
    for s in strings:
        flat += [s] if isinstance(s, str) else list(s)
    for s in flat:
        if len(s) > CAPTION_MAX or not set(s) <= set(CAPTION_ALPHABET):
            raise RuntimeError(f"caption_records: {s!r} has more than {CAPTION_MAX} characters or one outside {CAPTION_ALPHABET!r}")
    code = bytes(max(CAPTION_ALPHABET.find(chr(c)), 0) for c in range(256))
    packed = b"".join(s.encode("ascii").translate(code).ljust(CAPTION_MAX, b"\0") for s in flat)
    rec = np.zeros((len(flat), CAPTION_WORDS), np.int32)
    rec.view(np.uint8).reshape(len(flat), 4 * CAPTION_WORDS)[:, :CAPTION_MAX] = np.frombuffer(packed, np.uint8).reshape(len(flat), CAPTION_MAX)
    rec[:, 8] = [len(s) for s in flat]
    return rec


def caption_decode(records):
    """(n, 12) int32 records -> the list of their strings, as the draw kernel reads them: a count outside [0, 32] is clamped, a
    code above 17 reads as 17 (the space)."""
    rec = np.ascontiguousarray(np.asarray(records))
    if rec.dtype != np.int32 or rec.ndim != 2 or rec.shape[1] != CAPTION_WORDS:
        raise RuntimeError(f"caption_decode: expected int32 records (n, {CAPTION_WORDS}), got {rec.dtype} {rec.shape}")
    glyph = bytes(ord(CAPTION_ALPHABET[min(c, CAPTION_GLYPHS - 1)]) for c in range(256))
    text, step = rec.tobytes().translate(glyph).decode("ascii"), 4 * CAPTION_WORDS
    return [text[i * step:i * step + n] for i, n in enumerate(np.clip(rec[:, 8], 0, CAPTION_MAX).tolist())]


def _caption_setup(atlas, font_size, ih, fn):
    if not isinstance(atlas, GlyphAtlas):
        raise RuntimeError(f"{fn}: the atlas must be a render.GlyphAtlas, got {type(atlas).__name__}")
    font_size = label_font_size(ih) if font_size is None else int(font_size)
    if font_size < 0:
        raise RuntimeError(f"{fn}: font_size must not be negative, got {font_size}")
    if font_size > 0:
        atlas.size_index(font_size)
    return font_size


def draw_captions_host(picture, rows, strings, atlas, font_size, box_palette=None):
    """The caption rule in numpy, for ONE image: picture (ih, iw, 3) uint8, finished (outlines and labels are on it), rows
    (n, 5) int32 = left, top, right, bottom, class as `box_rows` gives them, strings the n captions (`caption_strings`).
    Captions are a pass of their own over the finished picture; the rows are drawn in order, rows past MAX_BOXES are ignored.
    Row i with a caption of n > 0 glyphs at this font size, W the sum of its cell widths and ch the cell height: (ox, oy) =
    (left, bottom + 1) if bottom + ch <= ih - 1, else (left, bottom - ch), left and bottom clamped to +-2^29; it paints the
    rectangle [ox, ox + W - 1] x [oy, oy + ch - 1], clipped to the image, in palette[class] (the class clamped into the
    palette; default `det_palette(4)`), then its cells left to right in black: v = DIV255(v * (255 - m)).  Text never leaves
    its own tag, so a pixel's final value follows from the HIGHEST row whose tag covers it; pixels no tag covers keep their
    bytes.  font_size None: `label_font_size(ih)`; 0 draws nothing.  Returns the new picture.  This is the statement the
    kernels of csrc/captions.hip are tested against."""
    fn = "draw_captions_host"
    pic, rows = np.asarray(picture), np.asarray(rows)
    if pic.dtype != np.uint8 or pic.ndim != 3 or pic.shape[2] != 3:
        raise RuntimeError(f"{fn}: expected a uint8 picture (ih, iw, 3), got {pic.dtype} {pic.shape}")
    if rows.dtype != np.int32 or rows.ndim != 2 or rows.shape[1] != 5 or len(strings) != len(rows):
        raise RuntimeError(f"{fn}: expected int32 rows (n, 5) and n captions, got {rows.dtype} {rows.shape} and {len(strings)}")
    ih, iw = pic.shape[:2]
    font_size = _caption_setup(atlas, font_size, ih, fn)
    pal = _palette(box_palette, det_palette(4), fn)
    pal = pal.cpu().numpy() if torch.is_tensor(pal) else pal
    out = pic.copy()
    if font_size == 0:
        return out
    limit = 1 << 29
    for (left, _, _, bottom, cls), text in zip(rows[:MAX_BOXES].tolist(), list(strings)[:MAX_BOXES]):
        if not text:
            continue
        cells = [atlas.cell(font_size, CAPTION_ALPHABET.index(ch)) for ch in text]
        tag = np.concatenate(cells, axis=1).astype(np.int64)
        ch, W = tag.shape
        left, bottom = min(max(left, -limit), limit), min(max(bottom, -limit), limit)
        ox, oy = (left, bottom + 1) if bottom + ch <= ih - 1 else (left, bottom - ch)
        x0, y0, x1, y1 = max(ox, 0), max(oy, 0), min(ox + W, iw), min(oy + ch, ih)
        if x0 < x1 and y0 < y1:
            colour = pal[min(max(cls, 0), len(pal) - 1)].astype(np.int64)
            m = tag[y0 - oy:y1 - oy, x0 - ox:x1 - ox, None]
            out[y0:y1, x0:x1] = _div255(colour * (255 - m)).astype(np.uint8)
    return out


def draw_captions(picture, results, captions, atlas, font_size=None, box_palette=None, geom=None, flag=None):
    """The captions on the device, in place on the finished (B, ih, iw, 3) uint8 DEVICE picture (vrnet_render_captions_u8):
    results as `draw_labels` takes them -- the list `non_max_suppression` returns, or a device pair / triple (rows (N, 5),
    offsets (B + 1)[, label_idx]) of int32 tensors; captions: the (N, 12) int32 device records `hip.caption_text` wrote, or
    host strings (`caption_records` packs them, one non-blocking copy).  font_size: default `label_font_size(ih)`, 0 draws
    nothing; box_palette: default `det_palette(4)`; flag: FLAG_BOX_ROWS for more than 1024 rows in an image.  With geom, the
    device table of `data.frame_geometry`, the picture is (B, ihm, iwm, 3) padded slots, results are device tensors and
    font_size is the (B) int32 device table `GlyphAtlas.size_table` gives, -1 for an image without captions
    (vrnet_render_captions_ragged_u8).  Returns the picture.  No host synchronisation."""
    from . import hip
    fn = "draw_captions"
    if not (torch.is_tensor(picture) and picture.is_cuda and picture.dtype == torch.uint8 and picture.dim() == 4 and
            picture.shape[-1] == 3 and picture.is_contiguous()):
        raise RuntimeError(f"{fn}: expected a contiguous uint8 picture (B, ih, iw, 3) on a GPU")
    B, ih, iw = picture.shape[:3]
    if geom is None:
        font_size = _caption_setup(atlas, font_size, ih, fn)
        size = atlas.size_index(font_size) if font_size > 0 else None
    else:
        if not isinstance(atlas, GlyphAtlas):
            raise RuntimeError(f"{fn}: the atlas must be a render.GlyphAtlas, got {type(atlas).__name__}")
        if not torch.is_tensor(font_size):
            raise RuntimeError(f"{fn}: with a geometry table font_size is the (B) int32 device table of GlyphAtlas.size_table")
        size = font_size
    bpal = _palette(box_palette, det_palette(4), fn)
    send, dev = _results(fn, results, B, ih, iw, host=geom is None), picture.device
    with torch.cuda.device(dev):
        rows, offsets, _ = send(dev, flag)
        if not torch.is_tensor(captions):
            captions = torch.from_numpy(caption_records(captions)).pin_memory().to(dev, non_blocking=True)
        if size is not None:
            blob, records = atlas.on(dev)
            hip.render_captions(picture, rows, offsets, _palette_on(bpal, dev), captions, blob, records, size, flag=flag, geom=geom)
    return picture


# ---- detection crops (csrc/crops.hip) ------------------------------------------------------------------------------------------
def _crop_rows(rows, fn):
    rows = np.asarray(rows)
    if rows.dtype != np.int32 or rows.ndim != 2 or rows.shape[1] != 5:
        raise RuntimeError(f"{fn}: expected int32 rows (n, 5), got {rows.dtype} {rows.shape}")
    return rows.astype(np.int64)


def _crop_windows(rows, ih, iw):
    """The clamp of the module docstring for (n, 5) int64 rows and per-row (or scalar) image sizes: l, t, w, h with
    w = h = 0 for an empty crop."""
    l, t = np.maximum(rows[:, 0], 0), np.maximum(rows[:, 1], 0)
    w, h = np.minimum(rows[:, 2], iw) - l, np.minimum(rows[:, 3], ih) - t
    empty = (w <= 0) | (h <= 0)
    return l, t, np.where(empty, 0, w), np.where(empty, 0, h)


def crop_boxes_host(frame, rows):
    """The crops of yolo.py:180-193 for ONE image in numpy: frame (ih, iw, 3) uint8, the ORIGINAL picture, and rows (n, 5)
    int32 = left, top, right, bottom, class as `box_rows` gives them.  Returns a list of n uint8 arrays: frame[t:bt, l:r]
    under the clamp of the module docstring -- bit for bit np.array(image.crop([left, top, right, bottom])) for the rows
    `box_rows` makes -- and an array of shape (0, 0, 3) for an empty crop (w <= 0 or h <= 0, where Pillow gives a zero-size
    image or raises).  This is the statement the kernels of csrc/crops.hip are tested against; tests/test_crops_host.py pins
    it to live Pillow."""
    fn = "crop_boxes_host"
    pic = np.asarray(frame)
    if pic.dtype != np.uint8 or pic.ndim != 3 or pic.shape[2] != 3:
        raise RuntimeError(f"{fn}: expected a uint8 frame (ih, iw, 3), got {pic.dtype} {pic.shape}")
    l, t, w, h = _crop_windows(_crop_rows(rows, fn), pic.shape[0], pic.shape[1])
    return [pic[t[n]:t[n] + h[n], l[n]:l[n] + w[n]].copy() if w[n] else np.zeros((0, 0, 3), np.uint8) for n in range(len(l))]


def crop_layout(rows, offsets, sizes, capacity):
    """Where `crop_boxes` puts every crop: rows (N, 5) int32 in the packed order of `box_rows`, offsets (B + 1) int32, sizes
    = (ih, iw) of all images or a (B, 2) array of each one's, capacity in pixels.  Returns (table, summary, flag): table (N)
    records of CROP_RECORD -- offset, w, h, image --, summary = (N, used) and flag = FLAG_CROP_ARENA if a crop was dropped,
    else 0.  Row n needs a = w * h rounded up to a multiple of 4 pixels (0 if empty); its offset is the sum of a over ALL
    earlier rows, in pixels.  An empty row has w = h = 0 and offset 0; a non-empty row with offset + a > capacity is dropped:
    it keeps w, h and gets offset -1, and since the sum runs over all rows, so does every later non-empty row.  used: the
    sum of a over the kept rows.  The image of a row: offsets made monotone, c[0] = 0, c[i] = min(N, max(0, offsets[0..i])),
    N = offsets[B] clamped to [0, len(rows)]; row n belongs to the image b with c[b] <= n < c[b + 1]."""
    fn = "crop_layout"
    rows = _crop_rows(rows, fn)
    offsets = np.asarray(offsets)
    if offsets.dtype != np.int32 or offsets.ndim != 1 or offsets.size < 2:
        raise RuntimeError(f"{fn}: expected int32 offsets (B + 1), got {offsets.dtype} {offsets.shape}")
    B = offsets.size - 1
    sizes = np.asarray(sizes, np.int64)
    sizes = np.broadcast_to(sizes, (B, 2)) if sizes.shape == (2,) else sizes
    if sizes.shape != (B, 2) or int(capacity) < 1:
        raise RuntimeError(f"{fn}: sizes is (ih, iw) or a ({B}, 2) array and the capacity at least one pixel")
    N = int(np.clip(offsets[B], 0, len(rows)))
    c = np.minimum(N, np.maximum.accumulate(np.maximum(offsets.astype(np.int64), 0)))
    image = np.minimum(np.searchsorted(c[1:], np.arange(N), side="right"), B - 1)
    _, _, w, h = _crop_windows(rows[:N], sizes[image, 0], sizes[image, 1])
    a = (w * h + 3) // 4 * 4
    off = np.cumsum(a) - a
    kept = (a > 0) & (off + a <= int(capacity))
    table = np.zeros(N, CROP_RECORD)
    table["offset"] = np.where(a == 0, 0, np.where(kept, off, -1))
    table["w"], table["h"], table["image"] = w, h, image
    return table, (N, int(a[kept].sum())), FLAG_CROP_ARENA if bool(((a > 0) & ~kept).any()) else 0


class Crops:
    """What `crop_boxes` leaves on the device: arena (3 * capacity) uint8, the crops back to back, crop n one contiguous
    (h, w, 3) block at arena[3 * offset:]; table (n_cap, 4) int32, one CROP_RECORD -- offset, w, h, image -- per draw row
    (offset -1: the arena was full and the crop was dropped; w = h = 0: an empty crop; image -1: behind the last row);
    summary (2) int32 = (rows, pixels in use); flag (1) int32.  A second stage that stays on the device reads arena and
    table directly.  From a pipeline these are its own buffers: the next run overwrites them."""
    __slots__ = ("arena", "table", "summary", "flag", "batch", "_packed")

    def __init__(self, arena, table, summary, flag, batch, packed=None):
        self.arena, self.table, self.summary, self.flag, self.batch, self._packed = arena, table, summary, flag, int(batch), packed

    def images(self):
        """The read-back: one list per image of its crops in row order as (h, w, 3) uint8 arrays -- shape (0, 0, 3) for an
        empty crop, None for one the arena dropped.  Two device-to-host copies: the table with the summary (which waits for
        the device), then arena[:3 * used]."""
        packed = self._packed if self._packed is not None else torch.cat([self.table.reshape(-1), self.summary])
        packed = packed.cpu().numpy()
        (N, used), table = (int(v) for v in packed[-2:]), packed[:-2].view(CROP_RECORD)
        arena = self.arena[:3 * used].cpu().numpy()
        out = [[] for _ in range(self.batch)]
        for off, w, h, b in table[:N].tolist():
            if off < 0:
                crop = None
            elif w <= 0 or h <= 0:
                crop = np.zeros((0, 0, 3), np.uint8)
            else:
                crop = arena[3 * off:3 * (off + w * h)].reshape(h, w, 3).copy()
            out[b].append(crop)
        return out


def crop_buffers(n_cap, capacity, batch, flag, device):
    """The device buffers of one `hip.crop_boxes` call as a `Crops`: table and summary share one int32 tensor, so the
    read-back fetches both in one copy."""
    capacity = int(capacity)
    if not 1 <= capacity <= 1 << 30:
        raise RuntimeError(f"crop_boxes: the capacity must lie in 1..2^30 pixels, got {capacity}")
    packed = torch.empty(n_cap * 4 + 2, dtype=torch.int32, device=device)
    arena = torch.empty(3 * capacity, dtype=torch.uint8, device=device)
    return Crops(arena, packed[:n_cap * 4].view(n_cap, 4), packed[n_cap * 4:], flag, batch, packed)


def crop_boxes(frames_u8, results, capacity=None, geom=None, flag=None, device="cuda"):
    """yolo.py:180-193 on the device: every detection cut out of the ORIGINAL frames (crop before you draw, as the reference
    does) into one packed arena, by the rule of `crop_boxes_host` and `crop_layout` (vrnet_crop_boxes_u8, two launches).
    frames_u8 (B, ih, iw, 3) uint8 RGB, numpy or tensor (a single (ih, iw, 3) frame counts as B = 1).  results: the list
    `non_max_suppression` returns -- packed by `box_rows` and sent in one pinned non-blocking copy -- or a pair (rows (n_cap,
    5) int32, offsets (B + 1) int32) of device tensors, exactly as `render_frame` accepts them.  geom: the (B,
    hip.GEOM_BYTES) device table of `data.frame_geometry` for padded ragged frames (image b in the top-left corner of slot
    b); no crop then holds a byte of the padding.  capacity: the arena in pixels, default 2 * B * ih * iw.  flag: a zeroed
    int32 device tensor of one element (a fresh one by default) that receives FLAG_CROP_ARENA -- a crop that did not fit,
    dropped with every non-empty one behind it -- and hip.FLAG_GEOMETRY.  Returns a `Crops`.  No host synchronisation."""
    from . import hip
    fn = "crop_boxes"
    img = _as_frames(frames_u8, "frames", _FRAMES, fn)
    B, ih, iw = img.shape[:3]
    if results is None:
        raise RuntimeError(f"{fn}: needs the results of non_max_suppression or a device pair (rows, offsets)")
    host = None
    if isinstance(results, tuple) and len(results) == 2 and all(torch.is_tensor(t) for t in results):
        rows, offsets = results
    else:
        if len(results) != B:
            raise RuntimeError(f"{fn}: {len(results)} result entries for {B} frames")
        host = box_rows(results, (ih, iw), MAX_COLORS)[:2]
    img = img.to(device, non_blocking=True).contiguous()
    dev = img.device
    with torch.cuda.device(dev):
        if host is not None:                  # offsets and rows in one pinned buffer; at least one row, so it has an address
            n = max(len(host[0]), 1)
            packed = torch.zeros(B + 1 + 5 * n, dtype=torch.int32).pin_memory()
            packed[:B + 1] = torch.from_numpy(host[1])
            packed[B + 1:B + 1 + host[0].size] = torch.from_numpy(host[0].reshape(-1))
            packed = packed.to(dev, non_blocking=True)
            offsets, rows = packed[:B + 1], packed[B + 1:].view(n, 5)
        else:
            rows, offsets = rows.to(dev).contiguous(), offsets.to(dev).contiguous()
        if flag is None:
            flag = torch.zeros(1, dtype=torch.int32, device=dev)
        crops = crop_buffers(rows.shape[0], min(2 * B * ih * iw, 1 << 30) if capacity is None else capacity, B, flag, dev)
        hip.crop_boxes(img, rows, offsets, crops.arena, crops.table, crops.summary, geom=geom, flag=flag)
    return crops


# ---- fixed-size detection chips (csrc/chips.hip) -------------------------------------------------------------------------------
def _chip_size(size, fn):
    try:
        sh, sw = (int(v) if isinstance(v, (int, np.integer)) and not isinstance(v, bool) else 0 for v in size)
    except (TypeError, ValueError):
        sh = sw = 0
    if not (1 <= sh <= CHIP_MAX and 1 <= sw <= CHIP_MAX):
        raise RuntimeError(f"{fn}: size is (sh, sw) with both sides integers in 1..{CHIP_MAX}, got {size!r}")
    return sh, sw


def chip_geometry(w, h, size, letterbox):
    """The integers of the chip rule for a clamped crop of w x h pixels and size = (sh, sw): (nw, nh, dx, dy), the size the
    crop is resized to and where it is pasted in the chip.  An empty crop (w <= 0 or h <= 0): (0, 0, 0, 0), an all-grey chip.
    letterbox False: (sw, sh, 0, 0).  letterbox True: resize_image's rule (utils/utils.py:19-32) on the crop in Python
    doubles, scale = min(sw / w, sh / h), nw = max(int(w * scale), 1), nh = max(int(h * scale), 1), pasted at ((sw - nw) //
    2, (sh - nh) // 2).  The max(.., 1) is a deliberate departure from the reference: a 1000 x 3 crop into 64 x 64 gives
    nh = 0 there, and Pillow raises on it; here the strip keeps one row."""
    sh, sw = _chip_size(size, "chip_geometry")
    w, h = int(w), int(h)
    if w <= 0 or h <= 0:
        return 0, 0, 0, 0
    if not letterbox:
        return sw, sh, 0, 0
    scale = min(sw / w, sh / h)
    nw, nh = max(int(w * scale), 1), max(int(h * scale), 1)
    return nw, nh, (sw - nw) // 2, (sh - nh) // 2


def chip_boxes_host(frame, rows, size, letterbox=False):
    """THE RULE of the fixed-size chips for ONE image, with Pillow itself: frame (ih, iw, 3) uint8, the ORIGINAL picture, rows
    (n, 5) int32 = left, top, right, bottom, class, size = (sh, sw).  Returns a list of n (sh, sw, 3) uint8 arrays.  The crop
    of a row is the one `crop_boxes_host` takes (each coordinate clamped to the image, w = r - l, h = bt - t).  letterbox
    False: image.crop((l, t, r, bt)).resize((sw, sh), BICUBIC) -- crop THEN resize: the taps stop at the crop's edge
    (resize(box=...) reads beyond it and gives other bytes).  letterbox True: the crop resized to `chip_geometry`'s (nw, nh)
    and pasted at its (dx, dy) on grey 128, resize_image's rule with nw, nh >= 1 (the departure `chip_geometry` states).  An
    empty crop (w <= 0 or h <= 0) is an all-grey chip in both modes.  A pass whose size does not change is the identity, as
    it is in Pillow.  The kernels of csrc/chips.hip are tested against this function, bit for bit."""
    from PIL import Image
    fn = "chip_boxes_host"
    pic = np.asarray(frame)
    if pic.dtype != np.uint8 or pic.ndim != 3 or pic.shape[2] != 3:
        raise RuntimeError(f"{fn}: expected a uint8 frame (ih, iw, 3), got {pic.dtype} {pic.shape}")
    sh, sw = _chip_size(size, fn)
    l, t, w, h = _crop_windows(_crop_rows(rows, fn), pic.shape[0], pic.shape[1])
    image = Image.fromarray(np.ascontiguousarray(pic))
    out = []
    for n in range(len(l)):
        chip = np.full((sh, sw, 3), 128, np.uint8)
        if w[n] > 0:
            nw, nh, dx, dy = chip_geometry(w[n], h[n], (sh, sw), letterbox)
            crop = image.crop((int(l[n]), int(t[n]), int(l[n] + w[n]), int(t[n] + h[n])))
            chip[dy:dy + nh, dx:dx + nw] = np.asarray(crop.resize((nw, nh), Image.BICUBIC))
        out.append(chip)
    return out


def _bicubic(x):
    """Resample.c bicubic_filter, a = -0.5, in Python doubles (one rounding per operation, as the C code)."""
    a = -0.5
    x = -x if x < 0.0 else x
    if x < 1.0:
        return ((a + 2.0) * x - (a + 3.0)) * x * x + 1
    if x < 2.0:
        return (((x - 5) * x + 8) * x - 4) * a
    return 0.0


def _chip_axis(n_in, n_out):
    """Per output index of an axis resized n_in -> n_out: (xmin, n, ww) of Resample.c precompute_coeffs -- the window and the
    sum of its bicubic values in the order x = 0 .. n - 1 -- and the integer weights recomputed from them alone, as the
    kernel recomputes them (normalize_coeffs_8bpc: 22 bits, rounded half away from zero)."""
    scale = n_in / n_out
    fs = max(scale, 1.0)
    support, ss = 2.0 * fs, 1.0 / fs
    table = []
    for xx in range(n_out):
        center = (xx + 0.5) * scale
        xmin = max(int(center - support + 0.5), 0)
        n = min(int(center + support + 0.5), n_in) - xmin
        ww = 0.0
        for x in range(n):
            ww += _bicubic((x + xmin - center + 0.5) * ss)
        k = np.zeros(n, np.int32)
        for x in range(n):                    # from (xmin, n, ww) alone
            wt = _bicubic((x + xmin - center + 0.5) * ss)
            if ww != 0.0:
                wt /= ww
            k[x] = int(-0.5 + wt * (1 << 22)) if wt < 0 else int(0.5 + wt * (1 << 22))
        table.append((xmin, n, ww, k))
    return table


def chip_resample_host(crop, nh, nw):
    """The arithmetic the kernels of csrc/chips.hip run, in numpy, without Pillow: crop (h, w, 3) uint8 -> (nh, nw, 3) uint8,
    byte for byte image.resize((nw, nh), BICUBIC).  Per axis a table of (xmin, n, ww) per output index (`_chip_axis`), every
    integer weight recomputed from its entry; each pass sums weight * byte in int32 on top of 1 << 21, shifts by 22 and clips;
    the horizontal pass is rounded to bytes before the vertical one, the only ordering Pillow imposes -- integer addition is
    associative, so the kernel may add the taps of the vertical pass in chunks of source rows.  A pass whose size does not
    change has the weights (0, 1, 0, 0) exactly and is the identity.  Kept so that the kernel's arithmetic is pinned to Pillow
    without a GPU (tests/test_chips_host.py)."""
    fn = "chip_resample_host"
    src = np.asarray(crop)
    if src.dtype != np.uint8 or src.ndim != 3 or src.shape[2] != 3 or min(src.shape) < 1:
        raise RuntimeError(f"{fn}: expected a non-empty uint8 crop (h, w, 3), got {src.dtype} {src.shape}")
    nh, nw = int(nh), int(nw)
    if nh < 1 or nw < 1:
        raise RuntimeError(f"{fn}: the new size must be at least 1 x 1, got {nh} x {nw}")
    h, w = src.shape[:2]

    def clip8(acc):
        return np.clip(acc >> 22, 0, 255).astype(np.uint8)

    mid = np.empty((h, nw, 3), np.uint8)
    for xx, (xmin, n, _, k) in enumerate(_chip_axis(w, nw)):
        acc = np.full((h, 3), 1 << 21, np.int32)
        for x in range(n):
            acc += k[x] * src[:, xmin + x, :].astype(np.int32)
        mid[:, xx] = clip8(acc)
    out = np.empty((nh, nw, 3), np.uint8)
    for yy, (ymin, n, _, k) in enumerate(_chip_axis(h, nh)):
        acc = np.full((nw, 3), 1 << 21, np.int32)
        for y in range(n):
            acc += k[y] * mid[ymin + y].astype(np.int32)
        out[yy] = clip8(acc)
    return out


def chip_table(rows, offsets, sizes, size, letterbox=False):
    """The records `chip_boxes` leaves for its rows: rows (N, 5) int32, offsets (B + 1) int32, sizes = (ih, iw) of all images
    or a (B, 2) array of each one's.  Returns (table, N): N = offsets[B] clamped to [0, len(rows)] records of CHIP_RECORD --
    image, w, h, nw, nh, dx, dy, state (1 resized, 2 empty) -- with the image of a row as `crop_layout` finds it."""
    fn = "chip_table"
    rows = _crop_rows(rows, fn)
    offsets = np.asarray(offsets)
    if offsets.dtype != np.int32 or offsets.ndim != 1 or offsets.size < 2:
        raise RuntimeError(f"{fn}: expected int32 offsets (B + 1), got {offsets.dtype} {offsets.shape}")
    B = offsets.size - 1
    sizes = np.asarray(sizes, np.int64)
    sizes = np.broadcast_to(sizes, (B, 2)) if sizes.shape == (2,) else sizes
    if sizes.shape != (B, 2):
        raise RuntimeError(f"{fn}: sizes is (ih, iw) or a ({B}, 2) array")
    N = int(np.clip(offsets[B], 0, len(rows)))
    c = np.minimum(N, np.maximum.accumulate(np.maximum(offsets.astype(np.int64), 0)))
    image = np.minimum(np.searchsorted(c[1:], np.arange(N), side="right"), B - 1)
    _, _, w, h = _crop_windows(rows[:N], sizes[image, 0], sizes[image, 1])
    table = np.zeros(N, CHIP_RECORD)
    for n in range(N):
        table[n] = (image[n], w[n], h[n]) + chip_geometry(w[n], h[n], size, letterbox) + (1 if w[n] > 0 else 2,)
    return table, N


class Chips:
    """What `chip_boxes` leaves on the device: chips (n_cap, sh, sw, 3) uint8, chip n of draw row n; chips_f32 (n_cap, 3, sh,
    sw) float32, the same bytes normalised as the network's input is (None unless asked for); table (n_cap, 8) int32, one
    CHIP_RECORD -- image, w, h, nw, nh, dx, dy, state -- per draw row (state 1: resized, 2: an empty crop, a grey chip, 0
    with image -1: behind the last row, whose chips are NOT written and hold what the buffer held); summary (1) int32 =
    rows; flag (1) int32.  A second stage that stays on the device reads chips_f32[:rows].  From a pipeline these are its
    own buffers: the next run overwrites them."""
    __slots__ = ("chips", "chips_f32", "table", "summary", "flag", "batch", "size", "letterbox", "workspace", "_packed")

    def __init__(self, chips, chips_f32, table, summary, flag, batch, size, letterbox, workspace, packed):
        self.chips, self.chips_f32, self.table, self.summary, self.flag = chips, chips_f32, table, summary, flag
        self.batch, self.size, self.letterbox, self.workspace, self._packed = int(batch), tuple(size), bool(letterbox), workspace, packed

    def images(self):
        """The read-back: one list per image of its chips in row order as (sh, sw, 3) uint8 arrays.  ONE device-to-host copy
        (table, summary and chips share a buffer), which waits for the device."""
        packed = self._packed.cpu().numpy()
        n_cap, (sh, sw) = self.table.shape[0], self.size
        table = packed[:32 * n_cap].view(CHIP_RECORD)
        N = int(packed[32 * n_cap:32 * n_cap + 4].view(np.int32)[0])
        chips = packed[32 * n_cap + 16:].reshape(n_cap, sh, sw, 3)
        out = [[] for _ in range(self.batch)]
        for n in range(min(max(N, 0), n_cap)):
            out[int(table["image"][n])].append(chips[n].copy())
        return out


def chip_buffers(n_cap, size, batch, letterbox, normalised, flag, device):
    """The device buffers of one `hip.chip_boxes` call as a `Chips`: table, summary and chips share one uint8 tensor (the
    table first, the summary in 16 bytes of its own, then the chips), so the read-back is one copy."""
    from . import hip
    sh, sw = _chip_size(size, "chip_boxes")
    packed = torch.zeros(32 * n_cap + 16 + n_cap * sh * sw * 3, dtype=torch.uint8, device=device)
    table = packed[:32 * n_cap].view(torch.int32).view(n_cap, 8)
    summary = packed[32 * n_cap:32 * n_cap + 4].view(torch.int32)
    chips = packed[32 * n_cap + 16:].view(n_cap, sh, sw, 3)
    f32 = torch.zeros((n_cap, 3, sh, sw), dtype=torch.float32, device=device) if normalised else None
    ws = torch.empty(hip.chip_workspace_bytes(n_cap, sh, sw), dtype=torch.uint8, device=device)
    return Chips(chips, f32, table, summary, flag, batch, (sh, sw), letterbox, ws, packed)


def chip_boxes(frames_u8, results, size, letterbox=False, normalised=False, geom=None, flag=None, device="cuda"):
    """Every detection cut out of the ORIGINAL frames and brought to size = (sh, sw) on the device, by the rule of
    `chip_boxes_host` (vrnet_chip_boxes_u8, two launches): one tensor of equal-sized pictures, what a second-stage
    classifier, an appearance descriptor or a thumbnail strip takes.  frames_u8, results, geom and flag as `crop_boxes` takes
    them; letterbox: keep the crop's aspect ratio on grey 128 (resize_image's rule) instead of stretching it; normalised:
    also write `Chips.chips_f32`, the chips as the network's input is normalised.  flag receives hip.FLAG_GEOMETRY alone.
    Returns a `Chips`.  No host synchronisation."""
    from . import hip
    fn = "chip_boxes"
    size = _chip_size(size, fn)
    img = _as_frames(frames_u8, "frames", _FRAMES, fn)
    B, ih, iw = img.shape[:3]
    if results is None:
        raise RuntimeError(f"{fn}: needs the results of non_max_suppression or a device pair (rows, offsets)")
    host = None
    if isinstance(results, tuple) and len(results) == 2 and all(torch.is_tensor(t) for t in results):
        rows, offsets = results
    else:
        if len(results) != B:
            raise RuntimeError(f"{fn}: {len(results)} result entries for {B} frames")
        host = box_rows(results, (ih, iw), MAX_COLORS)[:2]
    img = img.to(device, non_blocking=True).contiguous()
    dev = img.device
    with torch.cuda.device(dev):
        if host is not None:                  # offsets and rows in one pinned buffer; at least one row, so it has an address
            n = max(len(host[0]), 1)
            packed = torch.zeros(B + 1 + 5 * n, dtype=torch.int32).pin_memory()
            packed[:B + 1] = torch.from_numpy(host[1])
            packed[B + 1:B + 1 + host[0].size] = torch.from_numpy(host[0].reshape(-1))
            packed = packed.to(dev, non_blocking=True)
            offsets, rows = packed[:B + 1], packed[B + 1:].view(n, 5)
        else:
            rows, offsets = rows.to(dev).contiguous(), offsets.to(dev).contiguous()
        if flag is None:
            flag = torch.zeros(1, dtype=torch.int32, device=dev)
        chips = chip_buffers(rows.shape[0], size, B, letterbox, normalised, flag, dev)
        hip.chip_boxes(img, rows, offsets, chips.chips, chips.table, chips.summary, chips.workspace, letterbox=letterbox,
                       chips_f32=chips.chips_f32, geom=geom, flag=flag)
    return chips


# ---- dark-channel dehazing (csrc/dehaze.hip) -----------------------------------------------------------------------------------
def dehaze_params(sz=15, r=60, eps=1e-4, omega=0.95, tx=0.1, fn="dehaze"):
    """The parameters of the dehazing rule, checked: sz odd in 1..31, 2 <= r <= 128, eps > 0 (finite), 0 < omega <= 1,
    0 < tx <= 1.  Returns them as a dict of Python numbers."""
    ints = all(isinstance(v, (int, np.integer)) and not isinstance(v, bool) for v in (sz, r))
    if not ints or not 1 <= sz <= DEHAZE_MAX_SZ or sz % 2 == 0 or not 2 <= r <= DEHAZE_MAX_R:
        raise RuntimeError(f"{fn}: sz must be an odd integer in 1..{DEHAZE_MAX_SZ} and r an integer in 2..{DEHAZE_MAX_R}, got sz "
                           f"{sz!r}, r {r!r}")
    try:
        eps, omega, tx = float(eps), float(omega), float(tx)
    except (TypeError, ValueError):
        raise RuntimeError(f"{fn}: eps, omega and tx are numbers, got {eps!r}, {omega!r}, {tx!r}") from None
    if not (0.0 < eps < np.inf and 0.0 < omega <= 1.0 and 0.0 < tx <= 1.0):
        raise RuntimeError(f"{fn}: eps must be positive and finite, omega and tx in (0, 1], got eps {eps}, omega {omega}, tx {tx}")
    return dict(sz=int(sz), r=int(r), eps=eps, omega=omega, tx=tx)


def dehaze_size_ok(ih, iw, r):
    """Whether an (ih, iw) image allows the single reflection of an r x r box: r // 2 <= min(ih, iw) - 1."""
    return int(r) // 2 <= min(int(ih), int(iw)) - 1


def _erode_host(a, sz, fill):
    """The minimum over the sz x sz window centred on each pixel, positions outside the image ignored."""
    h = sz // 2
    ih, iw = a.shape
    p = np.full((ih + 2 * h, iw + 2 * h), fill, a.dtype)
    p[h:h + ih, h:h + iw] = a
    rows = p[:, 0:iw].copy()
    for j in range(1, sz):
        np.minimum(rows, p[:, j:j + iw], out=rows)
    out = rows[0:ih].copy()
    for j in range(1, sz):
        np.minimum(out, rows[j:j + ih], out=out)
    return out


def _refl_host(i, n):
    i = np.abs(i)
    return np.where(i < n, i, 2 * (n - 1) - i)


def box_filter_host(p, r):
    """cv2.boxFilter(p, CV_64F, (r, r)) restated: normalised, anchor r // 2, BORDER_REFLECT_101, the r taps of each pass added
    one after the other from the leftmost (topmost) on -- r shifted adds per pass, then one division by float(r * r)."""
    p = np.asarray(p, np.float64)
    ih, iw = p.shape
    o = r // 2
    if o > min(ih, iw) - 1:
        raise RuntimeError(f"box_filter_host: a {ih} x {iw} plane allows no single reflection of a box of {r}")
    q = p[:, _refl_host(np.arange(-o, iw - o + r - 1), iw)]
    h = q[:, 0:iw].copy()
    for j in range(1, r):
        h += q[:, j:j + iw]
    q = h[_refl_host(np.arange(-o, ih - o + r - 1), ih)]
    v = q[0:ih].copy()
    for j in range(1, r):
        v += q[j:j + ih]
    return v / float(r * r)


def gray_host(rgb):
    """OpenCV's 8-bit RGB -> gray: (4899 R + 9617 G + 1868 B + 8192) >> 14, uint8."""
    c = np.asarray(rgb).astype(np.int64)
    return ((4899 * c[..., 0] + 9617 * c[..., 1] + 1868 * c[..., 2] + 8192) >> 14).astype(np.uint8)


def atmospheric_light_host(rgb, dark8):
    """A of the rule: numpx = max(ih * iw // 1000, 1); the pixels in ascending (dark8, flat index) order, the last numpx
    without the first of those; A_c = (float(integer sum of byte_c) / 255.0) / float(numpx)."""
    n = dark8.size
    numpx = max(n // 1000, 1)
    idx = np.argsort(dark8.reshape(-1), kind="stable")[n - numpx:][1:]
    S = rgb.reshape(n, 3)[idx].astype(np.int64).sum(0)
    return (S.astype(np.float64) / 255.0) / float(numpx)


def saturate_host(v):
    """clip(rint(v), 0, 255) as uint8, half to even: the saturate_cast of a float64 picture."""
    return np.clip(np.rint(v), 0.0, 255.0).astype(np.uint8)


def dehaze_host(rgb, sz=15, r=60, eps=1e-4, omega=0.95, tx=0.1):
    """He et al.'s dark-channel-prior dehazing of ONE (ih, iw, 3) uint8 RGB frame in numpy float64, every operation rounded
    on its own in the order of the header's statement (include/vrnet_hip.h, vrnet_dehaze_u8): dark channel, atmospheric
    light from the brightest 0.1 % of it, transmission estimate, guided filter with an r x r box, recovery.  Returns
    (bytes (ih, iw, 3) uint8, t (ih, iw) float64, A (3) float64).  A degenerate image -- any A_c == 0 (which includes
    ih * iw < 2000, where nothing is summed) or r // 2 > min(ih, iw) - 1 -- comes back unchanged with t = 1.  This is the
    statement the kernels of csrc/dehaze.hip are tested against.  The OpenCV semantics in it (erode's border, BGR2GRAY's
    integers, boxFilter's anchor and border, saturate_cast) are restated from OpenCV's published behaviour and have never
    been run against cv2."""
    fn = "dehaze_host"
    q = dehaze_params(sz, r, eps, omega, tx, fn)
    sz, r, eps, omega, tx = q["sz"], q["r"], q["eps"], q["omega"], q["tx"]
    rgb = np.asarray(rgb)
    if rgb.dtype != np.uint8 or rgb.ndim != 3 or rgb.shape[2] != 3 or min(rgb.shape) <= 0:
        raise RuntimeError(f"{fn}: expected a uint8 frame (ih, iw, 3), got {rgb.dtype} {rgb.shape}")
    ih, iw = rgb.shape[:2]
    dark8 = _erode_host(rgb.min(2), sz, np.uint8(255))
    A = atmospheric_light_host(rgb, dark8)
    if bool((A == 0.0).any()) or not dehaze_size_ok(ih, iw, r):
        return rgb.copy(), np.ones((ih, iw), np.float64), A
    I = rgb.astype(np.float64) / 255.0
    te = 1.0 - omega * _erode_host((I / A).min(2), sz, np.inf)
    g = gray_host(rgb).astype(np.float64) / 255.0
    mI, mp, mIp, mII = box_filter_host(g, r), box_filter_host(te, r), box_filter_host(g * te, r), box_filter_host(g * g, r)
    a = (mIp - mI * mp) / ((mII - mI * mI) + eps)
    b = mp - a * mI
    t = box_filter_host(a, r) * g + box_filter_host(b, r)
    v = ((I - A) / np.maximum(t, tx)[..., None] + A) * 255.0
    return saturate_host(v), t, A


def dehaze(frames_u8, sizes=None, geom=None, sz=15, r=60, eps=1e-4, omega=0.95, tx=0.1, transmission=False, flag=None,
           device="cuda"):
    """`dehaze_host` on the device (vrnet_dehaze_u8, eleven launches, no host synchronisation): frames_u8 (B, ih, iw, 3) uint8
    RGB, numpy or tensor (a single (ih, iw, 3) frame counts as B = 1).  sizes: (B, 2) host integers (ih_b, iw_b) when the
    frames are padded slots with image b in the top-left corner of slot b -- a table is built from them --, or geom: the
    (B, hip.GEOM_BYTES) device table of `data.frame_geometry`; neither: every image fills its slot.  Outside an image's
    corner the results are 0.  Returns (out (B, ih, iw, 3) uint8, t (B, ih, iw) float64 or None without transmission=True,
    A (B, 3) float64), all on the device.  flag: a zeroed int32 device tensor of one element, or None: it receives
    FLAG_DEHAZE for a degenerate image, which comes back unchanged with t = 1, and hip.FLAG_GEOMETRY for a bad record of
    the table, which gives a zero image.  A size known on the host (no table, or sizes) that
    allows no single reflection of the box, r // 2 > min(ih, iw) - 1, raises before anything is enqueued."""
    from . import hip
    fn = "dehaze"
    q = dehaze_params(sz, r, eps, omega, tx, fn)
    img = _as_frames(frames_u8, "frames", _FRAMES, fn)
    B, ih, iw = img.shape[:3]

    def box_fits(b, h, w):                    # run per image behind its slot check, so the errors come in the order they did
        if not dehaze_size_ok(h, w, q["r"]):
            raise RuntimeError(f"{fn}: image {b}: {h} x {w} allows no single reflection of a box of r = {q['r']}")

    arr =_host_sizes(sizes, geom, B, ih, iw, fn, also=box_fits)
    if arr is None and geom is None and not dehaze_size_ok(ih, iw, q["r"]):
        raise RuntimeError(f"{fn}: frames of {ih} x {iw} allow no single reflection of a box of r = {q['r']}")
    img = img.to(device, non_blocking=True).contiguous()
    dev = img.device
    with torch.cuda.device(dev):
        if arr is not None:
            geom = _sizes_geom(arr, dev)
        out = torch.empty_like(img)
        t = torch.empty((B, ih, iw), dtype=torch.float64, device=dev) if transmission else None
        ws = torch.empty(hip.dehaze_workspace_bytes(B, ih, iw), dtype=torch.uint8, device=dev)
        hip.dehaze(img, out, ws, geom=geom, transmission=t, flag=flag, **q)
        A = ws[:32 * B].view(torch.float64).view(B, 4)[:, :3].clone()
    return out, t, A


# ---- ACE de-rain enhancement (csrc/ace.hip) ------------------------------------------------------------------------------------
def ace_params(ratio=4.0, radius=3, s=0.005, bins=2000, fn="ace"):
    """The parameters of the ACE rule, checked: ratio > 0 (finite), radius an integer in 1..8, 0 <= s < 0.5, bins an integer
    in 2..4096.  Returns them as a dict of Python numbers."""
    ints = all(isinstance(v, (int, np.integer)) and not isinstance(v, bool) for v in (radius, bins))
    if not ints or not 1 <= radius <= ACE_MAX_RADIUS or not 2 <= bins <= ACE_MAX_BINS:
        raise RuntimeError(f"{fn}: radius must be an integer in 1..{ACE_MAX_RADIUS} and bins an integer in 2..{ACE_MAX_BINS}, got "
                           f"radius {radius!r}, bins {bins!r}")
    try:
        ratio, s = float(ratio), float(s)
    except (TypeError, ValueError):
        raise RuntimeError(f"{fn}: ratio and s are numbers, got {ratio!r}, {s!r}") from None
    if not (0.0 < ratio < np.inf and 0.0 <= s < 0.5):
        raise RuntimeError(f"{fn}: ratio must be positive and finite and s in [0, 0.5), got ratio {ratio}, s {s}")
    return dict(ratio=ratio, radius=int(radius), s=s, bins=int(bins))


def ace_weights(radius):
    """The tap weights of the rule, (2 radius + 1, 2 radius + 1) float64: m[dy, dx] = 1.0 / sqrt(dy^2 + dx^2) with the centre
    0, then m /= m.sum() in numpy's own summation.  The device receives this table as data."""
    radius = ace_params(radius=radius, fn="ace_weights")["radius"]
    d = np.arange(-radius, radius + 1, dtype=np.float64)
    q = d[:, None] * d[:, None] + d[None, :] * d[None, :]
    m = np.zeros_like(q)
    m[q > 0.0] = 1.0 / np.sqrt(q[q > 0.0])
    m /= m.sum()
    return m


def _ace_taps_host(n, k):
    """cv2's INTER_LINEAR taps of one axis, source length n -> destination length k: (s0, s1, a0, a1)."""
    scale = float(n) / float(k)
    f = ((np.arange(k, dtype=np.float64) + 0.5) * scale - 0.5).astype(np.float32)
    s0 = np.floor(f)
    f = f - s0
    s0 = s0.astype(np.int64)
    f[s0 < 0] = 0.0
    s0[s0 < 0] = 0
    f[s0 >= n - 1] = 0.0
    s0[s0 >= n - 1] = n - 1
    s1 = np.minimum(s0 + 1, n - 1)
    return s0, s1, (np.float32(1.0) - f).astype(np.float64), f.astype(np.float64)


def ace_resize_host(S, h, w):
    """cv2.resize(S, (w, h)) with its default INTER_LINEAR on a float64 plane, restated.  A source of exactly (2 h, 2 w) takes
    OpenCV's exact-halving switch to the area path: (((S00 + S01) + S10) + S11) * 0.25 over each 2 x 2 block.  Otherwise two
    taps per axis at the half-pixel-centre position, the fraction held in float32 and clamped taps weighted (1, 0): columns
    first, H = S[:, x0] * a0 + S[:, x1] * a1, then rows, H[y0] * b0 + H[y1] * b1, every operation rounded on its own."""
    S = np.asarray(S, np.float64)
    h, w = int(h), int(w)
    if S.ndim != 2 or min(S.shape) <= 0 or h <= 0 or w <= 0:
        raise RuntimeError(f"ace_resize_host: expected a plane (n, m) and a size h, w >= 1, got {S.shape} -> {h} x {w}")
    if S.shape == (2 * h, 2 * w):
        return (((S[0::2, 0::2] + S[0::2, 1::2]) + S[1::2, 0::2]) + S[1::2, 1::2]) * 0.25
    x0, x1, a0, a1 = _ace_taps_host(S.shape[1], w)
    y0, y1, b0, b1 = _ace_taps_host(S.shape[0], h)
    H = S[:, x0] * a0 + S[:, x1] * a1
    return H[y0] * b0[:, None] + H[y1] * b1[:, None]


def ace_ice_host(P, ratio, weights):
    """The tap sum of the rule over one plane: res = 0.0, then for dy, and inside it dx, from -radius to radius without the
    centre, res += m[dy, dx] * clip((P(y, x) - P(cy, cx)) * ratio, -1, 1), (cy, cx) clamped to the plane."""
    h, w = P.shape
    radius = weights.shape[0] // 2
    ys, xs = np.arange(h), np.arange(w)
    res = np.zeros((h, w), np.float64)
    for dy in range(-radius, radius + 1):
        rows = P[np.clip(ys + dy, 0, h - 1)]
        for dx in range(-radius, radius + 1):
            if dy == 0 and dx == 0:
                continue
            res += weights[dy + radius, dx + radius] * np.clip((P - rows[:, np.clip(xs + dx, 0, w - 1)]) * ratio, -1.0, 1.0)
    return res


def ace_bins_host(x, bins):
    """numpy's uniform-bin rule restated as the device applies it: (counts (bins) int64, edges (bins + 1) float64) equal to
    np.histogram(x, bins).  first, last = min, max of x (widened by 0.5 each way when equal); step = (last - first) / bins;
    edge(i) = i * step + first, edge(bins) = last; idx = int(((v - first) / (last - first)) * bins), minus 1 at idx == bins,
    minus 1 where v < edge(idx), plus 1 where v >= edge(idx + 1) and idx != bins - 1."""
    x = np.asarray(x, np.float64).reshape(-1)
    bins = int(bins)
    first, last = float(x.min()), float(x.max())
    if first == last:
        first, last = first - 0.5, last + 0.5
    step = (last - first) / bins
    edges = np.arange(bins + 1, dtype=np.float64) * step + first
    edges[bins] = last
    idx = (((x - first) / (last - first)) * bins).astype(np.int64)
    idx[idx == bins] -= 1
    idx[x < edges[idx]] -= 1
    idx[(x >= edges[idx + 1]) & (idx != bins - 1)] += 1
    return np.bincount(idx, minlength=bins).astype(np.int64), edges


def ace_levels(ih, iw):
    """The pyramid's level sizes [(h_0, w_0), ...]: halved upwards, (n + 1) // 2, down to the first with min(h, w) <= 2."""
    sizes = [(int(ih), int(iw))]
    while min(sizes[-1]) > 2:
        sizes.append(((sizes[-1][0] + 1) // 2, (sizes[-1][1] + 1) // 2))
    return sizes


def ace_host(rgb, ratio=4.0, radius=3, s=0.005, bins=2000):
    """The fast Automatic Colour Equalisation of ONE (ih, iw, 3) uint8 RGB frame in numpy float64, each channel on its own and
    every operation rounded on its own in the order of the header's statement (include/vrnet_hip.h, vrnet_ace_u8):
    I_0 = byte / 255.0; the pyramid I_{L+1} = resize(I_L, (h_L + 1) // 2, (w_L + 1) // 2) down to the first level with
    min(h, w) <= 2, where R = 0.5; above it R_L = (resize(R_{L+1}) + ice(I_L)) - ice(resize(I_{L+1})), both resized to
    (h_L, w_L); then the stretch of R_0 between the edges of np.histogram(R_0, bins) at which the cumulative share reaches s
    and last stays at or below 1.0 - s, clipped to [0, 1], times 255.0 and `saturate_host`.  Returns (bytes (ih, iw, 3) uint8,
    degenerate): an image with min(ih, iw) <= 2, or with lmax <= lmin in any channel (a constant frame), is degenerate and
    comes back unchanged in all three channels.  This is the statement the kernels of csrc/ace.hip are tested against.  The
    OpenCV semantics in it (INTER_LINEAR's float32 fraction and clamped taps, the exact-halving switch to the area path) are
    restated from OpenCV's published behaviour and have never been run against cv2."""
    fn = "ace_host"
    q = ace_params(ratio, radius, s, bins, fn)
    ratio, radius, s, bins = q["ratio"], q["radius"], q["s"], q["bins"]
    rgb = np.asarray(rgb)
    if rgb.dtype != np.uint8 or rgb.ndim != 3 or rgb.shape[2] != 3 or min(rgb.shape) <= 0:
        raise RuntimeError(f"{fn}: expected a uint8 frame (ih, iw, 3), got {rgb.dtype} {rgb.shape}")
    ih, iw = rgb.shape[:2]
    sizes = ace_levels(ih, iw)
    if len(sizes) == 1:
        return rgb.copy(), True
    m = ace_weights(radius)
    out = np.empty_like(rgb)
    for c in range(3):
        planes = [rgb[..., c].astype(np.float64) / 255.0]
        for h, w in sizes[1:]:
            planes.append(ace_resize_host(planes[-1], h, w))
        R = np.full(sizes[-1], 0.5, np.float64)
        for L in range(len(sizes) - 2, -1, -1):
            h, w = sizes[L]
            R = (ace_resize_host(R, h, w) + ace_ice_host(planes[L], ratio, m)) - ace_ice_host(ace_resize_host(planes[L + 1], h, w), ratio, m)
        hist, edges = np.histogram(R, bins)
        d = np.cumsum(hist).astype(np.float64) / float(ih * iw)
        lmin = int(np.flatnonzero(d >= s)[0])
        below = np.flatnonzero(d <= 1.0 - s)
        lmax = int(below[-1]) if len(below) else -1
        if lmax <= lmin:
            return rgb.copy(), True
        v = np.clip((R - edges[lmin]) / (edges[lmax] - edges[lmin]), 0.0, 1.0)
        out[..., c] = saturate_host(v * 255.0)
    return out, False


def ace(frames_u8, sizes=None, geom=None, ratio=4.0, radius=3, s=0.005, bins=2000, flag=None, device="cuda"):
    """`ace_host` on the device (vrnet_ace_u8, two launches per pyramid level plus four, no host synchronisation): frames_u8
    (B, ih, iw, 3) uint8 RGB, numpy or tensor (a single (ih, iw, 3) frame counts as B = 1).  sizes: (B, 2) host integers
    (ih_b, iw_b) when the frames are padded slots with image b in the top-left corner of slot b -- a table is built from
    them --, or geom: the (B, hip.GEOM_BYTES) device table of `data.frame_geometry`; neither: every image fills its slot.
    Outside an image's corner the result is 0.  Returns out (B, ih, iw, 3) uint8 on the device.  flag: a zeroed int32 device
    tensor of one element, or None: it receives FLAG_ACE for a degenerate image (min(ih, iw) <= 2, or a constant R_0), which
    comes back unchanged, and hip.FLAG_GEOMETRY for a bad record of the table, which gives a zero image."""
    from . import hip
    fn = "ace"
    q = ace_params(ratio, radius, s, bins, fn)
    img = _as_frames(frames_u8, "frames", _FRAMES, fn)
    B, ih, iw = img.shape[:3]
    arr = _host_sizes(sizes, geom, B, ih, iw, fn)
    img = img.to(device, non_blocking=True).contiguous()
    dev = img.device
    with torch.cuda.device(dev):
        if arr is not None:
            geom = _sizes_geom(arr, dev)
        weights = torch.from_numpy(ace_weights(q["radius"])).to(dev)
        out = torch.empty_like(img)
        ws = torch.empty(hip.ace_workspace_bytes(B, ih, iw), dtype=torch.uint8, device=dev)
        hip.ace(img, out, ws, weights, geom=geom, flag=flag, **q)
    return out


# ---- baseline JPEG (csrc/jpeg.hip) ---------------------------------------------------------------------------------------------
FLAG_JPEG_ARENA = 262144     # VR_FLAG_JPEG_ARENA of csrc/common.h: a file that did not fit its slot of the arena, length 0
JPEG_HEADER = 623            # bytes in front of the scan data, the same in both modes
JPEG_MAX_BLOCKS = 1 << 20    # blocks of one image: 1658 bits a block at the most, so every bit offset fits 32 bits
# the natural (row-major) index of the coefficient at each zigzag position
JPEG_ZIGZAG = np.array([0, 1, 8, 16, 9, 2, 3, 10, 17, 24, 32, 25, 18, 11, 4, 5, 12, 19, 26, 33, 40, 48, 41, 34, 27, 20, 13, 6, 7, 14, 21, 28,
                        35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23, 30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47,
                        55, 62, 63])
# ITU-T T.81 Annex K.1: the luminance and chrominance quantisation tables at quality 50, row-major
_JPEG_BASE = np.array([[16, 11, 10, 16, 24, 40, 51, 61, 12, 12, 14, 19, 26, 58, 60, 55, 14, 13, 16, 24, 40, 57, 69, 56, 14, 17, 22, 29, 51,
                        87, 80, 62, 18, 22, 37, 56, 68, 109, 103, 77, 24, 35, 55, 64, 81, 104, 113, 92, 49, 64, 78, 87, 103, 121, 120, 101,
                        72, 92, 95, 98, 112, 100, 103, 99],
                       [17, 18, 24, 47, 99, 99, 99, 99, 18, 21, 26, 66, 99, 99, 99, 99, 24, 26, 56, 99, 99, 99, 99, 99, 47, 66, 99, 99, 99,
                        99, 99, 99] + [99] * 32])
# Annex K.3: (code lengths 1..16, values) of the DC luminance, AC luminance, DC chrominance and AC chrominance tables
_JPEG_HUFF = tuple((bytes.fromhex(b), bytes.fromhex(v)) for b, v in (
    ("00010501010101010100000000000000", "000102030405060708090a0b"),
    ("0002010303020403050504040000017d",
     "01020300041105122131410613516107227114328191a1082342b1c11552d1f02433627282090a161718191a25262728292a3435363738393a43444546"
     "4748494a535455565758595a636465666768696a737475767778797a838485868788898a92939495969798999aa2a3a4a5a6a7a8a9aab2b3b4b5b6b7b8"
     "b9bac2c3c4c5c6c7c8c9cad2d3d4d5d6d7d8d9dae1e2e3e4e5e6e7e8e9eaf1f2f3f4f5f6f7f8f9fa"),
    ("00030101010101010101010000000000", "000102030405060708090a0b"),
    ("00020102040403040705040400010277",
     "000102031104052131061241510761711322328108144291a1b1c109233352f0156272d10a162434e125f11718191a262728292a35363738393a434445"
     "464748494a535455565758595a636465666768696a737475767778797a82838485868788898a92939495969798999aa2a3a4a5a6a7a8a9aab2b3b4b5b6"
     "b7b8b9bac2c3c4c5c6c7c8c9cad2d3d4d5d6d7d8d9dae2e3e4e5e6e7e8e9eaf2f3f4f5f6f7f8f9fa")))


def _jpeg_params(quality, subsampling, fn):
    if isinstance(quality, bool) or not isinstance(quality, (int, np.integer)) or not 1 <= int(quality) <= 100:
        raise RuntimeError(f"{fn}: quality is an integer in 1..100, got {quality!r}")
    if isinstance(subsampling, bool) or subsampling not in (0, 2):
        raise RuntimeError(f"{fn}: subsampling is 0 (4:4:4) or 2 (4:2:0), got {subsampling!r}")
    return int(quality), int(subsampling)


def jpeg_tables(quality=95):
    """The two quantisation tables of a quality in 1..100, libjpeg's rule: scale = 5000 // q below 50, else 200 - 2 q, and
    t = clip((base * scale + 50) // 100, 1, 255) on the Annex K tables -> (2, 64) int64, luminance then chrominance, ROW-MAJOR
    (the header and the kernels hold them in zigzag order: `tables[:, JPEG_ZIGZAG]`)."""
    quality, _ = _jpeg_params(quality, 0, "jpeg_tables")
    scale = 5000 // quality if quality < 50 else 200 - 2 * quality
    return np.clip((_JPEG_BASE * scale + 50) // 100, 1, 255)


def jpeg_huffman():
    """The four Annex K Huffman tables as (code, length) pairs by symbol: a (4, 256, 2) int64 array, DC luminance, AC
    luminance, DC chrominance, AC chrominance; length 0: the table has no such symbol.  Codes are assigned as T.81 Annex C
    does: in order of length, counting up."""
    out = np.zeros((4, 256, 2), np.int64)
    for t, (bits, vals) in enumerate(_JPEG_HUFF):
        code, k = 0, 0
        for length in range(1, 17):
            for _ in range(bits[length - 1]):
                out[t, vals[k]] = code, length
                code, k = code + 1, k + 1
            code <<= 1
    return out


def jpeg_header(height, width, quality=95, subsampling=0):
    """The 623 bytes in front of the scan data, as libjpeg writes them for Pillow's `save(format="JPEG", quality=,
    subsampling=)`: SOI, the JFIF 1.01 segment (no units, density 1 x 1), the two quantisation tables in zigzag order, SOF0
    (components 1, 2, 3; sampling 0x11 each for 4:4:4, 0x22, 0x11, 0x11 for 4:2:0; tables 0, 1, 1), the four Annex K Huffman
    tables and the scan header.  Height and width are bytes 163..166, big-endian: the device patches them per image."""
    quality, subsampling = _jpeg_params(quality, subsampling, "jpeg_header")
    if not (0 <= int(height) <= 65535 and 0 <= int(width) <= 65535):
        raise RuntimeError(f"jpeg_header: a JPEG's sides are at most 65535, got {height} x {width}")
    seg = lambda marker, body: bytes([0xFF, marker]) + (len(body) + 2).to_bytes(2, "big") + body
    out = b"\xff\xd8" + seg(0xE0, b"JFIF\0" + bytes([1, 1, 0, 0, 1, 0, 1, 0, 0]))
    for i, t in enumerate(jpeg_tables(quality)):
        out += seg(0xDB, bytes([i]) + bytes(t[JPEG_ZIGZAG].tolist()))
    out += seg(0xC0, bytes([8]) + int(height).to_bytes(2, "big") + int(width).to_bytes(2, "big") +
               bytes([3, 1, 0x22 if subsampling else 0x11, 0, 2, 0x11, 1, 3, 0x11, 1]))
    for (bits, vals), ident in zip(_JPEG_HUFF, (0x00, 0x10, 0x01, 0x11)):
        out += seg(0xC4, bytes([ident]) + bits + vals)
    out += seg(0xDA, bytes([3, 1, 0x00, 2, 0x11, 3, 0x11, 0, 63, 0]))
    assert len(out) == JPEG_HEADER
    return out


def _jpeg_fdct(blocks):
    """libjpeg's jfdctint (CONST_BITS 13, PASS1_BITS 2) on (N, 8, 8) int64 samples minus 128: rows, then columns."""
    def descale(x, n):
        return (x + (1 << (n - 1))) >> n

    def one(d, first):
        t0, t7, t1, t6 = d[..., 0] + d[..., 7], d[..., 0] - d[..., 7], d[..., 1] + d[..., 6], d[..., 1] - d[..., 6]
        t2, t5, t3, t4 = d[..., 2] + d[..., 5], d[..., 2] - d[..., 5], d[..., 3] + d[..., 4], d[..., 3] - d[..., 4]
        t10, t13, t11, t12 = t0 + t3, t0 - t3, t1 + t2, t1 - t2
        n = 11 if first else 15
        out = np.empty_like(d)
        out[..., 0] = (t10 + t11) << 2 if first else descale(t10 + t11, 2)
        out[..., 4] = (t10 - t11) << 2 if first else descale(t10 - t11, 2)
        z1 = (t12 + t13) * 4433
        out[..., 2], out[..., 6] = descale(z1 + t13 * 6270, n), descale(z1 - t12 * 15137, n)
        z1, z2, z3, z4 = t4 + t7, t5 + t6, t4 + t6, t5 + t7
        z5 = (z3 + z4) * 9633
        t4, t5, t6, t7 = t4 * 2446, t5 * 16819, t6 * 25172, t7 * 12299
        z1, z2, z3, z4 = z1 * -7373, z2 * -20995, z3 * -16069 + z5, z4 * -3196 + z5
        out[..., 7], out[..., 5] = descale(t4 + z1 + z3, n), descale(t5 + z2 + z4, n)
        out[..., 3], out[..., 1] = descale(t6 + z2 + z3, n), descale(t7 + z1 + z4, n)
        return out

    rows = one(blocks, True)
    return one(rows.transpose(0, 2, 1), False).transpose(0, 2, 1)


def _jpeg_pad(plane, h, w):
    """plane replicated at its right and lower edge to (h, w)."""
    return np.pad(plane, ((0, h - plane.shape[0]), (0, w - plane.shape[1])), mode="edge")


def jpeg_blocks_host(image_u8, quality=95, subsampling=0):
    """The quantised coefficients of an (h, w, 3) uint8 RGB image in scan order -> (coefficients (N, 64) int64 in zigzag order,
    component (N) of each block: 0, 1, 2, dummy (N) bool).  A dummy block (a Y block of a 4:2:0 MCU beyond ceil(h / 8) block
    rows or ceil(w / 8) block columns) has no AC and the DC of the block in front of it."""
    fn = "jpeg_encode_host"
    quality, subsampling = _jpeg_params(quality, subsampling, fn)
    a = np.asarray(image_u8)
    if a.dtype != np.uint8 or a.ndim != 3 or a.shape[2] != 3 or min(a.shape) < 1 or max(a.shape[:2]) > 65535:
        raise RuntimeError(f"{fn}: expected an (h, w, 3) uint8 image with sides in 1..65535, got {a.dtype} {a.shape}")
    h, w = a.shape[:2]
    F = lambda x: int(x * 65536 + 0.5)
    R, G, B = (a[..., c].astype(np.int64) for c in range(3))
    Y = (F(.299) * R + F(.587) * G + F(.114) * B + 32768) >> 16
    Cb = (-F(.16874) * R - F(.33126) * G + F(.5) * B + (128 << 16) + 32767) >> 16
    Cr = (F(.5) * R - F(.41869) * G - F(.08131) * B + (128 << 16) + 32767) >> 16
    split = lambda p: p.reshape(p.shape[0] // 8, 8, p.shape[1] // 8, 8).transpose(0, 2, 1, 3)      # (block rows, block cols, 8, 8)
    if subsampling == 0:
        MH, MW = -(-h // 8), -(-w // 8)
        units = np.stack([split(_jpeg_pad(p, 8 * MH, 8 * MW)) for p in (Y, Cb, Cr)], axis=2)      # (MH, MW, 3, 8, 8)
        comp, dummy = np.tile(np.arange(3), MH * MW), np.zeros(3 * MH * MW, bool)
    else:
        MH, MW = -(-h // 16), -(-w // 16)
        yb = split(_jpeg_pad(Y, 16 * MH, 16 * MW)).reshape(MH, 2, MW, 2, 8, 8).transpose(0, 2, 1, 3, 4, 5).reshape(MH, MW, 4, 8, 8)
        by, bx = np.meshgrid(np.arange(2 * MH), np.arange(2 * MW), indexing="ij")
        dm = ((by >= -(-h // 8)) | (bx >= -(-w // 8))).reshape(MH, 2, MW, 2).transpose(0, 2, 1, 3).reshape(MH, MW, 4)
        bias = np.tile(np.array([1, 2]), 4 * MW)
        small = []
        for p in (Cb, Cr):
            p = _jpeg_pad(p, h + (h & 1), 16 * MW)
            p = (p[0::2, 0::2] + p[0::2, 1::2] + p[1::2, 0::2] + p[1::2, 1::2] + bias) >> 2
            small.append(split(_jpeg_pad(p, 8 * MH, 8 * MW))[:, :, None])
        units = np.concatenate([yb] + small, axis=2)                                               # (MH, MW, 6, 8, 8)
        comp = np.tile(np.array([0, 0, 0, 0, 1, 2]), MH * MW)
        dummy = np.concatenate([dm, np.zeros((MH, MW, 2), bool)], axis=2).reshape(-1)
    if len(comp) > JPEG_MAX_BLOCKS:
        raise RuntimeError(f"{fn}: {len(comp)} blocks; at most {JPEG_MAX_BLOCKS} an image")
    c = _jpeg_fdct(units.reshape(-1, 8, 8) - 128).reshape(-1, 64)[:, JPEG_ZIGZAG]
    d = 8 * jpeg_tables(quality)[:, JPEG_ZIGZAG][np.minimum(comp, 1)]
    q = np.sign(c) * ((np.abs(c) + (d >> 1)) // d)
    for k in np.flatnonzero(dummy):           # in order: a dummy may follow a dummy
        q[k, 0], q[k, 1:] = q[k - 1, 0], 0
    return q, comp, dummy


def _jpeg_bits(values, lengths):
    """The bits of (value, length <= 63) items, most significant first, as one uint8 array of 0 / 1."""
    lengths = np.asarray(lengths, np.int64)
    ends = np.cumsum(lengths)
    j = np.arange(int(ends[-1]) if len(ends) else 0) - np.repeat(ends - lengths, lengths)      # the bit's index in its item
    return ((np.repeat(np.asarray(values, np.uint64), lengths) >> (np.repeat(lengths, lengths) - 1 - j).astype(np.uint64)) & 1).astype(np.uint8)


def jpeg_scan_host(q, comp):
    """The entropy-coded scan of `jpeg_blocks_host`'s blocks, byte-stuffed, without EOI: one DC predictor per component from
    0 on, never reset; category bit_length(|v|), value bits the low s bits of v (of v - 1 when v < 0); AC as (run << 4) | s in
    zigzag order, 0xF0 for each full run of 16 zeros in front of a non-zero and 0x00 where the block ends in zeros; bits MSB
    first, the last byte padded with ones, every 0xFF byte followed by 0x00.  Returns (bytes, ZRL symbols coded)."""
    huff = jpeg_huffman()
    N = len(q)
    diff = q[:, 0].copy()
    for c in range(3):
        k = np.flatnonzero(comp == c)
        diff[k] = np.diff(q[k, 0], prepend=0)
    cat = lambda v: np.where(v == 0, 0, np.floor(np.log2(np.maximum(np.abs(v), 1))).astype(np.int64) + 1)   # exact below 2^52
    extra = lambda v, s: (np.where(v < 0, v - 1, v) & ((1 << s) - 1))
    chroma = np.minimum(comp, 1)
    s = cat(diff)
    code = huff[2 * chroma, s]
    items = [(np.arange(N) * 65, (code[:, 0] << s) | extra(diff, s), code[:, 1] + s)]           # key, value, length
    blk, pos = np.nonzero(q[:, 1:])
    pos = pos + 1
    first = np.ones(len(blk), bool)
    first[1:] = blk[1:] != blk[:-1]
    run = pos - np.where(first, 0, np.concatenate([[0], pos[:-1]])) - 1
    v = q[blk, pos]
    s = cat(v)
    tab = 2 * chroma[blk] + 1
    sym, zrl = huff[tab, ((run & 15) << 4) | s], huff[tab, 0xF0]
    val, length = (sym[:, 0] << s) | extra(v, s), sym[:, 1] + s
    for n in range(1, 4):                     # a run of up to 62 zeros: at most three ZRL in front of the symbol
        more = (run >> 4) >= n
        val, length = np.where(more, (zrl[:, 0] << length) | val, val), np.where(more, length + zrl[:, 1], length)
    items.append((blk * 65 + pos, val, length))
    eob = np.flatnonzero(q[:, 63] == 0)
    e = huff[2 * chroma[eob] + 1, 0]
    items.append((eob * 65 + 64, e[:, 0], e[:, 1]))
    key, val, length = (np.concatenate([it[i] for it in items]) for i in range(3))
    order = np.argsort(key, kind="stable")
    bits = _jpeg_bits(val[order], length[order])
    bits = np.concatenate([bits, np.ones(-len(bits) % 8, np.uint8)])
    raw = np.packbits(bits)
    at = np.flatnonzero(raw == 0xFF)
    return bytes(np.insert(raw, at + 1, 0).tolist()), int((run >> 4).sum())


def jpeg_encode_host(image_u8, quality=95, subsampling=0):
    """The rule of `jpeg_encode` in numpy: the baseline JPEG file of an (h, w, 3) uint8 RGB image, every byte the one Pillow
    (libjpeg-turbo) writes for `Image.save(format="JPEG", quality=quality, subsampling=subsampling)` -- `jpeg_header`, the
    scan of `jpeg_blocks_host` / `jpeg_scan_host` (integer colour conversion, edge replication, the 4:2:0 box reduction with
    its alternating bias, jfdctint, rounding quantisation, the Annex K Huffman tables, byte stuffing) and EOI.  Everything is
    integer arithmetic.  subsampling: 0 (4:4:4) or 2 (4:2:0)."""
    q, comp, _ = jpeg_blocks_host(image_u8, quality, subsampling)
    h, w = np.asarray(image_u8).shape[:2]
    return jpeg_header(h, w, quality, subsampling) + jpeg_scan_host(q, comp)[0] + b"\xff\xd9"


class Jpegs:
    """What `jpeg_encode` leaves on the device: arena (B, capacity) uint8, slot b a complete JPEG file in its first
    record[b, 0] bytes; record (B, 2) int32 = (length, state) -- state 1: a file; 2: the file did not fit the capacity, length
    0 and FLAG_JPEG_ARENA in flag; 3: an image without pixels --; flag (1) int32.  Bytes of a slot behind its length are not
    defined.  From a pipeline these are its own buffers: the next run overwrites them."""
    __slots__ = ("arena", "record", "flag", "quality", "subsampling", "header", "workspace")

    def __init__(self, arena, record, flag, quality, subsampling, header, workspace):
        self.arena, self.record, self.flag, self.quality, self.subsampling = arena, record, flag, int(quality), int(subsampling)
        self.header, self.workspace = header, workspace

    @property
    def capacity(self):
        return self.arena.shape[1]

    def bytes(self):
        """The files as a list of `bytes`, b"" for an image whose file did not fit: the record is read back first (which waits
        for the device), then only the used bytes of every slot, gathered into one copy."""
        lengths = np.clip(self.record.cpu().numpy()[:, 0].astype(np.int64), 0, self.capacity)
        if not lengths.sum():
            return [b""] * len(lengths)
        used = torch.cat([self.arena[b, :int(n)] for b, n in enumerate(lengths) if n]).cpu().numpy().tobytes()
        ends = np.cumsum(lengths)
        return [used[e - n:e] for e, n in zip(ends.tolist(), lengths.tolist())]

    def save(self, paths):
        """Writes file b to paths[b] (None, or an image without a file: nothing is written).  Returns the files of `bytes`."""
        files = self.bytes()
        if len(paths) != len(files):
            raise RuntimeError(f"Jpegs.save: {len(paths)} paths for {len(files)} images")
        for path, data in zip(paths, files):
            if path is not None and data:
                with open(path, "wb") as f:
                    f.write(data)
        return files


def jpeg_capacity(h, w):
    """The default bytes of a slot of the arena: the header plus 3 h w.  A cap the caller may change, not a bound: noise at
    quality 100 exceeds it."""
    return JPEG_HEADER + 3 * int(h) * int(w)


def jpeg_shape(h, w, subsampling, fn="jpeg_encode"):
    """The host check that bounds an image so that the kernels' 32-bit bit offsets suffice: sides in 1..65535 and at most
    JPEG_MAX_BLOCKS blocks (a block codes to at most 1658 bits).  Returns the blocks of an (h, w) image."""
    blocks = 6 * (-(-h // 16)) * (-(-w // 16)) if subsampling else 3 * (-(-h // 8)) * (-(-w // 8))
    if not (1 <= h <= 65535 and 1 <= w <= 65535) or blocks > JPEG_MAX_BLOCKS:
        raise RuntimeError(f"{fn}: images of {h} x {w}: sides are 1..65535 and an image has at most {JPEG_MAX_BLOCKS} blocks "
                           f"(bit offsets are 32-bit), this one {blocks}")
    return blocks


def jpeg_buffers(batch, h, w, quality=95, subsampling=0, capacity=None, flag=None, device="cuda", fn="jpeg_encode"):
    """The device buffers of one `hip.jpeg_encode` call on (batch, h, w, 3) slots as a `Jpegs`: arena, record, the header
    template and the workspace.  The keywords are checked here, on the host."""
    from . import hip
    quality, subsampling = _jpeg_params(quality, subsampling, fn)
    if capacity is None:
        capacity = jpeg_capacity(h, w)
    if isinstance(capacity, bool) or not isinstance(capacity, (int, np.integer)) or not JPEG_HEADER + 2 <= int(capacity) < (1 << 31) - 64:
        raise RuntimeError(f"{fn}: capacity is the bytes of one slot of the arena, {JPEG_HEADER + 2}..2^31 - 65, got {capacity!r}")
    jpeg_shape(h, w, subsampling, fn)
    ws = torch.empty(hip.jpeg_workspace_bytes(batch, h, w, subsampling, int(capacity)), dtype=torch.uint8, device=device)
    header = torch.from_numpy(np.frombuffer(jpeg_header(0, 0, quality, subsampling), np.uint8).copy()).to(device)
    if flag is None:
        flag = torch.zeros(1, dtype=torch.int32, device=device)
    return Jpegs(torch.empty((batch, int(capacity)), dtype=torch.uint8, device=device),
                 torch.zeros((batch, 2), dtype=torch.int32, device=device), flag, quality, subsampling, header, ws)


def jpeg_encode(images_u8, quality=95, subsampling=0, sizes=None, geom=None, capacity=None, flag=None, device="cuda"):
    """Baseline JPEG files on the device by the rule of `jpeg_encode_host` (vrnet_jpeg_encode_u8, eight launches, no host
    synchronisation): images_u8 (N, h, w, 3) uint8 RGB, numpy or tensor (a single (h, w, 3) image counts as N = 1) -- frames,
    rendered pictures, heat maps, the chips tensor of a `Chips`.  quality 1..100 and subsampling 0 (4:4:4) or 2 (4:2:0) as
    Pillow's `save`.  sizes: (N, 2) host integers (h_b, w_b) when the images are padded slots with image b in the top-left
    corner of slot b, or geom: the (N, hip.GEOM_BYTES) device table of `data.frame_geometry`; neither: every image fills its
    slot.  capacity: the bytes of one slot of the arena, default `jpeg_capacity(h, w)`; a file that does not fit gets length
    0 and FLAG_JPEG_ARENA in flag (a zeroed int32 device tensor of one element; None: one is made), the others are
    unaffected.  Returns a `Jpegs`."""
    from . import hip
    fn = "jpeg_encode"
    img = _as_frames(images_u8, "images", "(N, h, w, 3) or (h, w, 3)", fn)
    B, h, w = img.shape[:3]
    table = _host_sizes(sizes, geom, B, h, w, fn)
    _jpeg_params(quality, subsampling, fn)    # before anything is enqueued
    img = img.to(device, non_blocking=True).contiguous()
    dev = img.device
    with torch.cuda.device(dev):
        out = jpeg_buffers(B, h, w, quality, subsampling, capacity, flag, dev, fn)
        if table is not None:
            table = torch.from_numpy(np.ascontiguousarray(table, np.int32)).pin_memory().to(dev, non_blocking=True)
        hip.jpeg_encode(img, out.header, out.arena, out.record, out.workspace, out.subsampling, sizes=table, geom=geom, flag=out.flag)
    return out
