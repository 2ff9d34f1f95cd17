"""Frame-to-result inference as ONE replayed hipGraph: the joint detection + segmentation of a camera-plus-radar stream
that the reference runs frame by frame (predict.py modes `video` and `fps`; `detect_image` / `get_FPS` of yolo.py and
deeplab.py), from raw frame bytes and radar maps to detections, class map, counts and the rendered frame, all on the
device and without a host synchronisation until the caller reads a result.

The chain inside `FramePipeline` is data.device_letterbox -> (data.device_radar) -> the eval-mode forward ->
decode.decode_outputs -> hip.detect_select -> hip.nms_capped -> hip.detect_finish -> decode.seg_predict ->
render.render_frame on the device (draw_rows, offsets) pair.  `decode.non_max_suppression` sizes its buffers from a
read-back of the candidate counts and maps the kept rows on the host; here the candidate capacity is fixed
(`max_candidates`), every candidate is ranked and the best `cap` enter the NMS (the exact prefix of the uncapped result),
and the letterbox un-map, the renderer's integer rows and the class counts are made by one kernel from the kept rows.

Bits of `FrameResult.flag` (an int32 word, zeroed by every run; read it when you read a result): render.FLAG_CLASS,
FLAG_BOX_COLOUR, FLAG_BOX_ROWS (see render.render_frame), FLAG_CANDIDATES -- an image had more candidates than the
capacity, so only its `cap` best-scored ones were considered -- and FLAG_DET_CLASS -- a kept row with a class id
outside [0, num_classes), which is not counted -- and, in a ragged pipeline, FLAG_GEOMETRY -- a record of the geometry
table had to be clamped by a kernel, which the host checks of `run` rule out.  A pipeline built with crops= adds
hip.crop_boxes behind hip.detect_finish and FLAG_CROP_ARENA, a crop that did not fit into the arena.  A pipeline built with
chips= adds hip.chip_boxes behind that (behind hip.detect_finish without crops): the same crops at one size; no new bit.  A
pipeline built with dehaze= puts hip.dehaze in front of the letterbox, so that everything downstream reads the dehazed frames, and adds
FLAG_DEHAZE, a degenerate image that went on unchanged.  A pipeline built with ace= puts hip.ace there too, behind hip.dehaze
when both are on, and adds FLAG_ACE for its degenerate images.  A pipeline built with radar_points and box_radar= adds
hip.box_radar behind the finish node (behind the crops): the radar readout of every kept detection; FLAG_BOX_COUNT, a kept count
outside the row buffer, is ruled out by the NMS that writes it.  A pipeline built with track= adds hip.track_update behind
that (behind the crops or the finish node without box_radar) and in front of decode.seg_predict: every batch slot becomes a
stream whose track table lives on the device across runs, and FLAG_TRACK_FULL says that a valid row found no free slot in it
and got track id 0.  A pipeline built with captions= adds hip.caption_text behind that (behind hip.box_radar without a tracker) and
hip.render_captions behind the label launches (behind the render node without labels): '#<track id> <range>m <speed>m/s'
under every rendered box; FLAG_CAPTION says that a range or a speed could not be drawn and was left out.  A pipeline built
with regions= adds hip.seg_regions directly behind decode.seg_predict and in front of the render node: the connected regions
of the class map, linked both ways with the kept rows; FLAG_REGIONS says that an image had more regions than the table holds.

ragged=True lifts the one-size limit: the pipeline is built for a CAPACITY (ihm, iwm), every frame of a call has its own
size inside it, and the per-image geometry travels in a small device table (`data.frame_geometry`) instead of the launch
arguments, so ONE captured graph serves any mix of sizes.  `predict_dir` is predict.py's `dir_predict` mode on top of it."""
import os

import numpy as np
import torch

from . import data
from . import render as rendering

FLAG_CANDIDATES, FLAG_DET_CLASS = 8, 16          # NMS_FLAG_* of csrc/nms.hip, above render.FLAG_*
FLAG_GEOMETRY = 256                              # VR_FLAG_GEOMETRY of csrc/common.h, above evaluate.FLAG_EVAL_*
FLAG_BOX_COUNT = 512                             # VR_FLAG_BOX_COUNT of csrc/common.h (a pipeline built with box_radar): kept outside [0, cap]
FLAG_POINT_COUNT = 1024                          # VR_FLAG_POINT_COUNT of csrc/common.h (a pipeline built with radar_points)
FLAG_LABEL_SCORE = rendering.FLAG_LABEL_SCORE    # 2048, csrc/labels.hip (a pipeline built with labels): a score outside [0, 1]
FLAG_CROP_ARENA = rendering.FLAG_CROP_ARENA      # 4096, csrc/crops.hip (a pipeline built with crops): a crop that did not fit
FLAG_DEHAZE = rendering.FLAG_DEHAZE              # 8192, csrc/dehaze.hip (a pipeline built with dehaze): a degenerate image, unchanged
FLAG_ACE = rendering.FLAG_ACE                    # 16384, csrc/ace.hip (a pipeline built with ace): a degenerate image, unchanged
FLAG_TRACK_FULL = data.FLAG_TRACK_FULL           # 32768, VR_FLAG_TRACK_FULL of csrc/common.h (a pipeline built with track): the table was full
FLAG_CAPTION = rendering.FLAG_CAPTION            # 65536, VR_FLAG_CAPTION of csrc/common.h (a pipeline built with captions): a field left out
FLAG_REGIONS = 131072                            # VR_FLAG_REGIONS of csrc/common.h (a pipeline built with regions): more regions than the table
# the picture formats predict.py's dir_predict mode accepts, matched against the lower-cased file name
IMAGE_EXTENSIONS = tuple("." + e for e in "bmp dib jpeg jpg pbm pgm png ppm tif tiff".split())


def validate_config(model, frame_shape, input_shape, batch, max_candidates):
    """The constructor's checks that need no device; returns ((ih, iw), (H, W), batch, max_candidates) as ints."""
    if getattr(model, "training", True):
        raise RuntimeError("FramePipeline: the model must be in eval mode (model.eval()): a training-mode forward updates the "
                           "BatchNorm statistics with every frame")
    try:
        (ih, iw), (H, W) = (int(v) for v in frame_shape), (int(v) for v in input_shape)
    except (TypeError, ValueError):
        raise RuntimeError(f"FramePipeline: frame_shape and input_shape are (height, width) pairs, got {frame_shape!r} and "
                           f"{input_shape!r}") from None
    if min(ih, iw, H, W) <= 0 or int(batch) < 1:
        raise RuntimeError(f"FramePipeline: bad shapes (batch {batch}, frames {ih} x {iw}, input {H} x {W})")
    if isinstance(max_candidates, bool) or int(max_candidates) != max_candidates or \
            not 1 <= int(max_candidates) <= rendering.MAX_BOXES:
        raise RuntimeError(f"FramePipeline: max_candidates must be an integer in 1..{rendering.MAX_BOXES} (the renderer's box rows "
                           f"per image), got {max_candidates!r}")
    return (ih, iw), (H, W), int(batch), int(max_candidates)


def validate_inputs(frames_u8, radar, batch, frame_shape, input_shape, radar_points=None, calib=None, letterbox_image=True):
    """frames (B, ih, iw, 3) uint8 and radar (B, 4, H, W) float32 / float64, numpy arrays or tensors, of exactly the
    shapes the pipeline was built for (with batch 1 the leading axis may be missing); returns them as tensors.
    radar_points (a `RadarPoints`): radar holds points, and the pair `RadarPoints.validate` gives is returned for it."""
    f = frames_u8 if torch.is_tensor(frames_u8) else torch.from_numpy(np.ascontiguousarray(frames_u8))
    if f.dtype != torch.uint8:
        raise RuntimeError(f"FramePipeline: expected uint8 frames, got {f.dtype}")
    if radar_points is not None:
        r = radar_points.validate(radar, data.frame_geometry([tuple(frame_shape)] * batch, input_shape, letterbox_image,
                                                             fn="FramePipeline"), calib)
    else:
        r = validate_radar(radar, batch, input_shape)
    f = f[None] if batch == 1 and f.dim() == 3 else f
    want_f = (batch,) + tuple(frame_shape) + (3,)
    if tuple(f.shape) != want_f:
        raise RuntimeError(f"FramePipeline: built for frames of shape {want_f}, got {tuple(f.shape)} (a pipeline is tied to its "
                           "shapes: build another one for another frame size or batch)")
    return f, r


def validate_radar(radar, batch, input_shape):
    """The radar half of `validate_inputs`: (B, 4, H, W) float32 / float64 as a tensor."""
    r = radar if torch.is_tensor(radar) else torch.from_numpy(np.ascontiguousarray(radar))
    if r.dtype not in (torch.float32, torch.float64):
        raise RuntimeError(f"FramePipeline: expected float32 or float64 radar maps, got {r.dtype}")
    r = r[None] if batch == 1 and r.dim() == 3 else r
    if tuple(r.shape) != (batch, 4) + tuple(input_shape):
        raise RuntimeError(f"FramePipeline: built for radar maps of shape {(batch, 4) + tuple(input_shape)}, got {tuple(r.shape)}")
    return r


class RadarPoints:
    """The radar half of a pipeline built with radar_points: what every call brings in place of finished maps.  max_points is
    the capacity of the static point buffer, radius / min_depth the rule of `data.radar_map`, calib the default (3, 4) or
    (B, 3, 4) projection (a call may bring its own).  per_image > 1: the batch is that many SOURCES per output image (Mosaic),
    and a message names point set s as "image s // per_image, tile s % per_image".  Host only, but for `buffers` and
    `workspace`."""

    def __init__(self, max_points, radius=0, min_depth=0.1, calib=None, batch=1, fn="FramePipeline", per_image=1):
        if isinstance(max_points, bool) or not isinstance(max_points, (int, np.integer)) or not 1 <= int(max_points) <= 1 << 24:
            raise RuntimeError(f"{fn}: radar_points is the capacity of the point buffer, an integer in 1..{1 << 24}, got {max_points!r}")
        self.max_points, self.batch, self.fn = int(max_points), int(batch), fn
        self.where = None if per_image == 1 else (lambda s: f"image {s // per_image}, tile {s % per_image}")
        self.radius, self.min_depth = data.check_radar_rule(radius, min_depth, fn)
        self.calib = None if calib is None else data.check_calib(calib, self.batch, fn)

    def validate(self, points, table, calib=None):
        """points as `data.pack_points` takes them, the geometry or augmentation table of the call -> (the pinned (B,
        max_points, 7) tensor, the (B, hip.RADAR_VIEW_BYTES) uint8 view table).  table=None: a table that does not exist yet."""
        if (torch.is_tensor(points) or isinstance(points, np.ndarray)) and points.ndim == 4:
            raise RuntimeError(f"{self.fn}: built with radar_points: a call brings radar POINTS, B arrays of (n, 7) float32 rows, "
                               "not finished maps")
        P = self.calib if calib is None else data.check_calib(calib, self.batch, self.fn)
        if P is None:
            raise RuntimeError(f"{self.fn}: radar points need a projection: calib=(3, 4) or (B, 3, 4), here or at construction")
        packed, counts = data.pack_points(points, self.max_points, self.where)
        if len(counts) != self.batch:
            raise RuntimeError(f"{self.fn}: {len(counts)} point sets for a batch of {self.batch}")
        if table is None:                    # the caller's table follows: `views` finishes the pair
            return packed, (P, counts)
        return packed, self.views(table, (P, counts))

    @staticmethod
    def views(table, checked):
        """The view table from what `validate(points, None)` returned beside the points."""
        return data.radar_view_bytes(data.radar_views(table, checked[0], checked[1].numpy()))

    def buffers(self, table, device):
        """The static device buffers (points, views) of a pipeline, on a table without points."""
        B = self.batch
        P = self.calib if self.calib is not None else np.zeros((B, 3, 4), np.float32)
        views = data.radar_view_bytes(data.radar_views(table, P, np.zeros(B, np.int32))).to(device)
        return torch.zeros((B, self.max_points, 7), dtype=torch.float32, device=device), views

    def workspace(self, input_shape, device):
        from . import hip
        return torch.empty(hip.radar_map_workspace_bytes(self.batch, *input_shape), dtype=torch.uint8, device=device)


def validate_ragged_inputs(frames, radar, sizes, batch, capacity, input_shape, letterbox_image=True, max_taps=None,
                           radar_points=None, calib=None):
    """The host checks of a ragged `run`, which need no device: frames as a list of `batch` uint8 arrays (ih_b, iw_b, 3) of
    their own sizes (sizes optional, checked when given) or a padded (batch, ihp, iwp, 3) buffer with sizes (batch, 2);
    every size inside the capacity, with a non-empty window and within the tap capacity (`data.frame_geometry`: each
    error names the image index).  Returns (frames as `data.ragged_items` gives them, radar tensor, sizes (B, 2) int64,
    the geometry table).  radar_points (a `RadarPoints`): radar holds points, and the radar tensor returned is the pair
    `RadarPoints.validate` gives."""
    fn = "FramePipeline"
    items, own = data.ragged_items(frames, sizes, batch, (3,), "frames", fn)
    if torch.is_tensor(items) and (items.shape[1] > capacity[0] or items.shape[2] > capacity[1]):
        raise RuntimeError(f"{fn}: the padded buffer {tuple(items.shape[1:3])} is above the capacity {tuple(capacity)}")
    max_taps = data.default_max_taps(capacity, input_shape) if max_taps is None else max_taps
    table = data.frame_geometry(own, input_shape, letterbox_image, capacity, max_taps, fn)
    if radar_points is not None:
        return items, radar_points.validate(radar, table, calib), own, table
    return items, validate_radar(radar, batch, input_shape), own, table


def crop_capacity(crops, batch, frame_shape):
    """The pixels of a pipeline's crop arena from its crops= keyword: None (no crops), True (2 * batch * ihm * iwm, at most
    2^30) or the number itself, 1..2^30."""
    if crops is None or crops is False:
        return None
    if crops is True:
        return min(2 * int(batch) * int(frame_shape[0]) * int(frame_shape[1]), 1 << 30)
    if not isinstance(crops, (int, np.integer)) or not 1 <= int(crops) <= 1 << 30:
        raise RuntimeError(f"FramePipeline: crops is None, True or the capacity of the crop arena, 1..2^30 pixels, got {crops!r}")
    return int(crops)


def chip_config(chips):
    """The fixed-size chips of a pipeline from its chips= keyword: None (no chips), a size (sh, sw), or a dict of size,
    letterbox and normalised.  Returns None or a dict of all three, the size checked (sides in 1..render.CHIP_MAX)."""
    if chips is None or chips is False:
        return None
    cfg = dict(chips) if isinstance(chips, dict) else {"size": chips}
    if "size" not in cfg or set(cfg) - {"size", "letterbox", "normalised"}:
        raise RuntimeError(f"FramePipeline: chips is None, a size (sh, sw) or a dict of size, letterbox, normalised, got {chips!r}")
    return dict(size=rendering._chip_size(cfg["size"], "FramePipeline: chips"), letterbox=bool(cfg.get("letterbox", False)),
                normalised=bool(cfg.get("normalised", False)))


def dehaze_config(dehaze):
    """The parameters of a pipeline's dehazing stage from its dehaze= keyword: None (no stage), True (the defaults of
    `render.dehaze_host`) or a dict of its keywords sz, r, eps, omega, tx; checked by `render.dehaze_params`."""
    if dehaze is None or dehaze is False:
        return None
    if dehaze is True:
        dehaze = {}
    if not isinstance(dehaze, dict) or set(dehaze) - {"sz", "r", "eps", "omega", "tx"}:
        raise RuntimeError(f"FramePipeline: dehaze is None, True or a dict of sz, r, eps, omega, tx, got {dehaze!r}")
    return rendering.dehaze_params(fn="FramePipeline", **dehaze)


def ace_config(ace):
    """The parameters of a pipeline's ACE stage from its ace= keyword: None (no stage), True (the defaults of
    `render.ace_host`) or a dict of its keywords ratio, radius, s, bins; checked by `render.ace_params`."""
    if ace is None or ace is False:
        return None
    if ace is True:
        ace = {}
    if not isinstance(ace, dict) or set(ace) - {"ratio", "radius", "s", "bins"}:
        raise RuntimeError(f"FramePipeline: ace is None, True or a dict of ratio, radius, s, bins, got {ace!r}")
    return rendering.ace_params(fn="FramePipeline", **ace)


def caption_config(captions, render, track, box_radar, ragged, ih):
    """The captions= keyword of a pipeline, checked on the host: None (no captions), True, a `render.GlyphAtlas` or a dict of
    atlas, fps, font, sizes -> (composing, fps, size index); composing is the atlas, or True where a fixed-size pipeline of
    frames lower than 17 rows composes the text and draws nothing; the size index is that of a fixed-size pipeline's one
    font size (None: nothing is drawn, or a ragged pipeline, whose table follows each call).  Names what is missing."""
    fn = "FramePipeline"
    if captions is None or captions is False:
        return None, 0.0, None
    if captions is True:
        captions = {}
    elif isinstance(captions, rendering.GlyphAtlas):
        captions = {"atlas": captions}
    if not isinstance(captions, dict) or set(captions) - {"atlas", "fps", "font", "sizes"}:
        raise RuntimeError(f"{fn}: captions is None, True, a render.GlyphAtlas or a dict of atlas, fps, font, sizes, got {captions!r}")
    if not render:
        raise RuntimeError(f"{fn}: captions are drawn on the rendered frame; they need render=True")
    if not (track or box_radar):
        raise RuntimeError(f"{fn}: captions show track ids and radar ranges; they need track= or box_radar=True (or both), and this "
                           "pipeline has neither")
    fps = captions.get("fps", 0.0)
    if isinstance(fps, bool) or not isinstance(fps, (int, float, np.integer, np.floating)) or not 0.0 <= float(fps) <= 1e6:
        raise RuntimeError(f"{fn}: captions: fps is the frame rate of the streams, a number in [0, 1e6], got {fps!r}")
    if float(fps) > 0 and not (track and box_radar):
        raise RuntimeError(f"{fn}: captions: fps draws the closing speed, the rate of the tracker's filtered radar range; it needs "
                           f"track= together with box_radar=True, and this pipeline lacks {'box_radar=True' if track else 'track='}")
    atlas, size = captions.get("atlas"), rendering.label_font_size(ih)
    if atlas is not None:
        if not isinstance(atlas, rendering.GlyphAtlas) or captions.get("font") is not None or captions.get("sizes") is not None:
            raise RuntimeError(f"{fn}: captions: atlas is a render.GlyphAtlas, which brings its own font and sizes")
    elif not ragged and size == 0:
        if captions.get("sizes") is not None:
            raise RuntimeError(f"{fn}: captions: sizes belongs to a ragged pipeline; a fixed-size one builds font size {size}")
        return True, float(fps), None
    else:
        sizes = captions.get("sizes")
        if sizes is None:
            sizes = tuple(range(1, size + 1)) if ragged else (size,)
        elif not ragged:
            raise RuntimeError(f"{fn}: captions: sizes belongs to a ragged pipeline; a fixed-size one builds font size {size}")
        if not len(tuple(sizes)):
            raise RuntimeError(f"{fn}: captions: a capacity of {ih} rows has no font size >= 1 to build")
        atlas = rendering.GlyphAtlas(captions.get("font"), sizes)
    if ragged:
        return atlas, float(fps), None
    return atlas, float(fps), None if size == 0 else atlas.size_index(size)


def unmap_scalars(input_shape, image_shape, letterbox_image):
    """(offset, scale): the (y, x) float64 pairs with which decode.yolo_correct_boxes maps a centre, (c - offset) * scale, and a
    size, s * scale -- its own expressions, np.round included; (0, 0), (1, 1) without a letterbox."""
    if not letterbox_image:
        return (0.0, 0.0), (1.0, 1.0)
    net_hw = np.asarray(input_shape, dtype=np.float64)
    img_hw = np.asarray(image_shape, dtype=np.float64)
    inner = np.round(img_hw * (net_hw / img_hw).min())
    return tuple(0.5 * (net_hw - inner) / net_hw), tuple(net_hw / inner)


class FrameResult:
    """What one `FramePipeline.run` leaves on the device.  The tensors are the pipeline's own buffers: the next `run`
    overwrites them, so read (or clone) what you need first.
    rows (B, cap, 7) float32: top, left, bottom, right in pixels of the original frame, obj, class_conf, class, in descending
    score order, zero from row kept[b] on; kept (B) int32; det_counts (B, num_classes) int64; class_map (B, ih, iw) uint8;
    seg_counts (B, len(seg palette)) int64 pixels per class and rendered (B, ih, iw, 3) uint8, both None with render=False;
    flag (1) int32, the data-error bits of the module docstring.
    From a ragged pipeline class_map (B, ihm, iwm) and rendered (B, ihm, iwm, 3) are PADDED tensors of the capacity: image b
    is `class_map[b, :ih_b, :iw_b]` / `rendered[b, :ih_b, :iw_b]` with (ih_b, iw_b) = sizes[b], everything outside it is 0,
    and seg_counts[b] counts the image's own pixels only.  sizes: the (B, 2) host integers of that run (None from a
    fixed-size pipeline).
    From a pipeline with heatmap=True (None otherwise): heat_mask (B, ih, iw) uint8, heat_picture (B, ih, iw, 3) uint8 and
    heat_range (B, 2) int32 = each mask's (min, max), what `render.heatmap` returns for the frames and the raw detection
    maps of the run; padded like class_map / rendered from a ragged pipeline.
    From a pipeline built with crops (None otherwise): crops, the `render.Crops` of the run -- every kept detection cut out
    of the original frame, `crops.images()[b][i]` being row i of image b.
    From a pipeline built with chips (None otherwise): chips, the `render.Chips` of the run -- the same crops brought to one
    size, `chips.chips[n]` (and `chips.chips_f32[n]`) being draw row n and `chips.images()[b][i]` row i of image b.
    From a pipeline built with dehaze (None otherwise): dehazed (B, ih, iw, 3) uint8, the frames everything else of the
    result was computed from; padded like rendered from a ragged pipeline.
    From a pipeline built with ace (None otherwise): enhanced (B, ih, iw, 3) uint8, the output of the ACE stage, which then
    is what everything else of the result was computed from (the stage reads the dehazed frames when both are on).
    From a pipeline built with box_radar (None otherwise): box_points (B, cap) int32, the radar points inside each kept box,
    and box_radar (B, cap, 2, 5) float32, (depth, f0, f1, f2, f3) of the nearest of them and of their lower median by depth
    (`data.box_radar` is the rule), both zero from row kept[b] on; `radar_readout` brings them to the host.
    From a pipeline built with track (None otherwise): track_ids (B, cap) int32, the id of the track each row matched or
    started (0: none, and from row kept[b] on), track_table (B, T, 16) int32, the pipeline's own table of `data.TRACK_DTYPE`
    records as words, and track_head (B, 4) int32 (ids handed out, live tracks, calls, births of this call) -- the state after
    this run, which the next run updates in place; `tracks` brings them to the host.
    From a pipeline built with captions (None otherwise): captions (B * cap, 12) int32, the caption records of the kept rows,
    image b's from row `kept[:b].sum()` on (`render.caption_decode`); `caption_strings` brings them to the host.
    From a pipeline built with regions (None otherwise): region_labels (B, ih, iw) int32, the id of the connected region of
    every pixel of the class map (0: none; padded like class_map from a ragged pipeline), region_table (B, max_regions, 12)
    int32, the records of `decode.REGION_DTYPE` as words, region_head (B, 4) int32 (regions, records in the table, pixels in
    regions, pixels dropped by min_area) and box_regions (B, cap) int32, the region linked to each kept row (0: none, and from
    row kept[b] on) -- `decode.seg_regions_host` is the rule; `regions` brings them to the host."""
    __slots__ = ("rows", "kept", "det_counts", "class_map", "seg_counts", "rendered", "flag", "sizes", "heat_mask",
                 "heat_picture", "heat_range", "crops", "dehazed", "enhanced", "box_points", "box_radar", "track_ids",
                 "track_table", "track_head", "captions", "region_labels", "region_table", "region_head", "box_regions", "chips")

    def __init__(self, rows, kept, det_counts, class_map, seg_counts, rendered, flag, sizes=None, heat_mask=None,
                 heat_picture=None, heat_range=None, crops=None, dehazed=None, enhanced=None, box_points=None, box_radar=None,
                 track_ids=None, track_table=None, track_head=None, captions=None, region_labels=None, region_table=None,
                 region_head=None, box_regions=None, chips=None):
        self.chips = chips
        self.region_labels, self.region_table, self.region_head, self.box_regions = region_labels, region_table, region_head, box_regions
        self.track_ids, self.track_table, self.track_head, self.captions = track_ids, track_table, track_head, captions
        self.rows, self.kept, self.det_counts, self.class_map = rows, kept, det_counts, class_map
        self.seg_counts, self.rendered, self.flag, self.sizes = seg_counts, rendered, flag, sizes
        self.heat_mask, self.heat_picture, self.heat_range, self.crops = heat_mask, heat_picture, heat_range, crops
        self.dehazed, self.enhanced = dehazed, enhanced
        self.box_points, self.box_radar = box_points, box_radar

    def detections(self):
        """The list `decode.non_max_suppression` returns: per image an (N_b, 7) float32 numpy array in the same order,
        (0, 7) for an image without detections.  One device-to-host copy (rows and counts packed into one tensor), which
        waits for the frame."""
        B = self.kept.shape[0]
        packed = torch.cat([self.rows.reshape(-1), self.kept.view(torch.float32)]).cpu().numpy()
        kept = packed[-B:].view(np.int32)
        rows = packed[:-B].reshape(B, -1, 7)
        return [rows[b, :kept[b]].copy() for b in range(B)]

    def radar_readout(self):
        """The radar readout of a pipeline built with box_radar, beside `detections()` and in its row order: per image a
        (N_b, 11) float32 numpy array -- the points inside the box (a count, exact as a float32: at most 2^24), then depth, f0,
        f1, f2, f3 of the nearest point and the same five of the lower median by depth; (0, 11) for an image without
        detections.  One device-to-host copy (counts, readout and kept packed into one tensor), which waits for the frame."""
        if self.box_points is None or self.box_radar is None:
            raise RuntimeError("FrameResult.radar_readout: the pipeline was not built with box_radar")
        B, cap = self.box_points.shape
        packed = torch.cat([self.box_points.reshape(-1).view(torch.float32), self.box_radar.reshape(-1),
                            self.kept.view(torch.float32)]).cpu().numpy()
        counts = packed[:B * cap].view(np.int32).reshape(B, cap)
        readout = packed[B * cap:B * cap * 11].reshape(B, cap, 10)
        kept = packed[B * cap * 11:].view(np.int32)
        return [np.concatenate([counts[b, :kept[b], None].astype(np.float32), readout[b, :kept[b]]], axis=1) for b in range(B)]

    def tracks(self):
        """The tracks of a pipeline built with track, after this run: per stream a pair (the live records as a
        `data.TRACK_DTYPE` array in slot order, the track ids of the kept rows as an (N_b) int32 array in the order of
        `detections()`).  One device-to-host copy (table, ids and kept packed into one tensor), which waits for the frame."""
        if self.track_table is None or self.track_ids is None:
            raise RuntimeError("FrameResult.tracks: the pipeline was not built with track")
        B, T = self.track_table.shape[:2]
        cap = self.track_ids.shape[1]
        packed = torch.cat([self.track_table.reshape(-1), self.track_ids.reshape(-1), self.kept]).cpu().numpy()
        table = packed[:B * T * 16].view(data.TRACK_DTYPE).reshape(B, T)
        ids = packed[B * T * 16:B * T * 16 + B * cap].reshape(B, cap)
        kept = packed[B * T * 16 + B * cap:]
        return [(table[b][table[b]["id"] != 0].copy(), ids[b, :kept[b]].copy()) for b in range(B)]

    def regions(self):
        """The regions of a pipeline built with regions: per image a triple (the records as a `decode.REGION_DTYPE` array cut
        to their count, the (ih_b, iw_b) int32 label map cut to the image, the region ids of the kept rows as an (N_b) int32
        array in the order of `detections()`).  Two device-to-host copies: table, header, links and kept packed into one
        tensor, which waits for the frame, and the label maps."""
        if self.region_table is None or self.region_labels is None:
            raise RuntimeError("FrameResult.regions: the pipeline was not built with regions")
        from . import decode
        B, R = self.region_table.shape[:2]
        cap = self.box_regions.shape[1]
        packed = torch.cat([self.region_table.reshape(-1), self.region_head.reshape(-1), self.box_regions.reshape(-1),
                            self.kept]).cpu().numpy()
        table = packed[:B * R * 12].view(decode.REGION_DTYPE).reshape(B, R)
        head = packed[B * R * 12:B * R * 12 + 4 * B].reshape(B, 4)
        links = packed[B * R * 12 + 4 * B:B * R * 12 + 4 * B + B * cap].reshape(B, cap)
        kept = packed[B * R * 12 + 4 * B + B * cap:]
        labels = self.region_labels.cpu().numpy()
        sizes = [labels.shape[1:]] * B if self.sizes is None else [(int(h), int(w)) for h, w in self.sizes]
        return [(table[b, :head[b, 1]].copy(), labels[b, :sizes[b][0], :sizes[b][1]].copy(), links[b, :kept[b]].copy())
                for b in range(B)]

    def caption_strings(self):
        """The captions of a pipeline built with captions, as drawn: per image the list of its kept rows' strings, in the order
        of `detections()`.  One device-to-host copy (records and kept packed into one tensor), which waits for the frame."""
        if self.captions is None:
            raise RuntimeError("FrameResult.caption_strings: the pipeline was not built with captions")
        B = self.kept.shape[0]
        packed = torch.cat([self.captions.reshape(-1), self.kept]).cpu().numpy()
        ends = np.cumsum(packed[-B:])
        text = rendering.caption_decode(packed[:-B].reshape(-1, rendering.CAPTION_WORDS)[:ends[-1]])
        return [text[e - k:e] for e, k in zip(ends.tolist(), packed[-B:].tolist())]


class FramePipeline:
    """One object from raw frames to results: run(frames_u8, radar) -> FrameResult.

    model: an EfficientVRNet in eval mode on a HIP device.  frame_shape = (ih, iw) of the raw frames, input_shape = (H, W)
    of the network, batch = frames per call; all frames of a call share one size.  conf_thres / nms_thres /
    letterbox_image: as `decode.non_max_suppression` (with letterbox_image=False the frame is stretched to the input and
    the class map is the resize of the whole seg output).  max_candidates (1..render.MAX_BOXES): the fixed capacity of the
    captured NMS; the effective capacity is min(max_candidates, anchors).  An image with more candidates keeps its best-
    scored `cap` (score descending, anchor ascending) -- the result is then the prefix of `non_max_suppression`'s, and
    FLAG_CANDIDATES is set.  normalise_radar: False (the default) feeds the radar maps RAW, as deeplab.py and the training
    dataloader do; True min-max normalises every frame's maps on the device (`data.device_radar`), as yolo.py:134 does on
    the host.  radar_dtype: the type of the static radar buffer; float64 maps are normalised in float64, as the reference
    normalises a float64 .npz, only in a float64 buffer.  render / mix_type / alpha / seg_palette / box_palette: the
    `render.render_frame` picture (seg overlay, box outlines of thickness yolo.py:164) and the per-class pixel counts;
    default palettes `render.seg_palette(num_seg_classes)` and `render.det_palette(num_classes)`.  heatmap=True adds the
    detection heat map of yolo.py:288-351 (`render.heatmap` on the raw detection maps and the frames, jet blended at
    heat_alpha; aligned through the letterbox window when letterbox_image is set) to the chain and the result; with the
    default nothing about the chain, the result or the graph changes.

    graph=True warms the chain up (twice, on a side stream: workspaces and caches exist before the capture; the model's
    buffers are restored afterwards) and captures it as one hipGraph; run() then copies the inputs into the static
    buffers `frames_u8` (B, ih, iw, 3) / `radar` (B, 4, H, W) and replays.  graph=False runs the same calls eagerly, after one
    warm-up pass in the constructor (so `cap` and the buffers exist, and no run builds a cache).  Neither run synchronises
    with the host.

    ragged=True: frame_shape is the CAPACITY (ihm, iwm) and run(frames, radar, sizes=None) takes frames of their own sizes
    -- a list of B arrays, or a padded (B, ihp, iwp, 3) buffer plus sizes (B, 2).  Every size is validated on the host
    (inside the capacity, non-empty window, taps within max_taps: `data.default_max_taps`), each frame is copied into the
    corner of its slot of `frames_u8` and the geometry table into `geom`, all non_blocking, and the ONE graph is replayed:
    no recapture, no host synchronisation, no per-size cache.  The results are padded (see `FrameResult`).  The radar stays
    (B, 4, H, W).

    radar_points=max_points: run(frames, points, sizes=None, calib=None) takes radar POINTS where it took maps -- per image
    (n_b, 7) float32 rows x, y, z, f0, f1, f2, f3 with n_b <= max_points (`data.pack_points`) -- and calib, a (3, 4) or (B, 3, 4)
    projection from the radar's frame to continuous pixel coordinates of the original frame (here, or per call).
    vrnet_radar_map_f32, the first radar node of the chain, writes `radar` by the rule of `data.radar_map` under the window
    each frame goes through (its letterbox window, or the whole input with letterbox_image=False), radar_radius 0..8 the half
    width of a point's square footprint, radar_min_depth the nearest depth kept; normalise_radar still follows.  Fixed-size
    and ragged pipelines alike; the static inputs are then `points` (B, max_points, 7) and `views` (B, 80).  FLAG_POINT_COUNT
    (a count outside the buffer, which the host checks rule out) joins the bits of `flag`.

    labels: None (the default: the chain, the graph and every byte as before), a `render.LabelAtlas`, or True together with
    class_names= (one per detection class) and optionally font= (`render.LabelAtlas`: a TrueType path, a callable, or
    None = Pillow's built-in face) -- the tag and '<class name> <score:.2f>' of yolo.py:210-224 on every rendered box.  Two
    launches behind the render node: hip.label_index (the kept rows -> class * 101 + k) and the label renderer.  A fixed-size
    pipeline builds the one font size `render.label_font_size(ih)` (0, below 17 rows: no labels); a ragged one builds every
    size from 1 to label_font_size(ihm), or the sizes label_sizes= names, and sends the per-image size table up with the
    geometry table; a frame whose size was not built raises in the host validation of `run`, before anything is enqueued.
    FLAG_LABEL_SCORE joins the bits of `flag`.  labels needs render=True.

    crops: None (the default: the chain, the graph and the result as before), True or the capacity of the crop arena in
    pixels -- the `crop` switch of yolo.py:180-193: every kept detection is cut out of the ORIGINAL frame into a packed arena
    on the device (`render.crop_boxes`; fixed-size and ragged pipelines alike) and `FrameResult.crops` is its `render.Crops`.
    The arena, the table and the summary are allocated before the capture; the two launches of hip.crop_boxes sit right
    behind the detect_finish node.  True means 2 * batch * ihm * iwm pixels: a cap the caller may change, not a measured
    number -- 6 bytes per frame pixel, about 100 MB at batch 8 and 1080 x 1920.  Crops beyond the arena are dropped, a
    prefix is kept, and FLAG_CROP_ARENA joins the bits of `flag`.

    chips: None (the default: exactly the calls issued without it), a size (sh, sw) or a dict of size, letterbox and
    normalised -- every kept detection cut out of the ORIGINAL frame and brought to one size with Pillow's BICUBIC
    (`render.chip_boxes`, csrc/chips.hip; `render.chip_boxes_host` is the rule): one (batch * cap, sh, sw, 3) uint8 tensor of
    equal-sized pictures for a second stage, chip n of draw row n, and with normalised its (batch * cap, 3, sh, sw) float
    form; letterbox keeps the crop's aspect ratio on grey 128.  `FrameResult.chips` is its `render.Chips`.  Chips, table,
    summary and workspace are allocated with the NMS buffers, before the capture; the two launches of hip.chip_boxes sit
    directly behind the crop launches (behind the detect_finish node without crops), in front of hip.box_radar, and read the
    frames the crops read -- the dehazed or ACE frames when those stages are on.  Chips behind the last row are not written.
    Fixed-size and ragged pipelines alike; no new flag bit.

    dehaze: None (the default: exactly the calls issued without it), True or a dict of the keywords sz, r, eps, omega, tx of
    `render.dehaze_host` -- dark-channel-prior dehazing of the raw frames (`render.dehaze`, csrc/dehaze.hip) as the first
    stage: the eleven launches of hip.dehaze sit in front of the letterbox node, and the letterbox, `render_frame`, the heat
    map, the labels and the crops all read the dehazed frames, which are `FrameResult.dehazed`.  The workspace (seven
    float64 planes of batch * ihm * iwm, `hip.dehaze_workspace_bytes`) and the second frame buffer are allocated before the
    capture.  Fixed-size and ragged pipelines alike; a frame too small for the box (r // 2 > min(ih, iw) - 1) raises on the
    host, in the constructor or in the validation of `run`; an image without atmospheric light (a black one, or one below
    2000 pixels) goes on unchanged and FLAG_DEHAZE joins the bits of `flag`.

    ace: None (the default: exactly the calls issued without it), True or a dict of the keywords ratio, radius, s, bins of
    `render.ace_host` -- the fast Automatic Colour Equalisation of the reference's sharpen.py, its de-rain enhancement
    (`render.ace`, csrc/ace.hip): the launches of hip.ace sit in front of the letterbox node, behind those of hip.dehaze when
    both are on (ACE then reads the dehazed frames), and everything downstream reads its output, `FrameResult.enhanced`.  The
    buffer, the weights table and the workspace (`hip.ace_workspace_bytes`, about 40 bytes per frame pixel) are allocated
    before the capture.  Fixed-size and ragged pipelines alike; a degenerate image (min(ih, iw) <= 2, or a constant R_0)
    goes on unchanged and FLAG_ACE joins the bits of `flag`.

    box_radar: None (the default: exactly the calls issued without it) or True, in a pipeline built with radar_points -- the
    radar readout of every kept detection (`data.box_radar`, csrc/boxradar.hip): how many of the image's radar points lie in
    the box, and depth and features of the nearest of them and of their lower median by depth, as `FrameResult.box_points`
    and `FrameResult.box_radar`.  The two launches of hip.box_radar sit behind the detect_finish node (behind the crop
    launches when crops is on) and read the static `points` and `views` and the rows of the result, with radar_min_depth;
    box_shrink in (0, 1] scales every box about its centre first.  Outputs and workspace are allocated before the capture.
    Fixed-size and ragged pipelines alike, with and without letterbox_image: rows and projected points both live in the
    original frame.

    track: None (the default: exactly the calls issued without it), True or a dict of `data.check_track_params` (max_tracks,
    iou, max_age, gain, range_gain) -- multi-object tracking of the kept detections on the device (`data.track_update`,
    csrc/track.hip).  Every batch slot b becomes a STREAM: successive runs bring successive frames of camera b.  A table of
    max_tracks tracks per stream lives in device memory across the runs (and the replays of the graph); the one launch of
    hip.track_update behind hip.box_radar -- behind the crops or the finish node without it -- and in front of the seg node
    predicts, matches greedily by IoU within a class, filters box and rates, and with box_radar the range and its rate from
    the lower-median depth of the readout, coasts, frees and starts tracks, and writes `FrameResult.track_ids`.  Table, header
    and ids are allocated before the capture and zeroed after the warm-up, which runs the chain; `reset_tracks` zeroes them
    again.  Rates are per call: a stream must be fed at a constant frame rate.  Fixed-size and ragged pipelines alike.

    captions: None (the default: exactly the calls issued without it), True, a `render.GlyphAtlas`, or a dict of atlas, fps,
    font and sizes -- a second tag UNDER every rendered box, '#<track id> <range>m <closing speed>m/s' such as
    '#17 42.5m -1.2m/s' (`render.caption_strings` and `render.draw_captions_host` are the rule, csrc/captions.hip the
    kernels).  It needs render=True and at least one of track and box_radar: the id comes from the tracker, the range from the
    track's filtered range (with a tracker) or the lower-median depth of the readout (without one).  fps (default 0: no
    speed field) is the frame rate the streams are fed at, which turns the tracker's per-call range rate into metres per
    second; it needs track with box_radar.  font: as `render.GlyphAtlas` takes it.  A fixed-size pipeline builds the one font
    size `render.label_font_size(ih)` (0, below 17 rows: the text is composed, nothing is drawn); a ragged one builds every
    size from 1 to label_font_size(ihm), or those sizes= names, and a frame whose size was not built raises in the host
    validation of `run`, before anything is enqueued.  Two launches: hip.caption_text behind hip.track_update (behind
    hip.box_radar without a tracker) and hip.render_captions behind the label launches (behind the render node without
    labels); the records, `FrameResult.captions`, are allocated before the capture.  FLAG_CAPTION joins the bits of `flag`.

    regions: None (the default: exactly the calls issued without it), True or a dict of `decode.check_region_params`
    (connectivity, background, min_area, max_regions, det_to_seg -- one seg class per detection class of the model) -- the
    connected regions of the class map (`decode.seg_regions_host`, csrc/regions.hip): how many separate vessels or piers the
    class map holds, each one's class, area, bounding box and exact coordinate sums, and which kept row belongs to which of
    them, as `FrameResult.region_labels`, `region_table`, `region_head` and `box_regions`.  The seven launches of
    hip.seg_regions sit directly behind the seg node and in front of the render node and read the class map and the draw rows
    of the result.  Outputs and workspace (8 bytes per pixel of the batch) are allocated before the capture.  Fixed-size and
    ragged pipelines alike, with and without letterbox_image.  FLAG_REGIONS joins the bits of `flag`."""

    def __init__(self, model, frame_shape, input_shape, batch=1, conf_thres=0.5, nms_thres=0.4, letterbox_image=True,
                 max_candidates=1024, normalise_radar=False, render=True, mix_type=0, alpha=0.7, seg_palette=None,
                 box_palette=None, graph=True, radar_dtype=torch.float32, ragged=False, max_taps=None, heatmap=False,
                 heat_alpha=0.5, radar_points=None, radar_radius=0, radar_min_depth=0.1, calib=None, labels=None, class_names=None,
                 font=None, label_sizes=None, crops=None, dehaze=None, ace=None, box_radar=None, box_shrink=1.0, track=None,
                 captions=None, regions=None, chips=None):
        self.frame_shape, self.input_shape, self.batch, self.max_candidates = validate_config(
            model, frame_shape, input_shape, batch, max_candidates)
        self.chips = chip_config(chips)
        self.regions = None
        if regions is not None and regions is not False:
            from .decode import check_region_params
            self.regions = check_region_params(regions, "FramePipeline", num_classes=int(model.num_classes))
        self.track = None if track is None or track is False else data.check_track_params(track, "FramePipeline")
        self.crop_capacity = crop_capacity(crops, self.batch, self.frame_shape)
        self.dehaze = dehaze_config(dehaze)
        if self.dehaze is not None and not rendering.dehaze_size_ok(*self.frame_shape, self.dehaze["r"]):
            raise RuntimeError(f"FramePipeline: frames of {self.frame_shape[0]} x {self.frame_shape[1]} allow no single reflection "
                               f"of the dehazing box r = {self.dehaze['r']}")
        self.ace = ace_config(ace)
        self.radar_points = None
        if radar_points is not None:
            if radar_dtype != torch.float32:
                raise RuntimeError("FramePipeline: radar_points writes float32 maps; radar_dtype must be float32")
            self.radar_points = RadarPoints(radar_points, radar_radius, radar_min_depth, calib, self.batch)
        elif calib is not None or radar_radius != 0 or radar_min_depth != 0.1:
            raise RuntimeError("FramePipeline: calib, radar_radius and radar_min_depth belong to radar_points=max_points")
        self.box_radar = bool(box_radar)
        if self.box_radar:
            if self.radar_points is None:
                raise RuntimeError("FramePipeline: box_radar reads the radar POINTS of a pipeline built with radar_points=max_points; "
                                   "this one takes finished maps")
            self.box_shrink = float(data.check_box_shrink(box_shrink, "FramePipeline"))
        elif isinstance(box_shrink, bool) or box_shrink != 1.0:
            raise RuntimeError("FramePipeline: box_shrink belongs to box_radar=True")
        self.captions, self.caption_fps, self.caption_size_index = caption_config(
            captions, bool(render), self.track is not None, self.box_radar, bool(ragged), self.frame_shape[0])
        self.caption_size_tab = None
        if mix_type not in (0, 1, 2) or not 0.0 <= float(alpha) <= 1.0:
            raise RuntimeError(f"FramePipeline: mix_type must be 0, 1 or 2 and alpha in [0, 1], got {mix_type!r}, {alpha!r}")
        if not 0.0 <= float(heat_alpha) <= 1.0:
            raise RuntimeError(f"FramePipeline: heat_alpha must lie in [0, 1], got {heat_alpha!r}")
        self.heatmap, self.heat_alpha = bool(heatmap), float(heat_alpha)
        if radar_dtype not in (torch.float32, torch.float64) or (radar_dtype == torch.float64 and not normalise_radar):
            raise RuntimeError("FramePipeline: radar_dtype is float32, or float64 together with normalise_radar")
        self.model = model
        self.conf_thres, self.nms_thres, self.letterbox_image = float(conf_thres), float(nms_thres), bool(letterbox_image)
        self.normalise_radar, self.render, self.mix_type, self.alpha = bool(normalise_radar), bool(render), mix_type, float(alpha)
        p = next(model.parameters(), None)
        if p is None or not p.is_cuda:
            raise RuntimeError("FramePipeline: the model must be on a HIP device (there is no CPU fallback)")
        self.device = dev = p.device
        (ih, iw), (H, W), B = self.frame_shape, self.input_shape, self.batch
        self.num_classes = int(model.num_classes)
        pal = rendering.seg_palette(int(model.num_seg_classes)) if seg_palette is None else seg_palette
        bpal = rendering.det_palette(self.num_classes) if box_palette is None else box_palette
        self.seg_palette, self.box_palette = (t if torch.is_tensor(t) else torch.from_numpy(np.ascontiguousarray(t))
                                              for t in (pal, bpal))
        self.seg_palette, self.box_palette = self.seg_palette.to(dev), self.box_palette.to(dev)
        self.frames_u8 = torch.zeros((B, ih, iw, 3), dtype=torch.uint8, device=dev)
        self.radar = torch.zeros((B, 4, H, W), dtype=radar_dtype, device=dev)
        self.flag = torch.zeros(1, dtype=torch.int32, device=dev)
        self.ragged, self.sizes, self.label_size_tab = bool(ragged), None, None
        if self.ragged:                       # the warm-up and the capture run on a table of frames that fill their slots
            self.max_taps = data.default_max_taps(self.frame_shape, self.input_shape) if max_taps is None else int(max_taps)
            table = data.frame_geometry([self.frame_shape] * B, self.input_shape, self.letterbox_image, self.frame_shape,
                                        self.max_taps, "FramePipeline")
            self.geom = data.geometry_bytes(table).to(dev)
            # the table holds every image's shape, un-map scalars, thickness and window: the frame ops get the slots' capacity
            self.image_shape = self.offset = self.scale = self.thickness = None
            self._slots, self._heat_window = self.frame_shape, dict(window=self.letterbox_image)
        else:                                 # the same for all images: launch arguments of the frame ops
            self.image_shape, self._slots, self._heat_window = self.frame_shape, None, dict(letterbox_image=self.letterbox_image)
            self.thickness = int(max((iw + ih) // np.mean(self.input_shape), 1))                # yolo.py:164
            self.offset, self.scale = unmap_scalars(self.input_shape, self.frame_shape, self.letterbox_image)
        if self.radar_points is not None:     # the warm-up and the capture run on no points
            table = data.frame_geometry([self.frame_shape] * B, self.input_shape, self.letterbox_image, fn="FramePipeline")
            self.points, self.views = self.radar_points.buffers(table, dev)
            self._radar_ws = self.radar_points.workspace(self.input_shape, dev)
        self.labels = self._label_atlas(labels, class_names, font, label_sizes)
        if self.captions is not None and self.ragged:      # the warm-up and the capture run on frames that fill their slots
            size = rendering.label_font_size(ih)
            tab = np.full(B, self.captions.size_index(size) if size in self.captions.sizes else -1, np.int32)
            self.caption_size_tab = torch.from_numpy(tab).to(dev)
        if self.dehaze is not None:           # before the capture: the second frame buffer and the workspace
            from . import hip
            self._dehazed = torch.zeros_like(self.frames_u8)
            self._dehaze_ws = torch.empty(hip.dehaze_workspace_bytes(B, ih, iw), dtype=torch.uint8, device=dev)
        if self.ace is not None:              # before the capture: the stage's output, its weights table and its workspace
            from . import hip
            self._enhanced = torch.zeros_like(self.frames_u8)
            self._ace_weights = torch.from_numpy(rendering.ace_weights(self.ace["radius"])).to(dev)
            self._ace_ws = torch.empty(hip.ace_workspace_bytes(B, ih, iw), dtype=torch.uint8, device=dev)
        self.cap = None                       # the NMS buffers follow the anchor count of the first (warm-up) pass
        self.graph = self.result = None
        if graph:
            self._capture()
        else:
            self._warm_up(1)
        if self.track is not None:            # the warm-up and the capture ran the chain on zero input: back to the reset state
            self.reset_tracks()

    def _label_atlas(self, labels, class_names, font, label_sizes):
        """The atlas of the constructor's labels / class_names / font / label_sizes (None without labels), and the static
        size tables: `label_size_index` of a fixed-size pipeline (None: font size 0), `label_size_tab` (B) of a ragged one."""
        fn = "FramePipeline"
        if labels is None or labels is False:
            if class_names is not None or font is not None or label_sizes is not None:
                raise RuntimeError(f"{fn}: class_names, font and label_sizes belong to labels=")
            return None
        if not self.render:
            raise RuntimeError(f"{fn}: labels are drawn on the rendered frame; they need render=True")
        size = rendering.label_font_size(self.frame_shape[0])
        if labels is True:
            if class_names is None or len(class_names) != self.num_classes:
                raise RuntimeError(f"{fn}: labels=True needs class_names, one per detection class ({self.num_classes})")
            if label_sizes is None:
                label_sizes = tuple(range(1, size + 1)) if self.ragged else (size,)
            elif not self.ragged:
                raise RuntimeError(f"{fn}: label_sizes belongs to a ragged pipeline; a fixed-size one builds font size {size}")
            if not self.ragged and size == 0:
                atlas = None                  # frames lower than 17 rows: the outlines alone
            else:
                if not len(tuple(label_sizes)):
                    raise RuntimeError(f"{fn}: a capacity of {self.frame_shape[0]} rows has no font size >= 1 to build")
                atlas = rendering.LabelAtlas(class_names, font, label_sizes)
        elif isinstance(labels, rendering.LabelAtlas):
            if class_names is not None or font is not None or label_sizes is not None:
                raise RuntimeError(f"{fn}: class_names, font and label_sizes belong to labels=True; an atlas brings its own")
            atlas = labels
            if atlas.num_classes != self.num_classes:
                raise RuntimeError(f"{fn}: the atlas has {atlas.num_classes} classes, the model {self.num_classes}")
        else:
            raise RuntimeError(f"{fn}: labels is None, True or a render.LabelAtlas, got {type(labels).__name__}")
        if self.box_palette.shape[0] != self.num_classes:
            raise RuntimeError(f"{fn}: labels need a box palette of one colour per class ({self.num_classes}), got "
                               f"{self.box_palette.shape[0]}")
        if self.ragged:                       # the warm-up and the capture run on frames that fill their slots
            tab = np.full(self.batch, atlas.size_index(size) if size in atlas.sizes else -1, np.int32)
            self.label_size_tab = torch.from_numpy(tab).to(self.device)
        else:
            self.label_size_index = None if size == 0 else atlas.size_index(size)
            if self.label_size_index is None:
                return None
        return atlas

    def _allocate(self, anchors):
        from . import hip
        B, dev = self.batch, self.device
        self.cap = cap = min(self.max_candidates, anchors)
        i32 = dict(dtype=torch.int32, device=dev)
        self._cand = (torch.empty((B, anchors, 7), device=dev), torch.empty((B, anchors), device=dev),
                      torch.empty((B, anchors), dtype=torch.int64, device=dev), torch.empty((B, anchors), **i32),
                      torch.empty(B, **i32))                                    # rows, scores, classes, ids, counts
        self._nms_ws = torch.empty(hip.nms_workspace_bytes(B, cap), dtype=torch.uint8, device=dev)
        self._keep, self._kept = torch.empty((B, cap), **i32), torch.empty(B, **i32)
        self._kept_rows, self._rows = torch.empty((B, cap, 7), device=dev), torch.empty((B, cap, 7), device=dev)
        self._draw_rows, self._offsets = torch.empty((B * cap, 5), **i32), torch.empty(B + 1, **i32)
        self._det_counts = torch.empty((B, self.num_classes), dtype=torch.int64, device=dev)
        if self.labels is not None:
            self._label_idx = torch.zeros(B * cap, **i32)
        self._crops = None
        if self.crop_capacity is not None:
            self._crops = rendering.crop_buffers(B * cap, self.crop_capacity, B, self.flag, dev)
        self._chips = None
        if self.chips is not None:            # before the capture: chips, table, summary and the tap tables
            self._chips = rendering.chip_buffers(B * cap, self.chips["size"], B, self.chips["letterbox"],
                                                 self.chips["normalised"], self.flag, dev)
        self._box_points = self._box_radar = None
        if self.box_radar:                    # before the capture: the two outputs and the projected points
            self._box_points, self._box_radar = torch.zeros((B, cap), **i32), torch.zeros((B, cap, 2, 5), device=dev)
            self._box_ws = torch.empty(hip.box_radar_workspace_bytes(B, self.radar_points.max_points), dtype=torch.uint8, device=dev)
        self._track_table = self._track_head = self._track_ids = None
        if self.track is not None:            # before the capture: the state of every stream and the ids of the rows
            if cap > data.TRACK_MAX_ROWS:
                raise RuntimeError(f"FramePipeline: track takes at most {data.TRACK_MAX_ROWS} rows an image, max_candidates gives {cap}")
            self._track_table = torch.zeros((B, self.track["max_tracks"], hip.TRACK_WORDS), **i32)
            self._track_head, self._track_ids = torch.zeros((B, hip.TRACK_HEAD), **i32), torch.zeros((B, cap), **i32)
        self._captions = None
        if self.captions is not None:         # before the capture: one record per draw row
            self._captions = torch.zeros((B * cap, hip.CAPTION_WORDS), **i32)
        self._region_labels = self._region_table = self._region_head = self._box_regions = None
        if self.regions is not None:          # before the capture: the four outputs, the gate and the workspace
            ih, iw = self.frame_shape
            self._region_labels = torch.zeros((B, ih, iw), **i32)
            self._region_table = torch.zeros((B, self.regions["max_regions"], hip.REGION_WORDS), **i32)
            self._region_head, self._box_regions = torch.zeros((B, hip.REGION_HEAD), **i32), torch.zeros((B, cap), **i32)
            gate = self.regions["det_to_seg"]
            self._region_gate = None if gate is None else torch.tensor(gate, **i32)
            self._region_ws = torch.empty(hip.seg_regions_workspace_bytes(B, ih, iw), dtype=torch.uint8, device=dev)

    def _chain(self):
        """The chain of the module docstring.  A ragged pipeline reads the geometry of every image from `self.geom` on the
        device where a fixed one passes it in the launch arguments: every frame op takes either (`hip._table_call`), so the two
        chains are one but for the letterbox, which a fixed pipeline runs through `data.device_letterbox`, and for the
        stretched frame of a fixed pipeline without a letterbox, whose seg window is the whole input."""
        from . import decode, hip            # the library loads with the first pass, not with the package
        (H, W), F, B, dev = self.input_shape, self.frame_shape, self.batch, self.device
        geom = self.geom if self.ragged else None
        self.flag.zero_()                     # first: the ragged letterbox may raise FLAG_GEOMETRY
        frames = self.frames_u8
        if self.dehaze is not None:           # in front of the letterbox: everything below reads the dehazed frames
            frames = self._dehazed
            hip.dehaze(self.frames_u8, frames, self._dehaze_ws, geom=geom, flag=self.flag, **self.dehaze)
        dehazed = frames if self.dehaze is not None else None
        if self.ace is not None:              # behind the dehazing, in front of the letterbox
            hip.ace(frames, self._enhanced, self._ace_ws, self._ace_weights, geom=geom, flag=self.flag, **self.ace)
            frames = self._enhanced
        if self.ragged:
            images = torch.empty((B, 3, H, W), dtype=torch.float32, device=dev)
            hip.letterbox(frames, None, H, W, images=images, geom=geom, max_taps=self.max_taps, flag=self.flag)
        else:
            images, _ = data.device_letterbox(frames, (H, W), letterbox_image=self.letterbox_image, device=dev)
        if self.radar_points is not None:     # the first radar node: points -> self.radar under each frame's window
            hip.radar_map(self.points, self.views, H, W, self.radar_points.radius, float(self.radar_points.min_depth), self.radar,
                          flag=self.flag, ws=self._radar_ws)
        radar = data.device_radar(self.radar, True, dev) if self.normalise_radar else self.radar
        det, seg = self.model(images, radar)
        pred = decode.decode_outputs(det, (H, W))
        if self.cap is None:
            self._allocate(pred.shape[1])
        rows, scores, classes, ids, counts = self._cand
        hip.detect_select(pred, self.num_classes, self.conf_thres, rows, scores, classes, ids, counts)
        hip.nms_capped(rows, scores, classes, ids, counts, B, pred.shape[1], self.cap, self.nms_thres, self._nms_ws,
                       self._keep, self._kept, self._kept_rows, self.flag)
        hip.detect_finish(self._kept_rows, self._kept, self.num_classes, self.image_shape, self.offset, self.scale, self._rows,
                          self._draw_rows, self._offsets, self._det_counts, self.flag, geom=geom, capacity=self._slots)
        if self._crops is not None:           # right behind the finish node: from the original frames, which nothing draws on
            hip.crop_boxes(frames, self._draw_rows, self._offsets, self._crops.arena, self._crops.table,
                           self._crops.summary, geom=geom, flag=self.flag)
        if self._chips is not None:           # directly behind the crops: the same rows of the same frames, at one size
            hip.chip_boxes(frames, self._draw_rows, self._offsets, self._chips.chips, self._chips.table, self._chips.summary,
                           self._chips.workspace, letterbox=self._chips.letterbox, chips_f32=self._chips.chips_f32, geom=geom,
                           flag=self.flag)
        if self.box_radar:                    # behind the finish node (and the crops): rows and points share the original frame
            hip.box_radar(self.points, self.views, self._rows, self._kept, float(self.radar_points.min_depth), self.box_shrink,
                          self._box_points, self._box_radar, flag=self.flag, ws=self._box_ws)
        if self.track is not None:            # behind the readout, in front of the seg node: the state is updated in place
            hip.track_update(self._rows, self._kept, self._track_table, self._track_head, self._track_ids, self.track,
                             box_points=self._box_points, box_radar=self._box_radar, flag=self.flag)
        if self.captions is not None:         # behind the tracker (or the readout): the text of every kept row
            hip.caption_text(self._kept, self._offsets, self._captions, ids=self._track_ids, table=self._track_table,
                             box_points=self._box_points, box_radar=self._box_radar, rate_scale=self.caption_fps, flag=self.flag)
        if self.ragged or self.letterbox_image:
            class_map = decode.seg_predict(seg, (H, W), self.image_shape, geom=geom, capacity=self._slots, flag=self.flag)
        else:                                 # the frame was stretched over the whole input: the window is the input
            class_map = torch.empty((B,) + F, dtype=torch.uint8, device=dev)
            ws = torch.empty(hip.seg_predict_workspace_bytes(B, seg.shape[1], H, W), dtype=torch.uint8, device=dev)
            hip.seg_predict(seg.contiguous().float(), 0, 0, H, W, class_map, ws)
        if self.regions is not None:          # directly behind the seg node, in front of the render node
            hip.seg_regions(class_map, self._draw_rows, self._offsets, self._region_labels, self._region_table, self._region_head,
                            self._box_regions, self._region_ws, self.regions["connectivity"], self.regions["background"],
                            self.regions["min_area"], det_to_seg=self._region_gate, geom=geom, flag=self.flag)
        rendered = seg_counts = None
        if self.render:
            boxes = (self._draw_rows, self._offsets)
            if self.labels is not None:       # the two label launches sit behind the render node
                hip.label_index(self._rows, self._kept, self._offsets, self.num_classes, self._label_idx, self.flag)
                boxes += (self._label_idx,)
            rendered, seg_counts = rendering.render_frame(
                frames, class_map, boxes, palette=self.seg_palette, mix_type=self.mix_type, alpha=self.alpha, count=True,
                box_palette=self.box_palette, thickness=self.thickness, flag=self.flag, device=dev, labels=self.labels, geom=geom,
                label_sizes=self.label_size_tab)
            size = self.caption_size_tab if self.ragged else self.caption_size_index
            if self.captions is not None and size is not None:      # behind the label launches: a pass over the finished picture
                hip.render_captions(rendered, self._draw_rows, self._offsets, self.box_palette, self._captions,
                                    *self.captions.on(dev), size, flag=self.flag, geom=geom)
        result = FrameResult(self._rows, self._kept, self._det_counts, class_map, seg_counts, rendered, self.flag, crops=self._crops,
                             dehazed=dehazed, enhanced=frames if self.ace is not None else None, box_points=self._box_points,
                             box_radar=self._box_radar, track_ids=self._track_ids, track_table=self._track_table,
                             track_head=self._track_head, captions=self._captions, region_labels=self._region_labels,
                             region_table=self._region_table, region_head=self._region_head, box_regions=self._box_regions,
                             chips=self._chips)
        if self.heatmap:
            result.heat_picture, result.heat_mask, result.heat_range = rendering.heatmap(
                frames, det, (H, W), alpha=self.heat_alpha, geom=geom, flag=self.flag, **self._heat_window)
        self._tail(result)
        return result

    def _tail(self, result):
        """Called last in the chain, inside the capture: nothing here; a subclass appends device work on the result
        (evaluate.EvalPipeline)."""

    def _warm_up(self, passes, stream=None):
        """Runs the chain on the zeroed static buffers, on `stream` or the current one: the first pass sizes the NMS buffers
        from the anchor count (`cap`) and builds the caches with their host-to-device copies, so that no later run does."""
        dev = self.device
        saved = [(b, b.detach().clone()) for b in self.model.buffers() if b.numel()]
        cur = torch.cuda.current_stream(dev)
        stream = cur if stream is None else stream
        stream.wait_stream(cur)
        with torch.no_grad(), torch.cuda.stream(stream):
            for _ in range(passes):
                self._chain()
        cur.wait_stream(stream)
        torch.cuda.synchronize(dev)
        with torch.no_grad():
            for b, old in saved:                    # the warm-up's zero-input passes must leave the model as it was
                b.copy_(old)

    def _capture(self):
        self.stream = torch.cuda.Stream(self.device)    # warm-up AND capture run here: the scratch arenas of hip.Workspace are
        self._warm_up(2, self.stream)                   # keyed by stream, so they exist before the capture, in no graph pool
        self.graph = torch.cuda.CUDAGraph()
        from .graph import collector_held_off
        with collector_held_off(), torch.no_grad(), torch.cuda.graph(self.graph, stream=self.stream, capture_error_mode="thread_local"):
            self.result = self._chain()

    def reset_tracks(self, streams=None):
        """Zeroes the track state of the named streams (batch slots), or of all: table, header and ids, on the current
        stream, without a host synchronisation.  A stream that starts a new sequence is reset; ids start again at 1."""
        if self.track is None:
            raise RuntimeError("FramePipeline.reset_tracks: the pipeline was not built with track")
        if streams is None:
            streams = range(self.batch)
        streams = [int(b) for b in streams]
        if any(not 0 <= b < self.batch for b in streams):
            raise RuntimeError(f"FramePipeline.reset_tracks: streams are batch slots in [0, {self.batch}), got {streams}")
        with torch.cuda.device(self.device):
            for b in streams:
                self._track_table[b].zero_()
                self._track_head[b].zero_()
                self._track_ids[b].zero_()

    def run(self, frames_u8, radar, sizes=None, calib=None):
        """frames_u8 (B, ih, iw, 3) uint8 RGB and radar (B, 4, H, W) float32 / float64: numpy arrays or tensors, pageable,
        pinned or on the device -> FrameResult.  The inputs are copied into the static buffers (non_blocking), then the graph
        is replayed (graph=False: the chain is run); no host synchronisation.  A ragged pipeline takes frames_u8 as a list
        of B arrays of their own sizes, or as a padded buffer with sizes (B, 2) = (ih_b, iw_b); the result carries `sizes`.
        A pipeline built with radar_points takes radar POINTS where it took maps -- B arrays of (n_b, 7) float32 rows x, y, z,
        f0..f3, or a pair (padded array, counts), as `data.pack_points` takes them -- and calib, the (3, 4) or (B, 3, 4)
        projection of this call (default: the constructor's).  Points and the view table go up through fresh pinned staging
        tensors, and vrnet_radar_map_f32, inside the graph, writes `radar` under the window of each frame."""
        if calib is not None and self.radar_points is None:
            raise RuntimeError("FramePipeline: calib belongs to a pipeline built with radar_points")
        if not self.ragged:
            if sizes is not None:
                raise RuntimeError("FramePipeline: sizes belong to a ragged pipeline (ragged=True); this one is tied to frames of "
                                   f"{self.frame_shape[0]} x {self.frame_shape[1]}")
            f, r = validate_inputs(frames_u8, radar, self.batch, self.frame_shape, self.input_shape, self.radar_points, calib,
                                   self.letterbox_image)
            return self._launch(f, r)
        checked = validate_ragged_inputs(frames_u8, radar, sizes, self.batch, self.frame_shape, self.input_shape,
                                         self.letterbox_image, self.max_taps, self.radar_points, calib)
        if self.dehaze is not None:           # a frame too small for the box raises here, before anything is enqueued
            for b, (h, w) in enumerate(np.asarray(checked[2]).tolist()):
                if not rendering.dehaze_size_ok(h, w, self.dehaze["r"]):
                    raise RuntimeError(f"FramePipeline: image {b}: {h} x {w} allows no single reflection of the dehazing box "
                                       f"r = {self.dehaze['r']}")
        label_tab = None
        if self.labels is not None:           # a frame whose font size was not built raises here, before anything is enqueued
            label_tab = self.labels.size_table([int(s[0]) for s in checked[2]], "FramePipeline")
        caption_tab = None
        if self.captions is not None:         # the same for the glyph sizes
            caption_tab = self.captions.size_table([int(s[0]) for s in checked[2]], "FramePipeline")
        return self._launch(*checked, label_tab=label_tab, caption_tab=caption_tab)

    def _launch(self, f, r, sizes=None, table=None, label_tab=None, caption_tab=None):
        """The copies and the replay of `run`, on inputs that `validate_inputs` / `validate_ragged_inputs` returned."""
        with torch.cuda.device(self.device):
            if self.ragged:
                data.fill_slots(self.frames_u8, f, sizes)
                self.geom.copy_(data.geometry_bytes(table), non_blocking=True)
                if label_tab is not None:
                    self.label_size_tab.copy_(torch.from_numpy(label_tab).pin_memory(), non_blocking=True)
                if caption_tab is not None:
                    self.caption_size_tab.copy_(torch.from_numpy(caption_tab).pin_memory(), non_blocking=True)
                self.sizes = sizes
            else:
                self.frames_u8.copy_(f, non_blocking=True)
            if self.radar_points is not None:
                self.points.copy_(r[0], non_blocking=True)
                self.views.copy_(r[1].pin_memory(), non_blocking=True)
            else:
                self.radar.copy_(r, non_blocking=True)
            if self.graph is not None:
                self.graph.replay()
            else:
                with torch.no_grad():
                    self.result = self._chain()
        self.result.sizes = self.sizes
        return self.result


def radar_text(detections, readout):
    """The <stem>_radar.txt of `predict_dir` for one picture: detections (N, 7) as `FrameResult.detections` gives them and
    readout (N, 11) as `FrameResult.radar_readout` does -> one line per detection, space-separated: the class as an integer,
    the score obj * class_conf (the float32 product), left top right bottom, the points inside the box as an integer, then
    depth f0 f1 f2 f3 of the nearest point and of the lower median; every float as %.9g, which names a float32 exactly."""
    detections, readout = np.asarray(detections, np.float32), np.asarray(readout, np.float32)
    if detections.ndim != 2 or detections.shape[1] != 7 or readout.shape != (len(detections), 11):
        raise RuntimeError(f"radar_text: expected (N, 7) detections and (N, 11) readout rows, got {detections.shape} and {readout.shape}")
    lines = []
    for d, r in zip(detections, readout):
        top, left, bottom, right = d[:4]
        floats = [d[4] * d[5], left, top, right, bottom]
        lines.append(" ".join([str(int(d[6]))] + ["%.9g" % float(v) for v in floats] + [str(int(r[0]))] +
                              ["%.9g" % float(v) for v in r[1:]]) + "\n")
    return "".join(lines)


def predict_dir(pipeline, dir_origin_path, radar_root, dir_save_path=None):
    """predict.py's `dir_predict` mode on a ragged pipeline: every picture of the folder dir_origin_path whose name ends in
    one of IMAGE_EXTENSIONS (the reference's filter, lower case), in sorted order, with its radar maps
    radar_root/<frame id>.npz (`data.load_radar` by `data.frame_id` of the file name; for a pipeline built with radar_points
    `arr_0` of that file holds the image's (n, 7) point rows instead), in batches of pipeline.batch.  A
    final partial batch is filled by repeating the last picture; the repeats are dropped here.  Returns a list of
    (file name, (N, 7) detections) in that order; with dir_save_path the rendered frame of every picture, sliced to its own
    size, is saved there as <stem>.png through Pillow (the reference renames .jpg to .png; here every picture is a PNG), and
    from a pipeline with heatmap=True its heat picture as <stem>_heat.png beside it.  From a pipeline built with crops every
    non-empty crop the arena kept is saved as dir_save_path/img_crop/<stem>_crop_<i>.png, i being the row's index within its
    picture (the `i` of yolo.py:180-193); the crops of the repeated fill pictures are dropped with the repeats.  The reference
    writes img_crop/crop_<i>.png and so overwrites the crops of one picture with those of the next: the stem in the name is a
    deliberate departure.  From a pipeline built with chips every chip is saved as dir_save_path/img_chip/<stem>_chip_<i>.png,
    with the same i (the grey chip of an empty crop included, so that i stays the row's index).  From a pipeline built with
    dehaze the dehazed frame is saved as <stem>_dehaze.png, from one built
    with ace the enhanced frame as <stem>_ace.png, from one built with box_radar the radar readout of the picture's
    detections as <stem>_radar.txt (`radar_text`).  Two pictures that would share one output name (names that differ only in
    their extension, or `a_heat.jpg` next to `a.jpg` with heat maps on, or `a_dehaze.jpg` with dehazing on, or `a_ace.jpg`
    with ACE on, or `a_radar.jpg` with the readout on, or `a_tracks.jpg` with tracking on, or `a_regions.jpg` with regions
    on): with dir_save_path that raises before anything runs.  From a pipeline built with regions the records of the picture's
    connected regions are saved as <stem>_regions.txt (`decode.region_text`).  A pipeline built with track must have batch 1 -- the folder then is ONE sequence in its sorted
    order, fed to stream 0 of the pipeline as it stands (call `reset_tracks` first for a fresh sequence), and the live tracks
    after every picture are saved as <stem>_tracks.txt (`data.track_text`); with batch > 1 neighbouring files would land in
    different streams, which raises before anything runs."""
    from PIL import Image
    if not getattr(pipeline, "ragged", False):
        raise RuntimeError("predict_dir: needs a ragged pipeline (FramePipeline(..., ragged=True)): a folder holds pictures of any size")
    tracking = getattr(pipeline, "track", None) is not None
    if tracking and pipeline.batch != 1:
        raise RuntimeError(f"predict_dir: a tracking pipeline reads the folder as one sequence and needs batch 1, got batch "
                           f"{pipeline.batch}: neighbouring pictures would land in different streams")
    names = sorted(n for n in os.listdir(dir_origin_path) if n.lower().endswith(IMAGE_EXTENSIONS))
    if dir_save_path is not None:
        stems = {}
        for n in names:
            stem = os.path.splitext(n)[0]
            targets = (stem,) + ((stem + "_heat",) if getattr(pipeline, "heatmap", False) else ()) + \
                ((stem + "_dehaze",) if getattr(pipeline, "dehaze", None) is not None else ()) + \
                ((stem + "_ace",) if getattr(pipeline, "ace", None) is not None else ()) + \
                ((stem + "_radar",) if getattr(pipeline, "box_radar", False) else ()) + \
                ((stem + "_tracks",) if tracking else ()) + \
                ((stem + "_regions",) if getattr(pipeline, "regions", None) is not None else ())
            for target in targets:
                other = stems.setdefault(target, n)
                if other != n:
                    raise RuntimeError(f"predict_dir: {other} and {n} would both be saved as {target}.png")
    B, out = pipeline.batch, []
    if dir_save_path is not None:
        os.makedirs(dir_save_path, exist_ok=True)
    for k in range(0, len(names), B):
        chunk = names[k:k + B]
        frames = [np.array(Image.open(os.path.join(dir_origin_path, n)).convert("RGB"), dtype=np.uint8) for n in chunk]
        radar = [np.asarray(data.load_radar(radar_root, data.frame_id(n)), dtype=np.float32) for n in chunk]
        fill = B - len(chunk)
        if getattr(pipeline, "radar_points", None) is not None:        # arr_0 holds the (n, 7) point rows
            result = pipeline.run(frames + frames[-1:] * fill, radar + radar[-1:] * fill)
        else:
            result = pipeline.run(frames + frames[-1:] * fill, np.stack(radar + radar[-1:] * fill))
        dets = result.detections()
        rendered = None if dir_save_path is None or result.rendered is None else result.rendered.cpu().numpy()
        heat = None if dir_save_path is None else getattr(result, "heat_picture", None)
        heat = None if heat is None else heat.cpu().numpy()
        dehazed = None if dir_save_path is None else getattr(result, "dehazed", None)
        dehazed = None if dehazed is None else dehazed.cpu().numpy()
        enhanced = None if dir_save_path is None else getattr(result, "enhanced", None)
        enhanced = None if enhanced is None else enhanced.cpu().numpy()
        crops = None if dir_save_path is None else getattr(result, "crops", None)
        crops = None if crops is None else crops.images()
        chips = None if dir_save_path is None else getattr(result, "chips", None)
        chips = None if chips is None else chips.images()
        readout = None if dir_save_path is None or getattr(result, "box_radar", None) is None else result.radar_readout()
        tracks = None if dir_save_path is None or not tracking else result.tracks()
        regions = None if dir_save_path is None or getattr(result, "region_table", None) is None else result.regions()
        for b, n in enumerate(chunk):
            out.append((n, dets[b]))
            ih, iw = (int(v) for v in result.sizes[b])
            if tracks is not None:
                with open(os.path.join(dir_save_path, os.path.splitext(n)[0] + "_tracks.txt"), "w") as f:
                    f.write(data.track_text(tracks[b][0]))
            if regions is not None:
                from .decode import region_text
                with open(os.path.join(dir_save_path, os.path.splitext(n)[0] + "_regions.txt"), "w") as f:
                    f.write(region_text(regions[b][0]))
            if readout is not None:
                with open(os.path.join(dir_save_path, os.path.splitext(n)[0] + "_radar.txt"), "w") as f:
                    f.write(radar_text(dets[b], readout[b]))
            if rendered is not None:
                Image.fromarray(rendered[b, :ih, :iw]).save(os.path.join(dir_save_path, os.path.splitext(n)[0] + ".png"))
            if heat is not None:
                Image.fromarray(heat[b, :ih, :iw]).save(os.path.join(dir_save_path, os.path.splitext(n)[0] + "_heat.png"))
            if dehazed is not None:
                Image.fromarray(dehazed[b, :ih, :iw]).save(os.path.join(dir_save_path, os.path.splitext(n)[0] + "_dehaze.png"))
            if enhanced is not None:
                Image.fromarray(enhanced[b, :ih, :iw]).save(os.path.join(dir_save_path, os.path.splitext(n)[0] + "_ace.png"))
            for i, crop in enumerate(crops[b] if crops is not None else ()):
                if crop is not None and crop.size:
                    os.makedirs(os.path.join(dir_save_path, "img_crop"), exist_ok=True)
                    Image.fromarray(crop).save(os.path.join(dir_save_path, "img_crop", f"{os.path.splitext(n)[0]}_crop_{i}.png"))
            for i, chip in enumerate(chips[b] if chips is not None else ()):
                os.makedirs(os.path.join(dir_save_path, "img_chip"), exist_ok=True)
                Image.fromarray(chip).save(os.path.join(dir_save_path, "img_chip", f"{os.path.splitext(n)[0]}_chip_{i}.png"))
    return out
