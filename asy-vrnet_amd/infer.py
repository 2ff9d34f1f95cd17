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
table had to be clamped by a kernel, which the host checks of `run` rule out.  The optional stages add their own: FLAG_POINT_COUNT
(radar_points), FLAG_LABEL_SCORE, FLAG_CROP_ARENA, FLAG_DEHAZE, FLAG_ACE, FLAG_BOX_COUNT, FLAG_TRACK_FULL, FLAG_CAPTION and
FLAG_REGIONS and FLAG_JPEG_ARENA, each described with its stage.

Everything else a pipeline can do is an optional STAGE, one class of `stages.py` each, which holds the stage's keyword,
buffers, launches, result fields and documentation.  `stages.STAGES` is their order; a pipeline keeps those that are on, in
that order, as `stages`, and the chain calls them at five hook points, within a hook point in that order:

    frames      in front of the letterbox; each may replace the frames everything later reads     dehaze, ace
    rows        behind hip.detect_finish, in front of the seg node                                  crops, chips, box_radar, track,
                                                                                                    captions (hip.caption_text)
    class_map   behind the seg node, in front of the render node                                    regions, labels (hip.label_index;
                                                                                                    the render node draws them)
    picture     behind the render node, in front of `_tail`                                         captions (hip.render_captions),
                                                                                                    heatmap
    output      behind every picture, in front of `_tail`: what leaves the device in its final form  jpeg (`stages.OUTPUTS`,
                                                                                                    kept behind the ten)

ragged=True lifts the one-size limit: the pipeline is built for a CAPACITY (ihm, iwm), every frame of a call has its own
size inside it, and the per-image geometry travels in a small device table (`data.frame_geometry`) instead of the launch
arguments, so ONE captured graph serves any mix of sizes.  `predict_dir` is predict.py's `dir_predict` mode on top of it."""
import os
from types import SimpleNamespace

import numpy as np
import torch

from . import data
from . import render as rendering
from .stages import (OUTPUTS, STAGES, ace_config, caption_config, chip_config, crop_capacity, dehaze_config,    # noqa: F401
                     jpeg_config, radar_text)

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
FLAG_JPEG_ARENA = rendering.FLAG_JPEG_ARENA      # 262144, VR_FLAG_JPEG_ARENA of csrc/common.h (a pipeline built with jpeg): a file that did not fit
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
    The optional fields, each None unless its stage is on (the stage class of `stages.py` says the rest): dehazed and enhanced
    (B, ih, iw, 3) uint8, the frames everything else was computed from (`stages.Dehaze`, `stages.Ace`); crops, a
    `render.Crops` (`stages.Crops`); chips, a `render.Chips` (`stages.Chips`); box_points (B, cap) int32 and box_radar (B, cap,
    2, 5) float32 (`stages.BoxRadar`; `radar_readout`); track_ids (B, cap), track_table (B, T, 16) and track_head (B, 4) int32
    (`stages.Track`; `tracks`); captions (B * cap, 12) int32 (`stages.Captions`; `caption_strings`); region_labels (B, ih, iw),
    region_table (B, max_regions, 12), region_head (B, 4) and box_regions (B, cap) int32 (`stages.Regions`; `regions`);
    heat_mask (B, ih, iw) uint8, heat_picture (B, ih, iw, 3) uint8 and heat_range (B, 2) int32 (`stages.Heatmap`); jpeg, a
    `render.Jpegs` (`stages.Jpeg`, the one entry of `stages.OUTPUTS`).  The constructor takes them as keywords."""
    CORE = ("rows", "kept", "det_counts", "class_map", "seg_counts", "rendered", "flag", "sizes")
    __slots__ = CORE + tuple(f for stage in STAGES + OUTPUTS for f in stage.fields)

    def __init__(self, rows, kept, det_counts, class_map, seg_counts, rendered, flag, sizes=None, **fields):
        self.rows, self.kept, self.det_counts, self.class_map = rows, kept, det_counts, class_map
        self.seg_counts, self.rendered, self.flag, self.sizes = seg_counts, rendered, flag, sizes
        for name in self.__slots__[len(self.CORE):]:
            setattr(self, name, fields.pop(name, None))
        if fields:
            raise TypeError(f"FrameResult: no such fields: {', '.join(sorted(fields))}")

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
    default palettes `render.seg_palette(num_seg_classes)` and `render.det_palette(num_classes)`.

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

    The optional stages, each documented on its class of `stages.py`, in launch order: dehaze= (`stages.Dehaze`), ace=
    (`Ace`), crops= (`Crops`), chips= (`Chips`), box_radar= / box_shrink= (`BoxRadar`), track= (`Track`), captions=
    (`Captions`), regions= (`Regions`), labels= / class_names= / font= / label_sizes= (`Labels`), heatmap= / heat_alpha=
    (`Heatmap`), and behind them the outputs of `stages.OUTPUTS`: jpeg= (`Jpeg`).  With its default a stage changes nothing
    about the chain, the graph or the result.  `stages` holds those
    that are on; the attribute of each keyword's name holds its checked parameters (`crop_capacity` for crops=)."""

    def __init__(self, model, frame_shape, input_shape, batch=1, conf_thres=0.5, nms_thres=0.4, letterbox_image=True,
                 max_candidates=1024, normalise_radar=False, render=True, mix_type=0, alpha=0.7, seg_palette=None,
                 box_palette=None, graph=True, radar_dtype=torch.float32, ragged=False, max_taps=None, heatmap=False,
                 heat_alpha=0.5, radar_points=None, radar_radius=0, radar_min_depth=0.1, calib=None, labels=None, class_names=None,
                 font=None, label_sizes=None, crops=None, dehaze=None, ace=None, box_radar=None, box_shrink=1.0, track=None,
                 captions=None, regions=None, chips=None, jpeg=None):
        self.frame_shape, self.input_shape, self.batch, self.max_candidates = validate_config(
            model, frame_shape, input_shape, batch, max_candidates)
        self.model, self.render, self.ragged = model, bool(render), bool(ragged)
        self.radar_points = None
        if radar_points is not None:
            if radar_dtype != torch.float32:
                raise RuntimeError("FramePipeline: radar_points writes float32 maps; radar_dtype must be float32")
            self.radar_points = RadarPoints(radar_points, radar_radius, radar_min_depth, calib, self.batch)
        elif calib is not None or radar_radius != 0 or radar_min_depth != 0.1:
            raise RuntimeError("FramePipeline: calib, radar_radius and radar_min_depth belong to radar_points=max_points")
        kw = dict(dehaze=dehaze, ace=ace, crops=crops, chips=chips, box_radar=box_radar, box_shrink=box_shrink, track=track,
                  captions=captions, regions=regions, labels=labels, class_names=class_names, font=font, label_sizes=label_sizes,
                  heatmap=heatmap, heat_alpha=heat_alpha, jpeg=jpeg)
        self.stages = self._parse(kw, early=True)         # the keyword checks that need no device
        outputs = [s for s in (cls.parse(self, kw) for cls in OUTPUTS) if s is not None]
        if mix_type not in (0, 1, 2) or not 0.0 <= float(alpha) <= 1.0:
            raise RuntimeError(f"FramePipeline: mix_type must be 0, 1 or 2 and alpha in [0, 1], got {mix_type!r}, {alpha!r}")
        if radar_dtype not in (torch.float32, torch.float64) or (radar_dtype == torch.float64 and not normalise_radar):
            raise RuntimeError("FramePipeline: radar_dtype is float32, or float64 together with normalise_radar")
        self.conf_thres, self.nms_thres, self.letterbox_image = float(conf_thres), float(nms_thres), bool(letterbox_image)
        self.normalise_radar, self.mix_type, self.alpha = bool(normalise_radar), mix_type, float(alpha)
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
        self.sizes = None
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
        self.stages = sorted(self.stages + self._parse(kw, early=False), key=lambda s: STAGES.index(type(s))) + outputs
        from . import hip
        for s in self.stages:                 # before the capture: what follows from the frame shape alone
            s.static(self, hip)
        self.cap = None                       # the NMS buffers follow the anchor count of the first (warm-up) pass
        self.graph = self.result = None
        if graph:
            self._capture()
        else:
            self._warm_up(1)
        for s in self.stages:                 # the warm-up and the capture ran the chain on zero input
            s.ready(self)

    def _parse(self, kw, early):
        """The stages of STAGES whose keyword checks run in front of (early) or behind the device check, those that are on."""
        found = [cls.parse(self, kw) for cls in STAGES if cls.early == early]
        return [s for s in found if s is not None]

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
        for s in self.stages:                 # before the capture: what the stages keep per row
            s.allocate(self, hip, cap)

    def _at(self, point, c):
        """The launches of the stages at one hook point of the chain, in the order of STAGES."""
        for s in self.stages:
            getattr(s, point)(self, c)

    def _chain(self):
        """The chain of the module docstring.  A ragged pipeline reads the geometry of every image from `self.geom` on the
        device where a fixed one passes it in the launch arguments: every frame op takes either (`hip._table_call`), so the two
        chains are one but for the letterbox, which a fixed pipeline runs through `data.device_letterbox`, and for the
        stretched frame of a fixed pipeline without a letterbox, whose seg window is the whole input.  c is the context the
        stages' hooks read and write (`stages.Stage`)."""
        from . import decode, hip            # the library loads with the first pass, not with the package
        (H, W), F, B, dev = self.input_shape, self.frame_shape, self.batch, self.device
        c = SimpleNamespace(hip=hip, geom=self.geom if self.ragged else None, frames=self.frames_u8, out={}, labels=None,
                            label_sizes=None, rendered=None)
        self.flag.zero_()                     # first: the ragged letterbox may raise FLAG_GEOMETRY
        self._at("frames", c)
        if self.ragged:
            images = torch.empty((B, 3, H, W), dtype=torch.float32, device=dev)
            hip.letterbox(c.frames, None, H, W, images=images, geom=c.geom, max_taps=self.max_taps, flag=self.flag)
        else:
            images, _ = data.device_letterbox(c.frames, (H, W), letterbox_image=self.letterbox_image, device=dev)
        if self.radar_points is not None:     # the first radar node: points -> self.radar under each frame's window
            hip.radar_map(self.points, self.views, H, W, self.radar_points.radius, float(self.radar_points.min_depth), self.radar,
                          flag=self.flag, ws=self._radar_ws)
        radar = data.device_radar(self.radar, True, dev) if self.normalise_radar else self.radar
        c.det, seg = self.model(images, radar)
        pred = decode.decode_outputs(c.det, (H, W))
        if self.cap is None:
            self._allocate(pred.shape[1])
        rows, scores, classes, ids, counts = self._cand
        hip.detect_select(pred, self.num_classes, self.conf_thres, rows, scores, classes, ids, counts)
        hip.nms_capped(rows, scores, classes, ids, counts, B, pred.shape[1], self.cap, self.nms_thres, self._nms_ws,
                       self._keep, self._kept, self._kept_rows, self.flag)
        hip.detect_finish(self._kept_rows, self._kept, self.num_classes, self.image_shape, self.offset, self.scale, self._rows,
                          self._draw_rows, self._offsets, self._det_counts, self.flag, geom=c.geom, capacity=self._slots)
        self._at("rows", c)
        if self.ragged or self.letterbox_image:
            c.class_map = decode.seg_predict(seg, (H, W), self.image_shape, geom=c.geom, capacity=self._slots, flag=self.flag)
        else:                                 # the frame was stretched over the whole input: the window is the input
            c.class_map = torch.empty((B,) + F, dtype=torch.uint8, device=dev)
            ws = torch.empty(hip.seg_predict_workspace_bytes(B, seg.shape[1], H, W), dtype=torch.uint8, device=dev)
            hip.seg_predict(seg.contiguous().float(), 0, 0, H, W, c.class_map, ws)
        c.boxes = (self._draw_rows, self._offsets)
        self._at("class_map", c)
        seg_counts = None
        if self.render:
            c.rendered, seg_counts = rendering.render_frame(
                c.frames, c.class_map, c.boxes, palette=self.seg_palette, mix_type=self.mix_type, alpha=self.alpha, count=True,
                box_palette=self.box_palette, thickness=self.thickness, flag=self.flag, device=dev, labels=c.labels, geom=c.geom,
                label_sizes=c.label_sizes)
        self._at("picture", c)
        self._at("output", c)
        result = FrameResult(self._rows, self._kept, self._det_counts, c.class_map, seg_counts, c.rendered, self.flag, **c.out)
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
        # a frame a stage cannot take raises here, before anything is enqueued; the stages' per-image tables follow the geometry
        tables = [pair for s in self.stages for pair in s.check(self, checked[2])]
        return self._launch(*checked, tables=tables)

    def _launch(self, f, r, sizes=None, table=None, tables=()):
        """The copies and the replay of `run`, on inputs that `validate_inputs` / `validate_ragged_inputs` returned; tables: the
        (device table, host array) pairs of the stages' `check`."""
        with torch.cuda.device(self.device):
            if self.ragged:
                data.fill_slots(self.frames_u8, f, sizes)
                self.geom.copy_(data.geometry_bytes(table), non_blocking=True)
                for dst, host in tables:
                    dst.copy_(torch.from_numpy(host).pin_memory(), non_blocking=True)
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


def predict_dir(pipeline, dir_origin_path, radar_root, dir_save_path=None):
    """predict.py's `dir_predict` mode on a ragged pipeline: every picture of the folder dir_origin_path whose name ends in
    one of IMAGE_EXTENSIONS (the reference's filter, lower case), in sorted order, with its radar maps
    radar_root/<frame id>.npz (`data.load_radar` by `data.frame_id` of the file name; for a pipeline built with radar_points
    `arr_0` of that file holds the image's (n, 7) point rows instead), in batches of pipeline.batch.  A
    final partial batch is filled by repeating the last picture; the repeats are dropped here.  Returns a list of
    (file name, (N, 7) detections) in that order; with dir_save_path the rendered frame of every picture, sliced to its own
    size, is saved there as <stem>.png through Pillow (the reference renames .jpg to .png; here every picture is a PNG), and
    every stage of the pipeline saves its own beside it -- <stem>_heat.png, <stem>_dehaze.png, <stem>_ace.png,
    <stem>_radar.txt, <stem>_tracks.txt, <stem>_regions.txt, img_crop/<stem>_crop_<i>.png, img_chip/<stem>_chip_<i>.png, and
    <stem>.jpg, the device-encoded file of a pipeline built with jpeg=, written as it is, without Pillow: see
    the stage classes of `stages.py`; what belongs to the repeated fill pictures is dropped with the repeats.  Each stage
    reads its part of a batch back once, and nothing is read back without dir_save_path.  Two pictures that would share one
    output name (names that differ only in their extension, or `a_heat.jpg` next to `a.jpg` with heat maps on, and so for
    every suffix a stage claims): with dir_save_path that raises before anything runs.  A pipeline built with track must
    have batch 1 (`stages.Track`), which raises before anything runs too.  A pipeline without `stages` has none."""
    from PIL import Image
    if not getattr(pipeline, "ragged", False):
        raise RuntimeError("predict_dir: needs a ragged pipeline (FramePipeline(..., ragged=True)): a folder holds pictures of any size")
    stages = getattr(pipeline, "stages", ())
    for s in stages:
        s.folder(pipeline)
    names = sorted(n for n in os.listdir(dir_origin_path) if n.lower().endswith(IMAGE_EXTENSIONS))
    if dir_save_path is not None:
        owner = {}
        for n in names:
            stem = os.path.splitext(n)[0]
            for target in [stem] + [stem + suffix for s in stages for suffix in s.claims]:
                other = owner.setdefault(target, n)
                if other != n:
                    raise RuntimeError(f"predict_dir: {other} and {n} would both be saved as {target}.png")
        os.makedirs(dir_save_path, exist_ok=True)
    B, out = pipeline.batch, []
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
        out.extend(zip(chunk, dets))
        if dir_save_path is None:
            continue
        rendered = None if result.rendered is None else result.rendered.cpu().numpy()
        host = [(s, s.read(result)) for s in stages]
        for b, n in enumerate(chunk):
            stem, (ih, iw) = os.path.splitext(n)[0], (int(v) for v in result.sizes[b])
            if rendered is not None:
                Image.fromarray(rendered[b, :ih, :iw]).save(os.path.join(dir_save_path, stem + ".png"))
            for s, part in host:
                if part is not None:
                    s.save(part, b, stem, (ih, iw), dets[b], dir_save_path)
    return out
