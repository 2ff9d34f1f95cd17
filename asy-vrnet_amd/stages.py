"""The optional stages of `infer.FramePipeline`, one class each, and STAGES, their launch order.  A class holds everything
its feature needs of the pipeline: the keyword and its checks, the buffers, the launches, the result fields, the ragged
per-call check and its part of `infer.predict_dir`; its docstring is the feature's documentation.  `FramePipeline` parses
STAGES in order, keeps the stages that are on as `pipeline.stages` and calls their hooks where `infer`'s docstring says.
OUTPUTS, at the end of the file, holds the stages that turn a finished picture into what leaves the device (`Jpeg`): they are
parsed behind STAGES, kept behind them in `pipeline.stages` and run at the `output` hook point."""
import os

import numpy as np
import torch

from . import data
from . import render as rendering

FN = "FramePipeline"


def _off(keyword):
    return keyword is None or keyword is False


def _write(dst, name, text):
    with open(os.path.join(dst, name), "w") as f:
        f.write(text)


def _save(dst, name, picture):
    from PIL import Image
    os.makedirs(os.path.dirname(os.path.join(dst, name)), exist_ok=True)
    Image.fromarray(picture).save(os.path.join(dst, name))


class Stage:
    """What a stage may define; every hook but `parse` defaults to nothing.  p is the pipeline, hip the loaded `hip` module.
    parse(p, kw): the constructor's keywords kw, checked on the host -> the stage, or None for "off"; it sets the pipeline
    attributes callers read (`p.dehaze`, `p.chips`, ...) either way.  Stages are parsed in the order of STAGES, in front of
    the "must be on a HIP device" check; `early = False` moves a stage's parse behind it, where the palettes exist.
    static(p, hip): the buffers that follow from the frame shape alone; allocate(p, hip, cap): those that need `cap`.  Both
    run before the capture.  ready(p): after the warm-up and the capture, which ran the chain on zero input.
    frames / rows / class_map / picture / output (p, c): the launches at that hook point of the chain.  c is the context of one pass:
    hip, geom (the geometry table of a ragged pipeline, or None), frames (what everything later reads: a stage may replace
    it), det, class_map, boxes / labels / label_sizes (arguments of the render node), rendered, and out, the dict of the
    optional result fields -- a stage writes those it names in `fields` and may read those of the stages in front of it.
    check(p, sizes): the host check of one ragged call, which raises before anything is enqueued -> (device table, int32
    host array) pairs that `_launch` sends up with the geometry table.
    For `predict_dir`: claims, the suffixes of the output names <stem><suffix>.* the stage writes beside <stem>.png, which
    must not collide; folder(p): what it demands of the pipeline before anything runs; read(result): its ONE read-back of a
    batch -> host data; save(host, b, stem, size, det, dst): what it saves for picture b of (ih, iw) = size and detections
    det.  `saved` names a (B, ih, iw, 3) field that is read and saved as <stem><claims[0]>.png, cut to the picture."""
    name, fields, claims, saved, early = None, (), (), None, True

    @classmethod
    def parse(cls, p, kw):
        raise NotImplementedError

    def static(self, p, hip): pass
    def allocate(self, p, hip, cap): pass
    def ready(self, p): pass
    def frames(self, p, c): pass
    def rows(self, p, c): pass
    def class_map(self, p, c): pass
    def picture(self, p, c): pass
    def output(self, p, c): pass
    def folder(self, p): pass

    def check(self, p, sizes):
        return ()

    def read(self, result):
        return None if self.saved is None else getattr(result, self.saved).cpu().numpy()

    def save(self, host, b, stem, size, det, dst):
        if self.saved is not None:
            _save(dst, stem + self.claims[0] + ".png", host[b, :size[0], :size[1]])


def dehaze_config(dehaze):
    """The parameters of a pipeline's dehazing stage from its dehaze= keyword: None (no stage), True (the defaults of
    `render.dehaze_host`) or a dict of its keywords sz, r, eps, omega, tx; checked by `render.dehaze_params`."""
    if _off(dehaze):
        return None
    if dehaze is True:
        dehaze = {}
    if not isinstance(dehaze, dict) or set(dehaze) - {"sz", "r", "eps", "omega", "tx"}:
        raise RuntimeError(f"{FN}: dehaze is None, True or a dict of sz, r, eps, omega, tx, got {dehaze!r}")
    return rendering.dehaze_params(fn=FN, **dehaze)


class Dehaze(Stage):
    """dehaze: None (the default: exactly the calls issued without it), True or a dict of the keywords sz, r, eps, omega, tx of
    `render.dehaze_host` -- dark-channel-prior dehazing of the raw frames (`render.dehaze`, csrc/dehaze.hip) as the first
    stage: the eleven launches of hip.dehaze sit in front of the letterbox node, and the letterbox, `render_frame`, the heat
    map, the labels and the crops all read the dehazed frames, which are `FrameResult.dehazed` (B, ih, iw, 3) uint8, padded
    like rendered from a ragged pipeline.  The workspace (seven float64 planes of batch * ihm * iwm,
    `hip.dehaze_workspace_bytes`) and the second frame buffer are allocated before the capture.  Fixed-size and ragged
    pipelines alike; a frame too small for the box (r // 2 > min(ih, iw) - 1) raises on the host, in the constructor or in
    the validation of `run`; an image without atmospheric light (a black one, or one below 2000 pixels) goes on unchanged
    and FLAG_DEHAZE joins the bits of `flag`.  `predict_dir` saves the dehazed frame as <stem>_dehaze.png."""
    name, fields, claims, saved = "dehaze", ("dehazed",), ("_dehaze",), "dehazed"

    @classmethod
    def parse(cls, p, kw):
        p.dehaze = dehaze_config(kw["dehaze"])
        if p.dehaze is None:
            return None
        if not rendering.dehaze_size_ok(*p.frame_shape, p.dehaze["r"]):
            raise RuntimeError(f"{FN}: frames of {p.frame_shape[0]} x {p.frame_shape[1]} allow no single reflection of the "
                               f"dehazing box r = {p.dehaze['r']}")
        return cls()

    def static(self, p, hip):
        self.out = torch.zeros_like(p.frames_u8)
        self.ws = torch.empty(hip.dehaze_workspace_bytes(p.batch, *p.frame_shape), dtype=torch.uint8, device=p.device)

    def frames(self, p, c):
        c.hip.dehaze(c.frames, self.out, self.ws, geom=c.geom, flag=p.flag, **p.dehaze)
        c.frames = c.out["dehazed"] = self.out

    def check(self, p, sizes):
        for b, (h, w) in enumerate(np.asarray(sizes).tolist()):
            if not rendering.dehaze_size_ok(h, w, p.dehaze["r"]):
                raise RuntimeError(f"{FN}: image {b}: {h} x {w} allows no single reflection of the dehazing box r = {p.dehaze['r']}")
        return ()


def ace_config(ace):
    """The parameters of a pipeline's ACE stage from its ace= keyword: None (no stage), True (the defaults of
    `render.ace_host`) or a dict of its keywords ratio, radius, s, bins; checked by `render.ace_params`."""
    if _off(ace):
        return None
    if ace is True:
        ace = {}
    if not isinstance(ace, dict) or set(ace) - {"ratio", "radius", "s", "bins"}:
        raise RuntimeError(f"{FN}: ace is None, True or a dict of ratio, radius, s, bins, got {ace!r}")
    return rendering.ace_params(fn=FN, **ace)


class Ace(Stage):
    """ace: None (the default: exactly the calls issued without it), True or a dict of the keywords ratio, radius, s, bins of
    `render.ace_host` -- the fast Automatic Colour Equalisation of the reference's sharpen.py, its de-rain enhancement
    (`render.ace`, csrc/ace.hip): the launches of hip.ace sit in front of the letterbox node, behind those of hip.dehaze when
    both are on (ACE then reads the dehazed frames), and everything downstream reads its output, `FrameResult.enhanced` (B,
    ih, iw, 3) uint8.  The buffer, the weights table and the workspace (`hip.ace_workspace_bytes`, about 40 bytes per frame
    pixel) are allocated before the capture.  Fixed-size and ragged pipelines alike; a degenerate image (min(ih, iw) <= 2,
    or a constant R_0) goes on unchanged and FLAG_ACE joins the bits of `flag`.  `predict_dir` saves <stem>_ace.png."""
    name, fields, claims, saved = "ace", ("enhanced",), ("_ace",), "enhanced"

    @classmethod
    def parse(cls, p, kw):
        p.ace = ace_config(kw["ace"])
        return None if p.ace is None else cls()

    def static(self, p, hip):
        self.out = torch.zeros_like(p.frames_u8)
        self.weights = torch.from_numpy(rendering.ace_weights(p.ace["radius"])).to(p.device)
        self.ws = torch.empty(hip.ace_workspace_bytes(p.batch, *p.frame_shape), dtype=torch.uint8, device=p.device)

    def frames(self, p, c):
        c.hip.ace(c.frames, self.out, self.ws, self.weights, geom=c.geom, flag=p.flag, **p.ace)
        c.frames = c.out["enhanced"] = self.out


def crop_capacity(crops, batch, frame_shape):
    """The pixels of a pipeline's crop arena from its crops= keyword: None (no crops), True (2 * batch * ihm * iwm, at most
    2^30) or the number itself, 1..2^30."""
    if _off(crops):
        return None
    if crops is True:
        return min(2 * int(batch) * int(frame_shape[0]) * int(frame_shape[1]), 1 << 30)
    if not isinstance(crops, (int, np.integer)) or not 1 <= int(crops) <= 1 << 30:
        raise RuntimeError(f"{FN}: crops is None, True or the capacity of the crop arena, 1..2^30 pixels, got {crops!r}")
    return int(crops)


class Crops(Stage):
    """crops: None (the default: the chain, the graph and the result as before), True or the capacity of the crop arena in
    pixels -- the `crop` switch of yolo.py:180-193: every kept detection is cut out of the ORIGINAL frame into a packed arena
    on the device (`render.crop_boxes`; fixed-size and ragged pipelines alike) and `FrameResult.crops` is its `render.Crops`,
    `crops.images()[b][i]` being row i of image b.  The arena, the table and the summary are allocated before the capture;
    the two launches of hip.crop_boxes sit right behind the detect_finish node and read the frames the letterbox read, which
    nothing draws on.  True means 2 * batch * ihm * iwm pixels: a cap the caller may change, not a measured number -- 6 bytes
    per frame pixel, about 100 MB at batch 8 and 1080 x 1920.  Crops beyond the arena are dropped, a prefix is kept, and
    FLAG_CROP_ARENA joins the bits of `flag`.  `predict_dir` saves every non-empty crop the arena kept as
    img_crop/<stem>_crop_<i>.png, i being the row's index within its picture (the `i` of yolo.py:180-193).  The reference
    writes img_crop/crop_<i>.png and so overwrites the crops of one picture with those of the next: the stem in the name is a
    deliberate departure."""
    name, fields = "crops", ("crops",)

    @classmethod
    def parse(cls, p, kw):
        p.crop_capacity = crop_capacity(kw["crops"], p.batch, p.frame_shape)
        return None if p.crop_capacity is None else cls()

    def allocate(self, p, hip, cap):
        self.buffers = rendering.crop_buffers(p.batch * cap, p.crop_capacity, p.batch, p.flag, p.device)

    def rows(self, p, c):
        b = c.out["crops"] = self.buffers
        c.hip.crop_boxes(c.frames, p._draw_rows, p._offsets, b.arena, b.table, b.summary, geom=c.geom, flag=p.flag)

    def read(self, result):
        return result.crops.images()

    def save(self, host, b, stem, size, det, dst):
        for i, crop in enumerate(host[b]):
            if crop is not None and crop.size:
                _save(dst, os.path.join("img_crop", f"{stem}_crop_{i}.png"), crop)


def chip_config(chips):
    """The fixed-size chips of a pipeline from its chips= keyword: None (no chips), a size (sh, sw), or a dict of size,
    letterbox and normalised.  Returns None or a dict of all three, the size checked (sides in 1..render.CHIP_MAX)."""
    if _off(chips):
        return None
    cfg = dict(chips) if isinstance(chips, dict) else {"size": chips}
    if "size" not in cfg or set(cfg) - {"size", "letterbox", "normalised"}:
        raise RuntimeError(f"{FN}: chips is None, a size (sh, sw) or a dict of size, letterbox, normalised, got {chips!r}")
    return dict(size=rendering._chip_size(cfg["size"], f"{FN}: chips"), letterbox=bool(cfg.get("letterbox", False)),
                normalised=bool(cfg.get("normalised", False)))


class Chips(Stage):
    """chips: None (the default: exactly the calls issued without it), a size (sh, sw) or a dict of size, letterbox and
    normalised -- every kept detection cut out of the ORIGINAL frame and brought to one size with Pillow's BICUBIC
    (`render.chip_boxes`, csrc/chips.hip; `render.chip_boxes_host` is the rule): one (batch * cap, sh, sw, 3) uint8 tensor of
    equal-sized pictures for a second stage, chip n of draw row n, and with normalised its (batch * cap, 3, sh, sw) float
    form; letterbox keeps the crop's aspect ratio on grey 128.  `FrameResult.chips` is its `render.Chips`: `chips.chips[n]`
    (and `chips.chips_f32[n]`) is draw row n and `chips.images()[b][i]` row i of image b.  Chips, table, summary and
    workspace are allocated with the NMS buffers, before the capture; the two launches of hip.chip_boxes sit directly behind
    the crop launches, in front of hip.box_radar, and read the frames the crops read -- the dehazed or ACE frames when those
    stages are on.  Chips behind the last row are not written.  Fixed-size and ragged pipelines alike; no new flag bit.
    `predict_dir` saves every chip as img_chip/<stem>_chip_<i>.png, with the i of the crops (the grey chip of an empty crop
    included, so that i stays the row's index)."""
    name, fields = "chips", ("chips",)

    @classmethod
    def parse(cls, p, kw):
        p.chips = chip_config(kw["chips"])
        return None if p.chips is None else cls()

    def allocate(self, p, hip, cap):
        self.buffers = rendering.chip_buffers(p.batch * cap, p.chips["size"], p.batch, p.chips["letterbox"],
                                              p.chips["normalised"], p.flag, p.device)

    def rows(self, p, c):
        b = c.out["chips"] = self.buffers
        c.hip.chip_boxes(c.frames, p._draw_rows, p._offsets, b.chips, b.table, b.summary, b.workspace, letterbox=b.letterbox,
                         chips_f32=b.chips_f32, geom=c.geom, flag=p.flag)

    def read(self, result):
        return result.chips.images()

    def save(self, host, b, stem, size, det, dst):
        for i, chip in enumerate(host[b]):
            _save(dst, os.path.join("img_chip", f"{stem}_chip_{i}.png"), chip)


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


class BoxRadar(Stage):
    """box_radar: None (the default: exactly the calls issued without it) or True, in a pipeline built with radar_points --
    the radar readout of every kept detection (`data.box_radar`, csrc/boxradar.hip): `FrameResult.box_points` (B, cap) int32,
    the radar points inside each kept box, and `FrameResult.box_radar` (B, cap, 2, 5) float32, (depth, f0, f1, f2, f3) of the
    nearest of them and of their lower median by depth, both zero from row kept[b] on; `radar_readout` brings them to the
    host.  The two launches of hip.box_radar sit behind the chips and read the static `points` and `views` and the rows of
    the result, with radar_min_depth; box_shrink in (0, 1] scales every box about its centre first.  Outputs and workspace
    are allocated before the capture.  Fixed-size and ragged pipelines alike, with and without letterbox_image: rows and
    projected points both live in the original frame.  FLAG_BOX_COUNT, a kept count outside the row buffer, is ruled out by
    the NMS that writes it.  `predict_dir` saves the readout of a picture's detections as <stem>_radar.txt (`radar_text`)."""
    name, fields, claims = "box_radar", ("box_points", "box_radar"), ("_radar",)

    @classmethod
    def parse(cls, p, kw):
        p.box_radar, shrink = bool(kw["box_radar"]), kw["box_shrink"]
        if not p.box_radar:
            if isinstance(shrink, bool) or shrink != 1.0:
                raise RuntimeError(f"{FN}: box_shrink belongs to box_radar=True")
            return None
        if p.radar_points is None:
            raise RuntimeError(f"{FN}: box_radar reads the radar POINTS of a pipeline built with radar_points=max_points; "
                               "this one takes finished maps")
        p.box_shrink = float(data.check_box_shrink(shrink, FN))
        return cls()

    def allocate(self, p, hip, cap):
        self.points = torch.zeros((p.batch, cap), dtype=torch.int32, device=p.device)
        self.readout = torch.zeros((p.batch, cap, 2, 5), device=p.device)
        self.ws = torch.empty(hip.box_radar_workspace_bytes(p.batch, p.radar_points.max_points), dtype=torch.uint8, device=p.device)

    def rows(self, p, c):
        c.hip.box_radar(p.points, p.views, p._rows, p._kept, float(p.radar_points.min_depth), p.box_shrink, self.points,
                        self.readout, flag=p.flag, ws=self.ws)
        c.out.update(box_points=self.points, box_radar=self.readout)

    def read(self, result):
        return result.radar_readout()

    def save(self, host, b, stem, size, det, dst):
        _write(dst, stem + "_radar.txt", radar_text(det, host[b]))


class Track(Stage):
    """track: None (the default: exactly the calls issued without it), True or a dict of `data.check_track_params` (max_tracks,
    iou, max_age, gain, range_gain) -- multi-object tracking of the kept detections on the device (`data.track_update`,
    csrc/track.hip).  Every batch slot b becomes a STREAM: successive runs bring successive frames of camera b.  A table of
    max_tracks tracks per stream lives in device memory across the runs (and the replays of the graph); the one launch of
    hip.track_update behind the readout and in front of the seg node predicts, matches greedily by IoU within a class,
    filters box and rates, and with box_radar the range and its rate from the lower-median depth of the readout, coasts,
    frees and starts tracks.  `FrameResult.track_ids` (B, cap) int32 is the id of the track each row matched or started (0:
    none, and from row kept[b] on), `track_table` (B, T, 16) int32 the pipeline's own table of `data.TRACK_DTYPE` records as
    words and `track_head` (B, 4) int32 (ids handed out, live tracks, calls, births of this call) -- the state after this run,
    which the next run updates in place; `tracks` brings them to the host.  Table, header and ids (`_track_table`,
    `_track_head`, `_track_ids` of the pipeline) are allocated before the capture and zeroed after the warm-up, which runs
    the chain; `reset_tracks` zeroes them again.  Rates are per call: a stream must be fed at a constant frame rate.
    Fixed-size and ragged pipelines alike; FLAG_TRACK_FULL says that a valid row found no free slot and got track id 0.
    `predict_dir` needs batch 1 -- the folder then is ONE sequence in its sorted order, fed to stream 0 of the pipeline as
    it stands (call `reset_tracks` first for a fresh sequence), and the live tracks after every picture are saved as
    <stem>_tracks.txt (`data.track_text`); with batch > 1 neighbouring files would land in different streams."""
    name, fields, claims = "track", ("track_ids", "track_table", "track_head"), ("_tracks",)

    @classmethod
    def parse(cls, p, kw):
        p.track = None if _off(kw["track"]) else data.check_track_params(kw["track"], FN)
        return None if p.track is None else cls()

    def allocate(self, p, hip, cap):
        if cap > data.TRACK_MAX_ROWS:
            raise RuntimeError(f"{FN}: track takes at most {data.TRACK_MAX_ROWS} rows an image, max_candidates gives {cap}")
        i32 = dict(dtype=torch.int32, device=p.device)
        p._track_table = torch.zeros((p.batch, p.track["max_tracks"], hip.TRACK_WORDS), **i32)
        p._track_head, p._track_ids = torch.zeros((p.batch, hip.TRACK_HEAD), **i32), torch.zeros((p.batch, cap), **i32)

    def rows(self, p, c):
        c.hip.track_update(p._rows, p._kept, p._track_table, p._track_head, p._track_ids, p.track,
                           box_points=c.out.get("box_points"), box_radar=c.out.get("box_radar"), flag=p.flag)
        c.out.update(track_ids=p._track_ids, track_table=p._track_table, track_head=p._track_head)

    def ready(self, p):
        p.reset_tracks()

    def folder(self, p):
        if p.batch != 1:
            raise RuntimeError(f"predict_dir: a tracking pipeline reads the folder as one sequence and needs batch 1, got batch "
                               f"{p.batch}: neighbouring pictures would land in different streams")

    def read(self, result):
        return result.tracks()

    def save(self, host, b, stem, size, det, dst):
        _write(dst, stem + "_tracks.txt", data.track_text(host[b][0]))


def caption_config(captions, render, track, box_radar, ragged, ih):
    """The captions= keyword of a pipeline, checked on the host: None (no captions), True, a `render.GlyphAtlas` or a dict of
    atlas, fps, font, sizes -> (composing, fps, size index); composing is the atlas, or True where a fixed-size pipeline of
    frames lower than 17 rows composes the text and draws nothing; the size index is that of a fixed-size pipeline's one
    font size (None: nothing is drawn, or a ragged pipeline, whose table follows each call).  Names what is missing."""
    fn = FN
    if _off(captions):
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


class Captions(Stage):
    """captions: None (the default: exactly the calls issued without it), True, a `render.GlyphAtlas`, or a dict of atlas, fps,
    font and sizes -- a second tag UNDER every rendered box, '#<track id> <range>m <closing speed>m/s' such as
    '#17 42.5m -1.2m/s' (`render.caption_strings` and `render.draw_captions_host` are the rule, csrc/captions.hip the
    kernels).  It needs render=True and at least one of track and box_radar: the id comes from the tracker, the range from the
    track's filtered range (with a tracker) or the lower-median depth of the readout (without one).  fps (default 0: no
    speed field) is the frame rate the streams are fed at, which turns the tracker's per-call range rate into metres per
    second; it needs track with box_radar.  font: as `render.GlyphAtlas` takes it.  A fixed-size pipeline builds the one font
    size `render.label_font_size(ih)` (0, below 17 rows: the text is composed, nothing is drawn); a ragged one builds every
    size from 1 to label_font_size(ihm), or those sizes= names, and a frame whose size was not built raises in the host
    validation of `run`, before anything is enqueued.  Two launches: hip.caption_text at the rows point, behind the tracker,
    and hip.render_captions at the picture point, a pass over the finished picture behind the render node and its labels.
    `FrameResult.captions` (B * cap, 12) int32, allocated before the capture, holds the caption records of the kept rows,
    image b's from row `kept[:b].sum()` on (`render.caption_decode`); `caption_strings` brings them to the host.
    FLAG_CAPTION says that a range or a speed could not be drawn and was left out."""
    name, fields = "captions", ("captions",)

    @classmethod
    def parse(cls, p, kw):
        p.captions, p.caption_fps, index = caption_config(kw["captions"], p.render, p.track is not None, p.box_radar, p.ragged,
                                                          p.frame_shape[0])
        return None if p.captions is None else cls(index)

    def __init__(self, index):
        self.size = index                     # the size index of a fixed-size pipeline, the (B) size table of a ragged one

    def static(self, p, hip):
        if p.ragged:                          # the warm-up and the capture run on frames that fill their slots
            size = rendering.label_font_size(p.frame_shape[0])
            tab = np.full(p.batch, p.captions.size_index(size) if size in p.captions.sizes else -1, np.int32)
            self.size = torch.from_numpy(tab).to(p.device)

    def allocate(self, p, hip, cap):
        self.records = torch.zeros((p.batch * cap, hip.CAPTION_WORDS), dtype=torch.int32, device=p.device)

    def rows(self, p, c):
        c.hip.caption_text(p._kept, p._offsets, self.records, ids=c.out.get("track_ids"), table=c.out.get("track_table"),
                           box_points=c.out.get("box_points"), box_radar=c.out.get("box_radar"), rate_scale=p.caption_fps,
                           flag=p.flag)
        c.out["captions"] = self.records

    def picture(self, p, c):
        if self.size is not None:
            c.hip.render_captions(c.rendered, p._draw_rows, p._offsets, p.box_palette, self.records, *p.captions.on(p.device),
                                  self.size, flag=p.flag, geom=c.geom)

    def check(self, p, sizes):
        return [(self.size, p.captions.size_table([int(s[0]) for s in sizes], FN))]


class Regions(Stage):
    """regions: None (the default: exactly the calls issued without it), True or a dict of `decode.check_region_params`
    (connectivity, background, min_area, max_regions, det_to_seg -- one seg class per detection class of the model) -- the
    connected regions of the class map (`decode.seg_regions_host` is the rule, csrc/regions.hip): how many separate vessels
    or piers the class map holds, each one's class, area, bounding box and exact coordinate sums, and which kept row belongs
    to which of them.  `FrameResult.region_labels` (B, ih, iw) int32 is the id of the connected region of every pixel of the
    class map (0: none; padded like class_map from a ragged pipeline), `region_table` (B, max_regions, 12) int32 the records
    of `decode.REGION_DTYPE` as words, `region_head` (B, 4) int32 (regions, records in the table, pixels in regions, pixels
    dropped by min_area) and `box_regions` (B, cap) int32 the region linked to each kept row (0: none, and from row kept[b]
    on); `regions` brings them to the host.  The seven launches of hip.seg_regions sit directly behind the seg node and in
    front of the render node and read the class map and the draw rows of the result.  Outputs and workspace (8 bytes per
    pixel of the batch) are allocated before the capture.  Fixed-size and ragged pipelines alike, with and without
    letterbox_image.  FLAG_REGIONS says that an image had more regions than the table holds.  `predict_dir` saves the
    records of a picture's regions as <stem>_regions.txt (`decode.region_text`)."""
    name, fields, claims = "regions", ("region_labels", "region_table", "region_head", "box_regions"), ("_regions",)

    @classmethod
    def parse(cls, p, kw):
        p.regions = None
        if not _off(kw["regions"]):
            from .decode import check_region_params
            p.regions = check_region_params(kw["regions"], FN, num_classes=int(p.model.num_classes))
        return None if p.regions is None else cls()

    def allocate(self, p, hip, cap):
        B, (ih, iw), i32 = p.batch, p.frame_shape, dict(dtype=torch.int32, device=p.device)
        self.labels = torch.zeros((B, ih, iw), **i32)
        self.table = torch.zeros((B, p.regions["max_regions"], hip.REGION_WORDS), **i32)
        self.head, self.links = torch.zeros((B, hip.REGION_HEAD), **i32), torch.zeros((B, cap), **i32)
        gate = p.regions["det_to_seg"]
        self.gate = None if gate is None else torch.tensor(gate, **i32)
        self.ws = torch.empty(hip.seg_regions_workspace_bytes(B, ih, iw), dtype=torch.uint8, device=p.device)

    def class_map(self, p, c):
        c.hip.seg_regions(c.class_map, p._draw_rows, p._offsets, self.labels, self.table, self.head, self.links, self.ws,
                          p.regions["connectivity"], p.regions["background"], p.regions["min_area"], det_to_seg=self.gate,
                          geom=c.geom, flag=p.flag)
        c.out.update(region_labels=self.labels, region_table=self.table, region_head=self.head, box_regions=self.links)

    def read(self, result):
        return result.regions()

    def save(self, host, b, stem, size, det, dst):
        from .decode import region_text
        _write(dst, stem + "_regions.txt", region_text(host[b][0]))


class Labels(Stage):
    """labels: None (the default: the chain, the graph and every byte as before), a `render.LabelAtlas`, or True together with
    class_names= (one per detection class) and optionally font= (`render.LabelAtlas`: a TrueType path, a callable, or
    None = Pillow's built-in face) -- the tag and '<class name> <score:.2f>' of yolo.py:210-224 on every rendered box.  The
    stage owns hip.label_index (the kept rows -> class * 101 + k), the last launch in front of the render node, and hands
    its index, the atlas and the size table to `render.render_frame`, whose label renderer draws them behind the outlines.
    A fixed-size pipeline builds the one font size `render.label_font_size(ih)` (0, below 17 rows: no labels, the stage is
    off); a ragged one builds every size from 1 to label_font_size(ihm), or the sizes label_sizes= names, and sends the
    per-image size table `label_size_tab` up with the geometry table; a frame whose size was not built raises in the host
    validation of `run`, before anything is enqueued.  FLAG_LABEL_SCORE joins the bits of `flag`.  labels needs render=True
    and a box palette of one colour per class, so its checks run behind the device check (`early = False`)."""
    name, early = "labels", False

    @classmethod
    def parse(cls, p, kw):
        labels, class_names, font, label_sizes = (kw[k] for k in ("labels", "class_names", "font", "label_sizes"))
        p.labels = p.label_size_tab = None
        if _off(labels):
            if class_names is not None or font is not None or label_sizes is not None:
                raise RuntimeError(f"{FN}: class_names, font and label_sizes belong to labels=")
            return None
        if not p.render:
            raise RuntimeError(f"{FN}: labels are drawn on the rendered frame; they need render=True")
        size = rendering.label_font_size(p.frame_shape[0])
        if labels is True:
            if class_names is None or len(class_names) != p.num_classes:
                raise RuntimeError(f"{FN}: labels=True needs class_names, one per detection class ({p.num_classes})")
            if label_sizes is None:
                label_sizes = tuple(range(1, size + 1)) if p.ragged else (size,)
            elif not p.ragged:
                raise RuntimeError(f"{FN}: label_sizes belongs to a ragged pipeline; a fixed-size one builds font size {size}")
            if not p.ragged and size == 0:
                atlas = None                  # frames lower than 17 rows: the outlines alone
            else:
                if not len(tuple(label_sizes)):
                    raise RuntimeError(f"{FN}: a capacity of {p.frame_shape[0]} rows has no font size >= 1 to build")
                atlas = rendering.LabelAtlas(class_names, font, label_sizes)
        elif isinstance(labels, rendering.LabelAtlas):
            if class_names is not None or font is not None or label_sizes is not None:
                raise RuntimeError(f"{FN}: class_names, font and label_sizes belong to labels=True; an atlas brings its own")
            atlas = labels
            if atlas.num_classes != p.num_classes:
                raise RuntimeError(f"{FN}: the atlas has {atlas.num_classes} classes, the model {p.num_classes}")
        else:
            raise RuntimeError(f"{FN}: labels is None, True or a render.LabelAtlas, got {type(labels).__name__}")
        if p.box_palette.shape[0] != p.num_classes:
            raise RuntimeError(f"{FN}: labels need a box palette of one colour per class ({p.num_classes}), got "
                               f"{p.box_palette.shape[0]}")
        if p.ragged:                          # the warm-up and the capture run on frames that fill their slots
            tab = np.full(p.batch, atlas.size_index(size) if size in atlas.sizes else -1, np.int32)
            p.label_size_tab = torch.from_numpy(tab).to(p.device)
        else:
            p.label_size_index = None if size == 0 else atlas.size_index(size)
            if p.label_size_index is None:
                return None
        p.labels = atlas
        return cls()

    def allocate(self, p, hip, cap):
        p._label_idx = torch.zeros(p.batch * cap, dtype=torch.int32, device=p.device)

    def class_map(self, p, c):
        c.hip.label_index(p._rows, p._kept, p._offsets, p.num_classes, p._label_idx, p.flag)
        c.boxes, c.labels, c.label_sizes = c.boxes + (p._label_idx,), p.labels, p.label_size_tab

    def check(self, p, sizes):
        return [(p.label_size_tab, p.labels.size_table([int(s[0]) for s in sizes], FN))]


class Heatmap(Stage):
    """heatmap=True adds the detection heat map of yolo.py:288-351 (`render.heatmap` on the raw detection maps and the frames,
    jet blended at heat_alpha; aligned through the letterbox window when letterbox_image is set) as the last launches of the
    chain; with the default nothing about the chain, the result or the graph changes.  `FrameResult.heat_mask` (B, ih, iw)
    uint8, `heat_picture` (B, ih, iw, 3) uint8 and `heat_range` (B, 2) int32 = each mask's (min, max) are what
    `render.heatmap` returns for the frames and the raw detection maps of the run; padded like class_map / rendered from a
    ragged pipeline.  `predict_dir` saves the heat picture as <stem>_heat.png."""
    name, fields, claims, saved = "heatmap", ("heat_mask", "heat_picture", "heat_range"), ("_heat",), "heat_picture"

    @classmethod
    def parse(cls, p, kw):
        if not 0.0 <= float(kw["heat_alpha"]) <= 1.0:
            raise RuntimeError(f"{FN}: heat_alpha must lie in [0, 1], got {kw['heat_alpha']!r}")
        p.heatmap, p.heat_alpha = bool(kw["heatmap"]), float(kw["heat_alpha"])
        return cls() if p.heatmap else None

    def picture(self, p, c):
        c.out["heat_picture"], c.out["heat_mask"], c.out["heat_range"] = rendering.heatmap(
            c.frames, c.det, p.input_shape, alpha=p.heat_alpha, geom=c.geom, flag=p.flag, **p._heat_window)


# the launch order: within a hook point of the chain the stages run in this order (the table of infer's docstring)
STAGES = (Dehaze, Ace, Crops, Chips, BoxRadar, Track, Captions, Regions, Labels, Heatmap)


def jpeg_config(jpeg, render):
    """The encoder of a pipeline from its jpeg= keyword: None (no files), True (quality 95, 4:4:4, the rendered frame, the
    default capacity) or a dict of quality, subsampling, source and capacity.  Returns None or a dict of all four, checked:
    source is "rendered" (it needs render=True) or "frames"."""
    if _off(jpeg):
        return None
    cfg = {} if jpeg is True else jpeg
    if not isinstance(cfg, dict) or set(cfg) - {"quality", "subsampling", "source", "capacity"}:
        raise RuntimeError(f"{FN}: jpeg is None, True or a dict of quality, subsampling, source, capacity, got {jpeg!r}")
    quality, subsampling = rendering._jpeg_params(cfg.get("quality", 95), cfg.get("subsampling", 0), f"{FN}: jpeg")
    source, capacity = cfg.get("source", "rendered"), cfg.get("capacity")
    if source not in ("rendered", "frames"):
        raise RuntimeError(f"{FN}: jpeg: source is 'rendered' or 'frames', got {source!r}")
    if source == "rendered" and not render:
        raise RuntimeError(f"{FN}: jpeg: source='rendered' encodes the rendered frame; it needs render=True (or source='frames')")
    if capacity is not None and (isinstance(capacity, bool) or not isinstance(capacity, (int, np.integer)) or
                                 not rendering.JPEG_HEADER + 2 <= int(capacity) < (1 << 31) - 64):
        raise RuntimeError(f"{FN}: jpeg: capacity is the bytes of one slot of the arena, {rendering.JPEG_HEADER + 2}..2^31 - 65, "
                           f"got {capacity!r}")
    return dict(quality=quality, subsampling=subsampling, source=source, capacity=None if capacity is None else int(capacity))


class Jpeg(Stage):
    """jpeg: None (the default: exactly the calls issued without it), True or a dict of quality (95), subsampling (0: 4:4:4, or
    2: 4:2:0), source and capacity -- every picture of the batch leaves the device as a finished baseline JPEG file
    (`render.jpeg_encode`, csrc/jpeg.hip; `render.jpeg_encode_host` is the rule: the bytes Pillow's `save(format="JPEG",
    quality=, subsampling=)` writes).  source: "rendered" (the default; it needs render=True) or "frames", what the renderer
    reads -- the dehazed or enhanced frame when those stages are on.  `FrameResult.jpeg` is its `render.Jpegs`:
    `jpeg.bytes()[b]` is the file of picture b, of its own size from a ragged pipeline (SOF0 carries (ih_b, iw_b) of the
    geometry table).  Arena, record, header template and workspace are allocated before the capture; the eight launches of
    hip.jpeg_encode are the last of the chain, at the `output` hook point behind `picture`.  capacity: the bytes of a slot
    of the arena, default `render.jpeg_capacity(ih, iw)` = 623 + 3 ih iw; a file that does not fit gets length 0 and
    FLAG_JPEG_ARENA joins the bits of `flag`.  Not an entry of STAGES, whose ten names are pinned: an OUTPUT, parsed from
    OUTPUTS and kept behind the ten in `pipeline.stages`.  `predict_dir` writes <stem>.jpg straight from the bytes, beside
    <stem>.png."""
    name, fields = "jpeg", ("jpeg",)

    @classmethod
    def parse(cls, p, kw):
        p.jpeg = jpeg_config(kw["jpeg"], p.render)
        if p.jpeg is None:
            return None
        rendering.jpeg_shape(*p.frame_shape, p.jpeg["subsampling"], f"{FN}: jpeg")
        return cls()

    def static(self, p, hip):
        self.buffers = rendering.jpeg_buffers(p.batch, *p.frame_shape, p.jpeg["quality"], p.jpeg["subsampling"],
                                              p.jpeg["capacity"], p.flag, p.device, f"{FN}: jpeg")

    def output(self, p, c):
        b = c.out["jpeg"] = self.buffers
        c.hip.jpeg_encode(c.rendered if p.jpeg["source"] == "rendered" else c.frames, b.header, b.arena, b.record, b.workspace,
                          b.subsampling, geom=c.geom, flag=p.flag)

    def read(self, result):
        return result.jpeg.bytes()

    def save(self, host, b, stem, size, det, dst):
        if host[b]:
            with open(os.path.join(dst, stem + ".jpg"), "wb") as f:
                f.write(host[b])


# what leaves the device in its final form: parsed behind STAGES and kept behind them in `pipeline.stages`
OUTPUTS = (Jpeg,)
