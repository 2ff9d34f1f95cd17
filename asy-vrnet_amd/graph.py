"""HIP-graph capture of one training step (forward + backward) of the hot path.

The step is ~2000 kernel launches issued from Python; eager execution is launch-bound for the
narrow widths.  Shapes, buffers and the launch sequence are static (no host sync anywhere on the
path -- the reference's `if d_min < 0` sync, vr_coc.py:61, is dead code and dropped), so the step
is captured once and replayed.

Single GPU: one hipGraph per step.  Data parallel (the reference: DDP's reducer overlapping the
bucket all-reduces with autograd, train.py:367-368): the backward is cut at section boundaries into
2-3 consecutive hipGraphs that share one memory pool; after segment k has been enqueued, the RCCL
all-reduce of the gradient-arena slice it completed is issued (RCCL's stream waits for the work
enqueued so far) and overlaps the replay of segment k+1.  Collectives stay outside the captured
graphs.  Any change of shape (last batch of an epoch, validation loop) needs its own GraphedStep;
the plain `model(x, r)` path stays available for those.

`TrainStep` is the whole training step on top of that: the real loss on targets in static buffers, the optimizer step and
the EMA update as one more graph, and the epoch's loss statistics, without a host synchronisation.
"""
import contextlib
import gc

import numpy as np
import torch

from . import data, hip, losses, metrics, program


@contextlib.contextmanager
def collector_held_off():
    """Around a stream capture: no run of Python's cycle collector inside it.  A dead reference cycle that holds GPU objects of
    an EARLIER capture (a CUDAGraph, tensors of its pool) is otherwise destroyed at whatever allocation trips the collector's
    counter -- between two captured launches, and the process was seen to abort there (GraphedStep._capture, under
    program.backward_range, when the suite ran in another order).  torch.cuda.graph once collected before every capture and
    now does so only with torch.compiler.config.force_cudagraph_gc: collect here, once, and hold the collector off until the
    capture has ended."""
    gc.collect()
    was = gc.isenabled()
    gc.disable()
    try:
        yield
    finally:
        if was:
            gc.enable()


def replay_segments(graphs, bucketer):
    """One captured step: replays the segment graphs in order; with a data-parallel bucketer, the all-reduce of the arena
    slice segment k completed is issued right behind graph k (it runs beside the replay of k + 1), and the step ends when
    every collective has finished.  `graphs`: objects with .replay()."""
    if bucketer is None:
        graphs[0].replay()
    elif len(graphs) == 1:
        graphs[0].replay()
        bucketer.allreduce_all()
    else:
        for k, g in enumerate(graphs):
            g.replay()
            bucketer.allreduce_segment(k)
        bucketer.wait()


class GraphedStep:
    """step(x, x_radar) -> loss tensor; parameter .grad tensors are static and rewritten by each replay.

    `net` is EfficientVRNet or parallel.DataParallelVRNet; loss_fn(det list, seg) -> scalar tensor.
    Construction runs `warmup` (at least two) eager passes on zero inputs (workspaces, caches, with data parallelism the recording pass
    and its collectives -- so every rank must construct it) and then captures; the module's buffers (BatchNorm running
    statistics, num_batches_tracked) are restored afterwards, so building a GraphedStep on a loaded checkpoint leaves
    the checkpoint's statistics untouched."""

    def __init__(self, net, loss_fn, batch, size, device, warmup=2, segments=None):
        self.net, self.loss_fn = net, loss_fn
        self.model = getattr(net, "module", net)
        self.bucketer = getattr(self.model, "_grad_bucketer", None)
        if getattr(self.model, "_sync_bn", None) is not None:
            raise RuntimeError("GraphedStep: synchronised BatchNorm issues collectives inside the forward / backward program; "
                               "capture is for rank-local BatchNorm statistics (the default) -- run sync_bn steps eagerly")
        self.device = torch.device(device)
        h, w = (size, size) if isinstance(size, int) else size          # size: a side, or (H, W) for rectangular inputs
        self.x = torch.zeros((batch, 3, h, w), device=device)
        self.r = torch.zeros((batch, 4, h, w), device=device)
        cur = torch.cuda.current_stream(device)
        saved = [(b, b.detach().clone()) for b in self.model.buffers() if b.numel()]
        self.stream = torch.cuda.Stream(device)          # warm-up AND capture run here: scratch arenas (hip.Workspace is
        self.stream.wait_stream(cur)                     # keyed by stream) exist before the capture and belong to no graph pool
        with torch.cuda.stream(self.stream):
            # at least two passes: the first one's BACKWARD registers derived caches (the data-gradient weight planes) whose
            # table is rebuilt -- a host-to-device copy -- by the next forward; that must not be the captured one
            for _ in range(max(2, warmup)):              # allocates workspaces / caches outside the capture
                self._eager()
                if self.bucketer is not None and self.bucketer.recording:
                    self.bucketer.rebuild_from_recording()      # arena in execution order before anything is captured
        cur.wait_stream(self.stream)
        torch.cuda.synchronize(device)
        with torch.no_grad():
            for b, old in saved:                         # the warm-up's zero-input statistics must not leak into the model
                b.copy_(old)
        if self.bucketer is None:
            self.model.zero_grad(set_to_none=True)
            cuts = []
        else:
            cuts = list(self.bucketer.cuts) if (segments is None or segments > 1) else []
        self.graphs = []
        if self.bucketer is None:
            self._capture(cuts)
        else:
            # no collective may be issued from inside the captured backward; OUTSIDE the capture the bucketer is back in
            # its eager, overlapped mode, so a plain `net(x, r)` + backward (odd last batch, validation) still reduces
            with self.bucketer.deferring():
                self._capture(cuts)

    def _prologue(self):
        """Work a subclass puts in front of the forward pass: the first nodes of graph 0 (and of every warm-up pass)."""

    def _eager(self):
        self._prologue()
        det, seg = self.net(self.x, self.r)
        loss = self.loss_fn(det, seg)
        loss.backward()
        return loss.detach()

    def _capture(self, cuts):
        """cuts: descending tape positions; segment 0 = forward + loss + backward down to cuts[0], ..."""
        model = self.model
        pool = None
        state = {}

        def seg0():
            self._prologue()
            rt, inputs, dets, seg = program.forward_pass(model, self.x, self.r, record=True)
            leaves = [d.requires_grad_(True) for d in dets] + [seg.requires_grad_(True)]
            loss = self.loss_fn(leaves[:3], leaves[3])
            grads = torch.autograd.grad(loss, leaves, allow_unused=True)
            program.backward_begin(rt, grads[:3], grads[3])
            state.update(rt=rt, inputs=inputs, n=len(rt.tape))
            self.loss = loss.detach()

        bounds = None
        with collector_held_off():
            for k in range(len(cuts) + 1):
                g = torch.cuda.CUDAGraph()
                # thread_local: with a process group alive, RCCL's watchdog thread polls its work events (hipEventQuery) at any
                # moment; under the default "global" capture mode such a call from ANOTHER thread invalidates the capture
                # (hipErrorStreamCaptureInvalidated) and raises in the watchdog, which aborts the process at exit
                with torch.cuda.graph(g, pool=pool, stream=self.stream, capture_error_mode="thread_local"):
                    if k == 0:
                        seg0()
                        n = state["n"]
                        bounds = [n] + [c for c in cuts if 0 < c < n] + [0]
                    rt = state["rt"]
                    if k + 1 < len(bounds):
                        program.backward_range(rt, bounds[k + 1], bounds[k])
                    if k + 2 == len(bounds):
                        program.backward_end(rt, model, state["inputs"], (False, False))
                    else:
                        program.backward_cut(rt, final=False)
                pool = g.pool()
                self.graphs.append(g)
                if k + 2 >= len(bounds):
                    break

    def __call__(self, x, x_radar):
        self.x.copy_(x, non_blocking=True)
        self.r.copy_(x_radar, non_blocking=True)
        if getattr(self.net, "broadcast_buffers", False) and self.model.training:
            self.net.sync_buffers()
        replay_segments(self.graphs, self.bucketer)
        return self.loss


class _PlainFrames:
    """The frame mode of `TrainStep(from_frames=True)`: what the prologue does to the raw frames.  This one is the plain
    letterbox; `_AugmentFrames` and `_MosaicFrames` answer the same questions for the augmentation and for Mosaic.
    TrainStep picks one in its constructor and asks it wherever the three differ, so it branches nowhere itself; a
    further mode is a further subclass and one more line where the constructor picks."""
    per_image = 1                            # source slots per output image
    table_attr, keeps_table = "geom", False  # the step's device table; keeps_table: drawn per call, aug_table keeps the host copy
    ops = ("letterbox_ragged", "seg_targets_ragged", "box_targets_ragged", None)   # hip's frames, seg, boxes and radar calls
    workspace = "letterbox_ragged_workspace_bytes"
    to_bytes = staticmethod(data.geometry_bytes)

    def default_max_taps(self, step):
        return data.default_max_taps(step.capacity, step.hw)

    def warmup_table(self, step):
        """The table of the warm-up and the capture: frames that fill their slots."""
        return data.frame_geometry([step.capacity] * step.batch, step.hw, step.letterbox_image, step.capacity, step.max_taps, "TrainStep")

    def check(self, step, aug, own):
        """The table of a call from the caller's aug and the frames' own sizes, checked; None: `finish` draws it."""
        if aug is not None:
            raise RuntimeError("TrainStep: an aug table belongs to a step built with augment")
        return data.frame_geometry(own, step.hw, step.letterbox_image, step.capacity, step.max_taps, "TrainStep")

    def finish(self, step, own, table, counts):
        """The last host check of a call, after everything else has passed: what needs the box counts, then the draw from
        the step's generator where `check` left the table open.  A call that raises for another reason draws nothing."""
        return table

    def radar_dst(self, step):
        """Where a call's radar maps are copied to."""
        return step.r

    def frames(self, step, table, **kw):
        hip.letterbox_ragged(step.frames_u8, None, table, *step.hw, step.max_taps, **kw)

    def launch(self, step):
        """The prologue's launches: frames, segmentation targets, boxes, radar maps."""
        (h, w), table = step.hw, getattr(step, self.table_attr)
        self.frames(step, table, images=step.x, flag=step.flag, ws=step._lb_ws)
        getattr(hip, self.ops[1])(step.frame_labels_u8, table, h, w, step.ns, png_out=step.png, onehot=step.onehot, flag=step.flag)
        getattr(hip, self.ops[2])(step.boxes, step.box_counts, table, step.capacity, h, w, targets=step.labels, counts_out=step.counts,
                                  flag=step.flag)
        if step.radar_points is not None:                    # radar points: projected into step.r, no finished maps to move
            self.points(step, table)
        elif self.ops[3]:
            getattr(hip, self.ops[3])(step.radar_in, table, step.capacity, out=step.r, flag=step.flag)

    # radar points (step.radar_points, an `infer.RadarPoints` over the step's sources): the per-call device table beside the
    # points, the key workspace and the launch
    def point_table(self, step, table, checked):
        """The uint8 host table `points` reads beside the points, from the call's table and the (projection, counts) pair
        `RadarPoints.validate(points, None)` returned: one view record per image, under the window its frame goes through."""
        return step.radar_points.views(table, checked)

    def point_workspace_bytes(self, step):
        return hip.radar_map_workspace_bytes(step.batch, *step.hw)

    def points(self, step, table):
        """vrnet_radar_map_f32: the points of each image under the window (and flip) its frame just went through."""
        rp = step.radar_points
        hip.radar_map(step.points, step.views, *step.hw, rp.radius, float(rp.min_depth), step.r, flag=step.flag, ws=step._radar_ws)


class _AugmentFrames(_PlainFrames):
    """The single-image training augmentation: one `data.AUG_DTYPE` record per image, drawn per call."""
    table_attr, keeps_table = "aug", True
    ops = ("augment_frames", "augment_seg_targets", "augment_box_targets", "augment_radar")
    to_bytes = staticmethod(data.augment_bytes)

    def default_max_taps(self, step):
        kw = {k: step.augment[k] for k in ("jitter", "scale") if k in step.augment}
        return data.default_aug_max_taps(step.capacity, step.hw, **kw)

    def warmup_table(self, step):
        """... under the letterbox window of such a frame."""
        (ihm, iwm), (h, w) = step.capacity, step.hw
        rec = data.aug_record(step.capacity, step.hw, *data.letterbox_geometry(iwm, ihm, w, h))
        return data.check_aug_table(np.stack([rec] * step.batch), step.hw, step.capacity, step.max_taps, "TrainStep")

    def check(self, step, aug, own):
        return None if aug is None else data.check_aug_params(aug, own, step.hw, step.capacity, step.max_taps, "TrainStep")

    def finish(self, step, own, table, counts):
        if table is None:
            # a draw that fails its own checks (an empty window, a sliver's taps) has advanced the generator: the next call
            # draws anew
            table = data.augment_params(own, step.hw, step._aug_rng, capacity=step.capacity, max_taps=step.max_taps, fn="TrainStep",
                                        **step.augment)
        return table

    def radar_dst(self, step):
        return step.radar_in

    def frames(self, step, table, **kw):
        getattr(hip, self.ops[0])(step.frames_u8, table, *step.hw, step.max_taps, **kw)


class _MosaicFrames(_AugmentFrames):
    """Mosaic: one `data.MOSAIC_DTYPE` record per output image over four source slots each, drawn per call."""
    per_image = 4
    ops = ("mosaic_frames", "mosaic_seg_targets", "mosaic_box_targets", "mosaic_radar")
    workspace = "mosaic_workspace_bytes"
    to_bytes = staticmethod(data.mosaic_bytes)

    def default_max_taps(self, step):
        # mosaic_prob may change from call to call: the capacity serves the Mosaic draw and the plain one
        kw = {k: step.mosaic[k] for k in ("jitter", "scale") if k in step.mosaic}
        return data.default_mosaic_max_taps(step.capacity, step.hw, prob=0.0, plain=step.augment, **kw)

    def warmup_table(self, step):
        (ihm, iwm), (h, w) = step.capacity, step.hw
        lb = data.letterbox_geometry(iwm, ihm, w, h)
        recs = [data.mosaic_record(step.hw, (w, h), [(4 * b, step.capacity) + lb, None, None, None]) for b in range(step.batch)]
        return data.check_mosaic_table(np.stack(recs), step.hw, [step.capacity] * step.sources, step.capacity, step.max_taps, "TrainStep")

    def check(self, step, aug, own):
        if aug is None:
            return None
        if len(np.asarray(aug)) != step.batch:
            raise RuntimeError(f"TrainStep: the Mosaic table is a ({step.batch},) array of data.MOSAIC_DTYPE records")
        return data.check_mosaic_table(aug, step.hw, own, step.capacity, step.max_taps, "TrainStep")

    def finish(self, step, own, table, counts):
        # conservative: the sources of an output image TOGETHER bring at most max_gt boxes, whatever the cut would drop
        # (the kernel would keep the first max_gt of more and report FLAG_BOX_COUNT); a drawn table uses sources 4 b .. 4 b + 3
        for b in range(step.batch):
            srcs = range(4 * b, 4 * b + 4) if table is None else [int(s) for s in table[b]["tile"]["src"] if s >= 0]
            total = sum(int(counts[s]) for s in srcs)
            if total > step.max_gt:
                raise RuntimeError(f"TrainStep: image {b}: its sources bring {total} boxes together, above max_gt = {step.max_gt}")
        if table is None:
            table = data.mosaic_params(own, step.hw, step._aug_rng, step.batch, prob=float(step.mosaic_prob), plain=step.augment,
                                       capacity=step.capacity, max_taps=step.max_taps, fn="TrainStep", **step.mosaic)
        return table

    # radar points: the windows are the Mosaic table's own, which the kernel reads where the other Mosaic kernels do; the
    # table beside the points carries only what a SOURCE adds, its count and its projection
    def point_table(self, step, table, checked):
        return data.radar_source_bytes(data.radar_sources(checked[0], checked[1].numpy()))

    def point_workspace_bytes(self, step):
        return hip.mosaic_radar_points_workspace_bytes(step.batch, *step.hw)

    def points(self, step, table):
        """vrnet_mosaic_radar_points_f32: the points of every tile's source under the tile's window, inside its quadrant."""
        rp = step.radar_points
        hip.mosaic_radar_points(step.points, step.views, table, step.capacity, *step.hw, rp.radius, float(rp.min_depth), step.r,
                                flag=step.flag, ws=step._radar_ws)


class TrainStep(GraphedStep):
    """One captured training step: forward, the reference's loss (`losses.training_loss`: SimOTA YOLO loss, focal or CE,
    dice, det + 5 seg; utils_fit.py:96-106), backward, optimizer step and EMA update, replayed without a host sync.

        step = TrainStep(net, yolo_loss, optimizer, ema, batch, size, num_seg_classes, max_gt=64)
        res = step(images, radar, targets, pngs, seg_labels)      # device tensors, valid until the next call

    net: EfficientVRNet or parallel.DataParallelVRNet; optimizer: optim.SGD / optim.Adam; ema: optim.ModelEMA or None.
    images (B,3,H,W) float32, radar (B,4,H,W) float32, targets: B tensors of (n_i, 5) rows [cx, cy, w, h, cls] (None or
    empty: no boxes; n_i <= max_gt), pngs (B,H,W) integer labels, seg_labels (B,H,W,ns+1) one-hot (needed for the dice
    loss and the f-score).  With from_bytes=True images are the letterboxed canvas bytes (B,H,W,3) uint8 and pngs the label
    bytes (B,H,W) uint8, as `data.device_letterbox(..., normalise=False)` or a dataloader produces them: 4 B per pixel
    cross PCIe and vrnet_batch_formats_u8, the first node of graph 0, writes the float images, the int64 labels and the
    one-hot labels straight into the buffers the forward pass and the losses read; seg_labels stays None.
    Host or device inputs; numpy arrays are taken too.

    With from_frames=True (not together with from_bytes) the step takes RAW frames of mixed sizes and does the reference's
    `random=False` dataset item inside graph 0 as well:

        step = TrainStep(net, yolo_loss, optimizer, ema, batch, size, ns, from_frames=True, capacity=(ihm, iwm))
        res = step(frames, radar, boxes, labels, sizes=None)

    frames / labels: a list of B uint8 arrays (ih_b, iw_b, 3) / (ih_b, iw_b) of their own sizes, or padded buffers (B, ihp,
    iwp[, 3]) plus sizes (B, 2) host integers, as `FramePipeline(ragged=True)` takes them; radar (B,4,H,W) float32, taken as
    it is; boxes: B arrays of (n_i, 5) INTEGER rows x1, y1, x2, y2, cls in pixels of the original image
    (`data.parse_annotation_line`; None or empty: no boxes).  One host validation per call, before anything is enqueued:
    capacity, empty window, tap capacity (`data.frame_geometry`), box counts and dtypes (`data.pack_boxes`).  Then the
    frames and label maps are copied into the corners of their slots, the geometry table and the boxes go up through fresh
    pinned staging tensors, and the first nodes of graph 0 -- vrnet_letterbox_ragged_u8, vrnet_seg_targets_ragged_u8,
    vrnet_box_targets_ragged_f32 -- write the float images, the labels, the one-hot labels, the packed targets and their
    counts in place.  `stats()` then carries "flag": the flag word of those kernels (hip.FLAG_GEOMETRY, hip.FLAG_BOX_COUNT;
    0 for inputs that passed the host validation), read back in the same single read-back; `reset_stats()` clears it.

    With from_frames=True and augment set -- True, or a dict of `data.augment_params`' keywords (jitter, hue, sat, val,
    scale, flip, color) -- the prologue is the training augmentation instead of the letterbox: the random resize, placement,
    flip and colour jitter of utils/dataloader.py:187-247, applied by one record per image to the frame, the label map, the
    boxes AND the radar map (each radar map is aligned with the letterbox window of its frame, as the dataset stores it):

        step = TrainStep(..., from_frames=True, capacity=(ihm, iwm), augment=True, aug_seed=0)
        res = step(frames, radar, boxes, labels, sizes=None, aug=None)

    Six launches -- vrnet_augment_frames_u8 (tables, horizontal, vertical + paste + flip + colour), vrnet_augment_seg_targets_u8,
    vrnet_augment_box_targets_f32, vrnet_augment_radar_f32 -- write the float images, the radar input, the labels, the one-hot
    labels, the packed targets and their counts.  Every call draws its table on the host from the step's own
    numpy RandomState(aug_seed) (`data.augment_params`; `aug_table` keeps the last one) and copies it into the static device
    table before the replay, as the geometry table is copied; aug= hands in an explicit `data.AUG_DTYPE` table instead (a
    caller's own sampler; the step's generator is then not advanced).  The table is validated on the host with the rest,
    before anything is enqueued.  max_taps defaults to `data.default_aug_max_taps`.  augment without from_frames raises.

    With from_frames=True and mosaic set -- True, or a dict of `data.mosaic_params`' keywords (prob, jitter, hue, sat, val, scale,
    cut, flip, color) -- the prologue is Mosaic (utils/dataloader.py:251-426; train.py:108-112 `mosaic`, `mosaic_prob`): every
    output image is cut from four source frames, and one record per output image drives the frames, the label maps, the boxes
    and the radar maps alike (`data.mosaic_sample` is the rule, with its two departures from the reference):

        step = TrainStep(..., from_frames=True, capacity=(ihm, iwm), mosaic=True, augment=None | True | {...}, aug_seed=0)
        res = step(frames, radar, boxes, labels, sizes=None, aug=None)

    frames, labels and boxes are those of 4 B SOURCES, radar is (4 B, 4, H, W); output image b uses sources 4 b .. 4 b + 3.  Six
    launches -- vrnet_mosaic_frames_u8 (three), vrnet_mosaic_seg_targets_u8, vrnet_mosaic_box_targets_f32, vrnet_mosaic_radar_f32
    -- stand where the six of augment stood.  Every call draws its table from the step's RandomState(aug_seed)
    (`data.mosaic_params`); `step.mosaic_prob` (the `prob` keyword, default 1) is read at every call, so the `special_aug_ratio`
    policy -- Mosaic for the first share of the epochs -- is one assignment by the caller and needs no new capture; an image
    that is not mosaicked gets the single-image draw with the keywords of augment.  aug= hands in an explicit
    `data.MOSAIC_DTYPE` table instead (any tile may name any of the 4 B sources; the generator is then not advanced);
    `aug_table` keeps the last table.  Host validation as before, with one more rule: the sources of an output image together
    bring at most max_gt boxes -- conservative, since the cut may drop some, but known before anything is enqueued.  mosaic
    without from_frames or with letterbox_image=False raises at construction.

    With from_frames=True and radar_points=max_points the step takes radar POINTS where it took maps:

        step = TrainStep(..., from_frames=True, capacity=(ihm, iwm), radar_points=4096, radar_radius=0, radar_min_depth=0.1, calib=P)
        res = step(frames, points, boxes, labels, sizes=None, aug=None, calib=None)

    points: B arrays of (n_b, 7) float32 rows x, y, z, f0..f3, or a pair (padded array, counts) (`data.pack_points`); calib: the
    (3, 4) or (B, 3, 4) projection of `data.radar_map`, per call or from the constructor.  vrnet_radar_map_f32 (three launches)
    writes the radar input inside graph 0 by the rule of `data.radar_map`: without augment under the window of the geometry
    table, with augment under the window and flip of that call's augmentation table, in place of vrnet_augment_radar_f32 --
    every point moves exactly once, where the gather of a finished map duplicates or drops points.  Points and the view
    table go up through fresh pinned staging tensors; the kernel's bits (hip.FLAG_GEOMETRY, hip.FLAG_POINT_COUNT) join the
    step's flag word.  radar_points without from_frames raises.

    With mosaic AND radar_points the points are those of the 4 B SOURCES and every tile's points are projected into the tile's
    own window (`data.mosaic_radar_map` is the rule):

        step = TrainStep(..., from_frames=True, capacity=(ihm, iwm), mosaic=True, radar_points=4096, calib=P)
        res = step(frames, points, boxes, labels, sizes=None, aug=None, calib=None)

    points: 4 B point sets, one per source; calib: (3, 4) or (4 B, 3, 4), one projection per SOURCE.  The static buffers are the
    (4 B, max_points, 7) points, the (4 B, hip.RADAR_SOURCE_BYTES) table of counts and projections and the key workspace; no
    (4 B, 4, H, W) maps exist or cross PCIe.  vrnet_mosaic_radar_points_f32 (three launches) stands where vrnet_mosaic_radar_f32
    stood and reads the step's Mosaic table (`step.aug`) as the other Mosaic kernels do, so drawn tables, aug= tables and
    `mosaic_prob` behave as with maps.  An error that names a point set names its source as "image b, tile t".  The one
    asymmetry against the plain and the augment mode: here the projection is REQUIRED at construction (a per-call calib still
    overrides it).  `TrainStep(mosaic=True, radar_points=N)` without one has always been refused at construction and stays
    refused: such a step could otherwise only fail at its first call, after the warm-up and the capture were paid for.

    Two kinds of graph.  The forward / backward graph(s) are GraphedStep's (three segments under data parallelism, the
    all-reduces between them); the loss closure is `losses.training_loss_packed` on the static buffers, followed by the
    f-score (f_score=True) and the addition of the step's values to a running fp64 sum.  The UPDATE graph is always its own:
    optimizer.step(scalars=rec), then ema.update(model, scalars=rec); it replays behind the last segment, i.e. behind
    bucketer.wait() under data parallelism.  What changes from step to step -- the learning rate, the EMA decay, Adam's
    bias corrections -- is read by those kernels from `rec`, a hip.StepScalars record in device memory that every call
    writes in stream order through a fresh pinned staging tensor: a graph bakes launch scalars in.

    Counters.  Every call reads lr from optimizer.param_groups (so `optim.set_optimizer_lr` works as before), advances
    Adam's per-parameter `step` and `ema.updates` on the host (`Adam.advance`, `ModelEMA.advance`) and writes their values
    into the record.  optimizer.state_dict(), ema.updates, the EMA weights and the model's buffers are therefore what the
    eager loop would have left: checkpoints work, and so does an eager step (zero_grad, model, loss, backward, step,
    update) for an odd last batch in between.

    Statistics.  res holds total, loss_det, loss_seg (and f_score) of this step; `stats()` returns their means since the
    last `reset_stats()` with ONE read-back (utils_fit.py reads three values back per iteration).

    Rebuild rule.  The parameters' .grad tensors belong to the step, the momentum, betas, eps, nesterov and the set of
    updated parameters are baked into the update graph.  Un-freezing parameters (train.py:584), changing the momentum or
    any shape (batch, size, max_gt) needs a NEW TrainStep.

    Raises at construction: synchronised BatchNorm (inherited), an optimizer whose groups disagree on lr."""

    def __init__(self, net, yolo_loss, optimizer, ema, batch, size, num_seg_classes, max_gt=64, cls_weights=None,
                 focal_loss=True, dice_loss=True, f_score=False, from_bytes=False, device="cuda", warmup=2, segments=None,
                 from_frames=False, capacity=None, max_taps=None, letterbox_image=True, augment=None, aug_seed=None,
                 radar_points=None, radar_radius=0, radar_min_depth=0.1, calib=None, mosaic=None):
        optimizer._uniform("lr")
        if mosaic is not None and mosaic is not False:
            if not from_frames:
                raise RuntimeError("TrainStep: mosaic needs from_frames=True (the tiles are cut from the raw frames)")
            if radar_points is not None and calib is None:
                raise RuntimeError("TrainStep: mosaic with radar_points needs calib= at construction: one (3, 4) projection, or "
                                   "(4 * batch, 3, 4), one per SOURCE (a call may still bring its own)")
            if not letterbox_image:
                raise RuntimeError("TrainStep: mosaic places the tiles itself; letterbox_image=False does not apply")
        if radar_points is not None and not from_frames:
            raise RuntimeError("TrainStep: radar_points needs from_frames=True (the points are projected into the frame's window)")
        if radar_points is None and (calib is not None or radar_radius != 0 or radar_min_depth != 0.1):
            raise RuntimeError("TrainStep: calib, radar_radius and radar_min_depth belong to radar_points=max_points")
        self.augment = None if augment is None or augment is False else ({} if augment is True else dict(augment))
        self.mosaic = None if mosaic is None or mosaic is False else ({} if mosaic is True else dict(mosaic))
        if self.mosaic is not None:
            self.mosaic_prob = float(self.mosaic.pop("prob", 1.0))      # read at every call: the caller may assign it
        self.mode = _MosaicFrames() if self.mosaic is not None else _AugmentFrames() if self.augment is not None else _PlainFrames()
        self.sources = int(batch) * self.mode.per_image
        from .infer import RadarPoints                   # one point set and one projection per SOURCE
        self.radar_points = None if radar_points is None else RadarPoints(radar_points, radar_radius, radar_min_depth, calib,
                                                                          self.sources, "TrainStep", self.mode.per_image)
        if augment is not None and augment is not False and not from_frames:
            raise RuntimeError("TrainStep: augment needs from_frames=True (the augmentation starts from the raw frames)")
        if augment is not None and augment is not False and not letterbox_image:
            raise RuntimeError("TrainStep: augment places the frame itself; letterbox_image=False does not apply")
        if from_frames and from_bytes:
            raise RuntimeError("TrainStep: from_frames and from_bytes exclude each other (raw frames, or a letterboxed batch)")
        if from_frames and capacity is None:
            raise RuntimeError("TrainStep: from_frames=True needs capacity = (ihm, iwm), the largest frame a call may bring")
        dev = torch.device(device)
        h, w = (size, size) if isinstance(size, int) else size
        ns = int(num_seg_classes)
        self.yolo_loss, self.optimizer, self.ema = yolo_loss, optimizer, ema
        self.batch, self.hw, self.ns, self.max_gt = int(batch), (h, w), ns, int(max_gt)
        self.focal_loss, self.dice_loss, self.f_score, self.from_bytes = bool(focal_loss), bool(dice_loss), bool(f_score), bool(from_bytes)
        self.from_frames = bool(from_frames)
        self.names = ("total", "loss_det", "loss_seg") + (("f_score",) if self.f_score else ())
        with torch.cuda.device(dev):
            self.labels = torch.zeros((batch, max(self.max_gt, 1), 5), dtype=torch.float32, device=dev)
            self.counts = torch.zeros(batch, dtype=torch.int32, device=dev)
            self.png = torch.zeros((batch, h, w), dtype=torch.int64, device=dev)
            self.onehot = torch.zeros((batch, h, w, ns + 1), dtype=torch.float32, device=dev)
            self.images_u8 = torch.zeros((batch, h, w, 3), dtype=torch.uint8, device=dev) if self.from_bytes else None
            self.labels_u8 = torch.zeros((batch, h, w), dtype=torch.uint8, device=dev) if self.from_bytes else None
            self.weights = torch.ones(ns, dtype=torch.float32, device=dev)
            if cls_weights is not None:
                self.weights.copy_(torch.as_tensor(cls_weights, dtype=torch.float32).reshape(ns))
            self.rec = torch.zeros(4, dtype=torch.float32, device=dev)            # hip.StepScalars
            # running sums, step count; from_frames: the flag word too, so that stats() stays one read-back
            self._acc = torch.zeros(len(self.names) + 1 + int(self.from_frames), dtype=torch.float64, device=dev)
            if self.from_frames:
                self._frame_buffers(batch, capacity, max_taps, letterbox_image, dev, aug_seed)
        self._vals = None
        super().__init__(net, self._loss, batch, size, dev, warmup=warmup, segments=segments)
        self._capture_update()
        self.reset_stats()                               # the warm-up passes on zero inputs counted themselves
        torch.cuda.synchronize(dev)

    def _frame_buffers(self, batch, capacity, max_taps, letterbox_image, dev, aug_seed=None):
        """The static inputs of from_frames=True.  The warm-up and the capture run on a table of frames that fill their
        slots (as FramePipeline's do) and on no boxes; with augment, on the letterbox window of such a frame."""
        (h, w), B = self.hw, batch
        self.capacity = ihm, iwm = tuple(int(v) for v in capacity)
        self.letterbox_image = bool(letterbox_image)
        S, mode = self.sources, self.mode
        self.max_taps = mode.default_max_taps(self) if max_taps is None else int(max_taps)
        table = mode.warmup_table(self)
        if mode.keeps_table:
            self._aug_rng = np.random.RandomState(aug_seed)
            self.aug_table = table
        setattr(self, mode.table_attr, mode.to_bytes(table).to(dev))
        if self.radar_points is not None:    # no points in the warm-up and the capture: every count is 0
            rp = self.radar_points
            P = rp.calib if rp.calib is not None else np.zeros((S, 3, 4), np.float32)
            self.points = torch.zeros((S, rp.max_points, 7), dtype=torch.float32, device=dev)
            self.views = mode.point_table(self, table, (P, torch.zeros(S, dtype=torch.int32))).to(dev)
            self._radar_ws = torch.empty(mode.point_workspace_bytes(self), dtype=torch.uint8, device=dev)
        elif mode.ops[3]:                    # the prologue moves the radar maps: a call copies them here (mode.radar_dst)
            self.radar_in = torch.zeros((S, 4, h, w), dtype=torch.float32, device=dev)
        self.frames_u8 = torch.zeros((S, ihm, iwm, 3), dtype=torch.uint8, device=dev)
        self.frame_labels_u8 = torch.zeros((S, ihm, iwm), dtype=torch.uint8, device=dev)
        self.boxes = torch.zeros((S, max(self.max_gt, 1), 5), dtype=torch.int32, device=dev)
        self.box_counts = torch.zeros(S, dtype=torch.int32, device=dev)
        self.flag = torch.zeros(1, dtype=torch.int32, device=dev)
        self._lb_ws = torch.empty(getattr(hip, mode.workspace)(B, ihm, iwm, h, w, self.max_taps), dtype=torch.uint8, device=dev)

    def _prologue(self):
        if self.from_bytes:
            hip.batch_formats(self.images_u8, self.labels_u8, self.ns, images=self.x, png_out=self.png, onehot=self.onehot)
        elif self.from_frames:
            self.mode.launch(self)

    def _loss(self, det, seg):
        total, ldet, lseg = losses.training_loss_packed(self.yolo_loss, det, seg, self.labels, self.counts, self.max_gt, self.png,
                                                        self.onehot, self.weights, self.ns, self.focal_loss, self.dice_loss)
        vals = [total.detach(), ldet.detach(), lseg.detach()]
        if self.f_score:
            vals.append(metrics.f_score(seg.detach(), self.onehot))
        self._vals = torch.stack(vals)
        n = len(vals)
        self._acc[:n].add_(self._vals)
        self._acc[n:n + 1].add_(1.0)
        if self.from_frames:
            self._acc[n + 1:].copy_(self.flag)
        return total

    def _capture_update(self):
        """The update graph.  The address tables are laid out and uploaded BEFORE the capture (host-to-device copies); inside
        it the front ends find nothing changed and issue their one launch each."""
        model, opt = self.model, self.optimizer
        self._grads = [(p, p.grad) for p in model.parameters() if p.grad is not None]
        with torch.cuda.device(self.device):
            tab = opt._live()
            if tab is None:
                raise RuntimeError("TrainStep: no parameter of the optimizer received a gradient")
            self._opt_addrs = tab.addrs
            if self.ema is not None:
                self.ema._tensor_table(model)
            torch.cuda.synchronize(self.device)
            cur = torch.cuda.current_stream(self.device)
            self.stream.wait_stream(cur)
            self.update_graph = torch.cuda.CUDAGraph()
            with collector_held_off(), torch.cuda.graph(self.update_graph, pool=self.graphs[-1].pool(), stream=self.stream,
                                                        capture_error_mode="thread_local"):
                opt.step(scalars=self.rec)
                if self.ema is not None:
                    self.ema.update(model, scalars=self.rec)

    # ---- one step ------------------------------------------------------------------------------------------------
    @staticmethod
    def _tensor(a):
        return a if torch.is_tensor(a) else torch.from_numpy(np.ascontiguousarray(a))

    def _validate(self, images, radar, targets, pngs, seg_labels):
        B, (h, w), ns = self.batch, self.hw, self.ns
        images, radar, pngs = self._tensor(images), self._tensor(radar), self._tensor(pngs)

        def need(t, what, shape, dtypes):
            if tuple(t.shape) != shape or t.dtype not in dtypes:
                raise RuntimeError(f"TrainStep: {what} must be {' / '.join(str(d) for d in dtypes)} of shape {shape}, got "
                                   f"{t.dtype} {tuple(t.shape)}")
        ints = (torch.int64, torch.int32, torch.uint8)
        if self.from_bytes:
            need(images, "images (from_bytes=True: the letterboxed canvas bytes)", (B, h, w, 3), (torch.uint8,))
            need(pngs, "pngs (from_bytes=True: the label bytes)", (B, h, w), (torch.uint8,))
            if seg_labels is not None:
                raise RuntimeError("TrainStep: from_bytes=True makes the one-hot labels on the device; seg_labels must be None")
        else:
            need(images, "images", (B, 3, h, w), (torch.float32,))
            need(pngs, "pngs", (B, h, w), ints)
            if seg_labels is None:
                if self.dice_loss or self.f_score:
                    raise RuntimeError("TrainStep: the dice loss and the f-score need the one-hot seg_labels (B, H, W, ns + 1)")
            else:
                seg_labels = self._tensor(seg_labels)
                need(seg_labels, "seg_labels", (B, h, w, ns + 1), (torch.float32,))
        need(radar, "radar", (B, 4, h, w), (torch.float32,))
        if len(targets) != B:
            raise RuntimeError(f"TrainStep: {len(targets)} target lists for a batch of {B}")
        packed, counts = losses.pack_targets(targets, self.max_gt)        # raises, naming the image, above max_gt
        return images, radar, pngs, seg_labels, packed, counts

    def _validate_frames(self, frames, radar, boxes, labels, sizes, aug=None, calib=None):
        """The host checks of a from_frames call, which need no device; returns what the copies take, the geometry table
        (with augment: the augmentation table, drawn here unless the caller brought one) among it."""
        B, (h, w), fn = self.sources, self.hw, "TrainStep"          # with mosaic: the 4 B sources
        items, own = data.ragged_items(frames, sizes, B, (3,), "frames", fn)
        labs = data.ragged_items(labels, own, B, (), "label maps", fn)[0]
        for t in (items, labs):
            if torch.is_tensor(t) and (t.shape[1] > self.capacity[0] or t.shape[2] > self.capacity[1]):
                raise RuntimeError(f"{fn}: the padded buffer {tuple(t.shape[1:3])} is above the capacity {self.capacity}")
        table = self.mode.check(self, aug, own)          # None: drawn last, below: a call that raises for another reason draws nothing
        if calib is not None and self.radar_points is None:
            raise RuntimeError(f"{fn}: calib belongs to a step built with radar_points")
        if self.radar_points is None:
            radar = self._tensor(radar)
            if tuple(radar.shape) != (B, 4, h, w) or radar.dtype != torch.float32:
                raise RuntimeError(f"{fn}: radar must be torch.float32 of shape {(B, 4, h, w)}, got {radar.dtype} {tuple(radar.shape)}")
        else:                                # the views follow the table, which may yet be drawn
            radar = self.radar_points.validate(radar, None, calib)
        if len(boxes) != B:
            raise RuntimeError(f"{fn}: {len(boxes)} box lists for a batch of {B}")
        packed, counts = data.pack_boxes(boxes, self.max_gt)              # raises, naming the image
        table = self.mode.finish(self, own, table, counts)
        if self.radar_points is not None:
            radar = radar[0], self.mode.point_table(self, table, radar[1])
        return items, labs, own, table, radar, packed, counts

    def __call__(self, images, radar, targets, pngs, seg_labels=None, sizes=None, aug=None, calib=None):
        if self.from_frames:                 # step(frames, radar, boxes, labels, sizes=None, aug=None)
            if seg_labels is not None and sizes is not None:
                raise RuntimeError("TrainStep: from_frames=True takes (frames, radar, boxes, labels, sizes)")
            items, labs, own, table, radar, packed, counts = self._validate_frames(
                images, radar, targets, pngs, seg_labels if sizes is None else sizes, aug, calib)
        else:
            if sizes is not None or aug is not None or calib is not None:
                raise RuntimeError("TrainStep: sizes, aug and calib belong to from_frames=True")
            images, radar, pngs, seg_labels, packed, counts = self._validate(images, radar, targets, pngs, seg_labels)
        opt, ema = self.optimizer, self.ema
        lr = float(opt._uniform("lr"))
        with torch.cuda.device(self.device):
            if any(p.grad is not g for p, g in self._grads):          # an eager step in between took the .grad tensors
                for p, g in self._grads:
                    p.grad = g
                opt._live()                                           # ... and pointed the table's gradient row at its own
            if opt._table.addrs is not self._opt_addrs:
                raise RuntimeError("TrainStep: the optimizer's tensor table was laid out anew (parameters un-frozen or groups "
                                   "changed): build a new TrainStep")
            if self.from_frames:
                # the kernels read no input padding into a result: what an earlier call left in a slot is harmless
                data.fill_slots(self.frames_u8, items, own)
                data.fill_slots(self.frame_labels_u8, labs, own)
                # fresh pinned staging tensors (`pack_boxes` makes its own), as for the step record below
                if self.mode.keeps_table:
                    self.aug_table = table
                getattr(self, self.mode.table_attr).copy_(self.mode.to_bytes(table).pin_memory(), non_blocking=True)
                self.boxes.copy_(packed, non_blocking=True)
                self.box_counts.copy_(counts, non_blocking=True)
            elif self.from_bytes:
                self.images_u8.copy_(images, non_blocking=True)
                self.labels_u8.copy_(pngs, non_blocking=True)
            else:
                self.x.copy_(images, non_blocking=True)
                self.png.copy_(pngs, non_blocking=True)
                if seg_labels is not None:
                    self.onehot.copy_(seg_labels, non_blocking=True)
            # with augment the radar maps go through vrnet_augment_radar_f32, which writes self.r inside graph 0
            # and radar points through vrnet_radar_map_f32, likewise
            if self.radar_points is not None:
                self.points.copy_(radar[0], non_blocking=True)
                self.views.copy_(radar[1].pin_memory(), non_blocking=True)
            else:
                self.mode.radar_dst(self).copy_(radar, non_blocking=True)
            if not self.from_frames:
                self.labels.copy_(packed, non_blocking=True)
                self.counts.copy_(counts, non_blocking=True)
            bc = opt.advance() if hasattr(opt, "advance") else None
            decay = ema.advance() if ema is not None else 0.0
            # a FRESH pinned staging tensor per step (as optim._Table.set_row): a host that runs ahead never overwrites a
            # record a queued copy has yet to read
            staged = torch.tensor([lr, decay] + list(bc or (1.0, 1.0)), dtype=torch.float32).pin_memory()
            self.rec.copy_(staged, non_blocking=True)
            if getattr(self.net, "broadcast_buffers", False) and self.model.training:
                self.net.sync_buffers()
            replay_segments(self.graphs, self.bucketer)
            self.update_graph.replay()
        return {k: self._vals[i] for i, k in enumerate(self.names)}

    def stats(self):
        """{"steps": n, "total": mean, "loss_det": mean, "loss_seg": mean[, "f_score": mean]} over the calls since the last
        `reset_stats()`, accumulated in fp64 on the device: one read-back (and the only synchronisation of an epoch)."""
        a = self._acc.cpu()
        n = int(a[len(self.names)])
        out = {"steps": n}
        for i, k in enumerate(self.names):
            out[k] = float(a[i]) / n if n else float("nan")
        if self.from_frames:
            out["flag"] = int(a[-1])
        return out

    def reset_stats(self):
        self._acc.zero_()
        if self.from_frames:
            self.flag.zero_()
