"""Times the pieces of one REAL training step around the hot path on one GPU:
forward+backward with the reference's loss (YOLOLoss SimOTA + focal + dice, total = det + 5 seg) instead of bench.py's
synthetic scalar, the fused SGD step and the fused EMA update.  Eager launches, HIP events per piece.

    python tools/bench_train_step.py [--phi l] [--batch 8] [--size 512] [--steps 5]

--captured compares, in ONE process and in alternating rounds on the same seeded batch, whole steps per second of
  eager        that same eager loop (model, training_loss, backward, opt.step, ema.update, zero_grad)
  TrainStep    graph.TrainStep: the step as captured hipGraphs plus the update graph
  from_bytes   graph.TrainStep(from_bytes=True): 4 B per pixel over PCIe, the formats made on the device
each on a trainer of its own (same seed), the host-to-device copies of the batch included in all three (pinned host
tensors, non-blocking copies).  A round is `--steps` steps (more when a step is short: a window is at least ~0.5 s)
inside a host clock that ends in a device synchronise; the line gives the median round and the spread between rounds.

    python tools/bench_train_step.py --captured [--phi nano] [--rounds 5]

--frames IHxIW (with --captured) starts from RAW frames of that size instead: the batch of every contender is the host
letterbox (data.letterbox_sample) of one seeded set of frames, label maps and pixel boxes, and two contenders join
  host letterbox   data.letterbox_sample + boxes_xyxy_to_cxcywh per image on the host INSIDE the timed loop, then the
                   from_bytes step: what a single-process loop pays without the device path (decoding is in no mode)
  from_frames      graph.TrainStep(from_frames=True): the raw bytes over PCIe, letterbox and targets inside graph 0
so that from_bytes, fed pre-letterboxed bytes, is the device-only floor of the three.

    python tools/bench_train_step.py --captured --frames 1080x1920 [--phi nano]

--augment (with --frames) times the training augmentation against the plain frame path, in ONE process and in alternating
rounds: the three-launch prologue of TrainStep(from_frames=True) and the six-launch prologue of TrainStep(from_frames=True,
augment=True) on their own (eager launches of `_prologue()` between HIP events, no copies), and the whole step with each
(copies and the host's draw of the table included).  The last line is one JSON record.

    python tools/bench_train_step.py --augment --frames 1080x1920 [--phi l]

--mosaic (with --frames) times Mosaic against that augmentation the same way: the six-launch prologue of
TrainStep(from_frames=True, augment=True) on B frames and the six-launch prologue of TrainStep(from_frames=True, mosaic=True)
on 4 B frames, on their own and inside the whole step (copies and the host's draw included).

    python tools/bench_train_step.py --mosaic --frames 1080x1920 [--phi l]

--mosaic-points N (with --frames) times the two radar inputs of the Mosaic step against each other the same way: finished maps
(4 B maps of (4, S, S) floats a step, vrnet_mosaic_radar_f32) and radar POINTS (4 B clouds of N points, vrnet_mosaic_radar_points_f32,
radius --radius), the prologues on their own and the whole steps, copies, the host's draw and the packing of the points included.

    python tools/bench_train_step.py --mosaic-points 4096 --frames 1080x1920 [--phi l]
"""
import argparse
import math
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

import asy_vrnet_amd as A
from asy_vrnet_amd import losses, optim


def synthetic_batch(B, S, NC, NS, seed=0):
    """The seeded host batch of this tool: label rows, label map, and the letterboxed bytes the from_bytes step takes."""
    rng = np.random.default_rng(seed)
    labels = [torch.from_numpy(np.concatenate([rng.uniform(60, S - 60, (n, 2)), rng.uniform(16, 200, (n, 2)),
                                               rng.integers(0, NC, (n, 1))], 1).astype(np.float32))
              for n in rng.integers(3, 25, B)]
    png = np.kron(rng.integers(0, NS + 1, (B, S // 16, S // 16)), np.ones((16, 16), dtype=np.int64))
    img_u8 = rng.integers(0, 256, (B, S, S, 3), dtype=np.uint8)
    return labels, torch.from_numpy(png), torch.from_numpy(img_u8)


def synthetic_frames(B, ih, iw, S, NC, NS, seed=0):
    """The seeded RAW batch of --frames: frames, label maps and integer pixel boxes of one size, and their host letterbox
    in the form `synthetic_batch` returns."""
    from PIL import Image
    from asy_vrnet_amd import data
    rng = np.random.default_rng(seed)
    frames = rng.integers(0, 256, (B, ih, iw, 3), dtype=np.uint8)
    maps = np.kron(rng.integers(0, NS + 1, (B, -(-ih // 16), -(-iw // 16))), np.ones((16, 16), dtype=np.int64))[:, :ih, :iw]
    maps = np.ascontiguousarray(maps).astype(np.uint8)
    boxes = []
    for n in rng.integers(3, 25, B):
        c = np.stack([rng.integers(iw // 8, iw - iw // 8, n), rng.integers(ih // 8, ih - ih // 8, n)], 1)
        half = np.stack([rng.integers(iw // 64 + 2, iw // 5, n), rng.integers(ih // 64 + 2, ih // 5, n)], 1)
        boxes.append(np.concatenate([c - half, c + half, rng.integers(0, NC, (n, 1))], 1).astype(np.int64))
    pil = [(Image.fromarray(f), Image.fromarray(m)) for f, m in zip(frames, maps)]

    def host_letterbox():
        imgs, labs, targets = [], [], []
        for (f, m), bx in zip(pil, boxes):
            image, box, label = data.letterbox_sample(f, m, bx, (S, S))
            imgs.append(np.array(image))
            labs.append(np.array(label))
            targets.append(torch.from_numpy(data.boxes_xyxy_to_cxcywh(box).astype(np.float32)))
        return torch.from_numpy(np.stack(imgs)), torch.from_numpy(np.stack(labs)), targets
    return torch.from_numpy(frames), torch.from_numpy(maps), boxes, host_letterbox


def captured(a):
    from asy_vrnet_amd import data
    from asy_vrnet_amd.graph import TrainStep
    dev = torch.device("cuda:0")
    B, S, NC, NS = a.batch, a.size, 4, 9
    if a.frames:
        ih, iw = (int(v) for v in a.frames.lower().split("x"))
        raw_frames, raw_maps, boxes, host_letterbox = synthetic_frames(B, ih, iw, S, NC, NS)
        img_u8, png, labels = host_letterbox()
    else:
        labels, png, img_u8 = synthetic_batch(B, S, NC, NS)
    # every contender sees the same numbers: the float forms are the device's own conversion of the bytes
    x, png_d, onehot = data.device_batch(img_u8, png.to(torch.uint8), NS, device=dev)
    _, r = A.synthetic_inputs(B, S, 1, dev)
    pin = lambda t: t.cpu().contiguous().pin_memory()
    hx, hr, hpng, honehot, hu8, hlab8 = pin(x), pin(r), pin(png_d), pin(onehot), pin(img_u8), pin(png.to(torch.uint8))
    weights = torch.ones(NS, device=dev)

    def trainer():
        model = A.EfficientVRNet(NC, NS, a.phi, img_size=(S, S)).to(dev).train()
        A.randomize_state_dict(model.state_dict(), seed=0)
        return (model, losses.YOLOLoss(NC).to(dev), optim.build_optimizer(model, "sgd", 1.25e-3, 0.937, 5e-4),
                optim.ModelEMA(model))
    model, yl, opt, ema = trainer()

    def eager_step():
        x = hx.to(dev, non_blocking=True)
        r = hr.to(dev, non_blocking=True)
        png = hpng.to(dev, non_blocking=True)
        onehot = honehot.to(dev, non_blocking=True)
        det, seg = model(x, r)
        total, ldet, lseg = losses.training_loss(yl, det, seg, labels, png, onehot, weights, NS, True, True)
        total.backward()
        opt.step()
        ema.update(model)
        opt.zero_grad()
        return total.detach()
    t1, t2 = trainer(), trainer()
    step_f = TrainStep(t1[0], t1[1], t1[2], t1[3], B, S, NS, max_gt=32, device=dev)
    step_b = TrainStep(t2[0], t2[1], t2[2], t2[3], B, S, NS, max_gt=32, from_bytes=True, device=dev)
    runs = [("eager", eager_step),
            ("TrainStep", lambda: step_f(hx, hr, labels, hpng, honehot)["total"]),
            ("TrainStep(from_bytes)", lambda: step_b(hu8, hr, labels, hlab8)["total"])]
    if a.frames:
        t3 = trainer()
        step_r = TrainStep(t3[0], t3[1], t3[2], t3[3], B, S, NS, max_gt=32, from_frames=True, capacity=(ih, iw), device=dev)
        hraw, hmaps, sizes = pin(raw_frames), pin(raw_maps), [(ih, iw)] * B

        def host_letterbox_step():
            u8, lab8, targets = host_letterbox()
            return step_b(u8, hr, targets, lab8)["total"]
        runs += [("host letterbox + from_bytes", host_letterbox_step),
                 ("TrainStep(from_frames)", lambda: step_r(hraw, hr, boxes, hmaps, sizes)["total"])]

    def window(fn, n):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(n):
            last = fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) / n * 1e3, float(last)
    steps, last = {}, {}
    for name, fn in runs:                                   # warm-up, and the number of steps that fills a window
        window(fn, 2)
        ms, _ = window(fn, 3)
        steps[name] = max(a.steps, int(math.ceil(500.0 / ms)))
    per = {name: [] for name, _ in runs}
    for _ in range(a.rounds):                               # alternating: a drift of the box hits every contender alike
        for name, fn in runs:
            ms, last[name] = window(fn, steps[name])
            per[name].append(ms)
    print(f"phi={a.phi} bs={B} {S}x{S} sgd+ema, real loss, H2D copies included: ms per step, median of {a.rounds} "
          f"alternating rounds (min .. max); device {torch.cuda.get_device_name(dev)}")
    med = {}
    for name, _ in runs:
        v = sorted(per[name])
        med[name] = float(np.median(v))
        print(f"  {name:24s} {med[name]:9.3f}  ({v[0]:.3f} .. {v[-1]:.3f})  {steps[name]} steps per round, last total loss "
              f"{last[name]:.4f}")
    for name in ("TrainStep", "TrainStep(from_bytes)"):
        print(f"  eager / {name:22s} {med['eager'] / med[name]:6.2f} x")
    if a.frames:
        fb, hl, fr = med["TrainStep(from_bytes)"], med["host letterbox + from_bytes"], med["TrainStep(from_frames)"]
        px = B * S * S
        print(f"  frames {ih} x {iw}: from_frames - from_bytes = {fr - fb:.3f} ms (the prologue and its copies: "
              f"{B * ih * iw * 4 / 1e6:.1f} MB of frames and label maps in instead of {px * 4 / 1e6:.1f} MB of letterboxed bytes, "
              f"{px * 12 / 1e6:.1f} MB of float images and {px * (8 + 4 * (NS + 1)) / 1e6:.1f} MB of targets out); "
              f"host letterbox / from_frames = {hl / fr:.2f} x; flag {step_r.stats()['flag']}")


def augmented(a):
    import json
    from asy_vrnet_amd.graph import TrainStep
    dev = torch.device("cuda:0")
    B, S, NC, NS = a.batch, a.size, 4, 9
    ih, iw = (int(v) for v in a.frames.lower().split("x"))
    raw_frames, raw_maps, boxes, _ = synthetic_frames(B, ih, iw, S, NC, NS)
    _, r = A.synthetic_inputs(B, S, 1, dev)
    pin = lambda t: t.cpu().contiguous().pin_memory()
    hraw, hmaps, hr, sizes = pin(raw_frames), pin(raw_maps), pin(r), [(ih, iw)] * B

    def trainer():
        model = A.EfficientVRNet(NC, NS, a.phi, img_size=(S, S)).to(dev).train()
        A.randomize_state_dict(model.state_dict(), seed=0)
        return (model, losses.YOLOLoss(NC).to(dev), optim.build_optimizer(model, "sgd", 1.25e-3, 0.937, 5e-4),
                optim.ModelEMA(model))
    t1, t2 = trainer(), trainer()
    kw = dict(max_gt=32, from_frames=True, capacity=(ih, iw), device=dev)
    step_r = TrainStep(t1[0], t1[1], t1[2], t1[3], B, S, NS, **kw)
    step_a = TrainStep(t2[0], t2[1], t2[2], t2[3], B, S, NS, augment=True, aug_seed=0, **kw)

    def step_window(step, n):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(n):
            last = step(hraw, hr, boxes, hmaps, sizes)["total"]
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) / n * 1e3, float(last)

    def prologue_window(step, n):
        """The prologue alone on the slots, tables and boxes the last step left: device time between two events."""
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        step._prologue()
        torch.cuda.synchronize()
        e0.record()
        for _ in range(n):
            step._prologue()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) / n
    names = ("prologue from_frames (3 launches)", "prologue augment (6 launches)", "step from_frames", "step augment")
    for step in (step_r, step_a):
        step_window(step, 3)
    ms, _ = step_window(step_r, 3)
    n_steps = max(a.steps, int(math.ceil(500.0 / ms)))
    per, last = {n: [] for n in names}, {}
    for _ in range(a.rounds):                               # alternating: a drift of the box hits every contender alike
        per[names[0]].append(prologue_window(step_r, 50))
        per[names[1]].append(prologue_window(step_a, 50))
        for name, step in ((names[2], step_r), (names[3], step_a)):
            ms, last[name] = step_window(step, n_steps)
            per[name].append(ms)
    print(f"phi={a.phi} bs={B} {S}x{S} frames {ih}x{iw} sgd+ema, real loss: ms, median of {a.rounds} alternating rounds "
          f"(min .. max); device {torch.cuda.get_device_name(dev)}")
    rec = {"tool": "bench_train_step --augment", "phi": a.phi, "batch": B, "size": S, "frames": [ih, iw], "rounds": a.rounds,
           "steps_per_round": n_steps, "max_taps": [step_r.max_taps, step_a.max_taps],
           "flag": [step_r.stats()["flag"], step_a.stats()["flag"]]}
    for name in names:
        v = sorted(per[name])
        print(f"  {name:36s} {float(np.median(v)):9.3f}  ({v[0]:.3f} .. {v[-1]:.3f})" +
              (f"  last total loss {last[name]:.4f}" if name in last else ""))
        rec[name] = {"median_ms": round(float(np.median(v)), 4), "min_ms": round(v[0], 4), "max_ms": round(v[-1], 4)}
    print(json.dumps(rec))


def mosaicked(a):
    import json
    from asy_vrnet_amd.graph import TrainStep
    dev = torch.device("cuda:0")
    B, S, NC, NS = a.batch, a.size, 4, 9
    ih, iw = (int(v) for v in a.frames.lower().split("x"))
    raw_frames, raw_maps, boxes, _ = synthetic_frames(4 * B, ih, iw, S, NC, NS)
    boxes = [bx[:8] for bx in boxes]                        # four sources of an image bring at most max_gt = 32 together
    r = torch.cat([A.synthetic_inputs(B, S, 1 + k, dev)[1] for k in range(4)])
    pin = lambda t: t.cpu().contiguous().pin_memory()
    hraw, hmaps, hr = pin(raw_frames), pin(raw_maps), pin(r)
    batch = {1: (hraw[:B], hr[:B], boxes[:B], hmaps[:B], [(ih, iw)] * B), 4: (hraw, hr, boxes, hmaps, [(ih, iw)] * 4 * B)}

    def trainer():
        model = A.EfficientVRNet(NC, NS, a.phi, img_size=(S, S)).to(dev).train()
        A.randomize_state_dict(model.state_dict(), seed=0)
        return (model, losses.YOLOLoss(NC).to(dev), optim.build_optimizer(model, "sgd", 1.25e-3, 0.937, 5e-4),
                optim.ModelEMA(model))
    t1, t2 = trainer(), trainer()
    kw = dict(max_gt=32, from_frames=True, capacity=(ih, iw), device=dev, aug_seed=0)
    step_a = TrainStep(t1[0], t1[1], t1[2], t1[3], B, S, NS, augment=True, **kw)
    step_m = TrainStep(t2[0], t2[1], t2[2], t2[3], B, S, NS, mosaic=True, **kw)

    def step_window(step, n):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(n):
            last = step(*batch[step.sources // B])["total"]
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) / n * 1e3, float(last)

    def prologue_window(step, n):
        """The prologue alone on the slots, tables and boxes the last step left: device time between two events."""
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        step._prologue()
        torch.cuda.synchronize()
        e0.record()
        for _ in range(n):
            step._prologue()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) / n
    names = ("prologue augment (6 launches)", "prologue mosaic (6 launches)", "step augment", "step mosaic")
    for step in (step_a, step_m):
        step_window(step, 3)
    ms, _ = step_window(step_a, 3)
    n_steps = max(a.steps, int(math.ceil(500.0 / ms)))
    per, last = {n: [] for n in names}, {}
    for _ in range(a.rounds):                               # alternating: a drift of the box hits every contender alike
        per[names[0]].append(prologue_window(step_a, 50))
        per[names[1]].append(prologue_window(step_m, 50))
        for name, step in ((names[2], step_a), (names[3], step_m)):
            ms, last[name] = step_window(step, n_steps)
            per[name].append(ms)
    print(f"phi={a.phi} bs={B} {S}x{S} frames {ih}x{iw} sgd+ema, real loss: ms, median of {a.rounds} alternating rounds "
          f"(min .. max); augment: {B} frames per step, mosaic: {4 * B}; device {torch.cuda.get_device_name(dev)}")
    rec = {"tool": "bench_train_step --mosaic", "phi": a.phi, "batch": B, "size": S, "frames": [ih, iw], "rounds": a.rounds,
           "steps_per_round": n_steps, "max_taps": [step_a.max_taps, step_m.max_taps],
           "workspace_bytes": [step_a._lb_ws.numel(), step_m._lb_ws.numel()],
           "flag": [step_a.stats()["flag"], step_m.stats()["flag"]]}
    for name in names:
        v = sorted(per[name])
        print(f"  {name:36s} {float(np.median(v)):9.3f}  ({v[0]:.3f} .. {v[-1]:.3f})" +
              (f"  last total loss {last[name]:.4f}" if name in last else ""))
        rec[name] = {"median_ms": round(float(np.median(v)), 4), "min_ms": round(v[0], 4), "max_ms": round(v[-1], 4)}
    print(json.dumps(rec))


def mosaic_points(a):
    import json
    from asy_vrnet_amd.graph import TrainStep
    dev = torch.device("cuda:0")
    B, S, NC, NS, N = a.batch, a.size, 4, 9, a.mosaic_points
    ih, iw = (int(v) for v in a.frames.lower().split("x"))
    raw_frames, raw_maps, boxes, _ = synthetic_frames(4 * B, ih, iw, S, NC, NS)
    boxes = [bx[:8] for bx in boxes]                        # four sources of an image bring at most max_gt = 32 together
    r = torch.cat([A.synthetic_inputs(B, S, 1 + k, dev)[1] for k in range(4)])
    pin = lambda t: t.cpu().contiguous().pin_memory()
    hraw, hmaps, hr, sizes = pin(raw_frames), pin(raw_maps), pin(r), [(ih, iw)] * 4 * B
    # a pinhole with the principal point in the middle of the frame; N points per source spread over the frame and a margin
    P = np.array([[1000.0, 0, iw / 2, 0], [0, 1000.0, ih / 2, 0], [0, 0, 1, 0]], np.float32)
    rng = np.random.default_rng(1)
    z = rng.uniform(2, 120, (4 * B, N))
    clouds = np.zeros((4 * B, N, 7), np.float32)
    clouds[..., 0] = (rng.uniform(-0.05 * iw, 1.05 * iw, (4 * B, N)) - iw / 2) * z / 1000.0
    clouds[..., 1] = (rng.uniform(-0.05 * ih, 1.05 * ih, (4 * B, N)) - ih / 2) * z / 1000.0
    clouds[..., 2] = z
    clouds[..., 3:] = rng.standard_normal((4 * B, N, 4))
    points = (clouds, np.full(4 * B, N, np.int64))          # the padded form of data.pack_points

    def trainer():
        model = A.EfficientVRNet(NC, NS, a.phi, img_size=(S, S)).to(dev).train()
        A.randomize_state_dict(model.state_dict(), seed=0)
        return (model, losses.YOLOLoss(NC).to(dev), optim.build_optimizer(model, "sgd", 1.25e-3, 0.937, 5e-4),
                optim.ModelEMA(model))
    t1, t2 = trainer(), trainer()
    kw = dict(max_gt=32, from_frames=True, capacity=(ih, iw), device=dev, aug_seed=0, mosaic=True)
    step_m = TrainStep(t1[0], t1[1], t1[2], t1[3], B, S, NS, **kw)
    step_p = TrainStep(t2[0], t2[1], t2[2], t2[3], B, S, NS, radar_points=N, radar_radius=a.radius, calib=P, **kw)
    radar = {id(step_m): hr, id(step_p): points}

    def step_window(step, n):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(n):
            last = step(hraw, radar[id(step)], boxes, hmaps, sizes)["total"]
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) / n * 1e3, float(last)

    def prologue_window(step, n):
        """The prologue alone on the slots, tables, boxes and radar inputs the last step left: device time between two events."""
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        step._prologue()
        torch.cuda.synchronize()
        e0.record()
        for _ in range(n):
            step._prologue()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) / n

    def pack_window(n):
        """The host's share of the points path alone: validation and packing into the pinned staging tensor."""
        t0 = time.perf_counter()
        for _ in range(n):
            step_p.radar_points.validate(points, None)
        return (time.perf_counter() - t0) / n * 1e3
    names = ("prologue mosaic, maps (6 launches)", "prologue mosaic, points (8 launches)", "step mosaic, maps", "step mosaic, points",
             "host packing of the points")
    for step in (step_m, step_p):
        step_window(step, 3)
    ms, _ = step_window(step_m, 3)
    n_steps = max(a.steps, int(math.ceil(500.0 / ms)))
    per, last = {n: [] for n in names}, {}
    for _ in range(a.rounds):                               # alternating: a drift of the box hits every contender alike
        per[names[0]].append(prologue_window(step_m, 50))
        per[names[1]].append(prologue_window(step_p, 50))
        for name, step in ((names[2], step_m), (names[3], step_p)):
            ms, last[name] = step_window(step, n_steps)
            per[name].append(ms)
        per[names[4]].append(pack_window(10))
    lit = int((step_p.r != 0).any(dim=1).sum())
    print(f"phi={a.phi} bs={B} {S}x{S} frames {ih}x{iw} sgd+ema, real loss: ms, median of {a.rounds} alternating rounds "
          f"(min .. max); {4 * B} sources per step, {N} points per source, radius {a.radius}; device {torch.cuda.get_device_name(dev)}")
    rec = {"tool": "bench_train_step --mosaic-points", "phi": a.phi, "batch": B, "size": S, "frames": [ih, iw], "rounds": a.rounds,
           "steps_per_round": n_steps, "points": N, "radius": a.radius, "radar_bytes_per_step": [hr.numel() * 4, clouds.nbytes + 4 * B * 56],
           "lit_pixels_last_step": lit, "flag": [step_m.stats()["flag"], step_p.stats()["flag"]]}
    for name in names:
        v = sorted(per[name])
        print(f"  {name:40s} {float(np.median(v)):9.3f}  ({v[0]:.3f} .. {v[-1]:.3f})" +
              (f"  last total loss {last[name]:.4f}" if name in last else ""))
        rec[name] = {"median_ms": round(float(np.median(v)), 4), "min_ms": round(v[0], 4), "max_ms": round(v[-1], 4)}
    print(json.dumps(rec))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--phi", default="l")
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--size", type=int, default=512)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--captured", action="store_true", help="eager loop against graph.TrainStep, alternating rounds")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--frames", default=None, metavar="IHxIW",
                    help="with --captured: raw frames of this size; adds the host-letterbox and the from_frames contenders")
    ap.add_argument("--augment", action="store_true",
                    help="with --frames: the augmented prologue and step against the plain frame path, alternating rounds")
    ap.add_argument("--mosaic", action="store_true",
                    help="with --frames: the Mosaic prologue and step against the augmented frame path, alternating rounds")
    ap.add_argument("--mosaic-points", type=int, default=None, metavar="N",
                    help="with --frames: the Mosaic step fed N radar points per source against the one fed finished maps")
    ap.add_argument("--radius", type=int, default=0, help="with --mosaic-points: the footprint radius of a point")
    a = ap.parse_args()
    if a.mosaic_points:
        if not a.frames:
            ap.error("--mosaic-points needs --frames IHxIW")
        return mosaic_points(a)
    if a.mosaic:
        if not a.frames:
            ap.error("--mosaic needs --frames IHxIW")
        return mosaicked(a)
    if a.augment:
        if not a.frames:
            ap.error("--augment needs --frames IHxIW")
        return augmented(a)
    if a.captured:
        return captured(a)
    dev = torch.device("cuda:0")
    B, S, NC, NS = a.batch, a.size, 4, 9
    model = A.EfficientVRNet(NC, NS, a.phi, img_size=(S, S)).to(dev).train()
    A.randomize_state_dict(model.state_dict(), seed=0)
    yl = losses.YOLOLoss(NC).to(dev)
    opt = optim.build_optimizer(model, "sgd", 1.25e-3, 0.937, 5e-4)
    ema = optim.ModelEMA(model)
    rng = np.random.default_rng(0)
    x, r = A.synthetic_inputs(B, S, 1, dev)
    labels = [torch.from_numpy(np.concatenate([rng.uniform(60, S - 60, (n, 2)), rng.uniform(16, 200, (n, 2)),
                                               rng.integers(0, NC, (n, 1))], 1).astype(np.float32))
              for n in rng.integers(3, 25, B)]
    png = torch.from_numpy(np.kron(rng.integers(0, NS + 1, (B, S // 16, S // 16)), np.ones((16, 16), dtype=np.int64))).to(dev)
    onehot = torch.nn.functional.one_hot(png, NS + 1).float()
    weights = torch.ones(NS, device=dev)
    ev = lambda: torch.cuda.Event(enable_timing=True)
    names = ["forward", "loss (value + head grads)", "backward", "sgd step", "ema update"]
    tot = dict.fromkeys(names, 0.0)
    for it in range(a.steps + 2):
        marks = [ev() for _ in range(6)]
        marks[0].record()
        det, seg = model(x, r)
        marks[1].record()
        total, ldet, lseg = losses.training_loss(yl, det, seg, labels, png, onehot, weights, NS, True, True)
        marks[2].record()
        total.backward()
        marks[3].record()
        opt.step()
        marks[4].record()
        ema.update(model)
        marks[5].record()
        opt.zero_grad()
        torch.cuda.synchronize()
        if it >= 2:
            for i, n in enumerate(names):
                tot[n] += marks[i].elapsed_time(marks[i + 1])
    print(f"phi={a.phi} bs={B} {S}x{S}: loss_det={ldet.item():.4f} loss_seg={lseg.item():.4f} (eager, ms per step)")
    for n in names:
        print(f"  {n:28s} {tot[n] / a.steps:8.3f}")
    print(f"  {'sum':28s} {sum(tot.values()) / a.steps:8.3f}")


if __name__ == "__main__":
    main()
