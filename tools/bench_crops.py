"""Times the detection crops (vrnet_crop_boxes_u8: the layout and the copy launch) on one GPU, in one process:

  1. device time per captured replay of the two launches alone at --batch frames of --frame with --boxes boxes of about
     --box pixels per image, n_cap = batch x --cap rows as a FramePipeline has them (two events around --steps replays of a
     graph that holds the one call; median of --rounds rounds).  With the diagnostic library (make -C asy-vrnet_amd/csrc
     tuning; VRNET_HIP_LIB=.../libvrnet_hip_tuning.so) the same for every workgroup count per row of --sweep, the rounds
     alternating between the counts; the product library has the one count that is compiled in;
  2. FramePipeline.run() built with crops=None and with crops=True, host clock over --steps calls ending in a synchronise,
     rounds alternating between the two pipelines.

    python tools/bench_crops.py --batch 8 --frame 1080x1920 --boxes 20 --box 200x300
"""
import argparse
import os
import statistics
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import asy_vrnet_amd as A  # noqa: E402
from asy_vrnet_amd import hip, render  # noqa: E402


def device_ms(fn, steps):
    start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    for _ in range(steps):
        fn()
    end.record()
    end.synchronize()
    return start.elapsed_time(end) / steps


def host_ms(fn, steps):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3 / steps


def summary(rounds):
    return f"{statistics.median(rounds):.4f} ms (rounds {min(rounds):.4f}..{max(rounds):.4f})"


def boxes(rng, B, n, frame, box):
    """(B * n, 5) int32 draw rows of about box = (h, w) pixels inside the frame, and their offsets."""
    (ih, iw), (bh, bw) = frame, box
    h = np.clip(rng.integers(bh * 3 // 4, bh * 5 // 4 + 1, B * n), 1, ih)
    w = np.clip(rng.integers(bw * 3 // 4, bw * 5 // 4 + 1, B * n), 1, iw)
    top, left = rng.integers(0, ih - h + 1), rng.integers(0, iw - w + 1)
    rows = np.stack([left, top, left + w, top + h, rng.integers(0, 4, B * n)], 1).astype(np.int32)
    return rows, (np.arange(B + 1) * n).astype(np.int32)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--frame", default="1080x1920")
    ap.add_argument("--boxes", type=int, default=20)
    ap.add_argument("--box", default="200x300")
    ap.add_argument("--cap", type=int, default=1024, help="rows per image of the table, as FramePipeline's max_candidates")
    ap.add_argument("--sweep", default="1,2,4,8,16,32")
    ap.add_argument("--size", type=int, default=512)
    ap.add_argument("--phi", default="nano")
    ap.add_argument("--conf", type=float, default=0.5)
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--rounds", type=int, default=5)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_crops: needs a GPU; nothing is measured without one")
    B, S = args.batch, args.size
    frame, box = (tuple(int(v) for v in t.split("x")) for t in (args.frame, args.box))
    rng = np.random.default_rng(0)
    frames_h = torch.from_numpy(rng.integers(0, 256, (B,) + frame + (3,), dtype=np.uint8)).pin_memory()
    rows_h, offsets_h = boxes(rng, B, args.boxes, frame, box)
    n_cap = B * args.cap
    rows_d = torch.zeros((n_cap, 5), dtype=torch.int32, device="cuda")
    rows_d[:len(rows_h)] = torch.from_numpy(rows_h)
    frames_d, offsets_d = frames_h.cuda(), torch.from_numpy(offsets_h).cuda()
    flag = torch.zeros(1, dtype=torch.int32, device="cuda")
    crops = render.crop_buffers(n_cap, 2 * B * frame[0] * frame[1], B, flag, "cuda")
    table, (N, used), _ = render.crop_layout(rows_h, offsets_h, frame, crops.arena.numel() // 3)

    def call():
        hip.crop_boxes(frames_d, rows_d, offsets_d, crops.arena, crops.table, crops.summary, flag=flag)
    counts = [int(v) for v in args.sweep.split(",")] if hip.tuning_build() else [None]
    stream = torch.cuda.Stream()
    graphs, times = {}, {x: [] for x in counts}
    with torch.cuda.stream(stream):
        for x in counts:
            if x is not None:
                os.environ["VRNET_CROP_X"] = str(x)         # read by the diagnostic library at every call
            for _ in range(2):
                call()
            torch.cuda.synchronize()
            graphs[x] = torch.cuda.CUDAGraph()
            with torch.cuda.graph(graphs[x], stream=stream):
                call()
            crops.arena.zero_()
            graphs[x].replay()
            torch.cuda.synchronize()
            got = crops.images()
            same = crops.summary.tolist() == [N, used] and all(
                np.array_equal(c, w) for c, w in zip([c for g in got for c in g], [
                    w for b in range(B) for w in render.crop_boxes_host(frames_h[b].numpy(), rows_h[offsets_h[b]:offsets_h[b + 1]])]))
            if not same:
                raise SystemExit(f"bench_crops: the crops differ from render.crop_boxes_host (workgroups per row: {x})")
        for _ in range(args.rounds):
            for x in counts:
                times[x].append(device_ms(graphs[x].replay, args.steps))
    torch.cuda.synchronize()
    os.environ.pop("VRNET_CROP_X", None)
    mb = 3 * used / 1e6
    print(f"detection crops, bs={B}, frames {frame[0]}x{frame[1]}, {args.boxes} boxes of about {box[0]}x{box[1]} per image, "
          f"{N} rows in a table of {n_cap}, {mb:.1f} MB of crops (equal to render.crop_boxes_host), "
          f"{'diagnostic' if hip.tuning_build() else 'product'} library; device time per captured replay of the two launches, "
          f"median of {args.rounds} rounds of {args.steps}:")
    for x in counts:
        med = statistics.median(times[x])
        print(f"  workgroups per row {'as compiled' if x is None else x}: {summary(times[x])}, {2 * mb / med:.1f} GB/s read + written")
    if hip.tuning_build():
        return                                        # the pipelines are timed on the product library

    model = A.EfficientVRNet(4, 9, args.phi, img_size=S).cuda().eval()
    A.randomize_state_dict(model.state_dict(), seed=0)
    kw = dict(batch=B, conf_thres=args.conf, nms_thres=0.4, graph=True)
    radar = torch.from_numpy(rng.standard_normal((B, 4, S, S)).astype(np.float32)).pin_memory()
    pipes = {"crops=None": A.FramePipeline(model, frame, (S, S), **kw), "crops=True": A.FramePipeline(model, frame, (S, S), crops=True, **kw)}
    runs = {k: (lambda p=p: p.run(frames_h, radar)) for k, p in pipes.items()}
    rounds = {k: [] for k in runs}
    for k in runs:
        host_ms(runs[k], 3)
    for _ in range(args.rounds):
        for k in runs:
            rounds[k].append(host_ms(runs[k], args.steps))
    a, b = (pipes[k].run(frames_h, radar) for k in pipes)
    torch.cuda.synchronize()
    print(f"FramePipeline phi={args.phi} {S}x{S} bs={B} conf {args.conf}, frames {frame[0]}x{frame[1]}, host clock per run() incl. its copies, median "
          f"of {args.rounds} alternating rounds of {args.steps}; {int(b.kept.sum())} detections, {int(b.crops.summary[1])} pixels of "
          f"crops; rows and rendered equal: {torch.equal(a.rows, b.rows) and torch.equal(a.rendered, b.rendered)}")
    for k in runs:
        print(f"  {k}: {summary(rounds[k])}")


if __name__ == "__main__":
    main()
