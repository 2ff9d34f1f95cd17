"""Times the radar readout of the detections (vrnet_box_radar_f32) on one GPU, in one process:

  1. device time per captured replay of the two launches at --batch frames of --frame with --points points per frame and
     --boxes kept boxes per image (two events around --steps replays of a graph that holds the one call), beside what a caller
     does without the stage: the blocking read-back `FrameResult.detections()` plus the numpy rule `data.box_radar` per image
     on the host (host clock), rounds alternating between the two;
  2. FramePipeline.run() with and without the stage (box_radar=True), host clock over --steps calls ending in a synchronise,
     rounds alternating between the two pipelines.

    python tools/bench_box_radar.py --batch 8 --points 4096 --boxes 100 --frame 480x640

Medians (min .. max) of --rounds alternating rounds; the last line is one JSON record.
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import asy_vrnet_amd as A  # noqa: E402
from asy_vrnet_amd import data, hip, infer  # noqa: E402


def camera(size, f=0.9):
    ih, iw = size
    K = np.array([[f * iw, 0, iw / 2], [0, f * iw, ih / 2], [0, 0, 1]])
    return (K @ np.concatenate([np.eye(3), np.array([[0.3], [-0.2], [0.5]])], 1)).astype(np.float32)


def cloud(seed, n):
    rs = np.random.RandomState(seed)
    z = rs.uniform(1, 60, n)
    xy = rs.uniform(-0.6, 0.6, (n, 2)) * z[:, None]
    return np.concatenate([xy, z[:, None], rs.randn(n, 4)], 1).astype(np.float32)


def random_rows(seed, n, frame):
    """n boxes of 5 .. 40 % of the frame's sides, as FrameResult.rows has them."""
    rs = np.random.RandomState(seed)
    ih, iw = frame
    hw = rs.uniform(0.05, 0.4, (n, 2)) * (ih, iw)
    tl = rs.uniform(0, 1, (n, 2)) * ((ih, iw) - hw)
    return np.concatenate([tl, tl + hw, rs.uniform(0.5, 1, (n, 2)), rs.randint(0, 4, (n, 1))], 1).astype(np.float32)


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


def stats(rounds):
    return {"median_ms": round(statistics.median(rounds), 5), "min_ms": round(min(rounds), 5), "max_ms": round(max(rounds), 5)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--size", type=int, default=512)
    ap.add_argument("--points", type=int, default=4096)
    ap.add_argument("--boxes", type=int, default=100)
    ap.add_argument("--frame", default="480x640")
    ap.add_argument("--phi", default="nano")
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--host-steps", type=int, default=3, help="calls per round of the host path, which takes milliseconds each")
    ap.add_argument("--rounds", type=int, default=5)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_box_radar: needs a GPU; nothing is measured without one")
    B, S, N, M = args.batch, args.size, args.points, args.boxes
    frame = tuple(int(v) for v in args.frame.split("x"))
    P = camera(frame)
    pts = [cloud(b, N) for b in range(B)]
    table = data.frame_geometry([frame] * B, (S, S))
    packed, counts = data.pack_points(pts, N)
    points_d = packed.cuda()
    views_d = data.radar_view_bytes(data.radar_views(table, P, counts.numpy())).cuda()
    rows_h = np.stack([random_rows(100 + b, M, frame) for b in range(B)])
    rows_d, kept_d = torch.from_numpy(rows_h).cuda(), torch.full((B,), M, dtype=torch.int32, device="cuda")
    counts_d = torch.empty((B, M), dtype=torch.int32, device="cuda")
    readout_d = torch.empty((B, M, 2, 5), device="cuda")
    ws = torch.empty(hip.box_radar_workspace_bytes(B, N), dtype=torch.uint8, device="cuda")
    result = infer.FrameResult(rows_d, kept_d, None, None, None, None, None)

    def call():
        hip.box_radar(points_d, views_d, rows_d, kept_d, 0.1, 1.0, counts_d, readout_d, ws=ws)

    def on_the_host():
        return [data.box_radar(pts[b], P, frame, d) for b, d in enumerate(result.detections())]
    stream = torch.cuda.Stream()
    with torch.cuda.stream(stream):
        for _ in range(2):
            call()
        torch.cuda.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=stream):
            call()
        graph.replay()
        torch.cuda.synchronize()
        want = on_the_host()
        same = all(np.array_equal(counts_d[b].cpu().numpy(), c) and
                   np.array_equal(readout_d[b].cpu().numpy().view(np.uint32), r.view(np.uint32)) for b, (c, r) in enumerate(want))
        inside = int(counts_d.sum())
        times = {"device": [], "host": []}
        for _ in range(args.rounds):
            times["device"].append(device_ms(graph.replay, args.steps))
            times["host"].append(host_ms(on_the_host, args.host_steps))
    torch.cuda.synchronize()
    print(f"radar readout of the detections, bs={B}, frames {frame[0]}x{frame[1]}, {N} points per frame, {M} kept boxes per image "
          f"({inside} (point, box) members; equals data.box_radar: {same}); median of {args.rounds} alternating rounds; device "
          f"{torch.cuda.get_device_name(0)}")
    print(f"  vrnet_box_radar_f32, device time per captured replay ({args.steps} a round): {summary(times['device'])}")
    print(f"  detections() + data.box_radar per image on the host, host clock ({args.host_steps} a round): {summary(times['host'])}")

    model = A.EfficientVRNet(4, 9, args.phi, img_size=S).cuda().eval()
    A.randomize_state_dict(model.state_dict(), seed=0)
    kw = dict(batch=B, conf_thres=0.5, nms_thres=0.4, graph=True, radar_points=N, calib=P)
    frames = torch.from_numpy(np.random.default_rng(0).integers(0, 256, (B,) + frame + (3,), dtype=np.uint8)).pin_memory()
    without = A.FramePipeline(model, frame, (S, S), **kw)
    with_stage = A.FramePipeline(model, frame, (S, S), box_radar=True, **kw)
    runs = {"without the stage": lambda: without.run(frames, pts), "with box_radar": lambda: with_stage.run(frames, pts)}
    rounds = {k: [] for k in runs}
    for k in runs:
        host_ms(runs[k], 3)
    for _ in range(args.rounds):
        for k in runs:
            rounds[k].append(host_ms(runs[k], args.steps))
    a = without.run(frames, pts).rows.clone()
    b = with_stage.run(frames, pts)
    print(f"FramePipeline phi={args.phi} {S}x{S} bs={B}, frames {frame[0]}x{frame[1]}, host clock per run() incl. its copies, median "
          f"of {args.rounds} alternating rounds of {args.steps}; rows equal: {torch.equal(a, b.rows)}; kept {b.kept.tolist()}")
    for k in runs:
        print(f"  {k}: {summary(rounds[k])}")
    rec = {"tool": "bench_box_radar", "batch": B, "size": S, "points": N, "boxes": M, "frame": list(frame), "rounds": args.rounds,
           "steps": args.steps, "host_steps": args.host_steps, "equals_host": bool(same), "members": inside,
           "device": torch.cuda.get_device_name(0), "replay": stats(times["device"]), "host_path": stats(times["host"]),
           "pipeline_without": stats(rounds["without the stage"]), "pipeline_with": stats(rounds["with box_radar"])}
    print(json.dumps(rec))


if __name__ == "__main__":
    main()
