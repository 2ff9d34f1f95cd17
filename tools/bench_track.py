"""Times the tracker of the detections (vrnet_track_update_f32) on one GPU, in one process:

  1. device time per captured replay of the one launch at --batch streams with --boxes kept rows per stream and a table of
     --tracks slots (two events around --steps replays of a graph that holds the one call; the state persists across the
     replays, so after the first the same --live tracks are matched every time), beside what a caller does without the stage:
     the blocking read-back `FrameResult.detections()` plus the numpy rule `data.track_update` on the host (host clock),
     rounds alternating between the two.  Two scenes: `sparse`, --live valid boxes among the kept rows, the rest reduced to a
     line (bottom == top, as the clip at the frame's border leaves them), which neither match nor start a track; `full`,
     every kept row a valid box, so that the table is full, every slot matched and the other rows look for a slot in vain;
  2. FramePipeline.run() with and without the stage (track=True), host clock over --steps calls ending in a synchronise,
     rounds alternating between the two pipelines.

    python tools/bench_track.py --batch 8 --boxes 100 --tracks 64 --live 30 --frame 480x640

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
from tools.bench_box_radar import camera, cloud, device_ms, host_ms, random_rows, stats, summary  # noqa: E402


def scene_rows(seed, n, valid, frame):
    """n rows of which the first `valid`, shuffled among the others, are boxes; the rest have bottom == top."""
    rows = random_rows(seed, n, frame)
    order = np.random.RandomState(seed).permutation(n)
    rows[order[valid:], 2] = rows[order[valid:], 0]
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--size", type=int, default=512)
    ap.add_argument("--points", type=int, default=4096)
    ap.add_argument("--boxes", type=int, default=100)
    ap.add_argument("--tracks", type=int, default=64)
    ap.add_argument("--live", type=int, default=30)
    ap.add_argument("--frame", default="480x640")
    ap.add_argument("--phi", default="nano")
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--host-steps", type=int, default=3, help="calls per round of the host path, which takes milliseconds each")
    ap.add_argument("--rounds", type=int, default=5)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_track: needs a GPU; nothing is measured without one")
    B, S, M, T = args.batch, args.size, args.boxes, args.tracks
    frame = tuple(int(v) for v in args.frame.split("x"))
    params = data.check_track_params(dict(max_tracks=T))
    i32 = dict(dtype=torch.int32, device="cuda")
    rec = {"tool": "bench_track", "batch": B, "size": S, "boxes": M, "tracks": T, "live": args.live, "frame": list(frame),
           "rounds": args.rounds, "steps": args.steps, "host_steps": args.host_steps, "device": torch.cuda.get_device_name(0)}
    print(f"tracker of the detections, bs={B}, {M} kept rows per stream, table of {T}; median of {args.rounds} alternating rounds; "
          f"device {torch.cuda.get_device_name(0)}")
    for name, valid in (("sparse", args.live), ("full", M)):
        rows_h = np.stack([scene_rows(100 + b, M, valid, frame) for b in range(B)])
        rows_d, kept_d = torch.from_numpy(rows_h).cuda(), torch.full((B,), M, **i32)
        bp_d = torch.full((B, M), 3, **i32)
        br_d = torch.from_numpy(np.random.RandomState(1).uniform(5, 100, (B, M, 2, 5)).astype(np.float32)).cuda()
        table_d, head_d, ids_d = torch.zeros((B, T, 16), **i32), torch.zeros((B, 4), **i32), torch.zeros((B, M), **i32)
        flag_d = torch.zeros(1, **i32)
        result = infer.FrameResult(rows_d, kept_d, None, None, None, None, None)
        host = [np.zeros((B, T), data.TRACK_DTYPE), np.zeros((B, 4), np.int32)]
        bp_h, br_h = bp_d.cpu().numpy(), br_d.cpu().numpy()

        def call():
            hip.track_update(rows_d, kept_d, table_d, head_d, ids_d, params, box_points=bp_d, box_radar=br_d, flag=flag_d)

        def on_the_host():
            dets = result.detections()
            rows = np.zeros((B, M, 7), np.float32)
            for b, d in enumerate(dets):
                rows[b, :len(d)] = d
            host[0], host[1], ids, _ = data.track_update(host[0], host[1], rows, np.array([len(d) for d in dets], np.int32), bp_h,
                                                         br_h, params)
            return ids
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
            for _ in range(3):                              # the host state through the same three calls (the capture runs none)
                want_ids = on_the_host()
            same = np.array_equal(np.frombuffer(table_d.cpu().numpy().tobytes(), np.int32),
                                  np.frombuffer(host[0].tobytes(), np.int32)) and \
                np.array_equal(head_d.cpu().numpy(), host[1]) and np.array_equal(ids_d.cpu().numpy(), want_ids)
            live = head_d[:, 1].tolist()
            times = {"device": [], "host": []}
            for _ in range(args.rounds):
                times["device"].append(device_ms(graph.replay, args.steps))
                times["host"].append(host_ms(on_the_host, args.host_steps))
        torch.cuda.synchronize()
        print(f" scene `{name}`: {valid} valid boxes among the {M} rows of a stream; live tracks per stream {live}; flag "
              f"{int(flag_d.item())}; equals data.track_update after three calls: {same}")
        print(f"  vrnet_track_update_f32, device time per captured replay ({args.steps} a round): {summary(times['device'])}")
        print(f"  detections() + data.track_update on the host, host clock ({args.host_steps} a round): {summary(times['host'])}")
        rec[name] = {"valid": valid, "live": live, "equals_host": bool(same), "replay": stats(times["device"]),
                     "host_path": stats(times["host"])}

    N = args.points
    P = camera(frame)
    pts = [cloud(b, N) for b in range(B)]
    model = A.EfficientVRNet(4, 9, args.phi, img_size=S).cuda().eval()
    A.randomize_state_dict(model.state_dict(), seed=0)
    kw = dict(batch=B, conf_thres=0.5, nms_thres=0.4, graph=True, radar_points=N, calib=P, box_radar=True)
    frames = torch.from_numpy(np.random.default_rng(0).integers(0, 256, (B,) + frame + (3,), dtype=np.uint8)).pin_memory()
    without = A.FramePipeline(model, frame, (S, S), **kw)
    with_stage = A.FramePipeline(model, frame, (S, S), track=dict(max_tracks=T), **kw)
    runs = {"without the stage": lambda: without.run(frames, pts), "with track": lambda: with_stage.run(frames, pts)}
    rounds = {k: [] for k in runs}
    for k in runs:
        host_ms(runs[k], 3)
    for _ in range(args.rounds):
        for k in runs:
            rounds[k].append(host_ms(runs[k], args.steps))
    a = without.run(frames, pts).rows.clone()
    b = with_stage.run(frames, pts)
    print(f"FramePipeline phi={args.phi} {S}x{S} bs={B}, frames {frame[0]}x{frame[1]}, box_radar on, host clock per run() incl. its "
          f"copies, median of {args.rounds} alternating rounds of {args.steps}; rows equal: {torch.equal(a, b.rows)}; kept "
          f"{b.kept.tolist()}; live tracks {b.track_head[:, 1].tolist()}")
    for k in runs:
        print(f"  {k}: {summary(rounds[k])}")
    rec.update(pipeline_without=stats(rounds["without the stage"]), pipeline_with=stats(rounds["with track"]),
               pipeline_kept=b.kept.tolist(), pipeline_live=b.track_head[:, 1].tolist())
    print(json.dumps(rec))


if __name__ == "__main__":
    main()
