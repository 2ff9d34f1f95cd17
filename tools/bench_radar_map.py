"""Times the radar map from points (vrnet_radar_map_f32) against what it replaces, on one GPU, in one process:

  1. device time per captured replay of the three launches at --batch x --size^2 with --points points per frame, for every
     radius of --radii (two events around --steps replays of a graph that holds the one call; median of --rounds rounds);
  2. in the same rounds, the host-to-device copy of the (B, 4, S, S) float32 maps the call replaces, from pinned memory, and the
     copy of the points and the view table it needs instead;
  3. FramePipeline.run() fed maps (the path without radar_points) and fed points, host clock over --steps calls ending in a
     synchronise, rounds alternating between the two pipelines.

    python tools/bench_radar_map.py --batch 8 --size 512 --points 4096 --radii 0,2 --frame 480x640

--post times the radar map under the rotation of the post stage instead (vrnet_radar_map_post_f32), the same way (1): per radius,
in alternating rounds, a captured replay of vrnet_radar_map_f32, of vrnet_radar_map_post_f32 with no record rotating, of the same
with every record rotating by +-10 degrees, and of what a finished map needs instead: vrnet_radar_map_f32 followed by the nearest
gather vrnet_augment_post_radar_f32 on those records.  The last line is one JSON record.

    python tools/bench_radar_map.py --post --batch 8 --size 512 --points 4096 --radii 0,2 --frame 480x640 --steps 1000
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
from asy_vrnet_amd import data, hip  # noqa: E402


def camera(size, f=0.9):
    ih, iw = size
    K = np.array([[f * iw, 0, iw / 2], [0, f * iw, ih / 2], [0, 0, 1]])
    return (K @ np.concatenate([np.eye(3), np.array([[0.3], [-0.2], [0.5]])], 1)).astype(np.float32)


def cloud(seed, n):
    rs = np.random.RandomState(seed)
    z = rs.uniform(1, 60, n)
    xy = rs.uniform(-0.6, 0.6, (n, 2)) * z[:, None]
    return np.concatenate([xy, z[:, None], rs.randn(n, 4)], 1).astype(np.float32)


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


def post_main(args):
    import json
    B, S, N = args.batch, args.size, args.points
    frame = tuple(int(v) for v in args.frame.split("x"))
    radii = [int(r) for r in args.radii.split(",")]
    P = camera(frame)
    pts = [cloud(b, N) for b in range(B)]
    table = data.frame_geometry([frame] * B, (S, S))
    packed, counts = data.pack_points(pts, N)
    points_d = packed.cuda()
    views_d = data.radar_view_bytes(data.radar_views(table, P, counts.numpy())).cuda()
    off = np.stack([data.aug_post_record((S, S), False, 0)] * B)
    on = np.stack([data.aug_post_record((S, S), False, 10 if b % 2 else -10) for b in range(B)])
    tabs = {"off": data.aug_post_bytes(off).cuda(), "on": data.aug_post_bytes(on).cuda()}
    out, mid = torch.empty((B, 4, S, S), device="cuda"), torch.empty((B, 4, S, S), device="cuda")
    ws = torch.empty(hip.radar_map_workspace_bytes(B, S, S), dtype=torch.uint8, device="cuda")
    calls = {"vrnet_radar_map_f32": lambda r: hip.radar_map(points_d, views_d, S, S, r, 0.1, out, ws=ws),
             "vrnet_radar_map_post_f32, no record rotates": lambda r: hip.radar_map_post(points_d, views_d, tabs["off"], S, S, r, 0.1, 10, out, ws=ws),
             "vrnet_radar_map_post_f32, every record +-10": lambda r: hip.radar_map_post(points_d, views_d, tabs["on"], S, S, r, 0.1, 10, out, ws=ws),
             "vrnet_radar_map_f32 + vrnet_augment_post_radar_f32, +-10": lambda r: (
                 hip.radar_map(points_d, views_d, S, S, r, 0.1, mid, ws=ws), hip.augment_post_radar(mid, tabs["on"], 10, out=out))}
    stream = torch.cuda.Stream()
    graphs, lit = {}, {}
    with torch.cuda.stream(stream):
        for r in radii:
            for name, fn in calls.items():
                for _ in range(2):
                    fn(r)
                torch.cuda.synchronize()
                graphs[name, r] = torch.cuda.CUDAGraph()
                with torch.cuda.graph(graphs[name, r], stream=stream):
                    fn(r)
                graphs[name, r].replay()
                torch.cuda.synchronize()
                lit[name, r] = int((out != 0).any(1).sum())
        # image 0 at the first radius against the host rule, bit for bit
        graphs["vrnet_radar_map_post_f32, every record +-10", radii[0]].replay()
        torch.cuda.synchronize()
        want = data.radar_map(pts[0], P, frame, (S, S), data.letterbox_geometry(frame[1], frame[0], S, S), False, radii[0], 0.1, post=on[0])
        same = bool(np.array_equal(out[0].cpu().numpy().view(np.uint32), want.view(np.uint32)))
        times = {k: [] for k in graphs}
        for _ in range(args.rounds):                        # alternating: a drift of the box hits every contender alike
            for k in graphs:
                times[k].append(device_ms(graphs[k].replay, args.steps))
    torch.cuda.synchronize()
    print(f"radar map from points under a rotation, bs={B}, {S}x{S}, {N} points per frame, frames {frame[0]}x{frame[1]}; image 0 at radius "
          f"{radii[0]} equals data.radar_map(..., post=): {same}; device time per captured replay, median of {args.rounds} alternating "
          f"rounds of {args.steps}; device {torch.cuda.get_device_name(0)}")
    rec = {"tool": "bench_radar_map --post", "batch": B, "size": S, "points": N, "frame": list(frame), "rounds": args.rounds,
           "steps": args.steps, "equals_host": same}
    for (name, r), v in times.items():
        print(f"  radius {r}  {name:58s} {summary(v)}  {lit[name, r]} pixels lit")
        rec[f"radius {r}: {name}"] = {"median_ms": round(statistics.median(v), 5), "min_ms": round(min(v), 5), "max_ms": round(max(v), 5),
                                      "lit": lit[name, r]}
    print(json.dumps(rec))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--size", type=int, default=512)
    ap.add_argument("--points", type=int, default=4096)
    ap.add_argument("--radii", default="0,2")
    ap.add_argument("--frame", default="480x640")
    ap.add_argument("--phi", default="nano")
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--post", action="store_true", help="the map under the rotation of the post stage against the plain map and the gather")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_radar_map: needs a GPU; nothing is measured without one")
    if args.post:
        return post_main(args)
    B, S, N = args.batch, args.size, args.points
    frame = tuple(int(v) for v in args.frame.split("x"))
    radii = [int(r) for r in args.radii.split(",")]
    P = camera(frame)
    pts = [cloud(b, N) for b in range(B)]
    table = data.frame_geometry([frame] * B, (S, S))
    packed, counts = data.pack_points(pts, N)
    views_h = data.radar_view_bytes(data.radar_views(table, P, counts.numpy())).pin_memory()
    maps_h = torch.from_numpy(np.stack([data.radar_map(p, P, frame, (S, S), data.letterbox_geometry(frame[1], frame[0], S, S))
                                        for p in pts])).pin_memory()
    points_d, views_d = packed.cuda(), views_h.cuda()
    out = torch.empty((B, 4, S, S), device="cuda")
    ws = torch.empty(hip.radar_map_workspace_bytes(B, S, S), dtype=torch.uint8, device="cuda")
    stream = torch.cuda.Stream()
    graphs = {}
    with torch.cuda.stream(stream):
        for r in radii:
            for _ in range(2):
                hip.radar_map(points_d, views_d, S, S, r, 0.1, out, ws=ws)
            torch.cuda.synchronize()
            graphs[r] = torch.cuda.CUDAGraph()
            with torch.cuda.graph(graphs[r], stream=stream):
                hip.radar_map(points_d, views_d, S, S, r, 0.1, out, ws=ws)
        graphs[radii[0]].replay()
        torch.cuda.synchronize()
        lit = int((out != 0).any(1).sum())
        same = torch.equal(out.cpu().view(torch.int32), maps_h.view(torch.int32)) if radii[0] == 0 else None
        maps_d = torch.empty_like(out)

        def copy_maps():
            maps_d.copy_(maps_h, non_blocking=True)

        def copy_points():
            points_d.copy_(packed, non_blocking=True)
            views_d.copy_(views_h, non_blocking=True)
        times = {("map", r): [] for r in radii}
        times["copy_maps"], times["copy_points"] = [], []
        for fn in (copy_maps, copy_points):
            device_ms(fn, 3)
        for _ in range(args.rounds):
            for r in radii:
                times[("map", r)].append(device_ms(graphs[r].replay, args.steps))
            times["copy_maps"].append(device_ms(copy_maps, args.steps))
            times["copy_points"].append(device_ms(copy_points, args.steps))
    torch.cuda.synchronize()
    mb = maps_h.numel() * 4 / 1e6
    print(f"radar map from points, bs={B}, {S}x{S}, {N} points per frame ({lit} pixels lit at radius {radii[0]}; equals "
          f"data.radar_map: {same}), device time per captured replay, median of {args.rounds} rounds of {args.steps}:")
    for r in radii:
        print(f"  vrnet_radar_map_f32 radius {r}: {summary(times[('map', r)])}")
    med = statistics.median(times["copy_maps"])
    print(f"  host-to-device copy of the {mb:.1f} MB of maps it replaces (pinned): {summary(times['copy_maps'])}, {mb / med:.1f} GB/s")
    print(f"  host-to-device copy of the {packed.numel() * 4 / 1e6:.2f} MB of points and the view table (pinned): "
          f"{summary(times['copy_points'])}")

    model = A.EfficientVRNet(4, 9, args.phi, img_size=S).cuda().eval()
    A.randomize_state_dict(model.state_dict(), seed=0)
    kw = dict(batch=B, conf_thres=0.5, nms_thres=0.4, graph=True)
    frames = torch.from_numpy(np.random.default_rng(0).integers(0, 256, (B,) + frame + (3,), dtype=np.uint8)).pin_memory()
    with_maps = A.FramePipeline(model, frame, (S, S), **kw)
    with_points = A.FramePipeline(model, frame, (S, S), radar_points=N, radar_radius=radii[0], calib=P, **kw)
    runs = {"maps": lambda: with_maps.run(frames, maps_h), "points": lambda: with_points.run(frames, pts)}
    runs["points, packed by the caller"] = lambda: with_points._launch(frames, (packed, views_h))
    rounds = {k: [] for k in runs}
    for k in runs:
        host_ms(runs[k], 3)
    for _ in range(args.rounds):
        for k in runs:
            rounds[k].append(host_ms(runs[k], args.steps))
    a, b = with_maps.run(frames, maps_h), None
    rows_maps = a.rows.clone()
    b = with_points.run(frames, pts)
    print(f"FramePipeline phi={args.phi} {S}x{S} bs={B}, frames {frame[0]}x{frame[1]}, host clock per run() incl. its copies, median "
          f"of {args.rounds} alternating rounds of {args.steps}; rows equal: {torch.equal(rows_maps, b.rows) if radii[0] == 0 else None}")
    for k in runs:
        print(f"  fed {k}: {summary(rounds[k])}")


if __name__ == "__main__":
    main()
