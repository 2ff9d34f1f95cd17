"""Times the connected regions of the class map (vrnet_seg_regions_u8) on one GPU, in one process:

  1. device time per captured replay of the stage's seven launches at --batch images of each --frames size, on two kinds of
     class map: `blobs`, nine smoothed classes (what a segmentation network gives), and `noise`, independent pixels of two
     classes over background (the worst case: about one region per eight pixels), beside what a caller does without the
     stage: the blocking read-back of the class map plus scipy.ndimage.label per class on the host (host clock), rounds
     alternating between the two.  The bytes the stage moves at least, by arithmetic, over its time stand beside it;
  2. FramePipeline.run() with and without the stage (regions=True), host clock over --steps calls ending in a synchronise,
     rounds alternating between the two pipelines.

    python tools/bench_regions.py --batch 8 --frames 480x640,1080x1920

--stage-only N leaves the timing out and issues N eager calls per scene: the run to put under `rocprofv3 --kernel-trace
--stats`, whose rg_merge_kernel row is the border merge on its own, the one launch whose time depends on the picture.

Medians (min .. max) of --rounds alternating rounds; the last line is one JSON record.
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import asy_vrnet_amd as A  # noqa: E402
from asy_vrnet_amd import decode, hip  # noqa: E402
from tools.bench_box_radar import device_ms, host_ms, stats, summary  # noqa: E402


def blob_map(seed, size):
    from scipy import ndimage
    rs = np.random.RandomState(seed)
    sigma = max(size) / 40.0
    return np.stack([ndimage.gaussian_filter(rs.rand(*size).astype(np.float32), sigma) for _ in range(9)]).argmax(0).astype(np.uint8)


def noise_map(seed, size):
    rs = np.random.RandomState(seed)
    return ((rs.rand(*size) < 0.5) * rs.randint(1, 3, size)).astype(np.uint8)


def host_label(class_map):
    """What a caller does today: the read-back, then scipy.ndimage.label per class present."""
    from scipy import ndimage
    maps = class_map.cpu().numpy()
    total = 0
    for cm in maps:
        for c in np.unique(cm).tolist():
            if c:
                total += ndimage.label(cm == c, np.ones((3, 3), int))[1]
    return total


def stage_bytes(B, ih, iw, R):
    """The least the seven launches move, by arithmetic, 33 bytes per pixel: the tile pass reads the class map (1) and writes
    the parent and the area plane (4 + 4), the flatten pass reads and writes the parent plane (4 + 4), the count and the rank
    pass read it (4 + 4), the label pass reads it and writes the labels (4 + 4); the area plane is read at the roots only and
    the merge touches the tiles' borders only, neither is counted; the table is zeroed and written."""
    return B * ih * iw * 33 + 2 * B * R * 48


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--size", type=int, default=512)
    ap.add_argument("--frames", default="480x640,1080x1920")
    ap.add_argument("--boxes", type=int, default=100)
    ap.add_argument("--max-regions", type=int, default=1024)
    ap.add_argument("--phi", default="nano")
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--host-steps", type=int, default=1, help="calls per round of the host path, which takes tens of milliseconds each")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--stage-only", type=int, default=0)
    ap.add_argument("--no-pipeline", action="store_true")
    ap.add_argument("--no-scenes", action="store_true")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_regions: needs a GPU; nothing is measured without one")
    B, R, M = args.batch, args.max_regions, args.boxes
    i32 = dict(dtype=torch.int32, device="cuda")
    rec = {"tool": "bench_regions", "batch": B, "boxes": M, "max_regions": R, "rounds": args.rounds, "steps": args.steps,
           "host_steps": args.host_steps, "device": torch.cuda.get_device_name(0), "scenes": {}}
    print(f"connected regions of the class map, bs={B}, {M} rows per image, table of {R}; median of {args.rounds} alternating rounds; "
          f"device {torch.cuda.get_device_name(0)}")
    frames = [tuple(int(v) for v in f.split("x")) for f in args.frames.split(",")]
    for ih, iw in ([] if args.no_scenes else frames):
        rs = np.random.RandomState(1)
        x, y = np.sort(rs.randint(0, iw + 1, (B * M, 2)), 1), np.sort(rs.randint(0, ih + 1, (B * M, 2)), 1)
        rows = torch.from_numpy(np.stack([x[:, 0], y[:, 0], x[:, 1], y[:, 1], rs.randint(0, 4, B * M)], 1).astype(np.int32)).cuda()
        offsets = torch.arange(0, B * M + 1, M, **i32)
        labels, table = torch.empty((B, ih, iw), **i32), torch.empty((B, R, hip.REGION_WORDS), **i32)
        head, links, flag = torch.empty((B, 4), **i32), torch.empty((B, M), **i32), torch.zeros(1, **i32)
        ws = torch.empty(hip.seg_regions_workspace_bytes(B, ih, iw), dtype=torch.uint8, device="cuda")
        for name, make in (("blobs", blob_map), ("noise", noise_map)):
            maps_h = np.stack([make(10 + b, (ih, iw)) for b in range(B)])
            maps = torch.from_numpy(maps_h).cuda()

            def call():
                hip.seg_regions(maps, rows, offsets, labels, table, head, links, ws, flag=flag)
            if args.stage_only:
                for _ in range(args.stage_only):
                    call()
                torch.cuda.synchronize()
                print(f" {ih} x {iw} `{name}`: {args.stage_only} eager calls issued; regions per image {head[:, 0].tolist()}")
                continue
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
                want = decode.seg_regions_host(maps_h[0], rows[:M].cpu().numpy(), max_regions=R)
                same = np.array_equal(labels[0].cpu().numpy(), want[0]) and np.array_equal(head[0].cpu().numpy(), want[2]) and \
                    np.array_equal(np.frombuffer(table[0].cpu().numpy().tobytes(), np.int32), np.frombuffer(want[1].tobytes(), np.int32))
                counts = head[:, 0].tolist()
                times = {"device": [], "host": []}
                found = 0
                for _ in range(args.rounds):
                    times["device"].append(device_ms(graph.replay, args.steps))
                    times["host"].append(host_ms(lambda: host_label(maps), args.host_steps))
                found = host_label(maps)
            torch.cuda.synchronize()
            nbytes = stage_bytes(B, ih, iw, R)
            med = sorted(times["device"])[len(times["device"]) // 2]
            print(f" {ih} x {iw} `{name}`: regions per image {counts}, scipy finds {found} in all; flag {int(flag.item())}; image 0 equals "
                  f"decode.seg_regions_host: {same}")
            print(f"  vrnet_seg_regions_u8, device time per captured replay ({args.steps} a round): {summary(times['device'])}; at least "
                  f"{nbytes / 1e6:.1f} MB by arithmetic = {nbytes / med / 1e9:.3f} TB/s; workspace {ws.numel() / 1e6:.1f} MB")
            print(f"  class_map.cpu() + scipy.ndimage.label per class on the host, host clock ({args.host_steps} a round): "
                  f"{summary(times['host'])}")
            rec["scenes"][f"{ih}x{iw}_{name}"] = {"regions": counts, "scipy_regions": found, "equals_host": bool(same),
                                                   "replay": stats(times["device"]), "host_path": stats(times["host"]),
                                                   "bytes_by_arithmetic": nbytes, "workspace_bytes": ws.numel()}
    if not args.stage_only and not args.no_pipeline:
        S = args.size
        frame = frames[0]
        model = A.EfficientVRNet(4, 9, args.phi, img_size=S).cuda().eval()
        A.randomize_state_dict(model.state_dict(), seed=0)
        kw = dict(batch=B, conf_thres=0.5, nms_thres=0.4, graph=True)
        pics = torch.from_numpy(np.random.default_rng(0).integers(0, 256, (B,) + frame + (3,), dtype=np.uint8)).pin_memory()
        radar = torch.from_numpy(np.random.RandomState(0).rand(B, 4, S, S).astype(np.float32)).pin_memory()
        without = A.FramePipeline(model, frame, (S, S), **kw)
        with_stage = A.FramePipeline(model, frame, (S, S), regions=dict(background=-1, max_regions=R), **kw)
        runs = {"without the stage": lambda: without.run(pics, radar), "with regions": lambda: with_stage.run(pics, radar)}
        rounds = {k: [] for k in runs}
        for k in runs:
            host_ms(runs[k], 3)
        for _ in range(args.rounds):
            for k in runs:
                rounds[k].append(host_ms(runs[k], args.steps))
        a = without.run(pics, radar).class_map.clone()
        b = with_stage.run(pics, radar)
        print(f"FramePipeline phi={args.phi} {S}x{S} bs={B}, frames {frame[0]}x{frame[1]}, host clock per run() incl. its copies, median of "
              f"{args.rounds} alternating rounds of {args.steps}; class maps equal: {torch.equal(a, b.class_map)}; regions per image "
              f"{b.region_head[:, 0].tolist()} (background = -1)")
        for k in runs:
            print(f"  {k}: {summary(rounds[k])}")
        rec.update(pipeline_without=stats(rounds["without the stage"]), pipeline_with=stats(rounds["with regions"]),
                   pipeline_regions=b.region_head[:, 0].tolist())
    print(json.dumps(rec))


if __name__ == "__main__":
    main()
