"""Times the fixed-size detection chips (vrnet_chip_boxes_u8: the tables and the resample launch) on one GPU, in one process:

  1. device time per captured replay of the two launches alone at --batch frames of --frame with --boxes boxes of about
     --box pixels per image, n_cap = batch x --cap rows as a FramePipeline has them, for every size of --sizes, stretched and
     letterboxed, with and without the float form (two events around --steps replays of a graph that holds the one call;
     median of --rounds rounds); every configuration is first compared with render.chip_boxes_host;
  2. on the same inputs the two launches of the crops (vrnet_crop_boxes_u8), and the host path the chips replace: the read-back
     of the crop arena (`Crops.images`) and a Pillow loop, crop.resize(size, BICUBIC), on the host clock;
  3. FramePipeline.run() built without chips and with chips of the first size (normalised), host clock over --steps calls
     ending in a synchronise, rounds alternating between the two pipelines.

    python tools/bench_chips.py --batch 8 --frame 1080x1920 --boxes 20 --box 200x300 --sizes 64,128
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
from tools.bench_crops import boxes, device_ms, host_ms  # noqa: E402


def summary(rounds):
    return f"{statistics.median(rounds):.4f} ms ({min(rounds):.4f} .. {max(rounds):.4f})"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--frame", default="1080x1920")
    ap.add_argument("--boxes", type=int, default=20)
    ap.add_argument("--box", default="200x300")
    ap.add_argument("--sizes", default="64,128")
    ap.add_argument("--cap", type=int, default=1024, help="rows per image of the table, as FramePipeline's max_candidates")
    ap.add_argument("--size", type=int, default=512)
    ap.add_argument("--phi", default="nano")
    ap.add_argument("--conf", type=float, default=0.5)
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--rounds", type=int, default=7)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_chips: needs a GPU; nothing is measured without one")
    from PIL import Image
    B, S = args.batch, args.size
    frame, box = (tuple(int(v) for v in t.split("x")) for t in (args.frame, args.box))
    sizes = [(int(v), int(v)) for v in args.sizes.split(",")]
    rng = np.random.default_rng(0)
    frames_h = torch.from_numpy(rng.integers(0, 256, (B,) + frame + (3,), dtype=np.uint8)).pin_memory()
    rows_h, offsets_h = boxes(rng, B, args.boxes, frame, box)
    n_cap, N = B * args.cap, len(rows_h)
    rows_d = torch.zeros((n_cap, 5), dtype=torch.int32, device="cuda")
    rows_d[:N] = torch.from_numpy(rows_h)
    frames_d, offsets_d = frames_h.cuda(), torch.from_numpy(offsets_h).cuda()
    flag = torch.zeros(1, dtype=torch.int32, device="cuda")
    crops = render.crop_buffers(n_cap, 2 * B * frame[0] * frame[1], B, flag, "cuda")

    def crop_call():
        hip.crop_boxes(frames_d, rows_d, offsets_d, crops.arena, crops.table, crops.summary, flag=flag)
    calls = {"crops (layout + copy)": crop_call}
    for size in sizes:
        want = [w for b in range(B) for w in render.chip_boxes_host(frames_h[b].numpy(), rows_h[offsets_h[b]:offsets_h[b + 1]], size)]
        for letterbox in (False, True):
            if letterbox:
                want = [w for b in range(B) for w in render.chip_boxes_host(
                    frames_h[b].numpy(), rows_h[offsets_h[b]:offsets_h[b + 1]], size, True)]
            for f32 in (False, True):
                c = render.chip_buffers(n_cap, size, B, letterbox, f32, flag, "cuda")

                def call(c=c):
                    hip.chip_boxes(frames_d, rows_d, offsets_d, c.chips, c.table, c.summary, c.workspace, letterbox=c.letterbox,
                                   chips_f32=c.chips_f32, flag=flag)
                call()
                torch.cuda.synchronize()
                got = c.chips[:N].cpu().numpy()
                if c.summary.tolist() != [N] or not all(np.array_equal(g, w) for g, w in zip(got, want)):
                    raise SystemExit(f"bench_chips: the chips differ from render.chip_boxes_host ({size}, letterbox {letterbox})")
                calls[f"chips {size[0]}x{size[1]} {'letterbox' if letterbox else 'stretched'}{' + float form' if f32 else ''}"] = call
    stream = torch.cuda.Stream()
    graphs, times = {}, {k: [] for k in calls}
    with torch.cuda.stream(stream):
        for k, call in calls.items():
            for _ in range(2):
                call()
            torch.cuda.synchronize()
            graphs[k] = torch.cuda.CUDAGraph()
            with torch.cuda.graph(graphs[k], stream=stream):
                call()
        for _ in range(args.rounds):
            for k in calls:
                times[k].append(device_ms(graphs[k].replay, args.steps))
    torch.cuda.synchronize()
    print(f"detection chips, bs={B}, frames {frame[0]}x{frame[1]}, {args.boxes} boxes of about {box[0]}x{box[1]} per image, {N} rows in "
          f"a table of {n_cap}, every configuration equal to render.chip_boxes_host; device time per captured replay of the two "
          f"launches, median of {args.rounds} rounds of {args.steps} (min .. max):")
    for k in calls:
        print(f"  {k}: {summary(times[k])}")

    def host_path(size):
        got = crops.images()
        return [np.asarray(Image.fromarray(c).resize(size[::-1], Image.BICUBIC)) for g in got for c in g]
    for size in sizes:
        rounds = []
        for _ in range(args.rounds):
            crop_call()
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            host_path(size)
            rounds.append((time.perf_counter() - t0) * 1e3)
        print(f"  host path {size[0]}x{size[1]} (arena read-back + Pillow loop over {N} crops), host clock: {summary(rounds)}")

    model = A.EfficientVRNet(4, 9, args.phi, img_size=S).cuda().eval()
    A.randomize_state_dict(model.state_dict(), seed=0)
    kw = dict(batch=B, conf_thres=args.conf, nms_thres=0.4, graph=True)
    radar = torch.from_numpy(rng.standard_normal((B, 4, S, S)).astype(np.float32)).pin_memory()
    chips = dict(size=sizes[0], normalised=True)
    pipes = {"without chips": A.FramePipeline(model, frame, (S, S), **kw), f"chips={chips}": A.FramePipeline(model, frame, (S, S), chips=chips, **kw)}
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
          f"of {args.rounds} alternating rounds of {args.steps}; {int(b.kept.sum())} detections, {int(b.chips.summary[0])} chips; rows and "
          f"rendered equal: {torch.equal(a.rows, b.rows) and torch.equal(a.rendered, b.rendered)}")
    for k in runs:
        print(f"  {k}: {summary(rounds[k])}")


if __name__ == "__main__":
    main()
