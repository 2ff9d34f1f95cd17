"""Times the device-side JPEG encoder (vrnet_jpeg_encode_u8, eight launches) on one GPU, in one process:

  1. device time per captured replay of the eight launches at --batch pictures of --frame, for (quality 95, 4:4:4) and
     (quality 75, 4:2:0), on a natural-looking picture and on noise (two events around --steps replays of a graph that holds
     the one call; median of --rounds rounds); every configuration is first compared with Pillow, byte for byte;
  2. on the same pictures the host path the encoder replaces: the read-back of the pictures plus a Pillow `save` loop into
     memory, on the host clock; and the read-back of the files alone (`Jpegs.bytes`);
  3. FramePipeline.run() built without and with jpeg=True, host clock over --steps calls ending in a synchronise, rounds
     alternating between the two pipelines.

    python tools/bench_jpeg.py --batch 8 --frame 1080x1920
"""
import argparse
import io
import os
import statistics
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import asy_vrnet_amd as A  # noqa: E402
from asy_vrnet_amd import hip, render  # noqa: E402
from tools.bench_crops import device_ms, host_ms  # noqa: E402


def summary(rounds):
    return f"{statistics.median(rounds):.4f} ms ({min(rounds):.4f} .. {max(rounds):.4f})"


def natural(h, w, seed):
    """A smooth picture with edges and some noise: what a rendered frame looks like to an encoder."""
    y, x = np.mgrid[:h, :w].astype(np.float64)
    rng = np.random.default_rng(seed)
    planes = [127 + 80 * np.sin(x / (17.0 + 9 * c) + c + seed) * np.cos(y / (23.0 - 5 * c)) + 40 * ((x // 64 + y // 48) % 2) for c in range(3)]
    return np.clip(np.stack(planes, -1) + rng.normal(0, 4, (h, w, 3)), 0, 255).astype(np.uint8)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--frame", default="1080x1920")
    ap.add_argument("--size", type=int, default=512)
    ap.add_argument("--phi", default="nano")
    ap.add_argument("--conf", type=float, default=0.5)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=7)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_jpeg: needs a GPU; nothing is measured without one")
    from PIL import Image
    B, S = args.batch, args.size
    h, w = (int(v) for v in args.frame.split("x"))
    rng = np.random.default_rng(0)
    pictures = {"natural": np.stack([natural(h, w, b) for b in range(B)]), "noise": rng.integers(0, 256, (B, h, w, 3), dtype=np.uint8)}
    device = {k: torch.from_numpy(v).cuda() for k, v in pictures.items()}
    modes = ((95, 0), (75, 2))

    def pillow(a, q, s):
        out = io.BytesIO()
        Image.fromarray(a).save(out, format="JPEG", quality=q, subsampling=s)
        return out.getvalue()
    calls, buffers, sizes = {}, {}, {}
    for name, pics in device.items():
        for q, s in modes:
            key = f"{name}, quality {q}, {'4:2:0' if s else '4:4:4'}"
            buf = render.jpeg_buffers(B, h, w, q, s, capacity=render.JPEG_HEADER + 8 * h * w, device="cuda")

            def call(pics=pics, buf=buf):
                hip.jpeg_encode(pics, buf.header, buf.arena, buf.record, buf.workspace, buf.subsampling, flag=buf.flag)
            call()
            files = buf.bytes()
            if any(f != pillow(a, q, s) for f, a in zip(files, pictures[name])):
                raise SystemExit(f"bench_jpeg: the files differ from Pillow's ({key})")
            calls[key], buffers[key], sizes[key] = call, buf, sum(len(f) for f in files)
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
    print(f"JPEG encoder, bs={B}, pictures {h}x{w} ({B * h * w * 3 / 1e6:.1f} MB), every file equal to Pillow's; device time per "
          f"captured replay of the eight launches, median of {args.rounds} rounds of {args.steps} (min .. max):")
    for k in calls:
        print(f"  {k}: {summary(times[k])}, {sizes[k] / 1e6:.2f} MB of files")
    for name, pics in device.items():
        for q, s in modes:
            key = f"{name}, quality {q}, {'4:2:0' if s else '4:4:4'}"
            rounds, back = [], []
            for _ in range(args.rounds):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                host = pics.cpu().numpy()
                for b in range(B):
                    pillow(host[b], q, s)
                rounds.append((time.perf_counter() - t0) * 1e3)
                calls[key]()
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                buffers[key].bytes()
                back.append((time.perf_counter() - t0) * 1e3)
            print(f"  host path, {key} (read-back of the pictures + Pillow save loop into memory), host clock: {summary(rounds)}; "
                  f"the read-back of the files alone: {summary(back)}")

    model = A.EfficientVRNet(4, 9, args.phi, img_size=S).cuda().eval()
    A.randomize_state_dict(model.state_dict(), seed=0)
    kw = dict(batch=B, conf_thres=args.conf, nms_thres=0.4, graph=True)
    radar = torch.from_numpy(rng.standard_normal((B, 4, S, S)).astype(np.float32)).pin_memory()
    frames_h = torch.from_numpy(pictures["natural"]).pin_memory()
    pipes = {"without jpeg": A.FramePipeline(model, (h, w), (S, S), **kw), "jpeg=True": A.FramePipeline(model, (h, w), (S, S), jpeg=True, **kw)}
    runs = {k: (lambda p=p: p.run(frames_h, radar)) for k, p in pipes.items()}
    rounds = {k: [] for k in runs}
    for k in runs:
        host_ms(runs[k], 3)
    for _ in range(args.rounds):
        for k in runs:
            rounds[k].append(host_ms(runs[k], args.steps))
    a, b = (pipes[k].run(frames_h, radar) for k in pipes)
    torch.cuda.synchronize()
    files = b.jpeg.bytes()
    ok = all(f == pillow(r, 95, 0) for f, r in zip(files, b.rendered.cpu().numpy()))
    print(f"FramePipeline phi={args.phi} {S}x{S} bs={B} conf {args.conf}, frames {h}x{w}, host clock per run() incl. its copies, median of "
          f"{args.rounds} alternating rounds of {args.steps}; rendered equal: {torch.equal(a.rendered, b.rendered)}; the files are "
          f"Pillow's of the rendered frames: {ok}; {sum(len(f) for f in files) / 1e6:.2f} MB of files")
    for k in runs:
        print(f"  {k}: {summary(rounds[k])}")
    lo, hi = min(rounds["without jpeg"]), max(rounds["without jpeg"])
    med = statistics.median(rounds["jpeg=True"])
    print(f"  run() with jpeg lies {'inside' if lo <= med <= hi else 'outside'} the spread of run() without it "
          f"(+{med - statistics.median(rounds['without jpeg']):.4f} ms)")


if __name__ == "__main__":
    main()
