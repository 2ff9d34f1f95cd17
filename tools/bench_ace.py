"""Times the ACE de-rain enhancement (vrnet_ace_u8, two launches per pyramid level plus four) on one GPU, in one process:

  1. checks the device against render.ace_host first: image 0 of the batch at the full --frame, byte for byte, and prints the
     host time of that one numpy call -- the work the stage replaces.  It is a numpy figure, not an OpenCV one;
  2. device time per captured replay of the one call at --batch frames of --frame (two events around --steps replays of a
     graph that holds it; median of --rounds rounds), with the workspace size and the arithmetic float64 operation count of
     the call's tap sums, so that the achieved rate can be read off;
  3. FramePipeline.run() built with ace=None and with the stage, host clock over --steps calls ending in a synchronise,
     rounds alternating between the two pipelines.

    python tools/bench_ace.py --batch 8 --frame 1080x1920
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


def rainy(rng, ih, iw):
    """A blocky scene under bright vertical streaks and small noise."""
    scene = rng.integers(0, 256, (ih // 16 + 1, iw // 16 + 1, 3)).repeat(16, 0).repeat(16, 1)[:ih, :iw].astype(np.float64)
    streaks = (rng.random((1, iw, 1)) < 0.05) * rng.integers(40, 120, (ih // 8 + 1, iw, 1)).repeat(8, 0)[:ih]
    return np.clip(scene * 0.7 + streaks + rng.integers(-3, 4, (ih, iw, 3)), 0, 255).astype(np.uint8)


def tap_flops(ih, iw, radius):
    """The float64 operations of the two tap sums of one frame, by arithmetic: per pixel, channel and level two planes of
    (2 radius + 1)^2 - 1 taps, each a subtraction, a product, two clip comparisons, a product and an addition."""
    taps = (2 * radius + 1) ** 2 - 1
    return sum(3 * h * w * 2 * taps * 6 for h, w in render.ace_levels(ih, iw)[:-1])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--frame", default="1080x1920")
    ap.add_argument("--radius", type=int, default=3)
    ap.add_argument("--ratio", type=float, default=4.0)
    ap.add_argument("--size", type=int, default=512)
    ap.add_argument("--phi", default="nano")
    ap.add_argument("--conf", type=float, default=0.5)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--no-pipeline", action="store_true")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_ace: needs a GPU; nothing is measured without one")
    B, S = args.batch, args.size
    ih, iw = (int(v) for v in args.frame.split("x"))
    q = render.ace_params(ratio=args.ratio, radius=args.radius)
    rng = np.random.default_rng(0)
    frames_h = torch.from_numpy(np.stack([rainy(rng, ih, iw) for _ in range(B)])).pin_memory()
    frames_d = frames_h.cuda()
    out = torch.empty_like(frames_d)
    weights = torch.from_numpy(render.ace_weights(q["radius"])).cuda()
    ws = torch.empty(hip.ace_workspace_bytes(B, ih, iw), dtype=torch.uint8, device="cuda")
    flag = torch.zeros(1, dtype=torch.int32, device="cuda")
    launches = 2 * (len(render.ace_levels(ih, iw)) - 1) + 4

    def call():
        hip.ace(frames_d, out, ws, weights, flag=flag, **q)
    stream = torch.cuda.Stream()
    with torch.cuda.stream(stream):
        for _ in range(2):
            call()
        torch.cuda.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=stream):
            call()
        out.zero_()
        graph.replay()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        want, degenerate = render.ace_host(frames_h[0].numpy(), **q)
        host_s = time.perf_counter() - t0
        if degenerate or not np.array_equal(out[0].cpu().numpy(), want) or int(flag) != 0:
            raise SystemExit("bench_ace: the device differs from render.ace_host")
        times = [device_ms(graph.replay, args.steps) for _ in range(args.rounds)]
    torch.cuda.synchronize()
    changed = float((want != frames_h[0].numpy()).mean())
    ms, flops = statistics.median(times), B * tap_flops(ih, iw, q["radius"])
    print(f"ace, bs={B}, frames {ih}x{iw}, radius {q['radius']}, ratio {q['ratio']}; image 0 equal to render.ace_host byte for byte "
          f"({changed:.2f} of its bytes changed); workspace {ws.numel() / 1e6:.1f} MB; device time per captured replay of the "
          f"{launches} launches, median of {args.rounds} rounds of {args.steps}:")
    print(f"  {summary(times)}, {ms / B:.4f} ms per frame")
    print(f"  tap sums of the call by arithmetic: {flops / 1e9:.2f} GFLOP float64 ({flops / B / 1e9:.2f} per frame) -> "
          f"{flops / ms / 1e9:.2f} TFLOP/s over the whole call")
    print(f"  render.ace_host on ONE {ih}x{iw} frame on this host's CPU (numpy float64, not OpenCV): {host_s * 1e3:.0f} ms")
    if args.no_pipeline:
        return

    model = A.EfficientVRNet(4, 9, args.phi, img_size=S).cuda().eval()
    A.randomize_state_dict(model.state_dict(), seed=0)
    kw = dict(batch=B, conf_thres=args.conf, nms_thres=0.4, graph=True)
    radar = torch.from_numpy(rng.standard_normal((B, 4, S, S)).astype(np.float32)).pin_memory()
    pipes = {"ace=None": A.FramePipeline(model, (ih, iw), (S, S), **kw),
             "ace=True": A.FramePipeline(model, (ih, iw), (S, S), ace=q, **kw)}
    runs = {k: (lambda p=p: p.run(frames_h, radar)) for k, p in pipes.items()}
    rounds = {k: [] for k in runs}
    for k in runs:
        host_ms(runs[k], 3)
    for _ in range(args.rounds):
        for k in runs:
            rounds[k].append(host_ms(runs[k], args.steps))
    res = pipes["ace=True"].run(frames_h, radar)
    torch.cuda.synchronize()
    print(f"FramePipeline phi={args.phi} {S}x{S} bs={B} conf {args.conf}, frames {ih}x{iw}, host clock per run() incl. its copies, median "
          f"of {args.rounds} alternating rounds of {args.steps}; enhanced image 0 equal to the host's: "
          f"{np.array_equal(res.enhanced[0].cpu().numpy(), want)}, flag {int(res.flag)}")
    for k in runs:
        print(f"  {k}: {summary(rounds[k])}")


if __name__ == "__main__":
    main()
