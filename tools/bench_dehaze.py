"""Times the dark-channel dehazing (vrnet_dehaze_u8, eleven launches) on one GPU, in one process:

  1. checks the device against render.dehaze_host first: image 0 of the batch at the full --frame (bytes, transmission and
     atmospheric light, bit for bit), and prints the host time of that one numpy call -- the work the stage replaces.  It is a
     numpy figure, not an OpenCV one;
  2. device time per captured replay of the one call at --batch frames of --frame (two events around --steps replays of a
     graph that holds it; median of --rounds rounds), with the workspace size;
  3. FramePipeline.run() built with dehaze=None and with the stage, host clock over --steps calls ending in a synchronise,
     rounds alternating between the two pipelines.

    python tools/bench_dehaze.py --batch 8 --frame 1080x1920
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


def hazy(rng, ih, iw):
    """A blocky scene blended towards a bright airlight by a depth ramp, plus small noise."""
    scene = rng.integers(0, 256, (ih // 16 + 1, iw // 16 + 1, 3)).repeat(16, 0).repeat(16, 1)[:ih, :iw].astype(np.float64)
    depth = (0.3 + 0.7 * np.arange(ih) / ih)[:, None, None]
    return np.clip(scene * depth + 220 * (1 - depth) + rng.integers(-3, 4, (ih, iw, 3)), 0, 255).astype(np.uint8)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--frame", default="1080x1920")
    ap.add_argument("--sz", type=int, default=15)
    ap.add_argument("--r", type=int, default=60)
    ap.add_argument("--size", type=int, default=512)
    ap.add_argument("--phi", default="nano")
    ap.add_argument("--conf", type=float, default=0.5)
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--no-pipeline", action="store_true")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_dehaze: needs a GPU; nothing is measured without one")
    B, S = args.batch, args.size
    ih, iw = (int(v) for v in args.frame.split("x"))
    q = render.dehaze_params(sz=args.sz, r=args.r)
    rng = np.random.default_rng(0)
    frames_h = torch.from_numpy(np.stack([hazy(rng, ih, iw) for _ in range(B)])).pin_memory()
    frames_d = frames_h.cuda()
    out = torch.empty_like(frames_d)
    t = torch.empty((B, ih, iw), dtype=torch.float64, device="cuda")
    ws = torch.empty(hip.dehaze_workspace_bytes(B, ih, iw), dtype=torch.uint8, device="cuda")
    flag = torch.zeros(1, dtype=torch.int32, device="cuda")

    def call():
        hip.dehaze(frames_d, out, ws, transmission=t, flag=flag, **q)
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
        want, want_t, want_A = render.dehaze_host(frames_h[0].numpy(), **q)
        host_s = time.perf_counter() - t0
        got_A = ws[:32 * B].view(torch.float64).view(B, 4)[0, :3].cpu().numpy()
        same = np.array_equal(out[0].cpu().numpy(), want) and np.array_equal(t[0].cpu().numpy().view(np.int64), want_t.view(np.int64)) \
            and np.array_equal(got_A.view(np.int64), want_A.view(np.int64)) and int(flag) == 0
        if not same:
            raise SystemExit("bench_dehaze: the device differs from render.dehaze_host")
        times = [device_ms(graph.replay, args.steps) for _ in range(args.rounds)]
    torch.cuda.synchronize()
    changed = float((want != frames_h[0].numpy()).mean())
    print(f"dehaze, bs={B}, frames {ih}x{iw}, sz {q['sz']}, r {q['r']}; image 0 equal to render.dehaze_host bit for bit (bytes, t, A; "
          f"{changed:.2f} of its bytes changed); workspace {ws.numel() / 1e6:.1f} MB; device time per captured replay of the "
          f"eleven launches, median of {args.rounds} rounds of {args.steps}:")
    print(f"  {summary(times)}, {statistics.median(times) / B:.4f} ms per frame")
    print(f"  render.dehaze_host on ONE {ih}x{iw} frame on this host's CPU (numpy float64, not OpenCV): {host_s * 1e3:.0f} ms")
    if args.no_pipeline:
        return

    model = A.EfficientVRNet(4, 9, args.phi, img_size=S).cuda().eval()
    A.randomize_state_dict(model.state_dict(), seed=0)
    kw = dict(batch=B, conf_thres=args.conf, nms_thres=0.4, graph=True)
    radar = torch.from_numpy(rng.standard_normal((B, 4, S, S)).astype(np.float32)).pin_memory()
    pipes = {"dehaze=None": A.FramePipeline(model, (ih, iw), (S, S), **kw),
             "dehaze=True": A.FramePipeline(model, (ih, iw), (S, S), dehaze=q, **kw)}
    runs = {k: (lambda p=p: p.run(frames_h, radar)) for k, p in pipes.items()}
    rounds = {k: [] for k in runs}
    for k in runs:
        host_ms(runs[k], 3)
    for _ in range(args.rounds):
        for k in runs:
            rounds[k].append(host_ms(runs[k], args.steps))
    res = pipes["dehaze=True"].run(frames_h, radar)
    torch.cuda.synchronize()
    print(f"FramePipeline phi={args.phi} {S}x{S} bs={B} conf {args.conf}, frames {ih}x{iw}, host clock per run() incl. its copies, median "
          f"of {args.rounds} alternating rounds of {args.steps}; dehazed image 0 equal to the host's: "
          f"{np.array_equal(res.dehazed[0].cpu().numpy(), want)}, flag {int(res.flag)}")
    for k in runs:
        print(f"  {k}: {summary(rounds[k])}")


if __name__ == "__main__":
    main()
