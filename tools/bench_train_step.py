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


def captured(a):
    from asy_vrnet_amd import data
    from asy_vrnet_amd.graph import TrainStep
    dev = torch.device("cuda:0")
    B, S, NC, NS = a.batch, a.size, 4, 9
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--phi", default="l")
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--size", type=int, default=512)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--captured", action="store_true", help="eager loop against graph.TrainStep, alternating rounds")
    ap.add_argument("--rounds", type=int, default=5)
    a = ap.parse_args()
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
