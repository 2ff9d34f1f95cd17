"""Same bytes as another commit, for a change that must not move a result: a FramePipeline with every optional stage on, plus
jpeg=, fixed-size and ragged, graph=True, phi nano, 512 x 512, frames of 480 x 640, batch 8.  Three run() calls each on seeded
pictures and radar points; the SHA-256 of every result tensor goes into --out (json) -- crops.arena, the chips and the JPEG
arena over their written parts only, the rest being uninitialised memory -- and run() per batch is timed (host clock, median
and range of --rounds rounds of --steps).  Run it once per tree (--tree: the checkout whose package is imported) and compare
the two files' "tensors": equal digests are equal bytes.

    python tools/stages_digest.py --tree ../parent --out parent.json && python tools/stages_digest.py --tree . --out new.json
"""
import argparse
import hashlib
import json
import os
import statistics
import sys
import time

import numpy as np

ap = argparse.ArgumentParser()
ap.add_argument("--tree", required=True)
ap.add_argument("--out", required=True)
ap.add_argument("--steps", type=int, default=50)
ap.add_argument("--rounds", type=int, default=7)
args = ap.parse_args()
sys.path.insert(0, os.path.abspath(args.tree))
import torch  # noqa: E402
import asy_vrnet_amd as A  # noqa: E402

print("package from", os.path.dirname(A.__file__) if hasattr(A, "__file__") else A)
B, F, S, NC = 8, (480, 640), (512, 512), 4
CALIB = np.array([[400.0, 0, 320, 0], [0, 400.0, 240, 0], [0, 0, 1, 0]], np.float32)
ALL = dict(dehaze=True, ace=True, crops=True, chips=(64, 64), radar_points=4096, calib=CALIB, box_radar=True, track=True,
           captions=dict(fps=25.0), regions=True, labels=True, class_names=("a", "b", "c", "d"), heatmap=True, jpeg=True, graph=True)


def picture(rng, h, w):
    y, x = np.mgrid[:h, :w].astype(np.float64)
    ph = rng.uniform(0, 6, 3)
    planes = [127 + 80 * np.sin(x / (17.0 + 9 * c) + ph[c]) * np.cos(y / (23.0 - 5 * c)) + 40 * ((x // 64 + y // 48) % 2) for c in range(3)]
    return np.clip(np.stack(planes, -1) + rng.normal(0, 6, (h, w, 3)), 0, 255).astype(np.uint8)


def points(rng, n):
    z = rng.uniform(2, 50, n)
    return np.stack([rng.uniform(-0.7, 0.7, n) * z, rng.uniform(-0.5, 0.5, n) * z, z] + [rng.standard_normal(n) for _ in range(4)], 1).astype(np.float32)


def call_inputs(seed, sizes):
    rng = np.random.default_rng(seed)
    return [picture(rng, *s) for s in sizes], [points(rng, int(rng.integers(500, 3000))) for _ in sizes]


def tensors(res):
    out = {}
    for name in res.__slots__:
        v = getattr(res, name)
        if v is None or name == "sizes":
            continue
        if torch.is_tensor(v):
            out[name] = v
            continue
        attrs = vars(v) if hasattr(v, "__dict__") else {k: getattr(v, k) for k in getattr(v, "__slots__", ())}
        for k, t in attrs.items():
            if torch.is_tensor(t) and k != "workspace" and not k.startswith("_"):
                out[f"{name}.{k}"] = t
    torch.cuda.synchronize()
    out = {k: t.cpu().numpy() for k, t in out.items()}
    if "crops.arena" in out:
        used = int(out["crops.summary"][1])
        out["crops.arena"] = out["crops.arena"].reshape(-1)[:3 * used]
    for k in ("chips.chips", "chips.chips_f32"):      # rows behind the last one are not written
        if k in out:
            out[k] = out[k][:int(out["chips.summary"][0])]
    if "jpeg.arena" in out:
        lengths = out["jpeg.record"].reshape(-1, 2)[:, 0]
        out["jpeg.arena"] = np.concatenate([out["jpeg.arena"][b, :int(n)] for b, n in enumerate(lengths)])
    return out


model = A.EfficientVRNet(NC, 9, "nano", img_size=S[0]).cuda().eval()
A.randomize_state_dict(model.state_dict(), seed=4)
RAGGED = [(480, 640), (360, 640), (480, 500), (301, 417), (240, 320), (477, 639), (128, 96), (400, 600)]
dump, lines = {}, []
conf = None
for kind in ("fixed", "ragged"):
    sizes = [F] * B if kind == "fixed" else RAGGED
    if conf is None:          # the 40th-largest score of the first batch of the plain pipeline: detections exist, the cap is not hit
        probe = A.FramePipeline(model, F, S, batch=B, conf_thres=0.0, nms_thres=0.4, max_candidates=64, radar_points=4096, calib=CALIB,
                                graph=False)
        fr, pts = call_inputs(100, sizes)
        res = probe.run(np.stack(fr), pts)
        rows = res.rows.cpu().numpy()
        conf = float(np.sort((rows[..., 4] * rows[..., 5]).reshape(-1))[::-1][40])
        del probe
        print("conf_thres", conf)
    pipe = A.FramePipeline(model, F, S, batch=B, conf_thres=conf, nms_thres=0.4, max_candidates=64, ragged=kind == "ragged", **ALL)
    for call in range(3):
        fr, pts = call_inputs(100 + call + (10 if kind == "ragged" else 0), sizes)
        res = pipe.run(np.stack(fr) if kind == "fixed" else fr, pts)
        got = tensors(res)
        print(kind, call, "kept", got["kept"].tolist(), "flag", int(got["flag"][0]), "tensors", len(got),
              "jpeg lengths", got["jpeg.record"].reshape(-1, 2)[:, 0].tolist() if "jpeg.record" in got else None, flush=True)
        for k, v in got.items():
            v = np.ascontiguousarray(v)
            dump[f"{kind}/{call}/{k}"] = [str(v.dtype), list(v.shape), hashlib.sha256(v.tobytes()).hexdigest()]
    frames = np.stack(fr) if kind == "fixed" else fr
    rounds = []
    for _ in range(args.rounds):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(args.steps):
            pipe.run(frames, pts)
        torch.cuda.synchronize()
        rounds.append((time.perf_counter() - t0) * 1e3 / args.steps)
    lines.append(f"{kind}: run() per batch {statistics.median(rounds):.4f} ms (rounds {min(rounds):.4f}..{max(rounds):.4f})")
    print(lines[-1], flush=True)
    del pipe
os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
json.dump(dict(tensors=dump, timing=lines), open(args.out, "w"), indent=1)
print("saved", len(dump), "tensor digests")
