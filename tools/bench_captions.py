"""Times the captions under the rendered detections (vrnet_caption_text_f32, vrnet_render_captions_u8) on one GPU, in one
process:

  1. device time per captured replay of each of the two launches, and of both, at --batch images of --frame with --boxes kept
     rows per image of which --live carry a track with a radar range (two events around --steps replays of a graph that holds
     the call), rounds alternating between the three graphs.  The draw launch is in place and rewrites the same pixels, so the
     replays need no copy of the picture.  The pictures are checked against render.draw_captions_host once;
  2. FramePipeline.run() with and without captions (track and box_radar on in both), host clock over --steps calls ending in
     a synchronise, rounds alternating between the two pipelines.

    python tools/bench_captions.py --batch 8 --boxes 100 --live 30 --frame 480x640

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
from asy_vrnet_amd import data, hip, render  # noqa: E402
from tools.bench_box_radar import camera, cloud, device_ms, host_ms, random_rows, stats, summary  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--size", type=int, default=512)
    ap.add_argument("--points", type=int, default=4096)
    ap.add_argument("--boxes", type=int, default=100)
    ap.add_argument("--tracks", type=int, default=64)
    ap.add_argument("--live", type=int, default=30)
    ap.add_argument("--fps", type=float, default=25.0)
    ap.add_argument("--frame", default="480x640")
    ap.add_argument("--phi", default="nano")
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--rounds", type=int, default=5)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_captions: needs a GPU; nothing is measured without one")
    B, S, M, T = args.batch, args.size, args.boxes, args.tracks
    frame = tuple(int(v) for v in args.frame.split("x"))
    size = render.label_font_size(frame[0])
    atlas = render.GlyphAtlas(None, (size,))
    i32 = dict(dtype=torch.int32, device="cuda")
    rec = {"tool": "bench_captions", "batch": B, "size": S, "boxes": M, "tracks": T, "live": args.live, "frame": list(frame),
           "font_size": size, "rounds": args.rounds, "steps": args.steps, "device": torch.cuda.get_device_name(0)}
    print(f"captions under the detections, bs={B}, frames {frame[0]}x{frame[1]} (font size {size}), {M} kept rows per image, "
          f"{args.live} of them tracked with a range; median of {args.rounds} alternating rounds; device {torch.cuda.get_device_name(0)}")
    rs = np.random.RandomState(0)
    table, ids = np.zeros((B, T), data.TRACK_DTYPE), np.zeros((B, M), np.int32)
    for b in range(B):
        for s, row in enumerate(rs.permutation(M)[:args.live]):
            t = table[b, s]
            t["id"], t["row"], t["range_age"], t["hits"] = 100 * b + s + 1, row, 0, 2
            t["x"][4], t["v"][4] = rs.uniform(5, 300), rs.uniform(-0.5, 0.5)
            ids[b, row] = t["id"]
    rows_h = np.stack([random_rows(100 + b, M, frame) for b in range(B)])
    draw_h = np.concatenate([np.floor(rows_h[..., [1, 0, 3, 2]]).astype(np.int32), rows_h[..., 6:].astype(np.int32)], 2)
    draw_h = np.ascontiguousarray(draw_h.reshape(-1, 5))      # left, top, right, bottom, class
    offsets_h = (np.arange(B + 1) * M).astype(np.int32)
    frames_h = np.random.default_rng(0).integers(0, 256, (B,) + frame + (3,), dtype=np.uint8)
    kept_d, offsets_d, ids_d = torch.full((B,), M, **i32), torch.from_numpy(offsets_h).cuda(), torch.from_numpy(ids).cuda()
    table_d = torch.from_numpy(np.frombuffer(table.tobytes(), np.int32).reshape(B, T, 16).copy()).cuda()
    draw_d, pic_d, bpal = torch.from_numpy(draw_h).cuda(), torch.from_numpy(frames_h).cuda(), torch.from_numpy(render.det_palette(4)).cuda()
    records_d, flag_d = torch.zeros((B * M, hip.CAPTION_WORDS), **i32), torch.zeros(1, **i32)
    blob, glyphs = atlas.on("cuda")

    def text():
        hip.caption_text(kept_d, offsets_d, records_d, ids=ids_d, table=table_d, rate_scale=args.fps, flag=flag_d)

    def draw():
        hip.render_captions(pic_d, draw_d, offsets_d, bpal, records_d, blob, glyphs, atlas.size_index(size), flag=flag_d)

    def both():
        text()
        draw()
    calls = {"vrnet_caption_text_f32": text, "vrnet_render_captions_u8": draw, "both launches": both}
    stream, graphs = torch.cuda.Stream(), {}
    with torch.cuda.stream(stream):
        for _ in range(2):
            both()
        torch.cuda.synchronize()
        for name, call in calls.items():
            graphs[name] = torch.cuda.CUDAGraph()
            with torch.cuda.graph(graphs[name], stream=stream):
                call()
            graphs[name].replay()
        torch.cuda.synchronize()
        strings, bits = render.caption_strings(ids, [M] * B, table, rate_scale=args.fps)
        want = np.stack([render.draw_captions_host(frames_h[b], draw_h[b * M:(b + 1) * M], strings[b], atlas, size) for b in range(B)])
        same = np.array_equal(pic_d.cpu().numpy(), want) and render.caption_decode(records_d.cpu().numpy()) == sum(strings, [])
        area = int((want != frames_h).any(axis=3).sum())
        times = {name: [] for name in calls}
        for _ in range(args.rounds):
            for name in calls:
                times[name].append(device_ms(graphs[name].replay, args.steps))
    torch.cuda.synchronize()
    print(f" {sum(bool(s) for s in sum(strings, []))} captions, e.g. {strings[0][int(np.flatnonzero(ids[0])[0])]!r}; {area} pixels changed; "
          f"flag {int(flag_d.item())} (host {bits}); equals the host statements: {same}")
    for name in calls:
        print(f"  {name}, device time per captured replay ({args.steps} a round): {summary(times[name])}")
    rec.update(equals_host=bool(same), pixels_changed=area, text=stats(times["vrnet_caption_text_f32"]),
               draw=stats(times["vrnet_render_captions_u8"]), both=stats(times["both launches"]))

    N = args.points
    P = camera(frame)
    pts = [cloud(b, N) for b in range(B)]
    model = A.EfficientVRNet(4, 9, args.phi, img_size=S).cuda().eval()
    A.randomize_state_dict(model.state_dict(), seed=0)
    kw = dict(batch=B, conf_thres=0.5, nms_thres=0.4, graph=True, radar_points=N, calib=P, box_radar=True, track=dict(max_tracks=T))
    frames = torch.from_numpy(frames_h).pin_memory()
    without = A.FramePipeline(model, frame, (S, S), **kw)
    with_stage = A.FramePipeline(model, frame, (S, S), captions={"atlas": atlas, "fps": args.fps}, **kw)
    runs = {"without the stage": lambda: without.run(frames, pts), "with captions": lambda: with_stage.run(frames, pts)}
    rounds = {k: [] for k in runs}
    for k in runs:
        host_ms(runs[k], 3)
    for _ in range(args.rounds):
        for k in runs:
            rounds[k].append(host_ms(runs[k], args.steps))
    a = without.run(frames, pts).rows.clone()
    b = with_stage.run(frames, pts)
    shown = b.caption_strings()
    print(f"FramePipeline phi={args.phi} {S}x{S} bs={B}, frames {frame[0]}x{frame[1]}, track and box_radar on, host clock per run() incl. "
          f"its copies, median of {args.rounds} alternating rounds of {args.steps}; rows equal: {torch.equal(a, b.rows)}; kept "
          f"{b.kept.tolist()}; captions {sum(bool(s) for s in sum(shown, []))}, e.g. {next((s for s in sum(shown, []) if s), '')!r}")
    for k in runs:
        print(f"  {k}: {summary(rounds[k])}")
    rec.update(pipeline_without=stats(rounds["without the stage"]), pipeline_with=stats(rounds["with captions"]),
               pipeline_kept=b.kept.tolist())
    print(json.dumps(rec))


if __name__ == "__main__":
    main()
