"""Inference-side timing of the hot path on one GPU (not the BASELINE metric): eval-mode forward of EfficientVRNet +
the box decode (decode_outputs), captured in one hipGraph per batch size.  With --nms CONF/IOU[,CONF/IOU...] the timed
loop also runs non_max_suppression on the decoded boxes (outside the graph: its output size depends on the data), once
per threshold pair, and reports the NMS step alone as well.  With --seg HxW[,HxW...] it times the seg side after the
forward: decode.seg_predict into each original size H x W, metrics.fast_hist of that class map against random labels,
and, once per batch size, metrics.f_score of the seg logits against a random one-hot target next to an eager torch
expression of the same metric.  With --letterbox HxW[,HxW...] it times the input side: data.device_letterbox of a batch of
raw uint8 frames of each original size H x W into the network input -- on frames already resident on the device, and
including the host-to-device copy from pinned memory -- next to Pillow's data.resize_image of the same frames on one
core (where Pillow is installed), with the bytes per image that cross PCIe either way.  With --render HxW[,HxW...] it times
the output side after the forward: render.seg_render (mix_type 0, with the pixel counts) of the class map seg_predict makes
at each original size H x W, and render.render_frame of the same map with 100 boxes per image, on frames resident on the
device -- next to a plain device copy of the same frame bytes (out.copy_(frames): the bound of a byte-bound pass) and to the
host path on one core (numpy palette lookup + Image.blend, where Pillow is installed), with the bytes per image that
would otherwise cross PCIe.  With --pipeline HxW[,HxW...] it times frame-in to rendered-frame-out for frames of each original
size H x W resident on the device, three ways in alternating rounds (the minimum of three rounds each, on the same seeded
frames): the eager composition of the public calls (device_letterbox, the forward, decode_outputs, non_max_suppression with
its two read-backs, seg_predict, render_frame with its upload of the box rows), infer.FramePipeline(graph=False) and
infer.FramePipeline(graph=True), at the thresholds of the first --nms pair (default 0.5/0.4), with the candidate and kept
counts of the frames.  With --evaluate HxW[,HxW...] it times a validation pass of --steps batches of frames of each
original size H x W resident on the device, two ways in alternating rounds (the minimum of three rounds each, on the same
seeded frames, label maps and ground truths): evaluate.EvalPipeline.add per batch, and the per-image path that existed
before it -- infer.FramePipeline(batch=1).run + metrics.DetectionEvaluator.add (one device-to-host copy per image) +
metrics.fast_hist -- in images/s, at the thresholds of the first --nms pair (default 0.05/0.5, EvalCallback's), with the mAP
and mIoU of both.  With --ragged HxW[,HxW...] it compares infer.FramePipeline(ragged=True) of capacity H x W, every frame AT
the capacity (the ragged kernels then move the fixed ones' bytes plus the geometry table), with the fixed-size captured
pipeline at the same shapes on the same frames resident on the device: seven alternating rounds of --steps runs each, frames
per second from the median round of each, the fixed pipeline's own run-to-run spread beside the ratio, and whether the
results are equal.  With --heatmap HxW[,HxW...] it times the detection heat map of the raw detection maps of the forward at each
original size H x W, on frames resident on the device: render.heatmap_mask, render.heatmap and its aligned form, each captured
in a hipGraph of its own and replayed --steps times between two device events (device time: no launch gaps of the host), in
alternating rounds, next to a plain device copy of the same frame bytes measured the same way (the bound of a byte-bound
pass: the heat map reads 3 and writes 1 + 3 bytes per pixel, the copy reads 3 and writes 3); and the replay of
infer.FramePipeline with and without heatmap=True (without it: the chain as it was before the option existed).
With --labels HxW[,HxW...] it times the replay of infer.FramePipeline(graph=True) without labels (the chain as it was before
the option existed) and with labels=True (Pillow's built-in face) on the same seeded frames of each original size H x W, in
alternating rounds, once per --nms pair (default 0.5/0.4), with the kept counts and the atlas bytes; and, on the rows of that
run, the device time of the two label launches alone (hip.label_index + render.draw_labels, captured and replayed) at the
frame's own font size, at half that size (a quarter of the label area on the same frame) and on the first half of every
image's rows.

    python tools/bench_infer.py [--phi l] [--size 512] [--batches 1,8,32] [--dtype f32|bf16] [--nms 0.05/0.5,0.3/0.5]
                                [--seg 1080x1920,480x640] [--letterbox 1080x1920,480x640] [--render 1080x1920,480x640]
                                [--pipeline 1080x1920] [--evaluate 1080x1920] [--ragged 1080x1920]
                                [--heatmap 1080x1920,480x640] [--labels 1080x1920,540x960]
"""
import argparse
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--phi", default="l")
    ap.add_argument("--size", type=int, default=512)
    ap.add_argument("--batches", default="1,8,32")
    ap.add_argument("--dtype", default="f32", choices=["f32", "bf16"])
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--nms", default="", help="comma list of conf/iou threshold pairs (e.g. 0.05/0.5,0.001/0.5)")
    ap.add_argument("--seg", default="", help="comma list of original image sizes HxW (e.g. 1080x1920,480x640)")
    ap.add_argument("--letterbox", default="", help="comma list of original frame sizes HxW (e.g. 1080x1920,480x640)")
    ap.add_argument("--render", default="", help="comma list of original frame sizes HxW (e.g. 1080x1920,480x640)")
    ap.add_argument("--pipeline", default="", help="comma list of original frame sizes HxW (e.g. 1080x1920)")
    ap.add_argument("--evaluate", default="", help="comma list of original frame sizes HxW (e.g. 1080x1920)")
    ap.add_argument("--ragged", default="", help="comma list of capacities HxW (e.g. 1080x1920)")
    ap.add_argument("--heatmap", default="", help="comma list of original frame sizes HxW (e.g. 1080x1920,480x640)")
    ap.add_argument("--labels", default="", help="comma list of original frame sizes HxW (e.g. 1080x1920,540x960)")
    args = ap.parse_args()
    import asy_vrnet_amd as A
    from asy_vrnet_amd.data import device_letterbox, resize_image
    from asy_vrnet_amd.decode import decode_outputs, non_max_suppression, seg_predict
    from asy_vrnet_amd.metrics import f_score, fast_hist
    from asy_vrnet_amd.infer import FramePipeline
    from asy_vrnet_amd.render import MAX_BOXES, det_palette, render_frame, seg_palette, seg_render
    pairs = [tuple(float(v) for v in p.split("/")) for p in args.nms.split(",") if p]
    seg_sizes = [tuple(int(v) for v in p.split("x")) for p in args.seg.split(",") if p]
    frame_sizes = [tuple(int(v) for v in p.split("x")) for p in args.letterbox.split(",") if p]
    render_sizes = [tuple(int(v) for v in p.split("x")) for p in args.render.split(",") if p]
    pipeline_sizes = [tuple(int(v) for v in p.split("x")) for p in args.pipeline.split(",") if p]
    evaluate_sizes = [tuple(int(v) for v in p.split("x")) for p in args.evaluate.split(",") if p]
    ragged_sizes = [tuple(int(v) for v in p.split("x")) for p in args.ragged.split(",") if p]
    heat_sizes = [tuple(int(v) for v in p.split("x")) for p in args.heatmap.split(",") if p]
    label_sizes = [tuple(int(v) for v in p.split("x")) for p in args.labels.split(",") if p]

    def timed(fn):
        for _ in range(3):
            fn()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(args.steps):
            fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) / args.steps * 1e3

    def replayed(fn):
        """fn captured in a graph of its own (after two passes on the capture stream): a function that replays it --steps
        times and returns the device time per replay in ms, from two events on the stream."""
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.no_grad(), torch.cuda.stream(side):
            for _ in range(2):
                fn()
        torch.cuda.current_stream().wait_stream(side)
        torch.cuda.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.no_grad(), torch.cuda.graph(graph, stream=side):
            keep = fn()

        def measure():
            for _ in range(3):
                graph.replay()
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for _ in range(args.steps):
                graph.replay()
            b.record()
            torch.cuda.synchronize()
            return a.elapsed_time(b) / args.steps
        measure.keep = keep
        return measure
    dev = torch.device("cuda")
    model = A.EfficientVRNet(4, 9, args.phi, img_size=args.size).to(dev).eval()
    A.randomize_state_dict(model.state_dict(), seed=0)
    model.compute_dtype = args.dtype
    for bs in [int(b) for b in args.batches.split(",")]:
        x, r = A.synthetic_inputs(bs, args.size, 1, dev)

        def run():
            det, seg = model(x, r)
            return decode_outputs(det, (args.size, args.size)), seg

        with torch.no_grad():
            side = torch.cuda.Stream()
            side.wait_stream(torch.cuda.current_stream())
            with torch.cuda.stream(side):
                for _ in range(2):
                    run()
            torch.cuda.current_stream().wait_stream(side)
            torch.cuda.synchronize()
            g = torch.cuda.CUDAGraph()
            with torch.cuda.graph(g):
                out = run()
            for _ in range(3):
                g.replay()
            torch.cuda.synchronize()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(args.steps):
                g.replay()
            e1.record()
            torch.cuda.synchronize()
        ms = e0.elapsed_time(e1) / args.steps
        print(f"phi={args.phi} {args.size}x{args.size} {args.dtype} eval forward + decode, bs={bs}: {ms:.3f} ms/batch, "
              f"{bs / ms * 1e3:.1f} img/s; boxes {tuple(out[0].shape)}, seg {tuple(out[1].shape)}")
        S = (args.size, args.size)
        for conf, iou in pairs:
            def post():
                return non_max_suppression(out[0], model.num_classes, S, S, True, conf_thres=conf, nms_thres=iou)

            g.replay()
            dets = post()
            nms_ms = timed(post)
            full_ms = timed(lambda: (g.replay(), post()))
            cand = int(((out[0][..., 4:5] * out[0][..., 5:5 + model.num_classes]).amax(-1) >= conf).sum())
            print(f"  + non_max_suppression conf {conf} iou {iou}, bs={bs}: {full_ms:.3f} ms/batch "
                  f"(NMS alone {nms_ms:.3f} ms); candidates {cand}, kept {sum(len(d) for d in dets)}")

        if seg_sizes:
            g.replay()
            seg = out[1]
            ns = seg.shape[1]
            gen = torch.Generator(device=dev).manual_seed(bs)
            for ih, iw in seg_sizes:
                pred_ms = timed(lambda: seg_predict(seg, S, (ih, iw)))
                full_ms = timed(lambda: (g.replay(), seg_predict(seg, S, (ih, iw))))
                pred = seg_predict(seg, S, (ih, iw))
                labels = torch.randint(0, ns + 1, (bs, ih, iw), generator=gen, device=dev, dtype=torch.uint8)
                hist_ms = timed(lambda: fast_hist(labels, pred, ns))
                print(f"  + seg_predict to {ih}x{iw}, bs={bs}: {full_ms:.3f} ms/batch (seg_predict alone {pred_ms:.3f} ms); "
                      f"fast_hist of the {bs}x{ih}x{iw} map {hist_ms:.3f} ms")
            target = torch.nn.functional.one_hot(
                torch.randint(0, ns + 1, (bs,) + S, generator=gen, device=dev), ns + 1).float()
            f_ms = timed(lambda: f_score(seg, target))
            e_ms = timed(lambda: f_score_eager(seg, target))
            a, b = float(f_score(seg, target)), float(f_score_eager(seg, target))
            print(f"  + f_score {bs}x{ns}x{S[0]}x{S[1]}: {f_ms:.3f} ms (eager torch {e_ms:.3f} ms); value {a:.6f} "
                  f"(eager {b:.6f})")

        for ih, iw in frame_sizes:
            gen = torch.Generator().manual_seed(bs)
            pinned = torch.randint(0, 256, (bs, ih, iw, 3), generator=gen, dtype=torch.uint8).pin_memory()
            resident = pinned.to(dev)
            dev_ms = timed(lambda: device_letterbox(resident, S))
            copy_ms = timed(lambda: device_letterbox(pinned, S))
            line = (f"  + device_letterbox {ih}x{iw} -> {S[0]}x{S[1]}, bs={bs}: {dev_ms:.3f} ms/batch on resident frames, "
                    f"{copy_ms:.3f} ms/batch with the copy from pinned memory ({copy_ms / bs:.3f} ms/image; "
                    f"{ih * iw * 3 / 1e6:.2f} MB/image over PCIe, against {S[0] * S[1] * 3 / 1e6:.2f} MB letterboxed)")
            try:
                from PIL import Image
            except ImportError:
                print(line + "; Pillow not installed")
                continue
            pil = [Image.fromarray(f) for f in pinned.numpy()]
            resize_image(pil[0], (S[1], S[0]))
            t0 = time.perf_counter()
            for _ in range(3):
                for im in pil:
                    resize_image(im, (S[1], S[0]))
            pil_ms = (time.perf_counter() - t0) / (3 * bs) * 1e3
            print(line + f"; Pillow resize_image on one core {pil_ms:.3f} ms/image")

        for ih, iw in render_sizes:
            import numpy as np
            g.replay()
            gen = torch.Generator(device=dev).manual_seed(bs)
            frames = torch.randint(0, 256, (bs, ih, iw, 3), generator=gen, device=dev, dtype=torch.uint8)
            cmap = seg_predict(out[1], S, (ih, iw))
            pal, bpal = torch.from_numpy(seg_palette(9)).to(dev), torch.from_numpy(det_palette(4)).to(dev)
            rng = np.random.default_rng(bs)
            left, top = rng.integers(0, iw - 8, (bs * 100)), rng.integers(0, ih - 8, (bs * 100))
            rows = np.stack([left, top, np.minimum(left + rng.integers(8, iw // 3, bs * 100), iw),
                             np.minimum(top + rng.integers(8, ih // 3, bs * 100), ih), rng.integers(0, 4, bs * 100)], axis=1)
            boxes = (torch.from_numpy(rows.astype(np.int32)).to(dev), torch.arange(0, bs * 100 + 1, 100, dtype=torch.int32, device=dev))
            thick = max((ih + iw) // args.size, 1)
            dst = torch.empty_like(frames)
            inplace = frames.clone()
            # alternating rounds of the four device variants, so that a drift of the clock hits them alike
            variants = {"copy": lambda: dst.copy_(frames),
                        "seg_render": lambda: seg_render(frames, cmap, pal, 0, 0.7, count=True, out=dst),
                        "render_frame": lambda: render_frame(frames, cmap, boxes, palette=pal, box_palette=bpal, thickness=thick,
                                                             count=True, out=dst),
                        "boxes_in_place": lambda: render_frame(inplace, None, boxes, box_palette=bpal, thickness=thick, out=inplace)}
            ms = {k: min(timed(fn) for _ in range(3)) for k, fn in variants.items()}
            mb = bs * ih * iw * 3 / 1e6
            line = (f"  + render {ih}x{iw}, bs={bs}: device copy of the frames {ms['copy']:.4f} ms ({2 * mb / ms['copy']:.0f} GB/s read + "
                    f"written); seg_render mix 0 + counts {ms['seg_render']:.4f} ms ({7 * mb / 3 / ms['seg_render']:.0f} GB/s "
                    f"of its 7 B/pixel: {7 / 6 * ms['copy'] / ms['seg_render']:.2f} of the copy's rate); render_frame with 100 boxes/image, thickness {thick}, {ms['render_frame']:.4f} ms "
                    f"({ms['render_frame'] / ms['seg_render']:.2f} x the no-box call); the boxes alone in place "
                    f"{ms['boxes_in_place']:.4f} ms; {mb / bs:.2f} MB/image rendered on the device instead of "
                    f"{ih * iw / 1e6:.2f} MB of class map down and back")
            try:
                from PIL import Image
            except ImportError:
                print(line + "; Pillow not installed")
                continue
            host_frames, host_map, host_pal = frames.cpu().numpy(), cmap.cpu().numpy(), seg_palette(9)
            t0 = time.perf_counter()
            for b in range(min(bs, 2)):
                seg_img = np.reshape(host_pal[np.reshape(host_map[b], [-1])], [ih, iw, -1])
                Image.blend(Image.fromarray(host_frames[b]), Image.fromarray(np.uint8(seg_img)), 0.7)
                np.bincount(host_map[b].reshape(-1), minlength=9)
            host_ms = (time.perf_counter() - t0) / min(bs, 2) * 1e3
            print(line + f"; host path on one core (numpy palette lookup + Image.blend + bincount) {host_ms:.3f} ms/image")

        for ih, iw in pipeline_sizes:
            conf, iou = pairs[0] if pairs else (0.5, 0.4)
            gen = torch.Generator().manual_seed(bs)
            frames = torch.randint(0, 256, (bs, ih, iw, 3), generator=gen, dtype=torch.uint8).to(dev)
            pal, bpal = torch.from_numpy(seg_palette(9)).to(dev), torch.from_numpy(det_palette(model.num_classes)).to(dev)

            def composed():
                images, _ = device_letterbox(frames, S)
                with torch.no_grad():
                    det, seg = model(images, r)
                results = non_max_suppression(decode_outputs(det, S), model.num_classes, S, (ih, iw), True, conf_thres=conf,
                                              nms_thres=iou)
                cmap = seg_predict(seg, S, (ih, iw))
                return render_frame(frames, cmap, [d[:MAX_BOXES] for d in results], S, palette=pal, box_palette=bpal, count=True)

            pipes = {g: FramePipeline(model, (ih, iw), S, batch=bs, conf_thres=conf, nms_thres=iou, seg_palette=pal,
                                      box_palette=bpal, graph=g) for g in (False, True)}
            variants = {"composition": composed, "pipeline_eager": lambda: pipes[False].run(frames, r),
                        "pipeline_captured": lambda: pipes[True].run(frames, r)}
            rounds = {k: [] for k in variants}
            for _ in range(3):                       # alternating rounds, so that a drift of the clock hits them alike
                for k, fn in variants.items():
                    rounds[k].append(timed(fn))
            ms = {k: min(v) for k, v in rounds.items()}
            res = pipes[True].run(frames, r)
            same = torch.equal(res.rendered, composed()[0])
            print(f"  + pipeline {ih}x{iw} -> rendered frame, conf {conf} iou {iou}, bs={bs}: eager composition of the public calls "
                  f"{ms['composition']:.3f} ms/batch, FramePipeline eager {ms['pipeline_eager']:.3f} ms, captured "
                  f"{ms['pipeline_captured']:.3f} ms ({ms['composition'] / ms['pipeline_captured']:.2f} x the composition, "
                  f"{bs / ms['pipeline_captured'] * 1e3:.1f} frames/s); candidates {pipes[True]._cand[4].tolist()} of capacity "
                  f"{pipes[True].cap}, kept {res.kept.tolist()}, flag {int(res.flag)}; rendered frames equal the composition's: {same}")

        for ih, iw in heat_sizes:
            import statistics
            from asy_vrnet_amd.render import heatmap, heatmap_mask
            with torch.no_grad():
                det = [d.detach().float().contiguous() for d in model(x, r)[0]]
            gen = torch.Generator(device=dev).manual_seed(bs)
            frames = torch.randint(0, 256, (bs, ih, iw, 3), generator=gen, device=dev, dtype=torch.uint8)
            dst = torch.empty_like(frames)
            variants = {"copy": replayed(lambda: dst.copy_(frames)),
                        "mask": replayed(lambda: heatmap_mask(det, (ih, iw), S)),
                        "heatmap": replayed(lambda: heatmap(frames, det, S, out=dst)),
                        "aligned": replayed(lambda: heatmap(frames, det, S, letterbox_image=True, out=dst))}
            rounds = {k: [] for k in variants}
            for _ in range(5):                       # alternating rounds, so that a drift of the clock hits them alike
                for k, fn in variants.items():
                    rounds[k].append(fn())
            ms = {k: statistics.median(v) for k, v in rounds.items()}
            mb = bs * ih * iw / 1e6
            print(f"  + heatmap {ih}x{iw} from {S[0]}x{S[1]}, bs={bs}, device time per captured replay (median of 5 rounds of "
                  f"{args.steps}): device copy of the frames {ms['copy']:.4f} ms ({6 * mb / ms['copy']:.0f} GB/s read + written); "
                  f"heatmap_mask {ms['mask']:.4f} ms ({ms['mask'] / ms['copy']:.2f} x the copy, 1 B/pixel written); heatmap "
                  f"{ms['heatmap']:.4f} ms ({ms['heatmap'] / ms['copy']:.2f} x the copy; {8 * mb / ms['heatmap']:.0f} GB/s of its "
                  f"1 + 1 + 3 + 3 B/pixel); aligned form {ms['aligned']:.4f} ms; rounds of heatmap min {min(rounds['heatmap']):.4f} "
                  f"max {max(rounds['heatmap']):.4f} ms")
            pipes = {h: FramePipeline(model, (ih, iw), S, batch=bs, heatmap=h) for h in (False, True)}
            rounds = {h: [] for h in pipes}
            for _ in range(5):
                for h, pipe in pipes.items():
                    rounds[h].append(timed(lambda: pipe.run(frames, r)))
            med = {h: statistics.median(v) for h, v in rounds.items()}
            a, b = pipes[False].run(frames, r), pipes[True].run(frames, r)
            same = all(torch.equal(getattr(a, k), getattr(b, k)) for k in ("rows", "kept", "det_counts", "class_map", "seg_counts",
                                                                           "rendered"))
            print(f"  + heatmap {ih}x{iw}, bs={bs}: FramePipeline replay without heatmap {med[False]:.3f} ms/batch (rounds "
                  f"{min(rounds[False]):.3f}..{max(rounds[False]):.3f}), with heatmap=True {med[True]:.3f} ms/batch (rounds "
                  f"{min(rounds[True]):.3f}..{max(rounds[True]):.3f}): +{med[True] - med[False]:.3f} ms; heat range "
                  f"{b.heat_range.tolist()}; other fields equal: {same}")

        for ih, iw in label_sizes:
            import statistics
            from asy_vrnet_amd import hip, render as rendering
            gen = torch.Generator().manual_seed(bs)
            frames = torch.randint(0, 256, (bs, ih, iw, 3), generator=gen, dtype=torch.uint8).to(dev)
            names = [f"class {c}" for c in range(model.num_classes)]
            size = rendering.label_font_size(ih)
            atlas = rendering.LabelAtlas(names, None, sorted({size, max(size // 2, 1)}))
            for conf, iou in pairs or [(0.5, 0.4)]:
                pipes = {lab: FramePipeline(model, (ih, iw), S, batch=bs, conf_thres=conf, nms_thres=iou, labels=lab)
                         for lab in (None, atlas)}
                rounds = {lab: [] for lab in pipes}
                for _ in range(5):                   # alternating rounds, so that a drift of the clock hits them alike
                    for lab, pipe in pipes.items():
                        rounds[lab].append(timed(lambda: pipe.run(frames, r)))
                med = {lab: statistics.median(v) for lab, v in rounds.items()}
                a, b = pipes[None].run(frames, r), pipes[atlas].run(frames, r)
                same = all(torch.equal(getattr(a, k), getattr(b, k)) for k in ("rows", "kept", "det_counts", "class_map", "seg_counts"))
                kept = b.kept.tolist()
                print(f"  + labels {ih}x{iw}, font size {size}, conf {conf} iou {iou}, bs={bs}: FramePipeline replay without labels "
                      f"{med[None]:.3f} ms/batch (rounds {min(rounds[None]):.3f}..{max(rounds[None]):.3f}), with labels "
                      f"{med[atlas]:.3f} ms/batch (rounds {min(rounds[atlas]):.3f}..{max(rounds[atlas]):.3f}): "
                      f"{(med[atlas] - med[None]) / bs * 1e3:+.1f} us/frame; kept {kept}, flag {int(b.flag)}; atlas {atlas.nbytes} bytes "
                      f"for sizes {atlas.sizes}; other fields equal: {same}; picture changed: {not torch.equal(a.rendered, b.rendered)}")
                # the two label launches alone, on the rows of that run
                p = pipes[atlas]
                rows, offsets, idx = p._draw_rows.clone(), p._offsets.clone(), torch.zeros_like(p._label_idx)
                keptrows, kept_t, picture = p._rows.clone(), p._kept.clone(), a.rendered.clone()
                hip.label_index(keptrows, kept_t, offsets, model.num_classes, idx)
                o = offsets.tolist()
                firsts = [(o[i + 1] - o[i] + 1) // 2 for i in range(bs)]             # image b keeps the first half of its rows
                sel = torch.cat([torch.arange(o[i], o[i] + firsts[i]) for i in range(bs)]).to(dev)
                half = (rows[sel].contiguous(), torch.tensor([sum(firsts[:i]) for i in range(bs + 1)], dtype=torch.int32).to(dev),
                        idx[sel].contiguous())

                def alone(font, triple):
                    hip.label_index(keptrows, kept_t, offsets, model.num_classes, idx)
                    return rendering.draw_labels(picture, triple, atlas, thickness=p.thickness, font_size=font)

                variants = {"own size": replayed(lambda: alone(size, (rows, offsets, idx))),
                            "half size": replayed(lambda: alone(max(size // 2, 1), (rows, offsets, idx))),
                            "half the rows": replayed(lambda: alone(size, half))}
                rounds = {k: [] for k in variants}
                for _ in range(5):
                    for k, fn in variants.items():
                        rounds[k].append(fn())
                us = {k: statistics.median(v) * 1e3 for k, v in rounds.items()}
                area = {f: sum(int(atlas.records[atlas.size_index(f), i, 5] + 1) * int(atlas.records[atlas.size_index(f), i, 6] + 1)
                               for i in idx[:int(offsets[-1])].tolist()) for f in {size, max(size // 2, 1)}}
                print(f"  + labels {ih}x{iw}, bs={bs}, device time of label_index + render_labels per captured replay (median of 5 "
                      f"rounds of {args.steps}): font {size} {us['own size']:.1f} us (tags {area[size]} px of {bs * ih * iw} px); "
                      f"font {max(size // 2, 1)} {us['half size']:.1f} us (tags {area[max(size // 2, 1)]} px); font {size}, first half "
                      f"of every image's rows {us['half the rows']:.1f} us")

        for ih, iw in ragged_sizes:
            import statistics
            conf, iou = pairs[0] if pairs else (0.5, 0.4)
            gen = torch.Generator().manual_seed(bs)
            frames = torch.randint(0, 256, (bs, ih, iw, 3), generator=gen, dtype=torch.uint8).to(dev)
            sizes = [(ih, iw)] * bs
            pipes = {k: FramePipeline(model, (ih, iw), S, batch=bs, conf_thres=conf, nms_thres=iou, ragged=(k == "ragged"))
                     for k in ("fixed", "ragged")}
            variants = {"fixed": lambda: pipes["fixed"].run(frames, r), "ragged": lambda: pipes["ragged"].run(frames, r, sizes)}
            rounds = {k: [] for k in variants}
            for _ in range(7):                       # alternating rounds, so that a drift of the clock hits them alike
                for k, fn in variants.items():
                    rounds[k].append(timed(fn))
            med = {k: statistics.median(v) for k, v in rounds.items()}
            a, b = pipes["fixed"].run(frames, r), pipes["ragged"].run(frames, r, sizes)
            same = all(torch.equal(getattr(a, k), getattr(b, k)) for k in ("rows", "kept", "det_counts", "class_map", "seg_counts",
                                                                           "rendered"))
            for k in ("fixed", "ragged"):
                print(f"  + ragged {ih}x{iw}, conf {conf} iou {iou}, bs={bs}: {k} captured pipeline median {med[k]:.3f} ms/batch "
                      f"({bs / med[k] * 1e3:.1f} frames/s), rounds min {min(rounds[k]):.3f} max {max(rounds[k]):.3f} ms")
            print(f"  + ragged {ih}x{iw}, bs={bs}: ragged / fixed time {med['ragged'] / med['fixed']:.4f} (the fixed pipeline's own rounds "
                  f"span {max(rounds['fixed']) / min(rounds['fixed']):.4f}); flags {int(a.flag)} {int(b.flag)}; results equal: {same}")

        for ih, iw in evaluate_sizes:
            import numpy as np
            from asy_vrnet_amd.evaluate import EvalPipeline
            from asy_vrnet_amd.metrics import DetectionEvaluator
            conf, iou = pairs[0] if pairs else (0.05, 0.5)
            ns, names, n_batches = model.num_seg_classes, [str(c) for c in range(model.num_classes)], args.steps
            gen = torch.Generator().manual_seed(bs)
            frames = torch.randint(0, 256, (bs, ih, iw, 3), generator=gen, dtype=torch.uint8).to(dev)
            labels = torch.randint(0, ns + 1, (bs, ih, iw), generator=gen, dtype=torch.uint8).to(dev)
            rng = np.random.default_rng(bs)
            x1, y1 = rng.integers(0, iw // 2, (bs, 4)), rng.integers(0, ih // 2, (bs, 4))
            gts = [np.stack([x1[b], y1[b], x1[b] + iw // 4, y1[b] + ih // 4, rng.integers(0, model.num_classes, 4)], axis=1)
                   for b in range(bs)]
            batched = EvalPipeline(model, (ih, iw), S, names, ns, batch=bs, capacity=bs * n_batches, conf_thres=conf, nms_thres=iou)
            single = FramePipeline(model, (ih, iw), S, batch=1, conf_thres=conf, nms_thres=iou, render=False)
            ev, hist = DetectionEvaluator(names), torch.zeros((ns, ns), dtype=torch.int64, device=dev)

            def captured_pass():
                batched.reset()
                for k in range(n_batches):
                    batched.add([f"{k}_{b}" for b in range(bs)], frames, r, labels, gts)

            def per_image_pass():                 # the path before EvalPipeline: one device-to-host copy per image
                ev.reset()
                hist.zero_()
                for k in range(n_batches):
                    for b in range(bs):
                        res = single.run(frames[b:b + 1], r[b:b + 1])
                        ev.add(f"{k}_{b}", res.detections()[0], gts[b])
                        fast_hist(labels[b], res.class_map, ns, out=hist)

            def seconds(fn):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                fn()
                torch.cuda.synchronize()
                return time.perf_counter() - t0

            variants = {"captured": captured_pass, "per_image": per_image_pass}
            rounds = {k: [] for k in variants}
            for _ in range(3):                       # alternating rounds, so that a drift of the clock hits them alike
                for k, fn in variants.items():
                    rounds[k].append(seconds(fn))
            sec, n_img = {k: min(v) for k, v in rounds.items()}, bs * n_batches
            res = batched.compute(strict=False)
            print(f"  + evaluate {ih}x{iw}, conf {conf} iou {iou}, bs={bs}, {n_img} images: EvalPipeline.add {n_img / sec['captured']:.1f} "
                  f"images/s; per image (FramePipeline.run + DetectionEvaluator.add + fast_hist) {n_img / sec['per_image']:.1f} "
                  f"images/s ({sec['per_image'] / sec['captured']:.2f} x); mAP {float(res.det.map):.6f} (per image "
                  f"{float(ev.compute().map):.6f}), mIoU {res.miou:.6f}, flag {res.flag}; confusion matrices equal: "
                  f"{bool((torch.from_numpy(res.hist).to(dev) == hist).all())}")


def f_score_eager(x, target, beta=1, smooth=1e-5, threshold=0.5):
    """The f_score metric as plain torch operations, for comparison: softmax over the channels, threshold, per-class
    true-positive / predicted / target sums over every pixel, the F-beta mean."""
    n, c = x.shape[:2]
    p = torch.softmax(x.float().permute(0, 2, 3, 1).reshape(n, -1, c), dim=-1)
    hit = (p > threshold).float()
    t = target.reshape(n, -1, c + 1)[..., :c]
    tp = (t * hit).sum(dim=(0, 1))
    fp = hit.sum(dim=(0, 1)) - tp
    fn = t.sum(dim=(0, 1)) - tp
    b2 = beta * beta
    return (((1 + b2) * tp + smooth) / ((1 + b2) * tp + b2 * fn + fp + smooth)).mean()


if __name__ == "__main__":
    main()
