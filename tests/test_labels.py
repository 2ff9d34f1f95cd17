"""The label kernels (csrc/labels.hip) against render.draw_labels_host, byte for byte -- tests/test_labels_host.py pins that
statement to live Pillow -- and the score index on the device against render.score_index.  The atlas is built with Pillow
when it imports, otherwise it is the committed fixture of the same face."""
import numpy as np
import pytest
import torch

import asy_vrnet_amd as A
from asy_vrnet_amd import data, decode, render
from tests import labels_cases as LC

pytestmark = pytest.mark.gpu
NC = len(LC.CLASS_NAMES)
PAL = render.det_palette(NC)


def cuda(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def new_flag():
    return torch.zeros(1, dtype=torch.int32, device="cuda")


def host_pictures(frames, rows, offsets, scores, font_size, thickness):
    atlas = LC.atlas()
    return np.stack([render.draw_labels_host(frames[b], rows[offsets[b]:offsets[b + 1]], scores[offsets[b]:offsets[b + 1]], atlas,
                                             font_size, thickness, PAL) for b in range(len(frames))])


def check_device(frames, cases, font_size, thickness, want_flag=0):
    """render_frame then draw_labels on device triples, and render_frame(labels=) in one call, against the host statement."""
    atlas = LC.atlas()
    rows, offsets, scores = LC.pack(cases)
    triple = (cuda(rows), cuda(offsets), cuda(LC.label_indices(rows, scores)))
    src, flag = cuda(frames), new_flag()
    plain = render.render_frame(src, None, triple[:2], box_palette=PAL, thickness=thickness, flag=flag)
    outlines = plain.clone()
    got = render.draw_labels(plain, triple, atlas, thickness=thickness, font_size=font_size, box_palette=PAL, flag=flag)
    assert got is plain and torch.equal(src, cuda(frames))
    want = host_pictures(frames, rows, offsets, scores, font_size, thickness)
    bad = int((got.cpu().numpy() != want).any(axis=3).sum())
    print(f"labels {frames.shape} font {font_size} thickness {thickness} rows {np.diff(offsets).tolist()}: {bad} pixels differ, "
          f"flag {int(flag)}")
    assert np.array_equal(got.cpu().numpy(), want)
    assert int(flag) == want_flag
    once = render.render_frame(src, None, triple, box_palette=PAL, thickness=thickness, labels=atlas, font_size=font_size)
    assert torch.equal(once, got)
    if rows.size and (font_size is None or font_size > 0) and render.label_font_size(frames.shape[1]) > 0:
        assert not torch.equal(outlines, got)                # not vacuous: the labels changed the picture
    return got


@pytest.mark.parametrize("B,ih,iw,font_size", [(2, 64, 96, 10), (1, 33, 47, 8), (3, 270, 480, None), (1, 17, 17, None)])
def test_device_equals_the_host_statement(B, ih, iw, font_size):
    assert render.label_font_size(270) == 8 and render.label_font_size(17) == 1
    rng = np.random.default_rng(100 * ih + B)
    frames = rng.integers(0, 256, (B, ih, iw, 3), dtype=np.uint8)
    counts = {1: ([40], [1], [0]), 2: ([40, 1], [0, 40], [0, 0]), 3: ([40, 0, 1], [1, 40, 0])}[B]
    for thickness, per_image in zip((1, 3, 2), counts):
        cases = [LC.random_case(rng, ih, iw, n, thickness) for n in per_image]
        check_device(frames, cases, font_size, thickness)


def test_more_than_1024_rows_are_flagged_and_the_first_1024_drawn():
    rng = np.random.default_rng(5)
    frames = rng.integers(0, 256, (2, 64, 96, 3), dtype=np.uint8)
    cases = [LC.random_case(rng, 64, 96, 3, 1), LC.random_case(rng, 64, 96, render.MAX_BOXES + 1, 1)]
    cases[1][0][-1] = (0, 30, 90, 60, 2)                     # the row that is dropped would cover half the picture
    check_device(frames, cases, 10, 1, want_flag=render.FLAG_BOX_ROWS)
    kept = [cases[0], (cases[1][0][:-1], cases[1][1][:-1])]
    rows, offsets, scores = LC.pack(cases)
    assert np.array_equal(host_pictures(frames, rows, offsets, scores, 10, 1), host_pictures(frames, *LC.pack(kept), 10, 1))


def test_data_errors_are_clamped_and_flagged():
    """A label index and a colour outside their tables are clamped, never read past them."""
    rng = np.random.default_rng(6)
    frames = rng.integers(0, 256, (1, 64, 96, 3), dtype=np.uint8)
    rows, scores = LC.random_case(rng, 64, 96, 4, 2)
    rows[:3, 4] = (0, NC - 1, NC + 3)                        # the third colour lies outside the palette
    scores[:2] = (0.0, 1.0)
    offsets = np.array([0, 4], np.int32)
    wild = LC.label_indices(rows, scores)
    assert wild[0] == 0 and wild[1] == NC * 101 - 1 and wild[2] // 101 == NC - 1
    wild[0], wild[1] = -5, NC * 101 + 1000                   # clamped to the first and the last label: what the rows say
    flag = new_flag()
    pic = render.render_frame(cuda(frames), None, (cuda(rows), cuda(offsets)), box_palette=PAL, thickness=2, flag=flag)
    got = render.draw_labels(pic, (cuda(rows), cuda(offsets), cuda(wild)), LC.atlas(), thickness=2, font_size=10, box_palette=PAL,
                             flag=flag)
    want = render.draw_labels_host(frames[0], rows, scores, LC.atlas(), 10, 2, PAL)
    assert np.array_equal(got.cpu().numpy()[0], want) and int(flag) == render.FLAG_BOX_COLOUR


def test_label_index_equals_score_index():
    import asy_vrnet_amd.hip as hip
    import asy_vrnet_amd.ops  # noqa: F401
    ties = []
    for k in range(101):
        x = np.float32((k + 0.5) / 100)
        ties += [np.nextafter(x, np.float32(0)), x, np.nextafter(x, np.float32(2))]
    ties += [0.125, 0.375, 0.625, 0.875, 0.0, 1.0, 1e-45, 1e-40, 1.1754942e-38]
    s = np.array(ties, np.float32)
    s = s[s <= 1]
    rng = np.random.default_rng(8)
    obj, conf = rng.random(300, dtype=np.float32), rng.random(300, dtype=np.float32)
    B, kept = 3, np.array([len(s) - 200, 200, 300], np.int32)
    cap = int(kept.max()) + 7
    rows = np.zeros((B, cap, 7), np.float32)
    rows[..., 4:6] = np.nan                                   # rows at and past kept[b] are never read
    rows[0, :kept[0], 4], rows[0, :kept[0], 5] = s[:kept[0]], 1.0
    rows[1, :kept[1], 4], rows[1, :kept[1], 5] = 1.0, s[kept[0]:]
    rows[2, :kept[2], 4], rows[2, :kept[2], 5] = obj, conf
    cls = rng.integers(0, NC, (B, cap)).astype(np.float32)
    rows[..., 6] = cls
    offsets = np.concatenate([[0], np.cumsum(kept)]).astype(np.int32)
    out, flag = torch.full((B * cap,), -7, dtype=torch.int32, device="cuda"), new_flag()
    hip.label_index(cuda(rows), cuda(kept), cuda(offsets), NC, out, flag)
    got = out.cpu().numpy()
    scores = np.concatenate([s[:kept[0]], s[kept[0]:], obj * conf]).astype(np.float32)
    classes = np.concatenate([cls[b, :kept[b]] for b in range(B)]).astype(np.int64)
    want = classes * 101 + render.score_index(scores)
    assert [int("{:.2f}".format(float(v)).replace(".", "")) for v in scores] == render.score_index(scores).tolist()
    assert np.array_equal(got[:offsets[-1]], want) and (got[offsets[-1]:] == -7).all() and int(flag) == 0
    assert np.array_equal(torch.ops.vrnet.label_index(cuda(rows), cuda(kept), cuda(offsets), NC).cpu().numpy()[:offsets[-1]], want)
    # bad scores and classes: clamped, and each sets its bit
    bad = np.zeros((1, 8, 7), np.float32)
    bad[0, :6, 4] = (np.nan, -0.1, 1.5, 0.5, 0.5, 0.5)
    bad[0, :6, 5] = 1.0
    bad[0, :6, 6] = (0, 1, 2, -1, NC, 3)
    for n, want_idx, want_flag in ((3, [0, 101, 2 * 101 + 100], render.FLAG_LABEL_SCORE),
                                   (6, [0, 101, 302, 50, (NC - 1) * 101 + 50, 3 * 101 + 50], render.FLAG_LABEL_SCORE | 16)):
        out, flag = torch.zeros(8, dtype=torch.int32, device="cuda"), new_flag()
        hip.label_index(cuda(bad), cuda(np.array([n], np.int32)), cuda(np.array([0, n], np.int32)), NC, out, flag)
        assert out.cpu().numpy()[:n].tolist() == want_idx and int(flag) == want_flag
    out, flag = torch.zeros(8, dtype=torch.int32, device="cuda"), new_flag()
    hip.label_index(cuda(bad[:, 3:]), cuda(np.array([3], np.int32)), cuda(np.array([0, 3], np.int32)), NC, out, flag)
    assert int(flag) == 16                                    # FLAG_DET_CLASS alone


def geom_tensor(table):
    return cuda(table.view(np.uint8).reshape(len(table), -1))


def test_ragged_equals_the_fixed_call_per_image_and_is_zero_outside():
    atlas, S, cap = LC.atlas(), (64, 64), (320, 100)
    sizes = [(40, 60), (270, 100), (12, 50), (320, 90)]
    assert [render.label_font_size(h) for h, _ in sizes] == [1, 8, 0, 10]
    table = data.frame_geometry(sizes, S)
    size_tab = atlas.size_table([h for h, _ in sizes])
    assert size_tab.tolist() == [0, 1, -1, 2]
    rng = np.random.default_rng(9)
    frames = [rng.integers(0, 256, s + (3,), dtype=np.uint8) for s in sizes]
    cases = [LC.random_case(rng, h, w, n, int(t)) for (h, w), n, t in zip(sizes, (12, 40, 5, 30), table["thickness"])]
    rows, offsets, scores = LC.pack(cases)
    triple = (cuda(rows), cuda(offsets), cuda(LC.label_indices(rows, scores)))
    slots = np.full((len(sizes),) + cap + (3,), 0xA5, np.uint8)
    for b, f in enumerate(frames):
        slots[b, :f.shape[0], :f.shape[1]] = f
    flag = new_flag()
    for _ in range(2):                                        # twice into fresh memory: the padding is written, not inherited
        got = render.render_frame_ragged(cuda(slots), geom_tensor(table), None, triple, box_palette=PAL, flag=flag, labels=atlas,
                                         label_sizes=cuda(size_tab))
    plain = render.render_frame_ragged(cuda(slots), geom_tensor(table), None, triple[:2], box_palette=PAL)
    got, plain = got.cpu().numpy(), plain.cpu().numpy()
    assert int(flag) == 0
    for b, ((ih, iw), f) in enumerate(zip(sizes, frames)):
        one = (cuda(rows[offsets[b]:offsets[b + 1]]), cuda(np.array([0, len(cases[b][0])], np.int32)),
               triple[2][offsets[b]:offsets[b + 1]].contiguous())
        fixed = render.render_frame(cuda(f[None]), None, one, box_palette=PAL, thickness=int(table["thickness"][b]), labels=atlas)
        assert np.array_equal(got[b, :ih, :iw], fixed.cpu().numpy()[0]), b
        assert np.array_equal(got[b, :ih, :iw], render.draw_labels_host(f, *cases[b], atlas, None, int(table["thickness"][b]), PAL)), b
        outside = got[b].copy()
        outside[:ih, :iw] = 0
        assert not outside.any(), b
    assert np.array_equal(got[2], plain[2]) and not np.array_equal(got[1], plain[1])      # size index -1: the outlines alone


def test_labels_none_changes_nothing():
    rng = np.random.default_rng(10)
    frames = cuda(rng.integers(0, 256, (2, 64, 96, 3), dtype=np.uint8))
    cmap = cuda(rng.integers(0, 9, (2, 64, 96), dtype=np.uint8))
    results = [np.array([[4.5, 3.2, 30.9, 50.1, 0.9, 0.9, 1.0], [20.0, 40.0, 60.0, 90.0, 0.5, 0.25, 3.0]], np.float32), None]
    kw = dict(palette=render.seg_palette(9), box_palette=PAL, count=True)
    a, ca = render.render_frame(frames, cmap, results, (64, 64), **kw)
    b, cb = render.render_frame(frames, cmap, results, (64, 64), labels=None, **kw)
    assert torch.equal(a, b) and torch.equal(ca, cb)
    assert torch.equal(render.draw_boxes(frames, results, (64, 64), palette=PAL),
                       render.draw_boxes(frames, results, (64, 64), palette=PAL, labels=None))


def test_host_list_path_equals_the_statement():
    rng = np.random.default_rng(11)
    frames = rng.integers(0, 256, (2, 64, 96, 3), dtype=np.uint8)
    results = [np.array([[24.5, 3.2, 50.9, 50.1, 0.9, 0.9, 1.0], [20.0, 40.0, 60.0, 90.0, 0.5, 0.25, 3.0]], np.float32), None]
    flag = new_flag()
    rows, offsets, thickness, _ = render.box_rows(results, (64, 96), NC, (64, 64))
    assert thickness == 2
    scores = np.array([np.float32(0.9) * np.float32(0.9), np.float32(0.5) * np.float32(0.25)], np.float32)
    with pytest.raises(RuntimeError, match="was not built"):   # 64 rows ask for font size 2, which this atlas lacks
        render.draw_boxes(cuda(frames), results, (64, 64), palette=PAL, labels=LC.atlas())
    src = cuda(frames)
    out = render.render_frame(src, None, results, (64, 64), box_palette=PAL, labels=LC.atlas(), font_size=10, flag=flag)
    assert np.array_equal(out.cpu().numpy(), host_pictures(frames, rows, offsets, scores, 10, thickness))
    drawn = render.draw_labels(render.draw_boxes(src, results, (64, 64), palette=PAL), results, LC.atlas(), (64, 64), font_size=10,
                               box_palette=PAL, flag=flag)
    assert torch.equal(drawn, out) and int(flag) == 0
    bad = [np.array([[24.5, 3.2, 50.9, 50.1, 1.5, 1.0, 1.0]], np.float32), None]
    render.render_frame(src, None, bad, (64, 64), box_palette=PAL, labels=LC.atlas(), font_size=10, flag=flag)
    assert int(flag) == render.FLAG_LABEL_SCORE


def test_labels_in_a_captured_graph():
    rng = np.random.default_rng(12)
    B, ih, iw, atlas = 2, 90, 160, LC.atlas()

    def inputs():
        frames = rng.integers(0, 256, (B, ih, iw, 3), dtype=np.uint8)
        rows, offsets, scores = LC.pack([LC.random_case(rng, ih, iw, 20, 2) for _ in range(B)])
        return frames, rows, offsets, LC.label_indices(rows, scores), scores

    first, second = inputs(), inputs()
    src, rows, offsets, idx = (cuda(a) for a in first[:4])
    call = lambda: render.render_frame(src, None, (rows, offsets, idx), box_palette=PAL, thickness=2, labels=atlas, font_size=8)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        call()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        out = call()
    g.replay()
    torch.cuda.synchronize()
    assert torch.equal(out, call())
    assert np.array_equal(out.cpu().numpy(), host_pictures(first[0], first[1], first[2], first[4], 8, 2))
    for t, a in zip((src, rows, offsets, idx), second[:4]):
        t.copy_(torch.from_numpy(a))
    g.replay()
    torch.cuda.synchronize()
    want = host_pictures(second[0], second[1], second[2], second[4], 8, 2)
    assert np.array_equal(out.cpu().numpy(), want) and torch.equal(call(), out)
    assert not np.array_equal(want, host_pictures(first[0], first[1], first[2], first[4], 8, 2))


def test_labels_do_not_sync_and_op_matches():
    import asy_vrnet_amd.ops  # noqa: F401
    rng = np.random.default_rng(13)
    B, ih, iw, atlas = 2, 90, 160, LC.atlas()
    frames = rng.integers(0, 256, (B, ih, iw, 3), dtype=np.uint8)
    rows, offsets, scores = LC.pack([LC.random_case(rng, ih, iw, n, 3) for n in (10, 30)])
    src, rg, og, ig, bpal = cuda(frames), cuda(rows), cuda(offsets), cuda(LC.label_indices(rows, scores)), cuda(PAL)
    results = [np.array([[14.5, 3.2, 40.9, 50.1, 0.9, 0.9, 1.0]], np.float32), None]
    call = lambda: (render.render_frame(src, None, (rg, og, ig), box_palette=bpal, thickness=3, labels=atlas, font_size=10),
                    render.draw_boxes(src, results, (64, 64), palette=bpal, labels=atlas, thickness=1))
    assert render.label_font_size(ih) == 3
    with pytest.raises(RuntimeError, match="was not built"):
        call()
    call = lambda: (render.render_frame(src, None, (rg, og, ig), box_palette=bpal, thickness=3, labels=atlas, font_size=10),
                    render.render_frame(src, None, results, (64, 64), box_palette=bpal, labels=atlas, font_size=8))
    call()
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        out, drawn = call()
    finally:
        torch.cuda.set_sync_debug_mode("default")
    assert np.array_equal(out.cpu().numpy(), host_pictures(frames, rows, offsets, scores, 10, 3))
    blob, records = atlas.on("cuda")
    plain = render.render_frame(src, None, (rg, og), box_palette=bpal, thickness=3)
    assert torch.equal(torch.ops.vrnet.render_labels(plain, rg, og, bpal, 3, ig, blob, records, atlas.size_index(10)), out)
    r2, o2, t2, _ = render.box_rows(results, (ih, iw), NC, (64, 64))
    assert np.array_equal(drawn.cpu().numpy(), host_pictures(frames, r2, o2, np.array([np.float32(0.9) * np.float32(0.9)], np.float32), 8, t2))


def test_end_to_end_nano_pipeline():
    S, F, B = (64, 64), (270, 180), 2
    assert render.label_font_size(F[0]) == 8
    model = A.EfficientVRNet(NC, 9, "nano", img_size=S[0]).cuda().eval()
    A.randomize_state_dict(model.state_dict(), seed=4)
    rng = np.random.default_rng(14)
    frames = rng.integers(0, 256, (B,) + F + (3,), dtype=np.uint8)
    radar = (rng.standard_normal((B, 4) + S) * 2.0 + 1.0).astype(np.float32)
    fr = cuda(frames)
    images, _ = data.device_letterbox(fr, S)
    with torch.no_grad():
        det, seg = model(images, cuda(radar))
    pred = decode.decode_outputs(det, S)
    score = (pred[..., 4] * pred[..., 5:5 + NC].amax(-1)).flatten().sort(descending=True).values
    conf = float(score[11])                                   # the 12th-largest score of the batch
    common = dict(batch=B, conf_thres=conf, nms_thres=0.5, max_candidates=64)
    plain = A.FramePipeline(model, F, S, **common)
    how = dict(labels=True, class_names=LC.CLASS_NAMES) if LC.have_pillow() else dict(labels=LC.atlas())
    labelled = A.FramePipeline(model, F, S, **common, **how)
    assert plain.labels is None and not hasattr(plain, "_label_idx") and labelled.labels.sizes == ((8,) if LC.have_pillow() else (1, 8, 10))
    base = plain.run(frames, radar)
    base = dict(rendered=base.rendered.cpu().numpy(), dets=base.detections(), cmap=base.class_map.cpu().numpy(),
                seg_counts=base.seg_counts.cpu().numpy(), flag=int(base.flag))
    # labels=None: the outputs of the eager composition of the public calls, as before
    results = decode.non_max_suppression(pred, NC, S, F, True, conf_thres=conf, nms_thres=0.5)
    cmap = decode.seg_predict(seg, S, F)
    eager, eager_counts = render.render_frame(fr, cmap, results, S, palette=render.seg_palette(9), box_palette=PAL, count=True)
    assert np.array_equal(base["rendered"], eager.cpu().numpy()) and np.array_equal(base["seg_counts"], eager_counts.cpu().numpy())
    assert base["flag"] == 0 and np.array_equal(base["cmap"], cmap.cpu().numpy())
    for _ in range(2):                                        # a second replay: the picture is rebuilt, not drawn over
        res = labelled.run(frames, radar)
    dets = res.detections()
    n = [len(d) for d in dets]
    print("conf_thres", conf, "kept per image", n)
    assert sum(n) > 0 and int(res.flag) == 0
    assert all(np.array_equal(a, b) for a, b in zip(dets, base["dets"])) and np.array_equal(res.class_map.cpu().numpy(), base["cmap"])
    rows, offsets, thickness, _ = render.box_rows(dets, F, NC, S)
    assert thickness == labelled.thickness == 7
    scores = np.concatenate([d[:, 4] * d[:, 5] for d in dets]).astype(np.float32)
    want = host_pictures(base["rendered"], rows, offsets, scores, 8, thickness)
    assert np.array_equal(res.rendered.cpu().numpy(), want) and not np.array_equal(want, base["rendered"])
    with pytest.raises(RuntimeError, match="render=True"):
        A.FramePipeline(model, F, S, render=False, graph=False, **common, **how)


def test_ragged_pipeline_validates_the_font_sizes_before_it_enqueues():
    S, cap, B = (64, 64), (270, 180), 2
    model = A.EfficientVRNet(NC, 9, "nano", img_size=S[0]).cuda().eval()
    A.randomize_state_dict(model.state_dict(), seed=4)
    atlas = LC.atlas()                                        # sizes 1, 8, 10
    pipe = A.FramePipeline(model, cap, S, batch=B, conf_thres=0.05, max_candidates=32, ragged=True, graph=True, labels=atlas)
    rng = np.random.default_rng(15)
    radar = (rng.standard_normal((B, 4) + S) * 2.0 + 1.0).astype(np.float32)
    good = [rng.integers(0, 256, s + (3,), dtype=np.uint8) for s in ((270, 180), (40, 100))]
    res = pipe.run(good, radar)
    dets, rendered = res.detections(), res.rendered.cpu().numpy()
    print("kept per image", [len(d) for d in dets], "flag", int(res.flag))
    assert pipe.label_size_tab.cpu().tolist() == [1, 0] and len(dets[0]) > 0
    assert int(res.flag) & ~8 == 0                            # FLAG_CANDIDATES apart: the threshold is low on purpose
    # the same picture without labels, from the pipeline's own buffers, then the host statement per image at its own size
    plain = render.render_frame_ragged(pipe.frames_u8, pipe.geom, res.class_map, (pipe._draw_rows, pipe._offsets),
                                       palette=pipe.seg_palette, box_palette=pipe.box_palette).cpu().numpy()
    for b, f in enumerate(good):
        ih, iw = f.shape[:2]
        rows, _, thickness, _ = render.box_rows([dets[b]], (ih, iw), NC, S)
        scores = (dets[b][:, 4] * dets[b][:, 5]).astype(np.float32)
        want = render.draw_labels_host(plain[b, :ih, :iw], rows, scores, atlas, None, thickness, PAL)
        assert np.array_equal(rendered[b, :ih, :iw], want), b
        assert not rendered[b, ih:].any() and not rendered[b, :, iw:].any()
    assert not np.array_equal(rendered, plain)
    before = pipe.frames_u8.clone()
    with pytest.raises(RuntimeError, match="image 1 of 100 rows needs font size 3"):
        pipe.run([good[0], rng.integers(0, 256, (100, 100, 3), dtype=np.uint8)], radar)
    assert torch.equal(pipe.frames_u8, before)               # nothing was enqueued
