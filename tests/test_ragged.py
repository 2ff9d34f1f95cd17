"""Ragged batches: frames of mixed sizes through one letterbox / detect_finish / seg_predict / render call and through one
captured FramePipeline / EvalPipeline.  The ragged kernels restate the integer and fp64 arithmetic of the fixed-size ones
with the per-image geometry read from a device table, so every comparison is bit for bit: against Pillow itself for the
letterbox, against the fixed-size call on each image alone for the rest, with the zeroed padding of every slot part of the
expectation."""
import os

import numpy as np
import pytest
import torch

import asy_vrnet_amd as A
from asy_vrnet_amd import data, decode, evaluate, infer, metrics, render

NC, NSEG = 4, 9
NAMES = ["boat", "buoy", "pier", "ship"]
DIRTY = 0xA5


def cuda(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def geom_tensor(table):
    return cuda(table.view(np.uint8).reshape(len(table), -1))


def padded(items, capacity, fill=DIRTY):
    """The list of (ih, iw[, 3]) arrays in the corners of a (B, ihm, iwm[, 3]) buffer filled with `fill`."""
    buf = np.full((len(items),) + tuple(capacity) + items[0].shape[2:], fill, np.uint8)
    for b, a in enumerate(items):
        buf[b, :a.shape[0], :a.shape[1]] = a
    return buf


# ---------------------------------------------------------------------------------------------- 1. the table (no GPU)
SIZES = [(40, 56), (150, 97), (23, 41), (1080, 1920)]


@pytest.mark.parametrize("letterbox", [True, False])
@pytest.mark.parametrize("input_shape", [(64, 64), (64, 96)])
def test_frame_geometry_equals_the_per_image_helpers(input_shape, letterbox):
    H, W = input_shape
    table = data.frame_geometry(SIZES, input_shape, letterbox)
    assert table.dtype == data.GEOM_DTYPE and table.dtype.itemsize == 80 and table.shape == (len(SIZES),)
    for rec, (ih, iw) in zip(table, SIZES):
        nw, nh, dx, dy = data.letterbox_geometry(iw, ih, W, H) if letterbox else (W, H, 0, 0)
        top, left, snh, snw = decode.seg_window(input_shape, (ih, iw)) if letterbox else (0, 0, H, W)
        offset, scale = infer.unmap_scalars(input_shape, (ih, iw), letterbox)
        assert (rec["ih"], rec["iw"]) == (ih, iw)
        assert (rec["nw"], rec["nh"], rec["dx"], rec["dy"]) == (nw, nh, dx, dy)
        assert (rec["seg_top"], rec["seg_left"], rec["seg_nh"], rec["seg_nw"]) == (top, left, snh, snw)
        assert rec["thickness"] == max((iw + ih) // np.mean(input_shape), 1) and rec["reserved"] == 0
        got = np.array([rec["offset_y"], rec["offset_x"], rec["scale_y"], rec["scale_x"]])
        assert np.array_equal(got, np.array(offset + scale, dtype=np.float64))          # the same float64 bits
    # the packed form the device takes: 80 bytes per record, in the order of include/vrnet_hip.h
    raw = table.view(np.uint8).reshape(len(SIZES), -1)
    assert raw.shape == (len(SIZES), 80)
    assert np.array_equal(raw[:, :48].copy().view("<i4")[:, 0], [s[0] for s in SIZES])
    assert np.array_equal(raw[:, 48:].copy().view("<f8")[:, 2], table["scale_y"])


def test_default_max_taps_bound():
    """ksize(R) + 2 covers every frame inside the capacity whose window is at least 2 R pixels on both axes."""
    cap, S = (150, 200), (64, 64)
    taps = data.default_max_taps(cap, S)
    assert taps == int(np.ceil(2 * 200 / 64)) * 2 + 3
    R = max(cap[1] / S[1], cap[0] / S[0])
    worst = 0
    for ih in range(1, cap[0] + 1):
        for iw in (1, 2, 3, 7, 41, 97, 150, 199, 200):
            nw, nh, _, _ = data.letterbox_geometry(iw, ih, S[1], S[0])
            if min(nw, nh) >= 2 * R:
                worst = max(worst, data.resample_ksize(iw, nw), data.resample_ksize(ih, nh))
    assert 0 < worst <= taps


# ---------------------------------------------------------------------------------------------- 2. argument errors (no GPU)
def test_ragged_argument_errors():
    cap, S, B = (150, 200), (64, 64), 2
    rng = np.random.default_rng(5)
    radar = np.zeros((B, 4) + S, np.float32)

    def frame(ih, iw):
        return rng.integers(0, 256, (ih, iw, 3), dtype=np.uint8)

    def check(frames, sizes=None, radar=radar):
        return infer.validate_ragged_inputs(frames, radar, sizes, B, cap, S)
    items, r, sizes, table = check([frame(40, 56), frame(150, 200)])
    assert sizes.tolist() == [[40, 56], [150, 200]] and table["ih"].tolist() == [40, 150] and tuple(r.shape) == (B, 4) + S
    with pytest.raises(RuntimeError, match=r"image 1.*above the capacity"):
        check([frame(40, 56), frame(151, 200)])
    with pytest.raises(RuntimeError, match=r"image 0.*above the capacity"):
        check([frame(40, 201), frame(40, 56)])
    with pytest.raises(RuntimeError, match=r"image 1.*empty window"):
        check([frame(40, 56), frame(1, 200)])
    with pytest.raises(RuntimeError, match=r"image 1"):                       # int(2 * 0.32) = 0 rows: an empty window
        check([frame(40, 56), frame(2, 200)])
    with pytest.raises(RuntimeError, match=r"image 1.*tap capacity"):         # a sliver: one row out of five, 21 taps > 17
        check([frame(40, 56), frame(5, 200)])
    assert data.resample_ksize(5, 1) == 21 and data.default_max_taps(cap, S) == 17
    with pytest.raises(RuntimeError, match="for a batch of 2"):
        check([frame(40, 56)])
    with pytest.raises(RuntimeError, match="for a batch of 2"):
        check([frame(40, 56)] * 3)
    with pytest.raises(RuntimeError, match=r"image 1: sizes says \(41, 56\)"):
        check([frame(40, 56), frame(40, 56)], sizes=[(40, 56), (41, 56)])
    buf = padded([frame(40, 56), frame(23, 41)], cap)
    with pytest.raises(RuntimeError, match="needs sizes"):
        check(buf)
    with pytest.raises(RuntimeError, match=r"image 0.*padded buffer"):
        check(buf[:, :30], sizes=[(40, 56), (23, 41)])
    with pytest.raises(RuntimeError, match="uint8"):
        check([frame(40, 56).astype(np.float32), frame(40, 56)])
    with pytest.raises(RuntimeError, match="built for radar"):
        check([frame(40, 56)] * 2, radar=radar[:, :3])
    items, _, sizes, _ = check(buf, sizes=torch.tensor([(40, 56), (23, 41)]))            # host integers of any kind
    assert torch.is_tensor(items) and sizes.tolist() == [[40, 56], [23, 41]]
    with pytest.raises(RuntimeError, match=r"padded buffer \(150, 200\) is above the capacity \(100, 200\)"):
        data.device_letterbox_ragged(buf, [(40, 56), (23, 41)], S, capacity=(100, 200))
    with pytest.raises(RuntimeError, match=r"padded buffer \(150, 200\) is above the capacity"):
        infer.validate_ragged_inputs(buf, radar, [(40, 56), (23, 41)], B, (100, 200), S)
    # a fixed-size pipeline rejects sizes before it looks at anything else
    fixed = object.__new__(A.FramePipeline)
    fixed.ragged, fixed.frame_shape = False, (40, 56)
    with pytest.raises(RuntimeError, match="ragged"):
        fixed.run(None, None, sizes=[(40, 56)])
    # evaluate: the label maps follow the frames
    with pytest.raises(RuntimeError, match=r"image 1: sizes says"):
        evaluate.validate_add(["a", "b"], set(), [np.zeros((40, 56), np.uint8), np.zeros((23, 40), np.uint8)],
                              [np.zeros((0, 5), np.int64)] * 2, B, cap, NC, 4, sizes=sizes)
    ids, labs, _ = evaluate.validate_add(["a", "b"], set(), [np.zeros((40, 56), np.uint8), np.zeros((23, 41), np.uint8)],
                                         [np.zeros((0, 5), np.int64)] * 2, B, cap, NC, 4, sizes=sizes)
    assert ids == ["a", "b"] and [tuple(t.shape) for t in labs] == [(40, 56), (23, 41)]


# ---------------------------------------------------------------------------------------------- 3. predict_dir (no GPU)
class FakeResult:
    def __init__(self, frames, sizes, capacity):
        self.sizes = sizes
        self.rendered = torch.from_numpy(padded([255 - f for f in frames], capacity, 0))
        self._dets = [np.full((b + 1, 7), float(f[0, 0, 0]), np.float32) for b, f in enumerate(frames)]

    def detections(self):
        return self._dets


class FakePipeline:
    ragged, batch, frame_shape = True, 2, (12, 16)

    def __init__(self):
        self.calls = []

    def run(self, frames, radar, sizes=None):
        self.calls.append((frames, radar))
        return FakeResult(frames, np.array([f.shape[:2] for f in frames]), self.frame_shape)


def test_predict_dir_batches_pads_and_saves(tmp_path):
    from PIL import Image
    rng = np.random.default_rng(6)
    src, radar_root, dst = tmp_path / "in", tmp_path / "radar", tmp_path / "out"
    os.makedirs(src)
    os.makedirs(radar_root)
    pics = {"1665000003.00003.png": (9, 16), "1665000001.00001.PNG": (12, 7), "1665000002.00002.bmp": (5, 5)}
    frames, radars = {}, {}
    for name, (ih, iw) in pics.items():
        frames[name] = rng.integers(0, 256, (ih, iw, 3), dtype=np.uint8)
        Image.fromarray(frames[name]).save(src / name, format="BMP" if name.endswith("bmp") else "PNG")
        radars[name] = rng.standard_normal((4, 8, 8))
        np.savez(radar_root / (data.frame_id(name) + ".npz"), radars[name])
    (src / "1665000000.00000.txt").write_text("not a picture")
    (src / "notes.md").write_text("nor this")
    pipe = FakePipeline()
    out = infer.predict_dir(pipe, str(src), str(radar_root), str(dst))
    order = sorted(pics)                                                     # the extension filter and the sorted listing
    assert [n for n, _ in out] == order
    assert len(pipe.calls) == 2 and all(len(f) == 2 and r.shape == (2, 4, 8, 8) and r.dtype == np.float32 for f, r in pipe.calls)
    assert np.array_equal(pipe.calls[0][0][0], frames[order[0]]) and np.array_equal(pipe.calls[0][0][1], frames[order[1]])
    assert np.array_equal(pipe.calls[0][1][1], radars[order[1]].astype(np.float32))
    # the final batch is filled with a repeat of the last picture, which is dropped from the result
    assert np.array_equal(pipe.calls[1][0][0], frames[order[2]]) and np.array_equal(pipe.calls[1][0][1], frames[order[2]])
    assert np.array_equal(pipe.calls[1][1][0], pipe.calls[1][1][1])
    assert [d.shape for _, d in out] == [(1, 7), (2, 7), (1, 7)]
    assert all(float(d[0, 0]) == float(frames[n][0, 0, 0]) for n, d in out)
    assert sorted(os.listdir(dst)) == sorted(os.path.splitext(n)[0] + ".png" for n in order)
    for n in order:
        saved = np.array(Image.open(dst / (os.path.splitext(n)[0] + ".png")))
        assert np.array_equal(saved, 255 - frames[n])                        # sliced to the picture's own size
    assert infer.predict_dir(FakePipeline(), str(src), str(radar_root))[2][0] == order[2]       # nothing saved: no folder needed
    fixed = FakePipeline()
    fixed.ragged = False
    with pytest.raises(RuntimeError, match="ragged"):
        infer.predict_dir(fixed, str(src), str(radar_root))
    # two pictures that would be saved under one name: refused before anything runs, when there is something to save
    Image.fromarray(frames[order[2]]).save(src / "1665000003.00003.tif")
    clash = FakePipeline()
    with pytest.raises(RuntimeError, match=r"1665000003\.00003\.png and 1665000003\.00003\.tif would both be saved"):
        infer.predict_dir(clash, str(src), str(radar_root), str(tmp_path / "out2"))
    assert not clash.calls and not os.path.exists(tmp_path / "out2")
    assert len(infer.predict_dir(clash, str(src), str(radar_root))) == 4
    assert sorted(infer.IMAGE_EXTENSIONS) == sorted(".bmp .dib .png .jpg .jpeg .pbm .pgm .ppm .tif .tiff".split())


class StubEval:
    def __init__(self, batch, frame_shape):
        self.batch, self.frame_shape = batch, frame_shape

    def reset(self):
        pass


def test_evaluate_lines_with_a_fixed_pipeline_still_raises_on_another_size(tmp_path):
    from PIL import Image
    fid = "1665000001.12345"
    os.makedirs(tmp_path / "VOC2007" / "SegmentationClass")
    Image.fromarray(np.zeros((5, 7, 3), np.uint8)).save(tmp_path / (fid + ".png"))
    Image.fromarray(np.zeros((5, 7), np.uint8), mode="L").save(tmp_path / "VOC2007" / "SegmentationClass" / (fid + ".png"))
    np.savez(tmp_path / (fid + ".npz"), np.zeros((4, 8, 8)))
    with pytest.raises(RuntimeError, match=r"built for 6 x 7 frames"):
        evaluate.evaluate_lines(StubEval(1, (6, 7)), [f"{tmp_path}/{fid}.png\n"], str(tmp_path), str(tmp_path / "VOC2007"))
    # a ragged pipeline takes any frame size, but a label map of another size than its frame still raises with the file's name
    ragged = StubEval(1, (6, 7))
    ragged.ragged, ragged.calls = True, []
    ragged.add = lambda *a: ragged.calls.append(a)
    ragged.compute = lambda: "computed"
    assert evaluate.evaluate_lines(ragged, [f"{tmp_path}/{fid}.png\n"], str(tmp_path), str(tmp_path / "VOC2007")) == "computed"
    assert [a.shape for a in ragged.calls[0][1]] == [(5, 7, 3)] and ragged.calls[0][3][0].dtype == np.uint8
    Image.fromarray(np.zeros((5, 6), np.uint8), mode="L").save(tmp_path / "VOC2007" / "SegmentationClass" / (fid + ".png"))
    with pytest.raises(RuntimeError, match=fid.replace(".", r"\.") + r"\.png.*label map is \(5, 6\)"):
        evaluate.evaluate_lines(ragged, [f"{tmp_path}/{fid}.png\n"], str(tmp_path), str(tmp_path / "VOC2007"))


# ---------------------------------------------------------------------------------------------- 4. letterbox against Pillow
CAPACITY = (150, 200)
LB_SIZES = [(150, 97), (23, 41), (40, 64), (150, 200)]


def pillow_letterbox(frame, label, input_shape, letterbox):
    from PIL import Image
    H, W = input_shape
    ih, iw = label.shape
    nw, nh, dx, dy = data.letterbox_geometry(iw, ih, W, H) if letterbox else (W, H, 0, 0)
    canvas = Image.new("RGB", (W, H), (128, 128, 128))
    canvas.paste(Image.fromarray(frame).resize((nw, nh), Image.BICUBIC), (dx, dy))
    lab = Image.new("L", (W, H), 0)
    lab.paste(Image.fromarray(label).resize((nw, nh), Image.NEAREST), (dx, dy))
    return np.array(canvas), np.array(lab)


@pytest.mark.gpu
@pytest.mark.parametrize("letterbox", [True, False])
@pytest.mark.parametrize("input_shape", [(64, 64), (64, 96)])
def test_letterbox_ragged_equals_pillow_and_the_fixed_call(input_shape, letterbox):
    import asy_vrnet_amd.hip as hip
    H, W = input_shape
    sizes = LB_SIZES + ([(64, 150), (150, 96)] if (input_shape == (64, 96) and not letterbox) else [])
    rng = np.random.default_rng(11)
    frames = [rng.integers(0, 256, s + (3,), dtype=np.uint8) for s in sizes]
    labels = [rng.integers(0, 12, s, dtype=np.uint8) for s in sizes]
    B = len(sizes)
    taps = data.default_max_taps(CAPACITY, input_shape)
    table = data.frame_geometry(sizes, input_shape, letterbox, CAPACITY, taps)
    skipped = [(int(r["nw"]) == int(r["iw"]), int(r["nh"]) == int(r["ih"])) for r in table]
    if input_shape == (64, 64) and letterbox:
        assert skipped[2] == (True, True) and max(data.resample_ksize(97, int(table[0]["nw"])), 0) > 9     # scale 1; more than 4 taps
    if len(sizes) == 6:
        assert skipped[4] == (False, True) and skipped[5] == (True, False)
    img, lab = cuda(padded(frames, CAPACITY)), cuda(padded(labels, CAPACITY))                 # 0xA5 outside every frame
    ws = torch.full((hip.letterbox_ragged_workspace_bytes(B, *CAPACITY, H, W, taps),), DIRTY, dtype=torch.uint8, device="cuda")
    canvas = torch.full((B, H, W, 3), 7, dtype=torch.uint8, device="cuda")
    images = torch.full((B, 3, H, W), 7.0, device="cuda")
    out_lab = torch.full((B, H, W), 7, dtype=torch.uint8, device="cuda")
    flag = torch.zeros(1, dtype=torch.int32, device="cuda")
    hip.letterbox_ragged(img, lab, geom_tensor(table), H, W, taps, canvas=canvas, images=images, label_out=out_lab, flag=flag, ws=ws)
    assert int(flag) == 0
    # the public call, from the list of host arrays and from the padded buffer
    pub_images, pub_lab = data.device_letterbox_ragged(frames, None, input_shape, labels, letterbox, capacity=CAPACITY)
    pub_canvas, _ = data.device_letterbox_ragged(img, sizes, input_shape, None, letterbox, normalise=False)
    assert torch.equal(pub_images, images) and torch.equal(pub_lab, out_lab) and torch.equal(pub_canvas, canvas)
    canvas, images, out_lab = canvas.cpu().numpy(), images.cpu().numpy(), out_lab.cpu().numpy()
    for b in range(B):
        want_canvas, want_lab = pillow_letterbox(frames[b], labels[b], input_shape, letterbox)
        assert np.array_equal(canvas[b], want_canvas), (b, sizes[b])
        assert np.array_equal(out_lab[b], want_lab), (b, sizes[b])
        one_images, one_lab = data.device_letterbox(cuda(frames[b]), input_shape, cuda(labels[b]), letterbox)
        one_canvas, _ = data.device_letterbox(cuda(frames[b]), input_shape, None, letterbox, normalise=False)
        assert np.array_equal(images[b], one_images[0].cpu().numpy()), (b, sizes[b])
        assert np.array_equal(canvas[b], one_canvas[0].cpu().numpy()) and np.array_equal(out_lab[b], one_lab[0].cpu().numpy())


# ---------------------------------------------------------------------------------------------- 5. ragged against fixed
def finish_buffers(B, cap):
    dev = "cuda"
    return dict(rows=torch.full((B, cap, 7), 7.0, device=dev), draw_rows=torch.full((B * cap, 5), -3, dtype=torch.int32, device=dev),
                offsets=torch.full((B + 1,), -3, dtype=torch.int32, device=dev),
                det_counts=torch.full((B, NC), -3, dtype=torch.int64, device=dev),
                flag=torch.zeros(1, dtype=torch.int32, device=dev))


def synthetic_kept_rows(B, cap, seed):
    rng = np.random.default_rng(seed)
    rows = np.zeros((B, cap, 7), np.float32)
    lo = rng.uniform(-0.3, 0.9, (B, cap, 2))
    rows[..., 0:2] = lo
    rows[..., 2:4] = lo + rng.uniform(0.0, 0.6, (B, cap, 2))              # reaches below 0 and above 1 on every side
    rows[..., 4:6] = rng.uniform(0.5, 1.0, (B, cap, 2))
    rows[..., 6] = rng.integers(0, NC, (B, cap))
    assert rows[..., 0].min() < 0 and rows[..., 1].min() < 0 and rows[..., 2].max() > 1 and rows[..., 3].max() > 1
    return rows


@pytest.mark.gpu
@pytest.mark.parametrize("letterbox", [True, False])
def test_detect_finish_ragged_equals_the_fixed_call_per_image(letterbox):
    import asy_vrnet_amd.hip as hip
    sizes, S, cap, kept = [(37, 53), (1080, 1920), (40, 56)], (64, 64), 70, [17, 70, 1]
    rows = cuda(synthetic_kept_rows(3, cap, 72))
    kept_t = torch.tensor(kept, dtype=torch.int32, device="cuda")
    geom = geom_tensor(data.frame_geometry(sizes, S, letterbox))
    got = finish_buffers(3, cap)
    hip.detect_finish_ragged(rows, kept_t, geom, NC, (1080, 1920), got["rows"], got["draw_rows"], got["offsets"],
                             got["det_counts"], got["flag"])
    assert int(got["flag"]) == 0
    draw, clipped = [], False
    for b, shape in enumerate(sizes):
        one = finish_buffers(1, cap)
        offset, scale = infer.unmap_scalars(S, shape, letterbox)
        hip.detect_finish(rows[b:b + 1].contiguous(), kept_t[b:b + 1].contiguous(), NC, shape, offset, scale, one["rows"],
                          one["draw_rows"], one["offsets"], one["det_counts"], one["flag"])
        assert torch.equal(got["rows"][b], one["rows"][0]) and torch.equal(got["det_counts"][b], one["det_counts"][0]), b
        assert int(one["offsets"][1]) == kept[b]
        d = one["draw_rows"][:kept[b]]
        clipped = clipped or bool((d[:, 2] == shape[1]).any() and (d[:, 0] == 0).any())       # boxes that cross the image edge
        draw.append(d)
    assert clipped
    draw = torch.cat(draw)
    assert got["offsets"].tolist() == [0] + np.cumsum(kept).tolist()
    assert torch.equal(got["draw_rows"][:len(draw)], draw) and not got["draw_rows"][len(draw):].any()


@pytest.mark.gpu
@pytest.mark.parametrize("shape", [(3, 9, 64, 96), (3, 1, 64, 64)])
def test_seg_predict_ragged_equals_the_fixed_call_per_image(shape):
    sizes, cap = [(40, 56), (150, 97), (23, 41)], (150, 100)
    S = shape[2:]
    x = torch.randn(shape, generator=torch.Generator().manual_seed(13)).cuda() * 3.0
    flag = torch.zeros(1, dtype=torch.int32, device="cuda")
    for _ in range(2):                                   # twice into fresh memory: the padding is written, not inherited
        got = decode.seg_predict_ragged(x, geom_tensor(data.frame_geometry(sizes, S)), cap, flag)
    assert int(flag) == 0 and tuple(got.shape) == (3,) + cap and got.dtype == torch.uint8
    want = torch.zeros((3,) + cap, dtype=torch.uint8, device="cuda")
    for b, (ih, iw) in enumerate(sizes):
        want[b, :ih, :iw] = decode.seg_predict(x[b:b + 1], S, (ih, iw))[0]
    assert torch.equal(got, want)
    if shape[1] > 1:
        assert len(torch.unique(want)) > 2


RENDER_SIZES = {(48, 67): [(48, 67), (20, 33), (37, 64)],       # slots of 3216 pixels: dword accesses
                (45, 67): [(45, 66), (20, 33), (25, 67)]}       # 3015 pixels: no slot but the first is dword aligned


@pytest.mark.gpu
@pytest.mark.parametrize("capacity", sorted(RENDER_SIZES))
@pytest.mark.parametrize("mix_type", [0, 1, 2])
def test_render_ragged_equals_the_fixed_call_per_image(mix_type, capacity):
    sizes, S = RENDER_SIZES[capacity], (16, 16)
    table = data.frame_geometry(sizes, S)
    assert len(set(table["thickness"].tolist())) == 3                           # a thickness of its own per image
    rng = np.random.default_rng(17 + mix_type)
    frames = [rng.integers(0, 256, s + (3,), dtype=np.uint8) for s in sizes]
    cmaps = [np.repeat(np.repeat(rng.integers(0, NSEG, (-(-s[0] // 4), -(-s[1] // 8)), dtype=np.uint8), 4, 0), 8, 1)[:s[0], :s[1]]
             for s in sizes]                                                    # regions: waves of one class, and borders
    boxes, offsets = [], [0]
    for ih, iw in sizes:
        r = np.stack([rng.integers(-5, iw, 5), rng.integers(-5, ih, 5), rng.integers(0, iw + 6, 5), rng.integers(0, ih + 6, 5),
                      rng.integers(0, NC, 5)], axis=1)
        r = np.concatenate([r, [[0, 0, iw, ih, 1], [iw - 3, ih - 3, iw + 10, ih + 10, 2], [iw - 1, 0, iw - 1, ih - 1, 3]]])
        boxes.append(r.astype(np.int32))
        offsets.append(offsets[-1] + len(r))
    pal, bpal = render.seg_palette(NSEG), render.det_palette(NC)
    flag = torch.zeros(1, dtype=torch.int32, device="cuda")
    results = (cuda(np.concatenate(boxes)), cuda(np.array(offsets, np.int32)))
    for _ in range(2):
        got, counts = render.render_frame_ragged(cuda(padded(frames, capacity)), geom_tensor(table), cuda(padded(cmaps, capacity)),
                                                 results, palette=pal, mix_type=mix_type, alpha=0.7, count=True, box_palette=bpal,
                                                 flag=flag)
    assert int(flag) == 0                                # a padding byte (class 165) read as a class would raise FLAG_CLASS
    want = torch.zeros((3,) + capacity + (3,), dtype=torch.uint8, device="cuda")
    for b, (ih, iw) in enumerate(sizes):
        one, one_counts = render.render_frame(cuda(frames[b]), cuda(cmaps[b]),
                                              (cuda(boxes[b]), cuda(np.array([0, len(boxes[b])], np.int32))), palette=pal,
                                              mix_type=mix_type, alpha=0.7, count=True, box_palette=bpal,
                                              thickness=int(table["thickness"][b]))
        want[b, :ih, :iw] = one[0]
        assert torch.equal(counts[b], one_counts[0]) and int(counts[b].sum()) == ih * iw, b
        assert not torch.equal(one[0], render.render_frame(cuda(frames[b]), cuda(cmaps[b]), palette=pal, mix_type=mix_type)[0])
    assert torch.equal(got, want)


# ---------------------------------------------------------------------------------------------- 6. table validation
@pytest.mark.gpu
def test_a_wrong_table_is_clamped_and_flagged():
    """Clamped paths that are expected to succeed: a record that claims more rows than its slot has, and a window that
    reaches past the canvas.  The other images come out as with the right table, and FLAG_GEOMETRY is set."""
    import asy_vrnet_amd.hip as hip
    S, cap, sizes = (64, 64), (48, 68), [(40, 56), (48, 68), (23, 41)]
    H, W = S
    rng = np.random.default_rng(19)
    frames = cuda(padded([rng.integers(0, 256, s + (3,), dtype=np.uint8) for s in sizes], cap))
    cmaps = cuda(padded([rng.integers(0, NSEG, s, dtype=np.uint8) for s in sizes], cap))
    x = torch.randn((3, NSEG) + S, generator=torch.Generator().manual_seed(19)).cuda()
    rows, kept = cuda(synthetic_kept_rows(3, 8, 20)), torch.tensor([8, 5, 3], dtype=torch.int32, device="cuda")
    good = data.frame_geometry(sizes, S)
    tall, wide = good.copy(), good.copy()
    tall["ih"][1] = cap[0] + 1
    wide["dx"][1] = W - wide["nw"][1] + 5
    wide["seg_left"][1] = W - wide["seg_nw"][1] + 5
    taps = data.default_max_taps(cap, S)

    def run(table, everything):
        geom, out = geom_tensor(table), {}
        flags = {k: torch.zeros(1, dtype=torch.int32, device="cuda") for k in ("letterbox", "seg", "finish", "render")}
        out["images"] = torch.empty((3, 3, H, W), device="cuda")
        hip.letterbox_ragged(frames, None, geom, H, W, taps, images=out["images"], flag=flags["letterbox"])
        out["class_map"] = decode.seg_predict_ragged(x, geom, cap, flags["seg"])
        if everything:
            fin = finish_buffers(3, 8)
            hip.detect_finish_ragged(rows, kept, geom, NC, cap, fin["rows"], fin["draw_rows"], fin["offsets"], fin["det_counts"],
                                     flags["finish"])
            out["rows"] = fin["rows"]
            out["rendered"] = render.render_frame_ragged(frames, geom, cmaps, (fin["draw_rows"], fin["offsets"]),
                                                         palette=render.seg_palette(NSEG), box_palette=render.det_palette(NC),
                                                         flag=flags["render"])
        torch.cuda.synchronize()
        return out, {k: int(v) for k, v in flags.items()}
    want, flags = run(good, True)
    assert not any(flags.values())
    got, flags = run(tall, True)
    assert all(v == infer.FLAG_GEOMETRY == 256 for v in flags.values()), flags
    for k in want:
        assert torch.equal(got[k][0], want[k][0]) and torch.equal(got[k][2], want[k][2]), k
    for field in ("ih", "thickness"):                    # an image without rows and an outline without width: legal nowhere
        zero = good.copy()
        zero[field][1] = 0
        got, flags = run(zero, True)
        assert all(v == infer.FLAG_GEOMETRY for v in flags.values()), (field, flags)
        for k in want:
            assert torch.equal(got[k][0], want[k][0]) and torch.equal(got[k][2], want[k][2]), (field, k)
        if field == "ih":
            assert not got["class_map"][1].any() and not got["rendered"][1].any()        # its slot is all padding
    got, flags = run(wide, False)
    assert flags["letterbox"] == flags["seg"] == infer.FLAG_GEOMETRY
    for k in ("images", "class_map"):
        assert torch.equal(got[k][0], want[k][0]) and torch.equal(got[k][2], want[k][2]), k


# ---------------------------------------------------------------------------------------------- 7-8. the pipeline
S, CAP_SHAPE, CAND, NMS_THRES = (64, 64), (80, 112), 64, 0.4
RUNS = [[(40, 56), (80, 112), (61, 33)], [(80, 112), (17, 29), (40, 56)]]          # the biggest slot then takes the smallest


def make_run(sizes, seed):
    rng = np.random.default_rng(seed)
    frames = [rng.integers(0, 256, s + (3,), dtype=np.uint8) for s in sizes]
    radar = (rng.standard_normal((len(sizes), 4) + S) * 2.0 + 1.0).astype(np.float32)
    return frames, radar


def compose(model, frames, radar, conf, capacity=CAP_SHAPE):
    """The eager composition of the fixed-size public calls, image by image around one batched forward; the class map and
    the rendered frames padded with zeros to the capacity."""
    B = len(frames)
    images = torch.cat([data.device_letterbox(cuda(f), S)[0] for f in frames])
    with torch.no_grad():
        det, seg = model(images, cuda(radar))
    pred = decode.decode_outputs(det, S)
    out = dict(detections=[], det_counts=np.zeros((B, NC), np.int64), class_map=np.zeros((B,) + capacity, np.uint8),
               seg_counts=[], rendered=np.zeros((B,) + capacity + (3,), np.uint8), pred=pred)
    for b, f in enumerate(frames):
        shape = f.shape[:2]
        res = decode.non_max_suppression(pred[b:b + 1].contiguous(), NC, S, shape, True, conf_thres=conf, nms_thres=NMS_THRES)
        cmap = decode.seg_predict(seg[b:b + 1], S, shape)
        pic, counts = render.render_frame(cuda(f), cmap, res, S, palette=render.seg_palette(NSEG), box_palette=render.det_palette(NC),
                                          count=True)
        out["detections"].append(np.zeros((0, 7), np.float32) if res[0] is None else np.asarray(res[0], dtype=np.float32))
        out["det_counts"][b] = render.box_rows(res, shape, NC, S)[3][0]
        out["class_map"][b, :shape[0], :shape[1]] = cmap[0].cpu().numpy()
        out["rendered"][b, :shape[0], :shape[1]] = pic[0].cpu().numpy()
        out["seg_counts"].append(counts[0].cpu().numpy())
    out["seg_counts"] = np.stack(out["seg_counts"])
    return out


def snapshot(res):
    return dict(detections=res.detections(), det_counts=res.det_counts.cpu().numpy(), class_map=res.class_map.cpu().numpy(),
                seg_counts=res.seg_counts.cpu().numpy(), rendered=res.rendered.cpu().numpy(), kept=res.kept.cpu().numpy(),
                flag=int(res.flag))


def assert_same(got, want):
    assert len(got["detections"]) == len(want["detections"])
    for g, w in zip(got["detections"], want["detections"]):
        assert g.dtype == np.float32 and g.shape == w.shape and np.array_equal(g, w)
    for k in ("det_counts", "class_map", "seg_counts", "rendered"):
        assert got[k].dtype == want[k].dtype and got[k].shape == want[k].shape and np.array_equal(got[k], want[k]), k
    assert got["flag"] == 0


@pytest.fixture(scope="module")
def setup():
    model = A.EfficientVRNet(NC, NSEG, "nano", img_size=S[0]).cuda().eval()
    A.randomize_state_dict(model.state_dict(), seed=4)
    runs = [make_run(sizes, 81 + k) for k, sizes in enumerate(RUNS)]
    pred = compose(model, *runs[0], 0.5)["pred"]
    score = (pred[..., 4] * pred[..., 5:5 + NC].amax(-1)).flatten().sort(descending=True).values
    conf = float(score[17])                                # the 18th-largest score of the first batch
    buffers = [b.detach().clone() for b in model.buffers()]
    pipes = {g: A.FramePipeline(model, CAP_SHAPE, S, batch=3, conf_thres=conf, nms_thres=NMS_THRES, max_candidates=CAND,
                                graph=g, ragged=True) for g in (False, True)}
    assert all(torch.equal(a, b) for a, b in zip(buffers, model.buffers()))
    return dict(model=model, conf=conf, runs=runs, pipes=pipes, want=[compose(model, *r, conf) for r in runs])


@pytest.mark.gpu
@pytest.mark.parametrize("graph", [False, True])
def test_ragged_pipeline_equals_the_eager_composition(setup, graph):
    pipe, model, conf = setup["pipes"][graph], setup["model"], setup["conf"]
    assert (pipe.graph is not None) == graph and pipe.ragged and pipe.cap == CAND
    for k, sizes in enumerate(RUNS):
        want = setup["want"][k]
        n = [len(d) for d in want["detections"]]
        print("conf_thres", conf, "sizes", sizes, "kept per image", n)
        assert sum(n) > 0 and want["det_counts"].sum() == sum(n)
        res = pipe.run(*setup["runs"][k])
        got = snapshot(res)
        assert 0 < got["kept"].max() < CAND
        assert_same(got, want)
        assert np.asarray(res.sizes).tolist() == [list(s) for s in sizes]
        assert tuple(res.class_map.shape) == (3,) + CAP_SHAPE and tuple(res.rendered.shape) == (3,) + CAP_SHAPE + (3,)
        for b, (ih, iw) in enumerate(sizes):                                  # the padding of every slot is zero
            assert not got["class_map"][b, ih:].any() and not got["class_map"][b, :, iw:].any()
            assert not got["rendered"][b, ih:].any() and not got["rendered"][b, :, iw:].any()
            assert got["seg_counts"][b].sum() == ih * iw
    # the same run from a padded buffer with sizes
    frames, radar = setup["runs"][0]
    assert_same(snapshot(pipe.run(padded(frames, CAP_SHAPE), radar, sizes=RUNS[0])), setup["want"][0])
    # a fixed-size pipeline built beside it still equals its own composition
    F = (40, 56)
    frames, radar = make_run([F] * 3, 83)
    fixed = A.FramePipeline(model, F, S, batch=3, conf_thres=conf, nms_thres=NMS_THRES, max_candidates=CAND, graph=graph)
    res = fixed.run(np.stack(frames), radar)
    assert res.sizes is None and not fixed.ragged
    assert_same(snapshot(res), compose(model, frames, radar, conf, capacity=F))
    with pytest.raises(RuntimeError, match="ragged"):
        fixed.run(np.stack(frames), radar, sizes=[F] * 3)
    with pytest.raises(RuntimeError, match="host integers"):                 # a read-back would synchronise
        pipe.run(padded(setup["runs"][0][0], CAP_SHAPE), setup["runs"][0][1], sizes=cuda(np.array(RUNS[0])))


@pytest.mark.gpu
@pytest.mark.parametrize("graph", [False, True])
@pytest.mark.parametrize("form", ["device_padded", "host_list"])
def test_ragged_run_does_not_synchronise(setup, graph, form):
    pipe = setup["pipes"][graph]
    frames, radar = setup["runs"][1]
    if form == "device_padded":
        args = (cuda(padded(frames, CAP_SHAPE)), cuda(radar), RUNS[1])
    else:
        args = (frames, radar)
    pipe.run(*args)
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        res = pipe.run(*args)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    assert_same(snapshot(res), setup["want"][1])


# ---------------------------------------------------------------------------------------------- 9. EvalPipeline
EVAL_RUNS = [[(40, 56), (80, 112)], [(61, 33), (17, 29)]]
EVAL_IDS = [["1665000005", "1665000002"], ["1665000006", "1665000001"]]
MAX_BOXES, MAX_GT = 4, 4
DET_KEYS = ("map", "ap", "f1", "recall", "precision", "lamr", "n_gt", "n_det", "n_tp")


def eval_snapshot(res):
    got = {"det." + k: res.det[k].cpu().numpy() for k in DET_KEYS}
    got.update(hist=res.hist, iou=res.iou, pa_recall=res.pa_recall, precision=res.precision, accuracy=res.accuracy, miou=res.miou)
    return got


@pytest.mark.gpu
def test_eval_pipeline_ragged(tmp_path):
    from PIL import Image
    model = A.EfficientVRNet(NC, NSEG, "nano", img_size=S[0]).cuda().eval()
    A.randomize_state_dict(model.state_dict(), seed=4)
    rng = np.random.default_rng(91)
    batches = [make_run(sizes, 92 + k) for k, sizes in enumerate(EVAL_RUNS)]
    pred = compose(model, *batches[0], 0.5)["pred"]
    score = (pred[..., 4] * pred[..., 5:5 + NC].amax(-1)).flatten().sort(descending=True).values
    conf = float(score[29])
    assert conf >= evaluate.MIN_CONF
    # the expectation, image by image on the unpadded views, as tests/test_evaluate.py builds its own
    ev = metrics.DetectionEvaluator(NAMES, max_boxes=MAX_BOXES)
    hist = torch.zeros((NSEG, NSEG), dtype=torch.int64, device="cuda")
    labels, gts, pixels = [], [], 0
    for k, (frames, radar) in enumerate(batches):
        eager = compose(model, frames, radar, conf)
        labels.append([rng.integers(0, NSEG, f.shape[:2], dtype=np.uint8) for f in frames])
        gts.append([])
        for b, f in enumerate(frames):
            ih, iw = f.shape[:2]
            rows = eager["detections"][b]
            s = rows[:, 4] * rows[:, 5]
            assert len(np.unique(s)) == len(s), "equal scores in one image: the tie rule, not the code, would decide"
            label, _, box = metrics.format_detections(rows, MAX_BOXES)
            own = np.concatenate([box[:2], label[:2, None]], axis=1).astype(np.int64).reshape(-1, 5)
            x1, y1 = rng.integers(0, iw - 8, 2), rng.integers(0, ih - 8, 2)
            rand = np.stack([x1, y1, x1 + rng.integers(4, 8, 2), y1 + rng.integers(4, 8, 2), rng.integers(0, NC, 2)], axis=1)
            gts[k].append(np.concatenate([own, rand]))
            ev.add(EVAL_IDS[k][b], rows, gts[k][b])
            metrics.fast_hist(cuda(labels[k][b]), cuda(eager["class_map"][b, :ih, :iw]), NSEG, out=hist)
            pixels += ih * iw
    det = ev.compute()
    want = {"det." + k: det[k].cpu().numpy() for k in DET_KEYS}
    h = want["hist"] = hist.cpu().numpy()
    diag = np.diag(h)
    iou = diag / np.maximum(h.sum(1) + h.sum(0) - diag, 1)
    want.update(iou=iou, pa_recall=diag / np.maximum(h.sum(1), 1), precision=diag / np.maximum(h.sum(0), 1),
                accuracy=np.sum(diag) / np.maximum(np.sum(h), 1), miou=np.nanmean(iou))
    print("map", want["det.map"], "n_tp", want["det.n_tp"], "n_det", want["det.n_det"], "miou", want["miou"])
    assert want["det.n_tp"].sum() > 0 and h.sum() == pixels

    def same(res):
        got = eval_snapshot(res)
        assert res.flag == 0 and res.images == 4 and set(got) == set(want)
        for k in want:
            g, w = np.asarray(got[k]), np.asarray(want[k])
            assert g.dtype == w.dtype and g.shape == w.shape and np.array_equal(g, w, equal_nan=g.dtype.kind == "f"), (k, g, w)
        assert int(res.hist.sum()) == pixels                 # the 255 padding of the label buffer is not counted
    pipe = A.EvalPipeline(model, CAP_SHAPE, S, NAMES, NSEG, batch=2, capacity=4, max_boxes=MAX_BOXES, max_gt=MAX_GT, conf_thres=conf,
                          nms_thres=NMS_THRES, ragged=True)
    for k, (frames, radar) in enumerate(batches):
        res = pipe.add(EVAL_IDS[k], frames, radar, labels[k], gts[k])
        assert np.asarray(res.sizes).tolist() == [list(s) for s in EVAL_RUNS[k]]
    same(pipe.compute())
    # the label maps as padded buffers whose own padding is NOT 255 (0, a class that the padded class map also holds, and 3):
    # only the corners may reach labels_u8, so the matrix and its pixel total stay the same
    for fill, where in ((0, "host"), (3, "device")):
        pipe.reset()
        for k, (frames, radar) in enumerate(batches):
            lab = padded(labels[k], CAP_SHAPE, fill)
            pipe.add(EVAL_IDS[k], padded(frames, CAP_SHAPE), radar, cuda(lab) if where == "device" else lab, gts[k],
                     sizes=EVAL_RUNS[k])
        same(pipe.compute())
    # the same set from files, through evaluate_lines (which resets the pipeline first)
    radar_root, seg_root = tmp_path / "radar", tmp_path / "VOC2007"
    os.makedirs(radar_root)
    os.makedirs(seg_root / "SegmentationClass")
    os.makedirs(tmp_path / "JPEGImages")
    lines = []
    for k, (frames, radar) in enumerate(batches):
        for b, f in enumerate(frames):
            fid = EVAL_IDS[k][b] + ".12345"
            Image.fromarray(f).save(tmp_path / "JPEGImages" / (fid + ".png"))
            Image.fromarray(labels[k][b], mode="L").save(seg_root / "SegmentationClass" / (fid + ".png"))
            np.savez(radar_root / (fid + ".npz"), radar[b])
            lines.append(f"{tmp_path}/JPEGImages/{fid}.png " + " ".join(",".join(str(v) for v in g) for g in gts[k][b]) + "\n")
    same(evaluate.evaluate_lines(pipe, lines, str(radar_root), str(seg_root)))
