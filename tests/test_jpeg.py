"""The JPEG encoder on the device (csrc/jpeg.hip: vrnet_jpeg_encode_u8) against its host statement, render.jpeg_encode_host
(pinned to Pillow by tests/test_jpeg_host.py), byte for byte, and against Pillow directly on whole frames.  Then the surface
above the kernels: render.jpeg_encode / render.Jpegs, FramePipeline(jpeg=...) fixed-size and ragged, and infer.predict_dir."""
import io
import os

import numpy as np
import pytest
import torch
from PIL import Image

from asy_vrnet_amd import data, infer, render
from tests.test_chips import F, RAGGED_CAP, RAGGED_SIZES, S, fixed, inputs, model, ragged, recorded_calls  # noqa: F401
from tests.test_jpeg_host import CASES, QUALITIES, pictures, pillow

pytestmark = pytest.mark.gpu
FILL = 0xAB


def same(got, want, what):
    """Two files, with the place of the first difference in the message."""
    if got != want:
        n = min(len(got), len(want))
        at = next((i for i in range(n) if got[i] != want[i]), n)
        raise AssertionError(f"{what}: {len(got)} bytes against {len(want)}, first difference at byte {at}: "
                             f"{got[at:at + 8].hex()} against {want[at:at + 8].hex()}")


def encode(images, quality, subsampling, **kw):
    out = render.jpeg_encode(images, quality, subsampling, **kw)
    files = out.bytes()
    return out, files


@pytest.mark.parametrize("subsampling", [0, 2])
def test_the_small_shapes_equal_the_rule(subsampling):
    """Every size of the host test, every picture kind in one batch per size and quality."""
    for size in [s for s, sub in CASES if sub == subsampling]:
        batch = np.stack(list(pictures(*size).values()))
        for q in QUALITIES:
            out, files = encode(batch, q, subsampling, capacity=1 << 16)   # the default, 623 + 3 h w, is below a 1 x 1 file
            assert int(out.flag) == 0 and out.record.cpu().numpy()[:, 1].tolist() == [1] * 4
            for b, name in enumerate(pictures(*size)):
                same(files[b], render.jpeg_encode_host(batch[b], q, subsampling), (size, q, subsampling, name))


@pytest.mark.parametrize("subsampling", [0, 2])
def test_a_batch_of_mixed_sizes_in_one_call(subsampling):
    """sizes=: every file equals the image encoded alone, whatever the rest of its slot holds."""
    sizes = [(1, 1), (3, 40), (37, 53), (40, 3), (24, 40), (25, 8), (40, 56)]
    slots = np.full((len(sizes), 40, 56, 3), FILL, np.uint8)
    rng = np.random.default_rng(5)
    for b, (h, w) in enumerate(sizes):
        slots[b, :h, :w] = rng.integers(0, 256, (h, w, 3), dtype=np.uint8)
    out, files = encode(slots, 90, subsampling, sizes=sizes)
    assert int(out.flag) == 0
    for b, (h, w) in enumerate(sizes):
        same(files[b], render.jpeg_encode_host(slots[b, :h, :w], 90, subsampling), (b, h, w))
        same(files[b], encode(np.ascontiguousarray(slots[b, :h, :w]), 90, subsampling, capacity=1 << 16)[1][0], ("alone", b))
    # the geometry table of a ragged batch gives the same files
    geom = data.geometry_bytes(data.frame_geometry(sizes, S, True, (40, 56))).cuda()
    assert encode(slots, 90, subsampling, geom=geom)[1] == files
    with pytest.raises(RuntimeError, match="not both"):
        render.jpeg_encode(slots, 90, subsampling, sizes=sizes, geom=geom)


# blocks of an image on both sides of the 32 of a workgroup of the block kernel and the 256 of a scan chunk (an image has
# 3 or 6 blocks an MCU, so 256 itself is not a block count: 255 and 258 are its neighbours, 252 and 258 at 4:2:0)
@pytest.mark.parametrize("size, subsampling, blocks", [((8, 80), 0, 30), ((8, 88), 0, 33), ((40, 136), 0, 255), ((16, 344), 0, 258),
                                                       ((16, 672), 2, 252), ((16, 688), 2, 258), ((96, 176), 2, 396)])
def test_both_sides_of_the_scan_chunk(size, subsampling, blocks):
    a = np.random.default_rng(blocks).integers(0, 256, size + (3,), dtype=np.uint8)
    assert len(render.jpeg_blocks_host(a, 75, subsampling)[0]) == blocks
    for q in (30, 100):
        same(encode(a, q, subsampling, capacity=8 * a.size)[1][0], render.jpeg_encode_host(a, q, subsampling), (size, q))


@pytest.mark.parametrize("seed, raw", [(2, 1023), (7, 1024), (51, 1025)])
def test_both_sides_of_the_stuffing_chunk(seed, raw):
    """A scan of 1023, 1024 and 1025 bytes in front of the stuffing: the chunk of the count and pack kernels is 1024 bytes."""
    a = np.random.default_rng(seed).integers(0, 256, (16, 32, 3), dtype=np.uint8)
    a[:, 28:] //= 2
    want = render.jpeg_encode_host(a, 92, 0)
    scan = want[623:-2]
    assert len(scan) - scan.count(b"\xff\x00") == raw
    same(encode(a, 92, 0)[1][0], want, seed)


def test_many_stuffed_bytes_across_chunks():
    """Noise at quality 100: 0xFF bytes in every chunk of several, so the scan of the counts carries."""
    a = np.random.default_rng(9).integers(0, 256, (64, 96, 3), dtype=np.uint8)
    want = render.jpeg_encode_host(a, 100, 0)
    assert want.count(b"\xff\x00") >= 20 and len(want) > 8 * 1024
    same(encode(a, 100, 0, capacity=2 * len(want))[1][0], want, "noise")


def natural(h, w, seed=3):
    """A smooth picture with edges and some noise: what a rendered frame looks like to an encoder."""
    y, x = np.mgrid[:h, :w].astype(np.float64)
    rng = np.random.default_rng(seed)
    planes = [127 + 80 * np.sin(x / (17.0 + 9 * c) + c) * np.cos(y / (23.0 - 5 * c)) + 40 * ((x // 64 + y // 48) % 2) for c in range(3)]
    return np.clip(np.stack(planes, -1) + rng.normal(0, 4, (h, w, 3)), 0, 255).astype(np.uint8)


@pytest.mark.parametrize("size, quality, subsampling", [((480, 640), 95, 0), ((480, 640), 75, 2), ((1080, 1920), 95, 0),
                                                        ((1080, 1920), 75, 2)])
def test_a_whole_frame_against_pillow(size, quality, subsampling):
    a = natural(*size)
    same(encode(a, quality, subsampling)[1][0], pillow(a, quality, subsampling), (size, quality, subsampling))


def test_a_file_that_does_not_fit_its_slot():
    """Image 1 is noise and does not fit; 0 and 2 are unaffected.  Nothing of a slot behind its length is relied on: the
    arena is not initialised, and `bytes` reads the lengths alone."""
    batch = np.stack([np.full((24, 40, 3), 90, np.uint8), pictures(24, 40)["noise"], pictures(24, 40)["ramp"]])
    want = [render.jpeg_encode_host(a, 95, 0) for a in batch]
    capacity = max(len(want[0]), len(want[2]))
    assert capacity < len(want[1])
    out, files = encode(batch, 95, 0, capacity=capacity)
    assert int(out.flag) == render.FLAG_JPEG_ARENA == 262144
    assert out.record.cpu().numpy().tolist() == [[len(want[0]), 1], [0, 2], [len(want[2]), 1]]
    assert files[1] == b"" and files[0] == want[0] and files[2] == want[2]
    # one byte below the stuffed length does not fit, the length itself does
    for cap, fits in ((len(want[1]) - 1, False), (len(want[1]), True)):
        out, files = encode(batch[1], 95, 0, capacity=cap)
        assert (files[0] == want[1]) == fits and (int(out.flag) == 0) == fits


def test_a_record_above_its_slot_and_an_empty_one():
    """Image 1's record is no image.  ih = 25 in a slot of 16 rows is clamped to the slot: the file of the 16 x 20 picture;
    ih = 0 leaves it no pixel: no file, record (0, 3).  Either way FLAG_GEOMETRY, and image 0 as ever."""
    import asy_vrnet_amd.hip as hip
    slots = np.random.default_rng(12).integers(0, 256, (2, 16, 24, 3), dtype=np.uint8)
    geom = data.geometry_bytes(data.frame_geometry([(11, 17), (16, 20)], S, True, (16, 24))).cuda()
    good, clamped = (render.jpeg_encode_host(slots[0, :11, :17], 90, 0), render.jpeg_encode_host(slots[1, :16, :20], 90, 0))
    for ih, record, file in ((25, [len(clamped), 1], clamped), (0, [0, 3], b"")):
        hostile = geom.clone()
        hostile.view(torch.int32).view(2, -1)[1, 0] = ih
        out, files = encode(slots, 90, 0, geom=hostile, capacity=1 << 14)
        assert int(out.flag) == hip.FLAG_GEOMETRY == 256
        assert out.record.cpu().numpy().tolist() == [[len(good), 1], record]
        same(files[0], good, "image 0")
        same(files[1], file, "image 1")


def test_two_calls_give_the_same_bytes():
    a = np.stack([natural(72, 104, 1), pictures(72, 104)["noise"]])
    for subsampling in (0, 2):
        first = encode(a, 95, subsampling, capacity=8 * a[0].size)[1]
        for _ in range(3):
            assert encode(a, 95, subsampling, capacity=8 * a[0].size)[1] == first


def test_jpegs_save_and_the_chips_tensor(tmp_path):
    """Any (N, h, w, 3) uint8 tensor on the device: here N equal-sized chips."""
    chips = torch.from_numpy(np.random.default_rng(4).integers(0, 256, (5, 16, 12, 3), dtype=np.uint8)).cuda()
    out = render.jpeg_encode(chips, quality=80, subsampling=2)
    paths = [str(tmp_path / f"chip_{i}.jpg") for i in range(5)]
    paths[3] = None
    files = out.save(paths)
    assert sorted(os.listdir(tmp_path)) == ["chip_0.jpg", "chip_1.jpg", "chip_2.jpg", "chip_4.jpg"]
    for i in (0, 1, 2, 4):
        assert open(paths[i], "rb").read() == files[i] == render.jpeg_encode_host(chips[i].cpu().numpy(), 80, 2)


def test_keyword_errors_raise_before_anything_is_enqueued(model, fixed):
    import asy_vrnet_amd as A
    a = np.zeros((2, 8, 8, 3), np.uint8)
    for kw, match in ((dict(quality=0), "quality"), (dict(quality=101), "quality"), (dict(subsampling=1), "subsampling"),
                      (dict(capacity=100), "capacity"), (dict(sizes=[(9, 8), (8, 8)]), "bad size"),
                      (dict(sizes=[(8, 8)]), "sizes")):
        with pytest.raises(RuntimeError, match=match):
            render.jpeg_encode(a, **kw)
    for bad, extra, match in (({"quality": 0}, {}, "quality"), ({"subsampling": 1}, {}, "subsampling"),
                              ({"source": "heat"}, {}, "source"), ({"size": 3}, {}, "jpeg is"), (7, {}, "jpeg is"),
                              (True, {"render": False}, "render=True"), ({"source": "rendered"}, {"render": False}, "render=True"),
                              ({"capacity": 10}, {}, "capacity")):
        with pytest.raises(RuntimeError, match=match):
            A.FramePipeline(model, F, S, jpeg=bad, **extra, **fixed["kw"])
    assert infer.jpeg_config(None, True) is None
    assert infer.jpeg_config(True, True) == dict(quality=95, subsampling=0, source="rendered", capacity=None)
    torch.cuda.synchronize()


# ---- the pipeline ------------------------------------------------------------------------------------------------------------
def sizes_of(kind):
    return [F] * 2 if kind == "fixed" else RAGGED_SIZES


@pytest.mark.parametrize("graph", [True, False])
@pytest.mark.parametrize("kind", ["fixed", "ragged"])
def test_pipeline_files_are_the_rule_on_the_rendered_frame(kind, graph, model, request):
    import asy_vrnet_amd as A
    setup = request.getfixturevalue(kind)
    cfg = dict(quality=90, subsampling=2) if kind == "ragged" else True
    pipe = A.FramePipeline(model, F if kind == "fixed" else RAGGED_CAP, S, jpeg=cfg, graph=graph, **setup["kw"])
    assert (pipe.graph is not None) == graph and [type(s).__name__ for s in pipe.stages] == ["Jpeg"]
    q, sub = (95, 0) if cfg is True else (90, 2)
    seen = []
    for name, sizes in (("first", sizes_of(kind)), ("second", sizes_of(kind)[::-1]), ("first", sizes_of(kind))):
        res = pipe.run(*setup[name])
        assert isinstance(res.jpeg, render.Jpegs) and res.jpeg is pipe.result.jpeg
        files, rendered = res.jpeg.bytes(), res.rendered.cpu().numpy()
        assert int(res.flag) == 0
        for b, (ih, iw) in enumerate(sizes):
            same(files[b], render.jpeg_encode_host(rendered[b, :ih, :iw], q, sub), (kind, graph, name, b))
            assert Image.open(io.BytesIO(files[b])).size == (iw, ih)
        seen.append(files)
    assert seen[0] != seen[1] and seen[0] == seen[2]                       # each input's own files, and the same bytes again


def test_source_frames_encodes_the_dehazed_frame(model, fixed):
    import asy_vrnet_amd as A
    pipe = A.FramePipeline(model, F, S, dehaze=dict(r=8), render=False, jpeg=dict(source="frames", quality=85), **fixed["kw"])
    res = pipe.run(*fixed["first"])
    files, dehazed = res.jpeg.bytes(), res.dehazed.cpu().numpy()
    assert res.rendered is None and not np.array_equal(dehazed, fixed["first"][0])
    for b in range(2):
        same(files[b], render.jpeg_encode_host(dehazed[b], 85, 0), b)
    # without the stage in front, the frames as they came
    pipe = A.FramePipeline(model, F, S, jpeg=dict(source="frames"), graph=False, **fixed["kw"])
    files = pipe.run(*fixed["first"]).jpeg.bytes()
    for b in range(2):
        same(files[b], render.jpeg_encode_host(fixed["first"][0][b], 95, 0), b)


def test_a_pipeline_file_that_does_not_fit(model, fixed):
    import asy_vrnet_amd as A
    pipe = A.FramePipeline(model, F, S, jpeg=dict(capacity=700), graph=False, **fixed["kw"])
    res = pipe.run(*fixed["first"])
    assert res.jpeg.bytes() == [b"", b""] and int(res.flag) & infer.FLAG_JPEG_ARENA


def test_without_jpeg_the_chain_issues_the_calls_it_issued_before(model, fixed, monkeypatch):
    """Every wrapper of hip.py the chain calls, in order: jpeg=None never reaches jpeg_encode and issues the calls of a pipeline
    built without the keyword; jpeg=True adds exactly that one call, the last of the chain."""
    import asy_vrnet_amd as A
    calls = recorded_calls(monkeypatch)

    def chain(**extra):
        pipe = A.FramePipeline(model, F, S, graph=False, **extra, **fixed["kw"])
        del calls[:]
        with torch.no_grad():
            result = pipe._chain()
        torch.cuda.synchronize()
        return list(calls), result
    (without, bare), (none, _), (jpeg, full) = chain(), chain(jpeg=None), chain(jpeg=True)
    assert none == without and "jpeg_encode" not in without and bare.jpeg is None
    assert jpeg == without + ["jpeg_encode"] and isinstance(full.jpeg, render.Jpegs)
    heat, _ = chain(jpeg=True, heatmap=True, chips=(8, 8))
    assert heat[-2:] == ["heatmap", "jpeg_encode"] and heat.index("chip_boxes") < heat.index("render")


def test_predict_dir_writes_the_jpg_beside_the_png(model, ragged, tmp_path):
    import asy_vrnet_amd as A
    sizes = [(40, 56), (48, 68), (23, 41)]
    frames, radar = inputs(78, sizes)
    src, radar_root, dst = tmp_path / "in", tmp_path / "radar", tmp_path / "out"
    src.mkdir()
    radar_root.mkdir()
    names = [f"{1600000000 + b}.{b:05d}.png" for b in range(3)]
    for b, n in enumerate(names):
        Image.fromarray(frames[b]).save(src / n)
        np.savez(radar_root / (data.frame_id(n) + ".npz"), radar[b])
    pipe = A.FramePipeline(model, RAGGED_CAP, S, jpeg=dict(quality=75, subsampling=2), **ragged["kw"])
    out = infer.predict_dir(pipe, str(src), str(radar_root), str(dst))      # batch 2: the last call repeats picture 2
    assert [n for n, _ in out] == names
    assert sorted(os.listdir(dst)) == sorted([n[:-4] + ".png" for n in names] + [n[:-4] + ".jpg" for n in names])
    for n, (ih, iw) in zip(names, sizes):
        png = np.array(Image.open(dst / (n[:-4] + ".png")))
        assert png.shape == (ih, iw, 3)
        same(open(dst / (n[:-4] + ".jpg"), "rb").read(), pillow(png, 75, 2), n)
