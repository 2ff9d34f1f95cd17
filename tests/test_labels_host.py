"""The host half of the detection labels (render.LabelAtlas, score_index, draw_labels_host) against live Pillow: the atlas
holds exactly what ImageDraw.text pastes, the score index is Python's own '{:.2f}', and the numpy statement of the drawing
rule equals yolo.py:198-224 run with Pillow byte for byte.  No GPU."""
import glob
import os
import sys

import numpy as np
import pytest
import torch

from asy_vrnet_amd import render
from tests import labels_cases as LC

NAMES = LC.CLASS_NAMES


def dejavu_path():
    roots = ["/usr/share/fonts/truetype/dejavu"]
    try:
        import matplotlib
        roots.insert(0, os.path.join(matplotlib.get_data_path(), "fonts", "ttf"))
    except ImportError:
        pass
    for root in roots:
        hits = glob.glob(os.path.join(root, "DejaVuSans.ttf"))
        if hits:
            return hits[0]
    return None


def mask_array(mask):
    from PIL import Image
    w, h = mask.size
    return np.frombuffer(Image.Image()._new(mask).tobytes(), np.uint8).reshape(h, w) if w and h else np.zeros((h, w), np.uint8)


@pytest.mark.parametrize("face", ["builtin", "dejavu"])
def test_atlas_round_trip(face):
    ImageFont = pytest.importorskip("PIL.ImageFont")
    if face == "dejavu":
        path = dejavu_path()
        if path is None:
            pytest.skip("no DejaVuSans.ttf on this machine")
        font, make = path, lambda size: ImageFont.truetype(path, size)
    else:
        font, make = None, ImageFont.load_default
    sizes, names = (8, 10, 32), ("tv/monitor", "Wy", "a")
    atlas = render.LabelAtlas(names, font, sizes)
    assert atlas.records.shape == (3, 3 * 101, 8) and atlas.records.dtype == np.int32 and atlas.blob.dtype == np.uint8
    assert atlas.nbytes == atlas.blob.nbytes + atlas.records.nbytes and atlas.num_classes == 3
    end = 0
    for size in sizes:
        f = make(size)
        for c, name in enumerate(names):
            for k in range(101):
                label = f"{name} {k / 100:.2f}"
                assert label == "{} {:.2f}".format(name, k / 100)
                mask, off = f.getmask2(label, "L")
                got, got_off, got_size = atlas.record(size, c, k)
                assert np.array_equal(got, mask_array(mask)), (face, size, label)
                assert got_off == tuple(off) and got_size == tuple(f.getbbox(label)[2:4]), (face, size, label)
                rec = atlas.records[atlas.size_index(size), c * 101 + k]
                assert rec[0] == end and rec[7] == 0            # the masks lie back to back
                end += int(rec[1]) * int(rec[2])
    assert end == atlas.blob.size
    # a callable gives the same atlas, and the arrays alone rebuild it
    again = render.LabelAtlas(names, make, sizes)
    assert np.array_equal(again.blob, atlas.blob) and np.array_equal(again.records, atlas.records)
    copy = render.LabelAtlas.from_arrays(names, sizes, atlas.blob, atlas.records)
    assert copy.class_names == atlas.class_names and copy.sizes == atlas.sizes and copy.nbytes == atlas.nbytes


def test_committed_fixture_is_the_builtin_atlas():
    pytest.importorskip("PIL")
    fixture = render.LabelAtlas.load(LC.FIXTURE)
    assert os.path.getsize(LC.FIXTURE) < 1 << 20
    live = render.LabelAtlas(LC.CLASS_NAMES, None, LC.FIXTURE_SIZES)
    assert fixture.class_names == live.class_names and fixture.sizes == live.sizes
    assert np.array_equal(fixture.blob, live.blob) and np.array_equal(fixture.records, live.records)


def python_index(s):
    return int("{:.2f}".format(float(s)).replace(".", ""))


def tie_set():
    """The two float32 neighbours of every (k + 0.5) / 100 and the value itself, the exact ties, the ends and subnormals."""
    v = []
    for k in range(101):
        x = np.float32((k + 0.5) / 100)
        v += [np.nextafter(x, np.float32(0)), x, np.nextafter(x, np.float32(2))]
    v += [0.125, 0.375, 0.625, 0.875, 0.0, 1.0, 1e-45, 1e-40, 1.1754942e-38, 1.17549435e-38, 0.005, 0.995]
    v = np.array(v, np.float32)
    return v[v <= 1]


def test_score_index_is_pythons_format():
    s = tie_set()
    assert np.array_equal(render.score_index(s), [python_index(x) for x in s])
    got = dict(zip(s.tolist(), render.score_index(s).tolist()))
    assert (got[0.125], got[0.375], got[0.625], got[0.875], got[0.0], got[1.0]) == (12, 38, 62, 88, 0, 100)
    r = np.random.default_rng(7).random(100000, dtype=np.float32)
    k, bits = render.score_index(r, True)
    assert bits == 0 and k.dtype == np.int32 and np.array_equal(k, [python_index(x) for x in r])
    # one fp32 multiply, as yolo.py:157
    obj, conf = np.float32(0.7), np.float32(0.55)
    assert render.score_index(np.array([obj * conf]))[0] == python_index(np.float32(obj) * np.float32(conf))
    k, bits = render.score_index(np.array([np.nan, -0.1, 1.5, -0.0, 0.5], np.float32), True)
    assert bits == render.FLAG_LABEL_SCORE == 2048 and k.tolist() == [0, 0, 100, 0, 50]
    assert render.score_index(np.zeros((2, 3), np.float32)).shape == (2, 3)
    with pytest.raises(RuntimeError, match="float32"):
        render.score_index(np.zeros(3, np.float64))


def test_label_font_size():
    assert [render.label_font_size(h) for h in (1, 16, 17, 33, 64, 270, 1080)] == [0, 0, 1, 1, 2, 8, 32]
    assert all(render.label_font_size(h) == int(np.floor(3e-2 * h + 0.5).astype("int32")) for h in range(1, 3000))


# ---- draw_labels_host against yolo.py:198-224 run with live Pillow --------------------------------------------------------------

def pillow_picture(picture, rows, scores, names, font, thickness, palette):
    """yolo.py:198-224 with textbbox for the size (Pillow 12 has no textsize)."""
    from PIL import Image, ImageDraw
    image = Image.fromarray(picture)
    for (left, top, right, bottom, c), score in zip(rows.tolist(), scores):
        colour = tuple(int(v) for v in palette[c])
        label = "{} {:.2f}".format(names[c], score)
        draw = ImageDraw.Draw(image)
        label_size = np.array(draw.textbbox((0, 0), label, font)[2:4])
        if top - label_size[1] >= 0:
            text_origin = np.array([left, top - label_size[1]])
        else:
            text_origin = np.array([left, top + 1])
        for i in range(thickness):
            draw.rectangle([left + i, top + i, right - i, bottom - i], outline=colour)
        draw.rectangle([tuple(int(v) for v in text_origin), tuple(int(v) for v in text_origin + label_size)], fill=colour)
        draw.text(tuple(int(v) for v in text_origin), label, fill=(0, 0, 0), font=font)
        del draw
    return np.array(image)


def fixed_cases(ih, iw, t, lh):
    """Named layouts on an ih x iw image at thickness t for labels lh rows high; every box is at least 2 t wide and high."""
    m = 2 * t
    bw, bh = max(m, iw // 3), max(m, ih // 4)
    box = lambda left, top, w=bw, h=bh, c=0: (left, top, min(left + w, iw), min(top + h, ih), c)
    mid = min(max(lh + 2, ih // 3), ih - m)
    cases = {
        "above": [box(iw // 4, mid)],
        "flips below": [box(iw // 4, max(lh - 1, 0), c=1)],
        "clipped right": [box(iw - m - 1, mid, w=m, c=2)],
        "clipped bottom": [box(2, 0, h=max(ih - 3, m), c=3)],
        "corners": [box(0, 0, m, m), box(iw - m, 0, m, m, 1), box(0, ih - m, m, m, 2), box(iw - m, ih - m, m, m, 3)],
        "label over label text": [box(iw // 5, mid, c=0), box(iw // 5 + 3, mid + 2, c=1), box(iw // 5 + 1, mid + 1, c=3)],
        "ring across a label": [box(iw // 4, mid, c=2), box(iw // 4 + 4, max(mid - lh // 2 - 1, 0), w=max(m, iw // 2), h=max(m, lh), c=0)],
        "identical": [box(iw // 3, mid, c=1), box(iw // 3, mid, c=1)],
        "none": [],
    }
    for name, rows in cases.items():
        for left, top, right, bottom, _ in rows:
            assert right - left >= m and bottom - top >= m and 0 <= left and 0 <= top, (name, ih, iw, t)
    return cases


@pytest.mark.parametrize("thickness", [1, 3])
@pytest.mark.parametrize("ih,iw,size", [(64, 96, 10), (33, 47, 8), (120, 200, 32), (40, 60, 1)])
def test_host_statement_equals_live_pillow(ih, iw, size, thickness):
    ImageFont = pytest.importorskip("PIL.ImageFont")
    font = ImageFont.load_default(size)
    atlas = render.LabelAtlas(NAMES, None, (size,))
    pal = render.det_palette(len(NAMES))
    rng = np.random.default_rng(1000 * ih + 10 * size + thickness)
    picture = rng.integers(0, 256, (ih, iw, 3), dtype=np.uint8)
    lh = int(atlas.records[0, :, 6].max())
    cases = [(name, np.array(rows, np.int32).reshape(-1, 5)) for name, rows in fixed_cases(ih, iw, thickness, lh).items()]
    cases += [(f"random {n}", LC.random_case(rng, ih, iw, n, thickness)[0]) for n in (1, 7, 40)]
    flipped = clipped = 0
    for name, rows in cases:
        scores = rng.random(len(rows), dtype=np.float32) * rng.random(len(rows), dtype=np.float32)
        if len(scores):
            scores[0] = np.float32(0.125)
        want = pillow_picture(picture, rows, scores, NAMES, font, thickness, pal)
        got = render.draw_labels_host(picture, rows, scores, atlas, size, thickness, pal)
        bad = int((got != want).any(axis=2).sum())
        print(f"{ih}x{iw} font {size} thickness {thickness} {name}: {bad} pixels differ")
        assert np.array_equal(got, want), name
        # the outlines may already be on the picture (the device draws them first): the same bytes
        ringed = render.draw_labels_host(picture, rows, scores, atlas, 0, thickness, pal)
        assert np.array_equal(render.draw_labels_host(ringed, rows, scores, atlas, size, thickness, pal), want), name
        for (left, top, _, _, c), k in zip(rows.tolist(), render.score_index(scores).tolist()):
            _, _, (lw, h) = atlas.record(size, c, k)
            flipped += top - h < 0
            clipped += left + lw >= iw or (top - h < 0 and top + 1 + h >= ih)
    assert flipped > 0 and clipped > 0                       # the cases reach both branches and both clipped edges


def test_font_size_zero_draws_the_rings_only():
    pytest.importorskip("PIL")
    atlas = LC.atlas()
    rng = np.random.default_rng(3)
    picture = rng.integers(0, 256, (16, 40, 3), dtype=np.uint8)
    rows, scores = LC.random_case(rng, 16, 40, 5, 1)
    assert render.label_font_size(16) == 0
    got = render.draw_labels_host(picture, rows, scores, atlas, None, 1)
    from PIL import Image, ImageDraw
    image = Image.fromarray(picture)
    draw = ImageDraw.Draw(image)
    for left, top, right, bottom, c in rows.tolist():
        draw.rectangle([left, top, right, bottom], outline=tuple(int(v) for v in render.det_palette(4)[c]))
    assert np.array_equal(got, np.array(image))


def test_argument_errors(monkeypatch):
    atlas = render.LabelAtlas.load(LC.FIXTURE)               # needs no Pillow
    picture, rows, scores = np.zeros((40, 60, 3), np.uint8), np.array([[2, 20, 30, 35, 1]], np.int32), np.array([0.5], np.float32)
    with pytest.raises(RuntimeError, match="was not built"):
        atlas.size_index(9)
    with pytest.raises(RuntimeError, match="was not built"):
        render.draw_labels_host(picture, rows, scores, atlas, 9, 1)
    with pytest.raises(RuntimeError, match="image 1 of 1080 rows needs font size 32"):
        atlas.size_table([270, 1080])
    assert atlas.size_table([270, 12, 17, 320]).tolist() == [1, -1, 0, 2]
    with pytest.raises(RuntimeError, match="uint8"):
        render.draw_labels_host(picture.astype(np.float32), rows, scores, atlas, 8, 1)
    with pytest.raises(RuntimeError, match="int32"):
        render.draw_labels_host(picture, rows.astype(np.int64), scores, atlas, 8, 1)
    with pytest.raises(RuntimeError, match="float32"):
        render.draw_labels_host(picture, rows, scores.astype(np.float64), atlas, 8, 1)
    with pytest.raises(RuntimeError, match="4 classes, the box palette 5 colours"):
        render.draw_labels_host(picture, rows, scores, atlas, 8, 1, render.det_palette(5))
    with pytest.raises(RuntimeError, match="thickness"):
        render.draw_labels_host(picture, rows, scores, atlas, 8, 0)
    with pytest.raises(RuntimeError, match="LabelAtlas"):
        render.draw_labels_host(picture, rows, scores, "atlas", 8, 1)
    with pytest.raises(RuntimeError, match="sizes"):
        render.LabelAtlas(NAMES, None, (0,))
    with pytest.raises(RuntimeError, match="class names"):
        render.LabelAtlas((), None, (8,))
    with pytest.raises(RuntimeError, match="outside the blob"):
        render.LabelAtlas.from_arrays(atlas.class_names, atlas.sizes, atlas.blob[:-1], atlas.records)
    # the public entry points check before they touch a device
    frames = np.zeros((1, 40, 60, 3), np.uint8)
    results = [np.array([[20, 2, 35, 30, 0.9, 0.9, 1.0]], np.float32)]
    with pytest.raises(RuntimeError, match="LabelAtlas"):
        render.draw_boxes(frames, results, (64, 64), labels=True)
    with pytest.raises(RuntimeError, match="4 classes, the box palette 5 colours"):
        render.draw_boxes(frames, results, (64, 64), palette=5, labels=atlas)
    with pytest.raises(RuntimeError, match="was not built"):
        render.render_frame(frames, None, results, (64, 64), labels=atlas, font_size=9)
    with pytest.raises(RuntimeError, match="labels need results"):
        render.render_frame(frames, None, None, labels=atlas)
    with pytest.raises(RuntimeError, match="on a GPU"):
        render.draw_labels(torch.zeros(1, 40, 60, 3, dtype=torch.uint8), results, atlas, (64, 64))
    # without Pillow an atlas cannot be built, and says so; everything else keeps working
    monkeypatch.setitem(sys.modules, "PIL", None)
    with pytest.raises(RuntimeError, match="needs Pillow"):
        render.LabelAtlas(NAMES, None, (8,))
    assert render.LabelAtlas.load(LC.FIXTURE).nbytes == atlas.nbytes
    assert render.draw_labels_host(picture, rows, scores, atlas, 8, 1).shape == picture.shape


def test_exports_and_fake_kernels_give_the_output_shapes():
    import asy_vrnet_amd.hip as hip
    import asy_vrnet_amd.ops  # noqa: F401
    from torch._subclasses.fake_tensor import FakeTensorMode
    for name in ("vrnet_label_index_f32", "vrnet_render_labels_u8", "vrnet_render_labels_ragged_u8"):
        assert name in hip.EXPORTED
    assert hip.FLAG_LABEL_SCORE == render.FLAG_LABEL_SCORE and hip.LABEL_SCORES == render.LABEL_SCORES == 101
    for name in ("LabelAtlas", "label_font_size", "score_index", "draw_labels_host", "draw_labels"):
        assert callable(getattr(render, name))
    i32 = dict(dtype=torch.int32)
    with FakeTensorMode():
        picture = torch.empty((3, 40, 70, 3), dtype=torch.uint8)
        out = torch.ops.vrnet.render_labels(picture, torch.empty((5, 5), **i32), torch.empty(4, **i32),
                                            torch.empty((4, 3), dtype=torch.uint8), 2, torch.empty(5, **i32),
                                            torch.empty(1000, dtype=torch.uint8), torch.empty((2, 404, 8), **i32), 1)
        idx = torch.ops.vrnet.label_index(torch.empty((3, 6, 7)), torch.empty(3, **i32), torch.empty(4, **i32), 4)
    assert tuple(out.shape) == (3, 40, 70, 3) and out.dtype == torch.uint8
    assert tuple(idx.shape) == (18,) and idx.dtype == torch.int32
