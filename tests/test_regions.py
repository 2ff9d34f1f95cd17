"""The connected regions on the GPU: vrnet_seg_regions_u8 (csrc/regions.hip) against the host statement
`decode.seg_regions_host`, bit for bit on int32 views of labels, table, head, box_regions and the flag, with every output
pre-filled with -7; and the pipelines built with regions against the same pipelines without it.

B = 3 with a different image per slot; one slot all background and one a single class everywhere (one region, the deepest
tree).  Shapes: 150 x 260 -- three 64 x 16 tiles and a partial one across, nine and a partial one down, 20 chunks of 2048
pixels, the last partial -- for the noise maps of tests/test_regions_host.py and the patterns that break a labelling kernel
(checkerboard, serpentine, diagonal stripes of every phase, comb, U); the tiny sizes (1, 1), (1, 97), (97, 1), (2, 2); ragged
slots of (80, 112).  Pipelines: nano, 64 x 64, B = 2."""
import os

import numpy as np
import pytest
import torch

from tests.test_regions_host import (BIG, NOISE, SIZES, blobs, checkerboard, comb, noise, random_rows, serpentine, stripes,
                                     u_shape)

pytestmark = pytest.mark.gpu

NB = 3


@pytest.fixture(scope="module")
def A():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    import asy_vrnet_amd
    from asy_vrnet_amd import data, decode, hip, infer, evaluate  # noqa: F401  (A.data, A.decode, A.hip, ... below)
    return asy_vrnet_amd


def cuda(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def words(a):
    """Any array of 4-byte words (REGION_DTYPE records included) as int32."""
    a = a.detach().cpu().numpy() if torch.is_tensor(a) else np.asarray(a)
    return np.frombuffer(np.ascontiguousarray(a).tobytes(), np.int32)


class Buffers:
    """The outputs and the workspace of one shape, kept across calls."""

    def __init__(self, A, B, ihm, iwm, R, cap):
        i32 = dict(dtype=torch.int32, device="cuda")
        self.labels, self.table = torch.empty((B, ihm, iwm), **i32), torch.empty((B, R, 12), **i32)
        self.head, self.links, self.flag = torch.empty((B, 4), **i32), torch.empty((B, cap), **i32), torch.zeros(1, **i32)
        self.ws = torch.empty(A.hip.seg_regions_workspace_bytes(B, ihm, iwm), dtype=torch.uint8, device="cuda")

    def call(self, A, maps, rows, offsets, p, geom=None, fill=True):
        if fill:
            for t in (self.labels, self.table, self.head, self.links):
                t.fill_(-7)                                      # every element must be written
        self.flag.zero_()
        gate = None if p["det_to_seg"] is None else torch.tensor(p["det_to_seg"], dtype=torch.int32, device="cuda")
        A.hip.seg_regions(maps, rows, offsets, self.labels, self.table, self.head, self.links, self.ws, p["connectivity"],
                          p["background"], p["min_area"], det_to_seg=gate, geom=geom, flag=self.flag)
        return [t.cpu().numpy() for t in (self.labels, self.table, self.head, self.links)] + [int(self.flag.item())]


def packed_rows(rows_per_image):
    """(rows (N >= 1, 5), offsets (B + 1)) on the device and the widest image's count."""
    counts = [len(r) for r in rows_per_image]
    rows = np.concatenate([np.asarray(r, np.int32).reshape(-1, 5) for r in rows_per_image] + [np.zeros((1, 5), np.int32)])
    return cuda(rows), cuda(np.concatenate([[0], np.cumsum(counts)]).astype(np.int32)), max(max(counts), 1)


def compare(A, images, rows_per_image=None, slot=None, buffers=None, **params):
    """One device call on the images (one per slot; with `slot` a ragged batch in slots of that size) against the host rule
    per image.  Returns the host heads."""
    p = A.decode.check_region_params(params, "test")
    B = len(images)
    rows_per_image = [np.zeros((0, 5), np.int32)] * B if rows_per_image is None else rows_per_image
    rows, offsets, cap = packed_rows(rows_per_image)
    ihm, iwm = slot if slot is not None else images[0].shape
    maps = np.full((B, ihm, iwm), 3, np.uint8)                   # a class outside the images: it must connect nothing
    for b, im in enumerate(images):
        maps[b, :im.shape[0], :im.shape[1]] = im
    geom = None
    if slot is not None:
        table = A.data.frame_geometry([im.shape for im in images], (64, 64), True, slot)
        geom = A.data.geometry_bytes(table).cuda()
    buf = buffers or Buffers(A, B, ihm, iwm, p["max_regions"], cap)
    labels, table, head, links, flag = buf.call(A, cuda(maps), rows, offsets, p, geom)
    want_flag, heads = 0, []
    for b, im in enumerate(images):
        wl, wt, wh, wb, wf = A.decode.seg_regions_host(im, rows_per_image[b], **p)
        ih, iw = im.shape
        full = np.zeros((ihm, iwm), np.int32)
        full[:ih, :iw] = wl
        assert np.array_equal(labels[b], full), (b, np.argwhere(labels[b] != full)[:5].tolist())
        assert np.array_equal(head[b], wh), (b, head[b], wh)
        assert np.array_equal(words(table[b]), words(wt)), (b, np.flatnonzero(words(table[b]) != words(wt))[:12].tolist())
        assert np.array_equal(links[b], np.concatenate([wb, np.zeros(cap - len(wb), np.int32)])), b
        want_flag |= wf
        heads.append(wh)
    assert flag == want_flag
    return heads


def test_noise_against_the_host_rule(A):
    for connectivity in (8, 4):
        images = [noise(p, k, BIG) for p, k in NOISE]
        rows = [random_rows(20 + b, 30, BIG) for b in range(NB)]
        heads = compare(A, images, rows, connectivity=connectivity)
        assert all(h[0] > 1024 for h in heads)                   # the prefix and the flag
        heads = compare(A, images, rows, connectivity=connectivity, min_area=4, max_regions=4096, det_to_seg=(1, 2, 3, 9))
        assert all(0 < h[0] <= 4096 and h[3] > 0 for h in heads)
        compare(A, images, connectivity=connectivity, background=-1, max_regions=7)
        compare(A, [noise(p, k, (67, 131)) for p, k in NOISE], connectivity=connectivity, max_regions=4096)


@pytest.mark.parametrize("size", [s for s in SIZES if s[0] * s[1] < 100])
def test_tiny_sizes(A, size):
    for connectivity in (8, 4):
        compare(A, [noise(p, k, size) for p, k in NOISE], [random_rows(b, 3, size) for b in range(NB)], connectivity=connectivity)
        compare(A, [noise(p, k, size) for p, k in NOISE], connectivity=connectivity, background=-1)


def test_empty_full_and_blobs(A):
    images = [np.zeros(BIG, np.uint8), np.full(BIG, 5, np.uint8), blobs()]
    rows = [random_rows(7 + b, 25, BIG, classes=9) for b in range(NB)]
    for connectivity in (8, 4):
        heads = compare(A, images, rows, connectivity=connectivity)
        assert heads[0].tolist() == [0, 0, 0, 0] and heads[1].tolist() == [1, 1, BIG[0] * BIG[1], 0] and 100 < heads[2][0] < 1024
        compare(A, images, rows, connectivity=connectivity, det_to_seg=tuple(range(9)), min_area=50)
    heads = compare(A, images, rows, background=-1)
    assert heads[0].tolist() == [1, 1, BIG[0] * BIG[1], 0]


def test_patterns_that_break_a_labelling_kernel(A):
    heads = compare(A, [checkerboard(), serpentine(), comb()], connectivity=8)
    assert [h[0] for h in heads] == [1, 1, 1] and heads[1][2] == 19574
    heads = compare(A, [checkerboard(), serpentine(), u_shape()], connectivity=4, max_regions=4096)
    assert [h[0] for h in heads] == [19500, 1, 1]
    for sign in (1, -1):
        images = [stripes(sign, s) for s in range(3)]
        compare(A, images, connectivity=8)
        heads = compare(A, images, connectivity=4, max_regions=4096)
        assert [h[0] for h in heads] == [int(m.sum()) for m in images]
    compare(A, [u_shape(), comb(), 2 * checkerboard()], connectivity=8, rows_per_image=[random_rows(b, 5, BIG) for b in range(NB)])


def test_no_stale_state_and_equal_bytes_on_every_call(A):
    p = dict(connectivity=8, max_regions=1024)
    buf = Buffers(A, NB, BIG[0], BIG[1], 1024, 30)
    busy = [noise(pp, k, BIG) for pp, k in NOISE]
    empty = [np.zeros(BIG, np.uint8)] * NB
    rows = [random_rows(40 + b, 30, BIG) for b in range(NB)]
    for order in ((busy, empty, busy), (empty, busy, empty)):
        for images in order:
            compare(A, images, rows, buffers=buf, **p)
    # the same call twice, without refilling the outputs in between: equal bytes
    params = A.decode.check_region_params(p, "test")
    d_rows, d_offsets, _ = packed_rows(rows)
    maps = cuda(np.stack(busy))
    first = buf.call(A, maps, d_rows, d_offsets, params)
    second = buf.call(A, maps, d_rows, d_offsets, params, fill=False)
    assert all(np.array_equal(a, b) for a, b in zip(first[:4], second[:4])) and first[4] == second[4] == A.decode.FLAG_REGIONS


def test_ragged_slots(A):
    sizes = [(40, 56), (80, 112), (61, 33)]
    images = [np.random.RandomState(9 + b).randint(0, 3, s).astype(np.uint8) for b, s in enumerate(sizes)]
    rows = [random_rows(50 + b, 12, s) for b, s in enumerate(sizes)]
    for connectivity in (8, 4):
        compare(A, images, rows, slot=(80, 112), connectivity=connectivity, background=-1, max_regions=4096)
        compare(A, images, rows, slot=(80, 112), connectivity=connectivity, min_area=3, det_to_seg=(1, 2, 1, 2))
    # a constant class everywhere, padding included: nothing outside an image is labelled or connected
    same = [np.full(s, 3, np.uint8) for s in sizes]
    heads = compare(A, same, slot=(80, 112), background=-1)
    assert [h.tolist() for h in heads] == [[1, 1, s[0] * s[1], 0] for s in sizes]


def test_a_record_above_its_slot_and_an_empty_one(A):
    """Image 1's record is no image.  ih = 25 in a slot of 16 rows is clamped to the slot: the regions of a 16 x 20 image;
    ih = 0 leaves it no pixel: no label, no record, no link, a head of zeros.  Either way FLAG_GEOMETRY, and image 0 as ever."""
    slot, good = (16, 24), (11, 17)
    p = A.decode.check_region_params(dict(connectivity=8, background=-1), "test")
    maps = np.full((2,) + slot, 3, np.uint8)
    maps[0, :11, :17] = np.random.RandomState(70).randint(0, 3, good)
    maps[1, :16, :20] = np.random.RandomState(71).randint(0, 3, (16, 20))
    per_image = [random_rows(60, 3, good), random_rows(61, 3, (16, 20))]
    rows, offsets, cap = packed_rows(per_image)
    buf = Buffers(A, 2, slot[0], slot[1], p["max_regions"], cap)
    geom = A.data.geometry_bytes(A.data.frame_geometry([good, (16, 20)], (64, 64), True, slot)).cuda()
    for ih, seen in ((25, [good, (16, 20)]), (0, [good])):
        hostile = geom.clone()
        hostile.view(torch.int32).view(2, -1)[1, 0] = ih
        labels, table, head, links, flag = buf.call(A, cuda(maps), rows, offsets, p, hostile)
        assert flag == A.hip.FLAG_GEOMETRY == 256
        for b, (h, w) in enumerate(seen):
            wl, wt, wh, wb, wf = A.decode.seg_regions_host(maps[b, :h, :w], per_image[b], **p)
            assert wf == 0 and wh[0] > 3
            assert np.array_equal(labels[b, :h, :w], wl) and not labels[b, h:].any() and not labels[b, :, w:].any()
            assert np.array_equal(head[b], wh) and np.array_equal(words(table[b]), words(wt))
            assert np.array_equal(links[b], np.concatenate([wb, np.zeros(cap - len(wb), np.int32)]))
        if ih == 0:
            assert not labels[1].any() and head[1].tolist() == [0, 0, 0, 0] and not words(table[1]).any() and not links[1].any()


def test_the_eager_call(A):
    images = np.stack([blobs(), noise(0.5, 2, BIG)])
    dets = [np.array([[10.5, 20.2, 90.9, 200.0, 0.9, 0.8, 1], [0, 0, 150, 260, 0.9, 0.9, 2]], np.float32), None]
    labels, table, head, links, flag = A.decode.seg_regions(images, dets, min_area=2)
    assert tuple(table.shape) == (2, 1024, 12) and tuple(links.shape) == (2, 2) and tuple(head.shape) == (2, 4)
    rows = A.render.box_rows(dets, BIG, 4)[0]
    for b, r in enumerate((rows, np.zeros((0, 5), np.int32))):
        wl, wt, wh, wb, wf = A.decode.seg_regions_host(images[b], r, min_area=2)
        assert np.array_equal(labels[b].cpu().numpy(), wl) and np.array_equal(words(table[b]), words(wt))
        assert np.array_equal(head[b].cpu().numpy(), wh) and links[b, :len(wb)].tolist() == wb.tolist()
    assert int(flag.item()) == A.decode.FLAG_REGIONS
    one = A.decode.seg_regions(images[0], None, connectivity=4)
    assert tuple(one[0].shape) == (1,) + BIG and np.array_equal(one[0][0].cpu().numpy(), A.decode.seg_regions_host(images[0], None, 4)[0])


def test_binding_errors(A):
    hip = A.hip
    i32 = dict(dtype=torch.int32, device="cuda")
    cm = torch.zeros((2, 20, 30), dtype=torch.uint8, device="cuda")
    ok = dict(class_map=cm, rows=torch.zeros((4, 5), **i32), offsets=torch.zeros(3, **i32), labels=torch.zeros((2, 20, 30), **i32),
              table=torch.zeros((2, 8, 12), **i32), head=torch.zeros((2, 4), **i32), box_regions=torch.zeros((2, 4), **i32),
              ws=torch.empty(hip.seg_regions_workspace_bytes(2, 20, 30), dtype=torch.uint8, device="cuda"))
    hip.seg_regions(**ok)
    assert hip.REGION_WORDS == 12 and hip.FLAG_REGIONS == A.decode.FLAG_REGIONS == A.infer.FLAG_REGIONS == 131072
    assert "vrnet_seg_regions_u8" in hip.EXPORTED and "vrnet_seg_regions_workspace_bytes" in hip.EXPORTED
    assert hip.seg_regions_workspace_bytes(8, 1080, 1920) == 8 * 8 * 1080 * 1920 + 16 * 8 * 1013
    for bad in (dict(class_map=cm.int()), dict(class_map=cm[0]), dict(rows=torch.zeros((4, 4), **i32)), dict(rows=torch.zeros((0, 5), **i32)),
                dict(offsets=torch.zeros(2, **i32)), dict(labels=torch.zeros((2, 20, 30), device="cuda")),
                dict(table=torch.zeros((2, 8, 11), **i32)), dict(table=torch.zeros((2, 4097, 12), **i32)),
                dict(head=torch.zeros((2, 3), **i32)), dict(box_regions=torch.zeros((3, 4), **i32)), dict(ws=ok["ws"][:64]),
                dict(connectivity=6), dict(background=300), dict(min_area=0), dict(det_to_seg=torch.zeros(3, device="cuda")),
                dict(det_to_seg=torch.zeros(300, **i32)), dict(geom=torch.zeros((2, 8), dtype=torch.uint8, device="cuda"))):
        with pytest.raises(RuntimeError, match="seg_regions"):
            hip.seg_regions(**dict(ok, **bad))
    with pytest.raises(RuntimeError, match="seg_regions"):
        hip.seg_regions_workspace_bytes(1, 1 << 16, 1 << 16)


# ---- the pipelines (the setup of tests/test_box_radar.py) -----------------------------------------------------------------
from tests.test_box_radar import B, CAP, S, frames_of, model_of  # noqa: E402

RUN_SIZES = {True: [[(40, 56), (80, 112)], [(40, 56), (80, 112)], [(61, 33), (48, 80)]], False: [[CAP, CAP]] * 3}
REGIONS = dict(connectivity=8, background=-1, min_area=1, max_regions=4096, det_to_seg=(1, 2, 3, 4))


def host_regions(A, pipe, got, sizes, params):
    """decode.seg_regions_host on what a caller reads back: the class map and the draw rows of the run."""
    class_map = got.class_map.cpu().numpy()
    draw, offsets = pipe._draw_rows.cpu().numpy(), pipe._offsets.cpu().numpy()
    return [A.decode.seg_regions_host(class_map[b, :ih, :iw], draw[offsets[b]:offsets[b + 1]], **params)
            for b, (ih, iw) in enumerate(sizes)]


@pytest.mark.parametrize("letterbox", [True, False])
@pytest.mark.parametrize("ragged", [False, True])
def test_frame_pipeline_with_regions(A, ragged, letterbox):
    model = model_of(A)
    kw = dict(batch=B, conf_thres=0.05, nms_thres=0.4, max_candidates=64, ragged=ragged, letterbox_image=letterbox)
    plain = A.FramePipeline(model, CAP, (S, S), **kw)
    stage = A.FramePipeline(model, CAP, (S, S), regions=REGIONS, **kw)
    eager = A.FramePipeline(model, CAP, (S, S), regions=REGIONS, graph=False, **kw)
    assert stage.graph is not None and eager.graph is None and plain.regions is None
    params = A.decode.check_region_params(REGIONS, "test", num_classes=4)
    assert stage.regions == params
    names = ("rows", "kept", "det_counts", "class_map", "seg_counts", "rendered", "flag")
    radar = np.random.RandomState(3).rand(B, 4, S, S).astype(np.float32)
    most = linked = 0
    for k, (seed, sizes) in enumerate(zip((40, 41, 42), RUN_SIZES[ragged])):
        frames = frames_of(seed, sizes, ragged)
        want = plain.run(frames, radar)
        assert want.region_labels is None and want.region_table is None and want.region_head is None and want.box_regions is None
        want = [getattr(want, n).clone() for n in names]
        got = stage.run(frames, radar)
        for n, w in zip(names, want):
            g = getattr(got, n)
            if n == "flag":                                       # the stage may add its own bit, nothing else
                g, w = g & ~A.infer.FLAG_REGIONS, w & ~A.infer.FLAG_REGIONS
            assert g.dtype == w.dtype and torch.equal(g, w), (k, n)
        assert tuple(got.region_labels.shape) == (B,) + CAP and tuple(got.region_table.shape) == (B, 4096, 12)
        assert tuple(got.region_head.shape) == (B, 4) and tuple(got.box_regions.shape) == (B, stage.cap)
        host = host_regions(A, stage, got, sizes, params)
        back = got.regions()
        cap = stage.cap
        flag = 0
        for b, (wl, wt, wh, wb, wf) in enumerate(host):
            ih, iw = sizes[b]
            full = np.zeros(CAP, np.int32)
            full[:ih, :iw] = wl
            assert np.array_equal(got.region_labels[b].cpu().numpy(), full), (k, b)
            assert np.array_equal(words(got.region_table[b]), words(wt)), (k, b)
            assert np.array_equal(got.region_head[b].cpu().numpy(), wh), (k, b)
            assert np.array_equal(got.box_regions[b].cpu().numpy(), np.concatenate([wb, np.zeros(cap - len(wb), np.int32)])), (k, b)
            records, labels, links = back[b]
            assert records.dtype == A.decode.REGION_DTYPE and np.array_equal(words(records), words(wt[:wh[1]]))
            assert np.array_equal(labels, wl) and np.array_equal(links, wb) and len(wb) == int(got.kept[b])
            flag |= wf
            most, linked = max(most, int(wh[0])), linked + int((wb > 0).sum())
        assert int(got.flag.item()) & A.infer.FLAG_REGIONS == flag
        other = eager.run(frames, radar)                          # captured equals graph=False
        for n in ("region_labels", "region_table", "region_head", "box_regions", "class_map"):
            assert torch.equal(getattr(other, n), getattr(got, n)), (k, n)
    assert most >= 2, "the class maps of these runs hold fewer than two regions: they test nothing"
    assert int(got.kept.max()) > 0
    # a run enqueues and returns: no host synchronisation
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        stage.run(frames, radar)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    with pytest.raises(RuntimeError, match="not built with regions"):
        plain.result.regions()


def test_construction_errors_and_eval_pipeline(A):
    model = model_of(A)
    kw = dict(batch=B, max_candidates=64, graph=False)
    for bad in (dict(connectivity=5), dict(max_regions=0), dict(max_regions=5000), dict(min_area=0), dict(background=256),
                dict(det_to_seg=(1, 2, 3)), dict(det_to_seg=(1, 2, 3, 300)), dict(colour=1), 5):
        with pytest.raises(RuntimeError, match="FramePipeline"):
            A.FramePipeline(model, CAP, (S, S), regions=bad, **kw)
    with pytest.raises(TypeError, match="regions"):
        A.evaluate.EvalPipeline(model, CAP, (S, S), ["a", "b", "c", "d"], 9, regions=True, **kw)


def test_predict_dir_writes_the_regions(A, tmp_path):
    from PIL import Image
    model = model_of(A)
    sizes = [(61, 33), (48, 80), (80, 112)]
    stems = ["1234567890.00001", "1234567890.00002", "1234567890.00003"]
    src, radar_root, dst = tmp_path / "in", tmp_path / "radar", tmp_path / "out"
    src.mkdir()
    radar_root.mkdir()
    frames = frames_of(60, sizes, True)
    for stem, frame in zip(stems, frames):
        Image.fromarray(frame).save(src / (stem + ".png"))
        np.savez(radar_root / (stem + ".npz"), np.random.RandomState(1).rand(4, S, S).astype(np.float32))
    pipe = A.FramePipeline(model, CAP, (S, S), batch=2, conf_thres=0.05, nms_thres=0.4, max_candidates=64, graph=False, ragged=True,
                           regions=dict(background=-1))
    out = A.infer.predict_dir(pipe, str(src), str(radar_root), str(dst))
    assert [n for n, _ in out] == [s + ".png" for s in stems]
    texts = [open(os.path.join(dst, s + "_regions.txt")).read() for s in stems]
    assert texts[2] == A.decode.region_text(pipe.result.regions()[0][0])           # the last batch: the third picture, repeated
    for text, (ih, iw) in zip(texts, sizes):
        fields = [line.split() for line in text.splitlines()]
        assert len(fields) >= 1 and all(len(f) == 10 for f in fields) and [int(f[0]) for f in fields] == list(range(1, len(fields) + 1))
        assert sum(int(f[2]) for f in fields) == ih * iw           # background = -1: the regions tile the picture
    Image.fromarray(np.zeros((20, 20, 3), np.uint8)).save(src / (stems[0] + "_regions.png"))
    with pytest.raises(RuntimeError, match="would both be saved"):
        A.infer.predict_dir(pipe, str(src), str(radar_root), str(dst))
