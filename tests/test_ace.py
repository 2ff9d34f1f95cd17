"""ACE de-rain enhancement on the device (csrc/ace.hip: vrnet_ace_u8) against its host statement render.ace_host: every
comparison is np.array_equal on the bytes, the host result computed once per case.  out and the workspace are pre-filled with
garbage before every launch, so nothing read here was left by an earlier call.  Then the surface above the kernels:
render.ace and FramePipeline(ace=...), fixed-size and ragged.

Constant frames: the rule calls an image degenerate when lmax <= lmin, which a constant frame meets where its R_0 is exactly
0.5 -- at sizes whose up-resize fractions are exact in float32, such as 48 x 64, 16 x 16 and 8 x 8, the ones used here.  At
other sizes (40 x 56, 9 x 9) 0.5 * a0 + 0.5 * a1 leaves rounding in the last bits of R_0 and the rule is not degenerate."""
import inspect
import os

import numpy as np
import pytest
import torch

from asy_vrnet_amd import data, decode, render

pytestmark = pytest.mark.gpu


def cuda(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def rainy(seed, h, w):
    return np.random.RandomState(seed).randint(0, 256, (h, w, 3)).astype(np.uint8)


_host = {}


def host(frame, **kw):
    """render.ace_host, computed once per (frame, parameters) of this module."""
    key = (frame.tobytes(), frame.shape, tuple(sorted(kw.items())))
    if key not in _host:
        _host[key] = render.ace_host(frame, **kw)
    return _host[key]


def table_of(sizes):
    tab = np.zeros(len(sizes), data.GEOM_DTYPE)
    tab["ih"], tab["iw"], tab["thickness"] = [s[0] for s in sizes], [s[1] for s in sizes], 1
    return data.geometry_bytes(tab).cuda()


def launch(slots, sizes=None, ws=None, **kw):
    """One hip.ace call on padded slots (B, ihm, iwm, 3) -> (out as numpy, flag)."""
    import asy_vrnet_amd.hip as hip
    B, ihm, iwm = slots.shape[:3]
    frames = cuda(slots)
    out = torch.full_like(frames, 0xAB)
    if ws is None:
        ws = torch.full((hip.ace_workspace_bytes(B, ihm, iwm),), 0xCD, dtype=torch.uint8, device="cuda")
    flag = torch.zeros(1, dtype=torch.int32, device="cuda")
    q = render.ace_params(**kw)
    hip.ace(frames, out, ws, cuda(render.ace_weights(q["radius"])), geom=None if sizes is None else table_of(sizes), flag=flag, **q)
    torch.cuda.synchronize()
    assert torch.equal(frames, cuda(slots))                               # the input is not modified
    return out.cpu().numpy(), int(flag)


def same(got, b, frame, **kw):
    """Image b of a launch against the host statement of `frame`, everything outside its corner being zero."""
    out = got[0]
    ih, iw = frame.shape[:2]
    want, degenerate = host(frame, **kw)
    assert not degenerate
    bad = np.argwhere(out[b, :ih, :iw] != want)
    assert np.array_equal(out[b, :ih, :iw], want), (len(bad), bad[:5])
    assert not out[b, ih:].any() and not out[b, :, iw:].any()


SIZES = [(3, 3), (3, 7), (5, 4), (8, 8), (6, 10), (9, 16), (17, 23), (37, 53), (70, 131)]


@pytest.mark.parametrize("ih,iw", SIZES)
def test_one_image_equals_the_host_statement(ih, iw):
    frame = rainy(ih * 1000 + iw, ih, iw)
    got = launch(frame[None])
    same(got, 0, frame)
    assert got[1] == 0 and (host(frame)[0] != frame).mean() > 0.5         # not vacuous


@pytest.mark.parametrize("kw", [dict(radius=1), dict(radius=8), dict(ratio=2.5), dict(s=0.0), dict(s=0.2), dict(bins=7)],
                         ids=lambda kw: "-".join(f"{k}{v}" for k, v in kw.items()))
def test_other_parameters_than_the_defaults(kw):
    frame = rainy(24, 37, 53)
    got = launch(frame[None], **kw)
    same(got, 0, frame, **kw)
    assert got[1] == 0 and not np.array_equal(host(frame, **kw)[0], host(frame)[0])


def test_two_byte_values_in_vertical_stripes():
    """Every tap difference across a stripe edge saturates the clip, and many pixels share one R value at the histogram's
    last edge (idx == bins)."""
    frame = np.where((np.arange(53) // 3) % 2 == 0, 40, 200).astype(np.uint8)[None, :, None].repeat(37, 0).repeat(3, 2)
    frame = np.ascontiguousarray(frame)
    got = launch(frame[None])
    same(got, 0, frame)
    assert got[1] == 0 and (host(frame)[0] == 255).sum() >= 37 * 3        # a whole column of every channel at the maximum


def test_a_batch_of_three_different_images():
    frames = np.stack([rainy(s, 37, 53) for s in (21, 22, 23)])
    got = launch(frames)
    for b in range(3):
        same(got, b, frames[b])
    assert got[1] == 0 and not np.array_equal(got[0][0], got[0][1])


RAGGED = [(48, 64), (37, 53), (5, 4), (3, 3)]               # four different pyramid depths


def test_ragged_images_equal_the_call_on_each_image_alone():
    images = [rainy(40 + k, *s) for k, s in enumerate(RAGGED)]
    slots = np.random.RandomState(41).randint(0, 256, (4, 48, 64, 3)).astype(np.uint8)    # garbage in the padding
    for b, im in enumerate(images):
        slots[b, :im.shape[0], :im.shape[1]] = im
    got = launch(slots, RAGGED)
    assert got[1] == 0
    for b, im in enumerate(images):
        same(got, b, im)                                                  # the host statement, and zeros outside the corner
        alone = launch(im[None])
        assert np.array_equal(alone[0][0], got[0][b, :im.shape[0], :im.shape[1]])
    out = render.ace(slots, sizes=RAGGED)                                 # render.ace with sizes builds the same table
    assert np.array_equal(out.cpu().numpy(), got[0])
    out = render.ace(images[1])
    assert out.shape == (1, 37, 53, 3) and np.array_equal(out[0].cpu().numpy(), host(images[1])[0])


def test_degenerate_images_and_a_bad_record_inside_a_batch():
    import asy_vrnet_amd.hip as hip
    healthy, last = rainy(51, 48, 64), rainy(52, 48, 64)
    thin = rainy(53, 2, 9)
    slots = np.full((5, 48, 64, 3), 77, np.uint8)                         # image 1: the constant frame
    slots[0], slots[4] = healthy, last
    slots[2, :2, :9] = thin
    slots[3] = rainy(54, 48, 64)
    sizes = [(48, 64), (48, 64), (2, 9), (48, 64), (48, 64)]
    assert host(np.ascontiguousarray(slots[1]))[1] and host(thin)[1]      # the host statement calls them degenerate too
    out, flag = got = launch(slots, sizes)
    assert flag == hip.FLAG_ACE == render.FLAG_ACE == 16384
    for b in (0, 3, 4):
        same(got, b, np.ascontiguousarray(slots[b]))
    assert np.array_equal(out[1], slots[1])                               # unchanged
    assert np.array_equal(out[2, :2, :9], thin) and not out[2, 2:].any() and not out[2, :, 9:].any()
    for size in ((1, 1), (2, 2), (48, 2)):                                # degenerate by their size alone
        out, flag = launch(slots[:1], [size])
        assert flag == hip.FLAG_ACE and np.array_equal(out[0, :size[0], :size[1]], slots[0, :size[0], :size[1]])
        assert not out[0, size[0]:].any() and not out[0, :, size[1]:].any()
    for bad in ((0, 64), (48, 65), (-3, 10)):                             # records that are no image
        sizes[3] = bad
        got = launch(slots, sizes)
        assert got[1] == hip.FLAG_ACE | hip.FLAG_GEOMETRY and not got[0][3].any()
        same(got, 0, healthy)
        same(got, 4, last)
        assert np.array_equal(got[0][1], slots[1])


def test_a_record_above_its_slot_and_an_empty_one():
    """Image 1's record is no image, ih = 25 in a slot of 16 rows as much as ih = 0: a zero image and FLAG_GEOMETRY.  Image 0
    as ever."""
    import asy_vrnet_amd.hip as hip
    slots = np.stack([rainy(61, 16, 24), rainy(62, 16, 24)])
    for ih in (25, 0):
        got = launch(slots, [(11, 17), (ih, 20)])
        assert got[1] == hip.FLAG_GEOMETRY == 256 and not got[0][1].any()
        same(got, 0, np.ascontiguousarray(slots[0, :11, :17]))


def test_no_state_between_calls():
    import asy_vrnet_amd.hip as hip
    one = np.stack([rainy(61, 37, 53), rainy(62, 37, 53)])
    two = np.stack([rainy(63, 37, 53), np.full((37, 53, 3), 9, np.uint8)])
    two[1, :16, :16] = rainy(64, 16, 16)
    ws = torch.full((hip.ace_workspace_bytes(2, 37, 53),), 0xCD, dtype=torch.uint8, device="cuda")
    a1 = launch(one, ws=ws)
    b1 = launch(two, ws=ws)
    a2 = launch(one, ws=ws)
    ws.fill_(0x11)
    b2 = launch(two, ws=ws)
    a3 = launch(one, ws=ws)
    for x, y in ((a1, a2), (a1, a3), (b1, b2)):
        assert np.array_equal(x[0], y[0]) and x[1] == y[1]
    for got, frames in ((a1, one), (b1, two)):
        same(got, 0, frames[0])
        same(got, 1, frames[1])
        assert np.array_equal(launch(frames)[0], got[0])                  # a fresh call
    assert a1[1] == 0 and b1[1] == 0


def test_argument_checks():
    import asy_vrnet_amd.hip as hip
    frames = cuda(rainy(71, 37, 53)[None])
    out = torch.empty_like(frames)
    ws = torch.empty(hip.ace_workspace_bytes(1, 37, 53), dtype=torch.uint8, device="cuda")
    w3, w9 = cuda(render.ace_weights(3)), cuda(np.zeros((19, 19)))
    for kw in (dict(ratio=0.0), dict(ratio=float("inf")), dict(ratio=float("nan")), dict(s=-0.1), dict(s=0.5), dict(bins=1),
               dict(bins=4097)):
        with pytest.raises(RuntimeError, match="ace: (radius|ratio)"):
            hip.ace(frames, out, ws, w3, **kw)
    for radius, w in ((0, cuda(np.zeros((1, 1)))), (9, w9)):
        with pytest.raises(RuntimeError, match="ace: radius"):
            hip.ace(frames, out, ws, w, radius=radius)
    with pytest.raises(RuntimeError, match="expected a contiguous"):
        hip.ace(frames, out, ws, w3, radius=2)                            # a table of another radius
    with pytest.raises(RuntimeError, match="workspace holds"):
        hip.ace(frames, out, ws[:-256], w3)
    with pytest.raises(RuntimeError, match="other than frames"):
        hip.ace(frames, frames, ws, w3)
    with pytest.raises(RuntimeError, match="expected a contiguous"):
        hip.ace(frames, out[:, :30], ws, w3)
    with pytest.raises(RuntimeError, match="bad shape"):
        hip.ace_workspace_bytes(0, 48, 64)
    assert hip.ace_workspace_bytes(2, 48, 64) > 24 * 2 * 48 * 64
    torch.cuda.synchronize()


def test_the_abi_version_stays():
    import asy_vrnet_amd.hip as hip
    assert hip.ABI_VERSION == 11 and hip._lib.vrnet_abi_version() == 11
    assert "vrnet_ace_u8" in hip.EXPORTED and "vrnet_ace_workspace_bytes" in hip.EXPORTED


# ---- the pipeline: the sizes and the threshold of tests/test_infer.py ------------------------------------------------------
NC, S, F, CAP, NMS_THRES = 4, (64, 64), (40, 56), 64, 0.4
RAGGED_CAP, RAGGED_SIZES = (48, 68), [(40, 56), (45, 50)]
DH = dict(sz=5, r=12)


@pytest.fixture(scope="module")
def model():
    import asy_vrnet_amd as A
    net = A.EfficientVRNet(NC, 9, "nano", img_size=S[0]).cuda().eval()
    A.randomize_state_dict(net.state_dict(), seed=4)
    return net


def inputs(seed, sizes):
    rng = np.random.default_rng(seed)
    frames = [rainy(seed + k, *s) for k, s in enumerate(sizes)]
    return frames, (rng.standard_normal((len(sizes), 4) + S) * 2.0 + 1.0).astype(np.float32)


def twelfth_score(model, images, radar):
    """The 12th-largest score of the batch, the threshold tests/test_infer.py uses."""
    with torch.no_grad():
        det, _ = model(images, cuda(radar))
    pred = decode.decode_outputs(det, S)
    return float((pred[..., 4] * pred[..., 5:5 + NC].amax(-1)).flatten().sort(descending=True).values[11])


@pytest.mark.parametrize("kind", ["fixed", "ragged"])
def test_pipeline_with_the_stage_equals_the_pipeline_fed_the_host_frames(kind, model):
    import asy_vrnet_amd as A
    import asy_vrnet_amd.hip as hip
    ragged = kind == "ragged"
    shape, sizes = (RAGGED_CAP, RAGGED_SIZES) if ragged else (F, [F] * 2)
    frames, radar = inputs(80 if ragged else 90, sizes)
    clear = [host(f)[0] for f in frames]
    assert all((c != f).mean() > 0.5 for c, f in zip(clear, frames))
    if ragged:
        slots = np.zeros((2,) + RAGGED_CAP + (3,), np.uint8)
        for b, f in enumerate(clear):
            slots[b, :f.shape[0], :f.shape[1]] = f
        geom = data.geometry_bytes(data.frame_geometry(RAGGED_SIZES, S, True, RAGGED_CAP)).cuda()
        images = torch.empty((2, 3) + S, device="cuda")
        hip.letterbox(cuda(slots), None, S[0], S[1], images=images, geom=geom, max_taps=data.default_max_taps(RAGGED_CAP, S))
    else:
        images = data.device_letterbox(cuda(np.stack(clear)), S)[0]
    kw = dict(batch=2, conf_thres=twelfth_score(model, images, radar), nms_thres=NMS_THRES, max_candidates=CAP, ragged=ragged,
              heatmap=True, crops=True)
    plain = A.FramePipeline(model, shape, S, **kw)
    pipe = A.FramePipeline(model, shape, S, ace=True, **kw)
    assert pipe.graph is not None and plain.ace is None and pipe.ace == render.ace_params()
    feed = (lambda fs: fs) if ragged else np.stack
    res = pipe.run(feed(frames), radar)
    base = plain.run(feed(clear), radar)
    assert base.enhanced is None and res.dehazed is None and int(res.flag) == 0
    for b, c in enumerate(clear):
        got = res.enhanced[b].cpu().numpy()
        assert np.array_equal(got[:c.shape[0], :c.shape[1]], c) and not got[c.shape[0]:].any() and not got[:, c.shape[1]:].any()
    assert max(len(d) for d in res.detections()) >= 2                      # not vacuous
    for k in ("rows", "kept", "det_counts", "rendered", "class_map", "seg_counts", "flag", "heat_mask", "heat_picture", "heat_range"):
        assert torch.equal(getattr(base, k), getattr(res, k)), k
    got, want = res.crops.images(), base.crops.images()
    assert [len(g) for g in got] == [len(w) for w in want] and sum(len(g) for g in got) >= 2
    assert all(np.array_equal(x, y) for g, w in zip(got, want) for x, y in zip(g, w))
    # a replay on other frames follows them
    frames2, radar2 = inputs(85 if ragged else 95, sizes)
    res = pipe.run(feed(frames2), radar2)
    for b, f in enumerate(frames2):
        assert np.array_equal(res.enhanced[b].cpu().numpy()[:f.shape[0], :f.shape[1]], host(f)[0])
    if not ragged:
        with pytest.raises(RuntimeError, match="ace is None, True or a dict"):
            A.FramePipeline(model, F, S, ace=dict(sz=3), graph=False, batch=1)
        with pytest.raises(RuntimeError, match="FramePipeline: radius"):
            A.FramePipeline(model, F, S, ace=dict(radius=9), graph=False, batch=1)


def test_with_dehaze_and_ace_the_stage_reads_the_dehazed_frames(model):
    import asy_vrnet_amd as A
    frames, radar = inputs(110, [F] * 2)
    pipe = A.FramePipeline(model, F, S, batch=2, conf_thres=0.3, nms_thres=NMS_THRES, max_candidates=CAP, dehaze=DH,
                           ace=dict(radius=2), render=False)
    res = pipe.run(np.stack(frames), radar)
    assert pipe.graph is not None
    for b, f in enumerate(frames):
        clear = render.dehaze_host(f, **DH)[0]
        assert np.array_equal(res.dehazed[b].cpu().numpy(), clear)
        assert np.array_equal(res.enhanced[b].cpu().numpy(), host(clear, radius=2)[0])


def test_eval_pipeline_forwards_the_stage(model):
    import asy_vrnet_amd as A
    frames, radar = inputs(120, [F] * 2)
    pipe = A.EvalPipeline(model, F, S, ["boat", "buoy", "pier", "ship"], 9, batch=2, capacity=2, max_boxes=4, max_gt=4, graph=False,
                          ace=dict(radius=2))
    assert pipe.ace == render.ace_params(radius=2) and pipe.dehaze is None
    labels = np.zeros((2,) + F, np.uint8)
    pipe.add(["a", "b"], np.stack(frames), radar, labels, [np.zeros((0, 5), np.int64)] * 2)
    for b, f in enumerate(frames):
        assert np.array_equal(pipe.result.enhanced[b].cpu().numpy(), host(f, radius=2)[0])


def test_without_the_stage_the_chain_issues_the_calls_it_issued_before(model, monkeypatch):
    """Every wrapper of hip.py the chain calls, in order: ace=None never reaches hip.ace, and ace=True adds exactly that one
    call, in front of the letterbox and behind the dehazing."""
    import asy_vrnet_amd as A
    import asy_vrnet_amd.hip as hip
    calls = []
    quiet = ("ptr", "stream", "empty", "tuning_build", "kernel_launches", "last_kernel")
    for name, f in inspect.getmembers(hip, inspect.isfunction):
        if f.__module__ != hip.__name__ or name.startswith("_") or name in quiet or name.endswith("_bytes") or name.endswith("_ok"):
            continue

        def counted(*a, _f=f, _n=name, **k):
            calls.append(_n)
            return _f(*a, **k)
        monkeypatch.setattr(hip, name, counted)
    kw = dict(batch=2, conf_thres=0.3, nms_thres=NMS_THRES, max_candidates=CAP, graph=False)
    pipes = [A.FramePipeline(model, F, S, **kw), A.FramePipeline(model, F, S, ace=True, **kw),
             A.FramePipeline(model, F, S, dehaze=DH, **kw), A.FramePipeline(model, F, S, dehaze=DH, ace=True, **kw)]
    traces = []
    for pipe in pipes:
        del calls[:]
        with torch.no_grad():
            pipe._chain()
        traces.append(list(calls))
    torch.cuda.synchronize()
    without, stage, hazy, both = traces
    assert "ace" not in without and "ace" not in hazy and without.index("letterbox") == 0
    assert stage == ["ace"] + without and hazy == ["dehaze"] + without and both == ["dehaze", "ace"] + without
    tail = [c for c in without if c in ("letterbox", "detect_select", "nms_capped", "detect_finish", "seg_predict", "render")]
    assert tail == ["letterbox", "detect_select", "nms_capped", "detect_finish", "seg_predict", "render"]


def test_predict_dir_saves_the_enhanced_frame_of_every_picture(model, tmp_path):
    import asy_vrnet_amd as A
    from asy_vrnet_amd import infer
    from PIL import Image
    sizes = [(40, 56), (48, 68), (45, 50)]
    frames, radar = inputs(100, sizes)
    src, radar_root, dst = tmp_path / "in", tmp_path / "radar", tmp_path / "out"
    src.mkdir()
    radar_root.mkdir()
    names = [f"{1600000000 + b}.{b:05d}.png" for b in range(3)]
    for b, n in enumerate(names):
        Image.fromarray(frames[b]).save(src / n)
        np.savez(radar_root / (data.frame_id(n) + ".npz"), radar[b])
    pipe = A.FramePipeline(model, RAGGED_CAP, S, batch=2, conf_thres=0.3, nms_thres=NMS_THRES, max_candidates=CAP, ragged=True,
                           graph=False, ace=True)
    out = infer.predict_dir(pipe, str(src), str(radar_root), str(dst))         # batch 2: the last call repeats picture 2
    assert [n for n, _ in out] == names
    assert sorted(os.listdir(dst)) == sorted([n for n in names] + [n[:-4] + "_ace.png" for n in names])
    for n, f in zip(names, frames):
        assert np.array_equal(np.array(Image.open(dst / (n[:-4] + "_ace.png"))), host(f)[0]), n
    Image.fromarray(frames[0]).save(src / (names[0][:-4] + "_ace.png"))         # would be written twice
    with pytest.raises(RuntimeError, match="would both be saved as"):
        infer.predict_dir(pipe, str(src), str(radar_root), str(dst))
