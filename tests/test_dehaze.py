"""Dark-channel dehazing on the device (csrc/dehaze.hip: vrnet_dehaze_u8) against its host statement render.dehaze_host, bit
for bit: the bytes with ==, the transmission and the atmospheric light as bit patterns.  out, transmission and the workspace
are pre-filled with garbage before every launch, so nothing read here was left by an earlier call.  Then the surface above
the kernels: render.dehaze and FramePipeline(dehaze=...), fixed-size and ragged."""
import inspect
import os

import numpy as np
import pytest
import torch

from asy_vrnet_amd import data, decode, render

pytestmark = pytest.mark.gpu


def cuda(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.int64)


def hazy(seed, h, w):
    """A blocky scene blended towards a bright airlight by a depth ramp, plus small noise (tests/test_dehaze_host.py)."""
    rs = np.random.RandomState(seed)
    scene = rs.randint(0, 256, (h // 4 + 1, w // 4 + 1, 3)).repeat(4, 0).repeat(4, 1)[:h, :w].astype(np.float64)
    depth = (0.3 + 0.7 * np.mgrid[0:h, 0:w][0] / h)[..., None]
    return np.clip(scene * depth + 220 * (1 - depth) + rs.randint(-3, 4, (h, w, 3)), 0, 255).astype(np.uint8)


_host = {}


def host(frame, **kw):
    """render.dehaze_host, computed once per (frame, parameters) of this module."""
    key = (frame.tobytes(), frame.shape, tuple(sorted(kw.items())))
    if key not in _host:
        _host[key] = render.dehaze_host(frame, **kw)
    return _host[key]


def table_of(sizes):
    tab = np.zeros(len(sizes), data.GEOM_DTYPE)
    tab["ih"], tab["iw"], tab["thickness"] = [s[0] for s in sizes], [s[1] for s in sizes], 1
    return data.geometry_bytes(tab).cuda()


def launch(slots, sizes=None, ws=None, **kw):
    """One hip.dehaze call on padded slots (B, ihm, iwm, 3) -> (out, t, A (B, 3), degenerate (B), flag) as numpy."""
    import asy_vrnet_amd.hip as hip
    B, ihm, iwm = slots.shape[:3]
    frames = cuda(slots)
    out = torch.full_like(frames, 0xAB)
    t = torch.full((B, ihm, iwm), -7.0, dtype=torch.float64, device="cuda")
    if ws is None:
        ws = torch.full((hip.dehaze_workspace_bytes(B, ihm, iwm),), 0xCD, dtype=torch.uint8, device="cuda")
    flag = torch.zeros(1, dtype=torch.int32, device="cuda")
    hip.dehaze(frames, out, ws, geom=None if sizes is None else table_of(sizes), transmission=t, flag=flag, **kw)
    torch.cuda.synchronize()
    assert torch.equal(frames, cuda(slots))                               # the input is not modified
    rec = ws[:32 * B].view(torch.float64).view(B, 4).cpu().numpy()
    return out.cpu().numpy(), t.cpu().numpy(), rec[:, :3], rec[:, 3], int(flag)


def same(got, b, frame, **kw):
    """Image b of a launch against the host statement of `frame`, everything outside its corner being zero."""
    out, t, A, _, _ = got
    ih, iw = frame.shape[:2]
    want, want_t, want_A = host(frame, **kw)
    assert np.array_equal(bits(A[b]), bits(want_A)), (A[b], want_A)
    bad = np.argwhere(bits(t[b, :ih, :iw]) != bits(want_t))
    assert not len(bad), (len(bad), bad[:5], np.abs(t[b, :ih, :iw] - want_t).max())
    bad = np.argwhere(out[b, :ih, :iw] != want)
    assert not len(bad), (len(bad), bad[:5])
    for plane in (out[b], t[b]):
        assert not plane[ih:].any() and not plane[:, iw:].any()


CASES = [(48, 64, 5, 12), (45, 67, 5, 13), (64, 80, 15, 60), (40, 300, 7, 16), (48, 64, 1, 12), (33, 257, 31, 32), (70, 90, 3, 128)]


@pytest.mark.parametrize("ih,iw,sz,r", CASES)
def test_one_image_equals_the_host_statement(ih, iw, sz, r):
    frame = hazy(ih + iw + sz, ih, iw)
    got = launch(frame[None], sz=sz, r=r)
    same(got, 0, frame, sz=sz, r=r)
    want = host(frame, sz=sz, r=r)[0]
    v_inside = (want > 0) & (want < 255)
    assert got[4] == 0 and got[3][0] == 0.0 and v_inside.mean() > 0.2 and (want != frame).mean() > 0.5     # not vacuous


def test_a_batch_of_three_different_images():
    frames = np.stack([hazy(s, 48, 64) for s in (21, 22, 23)])
    got = launch(frames, sz=5, r=12)
    for b in range(3):
        same(got, b, frames[b], sz=5, r=12)
    assert got[4] == 0 and not np.array_equal(got[0][0], got[0][1])


def test_other_parameters_than_the_defaults():
    frame = hazy(24, 48, 64)
    kw = dict(sz=3, r=7, eps=1e-3, omega=0.8, tx=0.25)
    same(launch(frame[None], **kw), 0, frame, **kw)
    assert (host(frame, **kw)[1] < 0.25).any()                            # tx is in play


def test_ties_across_workgroups_are_decided_by_the_flat_index():
    """The dark channel is one constant over 40 x 300 = 12000 pixels, three chunks of the selection: the 11 taken pixels are
    the last 11 flat indices, whose ranks need the counts of the chunks before them."""
    rs = np.random.RandomState(31)
    frame = rs.randint(100, 256, (40, 300, 3)).astype(np.uint8)
    frame[..., 1] = 100
    got = launch(frame[None], sz=7, r=16)
    same(got, 0, frame, sz=7, r=16)
    S = frame.reshape(-1, 3)[-11:].astype(np.int64).sum(0)
    assert np.array_equal(bits(got[2][0]), bits(S / 255.0 / 12.0)) and got[4] == 0


def test_the_taken_pixels_of_the_threshold_bin_span_a_chunk_boundary():
    """sz = 1, so the dark channel is the frame's own minimum: 20 pixels of value 200 at the flat indices 4085 .. 4104 in a
    sea of 50.  numpx = 12: the last 12 of them are 4093 .. 4104, the first of those is dropped, 4094 .. 4104 are summed --
    two of one chunk of 4096 and nine of the next."""
    rs = np.random.RandomState(32)
    frame = rs.randint(50, 120, (40, 300, 3)).astype(np.uint8)
    frame[..., 2] = 50
    flat = frame.reshape(-1, 3)
    flat[4085:4105] = rs.randint(200, 256, (20, 3))
    flat[4085:4105, 0] = 200
    got = launch(frame[None], sz=1, r=16)
    same(got, 0, frame, sz=1, r=16)
    S = flat[4094:4105].astype(np.int64).sum(0)
    assert np.array_equal(bits(got[2][0]), bits(S / 255.0 / 12.0))


RAGGED = [(64, 80), (48, 64), (45, 67)]


def test_ragged_images_equal_the_call_on_each_image_alone():
    images = [hazy(40 + k, *s) for k, s in enumerate(RAGGED)]
    slots = np.random.RandomState(41).randint(0, 256, (3, 64, 80, 3)).astype(np.uint8)    # garbage in the padding
    for b, im in enumerate(images):
        slots[b, :im.shape[0], :im.shape[1]] = im
    got = launch(slots, RAGGED, sz=5, r=12)
    assert got[4] == 0
    for b, im in enumerate(images):
        same(got, b, im, sz=5, r=12)                                      # the host statement, and zeros outside the corner
        alone = launch(im[None], sz=5, r=12)
        ih, iw = im.shape[:2]
        assert np.array_equal(alone[0][0], got[0][b, :ih, :iw]) and np.array_equal(bits(alone[1][0]), bits(got[1][b, :ih, :iw]))
    # render.dehaze with sizes builds the same table; without transmission=True there is no t
    out, t, A = render.dehaze(slots, sizes=RAGGED, sz=5, r=12, transmission=True)
    assert np.array_equal(out.cpu().numpy(), got[0]) and np.array_equal(bits(t.cpu().numpy()), bits(got[1]))
    assert np.array_equal(bits(A.cpu().numpy()), bits(got[2]))
    out, t, A = render.dehaze(images[1], sz=5, r=12)
    assert t is None and out.shape == (1, 48, 64, 3) and np.array_equal(out[0].cpu().numpy(), host(images[1], sz=5, r=12)[0])


def test_degenerate_images_and_a_bad_record_inside_a_batch():
    import asy_vrnet_amd.hip as hip
    first, last = hazy(51, 48, 64), hazy(52, 48, 64)
    small = hazy(53, 30, 40)                                              # numpx = 1: A = 0
    narrow = hazy(54, 5, 64)                                              # r // 2 = 6 > 5 - 1
    slots = np.full((6, 48, 64, 3), 77, np.uint8)
    slots[0], slots[1], slots[5] = first, 0, last
    slots[2, :30, :40], slots[3, :5, :64] = small, narrow
    sizes = [(48, 64), (48, 64), (30, 40), (5, 64), (48, 64), (48, 64)]
    got = launch(slots, sizes, sz=5, r=12)
    out, t, A, degenerate, flag = got
    assert flag == hip.FLAG_DEHAZE == 8192 and degenerate.tolist() == [0, 1, 1, 1, 0, 0]
    same(got, 0, first, sz=5, r=12)
    same(got, 5, last, sz=5, r=12)
    for b, im in ((1, slots[1]), (2, small), (3, narrow)):
        ih, iw = im.shape[:2]
        assert np.array_equal(out[b, :ih, :iw], im) and (t[b, :ih, :iw] == 1.0).all()          # unchanged, t = 1
        assert not out[b, ih:].any() and not out[b, :, iw:].any() and not t[b, ih:].any() and not t[b, :, iw:].any()
        assert np.array_equal(bits(A[b]), bits(host(np.ascontiguousarray(im), sz=5, r=12)[2]))
    assert (A[1] == 0).all() and (A[2] == 0).all()
    # degenerate by its size alone: 6 x 400 has an atmospheric light, and r // 2 = 6 > 6 - 1
    low = hazy(55, 6, 400)
    out, t, A, degenerate, flag = launch(low[None], sz=5, r=12)
    assert np.array_equal(out[0], low) and (t == 1.0).all() and flag == hip.FLAG_DEHAZE and degenerate.tolist() == [1]
    assert (A[0] > 0).all() and np.array_equal(bits(A[0]), bits(host(low, sz=5, r=12)[2]))
    # records that are no image: empty, and above the slot
    for bad in ((0, 64), (48, 65), (-3, 10)):
        sizes[4] = bad
        got = launch(slots, sizes, sz=5, r=12)
        assert got[4] == hip.FLAG_DEHAZE | hip.FLAG_GEOMETRY and not got[0][4].any() and not got[1][4].any()
        assert got[3].tolist() == [0, 1, 1, 1, 1, 0]
        same(got, 0, first, sz=5, r=12)
        same(got, 5, last, sz=5, r=12)


def test_a_record_above_its_slot_and_an_empty_one():
    """Image 1's record is no image, ih = 25 in a slot of 16 rows as much as ih = 0: a zero image, t = 0, A = 0, the state
    1.0 and FLAG_GEOMETRY.  Image 0 as ever: at 11 x 17 nothing is summed into A, so the rule returns it unchanged (FLAG_DEHAZE)."""
    import asy_vrnet_amd.hip as hip
    slots = np.stack([hazy(61, 16, 24), hazy(62, 16, 24)])
    good = np.ascontiguousarray(slots[0, :11, :17])
    for ih in (25, 0):
        got = launch(slots, [(11, 17), (ih, 20)], sz=5, r=12)
        out, t, A, degenerate, flag = got
        assert flag == hip.FLAG_GEOMETRY | hip.FLAG_DEHAZE and degenerate.tolist() == [1, 1]
        same(got, 0, good, sz=5, r=12)
        assert np.array_equal(out[0, :11, :17], good)
        assert not out[1].any() and not t[1].any() and not bits(A[1]).any()


def test_no_state_between_calls():
    import asy_vrnet_amd.hip as hip
    one = np.stack([hazy(61, 48, 64), hazy(62, 48, 64)])
    two = np.stack([hazy(63, 48, 64), np.zeros((48, 64, 3), np.uint8)])
    ws = torch.full((hip.dehaze_workspace_bytes(2, 48, 64),), 0xCD, dtype=torch.uint8, device="cuda")
    a1 = launch(one, ws=ws, sz=5, r=12)
    b1 = launch(two, ws=ws, sz=5, r=12)
    a2 = launch(one, ws=ws, sz=5, r=12)
    ws.fill_(0x11)
    b2 = launch(two, ws=ws, sz=5, r=12)
    a3 = launch(one, ws=ws, sz=5, r=12)
    for x, y in ((a1, a2), (a1, a3), (b1, b2)):
        assert np.array_equal(x[0], y[0]) and np.array_equal(bits(x[1]), bits(y[1])) and np.array_equal(bits(x[2]), bits(y[2]))
        assert x[4] == y[4]
    same(a1, 0, one[0], sz=5, r=12)
    same(a1, 1, one[1], sz=5, r=12)
    same(b1, 0, two[0], sz=5, r=12)
    assert a1[4] == 0 and b1[4] == hip.FLAG_DEHAZE


def test_argument_checks():
    import asy_vrnet_amd.hip as hip
    frames = cuda(hazy(71, 48, 64)[None])
    out = torch.empty_like(frames)
    ws = torch.empty(hip.dehaze_workspace_bytes(1, 48, 64), dtype=torch.uint8, device="cuda")
    for kw in (dict(sz=4), dict(sz=33), dict(r=1), dict(r=129), dict(eps=0.0), dict(omega=0.0), dict(omega=1.5), dict(tx=0.0),
               dict(tx=2.0), dict(eps=float("nan"))):
        with pytest.raises(RuntimeError, match="dehaze: (sz|eps)"):
            hip.dehaze(frames, out, ws, **kw)
    with pytest.raises(RuntimeError, match="workspace holds"):
        hip.dehaze(frames, out, ws[:-256])
    with pytest.raises(RuntimeError, match="other than frames"):
        hip.dehaze(frames, frames, ws)
    with pytest.raises(RuntimeError, match="expected a contiguous"):
        hip.dehaze(frames, out[:, :40], ws)
    with pytest.raises(RuntimeError, match="bad shape"):
        hip.dehaze_workspace_bytes(0, 48, 64)
    assert hip.dehaze_workspace_bytes(2, 48, 64) > 7 * 8 * 2 * 48 * 64
    torch.cuda.synchronize()


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
    frames = [hazy(seed + k, *s) for k, s in enumerate(sizes)]
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
    clear = [host(f, **DH)[0] for f in frames]
    assert all((c != f).mean() > 0.5 for c, f in zip(clear, frames))
    if ragged:
        slots = np.zeros((2,) + RAGGED_CAP + (3,), np.uint8)
        for b, f in enumerate(clear):
            slots[b, :f.shape[0], :f.shape[1]] = f
        geom = data.geometry_bytes(data.frame_geometry(RAGGED_SIZES, S, True, RAGGED_CAP)).cuda()
        images = torch.empty((2, 3) + S, device="cuda")
        hip.letterbox_ragged(cuda(slots), None, geom, S[0], S[1], data.default_max_taps(RAGGED_CAP, S), images=images)
    else:
        images = data.device_letterbox(cuda(np.stack(clear)), S)[0]
    kw = dict(batch=2, conf_thres=twelfth_score(model, images, radar), nms_thres=NMS_THRES, max_candidates=CAP, ragged=ragged,
              heatmap=True, crops=True)
    plain = A.FramePipeline(model, shape, S, **kw)
    pipe = A.FramePipeline(model, shape, S, dehaze=DH, **kw)
    assert pipe.graph is not None and plain.dehaze is None and pipe.dehaze == render.dehaze_params(**DH)
    feed = (lambda fs: fs) if ragged else np.stack
    res = pipe.run(feed(frames), radar)
    base = plain.run(feed(clear), radar)
    assert base.dehazed is None and int(res.flag) == 0
    for b, c in enumerate(clear):
        got = res.dehazed[b].cpu().numpy()
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
        assert np.array_equal(res.dehazed[b].cpu().numpy()[:f.shape[0], :f.shape[1]], host(f, **DH)[0])
    # a frame too small for the box raises on the host
    if ragged:
        with pytest.raises(RuntimeError, match="image 1: 6 x 50 allows no single reflection"):
            pipe.run([frames[0], frames[1][:6]], radar)
    else:
        with pytest.raises(RuntimeError, match="allow no single reflection"):
            A.FramePipeline(model, F, S, dehaze=dict(r=128), graph=False, **{**kw, "heatmap": False, "crops": None, "batch": 1})
        with pytest.raises(RuntimeError, match="dehaze is None, True or a dict"):
            A.FramePipeline(model, F, S, dehaze=dict(radius=3), graph=False, batch=1)


def test_without_the_stage_the_chain_issues_the_calls_it_issued_before(model, monkeypatch):
    """Every wrapper of hip.py the chain calls, in order: dehaze=None never reaches hip.dehaze, and dehaze={...} adds exactly
    that one call, in front of the letterbox."""
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
    plain = A.FramePipeline(model, F, S, **kw)
    stage = A.FramePipeline(model, F, S, dehaze=DH, **kw)
    del calls[:]
    with torch.no_grad():
        plain._chain()
    without = [c for c in calls]
    del calls[:]
    with torch.no_grad():
        stage._chain()
    torch.cuda.synchronize()
    assert "dehaze" not in without and "letterbox" in without and calls[0] == "dehaze" and calls[1:] == without
    assert without.index("letterbox") == 0
    tail = [c for c in without if c in ("letterbox", "detect_select", "nms_capped", "detect_finish", "seg_predict", "render")]
    assert tail == ["letterbox", "detect_select", "nms_capped", "detect_finish", "seg_predict", "render"]


def test_predict_dir_saves_the_dehazed_frame_of_every_picture(model, tmp_path):
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
                           graph=False, dehaze=DH)
    out = infer.predict_dir(pipe, str(src), str(radar_root), str(dst))         # batch 2: the last call repeats picture 2
    assert [n for n, _ in out] == names
    assert sorted(os.listdir(dst)) == sorted([n for n in names] + [n[:-4] + "_dehaze.png" for n in names])
    for n, f in zip(names, frames):
        assert np.array_equal(np.array(Image.open(dst / (n[:-4] + "_dehaze.png"))), host(f, **DH)[0]), n
    Image.fromarray(frames[0]).save(src / (names[0][:-4] + "_dehaze.png"))      # would be written twice
    with pytest.raises(RuntimeError, match="would both be saved as"):
        infer.predict_dir(pipe, str(src), str(radar_root), str(dst))
