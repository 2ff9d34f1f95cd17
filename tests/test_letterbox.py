"""The device letterbox (csrc/letterbox.hip, data.device_letterbox): an INTEGER numpy restatement of Pillow's 8-bit bicubic
resample (Resample.c ImagingResample: 22-bit fixed-point taps, horizontal pass, rounded and clipped uint8 image, vertical
pass) and of its nearest resize (Geometry.c ImagingScaleAffine: a running double sum per axis), pinned byte for byte on the
reference's own letterboxes (tests/golden/letterbox_small.npz, tools/make_golden_letterbox.py) and, where Pillow is
installed, on Pillow itself at full size; then the HIP path against the goldens and the restatement.  Every comparison is
exact: no tolerance appears in this file."""
import os

import numpy as np
import pytest
import torch

from asy_vrnet_amd import data

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "letterbox_small.npz")
PRECISION_BITS = 32 - 8 - 2


# ---- the restatement ------------------------------------------------------------------------------------------------

def bicubic(x):
    a = -0.5
    x = abs(x)
    if x < 1.0:
        return ((a + 2.0) * x - (a + 3.0)) * x * x + 1
    if x < 2.0:
        return (((x - 5) * x + 8) * x - 4) * a
    return 0.0


def bicubic_table(n_in, n_out):
    """[(xmin, integer taps)] per output index of an axis resized n_in -> n_out (Python floats are IEEE doubles, one
    rounding per operation; int() truncates towards zero as the C cast does)."""
    scale = n_in / n_out
    fs = max(scale, 1.0)
    support, ss = 2.0 * fs, 1.0 / fs
    table = []
    for xx in range(n_out):
        center = (xx + 0.5) * scale
        xmin = max(int(center - support + 0.5), 0)
        xmax = min(int(center + support + 0.5), n_in)
        w = [bicubic((x + xmin - center + 0.5) * ss) for x in range(xmax - xmin)]
        ww = 0.0
        for v in w:
            ww += v
        if ww != 0.0:
            w = [v / ww for v in w]
        k = [int(v * (1 << PRECISION_BITS) + 0.5) if v >= 0 else int(v * (1 << PRECISION_BITS) - 0.5) for v in w]
        table.append((xmin, np.array(k, np.int64)))
    return table


def resample_axis(img, axis, n_out, raw=None):
    """One pass over `axis` of a uint8 array: out = clamp((2^21 + sum k * in) >> 22, 0, 255).  The sums are formed in int64
    and checked to fit Pillow's (and the kernel's) int32 accumulator.  raw (a list), if given, receives the unclamped values."""
    img = np.moveaxis(img, axis, 0)
    out = np.empty((n_out,) + img.shape[1:], np.int64)
    for xx, (xmin, k) in enumerate(bicubic_table(img.shape[0], n_out)):
        assert (1 << (PRECISION_BITS - 1)) + 255 * int(np.abs(k).sum()) < 2 ** 31        # the int32 accumulator's bound
        out[xx] = (1 << (PRECISION_BITS - 1)) + np.tensordot(k, img[xmin:xmin + len(k)].astype(np.int64), axes=1)
    out >>= PRECISION_BITS
    if raw is not None:
        raw.append(out.copy())
    return np.moveaxis(np.clip(out, 0, 255).astype(np.uint8), 0, axis)


def resize_bicubic(img, nh, nw, raw=None):
    """(..., ih, iw, 3) uint8 -> (..., nh, nw, 3): horizontal pass first; a pass whose axis keeps its size is skipped."""
    if img.shape[-2] != nw:
        img = resample_axis(img, img.ndim - 2, nw, raw)
    if img.shape[-3] != nh:
        img = resample_axis(img, img.ndim - 3, nh, raw)
    return img


def nearest_indices(n_in, n_out):
    a0 = n_in / n_out
    xo = a0 * 0.5
    idx = []
    for _ in range(n_out):
        idx.append(int(xo))
        xo += a0                          # a running sum, not x * a0
    return np.array(idx)


def resize_nearest(lab, nh, nw):
    """(..., ih, iw) -> (..., nh, nw); an index past the source leaves 0, as ImagingScaleAffine leaves such pixels unset."""
    ih, iw = lab.shape[-2:]
    yi, xi = nearest_indices(ih, nh), nearest_indices(iw, nw)
    out = lab[..., np.minimum(yi, ih - 1)[:, None], np.minimum(xi, iw - 1)[None, :]].copy()
    out[..., yi >= ih, :] = 0
    out[..., :, xi >= iw] = 0
    return out


def geometry(ih, iw, H, W, letterbox_image=True):
    if not letterbox_image:
        return W, H, 0, 0
    scale = min(W / iw, H / ih)
    nw, nh = int(iw * scale), int(ih * scale)
    return nw, nh, (W - nw) // 2, (H - nh) // 2


def letterbox_restated(img, lab, H, W, letterbox_image=True, raw=None):
    """(canvas (..., H, W, 3), label canvas (..., H, W) or None, (nw, nh))."""
    ih, iw = img.shape[-3:-1]
    nw, nh, dx, dy = geometry(ih, iw, H, W, letterbox_image)
    canvas = np.full(img.shape[:-3] + (H, W, 3), 128, np.uint8)
    canvas[..., dy:dy + nh, dx:dx + nw, :] = resize_bicubic(img, nh, nw, raw)
    lab_canvas = None
    if lab is not None:
        lab_canvas = np.zeros(lab.shape[:-2] + (H, W), np.uint8)
        lab_canvas[..., dy:dy + nh, dx:dx + nw] = resize_nearest(lab, nh, nw)
    return canvas, lab_canvas, (nw, nh)


def normalise_restated(canvas):
    """preprocess_input (utils_seg/utils.py:43-47) on a float64 copy, HWC -> CHW, float32."""
    v = canvas.astype(np.float64)
    v /= 255.0
    v -= data.MEAN
    v /= data.STD
    return np.moveaxis(v, -1, -3).astype(np.float32)


def frames(rng, B, ih, iw):
    """Seeded frames with content that exercises the clamp: noise, plus 0 / 255 blocks in one corner."""
    img = rng.integers(0, 256, (B, ih, iw, 3), dtype=np.uint8)
    bh, bw = max(ih // 4, 1), max(iw // 4, 1)
    blocks = rng.integers(0, 2, (B, (bh + 2) // 3, (bw + 2) // 3, 3), dtype=np.uint8) * 255
    img[:, :bh, :bw] = np.repeat(np.repeat(blocks, 3, axis=1), 3, axis=2)[:, :bh, :bw]
    lab = rng.integers(0, 256, (B, ih, iw), dtype=np.uint8)
    return img, lab


# ---- the restatement pinned on the reference's letterboxes and on Pillow ---------------------------------------------

@pytest.fixture(scope="module")
def golden():
    return np.load(GOLDEN)


def golden_cases(g):
    for name in g["names"]:
        name = str(name)
        H, W, lb, nw, nh, seg_same = (int(v) for v in g[name + "_meta"])
        yield name, g[name + "_src"], g[name + "_label"], (H, W), bool(lb), (nw, nh), bool(seg_same)


def test_golden_covers_the_required_cases(golden):
    seen = {}
    for name, src, lab, (H, W), lb, (nw, nh), seg_same in golden_cases(golden):
        ih, iw = src.shape[:2]
        seen[name] = (ih, iw, H, W, lb, nw, nh)
        assert lab.shape == (ih, iw) and lab.max() == 255
        assert seg_same == lb                                   # utils_seg's resize_image gave utils' canvas wherever it applies
    assert len(seen) >= 12
    by = lambda pred: [n for n, c in seen.items() if pred(*c)]
    assert by(lambda ih, iw, H, W, lb, nw, nh: lb and iw * 9 == ih * 16 and H == W and nw < iw)          # 16:9 down, square
    assert by(lambda ih, iw, H, W, lb, nw, nh: lb and iw * 9 == ih * 16 and (H, W) == (128, 192))        # 16:9, rectangular
    assert by(lambda ih, iw, H, W, lb, nw, nh: lb and nw < W and nh == H)                                # bars left and right
    assert by(lambda ih, iw, H, W, lb, nw, nh: lb and nw > iw and nh > ih)                               # up-scale
    assert by(lambda ih, iw, H, W, lb, nw, nh: (ih, iw) == (nh, nw) == (H, W))                           # identity
    assert by(lambda ih, iw, H, W, lb, nw, nh: lb and (ih, iw) == (nh, nw) and nh < H)                   # bars, no resize
    assert by(lambda ih, iw, H, W, lb, nw, nh: not lb and iw == W and ih != H)                           # vertical pass only
    assert by(lambda ih, iw, H, W, lb, nw, nh: lb and ((H - nh) % 2 == 1 or (W - nw) % 2 == 1))          # odd bar split
    assert by(lambda ih, iw, H, W, lb, nw, nh: not lb and iw != W and ih != H)                           # stretch
    assert by(lambda ih, iw, H, W, lb, nw, nh: iw >= 16 * nw and len(bicubic_table(iw, nw)[nw // 2][1]) >= 64)
    assert by(lambda ih, iw, H, W, lb, nw, nh: nw == iw and nh != ih)                                    # exactly one axis


def test_restatement_reproduces_every_golden_case(golden):
    for name, src, lab, (H, W), lb, nwnh, _ in golden_cases(golden):
        canvas, lab_canvas, got_nwnh = letterbox_restated(src, lab, H, W, lb)
        print(f"{name}: window {got_nwnh[1]} x {got_nwnh[0]}, "
              f"{int((canvas != golden[name + '_canvas']).sum())} image bytes and "
              f"{int((lab_canvas != golden[name + '_label_canvas']).sum())} label bytes differ")
        assert got_nwnh == nwnh
        assert np.array_equal(canvas, golden[name + "_canvas"])
        assert np.array_equal(lab_canvas, golden[name + "_label_canvas"])
        assert data.letterbox_geometry(src.shape[1], src.shape[0], W, H)[:2] == nwnh or not lb


def test_checker_cases_hit_both_ends_of_the_clamp(golden):
    for name in ("checker_down", "checker_up"):
        H, W, lb = (int(v) for v in golden[name + "_meta"][:3])
        raw = []
        letterbox_restated(golden[name + "_src"], None, H, W, bool(lb), raw)
        assert len(raw) == 2
        for r in raw:
            assert r.min() < 0 and r.max() > 255
        assert (golden[name + "_canvas"] == 0).any() and (golden[name + "_canvas"] == 255).any()


def test_restated_tap_counts_and_nearest_recurrence():
    assert 75 <= max(len(k) for _, k in bicubic_table(300, 16)) <= 77          # ksize = ceil(37.5) * 2 + 1 = 77 slots per index
    assert 15 <= max(len(k) for _, k in bicubic_table(1920, 512)) <= 17 and max(len(k) for _, k in bicubic_table(5, 45)) <= 5
    for _, k in bicubic_table(1080, 288):
        assert abs(int(k.sum()) - (1 << PRECISION_BITS)) <= len(k)
    assert np.array_equal(nearest_indices(7, 7), np.arange(7))
    assert np.array_equal(nearest_indices(4, 8), [0, 0, 1, 1, 2, 2, 3, 3])
    assert nearest_indices(1080, 288).max() < 1080 and nearest_indices(5, 45).max() == 4


@pytest.mark.parametrize("ih,iw,size", [(1080, 1920, 512), (480, 640, 512)])
def test_restatement_equals_pillow_at_full_size(ih, iw, size):
    Image = pytest.importorskip("PIL.Image")
    rng = np.random.default_rng(ih + size)
    img, lab = frames(rng, 1, ih, iw)
    canvas, lab_canvas, (nw, nh) = letterbox_restated(img[0], lab[0], size, size)
    new_image, new_label = data.letterbox_sample(Image.fromarray(img[0]), Image.fromarray(lab[0]), np.zeros((0, 5)), (size, size))[::2]
    print(f"{ih} x {iw} -> {size}: window {nh} x {nw}; {int((canvas != np.array(new_image)).sum())} image bytes, "
          f"{int((lab_canvas != np.array(new_label)).sum())} label bytes differ from Pillow")
    assert np.array_equal(canvas, np.array(new_image))
    assert np.array_equal(lab_canvas, np.array(new_label))
    boxed, nw2, nh2 = data.resize_image(Image.fromarray(img[0]), (size, size))
    assert (nw2, nh2) == (nw, nh) and np.array_equal(canvas, np.array(boxed))


# ---- the host interface: what needs no GPU ---------------------------------------------------------------------------

def test_exports():
    import asy_vrnet_amd.hip as hip
    assert {"vrnet_letterbox_workspace", "vrnet_letterbox_u8"} <= set(hip.EXPORTED)
    tables = 4 * (512 * (2 + 17 + 1) + 288 * (2 + 17 + 1))
    assert hip.letterbox_workspace_bytes(8, 1080, 1920, 288, 512) >= tables + 8 * 1080 * 512 * 3
    assert 0 < hip.letterbox_workspace_bytes(8, 288, 512, 288, 512) <= tables                    # no pass: no intermediate
    import asy_vrnet_amd.ops  # noqa: F401
    assert hasattr(torch.ops.vrnet, "letterbox")


def test_device_letterbox_argument_errors():
    img = np.zeros((2, 20, 30, 3), np.uint8)
    with pytest.raises(RuntimeError, match="uint8"):
        data.device_letterbox(img.astype(np.float32), (64, 64))
    with pytest.raises(RuntimeError, match="uint8"):
        data.device_letterbox(img, (64, 64), labels_u8=np.zeros((2, 20, 30), np.int64))
    with pytest.raises(RuntimeError, match="labels"):
        data.device_letterbox(img, (64, 64), labels_u8=np.zeros((2, 20, 31), np.uint8))
    with pytest.raises(RuntimeError, match="labels"):
        data.device_letterbox(img, (64, 64), labels_u8=np.zeros((1, 20, 30), np.uint8))
    with pytest.raises(RuntimeError, match="empty window"):
        data.device_letterbox(np.zeros((1, 1, 1000, 3), np.uint8), (64, 64))            # nh = int(1 * 0.064) = 0
    with pytest.raises(RuntimeError, match="empty window"):
        data.device_letterbox(torch.zeros(2, 1000, 3, 3, dtype=torch.uint8), (64, 64))
    with pytest.raises(RuntimeError, match="shape"):
        data.device_letterbox(np.zeros((2, 20, 30, 4), np.uint8), (64, 64))


def test_fake_kernel_gives_the_output_shapes():
    import asy_vrnet_amd.ops  # noqa: F401
    from torch._subclasses.fake_tensor import FakeTensorMode
    with FakeTensorMode():
        img = torch.empty((3, 40, 70, 3), dtype=torch.uint8)
        lab = torch.empty((3, 40, 70), dtype=torch.uint8)
        images, labels = torch.ops.vrnet.letterbox(img, lab, 64, 96, True)
    assert tuple(images.shape) == (3, 3, 64, 96) and images.dtype == torch.float32
    assert tuple(labels.shape) == (3, 64, 96) and labels.dtype == torch.uint8


# ---- the HIP path against the goldens and the restatement ------------------------------------------------------------

def check_device(img, lab, H, W, letterbox_image=True, want=None):
    """device_letterbox of (B, ih, iw, 3) frames (+ labels) in both output forms against `want` (default: the restatement):
    canvas, label and normalised image, each with array_equal; the normalised image also against device_batch(canvas)."""
    if want is None:
        want = letterbox_restated(img, lab, H, W, letterbox_image)[:2]
    src = torch.from_numpy(img).cuda()
    before = src.clone()
    canvas, labels = data.device_letterbox(src, (H, W), lab, letterbox_image, normalise=False)
    images, labels2 = data.device_letterbox(img, (H, W), None if lab is None else torch.from_numpy(lab), letterbox_image)
    assert torch.equal(src, before), "the frames were modified"
    B = img.shape[0]
    assert canvas.is_cuda and canvas.dtype == torch.uint8 and tuple(canvas.shape) == (B, H, W, 3)
    assert images.is_cuda and images.dtype == torch.float32 and tuple(images.shape) == (B, 3, H, W)
    bad = int((canvas.cpu().numpy() != want[0]).sum())
    print(f"device_letterbox {img.shape} -> {(H, W)} letterbox_image={letterbox_image}: {bad} canvas bytes differ")
    assert np.array_equal(canvas.cpu().numpy(), want[0])
    if lab is not None:
        assert labels.dtype == torch.uint8 and tuple(labels.shape) == (B, H, W)
        assert np.array_equal(labels.cpu().numpy(), want[1]) and torch.equal(labels, labels2)
    else:
        assert labels is None and labels2 is None
    assert torch.equal(images, data.device_batch(canvas, None, 9)[0])
    assert np.array_equal(images.cpu().numpy(), normalise_restated(want[0]))
    return canvas, images, labels


@pytest.mark.gpu
def test_device_letterbox_equals_the_goldens(golden):
    for name, src, lab, (H, W), lb, _, _ in golden_cases(golden):
        print(name)
        check_device(src[None], lab[None], H, W, lb, want=(golden[name + "_canvas"][None], golden[name + "_label_canvas"][None]))
    # a single (ih, iw, 3) frame counts as B = 1
    name = "odd_bar_split"
    H, W = (int(v) for v in golden[name + "_meta"][:2])
    canvas, labels = data.device_letterbox(golden[name + "_src"], (H, W), golden[name + "_label"], normalise=False)
    assert np.array_equal(canvas.cpu().numpy()[0], golden[name + "_canvas"]) and tuple(labels.shape) == (1, H, W)


FULL_SIZE_CASES = [  # (B, (ih, iw), (H, W), letterbox_image)
    (8, (1080, 1920), (512, 512), True), (1, (1080, 1920), (512, 512), True),
    (8, (1080, 1920), (1024, 1024), True), (1, (1080, 1920), (1024, 1024), True),
    (8, (480, 640), (512, 512), True), (1, (480, 640), (512, 512), True),
    (2, (2160, 3840), (512, 512), True), (3, (60, 100), (512, 512), True), (3, (360, 640), (128, 192), True),
    (2, (1080, 1920), (384, 640), False), (2, (300, 200), (16, 16), True), (1, (5, 7), (64, 64), True),
]


@pytest.mark.gpu
@pytest.mark.parametrize("B,image_shape,input_shape,letterbox_image", FULL_SIZE_CASES)
def test_device_letterbox_equals_the_restatement(B, image_shape, input_shape, letterbox_image):
    rng = np.random.default_rng(B * 100000 + image_shape[0] * 10 + input_shape[0])
    img, lab = frames(rng, B, *image_shape)
    check_device(img, lab, *input_shape, letterbox_image)


@pytest.mark.gpu
def test_each_output_alone_and_a_dirty_workspace():
    import asy_vrnet_amd.hip as hip
    rng = np.random.default_rng(21)
    big, big_lab = frames(rng, 2, 360, 640)
    small, small_lab = frames(rng, 2, 90, 50)
    ws = torch.full((max(hip.letterbox_workspace_bytes(2, 360, 640, 72, 128), hip.letterbox_workspace_bytes(2, 90, 50, 128, 71)),),
                    0xFF, dtype=torch.uint8, device="cuda")
    for img, lab, (H, W) in ((big, big_lab, (128, 128)), (small, small_lab, (128, 128)), (big, big_lab, (128, 128))):
        want_canvas, want_label, (nw, nh) = letterbox_restated(img, lab, H, W)
        nw2, nh2, dx, dy = data.letterbox_geometry(img.shape[2], img.shape[1], W, H)
        assert (nw2, nh2) == (nw, nh)
        ig, lg = torch.from_numpy(img).cuda(), torch.from_numpy(lab).cuda()
        B = img.shape[0]
        new = lambda *s, dtype=torch.uint8: torch.full(s, 77, dtype=dtype, device="cuda")
        canvas, images, label = new(B, H, W, 3), new(B, 3, H, W, dtype=torch.float32), new(B, H, W)
        hip.letterbox(ig, lg, H, W, nw, nh, dx, dy, canvas=canvas, images=images, label_out=label, ws=ws)   # the workspace of
        assert np.array_equal(canvas.cpu().numpy(), want_canvas)                                             # the call before
        assert np.array_equal(label.cpu().numpy(), want_label)
        assert np.array_equal(images.cpu().numpy(), normalise_restated(want_canvas))
        c1, i1, l1 = new(B, H, W, 3), new(B, 3, H, W, dtype=torch.float32), new(B, H, W)
        hip.letterbox(ig, None, H, W, nw, nh, dx, dy, canvas=c1, ws=ws)
        hip.letterbox(ig, None, H, W, nw, nh, dx, dy, images=i1, ws=ws)
        hip.letterbox(None, lg, H, W, nw, nh, dx, dy, label_out=l1, ws=ws)
        assert torch.equal(c1, canvas) and torch.equal(i1, images) and torch.equal(l1, label)
        l2 = new(B, H, W)
        hip.letterbox(ig, lg, H, W, nw, nh, dx, dy, label_out=l2)                # the scratch arena instead of `ws`
        assert torch.equal(l2, label)


@pytest.mark.gpu
@pytest.mark.parametrize("ih,iw", [(37, 53), (150, 70), (64, 53)])   # both passes up-scale, both down-scale, neither runs
def test_the_workspace_is_all_the_call_writes(ih, iw):
    """A workspace of exactly letterbox_workspace_bytes, carved from the front of a larger 0xA5 tensor: the bytes behind it
    stay 0xA5 (the tables and the horizontal result of the kernels fit the size the library reports) and the outputs
    equal the restatement."""
    import asy_vrnet_amd.hip as hip
    B, H, W = 3, 64, 96
    img, lab = frames(np.random.default_rng(ih * 1000 + iw), B, ih, iw)
    want_canvas, want_label, (nw, nh) = letterbox_restated(img, lab, H, W)
    nw2, nh2, dx, dy = data.letterbox_geometry(iw, ih, W, H)
    assert (nw2, nh2) == (nw, nh) and ((nw, nh) == (iw, ih)) == ((ih, iw) == (64, 53))
    need = hip.letterbox_workspace_bytes(B, ih, iw, nh, nw)
    big = torch.full((need + (1 << 20),), 0xA5, dtype=torch.uint8, device="cuda")
    new = lambda *s, dtype=torch.uint8: torch.full(s, 77, dtype=dtype, device="cuda")
    canvas, images, label = new(B, H, W, 3), new(B, 3, H, W, dtype=torch.float32), new(B, H, W)
    hip.letterbox(torch.from_numpy(img).cuda(), torch.from_numpy(lab).cuda(), H, W, nw, nh, dx, dy, canvas=canvas, images=images,
                  label_out=label, ws=big[:need])
    touched = int((big[need:] != 0xA5).sum())
    print(f"letterbox {ih} x {iw} -> window {nh} x {nw}: workspace {need} bytes, {touched} bytes behind it written")
    assert touched == 0
    assert np.array_equal(canvas.cpu().numpy(), want_canvas)
    assert np.array_equal(label.cpu().numpy(), want_label)
    assert np.array_equal(images.cpu().numpy(), normalise_restated(want_canvas))


@pytest.mark.gpu
def test_letterbox_in_a_captured_graph():
    rng = np.random.default_rng(22)
    first, first_lab = frames(rng, 2, 270, 480)
    second, second_lab = frames(rng, 2, 270, 480)
    src, lab = torch.from_numpy(first).cuda(), torch.from_numpy(first_lab).cuda()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        data.device_letterbox(src, (128, 128), lab)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        images, labels = data.device_letterbox(src, (128, 128), lab)
    src.copy_(torch.from_numpy(second))
    lab.copy_(torch.from_numpy(second_lab))
    g.replay()
    torch.cuda.synchronize()
    want_canvas, want_label, _ = letterbox_restated(second, second_lab, 128, 128)
    assert np.array_equal(images.cpu().numpy(), normalise_restated(want_canvas))
    assert np.array_equal(labels.cpu().numpy(), want_label)
    assert not np.array_equal(want_canvas, letterbox_restated(first, first_lab, 128, 128)[0])


@pytest.mark.gpu
def test_letterbox_does_not_sync_and_op_matches():
    import asy_vrnet_amd.ops  # noqa: F401
    rng = np.random.default_rng(23)
    img, lab = frames(rng, 2, 270, 480)
    src, lg = torch.from_numpy(img).cuda(), torch.from_numpy(lab).cuda()
    data.device_letterbox(src, (128, 192), lg)
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        images, labels = data.device_letterbox(src, (128, 192), lg)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    oi, ol = torch.ops.vrnet.letterbox(src, lg, 128, 192, True)
    assert torch.equal(oi, images) and torch.equal(ol, labels)
    want_canvas, want_label, _ = letterbox_restated(img, lab, 128, 192)
    assert np.array_equal(images.cpu().numpy(), normalise_restated(want_canvas))
    assert np.array_equal(labels.cpu().numpy(), want_label)


@pytest.mark.gpu
def test_error_cases_on_the_device():
    import asy_vrnet_amd.hip as hip
    test_device_letterbox_argument_errors()
    img = torch.zeros(1, 20, 30, 3, dtype=torch.uint8, device="cuda")
    lab = torch.zeros(1, 20, 30, dtype=torch.uint8, device="cuda")
    canvas = torch.zeros(1, 64, 64, 3, dtype=torch.uint8, device="cuda")
    label = torch.zeros(1, 64, 64, dtype=torch.uint8, device="cuda")
    with pytest.raises(RuntimeError, match="no output"):
        hip.letterbox(img, lab, 64, 64, 64, 42, 0, 11)
    with pytest.raises(RuntimeError, match="window"):
        hip.letterbox(img, None, 64, 64, 65, 42, 0, 11, canvas=canvas)
    with pytest.raises(RuntimeError, match="window"):
        hip.letterbox(img, None, 64, 64, 64, 0, 0, 11, canvas=canvas)
    with pytest.raises(RuntimeError, match="inside"):
        hip.letterbox(img, None, 64, 64, 64, 42, 0, 23, canvas=canvas)
    with pytest.raises(RuntimeError, match="label"):
        hip.letterbox(img, None, 64, 64, 64, 42, 0, 11, label_out=label)
    with pytest.raises(RuntimeError, match="workspace"):
        hip.letterbox(img, None, 64, 64, 64, 42, 0, 11, canvas=canvas, ws=torch.zeros(64, dtype=torch.uint8, device="cuda"))
    with pytest.raises(RuntimeError, match="GPU tensor"):
        hip.letterbox(img.cpu(), None, 64, 64, 64, 42, 0, 11, canvas=canvas)
    with pytest.raises(RuntimeError, match="shape"):
        hip.letterbox(img, None, 64, 64, 64, 42, 0, 11, canvas=canvas[:, :32].contiguous())
