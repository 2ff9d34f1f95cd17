"""render.dehaze_host, the numpy statement of the dark-channel dehazing rule (csrc/dehaze.hip is tested against it), pinned
piece by piece against independent formulations: scipy.ndimage for the two erosions and the odd box, an explicit double loop
for an even box, a literal stable argsort for the atmospheric light, and hand-made values for the gray formula and the
saturating cast.  No GPU."""
import numpy as np
import pytest
from scipy import ndimage as ndi

from asy_vrnet_amd import render


def hazy(seed, h, w):
    """A blocky scene blended towards a bright airlight by a depth ramp, plus small noise."""
    rs = np.random.RandomState(seed)
    scene = rs.randint(0, 256, (h // 4 + 1, w // 4 + 1, 3)).repeat(4, 0).repeat(4, 1)[:h, :w].astype(np.float64)
    depth = (0.3 + 0.7 * np.mgrid[0:h, 0:w][0] / h)[..., None]
    return np.clip(scene * depth + 220 * (1 - depth) + rs.randint(-3, 4, (h, w, 3)), 0, 255).astype(np.uint8)


@pytest.mark.parametrize("sz", [1, 5, 15])
def test_both_erosions_are_scipys_minimum_filter(sz):
    rs = np.random.RandomState(sz)
    a8 = rs.randint(0, 256, (23, 31)).astype(np.uint8)
    want8 = ndi.minimum_filter(a8.astype(np.float64), size=sz, mode="constant", cval=np.inf)
    got8 = render._erode_host(a8, sz, np.uint8(255))
    assert got8.dtype == np.uint8 and np.array_equal(got8, want8)
    a = rs.rand(23, 31)
    assert np.array_equal(render._erode_host(a, sz, np.inf), ndi.minimum_filter(a, size=sz, mode="constant", cval=np.inf))


@pytest.mark.parametrize("r", [3, 13, 61])
def test_the_odd_box_is_scipys_uniform_filter(r):
    p = np.random.RandomState(r).rand(45, 67)
    assert np.abs(render.box_filter_host(p, r) - ndi.uniform_filter(p, r, mode="mirror")).max() < 1e-12


def test_an_even_box_by_an_explicit_double_loop():
    r, o = 8, 4                                        # anchor r // 2: the window of x is x - 4 .. x + 3
    p = np.random.RandomState(8).rand(9, 11)
    ih, iw = p.shape

    def refl(i, n):
        i = abs(i)
        return i if i < n else 2 * (n - 1) - i
    want = np.zeros_like(p)
    for y in range(ih):
        for x in range(iw):
            want[y, x] = sum(p[refl(y - o + j, ih), refl(x - o + k, iw)] for j in range(r) for k in range(r)) / (r * r)
    assert np.abs(render.box_filter_host(p, r) - want).max() < 1e-12
    # the tap order itself: r shifted adds per pass from the leftmost / topmost tap on, exactly
    h = np.zeros_like(p)
    for y in range(ih):
        for x in range(iw):
            s = p[y, refl(x - o, iw)]
            for k in range(1, r):
                s = s + p[y, refl(x - o + k, iw)]
            h[y, x] = s
    v = np.zeros_like(p)
    for y in range(ih):
        for x in range(iw):
            s = h[refl(y - o, ih), x]
            for j in range(1, r):
                s = s + h[refl(y - o + j, ih), x]
            v[y, x] = s / float(r * r)
    assert np.array_equal(render.box_filter_host(p, r), v)
    with pytest.raises(RuntimeError, match="no single reflection"):
        render.box_filter_host(p[:4], r)               # r // 2 = 4 > 4 - 1


def test_the_atmospheric_light_follows_a_literal_stable_argsort():
    rs = np.random.RandomState(3)
    h, w = 50, 120                                     # numpx = 6
    rgb = rs.randint(0, 256, (h, w, 3)).astype(np.uint8)
    dark8 = rs.randint(0, 200, (h, w)).astype(np.uint8)
    dark8[rs.rand(h, w) < 0.3] = 200                   # the threshold bin holds about 1800 equal values
    dark8[7, 9] = dark8[30, 100] = 230                 # two above it
    n, numpx = h * w, h * w // 1000
    order = sorted(range(n), key=lambda i: (int(dark8.reshape(-1)[i]), i))
    taken = order[n - numpx:][1:]
    flat = np.flatnonzero(dark8.reshape(-1) == 200)
    assert sorted(taken) == sorted([7 * w + 9, 30 * w + 100] + flat[-3:].tolist())       # 4 of the bin, the lowest dropped
    S = [sum(int(rgb.reshape(n, 3)[i, c]) for i in taken) for c in range(3)]
    want = np.array([(float(s) / 255.0) / float(numpx) for s in S])
    assert np.array_equal(render.atmospheric_light_host(rgb, dark8), want)
    # through dehaze_host: A is its third result, from the eroded dark channel of the frame itself
    frame = hazy(4, 48, 64)
    dark = ndi.minimum_filter(frame.min(2), size=5, mode="constant", cval=255)
    assert np.array_equal(render.dehaze_host(frame, sz=5, r=12)[2], render.atmospheric_light_host(frame, dark))


def test_the_gray_formula_on_pure_channels():
    v = np.arange(256)
    z = np.zeros(256, np.int64)
    for c, k in enumerate((4899, 9617, 1868)):
        rgb = np.stack([v if i == c else z for i in range(3)], 1).astype(np.uint8)
        assert np.array_equal(render.gray_host(rgb), (k * v + 8192) >> 14)
    assert 4899 + 9617 + 1868 == 1 << 14
    assert render.gray_host(np.full((2, 2, 3), 255, np.uint8)).tolist() == [[255, 255], [255, 255]]
    assert render.gray_host(np.array([[255, 0, 0], [0, 255, 0], [0, 0, 255]], np.uint8)).tolist() == [76, 150, 29]


def test_the_saturating_cast_rounds_half_to_even_and_clips():
    v = np.array([-1e300, -3.0, -0.5, -0.0, 0.5, 1.5, 2.5, 2.5000000000000004, 126.5, 127.5, 254.5, 255.49, 255.5, 300.0, 1e300])
    assert render.saturate_host(v).tolist() == [0, 0, 0, 0, 0, 2, 2, 3, 126, 128, 254, 255, 255, 255, 255]
    assert render.saturate_host(v).dtype == np.uint8


def test_the_whole_rule_against_the_independent_pieces():
    """dehaze_host from scipy's erosions and (odd r) box: t within the summation-order bound, the bytes equal wherever v
    is not within that bound of a rounding boundary."""
    frame = hazy(5, 45, 67)
    sz, r, eps, omega, tx = 5, 13, 1e-4, 0.95, 0.1
    out, t, A = render.dehaze_host(frame, sz=sz, r=r)
    I = frame.astype(np.float64) / 255.0
    te = 1.0 - omega * ndi.minimum_filter((I / A).min(2), size=sz, mode="constant", cval=np.inf)
    g = render.gray_host(frame) / 255.0

    def box(p):
        return ndi.uniform_filter(p, r, mode="mirror")
    mI, mp = box(g), box(te)
    a = (box(g * te) - mI * mp) / (box(g * g) - mI * mI + eps)
    t2 = box(a) * g + box(mp - a * mI)
    assert np.abs(t - t2).max() < 1e-9                 # a's denominator is about eps: 1e-12 / 1e-4 and some room
    v = ((I - A) / np.maximum(t2, tx)[..., None] + A) * 255.0
    sure = np.abs(v - np.floor(v) - 0.5) > 1e-5
    assert sure.mean() > 0.99 and np.array_equal(out[sure], render.saturate_host(v)[sure])
    inside = (v > 0.5) & (v < 254.5)
    assert inside.mean() > 0.3 and (out != frame).mean() > 0.9       # a good part of v is unsaturated, and the frame changed


def test_degenerate_images_come_back_unchanged():
    black = np.zeros((48, 64, 3), np.uint8)
    out, t, A = render.dehaze_host(black, sz=5, r=12)
    assert np.array_equal(out, black) and (t == 1.0).all() and t.shape == (48, 64) and (A == 0.0).all()
    red = black.copy()
    red[..., 0] = 200                                  # A_g = A_b = 0
    out, t, A = render.dehaze_host(red, sz=5, r=12)
    assert np.array_equal(out, red) and (t == 1.0).all() and A[0] > 0 and (A[1:] == 0.0).all()
    small = hazy(6, 30, 40)                            # 1200 pixels: numpx = 1, nothing is summed
    out, t, A = render.dehaze_host(small, sz=5, r=12)
    assert np.array_equal(out, small) and (t == 1.0).all() and (A == 0.0).all()
    narrow = hazy(7, 6, 400)                           # r // 2 = 6 > 6 - 1: no single reflection
    out, t, A = render.dehaze_host(narrow, sz=5, r=12)
    assert np.array_equal(out, narrow) and (t == 1.0).all() and (A > 0.0).all()
    assert render.dehaze_size_ok(7, 400, 12) and not render.dehaze_size_ok(6, 400, 12) and render.dehaze_size_ok(6, 6, 11)


BAD_PARAMS = [dict(sz=4), dict(sz=0), dict(sz=33), dict(sz=5.0), dict(r=1), dict(r=129), dict(r=12.5), dict(eps=0.0),
              dict(eps=float("inf")), dict(eps=float("nan")), dict(omega=0.0), dict(omega=1.5), dict(tx=0.0), dict(tx=1.01),
              dict(tx=float("nan")), dict(eps="x")]


def test_parameter_and_size_errors_come_before_any_device_work(monkeypatch):
    import asy_vrnet_amd.hip as hip

    def device_work(*a, **k):
        raise AssertionError("device work")
    for name in ("dehaze", "dehaze_workspace_bytes", "ptr", "stream"):
        monkeypatch.setattr(hip, name, device_work)
    frames = np.zeros((2, 48, 64, 3), np.uint8)
    for kw in BAD_PARAMS:
        with pytest.raises(RuntimeError, match="sz must be|eps must be|are numbers"):
            render.dehaze_host(frames[0], **kw)
        with pytest.raises(RuntimeError, match="sz must be|eps must be|are numbers"):
            render.dehaze(frames, **kw)
    assert render.dehaze_params() == dict(sz=15, r=60, eps=1e-4, omega=0.95, tx=0.1)
    assert render.dehaze_params(sz=31, r=128, omega=1, tx=1) == dict(sz=31, r=128, eps=1e-4, omega=1.0, tx=1.0)
    with pytest.raises(RuntimeError, match="no single reflection"):
        render.dehaze(frames, r=128)                                   # 64 > 48 - 1
    with pytest.raises(RuntimeError, match="image 1: 6 x 64 allows no single reflection"):
        render.dehaze(frames, sizes=[(48, 64), (6, 64)], sz=5, r=12)
    with pytest.raises(RuntimeError, match="image 0: bad size"):
        render.dehaze(frames, sizes=[(49, 64), (48, 64)], sz=5, r=12)
    with pytest.raises(RuntimeError, match="2 frames|for a batch"):
        render.dehaze(frames, sizes=[(48, 64)], sz=5, r=12)
    with pytest.raises(RuntimeError, match="not both"):
        render.dehaze(frames, sizes=[(48, 64)] * 2, geom=object(), sz=5, r=12)
    with pytest.raises(RuntimeError, match="expected uint8"):
        render.dehaze(frames.astype(np.float32), sz=5, r=12)
    with pytest.raises(RuntimeError, match="expected frames of shape"):
        render.dehaze(np.zeros((2, 48, 64, 4), np.uint8), sz=5, r=12)
    with pytest.raises(RuntimeError, match="expected a uint8 frame"):
        render.dehaze_host(frames, sz=5, r=12)
    assert hip.FLAG_DEHAZE == render.FLAG_DEHAZE == 8192
