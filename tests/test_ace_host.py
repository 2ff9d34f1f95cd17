"""The pieces of render.ace_host, the numpy statement of the ACE rule, pinned independently of each other and without a GPU:
the tap weights against their closed form, the restated bin rule against np.histogram, the restated resize against a block
mean and an independent bilinear evaluation, the degenerate images, determinism and the independence of the channels."""
import math

import numpy as np
import pytest

from asy_vrnet_amd import render


@pytest.mark.parametrize("r", [1, 3, 8])
def test_the_weights_equal_the_closed_form(r):
    m = render.ace_weights(r)
    assert m.shape == (2 * r + 1, 2 * r + 1) and m.dtype == np.float64 and m[r, r] == 0.0
    total = math.fsum(1.0 / math.hypot(dy, dx) for dy in range(-r, r + 1) for dx in range(-r, r + 1) if dy or dx)
    for dy in range(-r, r + 1):
        for dx in range(-r, r + 1):
            if dy or dx:
                assert abs(m[dy + r, dx + r] - 1.0 / math.hypot(dy, dx) / total) < 1e-15
    assert abs(m.sum() - 1.0) < 1e-15
    assert np.array_equal(m, m.T) and np.array_equal(m, m[::-1]) and np.array_equal(m, m[:, ::-1])


def planes(bins):
    """Random planes, planes with many values exactly on edges, a constant plane and a two-valued plane."""
    rs = np.random.RandomState(bins)
    out = [rs.rand(37, 53), rs.standard_normal(4000) * 1e3, rs.rand(64, 64) * 1e-9 - 5.0]
    for x in (rs.rand(500), rs.standard_normal(300)):
        first, last = x.min(), x.max()
        step = (last - first) / bins
        k = rs.randint(0, bins + 1, 3000)
        out.append(np.concatenate([x, first + k * step, k * step + first, np.full(40, last), np.full(40, first)]))
    out += [np.full((9, 9), 0.5), np.full(7, -3.25), np.where(rs.rand(400) < 0.3, 0.25, 0.75), np.array([1.0, 2.0])]
    return out


@pytest.mark.parametrize("bins", [2, 7, 2000, 4096])
def test_the_restated_bin_rule_equals_numpy(bins):
    for x in planes(bins):
        counts, edges = render.ace_bins_host(x, bins)
        want, want_edges = np.histogram(x, bins)
        assert np.array_equal(edges.view(np.int64), want_edges.view(np.int64))
        assert counts.dtype == np.int64 and np.array_equal(counts, want) and counts.sum() == x.size


def test_the_halving_case_is_the_block_mean():
    rs = np.random.RandomState(1)
    for h, w in ((1, 1), (2, 3), (5, 4), (8, 8)):
        S = rs.rand(2 * h, 2 * w)
        got = render.ace_resize_host(S, h, w)
        assert got.shape == (h, w) and np.abs(got - S.reshape(h, 2, w, 2).mean((1, 3))).max() < 1e-15
        assert np.array_equal(got, (((S[0::2, 0::2] + S[0::2, 1::2]) + S[1::2, 0::2]) + S[1::2, 1::2]) * 0.25)


def bilinear(S, h, w):
    """Half-pixel-centre bilinear resize in float64, np.interp per axis (which clamps outside the sample centres)."""
    n, m = S.shape
    xs, ys = (np.arange(w) + 0.5) * (m / w) - 0.5, (np.arange(h) + 0.5) * (n / h) - 0.5
    H = np.stack([np.interp(xs, np.arange(m), row) for row in S])
    return np.stack([np.interp(ys, np.arange(n), col) for col in H.T], 1)


@pytest.mark.parametrize("src,dst", [((5, 4), (3, 2)), ((3, 2), (5, 4)), ((9, 16), (5, 8)), ((2, 2), (3, 3))])
def test_the_two_tap_case_is_half_pixel_centre_bilinear(src, dst):
    S = np.random.RandomState(sum(src)).rand(*src)
    got = render.ace_resize_host(S, *dst)
    assert got.shape == dst and got.dtype == np.float64
    assert np.abs(got - bilinear(S, *dst)).max() < 1e-6               # the weights are float32: the semantics, not the bits
    # a constant stays within 1 ulp of the WEIGHTS' format: a0 = float32(1 - f) misses 1 - f by at most 2^-25, so a0 + a1 misses
    # 1 by as much per axis, and c (a0 + a1)(b0 + b1) misses c by c * 2^-24 = 1.8e-8 at c = 0.3, below spacing(float32(0.3)) =
    # 2^-25 = 3.0e-8.  One float64 ulp cannot hold under the rule's float32 weights (the rule's own "0.5 a0 + 0.5 a1 is not always 0.5")
    const = render.ace_resize_host(np.full(src, 0.3), *dst)
    assert np.abs(const - 0.3).max() <= np.spacing(np.float32(0.3))


def test_the_pyramid_levels():
    assert render.ace_levels(1080, 1920)[-1] == (2, 2) and len(render.ace_levels(1080, 1920)) == 11
    assert render.ace_levels(9, 16) == [(9, 16), (5, 8), (3, 4), (2, 2)] and render.ace_levels(2, 9) == [(2, 9)]


@pytest.mark.parametrize("frame", [np.full((48, 64, 3), 77, np.uint8), np.full((8, 8, 3), 0, np.uint8),
                                   np.random.RandomState(2).randint(0, 256, (2, 9, 3)).astype(np.uint8),
                                   np.full((1, 1, 3), 200, np.uint8)], ids=["constant", "constant8", "2x9", "1x1"])
def test_degenerate_images_come_back_unchanged(frame):
    out, degenerate = render.ace_host(frame)
    assert degenerate is True and np.array_equal(out, frame) and out is not frame


def test_deterministic_and_the_channels_are_independent():
    frame = np.random.RandomState(3).randint(0, 256, (17, 23, 3)).astype(np.uint8)
    out, degenerate = render.ace_host(frame)
    again, _ = render.ace_host(frame.copy())
    assert not degenerate and out.dtype == np.uint8 and out.shape == frame.shape and np.array_equal(out, again)
    assert (out != frame).mean() > 0.5 and out.min() == 0 and out.max() == 255
    perm = [2, 0, 1]
    assert np.array_equal(render.ace_host(np.ascontiguousarray(frame[..., perm]))[0], out[..., perm])
    grey = np.repeat(frame[..., :1], 3, 2)
    g = render.ace_host(grey)[0]
    assert np.array_equal(g[..., 0], out[..., 0]) and np.array_equal(g[..., 1], g[..., 0]) and np.array_equal(g[..., 2], g[..., 0])


def test_argument_checks():
    frame = np.zeros((9, 9, 3), np.uint8)
    for kw in (dict(radius=0), dict(radius=9), dict(radius=2.0), dict(radius=True), dict(bins=1), dict(bins=4097), dict(bins=7.5)):
        with pytest.raises(RuntimeError, match="ace_host: radius must be an integer"):
            render.ace_host(frame, **kw)
    for kw in (dict(ratio=0.0), dict(ratio=-1.0), dict(ratio=float("inf")), dict(ratio=float("nan")), dict(s=-0.01), dict(s=0.5)):
        with pytest.raises(RuntimeError, match="ace_host: ratio must be positive"):
            render.ace_host(frame, **kw)
    with pytest.raises(RuntimeError, match="ratio and s are numbers"):
        render.ace_host(frame, ratio="a")
    for bad in (frame.astype(np.float32), frame[..., 0], frame[..., :2], np.zeros((0, 4, 3), np.uint8)):
        with pytest.raises(RuntimeError, match="expected a uint8 frame"):
            render.ace_host(bad)
    with pytest.raises(RuntimeError, match="ace_weights: radius"):
        render.ace_weights(0)
    with pytest.raises(RuntimeError, match="ace_resize_host: expected a plane"):
        render.ace_resize_host(np.zeros((3, 3)), 0, 2)
    assert render.ace_params() == dict(ratio=4.0, radius=3, s=0.005, bins=2000) and render.FLAG_ACE == 16384
