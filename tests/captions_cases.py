"""What tests/test_captions_host.py and tests/test_captions.py share: the glyph atlas, the tie sweep of the one-decimal
formatting and the seeded caption cases."""
import os

import numpy as np

from asy_vrnet_amd import render

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIXTURE = os.path.join(ROOT, "tests", "golden", "glyph_atlas_builtin.npz")
FIXTURE_SIZES = (1, 8, 10)                       # as tools/make_glyph_atlas_fixture.py
_atlas = {}


def have_pillow():
    try:
        import PIL  # noqa: F401
        return True
    except ImportError:
        return False


def atlas():
    """The glyph atlas of the built-in face at sizes 1, 8 and 10: from Pillow when it imports, otherwise the committed fixture."""
    if "a" not in _atlas:
        _atlas["a"] = render.GlyphAtlas(None, FIXTURE_SIZES) if have_pillow() else render.GlyphAtlas.load(FIXTURE)
    return _atlas["a"]


def tie_sweep():
    """Every float32 within 2 ulps of the tie (2k + 1) / 20 for k in 0 .. 99999: (100000 * 5,) float32, all positive."""
    if "ties" not in _atlas:
        x = ((2.0 * np.arange(100000, dtype=np.float64) + 1.0) / 20.0).astype(np.float32)
        lo1 = np.nextafter(x, np.float32(0))
        hi1 = np.nextafter(x, np.float32(np.inf))
        _atlas["ties"] = np.stack([np.nextafter(lo1, np.float32(0)), lo1, x, hi1, np.nextafter(hi1, np.float32(np.inf))], 1).reshape(-1)
    return _atlas["ties"]


def tenths_text(values, signed=False):
    """The strings `render.fixed_tenths` stands for, for values whose k is below the saturation."""
    k, neg = render.fixed_tenths(values)
    sign = {True: "-", False: "+" if signed else ""}
    return [f"{sign[bool(s)]}{int(v) // 10}.{int(v) % 10}" for v, s in zip(k.reshape(-1).tolist(), neg.reshape(-1).tolist())]


def random_strings(rng, n):
    """n captions as the text kernel composes them, every field combination and a few empty ones."""
    out = []
    for i in range(n):
        fields = []
        if rng.random() < 0.7:
            fields.append(f"#{int(rng.integers(1, 2 ** int(rng.integers(1, 32))))}")
        if rng.random() < 0.7:
            fields.append("{:.1f}m".format(float(rng.random() * 10 ** int(rng.integers(0, 5)))))
            if rng.random() < 0.5:
                fields.append("{:+.1f}m/s".format(float((rng.random() - 0.5) * 10 ** int(rng.integers(0, 4)))))
        out.append(" ".join(fields))
    return out


def random_case(rng, ih, iw, n, n_classes=4):
    """n draw rows whose corners reach over every border of the (ih, iw) image -- the caption hangs on left and bottom, so the
    tags overlap and are clipped on all sides -- and their captions."""
    rows = np.empty((n, 5), np.int32)
    for r in rows:
        left, top = int(rng.integers(-20, iw + 4)), int(rng.integers(-4, ih))
        r[:] = (left, top, left + int(rng.integers(1, iw)), int(rng.integers(top, ih + 6)), rng.integers(-1, n_classes + 1))
    return rows, random_strings(rng, n)


def pack(cases):
    """[(rows, strings)] per image -> packed rows, offsets (B + 1), the (N, 12) caption records."""
    offsets = np.cumsum([0] + [len(r) for r, _ in cases]).astype(np.int32)
    rows = np.concatenate([r for r, _ in cases]) if cases else np.zeros((0, 5), np.int32)
    return rows.astype(np.int32).reshape(-1, 5), offsets, render.caption_records([s for _, s in cases])
