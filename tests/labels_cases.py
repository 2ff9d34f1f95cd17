"""What tests/test_labels_host.py and tests/test_labels.py share: the class names, the atlas and the seeded box cases."""
import os

import numpy as np

from asy_vrnet_amd import render

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLASS_NAMES = ("tv/monitor", "Wy", "a", "boat")     # as tools/make_label_atlas_fixture.py
FIXTURE = os.path.join(ROOT, "tests", "golden", "label_atlas_builtin.npz")
FIXTURE_SIZES = (1, 8, 10)
_atlas = {}


def have_pillow():
    try:
        import PIL  # noqa: F401
        return True
    except ImportError:
        return False


def atlas():
    """The atlas of the built-in face at sizes 1, 8 and 10: from Pillow when it imports, otherwise the committed fixture."""
    if "a" not in _atlas:
        _atlas["a"] = render.LabelAtlas(CLASS_NAMES, None, FIXTURE_SIZES) if have_pillow() else render.LabelAtlas.load(FIXTURE)
    return _atlas["a"]


def random_case(rng, ih, iw, n, thickness, n_classes=len(CLASS_NAMES)):
    """n rows as `render.box_rows` gives them (corners inside [0, iw] x [0, ih]) with right - left >= 2 thickness and
    bottom - top >= 2 thickness -- a condition on the inputs that keeps Pillow's one-row rings and x1 < x0 out -- and float32
    scores obj * class_conf."""
    rows = np.empty((n, 5), np.int32)
    m = 2 * thickness
    for r in rows:
        w, h = int(rng.integers(m, max(iw // 2, m + 1))), int(rng.integers(m, max(ih // 2, m + 1)))
        w, h = min(w, iw), min(h, ih)
        left, top = int(rng.integers(0, iw - w + 1)), int(rng.integers(0, ih - h + 1))
        r[:] = (left, top, left + w, top + h, rng.integers(0, n_classes))
    scores = rng.random(n, dtype=np.float32) * rng.random(n, dtype=np.float32)
    return rows, scores


def pack(cases):
    """[(rows, scores)] per image -> packed rows, offsets (B + 1), scores."""
    offsets = np.cumsum([0] + [len(r) for r, _ in cases]).astype(np.int32)
    rows = np.concatenate([r for r, _ in cases]) if cases else np.zeros((0, 5), np.int32)
    scores = np.concatenate([s for _, s in cases]) if cases else np.zeros(0, np.float32)
    return rows.astype(np.int32).reshape(-1, 5), offsets, scores.astype(np.float32)


def label_indices(rows, scores, n_classes=len(CLASS_NAMES)):
    return (np.clip(rows[:, 4], 0, n_classes - 1) * render.LABEL_SCORES + render.score_index(scores)).astype(np.int32)
