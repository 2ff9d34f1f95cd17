"""Golden vectors for the device rendering (csrc/render.hip, asy-vrnet_amd/render.py), produced with Pillow and with the
reference's own colour lists.  deeplab.py and yolo.py cannot be imported here (cv2, the network, a weights file), so
  * the colour lists are EXECUTED from the reference's source at generation time: the `if self.num_classes <= 21` statement
    of deeplab.py's __init__ and the three colour statements of yolo.py's __init__ are cut out of the parsed file with
    `ast` and run against a stub `self` -- nothing of them is pasted here;
  * the pictures are produced by the same Pillow / numpy calls the predictors make (Image.blend, the palette lookup, the
    bool mask, ImageDraw.rectangle per ring), on seeded inputs.
Blend tables: a 256 x 256 "frame" whose byte is the row index blended with a 256-entry grey palette indexed by the column, so
every (a, b) pair occurs; one table per alpha.  Besides 0.7, 0.3, 0.5, 0 and 1 the alphas include values found by search at
which a contracted evaluation (a + alpha * (b - a) rounded once, what a fused multiply-add gives) differs from Pillow's two
roundings on at least one pair: the table then tells the two apart.  Commits arrays only: tests/golden/render_small.npz.
    python tools/make_golden_render.py <root of the reference checkout>"""
import ast
import colorsys
import os
import sys
import types

import numpy as np
import PIL
from PIL import Image, ImageDraw

ROOT = sys.argv[1]
rng = np.random.default_rng(20261017)


# ---- the reference's colour lists ---------------------------------------------------------------------------------

def init_statements(path):
    tree = ast.parse(open(os.path.join(ROOT, path)).read())
    for node in ast.walk(tree):
        if isinstance(node, ast.FunctionDef) and node.name == "__init__":
            return node.body
    raise SystemExit(f"no __init__ in {path}")


def run(stmts, num_classes):
    self = types.SimpleNamespace(num_classes=num_classes)
    mod = ast.fix_missing_locations(ast.Module(body=stmts, type_ignores=[]))
    exec(compile(mod, "<reference>", "exec"), {"colorsys": colorsys, "self": self})
    return np.array(self.colors, np.uint8).reshape(-1, 3)


def mentions_colors(node):
    return any(isinstance(n, ast.Attribute) and n.attr == "colors" for n in ast.walk(node)) or \
        any(isinstance(n, ast.Name) and n.id == "hsv_tuples" for n in ast.walk(node))


seg_stmts = [s for s in init_statements("deeplab.py") if isinstance(s, ast.If) and mentions_colors(s)]
det_stmts = [s for s in init_statements("yolo.py") if isinstance(s, ast.Assign) and mentions_colors(s)]
assert len(seg_stmts) == 1 and len(det_stmts) == 3, (len(seg_stmts), len(det_stmts))
out = {"pillow_version": np.array(PIL.__version__)}
for n in (9, 21, 30):
    out[f"seg_palette_{n}"] = run(seg_stmts, n)
out["det_palette_4"] = run(det_stmts, 4)
assert out["seg_palette_9"].shape == (22, 3) and out["seg_palette_30"].shape == (30, 3)


# ---- blend tables ---------------------------------------------------------------------------------------------------

A = np.repeat(np.arange(256, dtype=np.uint8)[:, None], 256, axis=1)       # the frame byte: the row index
Bm = np.repeat(np.arange(256, dtype=np.uint8)[None, :], 256, axis=0)      # the palette byte: the column index


def two_roundings(alpha):
    a, d = A.astype(np.float32), (Bm.astype(np.int32) - A.astype(np.int32)).astype(np.float32)
    return (a + np.float32(alpha) * d).astype(np.int32)                   # float32 product, float32 sum: each rounded


def one_rounding(alpha):
    exact = A.astype(np.float64) + np.float64(np.float32(alpha)) * (Bm.astype(np.float64) - A.astype(np.float64))
    return exact.astype(np.float32).astype(np.int32)                       # the sum is exact in double: ONE rounding to float32


found = []
for alpha in [k / 64 for k in range(1, 64)] + [k / 100 for k in range(1, 100)] + [k / 255 for k in range(1, 255)] + \
        [k / 1000 for k in range(1, 1000)]:
    pairs = int((two_roundings(alpha) != one_rounding(alpha)).sum())
    if pairs and alpha not in found:
        found.append(alpha)
print(f"alphas at which one rounding differs from two on some (a, b) pair: {len(found)} found; keeping {found[:3]}")
alphas = [0.7, 0.3, 0.5, 0.0, 1.0] + found[:3]
out["blend_alphas"] = np.array(alphas, np.float64)
out["blend_contract_sensitive"] = np.array([a in found[:3] for a in alphas])
tables = []
for alpha in alphas:
    t = np.array(Image.blend(Image.fromarray(A, "L"), Image.fromarray(Bm, "L"), alpha))
    print(f"alpha {alpha}: Pillow vs two roundings {int((t != two_roundings(alpha)).sum())} bytes differ, "
          f"vs one rounding {int((t != one_rounding(alpha)).sum())}")
    tables.append(t)
out["blend_tables"] = np.stack(tables)


# ---- the three mix types on a 37 x 53 frame ------------------------------------------------------------------------

def class_map(ih, iw, n):
    """Blocks of one class, 1-9 pixels wide, so that regions and single pixels both occur."""
    m = np.zeros((ih, iw), np.uint8)
    y = 0
    while y < ih:
        hh = int(rng.integers(1, 10))
        x = 0
        while x < iw:
            ww = int(rng.integers(1, 10))
            m[y:y + hh, x:x + ww] = rng.integers(0, n)
            x += ww
        y += hh
    return m


frame = rng.integers(0, 256, (37, 53, 3), dtype=np.uint8)
pr = class_map(37, 53, 9)
colors = out["seg_palette_9"]
seg_img = np.reshape(colors[np.reshape(pr, [-1])], [37, 53, -1])
out["mix_frame"], out["mix_class_map"] = frame, pr
out["mix0"] = np.array(Image.blend(Image.fromarray(frame), Image.fromarray(np.uint8(seg_img)), 0.7))
out["mix1"] = np.uint8(seg_img)
out["mix2"] = (np.expand_dims(pr != 0, -1) * np.array(frame, np.float32)).astype("uint8")
out["mix_counts"] = np.array([np.sum(pr == i) for i in range(len(colors))], np.int64)


# ---- box outlines ---------------------------------------------------------------------------------------------------

def draw(img, rows, thickness, palette):
    image = Image.fromarray(img.copy())
    d = ImageDraw.Draw(image)
    for left, top, right, bottom, c in rows:
        for i in range(thickness):
            if left + i > right - i or top + i > bottom - i:
                break                                             # Pillow raises ValueError; the project paints nothing
            assert bottom - i > top + i, "a one-row ring: Pillow paints it two rows high, keep it out of the golden"
            d.rectangle([left + i, top + i, right - i, bottom - i], outline=tuple(int(v) for v in palette[c]))
    return np.array(image)


IH, IW = 37, 53
BOX_CASES = [   # (name, thickness, rows of left, top, right, bottom, colour)
    ("inside_t1", 1, [(5, 4, 30, 20, 0), (33, 22, 47, 33, 1)]),
    ("inside_t5", 5, [(5, 4, 30, 24, 2), (28, 18, 50, 34, 3)]),
    ("touching_edges_t1", 1, [(0, 0, IW - 1, IH - 1, 1), (0, 10, 20, 20, 2), (10, 0, 25, 9, 3), (40, 5, IW - 1, 30, 0),
                              (30, 25, 45, IH - 1, 2)]),
    ("crossing_edges_t5", 5, [(-3, 5, 20, 30, 0), (30, -4, 50, 10, 1), (40, 14, IW + 5, 30, 2), (5, 28, 25, IH + 3, 3),
                              (-7, -7, IW + 7, IH + 7, 1)]),
    ("right_eq_iw_bottom_eq_ih_t1", 1, [(20, 10, IW, IH, 3)]),
    ("right_eq_iw_bottom_eq_ih_t5", 5, [(20, 10, IW, IH, 2), (0, 0, IW, IH, 0)]),
    ("overlap_a_then_b_t5", 5, [(6, 6, 34, 26, 0), (20, 14, 48, 32, 3)]),
    ("overlap_b_then_a_t5", 5, [(20, 14, 48, 32, 3), (6, 6, 34, 26, 0)]),
    ("too_small_for_all_rings_t5", 5, [(10, 10, 17, 15, 1), (30, 8, 33, 31, 2)]),
]
box_frame = rng.integers(0, 256, (IH, IW, 3), dtype=np.uint8)
out["box_frame"] = box_frame
out["box_names"] = np.array([c[0] for c in BOX_CASES])
for name, thickness, rows in BOX_CASES:
    out[f"box_{name}_rows"] = np.array(rows, np.int32)
    out[f"box_{name}_thickness"] = np.array(thickness)
    out[f"box_{name}_out"] = draw(box_frame, rows, thickness, out["det_palette_4"])

dst = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests", "golden", "render_small.npz")
np.savez_compressed(dst, **out)
print(f"wrote {dst}: {os.path.getsize(dst)} bytes, {len(out)} arrays")
