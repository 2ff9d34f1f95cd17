"""Writes tests/golden/label_atlas_builtin.npz: the `render.LabelAtlas` of four class names at font sizes 1, 8 and 10 from
Pillow's built-in face (`ImageFont.load_default(size)`), which the GPU label tests fall back to where Pillow is missing.

    python tools/make_label_atlas_fixture.py
"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

CLASS_NAMES = ("tv/monitor", "Wy", "a", "boat")
SIZES = (1, 8, 10)


def main():
    from asy_vrnet_amd import render
    atlas = render.LabelAtlas(CLASS_NAMES, None, SIZES)
    path = os.path.join(ROOT, "tests", "golden", "label_atlas_builtin.npz")
    atlas.save(path)
    print(f"{path}: {os.path.getsize(path)} bytes on disk, {atlas.nbytes} bytes as arrays")


if __name__ == "__main__":
    main()
