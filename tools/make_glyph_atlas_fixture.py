"""Writes tests/golden/glyph_atlas_builtin.npz: the `render.GlyphAtlas` of the caption alphabet at font sizes 1, 8 and 10 from
Pillow's built-in face (`ImageFont.load_default(size)`), which the GPU caption tests fall back to where Pillow is missing.

    python tools/make_glyph_atlas_fixture.py
"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SIZES = (1, 8, 10)


def main():
    from asy_vrnet_amd import render
    atlas = render.GlyphAtlas(None, SIZES)
    path = os.path.join(ROOT, "tests", "golden", "glyph_atlas_builtin.npz")
    atlas.save(path)
    print(f"{path}: {os.path.getsize(path)} bytes on disk, {atlas.nbytes} bytes as arrays")


if __name__ == "__main__":
    main()
