"""The host statements of the captions (render.fixed_tenths, GlyphAtlas, caption_strings, caption_records / caption_decode,
draw_captions_host): the formatting against Python's own, the glyph cells against live Pillow, the placement rule on a
hand-made atlas.  No GPU.  tests/test_captions.py holds the kernels of csrc/captions.hip to these statements."""
import numpy as np
import pytest

from asy_vrnet_amd import data, render
from tests import captions_cases as CC


def test_alphabet_and_constants():
    assert render.CAPTION_ALPHABET == "0123456789.-+#m/s " and render.CAPTION_GLYPHS == 18
    assert render.FLAG_CAPTION == 65536 and render.CAPTION_MAX == 32 and render.CAPTION_WORDS == 12
    from asy_vrnet_amd import infer
    assert infer.FLAG_CAPTION == render.FLAG_CAPTION


def test_fixed_tenths_equals_python_format_at_every_tie():
    ties = CC.tie_sweep()
    assert ties.dtype == np.float32 and ties.shape == (500000,) and (ties > 0).all()
    assert CC.tenths_text(ties) == ["{:.1f}".format(float(x)) for x in ties]


def test_fixed_tenths_equals_python_format_on_random_values():
    x = (np.random.default_rng(1).random(100000) * 10000).astype(np.float32)
    assert x.min() >= 0 and x.max() < 10000
    assert CC.tenths_text(x) == ["{:.1f}".format(float(v)) for v in x]


def test_signed_formatting():
    rng = np.random.default_rng(2)
    ties = CC.tie_sweep()
    ties = ties[ties < 1000]
    x = np.concatenate([ties, -ties, ((rng.random(50000) - 0.5) * 2000).astype(np.float32),
                        np.array([-0.04, -0.0, 0.0, 0.25, 0.75, -0.25, -0.75, 0.05, -0.05, 1e-45, -1e-45, 999.95], np.float32)])
    assert np.abs(x).max() <= 1000
    assert CC.tenths_text(x, signed=True) == ["{:+.1f}".format(float(v)) for v in x]
    named = dict(zip(x[-12:].tolist(), CC.tenths_text(x[-12:], signed=True)))
    assert CC.tenths_text(np.array([-0.04, -0.0, 0.25, 0.75], np.float32), signed=True) == ["-0.0", "-0.0", "+0.2", "+0.8"], named
    assert CC.tenths_text(np.array([-0.04, 0.25, 0.75], np.float32)) == ["-0.0", "0.2", "0.8"]


def test_fixed_tenths_saturates():
    x = np.array([np.inf, -np.inf, np.nan, 3e38, 2.0 ** 31, 214748368.0, 1e8, 2.0 ** 24, 16777216.0 * 8], np.float32)
    k, neg = render.fixed_tenths(x)
    sat = render.CAPTION_SATURATED
    assert k.tolist() == [sat, sat, sat, sat, sat, sat, 1000000000, 167772160, 1342177280] and neg.tolist()[:2] == [False, True]
    assert k.dtype == np.int32 and render.fixed_tenths(np.float32(9999.95))[0] == 99999 + 1      # 9999.9501953125: beyond the range
    assert render.fixed_tenths(np.float32(9999.94))[0] == 99999
    with pytest.raises(RuntimeError, match="float32"):
        render.fixed_tenths(np.zeros(3))


def pillow_cells(size):
    from PIL import Image, ImageDraw, ImageFont
    font = ImageFont.load_default(size)
    glyphs = [render._label_mask(font, ch) for ch in render.CAPTION_ALPHABET]
    shift_y = -min(0, min(int(off[1]) for _, _, off in glyphs))
    cell_h = max(int(off[1]) + wh[1] for _, wh, off in glyphs) + shift_y
    for ch, (mask, (mw, mh), off) in zip(render.CAPTION_ALPHABET, glyphs):
        mox, shift_x = int(off[0]), -min(int(off[0]), 0)
        cw = max(max(int(np.ceil(font.getlength(ch))), mox + mw) + shift_x, 1)
        img = Image.new("RGB", (cw, cell_h), (255, 255, 255))
        ImageDraw.Draw(img).text((shift_x, shift_y), ch, fill=0, font=font)
        yield ch, np.array(img), (mask, mw, mh, mox + shift_x, int(off[1]) + shift_y)


@pytest.mark.parametrize("size", [1, 8, 10, 32])
def test_every_cell_is_what_pillow_draws(size):
    pytest.importorskip("PIL")
    atlas = render.GlyphAtlas(None, (size,))
    assert atlas.sizes == (size,) and atlas.records.shape == (1, 18, 4) and atlas.nbytes == atlas.blob.nbytes + atlas.records.nbytes
    assert (atlas.records[0, :, 2] == atlas.records[0, 0, 2]).all() and (atlas.records[0, :, 3] == 0).all()
    offset = 0
    for code, (ch, drawn, (mask, mw, mh, x, y)) in enumerate(pillow_cells(size)):
        cell = atlas.cell(size, code)
        assert int(atlas.records[0, code, 0]) == offset and cell.shape == drawn.shape[:2], ch
        offset += cell.size
        want = render._div255(255 * (255 - cell.astype(np.int64))).astype(np.uint8)
        assert np.array_equal(drawn, np.repeat(want[..., None], 3, 2)), ch
        # no mask column or row is lost: the whole mask sits inside the cell, the rest of the cell is zero
        rest = cell.copy()
        if mw and mh:
            assert np.array_equal(cell[y:y + mh, x:x + mw], mask.reshape(mh, mw)), ch
            rest[y:y + mh, x:x + mw] = 0
        assert not rest.any(), ch
    assert offset == atlas.blob.size


def test_the_committed_fixture_is_the_built_atlas(tmp_path):
    fixture = render.GlyphAtlas.load(CC.FIXTURE)
    assert fixture.sizes == CC.FIXTURE_SIZES and fixture.nbytes < 8192
    assert fixture.size_table([17, 270, 320, 12]).tolist() == [0, 1, 2, -1]
    with pytest.raises(RuntimeError, match="image 1 of 100 rows needs font size 3"):
        fixture.size_table([17, 100])
    with pytest.raises(RuntimeError, match="was not built"):
        fixture.size_index(9)
    fixture.save(tmp_path / "again.npz")
    again = render.GlyphAtlas.load(tmp_path / "again.npz")
    assert np.array_equal(again.blob, fixture.blob) and np.array_equal(again.records, fixture.records)
    pytest.importorskip("PIL")
    built = render.GlyphAtlas(None, CC.FIXTURE_SIZES)
    assert np.array_equal(built.blob, fixture.blob) and np.array_equal(built.records, fixture.records)


def hand_atlas():
    """Two glyph shapes at font size 1, cell height 3: the digits and signs are 2 wide, 'm', '/', 's' and the space 3 wide."""
    cells, records, total = [], np.zeros((1, 18, 4), np.int32), 0
    for code in range(18):
        cw = 2 if code < 14 else 3
        cell = ((np.arange(3 * cw).reshape(3, cw) * 37 + 11 * code) % 256).astype(np.uint8)
        cell[0, 0], cell[2, cw - 1] = 255, 0
        records[0, code, :3] = (total, cw, 3)
        cells.append(cell.reshape(-1))
        total += cell.size
    return render.GlyphAtlas.from_arrays((1,), np.concatenate(cells), records)


PAL = np.array([[250, 10, 20], [30, 240, 50], [60, 70, 230], [200, 200, 40]], np.uint8)


def paint(pic, atlas, row, text):
    """One caption by the words of the rule, pixel by pixel."""
    left, _, _, bottom, cls = row
    ih, iw = pic.shape[:2]
    widths = [int(atlas.records[0, render.CAPTION_ALPHABET.index(c), 1]) for c in text]
    W, ch = sum(widths), 3
    ox, oy = (left, bottom + 1) if bottom + ch <= ih - 1 else (left, bottom - ch)
    for y in range(max(oy, 0), min(oy + ch, ih)):
        for x in range(max(ox, 0), min(ox + W, iw)):
            px, i = x - ox, 0
            while px >= widths[i]:
                px, i = px - widths[i], i + 1
            m = int(atlas.cell(1, render.CAPTION_ALPHABET.index(text[i]))[y - oy, px])
            a = PAL[min(max(cls, 0), 3)].astype(np.int64) * (255 - m) + 128
            pic[y, x] = (a + (a >> 8)) >> 8
    return (ox, oy, W)


def test_placement_on_a_hand_made_atlas():
    atlas, rng = hand_atlas(), np.random.default_rng(3)
    base = rng.integers(0, 256, (12, 16, 3), dtype=np.uint8)
    # ih = 12, ch = 3: bottom + ch == ih - 1 at bottom = 8 (below the box), one beyond at bottom = 9 (flipped into the box)
    cases = [
        ([(2, 1, 9, 8, 0)], ["#1"], (2, 9)),                          # the last row that fits below: rows 9..11
        ([(2, 1, 9, 9, 1)], ["#1"], (2, 6)),                          # one beyond: flipped, rows 6..8
        ([(-3, 0, 5, 4, 2)], ["12.5m"], (-3, 5)),                     # clipped at the left border
        ([(11, 0, 15, 4, 3)], ["-1.0m/s"], (11, 5)),                  # clipped at the right border
        ([(1, 0, 5, 12, 0)], ["7"], (1, 9)),                          # bottom = ih: flipped, rows 9..11
        ([(1, 0, 5, 14, 0)], ["7"], (1, 11)),                         # bottom beyond the image: flipped, clipped at the bottom border
        ([(4, 0, 8, 30, 0)], ["7"], None),                            # wholly below the image: nothing
        ([(3, 0, 9, 4, 0), (5, 0, 9, 5, 9)], ["#12 3.4m", "+5"], None),      # overlapping tags: the later one wins; class 9 clamps
        ([(3, 0, 9, 4, 0), (5, 0, 9, 5, 1)], ["#12 3.4m", ""], None),        # an empty caption draws nothing
    ]
    for rows, strings, origin in cases:
        rows = np.array(rows, np.int32)
        want = base.copy()
        origins = [paint(want, atlas, r, s) for r, s in zip(rows.tolist(), strings) if s]
        if origin is not None:
            assert origins[0][:2] == origin, (rows, origins)
        got = render.draw_captions_host(base, rows, strings, atlas, 1, PAL)
        assert np.array_equal(got, want), (rows.tolist(), strings)
        assert np.array_equal(got, base) == (strings == ["7"] and rows[0, 3] == 30)
    # the overlap case really overlaps, and the empty caption leaves the first tag whole
    a = render.draw_captions_host(base, np.array(cases[7][0], np.int32), cases[7][1], atlas, 1, PAL)
    b = render.draw_captions_host(base, np.array(cases[8][0], np.int32), cases[8][1], atlas, 1, PAL)
    assert (a != b).any(axis=2).sum() > 0 and np.array_equal(a[:6, :5], b[:6, :5])
    # font size 0 draws nothing; a 12-row image asks for size 0 by itself; a size-0 image is returned as it is
    rows = np.array(cases[0][0], np.int32)
    assert render.label_font_size(12) == 0
    assert np.array_equal(render.draw_captions_host(base, rows, ["#1"], atlas, 0, PAL), base)
    assert np.array_equal(render.draw_captions_host(base, rows, ["#1"], atlas, None, PAL), base)
    empty = np.zeros((0, 16, 3), np.uint8)
    assert render.draw_captions_host(empty, rows, ["#1"], atlas, 1, PAL).shape == (0, 16, 3)
    with pytest.raises(RuntimeError, match="was not built"):
        render.draw_captions_host(base, rows, ["#1"], atlas, 2, PAL)
    with pytest.raises(RuntimeError, match="n captions"):
        render.draw_captions_host(base, rows, [], atlas, 1, PAL)


def track(id=0, row=-1, range_age=-1, rng=0.0, rate=0.0):
    t = np.zeros((), data.TRACK_DTYPE)
    t["id"], t["row"], t["range_age"] = id, row, range_age
    t["x"][4], t["v"][4] = rng, rate
    return t


def test_caption_strings_on_a_hand_written_table():
    T = 6
    table = np.zeros((2, T), data.TRACK_DTYPE)
    table[0, 0] = track(7, 2, 0, 42.46, -0.048)                       # a filtered range and a closing rate
    table[0, 1] = track(8, 0, 3, 120.25, 0.5)                         # the radar coasts: the range is still drawn
    table[0, 2] = track(9, 1, -1, 5.0, 1.0)                           # born without a radar point: range_age -1
    table[0, 3] = track(10, 5, 0, 9.0, 0.0)                           # its slot names another row than the one that carries id 10
    table[0, 5] = track(7, 2, 0, 1.0, 0.0)                            # a corrupt duplicate: the lowest slot wins
    table[1] = [track(100 + s, s, 0, 10.0 * s, 0.0) for s in range(T)]       # a full table; row 6 got id 0
    ids = np.zeros((2, 8), np.int32)
    ids[0, :5] = (8, 9, 7, 10, 0)
    ids[1, :7] = (100, 101, 102, 103, 104, 105, 0)
    strings, bits = render.caption_strings(ids, [5, 7], table, rate_scale=25.0)
    assert bits == 0
    assert strings[0] == ["#8 120.2m +12.5m/s", "#9", "#7 42.5m -1.2m/s", "#10", ""]
    assert strings[1] == ["#100 0.0m +0.0m/s"] + [f"#{100 + s} {10 * s}.0m +0.0m/s" for s in range(1, T)] + [""]
    # rate_scale 0: no speed field; without the table: the ids alone
    assert render.caption_strings(ids, [5, 7], table)[0][0][:3] == ["#8 120.2m", "#9", "#7 42.5m"]
    assert render.caption_strings(ids, [3, 0])[0] == [["#8", "#9", "#7"], []]
    # kept outside [0, cap] is clamped and flagged
    s, bits = render.caption_strings(ids, [9, -1])
    assert bits == render.FLAG_BOX_COUNT and len(s[0]) == 8 and s[1] == []


def test_caption_strings_without_a_tracker_and_every_omission():
    points = np.array([[3, 0, 1, 2, 1, 1, 1, 1]], np.int32)
    readout = np.zeros((1, 8, 2, 5), np.float32)
    readout[0, :, 0, 0] = 1.0                                         # the nearest point: not what is drawn
    readout[0, :, 1, 0] = (42.46, 7.0, 0.04, 9999.94, 9999.95, np.nan, -1.0, np.inf)
    strings, bits = render.caption_strings(None, [8], box_points=points, box_radar=readout)
    assert strings == [["42.5m", "", "0.0m", "9999.9m", "", "", "", ""]] and bits == render.FLAG_CAPTION
    assert render.caption_strings(None, [4], box_points=points, box_radar=readout) == ([["42.5m", "", "0.0m", "9999.9m"]], 0)
    for bad in (9999.95, np.nan, -1.0, -0.0, np.inf):
        readout[0, 0, 1, 0] = bad
        assert render.caption_strings(None, [1], box_points=points, box_radar=readout) == ([[""]], render.FLAG_CAPTION), bad
    # with ids beside the readout: the id stays, the bad range is left out
    ids = np.full((1, 8), 5, np.int32)
    assert render.caption_strings(ids, [2], box_points=points, box_radar=readout) == ([["#5", "#5"]], render.FLAG_CAPTION)
    # the speed: a rate that is not finite or too large is left out, the range stays; a bad range takes the speed with it
    table = np.zeros((1, 4), data.TRACK_DTYPE)
    ids = np.array([[1, 2, 3, 4]], np.int32)
    for s, (rng, rate) in enumerate(((10.0, 4.0), (10.0, 40.0), (10.0, np.inf), (np.nan, 1.0))):
        table[0, s] = track(s + 1, s, 0, rng, rate)
    strings, bits = render.caption_strings(ids, [4], table, rate_scale=25.0)
    assert strings == [["#1 10.0m +100.0m/s", "#2 10.0m", "#3 10.0m", "#4"]] and bits == render.FLAG_CAPTION
    assert render.caption_strings(ids, [1], table, rate_scale=25.0)[1] == 0
    longest = np.zeros((1, 1), data.TRACK_DTYPE)
    longest[0, 0] = track(2 ** 31 - 1, 0, 0, 9999.9, -39.996)
    strings, bits = render.caption_strings(np.array([[2 ** 31 - 1]], np.int32), [1], longest, rate_scale=25.0)
    assert strings == [["#2147483647 9999.9m -999.9m/s"]] and bits == 0 and len(strings[0][0]) == 29
    for kw in (dict(ids=None, kept=[1]), dict(ids=None, kept=[1], table=table, box_points=points, box_radar=readout),
               dict(ids=ids, kept=[1], box_points=points)):
        with pytest.raises(RuntimeError, match="caption_strings"):
            render.caption_strings(**kw)


def test_records_round_trip():
    rng = np.random.default_rng(4)
    strings = CC.random_strings(rng, 200) + ["", "#2147483647 9999.9m -999.9m/s", "0123456789.-+#m/s 0123456789.-+#"]
    rec = render.caption_records(strings)
    assert rec.shape == (203, 12) and rec.dtype == np.int32 and (rec[:, 9:] == 0).all()
    assert rec[:, 8].tolist() == [len(s) for s in strings] and render.caption_decode(rec) == strings
    assert render.caption_records([strings[:3], [], strings[3:]]).tobytes() == rec.tobytes()
    one = render.caption_records(["#17 42.5m"])
    assert one.view(np.uint8)[0, :9].tolist() == [13, 1, 7, 17, 4, 2, 10, 5, 14] and one[0, 0] == 13 | 1 << 8 | 7 << 16 | 17 << 24
    # what the draw kernel makes of a corrupt record: the count clamped to 32, a code above 17 read as the space
    bad = rec[-1:].copy()
    bad[0, 8] = 40
    bad.view(np.uint8)[0, 5] = 200
    assert render.caption_decode(bad) == ["01234 6789.-+#m/s 0123456789.-+#"]
    bad[0, 8] = -3
    assert render.caption_decode(bad) == [""]
    for s in (["x"], ["0" * 33]):
        with pytest.raises(RuntimeError, match="caption_records"):
            render.caption_records(s)
