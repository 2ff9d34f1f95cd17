"""The host rule of the JPEG encoder, render.jpeg_encode_host, against live Pillow (libjpeg-turbo) without a GPU: the WHOLE
file -- header with its JFIF segment, quantisation and Annex K Huffman tables, scan data, EOI -- equals what
Image.save(format="JPEG", quality=q, subsampling=s) writes, for 4:4:4 and 4:2:0.  The kernels of csrc/jpeg.hip are held to
this rule by tests/test_jpeg.py."""
import io

import numpy as np
import pytest
from PIL import Image

from asy_vrnet_amd import render

SIZES_444 = [(1, 1), (8, 8), (9, 17), (24, 40), (37, 53)]
SIZES_420 = [(1, 1), (8, 8), (16, 16), (9, 17), (17, 7), (24, 40), (37, 53), (3, 40), (40, 3), (25, 8), (33, 49)]
QUALITIES = (1, 25, 50, 75, 95, 100)
CASES = [(s, 0) for s in SIZES_444] + [(s, 2) for s in SIZES_420]


def pillow(image, quality, subsampling):
    out = io.BytesIO()
    Image.fromarray(image).save(out, format="JPEG", quality=quality, subsampling=subsampling)
    return out.getvalue()


def pictures(h, w):
    """Seeded noise, a modular ramp, hard stripes and a constant image."""
    stripes = np.full((h, w, 3), 255, np.uint8)
    stripes[::3] = 0
    return dict(noise=np.random.default_rng(1000 * h + w).integers(0, 256, (h, w, 3), dtype=np.uint8),
                ramp=((np.arange(h * w * 3).reshape(h, w, 3) * 7) % 256).astype(np.uint8), stripes=stripes,
                constant=np.full((h, w, 3), 77, np.uint8))


@pytest.fixture(scope="module")
def encoded():
    """Every case once: {(size, subsampling, quality, picture name): (the rule's file, Pillow's file)}."""
    return {(size, s, q, name): (render.jpeg_encode_host(a, q, s), pillow(a, q, s))
            for size, s in CASES for q in QUALITIES for name, a in pictures(*size).items()}


def test_the_rule_writes_pillows_whole_file(encoded):
    assert len(encoded) == (len(SIZES_444) + len(SIZES_420)) * len(QUALITIES) * 4
    wrong = [key for key, (mine, theirs) in encoded.items() if mine != theirs]
    assert not wrong, wrong[:8]


def test_the_header_is_623_bytes_with_pillows_segments(encoded):
    for (size, s, q, name), (mine, theirs) in encoded.items():
        if name != "noise":
            continue
        head = render.jpeg_header(*size, q, s)
        assert len(head) == render.JPEG_HEADER == 623 and theirs[:623] == head and theirs[-2:] == b"\xff\xd9"
        assert head[163:167] == size[0].to_bytes(2, "big") + size[1].to_bytes(2, "big")
        assert head[25:89] == bytes(render.jpeg_tables(q)[0][render.JPEG_ZIGZAG].tolist())
        assert head[94:158] == bytes(render.jpeg_tables(q)[1][render.JPEG_ZIGZAG].tolist())
    assert render.jpeg_tables(50)[0].tolist()[:8] == [16, 11, 10, 16, 24, 40, 51, 61] and (render.jpeg_tables(100) == 1).all()
    assert render.jpeg_tables(1).max() == 255


def test_every_file_decodes(encoded):
    for (size, s, q, name), (mine, _) in encoded.items():
        picture = Image.open(io.BytesIO(mine))
        picture.load()
        assert picture.size == (size[1], size[0]) and picture.mode == "RGB"


def test_the_inputs_reach_the_paths_that_matter(encoded):
    """The cases cannot pass by skipping what is hard: stuffed bytes, ZRL symbols, dummy Y blocks in a row and in a column of
    one image, and a chroma block row that is padding as a whole."""
    assert any(b"\xff\x00" in mine[623:] for mine, _ in encoded.values())
    zrl = 0
    for size, s in CASES:
        for name, a in pictures(*size).items():
            q, comp, dummy = render.jpeg_blocks_host(a, 50, s)
            zrl += render.jpeg_scan_host(q, comp)[1]
    assert zrl > 0
    rows_and_columns = []
    for h, w in SIZES_420:
        dummy = render.jpeg_blocks_host(np.zeros((h, w, 3), np.uint8), 50, 2)[2]
        MH, MW = -(-h // 16), -(-w // 16)
        d = dummy.reshape(MH, MW, 6)[..., :4].reshape(MH, MW, 2, 2)
        in_row, in_column = bool(d[-1, :, 1, :].all() and d[-1, :, 1].any()), bool(d[:, -1, :, 1].all() and d[:, -1, :, 1].any())
        assert in_row == (-(-h // 8) < 2 * MH) and in_column == (-(-w // 8) < 2 * MW)
        rows_and_columns.append(in_row and in_column)
    assert any(rows_and_columns)                                           # (1, 1), (8, 8) and (25, 8)
    # h = 8 and h = 24: the last chroma block row of the reduced plane is replicated as a whole
    assert any(h in (8, 24) for h, _ in SIZES_420)
    for h, w in ((8, 8), (24, 40)):
        a = pictures(h, w)["noise"]
        assert 8 * -(-h // 16) - (h + 1) // 2 >= 4 and render.jpeg_encode_host(a, 95, 2) == pillow(a, 95, 2)


def test_a_dummy_block_codes_as_no_difference_and_an_end_of_block():
    a = pictures(8, 8)["noise"]
    q, comp, dummy = render.jpeg_blocks_host(a, 75, 2)
    assert comp.tolist() == [0, 0, 0, 0, 1, 2] and dummy.tolist() == [False, True, True, True, False, False]
    assert (q[1:4, 0] == q[0, 0]).all() and not q[1:4, 1:].any()


def test_bad_keywords_raise():
    a = np.zeros((8, 8, 3), np.uint8)
    for quality in (0, 101, 50.0, True):
        with pytest.raises(RuntimeError, match="quality"):
            render.jpeg_encode_host(a, quality)
    for subsampling in (1, 3, "4:2:0", True):
        with pytest.raises(RuntimeError, match="subsampling"):
            render.jpeg_encode_host(a, 95, subsampling)
    with pytest.raises(RuntimeError, match="uint8"):
        render.jpeg_encode_host(a.astype(np.float32))
    with pytest.raises(RuntimeError, match="uint8"):
        render.jpeg_encode_host(a[..., :1])
