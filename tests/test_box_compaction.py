"""The compaction of the three box-target kernels (csrc/traintargets.hip, augment.hip, mosaic.hip; its one copy is
augment.h's box_compact_slot) beyond a single wave: kept and dropped rows interleave across the wave boundaries at rows 64,
128, 192 and across the chunk boundary at row 256 of a 256-thread workgroup, so the cross-wave prefix and the running base
carry real counts.  Every result is compared bit for bit with the host functions of data.py, as in test_train_frames.py,
test_augment.py and test_mosaic.py, whose tables stop at 8 rows.  Canvas 64 x 64; images of 300, 257, 65 and 0 boxes under
max_gt = 300; about every third box is one source pixel wide or high and is dropped after the map.  Mosaic: sources of 70,
0, 260 and 3 rows under max_gt = 340, and four sources that keep more than 340 rows between them."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

S = (64, 64)
CAP = (96, 112)
SIZES = [(48, 80), (90, 60), (64, 64), (37, 111)]
ROWS = [300, 257, 65, 0]
MAX_GT = 300
MOS_ROWS = [70, 0, 260, 3]
MOS_MAX_GT = 340


@pytest.fixture(scope="module")
def A():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    import asy_vrnet_amd
    return asy_vrnet_amd


def table_tensor(table):
    return torch.from_numpy(np.ascontiguousarray(table.view(np.uint8).reshape(len(table), -1))).cuda()


def make_boxes(seed, size, n, thin=True):
    """n rows x1, y1, x2, y2, cls inside and a little around an image of size = (ih, iw), 8 .. 23 source pixels on a side;
    thin: rows 1, 4, 7, ... are one source pixel wide or high, in turn."""
    rng = np.random.default_rng(seed)
    ih, iw = size
    x1, y1 = rng.integers(-4, iw - 8, n), rng.integers(-4, ih - 8, n)
    w, h = rng.integers(8, 24, n), rng.integers(8, 24, n)
    if thin:
        i = np.arange(n)
        w[(i % 3 == 1) & (i % 2 == 0)] = 1
        h[(i % 3 == 1) & (i % 2 == 1)] = 1
    return np.stack([x1, y1, x1 + w, y1 + h, rng.integers(0, 4, n)], 1).astype(np.int64)


BOXES = [make_boxes(10 + b, size, n) for b, (size, n) in enumerate(zip(SIZES, ROWS))]


def run(fn, boxes, table, n_out, max_gt):
    """fn(boxes, counts, table, capacity, H, W, ...) over guard-filled outputs -> targets, counts_out, flag on the host."""
    from asy_vrnet_amd import data
    packed, cnt = data.pack_boxes(boxes, max_gt)
    targets = torch.full((n_out, max_gt, 5), -7.0, dtype=torch.float32, device="cuda")          # guard
    counts_out = torch.full((n_out,), -1, dtype=torch.int32, device="cuda")
    flag = torch.zeros(1, dtype=torch.int32, device="cuda")
    fn(packed.cuda(), cnt.cuda(), table_tensor(table), CAP, S[0], S[1], targets=targets, counts_out=counts_out, flag=flag)
    return targets.cpu().numpy(), counts_out.cpu().numpy(), int(flag)


def assert_rows(got, counts, want, max_gt):
    for b, w in enumerate(want):
        w = w.astype(np.float32)
        assert counts[b] == len(w) <= max_gt, (b, counts[b], len(w))
        assert np.array_equal(got[b, :len(w)], w), (b, np.argwhere(got[b, :len(w)] != w)[:4])      # kept rows in input order
        assert np.array_equal(got[b, len(w):], np.zeros((max_gt - len(w), 5), np.float32)), b      # the guard is gone


def assert_interleaved(want, rows):
    """The inputs do what they are for: a quarter or more of each image's rows are dropped, the rest kept."""
    for w, n in zip(want, rows):
        assert (n == 0 and len(w) == 0) or n // 4 <= n - len(w) < n, (n, len(w))


def test_box_targets_ragged_compacts_across_waves_and_chunks(A):
    from asy_vrnet_amd import data, hip
    want = [data.boxes_xyxy_to_cxcywh(data.adjust_boxes(bx, iw, ih, S[1], S[0])) for bx, (ih, iw) in zip(BOXES, SIZES)]
    assert_interleaved(want, ROWS)
    geom = data.frame_geometry(SIZES, S, True, CAP, None)
    got, counts, flag = run(hip.box_targets_ragged, BOXES, geom, len(SIZES), MAX_GT)
    assert flag == 0
    assert_rows(got, counts, want, MAX_GT)


def test_augment_box_targets_compacts_across_waves_and_chunks(A):
    from asy_vrnet_amd import data, hip
    # size, nw, nh, dx, dy, flip: scales at or below 1, so that a thin row stays thin; two records flip, two do not
    rows = [((48, 80), 70, 44, -3, 5, True), ((90, 60), 40, 60, 10, 2, False), ((64, 64), 64, 64, 5, -7, True),
            ((37, 111), 50, 17, 3, 20, False)]
    table = data.check_aug_table(np.stack([data.aug_record(size, S, nw, nh, dx, dy, flip) for size, nw, nh, dx, dy, flip in rows]),
                                 S, CAP)
    want = [data.boxes_xyxy_to_cxcywh(data.augment_boxes(bx, iw, ih, S[1], S[0], rec))
            for bx, (ih, iw), rec in zip(BOXES, SIZES, table)]
    assert_interleaved(want, ROWS)
    got, counts, flag = run(hip.augment_box_targets, BOXES, table, len(SIZES), MAX_GT)
    assert flag == 0
    assert_rows(got, counts, want, MAX_GT)


def mosaic_table():
    """One record: the cut at (30, 34), every tile a little larger than its quadrant, so that the cut clips some boxes and
    drops others; tiles 1 and 3 mirror their source."""
    from asy_vrnet_amd import data
    tiles = [(0, SIZES[0], 40, 40, -6, -4, 0), (1, SIZES[1], 36, 34, -2, 32, 1), (2, SIZES[2], 40, 36, 28, 30, 0),
             (3, SIZES[3], 38, 38, 28, -2, 1)]
    return data.check_mosaic_table(np.stack([data.mosaic_record(S, (30, 34), tiles)]), S, SIZES, CAP)


def test_mosaic_box_targets_compacts_across_tiles_waves_and_chunks(A):
    from asy_vrnet_amd import data, hip
    boxes = [make_boxes(20 + s, size, n) for s, (size, n) in enumerate(zip(SIZES, MOS_ROWS))]
    table = mosaic_table()
    want = [data.boxes_xyxy_to_cxcywh(data.mosaic_boxes(boxes, SIZES, S, rec)) for rec in table]
    first = len(data.mosaic_boxes([boxes[0], None, None, None], SIZES, S, table[0]))
    # tile 0's rows end inside a wave, tile 2's rows then cross a chunk boundary of their own, and rows are dropped
    assert 0 < first < 64 and 64 < len(want[0]) < sum(MOS_ROWS) * 3 // 4
    got, counts, flag = run(hip.mosaic_box_targets, boxes, table, 1, MOS_MAX_GT)
    assert flag == 0
    assert_rows(got, counts, want, MOS_MAX_GT)


def test_mosaic_box_targets_keep_the_first_max_gt_rows_at_that_size(A):
    from asy_vrnet_amd import data, hip
    boxes = [make_boxes(30 + s, size, 330, thin=False) for s, size in enumerate(SIZES)]
    table = mosaic_table()
    want = data.boxes_xyxy_to_cxcywh(data.mosaic_boxes(boxes, SIZES, S, table[0]))
    assert MOS_MAX_GT < len(want) < 4 * 330                                     # more than fit, and some are cut away
    got, counts, flag = run(hip.mosaic_box_targets, boxes, table, 1, MOS_MAX_GT)
    assert flag == hip.FLAG_BOX_COUNT
    assert_rows(got, counts, [want[:MOS_MAX_GT]], MOS_MAX_GT)
