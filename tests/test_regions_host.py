"""The host statement of the connected regions, `decode.seg_regions_host` (the rule csrc/regions.hip equals bit for bit),
against independent formulations: partition, count and order from scipy.ndimage.label per class mask with the 3 x 3 or the
cross structure, renumbered by first pixel; the records from ndimage.find_objects, ndimage.sum and direct coordinate sums;
the link from a brute force with fractions.Fraction.  No GPU.

Inputs: RandomState(5) noise (rand < p) * randint(1, k + 1) at (p, k) = (0.5, 2), (0.6, 4), (0.35, 9) on the sizes (1, 1),
(1, 97), (97, 1), (2, 2), (67, 131), (150, 260) -- with max_regions = 1024 the two large sizes overflow the table -- and
smoothed nine-class blobs, which stay under it.  The patterns and helpers here are shared with tests/test_regions.py."""
from fractions import Fraction

import numpy as np
import pytest
from scipy import ndimage

from asy_vrnet_amd import decode

RD = decode.REGION_DTYPE
NOISE = ((0.5, 2), (0.6, 4), (0.35, 9))
SIZES = ((1, 1), (1, 97), (97, 1), (2, 2), (67, 131), (150, 260))
BIG = (150, 260)
_cache = {}


def noise(p, k, size):
    """The noise map of (p, k) at `size`: one RandomState(5) per (p, k), the sizes drawn in the order of SIZES."""
    if (p, k) not in _cache:
        rs = np.random.RandomState(5)
        _cache[(p, k)] = {s: ((rs.rand(*s) < p) * rs.randint(1, k + 1, s)).astype(np.uint8) for s in SIZES}
    return _cache[(p, k)][size]


def blobs(size=BIG, seed=5):
    rs = np.random.RandomState(seed)
    return np.stack([ndimage.gaussian_filter(rs.rand(*size), 6) for _ in range(9)]).argmax(0).astype(np.uint8)


def checkerboard(size=BIG):
    y, x = np.indices(size)
    return ((x + y) & 1).astype(np.uint8)


def serpentine(size=BIG):
    """Every second row set, joined alternately at the right and the left end: one region reached only along the path."""
    ih, iw = size
    m = np.zeros(size, np.uint8)
    m[0::2] = 1
    for j, y in enumerate(range(1, ih - 1, 2)):
        m[y, iw - 1 if j % 2 == 0 else 0] = 1
    return m


def stripes(sign, s, size=BIG):
    y, x = np.indices(size)
    return ((x + sign * y + s) % 3 == 0).astype(np.uint8)


def comb(size=BIG):
    """Teeth every third column hanging from the first row."""
    m = np.zeros(size, np.uint8)
    m[0] = 1
    m[:, 0::3] = 1
    return m


def u_shape(size=BIG):
    """Two arms of class 2 along the first and the last column that join only in the last row."""
    m = np.zeros(size, np.uint8)
    m[:, 0] = m[:, -1] = m[-1] = 2
    return m


def random_rows(seed, n, size, classes=4):
    """n boxes as box_rows makes them (inside the image), a few of them empty."""
    rs = np.random.RandomState(seed)
    ih, iw = size
    x = np.sort(rs.randint(0, iw + 1, (n, 2)), axis=1)
    y = np.sort(rs.randint(0, ih + 1, (n, 2)), axis=1)
    return np.stack([x[:, 0], y[:, 0], x[:, 1], y[:, 1], rs.randint(0, classes, n)], axis=1).astype(np.int32)


def structure(connectivity):
    return np.ones((3, 3), int) if connectivity == 8 else ndimage.generate_binary_structure(2, 1)


def reference_regions(cm, connectivity, background, min_area):
    """scipy's statement: the kept regions as (first, cls, mask-label pair) sorted by first pixel, and the dropped pixels."""
    ih, iw = cm.shape
    found = []
    dropped = 0
    for c in np.unique(cm).tolist():
        if c == background:
            continue
        lab, n = ndimage.label(cm == c, structure(connectivity))
        if not n:
            continue
        index = np.arange(1, n + 1)
        area = ndimage.sum(np.ones_like(lab), lab, index).astype(np.int64)
        flat = lab.reshape(-1)
        first = np.full(n + 1, ih * iw, np.int64)
        np.minimum.at(first, flat, np.arange(ih * iw))
        slices = ndimage.find_objects(lab)
        for k in range(n):
            if area[k] < min_area:
                dropped += int(area[k])
                continue
            ys, xs = np.nonzero(lab == k + 1) if n <= 64 else (None, None)
            found.append(dict(first=int(first[k + 1]), cls=c, area=int(area[k]), lab=lab, k=k + 1, box=slices[k], ys=ys, xs=xs))
    found.sort(key=lambda r: r["first"])
    return found, dropped


def check_against_scipy(cm, connectivity=8, background=0, min_area=1, max_regions=1024):
    labels, table, head, box_regions, flag = decode.seg_regions_host(cm, None, connectivity, background, min_area, max_regions)
    ih, iw = cm.shape
    want, dropped = reference_regions(cm, connectivity, background, min_area)
    n = len(want)
    assert labels.dtype == np.int32 and labels.shape == cm.shape and table.dtype == RD and table.shape == (max_regions,)
    assert head.dtype == np.int32 and box_regions.shape == (0,) and box_regions.dtype == np.int32
    # the partition, renumbered by first pixel
    expect = np.zeros((ih, iw), np.int32)
    for i, r in enumerate(want):
        expect[r["lab"] == r["k"]] = i + 1
    assert np.array_equal(labels, expect)
    nrec = min(n, max_regions)
    assert head.tolist() == [n, nrec, int((expect > 0).sum()), dropped]
    assert flag == (decode.FLAG_REGIONS if n > max_regions else 0)
    assert not np.frombuffer(table[nrec:].tobytes(), np.uint8).any()
    sum_x = ndimage.sum(np.indices(cm.shape)[1], labels, np.arange(1, nrec + 1)) if nrec else []
    sum_y = ndimage.sum(np.indices(cm.shape)[0], labels, np.arange(1, nrec + 1)) if nrec else []
    for i, r in enumerate(want[:nrec]):
        rec = table[i]
        ys, xs = r["box"]
        assert (rec["cls"], rec["area"], rec["first"], rec["det"]) == (r["cls"], r["area"], r["first"], -1), i
        assert (rec["left"], rec["top"], rec["right"], rec["bottom"]) == (xs.start, ys.start, xs.stop, ys.stop), i
        assert (rec["sum_x"], rec["sum_y"]) == (int(sum_x[i]), int(sum_y[i])), i
        if r["ys"] is not None:                                   # the direct coordinate sums
            assert (rec["sum_x"], rec["sum_y"]) == (int(r["xs"].sum()), int(r["ys"].sum()))
    return n


@pytest.mark.parametrize("connectivity", [8, 4])
@pytest.mark.parametrize("size", SIZES)
@pytest.mark.parametrize("p,k", NOISE)
def test_noise_against_scipy(p, k, size, connectivity):
    n = check_against_scipy(noise(p, k, size), connectivity)
    if size in ((67, 131), BIG):
        assert n > 1024                                           # the prefix and the flag are exercised
    else:
        assert n <= 1024


@pytest.mark.parametrize("p,k", NOISE)
def test_min_area_and_a_large_table(p, k):
    cm = noise(p, k, BIG)
    kept = check_against_scipy(cm, 8, min_area=4)
    assert check_against_scipy(cm, 8, min_area=4, max_regions=4096) == kept
    assert (kept > 1024) == (k != 9) and kept <= 4096             # the first two overflow 1024 and fit 4096, the third fits both
    assert check_against_scipy(cm, 4, min_area=2, max_regions=7) > 7


def test_blobs_stay_under_capacity():
    cm = blobs()
    n = check_against_scipy(cm, 8)
    assert 100 < n < 1024
    assert check_against_scipy(cm, 4) >= n
    assert check_against_scipy(cm, 8, background=-1) > n          # class 0 is labelled too
    assert check_against_scipy(cm, 8, background=3) != 0


def test_background_minus_one_labels_every_class():
    cm = noise(0.5, 2, (67, 131))
    labels, _, head, _, _ = decode.seg_regions_host(cm, None, 8, background=-1, max_regions=4096)
    assert (labels > 0).all() and head[2] == cm.size and head[3] == 0
    check_against_scipy(cm, 8, background=-1, max_regions=4096)
    check_against_scipy(cm, 4, background=-1, max_regions=4096)
    check_against_scipy(np.full((5, 7), 255, np.uint8), 4, background=255)
    assert check_against_scipy(np.full((5, 7), 255, np.uint8), 4, background=-1) == 1


def test_patterns():
    assert check_against_scipy(checkerboard(), 8) == 1
    assert check_against_scipy(checkerboard(), 4, max_regions=4096) == 19500
    cm = serpentine()
    assert check_against_scipy(cm, 8) == 1 and check_against_scipy(cm, 4) == 1 and int(cm.sum()) == 19574
    for sign in (1, -1):
        for s in range(3):
            m = stripes(sign, s)
            n8 = check_against_scipy(m, 8)
            assert n8 == len(np.unique((np.indices(BIG)[1] + sign * np.indices(BIG)[0])[m > 0]))     # one region per stripe
            assert check_against_scipy(m, 4, max_regions=4096) == int(m.sum())
    assert check_against_scipy(comb(), 8) == 1 and check_against_scipy(comb(), 4) == 1
    assert check_against_scipy(u_shape(), 8) == 1 and check_against_scipy(u_shape(), 4) == 1
    assert check_against_scipy(np.zeros((9, 9), np.uint8)) == 0


def test_ids_follow_scipy_order_on_a_mask():
    """On a 0/1 mask the ids are scipy's own numbering: the rule's order is the order a caller of ndimage.label knows."""
    for p, k in NOISE[:1]:
        for connectivity in (4, 8):
            cm = noise(p, k, (67, 131)) == 1
            labels = decode.seg_regions_host(cm.astype(np.uint8), None, connectivity, max_regions=4096)[0]
            assert np.array_equal(labels, ndimage.label(cm, structure(connectivity))[0])


def test_record_layout():
    assert RD.itemsize == 48 and decode.REGION_HEAD == 4 and decode.FLAG_REGIONS == 131072
    names = ("cls", "area", "left", "top", "right", "bottom", "first", "det")
    assert RD.names == names + ("sum_x", "sum_y")
    assert [RD.fields[n][1] for n in names] == [4 * i for i in range(8)] and all(RD.fields[n][0] == np.dtype("<i4") for n in names)
    assert RD.fields["sum_x"] == (np.dtype("<i8"), 32) and RD.fields["sum_y"] == (np.dtype("<i8"), 40)
    rec = np.zeros(1, RD)
    rec["sum_x"], rec["det"] = 2 ** 40 + 5, -1
    assert np.frombuffer(rec.tobytes(), np.int32).tolist() == [0] * 7 + [-1, 5, 256, 0, 0]


# ---- the link ------------------------------------------------------------------------------------------------------------------
def brute_link(table, nrec, rows, size, det_to_seg=None):
    """Both directions with exact fractions: (det per record, region id per row)."""
    ih, iw = size

    def iou(a, b):
        w, h = min(a[2], b[2]) - max(a[0], b[0]), min(a[3], b[3]) - max(a[1], b[1])
        if w <= 0 or h <= 0:
            return None
        inter = w * h
        return Fraction(inter, (a[2] - a[0]) * (a[3] - a[1]) + (b[2] - b[0]) * (b[3] - b[1]) - inter)

    boxes = []
    for l, t, r, b, c in rows.tolist():
        l, r, t, b = min(max(l, 0), iw), min(max(r, 0), iw), min(max(t, 0), ih), min(max(b, 0), ih)
        boxes.append(None if r <= l or b <= t else (l, t, r, b))
    regions = [(int(x["left"]), int(x["top"]), int(x["right"]), int(x["bottom"])) for x in table[:nrec]]
    score = {}
    for i, box in enumerate(boxes):
        for j, reg in enumerate(regions):
            c = int(rows[i, 4])
            if det_to_seg is not None and (not 0 <= c < len(det_to_seg) or det_to_seg[c] != int(table[j]["cls"])):
                continue
            v = None if box is None else iou(box, reg)
            if v is not None:
                score[(i, j)] = v
    det = []
    for j in range(nrec):
        cand = [(score[(i, j)], -i) for i in range(len(boxes)) if (i, j) in score]
        det.append(-max(cand)[1] if cand else -1)
    box_regions = []
    for i in range(len(boxes)):
        cand = [(score[(i, j)], -j) for j in range(nrec) if (i, j) in score]
        box_regions.append(-max(cand)[1] + 1 if cand else 0)
    return det, box_regions


@pytest.mark.parametrize("gate", [None, (1, 2, 3, 4)])
def test_link_against_fractions(gate):
    cm = blobs((67, 131))
    rows = random_rows(3, 40, cm.shape)
    rows[5, 2] = rows[5, 0]                                       # empty
    rows[6, 3] = rows[6, 1] - 3                                   # bottom < top
    rows[7] = [-50, -40, 300, 200, 1]                             # larger than the image: clamped to it
    rows[8] = [131, 0, 200, 67, 1]                                # outside the image
    rows[9] = [-30, -30, 0, 0, 2]
    rows[10, 4] = 9                                               # a class the gate does not know
    rows[11, 4] = -1
    labels, table, head, box_regions, flag = decode.seg_regions_host(cm, rows, 8, det_to_seg=gate)
    plain = decode.seg_regions_host(cm, None, 8)
    assert np.array_equal(labels, plain[0]) and np.array_equal(head, plain[2]) and flag == plain[4] == 0
    det, want = brute_link(table, int(head[1]), rows, cm.shape, gate)
    assert table["det"][:head[1]].tolist() == det and box_regions.tolist() == want and box_regions.dtype == np.int32
    assert box_regions[[5, 6, 8, 9]].tolist() == [0, 0, 0, 0] and box_regions[7] != 0
    assert (np.array(det) >= 0).any() and (np.array(det) < 0).any() if gate else True
    if gate:
        assert box_regions[10] == 0 and box_regions[11] == 0
        linked = box_regions > 0
        assert (table["cls"][box_regions[linked] - 1] == np.array(gate)[rows[linked, 4]]).all()
    fields = [n for n in RD.names if n != "det"]
    assert np.array_equal(table[fields], plain[1][fields])        # the link changes nothing else


def test_link_ties_and_the_table_prefix():
    cm = np.zeros((12, 24), np.uint8)
    cm[2:6, 2:6] = 1                                              # region 1: box (2, 2, 6, 6)
    cm[2:6, 10:14] = 2                                            # region 2: box (10, 2, 14, 6)
    cm[8:10, 2:6] = 3                                             # region 3
    rows = np.array([[4, 2, 12, 6, 0],                            # overlaps regions 1 and 2 by 2 x 4 each: the tie goes to 1
                     [2, 2, 6, 6, 0], [2, 2, 6, 6, 0],            # twice the same box: region 1 takes the first
                     [10, 2, 14, 6, 1]], np.int32)
    labels, table, head, box_regions, flag = decode.seg_regions_host(cm, rows, 4)
    assert head.tolist() == [3, 3, 40, 0] and flag == 0
    assert box_regions.tolist() == [1, 1, 1, 2] and table["det"][:3].tolist() == [1, 3, -1]
    assert brute_link(table, 3, rows, cm.shape) == ([1, 3, -1], [1, 1, 1, 2])
    # with a table of one record only region 1 links; the labels do not change
    l1, t1, h1, b1, f1 = decode.seg_regions_host(cm, rows, 4, max_regions=1)
    assert np.array_equal(l1, labels) and h1.tolist() == [3, 1, 40, 0] and f1 == decode.FLAG_REGIONS
    assert b1.tolist() == [1, 1, 1, 0] and t1["det"].tolist() == [1]
    # no rows
    assert decode.seg_regions_host(cm, np.zeros((0, 5), np.int32))[3].shape == (0,)
    assert decode.seg_regions_host(cm)[1]["det"][:3].tolist() == [-1, -1, -1]
    # an equal fraction from different numbers: 8 / 24 against 4 / 12
    cm = np.zeros((10, 30), np.uint8)
    cm[0:4, 0:4] = 1
    cm[0:2, 10:14] = 1
    rows = np.array([[0, 0, 4, 6, 0], [10, 0, 12, 6, 0]], np.int32)             # I / U = 16 / 24 and 4 / 16
    _, table, _, box_regions, _ = decode.seg_regions_host(cm, rows, 4)
    assert box_regions.tolist() == [1, 2] and table["det"][:2].tolist() == [0, 1]


def test_region_text():
    cm = np.zeros((6, 9), np.uint8)
    cm[1:3, 2:5] = 4
    cm[4, 8] = 7
    rows = np.array([[8, 4, 9, 5, 0]], np.int32)
    _, table, head, _, _ = decode.seg_regions_host(cm, rows)
    assert decode.region_text(table[:head[1]]) == "1 4 6 2 1 5 3 3.0 1.5 -1\n2 7 1 8 4 9 5 8.0 4.0 0\n"
    assert decode.region_text(table[:0]) == ""


def test_argument_errors():
    cm = np.zeros((4, 4), np.uint8)
    for bad in (dict(connectivity=6), dict(connectivity=True), dict(background=-2), dict(background=256), dict(background=1.5),
                dict(min_area=0), dict(min_area=True), dict(max_regions=0), dict(max_regions=4097), dict(det_to_seg=[]),
                dict(det_to_seg=[1, 256]), dict(det_to_seg=[1, -1]), dict(det_to_seg=[[1, 2]]), dict(det_to_seg=[0.5]),
                dict(det_to_seg=list(range(256)) + [0]), dict(det_to_seg=3)):
        with pytest.raises(RuntimeError, match="seg_regions_host"):
            decode.seg_regions_host(cm, **bad)
        with pytest.raises(RuntimeError, match="somebody"):
            decode.check_region_params(bad, "somebody")
    for bad in (5, "yes", [8], dict(connectivty=4)):
        with pytest.raises(RuntimeError, match="somebody"):
            decode.check_region_params(bad, "somebody")
    with pytest.raises(RuntimeError, match="somebody"):
        decode.check_region_params(dict(det_to_seg=[1, 2, 3]), "somebody", num_classes=4)
    assert decode.check_region_params(dict(det_to_seg=[1, 2, 3, 4]), "x", num_classes=4)["det_to_seg"] == (1, 2, 3, 4)
    assert decode.check_region_params(True, "x") == decode.check_region_params(None, "x") == dict(
        connectivity=8, background=0, min_area=1, max_regions=1024, det_to_seg=None)
    assert decode.check_region_params(dict(connectivity=4, max_regions=4096, background=-1), "x")["max_regions"] == 4096
    for bad in (np.zeros((4, 4), np.int32), np.zeros((4,), np.uint8), np.zeros((0, 4), np.uint8), np.zeros((2, 4, 4), np.uint8)):
        with pytest.raises(RuntimeError, match="class map"):
            decode.seg_regions_host(bad)
    for bad in (np.zeros((2, 4), np.int32), np.zeros((2, 5), np.int64), np.zeros(5, np.int32)):
        with pytest.raises(RuntimeError, match="rows"):
            decode.seg_regions_host(cm, bad)
