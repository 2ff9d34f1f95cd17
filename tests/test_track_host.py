"""The host statement of the tracker, `data.track_update` (the rule csrc/track.hip equals bit for bit): against two
independent statements of the greedy matching -- all candidate pairs sorted by key and walked, and the mutually-best-pairs
form the kernel uses -- and on hand-built sequences for every step of the rule.  No GPU."""
import numpy as np
import pytest

from asy_vrnet_amd import data

F = np.float32
TD = data.TRACK_DTYPE


def rows_of(boxes, cls=0, cap=None):
    """(1, cap, 7) rows and kept from a list of (top, left, bottom, right) or (top, left, bottom, right, class)."""
    cap = max(len(boxes), 1) if cap is None else cap
    rows = np.zeros((1, cap, 7), F)
    for i, bx in enumerate(boxes):
        rows[0, i, :4] = bx[:4]
        rows[0, i, 4:6] = 0.9
        rows[0, i, 6] = bx[4] if len(bx) > 4 else cls
    return rows, np.array([len(boxes)], np.int32)


class Stream:
    """One stream through data.track_update."""

    def __init__(self, T=8, **params):
        self.params = data.check_track_params(dict(max_tracks=T, **params))
        self.table, self.head = np.zeros((1, T), TD), np.zeros((1, 4), np.int32)

    def step(self, boxes, cls=0, points=None, depth=None, cap=None):
        rows, kept = rows_of(boxes, cls, cap)
        bp = br = None
        if points is not None:
            bp, br = np.zeros(rows.shape[:2], np.int32), np.zeros(rows.shape[:2] + (2, 5), F)
            bp[0, :len(points)] = points
            br[0, :len(depth), 1, 0] = depth
            br[0, :len(depth), 0, 0] = 1.0                  # the nearest point: not what the tracker reads
        self.table, self.head, ids, self.flag = data.track_update(self.table, self.head, rows, kept, bp, br, self.params)
        return ids[0]

    @property
    def live(self):
        return self.table[0][self.table[0]["id"] != 0]


def test_record_layout_and_parameter_checks():
    assert TD.itemsize == 64 and TD.names == ("id", "cls", "hits", "misses", "row", "range_age", "x", "v")
    assert [TD.fields[n][1] for n in TD.names] == [0, 4, 8, 12, 16, 20, 24, 44]
    p = data.check_track_params(True)
    assert p == dict(max_tracks=64, max_age=5, iou=F(0.3), gain=(F(0.5), F(0.25)), range_gain=(F(0.5), F(0.25)))
    assert data.check_track_params(p) == p and data.check_track_params(None) == p
    assert data.check_track_params(dict(max_tracks=256, iou=1.0, max_age=0))["max_tracks"] == 256
    for bad in (dict(max_tracks=0), dict(max_tracks=257), dict(max_tracks=True), dict(iou=0.0), dict(iou=1.5), dict(iou=float("nan")),
                dict(max_age=-1), dict(max_age=1.5), dict(gain=0.5), dict(gain=(0.5, 3.0)), dict(range_gain=(0.5,)),
                dict(range_gain=(float("inf"), 0.1)), dict(speed=1), 3, "yes"):
        with pytest.raises(RuntimeError):
            data.check_track_params(bad)
    assert data.FLAG_TRACK_FULL == 32768


def scene(rs, T, n, ncls=2):
    """A random live table and rows with planted equal IoUs: integer boxes on a coarse grid, many of them copies."""
    def boxes(k):
        t, l = rs.randint(0, 6, k) * 4, rs.randint(0, 6, k) * 4
        return np.stack([t, l, t + rs.randint(1, 4, k) * 4, l + rs.randint(1, 4, k) * 4], 1).astype(F)
    table = np.zeros((1, T), TD)
    live = rs.rand(T) < 0.8
    table["id"][0] = np.where(live, np.arange(1, T + 1), 0)
    table["x"][0, :, :4] = np.where(live[:, None], boxes(T), 0)
    table["cls"][0] = np.where(live, rs.randint(0, ncls, T), 0)
    table["hits"][0] = live
    table["range_age"][0] = np.where(live, -1, 0)
    z = boxes(n)
    for i in range(n):                                      # copies of track boxes and of each other: exact ties
        if rs.rand() < 0.3 and live.any():
            z[i] = table["x"][0, rs.choice(np.flatnonzero(live)), :4]
        elif i and rs.rand() < 0.3:
            z[i] = z[rs.randint(i)]
    rows = np.zeros((1, n, 7), F)
    rows[0, :, :4], rows[0, :, 6] = z, rs.randint(0, ncls, n)
    return table, rows


def candidates(table, rows, thr):
    """(key, slot, row) of every candidate pair of stream 0, from data.track_iou / data.track_key."""
    tab, z, cls = table[0], rows[0, :, :4], data.track_class(rows[0, :, 6])
    iou = data.track_iou(tab["x"][:, :4], z)
    out = []
    for s in np.flatnonzero(tab["id"] != 0):
        for i in range(len(z)):
            if tab["cls"][s] == cls[i] and iou[s, i] >= thr:
                out.append((int(data.track_key(iou[s, i], s, i)), int(s), i))
    return out


def greedy_sorted(cands, T, n):
    slot_row, row_slot = [-1] * T, [-1] * n
    for _, s, i in sorted(cands, reverse=True):
        if slot_row[s] < 0 and row_slot[i] < 0:
            slot_row[s], row_slot[i] = i, s
    return slot_row


def greedy_mutual(cands, T, n):
    slot_row, row_slot, rounds = [-1] * T, [-1] * n, 0
    while True:
        best_s, best_r = {}, {}
        for key, s, i in cands:
            if slot_row[s] < 0 and row_slot[i] < 0:
                best_s[s], best_r[i] = max(best_s.get(s, 0), key), max(best_r.get(i, 0), key)
        new = [(s, i) for key, s, i in cands if best_s.get(s) == key and best_r.get(i) == key]
        if not new:
            return slot_row, rounds
        rounds += 1
        for s, i in new:
            slot_row[s], row_slot[i] = i, s


def test_greedy_matching_equals_the_sorted_walk_and_the_mutually_best_form():
    rs = np.random.RandomState(3)
    params = data.check_track_params(dict(iou=0.25))
    ties = matched = 0
    for _ in range(200):
        T, n = rs.randint(1, 13), rs.randint(1, 17)
        table, rows = scene(rs, T, n)
        cands = candidates(table, rows, params["iou"])
        ious = [k >> 32 for k, _, _ in cands]
        ties += len(ious) - len(set(ious))
        want = greedy_sorted(cands, T, n)
        assert greedy_mutual(cands, T, n)[0] == want
        got, _, ids, _ = data.track_update(table, np.zeros((1, 4), np.int32), rows, np.array([n], np.int32), params=params)
        # v = 0 in the scene, so prediction moves nothing; `row` of a live slot is its match
        live = table[0]["id"] != 0
        assert [int(r) for r in got[0]["row"][live]] == [want[s] for s in np.flatnonzero(live)]
        for s in np.flatnonzero(live):
            if want[s] >= 0:
                assert ids[0, want[s]] == table[0]["id"][s]
        matched += sum(w >= 0 for w in want)
    assert ties > 200 and matched > 200                     # the planted ties are there


def test_constant_translation_keeps_one_id_and_the_rates_converge():
    st = Stream()
    step = np.array([1.5, -2.0, 1.5, -2.0], F)
    box = np.array([40, 300, 80, 360], F)
    for k in range(60):
        ids = st.step([box + k * step])
        assert list(ids) == [1]
    (t,) = st.live
    assert t["hits"] == 60 and t["misses"] == 0 and t["row"] == 0 and st.head[0].tolist() == [1, 1, 60, 0]
    assert np.abs(t["v"][:4] - step).max() < 1e-3 and np.abs(t["x"][:4] - (box + 59 * step)).max() < 1e-2


def test_ids_are_never_reused_and_slots_are():
    st = Stream(T=2, max_age=0)
    a, b, c = (0, 0, 10, 10), (50, 50, 60, 60), (100, 100, 110, 110)
    assert list(st.step([a, b])) == [1, 2]
    assert list(st.step([a])) == [1] and st.table[0]["id"].tolist() == [1, 0]     # b is freed: max_age 0
    assert list(st.step([a, c])) == [1, 3] and st.table[0]["id"].tolist() == [1, 3]
    # freed and re-taken in ONE call: a and c vanish, two new boxes take their slots
    assert list(st.step([b, (200, 200, 210, 210)])) == [4, 5] and st.table[0]["id"].tolist() == [4, 5]
    assert st.head[0].tolist() == [5, 2, 4, 2] and st.flag == 0


def test_a_track_survives_exactly_max_age_empty_calls():
    st = Stream(max_age=3)
    st.step([(10, 10, 30, 30)])
    for k in range(3):
        st.step([])
        (t,) = st.live
        assert t["misses"] == k + 1 and t["row"] == -1 and t["id"] == 1
    st.step([])
    assert len(st.live) == 0 and not np.frombuffer(st.table.tobytes(), np.uint8).any() and st.head[0].tolist() == [1, 0, 5, 0]


def test_equal_ious_go_to_the_lowest_slot_then_the_lowest_row():
    st = Stream()
    box = (10, 10, 30, 30)
    assert list(st.step([box, box])) == [1, 2]              # two tracks on one box (the NMS would not let that through)
    ids = st.step([(40, 40, 50, 50), box, box])
    assert list(ids) == [3, 1, 2]                           # slot 0 takes the lower of the two equal rows
    st = Stream()
    st.step([(10, 10, 30, 30), (10, 20, 30, 40)])           # row (10, 15, 30, 35) overlaps both by the same IoU
    assert list(st.step([(10, 15, 30, 35)])) == [1] and st.table[0]["row"][:2].tolist() == [0, -1]


def test_a_pair_at_the_threshold_matches_and_one_below_does_not():
    # IoU of (0, 0, 4, 4) and (0, 2, 4, 6) is 8 / 24; float32(1/3) is what the rule computes
    thr = float(data.track_iou(np.array([[0, 0, 4, 4]], F), np.array([[0, 2, 4, 6]], F))[0, 0])
    st = Stream(iou=thr)
    st.step([(0, 0, 4, 4)])
    assert list(st.step([(0, 2, 4, 6)])) == [1]
    st = Stream(iou=float(np.nextafter(F(thr), F(1))))
    st.step([(0, 0, 4, 4)])
    assert list(st.step([(0, 2, 4, 6)])) == [2]


def test_a_class_mismatch_with_the_largest_iou_does_not_match():
    st = Stream()
    st.step([(10, 10, 30, 30, 1)])
    ids = st.step([(10, 10, 30, 30, 2), (12, 12, 32, 32, 1)])
    assert list(ids) == [2, 1] and st.table[0]["cls"][:2].tolist() == [1, 2]


def test_nan_and_inverted_rows_neither_match_nor_give_birth():
    st = Stream()
    st.step([(10, 10, 30, 30)])
    nan, inf = float("nan"), float("inf")
    bad = [(10, 10, nan, 30), (10, 10, 10, 30), (30, 10, 10, 30), (10, 30, 30, 10), (10, -inf, 30, inf), (10, 10, 30, 30)]
    ids = st.step(bad)
    assert list(ids) == [0, 0, 0, 0, 0, 1] and len(st.live) == 1 and st.head[0].tolist() == [1, 1, 2, 0]
    # a track whose prediction leaves the finite numbers is freed before the matching
    st.table["v"][0, 0, 2] = F(3e38)
    st.table["x"][0, 0, 2] = F(3e38)
    assert list(st.step([(10, 10, 30, 30)])) == [2] and st.table[0]["id"].tolist()[:2] == [2, 0]
    # a class that is no integer of 32 bits reads as -1
    assert data.track_class(np.array([nan, 3e9, -3e9, 2.9, -2.9, -2147483648.0], F)).tolist() == [-1, -1, -1, 2, -2, -2147483648]


def test_the_range_filter():
    st = Stream()
    box = (10, 10, 30, 30)
    st.step([box], points=[0], depth=[50.0])                # a birth without points: no range yet
    (t,) = st.live
    assert t["range_age"] == -1 and t["x"][4] == 0 and t["v"][4] == 0
    st.step([box], points=[3], depth=[20.0])                # the first hit sets it
    (t,) = st.live
    assert t["range_age"] == 0 and t["x"][4] == 20 and t["v"][4] == 0
    st.step([box], points=[3], depth=[24.0])                # later hits filter: r = 4, x = 20 + 0.5 * 4, v = 0.25 * 4
    (t,) = st.live
    assert t["range_age"] == 0 and t["x"][4] == 22 and t["v"][4] == 1
    st.step([box], points=[0], depth=[99.0])                # no points: the range is predicted only, x = 22 + 1
    (t,) = st.live
    assert t["range_age"] == 1 and t["x"][4] == 23 and t["v"][4] == 1
    st.step([box], points=[2], depth=[float("nan")])        # a NaN depth is no update either
    st.step([])                                             # coasting counts on
    (t,) = st.live
    assert t["range_age"] == 3 and t["x"][4] == 25 and t["misses"] == 1
    st.step([box])                                          # no radar pair at all: predicted only
    (t,) = st.live
    assert t["range_age"] == 4 and t["x"][4] == 26
    st = Stream()
    st.step([box], points=[5], depth=[12.5])                # a birth with points takes its range at once
    (t,) = st.live
    assert t["range_age"] == 0 and t["x"][4] == 12.5 and t["hits"] == 1


def test_a_full_table_gives_id_zero_and_the_flag():
    st = Stream(T=2)
    boxes = [(0, 0, 10, 10), (20, 20, 30, 30), (40, 40, 50, 50)]
    assert list(st.step(boxes, cap=5)) == [1, 2, 0, 0, 0] and st.flag == data.FLAG_TRACK_FULL and st.head[0].tolist() == [2, 2, 1, 2]
    assert list(st.step(boxes[:2], cap=5)) == [1, 2, 0, 0, 0] and st.flag == 0
    # kept outside [0, cap] is clamped and flagged
    rows, _ = rows_of(boxes)
    _, _, ids, flag = data.track_update(st.table, st.head, rows, np.array([7], np.int32), params=st.params)
    assert flag == 512 | data.FLAG_TRACK_FULL and list(ids[0]) == [1, 2, 0]
    _, head, ids, flag = data.track_update(st.table, st.head, rows, np.array([-1], np.int32), params=st.params)
    assert flag == 512 and not ids.any() and head[0].tolist() == [2, 2, 3, 0]


def test_track_text_and_argument_errors():
    st = Stream()
    st.step([(1.5, 2, 30, 40, 3)], points=[1], depth=[7.25])
    assert data.track_text(st.table[0]) == "1 3 1 0 1.5 2 30 40 7.25 0\n" and data.track_text(np.zeros(3, TD)) == ""
    rows, kept = rows_of([(0, 0, 1, 1)])
    with pytest.raises(RuntimeError, match="TRACK_DTYPE"):
        data.track_update(np.zeros((1, 4, 16), np.int32), st.head, rows, kept)
    with pytest.raises(RuntimeError, match="head"):
        data.track_update(st.table, np.zeros((1, 3), np.int32), rows, kept)
    with pytest.raises(RuntimeError, match="come together"):
        data.track_update(st.table, st.head, rows, kept, box_points=np.zeros((1, 1), np.int32))
    with pytest.raises(RuntimeError, match="TRACK_DTYPE"):
        data.track_text(np.zeros(3, np.int32))
