"""The detection metric (csrc/detmap.hip, metrics.voc_map / DetectionEvaluator / read_map_dir / get_map): a literal
sequential Python restatement of utils/utils_map.py `get_map` (:276-798: `used` flags mutated in confidence order,
Python-float arithmetic, `voc_ap` :95-136, `log_average_miss_rate` :31-67), pinned on the reference's own values
(tests/golden/detmap_small.npz, tools/make_golden_detmap.py), then the HIP path against it.

Tolerances (none of them taken from what the kernels give):
  order, tp, fp, rec, prec, n_gt, n_det, n_tp   bit-equal: integer-valued or plain fp64 boxes, IEEE fp64 operations in the
                                                reference's operand order, integer scans
  ap                                            1e-9 absolute: the order of an fp64 sum of at most D terms in [0, 1],
                                                bounded by D * 2^-53 ~ 1e-10 at D = 10^6
  lamr, f1, recall, precision, map              1e-9 absolute: device exp / log against numpy's
  restatement against the reference             lists equal element for element, ap / lamr / mAP within 1e-12"""
import math
import os

import numpy as np
import pytest
import torch

from asy_vrnet_amd import metrics
from asy_vrnet_amd.metrics import DetectionEvaluator, format_detections, get_map, read_map_dir, voc_map

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "detmap_small.npz")
ARRAYS = ("det_image", "det_label", "det_score", "det_box", "gt_image", "gt_label", "gt_box", "gt_difficult")
TOL = 1e-9


# ---- the restatement --------------------------------------------------------------------------------------------------

def voc_ap_restated(rec, prec):
    """utils_map.py:95-136."""
    mrec = [0.0] + list(rec) + [1.0]
    mpre = [0.0] + list(prec) + [0.0]
    for i in range(len(mpre) - 2, -1, -1):
        mpre[i] = max(mpre[i], mpre[i + 1])
    ap = 0.0
    for i in range(1, len(mrec)):
        if mrec[i] != mrec[i - 1]:
            ap += (mrec[i] - mrec[i - 1]) * mpre[i]
    return ap


def lamr_restated(rec, cfp, n_images):
    """utils_map.py:31-67 as get_map calls it (:599): the `precision` argument is the RECALL list."""
    rec, cfp = np.array(rec, dtype=np.float64), np.array(cfp, dtype=np.float64)
    if rec.size == 0:
        return 0.0
    fppi_tmp = np.insert(cfp / float(n_images), 0, -1.0)
    mr_tmp = np.insert(1 - rec, 0, 1.0)
    ref = np.logspace(-2.0, 0.0, num=9)
    for i, ref_i in enumerate(ref):
        ref[i] = mr_tmp[np.where(fppi_tmp <= ref_i)[-1][-1]]
    return math.exp(np.mean(np.log(np.maximum(1e-10, ref))))


def get_map_restated(det_image, det_label, det_score, det_box, gt_image, gt_label, gt_box, gt_difficult, num_classes,
                     min_overlap, score_threhold=0.5):
    """utils_map.py:276-798 on flat arrays, sequentially: per class the detections in a stable descending sort (:416), each
    compared with every ground truth of its image and class in input order (:462-477), `used` flags set in that order
    (:482-498).  Classes without a non-difficult ground truth are not evaluated by the reference: their curves are still
    restated (tp is then always 0) and their ap / f1 / recall / precision / lamr are NaN."""
    det_box, gt_box = np.asarray(det_box, dtype=np.float64).reshape(-1, 4), np.asarray(gt_box, dtype=np.float64).reshape(-1, 4)
    score = [float(s) for s in det_score]
    groups, n_gt, images_of = {}, [0] * num_classes, [set() for _ in range(num_classes)]
    for g in range(len(gt_label)):
        i, c, d = int(gt_image[g]), int(gt_label[g]), bool(gt_difficult[g])
        groups.setdefault((i, c), []).append({"bbox": [float(v) for v in gt_box[g]], "used": False, "difficult": d})
        if not d:
            n_gt[c] += 1
            images_of[c].add(i)
    by_class = [[] for _ in range(num_classes)]
    for d in range(len(det_label)):
        by_class[int(det_label[d])].append(d)
    out = {k: [] for k in ("order", "tp", "fp", "rec", "prec", "score", "ap", "f1", "recall", "precision", "lamr", "n_tp")}
    for c in range(num_classes):
        order = sorted(by_class[c], key=lambda d: score[d], reverse=True)
        nd = len(order)
        tp, fp, idx_thr = [0] * nd, [0] * nd, 0
        for idx, d in enumerate(order):
            if score[d] >= score_threhold:
                idx_thr = idx
            ovmax, gt_match = -1, -1
            bb = [float(v) for v in det_box[d]]
            for obj in groups.get((int(det_image[d]), c), ()):
                bbgt = obj["bbox"]
                bi = [max(bb[0], bbgt[0]), max(bb[1], bbgt[1]), min(bb[2], bbgt[2]), min(bb[3], bbgt[3])]
                iw = bi[2] - bi[0] + 1
                ih = bi[3] - bi[1] + 1
                if iw > 0 and ih > 0:
                    ua = (bb[2] - bb[0] + 1) * (bb[3] - bb[1] + 1) + (bbgt[2] - bbgt[0] + 1) * (bbgt[3] - bbgt[1] + 1) - iw * ih
                    ov = iw * ih / ua
                    if ov > ovmax:
                        ovmax, gt_match = ov, obj
            if ovmax >= min_overlap:
                if not gt_match["difficult"]:
                    if not gt_match["used"]:
                        tp[idx] = 1
                        gt_match["used"] = True
                    else:
                        fp[idx] = 1
            else:
                fp[idx] = 1
        ctp, cfp = list(np.cumsum(tp, dtype=np.int64)), list(np.cumsum(fp, dtype=np.int64))
        rec = [float(ctp[k]) / max(n_gt[c], 1) for k in range(nd)]
        prec = [float(ctp[k]) / max(int(cfp[k] + ctp[k]), 1) for k in range(nd)]
        out["order"] += order
        out["tp"] += tp
        out["fp"] += fp
        out["rec"] += rec
        out["prec"] += prec
        out["score"] += [score[d] for d in order]
        out["n_tp"].append(int(ctp[-1]) if nd else 0)
        if n_gt[c] == 0:
            vals = [float("nan")] * 5
        elif nd == 0:
            vals = [voc_ap_restated([], []), 0.0, 0.0, 0.0, 0.0]
        else:
            den = prec[idx_thr] + rec[idx_thr]
            vals = [voc_ap_restated(rec, prec), rec[idx_thr] * prec[idx_thr] * 2 / (1 if den == 0 else den), rec[idx_thr],
                    prec[idx_thr], lamr_restated(rec, cfp, len(images_of[c]))]
        for k, v in zip(("ap", "f1", "recall", "precision", "lamr"), vals):
            out[k].append(v)
    sum_ap, n_classes = 0.0, 0
    for c in range(num_classes):
        if n_gt[c] > 0:
            sum_ap += out["ap"][c]
            n_classes += 1
    res = {k: np.array(v, dtype=np.float64) for k, v in out.items()}
    res.update(order=np.array(out["order"], dtype=np.int64), tp=np.array(out["tp"], dtype=np.uint8),
               fp=np.array(out["fp"], dtype=np.uint8), n_tp=np.array(out["n_tp"], dtype=np.int32),
               n_gt=np.array(n_gt, dtype=np.int32), n_det=np.array([len(b) for b in by_class], dtype=np.int32),
               offsets=np.concatenate([[0], np.cumsum([len(b) for b in by_class])]).astype(np.int32),
               map=sum_ap / n_classes if n_classes else 0.0)
    return res


# ---- inputs -----------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def golden():
    return np.load(GOLDEN)


def fixture_set(golden, s):
    arr = {k: golden[f"s{s}_{k}"] for k in ARRAYS}
    return arr, [str(n) for n in golden[f"s{s}_names"]]


def random_case(seed, n_images, dets_per_image, num_classes=20, integer=True):
    """Seeded synthetic set: ground truths, jittered (sometimes duplicated, sometimes wrong-class) detections on them and
    boxes on nothing; skewed classes, 15 % difficult, scores to three decimals (ties), classes without detections /
    without ground truths."""
    rng = np.random.default_rng(seed)
    n_gt = rng.integers(0, 13, n_images)
    gt_image = np.repeat(np.arange(n_images), n_gt)
    G = len(gt_image)
    skew = lambda n: np.minimum((rng.random(n) ** 2 * (num_classes - 2)).astype(np.int64), num_classes - 3)   # never the last two
    gt_label = skew(G)
    lt = rng.integers(0, 400, (G, 2)).astype(np.float64)
    gt_box = np.concatenate([lt, lt + rng.integers(8, 120, (G, 2))], axis=1)
    gt_difficult = (rng.random(G) < 0.15).astype(np.uint8)
    D = n_images * dets_per_image
    det_image = np.sort(rng.integers(0, n_images, D))
    # 70 % of the detections of an image with ground truths sit on one of them
    first = np.concatenate([[0], np.cumsum(n_gt)])[:-1]
    has = n_gt[det_image] > 0
    src = np.where(has, first[det_image] + rng.integers(0, 1 << 30, D) % np.maximum(n_gt[det_image], 1), 0)
    on_gt = (rng.random(D) < 0.7) & has
    rnd_lt = rng.integers(0, 400, (D, 2)).astype(np.float64)
    rnd_box = np.concatenate([rnd_lt, rnd_lt + rng.integers(8, 120, (D, 2))], axis=1)
    jitter = rng.integers(-8, 9, (D, 4)).astype(np.float64)
    det_box = np.where(on_gt[:, None], gt_box[src] + jitter, rnd_box)
    det_label = np.where(on_gt & (rng.random(D) < 0.9), gt_label[src], skew(D))
    det_label = np.where(rng.random(D) < 0.01, num_classes - 1, det_label)          # a class without ground truths
    det_label = np.where(det_label == 3, 4, det_label)                              # class 3: ground truths, no detections
    det_score = np.round(rng.random(D), 3)
    if not integer:
        gt_box = gt_box + rng.random(gt_box.shape)
        det_box = det_box + rng.random(det_box.shape)
    return dict(det_image=det_image, det_label=det_label, det_score=det_score, det_box=det_box, gt_image=gt_image,
                gt_label=gt_label, gt_box=gt_box, gt_difficult=gt_difficult)


EXACT = ("order", "tp", "fp", "rec", "prec", "score", "offsets", "n_gt", "n_det", "n_tp")
CLOSE = ("ap", "f1", "recall", "precision", "lamr", "map")


def to_numpy(res):
    return {k: res[k].cpu().numpy() for k in res.keys()}


def assert_matches(got, want, where):
    """got: voc_map(..., return_curves=True) at one threshold, read back; want: the restatement.  Every detection is
    compared.  Prints each figure before it asserts."""
    for k in EXACT:
        g, w = np.asarray(got[k]), np.asarray(want[k])
        assert g.shape == w.shape, (where, k, g.shape, w.shape)
        same = np.array_equal(g, w)
        print(f"{where}: {k}: {g.size} values, {'bit-equal' if same else int((g != w).sum())}")
        assert same, (where, k, np.flatnonzero(g != w)[:10])
    for k in CLOSE:
        g, w = np.asarray(got[k], dtype=np.float64), np.asarray(want[k], dtype=np.float64)
        assert g.shape == w.shape, (where, k, g.shape, w.shape)
        assert np.array_equal(np.isnan(g), np.isnan(w)), (where, k, g, w)
        err = float(np.nanmax(np.abs(g - w))) if np.any(~np.isnan(w)) else 0.0
        print(f"{where}: {k}: max abs error {err:.3e}")
        assert err <= TOL, (where, k, err)


# ---- CPU: the restatement against the reference, the parser, the row formatting -----------------------------------------

def test_restatement_matches_reference(golden):
    for s in range(int(golden["n_sets"])):
        arr, names = fixture_set(golden, s)
        for j, thr in enumerate(golden["thresholds"]):
            r = get_map_restated(**arr, num_classes=len(names), min_overlap=float(thr))
            key = lambda k: golden[f"s{s}_t{j}_{k}"]
            evaluated = [int(c) for c in key("cls")]
            assert evaluated == [c for c in range(len(names)) if r["n_gt"][c] > 0]
            off = r["offsets"]
            rec = np.concatenate([r["rec"][off[c]:off[c + 1]] for c in evaluated])
            prec = np.concatenate([r["prec"][off[c]:off[c + 1]] for c in evaluated])
            assert [int(off[c + 1] - off[c]) for c in evaluated] == key("len").tolist()
            assert np.array_equal(rec, key("rec")) and np.array_equal(prec, key("prec")), (s, thr)
            assert np.abs(r["ap"][evaluated] - key("ap")).max() <= 1e-12
            assert np.abs(r["lamr"][evaluated] - key("lamr")).max() <= 1e-12
            assert abs(r["map"] - float(key("map"))) <= 1e-12
            # results.txt reports the tp count per detected class, keyed by the first token of the name: -1 = not reported
            reported = key("tp") >= 0
            assert reported.sum() >= 4 and np.array_equal(r["n_tp"][reported], key("tp")[reported]), (s, thr)
            # every class: the count is the last cumulative tp, which the recall list pins
            for c in evaluated:
                if off[c + 1] > off[c]:
                    assert r["n_tp"][c] == round(r["rec"][off[c + 1] - 1] * r["n_gt"][c])


def test_restatement_hand_built_cases():
    # IoU exactly at the threshold is a match (>=): det 0 0 9 9 on gt 0 0 9 19 is 100 / 200
    one = dict(det_image=[0], det_label=[0], det_score=[0.9], det_box=[[0, 0, 9, 9]], gt_image=[0], gt_label=[0],
               gt_box=[[0, 0, 9, 19]], gt_difficult=[0])
    assert get_map_restated(**one, num_classes=1, min_overlap=0.5)["tp"].tolist() == [1]
    assert get_map_restated(**one, num_classes=1, min_overlap=0.5000001)["tp"].tolist() == [0]
    # the best match is difficult: neither tp nor fp, although the non-difficult box passes too; a duplicate is an fp
    two = dict(det_image=[0, 0, 0], det_label=[0, 0, 0], det_score=[0.8, 0.7, 0.6],
               det_box=[[10, 10, 50, 50], [12, 12, 52, 52], [13, 13, 52, 52]], gt_image=[0, 0], gt_label=[0, 0],
               gt_box=[[10, 10, 50, 50], [12, 12, 52, 52]], gt_difficult=[1, 0])
    r = get_map_restated(**two, num_classes=1, min_overlap=0.5)
    assert r["tp"].tolist() == [0, 1, 0] and r["fp"].tolist() == [0, 0, 1] and r["n_gt"].tolist() == [1]
    assert r["ap"][0] == 1.0 and r["map"] == 1.0


def test_read_map_dir_on_the_fixture_text(golden, tmp_path):
    os.makedirs(tmp_path / "ground-truth")
    os.makedirs(tmp_path / "detection-results")
    for iid, g, d in zip(golden["s0_ids"], golden["s0_gt_text"], golden["s0_dr_text"]):
        (tmp_path / "ground-truth" / f"{iid}.txt").write_text(str(g))
        (tmp_path / "detection-results" / f"{iid}.txt").write_text(str(d))
    data = read_map_dir(str(tmp_path))
    arr, names = fixture_set(golden, 0)
    assert data["class_names"] == names and data["image_ids"] == [str(i) for i in golden["s0_ids"]]
    assert "traffic light" in names and arr["gt_difficult"].any()
    for k in ARRAYS:
        assert np.array_equal(np.asarray(data[k], dtype=np.float64), arr[k].astype(np.float64)), k
    os.remove(tmp_path / "detection-results" / f"{golden['s0_ids'][0]}.txt")
    with pytest.raises(RuntimeError):
        read_map_dir(str(tmp_path))
    with pytest.raises(RuntimeError):
        get_map(0.5, True, path=str(tmp_path))


def test_row_formatting_is_get_map_txt():
    """utils/callbacks.py:151-170 restated by hand on a few rows: top, left, bottom, right, obj, class_conf, class_pred."""
    rows = np.array([[12.9, 3.2, 80.7, 41.5, 0.5, 0.246913578, 2],          # score 0.123456789 -> '0.1234'
                     [-3.7, 0.9, 10.2, 9.99, 0.9, 0.9, 0],                   # int() truncates towards zero: -3
                     [5.0, 6.0, 7.0, 8.0, 1.0, 1e-5, 1],                     # '1e-05'
                     [1.5, 2.5, 3.5, 4.5, 0.99999, 0.99999, 1]], dtype=np.float32)
    top_conf = rows[:, 4] * rows[:, 5]
    want = []
    for i in np.argsort(top_conf)[::-1][:3]:
        top, left, bottom, right = rows[i, :4]
        line = "%s %s %s %s %s" % (str(top_conf[i])[:6], str(int(left)), str(int(top)), str(int(right)), str(int(bottom)))
        want.append((int(np.array(rows[:, 6], dtype="int32")[i]), [float(v) for v in line.split()]))
    label, score, box = format_detections(rows, max_boxes=3)
    assert label.tolist() == [w[0] for w in want] == [1, 0, 2]
    assert score.tolist() == [w[1][0] for w in want] == [0.9999, 0.8099, 0.1234]
    assert box.tolist() == [w[1][1:] for w in want] and box[1].tolist() == [0.0, -3.0, 9.0, 10.0] and box[2, 1] == 12.0
    assert float(str(np.float32(1e-5))[:6]) == 1e-5 == format_detections(rows[2:3])[1][0]
    ev = DetectionEvaluator(["a", "b", "c"], max_boxes=3)
    ev.add("b", rows, np.array([[1, 2, 30, 40, 2]]))
    ev.add("a", None, np.zeros((0, 5), dtype=np.int64))
    a = ev.arrays()
    assert a["det_image"].tolist() == [1, 1, 1] and a["gt_image"].tolist() == [1] and a["gt_box"].tolist() == [[1, 2, 30, 40]]
    assert a["det_score"].tolist() == score.tolist() and a["det_label"].tolist() == [1, 0, 2]
    with pytest.raises(RuntimeError):
        ev.add("a", None, np.zeros((0, 5), dtype=np.int64))
    ev.reset()
    assert len(ev.arrays()["det_score"]) == 0


def test_voc_map_argument_errors():
    one = random_case(1, 3, 4, num_classes=5)
    with pytest.raises(RuntimeError):
        voc_map(**one, num_classes=5, device="cpu")                   # no CPU fallback
    assert "vrnet_det_map_f64" in metrics.hip.EXPORTED and "vrnet_det_map_workspace_bytes" in metrics.hip.EXPORTED
    assert metrics.hip._lib.vrnet_det_map_workspace_bytes(1000, 100, 2) >= 4 * 2 * 100 + 8 * 2 * 1000


# ---- GPU --------------------------------------------------------------------------------------------------------------

gpu = pytest.mark.gpu


def run_and_compare(arr, num_classes, thr, where, score_threhold=0.5):
    got = to_numpy(voc_map(**arr, num_classes=num_classes, min_overlap=thr, score_threhold=score_threhold, return_curves=True))
    want = get_map_restated(**arr, num_classes=num_classes, min_overlap=thr, score_threhold=score_threhold)
    assert_matches(got, want, where)
    return got


@gpu
def test_voc_map_matches_restatement_on_the_fixture(golden):
    for s in range(int(golden["n_sets"])):
        arr, names = fixture_set(golden, s)
        for j, thr in enumerate(golden["thresholds"]):
            got = run_and_compare(arr, len(names), float(thr), f"set {s} thr {thr}")
            assert abs(float(got["map"]) - float(golden[f"s{s}_t{j}_map"])) <= TOL          # and the reference's own mAP
            ev = [int(c) for c in golden[f"s{s}_t{j}_cls"]]
            assert np.abs(got["ap"][ev] - golden[f"s{s}_t{j}_ap"]).max() <= TOL
            assert np.abs(got["lamr"][ev] - golden[f"s{s}_t{j}_lamr"]).max() <= TOL


@gpu
def test_voc_map_matches_restatement_on_a_large_case():
    arr = random_case(20261017, 2000, 55)
    assert len(arr["det_score"]) >= 100000 and arr["det_image"].max() + 1 >= 2000
    counts = np.bincount(arr["det_label"], minlength=20)
    assert counts.max() > 8 * 512            # several chunks and carries in the curve kernel
    got = run_and_compare(arr, 20, 0.5, "large thr 0.5")
    # the case is not a trivial one: over 5 % of the detections are true positives, some sit on difficult ground truths
    assert got["tp"].sum() > len(arr["det_score"]) // 20 and (got["tp"] + got["fp"] == 0).sum() > 100
    run_and_compare(arr, 20, 0.75, "large thr 0.75", score_threhold=0.3)


@gpu
def test_threshold_list_equals_single_calls(golden):
    arr, names = fixture_set(golden, 2)
    thr = [0.3, 0.5, 0.75, 0.5]
    many = to_numpy(voc_map(**arr, num_classes=len(names), min_overlap=thr, return_curves=True))
    assert many["map"].shape == (4,) and many["ap"].shape == (4, len(names)) and many["tp"].shape == (4, len(arr["det_score"]))
    assert many["order"].shape == many["tp"].shape and many["score"].shape == (len(arr["det_score"]),)
    for t, v in enumerate(thr):
        one = to_numpy(voc_map(**arr, num_classes=len(names), min_overlap=v, return_curves=True))
        for k in one:
            a, b = many[k] if k in ("score", "offsets") else many[k][t], one[k]
            assert a.shape == b.shape and a.tobytes() == b.tobytes(), (k, v)


@gpu
def test_degenerate_inputs():
    base = random_case(5, 30, 12, num_classes=6)
    none_det = dict(base, det_image=np.zeros(0, np.int64), det_label=np.zeros(0, np.int64), det_score=np.zeros(0),
                    det_box=np.zeros((0, 4)))
    got = run_and_compare(none_det, 6, 0.5, "no detections")
    assert float(got["map"]) == 0.0 and got["n_det"].sum() == 0
    none_gt = dict(base, gt_image=np.zeros(0, np.int64), gt_label=np.zeros(0, np.int64), gt_box=np.zeros((0, 4)),
                   gt_difficult=np.zeros(0, np.uint8))
    got = run_and_compare(none_gt, 6, 0.5, "no ground truths")
    assert float(got["map"]) == 0.0 and np.isnan(got["ap"]).all() and got["fp"].all()
    nothing = dict(none_det, **{k: none_gt[k] for k in ("gt_image", "gt_label", "gt_box", "gt_difficult")})
    got = run_and_compare(nothing, 6, 0.5, "nothing at all")
    assert float(got["map"]) == 0.0
    one_class = random_case(6, 40, 20, num_classes=4)
    for k in ("det_label", "gt_label"):
        one_class[k] = np.zeros_like(one_class[k])
    run_and_compare(one_class, 1, 0.5, "one class")
    run_and_compare(random_case(7, 200, 30, num_classes=8, integer=False), 8, 0.5, "fractional boxes")
    no_difficult = dict(base)
    no_difficult.pop("gt_difficult")
    got = to_numpy(voc_map(**no_difficult, num_classes=6, return_curves=True))
    assert_matches(got, get_map_restated(**dict(base, gt_difficult=np.zeros_like(base["gt_difficult"])), num_classes=6,
                                         min_overlap=0.5), "gt_difficult=None")
    with pytest.raises(RuntimeError):
        voc_map(**base, num_classes=3)                                 # class ids outside [0, 3)
    with pytest.raises(RuntimeError):
        voc_map(**base, num_classes=6, min_overlap=[0.5] * 17)


@gpu
def test_two_runs_are_bitwise_identical():
    arr = random_case(11, 1500, 40)
    a = to_numpy(voc_map(**arr, num_classes=20, min_overlap=[0.5, 0.75], return_curves=True))
    b = to_numpy(voc_map(**arr, num_classes=20, min_overlap=[0.5, 0.75], return_curves=True))
    assert set(a) == set(b)
    for k in a:
        assert a[k].tobytes() == b[k].tobytes(), k


@gpu
def test_get_map_on_a_directory_equals_the_reference(golden, tmp_path):
    os.makedirs(tmp_path / "ground-truth")
    os.makedirs(tmp_path / "detection-results")
    for iid, g, d in zip(golden["s0_ids"], golden["s0_gt_text"], golden["s0_dr_text"]):
        (tmp_path / "ground-truth" / f"{iid}.txt").write_text(str(g))
        (tmp_path / "detection-results" / f"{iid}.txt").write_text(str(d))
    before = sorted(os.listdir(tmp_path))
    for j, thr in enumerate(golden["thresholds"]):
        m = get_map(float(thr), False, path=str(tmp_path))
        assert isinstance(m, float) and abs(m - float(golden[f"s0_t{j}_map"])) <= TOL, (thr, m)
    assert sorted(os.listdir(tmp_path)) == before                      # nothing written, nothing deleted


@gpu
def test_evaluator_image_by_image_equals_voc_map_on_the_concatenation():
    rng = np.random.default_rng(3)
    names = [f"c{k}" for k in range(5)]
    ev = DetectionEvaluator(names, max_boxes=20)
    ids = [f"frame{int(v):05d}" for v in rng.permutation(60)]           # fed out of order: evaluated in sorted order
    per_image = {}
    for iid in ids:
        n, g = int(rng.integers(0, 30)), int(rng.integers(0, 6))
        lt = rng.random((n, 2)) * 300
        rows = np.concatenate([lt, lt + 10 + rng.random((n, 2)) * 90, rng.random((n, 2)), rng.integers(0, 5, (n, 1))],
                              axis=1).astype(np.float32)
        glt = rng.integers(0, 300, (g, 2))
        gt = np.concatenate([glt, glt + rng.integers(10, 100, (g, 2)), rng.integers(0, 5, (g, 1))], axis=1)
        if n and g:                                                      # some detections sit on ground truths
            k = min(n, g)
            rows[:k, :4] = gt[:k, [1, 0, 3, 2]] + rng.random((k, 4)).astype(np.float32) * 4
            rows[:k, 6] = gt[:k, 4]
        ev.add(iid, rows if n else None, gt)
        per_image[iid] = (rows, gt)
    cat = {k: [] for k in ARRAYS[:-1]}
    for i, iid in enumerate(sorted(ids)):
        rows, gt = per_image[iid]
        label, score, box = format_detections(rows, 20)
        for k, v in (("det_image", np.full(len(label), i)), ("det_label", label), ("det_score", score), ("det_box", box),
                     ("gt_image", np.full(len(gt), i)), ("gt_label", gt[:, 4]), ("gt_box", gt[:, :4].astype(np.float64))):
            cat[k].append(v)
    cat = {k: np.concatenate(v) for k, v in cat.items()}
    a = to_numpy(ev.compute(min_overlap=0.5, return_curves=True))
    b = to_numpy(voc_map(**cat, num_classes=5, min_overlap=0.5, return_curves=True))
    assert a["tp"].sum() > 10
    for k in a:
        assert a[k].tobytes() == b[k].tobytes(), k
    assert_matches(a, get_map_restated(**cat, gt_difficult=np.zeros(len(cat["gt_label"]), np.uint8), num_classes=5,
                                       min_overlap=0.5), "evaluator")
