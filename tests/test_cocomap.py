"""The COCO detection metrics (csrc/cocomap.hip, metrics.coco_map / get_coco_map / DetectionEvaluator.compute_coco,
EvalPipeline.compute(coco=True)): a sequential Python restatement of COCOeval(cocoGt, cocoDt, 'bbox') evaluate(),
accumulate(), summarize() as utils/utils_map.py:894-923 runs it, loop for loop (computeIoU with the IoU matrix of a group
computed once, evaluateImg, accumulate, _summarize), held to hand-built cases on the CPU, then the HIP path against it.
pycocotools is installed nowhere this project builds or runs: the restatement was written from COCOeval's published
source and has never been run against it.

Tolerances (none of them taken from what the kernels give):
  precision, recall, n_gt, dt_match, dt_ignore, kept   bit-equal: integers, or IEEE fp64 operations in COCOeval's order
  stats                                                1e-11 absolute: numpy's mean sums pairwise, the kernel in its own
                                                       fixed tree; for at most 10 * 101 * K values in [0, 1] with K <= 20
                                                       either sum is within n * 2^-53 ~ 2.3e-12 of exact
  hand cases                                           1e-11: "1" is 1 / (1 + 2^-52)"""
import os

import numpy as np
import pytest
import torch

from asy_vrnet_amd import metrics
from asy_vrnet_amd.metrics import DetectionEvaluator, coco_map, get_coco_map

STATS_TOL = 1e-11
IOU_THRS = np.linspace(.5, 0.95, int(np.round((0.95 - .5) / .05)) + 1, endpoint=True)
REC_THRS = np.linspace(.0, 1.00, int(np.round((1.00 - .0) / .01)) + 1, endpoint=True)
MAX_DETS = [1, 10, 100]
AREA_RNG = [[0 ** 2, 1e5 ** 2], [0 ** 2, 32 ** 2], [32 ** 2, 96 ** 2], [96 ** 2, 1e5 ** 2]]


# ---- the restatement --------------------------------------------------------------------------------------------------

def bb_iou(dt, gt, iscrowd):
    """maskApi.c bbIou on x, y, w, h boxes: (len(dt), len(gt))."""
    o = np.zeros((len(dt), len(gt)), dtype=np.float64)
    for g, G in enumerate(gt):
        ga = G[2] * G[3]
        for d, D in enumerate(dt):
            da = D[2] * D[3]
            w = min(D[2] + D[0], G[2] + G[0]) - max(D[0], G[0])
            if w <= 0:
                continue
            h = min(D[3] + D[1], G[3] + G[1]) - max(D[1], G[1])
            if h <= 0:
                continue
            i = w * h
            u = da if iscrowd[g] else da + ga - i
            o[d, g] = i / u
    return o


def coco_restated(det_image, det_label, det_score, det_box, gt_image, gt_label, gt_box, gt_difficult=None, num_classes=None,
                  gt_area=None, zero_id_gt=None):
    """COCOeval on flat arrays.  Annotation ids: ground truth i has id i + 1, or 0 if i == zero_id_gt; detection i has id
    i + 1 (loadRes).  Returns stats, precision, recall, n_gt and, in the detections' input order, dt_match (ground-truth
    input index or -1), dt_ignore, kept."""
    det_box = np.asarray(det_box, dtype=np.float64).reshape(-1, 4)
    gt_box = np.asarray(gt_box, dtype=np.float64).reshape(-1, 4)
    D, G = len(det_box), len(gt_box)
    diff = np.zeros(G, dtype=bool) if gt_difficult is None else np.asarray(gt_difficult).astype(bool)
    n_img = int(max([int(v) + 1 for v in det_image] + [int(v) + 1 for v in gt_image] + [0]))
    K = int(num_classes)
    T, R, A, M = len(IOU_THRS), len(REC_THRS), len(AREA_RNG), len(MAX_DETS)
    # _prepare
    gts, dts = {}, {}
    for i in range(G):
        l, t, r, b = (float(v) for v in gt_box[i])
        w, h = r - l, b - t
        area = w * h - 10.0 if gt_area is None else float(gt_area[i])
        gts.setdefault((int(gt_image[i]), int(gt_label[i])), []).append(
            dict(idx=i, id=0 if i == zero_id_gt else i + 1, bbox=[l, t, w, h], area=area, iscrowd=int(diff[i]), ignore=int(diff[i])))
    for i in range(D):
        l, t, r, b = (float(v) for v in det_box[i])
        w, h = r - l, b - t
        dts.setdefault((int(det_image[i]), int(det_label[i])), []).append(
            dict(idx=i, id=i + 1, bbox=[l, t, w, h], area=w * h, score=float(det_score[i])))
    dt_match = -np.ones((T, A, D), dtype=np.int32)
    dt_ignore = np.zeros((T, A, D), dtype=np.uint8)
    kept = np.zeros(D, dtype=np.uint8)
    # computeIoU, once per group
    ious, sorted_dts = {}, {}
    for key, dt in dts.items():
        inds = np.argsort([-d["score"] for d in dt], kind="mergesort")
        dt = [dt[i] for i in inds][:MAX_DETS[-1]]
        sorted_dts[key] = dt
        for d in dt:
            kept[d["idx"]] = 1
        gt = gts.get(key, [])
        ious[key] = bb_iou([d["bbox"] for d in dt], [g["bbox"] for g in gt], [g["iscrowd"] for g in gt]) if gt else []

    def evaluate_img(img, cat, a, rng):
        gt, dt = gts.get((img, cat), []), sorted_dts.get((img, cat), [])
        if len(gt) == 0 and len(dt) == 0:
            return None
        for g in gt:
            g["_ignore"] = 1 if (g["ignore"] or (g["area"] < rng[0] or g["area"] > rng[1])) else 0
        gtind = np.argsort([g["_ignore"] for g in gt], kind="mergesort")
        gt = [gt[i] for i in gtind]
        iscrowd = [int(o["iscrowd"]) for o in gt]
        iou_mat = ious[(img, cat)][:, gtind] if len(dt) and len(ious[(img, cat)]) > 0 else []
        gtm, dtm = np.zeros((T, len(gt))), np.zeros((T, len(dt)))
        gt_ig = np.array([g["_ignore"] for g in gt])
        dt_ig = np.zeros((T, len(dt)))
        if not len(iou_mat) == 0:
            for tind, t in enumerate(IOU_THRS):
                for dind, d in enumerate(dt):
                    iou = min([t, 1 - 1e-10])
                    m = -1
                    for gind, g in enumerate(gt):
                        if gtm[tind, gind] > 0 and not iscrowd[gind]:
                            continue
                        if m > -1 and gt_ig[m] == 0 and gt_ig[gind] == 1:
                            break
                        if iou_mat[dind, gind] < iou:
                            continue
                        iou = iou_mat[dind, gind]
                        m = gind
                    if m == -1:
                        continue
                    dt_ig[tind, dind] = gt_ig[m]
                    dtm[tind, dind] = gt[m]["id"]
                    gtm[tind, m] = d["id"]
                    dt_match[tind, a, d["idx"]] = gt[m]["idx"]
        out = np.array([d["area"] < rng[0] or d["area"] > rng[1] for d in dt]).reshape((1, len(dt)))
        dt_ig = np.logical_or(dt_ig, np.logical_and(dtm == 0, np.repeat(out, T, 0)))
        for dind, d in enumerate(dt):
            dt_ignore[:, a, d["idx"]] = dt_ig[:, dind]
        return dict(dtMatches=dtm, dtScores=[d["score"] for d in dt], gtIgnore=gt_ig, dtIgnore=dt_ig)

    eval_imgs = [evaluate_img(img, cat, a, rng) for cat in range(K) for a, rng in enumerate(AREA_RNG) for img in range(n_img)]
    # accumulate
    precision = -np.ones((T, R, K, A, M))
    recall = -np.ones((T, K, A, M))
    n_gt = np.zeros((K, A), dtype=np.int32)
    for k in range(K):
        for a in range(A):
            E = [eval_imgs[k * A * n_img + a * n_img + i] for i in range(n_img)]
            E = [e for e in E if e is not None]
            if len(E) == 0:
                continue
            for m, max_det in enumerate(MAX_DETS):
                dt_scores = np.concatenate([e["dtScores"][0:max_det] for e in E])
                inds = np.argsort(-dt_scores, kind="mergesort")
                dtm = np.concatenate([e["dtMatches"][:, 0:max_det] for e in E], axis=1)[:, inds]
                dt_ig = np.concatenate([e["dtIgnore"][:, 0:max_det] for e in E], axis=1)[:, inds]
                gt_ig = np.concatenate([e["gtIgnore"] for e in E])
                npig = np.count_nonzero(gt_ig == 0)
                n_gt[k, a] = npig
                if npig == 0:
                    continue
                tps = np.logical_and(dtm, np.logical_not(dt_ig))
                fps = np.logical_and(np.logical_not(dtm), np.logical_not(dt_ig))
                tp_sum = np.cumsum(tps, axis=1).astype(dtype=float)
                fp_sum = np.cumsum(fps, axis=1).astype(dtype=float)
                for t, (tp, fp) in enumerate(zip(tp_sum, fp_sum)):
                    tp, fp = np.array(tp), np.array(fp)
                    nd = len(tp)
                    rc = tp / npig
                    pr = tp / (fp + tp + np.spacing(1))
                    q = np.zeros((R,))
                    recall[t, k, a, m] = rc[-1] if nd else 0
                    pr, q = pr.tolist(), q.tolist()
                    for i in range(nd - 1, 0, -1):
                        if pr[i] > pr[i - 1]:
                            pr[i - 1] = pr[i]
                    inds_r = np.searchsorted(rc, REC_THRS, side="left")
                    try:
                        for ri, pi in enumerate(inds_r):
                            q[ri] = pr[pi]
                    except IndexError:
                        pass
                    precision[t, :, k, a, m] = np.array(q)

    def summarize(ap, iou_thr=None, a=0, m=2):
        if ap == 1:
            s = precision
            if iou_thr is not None:
                s = s[np.where(iou_thr == IOU_THRS)[0]]
            s = s[:, :, :, a, m]
        else:
            s = recall
            if iou_thr is not None:
                s = s[np.where(iou_thr == IOU_THRS)[0]]
            s = s[:, :, a, m]
        return -1 if len(s[s > -1]) == 0 else np.mean(s[s > -1])

    stats = np.array([summarize(1), summarize(1, iou_thr=.5), summarize(1, iou_thr=.75), summarize(1, a=1), summarize(1, a=2),
                      summarize(1, a=3), summarize(0, m=0), summarize(0, m=1), summarize(0, m=2), summarize(0, a=1),
                      summarize(0, a=2), summarize(0, a=3)], dtype=np.float64)
    return dict(stats=stats, precision=precision, recall=recall, n_gt=n_gt, dt_match=dt_match, dt_ignore=dt_ignore, kept=kept)


# ---- inputs -----------------------------------------------------------------------------------------------------------

def case(gts, dets, num_classes=1, **kw):
    """gts: (image, class, box, difficult); dets: (image, class, score, box)."""
    return dict(det_image=np.array([d[0] for d in dets], dtype=np.int64), det_label=np.array([d[1] for d in dets], dtype=np.int64),
                det_score=np.array([d[2] for d in dets], dtype=np.float64),
                det_box=np.array([d[3] for d in dets], dtype=np.float64).reshape(-1, 4),
                gt_image=np.array([g[0] for g in gts], dtype=np.int64), gt_label=np.array([g[1] for g in gts], dtype=np.int64),
                gt_box=np.array([g[2] for g in gts], dtype=np.float64).reshape(-1, 4),
                gt_difficult=np.array([g[3] for g in gts], dtype=np.uint8), num_classes=num_classes, **kw)


B100 = (0, 0, 100, 100)
HAND = {
    "A": (case([(0, 0, B100, 0)], [(0, 0, .9, B100)]), [1, 1, 1, -1, -1, 1, 1, 1, 1, -1, -1, 1]),
    "B": (case([(0, 0, B100, 0)], [(0, 0, .9, (0, 0, 100, 62))]), [.3, 1, 0, -1, -1, .3, .3, .3, .3, -1, -1, .3]),
    "F": (case([(0, 0, (0, 0, 50, 50), 0), (0, 0, (100, 100, 150, 150), 0)],
               [(0, 0, .9, (0, 0, 50, 50)), (0, 0, .8, (100, 100, 150, 150))]), [1, 1, 1, -1, 1, -1, .5, 1, 1, -1, 1, -1]),
    "D": (case([(0, 0, B100, 1), (0, 0, (200, 200, 240, 240), 0)],
               [(0, 0, .9, (0, 0, 40, 40)), (0, 0, .8, (10, 10, 50, 50)), (0, 0, .7, (200, 200, 240, 240))]),
          [1, 1, 1, -1, 1, -1, 0, 1, 1, -1, 1, -1]),
    "E": (case([(0, 0, B100, 0)], [(0, 0, .9, B100)], zero_id_gt=0), [0, 0, 0, -1, -1, 0, 0, 0, 0, -1, -1, 0]),
    "H": (case([(0, 0, (0, 0, 3, 3), 0)], [(0, 0, .9, (0, 0, 3, 3))]), [-1] * 12),
    "I": (case([(0, 0, (0, 0, 30, 30), 0)], [(0, 1, .9, (0, 0, 30, 30))], num_classes=2), [0, 0, 0, 0, -1, -1, 0, 0, 0, 0, -1, -1]),
}
TIES = case([(0, 0, (0, 0, 40, 40), 0), (0, 0, (0, 0, 40, 40), 0)], [(0, 0, .9, (0, 0, 40, 40))])
# image 1's detection comes first in the input; with equal scores image 0's is ranked first and takes the recall-0 points
TIE_ORDER = case([(0, 0, (0, 0, 40, 40), 0), (1, 0, (0, 0, 40, 40), 0)],
                 [(1, 0, .5, (0, 0, 40, 40)), (0, 0, .5, (100, 100, 140, 140))])


def random_set(seed, n_images=12, num_classes=3):
    """Seeded set: 0-5 ground truths per image with sides from {12, 24, 48, 80, 140, 220} plus jitter (all three area ranges
    occur), 15 % difficult, 0-2 jittered detections per ground truth, 0-2 random boxes per image, integer boxes, scores to
    two decimals (ties)."""
    rng = np.random.default_rng(seed)
    sides = np.array([12, 24, 48, 80, 140, 220])
    gts, dets = [], []
    box = lambda: (lambda l, t, w, h: (l, t, l + w, t + h))(int(rng.integers(0, 300)), int(rng.integers(0, 300)),
                                                              int(rng.choice(sides) + rng.integers(-3, 4)),
                                                              int(rng.choice(sides) + rng.integers(-3, 4)))
    for i in range(n_images):
        for _ in range(int(rng.integers(0, 6))):
            b, c = box(), int(rng.integers(0, num_classes))
            gts.append((i, c, b, int(rng.random() < 0.15)))
            for _ in range(int(rng.integers(0, 3))):
                j = rng.integers(-1, 2, 4) * np.array([b[2] - b[0], b[3] - b[1]] * 2) // 10
                dets.append((i, c, round(float(rng.random()), 2), tuple(int(v) for v in np.array(b) + j)))
        for _ in range(int(rng.integers(0, 3))):
            dets.append((i, int(rng.integers(0, num_classes)), round(float(rng.random()), 2), box()))
    perm = rng.permutation(len(dets))                                   # the input order is not the image order
    return case(gts, [dets[k] for k in perm], num_classes=num_classes)


SEEDS = (1, 2, 3, 4, 5)


@pytest.fixture(scope="module")
def random_sets():
    sets = {s: random_set(s) for s in SEEDS}
    return {s: (arr, coco_restated(**arr), coco_restated(**arr, zero_id_gt=0)) for s, arr in sets.items()}


def one_group(n_det, n_gt, seed, split=1):
    """One class, `split` images; n_det detections and n_gt ground truths spread evenly: a grid of ground truths, detections
    jittered on them (several per ground truth when n_det > n_gt), distinct scores."""
    rng = np.random.default_rng(seed)
    gts, dets = [], []
    for g in range(n_gt):
        l, t, s = 60 * (g % 15), 60 * (g // 15), int(rng.choice([20, 40, 50]))
        gts.append((g % split, 0, (l, t, l + s, t + s), int(rng.random() < 0.1)))
    scores = rng.permutation(n_det) / n_det
    for d in range(n_det):
        g = gts[d % n_gt]
        j = rng.integers(-4, 5, 4)
        dets.append((g[0], 0, float(scores[d]), tuple(int(v) for v in np.array(g[2]) + j)))
    return case(gts, dets)


# ---- CPU: the restatement on the hand-built cases ------------------------------------------------------------------------

def test_constants_are_numpys():
    assert IOU_THRS[8] == 0.8999999999999999 and IOU_THRS[5] == 0.75 and IOU_THRS[0] == 0.5 and len(IOU_THRS) == 10
    assert len(REC_THRS) == 101 and REC_THRS[-1] == 1.0
    assert np.array_equal(metrics.COCO_IOU_THRS, IOU_THRS) and np.array_equal(metrics.COCO_REC_THRS, REC_THRS)
    assert list(metrics.COCO_MAX_DETS) == MAX_DETS and [list(r) for r in metrics.COCO_AREA_RNG] == AREA_RNG


@pytest.mark.parametrize("name", sorted(HAND))
def test_restatement_on_hand_built_cases(name):
    arr, want = HAND[name]
    got = coco_restated(**arr)["stats"]
    print(name, got)
    assert np.abs(got - np.array(want, dtype=np.float64)).max() <= STATS_TOL, (name, got)


def test_restatement_crowd_absorbs_and_ties():
    r = coco_restated(**HAND["D"][0])
    # both detections inside the crowd are matched to it (index 0) and ignored, at every threshold and in every range
    assert (r["dt_match"][:, :, :2] == 0).all() and (r["dt_ignore"][:, :, :2] == 1).all()
    assert (r["dt_match"][:, 0, 2] == 1).all() and (r["dt_ignore"][:, 0, 2] == 0).all()
    # among equal IoUs the later ground truth wins
    assert (coco_restated(**TIES)["dt_match"][:, 0, 0] == 1).all()
    # equal scores: image 0's detection (a false positive) is ranked before image 1's true positive, although image 1's
    # comes first in the input: precision at recall 0 is 1/2, not 1
    r = coco_restated(**TIE_ORDER)
    assert abs(r["precision"][0, 0, 0, 0, 2] - 0.5) < 1e-12 and r["n_gt"][0, 0] == 2


def test_random_sets_meet_their_conditions(random_sets):
    shifted = 0
    for s, (arr, r, r0) in random_sets.items():
        ties = len(arr["det_score"]) - len(np.unique(arr["det_score"]))
        print(s, "dets", len(arr["det_score"]), "gts", len(arr["gt_label"]), "ties", ties, "stats", np.round(r["stats"], 3))
        assert ((r["stats"] > 0) & (r["stats"] < 1)).all(), (s, r["stats"])
        assert ties >= 2, (s, ties)
        shifted += bool(np.abs(r["stats"] - r0["stats"]).max() > 0)
    assert shifted >= 1


def test_coco_map_argument_errors():
    arr = dict(HAND["A"][0])
    with pytest.raises(RuntimeError):
        coco_map(**arr, device="cpu")                                   # no CPU fallback
    for name in ("vrnet_coco_map_f64", "vrnet_coco_map_workspace_bytes", "vrnet_coco_map_group_bytes"):
        assert name in metrics.hip.EXPORTED
    assert callable(metrics.hip.coco_map) and callable(DetectionEvaluator.compute_coco)
    gb = metrics.hip._lib.vrnet_coco_map_group_bytes
    assert gb(130, 70) == 8 * 100 * 70 + 160 * 3 + 72 and gb(100, 200) > metrics.COCO_LDS_BYTES >= gb(50, 100)
    assert metrics.hip._lib.vrnet_coco_map_workspace_bytes(1000, 4096) >= 40 * 1000 + 4096       # a byte per chain and detection


# ---- GPU --------------------------------------------------------------------------------------------------------------

gpu = pytest.mark.gpu
BITWISE = ("precision", "recall", "n_gt", "dt_match", "dt_ignore", "kept")


def to_numpy(res):
    return {k: res[k].cpu().numpy() for k in res.keys()}


def run_and_compare(arr, where, want=None):
    got = to_numpy(coco_map(**arr, return_matches=True))
    want = coco_restated(**arr) if want is None else want
    for k in BITWISE:
        g, w = got[k], np.asarray(want[k])
        assert g.shape == w.shape, (where, k, g.shape, w.shape)
        same = np.array_equal(g, w)
        print(f"{where}: {k}: {g.size} values, {'bit-equal' if same else int((g != w).sum())}")
        assert same, (where, k, np.argwhere(g != w)[:10])
    err = float(np.abs(got["stats"] - want["stats"]).max())
    print(f"{where}: stats {np.round(got['stats'], 4)} max abs error {err:.3e}")
    assert err <= STATS_TOL, (where, got["stats"], want["stats"])
    return got, want


@gpu
@pytest.mark.parametrize("name", sorted(HAND))
def test_hand_built_cases(name):
    arr, want = HAND[name]
    got, _ = run_and_compare(arr, name)
    assert np.abs(got["stats"] - np.array(want, dtype=np.float64)).max() <= STATS_TOL


@gpu
def test_ties_and_tie_order():
    got, _ = run_and_compare(TIES, "ties")
    assert (got["dt_match"][:, 0, 0] == 1).all()
    got, _ = run_and_compare(TIE_ORDER, "tie order")
    assert abs(got["precision"][0, 0, 0, 0, 2] - 0.5) < 1e-12


@gpu
@pytest.mark.parametrize("seed", SEEDS)
def test_random_sets(random_sets, seed):
    arr, want, want0 = random_sets[seed]
    run_and_compare(arr, f"seed {seed}", want)
    run_and_compare(dict(arr, zero_id_gt=0), f"seed {seed} id 0", want0)
    area = np.arange(len(arr["gt_label"]), dtype=np.float64) * 700.0     # an explicit gt_area replaces w * h - 10
    run_and_compare(dict(arr, gt_area=area), f"seed {seed} gt_area")


@gpu
def test_one_group_beyond_the_cut():
    arr = one_group(130, 70, 7)
    got, want = run_and_compare(arr, "130 x 70")
    assert got["kept"].sum() == 100 and (got["dt_match"][:, :, got["kept"] == 0] == -1).all()
    assert want["stats"][7] != want["stats"][8] and got["stats"][7] != got["stats"][8]           # AR10 != AR100
    assert (got["dt_match"][0, 0] >= 64).any()                                                   # past a 64-entry matched set


@gpu
def test_workspace_path_and_lds_path():
    gb = metrics.hip._lib.vrnet_coco_map_group_bytes
    assert gb(100, 200) > metrics.COCO_LDS_BYTES >= gb(50, 100)
    one = one_group(100, 200, 8)
    got, _ = run_and_compare(one, "100 x 200, one image: workspace")
    assert (got["dt_match"][0, 0] >= 0).sum() > 50
    two = one_group(100, 200, 8, split=2)
    assert np.array_equal(two["det_box"], one["det_box"]) and np.array_equal(two["gt_box"], one["gt_box"])
    assert np.bincount(two["det_image"]).tolist() == [50, 50] and np.bincount(two["gt_image"]).tolist() == [100, 100]
    run_and_compare(two, "100 x 200 over two images: LDS")
    # both kinds of group in one call
    both = {k: (np.concatenate([one[k], two[k] + (2 if k.endswith("image") else 0)]) if isinstance(one[k], np.ndarray) else one[k])
            for k in one}
    both["det_image"][:100] = 1
    both["gt_image"][:200] = 1
    run_and_compare(both, "workspace and LDS groups together")


@gpu
def test_one_class_across_scan_chunks():
    rng = np.random.default_rng(9)
    gts, dets = [], []
    for i in range(12):
        for g in range(30):
            l, t, s = 50 * (g % 10), 50 * (g // 10), int(rng.choice([16, 30, 40]))
            gts.append((i, 0, (l, t, l + s, t + s), int(rng.random() < 0.1)))
    for d in range(1100):
        g = gts[int(rng.integers(0, len(gts)))]
        dets.append((g[0], 0, round(float(rng.random()), 3), tuple(int(v) for v in np.array(g[2]) + rng.integers(-5, 6, 4))))
    arr = case(gts, dets)
    assert len(arr["det_score"]) == 1100 > 2 * 512                      # three chunks of the scan: two carries
    got, _ = run_and_compare(arr, "1100 detections of one class")
    assert 0 < got["stats"][0] < 1


@gpu
def test_degenerate_inputs():
    arr = random_set(1)
    e = dict(det_image=np.zeros(0, np.int64), det_label=np.zeros(0, np.int64), det_score=np.zeros(0), det_box=np.zeros((0, 4)))
    g = dict(gt_image=np.zeros(0, np.int64), gt_label=np.zeros(0, np.int64), gt_box=np.zeros((0, 4)),
             gt_difficult=np.zeros(0, np.uint8))
    got, _ = run_and_compare(dict(arr, **e), "no detections")
    assert got["stats"][0] == 0.0 and got["stats"][8] == 0.0 and (got["recall"][:, got["n_gt"] > 0] == 0).all()
    got, _ = run_and_compare(dict(arr, **g), "no ground truths")
    assert (got["stats"] == -1).all() and (got["precision"] == -1).all()
    got, _ = run_and_compare(dict(arr, **e, **g), "nothing at all")
    assert (got["stats"] == -1).all() and got["dt_match"].shape == (10, 4, 0)
    got, _ = run_and_compare(dict(arr, num_classes=5), "classes without boxes")
    assert (got["precision"][:, :, 3:] == -1).all() and (got["n_gt"][3:] == 0).all()
    no_diff = dict(arr)
    no_diff.pop("gt_difficult")
    no_classes = dict(no_diff, num_classes=None)
    assert max(arr["det_label"].max(), arr["gt_label"].max()) == 2     # the largest id + 1 is the 3 classes given above
    a, b = to_numpy(coco_map(**no_diff)), to_numpy(coco_map(**no_classes))
    want = coco_restated(**dict(arr, gt_difficult=None))
    assert np.array_equal(a["precision"], want["precision"]) and np.array_equal(b["precision"], want["precision"])


@gpu
def test_two_runs_are_bitwise_identical():
    arr = random_set(3, n_images=40)
    a, b = to_numpy(coco_map(**arr, return_matches=True)), to_numpy(coco_map(**arr, return_matches=True))
    assert set(a) == set(b) == {"stats", "precision", "recall", "n_gt", "dt_match", "dt_ignore", "kept"}
    for k in a:
        assert a[k].tobytes() == b[k].tobytes(), k


def write_dir(root, gt_text, dr_text):
    os.makedirs(root / "ground-truth")
    os.makedirs(root / "detection-results")
    for k, v in gt_text.items():
        (root / "ground-truth" / f"{k}.txt").write_text(v)
    for k, v in dr_text.items():
        (root / "detection-results" / f"{k}.txt").write_text(v)


@gpu
def test_get_coco_map_on_a_directory(tmp_path):
    names = ["boat", "traffic light", "pier"]
    gt_text = {"b2": "boat 10 10 110 110\ntraffic light 200 200 240 260 difficult\nkayak 5 5 50 50\n",
               "a10": "traffic light 30 30 60 90\nboat 100 100 180 150\n",
               "a9": "pier 0 0 300 40\n"}
    dr_text = {"b2": "boat 0.9 12 12 108 111\ntraffic light 0.8 205 205 235 255\nkayak 0.99 5 5 50 50\nboat 0.3 300 300 340 340\n",
               "a10": "traffic light 0.7 31 29 61 92\nboat 0.9 100 100 178 152\n",
               "a9": "pier 0.6 1 0 298 41\n"}
    write_dir(tmp_path / "set", gt_text, dr_text)
    root = tmp_path / "set"
    before = sorted(os.listdir(root))
    got = get_coco_map(names, str(root))
    assert isinstance(got, np.ndarray) and got.shape == (12,) and sorted(os.listdir(root)) == before
    # the restatement on arrays built the same way: images by sorted stem, ground truths in os.listdir order, its first
    # kept box with id 0
    index = {s: i for i, s in enumerate(sorted(gt_text))}
    gts, dets = [], []
    for f in os.listdir(root / "ground-truth"):
        for line in gt_text[f[:-4]].splitlines():
            tok = line.split()
            diff = "difficult" in line
            name = " ".join(tok[:-5] if diff else tok[:-4])
            if name in names:
                gts.append((index[f[:-4]], names.index(name), [float(v) for v in (tok[-5:-1] if diff else tok[-4:])], diff))
    for f in os.listdir(root / "detection-results"):
        for line in dr_text[f[:-4]].splitlines():
            tok = line.split()
            name = " ".join(tok[:-5])
            if name in names:
                dets.append((index[f[:-4]], names.index(name), float(tok[-5]), [float(v) for v in tok[-4:]]))
    assert len(gts) == 5 and len(dets) == 6 and any(g[3] for g in gts)
    want = coco_restated(**case(gts, dets, num_classes=3, zero_id_gt=0))
    assert np.abs(got - want["stats"]).max() <= STATS_TOL, (got, want["stats"])
    assert np.abs(want["stats"] - coco_restated(**case(gts, dets, num_classes=3))["stats"]).max() > 0      # id 0 matters here
    write_dir(tmp_path / "empty", gt_text, {k: "" for k in dr_text})
    assert get_coco_map(names, str(tmp_path / "empty")).tolist() == [0.0] * 12
    write_dir(tmp_path / "odd", gt_text, dict(dr_text, zz="boat 0.5 1 1 20 20\n"))
    with pytest.raises(RuntimeError):
        get_coco_map(names, str(tmp_path / "odd"))


@gpu
def test_evaluator_compute_coco_equals_coco_map():
    rng = np.random.default_rng(12)
    ev = DetectionEvaluator(["a", "b", "c"], max_boxes=20)
    for iid in rng.permutation(8):
        n, g = int(rng.integers(0, 12)), int(rng.integers(0, 5))
        glt = rng.integers(0, 200, (g, 2))
        gt = np.concatenate([glt, glt + rng.integers(10, 120, (g, 2)), rng.integers(0, 3, (g, 1))], axis=1)
        lt = rng.random((n, 2)) * 200
        rows = np.concatenate([lt, lt + 10 + rng.random((n, 2)) * 90, rng.random((n, 2)), rng.integers(0, 3, (n, 1))],
                              axis=1).astype(np.float32)
        k = min(n, g)
        if k:
            rows[:k, :4] = gt[:k, [1, 0, 3, 2]] + rng.random((k, 4)).astype(np.float32) * 4
            rows[:k, 6] = gt[:k, 4]
        ev.add(f"im{int(iid):03d}", rows if n else None, gt)
    a, b = to_numpy(ev.compute_coco()), to_numpy(coco_map(**ev.arrays(), num_classes=3))
    assert set(a) == set(b) == {"stats", "precision", "recall", "n_gt"}
    for k in a:
        assert a[k].tobytes() == b[k].tobytes(), k
    want = coco_restated(**ev.arrays(), num_classes=3)
    assert np.array_equal(a["precision"], want["precision"]) and 0 < a["stats"][1] <= 1


@gpu
def test_eval_pipeline_coco():
    import asy_vrnet_amd as A
    names, nseg, S, F = ["boat", "buoy", "pier", "ship"], 9, (64, 64), (40, 56)
    model = A.EfficientVRNet(4, nseg, "nano", img_size=S[0]).cuda().eval()
    A.randomize_state_dict(model.state_dict(), seed=4)
    pipe = A.EvalPipeline(model, F, S, names, nseg, batch=2, capacity=4, max_boxes=4, max_gt=4, conf_thres=0.05)
    rng = np.random.default_rng(97)
    for k in range(2):
        frames = rng.integers(0, 256, (2,) + F + (3,), dtype=np.uint8)
        radar = (rng.standard_normal((2, 4) + S) * 2.0 + 1.0).astype(np.float32)
        labels = rng.choice(np.array(list(range(10)) + [255], dtype=np.uint8), (2,) + F)
        x1, y1 = rng.integers(0, F[1] - 20, (2, 2)), rng.integers(0, F[0] - 20, (2, 2))
        gt = [np.stack([x1[b], y1[b], x1[b] + 18, y1[b] + 18, rng.integers(0, 4, 2)], axis=1) for b in range(2)]
        pipe.add([f"i{2 * k}", f"i{2 * k + 1}"], frames, radar, labels, gt)
    plain, with_coco = pipe.compute(strict=False), pipe.compute(strict=False, coco=True)
    assert plain.coco is None and isinstance(with_coco.coco, metrics.CocoMapResult)
    for k in ("map", "ap", "f1", "recall", "precision", "lamr", "n_gt", "n_det", "n_tp"):
        assert plain.det[k].cpu().numpy().tobytes() == with_coco.det[k].cpu().numpy().tobytes(), k
    assert np.array_equal(plain.hist, with_coco.hist) and plain.miou == with_coco.miou and plain.flag == with_coco.flag
    a, N = pipe.arena, 4
    perm = torch.tensor(sorted(range(N), key=pipe.image_ids.__getitem__), device="cuda")
    image = torch.arange(N, device="cuda")[:, None]
    dmask = torch.arange(4, device="cuda")[None, :] < a["det_count"][perm][:, None]
    gmask = torch.arange(4, device="cuda")[None, :] < a["gt_n"][perm][:, None]
    direct = coco_map(image.expand(N, 4)[dmask], a["det_label"][perm][dmask], a["det_score"][perm][dmask], a["det_box"][perm][dmask],
                      image.expand(N, 4)[gmask], a["gt_label"][perm][gmask], a["gt_box"][perm][gmask], num_classes=4)
    assert int(dmask.sum()) > 0 and int(gmask.sum()) == 8
    assert with_coco.coco.stats.cpu().numpy().tobytes() == direct.stats.cpu().numpy().tobytes()


@gpu
def test_argument_errors_on_the_device():
    arr = dict(HAND["F"][0])
    with pytest.raises(RuntimeError):
        coco_map(**dict(arr, det_score=arr["det_score"][:1]))          # lengths
    with pytest.raises(RuntimeError):
        coco_map(**dict(arr, gt_difficult=np.zeros(3, np.uint8)))
    with pytest.raises(RuntimeError):
        coco_map(**arr, gt_area=np.zeros(1))
    with pytest.raises(RuntimeError):
        coco_map(**dict(arr, det_score=np.array([0.5, float("nan")])))
    with pytest.raises(RuntimeError):
        coco_map(**arr, zero_id_gt=2)                                   # two ground truths: 0 and 1 only
    with pytest.raises(RuntimeError):
        coco_map(**arr, zero_id_gt=-1)
    with pytest.raises(RuntimeError):
        coco_map(**dict(arr, num_classes=1, det_label=np.array([0, 1])))
    with pytest.raises(RuntimeError):
        coco_map(**arr, device="cpu")
