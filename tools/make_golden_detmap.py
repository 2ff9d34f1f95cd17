"""Golden vectors for the detection metric: the reference's OWN `get_map` (utils/utils_map.py:276-798) run on seeded
synthetic directories at several IoU thresholds, with `voc_ap` and `log_average_miss_rate` wrapped to record the per-class
recall / precision lists they receive and the AP / lamr they return.  The module imports cv2 at the top (not installed
here) but get_map never calls it without an images-optional directory: a throw-away empty stub package satisfies the import.
The fixture holds arrays only: the flat input arrays of every set, the text of the smallest set's files (so the parser is
pinned too), and the reference's results.  tests/golden/detmap_small.npz.
    python tools/make_golden_detmap.py <path of the reference checkout>

Every situation the metric has a rule for must occur in the sets; `check_coverage` asserts each one, so a fixture that
misses one cannot be written."""
import contextlib
import io
import os
import re
import shutil
import sys
import tempfile

import numpy as np

THRESHOLDS = (0.3, 0.5, 0.75)
NAMES = ["boat", "buoy", "pier", "sailor", "traffic light", "vessel"]      # buoy: never detected
GHOST = "ghost"                                                             # detected, never annotated


def write_stub(d):
    os.makedirs(os.path.join(d, "cv2"))
    open(os.path.join(d, "cv2", "__init__.py"), "w").write("")


def synthetic_set(rng, n_img, hand_built):
    """[(image id, [(class, (l, t, r, b), difficult)], [(class, score text, (l, t, r, b))])] in sorted id order."""
    images = []
    for i in range(n_img):
        gts, dets = [], []
        for _ in range(int(rng.integers(0, 5))):
            l, t = int(rng.integers(0, 200)), int(rng.integers(0, 200))
            w, h = int(rng.integers(10, 80)), int(rng.integers(10, 80))
            gts.append((NAMES[int(rng.integers(0, len(NAMES)))], (l, t, l + w, t + h), bool(rng.random() < 0.15)))
        for name, box, _ in gts:
            for _ in range((rng.random() < 0.8) + (rng.random() < 0.3)):                 # 0, 1 or 2 jittered copies
                cls = name if rng.random() < 0.9 else NAMES[int(rng.integers(0, len(NAMES)))]
                dets.append((cls, tuple(int(v + rng.integers(-6, 7)) for v in box)))
        for _ in range(int(rng.integers(0, 3))):                                        # boxes on nothing, any class
            l, t = int(rng.integers(0, 200)), int(rng.integers(0, 200))
            dets.append(((NAMES + [GHOST])[int(rng.integers(0, len(NAMES) + 1))],
                         (l, t, l + int(rng.integers(10, 80)), t + int(rng.integers(10, 80)))))
        dets = [d for d in dets if d[0] != "buoy"]
        if rng.random() < 0.1:
            dets = []
        dets = [dets[k] for k in rng.permutation(len(dets))]
        # two decimals for most scores: about a quarter of them tie inside a class
        scored = [(c, repr(round(float(rng.random()), 2 if rng.random() < 0.6 else 4)), b) for c, b in dets]
        images.append((f"img{i:04d}", gts, scored))
    if hand_built:
        # IoU exactly 0.5: 100 / (100 + 200 - 100)
        images.append(("zz_exact", [("boat", (0, 0, 9, 19), False)], [("boat", "0.9", (0, 0, 9, 9))]))
        # best match difficult (IoU 1) while a non-difficult box passes every threshold too (IoU 0.826)
        images.append(("zz_hard", [("boat", (10, 10, 50, 50), True), ("boat", (12, 12, 52, 52), False)],
                       [("boat", "0.8", (10, 10, 50, 50))]))
        images.append(("zz_nodet", [("pier", (5, 5, 40, 40), False)], []))
        images.append(("zz_nogt", [], [("pier", "0.31", (5, 5, 40, 40)), ("traffic light", "0.31", (1, 2, 30, 40))]))
    return sorted(images)


def write_dir(root, images):
    os.makedirs(os.path.join(root, "ground-truth"))
    os.makedirs(os.path.join(root, "detection-results"))
    gt_text, dr_text = [], []
    for iid, gts, dets in images:
        g = "".join("%s %d %d %d %d%s\n" % ((n,) + b + (" difficult" if d else "",)) for n, b, d in gts)
        r = "".join("%s %s %d %d %d %d\n" % ((n, s) + b) for n, s, b in dets)
        open(os.path.join(root, "ground-truth", iid + ".txt"), "w").write(g)
        open(os.path.join(root, "detection-results", iid + ".txt"), "w").write(r)
        gt_text.append(g)
        dr_text.append(r)
    return gt_text, dr_text


def arrays(images):
    names = sorted({n for _, gts, dets in images for n, *_ in gts} | {n for _, gts, dets in images for n, *_ in dets})
    cid = {n: k for k, n in enumerate(names)}
    det = [(i, cid[n], float(s), b) for i, (_, _, dets) in enumerate(images) for n, s, b in dets]
    gt = [(i, cid[n], b, d) for i, (_, gts, _) in enumerate(images) for n, b, d in gts]
    return names, dict(det_image=np.array([d[0] for d in det], dtype=np.int32), det_label=np.array([d[1] for d in det], dtype=np.int32),
                       det_score=np.array([d[2] for d in det], dtype=np.float64),
                       det_box=np.array([d[3] for d in det], dtype=np.float64).reshape(-1, 4),
                       gt_image=np.array([g[0] for g in gt], dtype=np.int32), gt_label=np.array([g[1] for g in gt], dtype=np.int32),
                       gt_box=np.array([g[2] for g in gt], dtype=np.float64).reshape(-1, 4),
                       gt_difficult=np.array([g[3] for g in gt], dtype=np.uint8))


def iou(b, g):
    iw = min(b[2], g[2]) - max(b[0], g[0]) + 1
    ih = min(b[3], g[3]) - max(b[1], g[1]) + 1
    if iw <= 0 or ih <= 0:
        return -1.0
    return iw * ih / ((b[2] - b[0] + 1) * (b[3] - b[1] + 1) + (g[2] - g[0] + 1) * (g[3] - g[1] + 1) - iw * ih)


def check_coverage(sets):
    """Each situation of the issue's list, over all sets; the assertion is the condition."""
    seen = dict.fromkeys(("difficult", "tie", "several on one gt", "best is difficult, another passes", "gt without det",
                          "det without gt", "image without det", "image without gt", "iou == threshold"), False)
    for images in sets:
        gt_cls = {n for _, gts, _ in images for n, _, d in gts if not d}
        det_cls = {n for _, _, dets in images for n, *_ in dets}
        seen["gt without det"] |= bool(gt_cls - det_cls)
        seen["det without gt"] |= bool(det_cls - {n for _, gts, _ in images for n, *_ in gts})
        scores = {}
        for _, gts, dets in images:
            seen["difficult"] |= any(d for *_, d in gts)
            seen["image without det"] |= not dets and bool(gts)
            seen["image without gt"] |= not gts and bool(dets)
            claimed = {}
            for n, s, b in dets:
                scores.setdefault(n, []).append(float(s))
                ov = [(iou(b, g), k, d) for k, (gn, g, d) in enumerate(gts) if gn == n]
                if not ov:
                    continue
                best = max(ov, key=lambda x: x[0])
                seen["iou == threshold"] |= best[0] in THRESHOLDS
                if best[0] >= 0.5:
                    claimed[best[1]] = claimed.get(best[1], 0) + 1
                    seen["best is difficult, another passes"] |= best[2] and any(o >= 0.5 and not d for o, _, d in ov)
            seen["several on one gt"] |= any(v > 1 for v in claimed.values())
        seen["tie"] |= any(len(v) != len(set(v)) for v in scores.values())
    assert all(seen.values()), seen


def run_reference(um, root, names, thr):
    calls = {"ap": [], "lamr": []}
    voc_ap, lamr_fn = um.voc_ap, um.log_average_miss_rate

    def rec_voc_ap(rec, prec):
        r, p = list(rec), list(prec)
        out = voc_ap(rec, prec)
        calls["ap"].append((r, p, out[0]))
        return out

    def rec_lamr(precision, fp_cumsum, num_images):
        out = lamr_fn(precision, fp_cumsum, num_images)
        calls["lamr"].append(float(out[0]))
        return out

    um.voc_ap, um.log_average_miss_rate = rec_voc_ap, rec_lamr
    try:
        with contextlib.redirect_stdout(io.StringIO()):
            m = um.get_map(thr, False, path=root)
    finally:
        um.voc_ap, um.log_average_miss_rate = voc_ap, lamr_fn
    text = open(os.path.join(root, "results", "results.txt")).read()
    shutil.rmtree(os.path.join(root, "results"))                   # get_map removes an existing one and then cannot write
    # "# Number of detected objects per class": `name: n (tp:a, fp:b)`.  The reference keys these lines by the FIRST token
    # of a detection line (:670), so a class whose name has a space is not counted under its name: -1 = not reported.
    tp = {mm.group(1): int(mm.group(2)) for mm in re.finditer(r"^(.+): \d+ \(tp:(\d+), fp:\d+\)$", text, re.M)}
    evaluated = sorted({n for n in names} & set(gt_classes_of(root)))
    assert len(calls["ap"]) == len(calls["lamr"]) == len(evaluated)
    return dict(map=float(m), cls=np.array([names.index(n) for n in evaluated], dtype=np.int32),
                len=np.array([len(c[0]) for c in calls["ap"]], dtype=np.int32),
                rec=np.array([v for c in calls["ap"] for v in c[0]], dtype=np.float64),
                prec=np.array([v for c in calls["ap"] for v in c[1]], dtype=np.float64),
                ap=np.array([c[2] for c in calls["ap"]], dtype=np.float64), lamr=np.array(calls["lamr"], dtype=np.float64),
                tp=np.array([tp.get(n, -1) if " " not in n else -1 for n in names], dtype=np.int32))


def gt_classes_of(root):
    """Classes with a non-difficult ground truth: the ones get_map evaluates, in its sorted order (:380-381)."""
    out = set()
    for fn in os.listdir(os.path.join(root, "ground-truth")):
        for line in open(os.path.join(root, "ground-truth", fn)):
            tok = line.split()
            if tok and tok[-1] != "difficult":
                out.add(" ".join(tok[:-4]))
    return sorted(out)


def main():
    ref = sys.argv[1]
    rng = np.random.default_rng(20261017)
    sets = [synthetic_set(rng, 10, True), synthetic_set(rng, 40, False), synthetic_set(rng, 70, False)]
    check_coverage(sets)
    out = {"thresholds": np.array(THRESHOLDS), "n_sets": len(sets)}
    with tempfile.TemporaryDirectory() as tmp:
        write_stub(os.path.join(tmp, "stubs"))
        sys.path[:0] = [os.path.join(tmp, "stubs"), ref]
        sys.dont_write_bytecode = True
        from utils import utils_map as um
        for s, images in enumerate(sets):
            root = os.path.join(tmp, f"set{s}")
            gt_text, dr_text = write_dir(root, images)
            names, arr = arrays(images)
            out[f"s{s}_names"] = np.array(names)
            out.update({f"s{s}_{k}": v for k, v in arr.items()})
            if s == 0:
                out.update(s0_ids=np.array([i for i, _, _ in images]), s0_gt_text=np.array(gt_text), s0_dr_text=np.array(dr_text))
            for j, thr in enumerate(THRESHOLDS):
                res = run_reference(um, root, names, thr)
                out.update({f"s{s}_t{j}_{k}": v for k, v in res.items()})
                print(f"set {s} thr {thr}: {len(arr['det_score'])} detections, {len(arr['gt_label'])} ground truths, "
                      f"mAP {res['map']:.6f}, tp {res['tp'].tolist()}")
    dst = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "tests", "golden", "detmap_small.npz")
    np.savez_compressed(dst, **out)
    print("wrote", os.path.normpath(dst), os.path.getsize(dst), "bytes")


if __name__ == "__main__":
    main()
