"""Times metrics.coco_map on the seeded 2 000-image, 110 000-detection set of tests/test_detmap.py: the whole call from numpy
arrays on the host to the 12 COCO numbers on the host (upload, sorts, grouping, range check, kernels, read-back), and, in
the same process and alternating with it call by call, metrics.voc_map with ten thresholds on the same arrays -- the
nearest thing the package computed before coco_map existed.  Medians of `--runs` calls after a warm-up, with min and max.
Kernel times: run it under `rocprofv3 --kernel-trace --stats -- python tools/bench_cocomap.py` and read the cm_* rows.
    python tools/bench_cocomap.py [--runs 30]"""
import argparse
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

import numpy as np
import torch

from asy_vrnet_amd.metrics import COCO_IOU_THRS, coco_map, voc_map
from test_detmap import random_case


def once(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()                                       # ends in a read-back: the device is idle when it returns
    return (time.perf_counter() - t0) * 1e3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=30)
    runs = ap.parse_args().runs
    arr = random_case(20261017, 2000, 55)
    key = arr["det_image"] * 20 + arr["det_label"]
    groups, per_group = np.unique(key, return_counts=True)
    print(f"{len(arr['det_score'])} detections, {len(arr['gt_label'])} ground truths, 2000 images, 20 classes, "
          f"{len(groups)} (image, class) groups with a detection, at most {per_group.max()} detections in one", flush=True)
    thr = [float(v) for v in COCO_IOU_THRS]
    fns = (("coco_map", lambda: coco_map(**arr, num_classes=20).stats.cpu()),
           ("voc_map, 10 thresholds", lambda: voc_map(**arr, num_classes=20, min_overlap=thr).map.cpu()))
    for _ in range(5):
        for _, fn in fns:
            fn()
    ts = {name: [] for name, _ in fns}
    for _ in range(runs):
        for name, fn in fns:
            ts[name].append(once(fn))
    for name, _ in fns:
        v = ts[name]
        print(f"{name} end to end: median {statistics.median(v):.3f} ms (min {min(v):.3f}, max {max(v):.3f}) over {runs} runs",
              flush=True)
    stats = coco_map(**arr, num_classes=20).stats.cpu().numpy()
    print("stats", " ".join(f"{v:.4f}" for v in stats), flush=True)


if __name__ == "__main__":
    main()
