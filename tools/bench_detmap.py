"""Times metrics.voc_map on the seeded 2 000-image, 110 000-detection set of tests/test_detmap.py: the whole call from numpy
arrays on the host to the mAP as a Python float (upload, sort, grouping, kernels, read-back), as the median of `--runs`
calls after a warm-up, for one threshold, for ten, and with every detection in one class (the curve kernel is one
workgroup per (class, threshold)).  Kernel times: run it under `rocprofv3 --kernel-trace --stats -- python tools/bench_detmap.py`
and read the dm_* rows.
    python tools/bench_detmap.py [--runs 30]"""
import argparse
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

import numpy as np
import torch

from asy_vrnet_amd.metrics import voc_map
from test_detmap import random_case


def timed(fn, runs, warmup=5):
    for _ in range(warmup):
        fn()
    ts = []
    for _ in range(runs):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()                                   # ends in a read-back: the device is idle when it returns
        ts.append((time.perf_counter() - t0) * 1e3)
    return statistics.median(ts), min(ts), max(ts)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=30)
    runs = ap.parse_args().runs
    arr = random_case(20261017, 2000, 55)
    print(f"{len(arr['det_score'])} detections, {len(arr['gt_label'])} ground truths, 2000 images, 20 classes, "
          f"largest class {np.bincount(arr['det_label']).max()} detections", flush=True)
    one = dict(arr, det_label=np.zeros_like(arr["det_label"]), gt_label=np.zeros_like(arr["gt_label"]))
    for name, fn in (("1 threshold", lambda: float(voc_map(**arr, num_classes=20, min_overlap=0.5).map)),
                     ("10 thresholds", lambda: voc_map(**arr, num_classes=20, min_overlap=[0.5 + 0.05 * k for k in range(10)]).map.cpu()),
                     ("1 threshold, one class", lambda: float(voc_map(**one, num_classes=1, min_overlap=0.5).map))):
        med, lo, hi = timed(fn, runs)
        print(f"voc_map end to end, {name}: median {med:.3f} ms (min {lo:.3f}, max {hi:.3f}) over {runs} runs", flush=True)


if __name__ == "__main__":
    main()
