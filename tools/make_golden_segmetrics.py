"""Golden values for the segmentation metrics (csrc/segpost.hip, the f_score of csrc/loss.hip), from the reference's own
utils_seg/utils_metrics.py (`f_score`, `fast_hist`) and utils_seg/utils.py (`resize_image`, whose (nw, nh) is the
letterbox window seg_predict crops).  Both import without OpenCV.

Logits are N(0, 3^2) and every pixel that has an fp64 softmax probability within 1e-4 of a threshold used here is
redrawn, so every threshold decision of the fixture is unambiguous.

    python tools/make_golden_segmetrics.py       # writes tests/golden/segmetrics_small.npz
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, HERE)
from ref_harness import REF_ROOT  # noqa: E402

sys.dont_write_bytecode = True
sys.path.insert(0, REF_ROOT)
from PIL import Image  # noqa: E402
from utils_seg.utils import resize_image  # noqa: E402
from utils_seg.utils_metrics import f_score, fast_hist  # noqa: E402

THRESHOLDS = (0.5, 0.3)
BETAS = (1, 2)
MARGIN = 1e-4
SIZES = [(1080, 1920), (480, 640), (517, 333), (512, 512), (60, 100)]      # (ih, iw) of an original image
INPUT = (512, 512)                                                          # (H, W) of the network input


def softmax64(x):
    x = x.astype(np.float64)
    e = np.exp(x - x.max(axis=1, keepdims=True))
    return e / e.sum(axis=1, keepdims=True)


def draw_logits(rng, shape):
    """(B, C, H, W) float32, redrawing whole pixels until no probability lies within MARGIN of a threshold."""
    x = (3.0 * rng.standard_normal(shape)).astype(np.float32)
    while True:
        p = softmax64(x)
        close = np.zeros((shape[0], shape[2], shape[3]), bool)
        for t in THRESHOLDS:
            close |= (np.abs(p - t) < MARGIN).any(axis=1)
        if not close.any():
            return x
        b, i, j = np.nonzero(close)
        x[b, :, i, j] = (3.0 * rng.standard_normal((len(b), shape[1]))).astype(np.float32)


if __name__ == "__main__":
    rng = np.random.default_rng(1207)
    out = {}
    B, H, W = 2, 24, 40
    for C in (9, 21):
        x = draw_logits(rng, (B, C, H, W))
        labels = rng.integers(0, C + 1, size=(B, H, W)).astype(np.uint8)        # C = the ignore class (dropped channel)
        agree = rng.random((B, H, W)) < 0.6                                     # most labels follow the logits: tp > 0
        labels[agree] = x.argmax(axis=1).astype(np.uint8)[agree]
        onehot = np.eye(C + 1, dtype=np.float32)[labels]
        scores = np.array([[float(f_score(torch.from_numpy(x), torch.from_numpy(onehot), beta=b, smooth=1e-5, threhold=t))
                            for t in THRESHOLDS] for b in BETAS], np.float32)
        out[f"fscore_c{C}_logits"] = x
        out[f"fscore_c{C}_labels"] = labels
        out[f"fscore_c{C}_scores"] = scores                                     # [beta][threshold]
    n, N = 9, 5000
    a = rng.integers(0, n + 1, size=N).astype(np.uint8)                          # labels, n included
    a[rng.random(N) < 0.05] = 255                                               # VOC "void" pixels
    b = rng.integers(0, n, size=N).astype(np.uint8)
    out.update(hist_n=np.array(n), hist_label=a, hist_pred=b, hist=fast_hist(a, b, n).astype(np.int64))
    nwnh = [resize_image(Image.new("RGB", (iw, ih)), (INPUT[1], INPUT[0]))[1:] for ih, iw in SIZES]
    out.update(win_input=np.array(INPUT), win_sizes=np.array(SIZES), win_nwnh=np.array(nwnh))
    out.update(thresholds=np.array(THRESHOLDS), betas=np.array(BETAS), smooth=np.array(1e-5))
    path = os.path.join(ROOT, "tests", "golden", "segmetrics_small.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes; windows", nwnh)
