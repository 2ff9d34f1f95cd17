"""Golden vectors for `data.merge_boxes`: inputs and outputs of the reference's OWN `YoloDataset.merge_bboxes`
(utils/dataloader.py:251-295), imported behind the throw-away cv2 / albumentations stubs of tools/make_golden_dataset.py (the
method touches neither).  Three cuts on a 64 x 48 canvas, four box lists each; coordinates are drawn from a small set around
the cut, so that boxes touch the cut line exactly from either side, and the generator asserts that for every tile its inputs
reach the skip, the y clip alone, the x clip alone, both clips and no clip, and all four kinds of touch.  Arrays only:
tests/golden/mosaic_merge.npz.
    python tools/make_golden_mosaic.py [path of the reference checkout]"""
import os
import sys
import tempfile

import numpy as np

from make_golden_dataset import REF, write_stubs

W, H = 64, 48
CUTS = [(30, 20), (19, 33), (45, 24)]


def branch(i, box, cutx, cuty):
    """Which branch of merge_bboxes a box of tile i takes, restated from its conditions: "skip", or which clips fire."""
    x1, y1, x2, y2 = box[:4]
    skip = ((y1 > cuty or x1 > cutx), (y2 < cuty or x1 > cutx), (y2 < cuty or x2 < cutx), (y1 > cuty or x2 < cutx))[i]
    if skip:
        return "skip"
    return {(False, False): "none", (True, False): "y", (False, True): "x", (True, True): "xy"}[
        (bool(y2 >= cuty and y1 <= cuty), bool(x2 >= cutx and x1 <= cutx))]


def boxes_around(rng, cutx, cuty, n):
    xs = np.array([0, 3, cutx - 7, cutx - 1, cutx, cutx + 1, cutx + 8, W - 2, W])
    ys = np.array([0, 2, cuty - 6, cuty - 1, cuty, cuty + 1, cuty + 5, H - 3, H])
    out = np.zeros((n, 5))
    for k in range(n):
        x1, x2 = np.sort(rng.choice(xs, 2, replace=False))
        y1, y2 = np.sort(rng.choice(ys, 2, replace=False))
        out[k] = (x1, y1, x2, y2, rng.integers(0, 4))
    return out


def main():
    ref = sys.argv[1] if len(sys.argv) > 1 else REF
    rng = np.random.default_rng(20261019)
    with tempfile.TemporaryDirectory() as tmp:
        write_stubs(os.path.join(tmp, "stubs"))
        sys.path[:0] = [os.path.join(tmp, "stubs"), ref]
        sys.dont_write_bytecode = True
        from utils.dataloader import YoloDataset
        out = {"cuts": np.array(CUTS), "canvas": np.array([H, W])}
        seen = {i: set() for i in range(4)}
        touch = {i: set() for i in range(4)}
        for k, (cutx, cuty) in enumerate(CUTS):
            lists = [boxes_around(rng, cutx, cuty, 40) for _ in range(4)]
            lists[k % 4] = np.zeros((0, 5))                          # a tile without boxes
            for i, boxes in enumerate(lists):
                for box in boxes:
                    seen[i].add(branch(i, box, cutx, cuty))
                    touch[i] |= {name for name, hit in (("x1", box[0] == cutx), ("y1", box[1] == cuty), ("x2", box[2] == cutx),
                                                        ("y2", box[3] == cuty)) if hit}
                out[f"boxes_{k}_{i}"] = boxes
            merged = YoloDataset.merge_bboxes(None, [b.copy() for b in lists], cutx, cuty)
            out[f"merged_{k}"] = np.array(merged, dtype=np.float64).reshape(-1, 5)
    for i in range(4):
        assert seen[i] == {"skip", "none", "y", "x", "xy"}, (i, seen[i])
        assert touch[i] == {"x1", "y1", "x2", "y2"}, (i, touch[i])
    dst = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "tests", "golden", "mosaic_merge.npz")
    np.savez_compressed(dst, **out)
    print("wrote", dst, os.path.getsize(dst), "bytes; merged rows:", [len(out[f"merged_{k}"]) for k in range(len(CUTS))])


if __name__ == "__main__":
    main()
