"""Writes tests/golden/heatmap_jet.npz: what matplotlib does with the integer mask of yolo.py:344
`plt.imshow(mask, alpha=0.5, cmap="jet")`, recorded from matplotlib alone (nothing of the reference is imported or run).

  jet      (256, 3) uint8   matplotlib.colormaps["jet"](arange(256), bytes=True)[:, :3]
  pairs    (n, 2)   int32   (vmin, vmax) of a mask, vmin <= vmax: imshow's default normalisation takes them from the image
  indices  (n, 256) uint8   row k, column m: the colour index matplotlib gives mask value m under Normalize(*pairs[k]), for
                            vmin <= m <= vmax; 0 elsewhere (such values do not occur in the image)

The index is read back from a probe colour map whose entry i is the colour (i / 255, 0, 0): Colormap.__call__ is the same
code for every colour map, so the red channel of the float result names the entry that was looked up.

    python tools/make_golden_heatmap.py
"""
import os

import matplotlib
import numpy as np
from matplotlib.colors import ListedColormap, Normalize

OUT = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests", "golden", "heatmap_jet.npz")


def main():
    jet = matplotlib.colormaps["jet"](np.arange(256), bytes=True)[:, :3].astype(np.uint8)
    probe = ListedColormap([(i / 255.0, 0.0, 0.0) for i in range(256)])
    pairs = [(0, 255), (0, 1), (254, 255), (0, 0), (255, 255), (7, 7), (0, 254), (1, 255), (0, 2), (0, 3), (3, 250), (17, 200),
             (100, 101), (100, 103), (0, 127), (0, 128), (128, 255), (5, 12), (0, 85), (0, 170), (0, 51), (0, 49), (0, 7)]
    rng = np.random.default_rng(344)
    while len(pairs) < 40:
        lo, hi = sorted(int(v) for v in rng.integers(0, 256, 2))
        if (lo, hi) not in pairs:
            pairs.append((lo, hi))
    indices = np.zeros((len(pairs), 256), np.uint8)
    for k, (lo, hi) in enumerate(pairs):
        m = np.arange(lo, hi + 1, dtype=np.float64)            # the reference's mask is a float64 array of integers
        red = probe(Normalize(vmin=lo, vmax=hi)(m))[:, 0]
        idx = np.rint(red * 255.0).astype(np.int64)
        assert np.array_equal(probe(idx)[:, 0], red)
        indices[k, lo:hi + 1] = idx
    np.savez_compressed(OUT, jet=jet, pairs=np.array(pairs, np.int32), indices=indices)
    print(f"matplotlib {matplotlib.__version__}: {len(pairs)} pairs -> {OUT} ({os.path.getsize(OUT)} bytes)")


if __name__ == "__main__":
    main()
