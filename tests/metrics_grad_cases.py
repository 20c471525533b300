"""Shapes, weights and seeded frames shared by the gradient tests of the image metrics (host and device), and the recorded bars."""
import json
import os

import numpy as np

import metrics_cases as C

# (n, c, h, w), the smallest at which staging, halo or tile indexing can go wrong: one sample; smaller than the window; one window; c = 4;
# exactly one tile; one short of a tile each way; 2 x 2 tiles with one-sample slivers, two frames; 3 x 3 tiles, so that one tile takes its
# whole halo from neighbours
TILE_EDGE = ((1, 1, 1, 1), (2, 3, 3, 5), (1, 1, 11, 11), (1, 4, 12, 33), (1, 1, 16, 64), (1, 2, 15, 63), (2, 3, 17, 65), (1, 1, 33, 129))
# upstream {ssim, mse, l1} per frame (the second row is a second frame's): each alone, and mixed with train.py's negative ssim weight
WEIGHTS = {"ssim": [[1.0, 0.0, 0.0], [0.5, 0.0, 0.0]], "mse": [[0.0, 1.0, 0.0], [0.0, 3.0, 0.0]], "l1": [[0.0, 0.0, 1.0], [0.0, 0.0, 0.25]],
           "mixed": [[-0.2, 0.7, 0.8], [-1.5, -0.3, 0.4]]}


def edge_pair(shape, seed=11):
    """float32 NCHW frames (a, b) of ``shape``: noise against itself +-3 (noise against other noise for a single sample, which +-3 could
    leave equal)."""
    n, c, h, w = shape
    a, b = C.pair("near" if h * w > 1 else "noise", n, h, w, c, seed=seed)
    return C.to_nchw_f32(a), C.to_nchw_f32(b)


def bars():
    with open(os.path.join(C.GOLDEN, "grad_noise.json")) as f:
        return json.load(f)


def equal_frames(a, b):
    return [bool(np.array_equal(a[i], b[i])) for i in range(a.shape[0])]
