"""Seeded frame pairs for the image-metrics tests: the four families of tests/golden/metrics/cases.npz (made from here by
tests/golden/make_metrics_golden.py) and the larger shapes that come from the seed instead of a file."""
import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "metrics")
FAMILIES = ("noise", "near", "ramp", "flat")
GOLDEN_SIZES = ((1, 1), (3, 5), (11, 11), (12, 33), (37, 70))          # h, w
TILE_Y, TILE_X = 16, 64          # ADAIN_METRICS_TILE_Y, ADAIN_METRICS_TILE_X: rows x samples of a workgroup (a packed RGB row has 3 w samples)


def pair(family, n, h, w, c=3, seed=0):
    """(a, b) uint8 [n,h,w,c], every frame pair different:
    noise: uniform noise against other noise;  near: noise against itself +-3;  ramp: (3x + 2y + 5 channel + 7 frame) % 256 against
    itself +-1;  flat: 200 against itself with one sample changed."""
    rng = np.random.default_rng([seed, FAMILIES.index(family), n, h, w, c])
    shape = (n, h, w, c)
    if family == "noise":
        return rng.integers(0, 256, shape, dtype=np.uint8), rng.integers(0, 256, shape, dtype=np.uint8)
    if family == "near":
        a = rng.integers(0, 256, shape, dtype=np.uint8)
        return a, np.clip(a.astype(np.int16) + rng.integers(-3, 4, shape), 0, 255).astype(np.uint8)
    if family == "ramp":
        i, y, x, ch = np.meshgrid(np.arange(n), np.arange(h), np.arange(w), np.arange(c), indexing="ij")
        a = ((3 * x + 2 * y + 5 * ch + 7 * i) % 256).astype(np.uint8)
        return a, np.clip(a.astype(np.int16) + rng.choice([-1, 1], shape), 0, 255).astype(np.uint8)
    if family == "flat":
        a = np.full(shape, 200, dtype=np.uint8)
        b = a.copy()
        for i in range(n):
            b[i, rng.integers(h), rng.integers(w), rng.integers(c)] = 17 + 40 * i
        return a, b
    raise ValueError(family)


def golden_names():
    return [f"{family}_{h}x{w}_c{c}" for family in FAMILIES for h, w in GOLDEN_SIZES for c in (3, 1)]


def load_golden():
    return np.load(os.path.join(GOLDEN, "cases.npz"))


def golden_pair(z, name):
    """The uint8 pair [2,h,w,c] of a golden case: the c = 1 case is channel 0 of the c = 3 one."""
    base = name[:-1] + "3"
    a, b = z[base + "_a"], z[base + "_b"]
    return (a, b) if name.endswith("c3") else (np.ascontiguousarray(a[..., :1]), np.ascontiguousarray(b[..., :1]))


def to_nchw_f32(u8):
    """to_tensor: uint8 [n,h,w,c] -> float32 [n,c,h,w], x / 255 by a float32 division."""
    return np.ascontiguousarray((u8.astype(np.float32) / np.float32(255.0)).transpose(0, 3, 1, 2))


# seeded shapes around the kernel's tile: T - 1, T, T + 1, 2 T + 1 on each axis, in samples; a packed RGB row has 3 w samples, so w = 21,
# 22, 43 put 63, 66 and 129 samples in a row; 130 x 97; h < 11 <= w and w < 11 <= h.  (family, h, w)
TILE_SHAPES = (
    ("noise", TILE_Y - 1, TILE_X - 1), ("near", TILE_Y, TILE_X), ("ramp", TILE_Y + 1, TILE_X + 1), ("near", 2 * TILE_Y + 1, 2 * TILE_X + 1),
    ("ramp", TILE_Y + 1, 21), ("noise", TILE_Y, 22), ("near", 5, 43),
    ("noise", 130, 97), ("near", 7, 40), ("ramp", 40, 7), ("flat", 20, 70),
)
