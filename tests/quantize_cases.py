"""Frames for the palette chooser's tests (tests/quantize_ref.py states the rules): cases whose answer is worked out by hand, and the
generated frames the device tests share with tools/quantize_dump_cases.py."""
import numpy as np


def row(*pixels):
    """One frame of one row: uint8 [1,1,len,3]."""
    return np.asarray(pixels, dtype=np.uint8).reshape(1, 1, -1, 3)


def reds(*values):
    return row(*[(v, 0, 0) for v in values])


# (name, frames [1,1,N,3], K, the expected first `used` entries), each by hand from the rules
HAND = [
    ("one pixel", row((10, 20, 30)), 5, [(10, 20, 30)]),
    # S = 1, w = 2: (2 * 1 + 2) // 4 = 1 - round half up
    ("0 and 1 in one cell", row((0, 0, 0), (1, 1, 1)), 4, [(1, 1, 1)]),
    # slab counts (1, 1, 1, 1): ceil(4 / 2) = 2 is reached at the second slab
    ("slabs 1 1 1 1", reds(0, 8, 16, 24), 2, [(4, 0, 0), (20, 0, 0)]),
    # (3, 1): 2 is reached at lo
    ("slabs 3 1", reds(0, 1, 2, 8), 2, [(1, 0, 0), (8, 0, 0)]),
    # (1, 3): 2 is reached at hi, and k = hi - 1
    ("slabs 1 3", reds(0, 8, 9, 10), 2, [(0, 0, 0), (9, 0, 0)]),
    # (1, 1, 3): 3 is reached at hi = lo + 2, k = hi - 1: the lower box keeps two slabs
    ("slabs 1 1 3", reds(0, 8, 16, 17, 18), 2, [(4, 0, 0), (17, 0, 0)]),
    # after the first cut boxes 0 = {0, 8} and 1 = {16, 24} both have E = 32: box 0 is split, its upper half becomes box 2
    ("an E tie", reds(0, 8, 16, 24), 3, [(0, 0, 0), (20, 0, 0), (8, 0, 0)]),
    # a 2 x 2 x 2 block of cells: g is cut first
    ("equal sides g", row(*[(r, g, b) for r in (0, 8) for g in (0, 8) for b in (0, 8)]), 2, [(4, 0, 4), (4, 8, 4)]),
    # g has one cell, r and b two: r is cut
    ("equal sides r", row(*[(r, 0, b) for r in (0, 8) for b in (0, 8)]), 2, [(0, 0, 4), (8, 0, 4)]),
    # three cells, K = 10: used = 3.  First cut along r (slabs 1, 1, 1 -> k at the second): {0, 8} and {16}; then {0}, {16}, {8}
    ("K above the cells", reds(0, 8, 16), 10, [(0, 0, 0), (16, 0, 0), (8, 0, 0)]),
]


def expected(entries):
    """(uint8 [256,3], used) of a HAND case."""
    pal = np.zeros((256, 3), dtype=np.uint8)
    pal[:len(entries)] = entries
    return pal, len(entries)


def noise(n, h, w, seed=0):
    return np.random.default_rng(seed).integers(0, 256, (n, h, w, 3), dtype=np.uint8)


def gradient(n, h, w, seed=0):
    """A smooth ramp per channel with a few levels of noise on top: coherent, as a stylised frame is."""
    rng = np.random.default_rng(seed)
    y, x = np.mgrid[0:h, 0:w]
    frames = []
    for f in range(n):
        base = np.stack([(x * 255) // max(1, w - 1), (y * 255) // max(1, h - 1), ((x + y + 17 * f) * 255) // max(1, w + h + 17 * n)], axis=-1)
        frames.append(np.clip(base + rng.integers(-6, 7, base.shape), 0, 255))
    return np.stack(frames).astype(np.uint8)


def every_cell_once():
    """uint8 [1,128,256,3]: each of the 32 768 cells holds one pixel, the cell's lowest colour - every choice is a tie."""
    c = np.arange(32768)
    return np.stack([(c >> 10) << 3, ((c >> 5) & 31) << 3, (c & 31) << 3], axis=-1).astype(np.uint8).reshape(1, 128, 256, 3)


def mirrored(h=16, w=24, seed=3):
    """uint8 [1,h,2w,3]: a noise frame beside its mirror image in r (r -> 255 - r): the first cut is along r, between the halves,
    and leaves two boxes of equal E."""
    left = noise(1, h, w, seed)[0]
    left[..., 0] >>= 1          # r in 0..127, cells 0..15
    left[..., 1:] >>= 2         # g and b in 8 cells each: r is the longest side
    right = left[:, ::-1].copy()
    right[..., 0] = 255 - right[..., 0]
    return np.concatenate([left, right], axis=1)[None]


# (name, frames [n,h,w,3]) of the generated cases
def generated():
    return [("noise 3x37x53", noise(3, 37, 53, 1)), ("gradient 3x37x53", gradient(3, 37, 53, 2)), ("mirrored", mirrored()), ("every cell once", every_cell_once()),
            ("noise 1x90x100", noise(1, 90, 100, 4))]


KS = (2, 5, 16, 255, 256)
