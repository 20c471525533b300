"""Frames for the palette refinement's tests (tests/quantize_refine_ref.py states the rules): cases whose answer is worked out by hand
from rules 1-11, and the frames the device tests share."""
import numpy as np

from quantize_cases import gradient, noise, reds, row

TWO_IN_ONE_CELL = row((0, 0, 0), (7, 7, 7), (7, 7, 7), (0, 0, 0))
FLAT = row((9, 9, 9), (9, 9, 9), (9, 9, 9))
# cells 0: {7}, 1: {10, 15}, 2: {17}, 4: {32, 37}.  The cut: {7, 10, 15} | {17, 32, 37} (half of 6 is reached at cell 1); the right box has
# the larger error and is cut into {17} | {32, 37} (box 2); then the left into {7} | {10, 15} (box 3): P = 7, 17, 35, 13 and every box is
# one cell, so used = 4.  Round 1: 10 is 3 away from 7 and from 13 and goes to entry 0, 15 is 2 away from 17 and from 13 and goes to
# entry 1: entry 3 is live and has no pixel.  Entries 0..2: {7, 10} -> 9 (8.5 half up), far 10 at d = 9; {15, 17} -> 16, far 15 at d = 4;
# {32, 37} -> 35 (34.5), far 32 at d = 9.  The donors in order: 0 (d 9), 2 (d 9), 1 (d 4).
LOST = reds(37, 10, 32, 7, 15, 17)

# (name, frames [1,1,N,3], K, T, the expected first `used` entries), each by hand from the rules
HAND = [
    # the cut: {0, 0} | {8, 24}, P = 0, 16.  8 is 8 away from both and goes to entry 0: {0, 0, 8} -> (2 * 8 + 3) // 6 = 3, {24} -> 24.  (To
    # entry 1 it would give 0 and 16.)
    ("a tie goes to the lower index", reds(0, 0, 8, 24), 2, 1, [(3, 0, 0), (24, 0, 0)]),
    # the cut along g: {0, 1} | {255, 255}; round 1 keeps the clusters: S = 1, n = 2: (2 * 1 + 2) // 4 = 1 - round half up
    ("rule 9 rounds half up", row((0, 0, 0), (0, 1, 0), (0, 255, 0), (0, 255, 0)), 2, 1, [(0, 1, 0), (0, 255, 0)]),
    # one cell: used = 1 and P_0 = (2 * 14 + 4) // 8 = 4 per channel
    ("two colours in one cell, T = 0", TWO_IN_ONE_CELL, 2, 0, [(4, 4, 4)]),
    # (0, 0, 0) is 48 away, (7, 7, 7) 27: slot 1 takes (0, 0, 0); the centre stays (4, 4, 4)
    ("two colours in one cell, T = 1", TWO_IN_ONE_CELL, 2, 1, [(4, 4, 4), (0, 0, 0)]),
    # now (0, 0, 0) goes to entry 1 and (7, 7, 7) stays with entry 0 (27 against 147)
    ("two colours in one cell, T = 2", TWO_IN_ONE_CELL, 2, 2, [(7, 7, 7), (0, 0, 0)]),
    ("two colours in one cell, T = 3: a fixed point", TWO_IN_ONE_CELL, 2, 3, [(7, 7, 7), (0, 0, 0)]),
    # P_0 = (2 * 6 + 2) // 4 = 3: both colours are 9 away, the smaller r, g, b value is given
    ("equally far colours: the smaller value", row((0, 0, 0), (6, 0, 0)), 2, 1, [(3, 0, 0), (0, 0, 0)]),
    ("one flat colour has no donor, T = 1", FLAT, 2, 1, [(9, 9, 9)]),
    ("one flat colour has no donor, T = 64", FLAT, 2, 64, [(9, 9, 9)]),
    # two cells, K = 3: P = 1, 11 and one free slot; entry 1's far colour 8 is 9 away, entry 0's (0) only 1
    ("more donors than slots: the largest distance", reds(0, 2, 8, 14), 3, 1, [(1, 0, 0), (11, 0, 0), (8, 0, 0)]),
    # P = 1, 9: both far colours are 1 away; entry 0 gives, and of its 0 and 2 the smaller
    ("more donors than slots: the lower index", reds(0, 2, 8, 10), 3, 1, [(1, 0, 0), (9, 0, 0), (0, 0, 0)]),
    # the free slots are 3 (live, without a pixel) and 4: slot 3 takes the first donor's 10, slot 4 the second's 32
    ("a live entry without pixels is filled first", LOST, 5, 1, [(9, 0, 0), (16, 0, 0), (35, 0, 0), (10, 0, 0), (32, 0, 0)]),
    # K = 4: slot 3 is the only free one and used stays 4
    ("a live entry without pixels, no slot behind used", LOST, 4, 1, [(9, 0, 0), (16, 0, 0), (35, 0, 0), (10, 0, 0)]),
]


def expected(entries):
    """(uint8 [256,3], used) of a HAND case."""
    pal = np.zeros((256, 3), dtype=np.uint8)
    pal[:len(entries)] = entries
    return pal, len(entries)


def few_colours(n, h, w, colours, seed):
    """uint8 [n,h,w,3] of noise over ``colours`` distinct random colours: every pixel its own entry's run, and a restatement that loops
    over the distinct colours stays quick."""
    rng = np.random.default_rng(seed)
    table = rng.integers(0, 256, (colours, 3), dtype=np.uint8)
    return table[rng.integers(0, colours, (n, h, w))]


def banded(n, h, w, seed):
    """uint8 [n,h,w,3]: tests/quantize_cases.py's gradient with 16 levels a channel - stretches of one colour, as a stylised frame has
    them: the runs a thread merges and the waves that hold one entry."""
    return (gradient(n, h, w, seed) >> 4) * 17


# (name, frames [n,h,w,3]) of the device tests: one pixel; fewer pixels than a 16-byte load; two small clips; more slots than a cell has
# colours; the two hand cases; one pixel below a tile of 4096, a tile, one above; and a clip whose one palette has several workgroups
def device_frames():
    return [("1x1", np.asarray([[[[200, 100, 7]]]], dtype=np.uint8)), ("3x5", noise(1, 3, 5, 7)), ("gradient 2x9x11", gradient(2, 9, 11)),
            ("noise 2x16x24", noise(2, 16, 24)), ("two colours in one cell", TWO_IN_ONE_CELL), ("flat", FLAT), ("1x4095", few_colours(1, 1, 4095, 300, 11)),
            ("1x4096", few_colours(1, 1, 4096, 300, 12)), ("1x4097", few_colours(1, 1, 4097, 300, 13))]


def several_workgroups():
    return banded(3, 96, 97, 5)


TS = (1, 2, 8)
DEVICE_KS = (1, 2, 16, 256)
