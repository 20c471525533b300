"""The palette chooser's rules (top of csrc/quantize.hip) in plain Python ints and loops: what ``runtime.quantize_palette_u8`` and
``pixelize.extract_palette`` are compared with for equality.  Written apart from the package's NumPy form: cells live in a dict, a box is
the list of its non-empty cells, nothing is a prefix sum.

1. A pixel (r, g, b) falls into cell (r >> 3, g >> 3, b >> 3); a cell has the moments w, Sr, Sg, Sb, Q = sum of r^2 + g^2 + b^2.
2. A box is an inclusive cell range, always tight; its moments are the sums over its cells, its error E = Q - (Sr^2 + Sg^2 + Sb^2) / w.
3. While there are fewer than K boxes: of the boxes with more than one cell along some axis, the one with the largest E (exactly; the
   lowest index among equals) is split; without such a box the loop stops.
4. Along its longest side in cells; among equal sides g, then r, then b.
5. At k, the smallest t with m[lo] + ... + m[t] >= ceil(w / 2), at most hi - 1; [lo..k] keeps the index, [k + 1..hi] is appended.
6. Entry i is (2 S_c + w) // (2 w) per channel; entries used..255 are zero.
"""
from fractions import Fraction

import numpy as np

AXIS_ORDER = (1, 0, 2)          # g, then r, then b


def cells_of(pixels, weight=1, cells=None):
    """pixels: an iterable of (r, g, b), each counted ``weight`` times (a whole number: the moments are integers, so a pixel seen
    ``weight`` times adds ``weight`` times its own) -> {cell: [w, Sr, Sg, Sb, Q]}, added into ``cells`` when given."""
    cells = {} if cells is None else cells
    for r, g, b in pixels:
        m = cells.setdefault((r >> 3, g >> 3, b >> 3), [0, 0, 0, 0, 0])
        m[0] += weight
        m[1] += weight * r
        m[2] += weight * g
        m[3] += weight * b
        m[4] += weight * (r * r + g * g + b * b)
    return cells


class Box:
    def __init__(self, cells):
        """cells: a non-empty list of (cell, moments)."""
        self.cells = cells
        self.lo = [min(c[a] for c, _ in cells) for a in range(3)]
        self.hi = [max(c[a] for c, _ in cells) for a in range(3)]
        self.w, self.sr, self.sg, self.sb, self.q = (sum(m[i] for _, m in cells) for i in range(5))

    def error(self):
        return Fraction(self.q) - Fraction(self.sr ** 2 + self.sg ** 2 + self.sb ** 2, self.w)

    def sides(self):
        return [self.hi[a] - self.lo[a] + 1 for a in range(3)]

    def axis(self):
        longest = max(self.sides())
        return next(a for a in AXIS_ORDER if self.sides()[a] == longest)

    def cut(self):
        """(axis, k)."""
        a = self.axis()
        m = {}
        for c, mom in self.cells:
            m[c[a]] = m.get(c[a], 0) + mom[0]
        half = (self.w + 1) // 2
        total = 0
        for t in range(self.lo[a], self.hi[a] + 1):
            total += m.get(t, 0)
            if total >= half:
                return a, min(t, self.hi[a] - 1)
        raise AssertionError("the slab counts sum to w")

    def entry(self):
        return [(2 * s + self.w) // (2 * self.w) for s in (self.sr, self.sg, self.sb)]


def boxes_of(pixels, K, cells=None):
    """The boxes in index order; ``cells``: the moments when the caller has them already (``pixels`` is then not read)."""
    boxes = [Box(sorted((cells_of(pixels) if cells is None else cells).items()))]
    while len(boxes) < K:
        best = None
        for i, b in enumerate(boxes):
            if max(b.sides()) > 1 and (best is None or b.error() > boxes[best].error()):
                best = i
        if best is None:
            break
        b = boxes[best]
        a, k = b.cut()
        boxes[best] = Box([(c, m) for c, m in b.cells if c[a] <= k])
        boxes.append(Box([(c, m) for c, m in b.cells if c[a] > k]))
    return boxes


def palette(frames, K):
    """frames: uint8 [..., 3], all of it one palette's pixels -> (uint8 [256,3] with zeros from `used` on, used)."""
    px = np.asarray(frames).reshape(-1, 3).tolist()
    boxes = boxes_of(px, K)
    out = np.zeros((256, 3), dtype=np.uint8)
    for i, b in enumerate(boxes):
        out[i] = b.entry()
    return out, len(boxes)


def palette_weighted(frames, weights, K):
    """The palette of a clip in which frames[i] (uint8 [..., 3]) occurs weights[i] times, without building the clip: -> as ``palette``."""
    cells = {}
    for f, m in zip(frames, weights):
        assert int(m) == m and m >= 0
        if m:
            cells_of(np.asarray(f).reshape(-1, 3).tolist(), int(m), cells)
    boxes = boxes_of(None, K, cells)
    out = np.zeros((256, 3), dtype=np.uint8)
    for i, b in enumerate(boxes):
        out[i] = b.entry()
    return out, len(boxes)


def palettes(frames, K, per_frame):
    """frames uint8 [n,h,w,3] -> (uint8 [P,256,3], int32 [P]) as the device call returns them."""
    frames = np.asarray(frames)
    parts = [palette(f, K) for f in frames] if per_frame else [palette(frames, K)]
    return np.stack([p for p, _ in parts]), np.asarray([u for _, u in parts], dtype=np.int32)


def nearest(frames, pal):
    """The index of the nearest entry (sum of squared differences, the lowest index among equals) of every pixel: uint8 [...]."""
    a = np.asarray(frames).astype(np.int64)
    p = np.asarray(pal).astype(np.int64)
    d = ((a[..., None, :] - p) ** 2).sum(axis=-1)
    return d.argmin(axis=-1).astype(np.uint8)


def psnr(a, b):
    mse = float(((np.asarray(a).astype(np.float64) - np.asarray(b).astype(np.float64)) ** 2).mean())
    return float("inf") if mse == 0 else 10 * np.log10(255.0 ** 2 / mse)
