"""The frames of the PNG tests: the smallest that reach every rule of tests/png_ref.py.  cases() -> [(name, frame uint8 [h, w, c], filter)];
filter None is the adaptive choice.  Host only, deterministic."""
import functools
import os

import numpy as np

import png_ref

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def row_frame(data):
    """Grey frames of one row under filter 0: the filtered stream is a 0 and then exactly ``data``."""
    return np.frombuffer(bytes(data), np.uint8).reshape(1, -1, 1).copy()


def noisy_gradient(h, w, seed=1):
    rng = np.random.default_rng(seed)
    y, x = np.mgrid[0:h, 0:w]
    g = np.stack([x * 255 // w, y * 255 // h, (x + y) * 255 // (w + h)], 2) + rng.integers(-6, 7, (h, w, 3))
    return np.clip(g, 0, 255).astype(np.uint8)


def masked_view(h, w, seed=2):
    """An object on black, as a masked 3DGS view is."""
    y, x = np.mgrid[0:h, 0:w]
    inside = ((y - h / 2) ** 2 + (x - w / 2) ** 2) < (min(h, w) / 3) ** 2
    return noisy_gradient(h, w, seed) * inside[:, :, None].astype(np.uint8)


def stylised_sample():
    """The stylised 256 x 256 frame of the golden case 'f' (the decoder's output, quantised as save_image does), continued by its mirror
    image to 256 x 456."""
    with np.load(os.path.join(GOLDEN, "case_f.npz")) as z:
        out = z["out"]
    img = np.clip(out[0].transpose(1, 2, 0) * 255 + 0.5, 0, 255).astype(np.uint8)
    return np.ascontiguousarray(np.concatenate([img, img[:, ::-1]], axis=1)[:, :456])


def five_filters():
    """A frame in which every filter wins some row: strips of different structure, the first seed that shows all five."""
    for seed in range(200):
        rng = np.random.default_rng(seed)
        h, w = 16, 24
        y, x = np.mgrid[0:h, 0:w]
        f = (3 * x + 5 * y)[:, :, None] + rng.integers(-2, 3, (h, w, 3))
        f[0:2] = rng.integers(-1, 2, (2, w, 3))                     # near zero: None
        f[2:4] = (7 * x[2:4])[:, :, None] + rng.integers(0, 2, (2, 1, 3))          # a ramp along the row: Sub
        f[4:6] = f[3:4] + rng.integers(-1, 2, (2, w, 3))               # the row above again: Up
        f[6:10] = 10 + rng.integers(0, 17, (4, w, 3))          # flat and noisy: Average halves the noise of its two neighbours
        f[10:] = np.where((x[10:] > 11)[:, :, None], 200, 20) + (x[10:] * y[10:] // 3)[:, :, None]     # an edge: Paeth
        frame = (f & 255).astype(np.uint8)
        if set(png_ref.filter_rows(frame)[1].tolist()) == {0, 1, 2, 3, 4}:
            return frame
    raise AssertionError("no seed shows all five filters")


def noise_bytes(rng, count):
    """Bytes 1..255 in which no byte equals the one 1, 2, 3, 4 or 6 before it: no accidental match, no zero."""
    out = []
    while len(out) < count:
        v = int(rng.integers(1, 256))
        if all(len(out) < d or out[-d] != v for d in (1, 2, 3, 4, 6)):
            out.append(v)
    return out


def zero_runs(runs, seed=3):
    rng = np.random.default_rng(seed)
    data = []
    for r in runs:
        data += noise_bytes(rng, 5) + [0] * r
    return row_frame(data + noise_bytes(rng, 5))


def fibonacci(symbols, seed=4):
    """Symbol i appears fib(i + 2) times - with the row's filter byte and the end-of-block symbol as the two 1s in front, a histogram
    whose Huffman tree is a chain - drawn in random order, except that a byte which would
    be the fourth in a row to repeat the one 1, 2, 3, 4 or 6 before it is drawn again: no match takes literals out of the histogram."""
    fib = [1, 1]
    while len(fib) < symbols + 2:
        fib.append(fib[-1] + fib[-2])
    left = np.array(fib[2:])
    rng = np.random.default_rng(seed)
    data, run = [], {d: 0 for d in (1, 2, 3, 4, 6)}
    while left.sum():
        for _ in range(64):
            v = 3 * (1 + int(rng.choice(symbols, p=left / left.sum())))
            if all(run[d] < 3 or len(data) < d or data[-d] != v for d in run):
                break
        else:
            break                                      # only the commonest symbols are left: the tail is dropped
        left[v // 3 - 1] -= 1
        for d in run:
            run[d] = run[d] + 1 if len(data) >= d and data[-d] == v else 0
        data.append(v)
    return row_frame(data)


@functools.lru_cache(maxsize=None)
def cases():
    rng = np.random.default_rng(0)
    u8 = lambda *shape: rng.integers(0, 256, shape, dtype=np.uint8)
    out = []
    for c in (1, 3):                                               # degenerate shapes
        out += [(f"1x1x{c}", u8(1, 1, c), None), (f"1x7x{c}", u8(1, 7, c), None), (f"7x1x{c}", u8(7, 1, c), None)]
    out.append(("five_filters", five_filters(), None))
    tie = np.full((4, 9, 3), 7, np.uint8)
    tie[0] = 0                                                     # a zero row: all five cost 0; constant rows: Up and Paeth tie at 0
    out.append(("cost_ties", tie, None))
    out.append(("paeth_ties", rng.integers(0, 4, (9, 11, 3), dtype=np.uint8), 4))
    out.append(("paeth_ties_grey", rng.integers(0, 4, (9, 11, 1), dtype=np.uint8), 4))
    smooth = noisy_gradient(16, 20, 5)
    out += [(f"forced_{k}", smooth, k) for k in range(5)]
    out.append(("grey_adaptive", noisy_gradient(20, 33, 6)[:, :, :1].copy(), None))
    # block edges, by filter 0 on one grey row: the stream is 1 + w bytes
    low = lambda count: rng.integers(0, 4, count, dtype=np.uint8).tolist()
    for w in (32766, 32767, 32768):                                # one byte less than a block, exactly one, one more (a last block of one byte)
        data = low(w)
        data[32600:] = [0] * (w - 32600)                           # a zero run up to the stream's end: cut at the block's end
        out.append((f"stream_{w + 1}", row_frame(data), 0))
    rows = np.tile(u8(1, 16383, 1), (3, 1, 1))                      # stride 16384: the third row is a block whose sources lie in the one before
    out.append(("source_in_previous_block", rows, 0))
    out.append(("zero_runs", zero_runs([257, 258, 259, 600]), 0))
    ends = sorted({png_ref.LEN_BASE[k] + e for k in range(1, 29) for e in (0, (1 << png_ref.LEN_EXTRA[k]) - 1)} | {258})
    out.append(("length_symbols", zero_runs([v + 1 for v in ends if v >= png_ref.MIN_MATCH], 7), 0))
    base = u8(1, 1024 + 4, 1)[0, :, 0]
    out.append(("row_distances_1024", np.stack([base[2:1026], base[3:1027], base[3:1027], base[2:1026]])[:, :, None].copy(), 0))
    wide = u8(1, 32769, 1)[0, :, 0]
    out.append(("row_distance_32768", np.stack([wide[:32768], wide[1:]])[:, :, None].copy(), 0))
    out.append(("fibonacci_15", fibonacci(19), 0))
    out.append(("no_match_dynamic", row_frame(noise_bytes(np.random.default_rng(8), 3000)), 0))
    out.append(("no_match_100", rng.integers(0, 100, (40, 40, 1), dtype=np.uint8), 0))
    tie = [70, 105, 105, 105, 10, 100, 40, 65, 105, 0, 110, 40, 80, 50, 45, 60, 10, 35, 40, 50, 100, 50, 10, 110, 110, 15, 60, 60, 95, 30, 45, 40, 45, 15, 70, 90, 75, 20,
           85, 5, 85, 110, 45, 25, 85, 70, 50, 75, 70, 70, 40, 20, 90, 60, 45, 85, 20, 40, 60, 60, 45, 85, 25, 90]
    out.append(("dynamic_fixed_tie", row_frame(tie), 0))               # found by search: both forms of the block have the same bits; fixed is written
    out.append(("one_literal", np.zeros((1, 3, 1), np.uint8), 0))
    out.append(("zeros_64x100", np.zeros((64, 100, 3), np.uint8), None))
    out.append(("noise_64x96", u8(64, 96, 3), None))
    out.append(("gradient_128x228", noisy_gradient(128, 228), None))
    out.append(("masked_300x300", masked_view(300, 300), None))
    out.append(("stylised_256x456", stylised_sample(), None))
    return out


REALISTIC = ("stylised_256x456", "gradient_128x228", "masked_300x300")          # the frames of the size bar
