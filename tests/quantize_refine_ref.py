"""The palette refinement's rules (top of csrc/quantize_refine.hip) in plain Python ints and loops: what ``runtime.quantize_palette_u8(...,
refine=T)`` and ``pixelize``'s host form are compared with for equality.  Written apart from the package's NumPy form: the pixels live in a
dict of colour -> count (the rules see their multiset only), every distance is taken in a loop, nothing is an array operation.  Rules 1-6
are tests/quantize_ref.py's, by import: they give the start, a palette P[0..255] and used = u.  Then, for each of the T rounds:

7.  Assign.  Every pixel x goes to the entry j = argmin over i < u of |x - P_i|^2, the squared Euclidean distance in ints; the lowest i wins
    a tie.
8.  Moments.  Per entry i, over its pixels: the count n_i, the sums S_i[c], and the far key F_i = max((d << 24) | (0xFFFFFF - (r << 16 |
    g << 8 | b))) with d the pixel's distance to P_i: the farthest colour, among equally far colours the smallest r, g, b value.
9.  Centres.  n_i > 0: P'_i[c] = (2 S_i[c] + n_i) // (2 n_i).  n_i == 0: P'_i = P_i.
10. Fill.  The free slots are the i < K with n_i == 0, ascending: every i >= u and any live entry that got no pixel.  The donors are the
    entries with n_i > 0 and F_i >> 24 > 0, by that distance descending, then by index ascending.  The m-th free slot takes the m-th
    donor's far colour as long as both lists last; u' = max(u, 1 + the highest slot filled).  A free slot without a donor keeps what it held.
11. P, u <- P', u'.  After the last round entries u..255 are zero.
"""
import numpy as np

import quantize_ref as Q


def colours_of(pixels, weight=1, colours=None):
    """pixels: an iterable of (r, g, b), each counted ``weight`` times -> {(r, g, b): count}, added into ``colours`` when given."""
    colours = {} if colours is None else colours
    for r, g, b in pixels:
        colours[(r, g, b)] = colours.get((r, g, b), 0) + weight
    return colours


def one_round(colours, P, u, K):
    """Rules 7-10 once.  colours: {(r, g, b): count}; P: 256 [r, g, b] lists; -> (P', u')."""
    n = [0] * 256
    S = [[0, 0, 0] for _ in range(256)]
    F = [0] * 256
    live = P[:u]
    for (r, g, b), count in colours.items():
        ds = [(r - p[0]) * (r - p[0]) + (g - p[1]) * (g - p[1]) + (b - p[2]) * (b - p[2]) for p in live]
        d = min(ds)
        j = ds.index(d)          # the first: the lowest index among equals
        n[j] += count
        S[j][0] += count * r
        S[j][1] += count * g
        S[j][2] += count * b
        key = (d << 24) | (0xFFFFFF - (r << 16 | g << 8 | b))
        if key > F[j]:
            F[j] = key
    new = []
    for i in range(256):
        new.append([(2 * S[i][c] + n[i]) // (2 * n[i]) for c in range(3)] if n[i] > 0 else list(P[i]))
    free = [i for i in range(K) if n[i] == 0]
    donors = sorted((i for i in range(256) if n[i] > 0 and F[i] >> 24 > 0), key=lambda i: (-(F[i] >> 24), i))
    for slot, donor in zip(free, donors):
        rgb = 0xFFFFFF - (F[donor] & 0xFFFFFF)
        new[slot] = [rgb >> 16, (rgb >> 8) & 255, rgb & 255]
        u = max(u, slot + 1)
    return new, u


def steps(colours, start, K, T):
    """start: (uint8 [256,3], used) of rules 1-6 -> [(uint8 [256,3], used)] after 0, 1, ..., T rounds."""
    P, u = [[int(v) for v in row] for row in start[0]], int(start[1])
    out = [(np.asarray(P, dtype=np.uint8), u)]
    for _ in range(T):
        P, u = one_round(colours, P, u, K)
        assert all(row == [0, 0, 0] for row in P[u:])          # rule 11: nothing lies behind `used`
        out.append((np.asarray(P, dtype=np.uint8), u))
    return out


def trace(frames, K, T):
    """frames: uint8 [..., 3], all of it one palette's pixels -> [(palette, used)] after 0..T rounds."""
    px = np.asarray(frames).reshape(-1, 3).tolist()
    return steps(colours_of(px), Q.palette(frames, K), K, T)


def palette(frames, K, T):
    """-> (uint8 [256,3] with zeros from `used` on, used) after T rounds."""
    return trace(frames, K, T)[T]


def palette_weighted(frames, weights, K, T):
    """The palette of a clip in which frames[i] (uint8 [..., 3]) occurs weights[i] times, without building the clip: -> as ``palette``."""
    colours = {}
    for f, m in zip(frames, weights):
        assert int(m) == m and m >= 0
        if m:
            colours_of(np.asarray(f).reshape(-1, 3).tolist(), int(m), colours)
    return steps(colours, Q.palette_weighted(frames, weights, K), K, T)[T]


def palettes(frames, K, per_frame, T):
    """frames uint8 [n,h,w,3] -> (uint8 [P,256,3], int32 [P]) as the device call returns them."""
    frames = np.asarray(frames)
    parts = [palette(f, K, T) for f in frames] if per_frame else [palette(frames, K, T)]
    return np.stack([p for p, _ in parts]), np.asarray([u for _, u in parts], dtype=np.int32)
