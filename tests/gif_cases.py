"""The frames the GIF writer is held to (tests/test_gif_host.py on the restatement, tests/test_gpu_gif.py on the device).

Every palette size at which the code size or the colour table changes or just has (K), every pixel count around the segment's 2048
(SHAPES), and three kinds of indices: flat (one long run: the longest strings), run (i // 7 % K) and uniform noise, which at K = 256
drives a segment through the 9- to 12-bit widths.  EDGES: frames whose data lengths are 255 j - 1, 255 j and 255 j + 1 bytes, the
sub-block edges, found with the restatement (``python tests/gif_cases.py`` searches them again)."""
import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
KS = (1, 2, 3, 4, 5, 16, 17, 128, 129, 256)
SHAPES = ((1, 1), (23, 89), (32, 64), (3, 683), (17, 241))          # 1, 2047, 2048, 2049 and 4097 pixels
KINDS = ("flat", "run", "noise")
# (K, h, w, seed, data bytes): noise frames of one row
EDGES = ((256, 1, 225, 1, 254), (256, 1, 224, 0, 255), (256, 1, 225, 0, 256), (256, 1, 3343, 0, 4334), (256, 1, 3348, 2, 4335), (256, 1, 3349, 0, 4336),
         (17, 1, 1551, 0, 1019), (17, 1, 1559, 0, 1020), (17, 1, 1550, 0, 1021))


def indices(kind, K, h, w, seed=0):
    """uint8 [h,w] below K."""
    n = h * w
    if kind == "flat":
        a = np.full(n, K - 1)
    elif kind == "run":
        a = np.arange(n) // 7 % K
    else:
        a = np.random.default_rng([K, h, w, seed]).integers(0, K, n)
    return a.astype(np.uint8).reshape(h, w)


def palette(K):
    """K distinct colours, none of them grey (a decoder that fell back to an index would show)."""
    k = np.arange(K)
    return np.stack([(k * 37 + 11) % 256, (k * 101 + 3) % 256, 255 - k], axis=1).astype(np.uint8)


def cases():
    """[(name, K, index uint8 [h,w])]"""
    out = [(f"{kind}_K{K}_{h}x{w}", K, indices(kind, K, h, w)) for K in KS for h, w in SHAPES for kind in KINDS]
    out += [(f"edge_{D}_K{K}_{h}x{w}", K, indices("noise", K, h, w, seed)) for K, h, w, seed, D in EDGES]
    return out


def clip(n, K, h, w, kind="noise"):
    """uint8 [n,h,w]: frame i is the kind's frame of seed i (flat and run frames are shifted by i instead)."""
    if kind == "noise":
        return np.stack([indices(kind, K, h, w, i) for i in range(n)])
    return np.stack([(indices(kind, K, h, w).astype(np.int64) + i) % K for i in range(n)]).astype(np.uint8)


if __name__ == "__main__":
    import gif_ref as G

    found = {}
    for K, w0, j in ((256, 150, 1), (256, 3300, 17), (17, 1500, 4)):          # one sub-block, two segments, another code size
        for seed in range(6):
            for w in range(w0, w0 + 100):
                D = len(G.frame_data(indices("noise", K, 1, w, seed), K))
                if abs(D - 255 * j) <= 1 and (K, j, D) not in found:
                    found[(K, j, D)] = (K, 1, w, seed, D)
    print(tuple(found[k] for k in sorted(found)))
