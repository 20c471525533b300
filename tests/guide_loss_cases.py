"""The cases both guide-loss test files walk (test_guide_loss_host.py, test_gpu_guide_loss.py): shapes, byte offsets, the dispatch table of
csrc/guide_loss.hip's two launchers, and the seeded guides and renders."""
import functools

import numpy as np

import guide_loss_ref as R

F32, F64 = np.float32, np.float64

# (n, h, w, gh, gw): the smallest shapes at which indexing, clamping or the tile tail can go wrong
SHAPES = [
    (1, 1, 1, 1, 1),
    (1, 1, 1, 2, 2),            # one output mixing four taps
    (2, 3, 5, 3, 5),            # the same size: g is p exactly
    (1, 5, 7, 2, 3),            # upsampling: r clamped at 0 on the low edge, i1 clamped on the high edge
    (1, 4, 8, 9, 17),           # shrinking by more than 2: the taps skip guide pixels (F.interpolate does not antialias)
    (1, 16, 64, 8, 32),         # an exact 2x and whole tiles
    (2, 17, 65, 11, 23),        # one-sample slivers each way, two frames, w % 4 != 0
    (1, 33, 128, 20, 50),       # w % 4 == 0, several tiles
]
WORKLOAD = (1, 800, 800, 512, 512)          # the workload's own ratio, run once (offsets 0)
SAME_SIZE = (2, 3, 5, 3, 5)
GUIDE_OFFSETS = (0, 1, 2, 3)                # the guide's byte address modulo 4
FLOAT_OFFSETS = (0, 4)                      # image, resampled and grad: bytes from a 16-byte boundary
DELTA_MIN = 2.0 ** -10

# One row per branch a launcher of csrc/guide_loss.hip can take: key -> (kernel, predicate).  select() restates the launchers' predicate
# on the facts a caller controls; test_gpu_guide_loss.py asserts at import that its cases take every key.
DISPATCH = {
    "guide_l1/vec": ("guide_l1_tile_kernel<true> + guide_l1_finish_kernel", "w % 4 == 0, image and resampled (if any) 16-byte aligned"),
    "guide_l1/scalar_off": ("guide_l1_tile_kernel<false> + guide_l1_finish_kernel", "w % 4 == 0, image or resampled not 16-byte aligned"),
    "guide_l1/scalar": ("guide_l1_tile_kernel<false> + guide_l1_finish_kernel", "w % 4 != 0"),
    "guide_l1_grad/vec": ("guide_l1_grad_kernel<true>", "w % 4 == 0, image and grad 16-byte aligned"),
    "guide_l1_grad/scalar_off": ("guide_l1_grad_kernel<false>", "w % 4 == 0, image or grad not 16-byte aligned"),
    "guide_l1_grad/scalar": ("guide_l1_grad_kernel<false>", "w % 4 != 0"),
}


def select(call, w, image_off=0, out_off=0):
    """``call``: "guide_l1" (out_off: resampled's, 0 without one) or "guide_l1_grad" (out_off: grad's)."""
    if w % 4 != 0:
        return call + "/scalar"
    return call + ("/scalar_off" if image_off % 16 or out_off % 16 else "/vec")


def cases():
    """(shape, guide offset, float offset) of every case."""
    out = [(s, go, fo) for s in SHAPES for go in GUIDE_OFFSETS for fo in FLOAT_OFFSETS]
    return out + [(WORKLOAD, 0, 0)]


def case_id(case):
    shape, go, fo = case
    return "%dx%dx%d_from_%dx%d" % shape + f"_g{go}_f{fo}"


@functools.lru_cache(maxsize=None)
def guide(shape, seed=0):
    """uint8 [n][gh][gw][3], seeded, 0 and 255 among its bytes."""
    n, _, _, gh, gw = shape
    g = np.random.default_rng([seed, *shape]).integers(0, 256, (n, gh, gw, 3), dtype=np.uint8)
    g.flat[0], g.flat[-1] = 0, 255
    g.setflags(write=False)
    return g


@functools.lru_cache(maxsize=None)
def g_ref(shape, seed=0):
    g = R.resampled(guide(shape, seed), shape[1], shape[2])
    g.setflags(write=False)
    return g


@functools.lru_cache(maxsize=None)
def image_delta(shape, seed=0):
    """g_ref +- delta, 2^-10 <= delta < 2^-2 with a seeded sign: no sample sits near a tie, every sample is compared."""
    n, h, w, _, _ = shape
    rng = np.random.default_rng([seed + 1, *shape])
    delta = (F32(DELTA_MIN) * (F32(1) + F32(255) * rng.random((n, 3, h, w), dtype=F32))).astype(F32)
    sign = np.where(rng.integers(0, 2, (n, 3, h, w)) == 0, F32(-1), F32(1)).astype(F32)
    x = (g_ref(shape, seed) + sign * delta).astype(F32)
    assert np.all(np.abs(x.astype(F64) - g_ref(shape, seed).astype(F64)) >= DELTA_MIN / 2)
    x.setflags(write=False)
    return x


@functools.lru_cache(maxsize=None)
def image_ties(seed=0):
    """The same-size shape with x == g exactly (x = p) on a seeded half of the samples, g +- delta elsewhere -> (image, tie mask)."""
    shape = SAME_SIZE
    n, h, w, _, _ = shape
    p = g_ref(shape, seed)
    tie = np.random.default_rng([seed + 2, *shape]).integers(0, 2, (n, 3, h, w)) == 0
    assert tie.any() and not tie.all()
    x = np.where(tie, p, image_delta(shape, seed)).astype(F32)
    x.setflags(write=False)
    return x, tie
