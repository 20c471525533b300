"""``PIL.Image.Image.resize(size, resample)`` for uint8 ``L`` and ``RGB`` images restated in plain Python (Pillow 4.x .. 12.x:
libImaging/Resample.c, Geometry.c's ImagingScaleAffine for NEAREST, _imaging.c:_resize), no ``box=`` and no ``reducing_gap``.

The taps are computed with ``math.sin`` / ``math.cos`` - the C library's functions, which are the ones Pillow calls - in the order of
Resample.c's ``precompute_coeffs`` and ``normalize_coeffs_8bpc``; a Python float is a C double and ``+ - * /`` round the same way.
The two passes are integer arithmetic in NumPy.  tests/test_pil_resize_host.py holds this file to Pillow and the library's
``adain_pil_resize_taps`` to this file."""
import math

import numpy as np

NEAREST, LANCZOS, BILINEAR, BICUBIC, BOX, HAMMING = 0, 1, 2, 3, 4, 5          # PIL.Image.Resampling
FILTERS = {"NEAREST": NEAREST, "BOX": BOX, "BILINEAR": BILINEAR, "HAMMING": HAMMING, "BICUBIC": BICUBIC, "LANCZOS": LANCZOS}
SUPPORT = {BOX: 0.5, BILINEAR: 1.0, HAMMING: 1.0, BICUBIC: 2.0, LANCZOS: 3.0}
PRECISION_BITS = 32 - 8 - 2
MAX_SHRINK = 256          # the device call's limit on in / out per axis
_F32_054 = float(np.float32(0.54))          # Resample.c writes the window's constants as 0.54f and 0.46f: floats, widened to double
_F32_046 = float(np.float32(0.46))


def _sinc(x):
    if x == 0.0:
        return 1.0
    x = x * math.pi
    return math.sin(x) / x


def filter_value(f, x):
    if f == BOX:
        return 1.0 if -0.5 < x <= 0.5 else 0.0
    if f == BILINEAR:
        x = abs(x)
        return 1.0 - x if x < 1.0 else 0.0
    if f == HAMMING:
        x = abs(x)
        if x == 0.0:
            return 1.0
        if x >= 1.0:
            return 0.0
        x = x * math.pi
        return math.sin(x) / x * (_F32_054 + _F32_046 * math.cos(x))
    if f == BICUBIC:
        a = -0.5
        x = abs(x)
        if x < 1.0:
            return ((a + 2.0) * x - (a + 3.0)) * x * x + 1
        if x < 2.0:
            return (((x - 5) * x + 8) * x - 4) * a
        return 0.0
    if f == LANCZOS:
        return _sinc(x) * _sinc(x / 3) if -3.0 <= x < 3.0 else 0.0
    raise ValueError(f"no convolution filter {f}")


def ksize_of(f, in_size, out_size):
    if f == NEAREST:
        return 0
    filterscale = max(in_size / out_size, 1.0)
    return int(math.ceil(SUPPORT[f] * filterscale)) * 2 + 1


def taps(f, in_size, out_size):
    """-> (ksize, bounds int32 [out,2], taps int32 [out,ksize]).  A convolution filter: first source index and tap count, fixed-point
    taps (zero behind the count).  NEAREST: ksize 0, the source index and 1 (0 when the index is outside [0, in))."""
    bounds = np.zeros((out_size, 2), np.int32)
    if f == NEAREST:
        s = in_size / out_size
        o = s * 0.5
        for i in range(out_size):
            src = -1 if o < 0 else int(o)
            bounds[i] = (src, 1 if 0 <= src < in_size else 0)
            o += s
        return 0, bounds, np.zeros((out_size, 0), np.int32)
    scale = in_size / out_size
    filterscale = max(scale, 1.0)
    support = SUPPORT[f] * filterscale
    ksize = int(math.ceil(support)) * 2 + 1
    kk = np.zeros((out_size, ksize), np.int32)
    ss = 1.0 / filterscale
    for xx in range(out_size):
        center = (xx + 0.5) * scale
        xmin = max(int(center - support + 0.5), 0)
        xmax = min(int(center + support + 0.5), in_size) - xmin
        w = [filter_value(f, (x + xmin - center + 0.5) * ss) for x in range(xmax)]
        ww = 0.0
        for v in w:
            ww += v
        if ww != 0.0:
            w = [v / ww for v in w]
        for x, v in enumerate(w):
            kk[xx, x] = int(-0.5 + v * (1 << PRECISION_BITS)) if v < 0 else int(0.5 + v * (1 << PRECISION_BITS))
        bounds[xx] = (xmin, xmax)
    return ksize, bounds, kk


def _pass(a, bounds, kk, axis):
    """One pass of the 8-bit resample along ``axis`` of int64 [h,w,c]: clip8((2^21 + sum in * k) >> 22)."""
    a = np.moveaxis(a, axis, 0)
    out = np.empty((len(bounds),) + a.shape[1:], np.int64)
    for i, (lo, n) in enumerate(bounds):
        acc = np.tensordot(kk[i, :n].astype(np.int64), a[lo:lo + n], axes=(0, 0)) + (1 << (PRECISION_BITS - 1))
        out[i] = np.clip(acc >> PRECISION_BITS, 0, 255)
    return np.moveaxis(out, 0, axis)


def resize(a, size, f):
    """``a``: uint8 [h,w] (L) or [h,w,3] (RGB); ``size`` = (width, height) as PIL takes it -> uint8 of the same rank."""
    grey = a.ndim == 2
    x = a[..., None] if grey else a
    hi, wi = x.shape[:2]
    wo, ho = int(size[0]), int(size[1])
    if (wo, ho) == (wi, hi):
        return a.copy()
    if f == NEAREST:
        _, by, _ = taps(f, hi, ho)
        _, bx, _ = taps(f, wi, wo)
        out = x[np.clip(by[:, 0], 0, hi - 1)][:, np.clip(bx[:, 0], 0, wi - 1)] * (by[:, 1, None, None] & bx[None, :, 1, None]).astype(np.uint8)
    else:
        v = x.astype(np.int64)
        if wo != wi:          # Pillow skips a pass whose axis keeps its size
            _, b, k = taps(f, wi, wo)
            v = _pass(v, b, k, 1)
        if ho != hi:
            _, b, k = taps(f, hi, ho)
            v = _pass(v, b, k, 0)
        out = v.astype(np.uint8)
    return out[..., 0] if grey else out


def picture(seed, h, w):
    """uint8 RGB [h,w,3]: noise over a smooth ramp with saturated patches (tests/test_gpu_resize_pil.py's picture, restated), the right
    third a black / white checker of 1, 2 or 3 pixel cells: the negative lobes of BICUBIC and LANCZOS then reach clip8 at both ends."""
    g = np.random.default_rng(seed)
    a = g.random((h, w, 3), dtype=np.float32)
    yy, xx = np.mgrid[:h, :w].astype(np.float32)
    ramp = ((yy / max(h - 1, 1) + xx / max(w - 1, 1)) * 0.5)[..., None]
    v = np.where(a > 0.9, 1.0, np.where(a < 0.1, 0.0, 0.6 * a + 0.4 * ramp))
    out = (v * 255).astype(np.uint8)
    cell = 1 + seed % 3
    checker = ((((np.mgrid[:h, :w][0] // cell) + (np.mgrid[:h, :w][1] // cell)) & 1) * 255).astype(np.uint8)
    x0 = w - w // 3
    out[:, x0:] = checker[:, x0:, None]
    return out
