"""NumPy restatement of csrc/guide_loss.hip, one rounding at a time: train.py's l1_loss of a render against its uint8 guide view, resized
to the render by ATen's bilinear rule, and its gradient by the render.  Imported by tests only (test_guide_loss_host.py pins it to torch's
own four lines, test_gpu_guide_loss.py holds the kernels to it).

Built on pixel_ref.u8_to_f32 (ToTensor: f32(v) / f32(255)) and pixel_ref.resize_bilinear (bilinear_axis per axis, top / bot / out with a
tap of weight 0 still in the sum): every operand stays an np.float32 array, so each operation rounds once and nothing is fused.  The
float64 forms are the same index rules and expressions on the same float32 samples."""
import math

import numpy as np

import pixel_ref as P

F32, F64 = np.float32, np.float64


def _frames(image, guide):
    image, guide = P._np(image), P._np(guide)
    assert image.dtype == F32 and image.ndim == 4 and image.shape[1] == 3, image.shape
    assert guide.dtype == np.uint8 and guide.ndim == 4 and guide.shape[3] == 3 and guide.shape[0] == image.shape[0], guide.shape
    return image, guide


def resampled(guide, h, w, dtype=F32):
    """guide uint8 [n][gh][gw][3] -> g [n][3][h][w] in ``dtype``: p = f32(u8) / f32(255), then the bilinear resize of every plane."""
    guide = P._np(guide)
    assert guide.dtype == np.uint8 and guide.ndim == 4 and guide.shape[3] == 3
    return P.resize_bilinear(P.u8_to_f32(guide), h, w, dtype)


def terms(image, guide):
    """|x - g| per sample, float32 [n][3][h][w] (a NaN sample gives a NaN term)."""
    image, guide = _frames(image, guide)
    with np.errstate(invalid="ignore"):
        t = np.abs(image - resampled(guide, *image.shape[2:]))
    assert t.dtype == F32
    return t


def loss(image, guide):
    """Per frame: the exact sum (math.fsum) of the frame's float32 terms / count, count = 3 h w -> float64 [n]."""
    t = terms(image, guide)
    count = float(t[0].size)
    return np.array([math.fsum(frame.ravel().astype(F64).tolist()) / count if not np.isnan(frame).any() else np.nan for frame in t], dtype=F64)


def loss64(image, guide):
    """The float64 form: the mean of |x - g64| per frame, g64 by the same index rules in float64."""
    image, guide = _frames(image, guide)
    g = resampled(guide, *image.shape[2:], dtype=F64)
    return np.abs(image.astype(F64) - g).reshape(image.shape[0], -1).mean(axis=1)


def grad(image, guide, weights):
    """float32 [n][3][h][w]: (float)(weights[i] / count) * sign, sign = 1 where x > g, -1 where x < g, else d = x - g (zero, or the NaN of
    an input).  A frame whose weight is zero gets +0 everywhere, whatever its samples."""
    image, guide = _frames(image, guide)
    weights = np.asarray(weights, dtype=F64).reshape(-1)
    assert weights.shape[0] == image.shape[0]
    g = resampled(guide, *image.shape[2:])
    count = F64(image[0].size)
    out = np.zeros(image.shape, dtype=F32)
    for i, wt in enumerate(weights):
        if wt == 0.0:
            continue
        k = F32(wt / count)
        with np.errstate(invalid="ignore"):
            d = image[i] - g[i]
            sign = np.where(image[i] > g[i], F32(1), np.where(image[i] < g[i], F32(-1), d)).astype(F32)
            out[i] = k * sign
    assert out.dtype == F32
    return out


def loss_bound(image, ref_loss):
    """N 2^-52 ref.loss, N = 3 h w: a float64 sum of N non-negative terms in any order, and one division, cannot be further from the
    exact sum's quotient (each of the at most N - 1 additions and the division errs by at most 2^-53 of a value that is at most the
    sum)."""
    return float(np.prod(np.shape(image)[1:])) * 2.0 ** -52 * np.asarray(ref_loss)
