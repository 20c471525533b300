"""``coral(style, content)`` (reference Style_3DGS/AdaIN/function.py:26-67) restated in float64 numpy, stage by stage as
csrc/coral.hip computes it: moments -> symmetric eigen-decomposition -> one affine map per pair -> pixels.

An image is either uint8 HWC [h,w,3] or float32 CHW [3,h,w].  A uint8 image enters the moments as the exact integer sums of its byte
values (x = v / 255) and the pixel stage as ``float32(v) / float32(255)``, ToTensor's value; a float image enters both as it is.
With mu / sigma the channel means and UNBIASED deviations, C = norm norm^T + I = (N - 1) R + I (R: the correlation matrix, so every
eigenvalue of C is >= 1), sqrt(C) = V diag(sqrt(lambda)) V^T - what the reference's U diag(sqrt(D)) V^T of torch.linalg.svd is for a
symmetric positive definite matrix - and

    A = diag(sigma_content) . sqrt(C_content) . inverse(sqrt(C_style)) . diag(1 / sigma_style),   b = mu_content - A mu_style.

A side of fewer than two pixels or with a channel of zero variance (the reference divides by zero) gives the status bit(s) of
include/adain_hip.h, A = I, b = 0 and the style's own pixels."""
import numpy as np

# Relative L2 bound of anything held to the reference's float32 ``coral`` (the fixture case_d, the package's host ``coral``): 4 x the worst
# error this float64 restatement measured against them (1.47e-7; tests/test_coral_ref_host.py lists the measurements).
REFERENCE_FP32_BOUND = 4 * 1.47e-7

STYLE_FLAT, CONTENT_FLAT, STYLE_SINGLE, CONTENT_SINGLE = 1, 2, 4, 8      # ADAIN_CORAL_*
_PAIRS = [(0, 0), (0, 1), (0, 2), (1, 1), (1, 2), (2, 2)]


def planes(img):
    """[3, hw] of an image: integer (uint8 HWC, as int64 byte values) or float64 (float32 CHW)."""
    img = np.asarray(img)
    if img.dtype == np.uint8:
        assert img.ndim == 3 and img.shape[2] == 3
        return img.reshape(-1, 3).T.astype(np.int64)
    assert img.dtype == np.float32 and img.ndim == 3 and img.shape[0] == 3
    return img.reshape(3, -1).astype(np.float64)


def pixels(img):
    """[3, hw] float64 of the values the pixel stage reads: ToTensor's float32(v) / float32(255) for uint8."""
    img = np.asarray(img)
    if img.dtype == np.uint8:
        return (img.reshape(-1, 3).T.astype(np.float32) / np.float32(255)).astype(np.float64)
    return img.reshape(3, -1).astype(np.float64)


def moments(img):
    """dict(n, sum [3], sum2 [6] (00, 01, 02, 11, 12, 22) - exact Python ints for uint8, None for float -, mean [3], std [3] (unbiased; 0
    where there is none), D [3,3] = N sum x x^T - (sum x)(sum x)^T in the image's own units as float64, flat, single)."""
    p = planes(img)
    n = p.shape[1]
    if p.dtype == np.int64:
        s1 = [int(p[c].sum()) for c in range(3)]
        s2 = [int((p[i] * p[j]).sum()) for i, j in _PAIRS]
        D = np.zeros((3, 3))
        for q, (i, j) in enumerate(_PAIRS):
            D[i, j] = D[j, i] = float(n * s2[q] - s1[i] * s1[j])      # exact integer, rounded once
        mean, scale = np.array(s1, dtype=np.float64) / (255.0 * n), 1.0 / 255.0
    else:
        s1 = s2 = None
        d = p - p[:, :1]                                              # about the first pixel: a constant channel is exactly flat
        t1, t2 = d.sum(axis=1), d @ d.T
        D = n * t2 - np.outer(t1, t1)
        mean, scale = p[:, 0] + t1 / n, 1.0
    var = np.diag(D).copy()
    ok = n > 1 and bool(np.all(var > 0))
    std = scale * np.sqrt(np.where(var > 0, var, 0.0) / (n * (n - 1.0))) if n > 1 else np.zeros(3)
    return dict(n=n, sum=s1, sum2=s2, mean=mean, std=std, D=D, flat=n > 1 and not ok, single=n < 2)


def _sqrt_factors(m):
    """(sqrt(C), inverse(sqrt(C))) of C = (N - 1) R + I from one side's moments."""
    n1 = m["n"] - 1.0
    s = np.sqrt(np.diag(m["D"]))
    C = n1 * (m["D"] / np.outer(s, s))
    C[np.diag_indices(3)] = n1 + 1.0
    lam, V = np.linalg.eigh(C)
    lam = np.maximum(lam, 1.0)
    return (V * np.sqrt(lam)) @ V.T, (V / np.sqrt(lam)) @ V.T


def coral(style, content):
    """(out float64 [3,hs,ws] before the final rounding to float32, A [3,3], b [3], status, style moments, content moments)."""
    style, content = np.asarray(style), np.asarray(content)
    ms, mt = moments(style), moments(content)
    status = (STYLE_SINGLE if ms["single"] else 0) | (STYLE_FLAT if ms["flat"] else 0) | (CONTENT_SINGLE if mt["single"] else 0) | \
             (CONTENT_FLAT if mt["flat"] else 0)
    x = pixels(style)
    hs, ws = style.shape[:2] if style.dtype == np.uint8 else style.shape[1:]
    if status:
        return x.reshape(3, hs, ws), np.eye(3), np.zeros(3), status, ms, mt
    root_t, _ = _sqrt_factors(mt)
    _, inv_s = _sqrt_factors(ms)
    A = (mt["std"][:, None] * (root_t @ inv_s)) / ms["std"][None, :]
    b = mt["mean"] - A @ ms["mean"]
    out = (A[:, 0:1] * x[0] + A[:, 1:2] * x[1]) + A[:, 2:3] * x[2] + b[:, None]
    return out.reshape(3, hs, ws), A, b, status, ms, mt


def rel_l2(got, want):
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    return float(np.linalg.norm(got - want) / np.linalg.norm(want))


def u8_image(seed, h, w):
    """A seeded uint8 HWC image whose channels are correlated and differently spread, like a photograph's."""
    g = np.random.default_rng(seed)
    base = g.random((h, w, 1))
    img = 0.55 * base + 0.45 * g.random((h, w, 3)) * np.array([1.0, 0.7, 0.5]) + np.array([0.0, 0.1, 0.2])
    return np.clip(img * 255.0, 0, 255).astype(np.uint8)


def chw(u8):
    """ToTensor of a uint8 HWC image: float32 CHW."""
    return np.ascontiguousarray(u8.transpose(2, 0, 1).astype(np.float32) / np.float32(255))
