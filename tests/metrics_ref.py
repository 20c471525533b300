"""The image metrics' rules (top of csrc/metrics.hip) in float64 NumPy: what ``runtime.image_metrics`` and ``metrics.ssim`` / ``psnr`` are
held to.  The window is the reference's float32 2-D window g g^T, every product of two float32 weights rounded to float32; everything
behind it - scaled samples, convolutions, the map, the means - is float64.  ``pad`` and ``shift`` exist for the two mutations the host
test uses to show that the bars discriminate."""
import math

import numpy as np

# gaussian(11, 1.5) of utils/loss_utils.py as float32 bits (tests/golden/metrics/cases.npz holds the same eleven)
WINDOW_BITS = (981912246, 1006173953, 1024685452, 1038088319, 1046093343, 1049113264, 1046093343, 1038088319, 1024685452, 1006173953, 981912246)
C1, C2 = 0.01 ** 2, 0.03 ** 2


def window():
    return np.array(WINDOW_BITS, dtype=np.uint32).view(np.float32)


def window_2d():
    g = window()
    return (g[:, None] * g[None, :]).astype(np.float32)          # float32 products, as the reference's mm


def blur(x, pad="zero", shift=0):
    """x float64 [..., h, w] -> its correlation with the 2-D window, padding 5 (zeros, or ``reflect``), the window moved ``shift`` taps."""
    w2 = window_2d().astype(np.float64)
    h, w = x.shape[-2:]
    lead = [(0, 0)] * (x.ndim - 2)
    p = np.pad(x, lead + [(5, 5), (5 + abs(shift), 5 + abs(shift))], mode="constant" if pad == "zero" else "reflect")
    out = np.zeros_like(x)
    for i in range(11):
        for j in range(11):
            out += w2[i, j] * p[..., i:i + h, j + abs(shift) + shift:j + abs(shift) + shift + w]
    return out


def ssim_map(x, y, pad="zero", shift=0):
    """x, y float64 [..., h, w] planes -> the map, float64."""
    mu1, mu2 = blur(x, pad, shift), blur(y, pad, shift)
    s1 = blur(x * x, pad, shift) - mu1 * mu1
    s2 = blur(y * y, pad, shift) - mu2 * mu2
    s12 = blur(x * y, pad, shift) - mu1 * mu2
    return ((2 * mu1 * mu2 + C1) * (2 * s12 + C2)) / ((mu1 * mu1 + mu2 * mu2 + C1) * (s1 + s2 + C2))


def scaled(u8):
    """to_tensor's float32 x / 255, as float64."""
    return (u8.astype(np.float32) / np.float32(255.0)).astype(np.float64)


def psnr_of(mse):
    return math.inf if mse == 0 else 20.0 * math.log10(1.0 / math.sqrt(mse))


def metrics_f32(a, b, pad="zero", shift=0):
    """a, b float32 [n,c,h,w] -> dict of ssim, mse, l1, psnr (float64 [n]) and map (float64 [n,c,h,w])."""
    x, y = a.astype(np.float64), b.astype(np.float64)
    m = ssim_map(x, y, pad, shift)
    d = (a - b).astype(np.float64)          # the float32 difference
    n = a.shape[0]
    mse = np.array([math.fsum((d[i] * d[i]).ravel()) / d[i].size for i in range(n)])
    l1 = np.array([math.fsum(np.abs(d[i]).ravel()) / d[i].size for i in range(n)])
    return {"ssim": np.array([math.fsum(m[i].ravel()) / m[i].size for i in range(n)]), "mse": mse, "l1": l1, "psnr": np.array([psnr_of(v) for v in mse]), "map": m}


def metrics_u8(a, b, pad="zero", shift=0):
    """a, b uint8 [n,h,w,c] -> the same dict, the map [n,h,w,c]; mse and l1 are the exact integer sums over count 255^2 and count 255."""
    x, y = scaled(a).transpose(0, 3, 1, 2), scaled(b).transpose(0, 3, 1, 2)
    m = ssim_map(x, y, pad, shift).transpose(0, 2, 3, 1)
    n, count = a.shape[0], a[0].size
    d = a.astype(np.int64) - b.astype(np.int64)
    mse = np.array([int((d[i] * d[i]).sum()) / (count * 65025) for i in range(n)])
    l1 = np.array([int(np.abs(d[i]).sum()) / (count * 255) for i in range(n)])
    return {"ssim": np.array([math.fsum(m[i].ravel()) / m[i].size for i in range(n)]), "mse": mse, "l1": l1, "psnr": np.array([psnr_of(v) for v in mse]), "map": m}
