"""The gradient of the image metrics (top of csrc/metrics.hip, "The gradient") in float64 NumPy: what ``runtime.image_metrics_grad`` and
the device route of ``metrics.ssim`` / ``l1_loss`` / ``l2_loss`` under autograd are held to.  The window is the reference's float32 2-D
window g g^T (every product of two float32 weights rounded to float32) from ``metrics_ref.window()``; everything behind it is float64.

    A = 2 mu1 mu2 + C1,  B = 2 (e12 - mu1 mu2) + C2,  D = mu1^2 + mu2^2 + C1,  E = (e11 - mu1^2) + (e22 - mu2^2) + C2,  map = A B / (D E)
    d_mu1 = 2 mu2 (B - A) / (D E) - map (2 mu1 / D - 2 mu1 / E),   d_e11 = -map / E,   d_e12 = 2 A / (D E)
    d ssim_i / d x = (conv(d_mu1) + 2 x conv(d_e11) + y conv(d_e12)) / count,   count = c h w

``pad``, ``shift`` and ``drop_e11`` exist for the three wrong forms the host test uses to show that the bar discriminates."""
import numpy as np

import metrics_ref as R

C1, C2 = 0.01 ** 2, 0.03 ** 2


def conv(x, pad="zero", shift=0):
    """x float64 [..., h, w] -> its correlation with the 11 x 11 window, padding 5 (zeros, or ``reflect``), the window moved ``shift``
    taps along the row.  The window is symmetric, so with zeros and no shift this is its own adjoint."""
    g = R.window()
    w2 = (g[:, None] * g[None, :]).astype(np.float32).astype(np.float64)
    h, w = x.shape[-2:]
    s = abs(shift)
    p = np.pad(x, [(0, 0)] * (x.ndim - 2) + [(5, 5), (5 + s, 5 + s)], mode="constant" if pad == "zero" else "reflect")
    out = np.zeros(x.shape, dtype=np.float64)
    for i in range(11):
        for j in range(11):
            out += w2[i, j] * p[..., i:i + h, j + s + shift:j + s + shift + w]
    return out


def planes(x, y, pad="zero"):
    """x, y float64 [n,c,h,w] -> (d_mu1, d_e11, d_e12, d_mu2, d_e22), the map's derivatives by the window statistics."""
    mu1, mu2, e11, e22, e12 = conv(x, pad), conv(y, pad), conv(x * x, pad), conv(y * y, pad), conv(x * y, pad)
    A, B = 2 * mu1 * mu2 + C1, 2 * (e12 - mu1 * mu2) + C2
    D, E = mu1 * mu1 + mu2 * mu2 + C1, (e11 - mu1 * mu1) + (e22 - mu2 * mu2) + C2
    m = A * B / (D * E)
    d_mu = lambda mine, other: 2 * other * (B - A) / (D * E) - m * (2 * mine / D - 2 * mine / E)
    return d_mu(mu1, mu2), -m / E, 2 * A / (D * E), d_mu(mu2, mu1), -m / E


def grad(a, b, weights, pad="zero", shift=0, drop_e11=False):
    """a, b float32 [n,c,h,w], weights [n,3] = upstream d/d{ssim, mse, l1} per frame -> (grad_a, grad_b) float64 [n,c,h,w]."""
    x, y = a.astype(np.float64), b.astype(np.float64)
    wt = np.asarray(weights, dtype=np.float64).reshape(a.shape[0], 3)
    count = float(a[0].size)
    d_mu1, d_e11, d_e12, d_mu2, d_e22 = planes(x, y, pad)
    adj = lambda t: conv(t, pad, shift)
    c12 = adj(d_e12)
    out = []
    for u, v, d_mu, d_euu in ((x, y, d_mu1, d_e11), (y, x, d_mu2, d_e22)):
        s = adj(d_mu) + (0.0 if drop_e11 else 2 * u * adj(d_euu)) + v * c12
        d = u - v          # exact: the inputs are float32
        out.append((wt[:, 0, None, None, None] * s + wt[:, 1, None, None, None] * 2 * d + wt[:, 2, None, None, None] * np.sign(d)) / count)
    return out[0], out[1]


def distance(got, want):
    """Per frame: the largest |got - want| in units of the frame's largest |want|.  [n]"""
    n = want.shape[0]
    err = np.abs(got.astype(np.float64) - want).reshape(n, -1).max(axis=1)
    return err / np.abs(want).reshape(n, -1).max(axis=1)
