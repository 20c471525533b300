"""NumPy restatement of OpenCV 4.x's CPU ``calcOpticalFlowFarneback`` (flags = 0) and of the reference video callers' frame
preparation (video/utils.py:75-86, :330-332): the yardstick of csrc/flow.hip.

The rules are written from OpenCV's published source (modules/video/src/optflowgf.cpp, imgproc/src/resize.cpp,
smooth.dispatch.cpp); nothing in this project runs cv2, so parity with cv2 itself is unpinned (as for resize_area_u8 and warp_u8).

* Level count: ``scale = 1; for k in 0..levels-1: scale *= pyr_scale; break if cols*scale < 32 or rows*scale < 32``; the
  effective ``levels`` is the k where the loop stopped and levels k .. 0 (k + 1 of them) are processed, coarse to fine.
* Level size: ``cvRound(cols*scale) x cvRound(rows*scale)``, round half to even.
* Level image, always from the full-resolution frame: float, GaussianBlur with sigma = (1/scale - 1)/2 and ksize =
  max(cvRound(5 sigma) | 1, 3), separable, BORDER_REFLECT_101 (sigma 0 at k = 0: the fixed table 0.25 0.5 0.25); then resize
  INTER_LINEAR with float taps fx = (float)((dx+0.5)*scale_x - 0.5) clamped at both ends (rows clamped, their weights kept); an
  exact 2x shrink on both axes is INTER_AREA (2x2 mean), an equal size a copy.
* Polynomial expansion (FarnebackPolyExp): half-width n = poly_n, weights g, x g, x^2 g of a Gaussian of poly_sigma,
  coefficients ig11, ig03, ig33, ig55 of the inverse 6x6 moment matrix; vertical pass into 3 values per pixel, horizontal pass
  (OpenCV: float vertical pass, double horizontal accumulation); replicated borders; 5 outputs in OpenCV's order y, x, yy, xx, xy.
* Matrix update (FarnebackUpdateMatrices): R1 sampled bilinearly at (x+dx, y+dy) when 0 <= floor(x+dx) < w-1 and
  0 <= floor(y+dy) < h-1, OpenCV's "else" branch otherwise; border weights {0.14, 0.14, 0.4472, 0.4472, 0.4472} on the outer 5
  pixels, applied where OpenCV's unsigned test holds (border_scale: on frames narrower than 10 that is not "the outer 5");
  outputs G11, G12, G22, h1, h2.
* Flow update (FarnebackUpdateFlow_Blur): box sum over 2*(winsize//2)+1 pixels each way, replicated borders, scaled by
  1/winsize^2 (double); idet = 1/(g11 g22 - g12^2 + 1e-3), flow_x = (g11 h2 - g12 h1) idet, flow_y = (g22 h1 - g12 h2) idet; M
  is recomputed from the new flow after every iteration but the last; ``iterations`` rounds per level.
* Between levels the flow is resized with the float INTER_LINEAR and multiplied by 1/pyr_scale (also where cvRound made the size
  ratio differ); the coarsest level starts from zero flow.
* Frame preparation: cv2.imread gives BGR; cv2.resize to target_resolution (uint8 INTER_LINEAR: 2048-scaled taps and
  VResizeLinear's fixed-point combine; exact 2x shrink: INTER_AREA's (a+b+c+d+2)>>2; equal size: copy), then COLOR_RGB2GRAY on the
  BGR data, i.e. in PIL's RGB order gray = (4899 B + 9617 G + 1868 R + 8192) >> 14.  Unpinned too: OpenCV applies EXIF
  orientation and PIL does not, and JPEG decoders may differ.

``dtype=np.float64`` is the yardstick; ``np.float32`` puts fp32 where OpenCV uses float (taps, level images, the vertical
expansion pass, R, M, flows) to measure the noise floor of a float implementation.  The box sums are exact cumulative sums in
double in both modes (OpenCV's running sums add float differences - a rounding of the same order this mode does not copy).
"""
import numpy as np

BORDER = np.array([0.14, 0.14, 0.4472, 0.4472, 0.4472], dtype=np.float32)


def cv_round(x):
    return int(np.rint(x))


def level_schedule(h, w, pyr_scale=0.5, levels=5):
    """[(w_k, h_k, ksize, sigma, scale)] for k = 0 (full size) .. L (coarsest)."""
    k, scale = 0, 1.0
    while k < levels:
        scale *= pyr_scale
        if w * scale < 32 or h * scale < 32:
            break
        k += 1
    out = []
    for i in range(k + 1):
        s = 1.0
        for _ in range(i):
            s *= pyr_scale
        sigma = (1.0 / s - 1) * 0.5
        ks = max(cv_round(sigma * 5) | 1, 3)
        out.append((cv_round(w * s), cv_round(h * s), ks, sigma, s))
    return out


def gaussian_taps(n, sigma, dtype):
    """getGaussianKernel(n, sigma) in float (OpenCV's CV_32F kernel) or double."""
    x = np.arange(n) - (n - 1) * 0.5
    if n == 3 and sigma <= 0:
        t = np.array([0.25, 0.5, 0.25])
    else:
        sx = sigma if sigma > 0 else ((n - 1) * 0.5 - 1) * 0.3 + 0.8
        t = np.exp(-0.5 / (sx * sx) * x * x)
    t = t.astype(dtype)
    return (t.astype(np.float64) * (1.0 / t.astype(np.float64).sum())).astype(dtype)


def reflect101(p, n):
    if n == 1:
        return np.zeros_like(p)
    period = 2 * n - 2
    p = np.mod(p, period)
    return np.where(p < n, p, period - p)


def gaussian_blur(img, ks, sigma, dtype):
    taps = gaussian_taps(ks, sigma, dtype)
    h, w = img.shape
    r = ks // 2
    tmp = np.zeros((h, w), dtype)
    for t in range(ks):
        tmp = tmp + taps[t] * img[:, reflect101(np.arange(w) - r + t, w)]
    out = np.zeros((h, w), dtype)
    for t in range(ks):
        out = out + taps[t] * tmp[reflect101(np.arange(h) - r + t, h), :]
    return out


def resize_mode(hi, wi, ho, wo, sx, sy):
    """cv::resize's choice for (hi, wi) -> (ho, wo) with the source-per-destination scales sx, sy (csrc/cv_resize.h): 0 copy,
    1 INTER_AREA's 2x2 mean at an exact 2x shrink, 2 linear."""
    if (ho, wo) == (hi, wi):
        return 0
    ix, iy = cv_round(sx), cv_round(sy)
    fast = abs(sx - ix) < 2.220446049250313e-16 and abs(sy - iy) < 2.220446049250313e-16
    return 1 if fast and ix == 2 and iy == 2 else 2


def _resize_mode(hi, wi, ho, wo):
    sx, sy = 1.0 / (wo / wi), 1.0 / (ho / hi)
    return resize_mode(hi, wi, ho, wo, sx, sy), sx, sy


def _lin_taps(dsize, ssize, scale, xaxis):
    f = ((np.arange(dsize) + 0.5) * scale - 0.5).astype(np.float32)
    s = np.floor(f).astype(np.int64)
    f = (f - s.astype(np.float32)).astype(np.float32)
    if xaxis:
        lo = s < 0
        f[lo], s[lo] = 0, 0
        hi = s >= ssize - 1
        f[hi], s[hi] = 0, ssize - 1
        s1 = np.minimum(s + 1, ssize - 1)
    else:
        s1 = np.clip(s + 1, 0, ssize - 1)
        s = np.clip(s, 0, ssize - 1)
    return s, s1, f


def resize_linear(src, wo, ho, dtype):
    """cv2.resize(float image, (wo, ho)) with INTER_LINEAR on [h, w] or [c, h, w] planes."""
    hi, wi = src.shape[-2:]
    mode, sx, sy = _resize_mode(hi, wi, ho, wo)
    if mode == 0:
        return src.astype(dtype).copy()
    if mode == 1:
        s = src.astype(dtype)
        return (((s[..., 0::2, 0::2] + s[..., 0::2, 1::2]) + s[..., 1::2, 0::2]) + s[..., 1::2, 1::2]) * dtype(0.25)
    x0, x1, fx = _lin_taps(wo, wi, sx, True)
    y0, y1, fy = _lin_taps(ho, hi, sy, False)
    a0, a1 = (np.float32(1) - fx).astype(dtype), fx.astype(dtype)
    b0, b1 = (np.float32(1) - fy).astype(dtype)[:, None], fy.astype(dtype)[:, None]
    s = src.astype(dtype)
    hr = s[..., :, x0] * a0 + s[..., :, x1] * a1
    return hr[..., y0, :] * b0 + hr[..., y1, :] * b1


def level_image(gray, wl, hl, ks, sigma, dtype):
    return resize_linear(gaussian_blur(gray.astype(dtype), ks, sigma, dtype), wl, hl, dtype)


def poly_coeffs(n, sigma, dtype):
    if sigma < 1.1920928955078125e-07:
        sigma = n * 0.3
    x = np.arange(-n, n + 1)
    g = np.exp(-x * x / (2 * sigma * sigma)).astype(dtype)
    g = (g.astype(np.float64) * (1.0 / g.astype(np.float64).sum())).astype(dtype)
    xg, xxg = (x * g.astype(np.float64)).astype(dtype), (x * x * g.astype(np.float64)).astype(dtype)
    gd = g.astype(np.float64)
    G = np.zeros((6, 6))
    gg = np.outer(gd, gd)
    X, Y = np.meshgrid(x, x)
    G[0, 0] = gg.sum()
    G[1, 1] = (gg * X * X).sum()
    G[3, 3] = (gg * X ** 4).sum()
    G[5, 5] = (gg * X * X * Y * Y).sum()
    G[2, 2] = G[0, 3] = G[0, 4] = G[3, 0] = G[4, 0] = G[1, 1]
    G[4, 4] = G[3, 3]
    G[3, 4] = G[4, 3] = G[5, 5]
    iG = np.linalg.inv(G)
    return g[n:], xg[n:], xxg[n:], iG[1, 1], iG[0, 3], iG[3, 3], iG[5, 5]


def poly_exp(img, n, sigma, dtype):
    """[h, w] -> R [h, w, 5] (y, x, yy, xx, xy)."""
    g, xg, xxg, ig11, ig03, ig33, ig55 = poly_coeffs(n, sigma, dtype)
    h, w = img.shape
    I = img.astype(dtype)
    ys = np.arange(h)
    r0 = I * g[0]
    r1 = np.zeros_like(I)
    r2 = np.zeros_like(I)
    for k in range(1, n + 1):
        s0, s1 = I[np.maximum(ys - k, 0)], I[np.minimum(ys + k, h - 1)]
        p = s0 + s1
        r0 = r0 + g[k] * p
        r1 = r1 + xg[k] * (s1 - s0)
        r2 = r2 + xxg[k] * p
    xs = np.arange(w)
    f64 = np.float64
    b1 = (r0 * g[0]).astype(f64)
    b3 = (r1 * g[0]).astype(f64)
    b5 = (r2 * g[0]).astype(f64)
    b2 = np.zeros((h, w))
    b4 = np.zeros((h, w))
    b6 = np.zeros((h, w))
    for k in range(1, n + 1):
        R, L = np.minimum(xs + k, w - 1), np.maximum(xs - k, 0)
        tg = (r0[:, R] + r0[:, L]).astype(f64)
        b1 += tg * f64(g[k])
        b4 += tg * f64(xxg[k])
        b2 += ((r0[:, R] - r0[:, L]) * xg[k]).astype(f64)
        b3 += ((r1[:, R] + r1[:, L]) * g[k]).astype(f64)
        b6 += ((r1[:, R] - r1[:, L]) * xg[k]).astype(f64)
        b5 += ((r2[:, R] + r2[:, L]) * g[k]).astype(f64)
    out = np.stack([b3 * ig11, b2 * ig11, b1 * ig03 + b5 * ig33, b1 * ig03 + b4 * ig33, b6 * ig55], axis=-1)
    return out.astype(dtype)


def border_scale(h, w):
    """FarnebackUpdateMatrices' border weight per pixel, float32 [h, w].  OpenCV tests ``(unsigned)(x - 5) >= (unsigned)(width - 10)
    || (unsigned)(y - 5) >= (unsigned)(height - 10)`` in 32-bit unsigned arithmetic and, where that holds, multiplies by
    border[x] (x < 5), border[width - x - 1] (x >= width - 5) and the same two factors in y.  For width >= 10 the x test is
    "x < 5 or x >= width - 5".  Below 10 ``width - 10`` wraps to 2^32 - (10 - width) and the test holds only for
    max(width - 5, 0) <= x < 5: columns 3, 4 of an 8-wide frame, every column of one at most 5 wide.  A pixel that passes through
    its row takes the column factors as well, whatever the column test said."""
    def test(n):
        i = np.arange(n, dtype=np.int64)
        return ((i - 5) % (1 << 32)) >= ((n - 10) % (1 << 32))

    def factors(n):
        lo = np.ones(n, np.float32)
        hi = np.ones(n, np.float32)
        i = np.arange(n)
        lo[i < 5] = BORDER[i[i < 5]]
        hi[i >= n - 5] = BORDER[(n - i - 1)[i >= n - 5]]
        return lo, hi

    xl, xh = factors(w)
    yl, yh = factors(h)
    scale = ((xl[None, :] * xh[None, :]) * yl[:, None]) * yh[:, None]
    return np.where(test(w)[None, :] | test(h)[:, None], scale, np.float32(1)).astype(np.float32)


def update_matrices(R0, R1, flow, dtype):
    """R0, R1 [h, w, 5]; flow [2, h, w] (x, y) -> M [h, w, 5]."""
    h, w = flow.shape[1:]
    t = dtype
    dx, dy = flow[0].astype(t), flow[1].astype(t)
    X, Y = np.meshgrid(np.arange(w), np.arange(h))
    fx, fy = X.astype(t) + dx, Y.astype(t) + dy
    x1, y1 = np.floor(fx).astype(np.int64), np.floor(fy).astype(np.int64)
    fx, fy = fx - x1.astype(t), fy - y1.astype(t)
    inside = (x1 >= 0) & (x1 < w - 1) & (y1 >= 0) & (y1 < h - 1)
    xa, ya = np.clip(x1, 0, max(w - 2, 0)), np.clip(y1, 0, max(h - 2, 0))
    xb, yb = np.minimum(xa + 1, w - 1), np.minimum(ya + 1, h - 1)
    one = t(1)
    a00, a01, a10, a11 = (one - fx) * (one - fy), fx * (one - fy), (one - fx) * fy, fx * fy
    R1 = R1.astype(t)
    R0 = R0.astype(t)
    s = [a00 * R1[ya, xa, c] + a01 * R1[ya, xb, c] + a10 * R1[yb, xa, c] + a11 * R1[yb, xb, c] for c in range(5)]
    half, quarter = t(0.5), t(0.25)
    r2 = np.where(inside, s[0], t(0))
    r3 = np.where(inside, s[1], t(0))
    r4 = np.where(inside, (R0[..., 2] + s[2]) * half, R0[..., 2])
    r5 = np.where(inside, (R0[..., 3] + s[3]) * half, R0[..., 3])
    r6 = np.where(inside, (R0[..., 4] + s[4]) * quarter, R0[..., 4] * half)
    r2 = (R0[..., 0] - r2) * half
    r3 = (R0[..., 1] - r3) * half
    r2 = r2 + (r4 * dy + r6 * dx)
    r3 = r3 + (r6 * dy + r5 * dx)

    scale = border_scale(h, w).astype(t)
    r2, r3, r4, r5, r6 = (v * scale for v in (r2, r3, r4, r5, r6))
    return np.stack([r4 * r4 + r6 * r6, (r4 + r5) * r6, r5 * r5 + r6 * r6, r4 * r2 + r6 * r3, r6 * r2 + r5 * r3], axis=-1).astype(t)


def box_sum(M, m):
    """Sum over (2m+1)^2 with replicated borders, in double."""
    h, w = M.shape[:2]
    P = np.pad(M.astype(np.float64), ((m + 1, m), (m + 1, m), (0, 0)), mode="edge")
    P[0, :] = 0
    P[:, 0] = 0
    C = P.cumsum(0).cumsum(1)
    k = 2 * m + 1
    return C[k:k + h, k:k + w] - C[0:h, k:k + w] - C[k:k + h, 0:w] + C[0:h, 0:w]


def solve_flow(M, winsize, dtype):
    S = box_sum(M, winsize // 2) * (1.0 / (winsize * winsize))
    g11, g12, g22, h1, h2 = (S[..., c] for c in range(5))
    idet = 1.0 / (g11 * g22 - g12 * g12 + 1e-3)
    return np.stack([(g11 * h2 - g12 * h1) * idet, (g22 * h1 - g12 * h2) * idet]).astype(dtype)


def pyramid(gray, pyr_scale=0.5, levels=5, poly_n=7, poly_sigma=1.5, dtype=np.float64):
    """[(level image, R)] for k = 0 .. L: what adain_farneback_expand stores."""
    h, w = gray.shape
    out = []
    for (wl, hl, ks, sigma, _s) in level_schedule(h, w, pyr_scale, levels):
        I = level_image(gray, wl, hl, ks, sigma, dtype)
        out.append((I, poly_exp(I, poly_n, poly_sigma, dtype)))
    return out


def flow_from_pyramids(p0, p1, pyr_scale=0.5, winsize=15, iterations=3, dtype=np.float64):
    flow = None
    for k in range(len(p0) - 1, -1, -1):
        R0, R1 = p0[k][1], p1[k][1]
        hl, wl = R0.shape[:2]
        if flow is None:
            flow = np.zeros((2, hl, wl), dtype)
        else:
            inv = np.float32(1.0 / pyr_scale) if dtype == np.float32 else 1.0 / pyr_scale
            flow = (resize_linear(flow, wl, hl, dtype) * inv).astype(dtype)
        M = update_matrices(R0, R1, flow, dtype)
        for i in range(iterations):
            flow = solve_flow(M, winsize, dtype)
            if i < iterations - 1:
                M = update_matrices(R0, R1, flow, dtype)
    return flow


def farneback(prev, nxt, pyr_scale=0.5, levels=5, winsize=15, iterations=3, poly_n=7, poly_sigma=1.5, dtype=np.float64):
    """calcOpticalFlowFarneback(prev, next, None, ..., flags=0) -> [2, h, w] (x, y)."""
    p0 = pyramid(prev, pyr_scale, levels, poly_n, poly_sigma, dtype)
    p1 = pyramid(nxt, pyr_scale, levels, poly_n, poly_sigma, dtype)
    return flow_from_pyramids(p0, p1, pyr_scale, winsize, iterations, dtype)


def resize_linear_u8(img, wo, ho):
    """cv2.resize(uint8 [h, w, c], (wo, ho)) INTER_LINEAR in OpenCV's fixed point."""
    hi, wi = img.shape[:2]
    mode, sx, sy = _resize_mode(hi, wi, ho, wo)
    if mode == 0:
        return img.copy()
    s = img.astype(np.int64)
    if mode == 1:
        return ((s[0::2, 0::2] + s[0::2, 1::2] + s[1::2, 0::2] + s[1::2, 1::2] + 2) >> 2).astype(np.uint8)
    x0, x1, fx = _lin_taps(wo, wi, sx, True)
    y0, y1, fy = _lin_taps(ho, hi, sy, False)
    a0 = np.rint((np.float32(1) - fx) * np.float32(2048)).astype(np.int64)[None, :, None]
    a1 = np.rint(fx * np.float32(2048)).astype(np.int64)[None, :, None]
    b0 = np.rint((np.float32(1) - fy) * np.float32(2048)).astype(np.int64)[:, None, None]
    b1 = np.rint(fy * np.float32(2048)).astype(np.int64)[:, None, None]
    H = s[:, x0] * a0 + s[:, x1] * a1
    return ((((b0 * (H[y0] >> 4)) >> 16) + ((b1 * (H[y1] >> 4)) >> 16) + 2) >> 2).astype(np.uint8)


def frame_to_gray(rgb, wo, ho):
    """The reference's frame preparation on a PIL-order RGB uint8 frame: resize the BGR frame, COLOR_RGB2GRAY on BGR data."""
    v = resize_linear_u8(rgb, wo, ho).astype(np.int64)
    return ((4899 * v[..., 2] + 9617 * v[..., 1] + 1868 * v[..., 0] + 8192) >> 14).astype(np.uint8)


def texture(h, w, shift=(0.0, 0.0), seed=0):
    """A band-limited texture sampled analytically at (x - sx, y - sy): frame 2 of a pure sub-pixel translation by (sx, sy)."""
    rng = np.random.default_rng(seed)
    Y, X = np.mgrid[0:h, 0:w].astype(np.float64)
    X, Y = X - shift[0], Y - shift[1]
    v = np.zeros((h, w))
    for _ in range(12):
        fx, fy = rng.uniform(-0.08, 0.08, 2)
        v += rng.uniform(0.5, 1.0) * np.cos(2 * np.pi * (fx * X + fy * Y) + rng.uniform(0, 2 * np.pi))
    v = 128 + 100 * v / np.abs(v).max()
    return np.clip(np.rint(v), 0, 255).astype(np.uint8)


def endpoint_error(a, b):
    return np.hypot(a[0] - b[0], a[1] - b[1])
