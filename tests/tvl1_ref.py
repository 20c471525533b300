"""NumPy restatement of OpenCV 4.x's contrib ``DualTVL1OpticalFlow`` (optflow module, CPU path), as the reference's video callers
run it (video/utils.py:75-86: ``cv2.optflow.DualTVL1OpticalFlow_create().calc(prev, next, None)``): the yardstick of csrc/tvl1.hip.

The rules are written from OpenCV's published source (optflow/src/tvl1flow.cpp, imgproc resize.cpp / imgwarp.cpp /
median_blur.simd.hpp); nothing in this project runs cv2, so parity with cv2 itself is unpinned (DESIGN.md section 8 lists the
uncertain readings in item 11).

* Input: uint8 gray -> float, values 0..255.
* Scales: level s = resize(level s-1, Size(), scaleStep, scaleStep, INTER_LINEAR), size cvRound(w*scaleStep) x cvRound(h*scaleStep),
  source coordinates scaled by 1/scaleStep; stop (and drop the level) as soon as it has fewer than 16 columns or rows.
* Per scale: u = 0 at the coarsest, else the coarser u resized to this size (INTER_LINEAR, size ratio) times (float)(1/scaleStep);
  p = 0; I1x, I1y centred differences (one-sided at the borders, times 0.5); scaledEpsilon = (float)(epsilon^2 w h);
  l_t = (float)(lambda theta), taut = (float)(tau / theta).
* Per warp: remap I1, I1x, I1y at (x + u1, y + u2) with INTER_CUBIC (map rounded to 1/32 px, window from floor - 1, taps the
  float products of interpolateCubic's coefficients (A = -0.75) at k/32, BORDER_CONSTANT 0); grad = I1wx^2 + I1wy^2,
  rho_c = I1w - I1wx u1 - I1wy u2 - I0.  error = FLT_MAX.
* Outer loop (while error > scaledEpsilon, at most outerIterations): medianBlur(u1 | u2, medianFiltering) if > 1 (replicate
  border); inner loop (while error > scaledEpsilon, at most innerIterations): thresholding V, divergence of p (backward
  differences; row 0 / column 0 keep the value), u = v + theta div, error = sum du^2, forward gradient of u (0 in the last column /
  row), p = (p + taut grad u) / (1 + taut |grad u|).

``dtype=np.float64`` is the yardstick (the tap tables and the float-cast constants stay OpenCV's floats: they are part of the rule);
``np.float32`` does every per-pixel operation in float, in OpenCV's order, to measure the noise floor of a float implementation.
The stop rule's error is summed in float64 in both modes (OpenCV sums it in float in an unpinned thread order).
"""
import numpy as np

import farneback_ref as F

FLT_MAX = float(np.finfo(np.float32).max)
FLT_EPSILON = float(np.finfo(np.float32).eps)
DEFAULTS = dict(tau=0.25, lambda_=0.15, theta=0.3, nscales=5, warps=5, epsilon=0.01, innerIterations=30, outerIterations=10,
                scaleStep=0.8, gamma=0.0, medianFiltering=5, useInitialFlow=False)


def scales(h, w, nscales=5, scaleStep=0.8):
    """[(w_s, h_s)] for s = 0 (full size) .. coarsest."""
    out = [(w, h)]
    for _ in range(1, nscales):
        pw, ph = out[-1]
        nw, nh = F.cv_round(pw * scaleStep), F.cv_round(ph * scaleStep)
        if nw < 16 or nh < 16:
            break
        out.append((nw, nh))
    return out


def resize(src, wo, ho, sx, sy, dtype):
    """cv::resize INTER_LINEAR of a float plane with source-per-destination scales sx, sy (copy at an equal size; INTER_AREA's 2x2
    mean, over the source pixels inside the image, at an exact 2x)."""
    hi, wi = src.shape
    s = src.astype(dtype)
    mode = F.resize_mode(hi, wi, ho, wo, sx, sy)
    if mode == 0:
        return s.copy()
    if mode == 1:
        out = np.zeros((ho, wo), dtype)
        for y in range(ho):
            for x in range(wo):
                ys, xs = [v for v in (2 * y, 2 * y + 1) if v < hi], [v for v in (2 * x, 2 * x + 1) if v < wi]
                if len(ys) == 2 and len(xs) == 2:
                    out[y, x] = (((s[ys[0], xs[0]] + s[ys[0], xs[1]]) + s[ys[1], xs[0]]) + s[ys[1], xs[1]]) * dtype(0.25)
                else:
                    acc = dtype(0)
                    for yy in ys:
                        for xx in xs:
                            acc = acc + s[yy, xx]
                    out[y, x] = acc / dtype(len(ys) * len(xs)) if ys and xs else 0
        return out
    x0, x1, fx = F._lin_taps(wo, wi, sx, True)
    y0, y1, fy = F._lin_taps(ho, hi, sy, False)
    a0, a1 = (np.float32(1) - fx).astype(dtype), fx.astype(dtype)
    b0, b1 = (np.float32(1) - fy).astype(dtype)[:, None], fy.astype(dtype)[:, None]
    hr0 = s[y0][:, x0] * a0 + s[y0][:, x1] * a1
    hr1 = s[y1][:, x0] * a0 + s[y1][:, x1] * a1
    return hr0 * b0 + hr1 * b1


def centered_gradient(I, dtype):
    h, w = I.shape
    xs, ys = np.arange(w), np.arange(h)
    half = dtype(0.5)
    gx = half * (I[:, np.minimum(xs + 1, w - 1)] - I[:, np.maximum(xs - 1, 0)])
    gy = half * (I[np.minimum(ys + 1, h - 1)] - I[np.maximum(ys - 1, 0)])
    return gx.astype(dtype), gy.astype(dtype)


def prepare(gray, nscales=5, scaleStep=0.8, dtype=np.float64):
    """[(I, I_x, I_y)] per scale of one frame."""
    out = []
    I = gray.astype(dtype)
    sc = scales(gray.shape[0], gray.shape[1], nscales, scaleStep)
    for s, (ws, hs) in enumerate(sc):
        if s > 0:
            I = resize(I, ws, hs, 1.0 / scaleStep, 1.0 / scaleStep, dtype)
        out.append((I,) + centered_gradient(I, dtype))
    return out


def cubic_coeffs(x):
    """interpolateCubic(x) in float, OpenCV's operation order."""
    f = np.float32
    A, x = f(-0.75), f(x)
    c0 = ((A * (x + f(1)) - f(5) * A) * (x + f(1)) + f(8) * A) * (x + f(1)) - f(4) * A
    c1 = ((A + f(2)) * x - (A + f(3))) * x * x + f(1)
    c2 = ((A + f(2)) * (f(1) - x) - (A + f(3))) * (f(1) - x) * (f(1) - x) + f(1)
    c3 = f(1) - c0 - c1 - c2
    return np.array([c0, c1, c2, c3], np.float32)


CUBIC = np.stack([cubic_coeffs(np.float32(i) * np.float32(1.0 / 32)) for i in range(32)])   # [32][4] float32


def _round_sat(v):
    v = np.asarray(v, np.float64)
    ok = np.isfinite(v) & (np.abs(v) < 2147483648.0)
    return np.where(ok, np.rint(np.where(ok, v, 0)), -2147483648).astype(np.int64)


def remap_cubic(src_planes, mx, my, dtype):
    """cv::remap(INTER_CUBIC, BORDER_CONSTANT 0) of each plane at float maps (mx, my); the taps are float products."""
    h, w = src_planes[0].shape
    X, Y = _round_sat(mx * dtype(32)), _round_sat(my * dtype(32))
    sx = np.clip(X >> 5, -32768, 32767) - 1
    sy = np.clip(Y >> 5, -32768, 32767) - 1
    wx, wy = CUBIC[X & 31], CUBIC[Y & 31]                 # [h,w,4]
    inside = ((sx >= 0) & (sx < max(w - 3, 0))) & ((sy >= 0) & (sy < max(h - 3, 0)))
    outside = (sx >= w) | (sx + 4 <= 0) | (sy >= h) | (sy + 4 <= 0)
    outs = []
    for S in src_planes:
        S = S.astype(dtype)
        terms = [[None] * 4 for _ in range(4)]
        for r in range(4):
            yy = sy + r
            vy = (yy >= 0) & (yy < h)
            for k in range(4):
                xx = sx + k
                v = vy & (xx >= 0) & (xx < w)
                val = np.where(v, S[np.clip(yy, 0, h - 1), np.clip(xx, 0, w - 1)], dtype(0)).astype(dtype)
                terms[r][k] = (val * (wy[..., r] * wx[..., k]).astype(dtype)).astype(dtype)
        rows = [((t[0] + t[1]) + t[2]) + t[3] for t in terms]
        s_in = ((rows[0] + rows[1]) + rows[2]) + rows[3]
        s_b = np.zeros((h, w), dtype)
        for r in range(4):
            for k in range(4):
                s_b = s_b + terms[r][k]
        outs.append(np.where(inside, s_in, np.where(outside, dtype(0), s_b)).astype(dtype))
    return outs


def median(u, k):
    """medianBlur(u, k) for float data: BORDER_REPLICATE, an exact selection."""
    h, w = u.shape
    r = k // 2
    ys, xs = np.arange(h), np.arange(w)
    vals = np.stack([u[np.clip(ys + dy, 0, h - 1)][:, np.clip(xs + dx, 0, w - 1)] for dy in range(-r, r + 1) for dx in range(-r, r + 1)])
    return np.partition(vals, k * k // 2, axis=0)[k * k // 2]


def divergence(v1, v2):
    div = np.empty_like(v1)
    div[1:, 1:] = (v1[1:, 1:] - v1[1:, :-1]) + (v2[1:, 1:] - v2[:-1, 1:])
    div[0, 1:] = (v1[0, 1:] - v1[0, :-1]) + v2[0, 1:]
    div[1:, 0] = (v1[1:, 0] + v2[1:, 0]) - v2[:-1, 0]
    div[0, 0] = v1[0, 0] + v2[0, 0]
    return div


def forward_gradient(u):
    dx = np.zeros_like(u)
    dy = np.zeros_like(u)
    dx[:, :-1] = u[:, 1:] - u[:, :-1]
    dy[:-1, :] = u[1:, :] - u[:-1, :]
    return dx, dy


def estimate_v(I1wx, I1wy, u1, u2, grad, rho_c, l_t, dtype):
    rho = rho_c + (I1wx * u1 + I1wy * u2)
    lt = dtype(l_t)
    a = rho < -lt * grad
    b = ~a & (rho > lt * grad)
    c = ~a & ~b & (grad > FLT_EPSILON)
    with np.errstate(divide="ignore", invalid="ignore"):
        fi = np.where(c, -rho / np.where(c, grad, dtype(1)), dtype(0)).astype(dtype)
    d1 = np.where(a, lt * I1wx, np.where(b, -lt * I1wx, np.where(c, fi * I1wx, dtype(0)))).astype(dtype)
    d2 = np.where(a, lt * I1wy, np.where(b, -lt * I1wy, np.where(c, fi * I1wy, dtype(0)))).astype(dtype)
    return (u1 + d1).astype(dtype), (u2 + d2).astype(dtype)


def inner_step(state, C, l_t, theta, taut, dtype):
    """One inner step; returns the error (float64 sum)."""
    I1wx, I1wy, grad, rho_c = C
    u1, u2, p11, p12, p21, p22 = state
    v1, v2 = estimate_v(I1wx, I1wy, u1, u2, grad, rho_c, l_t, dtype)
    th = dtype(theta)
    n1 = (v1 + th * divergence(p11, p12)).astype(dtype)
    n2 = (v2 + th * divergence(p21, p22)).astype(dtype)
    e1, e2 = n1 - u1, n2 - u2
    err = float(np.sum((e1 * e1 + e2 * e2).astype(np.float64)))
    u1x, u1y = forward_gradient(n1)
    u2x, u2y = forward_gradient(n2)
    t = dtype(taut)
    g1 = np.hypot(u1x.astype(np.float64), u1y.astype(np.float64)).astype(dtype)
    g2 = np.hypot(u2x.astype(np.float64), u2y.astype(np.float64)).astype(dtype)
    ng1, ng2 = dtype(1) + t * g1, dtype(1) + t * g2
    state[:] = [n1, n2, ((p11 + t * u1x) / ng1).astype(dtype), ((p12 + t * u1y) / ng1).astype(dtype),
                ((p21 + t * u2x) / ng2).astype(dtype), ((p22 + t * u2y) / ng2).astype(dtype)]
    return err


def warp_constants(I0, I1, u1, u2, dtype):
    h, w = I0[0].shape
    ys, xs = np.mgrid[0:h, 0:w]
    mx = (xs.astype(dtype) + u1).astype(dtype)
    my = (ys.astype(dtype) + u2).astype(dtype)
    I1w, I1wx, I1wy = remap_cubic(I1, mx, my, dtype)
    grad = (I1wx * I1wx + I1wy * I1wy).astype(dtype)
    rho_c = (((I1w - I1wx * u1) - I1wy * u2) - I0[0]).astype(dtype)
    return I1wx, I1wy, grad, rho_c


def tvl1_prepared(P0, P1, dtype=np.float64, **params):
    """The flow of two prepared frames (lists of (I, I_x, I_y) per scale) -> (flow [2,h,w], iters [nscales][warps], margins)."""
    p = dict(DEFAULTS, **params)
    f32 = np.float32
    l_t, taut, theta = f32(p["lambda_"] * p["theta"]), f32(p["tau"] / p["theta"]), f32(p["theta"])
    inv_step = f32(1.0 / p["scaleStep"])
    ns = len(P0)
    iters = np.zeros((ns, p["warps"]), np.int64)
    margins = []
    u1 = u2 = None
    for s in range(ns - 1, -1, -1):
        h, w = P0[s][0].shape
        if u1 is None:
            u1, u2 = np.zeros((h, w), dtype), np.zeros((h, w), dtype)
        else:
            ch, cw = u1.shape
            sx, sy = 1.0 / (w / cw), 1.0 / (h / ch)
            u1 = (resize(u1, w, h, sx, sy, dtype) * dtype(inv_step)).astype(dtype)
            u2 = (resize(u2, w, h, sx, sy, dtype) * dtype(inv_step)).astype(dtype)
        z = np.zeros((h, w), dtype)
        state = [u1, u2, z, z.copy(), z.copy(), z.copy()]
        eps = float(f32(p["epsilon"] * p["epsilon"] * (w * h)))
        for wi in range(p["warps"]):
            C = warp_constants(P0[s], P1[s], state[0], state[1], dtype)
            error = FLT_MAX
            n_outer = 0
            while error > eps and n_outer < p["outerIterations"]:
                if p["medianFiltering"] > 1:
                    state[0] = median(state[0], p["medianFiltering"])
                    state[1] = median(state[1], p["medianFiltering"])
                n_inner = 0
                while error > eps and n_inner < p["innerIterations"]:
                    error = inner_step(state, C, l_t, theta, taut, dtype)
                    margins.append(abs(error - eps) / eps if eps > 0 else np.inf)   # epsilon 0: nothing is near the threshold
                    iters[s, wi] += 1
                    n_inner += 1
                n_outer += 1
        u1, u2 = state[0], state[1]
    return np.stack([u1, u2]), iters, np.array(margins)


def tvl1(I0, I1, dtype=np.float64, **params):
    """``DualTVL1OpticalFlow_create(**params).calc(I0, I1, None)`` on uint8 [h,w] frames -> (flow [2,h,w], iters, margins)."""
    p = dict(DEFAULTS, **params)
    P0 = prepare(I0, p["nscales"], p["scaleStep"], dtype)
    P1 = prepare(I1, p["nscales"], p["scaleStep"], dtype)
    return tvl1_prepared(P0, P1, dtype, **params)


texture = F.texture
endpoint_error = F.endpoint_error
