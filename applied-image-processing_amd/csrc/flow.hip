// Dense optical flow: OpenCV 4.x's CPU calcOpticalFlowFarneback with flags = 0 (Farneback 2003, "Two-frame motion estimation
// based on polynomial expansion"), as the reference's video callers run it per frame pair (video/utils.py:75-86:
// cv2.calcOpticalFlowFarneback(prev, next, None, 0.5, 5, 15, 3, 7, 1.5, 0)), plus the frame preparation those callers do.
//
// Rules (restated from OpenCV's published optflowgf.cpp / resize.cpp / smooth.dispatch.cpp; parity with cv2 itself is not pinned
// on any machine of this project - tests/farneback_ref.py restates the same rules in NumPy and is the yardstick):
//   levels    scale = 1; for k in 0..levels-1 { scale *= pyr_scale; if cols*scale < 32 || rows*scale < 32: break }; the effective
//             count is that k, and levels k .. 0 are processed (k + 1 pyramid levels), coarse to fine.
//   level k   scale = pyr_scale^k (repeated multiplication), size cvRound(cols*scale) x cvRound(rows*scale) (round half to even);
//             image = resize(GaussianBlur(float(frame), ksize, sigma), size, INTER_LINEAR) from the FULL-resolution frame, with
//             sigma = (1/scale - 1)/2, ksize = max(cvRound(5 sigma) | 1, 3), separable float taps of getGaussianKernel (sigma 0:
//             the fixed table 0.25 0.5 0.25), BORDER_REFLECT_101.  The float resize: fx = (float)((dx+0.5)*scale_x - 0.5), taps
//             (1-fx, fx), clamped at both ends (rows clamped, their weights kept); an exact 2x shrink on both axes is INTER_AREA
//             (2x2 mean), an equal size a copy.
//   R         FarnebackPolyExp: separable (2n+1)^2 window (n = poly_n) of g, x g, x^2 g (g: Gaussian of poly_sigma normalised in
//             double, stored as float), coefficients ig11, ig03, ig33, ig55 of the inverse 6x6 moment matrix; a float vertical
//             pass, a horizontal pass accumulated in double; replicated borders; 5 floats per pixel: y, x, yy, xx, xy.
//   M         FarnebackUpdateMatrices: R1 sampled bilinearly at (x+dx, y+dy) when floor(x+dx) < w-1 and floor(y+dy) < h-1 (both
//             >= 0), OpenCV's "else" branch otherwise; the 5-pixel border weights 0.14 0.14 0.4472 0.4472 0.4472; 5 floats:
//             G11, G12, G22, h1, h2.
//   flow      FarnebackUpdateFlow_Blur: winsize^2 box mean of M (window 2*(winsize/2)+1, scale 1/winsize^2, replicated borders,
//             double), idet = 1/(g11 g22 - g12^2 + 1e-3), flow_x = (g11 h2 - g12 h1) idet, flow_y = (g22 h1 - g12 h2) idet; M is
//             recomputed from the new flow after every iteration but the last.
//   between   the coarser flow is resized with the float INTER_LINEAR to the next level's size and multiplied by 1/pyr_scale
//             (even when cvRound made the size ratio differ from 1/pyr_scale); the coarsest level starts from zero flow.
//
// Kernels: a frame's pyramid (level images + R, adain_farneback_expand) depends on that frame only, so a clip of N frames needs N
// expansions; the flow (adain_farneback_flow) of a pair runs per level one matrix update (fused with the flow upscale) and
// `iterations` fused box-blur + solve + matrix-update launches that ping-pong M between two buffers.  No atomics, no data-
// dependent order: the same inputs give the same bits.  The file is compiled with -ffp-contract=off: the float operations stay
// OpenCV's, one by one, and the flow equals the float32 mode of tests/farneback_ref.py bit for bit (fused multiply-adds are no less
// accurate on average, but on narrow frames, where every pixel solves nearly the same ill-conditioned 2 x 2 system, they moved the
// flow by up to 4.5e-5 px, more than twice the float32 restatement's own distance from float64 on some fixtures).
#include "common.h"
#include "cv_resize.h"

namespace adain {

constexpr int FB_MAX_LEVELS = 64;
constexpr int FB_MAX_TAPS = 512;      // Gaussian taps per level (ksize <= 511: frames whose shorter side is below ~6000 pixels)
constexpr int FB_MAX_POLY_N = 7;
constexpr int FB_MAX_HALF_WIN = 31;   // winsize <= 63

struct FbTaps { float t[FB_MAX_TAPS]; };
struct FbPoly { float g[FB_MAX_POLY_N + 1], xg[FB_MAX_POLY_N + 1], xxg[FB_MAX_POLY_N + 1]; double ig11, ig03, ig33, ig55; };

struct FbLevel { int w, h, ksize; double scale, sigma; size_t img_off, r_off; };   // offsets in floats into the pyramid

// the level schedule; returns the effective `levels` (the coarsest k) or ADAIN_EINVAL (< 0) when the parameters are refused.  The
// single source of a pyramid's layout: every level's image and its polynomial expansion start on a multiple of 256 bytes.
static int fb_schedule(int h, int w, double pyr_scale, int levels, FbLevel* L, size_t* pyramid_floats) {
    if (h < 1 || w < 1 || !(pyr_scale > 0.0 && pyr_scale < 1.0) || levels < 0) return ADAIN_EINVAL;
    int k = 0;
    double scale = 1.0;
    for (k = 0; k < levels; ++k) {
        scale *= pyr_scale;
        if (w * scale < 32 || h * scale < 32) break;
    }
    if (k + 1 > FB_MAX_LEVELS) return ADAIN_EINVAL;
    Carve c;
    for (int i = 0; i <= k; ++i) {
        double s = 1.0;
        for (int j = 0; j < i; ++j) s *= pyr_scale;
        const double sigma = (1. / s - 1) * 0.5;
        int ks = (int)nearbyint(sigma * 5) | 1;
        ks = ks < 3 ? 3 : ks;
        L[i].scale = s;
        L[i].sigma = sigma;
        L[i].ksize = ks;
        L[i].w = (int)nearbyint(w * s);
        L[i].h = (int)nearbyint(h * s);
        L[i].img_off = c.take((size_t)L[i].w * L[i].h * sizeof(float)) / sizeof(float);
        L[i].r_off = c.take((size_t)L[i].w * L[i].h * 5 * sizeof(float)) / sizeof(float);
    }
    if (pyramid_floats) *pyramid_floats = c.at / sizeof(float);
    return k;
}

// getGaussianKernel(ksize, sigma, CV_32F): taps computed in double, stored as float, normalised by the double sum of the floats
static void fb_gauss_taps(int n, double sigma, FbTaps& T) {
    static const float tab3[3] = {0.25f, 0.5f, 0.25f};
    const bool fixed = n == 3 && sigma <= 0;
    const double sx = sigma > 0 ? sigma : ((n - 1) * 0.5 - 1) * 0.3 + 0.8;
    const double scale2x = -0.5 / (sx * sx);
    double sum = 0;
    for (int i = 0; i < n; ++i) {
        const double x = i - (n - 1) * 0.5;
        const double t = fixed ? (double)tab3[i] : exp(scale2x * x * x);
        T.t[i] = (float)t;
        sum += T.t[i];
    }
    sum = 1. / sum;
    for (int i = 0; i < n; ++i) T.t[i] = (float)(T.t[i] * sum);
}

// FarnebackPrepareGaussian: g, x g, x^2 g as float and the entries of the inverse moment matrix.  The 6x6 matrix over (1, x, y,
// x^2, y^2, xy) is diagonal in x, y, xy and couples (1, x^2, y^2) as [[a b b] [b c d] [b d c]]: its inverse is closed-form.
static void fb_poly_coeffs(int n, double sigma, FbPoly& P) {
    if (sigma < 1.1920928955078125e-07) sigma = n * 0.3;
    float g[2 * FB_MAX_POLY_N + 1];
    double s = 0;
    for (int x = -n; x <= n; ++x) {
        g[x + n] = (float)exp(-x * x / (2 * sigma * sigma));
        s += g[x + n];
    }
    s = 1. / s;
    for (int x = -n; x <= n; ++x) g[x + n] = (float)(g[x + n] * s);
    double a = 0, b = 0, c = 0, d = 0;
    for (int y = -n; y <= n; ++y)
        for (int x = -n; x <= n; ++x) {
            const double gg = (double)g[y + n] * g[x + n];
            a += gg;
            b += gg * x * x;
            c += gg * x * x * x * x;
            d += gg * x * x * y * y;
        }
    for (int k = 0; k <= n; ++k) {
        P.g[k] = g[k + n];
        P.xg[k] = (float)(k * g[k + n]);
        P.xxg[k] = (float)(k * k * g[k + n]);
    }
    const double D = a * (c + d) - 2 * b * b;
    P.ig11 = 1. / b;
    P.ig03 = -b / D;
    P.ig33 = 0.5 * (a / D + 1. / (c - d));
    P.ig55 = 1. / d;
}

__device__ __forceinline__ int reflect101(int p, int n) {
    if (n == 1) return 0;
    const int period = 2 * n - 2;
    p %= period;
    if (p < 0) p += period;
    return p < n ? p : period - p;
}

// ---- frame preparation: cv2.resize(bgr, (wo, ho)) [uint8 INTER_LINEAR fixed point] + cv2.COLOR_RGB2GRAY on BGR data ----------
// in: PIL's RGB order [n][hi][wi][3]; gray = (4899 B + 9617 G + 1868 R + 8192) >> 14 of the resized channels
__global__ __launch_bounds__(256) void fb_gray_kernel(const uint8_t* __restrict__ rgb, int hi, int wi, uint8_t* __restrict__ gray, int ho,
                                                      int wo, int mode, double scale_x, double scale_y) {
    const int dx = blockIdx.x * 64 + threadIdx.x, dy = blockIdx.y * 4 + threadIdx.y;
    if (dx >= wo || dy >= ho) return;
    const uint8_t* __restrict__ src = rgb + (size_t)blockIdx.z * hi * wi * 3;
    int v[3];
    if (mode == 0) {
        for (int c = 0; c < 3; ++c) v[c] = src[((size_t)dy * wi + dx) * 3 + c];
    } else if (mode == 1) {
        const uint8_t* p = src + ((size_t)(2 * dy) * wi + 2 * dx) * 3;
        for (int c = 0; c < 3; ++c) v[c] = (p[c] + p[c + 3] + p[(size_t)wi * 3 + c] + p[(size_t)wi * 3 + c + 3] + 2) >> 2;
    } else {
        const LinTap tx = lin_tap(dx, wi, scale_x, true), ty = lin_tap(dy, hi, scale_y, false);
        const int a0 = __float2int_rn((1.f - tx.f) * 2048.f), a1 = __float2int_rn(tx.f * 2048.f);
        const int b0 = __float2int_rn((1.f - ty.f) * 2048.f), b1 = __float2int_rn(ty.f * 2048.f);
        const uint8_t* r0 = src + (size_t)ty.s0 * wi * 3;
        const uint8_t* r1 = src + (size_t)ty.s1 * wi * 3;
        for (int c = 0; c < 3; ++c) {
            const int h0 = r0[tx.s0 * 3 + c] * a0 + r0[tx.s1 * 3 + c] * a1;
            const int h1 = r1[tx.s0 * 3 + c] * a0 + r1[tx.s1 * 3 + c] * a1;
            v[c] = (((b0 * (h0 >> 4)) >> 16) + ((b1 * (h1 >> 4)) >> 16) + 2) >> 2;
        }
    }
    gray[(size_t)blockIdx.z * ho * wo + (size_t)dy * wo + dx] = (uint8_t)((4899 * v[2] + 9617 * v[1] + 1868 * v[0] + 8192) >> 14);
}

// ---- level image, row pass: tmp[y][x] = sum_t taps[t] * frame[y][reflect101(x + t - r)], a 256-column LDS segment per block ----
__global__ __launch_bounds__(256) void fb_blur_rows_kernel(const uint8_t* __restrict__ gray, int h, int w, int ks, FbTaps taps,
                                                           float* __restrict__ tmp) {
    extern __shared__ float seg[];                                  // 256 + ks - 1 floats
    const int r = ks / 2, x0 = blockIdx.x * 256, y = blockIdx.y;
    const uint8_t* __restrict__ row = gray + (size_t)y * w;
    for (int i = threadIdx.x; i < 256 + ks - 1; i += 256) seg[i] = (float)row[reflect101(x0 - r + i, w)];
    __syncthreads();
    const int x = x0 + threadIdx.x;
    if (x >= w) return;
    float s = 0.f;
    for (int t = 0; t < ks; ++t) s += taps.t[t] * seg[threadIdx.x + t];
    tmp[(size_t)y * w + x] = s;
}

// ---- level image, column pass fused with the float resize: every source sample the resize reads is blurred down its column ------
__device__ __forceinline__ float col_blur(const float* __restrict__ tmp, int h, int w, int ks, const FbTaps& taps, int y, int x) {
    const int r = ks / 2;
    float s = 0.f;
    for (int t = 0; t < ks; ++t) s += taps.t[t] * tmp[(size_t)reflect101(y - r + t, h) * w + x];
    return s;
}

__global__ __launch_bounds__(256) void fb_level_image_kernel(const float* __restrict__ tmp, int h, int w, int ks, FbTaps taps,
                                                             float* __restrict__ img, int lh, int lw, int mode, double scale_x,
                                                             double scale_y) {
    const int dx = blockIdx.x * 64 + threadIdx.x, dy = blockIdx.y * 4 + threadIdx.y;
    if (dx >= lw || dy >= lh) return;
    auto at = [&](int yy, int xx) { return col_blur(tmp, h, w, ks, taps, yy, xx); };
    img[(size_t)dy * lw + dx] = resample(at, h, w, dx, dy, mode, scale_x, scale_y);
}

// ---- polynomial expansion of one level: a 64 x 8 output tile, its (8 + 2n) x (64 + 2n) source window in LDS ---------------------
constexpr int PE_TX = 64, PE_TY = 8, PE_W = PE_TX + 2 * FB_MAX_POLY_N, PE_H = PE_TY + 2 * FB_MAX_POLY_N;
__global__ __launch_bounds__(256) void fb_polyexp_kernel(const float* __restrict__ img, int h, int w, int n, FbPoly P,
                                                         float* __restrict__ R) {
    __shared__ float src[PE_H][PE_W];
    __shared__ float vr[PE_TY][PE_W][3];
    const int x0 = blockIdx.x * PE_TX, y0 = blockIdx.y * PE_TY, tid = threadIdx.y * 64 + threadIdx.x;
    const int sw = PE_TX + 2 * n, sh = PE_TY + 2 * n;
    for (int i = tid; i < sw * sh; i += 256) {
        const int ly = i / sw, lx = i % sw;
        src[ly][lx] = img[(size_t)clampi(y0 - n + ly, 0, h - 1) * w + clampi(x0 - n + lx, 0, w - 1)];
    }
    __syncthreads();
    // vertical part: row[0] = sum g (s0 + s1), row[1] = sum xg (s1 - s0), row[2] = sum xxg (s0 + s1), float, OpenCV's order
    for (int i = tid; i < PE_TY * sw; i += 256) {
        const int ly = i / sw, lx = i % sw, cy = ly + n;
        float t0 = src[cy][lx] * P.g[0], t1 = 0.f, t2 = 0.f;
        for (int k = 1; k <= n; ++k) {
            const float s0 = src[cy - k][lx], s1 = src[cy + k][lx], p = s0 + s1;
            t0 = t0 + P.g[k] * p;
            t1 = t1 + P.xg[k] * (s1 - s0);
            t2 = t2 + P.xxg[k] * p;
        }
        vr[ly][lx][0] = t0;
        vr[ly][lx][1] = t1;
        vr[ly][lx][2] = t2;
    }
    __syncthreads();
    const int x = x0 + threadIdx.x;
    if (x >= w) return;
    const int cx = threadIdx.x + n;
    for (int j = 0; j < PE_TY / 4; ++j) {
        const int ly = threadIdx.y + 4 * j, y = y0 + ly;
        if (y >= h) break;
        const float g0 = P.g[0];
        double b1 = vr[ly][cx][0] * g0, b2 = 0, b3 = vr[ly][cx][1] * g0, b4 = 0, b5 = vr[ly][cx][2] * g0, b6 = 0;
        for (int k = 1; k <= n; ++k) {
            const float* a = vr[ly][cx + k];
            const float* b = vr[ly][cx - k];
            const double tg = (double)(a[0] + b[0]);
            b1 += tg * P.g[k];
            b4 += tg * P.xxg[k];
            b2 += (double)((a[0] - b[0]) * P.xg[k]);
            b3 += (double)((a[1] + b[1]) * P.g[k]);
            b6 += (double)((a[1] - b[1]) * P.xg[k]);
            b5 += (double)((a[2] + b[2]) * P.g[k]);
        }
        float* o = R + ((size_t)y * w + x) * 5;
        o[0] = (float)(b3 * P.ig11);
        o[1] = (float)(b2 * P.ig11);
        o[2] = (float)(b1 * P.ig03 + b5 * P.ig33);
        o[3] = (float)(b1 * P.ig03 + b4 * P.ig33);
        o[4] = (float)(b6 * P.ig55);
    }
}

// ---- FarnebackUpdateMatrices at one pixel ------------------------------------------------------------------------------------
__device__ __forceinline__ void update_matrix(const float* __restrict__ R0, const float* __restrict__ R1, int w, int h, int x, int y,
                                              float dx, float dy, float* __restrict__ M) {
    const float border[5] = {0.14f, 0.14f, 0.4472f, 0.4472f, 0.4472f};
    float fx = (float)x + dx, fy = (float)y + dy;
    const int x1 = (int)floorf(fx), y1 = (int)floorf(fy);
    fx -= (float)x1;
    fy -= (float)y1;
    const float* r0 = R0 + ((size_t)y * w + x) * 5;
    float r2, r3, r4, r5, r6;
    if ((unsigned)x1 < (unsigned)(w - 1) && (unsigned)y1 < (unsigned)(h - 1)) {
        const float a00 = (1.f - fx) * (1.f - fy), a01 = fx * (1.f - fy), a10 = (1.f - fx) * fy, a11 = fx * fy;
        const float* p = R1 + ((size_t)y1 * w + x1) * 5;
        const float* q = p + (size_t)w * 5;
        float v[5];
#pragma unroll
        for (int c = 0; c < 5; ++c) v[c] = a00 * p[c] + a01 * p[c + 5] + a10 * q[c] + a11 * q[c + 5];
        r2 = v[0];
        r3 = v[1];
        r4 = (r0[2] + v[2]) * 0.5f;
        r5 = (r0[3] + v[3]) * 0.5f;
        r6 = (r0[4] + v[4]) * 0.25f;
    } else {
        r2 = r3 = 0.f;
        r4 = r0[2];
        r5 = r0[3];
        r6 = r0[4] * 0.5f;
    }
    r2 = (r0[0] - r2) * 0.5f;
    r3 = (r0[1] - r3) * 0.5f;
    r2 += r4 * dy + r6 * dx;
    r3 += r6 * dy + r5 * dx;
    if ((unsigned)(x - 5) >= (unsigned)(w - 10) || (unsigned)(y - 5) >= (unsigned)(h - 10)) {
        const float scale = (x < 5 ? border[x] : 1.f) * (x >= w - 5 ? border[w - x - 1] : 1.f) * (y < 5 ? border[y] : 1.f) *
                            (y >= h - 5 ? border[h - y - 1] : 1.f);
        r2 *= scale; r3 *= scale; r4 *= scale; r5 *= scale; r6 *= scale;
    }
    float* m = M + ((size_t)y * w + x) * 5;
    m[0] = r4 * r4 + r6 * r6;
    m[1] = (r4 + r5) * r6;
    m[2] = r5 * r5 + r6 * r6;
    m[3] = r4 * r2 + r6 * r3;
    m[4] = r6 * r2 + r5 * r3;
}

// ---- a level's first matrix update, fused with the upscale of the coarser level's flow (planar [2][ph][pw]; nullptr: zero flow) --
__global__ __launch_bounds__(256) void fb_update_kernel(const float* __restrict__ R0, const float* __restrict__ R1, int w, int h,
                                                        const float* __restrict__ pflow, int ph, int pw, int mode, double scale_x,
                                                        double scale_y, float inv_pyr, float* __restrict__ M) {
    const int x = blockIdx.x * 64 + threadIdx.x, y = blockIdx.y * 4 + threadIdx.y;
    if (x >= w || y >= h) return;
    float fl[2] = {0.f, 0.f};
    if (pflow) {
        const size_t plane = (size_t)ph * pw;
        if (mode == 0) {
            fl[0] = pflow[(size_t)y * pw + x];
            fl[1] = pflow[plane + (size_t)y * pw + x];
        } else {                          // the finer level is never an exact 2x SHRINK of the coarser one: linear
            // cv_resize.h's linear arm with the taps shared by both components, written out
            const LinTap tx = lin_tap(x, pw, scale_x, true), ty = lin_tap(y, ph, scale_y, false);
            const float a0 = 1.f - tx.f, a1 = tx.f, b0 = 1.f - ty.f, b1 = ty.f;
#pragma unroll
            for (int c = 0; c < 2; ++c) {
                const float* f = pflow + c * plane;
                const float h0 = f[(size_t)ty.s0 * pw + tx.s0] * a0 + f[(size_t)ty.s0 * pw + tx.s1] * a1;
                const float h1 = f[(size_t)ty.s1 * pw + tx.s0] * a0 + f[(size_t)ty.s1 * pw + tx.s1] * a1;
                fl[c] = h0 * b0 + h1 * b1;
            }
        }
        fl[0] *= inv_pyr;
        fl[1] *= inv_pyr;
    }
    update_matrix(R0, R1, w, h, x, y, fl[0], fl[1], M);
}

// ---- one iteration: box mean of M (double), 2x2 solve, flow out, and (M_out != nullptr) the matrix update from the new flow ---------
// A 64 x 8 output tile; LDS holds the vertical window sums of its (64 + 2m) columns for its 8 rows in double.
constexpr int IT_TX = 64, IT_TY = 8;
__global__ __launch_bounds__(256) void fb_iter_kernel(const float* __restrict__ Min, int w, int h, int m, double scale,
                                                      const float* __restrict__ R0, const float* __restrict__ R1,
                                                      float* __restrict__ flow, float* __restrict__ Mout) {
    extern __shared__ double vs[];                                  // [IT_TY][IT_TX + 2m][5]
    const int x0 = blockIdx.x * IT_TX, y0 = blockIdx.y * IT_TY, tid = threadIdx.y * 64 + threadIdx.x;
    const int cols = IT_TX + 2 * m;
    for (int i = tid; i < cols * 5; i += 256) {
        const int lc = i / 5, ch = i % 5;
        const float* col = Min + (size_t)clampi(x0 - m + lc, 0, w - 1) * 5 + ch;
        const size_t rs = (size_t)w * 5;
        double s = 0;
        for (int k = -m; k <= m; ++k) s += col[clampi(y0 + k, 0, h - 1) * rs];
        vs[(0 * cols + lc) * 5 + ch] = s;
        for (int r = 1; r < IT_TY; ++r) {
            s += (double)col[clampi(y0 + r + m, 0, h - 1) * rs] - (double)col[clampi(y0 + r - m - 1, 0, h - 1) * rs];
            vs[(r * cols + lc) * 5 + ch] = s;
        }
    }
    __syncthreads();
    const int x = x0 + threadIdx.x;
    if (x >= w) return;
    for (int j = 0; j < IT_TY / 4; ++j) {
        const int ly = threadIdx.y + 4 * j, y = y0 + ly;
        if (y >= h) break;
        const double* v = vs + ((size_t)ly * cols + threadIdx.x) * 5;
        double g11 = 0, g12 = 0, g22 = 0, h1 = 0, h2 = 0;
        for (int k = 0; k <= 2 * m; ++k) {
            g11 += v[k * 5];
            g12 += v[k * 5 + 1];
            g22 += v[k * 5 + 2];
            h1 += v[k * 5 + 3];
            h2 += v[k * 5 + 4];
        }
        g11 *= scale; g12 *= scale; g22 *= scale; h1 *= scale; h2 *= scale;
        const double idet = 1. / (g11 * g22 - g12 * g12 + 1e-3);
        const float fx = (float)((g11 * h2 - g12 * h1) * idet), fy = (float)((g22 * h1 - g12 * h2) * idet);
        flow[(size_t)y * w + x] = fx;
        flow[(size_t)h * w + (size_t)y * w + x] = fy;
        if (Mout) update_matrix(R0, R1, w, h, x, y, fx, fy, Mout);
    }
}

// ---- launchers -------------------------------------------------------------------------------------------------------------------
static bool fb_check_frame(int h, int w, const char* what) {
    if (h < 1 || w < 1 || h > 65535 || (size_t)h * w * 5 >= 0x7fffffffULL) {
        set_error("%s: bad frame size %d x %d", what, w, h);
        return false;
    }
    return true;
}

int launch_flow_gray_u8(const uint8_t* rgb, int n, int hi, int wi, uint8_t* gray, int ho, int wo, hipStream_t s) {
    if (n < 1 || n > 65535 || !fb_check_frame(hi, wi, "flow_gray_u8") || !fb_check_frame(ho, wo, "flow_gray_u8")) {
        if (n < 1 || n > 65535) set_error("flow_gray_u8: bad frame count %d", n);
        return ADAIN_EINVAL;
    }
    const double sx = 1. / ((double)wo / wi), sy = 1. / ((double)ho / hi);
    const int mode = resize_mode(hi, wi, ho, wo, sx, sy);
    hipLaunchKernelGGL(fb_gray_kernel, dim3((wo + 63) / 64, (ho + 3) / 4, n), dim3(64, 4), 0, s, rgb, hi, wi, gray, ho, wo, mode, sx, sy);
    return check_launch("flow_gray_u8");
}

int farneback_levels(int h, int w, double pyr_scale, int levels, int* out_levels, int* sizes_wh, int* ksizes, double* sigmas) {
    FbLevel L[FB_MAX_LEVELS];
    const int k = fb_schedule(h, w, pyr_scale, levels, L, nullptr);
    if (k < 0) {
        set_error("farneback_levels: need h, w >= 1, 0 < pyr_scale < 1, levels >= 0 and at most %d pyramid levels", FB_MAX_LEVELS);
        return ADAIN_EINVAL;
    }
    if (out_levels) *out_levels = k;
    for (int i = 0; i <= k; ++i) {
        if (sizes_wh) { sizes_wh[2 * i] = L[i].w; sizes_wh[2 * i + 1] = L[i].h; }
        if (ksizes) ksizes[i] = L[i].ksize;
        if (sigmas) sigmas[i] = L[i].sigma;
    }
    return 0;
}

size_t farneback_pyramid_bytes(int h, int w, double pyr_scale, int levels) {
    FbLevel L[FB_MAX_LEVELS];
    size_t floats = 0;
    return fb_schedule(h, w, pyr_scale, levels, L, &floats) < 0 ? 0 : floats * sizeof(float);
}

// The one workspace of both calls (offsets in bytes), in planes of a full-size frame rounded up to 256 bytes.  The flow call: the
// ping-pong matrices M (5 planes each) and the two level flows F (2 planes each).  The expand call: its row pass's buffer (1 plane),
// which is the front of M[0].
struct FbLayout { size_t o_M[2], o_F[2], o_rows, total; };
static FbLayout fb_layout(int h, int w) {
    const size_t plane = align256((size_t)h * w * sizeof(float));
    FbLayout l{};
    Carve c;
    for (size_t& o : l.o_M) o = c.take(5 * plane);
    for (size_t& o : l.o_F) o = c.take(2 * plane);
    l.o_rows = l.o_M[0];
    l.total = c.at;
    return l;
}

size_t farneback_workspace_bytes(int h, int w) {
    if (h < 1 || w < 1) return 0;
    return fb_layout(h, w).total;
}

// the checks both calls share; *layout: the workspace they passed
static bool fb_common_checks(int h, int w, double pyr_scale, int levels, const void* ws, size_t ws_bytes, const char* what, FbLayout* layout) {
    if (!fb_check_frame(h, w, what)) return false;
    if (!(pyr_scale > 0.0 && pyr_scale < 1.0)) { set_error("%s: pyr_scale must be in (0, 1), got %g", what, pyr_scale); return false; }
    if (levels < 0) { set_error("%s: levels must be >= 0", what); return false; }
    *layout = fb_layout(h, w);
    return check_workspace(what, ws, ws_bytes, layout->total, 1) == 0;
}

int launch_farneback_expand(const uint8_t* gray, int h, int w, double pyr_scale, int levels, int poly_n, double poly_sigma,
                            float* pyramid, void* ws, size_t ws_bytes, hipStream_t s) {
    FbLayout lay;
    if (!fb_common_checks(h, w, pyr_scale, levels, ws, ws_bytes, "farneback_expand", &lay)) return ADAIN_EINVAL;
    if (poly_n != 5 && poly_n != 7) { set_error("farneback_expand: poly_n must be 5 or 7, got %d", poly_n); return ADAIN_EINVAL; }
    FbLevel L[FB_MAX_LEVELS];
    const int k = fb_schedule(h, w, pyr_scale, levels, L, nullptr);
    if (k < 0) { set_error("farneback_expand: more than %d pyramid levels", FB_MAX_LEVELS); return ADAIN_EINVAL; }
    for (int i = 0; i <= k; ++i)
        if (L[i].ksize >= FB_MAX_TAPS) {
            set_error("farneback_expand: level %d needs %d Gaussian taps, at most %d are supported", i, L[i].ksize, FB_MAX_TAPS - 1);
            return ADAIN_EINVAL;
        }
    FbPoly P;
    fb_poly_coeffs(poly_n, poly_sigma, P);
    float* tmp = (float*)((char*)ws + lay.o_rows);
    FbTaps T;                                 // 2 KB: passed by value into the launches below
    for (int i = 0; i <= k; ++i) {
        const FbLevel& l = L[i];
        fb_gauss_taps(l.ksize, l.sigma, T);
        hipLaunchKernelGGL(fb_blur_rows_kernel, dim3((w + 255) / 256, h), dim3(256), (256 + l.ksize - 1) * sizeof(float), s, gray, h, w,
                           l.ksize, T, tmp);
        const double sx = 1. / ((double)l.w / w), sy = 1. / ((double)l.h / h);
        const int mode = resize_mode(h, w, l.h, l.w, sx, sy);
        float* img = pyramid + l.img_off;
        hipLaunchKernelGGL(fb_level_image_kernel, dim3((l.w + 63) / 64, (l.h + 3) / 4), dim3(64, 4), 0, s, tmp, h, w, l.ksize, T, img,
                           l.h, l.w, mode, sx, sy);
        hipLaunchKernelGGL(fb_polyexp_kernel, dim3((l.w + PE_TX - 1) / PE_TX, (l.h + PE_TY - 1) / PE_TY), dim3(64, 4), 0, s, img, l.h,
                           l.w, poly_n, P, pyramid + l.r_off);
        if (int rc = check_launch("farneback_expand")) return rc;
    }
    return 0;
}

int launch_farneback_flow(const float* pyr_prev, const float* pyr_next, int h, int w, double pyr_scale, int levels, int winsize,
                          int iterations, int flags, float* flow_out, void* ws, size_t ws_bytes, hipStream_t s) {
    FbLayout lay;
    if (!fb_common_checks(h, w, pyr_scale, levels, ws, ws_bytes, "farneback_flow", &lay)) return ADAIN_EINVAL;
    if (flags != 0) {
        set_error("farneback_flow: only flags = 0 is supported (no OPTFLOW_USE_INITIAL_FLOW, no OPTFLOW_FARNEBACK_GAUSSIAN), got %d", flags);
        return ADAIN_EINVAL;
    }
    if (winsize < 2 || winsize / 2 > FB_MAX_HALF_WIN) {
        set_error("farneback_flow: winsize must be in [2, %d], got %d", 2 * FB_MAX_HALF_WIN + 1, winsize);
        return ADAIN_EINVAL;
    }
    if (iterations < 1) { set_error("farneback_flow: iterations must be >= 1, got %d", iterations); return ADAIN_EINVAL; }
    FbLevel L[FB_MAX_LEVELS];
    const int k = fb_schedule(h, w, pyr_scale, levels, L, nullptr);
    if (k < 0) { set_error("farneback_flow: more than %d pyramid levels", FB_MAX_LEVELS); return ADAIN_EINVAL; }
    char* base = (char*)ws;
    float* Mb[2] = {(float*)(base + lay.o_M[0]), (float*)(base + lay.o_M[1])};
    float* Fb[2] = {(float*)(base + lay.o_F[0]), (float*)(base + lay.o_F[1])};
    const int m = winsize / 2;
    const double bscale = 1. / ((double)winsize * winsize);
    const size_t lds = (size_t)IT_TY * (IT_TX + 2 * m) * 5 * sizeof(double);
    const float inv_pyr = (float)(1. / pyr_scale);
    const float* prev_flow = nullptr;
    int pw = 0, ph = 0;
    for (int i = k; i >= 0; --i) {
        const FbLevel& l = L[i];
        const float* R0 = pyr_prev + l.r_off;
        const float* R1 = pyr_next + l.r_off;
        float* fl = i == 0 ? flow_out : Fb[i & 1];
        const double sx = prev_flow ? 1. / ((double)l.w / pw) : 0, sy = prev_flow ? 1. / ((double)l.h / ph) : 0;
        const int mode = prev_flow ? resize_mode(ph, pw, l.h, l.w, sx, sy) : 0;
        hipLaunchKernelGGL(fb_update_kernel, dim3((l.w + 63) / 64, (l.h + 3) / 4), dim3(64, 4), 0, s, R0, R1, l.w, l.h, prev_flow, ph, pw,
                           mode, sx, sy, inv_pyr, Mb[0]);
        for (int it = 0; it < iterations; ++it) {
            const bool last = it == iterations - 1;
            hipLaunchKernelGGL(fb_iter_kernel, dim3((l.w + IT_TX - 1) / IT_TX, (l.h + IT_TY - 1) / IT_TY), dim3(64, 4), lds, s,
                               Mb[it & 1], l.w, l.h, m, bscale, R0, R1, fl, last ? nullptr : Mb[(it + 1) & 1]);
        }
        if (int rc = check_launch("farneback_flow")) return rc;
        prev_flow = fl;
        pw = l.w;
        ph = l.h;
    }
    return 0;
}

}  // namespace adain
