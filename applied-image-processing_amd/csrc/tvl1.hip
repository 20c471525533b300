// Dense optical flow: OpenCV 4.x's contrib DualTVL1OpticalFlow (optflow module, CPU path; Zach, Pock, Bischof 2007 / Sanchez,
// Meinhardt-Llopis, Facciolo 2013), the reference's second flow method (video/utils.py:75-86: cv2.optflow.DualTVL1OpticalFlow_create()
// .calc(prev, next, None) with the default parameters; the method its own driver picks, video/utils.py:416).
//
// Rules (restated from OpenCV's published tvl1flow.cpp / resize.cpp / imgwarp.cpp / median_blur.simd.hpp; parity with cv2 itself is
// not pinned on any machine of this project - tests/tvl1_ref.py restates the same rules in NumPy and is the yardstick; the uncertain
// readings are listed in DESIGN.md section 8, item 11):
//   params    tau 0.25, lambda 0.15, theta 0.3, nscales 5, warps 5, epsilon 0.01, innerIterations 30, outerIterations 10, scaleStep
//             0.8, gamma 0, medianFiltering 5, useInitialFlow false.  Refused: gamma != 0, useInitialFlow, medianFiltering other than
//             <= 1 (off), 3 or 5 (medianBlur on float data), nscales < 1, negative warps / iterations, scaleStep outside (0, 1].
//   input     uint8 gray [H][W] -> float32, values 0..255 (convertTo with scale 1).
//   scales    level s = resize(level s-1, Size(), scaleStep, scaleStep, INTER_LINEAR): size cvRound(w*scaleStep) x cvRound(h*scaleStep)
//             (half to even), source coordinates with scale 1/scaleStep (not the size ratio); the float INTER_LINEAR of cv_resize.h
//             (an equal size is a copy, an exact 2x shrink INTER_AREA's 2x2 mean over the source pixels inside the image).  The
//             first level with fewer than 16 columns or rows ends the list (discarded).
//   gradient  I1x, I1y = centred differences 0.5f*(next - previous), one-sided 0.5f*(x1 - x0) on the first / last row and column.
//   per scale coarsest: u = 0; finer: u = resize(u_coarser, this size, INTER_LINEAR with the size ratio) * (float)(1/scaleStep);
//             p11 = p12 = p21 = p22 = 0; scaledEpsilon = (float)(epsilon^2 * w*h); l_t = (float)(lambda*theta); taut = (float)(tau/theta).
//   per warp  map = (x + u1, y + u2); I1w, I1wx, I1wy = remap(I1 | I1x | I1y, map, INTER_CUBIC, BORDER_CONSTANT 0): X = cvRound(mx*32),
//             window from (X>>5) - 1, 4x4 taps tab[Y&31][k1] * tab[X&31][k2] of interpolateCubic (A = -0.75) at i/32 (float); a window
//             inside the image sums row by row (S0 w0 + S1 w1 + S2 w2 + S3 w3 per row), one touching the border adds the taps inside
//             one by one (the others contribute 0), one wholly outside is 0.  grad = I1wx^2 + I1wy^2, rho_c = I1w - I1wx u1 - I1wy u2 - I0.
//   loops     error = FLT_MAX; for (outer < outerIterations && error > scaledEpsilon) { medianBlur(u1, u2, medianFiltering) if > 1
//             (BORDER_REPLICATE); for (inner < innerIterations && error > scaledEpsilon) one inner step }.
//   step      rho = rho_c + (I1wx u1 + I1wy u2); v = u + l_t I1w* if rho < -l_t grad, u - l_t I1w* if rho > l_t grad, else u + fi I1w*
//             with fi = -rho/grad when grad > FLT_EPSILON (else u);  div p: backward differences, row 0 / column 0 take the value itself
//             ((p1[x] - p1[x-1]) + (p2[y] - p2[y-1]); row 0: (p1[x] - p1[x-1]) + p2; column 0: (p1 + p2) - p2[y-1]; corner p1 + p2);
//             u = v + theta div; error = sum (du1^2 + du2^2); forward gradient of u (0 in the last column for d/dx, in the last row for
//             d/dy); ng = 1 + taut hypot(ux, uy); p = (p + taut grad u) / ng.
//   output    (u1, u2) at scale 0 = the flow, x then y.
// The device keeps OpenCV's float operations one by one (this file is compiled with -ffp-contract=off); hypot is computed in double
// and rounded once.  The stop rule's error is summed in DOUBLE in a fixed order (per thread, then a fixed tree per tile, then the tile
// partials in index order by whichever tile of the pair arrives last): OpenCV's float sum in thread order is not reproducible, this
// one makes a pair's result independent of batch size, position and run.
//
// Kernels: a frame's scale images and gradients depend on the frame only (adain_tvl1_prepare, once per frame of a clip).  The flow of
// a batch of pairs (adain_tvl1_flow) runs, per scale, one init launch (upscale + dual reset), per warp one remap launch and per outer
// pass one median launch and `innerIterations` fused step launches, then one store launch; every launch spans all pairs (blockIdx.z).
// Each pair carries its own stop state (done flag, buffer parities, arrival counter): a step's last-arriving tile reduces the pair's
// error partials, counts the step and sets the flag; later launches of that warp skip a flagged pair.  After each outer pass the host
// reads how many pairs are done and skips the rest of the warp when all are.
#include "common.h"
#include "cv_resize.h"

#include <float.h>
#include <math.h>

namespace adain {

constexpr int TV_MAX_SCALES = 64;
constexpr int TV_MIN_SIZE = 16;

struct TvScale { int w, h; size_t off; };   // off: floats into a prepared frame, float4 (img, I_x, I_y, 0) per pixel

// the scale list; returns the effective count or ADAIN_EINVAL (< 0: too many scales).  The single source of a prepared frame's layout: every scale's
// block starts on a multiple of 256 bytes.
static int tv_schedule(int h, int w, int nscales, double step, TvScale* S, size_t* frame_floats) {
    int n = 1;
    S[0].w = w;
    S[0].h = h;
    for (int s = 1; s < nscales; ++s) {
        const int nw = (int)nearbyint(S[s - 1].w * step), nh = (int)nearbyint(S[s - 1].h * step);
        if (nw < TV_MIN_SIZE || nh < TV_MIN_SIZE) break;
        if (n == TV_MAX_SCALES) return ADAIN_EINVAL;
        S[s].w = nw;
        S[s].h = nh;
        n = s + 1;
    }
    Carve c;
    for (int s = 0; s < n; ++s) S[s].off = c.take((size_t)S[s].w * S[s].h * 4 * sizeof(float)) / sizeof(float);
    if (frame_floats) *frame_floats = c.at / sizeof(float);
    return n;
}

static bool tv_check(const adain_tvl1_params* p, int h, int w, const char* what) {
    if (!p) { set_error("%s: null parameters", what); return false; }
    if (p->gamma != 0.0) { set_error("%s: gamma != 0 is not supported (got %g)", what, p->gamma); return false; }
    if (p->useInitialFlow != 0) { set_error("%s: useInitialFlow is not supported", what); return false; }
    if (p->medianFiltering > 1 && p->medianFiltering != 3 && p->medianFiltering != 5) {
        set_error("%s: medianFiltering must be <= 1 (off), 3 or 5, got %d", what, p->medianFiltering);
        return false;
    }
    if (p->nscales < 1) { set_error("%s: nscales must be >= 1, got %d", what, p->nscales); return false; }
    if (p->warps < 0 || p->innerIterations < 0 || p->outerIterations < 0) {
        set_error("%s: warps, innerIterations and outerIterations must be >= 0", what);
        return false;
    }
    if (!(p->scaleStep > 0.0 && p->scaleStep <= 1.0)) { set_error("%s: scaleStep must be in (0, 1], got %g", what, p->scaleStep); return false; }
    if (h < 3 || w < 3 || h > 65535 || w > 65535 || (size_t)h * w * 4 >= 0x7fffffffULL) {
        set_error("%s: bad frame size %d x %d", what, w, h);
        return false;
    }
    TvScale S[TV_MAX_SCALES];
    if (tv_schedule(h, w, p->nscales, p->scaleStep, S, nullptr) < 0) {
        set_error("%s: more than %d scales", what, TV_MAX_SCALES);
        return false;
    }
    return true;
}

// ---- frame preparation ---------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void tv_to_float_kernel(const uint8_t* __restrict__ gray, int h, int w, float* __restrict__ prep,
                                                          size_t frame_floats) {
    const int x = blockIdx.x * 64 + threadIdx.x, y = blockIdx.y * 4 + threadIdx.y;
    if (x >= w || y >= h) return;
    prep[(size_t)blockIdx.z * frame_floats + ((size_t)y * w + x) * 4] = (float)gray[(size_t)blockIdx.z * h * w + (size_t)y * w + x];
}

__global__ __launch_bounds__(256) void tv_scale_kernel(float* __restrict__ prep, size_t frame_floats, size_t src_off, int sh, int sw,
                                                       size_t dst_off, int dh, int dw, int mode, double sx, double sy) {
    const int x = blockIdx.x * 64 + threadIdx.x, y = blockIdx.y * 4 + threadIdx.y;
    if (x >= dw || y >= dh) return;
    float* f = prep + (size_t)blockIdx.z * frame_floats;
    const float* src = f + src_off;
    auto at = [&](int yy, int xx) { return src[((size_t)yy * sw + xx) * 4]; };
    f[dst_off + ((size_t)y * dw + x) * 4] = resample(at, sh, sw, x, y, mode, sx, sy);
}

__global__ __launch_bounds__(256) void tv_gradient_kernel(float* __restrict__ prep, size_t frame_floats, size_t off, int h, int w) {
    const int x = blockIdx.x * 64 + threadIdx.x, y = blockIdx.y * 4 + threadIdx.y;
    if (x >= w || y >= h) return;
    float* f = prep + (size_t)blockIdx.z * frame_floats + off;
    auto at = [&](int yy, int xx) { return f[((size_t)yy * w + xx) * 4]; };
    const float gx = 0.5f * (at(y, min(x + 1, w - 1)) - at(y, max(x - 1, 0)));
    const float gy = 0.5f * (at(min(y + 1, h - 1), x) - at(max(y - 1, 0), x));
    f[((size_t)y * w + x) * 4 + 1] = gx;
    f[((size_t)y * w + x) * 4 + 2] = gy;
    f[((size_t)y * w + x) * 4 + 3] = 0.f;
}

// ---- the flow of a batch of pairs ----------------------------------------------------------------------------------------------
// Per pair: U[2] float2 (u1, u2) and P[2] float4 (p11, p12, p21, p22) ping-pong buffers, C float4 (I1wx, I1wy, grad, rho_c), all at
// the full frame size; the pair's state words; its error partials.
struct TvPair {                   // the buffers of one pair; the ping-pong slot is computed, never an indexed array (no private copy)
    float* b;
    size_t plane;
    __device__ float2* U(int par) const { return (float2*)(b + (size_t)par * 2 * plane); }
    __device__ float4* P(int par) const { return (float4*)(b + (4 + (size_t)par * 4) * plane); }
    __device__ float4* C() const { return (float4*)(b + 12 * plane); }
};
struct TvState { int done, upar, ppar, cnt; };       // per pair; zeroed per call, the parities and the counter reset per scale

struct TvArgs {
    const float* const* prev;    // [npairs] prepared I0 frames
    const float* const* next;    // [npairs] prepared I1 frames
    size_t scale_off;            // this scale's offset in a prepared frame
    int h, w;                    // this scale's size
    int npairs;
    float* ws_pairs;             // per-pair buffers, pair_floats apart
    size_t pair_floats, plane;   // plane: floats per pixel-plane at full size (aligned)
    TvState* state;
    int* ndone;
    double* partials;            // [npairs][nblk]
    int nblk;
    int* iters;                  // [npairs][nscales][warps] or nullptr
    int iter_idx, iters_stride;  // this (scale, warp)'s index, the per-pair stride
    float l_t, theta, taut;
    double eps;
};

__device__ __forceinline__ TvPair tv_pair(const TvArgs& a, int p) {
    TvPair r;
    r.b = a.ws_pairs + (size_t)p * a.pair_floats;
    r.plane = a.plane;
    return r;
}

__device__ __forceinline__ int tv_load_state(const int* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
__device__ __forceinline__ void tv_store_state(int* p, int v) { __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

// the start of a scale: u from the coarser scale's flow (planar [2][ch][cw] in the pair's output slot; cw == 0: zero), p = 0
__global__ __launch_bounds__(256) void tv_init_kernel(TvArgs a, const float* __restrict__ coarse, size_t out_stride, int ch, int cw,
                                                      int mode, double sx, double sy, float inv_step) {
    const int x = blockIdx.x * 64 + threadIdx.x, y = blockIdx.y * 4 + threadIdx.y, p = blockIdx.z;
    if (blockIdx.x == 0 && blockIdx.y == 0 && threadIdx.x == 0 && threadIdx.y == 0) {
        TvState* st = a.state + p;
        tv_store_state(&st->done, 0);
        tv_store_state(&st->upar, 0);
        tv_store_state(&st->ppar, 0);
        tv_store_state(&st->cnt, 0);
    }
    if (x >= a.w || y >= a.h) return;
    const TvPair b = tv_pair(a, p);
    float2 u = make_float2(0.f, 0.f);
    if (cw > 0) {
        const float* c0 = coarse + (size_t)p * out_stride;
        const float* c1 = c0 + (size_t)ch * cw;
        auto at0 = [&](int yy, int xx) { return c0[(size_t)yy * cw + xx]; };
        auto at1 = [&](int yy, int xx) { return c1[(size_t)yy * cw + xx]; };
        u.x = resample(at0, ch, cw, x, y, mode, sx, sy) * inv_step;
        u.y = resample(at1, ch, cw, x, y, mode, sx, sy) * inv_step;
    }
    const size_t i = (size_t)y * a.w + x;
    b.U(0)[i] = u;
    b.P(0)[i] = make_float4(0.f, 0.f, 0.f, 0.f);
}

struct TvCubic { float t[32][4]; };   // interpolateCubic(i / 32) for i = 0..31

// INTER_CUBIC remap of one plane (component c of the float4 prepared scale) at the precomputed window
__device__ __forceinline__ float tv_cubic(const float4* __restrict__ src, int c, int h, int w, int sx, int sy, const float* wy,
                                          const float* wx) {
    auto S = [&](int yy, int xx) {
        const float4 v = src[(size_t)yy * w + xx];
        return c == 0 ? v.x : (c == 1 ? v.y : v.z);
    };
    if ((unsigned)sx < (unsigned)max(w - 3, 0) && (unsigned)sy < (unsigned)max(h - 3, 0)) {
        float sum = S(sy, sx) * (wy[0] * wx[0]) + S(sy, sx + 1) * (wy[0] * wx[1]) + S(sy, sx + 2) * (wy[0] * wx[2]) +
                    S(sy, sx + 3) * (wy[0] * wx[3]);
#pragma unroll
        for (int r = 1; r < 4; ++r)
            sum += S(sy + r, sx) * (wy[r] * wx[0]) + S(sy + r, sx + 1) * (wy[r] * wx[1]) + S(sy + r, sx + 2) * (wy[r] * wx[2]) +
                   S(sy + r, sx + 3) * (wy[r] * wx[3]);
        return sum;
    }
    if (sx >= w || sx + 4 <= 0 || sy >= h || sy + 4 <= 0) return 0.f;
    float sum = 0.f;
    for (int r = 0; r < 4; ++r) {
        const int yy = sy + r;
        if (yy < 0 || yy >= h) continue;
        for (int k = 0; k < 4; ++k) {
            const int xx = sx + k;
            if (xx >= 0 && xx < w) sum += S(yy, xx) * (wy[r] * wx[k]);
        }
    }
    return sum;
}

// saturate_cast<int>(float): cvRound, out-of-range and NaN give INT_MIN (x86's conversion)
__device__ __forceinline__ int tv_round_sat(float v) {
    return (v == v && fabsf(v) < 2147483648.f) ? __float2int_rn(v) : INT_MIN;
}
__device__ __forceinline__ int tv_short(int v) { return v < -32768 ? -32768 : (v > 32767 ? 32767 : v); }

// a warp: remap of I1, I1x, I1y at x + u, then grad and rho_c; resets the pair's stop flag and this warp's step count
__global__ __launch_bounds__(256) void tv_warp_kernel(TvArgs a, TvCubic tab) {
    const int x = blockIdx.x * 64 + threadIdx.x, y = blockIdx.y * 4 + threadIdx.y, p = blockIdx.z;
    if (blockIdx.x == 0 && blockIdx.y == 0 && threadIdx.x == 0 && threadIdx.y == 0) {
        tv_store_state(&a.state[p].done, 0);
        if (p == 0) tv_store_state(a.ndone, 0);
        if (a.iters) a.iters[(size_t)p * a.iters_stride + a.iter_idx] = 0;
    }
    if (x >= a.w || y >= a.h) return;
    const TvPair b = tv_pair(a, p);
    const int upar = tv_load_state(&a.state[p].upar);
    const size_t i = (size_t)y * a.w + x;
    const float2 u = b.U(upar)[i];
    const float4* I0 = (const float4*)(a.prev[p] + a.scale_off);
    const float4* I1 = (const float4*)(a.next[p] + a.scale_off);
    const float mx = (float)x + u.x, my = (float)y + u.y;
    const int X = tv_round_sat(mx * 32.f), Y = tv_round_sat(my * 32.f);
    const int sx = tv_short(X >> 5) - 1, sy = tv_short(Y >> 5) - 1;
    const float* wx = tab.t[X & 31];
    const float* wy = tab.t[Y & 31];
    const float w0 = tv_cubic(I1, 0, a.h, a.w, sx, sy, wy, wx);
    const float wgx = tv_cubic(I1, 1, a.h, a.w, sx, sy, wy, wx);
    const float wgy = tv_cubic(I1, 2, a.h, a.w, sx, sy, wy, wx);
    const float grad = wgx * wgx + wgy * wgy;
    const float rho_c = w0 - wgx * u.x - wgy * u.y - I0[i].x;
    b.C()[i] = make_float4(wgx, wgy, grad, rho_c);
}

// the 5x5 / 3x3 replicate median of u1 and u2 (an exact selection: a bitonic sort of 32 with +inf padding)
template <int K>
__device__ __forceinline__ float tv_median(const float2* __restrict__ U, int h, int w, int x, int y, int c) {
    float v[32];
    constexpr int R = K / 2;
#pragma unroll
    for (int dy = 0; dy < K; ++dy)
#pragma unroll
        for (int dx = 0; dx < K; ++dx) {
            const float2 q = U[(size_t)clampi(y + dy - R, 0, h - 1) * w + clampi(x + dx - R, 0, w - 1)];
            v[dy * K + dx] = c == 0 ? q.x : q.y;
        }
#pragma unroll
    for (int i = K * K; i < 32; ++i) v[i] = INFINITY;
#pragma unroll
    for (int k = 2; k <= 32; k <<= 1)
#pragma unroll
        for (int j = k >> 1; j > 0; j >>= 1)
#pragma unroll
            for (int i = 0; i < 32; ++i) {
                const int l = i ^ j;
                if (l > i) {
                    const float lo = fminf(v[i], v[l]), hi = fmaxf(v[i], v[l]);
                    const bool up = (i & k) == 0;
                    v[i] = up ? lo : hi;
                    v[l] = up ? hi : lo;
                }
            }
    return v[K * K / 2];
}

// the last-arriving block of a pair's launch: every block's stores drained and released before its ticket, the last one acquires
__device__ __forceinline__ bool tv_arrive(int* cnt, int nblk, int* flag_lds) {
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    if (threadIdx.x == 0 && threadIdx.y == 0) {
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        const int t = __hip_atomic_fetch_add(cnt, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        const int last = t == nblk - 1;
        if (last) {
            __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        }
        *flag_lds = last;
    }
    __syncthreads();
    return *flag_lds != 0;
}

template <int K>
__global__ __launch_bounds__(256) void tv_median_kernel(TvArgs a) {
    __shared__ int flag;
    const int p = blockIdx.z;
    TvState* st = a.state + p;
    if (tv_load_state(&st->done)) return;
    const int upar = tv_load_state(&st->upar);
    const TvPair b = tv_pair(a, p);
    const int x = blockIdx.x * 64 + threadIdx.x, y = blockIdx.y * 4 + threadIdx.y;
    if (x < a.w && y < a.h) {
        const float m1 = tv_median<K>(b.U(upar), a.h, a.w, x, y, 0), m2 = tv_median<K>(b.U(upar), a.h, a.w, x, y, 1);
        b.U(upar ^ 1)[(size_t)y * a.w + x] = make_float2(m1, m2);
    }
    if (tv_arrive(&st->cnt, gridDim.x * gridDim.y, &flag) && threadIdx.x == 0 && threadIdx.y == 0) {
        tv_store_state(&st->upar, upar ^ 1);
        tv_store_state(&st->cnt, 0);
    }
}

// one inner step on a 64 x 16 tile: u on the tile plus one column right and one row below (old p one further left and up), then p on
// the tile; the tile's error partial in double, the pair's last-arriving tile reduces the partials in index order
constexpr int ST_TX = 64, ST_TY = 16;
constexpr int ST_PW = ST_TX + 2, ST_PH = ST_TY + 2, ST_UW = ST_TX + 1, ST_UH = ST_TY + 1;
struct TvStepLds {
    float4 p[ST_PH][ST_PW];          // old p at (x0 - 1 + lx, y0 - 1 + ly)
    float2 u[ST_UH][ST_UW];          // new u at (x0 + lx, y0 + ly)
    double red[256];
    int flag;
};

__global__ __launch_bounds__(256) void tv_step_kernel(TvArgs a) {
    __shared__ TvStepLds L;
    const int p = blockIdx.z;
    TvState* st = a.state + p;
    if (tv_load_state(&st->done)) return;
    const int upar = tv_load_state(&st->upar), ppar = tv_load_state(&st->ppar);
    const TvPair b = tv_pair(a, p);
    const float2* __restrict__ Uo = b.U(upar);
    const float4* __restrict__ Po = b.P(ppar);
    const int w = a.w, h = a.h, x0 = blockIdx.x * ST_TX, y0 = blockIdx.y * ST_TY, tid = threadIdx.y * 64 + threadIdx.x;
    for (int i = tid; i < ST_PW * ST_PH; i += 256) {
        const int ly = i / ST_PW, lx = i - ly * ST_PW, x = x0 - 1 + lx, y = y0 - 1 + ly;
        L.p[ly][lx] = (x >= 0 && x < w && y >= 0 && y < h) ? Po[(size_t)y * w + x] : make_float4(0.f, 0.f, 0.f, 0.f);
    }
    __syncthreads();
    double err = 0.0;
    for (int i = tid; i < ST_UW * ST_UH; i += 256) {
        const int ly = i / ST_UW, lx = i - ly * ST_UW, x = x0 + lx, y = y0 + ly;
        if (x >= w || y >= h) continue;
        const size_t k = (size_t)y * w + x;
        const float2 u = Uo[k];
        const float4 c = b.C()[k];                     // I1wx, I1wy, grad, rho_c
        const float rho = c.w + (c.x * u.x + c.y * u.y);
        float d1 = 0.f, d2 = 0.f;
        if (rho < -a.l_t * c.z) {
            d1 = a.l_t * c.x;
            d2 = a.l_t * c.y;
        } else if (rho > a.l_t * c.z) {
            d1 = -a.l_t * c.x;
            d2 = -a.l_t * c.y;
        } else if (c.z > FLT_EPSILON) {
            const float fi = -rho / c.z;
            d1 = fi * c.x;
            d2 = fi * c.y;
        }
        const float v1 = u.x + d1, v2 = u.y + d2;
        const float4 q = L.p[ly + 1][lx + 1];
        float div1, div2;
        if (x > 0 && y > 0) {
            const float4 l = L.p[ly + 1][lx], t = L.p[ly][lx + 1];
            div1 = (q.x - l.x) + (q.y - t.y);
            div2 = (q.z - l.z) + (q.w - t.w);
        } else if (x > 0) {
            const float4 l = L.p[ly + 1][lx];
            div1 = (q.x - l.x) + q.y;
            div2 = (q.z - l.z) + q.w;
        } else if (y > 0) {
            const float4 t = L.p[ly][lx + 1];
            div1 = (q.x + q.y) - t.y;
            div2 = (q.z + q.w) - t.w;
        } else {
            div1 = q.x + q.y;
            div2 = q.z + q.w;
        }
        const float n1 = v1 + a.theta * div1, n2 = v2 + a.theta * div2;
        L.u[ly][lx] = make_float2(n1, n2);
        if (lx < ST_TX && ly < ST_TY) {
            const float e1 = n1 - u.x, e2 = n2 - u.y;
            err += (double)(e1 * e1 + e2 * e2);
        }
    }
    L.red[tid] = err;
    __syncthreads();
    float2* __restrict__ Un = b.U(upar ^ 1);
    float4* __restrict__ Pn = b.P(ppar ^ 1);
    for (int i = tid; i < ST_TX * ST_TY; i += 256) {
        const int ly = i / ST_TX, lx = i - ly * ST_TX, x = x0 + lx, y = y0 + ly;
        if (x >= w || y >= h) continue;
        const float2 u = L.u[ly][lx];
        float u1x = 0.f, u2x = 0.f, u1y = 0.f, u2y = 0.f;
        if (x < w - 1) { const float2 r = L.u[ly][lx + 1]; u1x = r.x - u.x; u2x = r.y - u.y; }
        if (y < h - 1) { const float2 d = L.u[ly + 1][lx]; u1y = d.x - u.x; u2y = d.y - u.y; }
        const float g1 = (float)sqrt((double)u1x * u1x + (double)u1y * u1y);
        const float g2 = (float)sqrt((double)u2x * u2x + (double)u2y * u2y);
        const float ng1 = 1.0f + a.taut * g1, ng2 = 1.0f + a.taut * g2;
        const float4 q = L.p[ly + 1][lx + 1];
        const size_t k = (size_t)y * w + x;
        Un[k] = u;
        Pn[k] = make_float4((q.x + a.taut * u1x) / ng1, (q.y + a.taut * u1y) / ng1, (q.z + a.taut * u2x) / ng2, (q.w + a.taut * u2y) / ng2);
    }
    for (int s = 128; s > 0; s >>= 1) {             // fixed tree over the 256 thread sums
        if (tid < s) L.red[tid] += L.red[tid + s];
        __syncthreads();
    }
    double* part = a.partials + (size_t)p * a.nblk;
    if (tid == 0) part[blockIdx.y * gridDim.x + blockIdx.x] = L.red[0];
    if (!tv_arrive(&st->cnt, a.nblk, &L.flag)) return;
    double s = 0.0;                                   // every partial, in index order per thread, then the same fixed tree
    for (int j = tid; j < a.nblk; j += 256) s += part[j];
    __syncthreads();
    L.red[tid] = s;
    __syncthreads();
    for (int k = 128; k > 0; k >>= 1) {
        if (tid < k) L.red[tid] += L.red[tid + k];
        __syncthreads();
    }
    if (tid == 0) {
        const double total = L.red[0];
        if (a.iters) a.iters[(size_t)p * a.iters_stride + a.iter_idx] += 1;
        tv_store_state(&st->upar, upar ^ 1);
        tv_store_state(&st->ppar, ppar ^ 1);
        tv_store_state(&st->cnt, 0);
        if (!(total > a.eps)) {
            tv_store_state(&st->done, 1);
            __hip_atomic_fetch_add(a.ndone, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
    }
}

// the end of a scale: u (planar, compact at this scale's size) into the pair's output slot - the flow at scale 0, else the next
// scale's upscale source
__global__ __launch_bounds__(256) void tv_store_kernel(TvArgs a, float* __restrict__ out, size_t out_stride) {
    const int x = blockIdx.x * 64 + threadIdx.x, y = blockIdx.y * 4 + threadIdx.y, p = blockIdx.z;
    if (x >= a.w || y >= a.h) return;
    const TvPair b = tv_pair(a, p);
    const float2 u = b.U(tv_load_state(&a.state[p].upar))[(size_t)y * a.w + x];
    float* o = out + (size_t)p * out_stride;
    o[(size_t)y * a.w + x] = u.x;
    o[(size_t)a.h * a.w + (size_t)y * a.w + x] = u.y;
}

// ---- host side --------------------------------------------------------------------------------------------------------------------
// interpolateCubic(x = i/32) in float, OpenCV's operation order (no contraction: the file is built with -ffp-contract=off)
static void tv_cubic_table(TvCubic& T) {
    const float A = -0.75f;
    for (int i = 0; i < 32; ++i) {
        const float x = (float)i * (1.f / 32);
        float* c = T.t[i];
        c[0] = ((A * (x + 1) - 5 * A) * (x + 1) + 8 * A) * (x + 1) - 4 * A;
        c[1] = ((A + 2) * x - (A + 3)) * x * x + 1;
        c[2] = ((A + 2) * (1 - x) - (A + 3)) * (1 - x) * (1 - x) + 1;
        c[3] = 1.f - c[0] - c[1] - c[2];
    }
}

int tvl1_scales(int h, int w, const adain_tvl1_params* p, int* out_nscales, int* sizes_wh) {
    if (!tv_check(p, h, w, "tvl1_scales")) return ADAIN_EINVAL;
    TvScale S[TV_MAX_SCALES];
    const int n = tv_schedule(h, w, p->nscales, p->scaleStep, S, nullptr);
    if (out_nscales) *out_nscales = n;
    if (sizes_wh)
        for (int s = 0; s < n; ++s) { sizes_wh[2 * s] = S[s].w; sizes_wh[2 * s + 1] = S[s].h; }
    return 0;
}

size_t tvl1_frame_bytes(int h, int w, const adain_tvl1_params* p) {
    if (!tv_check(p, h, w, "tvl1_frame_bytes")) return 0;
    TvScale S[TV_MAX_SCALES];
    size_t floats = 0;
    tv_schedule(h, w, p->nscales, p->scaleStep, S, &floats);
    return floats * sizeof(float);
}

static int tv_nblk(int h, int w) { return ((w + ST_TX - 1) / ST_TX) * ((h + ST_TY - 1) / ST_TY); }

// One call's workspace (offsets in bytes).  The stop counter and the pair states share the first block - the counter in a slot of a
// state's size, the states behind it - and are cleared together at the start of a call; then every pair's error partials
// [npairs][nblk] at the full size, then every pair's 16 pixel planes.
struct TvLayout {
    size_t o_ndone, o_state, clear_bytes, o_partials, o_pairs, total;
    size_t plane, pair_floats;      // floats: one full-size pixel plane (a multiple of 256 bytes), a pair's buffers
};
static TvLayout tv_layout(int h, int w, int npairs) {
    TvLayout l{};
    Carve c;
    l.o_ndone = c.take((size_t)(npairs + 1) * sizeof(TvState));
    l.o_state = l.o_ndone + sizeof(TvState);
    l.clear_bytes = c.at;
    l.o_partials = c.take((size_t)npairs * tv_nblk(h, w) * sizeof(double));
    l.plane = align256((size_t)h * w * sizeof(float)) / sizeof(float);
    l.pair_floats = 16 * l.plane;
    l.o_pairs = c.take((size_t)npairs * l.pair_floats * sizeof(float));
    l.total = c.at;
    return l;
}

size_t tvl1_workspace_bytes(int h, int w, int npairs, const adain_tvl1_params* p) {
    if (!tv_check(p, h, w, "tvl1_workspace_bytes") || npairs < 1 || npairs > 65535) return 0;
    return tv_layout(h, w, npairs).total;
}

int launch_tvl1_prepare(const uint8_t* gray, int n, int h, int w, const adain_tvl1_params* p, float* prep, hipStream_t s) {
    if (!tv_check(p, h, w, "tvl1_prepare")) return ADAIN_EINVAL;
    if (n < 1 || n > 65535) { set_error("tvl1_prepare: bad frame count %d", n); return ADAIN_EINVAL; }
    TvScale S[TV_MAX_SCALES];
    size_t ff = 0;
    const int ns = tv_schedule(h, w, p->nscales, p->scaleStep, S, &ff);
    const dim3 blk(64, 4);
    hipLaunchKernelGGL(tv_to_float_kernel, dim3((w + 63) / 64, (h + 3) / 4, n), blk, 0, s, gray, h, w, prep, ff);
    for (int k = 0; k < ns; ++k) {
        const TvScale& c = S[k];
        if (k > 0) {
            const double sc = 1. / p->scaleStep;
            const int mode = resize_mode(S[k - 1].h, S[k - 1].w, c.h, c.w, sc, sc);
            hipLaunchKernelGGL(tv_scale_kernel, dim3((c.w + 63) / 64, (c.h + 3) / 4, n), blk, 0, s, prep, ff, S[k - 1].off, S[k - 1].h,
                               S[k - 1].w, c.off, c.h, c.w, mode, sc, sc);
        }
        hipLaunchKernelGGL(tv_gradient_kernel, dim3((c.w + 63) / 64, (c.h + 3) / 4, n), blk, 0, s, prep, ff, c.off, c.h, c.w);
    }
    return check_launch("tvl1_prepare");
}

int launch_tvl1_flow(const float* const* prev, const float* const* next, int npairs, int h, int w, const adain_tvl1_params* p, float* flows, int* iters,
                     void* ws, size_t ws_bytes, hipStream_t s) {
    if (!tv_check(p, h, w, "tvl1_flow")) return ADAIN_EINVAL;
    if (npairs < 1 || npairs > 65535) { set_error("tvl1_flow: bad pair count %d", npairs); return ADAIN_EINVAL; }
    const TvLayout l = tv_layout(h, w, npairs);
    if (int rc = check_workspace("tvl1_flow", ws, ws_bytes, l.total, 1)) return rc;
    TvScale S[TV_MAX_SCALES];
    size_t ff = 0;
    const int ns = tv_schedule(h, w, p->nscales, p->scaleStep, S, &ff);
    char* base = (char*)ws;
    TvArgs a{};
    a.prev = prev;
    a.next = next;
    a.npairs = npairs;
    a.ndone = (int*)(base + l.o_ndone);
    a.state = (TvState*)(base + l.o_state);
    a.partials = (double*)(base + l.o_partials);
    a.ws_pairs = (float*)(base + l.o_pairs);
    a.pair_floats = l.pair_floats;
    a.plane = l.plane;
    a.iters = iters;
    a.iters_stride = ns * p->warps;
    a.l_t = (float)(p->lambda * p->theta);
    a.theta = (float)p->theta;
    a.taut = (float)(p->tau / p->theta);
    const float inv_step = (float)(1. / p->scaleStep);
    const size_t out_stride = 2 * (size_t)h * w;
    TvCubic tab;
    tv_cubic_table(tab);
    if (hipMemsetAsync(base + l.o_ndone, 0, l.clear_bytes, s) != hipSuccess) { set_error("tvl1_flow: hipMemsetAsync failed"); return ADAIN_ELAUNCH; }
    const dim3 blk(64, 4);
    for (int k = ns - 1; k >= 0; --k) {
        const TvScale& c = S[k];
        a.scale_off = c.off;
        a.h = c.h;
        a.w = c.w;
        a.nblk = tv_nblk(c.h, c.w);
        a.eps = (double)(float)(p->epsilon * p->epsilon * (double)((size_t)c.w * c.h));
        const dim3 pix((c.w + 63) / 64, (c.h + 3) / 4, npairs), tiles((c.w + ST_TX - 1) / ST_TX, (c.h + ST_TY - 1) / ST_TY, npairs);
        int mode = 0, cw = 0, ch = 0;
        double sx = 0, sy = 0;
        if (k < ns - 1) {
            cw = S[k + 1].w;
            ch = S[k + 1].h;
            sx = 1. / ((double)c.w / cw);
            sy = 1. / ((double)c.h / ch);
            mode = resize_mode(ch, cw, c.h, c.w, sx, sy);
        }
        hipLaunchKernelGGL(tv_init_kernel, pix, blk, 0, s, a, flows, out_stride, ch, cw, mode, sx, sy, inv_step);
        for (int wi = 0; wi < p->warps; ++wi) {
            a.iter_idx = k * p->warps + wi;
            hipLaunchKernelGGL(tv_warp_kernel, pix, blk, 0, s, a, tab);
            for (int o = 0; o < p->outerIterations; ++o) {
                if (p->medianFiltering == 3) hipLaunchKernelGGL(tv_median_kernel<3>, pix, blk, 0, s, a);
                if (p->medianFiltering == 5) hipLaunchKernelGGL(tv_median_kernel<5>, pix, blk, 0, s, a);
                for (int it = 0; it < p->innerIterations; ++it) hipLaunchKernelGGL(tv_step_kernel, tiles, blk, 0, s, a);
                if (int rc = check_launch("tvl1_flow")) return rc;
                if (o + 1 < p->outerIterations) {      // every pair done for this warp: skip its remaining launches
                    int done = 0;
                    if (hipMemcpyAsync(&done, a.ndone, sizeof(int), hipMemcpyDeviceToHost, s) != hipSuccess ||
                        hipStreamSynchronize(s) != hipSuccess) {
                        set_error("tvl1_flow: reading the stop count failed");
                        return ADAIN_ELAUNCH;
                    }
                    if (done >= npairs) break;
                }
            }
        }
        hipLaunchKernelGGL(tv_store_kernel, pix, blk, 0, s, a, flows, out_stride);
        if (int rc = check_launch("tvl1_flow")) return rc;
    }
    return 0;
}

}  // namespace adain
