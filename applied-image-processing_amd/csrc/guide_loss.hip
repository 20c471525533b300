// The guide-view loss of Style_3DGS/train.py:208-221 on the device (gfx950): from freeze_iters on every iteration opens the stylised guide
// picture of the view, turns it into a float tensor, F.interpolate()s it to the render's size (bilinear, align_corners=False) and takes
// l1_loss(image, guide) and its backward.  Here the guide stays uint8 HWC at its own size and the resample, the difference, the
// reduction and the gradient are one pass each; no float guide is written (unless the caller asks for it).
//
// The value of one sample.  Every line rounds once, in float32 (the file is built without FMA contraction); restated in
// tests/guide_loss_ref.py:
//   p     = float(u8) / 255.0f                      a true division, the rule of adain_u8_to_f32
//   per axis (ATen's area_pixel_compute_source_index, tests/pixel_ref.py:bilinear_axis):
//     scale = f32(in) / f32(out)
//     r     = max(scale * (o + 0.5f) - 0.5f, 0)
//     i0    = min(int(r), in - 1)
//     i1    = i0 + (i0 < in - 1)
//     l1    = clamp(r - i0, 0, 1)
//     l0    = 1 - l1
//   top   = lx0 * p[y0][x0] + lx1 * p[y0][x1],  bot likewise on row y1,  g = ly0 * top + ly1 * bot
//           (the bits adain_u8_to_f32 followed by adain_resize_bilinear produce; a tap of weight 0 still enters the sum)
//   d     = x - g
//   term  = |d|
//   sign  = x > g ? 1 : x < g ? -1 : d              zero, or an input's NaN (the rule of metrics.hip's combine pass)
//   l1_i  = (sum of term over the frame, in float64) / count,  count = 3 h w, one float64 division
//   grad_j = (float)(weights[i] / count) * sign_j   the scalar formed in float64 and rounded once
//
// Geometry of both passes: a thread owns four consecutive outputs of one row in all three planes (the six guide bytes of a tap pair
// serve the three channels), a workgroup 256 such quads in row-major order of the frame; grid (ceil(h ceil(w / 4) / 256), n).
// With w % 4 == 0 and 16-byte aligned float buffers the image is read and the gradient written 16 bytes at a time, otherwise sample by
// sample.  The guide is gathered byte by byte from global memory (a 512 x 512 guide is 0.75 MB: it stays in L2).
//
// Forward (2 launches, whatever n; nothing allocates or waits):
//   tile   : per thread the twelve terms in a fixed order (plane, then column) as float64, then a butterfly over the wave's lanes,
//            then the four waves in index order through LDS; one float64 partial per workgroup into the workspace, every one written
//            by every call.
//   finish : a workgroup per frame; thread t adds partials t, t + 256, ... in index order, then the same butterfly and the waves in
//            index order: a fixed tree.
// Gradient (1 launch): recomputes g; a frame whose weight is zero receives +0 and neither its image nor its guide is read.
// No float atomics, spin-waits or flags: a frame's out and grad bits are a function of its image, its guide and its weight alone.
#include "common.h"

namespace adain {
namespace {

constexpr int THREADS = 256, QUAD = 4;

struct GuideArgs {
    const float* image;       // [n][3][h][w]
    const uint8_t* guide;     // [n][gh][gw][3]
    int h, w, gh, gw;
    int qw;                   // quads of a row: ceil(w / 4)
    unsigned quads;           // of a frame: h qw
    // forward
    float* resampled;         // or nullptr
    double* partials;         // [n][gridDim.x]
    // gradient
    const double* weights;    // [n]
    float* grad;
};

__device__ __forceinline__ double wave_sum(double v) {
    for (int d = 32; d > 0; d >>= 1) v += __shfl_xor(v, d);
    return v;
}

// the workgroup's sum (in every thread): a butterfly over each wave's lanes, then the waves in index order through LDS
__device__ __forceinline__ double block_sum(double v, double (&part)[THREADS / 64]) {
    const int t = threadIdx.x;
    v = wave_sum(v);
    if ((t & 63) == 0) part[t >> 6] = v;
    __syncthreads();
    double p = part[0];
    for (int k = 1; k < THREADS / 64; ++k) p += part[k];
    return p;
}

__device__ __forceinline__ float tap(const uint8_t* p, int i) { return __fdiv_rn((float)p[i], 255.0f); }

// g of row oy, columns x .. x + 3 (those past the row's end repeat its last column), all three channels, of one guide frame
__device__ __forceinline__ void resample_quad(const uint8_t* __restrict__ frame, int gh, int gw, int h, int w, int oy, int x, float (&g)[3][QUAD]) {
    const float sy = (float)gh / (float)h, sx = (float)gw / (float)w;
    const float ry = fmaxf(sy * ((float)oy + 0.5f) - 0.5f, 0.f);
    const int y0 = min((int)ry, gh - 1), y1 = y0 + (y0 < gh - 1 ? 1 : 0);
    const float ly1 = fminf(fmaxf(ry - (float)y0, 0.f), 1.f), ly0 = 1.f - ly1;
    const uint8_t* __restrict__ p0 = frame + (size_t)y0 * gw * 3;
    const uint8_t* __restrict__ p1 = frame + (size_t)y1 * gw * 3;
#pragma unroll
    for (int k = 0; k < QUAD; ++k) {
        const int ox = min(x + k, w - 1);
        const float rx = fmaxf(sx * ((float)ox + 0.5f) - 0.5f, 0.f);
        const int x0 = min((int)rx, gw - 1), x1 = x0 + (x0 < gw - 1 ? 1 : 0);
        const float lx1 = fminf(fmaxf(rx - (float)x0, 0.f), 1.f), lx0 = 1.f - lx1;
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            const float top = lx0 * tap(p0, x0 * 3 + c) + lx1 * tap(p0, x1 * 3 + c);
            const float bot = lx0 * tap(p1, x0 * 3 + c) + lx1 * tap(p1, x1 * 3 + c);
            g[c][k] = ly0 * top + ly1 * bot;
        }
    }
}

// grid (tiles, n).  VEC: w % 4 == 0, image and resampled 16-byte aligned
template <bool VEC>
__global__ __launch_bounds__(THREADS) void guide_l1_tile_kernel(GuideArgs a) {
    __shared__ double part[THREADS / 64];
    const int t = threadIdx.x;
    const unsigned q = blockIdx.x * THREADS + t;
    double sum = 0.0;
    if (q < a.quads) {
        const int oy = (int)(q / (unsigned)a.qw), x = (int)(q % (unsigned)a.qw) * QUAD;
        const size_t hw = (size_t)a.h * a.w;
        const size_t at = (size_t)blockIdx.y * 3 * hw + (size_t)oy * a.w + x;          // the quad's first sample in plane 0
        float g[3][QUAD];
        resample_quad(a.guide + (size_t)blockIdx.y * a.gh * a.gw * 3, a.gh, a.gw, a.h, a.w, oy, x, g);
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            const float* __restrict__ px = a.image + at + c * hw;
            if constexpr (VEC) {
                const f32x4 xv = *(const f32x4*)px;
#pragma unroll
                for (int k = 0; k < QUAD; ++k) sum += (double)fabsf(xv[k] - g[c][k]);
                if (a.resampled) *(f32x4*)(a.resampled + at + c * hw) = f32x4{g[c][0], g[c][1], g[c][2], g[c][3]};
            } else {
#pragma unroll
                for (int k = 0; k < QUAD; ++k) {
                    if (x + k >= a.w) continue;
                    sum += (double)fabsf(px[k] - g[c][k]);
                    if (a.resampled) a.resampled[at + c * hw + k] = g[c][k];
                }
            }
        }
    }
    // over the workgroup, in a fixed order
    sum = block_sum(sum, part);
    if (t == 0) a.partials[(size_t)blockIdx.y * gridDim.x + blockIdx.x] = sum;
}

// grid n: frame blockIdx.x's `tiles` partials.  Thread t adds partials t, t + 256, ... in index order (lane-parallel: the loads of a
// thread are independent of its additions), then the fixed tree of block_sum
__global__ __launch_bounds__(THREADS) void guide_l1_finish_kernel(const double* __restrict__ partials, unsigned tiles, double count, double* __restrict__ out) {
    __shared__ double part[THREADS / 64];
    const double* p = partials + (size_t)blockIdx.x * tiles;
    double s = 0.0;
    for (unsigned i = threadIdx.x; i < tiles; i += THREADS) s += p[i];
    s = block_sum(s, part);
    if (threadIdx.x == 0) out[blockIdx.x] = s / count;
}

// grid (tiles, n).  VEC: w % 4 == 0, image and grad 16-byte aligned
template <bool VEC>
__global__ __launch_bounds__(THREADS) void guide_l1_grad_kernel(GuideArgs a) {
    const unsigned q = blockIdx.x * THREADS + threadIdx.x;
    if (q >= a.quads) return;
    const int oy = (int)(q / (unsigned)a.qw), x = (int)(q % (unsigned)a.qw) * QUAD;
    const size_t hw = (size_t)a.h * a.w;
    const size_t at = (size_t)blockIdx.y * 3 * hw + (size_t)oy * a.w + x;
    const double weight = a.weights[blockIdx.y];
    if (weight == 0.0) {          // the same in every thread of the grid row: nothing of the frame is read
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            if constexpr (VEC) {
                *(f32x4*)(a.grad + at + c * hw) = f32x4{0.f, 0.f, 0.f, 0.f};
            } else {
#pragma unroll
                for (int k = 0; k < QUAD; ++k)
                    if (x + k < a.w) a.grad[at + c * hw + k] = 0.f;
            }
        }
        return;
    }
    const float k_l1 = (float)(weight / (3.0 * (double)a.h * (double)a.w));
    float g[3][QUAD];
    resample_quad(a.guide + (size_t)blockIdx.y * a.gh * a.gw * 3, a.gh, a.gw, a.h, a.w, oy, x, g);
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        const float* __restrict__ px = a.image + at + c * hw;
        float xs[QUAD];
        if constexpr (VEC) {
            const f32x4 xv = *(const f32x4*)px;
#pragma unroll
            for (int k = 0; k < QUAD; ++k) xs[k] = xv[k];
        } else {
#pragma unroll
            for (int k = 0; k < QUAD; ++k) xs[k] = x + k < a.w ? px[k] : 0.f;
        }
        float r[QUAD];
#pragma unroll
        for (int k = 0; k < QUAD; ++k) {
            const float xv = xs[k], gv = g[c][k];
            const float d = xv - gv;
            const float sign = xv > gv ? 1.0f : xv < gv ? -1.0f : d;          // d: zero, or the NaN of an input
            r[k] = k_l1 * sign;
        }
        if constexpr (VEC) {
            *(f32x4*)(a.grad + at + c * hw) = f32x4{r[0], r[1], r[2], r[3]};
        } else {
#pragma unroll
            for (int k = 0; k < QUAD; ++k)
                if (x + k < a.w) a.grad[at + c * hw + k] = r[k];
        }
    }
}

// ---- the calls ------------------------------------------------------------------------------------------------------------------------------
struct GuidePlan {
    int qw;
    unsigned quads, tiles;          // of one frame
    size_t frame_samples;
    size_t o_partials, total;
};

const char* check_render_shape(int n, int h, int w) {
    if (n < 1 || n > 65535) return "n outside 1..65535";
    if (h < 1) return "h below 1";
    if (w < 1) return "w below 1";
    if ((uint64_t)h * (uint64_t)w > (uint64_t)0x7fffffff / 3) return "a frame beyond 2^31 - 1 samples";
    return nullptr;
}

const char* check_guide_shape(int gh, int gw) {
    if (gh < 1) return "gh below 1";
    if (gw < 1) return "gw below 1";
    if ((uint64_t)gh * (uint64_t)gw > (uint64_t)0x7fffffff / 3) return "a guide beyond 2^31 - 1 samples";
    return nullptr;
}

// The one layout of a call
GuidePlan make_guide_plan(int n, int h, int w) {
    GuidePlan p{};
    p.qw = (w + QUAD - 1) / QUAD;
    p.quads = (unsigned)h * (unsigned)p.qw;          // at most h w: below 2^31 / 3
    p.tiles = (p.quads + THREADS - 1) / THREADS;
    p.frame_samples = (size_t)3 * h * w;
    Carve ws;
    p.o_partials = ws.take((size_t)n * p.tiles * sizeof(double));
    p.total = ws.at;
    return p;
}

bool overlaps(const void* a, size_t a_bytes, const void* b, size_t b_bytes) {
    return (uintptr_t)a < (uintptr_t)b + b_bytes && (uintptr_t)b < (uintptr_t)a + a_bytes;
}

struct Span { const char* name; const void* ptr; size_t bytes; };

// does an output lie over an input, or over an output listed before it?  Sets the error text.
template <int NI, int NO>
bool any_overlap(const char* who, const Span (&ins)[NI], const Span (&outs)[NO]) {
    for (int i = 0; i < NO; ++i) {
        if (!outs[i].ptr) continue;
        for (const Span& in : ins)
            if (overlaps(outs[i].ptr, outs[i].bytes, in.ptr, in.bytes)) { set_error("%s: %s overlaps %s", who, outs[i].name, in.name); return true; }
        for (int k = 0; k < i; ++k)
            if (outs[k].ptr && overlaps(outs[i].ptr, outs[i].bytes, outs[k].ptr, outs[k].bytes)) { set_error("%s: %s overlaps %s", who, outs[i].name, outs[k].name); return true; }
    }
    return false;
}

bool aligned16(const void* p) { return ((uintptr_t)p & 15) == 0; }

GuideArgs guide_args(const float* image, const uint8_t* guide, int h, int w, int gh, int gw, const GuidePlan& p) {
    GuideArgs a{};
    a.image = image, a.guide = guide, a.h = h, a.w = w, a.gh = gh, a.gw = gw, a.qw = p.qw, a.quads = p.quads;
    return a;
}

}  // namespace

int guide_l1_f32_bytes(int n, int h, int w, size_t* workspace_bytes) {
    if (const char* bad = check_render_shape(n, h, w)) { set_error("guide_l1_f32: %s (n %d, %d x %d)", bad, n, h, w); return ADAIN_EINVAL; }
    if (workspace_bytes) *workspace_bytes = make_guide_plan(n, h, w).total;
    return 0;
}

int launch_guide_l1_f32(const float* image, const uint8_t* guide, int n, int h, int w, int gh, int gw, double* out, float* resampled, void* workspace,
                        size_t workspace_bytes, hipStream_t s) {
    const char* who = "guide_l1_f32";
    if (!image) { set_error("%s: image is a null pointer", who); return ADAIN_EINVAL; }
    if (!guide) { set_error("%s: guide is a null pointer", who); return ADAIN_EINVAL; }
    if (!out) { set_error("%s: out is a null pointer", who); return ADAIN_EINVAL; }
    if (const char* bad = check_render_shape(n, h, w)) { set_error("%s: %s (n %d, %d x %d)", who, bad, n, h, w); return ADAIN_EINVAL; }
    if (const char* bad = check_guide_shape(gh, gw)) { set_error("%s: %s (%d x %d)", who, bad, gh, gw); return ADAIN_EINVAL; }
    const GuidePlan p = make_guide_plan(n, h, w);
    if (int rc = check_workspace(who, workspace, workspace_bytes, p.total, 8)) return rc;
    if ((uintptr_t)out % 8) { set_error("%s: out must be 8-byte aligned", who); return ADAIN_EINVAL; }
    if ((uintptr_t)image % 4) { set_error("%s: image must be 4-byte aligned", who); return ADAIN_EINVAL; }
    if ((uintptr_t)resampled % 4) { set_error("%s: resampled must be 4-byte aligned", who); return ADAIN_EINVAL; }
    const size_t image_bytes = (size_t)n * p.frame_samples * sizeof(float);
    const Span ins[2] = {{"image", image, image_bytes}, {"guide", guide, (size_t)n * gh * gw * 3}};
    const Span outs[3] = {{"out", out, (size_t)n * sizeof(double)}, {"resampled", resampled, image_bytes}, {"the workspace", workspace, p.total}};
    if (any_overlap(who, ins, outs)) return ADAIN_EINVAL;
    GuideArgs a = guide_args(image, guide, h, w, gh, gw, p);
    a.resampled = resampled, a.partials = (double*)((char*)workspace + p.o_partials);
    const dim3 grid(p.tiles, (unsigned)n);
    if (w % 4 == 0 && aligned16(image) && aligned16(resampled)) guide_l1_tile_kernel<true><<<grid, THREADS, 0, s>>>(a);
    else guide_l1_tile_kernel<false><<<grid, THREADS, 0, s>>>(a);
    guide_l1_finish_kernel<<<(unsigned)n, THREADS, 0, s>>>(a.partials, p.tiles, (double)p.frame_samples, out);
    return check_launch(who);
}

int launch_guide_l1_grad_f32(const float* image, const uint8_t* guide, int n, int h, int w, int gh, int gw, const double* weights, float* grad, hipStream_t s) {
    const char* who = "guide_l1_grad_f32";
    if (!image) { set_error("%s: image is a null pointer", who); return ADAIN_EINVAL; }
    if (!guide) { set_error("%s: guide is a null pointer", who); return ADAIN_EINVAL; }
    if (!weights) { set_error("%s: weights is a null pointer", who); return ADAIN_EINVAL; }
    if (!grad) { set_error("%s: grad is a null pointer", who); return ADAIN_EINVAL; }
    if (const char* bad = check_render_shape(n, h, w)) { set_error("%s: %s (n %d, %d x %d)", who, bad, n, h, w); return ADAIN_EINVAL; }
    if (const char* bad = check_guide_shape(gh, gw)) { set_error("%s: %s (%d x %d)", who, bad, gh, gw); return ADAIN_EINVAL; }
    if ((uintptr_t)weights % 8) { set_error("%s: weights must be 8-byte aligned", who); return ADAIN_EINVAL; }
    if ((uintptr_t)image % 4) { set_error("%s: image must be 4-byte aligned", who); return ADAIN_EINVAL; }
    if ((uintptr_t)grad % 4) { set_error("%s: grad must be 4-byte aligned", who); return ADAIN_EINVAL; }
    const GuidePlan p = make_guide_plan(n, h, w);
    const size_t image_bytes = (size_t)n * p.frame_samples * sizeof(float);
    const Span ins[3] = {{"image", image, image_bytes}, {"guide", guide, (size_t)n * gh * gw * 3}, {"weights", weights, (size_t)n * sizeof(double)}};
    const Span outs[1] = {{"grad", grad, image_bytes}};
    if (any_overlap(who, ins, outs)) return ADAIN_EINVAL;
    GuideArgs a = guide_args(image, guide, h, w, gh, gw, p);
    a.weights = weights, a.grad = grad;
    const dim3 grid(p.tiles, (unsigned)n);
    if (w % 4 == 0 && aligned16(image) && aligned16(grad)) guide_l1_grad_kernel<true><<<grid, THREADS, 0, s>>>(a);
    else guide_l1_grad_kernel<false><<<grid, THREADS, 0, s>>>(a);
    return check_launch(who);
}

}  // namespace adain
