// Per-channel statistics and the AdaIN feature blend (HBM-bound kernels).
//
// Replaces calc_mean_std (Style_3DGS/AdaIN/function.py:4-12), adaptive_instance_normalization
// (function.py:15-23) and the two feature blends of the reference:
//   style_transfer_simple  feat = AdaIN * alpha + content_f * (1 - alpha)      (test.py:79-80)
//   style_transfer         feat = AdaIN * (1 - P) + content_f * P              (test.py:69-70)
// Both layouts are served: NHWC (the internal activation layout, stats are column reductions over
// pixel rows) and NCHW (the reference's tensor layout, used when a caller hands in its own tensors).
//
// Sums are accumulated in fp64 (sum and sum of squares): the unbiased variance is then exact to
// fp32 rounding without a second pass over the 33.5 MB feature map, and partial sums are combined in
// a fixed order, so results are bitwise reproducible run to run.
#include "common.h"

namespace adain {

constexpr int MS_THREADS = 256;

// ---- NHWC: feat [n][hw][c] ; block (b, img) reduces pixels b, b+nblk, ... (in row groups) ----------
// thread layout: cols = c/4 thread-columns (4 channels each), rows = MS_THREADS / cols pixel rows.
__global__ __launch_bounds__(MS_THREADS) void mean_std_nhwc_partial(const float* __restrict__ feat, int c, int hw,
                                                                    int nblk, double* __restrict__ part) {
    const int cols = c >> 2;
    const int rows = MS_THREADS / cols;
    const int tid = threadIdx.x;
    const int col = tid % cols, row = tid / cols;
    const int img = blockIdx.y, b = blockIdx.x;
    const float* __restrict__ base = feat + (size_t)img * hw * c;
    double s[4] = {0, 0, 0, 0}, q[4] = {0, 0, 0, 0};
    if (row < rows) {
        const unsigned step = nblk * rows, uhw = (unsigned)hw;          // unsigned: p + 3 step may pass 2^31 - 1 before it fails the test
        auto add = [&](const f32x4 v) {
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const double d = (double)v[k];
                s[k] += d;
                q[k] += d * d;
            }
        };
        auto at = [&](unsigned p) { return *(const f32x4*)(base + (size_t)p * c + col * 4); };
        unsigned p = b * rows + row;
        // four loads in flight per thread, summed in pixel order (the order of a plain loop: results unchanged bit for bit);
        // one dependent 16-byte load per iteration left the kernel latency-bound (1 workgroup per CU: 1.9 TB/s)
        for (; p + 3 * step < uhw; p += 4 * step) {
            const f32x4 v0 = at(p), v1 = at(p + step), v2 = at(p + 2 * step), v3 = at(p + 3 * step);
            add(v0); add(v1); add(v2); add(v3);
        }
        for (; p < uhw; p += step) add(at(p));
    }
    // combine the row groups through LDS in a fixed order
    __shared__ double sh[MS_THREADS * 8];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        sh[tid * 8 + k] = s[k];
        sh[tid * 8 + 4 + k] = q[k];
    }
    __syncthreads();
    if (tid < cols) {
        double ts[4] = {0, 0, 0, 0}, tq[4] = {0, 0, 0, 0};
        for (int r = 0; r < rows; ++r) {
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                ts[k] += sh[(r * cols + tid) * 8 + k];
                tq[k] += sh[(r * cols + tid) * 8 + 4 + k];
            }
        }
        double* __restrict__ o = part + (((size_t)img * nblk + b) * c + tid * 4) * 2;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            o[k * 2] = ts[k];
            o[k * 2 + 1] = tq[k];
        }
    }
}

// one wave per channel: lanes stride over the partial blocks, then a fixed-order butterfly reduction
__global__ __launch_bounds__(256) void mean_std_finalize(const double* __restrict__ part, int c, int hw, int nblk, float eps,
                                                         float* __restrict__ mean, float* __restrict__ std_) {
    const int lane = threadIdx.x & 63;
    const int ch = blockIdx.x * 4 + (threadIdx.x >> 6);
    const int img = blockIdx.y;
    if (ch >= c) return;
    double s = 0, q = 0;
    for (int b = lane; b < nblk; b += 64) {
        const double* p = part + (((size_t)img * nblk + b) * c + ch) * 2;
        s += p[0];
        q += p[1];
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        s += __shfl_xor(s, off, 64);
        q += __shfl_xor(q, off, 64);
    }
    if (lane == 0) {
        const double m = s / hw;
        // unbiased variance (torch.var default, function.py:9); hw == 1 gives 0/0 = NaN like torch
        const double var = (q - s * m) / (double)(hw - 1);
        mean[(size_t)img * c + ch] = (float)m;
        std_[(size_t)img * c + ch] = sqrtf((float)var + eps);
    }
}

// ---- NCHW: feat [n][c][hw] ; one block per (n, c) plane -------------------------------------------------
__global__ __launch_bounds__(MS_THREADS) void mean_std_nchw_kernel(const float* __restrict__ feat, int hw, float eps,
                                                                   float* __restrict__ mean, float* __restrict__ std_) {
    const size_t plane = blockIdx.x;
    const float* __restrict__ p = feat + plane * hw;
    double s = 0, q = 0;
    for (unsigned i = threadIdx.x; i < (unsigned)hw; i += MS_THREADS) {          // unsigned: the last step may pass 2^31 - 1
        const double d = (double)p[i];
        s += d;
        q += d * d;
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        s += __shfl_down(s, off, 64);
        q += __shfl_down(q, off, 64);
    }
    __shared__ double sh[2 * (MS_THREADS / 64)];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    if (lane == 0) {
        sh[wave * 2] = s;
        sh[wave * 2 + 1] = q;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        double ts = 0, tq = 0;
        for (int w = 0; w < MS_THREADS / 64; ++w) {
            ts += sh[w * 2];
            tq += sh[w * 2 + 1];
        }
        const double m = ts / hw;
        const double var = (tq - ts * m) / (double)(hw - 1);
        mean[plane] = (float)m;
        std_[plane] = sqrtf((float)var + eps);
    }
}

static int nhwc_blocks(int c, int hw) {
    const int rows = MS_THREADS / (c >> 2);
    long long nblk = ((long long)hw + rows * 16 - 1) / (rows * 16);   // >= 16 row groups of work per block
    constexpr int cap = 256;
    if (nblk > cap) nblk = cap;
    if (nblk < 1) nblk = 1;
    return (int)nblk;
}

// The workspace is one block, the NHWC form's partial sums [n][nblk][c][2] double: nothing to lay out, and its size is not rounded up
// to 256 bytes (a caller's buffer of exactly this size must stay enough).
size_t mean_std_workspace_bytes(int nhwc, int n, int c, int hw) {
    if (!nhwc) return 0;
    if (c < 4 || (c & 3) || (c >> 2) > MS_THREADS) return 0;
    return (size_t)n * nhwc_blocks(c, hw) * c * 2 * sizeof(double);
}

int launch_mean_std(const float* feat, int nhwc, int n, int c, int hw, float eps, float* mean, float* std_,
                    void* workspace, size_t ws_bytes, hipStream_t s) {
    if (n < 1 || c < 1 || hw < 1) { set_error("mean_std: bad shape n=%d c=%d hw=%d", n, c, hw); return ADAIN_EINVAL; }
    // the blends' limit; with it the NCHW form's n c planes of 256 threads stay below the 2^32 threads of a launch for hw >= 128
    if ((size_t)n * c * hw >= 0x7fffffffULL) { set_error("mean_std: more than 2^31 elements per call"); return ADAIN_EINVAL; }
    if (nhwc ? n > 65535 : (size_t)n * c > 0xffffffULL) {
        set_error("mean_std: more than 65535 images (NHWC) or 16777215 planes (NCHW) per call");
        return ADAIN_EINVAL;
    }
    if (nhwc) {
        if ((c & 3) || (c >> 2) > MS_THREADS) { set_error("mean_std(NHWC): c=%d must be a multiple of 4 and <= 1024", c); return ADAIN_EINVAL; }
        const int nblk = nhwc_blocks(c, hw);
        if (int rc = check_workspace("mean_std", workspace, ws_bytes, mean_std_workspace_bytes(1, n, c, hw), 1)) return rc;
        hipLaunchKernelGGL(mean_std_nhwc_partial, dim3(nblk, n), dim3(MS_THREADS), 0, s, feat, c, hw, nblk, (double*)workspace);
        hipLaunchKernelGGL(mean_std_finalize, dim3((c + 3) / 4, n), dim3(256), 0, s, (const double*)workspace, c, hw, nblk, eps, mean, std_);
    } else {
        hipLaunchKernelGGL(mean_std_nchw_kernel, dim3((unsigned)((size_t)n * c)), dim3(MS_THREADS), 0, s, feat, hw, eps, mean, std_);
    }
    return check_launch("mean_std");
}

// ---- AdaIN + blend, of one style or of a weighted mix of K styles (style interpolation) ------------------------------------------
// The reference's style_transfer (Style_3DGS/AdaIN/test.py:70,80; with interpolation_weights test_video.py:30-45) in its operation
// order, one rounding per operation, no FMA contraction:
//   nrm  = (x - mu_c) / sigma_c                                  function.py:21-22, the same for every style
//   b_k  = nrm * sigma_s[k] + mu_s[k]                            function.py:23
//   feat = b_0                                                   one style (StyleTerm::weights == nullptr): nothing is multiplied
//   feat = w_0 * b_0 ; feat = feat + w_k * b_k, k = 1 .. K-1     a mix, test_video.py:37-40 (its leading 0 + w_0 * b_0 is w_0 * b_0)
//   out  = feat * w1 + x * w2                                    test.py:70,80, test_video.py:44
//   alpha mode (pmap == nullptr): w1 = alpha, w2 = one_minus_alpha (computed on the host in double)
//   pmap  mode                  : w1 = 1 - P[pixel], w2 = P[pixel]      (P broadcast over channels)
// w_k is a scalar (weights_hw == 1) or a per-pixel map W[k][pixel]; the weights are used as given.
struct BlendArgs {
    const float* x;
    const float *c_mean, *c_std, *s_mean, *s_std;   // [n][c], [n][c], [k][c] or (per_frame) [n][k][c]
    const float* weights;                           // nullptr: one style, k = 1
    const float* pmap;                              // nullptr: alpha form
    float* out;
    int c, hw, k, per_frame, weights_n, weights_hw, pmap_n;
    float alpha, one_minus_alpha;
};

// The product shape (NHWC, c = 512) and every other NHWC shape whose c / 4 channel quads divide the workgroup: a workgroup owns
// whole pixels of ONE image, a thread one channel quad of them.  The thread keeps its quad of the content statistics and of the K
// styles' (2 K + 2 b128 loads, once) in registers and then walks pixels with one b128 load and one b128 store each: 8 bytes per
// element whatever K is.  KB bounds K at compile time so that the statistics are registers, not scratch: 4 (34 VGPRs of statistics)
// or MIX_MAX_STYLES (130).  A pixel's weights and strength are the same for the lanes of its row (at c = 512 a row is two waves).
// Mixes only: never launched without weights or with per_frame.
template <int KB, bool MAPS>
__global__ __launch_bounds__(256) void adain_mix_walk_kernel(const BlendArgs a, int cols_log2, int bpi) {
#pragma clang fp contract(off)
    constexpr int UN = KB <= 4 ? 4 : 2;             // pixels in flight per thread
    const unsigned c = (unsigned)a.c, hw = (unsigned)a.hw;
    const unsigned tid = threadIdx.x, col = tid & ((1u << cols_log2) - 1u), row = tid >> cols_log2;
    const unsigned rows = 256u >> cols_log2;
    const unsigned img = blockIdx.x / (unsigned)bpi, b = blockIdx.x - img * (unsigned)bpi;
    const unsigned ch = col * 4u;
    const f32x4 mc = *(const f32x4*)(a.c_mean + (size_t)img * c + ch), sc = *(const f32x4*)(a.c_std + (size_t)img * c + ch);
    const float* __restrict__ wrow = a.weights + (size_t)(a.weights_n == 1 ? 0u : img) * a.k * a.weights_hw;
    f32x4 ms[KB], ss[KB];
    float wk[KB];
#pragma unroll
    for (int j = 0; j < KB; ++j) {
        ms[j] = ss[j] = f32x4{0.f, 0.f, 0.f, 0.f};
        wk[j] = 0.f;
        if (j < a.k) {
            ms[j] = *(const f32x4*)(a.s_mean + (unsigned)j * c + ch);
            ss[j] = *(const f32x4*)(a.s_std + (unsigned)j * c + ch);
            if (!MAPS) wk[j] = wrow[j];
        }
    }
    const float* __restrict__ xb = a.x + (size_t)img * hw * c + ch;
    float* __restrict__ ob = a.out + (size_t)img * hw * c + ch;
    const float* __restrict__ pb = a.pmap ? a.pmap + (size_t)(a.pmap_n == 1 ? 0u : img) * hw : nullptr;
    auto one = [&](unsigned p, const f32x4 v) {
#pragma clang fp contract(off)
        float w1 = a.alpha, w2 = a.one_minus_alpha;
        if (pb) {
            const float pp = pb[p];
            w1 = 1.0f - pp;
            w2 = pp;
        }
        const f32x4 nrm = (v - mc) / sc;
        f32x4 feat = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int j = 0; j < KB; ++j) {
            if (j < a.k) {
                const float w = MAPS ? wrow[(size_t)j * hw + p] : wk[j];
                const f32x4 t = nrm * ss[j] + ms[j];
                const f32x4 wt = t * w;
                feat = j ? feat + wt : wt;
            }
        }
        const f32x4 l = feat * w1, r = v * w2;
        *(f32x4*)(ob + p * c) = l + r;
    };
    if (row < rows) {
        const unsigned step = (unsigned)bpi * rows;
        unsigned p = b * rows + row;
        for (; p + (UN - 1) * step < hw; p += UN * step) {
            f32x4 v[UN];
#pragma unroll
            for (int u = 0; u < UN; ++u) v[u] = *(const f32x4*)(xb + (p + u * step) * c);
#pragma unroll
            for (int u = 0; u < UN; ++u) one(p + u * step, v[u]);
        }
        for (; p < hw; p += step) one(p, *(const f32x4*)(xb + p * c));
    }
}

// T = f32x4: four consecutive channels from ch of NHWC pixel pix, one b128 load per statistic; T = float: one element.  Of image img.
template <typename T>
__device__ __forceinline__ T blend_one(const BlendArgs& a, T v, unsigned img, unsigned ch, unsigned pix) {
#pragma clang fp contract(off)
    const unsigned c = (unsigned)a.c, hw = (unsigned)a.hw, k = (unsigned)a.k, whw = (unsigned)a.weights_hw;
    const T mc = *(const T*)(a.c_mean + img * c + ch), sc = *(const T*)(a.c_std + img * c + ch);
    float w1 = a.alpha, w2 = a.one_minus_alpha;
    if (a.pmap) {
        const float p = a.pmap[(a.pmap_n == 1 ? 0u : img) * hw + pix];
        w1 = 1.0f - p;
        w2 = p;
    }
    const unsigned srow = ((a.per_frame ? img : 0u) * k) * c + ch;
    const float* __restrict__ wp = a.weights ? a.weights + (size_t)(a.weights_n == 1 ? 0u : img) * k * whw + (whw == 1 ? 0u : pix) : nullptr;
    const T nrm = (v - mc) / sc;
    T feat{};
    for (unsigned j = 0; j < k; ++j) {
        T t = nrm * *(const T*)(a.s_std + srow + j * c) + *(const T*)(a.s_mean + srow + j * c);
        if (wp) t = t * wp[(size_t)j * whw];
        feat = j ? feat + t : t;
    }
    const T l = feat * w1, r = v * w2;
    return l + r;
}

// Every other launch: quads of four elements, 32-bit index arithmetic (the launcher checks total < 2^31).  NHWC with any c % 4 == 0:
// a quad is four channels of one pixel.  NCHW: the launcher asks n*c*hw % 4 == 0, not c*hw % 4 == 0, so a quad may run over the end
// of its first element's image (over three of them when c*hw == 1): every element takes its own image, and with it its own style,
// strength-map and weight rows.
template <bool NHWC>
__global__ __launch_bounds__(256) void adain_blend_kernel(const BlendArgs a, size_t total4) {
    const unsigned c = (unsigned)a.c, hw = (unsigned)a.hw, per_img = c * hw;
    for (unsigned i = blockIdx.x * blockDim.x + threadIdx.x; i < (unsigned)total4; i += gridDim.x * blockDim.x) {
        const unsigned e = i * 4u;
        const f32x4 v = *(const f32x4*)(a.x + e);
        f32x4 r;
        unsigned img = e / per_img, rem = e - img * per_img;
        if (NHWC) {
            r = blend_one(a, v, img, rem % c, rem / c);
        } else {
#pragma unroll
            for (int q = 0; q < 4; ++q, ++rem) {
                if (rem >= per_img) {
                    rem -= per_img;
                    ++img;
                }
                r[q] = blend_one(a, v[q], img, rem / hw, rem % hw);
            }
        }
        *(f32x4*)(a.out + e) = r;
    }
}

int check_adain_blend(const char* what, int nhwc, int n, int c, int hw, const StyleTerm& st, const BlendTerm& b) {
    if (n < 1 || c < 1 || hw < 1) { set_error("%s: bad shape n=%d c=%d hw=%d", what, n, c, hw); return ADAIN_EINVAL; }
    if (st.k < 1 || st.k > MIX_MAX_STYLES) { set_error("%s: %d styles (1..%d)", what, st.k, MIX_MAX_STYLES); return ADAIN_EINVAL; }
    if (st.weights ? st.per_frame : st.k != 1) { set_error("%s: a mix needs weights and one set of styles for all frames", what); return ADAIN_EINVAL; }
    if (st.weights && st.weights_n != 1 && st.weights_n != n) { set_error("%s: weights batch %d must be 1 or %d", what, st.weights_n, n); return ADAIN_EINVAL; }
    if (st.weights && st.weights_hw != 1 && st.weights_hw != hw) { set_error("%s: weights per style %d must be 1 or %d (hw)", what, st.weights_hw, hw); return ADAIN_EINVAL; }
    if (b.pmap && b.pmap_n != 1 && b.pmap_n != n) { set_error("%s: pmap batch %d must be 1 or %d", what, b.pmap_n, n); return ADAIN_EINVAL; }
    const size_t total = (size_t)n * c * hw;
    if (nhwc ? (c & 3) : (total & 3)) { set_error("%s: element count / channels must be a multiple of 4", what); return ADAIN_EINVAL; }
    if (total >= 0x7fffffffULL) { set_error("%s: more than 2^31 elements per call", what); return ADAIN_EINVAL; }
    return 0;
}

// Launcher branches:
//   a mix, NHWC, c / 4 a power of two <= 256 (c = 4 .. 1024; the product's 512): adain_mix_walk_kernel, KB = 4 for k <= 4 and
//     MIX_MAX_STYLES above, scalar weights or maps; ceil(pixel rows / 8) workgroups per image, at most 2048 / n (at least 1): more
//     pixels per thread on large maps, so that the statistics' loads stay a small share
//   one style, any other NHWC c, and NCHW: adain_blend_kernel, at most 8192 workgroups, grid-stride
int launch_adain_blend(const float* content, int nhwc, int n, int c, int hw, const float* c_mean, const float* c_std, const StyleTerm& st,
                       const BlendTerm& b, float* out, hipStream_t s) {
    const char* what = st.weights ? "adain_blend_mix" : "adain_blend";
    if (check_adain_blend(what, nhwc, n, c, hw, st, b)) return ADAIN_EINVAL;
    const BlendArgs a{content, c_mean, c_std, st.s_mean, st.s_std, st.weights, b.pmap, out, c, hw, st.k, st.per_frame, st.weights_n, st.weights_hw,
                      b.pmap_n, b.alpha, b.one_minus_alpha};
    const int cols = c >> 2;
    if (st.weights && nhwc && cols <= 256 && (cols & (cols - 1)) == 0) {
        int cols_log2 = 0;
        while ((1 << cols_log2) < cols) ++cols_log2;
        const int rows = 256 / cols;
        const int groups = (hw + rows - 1) / rows;
        int bpi = (groups + 7) / 8;
        const int cap = n < 2048 ? 2048 / n : 1;
        if (bpi > cap) bpi = cap;
        const dim3 grid((unsigned)((size_t)n * bpi));
        const bool maps = st.weights_hw != 1;
        if (st.k <= 4) {
            if (maps) hipLaunchKernelGGL((adain_mix_walk_kernel<4, true>), grid, dim3(256), 0, s, a, cols_log2, bpi);
            else hipLaunchKernelGGL((adain_mix_walk_kernel<4, false>), grid, dim3(256), 0, s, a, cols_log2, bpi);
        } else {
            if (maps) hipLaunchKernelGGL((adain_mix_walk_kernel<MIX_MAX_STYLES, true>), grid, dim3(256), 0, s, a, cols_log2, bpi);
            else hipLaunchKernelGGL((adain_mix_walk_kernel<MIX_MAX_STYLES, false>), grid, dim3(256), 0, s, a, cols_log2, bpi);
        }
        return check_launch(what);
    }
    const size_t total4 = (size_t)n * c * hw / 4;
    const unsigned blocks = (unsigned)((total4 + 255) / 256 < 8192 ? (total4 + 255) / 256 : 8192);
    if (nhwc) hipLaunchKernelGGL(adain_blend_kernel<true>, dim3(blocks), dim3(256), 0, s, a, total4);
    else hipLaunchKernelGGL(adain_blend_kernel<false>, dim3(blocks), dim3(256), 0, s, a, total4);
    return check_launch(what);
}

}  // namespace adain
