// Colour-preserving stylisation on the device: coral(style, content) of the reference (Style_3DGS/AdaIN/function.py:26-67), which
// adain_inference(preserve_color=True) applies to the transformed style image before it is encoded (test.py:201-202).
//
// With x the style's pixels [3][HW], y the content's, mu / sigma the per-channel mean and UNBIASED standard deviation:
//     norm(x) = (x - mu) / sigma,   C = norm norm^T + I   (3 x 3, both sides),
//     coral   = (sqrt(C_content) . inverse(sqrt(C_style)) . norm(style)) * sigma_content + mu_content,
// sqrt(C) = U diag(sqrt(D)) V^T from torch.linalg.svd.  C is symmetric: (HW - 1) R + I with R the channels' correlation matrix, whose
// eigenvalues are >= 0, so every eigenvalue of C is >= 1, its SVD square root is the symmetric square root V diag(sqrt(lambda)) V^T
// and the inverse is V diag(1 / sqrt(lambda)) V^T with 1 / sqrt(lambda) <= 1: nothing to pivot, nothing ill-conditioned.  Everything
// folds into ONE affine map per (style, content) pair,
//     A = diag(sigma_content) . M . diag(1 / sigma_style),  M = sqrt(C_content) . inverse(sqrt(C_style)),  b = mu_content - A mu_style,
// so the transform is three stages:
//   1. moments per image: HW, sum x_i, sum x_i x_j (9 sums).  uint8 images: 64-bit integer sums of the BYTE values - exact, whatever
//      the grid and the order.  float images: float64 sums of (x - K), K the image's first pixel (a constant channel then sums to an
//      exact zero, and the cancellation in sum d d^T - N dbar dbar^T is that of the image's spread, not of its level).  A thread
//      adds groups of 4 consecutive pixels in index order, a workgroup combines its threads with a butterfly and a fixed walk over
//      its waves, the matrix kernel combines the workgroups the same way; groups and grid depend on HW alone, never on the address:
//      the same input gives the same bytes on every run, stream, batch position and device size.
//   2. one wave per pair: the workgroups' partial sums, then one lane in float64: means, deviations, both C, a cyclic Jacobi
//      eigen-solve (device_utils.h), A and b, written to the pair's adain_coral_record at the head of the workspace.
//   3. per style pixel A x + b in float64, rounded once to float, written planar (NCHW), 4 pixels per thread.
// uint8 pixels enter the moments as v / 255 (exactly, through the integer sums) and stage 3 as float(v) / 255.0f correctly rounded -
// adain_u8_to_f32's value, what the encoder's first layer reads.  The output is NOT clamped (the reference does not clamp).
// A side of fewer than two pixels or with a channel of zero variance (the reference divides by zero: NaNs) sets the record's status
// and leaves the pair's output a plain copy of its style.
#include "common.h"
#include "device_utils.h"

namespace adain {

namespace {

constexpr int CO_THREADS = 256;
constexpr int CO_GROUP = 4;                  // consecutive pixels a thread takes at a time
constexpr int CO_GROUPS_PER_THREAD = 4;      // sizes the grid: 4096 pixels per workgroup ...
constexpr int CO_MAX_BLOCKS = 256;           // ... up to this many (a 1080p frame: 8 groups per thread)
constexpr int CO_SUMS = 9;                   // sum x (3), sum x x^T (00, 01, 02, 11, 12, 22)

int moment_blocks(size_t hw) {
    const size_t per_block = (size_t)CO_THREADS * CO_GROUP * CO_GROUPS_PER_THREAD;
    const size_t b = (hw + per_block - 1) / per_block;
    return (int)(b < 1 ? 1 : (b > (size_t)CO_MAX_BLOCKS ? (size_t)CO_MAX_BLOCKS : b));
}

template <class T>
__device__ __forceinline__ void add_sums(T m[CO_SUMS], T r, T g, T b) {
    m[0] += r; m[1] += g; m[2] += b;
    m[3] += r * r; m[4] += r * g; m[5] += r * b;
    m[6] += g * g; m[7] += g * b; m[8] += b * b;
}

// a workgroup's sums -> partial[CO_SUMS]: butterfly inside each wave, then the waves in index order
template <class T>
__device__ __forceinline__ void block_sums(T m[CO_SUMS], T* __restrict__ partial) {
    __shared__ T sh[CO_THREADS / 64][CO_SUMS];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
    for (int k = 0; k < CO_SUMS; ++k) {
        T v = m[k];
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
        if (lane == 0) sh[wave][k] = v;
    }
    __syncthreads();
    if (threadIdx.x < CO_SUMS) {
        T t = 0;
        for (int wv = 0; wv < CO_THREADS / 64; ++wv) t += sh[wv][threadIdx.x];
        partial[threadIdx.x] = t;
    }
}

// uint8 HWC images [k][hw][3]; partial [k][gridDim.x][CO_SUMS] unsigned 64-bit.  The pixels from the first 4-byte aligned pixel
// address on go 4 at a time as 3 dwords; the up to 3 pixels in front and behind are workgroup 0's (integer sums: the split is free).
__global__ __launch_bounds__(CO_THREADS) void coral_moments_u8_kernel(const uint8_t* __restrict__ img, int hw, unsigned long long* __restrict__ partial) {
    const uint8_t* __restrict__ p = img + (size_t)blockIdx.y * hw * 3;
    const int head = min((int)((uintptr_t)p & 3), hw);        // (p + 3 head) % 4 == 0
    const int groups = (hw - head) / CO_GROUP;
    unsigned long long m[CO_SUMS] = {};
    const uint32_t* __restrict__ q = (const uint32_t*)(p + 3 * head);
    for (int g = blockIdx.x * CO_THREADS + threadIdx.x; g < groups; g += gridDim.x * CO_THREADS) {
        const uint32_t w[3] = {q[3 * (size_t)g], q[3 * (size_t)g + 1], q[3 * (size_t)g + 2]};
        unsigned s[CO_SUMS] = {};                             // 4 pixels: at most 4 x 255^2
#pragma unroll
        for (int k = 0; k < CO_GROUP; ++k) {
            const int e = 3 * k;
            add_sums(s, (w[e >> 2] >> (8 * (e & 3))) & 255u, (w[(e + 1) >> 2] >> (8 * ((e + 1) & 3))) & 255u,
                     (w[(e + 2) >> 2] >> (8 * ((e + 2) & 3))) & 255u);
        }
#pragma unroll
        for (int k = 0; k < CO_SUMS; ++k) m[k] += s[k];
    }
    if (blockIdx.x == 0 && threadIdx.x < 2 * (CO_GROUP - 1)) {
        const int t = threadIdx.x, tail0 = head + groups * CO_GROUP;
        const int px = t < CO_GROUP - 1 ? (t < head ? t : -1) : (tail0 + t - (CO_GROUP - 1) < hw ? tail0 + t - (CO_GROUP - 1) : -1);
        if (px >= 0) add_sums(m, (unsigned long long)p[3 * (size_t)px], (unsigned long long)p[3 * (size_t)px + 1], (unsigned long long)p[3 * (size_t)px + 2]);
    }
    block_sums(m, partial + ((size_t)blockIdx.y * gridDim.x + blockIdx.x) * CO_SUMS);
}

// float NCHW images [k][3][hw]; partial [k][gridDim.x][CO_SUMS] float64 sums of (x - first pixel).  Group g is pixels 4g .. 4g + 3
// whatever the planes' alignment; an aligned full group is one 16-byte load per plane.
__global__ __launch_bounds__(CO_THREADS) void coral_moments_f32_kernel(const float* __restrict__ img, int hw, double* __restrict__ partial) {
    const float* __restrict__ p = img + (size_t)blockIdx.y * 3 * hw;
    const double k0 = (double)p[0], k1 = (double)p[hw], k2 = (double)p[2 * (size_t)hw];
    const bool aligned = (((uintptr_t)p | (uintptr_t)(p + hw) | (uintptr_t)(p + 2 * (size_t)hw)) & 15) == 0;
    const int groups = (hw + CO_GROUP - 1) / CO_GROUP;
    double m[CO_SUMS] = {};
    for (int g = blockIdx.x * CO_THREADS + threadIdx.x; g < groups; g += gridDim.x * CO_THREADS) {
        const int i0 = g * CO_GROUP, cnt = min(CO_GROUP, hw - i0);
        float x[3][CO_GROUP];
        if (aligned && cnt == CO_GROUP) {
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                const f32x4 v = *(const f32x4*)(p + (size_t)c * hw + i0);
                x[c][0] = v.x; x[c][1] = v.y; x[c][2] = v.z; x[c][3] = v.w;
            }
        } else {
#pragma unroll
            for (int c = 0; c < 3; ++c)
#pragma unroll
                for (int k = 0; k < CO_GROUP; ++k) x[c][k] = k < cnt ? p[(size_t)c * hw + i0 + k] : 0.f;
        }
#pragma unroll
        for (int k = 0; k < CO_GROUP; ++k)
            if (k < cnt) add_sums(m, (double)x[0][k] - k0, (double)x[1][k] - k1, (double)x[2][k] - k2);
    }
    block_sums(m, partial + ((size_t)blockIdx.y * gridDim.x + blockIdx.x) * CO_SUMS);
}

// |a * b - c * d| and its sign for a, b, c, d < 2^63 as a float64 (two roundings): the products are up to 2^78 for the largest image
__device__ double diff_of_products(unsigned long long a, unsigned long long b, unsigned long long c, unsigned long long d) {
    const unsigned __int128 x = (unsigned __int128)a * b, y = (unsigned __int128)c * d;
    const bool neg = y > x;
    const unsigned __int128 z = neg ? y - x : x - y;
    const double v = (double)(unsigned long long)(z >> 64) * 18446744073709551616.0 + (double)(unsigned long long)z;
    return neg ? -v : v;
}

struct Side {
    const void* img;        // [k][hw][3] uint8 or [k][3][hw] float
    const void* partial;    // [k][blocks][CO_SUMS]
    int is_u8, k, hw, blocks;
};

// One side of pair `pair`: the record's counts, mean and deviation, and D = N sum x x^T - (sum x)(sum x)^T (the N (N - 1)-fold
// covariance; in byte units for uint8).  Called by a whole wave; every lane returns the same values.
__device__ void side_moments(const Side& s, int pair, adain_coral_side* __restrict__ out, double D[6]) {
    const int img = s.k == 1 ? 0 : pair, lane = threadIdx.x & 63;
    const size_t base = (size_t)img * s.blocks * CO_SUMS;
    unsigned long long iu[CO_SUMS];
    double fd[CO_SUMS];
    for (int q = 0; q < CO_SUMS; ++q) {
        if (s.is_u8) {
            unsigned long long v = 0;
            for (int b = lane; b < s.blocks; b += 64) v += ((const unsigned long long*)s.partial)[base + (size_t)b * CO_SUMS + q];
#pragma unroll
            for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
            iu[q] = v;
        } else {
            double v = 0;
            for (int b = lane; b < s.blocks; b += 64) v += ((const double*)s.partial)[base + (size_t)b * CO_SUMS + q];
#pragma unroll
            for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
            fd[q] = v;
        }
    }
    const double n = (double)s.hw;
    out->n = s.hw;
    // index of sum x_i x_j in the 6 second moments
    const int I[6] = {0, 0, 0, 1, 1, 2}, J[6] = {0, 1, 2, 1, 2, 2};
    double scale = 1.0;
    if (s.is_u8) {
        for (int c = 0; c < 3; ++c) { out->sum[c] = (int64_t)iu[c]; out->mean[c] = (double)iu[c] / (255.0 * n); }
        for (int q = 0; q < 6; ++q) {
            out->sum2[q] = (int64_t)iu[3 + q];
            D[q] = diff_of_products((unsigned long long)s.hw, iu[3 + q], iu[I[q]], iu[J[q]]);
        }
        scale = 1.0 / 255.0;
    } else {
        const float* p = (const float*)s.img + (size_t)img * 3 * s.hw;
        for (int c = 0; c < 3; ++c) { out->sum[c] = 0; out->mean[c] = (double)p[(size_t)c * s.hw] + fd[c] / n; }
        for (int q = 0; q < 6; ++q) {
            out->sum2[q] = 0;
            D[q] = n * fd[3 + q] - fd[I[q]] * fd[J[q]];
        }
    }
    const int diag[3] = {0, 3, 5};
    for (int c = 0; c < 3; ++c) out->std[c] = s.hw > 1 && D[diag[c]] > 0.0 ? scale * sqrt(D[diag[c]] / (n * (n - 1.0))) : 0.0;
}

// C = (N - 1) D_ij / sqrt(D_ii D_jj) + I (the diagonal is exactly N) -> its eigenpairs (lambda >= 1, the columns of v)
__device__ void correlation_eigen(const double D[6], int hw, double lambda[3], double v[3][3]) {
    const double n1 = (double)hw - 1.0;
    const double r01 = n1 * (D[1] / sqrt(D[0] * D[3])), r02 = n1 * (D[2] / sqrt(D[0] * D[5])), r12 = n1 * (D[4] / sqrt(D[3] * D[5]));
    double a[3][3] = {{n1 + 1.0, r01, r02}, {r01, n1 + 1.0, r12}, {r02, r12, n1 + 1.0}};
    jacobi3(a, v);
    for (int k = 0; k < 3; ++k) lambda[k] = fmax(a[k][k], 1.0);
}

// grid: one wave per pair
__global__ __launch_bounds__(64) void coral_matrix_kernel(Side style, Side content, adain_coral_record* __restrict__ records) {
    const int pair = blockIdx.x;
    adain_coral_record* __restrict__ rec = records + pair;
    double Ds[6], Dt[6];
    adain_coral_side S, T;
    side_moments(style, pair, &S, Ds);       // the whole wave: its lanes share the walk over the partial sums
    side_moments(content, pair, &T, Dt);
    if (threadIdx.x != 0) return;
    rec->style = S;
    rec->content = T;
    int status = 0;
    if (style.hw < 2) status |= ADAIN_CORAL_STYLE_SINGLE;
    else if (!(Ds[0] > 0.0 && Ds[3] > 0.0 && Ds[5] > 0.0)) status |= ADAIN_CORAL_STYLE_FLAT;
    if (content.hw < 2) status |= ADAIN_CORAL_CONTENT_SINGLE;
    else if (!(Dt[0] > 0.0 && Dt[3] > 0.0 && Dt[5] > 0.0)) status |= ADAIN_CORAL_CONTENT_FLAT;
    rec->status = status;
    rec->reserved = 0;
    if (status) {
        for (int i = 0; i < 3; ++i) {
            rec->b[i] = 0.0;
            for (int j = 0; j < 3; ++j) rec->A[3 * i + j] = i == j ? 1.0 : 0.0;
        }
        return;
    }
    double ls[3], lt[3], vs[3][3], vt[3][3];
    correlation_eigen(Ds, style.hw, ls, vs);
    correlation_eigen(Dt, content.hw, lt, vt);
    double rt_[3][3], inv[3][3];          // sqrt(C_content), inverse(sqrt(C_style))
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j) {
            double a = 0.0, b = 0.0;
            for (int k = 0; k < 3; ++k) {
                a += vt[i][k] * sqrt(lt[k]) * vt[j][k];
                b += vs[i][k] / sqrt(ls[k]) * vs[j][k];
            }
            rt_[i][j] = a;
            inv[i][j] = b;
        }
    for (int i = 0; i < 3; ++i) {
        double bi = T.mean[i];
        for (int j = 0; j < 3; ++j) {
            double m = 0.0;
            for (int k = 0; k < 3; ++k) m += rt_[i][k] * inv[k][j];
            const double a = T.std[i] * m / S.std[j];
            rec->A[3 * i + j] = a;
            bi -= a * S.mean[j];
        }
        rec->b[i] = bi;
    }
}

// grid (groups of 4 style pixels / CO_THREADS, pairs); out NCHW [pairs][3][hw]
template <bool U8>
__global__ __launch_bounds__(CO_THREADS) void coral_apply_kernel(const void* __restrict__ style, int style_k, int hw,
                                                                const adain_coral_record* __restrict__ records, float* __restrict__ out) {
    const int pair = blockIdx.y, img = style_k == 1 ? 0 : pair;
    const int g = blockIdx.x * CO_THREADS + threadIdx.x, i0 = g * CO_GROUP;
    if (i0 >= hw) return;
    const int cnt = min(CO_GROUP, hw - i0);
    const adain_coral_record* __restrict__ rec = records + pair;
    float x[3][CO_GROUP];
    if (U8) {
        const uint8_t* __restrict__ p = (const uint8_t*)style + ((size_t)img * hw + i0) * 3;
        if (cnt == CO_GROUP && ((uintptr_t)p & 3) == 0) {
            const uint32_t* __restrict__ q = (const uint32_t*)p;
            const uint32_t w[3] = {q[0], q[1], q[2]};
#pragma unroll
            for (int e = 0; e < 3 * CO_GROUP; ++e) x[e % 3][e / 3] = __fdiv_rn((float)((w[e >> 2] >> (8 * (e & 3))) & 255u), 255.0f);
        } else {
#pragma unroll
            for (int k = 0; k < CO_GROUP; ++k)
#pragma unroll
                for (int c = 0; c < 3; ++c) x[c][k] = k < cnt ? __fdiv_rn((float)p[3 * k + c], 255.0f) : 0.f;
        }
    } else {
        const float* __restrict__ p = (const float*)style + (size_t)img * 3 * hw + i0;
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            const float* __restrict__ pc = p + (size_t)c * hw;
            if (cnt == CO_GROUP && ((uintptr_t)pc & 15) == 0) {
                const f32x4 v = *(const f32x4*)pc;
                x[c][0] = v.x; x[c][1] = v.y; x[c][2] = v.z; x[c][3] = v.w;
            } else {
#pragma unroll
                for (int k = 0; k < CO_GROUP; ++k) x[c][k] = k < cnt ? pc[k] : 0.f;
            }
        }
    }
    const bool copy = rec->status != 0;
    float* __restrict__ o = out + (size_t)pair * 3 * hw + i0;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        const double a0 = rec->A[3 * c], a1 = rec->A[3 * c + 1], a2 = rec->A[3 * c + 2], b = rec->b[c];
        float y[CO_GROUP];
#pragma unroll
        for (int k = 0; k < CO_GROUP; ++k)
            y[k] = copy ? x[c][k] : (float)(((a0 * (double)x[0][k] + a1 * (double)x[1][k]) + a2 * (double)x[2][k]) + b);
        float* __restrict__ oc = o + (size_t)c * hw;
        if (cnt == CO_GROUP && ((uintptr_t)oc & 15) == 0) {
            *(f32x4*)oc = f32x4{y[0], y[1], y[2], y[3]};
        } else {
#pragma unroll
            for (int k = 0; k < CO_GROUP; ++k)
                if (k < cnt) oc[k] = y[k];
        }
    }
}

struct Layout {
    int blocks_s, blocks_c;
    size_t records, partial_s, partial_c, total;
};

// false: a refused shape
bool layout(int n, int style_n, int hs, int ws, int hc, int wc, Layout* l) {
    if (n < 1 || n > 65535 || (style_n != 1 && style_n != n) || hs < 1 || ws < 1 || hc < 1 || wc < 1) return false;
    if ((size_t)hs * ws > 0x3fffffffULL || (size_t)hc * wc > 0x3fffffffULL) return false;
    l->blocks_s = moment_blocks((size_t)hs * ws);
    l->blocks_c = moment_blocks((size_t)hc * wc);
    Carve c;
    l->records = c.take((size_t)n * sizeof(adain_coral_record));
    l->partial_s = c.take((size_t)style_n * l->blocks_s * CO_SUMS * 8);
    l->partial_c = c.take((size_t)n * l->blocks_c * CO_SUMS * 8);
    l->total = c.at;
    return true;
}

void launch_moments(const void* img, int is_u8, int k, int hw, int blocks, void* partial, hipStream_t s) {
    if (is_u8)
        hipLaunchKernelGGL(coral_moments_u8_kernel, dim3(blocks, k), dim3(CO_THREADS), 0, s, (const uint8_t*)img, hw, (unsigned long long*)partial);
    else
        hipLaunchKernelGGL(coral_moments_f32_kernel, dim3(blocks, k), dim3(CO_THREADS), 0, s, (const float*)img, hw, (double*)partial);
}

}  // namespace

size_t coral_workspace_bytes(int n, int style_n, int hs, int ws, int hc, int wc) {
    Layout l;
    return layout(n, style_n, hs, ws, hc, wc, &l) ? l.total : 0;
}

int launch_coral(const void* style, int style_is_u8, int style_n, int hs, int ws, const void* content, int content_is_u8, int n, int hc, int wc,
                 float* out, void* workspace, size_t ws_bytes, hipStream_t s) {
    Layout l;
    if (!style || !content || !out || !workspace) { set_error("coral: null pointer"); return ADAIN_EINVAL; }
    if (!layout(n, style_n, hs, ws, hc, wc, &l)) {
        set_error("coral: unsupported shape: %d content image(s) %d x %d, %d style image(s) %d x %d (style_n is 1 or n; at most 65535 pairs, 2^30 - 1 pixels)",
                  n, hc, wc, style_n, hs, ws);
        return ADAIN_EINVAL;
    }
    if (int rc = check_workspace("coral", workspace, ws_bytes, l.total, 8)) return rc;
    if ((!style_is_u8 && (uintptr_t)style % 4) || (!content_is_u8 && (uintptr_t)content % 4) || (uintptr_t)out % 4) {
        set_error("coral: float images must be 4-byte aligned");
        return ADAIN_EINVAL;
    }
    char* base = (char*)workspace;
    auto* records = (adain_coral_record*)(base + l.records);
    const int hw_s = hs * ws, hw_c = hc * wc;
    launch_moments(style, style_is_u8, style_n, hw_s, l.blocks_s, base + l.partial_s, s);
    launch_moments(content, content_is_u8, n, hw_c, l.blocks_c, base + l.partial_c, s);
    hipLaunchKernelGGL(coral_matrix_kernel, dim3(n), dim3(64), 0, s, Side{style, base + l.partial_s, style_is_u8 ? 1 : 0, style_n, hw_s, l.blocks_s},
                       Side{content, base + l.partial_c, content_is_u8 ? 1 : 0, n, hw_c, l.blocks_c}, records);
    const dim3 grid((unsigned)(((size_t)hw_s + CO_GROUP * CO_THREADS - 1) / (CO_GROUP * CO_THREADS)), n);
    if (style_is_u8)
        hipLaunchKernelGGL(coral_apply_kernel<true>, grid, dim3(CO_THREADS), 0, s, style, style_n, hw_s, (const adain_coral_record*)records, out);
    else
        hipLaunchKernelGGL(coral_apply_kernel<false>, grid, dim3(CO_THREADS), 0, s, style, style_n, hw_s, (const adain_coral_record*)records, out);
    return check_launch("coral");
}

}  // namespace adain
