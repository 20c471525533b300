// Device-side helpers shared by the convolution kernels (conv_edge.hip, conv_wino4.hip) and the colour kernels (colour.hip, coral.hip);
// the workgroup scan and the bit writer of the file encoders (png.hip, gif.hip).
#pragma once
#include "common.h"

namespace adain {

__device__ __forceinline__ int reflect1(int v, int n) {
    // ReflectionPad2d(1) index map, after clamping to [-1, n] (tiles may overhang the image).
    v = max(-1, min(v, n));
    v = v < 0 ? -v : v;
    return v >= n ? 2 * n - 2 - v : v;
}

// element-wise max as ONE v_med3_f32 per element: max(a, b) = med3(a, b, +inf).  fmaxf costs three instructions here (a
// canonicalising v_max of each operand in front of the real one), and beside MFMAs every vector instruction counts.
__device__ __forceinline__ f32x4 max4(f32x4 a, f32x4 b) {
    f32x4 r;
    r.x = __builtin_amdgcn_fmed3f(a.x, b.x, __builtin_inff()); r.y = __builtin_amdgcn_fmed3f(a.y, b.y, __builtin_inff());
    r.z = __builtin_amdgcn_fmed3f(a.z, b.z, __builtin_inff()); r.w = __builtin_amdgcn_fmed3f(a.w, b.w, __builtin_inff());
    return r;
}

// Buffer-descriptor loads: 32-bit per-lane byte offset + scalar byte offset, hardware range check
// (out-of-range reads return 0), no 64-bit address arithmetic in the loop.
using rsrc_t = __amdgpu_buffer_rsrc_t;
using u32x4 = __attribute__((__vector_size__(4 * sizeof(unsigned int)))) unsigned int;

__device__ __forceinline__ rsrc_t make_rsrc(const void* base, unsigned bytes) {
    return __builtin_amdgcn_make_buffer_rsrc(const_cast<void*>(base), 0, bytes, 0x00020000);
}
__device__ __forceinline__ f32x4 buf_load4(rsrc_t r, int voff, int soff) {
    const u32x4 v = __builtin_amdgcn_raw_buffer_load_b128(r, voff, soff, 0);
    return __builtin_bit_cast(f32x4, v);
}

// Eigenvalues (the diagonal of a on return) and eigenvectors (the columns of v) of a symmetric 3 x 3 matrix: cyclic Jacobi.
__device__ inline void jacobi3(double a[3][3], double v[3][3]) {
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j) v[i][j] = i == j ? 1.0 : 0.0;
    for (int sweep = 0; sweep < 32; ++sweep) {
        if (fabs(a[0][1]) + fabs(a[0][2]) + fabs(a[1][2]) == 0.0) break;
        for (int p = 0; p < 2; ++p)
            for (int q = p + 1; q < 3; ++q) {
                const double apq = a[p][q];
                if (apq == 0.0) continue;
                const double g = 100.0 * fabs(apq);
                if (fabs(a[p][p]) + g == fabs(a[p][p]) && fabs(a[q][q]) + g == fabs(a[q][q])) {   // below the diagonal's rounding
                    a[p][q] = a[q][p] = 0.0;
                    continue;
                }
                const double theta = (a[q][q] - a[p][p]) / (2.0 * apq);
                const double t = (theta < 0.0 ? -1.0 : 1.0) / (fabs(theta) + sqrt(theta * theta + 1.0));
                const double c = 1.0 / sqrt(t * t + 1.0), s = t * c;
                for (int k = 0; k < 3; ++k) {
                    const double akp = a[k][p], akq = a[k][q];
                    a[k][p] = c * akp - s * akq;
                    a[k][q] = s * akp + c * akq;
                }
                for (int k = 0; k < 3; ++k) {
                    const double apk = a[p][k], aqk = a[q][k];
                    a[p][k] = c * apk - s * aqk;
                    a[q][k] = s * apk + c * aqk;
                }
                a[p][q] = a[q][p] = 0.0;
                for (int k = 0; k < 3; ++k) {
                    const double vkp = v[k][p], vkq = v[k][q];
                    v[k][p] = c * vkp - s * vkq;
                    v[k][q] = s * vkp + c * vkq;
                }
            }
    }
}

// exclusive prefix of v over the workgroup's THREADS threads; *total: the sum; part: THREADS / 64 entries of LDS (png.hip, gif.hip)
template <int THREADS, class V>
__device__ __forceinline__ V wg_exclusive(V v, V* part, V* total) {
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    V inc = v;
    for (int d = 1; d < 64; d <<= 1) {
        const V up = __shfl_up(inc, d);
        if (lane >= d) inc += up;
    }
    __syncthreads();
    if (lane == 63) part[wv] = inc;
    __syncthreads();
    V before = 0, all = 0;
    for (int k = 0; k < THREADS / 64; ++k) {
        if (k < wv) before += part[k];
        all += part[k];
    }
    *total = all;
    return before + inc - v;
}

// LSB-first bits into a zeroed stream of 32-bit words, shared between writers by atomicOr (png.hip, gif.hip)
struct BitWriter {
    uint32_t* words;
    size_t at;              // word being filled
    uint64_t acc;
    int have;               // bits of acc that belong to words[at] and the one behind it
    __device__ BitWriter(uint32_t* stream, uint64_t bit) : words(stream), at((size_t)(bit >> 5)), acc(0), have((int)(bit & 31)) {}
    __device__ void put(uint32_t value, int count) {          // count <= 32
        acc |= (uint64_t)value << have;
        have += count;
        if (have >= 32) {
            atomicOr(words + at, (uint32_t)acc);
            acc >>= 32, have -= 32, ++at;
        }
    }
    __device__ void flush() {
        if (have > 0 && acc) atomicOr(words + at, (uint32_t)acc);
    }
};

}  // namespace adain
