// Pixel-art palette control (the reference's gui/second_page.py, MainWindow._convert_image and its helpers) on finished uint8 frames:
// grey, brightness / contrast, nearest-colour recolouring and Floyd-Steinberg error diffusion.  Restated in tests/palette_ref.py.
//
// Frames are HWC uint8 [n][h][w][3] at any byte address; the palette is K x 3 uint8, 1 <= K <= 256, held in LDS.
//
// tone (the prologue of every kernel here, and a kernel of its own):
//   grey : Pillow's convert("L").convert("RGB"): L = (19595 R + 38470 G + 7471 B + 0x8000) >> 16 in all three channels
//   lut  : uint8 [3][256], channel c becomes lut[c][value] - _adjust_brightness_and_contrast is a function of the channel value alone,
//          so the host evaluates the reference's float64 expression on 0..255 once and the device looks it up
//   grey runs first, as _convert_image orders them.
// palette_map, integer arithmetic, the lowest index among equal distances:
//   metric 0 "rgb"     : sum_c ((p_c - P_kc) & 255)^2 - _recolor_image subtracts uint8 from uint8, so every difference wraps
//   metric 1 "nearest" : sum_c (p_c - P_kc)^2         - _recolor_image_kd, and what _recolor_image_floyd computes (its error is
//                        taken through a view of the pixel it has just overwritten, so it diffuses nothing)
// palette_dither, _recolor_image_floyd's loop as its lines describe it (the error copied before the pixel is overwritten), float32, this
// file compiles with -ffp-contract=off:
//   v   = ((((p + e[y-1][x-1] * 1/16) + e[y-1][x] * 5/16) + e[y-1][x+1] * 3/16) + e[y][x-1] * 7/16), every product rounded before
//         its add, terms outside the frame left out (a zero error stands for them: v + 0 is v); v is NOT clamped
//   t_k = sqrt_rn((d0 d0 + d1 d1) + d2 d2), d = P_k - v; the entry is the first k with the smallest t_k (np.linalg.norm, np.argmin).
//         The square root merges neighbouring sums, so t is what is compared; a sum that is not below the best one's cannot give a
//         smaller root and is skipped before its root is taken.
//   e   = v - P_k; the output pixel is P_k.
// One workgroup per frame, one thread per row of a band of PALETTE_DITHER_BAND rows; row y runs two columns behind row y - 1, so that
// at step s thread r works on column s - 2 r and the error row r - 1 produced one step earlier is the column to its upper right.  That
// value moves down by a lane shuffle inside a wave and through LDS from a wave's last lane to the next wave's first; a thread keeps the
// three upper errors and its own left one in registers.  A band's last row leaves its errors ([w][3] float) in the workspace, the next
// band's first row reads them; a column is read 2 (band - 1) + 1 steps before it is rewritten.  Every thread runs w + 2 (rows - 1)
// steps of a band and meets every barrier; nothing spins, no flag, no atomic, and a frame depends on neither n, the stream nor what
// the workspace held.
#include "common.h"

namespace adain {
namespace {

constexpr int BAND = ADAIN_PALETTE_DITHER_BAND;
constexpr int WAVES = BAND / 64;
static_assert(BAND % 64 == 0 && BAND <= 1024, "a band is whole waves of one workgroup");

__device__ __forceinline__ void tone_px(unsigned& r, unsigned& g, unsigned& b, const uint8_t* __restrict__ lut, int grey) {
    if (grey) r = g = b = (19595u * r + 38470u * g + 7471u * b + 0x8000u) >> 16;
    if (lut) r = lut[r], g = lut[256 + g], b = lut[512 + b];
}

// the tables of a workgroup: the palette's channels as int, the LUT (when there is one)
__device__ __forceinline__ void stage_lut(const uint8_t* __restrict__ lut, uint8_t* slut, int threads) {
    if (lut)
        for (int i = threadIdx.x; i < 768; i += threads) slut[i] = lut[i];
}

template <int METRIC>
__device__ __forceinline__ unsigned nearest(const int* spal, int K, int r, int g, int b) {
    unsigned best = 0xffffffffu, kb = 0;
    for (int k = 0; k < K; ++k) {
        int d0 = r - spal[3 * k], d1 = g - spal[3 * k + 1], d2 = b - spal[3 * k + 2];
        if (METRIC == 0) d0 &= 255, d1 &= 255, d2 &= 255;
        const unsigned s = (unsigned)(d0 * d0 + d1 * d1 + d2 * d2);
        if (s < best) best = s, kb = (unsigned)k;          // strict: the lowest index among equals
    }
    return kb;
}

// total pixels of all frames, 4 per thread (VEC4: total % 4 == 0, src / out / index 4-byte aligned) or one.  A grid-stride walk: a launch
// holds fewer than 2^32 threads (MAP_MAX_BLOCKS workgroups), a batch may hold more pixels than that.
template <int METRIC, bool VEC4>
__global__ __launch_bounds__(256) void palette_map_kernel(const uint8_t* __restrict__ src, size_t total, const uint8_t* __restrict__ pal, int K,
                                                          const uint8_t* __restrict__ lut, int grey, uint8_t* __restrict__ out,
                                                          uint8_t* __restrict__ index) {
    __shared__ int spal[256 * 3];
    __shared__ uint8_t slut[768];
    for (int i = threadIdx.x; i < 3 * K; i += 256) spal[i] = pal[i];
    stage_lut(lut, slut, 256);
    __syncthreads();
    const uint8_t* l = lut ? slut : nullptr;
    const size_t units = VEC4 ? total / 4 : total, stride = (size_t)gridDim.x * 256;
    for (size_t q = (size_t)blockIdx.x * 256 + threadIdx.x; q < units; q += stride) {
        if (VEC4) {
            using u32x3 = __attribute__((ext_vector_type(3))) unsigned;
            const u32x3 in = *(const u32x3*)(src + q * 12);
            unsigned by[12], idx = 0;
#pragma unroll
            for (int e = 0; e < 12; ++e) by[e] = (in[e >> 2] >> (8 * (e & 3))) & 255u;
#pragma unroll
            for (int p = 0; p < 4; ++p) {
                tone_px(by[3 * p], by[3 * p + 1], by[3 * p + 2], l, grey);
                const unsigned k = nearest<METRIC>(spal, K, (int)by[3 * p], (int)by[3 * p + 1], (int)by[3 * p + 2]);
                by[3 * p] = (unsigned)spal[3 * k], by[3 * p + 1] = (unsigned)spal[3 * k + 1], by[3 * p + 2] = (unsigned)spal[3 * k + 2];
                idx |= k << (8 * p);
            }
            u32x3 o;
#pragma unroll
            for (int d = 0; d < 3; ++d) o[d] = by[4 * d] | (by[4 * d + 1] << 8) | (by[4 * d + 2] << 16) | (by[4 * d + 3] << 24);
            *(u32x3*)(out + q * 12) = o;
            if (index) *(unsigned*)(index + q * 4) = idx;
        } else {
            unsigned r = src[q * 3], g = src[q * 3 + 1], b = src[q * 3 + 2];
            tone_px(r, g, b, l, grey);
            const unsigned k = nearest<METRIC>(spal, K, (int)r, (int)g, (int)b);
            out[q * 3] = (uint8_t)spal[3 * k], out[q * 3 + 1] = (uint8_t)spal[3 * k + 1], out[q * 3 + 2] = (uint8_t)spal[3 * k + 2];
            if (index) index[q] = (uint8_t)k;
        }
    }
}

// one thread per pixel; src may be out (every pixel is read and written by its own thread)
__global__ __launch_bounds__(256) void tone_kernel(const uint8_t* src, size_t total, const uint8_t* __restrict__ lut, int grey, uint8_t* out) {
    __shared__ uint8_t slut[768];
    stage_lut(lut, slut, 256);
    __syncthreads();
    for (size_t q = (size_t)blockIdx.x * 256 + threadIdx.x; q < total; q += (size_t)gridDim.x * 256) {          // as palette_map_kernel walks
        unsigned r = src[q * 3], g = src[q * 3 + 1], b = src[q * 3 + 2];
        tone_px(r, g, b, lut ? slut : nullptr, grey);
        out[q * 3] = (uint8_t)r, out[q * 3 + 1] = (uint8_t)g, out[q * 3 + 2] = (uint8_t)b;
    }
}

// the exchange of a step needs the LDS writes only: the frame's own loads and stores stay in flight across it
__device__ __forceinline__ void step_barrier() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup", "local");
    __builtin_amdgcn_s_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup", "local");
}

// grid n, BAND threads; carry: [n][w][3] float
__global__ __launch_bounds__(BAND) void palette_dither_kernel(const uint8_t* __restrict__ src, int h, int w, const uint8_t* __restrict__ pal, int K,
                                                              const uint8_t* __restrict__ lut, int grey, uint8_t* __restrict__ out,
                                                              uint8_t* __restrict__ index, float* carry_all) {
    __shared__ float spal[256 * 3];
    __shared__ uint8_t slut[768];
    __shared__ float cross[2][WAVES][3];          // [step parity][wave]: the error its last lane produced in that step
    const int r = threadIdx.x, lane = r & 63, wave = r >> 6;
    const size_t f = blockIdx.x;
    for (int i = r; i < 3 * K; i += BAND) spal[i] = (float)pal[i];
    stage_lut(lut, slut, BAND);
    __syncthreads();
    const uint8_t* l = lut ? slut : nullptr;
    float* carry = carry_all + f * (size_t)w * 3;
    const uint8_t* sf = src + f * (size_t)h * w * 3;
    uint8_t* of = out + f * (size_t)h * w * 3;
    uint8_t* xf = index ? index + f * (size_t)h * w : nullptr;

    for (int y0 = 0; y0 < h; y0 += BAND) {
        const int rows = h - y0 < BAND ? h - y0 : BAND;
        const int steps = w + 2 * (rows - 1);
        const bool row = r < rows, from_carry = r == 0 && y0 > 0, to_carry = r == rows - 1 && y0 + rows < h;
        const size_t y = (size_t)y0 + r;
        const uint8_t* sp = sf + y * w * 3;       // formed for every thread, dereferenced only under `row`
        uint8_t* op = of + y * w * 3;
        // the errors above columns x - 1, x, x + 1, the one to the left, and this thread's of the previous step (what the row below takes)
        float um[3] = {0.f, 0.f, 0.f}, u0[3] = {0.f, 0.f, 0.f}, up[3] = {0.f, 0.f, 0.f}, el[3] = {0.f, 0.f, 0.f}, mine[3] = {0.f, 0.f, 0.f};
        // read one step ahead, so that neither load's latency lies between two barriers: the carry row's next column (first row of a
        // later band only) and the row's next pixel
        float pre[3] = {0.f, 0.f, 0.f};
        unsigned nxt[3] = {0u, 0u, 0u};
        if (from_carry)
            for (int c = 0; c < 3; ++c) {
                up[c] = carry[c];          // column 0: the step-0 shift below makes it u0
                if (w > 1) pre[c] = carry[3 + c];
            }
        if (r == 0)          // its first step is column 0; every other row passes column -1 first and loads there
            for (int c = 0; c < 3; ++c) nxt[c] = sp[c];
        for (int s = 0; s < steps; ++s) {
            const int x = s - 2 * r;
            float a[3];
#pragma unroll
            for (int c = 0; c < 3; ++c) a[c] = __shfl_up(mine[c], 1);
            if (lane == 0) {
#pragma unroll
                for (int c = 0; c < 3; ++c) a[c] = (wave > 0 && s > 0) ? cross[(s - 1) & 1][wave - 1][c] : 0.f;
            }
            if (r == 0) {          // x = s: column x + 1 was loaded a step ago, column x + 2 is for the next step
#pragma unroll
                for (int c = 0; c < 3; ++c) {
                    a[c] = pre[c];
                    pre[c] = (from_carry && x + 2 < w) ? carry[(size_t)(x + 2) * 3 + c] : 0.f;
                }
            }
            const unsigned cur[3] = {nxt[0], nxt[1], nxt[2]};
            if (row && x + 1 >= 0 && x + 1 < w) {
#pragma unroll
                for (int c = 0; c < 3; ++c) nxt[c] = sp[(size_t)(x + 1) * 3 + c];
            }
#pragma unroll
            for (int c = 0; c < 3; ++c) um[c] = u0[c], u0[c] = up[c], up[c] = a[c];
            float e[3] = {0.f, 0.f, 0.f};
            if (row && x >= 0 && x < w) {
                unsigned p0 = cur[0], p1 = cur[1], p2 = cur[2];
                tone_px(p0, p1, p2, l, grey);
                float v[3] = {(float)p0, (float)p1, (float)p2};
#pragma unroll
                for (int c = 0; c < 3; ++c)
                    v[c] = (((v[c] + um[c] * 0.0625f) + u0[c] * 0.3125f) + up[c] * 0.1875f) + el[c] * 0.4375f;
                float sb = __builtin_inff(), tb = __builtin_inff();
                int kb = 0;
                for (int k = 0; k < K; ++k) {
                    const float d0 = spal[3 * k] - v[0], d1 = spal[3 * k + 1] - v[1], d2 = spal[3 * k + 2] - v[2];
                    const float q = (d0 * d0 + d1 * d1) + d2 * d2;
                    if (q < sb) {                 // sqrt_rn is monotone: q >= sb cannot give a root below tb
                        const float t = sqrtf(q);          // the correctly rounded root (v_sqrt_f32 alone, which __fsqrt_rn compiles to, is within 1 ulp)
                        if (t < tb) tb = t, sb = q, kb = k;
                    }
                }
#pragma unroll
                for (int c = 0; c < 3; ++c) {
                    const float P = spal[3 * kb + c];
                    e[c] = v[c] - P;
                    op[(size_t)x * 3 + c] = (uint8_t)P;
                }
                if (xf) xf[y * w + x] = (uint8_t)kb;
                if (to_carry)
                    for (int c = 0; c < 3; ++c) carry[(size_t)x * 3 + c] = e[c];
            }
#pragma unroll
            for (int c = 0; c < 3; ++c) el[c] = mine[c] = e[c];
            if (lane == 63) {
#pragma unroll
                for (int c = 0; c < 3; ++c) cross[s & 1][wave][c] = e[c];
            }
            step_barrier();
        }
        __syncthreads();          // the band's carry row, written to memory, is the next band's upper row
    }
}

// 2^32 - 256 threads: a launch's threads per dimension are a 32-bit count, and 2^32 or more of them are not refused by the runtime
// but cut to their low 32 bits (a batch of 65535 frames of 257 x 259 pixels then left every frame from the 1010th on unwritten)
constexpr size_t MAP_MAX_BLOCKS = 0xffffff;

const char* check_palette_shape(int n, int h, int w, int K) {
    if (n < 1 || n > 65535) return "n outside 1..65535";
    if (h < 1 || w < 1) return "height or width below 1";
    if (K < 1 || K > 256) return "K outside 1..256";
    if ((size_t)h * w * 3 > (size_t)INT32_MAX) return "a frame beyond 2^31 - 1 bytes";
    return nullptr;
}

}  // namespace

int launch_palette_map_u8(const uint8_t* src, int n, int h, int w, const uint8_t* palette, int K, int metric, const uint8_t* lut, int grey, uint8_t* out,
                          uint8_t* index, hipStream_t s) {
    const char* who = "palette_map_u8";
    if (!src) { set_error("%s: src is a null pointer", who); return ADAIN_EINVAL; }
    if (!palette) { set_error("%s: palette is a null pointer", who); return ADAIN_EINVAL; }
    if (!out) { set_error("%s: out is a null pointer", who); return ADAIN_EINVAL; }
    const char* bad = check_palette_shape(n, h, w, K);
    if (!bad && metric != 0 && metric != 1) bad = "metric other than 0 (rgb) and 1 (nearest)";
    if (bad) { set_error("%s: %s (n %d, %d x %d, K %d, metric %d)", who, bad, n, h, w, K, metric); return ADAIN_EINVAL; }
    const size_t total = (size_t)n * h * w;
    const bool vec = total % 4 == 0 && (((uintptr_t)src | (uintptr_t)out | (uintptr_t)index) & 3) == 0;
    const size_t blocks = (total / (vec ? 4 : 1) + 255) / 256;
    const dim3 g((unsigned)(blocks < MAP_MAX_BLOCKS ? blocks : MAP_MAX_BLOCKS));
    grey = grey ? 1 : 0;
    if (metric == 0) {
        if (vec) palette_map_kernel<0, true><<<g, 256, 0, s>>>(src, total, palette, K, lut, grey, out, index);
        else palette_map_kernel<0, false><<<g, 256, 0, s>>>(src, total, palette, K, lut, grey, out, index);
    } else {
        if (vec) palette_map_kernel<1, true><<<g, 256, 0, s>>>(src, total, palette, K, lut, grey, out, index);
        else palette_map_kernel<1, false><<<g, 256, 0, s>>>(src, total, palette, K, lut, grey, out, index);
    }
    return check_launch(who);
}

int launch_tone_u8(const uint8_t* src, int n, int h, int w, const uint8_t* lut, int grey, uint8_t* out, hipStream_t s) {
    const char* who = "tone_u8";
    if (!src) { set_error("%s: src is a null pointer", who); return ADAIN_EINVAL; }
    if (!out) { set_error("%s: out is a null pointer", who); return ADAIN_EINVAL; }
    if (const char* bad = check_palette_shape(n, h, w, 1)) { set_error("%s: %s (n %d, %d x %d)", who, bad, n, h, w); return ADAIN_EINVAL; }
    const size_t total = (size_t)n * h * w, blocks = (total + 255) / 256;
    tone_kernel<<<dim3((unsigned)(blocks < MAP_MAX_BLOCKS ? blocks : MAP_MAX_BLOCKS)), 256, 0, s>>>(src, total, lut, grey ? 1 : 0, out);
    return check_launch(who);
}

int palette_dither_bytes(int n, int h, int w, size_t* workspace_bytes) {
    if (const char* bad = check_palette_shape(n, h, w, 1)) { set_error("palette_dither_u8: %s (n %d, %d x %d)", bad, n, h, w); return ADAIN_EINVAL; }
    Carve c;
    c.take((size_t)n * w * 3 * sizeof(float));          // per frame the error row between two bands
    if (workspace_bytes) *workspace_bytes = c.at;
    return 0;
}

int launch_palette_dither_u8(const uint8_t* src, int n, int h, int w, const uint8_t* palette, int K, const uint8_t* lut, int grey, uint8_t* out, uint8_t* index,
                             void* workspace, size_t workspace_bytes, hipStream_t s) {
    const char* who = "palette_dither_u8";
    if (!src) { set_error("%s: src is a null pointer", who); return ADAIN_EINVAL; }
    if (!palette) { set_error("%s: palette is a null pointer", who); return ADAIN_EINVAL; }
    if (!out) { set_error("%s: out is a null pointer", who); return ADAIN_EINVAL; }
    if (const char* bad = check_palette_shape(n, h, w, K)) { set_error("%s: %s (n %d, %d x %d, K %d)", who, bad, n, h, w, K); return ADAIN_EINVAL; }
    size_t need = 0;
    palette_dither_bytes(n, h, w, &need);
    if (int rc = check_workspace(who, workspace, workspace_bytes, need, 8)) return rc;
    palette_dither_kernel<<<n, BAND, 0, s>>>(src, h, w, palette, K, lut, grey ? 1 : 0, out, index, (float*)workspace);
    return check_launch(who);
}

}  // namespace adain
