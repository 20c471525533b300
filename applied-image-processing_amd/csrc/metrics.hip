// Image quality metrics on the device (gfx950): per frame SSIM, MSE, L1 and PSNR of two clips that are already there - what the modelled
// project's Style_3DGS/metrics.py computes per view with utils/loss_utils.py ssim and utils/image_utils.py psnr, and train.py's ssim against
// the stylised guide views.  The rules, restated in float64 in tests/metrics_ref.py:
//
//   1. Window.  g = gaussian(11, 1.5): exp(-(x - 5)^2 / 4.5), x = 0..10, as float32, divided by its float32 sum (SSIM_WINDOW below holds
//      the reference's bits).  The reference convolves with the 2-D window g g^T; here the window is applied as a row pass and a column
//      pass of 11 taps each, float32.  The two forms round differently, by less than the reference's own distance from float64.
//   2. Padding.  Samples outside the image are zero; the window is not renormalised at the border.
//   3. Map.  Per sample and channel mu1 = E[x], mu2 = E[y], s1 = E[x^2] - mu1^2, s2 = E[y^2] - mu2^2, s12 = E[xy] - mu1 mu2 and
//      map = ((2 mu1 mu2 + C1)(2 s12 + C2)) / ((mu1^2 + mu2^2 + C1)(s1 + s2 + C2)), C1 = 0.01^2, C2 = 0.03^2, float32.  The file is
//      built without FMA contraction and both inputs run one instruction sequence, so with x == y numerator and denominator are the same
//      number and the map is exactly 1.
//   4. Records.  ssim = the float64 sum of the frame's map values / their count.  uint8 input is scaled as to_tensor does, float(x) /
//      255.0f by a division; its error terms are exact integers: mse = sum (a - b)^2 / (count 255^2), l1 = sum |a - b| / (count 255), one
//      float64 division each.  float input: float64 sums of the float32 differences' squares and magnitudes / count.  psnr =
//      20 log10(1 / sqrt(mse)), +inf at mse == 0.
//
// One view for both layouts: a frame is `planes` planes of H rows of Wp samples whose window taps lie `cs` samples apart.  Packed HWC
// uint8 [h][w][c] is one plane of Wp = w c samples with cs = c; NCHW float32 is c planes of Wp = w samples with cs = 1.  The map has the
// input's layout.
//
// Stages (2 launches, whatever n; nothing allocates or waits):
//   tile   : a workgroup owns TILE_X x TILE_Y samples of one plane.  It stages them and a halo of 5 rows and 5 cs samples of both inputs
//            in LDS as float32, zeros outside the plane; runs the row pass for the five quantities into LDS and the column pass from
//            there, four rows of one column to a thread; evaluates the map, writes it if asked, and reduces the map values (float64) and
//            the error terms (64-bit integers or float64) over the workgroup in a fixed order: a butterfly over each wave's lanes, then
//            the waves in index order.  One partial record per tile goes into the workspace; every record is written by every call.
//   finish : a wave per frame adds the frame's partial records in index order and writes the frame's double[4].
// No float atomics, spin-waits or flags: a frame's record is a function of its pixels alone.
//
// The gradient (adain_image_metrics_grad_f32: what autograd hands back through train.py's (1 - lambda) l1_loss + lambda (1 - ssim)),
// restated in float64 in tests/metrics_grad_ref.py.  With A = 2 mu1 mu2 + C1, B = 2 s12 + C2, D = mu1^2 + mu2^2 + C1, E = s1 + s2 + C2,
// map = A B / (D E), the map's derivatives by the five window statistics are
//      d_mu1 = 2 mu2 (B - A) / (D E) - map (2 mu1 / D - 2 mu1 / E),   d_e11 = d_e22 = -map / E,   d_e12 = 2 A / (D E)
// (d_mu2: mu1 and mu2 swapped), and because the window is symmetric and the padding is zeros, the convolution is its own adjoint:
//      d ssim / d x = (conv(d_mu1) + 2 x conv(d_e11) + y conv(d_e12)) / count,
// to which mse adds 2 (x - y) / count and l1 sign(x - y) / count, sign(0) = 0.  The call recomputes the statistics from a and b.
//   planes  : the tile pass above with another tail: in place of the records it writes the derivative planes of its samples into the
//             workspace, float32 in the inputs' layout: d_mu1, d_e11, d_e12, and for the gradient of b d_mu2, d_e22 as well.  They are
//             written as p = A / D, q = B / E, d_mu1 = 2 ((mu2 q - mu1 p q) / D - (mu2 p - mu1 p q) / E), d_e11 = -(p q) / E, d_e12 =
//             2 p / E: A, B, D, E, p and q are the same numbers with the inputs swapped, and with x == y p = q = 1, so d_mu1 = 0 and
//             d_e12 = -2 d_e11 exactly.
//   combine : the same tile geometry; stages three planes with a halo of 5 (zeros outside the frame), row pass, column pass, then
//             grad = ((c_mu + (2 x) c_11) + y c_12) (float)(w_ssim / count) + (x - y) (float)(2 w_mse / count) + sign (float)(w_l1 / count).
//             The gradient of b is a second pass over d_mu2, d_e22, d_e12 with the inputs swapped.
// Held: a frame's gradient bits are a function of its two frames and its three weights alone (not of n, the frame's index, the stream
// or what the workspace held: every plane sample a combine pass reads was written by the same call's planes pass); a frame whose
// weights are all zero gets zeros of either sign (a zero ssim weight skips both passes for the frame); grad_b(a, b) is bit for bit
// grad_a(b, a), and grad_a is the same with and without grad_b; equal frames get exactly zero from the ssim term.
#include "common.h"

namespace adain {
namespace {

typedef unsigned long long ull;

constexpr int WIN = 11, HALO = WIN / 2;
// gaussian(11, 1.5) of utils/loss_utils.py: the reference's float32 bits (torch's sum of the eleven floats, not the sequential one)
constexpr float SSIM_WINDOW[WIN] = {0x1.0d956cp-10f, 0x1.f1fe02p-8f, 0x1.26eb18p-5f, 0x1.bff0fep-4f, 0x1.b43c3ep-3f, 0x1.10656p-2f,
                                    0x1.b43c3ep-3f,  0x1.bff0fep-4f, 0x1.26eb18p-5f, 0x1.f1fe02p-8f, 0x1.0d956cp-10f};
constexpr float C1 = 0.01f * 0.01f, C2 = 0.03f * 0.03f;

constexpr int TILE_X = ADAIN_METRICS_TILE_X, TILE_Y = ADAIN_METRICS_TILE_Y;
constexpr int THREADS = 256, ROWS_PER_THREAD = TILE_Y * TILE_X / THREADS;
constexpr int MAX_CS = 3;                                   // tap stride: the channels of packed uint8
constexpr int STAGE_Y = TILE_Y + 2 * HALO;                  // 26 rows
constexpr int STAGE_X = 96;                                 // row pitch of the staged inputs: TILE_X + 2 * HALO * MAX_CS = 94 at most
static_assert(TILE_X == 64 && THREADS == 4 * TILE_X && ROWS_PER_THREAD == 4, "a thread takes four rows of one column");
static_assert(TILE_X + 2 * HALO * MAX_CS <= STAGE_X, "the halo fits the pitch");

// what a tile leaves for the finish: the map sum, and the two error sums as integers (uint8) or as the bits of doubles (float32)
struct Partial {
    double ssim;
    ull se, ae;
};

struct Shared {
    float in[2][STAGE_Y][STAGE_X];                          // 19968 bytes
    float row[5][STAGE_Y][TILE_X];                          // 33280 bytes: mu1, mu2, E[x^2], E[y^2], E[xy] after the row pass
    double part_ssim[THREADS / 64];
    ull part_se[THREADS / 64], part_ae[THREADS / 64];
};

struct TileArgs {
    const void *a, *b;
    float* map;               // or nullptr
    Partial* partials;        // [n][tiles]
    int planes, H, Wp;        // of one frame
    int tiles_x, tiles_y;     // of one plane
    // the planes tail only
    const double* weights;    // [n][3]
    float* dplanes;           // plane j of the derivatives starts dplane_pitch floats behind plane j - 1
    size_t dplane_pitch;
};

// what the tile pass leaves: the partial records of the scores, or the derivative planes for the gradient of a, or of a and b
constexpr int TAIL_RECORDS = 0, TAIL_PLANES_A = 3, TAIL_PLANES_AB = 5;
// the planes' order in the workspace
constexpr int P_MU1 = 0, P_E11 = 1, P_E12 = 2, P_MU2 = 3, P_E22 = 4;

__device__ __forceinline__ float sample(const uint8_t* p, size_t i) { return (float)p[i] / 255.0f; }
__device__ __forceinline__ float sample(const float* p, size_t i) { return p[i]; }

template <class V>
__device__ __forceinline__ V wave_sum(V v) {
    for (int d = 32; d > 0; d >>= 1) v += __shfl_xor(v, d);
    return v;
}

// column pass of J quantities: rows r0 .. r0 + 3 of column c, from the row pass's results
template <int J>
__device__ __forceinline__ void column_pass(const float (*row)[STAGE_Y][TILE_X], int c, int r0, float (&q)[J][ROWS_PER_THREAD]) {
#pragma unroll
    for (int j = 0; j < J; ++j)
#pragma unroll
        for (int o = 0; o < ROWS_PER_THREAD; ++o) q[j][o] = 0.0f;
#pragma unroll
    for (int r = 0; r < ROWS_PER_THREAD + WIN - 1; ++r)
#pragma unroll
        for (int j = 0; j < J; ++j) {
            const float v = row[j][r0 + r][c];
#pragma unroll
            for (int o = 0; o < ROWS_PER_THREAD; ++o)
                if (r - o >= 0 && r - o < WIN) q[j][o] = fmaf(SSIM_WINDOW[r - o], v, q[j][o]);
        }
}

// the map's derivative by one input's window mean: `mine` that input's mean, `other` the other's
__device__ __forceinline__ float d_mean(float mine, float other, float p, float q, float pq, float D, float E) {
    return 2.0f * ((other * q - mine * pq) / D - (other * p - mine * pq) / E);
}

// grid (planes * tiles_y * tiles_x, n); CS: the plan's tap stride cs, a constant of the instantiation; TAIL: what it leaves
template <class T, int CS, int TAIL>
__global__ __launch_bounds__(THREADS) void metrics_tile_kernel(TileArgs g) {
    __shared__ Shared sh;
    const int t = threadIdx.x;
    if constexpr (TAIL != TAIL_RECORDS) {
        if (g.weights[(size_t)blockIdx.y * 3] == 0.0) return;          // the frame's ssim weight: no combine pass reads its planes
    }
    const int per_plane = g.tiles_x * g.tiles_y;
    const int plane = blockIdx.x / per_plane, tile = blockIdx.x % per_plane;
    const int x0 = (tile % g.tiles_x) * TILE_X, y0 = (tile / g.tiles_x) * TILE_Y;
    const size_t plane_at = ((size_t)blockIdx.y * g.planes + plane) * (size_t)g.H * (size_t)g.Wp;          // samples in front of the plane
    const T* a = (const T*)g.a + plane_at;
    const T* b = (const T*)g.b + plane_at;
    constexpr int cs = CS, halo_x = HALO * cs, stage_w = TILE_X + 2 * halo_x;
    static_assert(CS >= 1 && CS <= MAX_CS, "the halo fits the pitch");

    // the tile and its halo, zeros outside the plane
    for (int i = t; i < STAGE_Y * stage_w; i += THREADS) {
        const int r = i / stage_w, c = i % stage_w;
        // the staged sample lies dy rows and dx samples from the tile's corner.  y0 + dy and x0 + dx are formed for a sample of the plane
        // only: at H or Wp = 2^31 - 1 the last tile's corner is within 64 of INT_MAX and its halo's own coordinates do not fit an int
        const int dy = r - HALO, dx = c - halo_x;
        float va = 0.0f, vb = 0.0f;
        if (dy >= -y0 && dy < g.H - y0 && dx >= -x0 && dx < g.Wp - x0) {
            const size_t at = (size_t)(y0 + dy) * g.Wp + (x0 + dx);
            va = sample(a, at), vb = sample(b, at);
        }
        sh.in[0][r][c] = va, sh.in[1][r][c] = vb;
    }
    __syncthreads();

    // row pass: the five quantities of every staged row at the tile's columns
    for (int i = t; i < STAGE_Y * TILE_X; i += THREADS) {
        const int r = i / TILE_X, c = i % TILE_X;
        float m1 = 0.0f, m2 = 0.0f, e11 = 0.0f, e22 = 0.0f, e12 = 0.0f;
#pragma unroll
        for (int k = 0; k < WIN; ++k) {
            const float va = sh.in[0][r][c + k * cs], vb = sh.in[1][r][c + k * cs], wk = SSIM_WINDOW[k];
            m1 = fmaf(wk, va, m1), m2 = fmaf(wk, vb, m2);
            e11 = fmaf(wk, va * va, e11), e22 = fmaf(wk, vb * vb, e22), e12 = fmaf(wk, va * vb, e12);
        }
        sh.row[0][r][c] = m1, sh.row[1][r][c] = m2, sh.row[2][r][c] = e11, sh.row[3][r][c] = e22, sh.row[4][r][c] = e12;
    }
    __syncthreads();

    // column pass: rows r0 .. r0 + 3 of column c
    const int c = t % TILE_X, r0 = (t / TILE_X) * ROWS_PER_THREAD;
    float q[5][ROWS_PER_THREAD];
    column_pass<5>(sh.row, c, r0, q);

    double ssim = 0.0;
    uint32_t se_i = 0, ae_i = 0;
    double se_f = 0.0, ae_f = 0.0;
    const int x = x0 + c;
#pragma unroll
    for (int o = 0; o < ROWS_PER_THREAD; ++o) {
        const int y = y0 + r0 + o;
        if (x >= g.Wp || y >= g.H) continue;
        const float mu1 = q[0][o], mu2 = q[1][o];
        const float mu1_sq = mu1 * mu1, mu2_sq = mu2 * mu2, mu12 = mu1 * mu2;
        const float s1 = q[2][o] - mu1_sq, s2 = q[3][o] - mu2_sq, s12 = q[4][o] - mu12;
        const float A = 2.0f * mu12 + C1, B = 2.0f * s12 + C2, D = mu1_sq + mu2_sq + C1, E = s1 + s2 + C2;
        if constexpr (TAIL != TAIL_RECORDS) {
            const float p = A / D, pe = B / E, pq = p * pe;
            float* out = g.dplanes + plane_at + (size_t)y * g.Wp + x;
            out[P_MU1 * g.dplane_pitch] = d_mean(mu1, mu2, p, pe, pq, D, E);
            out[P_E11 * g.dplane_pitch] = -pq / E;
            out[P_E12 * g.dplane_pitch] = (2.0f * p) / E;
            if constexpr (TAIL == TAIL_PLANES_AB) {
                out[P_MU2 * g.dplane_pitch] = d_mean(mu2, mu1, p, pe, pq, D, E);
                out[P_E22 * g.dplane_pitch] = -pq / E;
            }
            continue;
        }
        const float value = (A * B) / (D * E);
        if (g.map) g.map[plane_at + (size_t)y * g.Wp + x] = value;
        ssim += (double)value;
        const float va = sh.in[0][r0 + o + HALO][c + halo_x], vb = sh.in[1][r0 + o + HALO][c + halo_x];
        if constexpr (sizeof(T) == 1) {
            // the staged float(v) / 255.0f is within v 2^-24 of v / 255: times 255 it rounds back to the byte
            const int d = __float2int_rn(va * 255.0f) - __float2int_rn(vb * 255.0f);
            se_i += (uint32_t)(d * d), ae_i += (uint32_t)abs(d);
        } else {
            const double d = (double)(va - vb);
            se_f += d * d, ae_f += fabs(d);
        }
    }

    if constexpr (TAIL != TAIL_RECORDS) return;
    // over the workgroup, in a fixed order
    ssim = wave_sum(ssim);
    ull se, ae;
    if constexpr (sizeof(T) == 1) {
        se = wave_sum((ull)se_i), ae = wave_sum((ull)ae_i);
    } else {
        se = (ull)__double_as_longlong(wave_sum(se_f)), ae = (ull)__double_as_longlong(wave_sum(ae_f));
    }
    if ((t & 63) == 0) sh.part_ssim[t >> 6] = ssim, sh.part_se[t >> 6] = se, sh.part_ae[t >> 6] = ae;
    __syncthreads();
    if (t == 0) {
        Partial p;
        p.ssim = sh.part_ssim[0];
        for (int k = 1; k < THREADS / 64; ++k) p.ssim += sh.part_ssim[k];
        if constexpr (sizeof(T) == 1) {
            p.se = sh.part_se[0], p.ae = sh.part_ae[0];
            for (int k = 1; k < THREADS / 64; ++k) p.se += sh.part_se[k], p.ae += sh.part_ae[k];
        } else {
            double s = __longlong_as_double((long long)sh.part_se[0]), m = __longlong_as_double((long long)sh.part_ae[0]);
            for (int k = 1; k < THREADS / 64; ++k) s += __longlong_as_double((long long)sh.part_se[k]), m += __longlong_as_double((long long)sh.part_ae[k]);
            p.se = (ull)__double_as_longlong(s), p.ae = (ull)__double_as_longlong(m);
        }
        g.partials[(size_t)blockIdx.y * gridDim.x + blockIdx.x] = p;
    }
}

// lane `lane`'s v in every thread; `lane` is the same in all of them, so this is two register reads, not a trip through LDS
__device__ __forceinline__ ull lane_value(ull v, int lane) {
    const uint32_t lo = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)v, lane), hi = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)(v >> 32), lane);
    return ((ull)hi << 32) | lo;
}

// grid n, one wave: frame blockIdx.x's `tiles` partial records added in index order.  The lanes load 64 records at a time; every lane
// then adds them one by one, so the chain of float64 additions is the sequential one (a lane behind the last record holds zeros, which
// change no sum).  count: samples of a frame; out: [n][4] = ssim, mse, l1, psnr
template <bool U8>
__global__ __launch_bounds__(64) void metrics_finish_kernel(const Partial* __restrict__ partials, unsigned tiles, double count, double* __restrict__ out) {
    const Partial* p = partials + (size_t)blockIdx.x * tiles;
    const unsigned lane = threadIdx.x;
    double ssim = 0.0, se_f = 0.0, ae_f = 0.0;
    ull se_i = 0, ae_i = 0;
    for (unsigned base = 0; base < tiles; base += 64) {
        Partial mine{0.0, 0, 0};
        if (base + lane < tiles) mine = p[base + lane];
        const ull mine_ssim = (ull)__double_as_longlong(mine.ssim);
        if (U8) se_i += mine.se, ae_i += mine.ae;          // integers: a lane's own sum now, the lanes' at the end, the same number in any order
#pragma unroll
        for (int i = 0; i < 64; ++i) {
            ssim += __longlong_as_double((long long)lane_value(mine_ssim, i));
            if (!U8) se_f += __longlong_as_double((long long)lane_value(mine.se, i)), ae_f += __longlong_as_double((long long)lane_value(mine.ae, i));
        }
    }
    if (U8) se_i = wave_sum(se_i), ae_i = wave_sum(ae_i);
    if (lane == 0) {
        // uint8: sums and divisors are integers below 2^53, so each quotient is the correctly rounded one of the exact ratio
        const double mse = U8 ? (double)se_i / (count * 65025.0) : se_f / count;
        const double l1 = U8 ? (double)ae_i / (count * 255.0) : ae_f / count;
        double* o = out + (size_t)blockIdx.x * 4;
        o[0] = ssim / count, o[1] = mse, o[2] = l1, o[3] = 20.0 * log10(1.0 / sqrt(mse));
    }
}

// ---- the gradient's second pass -----------------------------------------------------------------------------------------------------------
constexpr int GRAD_STAGE_W = TILE_X + 2 * HALO;             // 74: the tile's columns and the halo, tap stride 1

struct CombineShared {
    float in[3][STAGE_Y][GRAD_STAGE_W];                     // 23088 bytes: the derivative planes with their halo
    float row[3][STAGE_Y][TILE_X];                          // 19968 bytes: after the row pass
};
static_assert(sizeof(CombineShared) <= sizeof(Shared), "the combine pass keeps within the tile pass's LDS");

struct CombineArgs {
    const float *x, *y;       // the input whose gradient this is, and the other one
    const float *d_mu, *d_exx, *d_exy;          // the planes: by x's mean, by E[x^2], by E[xy]
    const double* weights;    // [n][3]
    float* grad;
    int planes, H, Wp;        // of one frame
    int tiles_x, tiles_y;     // of one plane
};

// grid (planes * tiles_y * tiles_x, n), as the tile pass
__global__ __launch_bounds__(THREADS) void metrics_combine_kernel(CombineArgs g) {
    __shared__ CombineShared sh;
    const int t = threadIdx.x;
    const int per_plane = g.tiles_x * g.tiles_y;
    const int plane = blockIdx.x / per_plane, tile = blockIdx.x % per_plane;
    const int x0 = (tile % g.tiles_x) * TILE_X, y0 = (tile / g.tiles_x) * TILE_Y;
    const size_t plane_at = ((size_t)blockIdx.y * g.planes + plane) * (size_t)g.H * (size_t)g.Wp;          // samples in front of the plane
    const double* w = g.weights + (size_t)blockIdx.y * 3;
    const double count = (double)g.planes * (double)g.H * (double)g.Wp;
    // the frame's three scalars, one rounding each
    const float k_ssim = (float)(w[0] / count), k_mse = (float)(2.0 * w[1] / count), k_l1 = (float)(w[2] / count);
    const bool with_ssim = w[0] != 0.0;          // the same in every thread of the workgroup

    const int c = t % TILE_X, r0 = (t / TILE_X) * ROWS_PER_THREAD;
    float q[3][ROWS_PER_THREAD];
    if (with_ssim) {
        // the planes' tile and its halo, zeros outside the plane
        const float* src[3] = {g.d_mu + plane_at, g.d_exx + plane_at, g.d_exy + plane_at};
        for (int i = t; i < STAGE_Y * GRAD_STAGE_W; i += THREADS) {
            const int r = i / GRAD_STAGE_W, cc = i % GRAD_STAGE_W;
            const int dy = r - HALO, dx = cc - HALO;          // from the tile's corner, as in the tile pass: no coordinate outside the plane is formed
            const bool inside = dy >= -y0 && dy < g.H - y0 && dx >= -x0 && dx < g.Wp - x0;
            const size_t at = inside ? (size_t)(y0 + dy) * g.Wp + (x0 + dx) : 0;
#pragma unroll
            for (int j = 0; j < 3; ++j) sh.in[j][r][cc] = inside ? src[j][at] : 0.0f;
        }
        __syncthreads();
        for (int i = t; i < STAGE_Y * TILE_X; i += THREADS) {
            const int r = i / TILE_X, cc = i % TILE_X;
            float acc[3] = {0.0f, 0.0f, 0.0f};
#pragma unroll
            for (int k = 0; k < WIN; ++k)
#pragma unroll
                for (int j = 0; j < 3; ++j) acc[j] = fmaf(SSIM_WINDOW[k], sh.in[j][r][cc + k], acc[j]);
#pragma unroll
            for (int j = 0; j < 3; ++j) sh.row[j][r][cc] = acc[j];
        }
        __syncthreads();
        column_pass<3>(sh.row, c, r0, q);
    }

    const int x = x0 + c;
#pragma unroll
    for (int o = 0; o < ROWS_PER_THREAD; ++o) {
        const int y = y0 + r0 + o;
        if (x >= g.Wp || y >= g.H) continue;
        const size_t at = plane_at + (size_t)y * g.Wp + x;
        const float xv = g.x[at], yv = g.y[at];
        const float d = xv - yv;
        const float sign = xv > yv ? 1.0f : xv < yv ? -1.0f : d;          // d: zero, or the NaN of an input
        float v = 0.0f;
        if (with_ssim) v = k_ssim * ((q[0][o] + (2.0f * xv) * q[1][o]) + yv * q[2][o]);
        g.grad[at] = (v + k_mse * d) + k_l1 * sign;
    }
}

// ---- the call -----------------------------------------------------------------------------------------------------------------------------
struct MetricsPlan {
    int planes, H, Wp, cs;          // the view of one frame
    int tiles_x, tiles_y;
    size_t tiles;                   // of one frame
    size_t frame_samples;
    size_t o_partials, total;
};

// u8: HWC uint8 frames, else NCHW float32
const char* check_metrics_shape(bool u8, int n, int h, int w, int c) {
    if (u8 ? (c != 1 && c != 3) : (c < 1 || c > 4)) return u8 ? "c other than 1 and 3" : "c outside 1..4";
    if (n < 1 || n > 65535) return "n outside 1..65535";
    if (h < 1) return "h below 1";
    if (w < 1) return "w below 1";
    if ((uint64_t)h * (uint64_t)w > (uint64_t)0x7fffffff / (uint64_t)c) return "a frame beyond 2^31 - 1 samples";
    return nullptr;
}

// The one layout of a call
MetricsPlan make_metrics_plan(bool u8, int n, int h, int w, int c) {
    MetricsPlan p{};
    p.planes = u8 ? 1 : c, p.H = h, p.Wp = u8 ? w * c : w, p.cs = u8 ? c : 1;
    p.tiles_x = (p.Wp - 1) / TILE_X + 1, p.tiles_y = (p.H - 1) / TILE_Y + 1;          // Wp + TILE_X - 1 does not fit an int at Wp = 2^31 - 1
    p.tiles = (size_t)p.planes * p.tiles_x * p.tiles_y;          // below 2^31: a tile holds a sample at least, 16 unless the plane is one tile high
    p.frame_samples = (size_t)h * w * c;
    Carve ws;
    p.o_partials = ws.take((size_t)n * p.tiles * sizeof(Partial));
    p.total = ws.at;
    return p;
}

bool overlaps(const void* a, size_t a_bytes, const void* b, size_t b_bytes) {
    return (uintptr_t)a < (uintptr_t)b + b_bytes && (uintptr_t)b < (uintptr_t)a + a_bytes;
}

int metrics_bytes(bool u8, int n, int h, int w, int c, size_t* workspace_bytes) {
    const char* who = u8 ? "image_metrics_u8" : "image_metrics_f32";
    if (const char* bad = check_metrics_shape(u8, n, h, w, c)) { set_error("%s: %s (n %d, %d x %d, c %d)", who, bad, n, h, w, c); return ADAIN_EINVAL; }
    if (workspace_bytes) *workspace_bytes = make_metrics_plan(u8, n, h, w, c).total;
    return 0;
}

int launch_metrics(bool u8, const void* a, const void* b, int n, int h, int w, int c, double* out, float* map, void* workspace, size_t workspace_bytes,
                   hipStream_t s) {
    const char* who = u8 ? "image_metrics_u8" : "image_metrics_f32";
    if (!a) { set_error("%s: a is a null pointer", who); return ADAIN_EINVAL; }
    if (!b) { set_error("%s: b is a null pointer", who); return ADAIN_EINVAL; }
    if (!out) { set_error("%s: out is a null pointer", who); return ADAIN_EINVAL; }
    if (const char* bad = check_metrics_shape(u8, n, h, w, c)) { set_error("%s: %s (n %d, %d x %d, c %d)", who, bad, n, h, w, c); return ADAIN_EINVAL; }
    const MetricsPlan p = make_metrics_plan(u8, n, h, w, c);
    if (int rc = check_workspace(who, workspace, workspace_bytes, p.total, 8)) return rc;
    if ((uintptr_t)out % 8) { set_error("%s: out must be 8-byte aligned", who); return ADAIN_EINVAL; }
    if ((uintptr_t)map % 4) { set_error("%s: ssim_map must be 4-byte aligned", who); return ADAIN_EINVAL; }
    if (!u8 && ((uintptr_t)a % 4 || (uintptr_t)b % 4)) { set_error("%s: %s must be 4-byte aligned", who, (uintptr_t)a % 4 ? "a" : "b"); return ADAIN_EINVAL; }
    const size_t samples = (size_t)n * p.frame_samples, src_bytes = samples * (u8 ? 1 : sizeof(float));
    const struct { const char* name; const void* ptr; size_t bytes; } outs[3] = {
        {"out", out, (size_t)n * 4 * sizeof(double)}, {"ssim_map", map, samples * sizeof(float)}, {"the workspace", workspace, p.total}};
    for (const auto& o : outs) {
        if (!o.ptr) continue;
        if (overlaps(o.ptr, o.bytes, a, src_bytes)) { set_error("%s: %s overlaps a", who, o.name); return ADAIN_EINVAL; }
        if (overlaps(o.ptr, o.bytes, b, src_bytes)) { set_error("%s: %s overlaps b", who, o.name); return ADAIN_EINVAL; }
    }
    TileArgs g{};
    g.a = a, g.b = b, g.map = map, g.partials = (Partial*)((char*)workspace + p.o_partials);
    g.planes = p.planes, g.H = p.H, g.Wp = p.Wp, g.tiles_x = p.tiles_x, g.tiles_y = p.tiles_y;
    const dim3 grid((unsigned)p.tiles, (unsigned)n);
    if (u8) {
        if (p.cs == 1) metrics_tile_kernel<uint8_t, 1, TAIL_RECORDS><<<grid, THREADS, 0, s>>>(g);
        else metrics_tile_kernel<uint8_t, 3, TAIL_RECORDS><<<grid, THREADS, 0, s>>>(g);
        metrics_finish_kernel<true><<<(unsigned)n, 64, 0, s>>>(g.partials, (unsigned)p.tiles, (double)p.frame_samples, out);
    } else {
        metrics_tile_kernel<float, 1, TAIL_RECORDS><<<grid, THREADS, 0, s>>>(g);
        metrics_finish_kernel<false><<<(unsigned)n, 64, 0, s>>>(g.partials, (unsigned)p.tiles, (double)p.frame_samples, out);
    }
    return check_launch(who);
}

// The one layout of a gradient call: the derivative planes, each the clip's size
struct GradPlan {
    MetricsPlan m;
    int nplanes;
    size_t plane_bytes, pitch_bytes;          // of one plane; from one plane's start to the next
    size_t total;
};

GradPlan make_grad_plan(int n, int h, int w, int c, bool with_grad_b) {
    GradPlan p{};
    p.m = make_metrics_plan(false, n, h, w, c);
    p.nplanes = with_grad_b ? TAIL_PLANES_AB : TAIL_PLANES_A;
    p.plane_bytes = (size_t)n * p.m.frame_samples * sizeof(float);
    Carve ws;
    for (int j = 0; j < p.nplanes; ++j) ws.take(p.plane_bytes);
    p.pitch_bytes = align256(p.plane_bytes);
    p.total = ws.at;
    return p;
}

int launch_metrics_grad(const float* a, const float* b, int n, int h, int w, int c, const double* weights, float* grad_a, float* grad_b, void* workspace,
                        size_t workspace_bytes, hipStream_t s) {
    const char* who = "image_metrics_grad_f32";
    if (!a) { set_error("%s: a is a null pointer", who); return ADAIN_EINVAL; }
    if (!b) { set_error("%s: b is a null pointer", who); return ADAIN_EINVAL; }
    if (!weights) { set_error("%s: weights is a null pointer", who); return ADAIN_EINVAL; }
    if (!grad_a) { set_error("%s: grad_a is a null pointer", who); return ADAIN_EINVAL; }
    if (const char* bad = check_metrics_shape(false, n, h, w, c)) { set_error("%s: %s (n %d, %d x %d, c %d)", who, bad, n, h, w, c); return ADAIN_EINVAL; }
    const GradPlan p = make_grad_plan(n, h, w, c, grad_b != nullptr);
    if (int rc = check_workspace(who, workspace, workspace_bytes, p.total, 8)) return rc;
    if ((uintptr_t)weights % 8) { set_error("%s: weights must be 8-byte aligned", who); return ADAIN_EINVAL; }
    const struct { const char* name; const void* ptr; size_t bytes; } ins[3] = {{"a", a, p.plane_bytes}, {"b", b, p.plane_bytes}, {"weights", weights, (size_t)n * 3 * sizeof(double)}},
      outs[3] = {{"grad_a", grad_a, p.plane_bytes}, {"grad_b", grad_b, p.plane_bytes}, {"the workspace", workspace, p.total}};
    for (const auto* f : {&ins[0], &ins[1], &outs[0], &outs[1]})
        if ((uintptr_t)f->ptr % 4) { set_error("%s: %s must be 4-byte aligned", who, f->name); return ADAIN_EINVAL; }
    for (int i = 0; i < 3; ++i) {
        if (!outs[i].ptr) continue;
        for (const auto& in : ins)
            if (overlaps(outs[i].ptr, outs[i].bytes, in.ptr, in.bytes)) { set_error("%s: %s overlaps %s", who, outs[i].name, in.name); return ADAIN_EINVAL; }
        for (int k = 0; k < i; ++k)
            if (outs[k].ptr && overlaps(outs[i].ptr, outs[i].bytes, outs[k].ptr, outs[k].bytes)) { set_error("%s: %s overlaps %s", who, outs[i].name, outs[k].name); return ADAIN_EINVAL; }
    }
    TileArgs g{};
    g.a = a, g.b = b, g.planes = p.m.planes, g.H = p.m.H, g.Wp = p.m.Wp, g.tiles_x = p.m.tiles_x, g.tiles_y = p.m.tiles_y;
    g.weights = weights, g.dplanes = (float*)workspace, g.dplane_pitch = p.pitch_bytes / sizeof(float);
    const dim3 grid((unsigned)p.m.tiles, (unsigned)n);
    if (grad_b) metrics_tile_kernel<float, 1, TAIL_PLANES_AB><<<grid, THREADS, 0, s>>>(g);
    else metrics_tile_kernel<float, 1, TAIL_PLANES_A><<<grid, THREADS, 0, s>>>(g);
    const auto plane = [&](int j) { return (const float*)g.dplanes + (size_t)j * g.dplane_pitch; };
    CombineArgs k{};
    k.weights = weights, k.planes = g.planes, k.H = g.H, k.Wp = g.Wp, k.tiles_x = g.tiles_x, k.tiles_y = g.tiles_y;
    k.x = a, k.y = b, k.d_mu = plane(P_MU1), k.d_exx = plane(P_E11), k.d_exy = plane(P_E12), k.grad = grad_a;
    metrics_combine_kernel<<<grid, THREADS, 0, s>>>(k);
    if (grad_b) {
        k.x = b, k.y = a, k.d_mu = plane(P_MU2), k.d_exx = plane(P_E22), k.grad = grad_b;
        metrics_combine_kernel<<<grid, THREADS, 0, s>>>(k);
    }
    return check_launch(who);
}

}  // namespace

int image_metrics_u8_bytes(int n, int h, int w, int c, size_t* workspace_bytes) { return metrics_bytes(true, n, h, w, c, workspace_bytes); }
int image_metrics_f32_bytes(int n, int c, int h, int w, size_t* workspace_bytes) { return metrics_bytes(false, n, h, w, c, workspace_bytes); }

int launch_image_metrics_u8(const uint8_t* a, const uint8_t* b, int n, int h, int w, int c, double* out, float* ssim_map, void* workspace, size_t workspace_bytes,
                            hipStream_t s) {
    return launch_metrics(true, a, b, n, h, w, c, out, ssim_map, workspace, workspace_bytes, s);
}

int launch_image_metrics_f32(const float* a, const float* b, int n, int c, int h, int w, double* out, float* ssim_map, void* workspace, size_t workspace_bytes,
                             hipStream_t s) {
    return launch_metrics(false, a, b, n, h, w, c, out, ssim_map, workspace, workspace_bytes, s);
}

int image_metrics_grad_f32_bytes(int n, int c, int h, int w, int with_grad_b, size_t* workspace_bytes) {
    if (const char* bad = check_metrics_shape(false, n, h, w, c)) { set_error("image_metrics_grad_f32: %s (n %d, %d x %d, c %d)", bad, n, h, w, c); return ADAIN_EINVAL; }
    if (workspace_bytes) *workspace_bytes = make_grad_plan(n, h, w, c, with_grad_b != 0).total;
    return 0;
}

int launch_image_metrics_grad_f32(const float* a, const float* b, int n, int c, int h, int w, const double* weights, float* grad_a, float* grad_b, void* workspace,
                                  size_t workspace_bytes, hipStream_t s) {
    return launch_metrics_grad(a, b, n, h, w, c, weights, grad_a, grad_b, workspace, workspace_bytes, s);
}

void ssim_window(float out[11]) {
    for (int k = 0; k < WIN; ++k) out[k] = SSIM_WINDOW[k];
}

}  // namespace adain
