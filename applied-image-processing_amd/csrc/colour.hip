// Foreground colour harmonisation of the localized pipeline on the device (Style_3DGS/localized_style_transfer.py:128-168 and the
// composite around it, :232-238; the host form is applied-image-processing_amd/localized.py).
//
// Two uint8 HWC images of one size; a REGION is the set of pixels whose three channels do not sum to zero (:134-135).  Everything
// after `float32(u8) / 255.0f` is float64, as numpy makes it at the first np.dot with the float64 matrices.  The rules, stage by stage:
//   1. lab: x = LMS_TO_LAB . log10(max(RGB_TO_LMS . rgb, 1e-6)), every product summed over k = 0, 1, 2 in that order, no FMA
//      contraction (the file is compiled with -ffp-contract=off): equal colours give bit-equal l-alpha-beta values and projections.
//      numpy's dot goes through BLAS, so the float64 intermediates agree with the host path to rounding, not bit for bit.
//   2. moments per region: N, sum x, sum x x^T in float64.  Each thread adds its pixels in index order, a workgroup combines its threads
//      with a butterfly and a fixed walk over its waves, a second kernel combines the workgroups the same way.  The grid depends on
//      h * w alone: the sums do not depend on scheduling, the stream or the device's size.
//   3. PCA(n_components = 1) as scikit-learn >= 1.5 fits it: mean, covariance (X^T X - N mu mu^T) / (N - 1), leading eigenvector (cyclic
//      Jacobi, one thread), sign that makes the largest-magnitude loading positive.
//   4. keys: x . v - mu . v per region pixel, +infinity elsewhere, in a dense [h * w] float64 array per image; both arrays are sorted
//      ascending (rocprim::radix_sort_keys), so the first N keys of each are its region's quantile function.
//   5. match_cdf (:99-125) with numpy's rules: np.linspace(0, 1, n)[i] = i * (1.0 / (n - 1)), the last element exactly 1, n = 1 gives
//      [0.]; np.interp(x, xp, fp) takes j = the LAST index with xp[j] <= x: x < xp[0] gives fp[0], j = len - 1 gives fp[-1], x == xp[j]
//      gives fp[j], otherwise (fp[j+1] - fp[j]) / (xp[j+1] - xp[j]) * (x - xp[j]) + fp[j] with numpy's two fallbacks when that is NaN.
//      The shorter quantile function is resampled to the longer one's length, then each foreground key is looked up in the foreground
//      quantiles (a binary search per pixel) and read off the background's.
//   6. back: matched * v + mu, LAB_TO_LMS, pow(10, .), LMS_TO_RGB, clip to [0, 1], * 255, truncation to uint8 (:84-88).
// An empty region leaves the output a copy of the foreground (:141-147); so does a region of one pixel, whose covariance divides by
// zero in the reference: the record's status word says which, and the caller decides what to make of it.  Nothing is copied to the
// host and nothing waits on it: counts, PCA results and the status live in the record at the start of the workspace.
#include <cstdlib>
#include <cstring>   // rocprim's texture_cache_iterator.hpp calls memset without including it

// The product library reads no environment.  rocprim looks at it once (ROCPRIM_USE_ATOMIC_BLOCK_ID, ordered_block_id.hpp: a tuning
// switch of its look-back scans) through std::getenv; it is told "unset", its default.
namespace std {
inline char* adain_env_unset(const char*) { return nullptr; }
}  // namespace std
#define getenv adain_env_unset
#include <rocprim/rocprim.hpp>
#undef getenv

#include "common.h"
#include "device_utils.h"

namespace adain {

namespace {

constexpr int CT_THREADS = 256;
constexpr int CT_MAX_BLOCKS = 512;
constexpr int CT_PIX_PER_THREAD = 8;
constexpr int CT_MOMENTS = 10;   // N, sum x (3), sum x x^T (xx, xy, xz, yy, yz, zz)

// localized_style_transfer.py:11-19.  LMS_TO_LAB = diag(1/sqrt3, 1/sqrt6, 1/sqrt2) @ [[1,1,1],[1,1,-2],[1,-1,0]] is exact in that
// product (one non-zero term per element); the two inverses are numpy.linalg.inv's float64 results.
__constant__ double RGB_TO_LMS[3][3] = {{0.3811, 0.5783, 0.0402}, {0.1967, 0.7244, 0.0782}, {0.0241, 0.1288, 0.8444}};
__constant__ double LMS_TO_LAB[3][3] = {{0.5773502691896258, 0.5773502691896258, 0.5773502691896258},
                                        {0.4082482904638631, 0.4082482904638631, -0.8164965809277261},
                                        {0.7071067811865475, -0.7071067811865475, 0.0}};
__constant__ double LAB_TO_LMS[3][3] = {{0.5773502691896257, 0.40824829046386296, 0.7071067811865476},
                                        {0.5773502691896257, 0.40824829046386296, -0.7071067811865476},
                                        {0.5773502691896255, -0.8164965809277259, 1.1404650007967886e-16}};
__constant__ double LMS_TO_RGB[3][3] = {{4.468669863496255, -3.5886759034721267, 0.11960436657860116},
                                        {-1.2197166276177631, 2.3830879129554567, -0.16263011175140055},
                                        {0.058508476938545856, -0.2610784390276937, 1.205665908525623}};

// The two images of a call.  mask == nullptr: a is the foreground, b the background.  Otherwise a is the content, b the stylised image
// and mask the {0,1} background mask: foreground = a * (1 - m), background = b * m, never materialised.
struct Images {
    const uint8_t* a;
    const uint8_t* b;
    const uint8_t* mask;
};

struct Rgb {
    unsigned r, g, b;
    __device__ bool in_region() const { return r + g + b > 0; }
};

__device__ __forceinline__ Rgb load_rgb(const uint8_t* p, int i) {      // a byte offset: 3 i passes 2^31 - 1 from 715 827 883 pixels on (2^30 - 1 are admitted)
    const size_t o = 3 * (size_t)i;
    return Rgb{p[o], p[o + 1], p[o + 2]};
}

template <int REGION>   // 0: foreground, 1: background
__device__ __forceinline__ Rgb region_pixel(const Images& im, int i) {
    if (im.mask && (im.mask[i] != 0) != (REGION == 1)) return Rgb{0, 0, 0};
    return load_rgb(REGION == 0 ? im.a : im.b, i);
}

__device__ __forceinline__ double dot3(const double m[3], double x, double y, double z) { return (m[0] * x + m[1] * y) + m[2] * z; }

__device__ __forceinline__ void rgb_to_lab(Rgb p, double lab[3]) {
    // numpy's float32 division (correctly rounded), then the promotion to float64
    const double r = (double)__fdiv_rn((float)p.r, 255.0f), g = (double)__fdiv_rn((float)p.g, 255.0f), b = (double)__fdiv_rn((float)p.b, 255.0f);
    double lg[3];
#pragma unroll
    for (int c = 0; c < 3; ++c) lg[c] = log10(fmax(dot3(RGB_TO_LMS[c], r, g, b), 1e-6));
#pragma unroll
    for (int c = 0; c < 3; ++c) lab[c] = dot3(LMS_TO_LAB[c], lg[0], lg[1], lg[2]);
}

__device__ __forceinline__ void add_moments(double m[CT_MOMENTS], const double x[3]) {
    m[0] += 1.0;
    m[1] += x[0]; m[2] += x[1]; m[3] += x[2];
    m[4] += x[0] * x[0]; m[5] += x[0] * x[1]; m[6] += x[0] * x[2];
    m[7] += x[1] * x[1]; m[8] += x[1] * x[2]; m[9] += x[2] * x[2];
}

// partial [blocks][2][CT_MOMENTS]
__global__ __launch_bounds__(CT_THREADS) void colour_moments_kernel(Images im, int hw, double* __restrict__ partial) {
    double m[2][CT_MOMENTS] = {};
    for (int i = blockIdx.x * CT_THREADS + threadIdx.x; i < hw; i += gridDim.x * CT_THREADS) {
        double x[3];
        const Rgb f = region_pixel<0>(im, i), b = region_pixel<1>(im, i);
        if (f.in_region()) { rgb_to_lab(f, x); add_moments(m[0], x); }
        if (b.in_region()) { rgb_to_lab(b, x); add_moments(m[1], x); }
    }
    __shared__ double sh[CT_THREADS / 64][2 * CT_MOMENTS];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
    for (int r = 0; r < 2; ++r)
#pragma unroll
        for (int k = 0; k < CT_MOMENTS; ++k) {
            double v = m[r][k];
#pragma unroll
            for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
            if (lane == 0) sh[wave][r * CT_MOMENTS + k] = v;
        }
    __syncthreads();
    if (threadIdx.x < 2 * CT_MOMENTS) {
        double t = 0;
        for (int wv = 0; wv < CT_THREADS / 64; ++wv) t += sh[wv][threadIdx.x];
        partial[(size_t)blockIdx.x * 2 * CT_MOMENTS + threadIdx.x] = t;
    }
}

__device__ void fit_pca1(const double m[CT_MOMENTS], adain_colour_region* out) {
    const double n = m[0];
    out->n = (int64_t)n;
    for (int k = 0; k < 3; ++k) out->mean[k] = out->component[k] = 0.0;
    out->explained_variance = 0.0;
    if (n < 1.0) return;
    double mu[3];
    for (int k = 0; k < 3; ++k) out->mean[k] = mu[k] = m[1 + k] / n;
    if (n < 2.0) return;
    const double xx[3][3] = {{m[4], m[5], m[6]}, {m[5], m[7], m[8]}, {m[6], m[8], m[9]}};
    double a[3][3], v[3][3];
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j) a[i][j] = (xx[i][j] - n * (mu[i] * mu[j])) / (n - 1.0);
    jacobi3(a, v);
    int top = 0;
    for (int k = 1; k < 3; ++k)
        if (a[k][k] > a[top][top]) top = k;
    double c[3] = {v[0][top], v[1][top], v[2][top]};
    const double len = sqrt((c[0] * c[0] + c[1] * c[1]) + c[2] * c[2]);
    int big = 0;
    for (int k = 1; k < 3; ++k)
        if (fabs(c[k]) > fabs(c[big])) big = k;
    const double sgn = c[big] < 0.0 ? -1.0 : 1.0;
    for (int k = 0; k < 3; ++k) out->component[k] = sgn * c[k] / len;
    out->explained_variance = fmax(a[top][top], 0.0);
}

// one workgroup: wave w combines moment q = w, w + 4, ... over the partial blocks, then thread 0 fits both regions
__global__ __launch_bounds__(CT_THREADS) void colour_pca_kernel(const double* __restrict__ partial, int blocks, adain_colour_record* __restrict__ rec) {
    __shared__ double tot[2 * CT_MOMENTS];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    for (int q = wave; q < 2 * CT_MOMENTS; q += CT_THREADS / 64) {
        double v = 0;
        for (int b = lane; b < blocks; b += 64) v += partial[(size_t)b * 2 * CT_MOMENTS + q];
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
        if (lane == 0) tot[q] = v;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        fit_pca1(tot, &rec->fg);
        fit_pca1(tot + CT_MOMENTS, &rec->bg);
        int status = 0;
        if (rec->fg.n == 0) status |= ADAIN_COLOUR_FG_EMPTY;
        if (rec->bg.n == 0) status |= ADAIN_COLOUR_BG_EMPTY;
        if (rec->fg.n == 1) status |= ADAIN_COLOUR_FG_SINGLE;
        if (rec->bg.n == 1) status |= ADAIN_COLOUR_BG_SINGLE;
        rec->status = status;
        rec->reserved = 0;
    }
}

__device__ __forceinline__ double project(const adain_colour_region& r, const double x[3]) {
    return dot3(r.component, x[0], x[1], x[2]) - dot3(r.component, r.mean[0], r.mean[1], r.mean[2]);
}

__global__ __launch_bounds__(CT_THREADS) void colour_keys_kernel(Images im, int hw, const adain_colour_record* __restrict__ rec,
                                                                 double* __restrict__ keys_fg, double* __restrict__ keys_bg) {
    const adain_colour_region fg = rec->fg, bg = rec->bg;
    const double inf = __builtin_inf();
    for (int i = blockIdx.x * CT_THREADS + threadIdx.x; i < hw; i += gridDim.x * CT_THREADS) {
        double x[3], kf = inf, kb = inf;
        const Rgb f = region_pixel<0>(im, i), b = region_pixel<1>(im, i);
        if (f.in_region()) { rgb_to_lab(f, x); kf = project(fg, x); }
        if (b.in_region()) { rgb_to_lab(b, x); kb = project(bg, x); }
        keys_fg[i] = kf;
        keys_bg[i] = kb;
    }
}

// np.linspace(0, 1, n)[i]
__device__ __forceinline__ double linspace01(int64_t i, int64_t n, double step) { return i == 0 ? 0.0 : (i == n - 1 ? 1.0 : (double)i * step); }

// np.interp's value at x once j, the last index with xp[j] <= x (-1: none), is known
template <class XP>
__device__ __forceinline__ double interp_at(double x, int64_t j, int64_t len, XP xp, const double* __restrict__ fp) {
    if (j < 0) return fp[0];
    if (j >= len - 1) return fp[len - 1];
    const double xj = xp(j), fj = fp[j];
    if (xj == x) return fj;
    const double xn = xp(j + 1), fn = fp[j + 1];
    const double slope = (fn - fj) / (xn - xj);
    double r = slope * (x - xj) + fj;
    if (isnan(r)) {
        r = slope * (x - xn) + fn;
        if (isnan(r) && fj == fn) r = fj;
    }
    return r;
}

// the shorter of the two sorted key arrays resampled to the longer one's length (match_cdf, :108-121); nothing to do for equal lengths
__global__ __launch_bounds__(CT_THREADS) void colour_resample_kernel(int hw, const adain_colour_record* __restrict__ rec, const double* __restrict__ sorted_fg,
                                                                     const double* __restrict__ sorted_bg, double* __restrict__ resampled) {
    const int64_t nt = rec->fg.n, ns = rec->bg.n;
    if (rec->status != 0 || nt == ns) return;
    const int64_t len = nt > ns ? nt : ns, n = nt > ns ? ns : nt;       // output and input lengths
    const double* __restrict__ src = nt > ns ? sorted_bg : sorted_fg;
    const double gstep = 1.0 / (double)(len - 1), hstep = 1.0 / (double)(n - 1);
    auto h = [&](int64_t k) { return linspace01(k, n, hstep); };
    for (int64_t i = blockIdx.x * CT_THREADS + threadIdx.x; i < hw; i += (int64_t)gridDim.x * CT_THREADS) {
        if (i >= len) return;
        const double g = linspace01(i, len, gstep);
        // j = the last index of the input grid at or below g: an estimate, then a walk to the exact one
        int64_t j = (int64_t)(g * (double)(n - 1));
        j = j < 0 ? 0 : (j > n - 1 ? n - 1 : j);
        while (j + 1 <= n - 1 && h(j + 1) <= g) ++j;
        while (j > 0 && h(j) > g) --j;
        resampled[i] = interp_at(g, j, n, h, src);
    }
}

__global__ __launch_bounds__(CT_THREADS) void colour_match_kernel(Images im, int hw, const adain_colour_record* __restrict__ rec,
                                                                  const double* __restrict__ keys_fg, const double* __restrict__ sorted_fg,
                                                                  const double* __restrict__ sorted_bg, const double* __restrict__ resampled,
                                                                  uint8_t* __restrict__ out) {
    const adain_colour_region fg = rec->fg;
    const int64_t nt = fg.n, ns = rec->bg.n;
    const bool transfer = rec->status == 0;
    const int64_t len = nt > ns ? nt : ns;
    const double* __restrict__ xp = nt >= ns ? sorted_fg : resampled;
    const double* __restrict__ fp = nt > ns ? resampled : sorted_bg;
    for (int i = blockIdx.x * CT_THREADS + threadIdx.x; i < hw; i += gridDim.x * CT_THREADS) {
        const Rgb f = region_pixel<0>(im, i);
        unsigned o[3] = {f.r, f.g, f.b};
        if (im.mask && im.mask[i] != 0) {
            // adjusted * (1 - m) + background with m = 1
            const Rgb b = load_rgb(im.b, i);
            o[0] = b.r; o[1] = b.g; o[2] = b.b;
        } else if (transfer && f.in_region()) {
            const double x = keys_fg[i];
            int64_t lo = 0, hi = len;                 // first index with xp[index] > x
            while (lo < hi) {
                const int64_t mid = (lo + hi) >> 1;
                if (xp[mid] <= x) lo = mid + 1; else hi = mid;
            }
            const double matched = interp_at(x, lo - 1, len, [&](int64_t k) { return xp[k]; }, fp);
            double lab[3], lms[3];
#pragma unroll
            for (int c = 0; c < 3; ++c) lab[c] = matched * fg.component[c] + fg.mean[c];
#pragma unroll
            for (int c = 0; c < 3; ++c) lms[c] = pow(10.0, dot3(LAB_TO_LMS[c], lab[0], lab[1], lab[2]));
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                const double v = dot3(LMS_TO_RGB[c], lms[0], lms[1], lms[2]);
                o[c] = (unsigned)(fmin(fmax(v, 0.0), 1.0) * 255.0);
            }
        }
        out[3 * (size_t)i] = (uint8_t)o[0];
        out[3 * (size_t)i + 1] = (uint8_t)o[1];
        out[3 * (size_t)i + 2] = (uint8_t)o[2];
    }
}

int moment_blocks(size_t hw) {
    const size_t per_block = (size_t)CT_THREADS * CT_PIX_PER_THREAD;
    const size_t b = (hw + per_block - 1) / per_block;
    return (int)(b < 1 ? 1 : (b > (size_t)CT_MAX_BLOCKS ? (size_t)CT_MAX_BLOCKS : b));
}

int pixel_blocks(size_t hw) {
    const size_t b = (hw + CT_THREADS - 1) / CT_THREADS;
    return (int)(b > 8192 ? 8192 : b);
}

struct Layout {
    size_t record, partial, keys_fg, keys_bg, sorted_fg, sorted_bg, sort_tmp, sort_tmp_bytes, total;
};

// false: the size is refused or rocprim could not size its temporary storage
bool layout(int h, int w, Layout* l) {
    if (h < 1 || w < 1 || (size_t)h * w > 0x3fffffffULL) return false;
    const size_t hw = (size_t)h * w;
    size_t tmp = 0;
    if (rocprim::radix_sort_keys(nullptr, tmp, (const double*)nullptr, (double*)nullptr, hw) != hipSuccess) return false;
    Carve c;
    l->record = c.take(sizeof(adain_colour_record));
    l->partial = c.take((size_t)moment_blocks(hw) * 2 * CT_MOMENTS * sizeof(double));
    l->keys_fg = c.take(hw * sizeof(double));
    l->keys_bg = c.take(hw * sizeof(double));
    l->sorted_fg = c.take(hw * sizeof(double));
    l->sorted_bg = c.take(hw * sizeof(double));
    l->sort_tmp_bytes = tmp;
    l->sort_tmp = c.take(tmp);
    l->total = c.at;
    return true;
}

int run(const Images& im, uint8_t* out, int h, int w, void* workspace, hipStream_t s, const char* what) {
    Layout l;
    if (!im.a || !im.b || !out || !workspace) { set_error("%s: null pointer", what); return ADAIN_EINVAL; }
    if (!layout(h, w, &l)) { set_error("%s: unsupported size %d x %d", what, h, w); return ADAIN_EINVAL; }
    // the entries carry no byte count: the caller's buffer is taken to have the layout's size, its pointer and alignment are checked
    if (int rc = check_workspace(what, workspace, l.total, l.total, 8)) return rc;
    char* ws = (char*)workspace;
    auto* rec = (adain_colour_record*)(ws + l.record);
    double* partial = (double*)(ws + l.partial);
    double *keys_fg = (double*)(ws + l.keys_fg), *keys_bg = (double*)(ws + l.keys_bg);
    double *sorted_fg = (double*)(ws + l.sorted_fg), *sorted_bg = (double*)(ws + l.sorted_bg);
    const int hw = h * w, mb = moment_blocks(hw), pb = pixel_blocks(hw);
    hipLaunchKernelGGL(colour_moments_kernel, dim3(mb), dim3(CT_THREADS), 0, s, im, hw, partial);
    hipLaunchKernelGGL(colour_pca_kernel, dim3(1), dim3(CT_THREADS), 0, s, (const double*)partial, mb, rec);
    hipLaunchKernelGGL(colour_keys_kernel, dim3(pb), dim3(CT_THREADS), 0, s, im, hw, (const adain_colour_record*)rec, keys_fg, keys_bg);
    if (int rc = check_launch(what)) return rc;
    size_t tmp = l.sort_tmp_bytes;
    if (rocprim::radix_sort_keys(ws + l.sort_tmp, tmp, (const double*)keys_fg, sorted_fg, (size_t)hw, 0, 64, s) != hipSuccess ||
        rocprim::radix_sort_keys(ws + l.sort_tmp, tmp, (const double*)keys_bg, sorted_bg, (size_t)hw, 0, 64, s) != hipSuccess) {
        set_error("%s: the key sort failed: %s", what, hipGetErrorString(hipGetLastError()));
        return ADAIN_ELAUNCH;
    }
    // the background's unsorted keys are dead once sorted: their array takes the resampled quantile function
    double* resampled = keys_bg;
    hipLaunchKernelGGL(colour_resample_kernel, dim3(pb), dim3(CT_THREADS), 0, s, hw, (const adain_colour_record*)rec, (const double*)sorted_fg,
                       (const double*)sorted_bg, resampled);
    hipLaunchKernelGGL(colour_match_kernel, dim3(pb), dim3(CT_THREADS), 0, s, im, hw, (const adain_colour_record*)rec, (const double*)keys_fg,
                       (const double*)sorted_fg, (const double*)sorted_bg, (const double*)resampled, out);
    return check_launch(what);
}

}  // namespace

}  // namespace adain

using namespace adain;

extern "C" {

size_t adain_colour_transfer_workspace_bytes(int h, int w) {
    Layout l;
    return layout(h, w, &l) ? l.total : 0;
}

int adain_colour_transfer_u8(const uint8_t* fg_u8, const uint8_t* bg_u8, uint8_t* out_u8, int h, int w, void* workspace, adain_stream_t stream) {
    return run(Images{fg_u8, bg_u8, nullptr}, out_u8, h, w, workspace, (hipStream_t)stream, "colour_transfer_u8");
}

int adain_localized_combine_u8(const uint8_t* content_u8, const uint8_t* stylised_u8, const uint8_t* mask_u8, uint8_t* out_u8, int h, int w,
                               void* workspace, adain_stream_t stream) {
    if (!mask_u8) { set_error("localized_combine_u8: null pointer"); return ADAIN_EINVAL; }
    return run(Images{content_u8, stylised_u8, mask_u8}, out_u8, h, w, workspace, (hipStream_t)stream, "localized_combine_u8");
}

}  // extern "C"
