// PIL.Image.resize(size, resample) of uint8 L and RGB images for all six filters, bit for bit, on gfx950 - the palette page's
// _downsample_image (gui/second_page.py), the NEAREST resize of the localized composite (localized.py), the LANCZOS and BICUBIC
// resizes of the modelled project's loaders.  The rules: include/adain_hip.h, "PIL.Image.resize for all six filters".
//
// The work is split where the arithmetic splits.  The tap tables are double arithmetic through sin and cos: the host builds them
// (pil_taps.h; adain_pil_resize_taps) and the caller uploads them.  The pixels are integer arithmetic: Pillow's own two passes, a
// horizontal one into a uint8 intermediate in the caller's workspace and a vertical one over it, kx + ky taps per pixel where the
// one-pass kernel of resample.hip pays kx * ky.  A pass whose axis keeps its size is not launched (its fixed-point taps are the
// identity), and a crop window limits the intermediate to the rows and columns it needs.  NEAREST is a gather through two index
// tables.
#include "common.h"
#include "pil_taps.h"

namespace adain {

namespace {

constexpr int PRECISION_BITS = piltaps::PRECISION_BITS;

__device__ __forceinline__ int clip8(int v) {
    v >>= PRECISION_BITS;
    return v < 0 ? 0 : (v > 255 ? 255 : v);
}

constexpr int out_channels(int pix) { return pix == 1 ? 1 : 3; }

// One axis of a launch: the tables (device) and what the kernels clamp them to
struct Axis {
    const int32_t* __restrict__ bounds;      // [out][2]
    const int32_t* __restrict__ taps;        // [out][ksize]
    int in_size, ksize;
};

// first source index and tap count of output index i, held inside the source and the table whatever the table says
__device__ __forceinline__ void tap_window(const Axis& a, int i, int* lo, int* n) {
    int first = a.bounds[2 * i], count = a.bounds[2 * i + 1];
    first = first < 0 ? 0 : (first > a.in_size ? a.in_size : first);
    count = count < 0 ? 0 : (count > a.ksize ? a.ksize : count);
    if (count > a.in_size - first) count = a.in_size - first;
    *lo = first;
    *n = count;
}

// HORIZONTAL pass: dst[img][r][ox][C] = clip8(2^21 + sum_x src[img][row0 + r][xmin + x][.] * k[x]) for the window columns x0 + ox.
// One thread per intermediate pixel and all its channels; lanes run along ox, so a shrink reads the row in strides of the scale and
// an enlargement reads neighbouring bytes.
template <int PIX>
__global__ __launch_bounds__(256) void pil_horizontal_kernel(const uint8_t* __restrict__ src, uint8_t* __restrict__ dst, int hi, int wi, Axis ax, int row0,
                                                             int rows, int x0, int cw) {
    constexpr int C = out_channels(PIX);
    const int ox = blockIdx.x * 64 + threadIdx.x, r = blockIdx.y * 4 + threadIdx.y;
    if (ox >= cw || r >= rows) return;
    int xmin, xn;
    tap_window(ax, ox + x0, &xmin, &xn);
    const int32_t* __restrict__ k = ax.taps + (size_t)(ox + x0) * ax.ksize;
    const uint8_t* __restrict__ row = src + (((size_t)blockIdx.z * hi + row0 + r) * wi + xmin) * PIX;
    int acc[C];
#pragma unroll
    for (int c = 0; c < C; ++c) acc[c] = 1 << (PRECISION_BITS - 1);
    for (int x = 0; x < xn; ++x) {
        const int kv = k[x];
#pragma unroll
        for (int c = 0; c < C; ++c) acc[c] += (int)row[(size_t)x * PIX + c] * kv;
    }
    uint8_t* __restrict__ o = dst + (((size_t)blockIdx.z * rows + r) * cw + ox) * C;
#pragma unroll
    for (int c = 0; c < C; ++c) o[c] = (uint8_t)clip8(acc[c]);
}

// VERTICAL pass: dst[img][oy][ox][C] = clip8(2^21 + sum_y src[img][ymin - row0 + y][col0 + ox][.] * k[y]) for the window rows y0 + oy.
// src: the intermediate (rows from source row row0, cw columns, PIX = C) or, when the horizontal pass is skipped, the source itself.
// One thread per output pixel; a wave is 64 neighbouring columns of one output row, so its taps are one scalar read per row of the
// column and its loads are neighbouring bytes.
template <int PIX>
__global__ __launch_bounds__(256) void pil_vertical_kernel(const uint8_t* __restrict__ src, uint8_t* __restrict__ dst, int src_rows, int src_w, int row0,
                                                           int col0, Axis ay, int y0, int ch, int cw) {
    constexpr int C = out_channels(PIX);
    const int ox = blockIdx.x * 64 + threadIdx.x;
    const int oy = __builtin_amdgcn_readfirstlane(blockIdx.y * 4 + threadIdx.y);      // a wave is one threadIdx.y
    if (oy >= ch) return;
    int ymin, yn;
    tap_window(ay, oy + y0, &ymin, &yn);
    ymin -= row0;
    if (ymin < 0) ymin = 0;
    if (yn > src_rows - ymin) yn = src_rows - ymin;
    if (ox >= cw) return;
    const int32_t* __restrict__ k = ay.taps + (size_t)(oy + y0) * ay.ksize;
    const uint8_t* __restrict__ col = src + (((size_t)blockIdx.z * src_rows + ymin) * src_w + col0 + ox) * PIX;
    int acc[C];
#pragma unroll
    for (int c = 0; c < C; ++c) acc[c] = 1 << (PRECISION_BITS - 1);
    for (int y = 0; y < yn; ++y) {
        const int kv = k[y];
        const uint8_t* __restrict__ p = col + (size_t)y * src_w * PIX;
#pragma unroll
        for (int c = 0; c < C; ++c) acc[c] += (int)p[c] * kv;
    }
    uint8_t* __restrict__ o = dst + (((size_t)blockIdx.z * ch + oy) * cw + ox) * C;
#pragma unroll
    for (int c = 0; c < C; ++c) o[c] = (uint8_t)clip8(acc[c]);
}

// NEAREST: dst[img][oy][ox] = src[img][yidx][xidx], or 0 where either table marks its index as outside the source.
// COPY (both tables null): the window of a resize that keeps the size.
template <int PIX>
__global__ __launch_bounds__(256) void pil_gather_kernel(const uint8_t* __restrict__ src, uint8_t* __restrict__ dst, int hi, int wi,
                                                         const int32_t* __restrict__ xb, const int32_t* __restrict__ yb, int y0, int x0, int ch, int cw) {
    constexpr int C = out_channels(PIX);
    const int ox = blockIdx.x * 64 + threadIdx.x, oy = blockIdx.y * 4 + threadIdx.y;
    if (ox >= cw || oy >= ch) return;
    int sx = ox + x0, sy = oy + y0;
    bool inside = true;
    if (xb) {
        inside = xb[2 * sx + 1] != 0 && yb[2 * sy + 1] != 0;
        sx = xb[2 * sx];
        sy = yb[2 * sy];
        inside = inside && sx >= 0 && sx < wi && sy >= 0 && sy < hi;
    }
    uint8_t* __restrict__ o = dst + (((size_t)blockIdx.z * ch + oy) * cw + ox) * C;
    const uint8_t* __restrict__ p = src + (((size_t)blockIdx.z * hi + (inside ? sy : 0)) * wi + (inside ? sx : 0)) * PIX;
#pragma unroll
    for (int c = 0; c < C; ++c) o[c] = inside ? p[c] : (uint8_t)0;
}

// What a launch does, from sizes alone (host): which passes run, the source rows the horizontal pass covers, the workspace
struct Plan {
    bool nearest, horizontal, vertical;
    int row0, rows;              // source rows [row0, row0 + rows) the vertical taps of the window reach
    size_t workspace;            // the uint8 intermediate [n][rows][cw][C] when both passes run, else 0
};

bool good_pixel_bytes(int pixel_bytes) { return pixel_bytes == 1 || pixel_bytes == 3 || pixel_bytes == 4; }

// -> 0 and the plan, or ADAIN_EINVAL with the error set
int make_plan(const char* who, int n, int hi, int wi, int ho, int wo, int channels, int filter, int y0, int x0, int ch, int cw, Plan* p) {
    char why[160];
    if (!good_pixel_bytes(channels)) { set_error("%s: pixels of 1 (L), 3 (RGB) or 4 (RGBX) bytes, got %d", who, channels); return ADAIN_EINVAL; }
    if (n < 1) { set_error("%s: n must be at least 1, got %d", who, n); return ADAIN_EINVAL; }
    if (piltaps::check_axis(filter, wi, wo, why, sizeof why) || piltaps::check_axis(filter, hi, ho, why, sizeof why)) {
        set_error("%s: %dx%d -> %dx%d: %s", who, hi, wi, ho, wo, why);
        return ADAIN_EINVAL;
    }
    if (y0 < 0 || x0 < 0 || ch < 1 || cw < 1 || (long long)y0 + ch > ho || (long long)x0 + cw > wo) {
        set_error("%s: crop window (%d, %d, %d x %d) outside the %d x %d result", who, y0, x0, ch, cw, ho, wo);
        return ADAIN_EINVAL;
    }
    p->nearest = filter == piltaps::NEAREST;
    p->horizontal = !p->nearest && wi != wo;
    p->vertical = !p->nearest && hi != ho;
    p->row0 = y0, p->rows = ch;
    p->workspace = 0;
    if (p->horizontal && p->vertical) {
        int first, count, last, last_count;
        piltaps::axis_bounds(filter, hi, ho, y0, &first, &count);
        piltaps::axis_bounds(filter, hi, ho, y0 + ch - 1, &last, &last_count);
        p->row0 = first;
        p->rows = last + last_count - first;          // xmin and xmin + count both grow with the index
        p->workspace = (size_t)n * p->rows * cw * (channels == 1 ? 1 : 3);
    }
    return 0;
}

bool overlap(const void* a, size_t a_bytes, const void* b, size_t b_bytes) {
    const uintptr_t a0 = (uintptr_t)a, b0 = (uintptr_t)b;
    return a_bytes && b_bytes && a0 < b0 + b_bytes && b0 < a0 + a_bytes;
}

template <int PIX>
int launch_passes(const Plan& p, const uint8_t* src, int n, int hi, int wi, uint8_t* dst, const Axis& ax, const Axis& ay, int y0, int x0, int ch, int cw,
                  uint8_t* mid, hipStream_t s) {
    constexpr int C = out_channels(PIX);
    const dim3 b(64, 4);
    const auto grid = [&](int rows) { return dim3((cw + 63) / 64, (rows + 3) / 4, n); };
    if (p.nearest || (!p.horizontal && !p.vertical)) {
        hipLaunchKernelGGL(pil_gather_kernel<PIX>, grid(ch), b, 0, s, src, dst, hi, wi, p.nearest ? ax.bounds : nullptr, p.nearest ? ay.bounds : nullptr, y0,
                           x0, ch, cw);
        return check_launch(p.nearest ? "resize_pil_u8 (gather)" : "resize_pil_u8 (copy)");
    }
    if (p.horizontal) {
        hipLaunchKernelGGL(pil_horizontal_kernel<PIX>, grid(p.rows), b, 0, s, src, p.vertical ? mid : dst, hi, wi, ax, p.row0, p.rows, x0, cw);
        if (int r = check_launch("resize_pil_u8 (horizontal pass)")) return r;
        if (!p.vertical) return 0;
        hipLaunchKernelGGL(pil_vertical_kernel<C>, grid(ch), b, 0, s, mid, dst, p.rows, cw, p.row0, 0, ay, y0, ch, cw);
    } else {
        hipLaunchKernelGGL(pil_vertical_kernel<PIX>, grid(ch), b, 0, s, src, dst, hi, wi, 0, x0, ay, y0, ch, cw);
    }
    return check_launch("resize_pil_u8 (vertical pass)");
}

}  // namespace

int pil_resize_taps_bytes(int filter, int in_size, int out_size, int* ksize, size_t* bytes) {
    char why[160];
    if (!ksize || !bytes) { set_error("pil_resize_taps_bytes: null result pointer"); return ADAIN_EINVAL; }
    if (piltaps::check_axis(filter, in_size, out_size, why, sizeof why)) { set_error("pil_resize_taps_bytes: %s", why); return ADAIN_EINVAL; }
    *ksize = piltaps::axis_ksize(filter, in_size, out_size);
    *bytes = piltaps::axis_bytes(out_size, *ksize);
    return 0;
}

int pil_resize_taps(int filter, int in_size, int out_size, int32_t* bounds, int32_t* taps) {
    char why[160];
    if (piltaps::check_axis(filter, in_size, out_size, why, sizeof why)) { set_error("pil_resize_taps: %s", why); return ADAIN_EINVAL; }
    if (!bounds || (!taps && filter != piltaps::NEAREST)) { set_error("pil_resize_taps: null table pointer"); return ADAIN_EINVAL; }
    piltaps::axis_tables(filter, in_size, out_size, bounds, taps);
    return 0;
}

int resize_pil_u8_bytes(int n, int hi, int wi, int ho, int wo, int channels, int filter, int y0, int x0, int ch, int cw, size_t* workspace_bytes) {
    Plan p;
    if (!workspace_bytes) { set_error("resize_pil_u8_bytes: null result pointer"); return ADAIN_EINVAL; }
    if (int r = make_plan("resize_pil_u8_bytes", n, hi, wi, ho, wo, channels, filter, y0, x0, ch, cw, &p)) return r;
    *workspace_bytes = p.workspace;
    return 0;
}

int launch_resize_pil_u8(const uint8_t* src, int pixel_bytes, int n, int hi, int wi, uint8_t* dst, int ho, int wo, int filter, const int32_t* x_bounds,
                         const int32_t* x_taps, int x_ksize, const int32_t* y_bounds, const int32_t* y_taps, int y_ksize, int y0, int x0, int ch, int cw,
                         void* workspace, size_t workspace_bytes, hipStream_t s) {
    const char* who = "resize_pil_u8";
    Plan p;
    if (int r = make_plan(who, n, hi, wi, ho, wo, pixel_bytes, filter, y0, x0, ch, cw, &p)) return r;
    const int kx = piltaps::axis_ksize(filter, wi, wo), ky = piltaps::axis_ksize(filter, hi, ho);
    if (x_ksize != kx || y_ksize != ky) {
        set_error("%s: tap tables of %d and %d taps, filter %d needs %d for %d -> %d and %d for %d -> %d", who, x_ksize, y_ksize, filter, kx, wi, wo, ky, hi, ho);
        return ADAIN_EINVAL;
    }
    if (!src || !dst || !x_bounds || !y_bounds || (!p.nearest && (!x_taps || !y_taps))) { set_error("%s: null pointer", who); return ADAIN_EINVAL; }
    if (p.workspace) {
        if (int r = check_workspace(who, workspace, workspace_bytes, p.workspace, 1)) return r;
    }
    const int C = out_channels(pixel_bytes);
    const size_t src_bytes = (size_t)n * hi * wi * pixel_bytes, dst_bytes = (size_t)n * ch * cw * C;
    const void* reads[5] = {src, x_bounds, x_taps, y_bounds, y_taps};
    const size_t read_bytes[5] = {src_bytes, (size_t)wo * 2 * sizeof(int32_t), (size_t)wo * kx * sizeof(int32_t), (size_t)ho * 2 * sizeof(int32_t),
                                  (size_t)ho * ky * sizeof(int32_t)};
    for (int i = 0; i < 5; ++i)
        if (reads[i] && (overlap(reads[i], read_bytes[i], dst, dst_bytes) || overlap(reads[i], read_bytes[i], workspace, p.workspace))) {
            set_error("%s: the result and the workspace must not overlap the source or the tables", who);
            return ADAIN_EINVAL;
        }
    if (overlap(dst, dst_bytes, workspace, p.workspace)) { set_error("%s: the result and the workspace overlap", who); return ADAIN_EINVAL; }
    if (n > 65535 || (p.rows + 3) / 4 > 65535 || (ch + 3) / 4 > 65535) { set_error("%s: grid too large", who); return ADAIN_EINVAL; }
    const Axis ax{x_bounds, x_taps, wi, kx}, ay{y_bounds, y_taps, hi, ky};
    uint8_t* mid = (uint8_t*)workspace;
    switch (pixel_bytes) {
        case 1: return launch_passes<1>(p, src, n, hi, wi, dst, ax, ay, y0, x0, ch, cw, mid, s);
        case 3: return launch_passes<3>(p, src, n, hi, wi, dst, ax, ay, y0, x0, ch, cw, mid, s);
        default: return launch_passes<4>(p, src, n, hi, wi, dst, ax, ay, y0, x0, ch, cw, mid, s);
    }
}

}  // namespace adain
