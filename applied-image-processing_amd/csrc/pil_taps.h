// The tap and index tables of PIL.Image.resize for uint8 images, on the host: Resample.c's precompute_coeffs + normalize_coeffs_8bpc for
// the five convolution filters and Geometry.c's ImagingScaleAffine index walk for NEAREST (the rules: include/adain_hip.h,
// "PIL.Image.resize for all six filters"; tests/pil_resize_ref.py restates them in Python).
//
// Plain C++ with <cmath> and no HIP call: HAMMING and LANCZOS go through sin and cos, and only the C library's are the ones Pillow
// called - a tap that differs by one unit of 2^-22 changes pixels.  Included by resample_filters.hip (the library's
// adain_pil_resize_taps*) and by tools/pil_taps_check.cpp (a stand-alone program for a sanitised build).
#pragma once
#include <math.h>
#include <stddef.h>
#include <stdint.h>
#include <stdio.h>

#include <vector>

namespace adain {
namespace piltaps {

// +, -, *, / on doubles one by one, as the x86-64 build of Pillow rounds them
#if defined(__clang__)
#pragma clang fp contract(off)
#else
#pragma STDC FP_CONTRACT OFF
#endif

constexpr int NEAREST = 0, LANCZOS = 1, BILINEAR = 2, BICUBIC = 3, BOX = 4, HAMMING = 5;      // PIL.Image.Resampling
constexpr int PRECISION_BITS = 32 - 8 - 2;                                                     // Resample.c: 22
constexpr int MAX_SIDE = 1 << 24;          // every side in [1, 2^24)
constexpr int MAX_SHRINK = 256;            // in <= 256 * out: at most 3 * 256 * 2 + 1 = 1537 taps (LANCZOS)
constexpr double PI = 3.14159265358979323846;      // M_PI

inline double filter_support(int filter) {
    switch (filter) {
        case BOX: return 0.5;
        case BILINEAR: return 1.0;
        case HAMMING: return 1.0;
        case BICUBIC: return 2.0;
        case LANCZOS: return 3.0;
        default: return 0.0;
    }
}

inline double sinc(double x) {
    if (x == 0.0) return 1.0;
    x = x * PI;
    return sin(x) / x;
}

inline double filter_value(int filter, double x) {
    switch (filter) {
        case BOX: return (x > -0.5 && x <= 0.5) ? 1.0 : 0.0;
        case BILINEAR:
            if (x < 0.0) x = -x;
            return x < 1.0 ? 1.0 - x : 0.0;
        case HAMMING:
            if (x < 0.0) x = -x;
            if (x == 0.0) return 1.0;
            if (x >= 1.0) return 0.0;
            x = x * PI;
            return sin(x) / x * (0.54f + 0.46f * cos(x));      // float constants widened to double, as Resample.c writes them
        case BICUBIC: {
            const double a = -0.5;
            if (x < 0.0) x = -x;
            if (x < 1.0) return ((a + 2.0) * x - (a + 3.0)) * x * x + 1;
            if (x < 2.0) return (((x - 5) * x + 8) * x - 4) * a;
            return 0.0;
        }
        case LANCZOS: return (-3.0 <= x && x < 3.0) ? sinc(x) * sinc(x / 3) : 0.0;
        default: return 0.0;
    }
}

// in / out as Pillow forms it: the box's float corners, widened (exact below 2^24)
inline double axis_scale(int in_size, int out_size) { return (double)((float)in_size - 0.f) / out_size; }

// nullptr, or why the axis is refused (text into err)
inline const char* check_axis(int filter, int in_size, int out_size, char* err, size_t err_len) {
    if (filter < NEAREST || filter > HAMMING)
        snprintf(err, err_len, "unknown filter %d (Pillow's codes: 0 NEAREST, 1 LANCZOS, 2 BILINEAR, 3 BICUBIC, 4 BOX, 5 HAMMING)", filter);
    else if (in_size < 1 || out_size < 1 || in_size >= MAX_SIDE || out_size >= MAX_SIDE)
        snprintf(err, err_len, "bad size %d -> %d (every side must be in [1, 2^24))", in_size, out_size);
    else if ((long long)in_size > (long long)MAX_SHRINK * out_size)
        snprintf(err, err_len, "shrink factor above %d (%d -> %d) is not supported", MAX_SHRINK, in_size, out_size);
    else
        return nullptr;
    return err;
}

// taps per output index of a checked axis; 0 for NEAREST
inline int axis_ksize(int filter, int in_size, int out_size) {
    if (filter == NEAREST) return 0;
    double filterscale = axis_scale(in_size, out_size);
    if (filterscale < 1.0) filterscale = 1.0;
    return (int)ceil(filter_support(filter) * filterscale) * 2 + 1;
}

// first source index and tap count of output index xx of a convolution filter (no sin, no cos: the launcher asks for the rows and
// columns a crop window needs without the tables)
inline void axis_bounds(int filter, int in_size, int out_size, int xx, int* xmin_out, int* count_out) {
    const double scale = axis_scale(in_size, out_size);
    double filterscale = scale;
    if (filterscale < 1.0) filterscale = 1.0;
    const double support = filter_support(filter) * filterscale;
    const double center = 0.0 + (xx + 0.5) * scale;
    int xmin = (int)(center - support + 0.5);
    if (xmin < 0) xmin = 0;
    int xmax = (int)(center + support + 0.5);
    if (xmax > in_size) xmax = in_size;
    *xmin_out = xmin;
    *count_out = xmax - xmin;
}

inline size_t axis_bytes(int out_size, int ksize) { return (size_t)out_size * (2 + (size_t)ksize) * sizeof(int32_t); }

// bounds [out][2], taps [out][ksize] of a checked axis
inline void axis_tables(int filter, int in_size, int out_size, int32_t* bounds, int32_t* taps) {
    if (filter == NEAREST) {
        // ImagingScaleAffine: a running sum, not (i + 0.5) * s.  o starts positive and grows, and without a box the last index stays
        // below in - Pillow's own bounds test is kept all the same: an index outside [0, in) leaves the pixel 0
        const double s = axis_scale(in_size, out_size);
        double o = s * 0.5;
        for (int i = 0; i < out_size; ++i) {
            const int src = o < 0 ? -1 : (int)o;
            bounds[2 * i] = src;
            bounds[2 * i + 1] = (src >= 0 && src < in_size) ? 1 : 0;
            o += s;
        }
        return;
    }
    const int ksize = axis_ksize(filter, in_size, out_size);
    const double scale = axis_scale(in_size, out_size);
    double filterscale = scale;
    if (filterscale < 1.0) filterscale = 1.0;
    const double ss = 1.0 / filterscale;
    std::vector<double> w((size_t)ksize);
    for (int xx = 0; xx < out_size; ++xx) {
        const double center = 0.0 + (xx + 0.5) * scale;
        int xmin, xmax;
        axis_bounds(filter, in_size, out_size, xx, &xmin, &xmax);
        double ww = 0.0;
        for (int x = 0; x < xmax; ++x) {
            w[x] = filter_value(filter, (x + xmin - center + 0.5) * ss);
            ww += w[x];
        }
        int32_t* k = taps + (size_t)xx * ksize;
        for (int x = 0; x < ksize; ++x) {
            double v = 0.0;
            if (x < xmax) {
                v = w[x];
                if (ww != 0.0) v /= ww;
            }
            k[x] = v < 0 ? (int)(-0.5 + v * (1 << PRECISION_BITS)) : (int)(0.5 + v * (1 << PRECISION_BITS));
        }
        bounds[2 * xx] = xmin;
        bounds[2 * xx + 1] = xmax;
    }
}

}  // namespace piltaps
}  // namespace adain
