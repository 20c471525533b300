// OpenCV's float cv::resize (resize.cpp, INTER_LINEAR on float data) as the flow estimators use it: flow.hip (level images; the
// frame preparation and the flow upscale take the taps) and tvl1.hip (scale images, flow upscale).
//   mode      an equal size is a copy (0); an exact 2x shrink on both axes is INTER_AREA's fast path (1: 2x2 mean over the source
//             pixels inside the image); anything else is linear (2).
//   linear    fx = (float)((dx+0.5)*scale - 0.5), taps (1-fx, fx); x taps clamped at both ends with fraction 0, rows clamped with
//             their weights kept.
// Both files are compiled with -ffp-contract=off: every multiply and add below is rounded on its own, as in OpenCV's CPU build and
// in the NumPy restatements.
#pragma once
#include <hip/hip_runtime.h>
#include <math.h>
#include <stddef.h>

namespace adain {

__device__ __forceinline__ int clampi(int v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : v); }

// cv::resize's choice for (ssize -> dsize) with the source-per-destination scales sx, sy
inline int resize_mode(int hi, int wi, int ho, int wo, double sx, double sy) {
    if (ho == hi && wo == wi) return 0;
    const int ix = (int)nearbyint(sx), iy = (int)nearbyint(sy);
    const bool fast = fabs(sx - ix) < 2.220446049250313e-16 && fabs(sy - iy) < 2.220446049250313e-16;
    return fast && ix == 2 && iy == 2 ? 1 : 2;
}

// INTER_LINEAR source index and fraction of one output index (resize.cpp's coefficient loop): xaxis = the x axis rule (fraction 0
// at both ends); the y axis keeps its fraction and clamps the rows
struct LinTap { int s0, s1; float f; };
__device__ __forceinline__ LinTap lin_tap(int d, int ssize, double scale, bool xaxis) {
    float f = (float)((d + 0.5) * scale - 0.5);
    int s = (int)floorf(f);
    f -= (float)s;
    LinTap t;
    if (xaxis) {
        if (s < 0) { f = 0.f; s = 0; }
        if (s >= ssize - 1) { f = 0.f; s = ssize - 1; }
        t.s0 = s;
        t.s1 = min(s + 1, ssize - 1);
    } else {
        t.s0 = clampi(s, 0, ssize - 1);
        t.s1 = clampi(s + 1, 0, ssize - 1);
    }
    t.f = f;
    return t;
}

// output pixel (x, y) of an sh x sw source in `mode` (resize_mode's); `at(y, x)` reads the source
template <class F>
__device__ __forceinline__ float resample(F at, int sh, int sw, int x, int y, int mode, double sx, double sy) {
    if (mode == 0) return at(y, x);
    if (mode == 1) {
        const int x0 = 2 * x, y0 = 2 * y;
        if (x0 + 1 < sw && y0 + 1 < sh) return (((at(y0, x0) + at(y0, x0 + 1)) + at(y0 + 1, x0)) + at(y0 + 1, x0 + 1)) * 0.25f;
        float sum = 0.f;
        int cnt = 0;
        for (int yy = y0; yy < y0 + 2 && yy < sh; ++yy)
            for (int xx = x0; xx < x0 + 2 && xx < sw; ++xx) { sum += at(yy, xx); ++cnt; }
        return cnt ? sum / (float)cnt : 0.f;
    }
    const LinTap tx = lin_tap(x, sw, sx, true), ty = lin_tap(y, sh, sy, false);
    const float a0 = 1.f - tx.f, a1 = tx.f, b0 = 1.f - ty.f, b1 = ty.f;
    const float h0 = at(ty.s0, tx.s0) * a0 + at(ty.s0, tx.s1) * a1;
    const float h1 = at(ty.s1, tx.s0) * a0 + at(ty.s1, tx.s1) * a1;
    return h0 * b0 + h1 * b1;
}

}  // namespace adain
