// The integer core of the palette chooser (csrc/quantize.hip): the grid of cell moments, its summed-area form, and the box and cut rules.
// Plain C++ that compiles for the device and for the host; tools/quantize_check.cpp runs it on the CPU under the sanitizers.  The rules:
// top of quantize.hip.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include "../../include/adain_hip.h"

#if defined(__HIPCC__)
#define QUANT_HD __host__ __device__
#else
#define QUANT_HD
#endif

namespace adain {
namespace quant {

typedef unsigned __int128 u128;          // products only: nothing here divides one

constexpr int SIDE = 32;                          // cells along a channel: value >> 3
constexpr int CELLS = SIDE * SIDE * SIDE;
constexpr size_t GRID_BYTES = (size_t)CELLS * (sizeof(uint32_t) + 4 * sizeof(uint64_t));          // one palette's five planes
constexpr int MAX_COLOURS = 256;

QUANT_HD inline uint32_t cell_of(uint32_t r, uint32_t g, uint32_t b) { return (r >> 3) << 10 | (g >> 3) << 5 | (b >> 3); }

// The five planes of palette p in a workspace: the count, then Sr, Sg, Sb and Q.  First the cells' own moments, after sat_* their
// inclusive prefix sums over (r, g, b).
struct Grid {
    uint32_t* w;
    uint64_t* s[3];
    uint64_t* q;
};
QUANT_HD inline Grid grid_at(void* workspace, size_t p) {
    char* base = (char*)workspace + p * GRID_BYTES;
    Grid g;
    g.w = (uint32_t*)base;
    uint64_t* wide = (uint64_t*)(base + (size_t)CELLS * sizeof(uint32_t));
    for (int c = 0; c < 3; ++c) g.s[c] = wide + (size_t)c * CELLS;
    g.q = wide + (size_t)3 * CELLS;
    return g;
}

// One line of a prefix pass: 32 elements `stride` apart.  All of them are read before the first is written, so that the loads do not
// wait for one another behind stores they might alias.
template <class T>
QUANT_HD inline void scan_line(T* p, int stride) {
    T v[SIDE];
#pragma unroll
    for (int i = 0; i < SIDE; ++i) v[i] = p[(size_t)i * stride];
#pragma unroll
    for (int i = 1; i < SIDE; ++i) v[i] += v[i - 1];
#pragma unroll
    for (int i = 0; i < SIDE; ++i) p[(size_t)i * stride] = v[i];
}
// The three passes, `line` of 1024 in each: along b, along g, along r.  A pass reads what the pass before wrote in other lines.
template <class T>
QUANT_HD inline void scan_pass(T* plane, int pass, int line) {
    if (pass == 0) scan_line(plane + ((size_t)line << 5), 1);
    else if (pass == 1) scan_line(plane + ((size_t)(line >> 5) << 10 | (size_t)(line & 31)), SIDE);
    else scan_line(plane + line, SIDE * SIDE);
}

// An inclusive range of cells; axis 0 r, 1 g, 2 b
struct Box {
    int8_t lo[3], hi[3];
};

// The sum of a plane's cells inside the box from the plane's prefix sums: 8 reads.  Unsigned arithmetic wraps and lands on the sum.
template <class T>
QUANT_HD inline uint64_t box_sum(const T* sat, const Box& x) {
    uint64_t acc = 0;
    for (int c = 0; c < 8; ++c) {
        const int r = c & 4 ? x.lo[0] - 1 : x.hi[0], g = c & 2 ? x.lo[1] - 1 : x.hi[1], b = c & 1 ? x.lo[2] - 1 : x.hi[2];
        if (r < 0 || g < 0 || b < 0) continue;
        const uint64_t v = sat[r << 10 | g << 5 | b];
        acc += ((c >> 2) + (c >> 1) + c) & 1 ? (uint64_t)0 - v : v;
    }
    return acc;
}

// The pixels of the box's slab at position t of `axis`
QUANT_HD inline uint64_t slab_count(const uint32_t* sat_w, Box x, int axis, int t) {
    x.lo[axis] = x.hi[axis] = (int8_t)t;
    return box_sum(sat_w, x);
}

struct Moments {
    uint64_t w, s[3], q;
};
QUANT_HD inline Moments box_moments(const Grid& g, const Box& x) {
    Moments m;
    m.w = box_sum(g.w, x);
    for (int c = 0; c < 3; ++c) m.s[c] = box_sum(g.s[c], x);
    m.q = box_sum(g.q, x);
    return m;
}

// w E = w Q - |S|^2, below 2^82 for w < 2^32
QUANT_HD inline u128 error_numerator(const Moments& m) {
    return (u128)m.w * m.q - ((u128)m.s[0] * m.s[0] + (u128)m.s[1] * m.s[1] + (u128)m.s[2] * m.s[2]);
}

// What the choice looks at: a box can be split when it has more than one cell along some axis
struct Key {
    u128 num;
    uint64_t w;
    int splittable;
};
QUANT_HD inline int splittable(const Box& x) { return x.hi[0] > x.lo[0] || x.hi[1] > x.lo[1] || x.hi[2] > x.lo[2]; }

// Box ia is split rather than box ib: the larger E = num / w, compared exactly as num_a w_b against num_b w_a (below 2^114); the lower
// index among equals
QUANT_HD inline bool chosen_over(const Key& a, int ia, const Key& b, int ib) {
    if (!a.splittable) return false;
    if (!b.splittable) return true;
    const u128 l = a.num * b.w, r = b.num * a.w;
    if (l != r) return l > r;
    return ia < ib;
}

// The longest side in cells; among equals g, then r, then b
QUANT_HD inline int split_axis(const Box& x) {
    const int lr = x.hi[0] - x.lo[0], lg = x.hi[1] - x.lo[1], lb = x.hi[2] - x.lo[2];
    if (lg >= lr && lg >= lb) return 1;
    return lr >= lb ? 0 : 2;
}

// m[t]: the slab counts at positions lo..hi (indexed by position), w their sum: the smallest k with m[lo] + ... + m[k] >= ceil(w / 2),
// at most hi - 1.  [lo..k] stays, [k + 1..hi] is the new box.
QUANT_HD inline int cut_position(const uint32_t* m, int lo, int hi, uint64_t w) {
    const uint64_t half = (w + 1) / 2;
    uint64_t sum = 0;
    int k = hi;
    for (int t = lo; t <= hi; ++t) {
        sum += m[t];
        if (sum >= half) { k = t; break; }
    }
    return k < hi - 1 ? k : hi - 1;
}

// mask: bit t set when the slab at t holds a pixel (never zero for a box with pixels) -> the tight range
QUANT_HD inline void tight_range(uint32_t mask, int8_t* lo, int8_t* hi) {
    *lo = (int8_t)__builtin_ctz(mask);
    *hi = (int8_t)(31 - __builtin_clz(mask));
}

// round half up of S / w
QUANT_HD inline uint8_t entry(uint64_t s, uint64_t w) { return (uint8_t)((2 * s + w) / (2 * w)); }

// ---- the rules in sequence (the host's form; the device runs the same functions with a workgroup's threads side by side) -------------------
inline Box tightened(const Grid& g, Box x) {
    for (int a = 0; a < 3; ++a) {
        uint32_t mask = 0;
        for (int t = x.lo[a]; t <= x.hi[a]; ++t)
            if (slab_count(g.w, x, a, t)) mask |= 1u << t;
        tight_range(mask, &x.lo[a], &x.hi[a]);          // the other axes' slabs hold the same pixels: the order does not matter
    }
    return x;
}

// g: prefix sums of at least one pixel.  palette: 256 x 3, entries from `used` on zero.  Returns used.
inline int median_cut(const Grid& g, int K, uint8_t* palette) {
    Box box[MAX_COLOURS];
    Moments mom[MAX_COLOURS];
    Key key[MAX_COLOURS];
    auto settle = [&](int i, const Box& loose) {
        box[i] = tightened(g, loose);
        mom[i] = box_moments(g, box[i]);
        key[i] = Key{error_numerator(mom[i]), mom[i].w, splittable(box[i])};
    };
    settle(0, Box{{0, 0, 0}, {SIDE - 1, SIDE - 1, SIDE - 1}});
    int used = 1;
    while (used < K) {
        int best = 0;
        for (int i = 1; i < used; ++i)
            if (chosen_over(key[i], i, key[best], best)) best = i;
        if (!key[best].splittable) break;
        const Box x = box[best];
        const int a = split_axis(x);
        uint32_t m[SIDE] = {};
        for (int t = x.lo[a]; t <= x.hi[a]; ++t) m[t] = (uint32_t)slab_count(g.w, x, a, t);
        const int k = cut_position(m, x.lo[a], x.hi[a], mom[best].w);
        Box low = x, high = x;
        low.hi[a] = (int8_t)k, high.lo[a] = (int8_t)(k + 1);
        settle(best, low);
        settle(used++, high);
    }
    for (int i = 0; i < MAX_COLOURS; ++i)
        for (int c = 0; c < 3; ++c) palette[3 * i + c] = i < used ? entry(mom[i].s[c], mom[i].w) : 0;
    return used;
}

}  // namespace quant
}  // namespace adain
