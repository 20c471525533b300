// The integer rules of the palette's k-means refinement (csrc/quantize_refine.hip), rules 7-11 behind rules 1-6 of csrc/quantize.hip.
// Plain C++ that compiles for the device and for the host; tools/quantize_refine_check.cpp runs it on the CPU under the sanitizers.  The
// rules: top of quantize_refine.hip.
#pragma once
#include "quantize_cut.h"

namespace adain {
namespace quant {

// One palette's accumulators in a workspace: per entry the count n, the sums S[3] and the far key F, 64 bits each.  n is below 2^32
// (a palette has fewer than 2^32 pixels), S at most 255 n, below 2^40, F below 2^42.
constexpr size_t REFINE_BYTES = (size_t)MAX_COLOURS * 5 * sizeof(uint64_t);
struct Acc {
    uint64_t* n;
    uint64_t* s[3];
    uint64_t* f;
};
QUANT_HD inline Acc acc_at(void* accumulators, size_t p) {
    uint64_t* base = (uint64_t*)((char*)accumulators + p * REFINE_BYTES);
    Acc a;
    a.n = base;
    for (int c = 0; c < 3; ++c) a.s[c] = base + (size_t)(1 + c) * MAX_COLOURS;
    a.f = base + (size_t)4 * MAX_COLOURS;
    return a;
}

// a colour as one number: r << 16 | g << 8 | b, so that "the smallest r, g, b" is the smallest number
QUANT_HD inline uint32_t rgb_of(uint32_t r, uint32_t g, uint32_t b) { return r << 16 | g << 8 | b; }

// rule 7: the squared distance, at most 3 x 255^2 = 195 075, and the key whose minimum over i is the nearest entry, the lowest i among
// equals: d << 8 | i, below 2^26
QUANT_HD inline uint32_t distance(uint32_t r, uint32_t g, uint32_t b, uint32_t entry) {
    const int dr = (int)r - (int)(entry >> 16), dg = (int)g - (int)((entry >> 8) & 255u), db = (int)b - (int)(entry & 255u);
    return (uint32_t)(dr * dr + dg * dg + db * db);
}
QUANT_HD inline uint32_t nearest_key(uint32_t d, uint32_t i) { return d << 8 | i; }

// rule 8: the far key of a pixel at distance d from its entry, and what the maximum of the keys says
QUANT_HD inline uint64_t far_key(uint32_t d, uint32_t rgb) { return (uint64_t)d << 24 | (uint64_t)(0xFFFFFFu - rgb); }
QUANT_HD inline uint32_t far_distance(uint64_t f) { return (uint32_t)(f >> 24); }
QUANT_HD inline uint32_t far_colour(uint64_t f) { return 0xFFFFFFu - (uint32_t)(f & 0xFFFFFFu); }

// rule 9: the centre of n > 0 pixels is rule 6's rounding (quant::entry); an entry without pixels stays
QUANT_HD inline uint32_t centre(uint64_t n, uint64_t s0, uint64_t s1, uint64_t s2, uint32_t old) {
    return n ? rgb_of(entry(s0, n), entry(s1, n), entry(s2, n)) : old;
}

// rule 10: a donor has pixels and one of them away from the entry; donor ia gives before donor ib: the larger distance, then the lower index
QUANT_HD inline bool is_donor(uint64_t n, uint64_t f) { return n > 0 && far_distance(f) > 0; }
QUANT_HD inline bool gives_before(uint64_t fa, int ia, uint64_t fb, int ib) {
    const uint32_t da = far_distance(fa), db = far_distance(fb);
    return da != db ? da > db : ia < ib;
}
QUANT_HD inline bool is_free(uint64_t n, int i, int K) { return i < K && n == 0; }

// ---- the rules in sequence (the host's form; the device runs the same functions with a workgroup's threads side by side) -------------------
// rules 7 and 8 for `count` pixels: added into the accumulators
inline void refine_assign(const uint8_t* pixels, size_t count, const uint32_t* colours, int used, const Acc& a) {
    for (size_t p = 0; p < count; ++p) {
        const uint32_t r = pixels[3 * p], g = pixels[3 * p + 1], b = pixels[3 * p + 2];
        uint32_t best = 0xffffffffu;
        for (int i = 0; i < used; ++i) {
            const uint32_t key = nearest_key(distance(r, g, b, colours[i]), (uint32_t)i);
            if (key < best) best = key;
        }
        const uint32_t j = best & 255u, d = best >> 8;
        a.n[j] += 1, a.s[0][j] += r, a.s[1][j] += g, a.s[2][j] += b;
        const uint64_t f = far_key(d, rgb_of(r, g, b));
        if (f > a.f[j]) a.f[j] = f;
    }
}

// rules 9 to 11 for one palette: colours[256] (zero from *used on) and *used are replaced, the accumulators cleared
inline void refine_update(const Acc& a, int K, uint32_t* colours, int* used) {
    uint32_t gift[MAX_COLOURS];
    int donors = 0;
    for (int i = 0; i < MAX_COLOURS; ++i) {
        if (!is_donor(a.n[i], a.f[i])) continue;
        int rank = 0;
        for (int o = 0; o < MAX_COLOURS; ++o)
            if (o != i && is_donor(a.n[o], a.f[o]) && gives_before(a.f[o], o, a.f[i], i)) ++rank;
        gift[rank] = far_colour(a.f[i]);
        ++donors;
    }
    int taken = 0, next_used = *used;
    for (int i = 0; i < MAX_COLOURS; ++i) {
        if (is_free(a.n[i], i, K) && taken < donors) {
            colours[i] = gift[taken++];
            if (i + 1 > next_used) next_used = i + 1;
        } else {
            colours[i] = centre(a.n[i], a.s[0][i], a.s[1][i], a.s[2][i], colours[i]);
        }
    }
    *used = next_used;
    for (int i = 0; i < MAX_COLOURS; ++i) a.n[i] = a.s[0][i] = a.s[1][i] = a.s[2][i] = a.f[i] = 0;
}

}  // namespace quant
}  // namespace adain
