// The integer core of the GIF writer (csrc/gif.hip): code sizes, code widths and the LZW coder of one segment.  Plain C++ that compiles
// for the device and for the host; tools/gif_lzw_check.cpp runs it on the CPU under the sanitizers.  The rules: top of gif.hip.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include "../../include/adain_hip.h"          // ADAIN_GIF_SEGMENT: the pixels of a segment

#if defined(__HIPCC__)
#define GIF_HD __host__ __device__
#else
#define GIF_HD
#endif

namespace adain {
namespace gif {

constexpr int SEGMENT = ADAIN_GIF_SEGMENT;
constexpr int TABLE_SLOTS = 4096;               // open addressing; a segment adds at most SEGMENT - 1 entries: half load
constexpr uint32_t EMPTY = 0xffffffffu;         // key 0xfffff would need prefix code 4095; no code passes 2^8 + 1 + 2048 = 2305
constexpr int HEAD = 19;                        // graphic control extension 8, image descriptor 10, minimum code size 1

// m: 2 for K <= 4, else ceil(log2 K)
GIF_HD inline int min_code_size(int K) {
    int m = 2;
    while ((1 << m) < K) ++m;
    return m;
}

// bits of the k-th code behind a CLEAR (k = 1, 2, ...): the smallest w >= m + 1 with 2^m + 1 + k <= 2^w
GIF_HD inline int code_width(int k, int m) {
    int w = m + 1;
    while ((1 << m) + 1 + k > (1 << w)) ++w;
    return w;
}

// W(c) = w(1) + ... + w(c): width w holds for k up to 2^w - 2^m - 1
GIF_HD inline uint32_t code_bits(int c, int m) {
    uint32_t bits = 0;
    int done = 0;
    for (int w = m + 1; done < c; ++w) {
        const int last = (1 << w) - (1 << m) - 1, upto = c < last ? c : last;
        bits += (uint32_t)(upto - done) * w;
        done = upto;
    }
    return bits;
}

GIF_HD inline uint32_t hash_slot(uint32_t key) { return (key * 2654435761u) >> 20; }         // 12 bits

// Greedy LZW of px[0..count), 1 <= count <= SEGMENT, every px below 2^m, from an empty dictionary: the longest known string, one new
// entry per emitted code except the last.  table: TABLE_SLOTS slots, all EMPTY on entry; a slot is key << 12 | code with key = prefix
// code << 8 | byte.  codes: room for `count`.  Returns the number of codes.  The probe is bounded by the table's size.
GIF_HD inline int lzw_segment(const uint8_t* px, int count, int m, uint32_t* table, uint16_t* codes) {
    uint32_t next = (1u << m) + 2, cur = px[0];
    int c = 0;
    for (int i = 1; i < count; ++i) {
        const uint32_t key = cur << 8 | px[i];
        uint32_t slot = hash_slot(key), found = EMPTY;
        for (int probe = 0; probe < TABLE_SLOTS; ++probe, slot = (slot + 1) & (TABLE_SLOTS - 1)) {
            const uint32_t v = table[slot];
            if (v == EMPTY) break;
            if (v >> 12 == key) { found = v & 0xfff; break; }
        }
        if (found != EMPTY) { cur = found; continue; }
        codes[c++] = (uint16_t)cur;
        if (table[slot] == EMPTY) table[slot] = key << 12 | next;          // always: the table is never more than half full
        ++next;
        cur = px[i];
    }
    codes[c++] = (uint16_t)cur;
    return c;
}

// the data bytes of a frame whose segments sum to `bits` behind the first CLEAR's m + 1
GIF_HD inline uint64_t data_bytes(uint64_t bits) { return (bits + 7) / 8; }
// GCE, descriptor, code size, the data in sub-blocks of 255 with their length bytes, the terminator
GIF_HD inline uint64_t record_bytes(uint64_t D) { return 20 + D + (D + 254) / 255; }

// the proven worst case of a frame of `pixels`: a segment of p pixels emits at most p codes and is closed by one more, W(p + 1) bits
GIF_HD inline uint64_t worst_data_bytes(uint64_t pixels, int m) {
    const uint64_t full = pixels / SEGMENT, rest = pixels % SEGMENT;
    return data_bytes((uint64_t)(m + 1) + full * code_bits(SEGMENT + 1, m) + (rest ? code_bits((int)rest + 1, m) : 0));
}

}  // namespace gif
}  // namespace adain
