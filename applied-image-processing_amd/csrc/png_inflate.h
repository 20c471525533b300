// The inflate and unfilter cores of the PNG decoder (png_decode.hip), written so that the same source compiles for the host: the device
// kernels and tools/png_decode_check.cpp (a stand-alone program for a sanitised CPU build) both run exactly this code.  The rules are
// RFC 1950 / 1951 and the PNG specification's filters, restated in tests/png_decode_ref.py.
//
// inflate: ONE thread runs `step` - a block header with its code tables, up to BATCH tokens, or the trailer - and leaves the tokens with
//   their output positions in the State; then LANES threads write them (`write_stored`, `write_literals`, `write_match` per match in
//   order; on the device a barrier stands between them, on the host the lanes run one after the other).  The last 64 KiB of output live
//   in `ring`, which is what matches read; `out` is only written.
// unfilter: bands of 64 rows as a diagonal wavefront - lane j works on row r0 + j one pixel behind lane j - 1 and gets `up` and `up-left`
//   from that lane's last two results.  On the device a lane is a thread and the results travel by shuffle (L = 1); on the host one
//   thread carries all 64 lanes in arrays (L = 64).
//
// Totality on damaged input: every read of the stream goes through Bits, which never passes `limit` (<= the file's own length); every
// token is checked against the output's size S before it is recorded and a distance against the bytes written so far; every step
// consumes at least one bit of input, ends the stream or sets a status, so a file takes at most 8 * length + 2 steps.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include "../../include/adain_hip.h"

#if defined(__HIPCC__)
#define PNGD_HD __host__ __device__
#else
#define PNGD_HD
#endif

namespace adain {
namespace pngd {

constexpr int BATCH = 64;                   // tokens per step
constexpr int FAST_BITS = 10;               // codes up to this length are found by one lookup
constexpr uint32_t RING = 65536;            // the window (32768) and a batch's output (at most 64 * 258) behind it, a power of two
constexpr uint32_t RING_MASK = RING - 1;
constexpr int STAGE = 1024;                 // input bytes a step can see: a dynamic header has at most 4498 bits, a batch 64 * 48
constexpr uint32_t ADLER_MOD = 65521;
constexpr int BAND = 64;                    // rows the unfilter handles at once

enum Mode { MODE_HEADER = 0, MODE_CODES = 1, MODE_TRAILER = 2, MODE_DONE = 3 };

struct Huff {
    uint16_t fast[1 << FAST_BITS];          // for the next FAST_BITS bits: length << 9 | symbol of the code that starts there, 0: none that short
    uint16_t count[16];                     // codes per length
    uint16_t symbol[288];                   // symbols ordered by (length, symbol)
};

struct Tables {
    Huff ll, d;
    uint8_t lens[320];                      // the lengths being read: HLIT + HDIST of them
};

struct State {
    uint64_t bitbuf;                        // bits loaded and not consumed, LSB first
    int bitcnt;
    size_t next;                            // the stream byte that is loaded next
    size_t in_len;
    uint64_t outpos, S;
    int mode, final, status, blocks;
    // what the last step left to write
    int count;                              // tokens
    uint64_t batch_out;                     // where token 0 goes
    size_t stored_src;                      // a stored block's bytes in the stream ...
    uint32_t stored_len;                    // ... and how many (0: none); they go to batch_out, in front of nothing else
    uint32_t adler;                         // the trailer, once mode is MODE_DONE
    uint16_t tlen[BATCH];                   // bytes of token k: 1 for a literal, 3..258
    uint16_t tval[BATCH];                   // 0x8000 | byte for a literal, distance - 1 for a match
    uint32_t tstart[BATCH];                 // its first byte, from batch_out
};

// ---- bits ---------------------------------------------------------------------------------------------------------------------------------
// `in` holds the stream's bytes [base, limit): byte i of the stream is in[i - base].  The device stages STAGE bytes in LDS per step.
struct Bits {
    uint64_t buf;
    int cnt;
    size_t next;
    const uint8_t* in;
    size_t base, limit;
};
PNGD_HD inline void refill(Bits& b) {
    while (b.cnt <= 56 && b.next < b.limit) {
        b.buf |= (uint64_t)b.in[b.next - b.base] << b.cnt;
        b.cnt += 8, ++b.next;
    }
}
// n <= 32 bits, or -1: the stream ends before them
PNGD_HD inline int64_t take(Bits& b, int n) {
    refill(b);
    if (b.cnt < n) return -1;
    const uint32_t v = (uint32_t)(b.buf & ((1ull << n) - 1));
    b.buf >>= n, b.cnt -= n;
    return v;
}

// ---- code tables --------------------------------------------------------------------------------------------------------------------------
PNGD_HD inline uint32_t reverse_bits(uint32_t v, int n) {
    uint32_t r = 0;
    for (int i = 0; i < n; ++i) r = r << 1 | (v >> i & 1);
    return r;
}

// lens[0..n) -> h.  one_code_ok: an incomplete set that is a single code of one bit is taken, as zlib takes it for both alphabets of a
// block (not for the code-length alphabet); a set without any code is taken too - using it is ADAIN_PNGD_UNUSED_CODE
PNGD_HD inline int build(Huff& h, const uint8_t* lens, int n, bool one_code_ok) {
    for (int i = 0; i < 16; ++i) h.count[i] = 0;
    for (int i = 0; i < n; ++i) ++h.count[lens[i] & 15];
    for (int i = 0; i < (1 << FAST_BITS); ++i) h.fast[i] = 0;
    if (h.count[0] == n) return 0;
    int left = 1, longest = 0;
    for (int len = 1; len < 16; ++len) {
        left = (left << 1) - h.count[len];
        if (left < 0) return ADAIN_PNGD_OVERSUBSCRIBED;
        if (h.count[len]) longest = len;
    }
    if (left > 0 && !(one_code_ok && longest == 1)) return ADAIN_PNGD_INCOMPLETE;
    uint16_t offs[16], next[16];
    offs[1] = 0, next[1] = 0;
    for (int len = 1; len < 15; ++len) {
        offs[len + 1] = (uint16_t)(offs[len] + h.count[len]);
        next[len + 1] = (uint16_t)((next[len] + h.count[len]) << 1);
    }
    for (int i = 0; i < n; ++i) {
        const int len = lens[i] & 15;
        if (!len) continue;
        h.symbol[offs[len]++] = (uint16_t)i;
        if (len > FAST_BITS) continue;
        const uint32_t code = next[len]++;
        for (uint32_t k = reverse_bits(code, len); k < (1u << FAST_BITS); k += 1u << len) h.fast[k] = (uint16_t)(len << 9 | i);
    }
    return 0;
}

// the next symbol, or -1 with *status: the stream ends inside the code, or the bits are no code of an incomplete set
PNGD_HD inline int decode(Bits& b, const Huff& h, int* status) {
    refill(b);
    const uint32_t e = h.fast[b.buf & ((1u << FAST_BITS) - 1)];
    if (e) {
        const int len = (int)(e >> 9);
        if (len > b.cnt) { *status = ADAIN_PNGD_TRUNCATED; return -1; }
        b.buf >>= len, b.cnt -= len;
        return (int)(e & 511);
    }
    int code = 0, first = 0, index = 0;
    uint64_t bits = b.buf;
    for (int len = 1; len < 16; ++len) {
        code |= (int)(bits & 1);
        bits >>= 1;
        const int count = h.count[len];
        if (code - count < first) {
            if (len > b.cnt) { *status = ADAIN_PNGD_TRUNCATED; return -1; }
            b.buf >>= len, b.cnt -= len;
            return h.symbol[index + (code - first)];
        }
        index += count, first += count;
        first <<= 1, code <<= 1;
    }
    *status = b.cnt < 15 ? ADAIN_PNGD_TRUNCATED : ADAIN_PNGD_UNUSED_CODE;
    return -1;
}

PNGD_HD inline void fixed_tables(Tables& t) {
    for (int i = 0; i < 288; ++i) t.lens[i] = (uint8_t)(i < 144 ? 8 : i < 256 ? 9 : i < 280 ? 7 : 8);
    build(t.ll, t.lens, 288, false);
    for (int i = 0; i < 32; ++i) t.lens[i] = 5;
    build(t.d, t.lens, 32, false);
}

// HLIT, HDIST, HCLEN, the code-length code and both alphabets, checked in zlib's order
PNGD_HD inline int dynamic_tables(Bits& b, Tables& t) {
    const int64_t head = take(b, 14);
    if (head < 0) return ADAIN_PNGD_TRUNCATED;
    const int nlen = (int)(head & 31) + 257, ndist = (int)(head >> 5 & 31) + 1, ncode = (int)(head >> 10 & 15) + 4;
    if (nlen > 286 || ndist > 30) return ADAIN_PNGD_TOO_MANY_SYMBOLS;
    const uint8_t order[19] = {16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15};
    uint8_t cl[19];
    for (int i = 0; i < 19; ++i) cl[i] = 0;
    for (int i = 0; i < ncode; ++i) {
        const int64_t v = take(b, 3);
        if (v < 0) return ADAIN_PNGD_TRUNCATED;
        cl[order[i]] = (uint8_t)v;
    }
    if (int bad = build(t.ll, cl, 19, false)) return bad;          // t.ll serves as the code-length code until the lengths are read
    int have = 0;
    while (have < nlen + ndist) {
        int status = 0;
        const int sym = decode(b, t.ll, &status);
        if (sym < 0) return status;
        if (sym < 16) { t.lens[have++] = (uint8_t)sym; continue; }
        int prev = 0, copy;
        int64_t extra;
        if (sym == 16) {
            if (have == 0) return ADAIN_PNGD_REPEAT;
            prev = t.lens[have - 1];
            extra = take(b, 2), copy = 3 + (int)extra;
        } else if (sym == 17) extra = take(b, 3), copy = 3 + (int)extra;
        else extra = take(b, 7), copy = 11 + (int)extra;
        if (extra < 0) return ADAIN_PNGD_TRUNCATED;
        if (have + copy > nlen + ndist) return ADAIN_PNGD_REPEAT;
        while (copy--) t.lens[have++] = (uint8_t)prev;
    }
    if (t.lens[256] == 0) return ADAIN_PNGD_NO_END_OF_BLOCK;
    if (int bad = build(t.ll, t.lens, nlen, true)) return bad;
    return build(t.d, t.lens + nlen, ndist, true);
}

// ---- one step -----------------------------------------------------------------------------------------------------------------------------
PNGD_HD inline void start(State& st, size_t in_len, uint64_t S) {
    st.bitbuf = 0, st.bitcnt = 0, st.next = in_len < 2 ? in_len : 2;        // behind the zlib header, which the host has checked
    st.in_len = in_len, st.outpos = 0, st.S = S;
    st.mode = MODE_HEADER, st.final = 0, st.blocks = 0, st.count = 0, st.batch_out = 0, st.stored_src = 0, st.stored_len = 0, st.adler = 0;
    st.status = in_len < 2 ? ADAIN_PNGD_TRUNCATED : 0;
}

PNGD_HD inline int step_header(State& st, Tables& t, Bits& b) {
    const int64_t head = take(b, 3);
    if (head < 0) return ADAIN_PNGD_TRUNCATED;
    st.final = (int)(head & 1);
    ++st.blocks;
    const int type = (int)(head >> 1);
    if (type == 3) return ADAIN_PNGD_BLOCK_TYPE;
    if (type == 0) {
        b.buf >>= b.cnt & 7, b.cnt -= b.cnt & 7;
        const int64_t v = take(b, 32);
        if (v < 0) return ADAIN_PNGD_TRUNCATED;
        const uint32_t len = (uint32_t)v & 0xffff, nlen = (uint32_t)v >> 16;
        if (len != (nlen ^ 0xffff)) return ADAIN_PNGD_STORED_LEN;
        const size_t src = b.next - (size_t)(b.cnt >> 3);          // bytes loaded and not consumed go back to the stream
        if (len > st.in_len - src) return ADAIN_PNGD_TRUNCATED;
        if (len > st.S - st.outpos) return ADAIN_PNGD_TOO_MUCH;
        st.stored_src = src, st.stored_len = len;
        st.outpos += len;
        b.buf = 0, b.cnt = 0, b.next = src + len;
        st.mode = st.final ? MODE_TRAILER : MODE_HEADER;
        return 0;
    }
    if (type == 1) fixed_tables(t);
    else if (int bad = dynamic_tables(b, t)) return bad;
    st.mode = MODE_CODES;
    return 0;
}

PNGD_HD inline int step_codes(State& st, const Tables& t, Bits& b) {
    while (st.count < BATCH) {
        int status = 0;
        int sym = decode(b, t.ll, &status);
        if (sym < 0) return status;
        uint32_t len = 1, val;
        if (sym < 256) val = 0x8000u | (uint32_t)sym;
        else if (sym == 256) {
            st.mode = st.final ? MODE_TRAILER : MODE_HEADER;
            return 0;
        } else {
            sym -= 257;
            if (sym >= 29) return ADAIN_PNGD_BAD_SYMBOL;
            int e = 0;
            if (sym < 8) len = 3 + sym;
            else if (sym == 28) len = 258;
            else e = (sym >> 2) - 1, len = 3 + ((4 + (sym & 3)) << e);
            int64_t extra = take(b, e);
            if (extra < 0) return ADAIN_PNGD_TRUNCATED;
            len += (uint32_t)extra;
            const int dsym = decode(b, t.d, &status);
            if (dsym < 0) return status;
            if (dsym >= 30) return ADAIN_PNGD_BAD_SYMBOL;
            uint32_t dist;
            e = 0;
            if (dsym < 4) dist = 1 + dsym;
            else e = (dsym >> 1) - 1, dist = 1 + ((2 + (dsym & 1)) << e);
            extra = take(b, e);
            if (extra < 0) return ADAIN_PNGD_TRUNCATED;
            dist += (uint32_t)extra;
            if (dist > st.outpos) return ADAIN_PNGD_FAR_DISTANCE;
            val = dist - 1;
        }
        if (len > st.S - st.outpos) return ADAIN_PNGD_TOO_MUCH;
        st.tlen[st.count] = (uint16_t)len, st.tval[st.count] = (uint16_t)val, st.tstart[st.count] = (uint32_t)(st.outpos - st.batch_out);
        ++st.count;
        st.outpos += len;
    }
    return 0;
}

PNGD_HD inline int step_trailer(State& st, Bits& b) {
    b.buf >>= b.cnt & 7, b.cnt -= b.cnt & 7;
    const size_t at = b.next - (size_t)(b.cnt >> 3), left = st.in_len - at;
    if (left < 4) return ADAIN_PNGD_TRUNCATED;
    if (st.outpos < st.S) return ADAIN_PNGD_TOO_LITTLE;
    if (left > 4) return ADAIN_PNGD_TRAILING;
    const int64_t v = take(b, 32);
    if (v < 0) return ADAIN_PNGD_TRUNCATED;
    const uint32_t u = (uint32_t)v;
    st.adler = u << 24 | (u & 0xff00) << 8 | (u >> 8 & 0xff00) | u >> 24;
    st.mode = MODE_DONE;
    return 0;
}

// One step of ONE thread.  stage: the stream's bytes [st.next, min(in_len, st.next + STAGE)) - or, with staged = false, the whole stream.
PNGD_HD inline void step(State& st, Tables& t, const uint8_t* stage, bool staged) {
    Bits b;
    b.buf = st.bitbuf, b.cnt = st.bitcnt, b.next = st.next, b.in = stage;
    b.base = staged ? st.next : 0;
    b.limit = staged && st.in_len - st.next > (size_t)STAGE ? st.next + STAGE : st.in_len;
    st.count = 0, st.stored_len = 0, st.batch_out = st.outpos;
    int status = 0;
    if (st.mode == MODE_HEADER) status = step_header(st, t, b);
    else if (st.mode == MODE_CODES) status = step_codes(st, t, b);
    else if (st.mode == MODE_TRAILER) status = step_trailer(st, b);
    st.bitbuf = b.buf, st.bitcnt = b.cnt, st.next = b.next;
    if (status) st.status = status;
}

// ---- the writes of a step, per lane -------------------------------------------------------------------------------------------------------
// A lane's share of the Adler-32: a = sum of its bytes, b = sum of (S - position) * byte; both stay below 2^64 (settle() between steps)
struct AdlerPart {
    uint64_t a, b;
};
PNGD_HD inline void put(uint8_t* ring, uint8_t* out, uint64_t S, uint64_t pos, uint32_t v, AdlerPart& acc) {
    ring[pos & RING_MASK] = (uint8_t)v;
    out[pos] = (uint8_t)v;
    acc.a += v, acc.b += (S - pos) * v;
}
PNGD_HD inline void settle(AdlerPart& acc) {
    if (acc.b >> 62) acc.b %= ADLER_MOD;
}
// in: the WHOLE stream
PNGD_HD inline void write_stored(const State& st, int lane, int lanes, const uint8_t* in, uint8_t* ring, uint8_t* out, AdlerPart& acc) {
    for (uint32_t i = (uint32_t)lane; i < st.stored_len; i += (uint32_t)lanes) put(ring, out, st.S, st.batch_out + i, in[st.stored_src + i], acc);
}
PNGD_HD inline void write_literals(const State& st, int lane, int lanes, uint8_t* ring, uint8_t* out, AdlerPart& acc) {
    for (int k = lane; k < st.count; k += lanes)
        if (st.tval[k] & 0x8000) put(ring, out, st.S, st.batch_out + st.tstart[k], st.tval[k] & 255u, acc);
}
PNGD_HD inline bool is_match(const State& st, int k) { return !(st.tval[k] & 0x8000); }
// match k; every byte it reads lies in front of its first, written by an earlier token
PNGD_HD inline void write_match(const State& st, int k, int lane, int lanes, uint8_t* ring, uint8_t* out, AdlerPart& acc) {
    const uint32_t len = st.tlen[k], d = (uint32_t)st.tval[k] + 1;
    const uint64_t p = st.batch_out + st.tstart[k];
    for (uint32_t i = (uint32_t)lane; i < len; i += (uint32_t)lanes) {
        const uint32_t off = d >= len ? i : i % d;
        put(ring, out, st.S, p + i, ring[(p - d + off) & RING_MASK], acc);
    }
}
PNGD_HD inline uint32_t adler_of(uint64_t a, uint64_t b, uint64_t S) {
    return (uint32_t)((S % ADLER_MOD + b % ADLER_MOD) % ADLER_MOD) << 16 | (uint32_t)((1 + a % ADLER_MOD) % ADLER_MOD);
}
PNGD_HD inline uint64_t max_steps(size_t in_len) { return 8 * (uint64_t)in_len + 2; }

// ---- unfilter -----------------------------------------------------------------------------------------------------------------------------
// pixels ride in a uint32, channel k in byte k
PNGD_HD inline uint32_t load_px(const uint8_t* p, int bpp) {
    uint32_t v = 0;
    for (int k = 0; k < bpp; ++k) v |= (uint32_t)p[k] << (8 * k);
    return v;
}
PNGD_HD inline int paeth(int a, int b, int c) {
    const int p = a + b - c;
    const int pa = p > a ? p - a : a - p, pb = p > b ? p - b : b - p, pc = p > c ? p - c : c - p;
    return pa <= pb && pa <= pc ? a : pb <= pc ? b : c;
}
PNGD_HD inline uint32_t unfilter_px(int ft, uint32_t raw, uint32_t left, uint32_t up, uint32_t ul, int bpp) {
    uint32_t v = 0;
    for (int k = 0; k < bpp; ++k) {
        const int x = raw >> (8 * k) & 255, a = left >> (8 * k) & 255, b = up >> (8 * k) & 255, c = ul >> (8 * k) & 255;
        const int pred = ft == 0 ? 0 : ft == 1 ? a : ft == 2 ? b : ft == 3 ? (a + b) >> 1 : paeth(a, b, c);
        v |= (uint32_t)((x + pred) & 255) << (8 * k);
    }
    return v;
}
// c_out is c, or 3: grey replicated, alpha dropped
PNGD_HD inline void store_px(uint8_t* p, uint32_t v, int c, int c_out) {
    if (c_out == c)
        for (int k = 0; k < c; ++k) p[k] = (uint8_t)(v >> (8 * k));
    else
        for (int k = 0; k < 3; ++k) p[k] = (uint8_t)(c == 1 ? v : v >> (8 * k));
}

// what lane - 1 holds, to every lane; lane 0 gets 0.  L = 1: a thread per lane (device only); L = 64: all lanes in one thread
template <int L>
PNGD_HD inline void from_lane_above(uint32_t (&dst)[L], const uint32_t (&src)[L], int lane0) {
    if (L == 1) {
#if defined(__HIP_DEVICE_COMPILE__)
        const uint32_t v = (uint32_t)__shfl_up((int)src[0], 1);
        dst[0] = lane0 ? v : 0;
#else
        dst[0] = 0;
#endif
    } else {
        for (int l = L - 1; l > 0; --l) dst[l] = src[l - 1];
        dst[0] = 0;
    }
}

// The rows [r0, r0 + BAND) of one file.  filt: its filtered stream h x (w c + 1); the band's last row is written back unfiltered in its
// place, which is where the next band's first row reads `up`.  lane0: the first lane this thread carries (0 when L = 64).  Returns
// whether one of the thread's rows has a filter byte above 4 (such a row is read as filter 0).
template <int L>
PNGD_HD inline bool unfilter_band(uint8_t* filt, int h, int w, int c, int c_out, int r0, uint8_t* out, int lane0) {
    const size_t stride = (size_t)w * c + 1;
    int ft[L];
    bool active[L], bad = false;
    uint32_t left[L], last[L], last2[L], up[L], ul[L], above_prev[L];
    for (int l = 0; l < L; ++l) {
        const int row = r0 + lane0 + l;
        active[l] = row < h;
        ft[l] = active[l] ? filt[row * stride] : 0;
        if (ft[l] > 4) bad = true, ft[l] = 0;
        left[l] = last[l] = last2[l] = above_prev[l] = 0;
    }
    for (int t = 0; t < w + BAND - 1; ++t) {
        from_lane_above<L>(up, last, lane0);
        from_lane_above<L>(ul, last2, lane0);
        for (int l = 0; l < L; ++l) {
            const int lane = lane0 + l, row = r0 + lane, x = t - lane;
            if (!active[l] || x < 0 || x >= w) continue;
            uint8_t* mine = filt + row * stride + 1 + (size_t)x * c;
            uint32_t b = up[l], cc = x > 0 ? ul[l] : 0;
            if (lane == 0) {                    // the band's first row: the row above lies in memory, unfiltered
                b = row > 0 ? load_px(mine - stride, c) : 0;
                cc = above_prev[l], above_prev[l] = b;
            }
            const uint32_t v = unfilter_px(ft[l], load_px(mine, c), left[l], b, cc, c);
            store_px(out + ((size_t)row * w + x) * c_out, v, c, c_out);
            if (lane == BAND - 1)
                for (int k = 0; k < c; ++k) mine[k] = (uint8_t)(v >> (8 * k));
            last2[l] = last[l], last[l] = v, left[l] = v;
        }
    }
    return bad;
}

}  // namespace pngd
}  // namespace adain
