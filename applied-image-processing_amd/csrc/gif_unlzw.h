// The LZW core and the per-pixel walk of the GIF decoder (gif_decode.hip), written so that the same source compiles for the host: the
// device kernels and tools/gif_decode_check.cpp (a stand-alone program for a sanitised CPU build) both run exactly this code.  The rules
// are at the top of gif_decode.hip and restated in tests/gif_decode_ref.py.
//
// A string of the table is a piece of the output that is already written: the entry made when a code is read is the previous code's
// string and one more byte, and that byte is the next one written, so the entry is (where the previous code's output starts, its length
// + 1).  Decoding a code is a copy inside the plane; the code that names the entry being made (KwKwK) is a copy that overlaps its own
// output, read modulo its distance.
//
// Bounds.  Every position of a plane is below `total` = w h of the rectangle, which the row check holds to the plane's size: a token is
// cut at `total`, and a string starts below the position it was made at.  The stage holds STAGE bytes from the byte of the next bit; a
// batch reads at most BATCH codes of at most 12 bits, 96 bytes, and three bytes at the last one.  The table has 4096 entries and a code
// has at most 12 bits.  A batch reads at least one code or ends the stream, so max_batches() bounds the loop.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include "../../include/adain_gif_decode.h"

#if defined(__HIPCC__)
#define GIFD_FN __host__ __device__ inline
#else
#define GIFD_FN inline
#endif

namespace adain {
namespace gifd {

constexpr int BATCH = 64;            // codes a batch reads at most
constexpr int STAGE = 128;           // bytes of the stream in front of the parse
constexpr int TABLE = 4096;
constexpr uint32_t LITERAL = 0x80000000u;        // a token's src: a root's byte instead of a position (positions are below 2^31)
constexpr int SHORT_COPY = 16;       // a copy of at most this many bytes from before the batch is one lane's

struct Row {
    uint64_t data_at, data_len, table_at;
    uint32_t left, top, w, h, entries, background;
    int code_size, interlace, disposal, transparent;         // transparent: -1 for none
};

GIFD_FN Row read_row(const uint64_t* r) {
    Row o;
    o.data_at = r[0], o.data_len = r[1], o.table_at = r[4];
    o.left = (uint32_t)(r[2] & 0xffff), o.top = (uint32_t)(r[2] >> 16 & 0xffff), o.w = (uint32_t)(r[2] >> 32 & 0xffff), o.h = (uint32_t)(r[2] >> 48);
    o.code_size = (int)(r[3] & 0xff), o.interlace = (int)(r[3] >> 8 & 1), o.disposal = (int)(r[3] >> 16 & 0xff), o.transparent = (int)(r[3] >> 32 & 0xffff) - 1;
    o.entries = r[5] > 0xffffffffu ? 0xffffffffu : (uint32_t)r[5], o.background = (uint32_t)(r[6] & 0xff);
    return o;
}

// What the kernels rely on, checked where the row is read
GIFD_FN bool row_ok(const Row& r, const uint64_t* words, uint32_t H, uint32_t W, size_t slot, size_t blob_bytes) {
    if (r.w < 1 || r.h < 1 || r.left + r.w > W || r.top + r.h > H || (uint64_t)r.w * r.h > slot) return false;
    if (r.code_size < 2 || r.code_size > 8 || r.disposal > 3 || r.transparent > 255 || (words[3] >> 48) || (words[3] >> 9 & 0x7f) || (words[3] >> 24 & 0xff)) return false;
    if (r.entries < 2 || r.entries > 256 || words[6] > 255 || words[7]) return false;
    if (r.data_at > blob_bytes || r.data_len > blob_bytes - r.data_at || r.data_len >= ((uint64_t)1 << 40)) return false;
    if (r.table_at > blob_bytes || (uint64_t)3 * r.entries > blob_bytes - r.table_at) return false;
    return true;
}

struct State {
    uint64_t bitpos, bits_total;
    uint32_t produced, total, batch_start;
    uint32_t prev_start, prev_len;          // where the previous code's output starts, and its length
    int32_t status, done, codes;
    int m, width, next, fresh;              // fresh: the next code is the first behind a CLEAR (or of the stream)
    int count, nbig, ndep;                  // this batch's tokens, and how many of them are in big[] and dep[]
};
struct Table {
    uint32_t start[TABLE];
    uint16_t len[TABLE];
};
struct Tokens {
    uint32_t dst[BATCH], src[BATCH], len[BATCH];
    uint8_t kind[BATCH], big[BATCH], dep[BATCH];
};
enum { KIND_LITERAL = 0, KIND_SHORT = 1, KIND_BIG = 2, KIND_DEPENDENT = 3 };

GIFD_FN void start(State& st, uint64_t data_len, uint32_t total, int code_size) {
    st.bitpos = 0, st.bits_total = data_len * 8;
    st.produced = 0, st.total = total, st.batch_start = 0, st.prev_start = 0, st.prev_len = 0;
    st.status = 0, st.done = 0, st.codes = 0;
    st.m = code_size, st.width = code_size + 1, st.next = (1 << code_size) + 2, st.fresh = 1;
    st.count = st.nbig = st.ndep = 0;
}

GIFD_FN uint64_t max_batches(uint64_t data_len) { return data_len * 8 / 3 / BATCH + 2; }

// One lane: up to BATCH codes from the stage (the bytes from st.bitpos / 8 on, zeros behind the data) into tokens
GIFD_FN void parse(State& st, Table& tb, Tokens& tk, const uint8_t* stage) {
    const uint64_t base = st.bitpos >> 3;
    const int clear = 1 << st.m, end = clear + 1;
    int count = 0, nbig = 0, ndep = 0;
    st.batch_start = st.produced;
    for (int i = 0; i < BATCH; ++i) {
        if (st.bitpos + (uint64_t)st.width > st.bits_total) { st.status = ADAIN_GIFD_TRUNCATED; break; }
        const uint32_t at = (uint32_t)((st.bitpos >> 3) - base);          // <= 96, so at + 2 < STAGE
        const uint32_t word = (uint32_t)stage[at] | (uint32_t)stage[at + 1] << 8 | (uint32_t)stage[at + 2] << 16;
        const int c = (int)(word >> (st.bitpos & 7) & ((1u << st.width) - 1));
        st.bitpos += st.width;
        st.codes++;
        if (c == clear) {
            st.width = st.m + 1, st.next = clear + 2, st.fresh = 1;
            continue;
        }
        if (c == end) { st.status = ADAIN_GIFD_EOI; break; }
        uint32_t src, len;
        if (st.fresh) {
            if (c > clear) { st.status = ADAIN_GIFD_BAD_FIRST; break; }
            src = LITERAL | (uint32_t)c, len = 1;
            st.fresh = 0;
        } else {
            if (c > st.next) { st.status = ADAIN_GIFD_BAD_CODE; break; }
            if (c < clear) src = LITERAL | (uint32_t)c, len = 1;
            else if (c == st.next) src = st.prev_start, len = st.prev_len + 1;          // KwKwK; next < TABLE here, c has 12 bits
            else src = tb.start[c], len = tb.len[c];
            if (st.next < TABLE) {
                tb.start[st.next] = st.prev_start, tb.len[st.next] = (uint16_t)(st.prev_len + 1);
                if (st.next == (1 << st.width) - 1 && st.width < 12) st.width++;
                st.next++;
            }
        }
        st.prev_start = st.produced, st.prev_len = len;
        const uint32_t room = st.total - st.produced, n = len < room ? len : room;
        tk.dst[count] = st.produced, tk.src[count] = src, tk.len[count] = n;
        int kind;
        if (src & LITERAL) kind = KIND_LITERAL;
        else if (src + n > st.batch_start) kind = KIND_DEPENDENT, tk.dep[ndep++] = (uint8_t)count;
        else if (n > (uint32_t)SHORT_COPY) kind = KIND_BIG, tk.big[nbig++] = (uint8_t)count;
        else kind = KIND_SHORT;
        tk.kind[count++] = (uint8_t)kind;
        st.produced += n;
        if (st.produced == st.total) { st.done = 1; break; }
    }
    st.count = count, st.nbig = nbig, st.ndep = ndep;
}

// Everything that reads nothing of this batch: the literals and the short copies a lane each, the long copies all lanes together.
// Call with every lane; the sources were written before the batch began
GIFD_FN void write_independent(const State& st, const Tokens& tk, int lane, int lanes, uint8_t* out) {
    for (int k = lane; k < st.count; k += lanes) {
        const size_t dst = tk.dst[k];
        if (tk.kind[k] == KIND_LITERAL) out[dst] = (uint8_t)tk.src[k];
        else if (tk.kind[k] == KIND_SHORT)
            for (uint32_t i = 0; i < tk.len[k]; ++i) out[dst + i] = out[(size_t)tk.src[k] + i];
    }
    for (int j = 0; j < st.nbig; ++j) {
        const int k = tk.big[j];
        const size_t dst = tk.dst[k], src = tk.src[k];
        for (uint32_t i = lane; i < tk.len[k]; i += lanes) out[dst + i] = out[src + i];
    }
}

// Dependent token j of the batch (it reads what the batch wrote, its own output too): every lane, after everything before it is visible
GIFD_FN void write_dependent(const Tokens& tk, int j, int lane, int lanes, uint8_t* out) {
    const int k = tk.dep[j];
    const size_t dst = tk.dst[k], src = tk.src[k];
    const uint32_t dist = (uint32_t)(dst - src);                 // >= 1: a string starts below the position it is copied to
    for (uint32_t i = lane; i < tk.len[k]; i += lanes) out[dst + i] = out[src + i % dist];
}

// ---- the walk of one screen pixel through the clip -------------------------------------------------------------------------------
// The stored row of row y of an interlaced rectangle of h rows: the four passes one behind the other
GIFD_FN uint32_t stored_row(uint32_t y, uint32_t h, int interlace) {
    if (!interlace) return y;
    const uint32_t n1 = (h + 7) / 8, n2 = (h + 3) / 8, n3 = (h + 1) / 4;
    if (y % 8 == 0) return y / 8;
    if (y % 8 == 4) return n1 + y / 8;
    if (y % 4 == 2) return n1 + n2 + y / 4;
    return n1 + n2 + n3 + y / 2;
}

struct Rgb {
    uint8_t r, g, b;
};

// Entry `index` of a table as Pillow holds it: padded to 256 entries with zeros
GIFD_FN Rgb table_colour(const uint8_t* blob, const Row& r, uint32_t index) {
    if (index >= r.entries) return Rgb{0, 0, 0};
    const uint8_t* p = blob + r.table_at + (size_t)3 * index;
    return Rgb{p[0], p[1], p[2]};
}

struct Walk {
    Rgb canvas{0, 0, 0}, fill{0, 0, 0};
    bool pending = false;               // the frame before left a disposal for this pixel's rectangle
    bool was_inside = false;            // this pixel lies in the rectangle of the frame before
    int disposal = 0;                   // the method in force: a frame with 0 inherits it
};

// Frame k at screen pixel (y, x): moves the walk on and returns the pixel of frame k.  plane: the frame's indices in stored row order
GIFD_FN Rgb walk_frame(Walk& s, int k, const Row& r, const uint8_t* blob, const uint8_t* plane, uint32_t y, uint32_t x) {
    if (s.pending && s.was_inside) s.canvas = s.fill;                      // rule 3: the disposal of the frame before, first
    s.pending = false;
    const bool inside = x >= r.left && x < r.left + r.w && y >= r.top && y < r.top + r.h;
    if (r.disposal) s.disposal = r.disposal;
    const bool keyed = r.transparent >= 0;
    if (s.disposal == 2) {                                                  // rule 4
        uint32_t index = keyed ? (uint32_t)r.transparent : r.background;
        if (k > 0 && index >= r.entries) index = 0;
        s.fill = table_colour(blob, r, index), s.pending = true;
    } else if (s.disposal == 3) {                                           // rule 5
        if (k > 0) s.fill = s.canvas, s.pending = true;
        else if (keyed) s.fill = table_colour(blob, r, (uint32_t)r.transparent), s.pending = true;
    }
    uint32_t index = 0;
    if (inside) index = plane[(size_t)stored_row(y - r.top, r.h, r.interlace) * r.w + (x - r.left)];
    if (k == 0) s.canvas = table_colour(blob, r, inside ? index : keyed ? (uint32_t)r.transparent : 0u);       // rule 1
    else if (inside && !(keyed && index == (uint32_t)r.transparent)) s.canvas = table_colour(blob, r, index);   // rule 2
    s.was_inside = inside;
    return s.canvas;
}

}  // namespace gifd
}  // namespace adain
