// PNG output files on the device (gfx950): lossless, read back by any PNG reader to the frame's pixels.  Replaces the host's
// Image.save of a .png path (test.py:243-244, video/utils.py:292-296, train.py:104-114).  The rules, byte for byte: tests/png_ref.py.
//
// The file: signature, IHDR, one IDAT, IEND; 8-bit, colour type 2 (c = 3) or 0 (c = 1), non-interlaced.
//   rows    : filter -1 tries all five filters on the raw previous row and keeps the one whose filtered bytes have the smallest sum of
//             magnitudes (b < 128 ? b : 256 - b), ties to the lowest number (libpng's heuristic); 0..4 forces one.  The filtered stream
//             is, per row, the filter's number and the w c filtered bytes: stride = w c + 1.
//   blocks  : PNG_BLOCK filtered bytes each.  A block is a dynamic-Huffman block or a fixed-Huffman one, whichever has fewer bits, ties
//             to fixed; no stored blocks.  BFINAL on the last, which is zero-padded to a byte.
//   matches : at every position the longest match among {1, 2, 3, 4, 6, stride - c, stride, stride + c} (those in 1..32768, never a
//             source before the stream's start; a source before the block's start is fine), ties to the smallest distance, at most 258
//             bytes and never past the block's end; then a greedy parse from the block's start taking matches of 4 bytes or more.
//   lengths : Huffman by the two-queue merge over the symbols sorted by (count, symbol), a leaf before an internal node of the same
//             weight; a tree deeper than the limit (15; 7 for the code-length alphabet) is rebuilt with every count halved, rounding up.
//             One used symbol gets one bit; a block without matches sends distance symbol 0 with one bit.
//   header  : the code lengths of both alphabets as one sequence, run-length coded greedily (18 while 11 or more zeros remain, then 17,
//             then singly; another length once, then 16 while 3 or more remain, then singly).
//   wrapper : zlib header 78 01, Adler-32 of the filtered stream, CRC-32 on every chunk.
// Integer arithmetic throughout: the bytes are a function of the frame and `filter` alone.
//
// Stages (7 launches and a memset, whatever n; nothing allocates or waits):
//   filter  : a workgroup per row - costs, the chosen filter's bytes, the row's share of the Adler sums (integer atomics)
//   match   : a workgroup per block - best candidate per position, the greedy walk, both histograms, the tables, the block's bit count
//   scan    : a workgroup per frame - where every block's bits start
//   zero    : the frame's bit stream, as far as it will be written
//   emit    : a workgroup per block - header, tokens, end of block (and the Adler-32 behind the last) by atomicOr, LSB first
//   scatter : the zlib stream behind the file's first 41 bytes, and the CRC-32 of 256-byte pieces shifted to the stream's end
//   finish  : a thread per frame - signature, IHDR, IDAT's length, type and CRC, IEND, lengths[i]
#include "device_utils.h"

namespace adain {
namespace {

constexpr int PNG_BLOCK = 32768;        // filtered bytes per deflate block
constexpr int THREADS = 256;
constexpr int PER_THREAD = PNG_BLOCK / THREADS;
constexpr int MIN_MATCH = 4, MAX_MATCH = 258, MAX_DIST = 32768;
constexpr int NLL = 286, NLLF = 288, ND = 30, NCL = 19;
constexpr int HDR_WORDS = 144;          // 17 + 3 * 19 + 316 * 14 = 4498 bits at most
constexpr int FILE_HEAD = 41;           // signature 8, IHDR 25, IDAT's length and type 8
constexpr int FILE_FRAME = 57;          // + IDAT's CRC 4, IEND 12
constexpr int PIECE = 256;              // bytes per CRC piece
constexpr uint32_t CRC_POLY = 0xedb88320u;
constexpr uint32_t ADLER = 65521;

__device__ const uint8_t CL_ORDER[NCL] = {16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15};      // RFC 1951 3.2.7

struct Dists { int count; int d[8]; };

struct BlockTab {
    uint16_t ll_code[NLLF];             // bit-reversed, ready for LSB-first packing
    uint16_t d_code[32];
    uint8_t ll_len[NLLF];
    uint8_t d_len[32];
    uint32_t hdr_bits;
    uint32_t hdr[HDR_WORDS];            // BFINAL, BTYPE and (dynamic) the code lengths
};

struct PngPlan {
    size_t stride, S, nblk, max_zlib, stream_words, out_stride;
    size_t o_filt, o_tok, o_tabs, o_bbits, o_boff, o_total, o_acc, o_stream, total;
    Dists dists;
};

// The one layout of a call.  out_stride: a literal costs at most 9 bits under the fixed code, a match (4..258 bytes: at most 8 + 5 + 5 + 13 =
// 31 bits) less than the 4 literals it replaces at least, a block adds 3 header bits and the 7 of its end-of-block; the cheaper of
// fixed and dynamic is at most the fixed one.
PngPlan make_png_plan(int n, int h, int w, int c) {
    PngPlan p{};
    p.stride = (size_t)w * c + 1;
    p.S = p.stride * h;
    p.nblk = (p.S + PNG_BLOCK - 1) / PNG_BLOCK;
    p.max_zlib = 2 + (9 * p.S + 10 * p.nblk + 7) / 8 + 4;
    p.stream_words = (p.max_zlib + 3) / 4 + 1;
    p.out_stride = FILE_FRAME + p.max_zlib;
    const long long cand[8] = {1, 2, 3, 4, 6, (long long)p.stride - c, (long long)p.stride, (long long)p.stride + c};
    for (int i = 0; i < 8; ++i) {           // ascending, without repeats, 1..32768
        long long best = -1;
        for (int j = 0; j < 8; ++j)
            if (cand[j] >= 1 && cand[j] <= MAX_DIST && (p.dists.count == 0 || cand[j] > p.dists.d[p.dists.count - 1]) && (best < 0 || cand[j] < best)) best = cand[j];
        if (best < 0) break;
        p.dists.d[p.dists.count++] = (int)best;
    }
    const size_t N = (size_t)n;
    Carve ws;
    p.o_filt = ws.take(N * p.S);
    p.o_tok = ws.take(N * p.S * sizeof(uint16_t));
    p.o_tabs = ws.take(N * p.nblk * sizeof(BlockTab));
    p.o_bbits = ws.take(N * p.nblk * sizeof(uint32_t));
    p.o_boff = ws.take(N * p.nblk * sizeof(uint64_t));
    p.o_total = ws.take(N * sizeof(uint64_t));
    p.o_acc = ws.take(N * 4 * sizeof(uint64_t));
    p.o_stream = ws.take(N * p.stream_words * sizeof(uint32_t));
    p.total = ws.at;
    return p;
}

// ---- workgroup helpers --------------------------------------------------------------------------------------------------------------------
// the sum of v over the workgroup's THREADS threads, to every thread; part: THREADS / 64 entries of LDS
template <class V>
__device__ __forceinline__ V wg_sum(V v, V* part) {
    for (int d = 32; d > 0; d >>= 1) v += __shfl_down(v, d);
    __syncthreads();
    if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = v;
    __syncthreads();
    V s = 0;
    for (int k = 0; k < THREADS / 64; ++k) s += part[k];
    return s;
}

__device__ __forceinline__ int length_symbol(int len, int* extra_bits, int* extra) {         // len 3..258 -> symbol - 257
    if (len == MAX_MATCH) { *extra_bits = 0, *extra = 0; return 28; }
    const int l = len - 3;
    if (l < 8) { *extra_bits = 0, *extra = 0; return l; }
    const int e = 29 - __clz(l);
    *extra_bits = e, *extra = l & ((1 << e) - 1);
    return 4 * e + 4 + ((l >> e) & 3);
}
__device__ __forceinline__ int dist_symbol(int dist, int* extra_bits, int* extra) {          // dist 1..32768
    const int d = dist - 1;
    if (d < 4) { *extra_bits = 0, *extra = 0; return d; }
    const int e = 30 - __clz(d);
    *extra_bits = e, *extra = d & ((1 << e) - 1);
    return 2 * e + 2 + ((d >> e) & 1);
}

// ---- filter -------------------------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ int paeth(int a, int b, int c) {
    const int p = a + b - c, pa = abs(p - a), pb = abs(p - b), pc = abs(p - c);
    return pa <= pb && pa <= pc ? a : pb <= pc ? b : c;
}
__device__ __forceinline__ int filtered(int k, int raw, int a, int b, int c) {
    const int pred = k == 0 ? 0 : k == 1 ? a : k == 2 ? b : k == 3 ? (a + b) >> 1 : paeth(a, b, c);
    return (raw - pred) & 255;
}
__device__ __forceinline__ uint32_t magnitude(int v) { return (uint32_t)(v < 128 ? v : 256 - v); }

// grid (h, n).  acc: per frame {sum of the bytes, sum of (bytes behind and including j) * byte j} both as sums of residues mod 65521
__global__ __launch_bounds__(THREADS) void png_filter_kernel(const uint8_t* __restrict__ src, int h, int w, int c, int filter, uint8_t* __restrict__ filt, size_t S,
                                                             unsigned long long* __restrict__ acc) {
    __shared__ unsigned long long part[THREADS / 64];
    const int y = blockIdx.x, t = threadIdx.x, rb = w * c;
    const size_t f = blockIdx.y;
    const uint8_t* row = src + (f * h + y) * (size_t)rb;
    const uint8_t* up = y ? row - rb : nullptr;
    uint8_t* out = filt + f * S + (size_t)y * (rb + 1);
    int which = filter;
    if (filter < 0) {
        unsigned long long cost[5] = {0, 0, 0, 0, 0};
        for (int x = t; x < rb; x += THREADS) {
            const int raw = row[x], a = x >= c ? row[x - c] : 0, b = up ? up[x] : 0, cc = up && x >= c ? up[x - c] : 0;
            for (int k = 0; k < 5; ++k) cost[k] += magnitude(filtered(k, raw, a, b, cc));
        }
        which = 0;
        unsigned long long best = 0;
        for (int k = 0; k < 5; ++k) {
            const unsigned long long s = wg_sum(cost[k], part);
            if (k == 0 || s < best) best = s, which = k;
        }
    }
    const unsigned long long R = (unsigned long long)rb + 1;
    unsigned long long sa = 0, sb = 0;
    if (t == 0) out[0] = (uint8_t)which, sa = which, sb = R * which;
    for (int x = t; x < rb; x += THREADS) {
        const int raw = row[x], a = x >= c ? row[x - c] : 0, b = up ? up[x] : 0, cc = up && x >= c ? up[x - c] : 0;
        const int v = filtered(which, raw, a, b, cc);
        out[1 + x] = (uint8_t)v;
        sa += v, sb += (R - 1 - x) * v;
    }
    sa = wg_sum(sa, part);
    sb = wg_sum(sb, part);
    if (t == 0) {
        const unsigned long long am = sa % ADLER;
        const unsigned long long behind = ((unsigned long long)(h - 1 - y) * am) % ADLER;       // rows behind this one see its bytes R times each
        atomicAdd(acc + f * 4, am);
        atomicAdd(acc + f * 4 + 1, (sb + (R % ADLER) * behind) % ADLER);
    }
}

// ---- code lengths -------------------------------------------------------------------------------------------------------------------------
struct TableScratch {
    uint32_t f[NLLF], wt[NLLF], iw[NLLF];
    uint16_t leaf[NLLF], pl[NLLF], pi[NLLF], depth[NLLF];
    int again;
};

// lens[0..n) of freq[0..n) under `limit`, by the whole workgroup; the serial parts run on thread 0
__device__ void build_lengths(const uint32_t* freq, int n, int limit, uint8_t* lens, TableScratch& s) {
    const int t = threadIdx.x;
    __syncthreads();
    for (int i = t; i < n; i += THREADS) s.f[i] = freq[i], lens[i] = 0;
    __syncthreads();
    int m = 0;
    if (t == 0) {
        int last = -1;
        for (int i = 0; i < n; ++i)
            if (s.f[i]) ++m, last = i;
        if (m == 1) lens[last] = 1;
        s.again = m >= 2;
    }
    __syncthreads();
    while (s.again) {
        for (int i = t; i < n; i += THREADS) {
            const uint32_t fi = s.f[i];
            if (!fi) continue;
            int r = 0;
            for (int j = 0; j < n; ++j) {
                const uint32_t fj = s.f[j];
                r += fj && (fj < fi || (fj == fi && j < i));
            }
            s.leaf[r] = (uint16_t)i, s.wt[r] = fi;
        }
        __syncthreads();
        if (t == 0) {
            int li = 0, ii = 0;
            for (int k = 0; k < m - 1; ++k) {
                uint32_t total = 0;
                for (int pick = 0; pick < 2; ++pick) {
                    if (li < m && (ii >= k || s.wt[li] <= s.iw[ii])) total += s.wt[li], s.pl[li++] = (uint16_t)k;
                    else total += s.iw[ii], s.pi[ii++] = (uint16_t)k;
                }
                s.iw[k] = total;
            }
            s.depth[m - 2] = 0;
            for (int k = m - 3; k >= 0; --k) s.depth[k] = s.depth[s.pi[k]] + 1;
            int deepest = 0;
            for (int j = 0; j < m; ++j) {
                const int d = s.depth[s.pl[j]] + 1;
                lens[s.leaf[j]] = (uint8_t)min(d, 255);
                deepest = max(deepest, d);
            }
            if (deepest <= limit) s.again = 0;
            else
                for (int i = 0; i < n; ++i)
                    if (s.f[i]) s.f[i] = (s.f[i] + 1) >> 1;
        }
        __syncthreads();
    }
}

// RFC 1951 3.2.2 on lens[0..n), the codes bit-reversed.  One thread.
__device__ void canonical_codes(const uint8_t* lens, int n, uint16_t* codes) {
    int count[16] = {};
    for (int i = 0; i < n; ++i) ++count[lens[i]];
    count[0] = 0;
    uint32_t next[16] = {}, code = 0;
    for (int b = 1; b < 16; ++b) code = (code + count[b - 1]) << 1, next[b] = code;
    for (int i = 0; i < n; ++i) {
        const int k = lens[i];
        codes[i] = k ? (uint16_t)(__brev(next[k]++) >> (32 - k)) : 0;
    }
}

__device__ __forceinline__ int fixed_ll_len(int i) { return i < 144 ? 8 : i < 256 ? 9 : i < 280 ? 7 : 8; }

// ---- match --------------------------------------------------------------------------------------------------------------------------------
struct MatchShared {
    uint8_t v[PNG_BLOCK];               // 0: a literal here; else the best match's length - 3
    uint32_t start[PNG_BLOCK / 32];     // token starts of the greedy walk
    uint32_t ll_freq[NLLF], d_freq[32], cl_freq[NCL + 1], extra_bits;
    uint8_t ll_len[NLLF], d_len[32], cl_len[NCL + 1];
    uint16_t cl_code[NCL + 1];
    uint8_t rle_sym[NLL + ND + 4], rle_extra[NLL + ND + 4];
    int rle_count;
    uint32_t hdr[HDR_WORDS];
    TableScratch tab;
};

// grid (blocks of the frame, n).  tok: per position 0xffff (inside a match) or distance index << 8 | v
__global__ __launch_bounds__(THREADS) void png_match_kernel(const uint8_t* __restrict__ filt, size_t S, size_t nblk, Dists dists, uint16_t* __restrict__ tok,
                                                            BlockTab* __restrict__ tabs, uint32_t* __restrict__ bbits) {
    __shared__ MatchShared sh;
    const int t = threadIdx.x;
    const size_t f = blockIdx.y, blk = blockIdx.x, b0 = blk * PNG_BLOCK;
    const int len = (int)min((size_t)PNG_BLOCK, S - b0);
    const uint8_t* F = filt + f * S;
    uint16_t* T = tok + f * S + b0;
    for (int i = t; i < PNG_BLOCK / 32; i += THREADS) sh.start[i] = 0;
    for (int i = t; i < NLLF; i += THREADS) sh.ll_freq[i] = 0;
    if (t < 32) sh.d_freq[t] = 0;
    if (t == 0) sh.extra_bits = 0;
    for (int i = t; i < len; i += THREADS) {
        const size_t p = b0 + i;
        const int cap = min(MAX_MATCH, len - i);
        int best = 0, which = 0;
        for (int k = 0; k < dists.count; ++k) {
            const size_t d = (size_t)dists.d[k];
            if (d > p) break;                   // ascending: the rest would start before the stream too
            int run = 0;
            while (run < cap && F[p + run] == F[p + run - d]) ++run;
            if (run > best) best = run, which = k;
            if (best == cap) break;
        }
        const int v = best >= MIN_MATCH ? best - 3 : 0;
        sh.v[i] = (uint8_t)v;
        T[i] = (uint16_t)(which << 8 | v);
    }
    __syncthreads();
    if (t == 0) {
        uint32_t word = 0;
        int at = 0;
        for (int p = 0; p < len;) {
            if (p >> 5 != at) sh.start[at] = word, word = 0, at = p >> 5;
            word |= 1u << (p & 31);
            const int v = sh.v[p];
            p += v ? v + 3 : 1;
        }
        sh.start[at] = word;
    }
    __syncthreads();
    uint32_t extra = 0;
    for (int i = t; i < len; i += THREADS) {
        if (!(sh.start[i >> 5] >> (i & 31) & 1)) { T[i] = 0xffff; continue; }
        const int v = sh.v[i];
        if (!v) { atomicAdd(&sh.ll_freq[F[b0 + i]], 1u); continue; }
        int eb, ev;
        atomicAdd(&sh.ll_freq[257 + length_symbol(v + 3, &eb, &ev)], 1u);
        extra += eb;
        atomicAdd(&sh.d_freq[dist_symbol(dists.d[T[i] >> 8], &eb, &ev)], 1u);
        extra += eb;
    }
    if (extra) atomicAdd(&sh.extra_bits, extra);
    if (t == 0) sh.ll_freq[256] = 1;
    build_lengths(sh.ll_freq, NLL, 15, sh.ll_len, sh.tab);
    build_lengths(sh.d_freq, ND, 15, sh.d_len, sh.tab);
    int hlit = 0, hdist = 0;
    if (t == 0) {
        bool any = false;
        for (int i = 0; i < ND; ++i) any |= sh.d_len[i] != 0;
        if (!any) sh.d_len[0] = 1;
        for (int i = 0; i < NLL; ++i)
            if (sh.ll_len[i]) hlit = i + 1;
        for (int i = 0; i < ND; ++i)
            if (sh.d_len[i]) hdist = i + 1;
        for (int i = 0; i < NCL + 1; ++i) sh.cl_freq[i] = 0;
        // the run-length code of ll_len[0..hlit) ++ d_len[0..hdist)
        const int total = hlit + hdist;
        auto at = [&](int i) { return (int)(i < hlit ? sh.ll_len[i] : sh.d_len[i - hlit]); };
        int count = 0;
        auto emit = [&](int sym, int ex) { sh.rle_sym[count] = (uint8_t)sym, sh.rle_extra[count++] = (uint8_t)ex, ++sh.cl_freq[sym]; };
        for (int i = 0; i < total;) {
            const int v = at(i);
            int r = 1;
            while (i + r < total && at(i + r) == v) ++r;
            i += r;
            if (v == 0) {
                while (r >= 11) { const int k = min(r, 138); emit(18, k - 11), r -= k; }
                if (r >= 3) emit(17, r - 3), r = 0;
            } else {
                emit(v, 0), --r;
                while (r >= 3) { const int k = min(r, 6); emit(16, k - 3), r -= k; }
            }
            for (; r > 0; --r) emit(v, 0);
        }
        sh.rle_count = count;
    }
    build_lengths(sh.cl_freq, NCL, 7, sh.cl_len, sh.tab);
    if (t != 0) return;
    const uint8_t* order = CL_ORDER;
    int hclen = 4;
    for (int i = 0; i < NCL; ++i)
        if (sh.cl_len[order[i]]) hclen = max(hclen, i + 1);
    uint32_t dyn = 2 + 14 + 3 * hclen + sh.extra_bits, fixed = 2 + sh.extra_bits;
    for (int i = 0; i < sh.rle_count; ++i) {
        const int s = sh.rle_sym[i];
        dyn += sh.cl_len[s] + (s == 16 ? 2 : s == 17 ? 3 : s == 18 ? 7 : 0);
    }
    for (int i = 0; i < NLL; ++i) dyn += sh.ll_freq[i] * sh.ll_len[i], fixed += sh.ll_freq[i] * fixed_ll_len(i);
    for (int i = 0; i < ND; ++i) dyn += sh.d_freq[i] * sh.d_len[i], fixed += sh.d_freq[i] * 5;
    const bool dynamic = dyn < fixed;
    BlockTab& tab = tabs[f * nblk + blk];
    const uint32_t last = blk + 1 == nblk;
    uint32_t hdr_bits = 3;
    if (!dynamic) {
        for (int i = 0; i < NLLF; ++i) sh.ll_len[i] = (uint8_t)fixed_ll_len(i);
        for (int i = 0; i < 32; ++i) sh.d_len[i] = i < ND ? 5 : 0;
        tab.hdr[0] = last | 1u << 1;
    } else {
        for (int i = NLL; i < NLLF; ++i) sh.ll_len[i] = 0;
        for (int i = ND; i < 32; ++i) sh.d_len[i] = 0;
        canonical_codes(sh.cl_len, NCL, sh.cl_code);
        // the header, packed LSB first into LDS words and copied out
        uint64_t acc = 0;
        int have = 0, words = 0;
        auto put = [&](uint32_t value, int count) {
            acc |= (uint64_t)value << have, have += count;
            if (have >= 32) sh.hdr[words++] = (uint32_t)acc, acc >>= 32, have -= 32;
        };
        put(last, 1), put(2, 2), put(hlit - 257, 5), put(hdist - 1, 5), put(hclen - 4, 4);
        for (int i = 0; i < hclen; ++i) put(sh.cl_len[order[i]], 3);
        for (int i = 0; i < sh.rle_count; ++i) {
            const int s = sh.rle_sym[i];
            put(sh.cl_code[s], sh.cl_len[s]);
            if (s >= 16) put(sh.rle_extra[i], s == 16 ? 2 : s == 17 ? 3 : 7);
        }
        hdr_bits = (uint32_t)(words * 32 + have);
        if (have) sh.hdr[words++] = (uint32_t)acc;
        for (int i = 0; i < words; ++i) tab.hdr[i] = sh.hdr[i];
    }
    canonical_codes(sh.ll_len, NLLF, tab.ll_code);
    canonical_codes(sh.d_len, 32, tab.d_code);
    for (int i = 0; i < NLLF; ++i) tab.ll_len[i] = sh.ll_len[i];
    for (int i = 0; i < 32; ++i) tab.d_len[i] = sh.d_len[i];
    tab.hdr_bits = hdr_bits;
    bbits[f * nblk + blk] = 1 + (dynamic ? dyn : fixed);
}

// ---- scan, zero ---------------------------------------------------------------------------------------------------------------------------
// grid n.  boff: the stream bit at which every block starts (the zlib header's 16 in front); total: the bit behind the last block
__global__ __launch_bounds__(THREADS) void png_scan_kernel(const uint32_t* __restrict__ bbits, size_t nblk, uint64_t* __restrict__ boff, uint64_t* __restrict__ total) {
    __shared__ unsigned long long part[THREADS / 64];
    const size_t f = blockIdx.x, per = (nblk + THREADS - 1) / THREADS, i0 = min(nblk, threadIdx.x * per), i1 = min(nblk, i0 + per);
    unsigned long long mine = 0, all;
    for (size_t i = i0; i < i1; ++i) mine += bbits[f * nblk + i];
    unsigned long long at = 16 + wg_exclusive<THREADS>(mine, part, &all);
    for (size_t i = i0; i < i1; ++i) boff[f * nblk + i] = at, at += bbits[f * nblk + i];
    if (threadIdx.x == 0) total[f] = 16 + all;
}

__device__ __forceinline__ size_t zlib_bytes(uint64_t total_bits) { return (size_t)((total_bits + 7) / 8) + 4; }

// grid (any, n).  The words the frame's zlib stream will touch; the first one carries the zlib header 78 01
__global__ __launch_bounds__(THREADS) void png_zero_kernel(uint32_t* __restrict__ stream, size_t stream_words, const uint64_t* __restrict__ total) {
    const size_t f = blockIdx.y, words = min(stream_words, (zlib_bytes(total[f]) + 3) / 4);
    uint32_t* s = stream + f * stream_words;
    for (size_t i = (size_t)blockIdx.x * THREADS + threadIdx.x; i < words; i += (size_t)gridDim.x * THREADS) s[i] = i ? 0u : 0x0178u;
}

// ---- emit ---------------------------------------------------------------------------------------------------------------------------------
// grid (blocks of the frame, n)
__global__ __launch_bounds__(THREADS) void png_emit_kernel(const uint8_t* __restrict__ filt, size_t S, size_t nblk, Dists dists, const uint16_t* __restrict__ tok,
                                                           const BlockTab* __restrict__ tabs, const uint64_t* __restrict__ boff, const uint64_t* __restrict__ total,
                                                           const unsigned long long* __restrict__ acc, uint32_t* __restrict__ stream, size_t stream_words) {
    __shared__ uint16_t ll_code[NLLF], d_code[32];
    __shared__ uint8_t ll_len[NLLF], d_len[32];
    __shared__ uint32_t part[THREADS / 64];
    const int t = threadIdx.x;
    const size_t f = blockIdx.y, blk = blockIdx.x, b0 = blk * PNG_BLOCK;
    const int len = (int)min((size_t)PNG_BLOCK, S - b0);
    const BlockTab& tab = tabs[f * nblk + blk];
    for (int i = t; i < NLLF; i += THREADS) ll_code[i] = tab.ll_code[i], ll_len[i] = tab.ll_len[i];
    if (t < 32) d_code[t] = tab.d_code[t], d_len[t] = tab.d_len[t];
    __syncthreads();
    const uint8_t* F = filt + f * S + b0;
    const uint16_t* T = tok + f * S + b0;
    uint32_t* s = stream + f * stream_words;
    const int i0 = min(len, t * PER_THREAD), i1 = min(len, i0 + PER_THREAD);
    uint32_t bits = 0;
    for (int i = i0; i < i1; ++i) {
        const uint32_t k = T[i];
        if (k == 0xffff) continue;
        const int v = k & 255;
        if (!v) { bits += ll_len[F[i]]; continue; }
        int eb, ev;
        bits += ll_len[257 + length_symbol(v + 3, &eb, &ev)] + eb;
        bits += d_len[dist_symbol(dists.d[k >> 8], &eb, &ev)] + eb;
    }
    uint32_t all;
    const uint32_t before = wg_exclusive<THREADS>(bits, part, &all);
    const uint64_t base = boff[f * nblk + blk], body = base + tab.hdr_bits;
    {
        BitWriter out(s, body + before);
        for (int i = i0; i < i1; ++i) {
            const uint32_t k = T[i];
            if (k == 0xffff) continue;
            const int v = k & 255;
            if (!v) { out.put(ll_code[F[i]], ll_len[F[i]]); continue; }
            int eb, ev;
            const int ls = 257 + length_symbol(v + 3, &eb, &ev);
            out.put(ll_code[ls], ll_len[ls]);
            out.put(ev, eb);
            const int ds = dist_symbol(dists.d[k >> 8], &eb, &ev);
            out.put(d_code[ds], d_len[ds]);
            out.put(ev, eb);
        }
        out.flush();
    }
    const int hdr_words = (int)((tab.hdr_bits + 31) / 32);
    if (t < hdr_words) {
        BitWriter out(s, base + 32ull * t);
        const int count = min(32, (int)tab.hdr_bits - 32 * t);
        out.put(count < 32 ? tab.hdr[t] & ((1u << count) - 1) : tab.hdr[t], count);
        out.flush();
    }
    if (t == THREADS - 1) {
        BitWriter out(s, body + all);
        out.put(ll_code[256], ll_len[256]);
        out.flush();
        if (blk + 1 == nblk) {              // the Adler-32 of the filtered stream, big-endian, at the next whole byte
            const uint32_t a = (uint32_t)((1 + acc[f * 4]) % ADLER), b = (uint32_t)((S % ADLER + acc[f * 4 + 1]) % ADLER);
            const uint32_t adler = b << 16 | a;
            BitWriter tail(s, (total[f] + 7) / 8 * 8);
            for (int k = 0; k < 4; ++k) tail.put(adler >> (24 - 8 * k) & 255, 8);
            tail.flush();
        }
    }
}

// ---- scatter, finish ----------------------------------------------------------------------------------------------------------------------
// a(x) b(x) mod the CRC-32 polynomial, reflected as CRC registers are
__device__ __forceinline__ uint32_t crc_multiply(uint32_t a, uint32_t b) {
    uint32_t p = 0;
    for (uint32_t m = 1u << 31; m; m >>= 1) {
        if (a & m) p ^= b;
        b = b & 1 ? (b >> 1) ^ CRC_POLY : b >> 1;
    }
    return p;
}
// x^bits mod the polynomial
__device__ __forceinline__ uint32_t crc_power(uint64_t bits) {
    uint32_t p = 1u << 31, sq = 1u << 30;
    for (; bits; bits >>= 1) {
        if (bits & 1) p = crc_multiply(sq, p);
        sq = crc_multiply(sq, sq);
    }
    return p;
}
__device__ __forceinline__ uint32_t crc_byte(uint32_t crc, uint32_t byte) {
    crc ^= byte;
    for (int k = 0; k < 8; ++k) crc = crc & 1 ? (crc >> 1) ^ CRC_POLY : crc >> 1;
    return crc;
}

// grid (any, n).  The zlib stream to out + 41, and into acc[2] the CRC register (from 0, no final inversion) of each PIECE of it advanced
// to the stream's end: their XOR is the register of the whole stream.
__global__ __launch_bounds__(THREADS) void png_scatter_kernel(const uint32_t* __restrict__ stream, size_t stream_words, const uint64_t* __restrict__ total,
                                                              unsigned long long* __restrict__ acc, uint8_t* __restrict__ out, size_t out_stride) {
    __shared__ uint32_t table[256];
    table[threadIdx.x] = crc_byte(0, threadIdx.x);
    __syncthreads();
    const size_t f = blockIdx.y, zlen = zlib_bytes(total[f]), pieces = (zlen + PIECE - 1) / PIECE;
    const uint32_t* s = stream + f * stream_words;
    uint8_t* o = out + f * out_stride + FILE_HEAD;
    for (size_t q = (size_t)blockIdx.x * THREADS + threadIdx.x; q < pieces; q += (size_t)gridDim.x * THREADS) {
        const size_t b0 = q * PIECE, b1 = min(zlen, b0 + PIECE);
        uint32_t crc = 0;
        for (size_t i = b0; i < b1; i += 4) {
            uint32_t word = s[i >> 2];
            for (size_t j = i; j < min(b1, i + 4); ++j, word >>= 8) {
                o[j] = (uint8_t)word;
                crc = table[(crc ^ word) & 255] ^ (crc >> 8);
            }
        }
        atomicXor(acc + f * 4 + 2, (unsigned long long)crc_multiply(crc, crc_power(8ull * (zlen - b1))));
    }
}

__device__ __forceinline__ void put_be32(uint8_t* p, uint32_t v) { p[0] = (uint8_t)(v >> 24), p[1] = (uint8_t)(v >> 16), p[2] = (uint8_t)(v >> 8), p[3] = (uint8_t)v; }

// grid ceil(n / 64), 64 threads: a thread per frame
__global__ void png_finish_kernel(int n, int h, int w, int c, const uint64_t* __restrict__ total, const unsigned long long* __restrict__ acc, uint8_t* __restrict__ out,
                                  size_t out_stride, int32_t* __restrict__ lengths) {
    const int f = blockIdx.x * 64 + threadIdx.x;
    if (f >= n) return;
    uint8_t* o = out + (size_t)f * out_stride;
    const size_t zlen = zlib_bytes(total[f]);
    const uint8_t sig[8] = {0x89, 'P', 'N', 'G', '\r', '\n', 0x1a, '\n'};
    for (int i = 0; i < 8; ++i) o[i] = sig[i];
    put_be32(o + 8, 13);
    o[12] = 'I', o[13] = 'H', o[14] = 'D', o[15] = 'R';
    put_be32(o + 16, (uint32_t)w), put_be32(o + 20, (uint32_t)h);
    o[24] = 8, o[25] = c == 3 ? 2 : 0, o[26] = 0, o[27] = 0, o[28] = 0;
    uint32_t crc = 0xffffffffu;
    for (int i = 12; i < 29; ++i) crc = crc_byte(crc, o[i]);
    put_be32(o + 29, ~crc);
    put_be32(o + 33, (uint32_t)zlen);
    o[37] = 'I', o[38] = 'D', o[39] = 'A', o[40] = 'T';
    // CRC-32 of "IDAT" ++ stream: the register starts at all ones, which is the type's four bytes inverted in a register that starts at 0
    uint32_t type = 0;
    for (int i = 37; i < 41; ++i) type = crc_byte(type, o[i] ^ 0xffu);
    crc = crc_multiply(type, crc_power(8ull * zlen)) ^ (uint32_t)acc[(size_t)f * 4 + 2];
    uint8_t* e = o + FILE_HEAD + zlen;
    put_be32(e, ~crc);
    put_be32(e + 4, 0);
    e[8] = 'I', e[9] = 'E', e[10] = 'N', e[11] = 'D';
    put_be32(e + 12, 0xae426082u);
    lengths[f] = (int32_t)(FILE_FRAME + zlen);
}

const char* check_png_shape(int n, int h, int w, int c) {
    if (n < 1 || n > 65535) return "n outside 1..65535";
    if (c != 1 && c != 3) return "channels other than 1 (L) and 3 (RGB)";
    if (h < 1 || h > 65535 || w < 1 || w > 65535) return "height or width outside 1..65535";
    if (make_png_plan(1, h, w, c).out_stride > (size_t)INT32_MAX) return "a worst-case file beyond 2^31 - 1 bytes (lengths are int32)";
    return nullptr;
}

}  // namespace

int png_encode_bytes(int n, int h, int w, int c, size_t* out_stride, size_t* workspace_bytes) {
    if (const char* bad = check_png_shape(n, h, w, c)) { set_error("png_encode_u8: %s (n %d, %d x %d x %d)", bad, n, h, w, c); return ADAIN_EINVAL; }
    const PngPlan p = make_png_plan(n, h, w, c);
    if (out_stride) *out_stride = p.out_stride;
    if (workspace_bytes) *workspace_bytes = p.total;
    return 0;
}

int launch_png_encode_u8(const uint8_t* src, int n, int h, int w, int c, int filter, uint8_t* out, size_t out_stride, int32_t* lengths, void* workspace,
                         size_t workspace_bytes, hipStream_t s) {
    const char* who = "png_encode_u8";
    if (!src || !out || !lengths) { set_error("%s: null pointer", who); return ADAIN_EINVAL; }
    const char* bad = check_png_shape(n, h, w, c);
    if (!bad && (filter < -1 || filter > 4)) bad = "filter outside -1 (adaptive), 0..4";
    if (bad) { set_error("%s: %s (n %d, %d x %d x %d, filter %d)", who, bad, n, h, w, c, filter); return ADAIN_EINVAL; }
    const PngPlan p = make_png_plan(n, h, w, c);
    if (out_stride < p.out_stride) { set_error("%s: out_stride %zu below the %zu of the size query", who, out_stride, p.out_stride); return ADAIN_EINVAL; }
    if (int rc = check_workspace(who, workspace, workspace_bytes, p.total, 8)) return rc;
    if ((uintptr_t)lengths % 4) { set_error("%s: lengths must be 4-byte aligned", who); return ADAIN_EINVAL; }
    char* ws = (char*)workspace;
    uint8_t* filt = (uint8_t*)(ws + p.o_filt);
    uint16_t* tok = (uint16_t*)(ws + p.o_tok);
    BlockTab* tabs = (BlockTab*)(ws + p.o_tabs);
    uint32_t* bbits = (uint32_t*)(ws + p.o_bbits);
    uint64_t* boff = (uint64_t*)(ws + p.o_boff);
    uint64_t* total = (uint64_t*)(ws + p.o_total);
    unsigned long long* acc = (unsigned long long*)(ws + p.o_acc);
    uint32_t* stream = (uint32_t*)(ws + p.o_stream);
    if (hipMemsetAsync(acc, 0, (size_t)n * 4 * sizeof(uint64_t), s) != hipSuccess) { set_error("%s: hipMemsetAsync failed", who); return ADAIN_ELAUNCH; }
    const unsigned spread = (unsigned)min((size_t)1024, (p.stream_words + THREADS - 1) / THREADS);
    const unsigned pieces = (unsigned)min((size_t)1024, (p.max_zlib / PIECE + THREADS) / THREADS);
    png_filter_kernel<<<dim3(h, n), THREADS, 0, s>>>(src, h, w, c, filter, filt, p.S, acc);
    png_match_kernel<<<dim3((unsigned)p.nblk, n), THREADS, 0, s>>>(filt, p.S, p.nblk, p.dists, tok, tabs, bbits);
    png_scan_kernel<<<n, THREADS, 0, s>>>(bbits, p.nblk, boff, total);
    png_zero_kernel<<<dim3(spread, n), THREADS, 0, s>>>(stream, p.stream_words, total);
    png_emit_kernel<<<dim3((unsigned)p.nblk, n), THREADS, 0, s>>>(filt, p.S, p.nblk, p.dists, tok, tabs, boff, total, acc, stream, p.stream_words);
    png_scatter_kernel<<<dim3(pieces, n), THREADS, 0, s>>>(stream, p.stream_words, total, acc, out, out_stride);
    png_finish_kernel<<<(n + 63) / 64, 64, 0, s>>>(n, h, w, c, total, acc, out, out_stride, lengths);
    return check_launch(who);
}

}  // namespace adain
