// Animated-GIF frame records on the device (gfx950), from the palette index planes csrc/palette.hip writes.  Replaces the host's
// Pillow save(save_all=True) of a clip (Style_3DGS/render.py:29-33 create_gif; video/utils.py:374-392 frames_to_video needs cv2's
// VideoWriter).  The file around the records is the host's: gif_file.py.  The rules, byte for byte: tests/gif_ref.py.
//
// One record per frame; its bytes are a function of the frame's indices, K and the delay alone.  The palette of a full-colour clip is chosen
// by csrc/quantize.hip; a frame's own colour table is spliced into its record by the host (gif_file.records_bytes), which these kernels
// know nothing of.
//   GCE        : 21 F9 04 04 dl dh 00 00 - disposal 1, no transparency, the delay in centiseconds, little endian.
//   descriptor : 2C 00 00 00 00 wl wh hl hh 00 - the full frame, no local table, not interlaced.
//   code size  : m = max(2, ceil(log2 K)); CLEAR = 2^m, EOI = CLEAR + 1, the first dictionary code is CLEAR + 2.
//   segments   : the h w indices in raster order, ADAIN_GIF_SEGMENT = 2048 to a segment, the last one may be shorter.  A segment is
//                CLEAR, then plain greedy LZW from an empty dictionary: the longest known string, one new entry per emitted code except
//                the segment's last.  EOI behind the last segment's codes.  With K <= 256 no code passes 2305: the 4096-code table never
//                fills.
//   widths     : the k-th code behind a CLEAR (k = 1, 2, ...) has w(k) bits, the smallest w >= m + 1 with 2^m + 1 + k <= 2^w.  A segment of
//                c codes is closed by the next CLEAR, or by EOI, as its code number c + 1 with w(c + 1) bits; the frame's first CLEAR has
//                m + 1.
//   packing    : codes LSB first, the last byte zero-padded; the D data bytes in sub-blocks of 255, each behind its length byte, the last
//                one may be shorter; a 00 terminator.  The record has 20 + D + ceil(D / 255) bytes.
// The bound: with W(c) = w(1) + ... + w(c), a segment of p pixels emits at most p codes and its closing code: at most W(p + 1) bits, so
// D <= ceil(((m + 1) + sum over the segments of W(p_s + 1)) / 8).
// An index >= K would collide with CLEAR: such a frame gets lengths[i] = 0 and no byte of its row; what the kernels use as an address is
// clamped to K - 1 first.
//
// Stages (5 launches and a memset, whatever n; nothing allocates or waits):
//   code   : a wave per segment, 8 segments to a workgroup.  The lanes stage the segment's indices in LDS (checked against K) and clear
//            the dictionary - 4096 slots of (prefix code, byte) << 12 | code, open addressing - then lane 0 walks the segment
//            (gif_lzw.h) and writes 16-bit codes and their count.  The probe is a bounded for loop; no wave waits for another.
//   scan   : a workgroup per frame - W(c + 1) of every segment, where its bits start, the frame's total
//   zero   : the frame's bit stream, as far as it will be written
//   emit   : a workgroup per segment - code k starts W(k - 1) bits into the segment, so every thread places its codes without a scan;
//            CLEAR in front of the first segment, CLEAR or EOI behind each, by atomicOr, LSB first
//   blocks : data byte j to 19 + j + j / 255 + 1 of the record, the length bytes, the terminator, GCE, descriptor, code size, lengths[i]
#include "device_utils.h"
#include "gif_lzw.h"

namespace adain {
namespace {

using gif::SEGMENT;
constexpr int THREADS = 256;
constexpr int SEGS = 8;                 // segments (waves) per workgroup of the code kernel: 8 (16 KiB + 2 KiB) = 144 of the CU's 160 KiB
constexpr int PER_THREAD = (SEGMENT + 1 + THREADS - 1) / THREADS;         // codes per thread of emit, the closing one included

struct GifPlan {
    int m;
    size_t pixels, nseg, max_data, stream_words, out_stride;
    size_t o_codes, o_counts, o_soff, o_total, o_bad, o_stream, total;
};

// The one layout of a call
GifPlan make_gif_plan(int n, int h, int w, int K) {
    GifPlan p{};
    p.m = gif::min_code_size(K);
    p.pixels = (size_t)h * w;
    p.nseg = (p.pixels + SEGMENT - 1) / SEGMENT;
    p.max_data = (size_t)gif::worst_data_bytes(p.pixels, p.m);
    p.stream_words = (p.max_data + 3) / 4 + 1;
    p.out_stride = (size_t)gif::record_bytes(p.max_data);
    const size_t N = (size_t)n;
    Carve ws;
    p.o_codes = ws.take(N * p.nseg * SEGMENT * sizeof(uint16_t));
    p.o_counts = ws.take(N * p.nseg * sizeof(uint32_t));
    p.o_soff = ws.take(N * p.nseg * sizeof(uint64_t));
    p.o_total = ws.take(N * sizeof(uint64_t));
    p.o_bad = ws.take(N * sizeof(uint32_t));
    p.o_stream = ws.take(N * p.stream_words * sizeof(uint32_t));
    p.total = ws.at;
    return p;
}

// ---- code ---------------------------------------------------------------------------------------------------------------------------------
struct CodeShared {
    uint32_t table[SEGS][gif::TABLE_SLOTS];
    uint8_t px[SEGS][SEGMENT];
};

// grid (ceil(segments / SEGS), n), SEGS waves.  codes: SEGMENT per segment; counts: the codes of every segment; bad[f]: set when frame f has
// an index >= K (zeroed by the launcher)
__global__ __launch_bounds__(SEGS * 64) void gif_code_kernel(const uint8_t* __restrict__ index, size_t pixels, size_t nseg, int K, int m,
                                                             uint16_t* __restrict__ codes, uint32_t* __restrict__ counts, uint32_t* __restrict__ bad) {
    __shared__ CodeShared sh;
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const size_t f = blockIdx.y, seg = (size_t)blockIdx.x * SEGS + wv;
    const bool live = seg < nseg;
    int count = 0;
    if (live) {
        const size_t p0 = seg * SEGMENT;
        count = (int)min((size_t)SEGMENT, pixels - p0);
        const uint8_t* src = index + f * pixels + p0;
        bool over = false;
        for (int i = lane; i < count; i += 64) {
            const int v = src[i];
            over |= v >= K;
            sh.px[wv][i] = (uint8_t)min(v, K - 1);
        }
        if (over) bad[f] = 1;            // every writer writes the same value
        for (int i = lane; i < gif::TABLE_SLOTS; i += 64) sh.table[wv][i] = gif::EMPTY;
    }
    __syncthreads();
    if (live && lane == 0) counts[f * nseg + seg] = (uint32_t)gif::lzw_segment(sh.px[wv], count, m, sh.table[wv], codes + (f * nseg + seg) * SEGMENT);
}

// ---- scan, zero ---------------------------------------------------------------------------------------------------------------------------
// grid n.  soff: the stream bit at which every segment's first code starts (the first CLEAR's m + 1 in front); total: the frame's bits
__global__ __launch_bounds__(THREADS) void gif_scan_kernel(const uint32_t* __restrict__ counts, size_t nseg, int m, uint64_t* __restrict__ soff,
                                                           uint64_t* __restrict__ total) {
    __shared__ unsigned long long part[THREADS / 64];
    const size_t f = blockIdx.x, per = (nseg + THREADS - 1) / THREADS, i0 = min(nseg, threadIdx.x * per), i1 = min(nseg, i0 + per);
    unsigned long long mine = 0, all;
    for (size_t i = i0; i < i1; ++i) mine += gif::code_bits((int)min(counts[f * nseg + i], (uint32_t)SEGMENT) + 1, m);
    unsigned long long at = (unsigned long long)(m + 1) + wg_exclusive<THREADS>(mine, part, &all);
    for (size_t i = i0; i < i1; ++i) soff[f * nseg + i] = at, at += gif::code_bits((int)min(counts[f * nseg + i], (uint32_t)SEGMENT) + 1, m);
    if (threadIdx.x == 0) total[f] = (unsigned long long)(m + 1) + all;
}

// grid (any, n).  The words the frame's data bytes will touch
__global__ __launch_bounds__(THREADS) void gif_zero_kernel(uint32_t* __restrict__ stream, size_t stream_words, const uint64_t* __restrict__ total) {
    const size_t f = blockIdx.y, words = min(stream_words, (size_t)((gif::data_bytes(total[f]) + 3) / 4));
    uint32_t* s = stream + f * stream_words;
    for (size_t i = (size_t)blockIdx.x * THREADS + threadIdx.x; i < words; i += (size_t)gridDim.x * THREADS) s[i] = 0u;
}

// ---- emit ---------------------------------------------------------------------------------------------------------------------------------
// grid (segments, n)
__global__ __launch_bounds__(THREADS) void gif_emit_kernel(const uint16_t* __restrict__ codes, const uint32_t* __restrict__ counts, const uint64_t* __restrict__ soff,
                                                           size_t nseg, int m, uint32_t* __restrict__ stream, size_t stream_words) {
    const size_t f = blockIdx.y, seg = blockIdx.x;
    const int c = (int)min(counts[f * nseg + seg], (uint32_t)SEGMENT);
    const uint16_t* C = codes + (f * nseg + seg) * SEGMENT;
    uint32_t* s = stream + f * stream_words;
    const uint64_t base = soff[f * nseg + seg];
    const uint32_t clear = 1u << m;
    // codes k0 + 1 .. k1 of the segment's c + 1, the last of which closes it
    const int k0 = min(c + 1, (int)threadIdx.x * PER_THREAD), k1 = min(c + 1, k0 + PER_THREAD);
    if (k0 < k1) {
        BitWriter out(s, base + gif::code_bits(k0, m));
        for (int k = k0; k < k1; ++k) out.put(k < c ? C[k] : seg + 1 == nseg ? clear + 1 : clear, gif::code_width(k + 1, m));
        out.flush();
    }
    if (seg == 0 && threadIdx.x == THREADS - 1) {
        BitWriter out(s, 0);
        out.put(clear, m + 1);
        out.flush();
    }
}

// ---- blocks -------------------------------------------------------------------------------------------------------------------------------
// grid (any, n).  Frame f's record into row f of out, lengths[f]; nothing for a frame with a bad index but lengths[f] = 0
__global__ __launch_bounds__(THREADS) void gif_blocks_kernel(const uint32_t* __restrict__ stream, size_t stream_words, const uint64_t* __restrict__ total,
                                                             const uint32_t* __restrict__ bad, int h, int w, int m, int delay_cs, uint8_t* __restrict__ out,
                                                             size_t out_stride, int32_t* __restrict__ lengths) {
    const size_t f = blockIdx.y;
    const bool first = blockIdx.x == 0 && threadIdx.x == 0;
    if (bad[f]) {
        if (first) lengths[f] = 0;
        return;
    }
    const size_t D = (size_t)gif::data_bytes(total[f]), nblocks = (D + 254) / 255;
    const uint8_t* s = (const uint8_t*)(stream + f * stream_words);
    uint8_t* o = out + f * out_stride;
    const size_t step = (size_t)gridDim.x * THREADS, t = (size_t)blockIdx.x * THREADS + threadIdx.x;
    for (size_t j = t; j < D; j += step) o[gif::HEAD + j + j / 255 + 1] = s[j];
    for (size_t b = t; b < nblocks; b += step) o[gif::HEAD + b * 256] = (uint8_t)min((size_t)255, D - b * 255);
    if (first) {
        const uint8_t head[gif::HEAD] = {0x21, 0xf9, 0x04, 0x04, (uint8_t)delay_cs, (uint8_t)(delay_cs >> 8), 0, 0,
                                         0x2c, 0, 0, 0, 0, (uint8_t)w, (uint8_t)(w >> 8), (uint8_t)h, (uint8_t)(h >> 8), 0, (uint8_t)m};
        for (int i = 0; i < gif::HEAD; ++i) o[i] = head[i];
        o[gif::HEAD + D + nblocks] = 0;
        lengths[f] = (int32_t)gif::record_bytes(D);
    }
}

const char* check_gif_shape(int n, int h, int w, int K) {
    if (n < 1 || n > 65535) return "n outside 1..65535";
    if (K < 1 || K > 256) return "K outside 1..256";
    if (h < 1 || h > 65535 || w < 1 || w > 65535) return "height or width outside 1..65535";
    if (gif::record_bytes(gif::worst_data_bytes((uint64_t)h * w, gif::min_code_size(K))) > (uint64_t)INT32_MAX) return "a worst-case record beyond 2^31 - 1 bytes (lengths are int32)";
    return nullptr;
}

}  // namespace

int gif_encode_bytes(int n, int h, int w, int K, size_t* out_stride, size_t* workspace_bytes) {
    if (const char* bad = check_gif_shape(n, h, w, K)) { set_error("gif_encode_u8: %s (n %d, %d x %d, K %d)", bad, n, h, w, K); return ADAIN_EINVAL; }
    const GifPlan p = make_gif_plan(n, h, w, K);
    if (out_stride) *out_stride = p.out_stride;
    if (workspace_bytes) *workspace_bytes = p.total;
    return 0;
}

int launch_gif_encode_u8(const uint8_t* index, int n, int h, int w, int K, int delay_cs, uint8_t* out, size_t out_stride, int32_t* lengths, void* workspace,
                         size_t workspace_bytes, hipStream_t s) {
    const char* who = "gif_encode_u8";
    if (!index || !out || !lengths) { set_error("%s: null pointer", who); return ADAIN_EINVAL; }
    const char* bad = check_gif_shape(n, h, w, K);
    if (!bad && (delay_cs < 0 || delay_cs > 65535)) bad = "delay_cs outside 0..65535";
    if (bad) { set_error("%s: %s (n %d, %d x %d, K %d, delay_cs %d)", who, bad, n, h, w, K, delay_cs); return ADAIN_EINVAL; }
    const GifPlan p = make_gif_plan(n, h, w, K);
    if (out_stride < p.out_stride) { set_error("%s: out_stride %zu below the %zu of the size query", who, out_stride, p.out_stride); return ADAIN_EINVAL; }
    if (int rc = check_workspace(who, workspace, workspace_bytes, p.total, 8)) return rc;
    if ((uintptr_t)lengths % 4) { set_error("%s: lengths must be 4-byte aligned", who); return ADAIN_EINVAL; }
    char* ws = (char*)workspace;
    uint16_t* codes = (uint16_t*)(ws + p.o_codes);
    uint32_t* counts = (uint32_t*)(ws + p.o_counts);
    uint64_t* soff = (uint64_t*)(ws + p.o_soff);
    uint64_t* total = (uint64_t*)(ws + p.o_total);
    uint32_t* flags = (uint32_t*)(ws + p.o_bad);
    uint32_t* stream = (uint32_t*)(ws + p.o_stream);
    if (hipMemsetAsync(flags, 0, (size_t)n * sizeof(uint32_t), s) != hipSuccess) { set_error("%s: hipMemsetAsync failed", who); return ADAIN_ELAUNCH; }
    const unsigned groups = (unsigned)((p.nseg + SEGS - 1) / SEGS);
    const unsigned spread = (unsigned)min((size_t)1024, (p.max_data + THREADS - 1) / THREADS);
    gif_code_kernel<<<dim3(groups, n), SEGS * 64, 0, s>>>(index, p.pixels, p.nseg, K, p.m, codes, counts, flags);
    gif_scan_kernel<<<n, THREADS, 0, s>>>(counts, p.nseg, p.m, soff, total);
    gif_zero_kernel<<<dim3(spread, n), THREADS, 0, s>>>(stream, p.stream_words, total);
    gif_emit_kernel<<<dim3((unsigned)p.nseg, n), THREADS, 0, s>>>(codes, counts, soff, p.nseg, p.m, stream, p.stream_words);
    gif_blocks_kernel<<<dim3(spread, n), THREADS, 0, s>>>(stream, p.stream_words, total, flags, h, w, p.m, delay_cs, out, out_stride, lengths);
    return check_launch(who);
}

}  // namespace adain
