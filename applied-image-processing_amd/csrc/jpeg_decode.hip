// The JPEG file decoders on the device: a file's entropy-coded segments -> the pixels Pillow decodes from the file.  The tables, the IDCT
// with its plane geometry and the colour arithmetic are the round trip's (jpeg.hip), shared through jpeg_common.h.
//
// The file decoder (adain_jpeg_decode_u8, adain_jpeg_decode_restart_u8): a baseline file's entropy-coded segment -> the pixels Pillow decodes from the file.  In short
//   taken     8-bit sequential Huffman files, one interleaved scan, grey or YCbCr with luma 1 x 1 / 2 x 1 / 2 x 2, with or without a
//             restart interval; the host (jpeg_file.py) walks the markers, refuses everything else and packs the file's tables into one blob
//   restart   the RSTn markers are found and removed HERE, while unstuffing; every interval is decoded from its own byte-aligned all-zero
//             state on a subsequence grid of its own, and the DC sums restart with it
//   entropy   the unstuffed stream is cut into subsequences; their exit states (bit position, block in the MCU, zigzag index) are iterated
//             inside one workgroup per file until a round changes none - the fixed point is the sequential decoder's, whatever the data -
//             then every subsequence writes its coefficients in parallel; garbage is decoded without leaving a buffer: a code in no table
//             costs one bit, a run past 63 ends the block, the reader pads with 1-bits, every index is clamped
//   status    per file: 0, or the stream (every interval of it) did not hold exactly the expected blocks ending inside its last byte,
//             or the restart markers are not the expected ones in order (the caller then uses PIL)
//   back half the round trip's, with the file's own quantisation tables, three chroma layouts and a grey path
//
// The progressive file decoder (adain_jpeg_decode_progressive_u8): the scans of an 8-bit progressive Huffman (SOF2) file with a complete
// script -> the same coefficient buffer, then the file decoder's back half unchanged.  Its rules, stages and launches per call follow the
// file decoder's below ("the progressive file decoder"); in short: every scan's segment is unstuffed on its own, the scans apply in
// file order, every Huffman-coded scan goes through the fixed-point scheme above with a state of its kind, a DC refinement is one lane
// per block, and an AC refinement's state carries the block it is in because the bits a block takes depend on the coefficients before it
//
// ---- the file decoder: a baseline file's entropy-coded segment -> pixels -----------------------------------------------------------------
// adain_jpeg_decode_u8 and adain_jpeg_decode_restart_u8.  The host (jpeg_file.py) walks the markers and hands over the file's bytes, where
// its entropy-coded segment lies, one blob of tables (FileTables) and the call's restart interval; everything behind that runs here.
// tests/jpeg_file_ref.py restates it in Python, tests/jpeg_restart_ref.py the restart rules.
//
// Its rules
//   files     one scan, 8-bit tables, one restart interval Ri per call (0: none; the old entry is the new one at 0)
//   stream    the segment with the 00 behind every FF removed; bits big-endian; the reader returns 1-bits past its end
//   restart   Ri > 0 MCUs, nmcu = mw mh, nint = ceil(nmcu / Ri): interval k holds the MCUs k Ri .. min((k+1) Ri, nmcu) - 1 and expects
//             bpm min(Ri, nmcu - k Ri) blocks.  Ri = 0: the whole stream is one interval of nmcu MCUs and nothing below changes today's scheme
//     segment   from behind SOS to EOI as before; it now holds FF D0..D7 pairs, and as unstuffed entropy data cannot, each such pair
//               is a marker.  Byte by byte, with Ri > 0 a byte is dropped when it is a 00 behind an FF, an FF in front of a D0..D7 that is
//               still in the segment, or a D0..D7 behind an FF; every other byte is kept
//     stream    the kept bytes.  Marker m (0-based, in file order) ends interval m; interval m + 1 begins at the stream byte behind it,
//               interval 0 at byte 0.  THIS code finds the markers, in the unstuff stage, and records each interval's first stream byte in
//               a per-file table in the workspace (a call still needs only its arguments and one upload).  A marker split over two
//               threads' bytes or two 4096-byte pieces, and a stuffed FF 00 directly in front of a marker (the common case, as the pad
//               bits are ones), are nothing special: every byte is judged by its two neighbours in the segment
//     reader    inside interval k the bits at or beyond the interval's end read as 1; decoding never continues from one interval into
//               the next; pad bits (at most 7 ones) complete no code, so they begin no block
//     grid      interval k is cut into subsequences of chunk_bits bits from its own first bit, the last one shorter: no subsequence
//               straddles an interval start.  In every round the first subsequence of an interval enters from (its first bit, block 0,
//               index 0), every other one from its left neighbour's exit state of the round before; the loop ends after the first round
//               that changed no exit state in any interval (which is the largest round count any interval needs on its own)
//     blocks    a block's index is k Ri bpm plus the number of blocks begun before it in interval k: a segmented exclusive scan of the
//               per-subsequence counts.  Blocks whose in-interval index is at or above the interval's expected count are written by
//               nobody and are not damage
//     DC        the running sum per component restarts at 0 at every interval's first MCU
//     status    non-zero when, in some interval: damage inside an expected block, a DC sum outside -2047..2047, fewer blocks than
//               expected, or the last expected block not ending inside the interval's last byte; when the markers found are not
//               nint - 1, or marker m is not FF D(m mod 8); when the decode did not settle.  With a wrong marker count or order the
//               entropy decode is skipped (no table entry is trusted) and the frame is that of all-zero coefficients.  Whatever the
//               bytes, every write stays inside dst, record and the workspace and the kernels terminate: a marker beyond the expected
//               count indexes nothing
//   symbol    libjpeg's look-up: the next 8 bits index look[] (length << 8 | symbol); a longer code is the first length l in 9..16 with
//             code <= maxcode[l], its symbol val[(valoff[l] + code) & 255]; when no length matches ONE bit is consumed and nothing else
//             changes (garbage is the normal case in round 0 of the decode, and a damaged file must not hang or leave its buffers)
//   DC        zigzag index 0: symbol & 15 = size s, then s bits v; difference = v when v >= 2^(s-1), else v - 2^s + 1; the index becomes 1
//   AC        symbol = run r << 4 | size s.  s = 0: r = 15 moves the index 16 on, any other r ends the block.  s > 0: the coefficient at
//             index + r (past 63: not written), the index moves behind it.  An index of 64 or more ends the block
//   blocks    per MCU the H x V luma blocks row-major, then Cb, Cr (grey: one block per MCU); a finished block moves on to the next
//   status    0, or: a code that is in no table, a DC size above 11, an AC size above 10 or a coefficient past 63 in one of the expected
//             blocks; a DC sum outside -2047..2047; fewer blocks than expected; a last block that does not end inside the last byte; a
//             decode that did not settle.  Blocks beyond the expected count are decoded by nobody.
//   DC        the differences are summed per component in scan order, kept as int16
//   samples   coefficient times the FILE's table entry of its component, then the IDCT of the round trip (jpeg.hip), unchanged
//   chroma    cropped to the real samples first (ch x cw; 4:2:0: ceil(h/2) x ceil(w/2), 4:2:2: h x ceil(w/2), 4:4:4: h x w).
//             4:2:0: h2v2_fancy_upsample as in the round trip (jpeg.hip).  4:2:2: h2v1_fancy_upsample - out[2c] = (3 C[c] + C[c-1] + 1) >> 2,
//             out[2c+1] = (3 C[c] + C[c+1] + 2) >> 2, the column clamped to 0..cw-1 (which gives libjpeg's end cases out[0] = C[0] and
//             out[2cw-1] = C[cw-1]).  Both: cw <= 2 (w <= 4) leaves the filter out and replicates every sample.  4:4:4: fullsize_upsample,
//             the samples themselves.  Grey: the luma plane is the output.
//
// Its stages (one workgroup per file where a stage is sequential in the file, otherwise one launch over all files)
//   table     the host's segment offsets and lengths reach the device as kernel arguments, 64 files per launch
//   unstuff   per 4096-byte piece: count the stuffed zeros (Ri > 0: and the marker bytes, and the markers), scan, scatter; the tail of
//             the stream is filled with FF.  Ri > 0: marker m puts its stream position at entry m + 1 of the file's interval table
//   settle    the stream is cut into subsequences of chunk_bits bits.  Round 0: every lane decodes its subsequence from the all-zero state
//             at its first bit until its position passes the subsequence's end, and stores its exit state (position, block in the MCU,
//             zigzag index).  Round r: lane s decodes subsequence s again from lane s - 1's exit state of round r - 1 (lane 0: from the
//             true start) - or copies its own, when that input did not change.  The loop ends after the first round that changed no exit
//             state, at most subsequences + 1 rounds.  The states then satisfy exit[s] = decode(s, exit[s-1]) for every s, a system with
//             one solution: the sequential decoder's.  No luck is involved, a periodic stream only takes more rounds.  Two state arrays
//             alternate, a workgroup barrier separates the rounds, nothing waits on another workgroup.  The blocks each subsequence
//             begins are counted on the way and scanned at the end.  Ri > 0: a scan over the interval table first gives every interval
//             its first subsequence (the table's second half); a subsequence finds its interval there by bisection, and every interval's
//             first subsequence enters from the known state in every round
//   write     fully parallel: every subsequence once more from its now known state and block index, the coefficients de-zigzagged as
//             int16 into the zero-filled buffer, each by exactly one lane, DC terms as differences
//   dc        per component the running sum in scan order, restarted at every interval's first MCU (a segmented sum over the
//             workgroup); the record (status, rounds) is written here
//   idct / pixels   the round trip's IDCT (jpeg_common.h) with the file's tables, and the three layouts
// Launches per call, whatever Ri: ceil(n / 64) table + unstuff + one memset + settle + write + dc + idct + pixels.
//
// ---- the progressive file decoder: the scans of an SOF2 file -> the coefficient buffer of the file decoder above ---------------------------
// adain_jpeg_decode_progressive_u8.  The host (jpeg_file.py, parse(progressive=True)) walks the markers, checks the scan script (every
// coefficient's first scan has Ah = 0, every later one Ah = its current Al and Al = Ah - 1, and at EOI every coefficient stands at Al = 0)
// and hands over, per file and scan, where the scan's entropy-coded segment lies and one FileTables blob with the Huffman tables in force
// at that SOS; per call the scan descriptors (components, Ss, Se, Ah, Al).  A complete progressive file holds the quantised coefficients of
// its sequential twin, so behind the scans the back half above runs unchanged.  tests/jpeg_progressive_ref.py restates the rules in Python.
//
// Its rules
//   streams   every scan's segment is unstuffed on its own (the 00 behind every FF removed); bits big-endian; the reader returns 1-bits
//             past the stream's end.  No restart intervals.
//   blocks    an interleaved scan (all components, DC only) covers the MCU grid in the baseline order; a one-component scan covers the
//             component's own raster, ceil(ceil(w Hi / Hmax) / 8) blocks a row and the same in h rows, row-major - for luma up to one
//             column and one row less than the MCU grid - and block (by, bx) of it is block (by % V) H + bx % H of MCU (by / V) mw + bx / H
//             in the coefficient buffer.  Blocks no scan codes stay zero.
//   symbol    as above: a code in no table costs ONE bit and is damage
//   DC first  (Ss = Se = 0, Ah = 0) symbol & 15 = size s, s bits v, the difference as above; the differences are summed per component
//             in SCAN order and the DC term is the sum << Al.  State: position, block in the MCU.
//   DC refine (Ah > 0) no Huffman code: bit i of the stream belongs to block i of the scan order; a set bit ORs 1 << Al into the DC term
//   AC first  (1 <= Ss <= Se, Ah = 0, one component) symbol = r << 4 | s at zigzag index k (a block begins at Ss).  s > 0: k += r, the
//             coefficient there is the value << Al, k += 1.  s = 0, r = 15: k += 16.  s = 0, r < 15: an end-of-band run of 2^r + the next
//             r bits: this block ends and run - 1 further blocks are empty - the whole run is taken in the step that reads it, so the
//             state is position and k alone and a step can begin tens of thousands of blocks.  k > Se ends the block.
//   AC refine (Ah > 0) libjpeg's decode_mcu_AC_refine.  Outside an end-of-band run: symbol r << 4 | s; s = 1: one sign bit follows AT ONCE;
//             s = 0, r < 15: run = 2^r + r bits, and the rest of this block is walked as a block inside the run; otherwise (s = 1, or
//             ZRL with r = 15) walk from k: a coefficient with history (non-zero before this scan) reads one correction bit, one
//             without counts r down and the walk stops at the first of them met with r = 0; s = 1 puts +-(1 << Al) there; k moves behind
//             it.  Inside a run a block reads one correction bit per coefficient with history from k to Se and ends.  A correction bit
//             that is set adds (1 << Al) away from zero where (coefficient & (1 << Al)) is 0.  The bits a block takes depend on which of
//             its coefficients have history, so the state is (position, block of the scan, k, blocks of the run still to end), the
//             history is a 64-bit mask per block taken BEFORE the scan's settle stage (which therefore reads no coefficient and writes
//             none), and decoding stops at the scan's last block: steps inside a run may take no bit at all
//   status    non-zero when in one of the blocks a scan covers: a code in no table, a DC size above 11, an AC size above 10 (first) or
//             above 1 (refine), a coefficient index past Se, a value << Al that is no int16; when a scan's last block does not end inside
//             its stream's last byte or is never reached (a DC refinement: the stream's last byte does not hold bit blocks - 1); when a
//             scan did not settle; when a final DC term is outside -2047..2047.  Whatever the bytes, every index is clamped or checked.
//
// Its stages
//   table, unstuff   the file decoder's kernels over n x scans streams, one launch of each (table: per 64 streams)
//   per scan, in file order
//     DC first    settle (the file decoder's scheme, one workgroup per file) + write (differences) + sum (per component in scan order)
//     DC refine   one launch, a lane per block
//     AC first    settle + write
//     AC refine   mask + settle + write
//   finish    the DC bound and the record: status, and the rounds summed over the Huffman-coded scans
//   idct / pixels   the file decoder's kernels, unchanged
// Launches per call: ceil(n scans / 64) table + unstuff + one memset + per scan 3 (DC first), 1 (DC refine), 2 (AC first) or 3 (AC refine)
// + finish + idct + pixels.
#include "jpeg_common.h"

namespace adain {
namespace {

constexpr int DEC_THREADS = 1024;       // of the per-file workgroups (unstuff, settle, dc)
constexpr int DEC_SEG_BATCH = 64;       // files per launch of the table kernel
constexpr int DEC_DEFAULT_CHUNK_BITS = 1024;

struct HuffTab {
    uint16_t look[256];
    int32_t maxcode[18];
    int32_t valoff[18];
    uint8_t val[256];
};
struct FileTables {             // the blob of jpeg_file.py
    HuffTab huff[4];            // DC0, DC1, AC0, AC1
    uint8_t q[3][64];           // per component, natural order
    uint8_t sel[8];             // DC table of components 0..2, AC table of components 0..2
};
static_assert(sizeof(HuffTab) == 912 && sizeof(FileTables) == 3848, "the blob layout of jpeg_file.py");

struct DecSeg { uint64_t off; uint32_t len, pad; };
struct DecSegBatch { uint64_t off[DEC_SEG_BATCH]; uint32_t len[DEC_SEG_BATCH]; };
struct DecMeta { uint32_t ulen, rounds, settled, err, done, nmark, merr, nsub; };        // per file, in the workspace
// ulen: stream bytes; err: damage in an expected block or an interval's last block ending outside its last byte; done: intervals whose last
// expected block ended; nmark: markers found; merr: a marker out of order; nsub: subsequences (0 when the marker structure is wrong)

// One call's geometry, sizes and workspace offsets (bytes), for both decoders.  A progressive call has `scans` streams per file, a wider
// state and the history mask, and no interval table; a baseline call has one stream per file, no mask, and the table when Ri > 0
struct DecPlan {
    DecPlanes g;
    uint32_t cap_words, nsub_max, chunk_bits;
    uint32_t ri, nint;          // MCUs per interval (Ri, or all of them at Ri = 0) and intervals
    size_t o_seg, o_meta, o_stream, o_state, o_count, o_mask, o_coef, o_planes, o_itab, total;          // itab: per file nint + 1 first stream bytes, nint + 1 first subsequences
};

const char* check_decode_shape(int n, int h, int w, int c, int sampling, int restart_interval, size_t max_segment_bytes, int chunk_bits) {
    if (n < 1 || n > 65535) return "n outside 1..65535";
    if (restart_interval < 0 || restart_interval > 65535) return "restart_interval outside 0..65535";
    if (c != 1 && c != 3) return "components other than 1 (grey) and 3 (YCbCr)";
    if (h < 1 || h > 65535 || w < 1 || w > 65535) return "height or width outside 1..65535";
    if (sampling < 0 || sampling > 2 || (c == 1 && sampling != 0)) return "sampling other than 0 (4:4:4, grey), 1 (4:2:2) and 2 (4:2:0)";
    if (max_segment_bytes >= ((size_t)1 << 28)) return "a segment of 2^28 bytes or more";
    if (chunk_bits != 0 && (chunk_bits < 32 || chunk_bits % 32 != 0)) return "chunk_bits that is neither 0 nor a multiple of 32 from 32 up";
    return nullptr;
}

DecPlan make_decode_plan(int n, int h, int w, int c, int sampling, int restart_interval, size_t max_segment_bytes, int chunk_bits, int scans, size_t state_bytes,
                         bool mask) {
    DecPlan p{};
    p.g = make_planes(h, w, c, sampling >= 1 ? 2 : 1, sampling == 2 ? 2 : 1);
    p.chunk_bits = chunk_bits ? (uint32_t)chunk_bits : (uint32_t)DEC_DEFAULT_CHUNK_BITS;
    p.cap_words = (uint32_t)((max_segment_bytes + 3) / 4 + 3);
    const uint32_t nmcu = (uint32_t)p.g.mw * (uint32_t)p.g.mh;
    p.ri = restart_interval ? (uint32_t)restart_interval : nmcu;
    p.nint = (nmcu + p.ri - 1) / p.ri;
    // every interval rounds its last subsequence up: the sum of ceil(bits_k / chunk_bits) is below ceil(bits / chunk_bits) + nint
    p.nsub_max = (uint32_t)((max_segment_bytes * 8 + p.chunk_bits - 1) / p.chunk_bits) + (restart_interval ? p.nint : 0u);
    if (p.nsub_max == 0) p.nsub_max = 1;
    const size_t N = (size_t)n, S = (size_t)scans;
    Carve ws;
    p.o_seg = ws.take(N * S * sizeof(DecSeg));
    p.o_meta = ws.take(N * S * sizeof(DecMeta));
    p.o_stream = ws.take(N * S * p.cap_words * sizeof(uint32_t));
    p.o_state = ws.take(3 * N * p.nsub_max * state_bytes);
    p.o_count = ws.take(N * p.nsub_max * sizeof(uint32_t));
    p.o_mask = ws.take(mask ? N * p.g.nblk * sizeof(uint64_t) : 0);
    p.o_coef = ws.take(N * p.g.nblk * 64 * sizeof(int16_t));
    p.o_planes = ws.take(N * p.g.stride);
    p.o_itab = ws.take(restart_interval ? N * 2 * ((size_t)p.nint + 1) * sizeof(uint32_t) : 0);
    p.total = ws.at;
    return p;
}

__global__ void jpegd_table_kernel(DecSegBatch b, int first, int count, DecSeg* __restrict__ seg, DecMeta* __restrict__ meta) {
    const int i = threadIdx.x;
    if (i >= count) return;
    seg[first + i] = DecSeg{b.off[i], b.len[i], 0u};
    meta[first + i] = DecMeta{0u, 0u, 0u, 0u, 0u, 0u, 0u, 0u};
}

// One DEC_THREADS-wide step of an exclusive scan over more entries than the workgroup has threads: the sum of the step's entries before
// this thread's v; *total: the sum of all of them, the same in every thread
__device__ __forceinline__ uint32_t scan_step(uint32_t v, uint32_t* part, uint32_t* total) {
    const uint32_t incl = workgroup_inclusive(v, part);
    __syncthreads();
    if (threadIdx.x == DEC_THREADS - 1) part[15] = incl;          // wave 15's slot is read only by waves above it: none
    __syncthreads();
    *total = part[15];
    return incl - v;
}

// out[i] = value(0) + ... + value(i - 1) for i < n, by the whole workgroup (out[i] may be what value(i) reads); returns the sum of all n
template <class Value>
__device__ __forceinline__ uint32_t scan_exclusive(uint32_t n, uint32_t* out, uint32_t* part, Value value) {
    uint32_t carry = 0, total;
    for (uint32_t base = 0; base < n; base += DEC_THREADS) {
        const uint32_t i = base + threadIdx.x;
        const uint32_t before = scan_step(i < n ? value(i) : 0u, part, &total);
        if (i < n) out[i] = carry + before;
        carry += total;
    }
    return carry;
}

// One workgroup per file: stream byte j = the j-th kept byte of the segment; then FF up to a whole word plus 8 bytes.  Dropped: a 00 behind
// an FF and, with RESTART, both bytes of every FF D0..D7 pair; marker m (counted over the file) puts the stream position behind it at
// itab[m + 1] when that is an interval's entry (m + 1 < nint) and is held to FF D(m mod 8).  itab[0] = 0 and itab[nint] = the stream's length.
template <bool RESTART>
__global__ __launch_bounds__(DEC_THREADS) void jpegd_unstuff_kernel(const uint8_t* __restrict__ files, const DecSeg* __restrict__ seg, DecMeta* __restrict__ meta,
                                                                    uint8_t* __restrict__ stream, uint32_t cap_words, uint32_t* __restrict__ itab, uint32_t nint) {
    __shared__ uint32_t part[16];
    const size_t f = blockIdx.x;
    const uint8_t* src = files + seg[f].off;
    const uint32_t len = seg[f].len;
    uint8_t* out = stream + f * cap_words * 4;          // len + 12 <= 4 cap_words
    uint32_t* tab = RESTART ? itab + f * 2 * ((size_t)nint + 1) : nullptr;
    uint32_t carry = 0, mcarry = 0;                     // stream bytes written, and markers met, by the pieces before
    bool order = false;
    for (uint32_t base = 0; base < len; base += DEC_THREADS * 4) {
        const uint32_t i0 = base + threadIdx.x * 4;
        uint8_t b[6];
#pragma unroll
        for (int k = 0; k < 6; ++k) {
            const uint32_t i = i0 + k;                  // b[0] is the byte before the thread's four, b[5] the one behind them
            b[k] = (i >= 1 && i - 1 < len) ? src[i - 1] : (uint8_t)0;
        }
        bool kept[4], mark[4];
        uint32_t keep = 0, marks = 0;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const uint32_t i = i0 + k;
            const bool behind_ff = i >= 1 && b[k] == 0xff;
            mark[k] = RESTART && i + 1 < len && b[k + 1] == 0xff && (b[k + 2] & 0xf8) == 0xd0;
            kept[k] = i < len && !(behind_ff && b[k + 1] == 0) && !mark[k] && !(RESTART && behind_ff && (b[k + 1] & 0xf8) == 0xd0);
            keep += kept[k] ? 1u : 0u, marks += mark[k] ? 1u : 0u;
        }
        // one scan for both counts: at most 4096 kept bytes and 2048 markers a piece
        uint32_t total;
        const uint32_t before = scan_step(keep | (marks << 16), part, &total);
        uint32_t at = carry + (before & 0xffffu), m = mcarry + (before >> 16);
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            if (kept[k]) out[at++] = b[k + 1];
            if (mark[k]) {
                if (m + 1 < nint) tab[m + 1] = at;
                if ((b[k + 2] & 7u) != (m & 7u)) order = true;
                ++m;
            }
        }
        carry += total & 0xffffu, mcarry += total >> 16;
    }
    const uint32_t end = ((carry + 3) & ~3u) + 8;
    for (uint32_t i = carry + threadIdx.x; i < end; i += DEC_THREADS) out[i] = 0xff;
    if (RESTART && order) meta[f].merr = 1;
    if (threadIdx.x == 0) {
        meta[f].ulen = carry, meta[f].nmark = mcarry;
        if (RESTART) tab[0] = 0, tab[nint] = carry;
    }
}

// 32 bits of the stream at bit position pos (big-endian), the bits at or beyond `stop` (the interval's end) as ones; the stream holds FF
// bytes past its own end, and the word index is clamped
__device__ __forceinline__ uint32_t peek32(const uint32_t* __restrict__ s, uint32_t last_word, uint32_t pos, uint32_t stop) {
    const uint32_t wi = min(pos >> 5, last_word - 1);
    const uint64_t v = ((uint64_t)__builtin_bswap32(s[wi]) << 32) | __builtin_bswap32(s[wi + 1]);
    const uint32_t bits = (uint32_t)((v << (pos & 31)) >> 32);
    if (pos + 32 <= stop) return bits;
    return pos >= stop ? 0xffffffffu : bits | (0xffffffffu >> (stop - pos));
}

// (length << 8) | symbol of the code at the top of `bits`, 0 when none matches
__device__ __forceinline__ uint32_t huff_symbol(const HuffTab& t, uint32_t bits) {
    const uint32_t e = t.look[bits >> 24];
    if (e) return e;
    for (int l = 9; l <= 16; ++l) {
        const int code = (int)(bits >> (32 - l));
        if (code <= t.maxcode[l]) return ((uint32_t)l << 8) | t.val[(t.valoff[l] + code) & 255];
    }
    return 0;
}

struct DecShape { int H, V, bpm, c; size_t nblk; uint32_t ri, nint; };

// The interval of subsequence i: its index, its first subsequence, its first bit and its end.  tab: the file's interval table (null at
// Ri = 0: one interval, the stream); its second half is searched for the last interval that begins at or before i (empty ones begin nothing).
struct DecInterval { uint32_t k, sub0, begin, stop; };
__device__ __forceinline__ DecInterval interval_of(uint32_t i, const uint32_t* __restrict__ tab, uint32_t nint, uint32_t nbits) {
    if (!tab) return DecInterval{0u, 0u, 0u, nbits};
    const uint32_t* sub = tab + nint + 1;
    uint32_t lo = 0, hi = nint;                         // sub[lo] <= i < sub[hi] = nsub
    while (hi - lo > 1) {
        const uint32_t mid = lo + (hi - lo) / 2;
        if (sub[mid] <= i) lo = mid; else hi = mid;
    }
    return DecInterval{lo, sub[lo], tab[lo] * 8, tab[lo + 1] * 8};
}

// Decodes from state st = (position, block in MCU << 8 | zigzag index) while position < end; the bits from `stop` on, the interval's end,
// read as ones.  Returns the exit state and counts the blocks begun.  WRITE: b is the index of the block current at st; coefficients of the
// interval's expected blocks b_lo <= b < b_end go to coef (natural order), and the last of them must end inside the interval's last byte.
template <bool WRITE>
__device__ __forceinline__ uint2 decode_span(const uint32_t* __restrict__ s, uint32_t last_word, uint32_t end, uint32_t stop, uint2 st, const FileTables& T_,
                                             const DecShape& g, uint32_t* begun, int16_t* __restrict__ coef, long long b, long long b_lo, long long b_end,
                                             DecMeta* __restrict__ meta) {
    uint32_t pos = st.x, blk = st.y >> 8, zz = st.y & 255, nb = 0;
    blk = blk < (uint32_t)g.bpm ? blk : 0;
    while (pos < end) {
        const int comp = g.c == 3 && (int)blk >= g.H * g.V ? (int)blk - g.H * g.V + 1 : 0;
        const uint32_t bits = peek32(s, last_word, pos, stop);
        const bool live = WRITE && b >= b_lo && b < b_end;
        const uint32_t e = huff_symbol(T_.huff[zz == 0 ? (T_.sel[comp] & 1) : 2 + (T_.sel[3 + comp] & 1)], bits);
        if (e == 0) {
            pos += 1;
            if (live) meta->err = 1;
            continue;
        }
        const uint32_t len = e >> 8, sym = e & 255, sz = sym & 15;
        // the value bits: len + sz <= 31
        const uint32_t v = sz ? (bits << len) >> (32 - sz) : 0u;
        const int value = (sz == 0 || v >= (1u << (sz - 1))) ? (int)v : (int)v - (1 << sz) + 1;
        if (zz == 0) {
            ++nb;
            pos += len + sz;
            if (live) {
                coef[(size_t)b * 64] = (int16_t)value;
                if (sym > 11) meta->err = 1;
            }
            zz = 1;
        } else if (sz == 0) {
            pos += len;
            zz = (sym >> 4) == 15 ? zz + 16 : 64;
        } else {
            pos += len + sz;
            const uint32_t k = zz + (sym >> 4);
            if (live) {
                if (k <= 63) coef[(size_t)b * 64 + T.zigzag[k]] = (int16_t)value;
                if (k > 63 || sz > 10) meta->err = 1;
            }
            zz = k + 1;
        }
        if (zz >= 64) {
            if (live && b == b_end - 1) {
                if (pos <= stop && pos + 8 > stop) atomicAdd(&meta->done, 1u); else meta->err = 1;
            }
            zz = 0, blk = blk + 1 == (uint32_t)g.bpm ? 0 : blk + 1, ++b;
        }
    }
    *begun = nb;
    return make_uint2(pos, (blk << 8) | zz);
}

__device__ __forceinline__ void load_tables(FileTables* dst, const uint8_t* __restrict__ blob) {
    for (int i = threadIdx.x; i < (int)sizeof(FileTables); i += blockDim.x) ((uint8_t*)dst)[i] = blob[i];
    __syncthreads();
}

__device__ __forceinline__ bool same_state(uint2 a, uint2 b) { return a.x == b.x && a.y == b.y; }
__device__ __forceinline__ bool same_state(uint4 a, uint4 b) { return a.x == b.x && a.y == b.y && a.z == b.z && a.w == b.w; }

// Subsequence i of a stream: its first bit, its end, the bit from which the reader returns ones, and whether it enters from the known
// state (its first bit, then zeros) in every round, as the first subsequence of a stream or of a restart interval does
struct DecSpan { uint32_t begin, end, stop; bool first; };

// The settle stage of one stream, by the whole workgroup: the rounds, then the scan of the block counts (cnt[s] becomes the blocks begun
// before subsequence s).  state: the stream's three arrays of nsub_max states - two that alternate as the rounds' exit states, and the
// state each subsequence was last decoded from.  span(i): the DecSpan of subsequence i; decode(sp, in, &begun): the exit state of
// decoding it from `in`, and the blocks begun on the way.  empty_settles: what a stream without subsequences is recorded as.
template <class S, class Span, class Decode>
__device__ __forceinline__ void settle(S* __restrict__ state, uint32_t* __restrict__ cnt, uint32_t nsub, uint32_t nsub_max, bool empty_settles,
                                       DecMeta* __restrict__ meta, uint32_t* part, Span span, Decode decode) {
    __shared__ int changed[2];
    const uint32_t t = threadIdx.x;
    S* st[2] = {state, state + nsub_max};
    S* last_in = state + 2 * (size_t)nsub_max;          // read and written by its lane only
    uint32_t rounds = 0, settled = 0;
    for (uint32_t r = 0; r <= nsub; ++r) {              // at most nsub + 1 rounds
        if (t == 0) changed[r & 1] = 0;
        __syncthreads();
        S* cur = st[r & 1];                             // written in this round, by lane i at i only
        const S* prev = st[(r & 1) ^ 1];                // the exit states of round r - 1: only read in this round
        int any = 0;
        for (uint32_t i = t; i < nsub; i += DEC_THREADS) {
            const DecSpan sp = span(i);
            S in{};
            in.x = sp.begin;
            if (r > 0 && !sp.first) in = prev[i - 1];
            S out;
            if (r > 0 && same_state(last_in[i], in)) {
                out = prev[i];                          // the same input as last time: the same exit state
            } else {
                uint32_t nb = 0;
                out = decode(sp, in, &nb);
                cnt[i] = nb;
                last_in[i] = in;
                if (r > 0 && !same_state(out, prev[i])) any = 1;
            }
            cur[i] = out;
        }
        if (any) changed[r & 1] = 1;
        __syncthreads();
        ++rounds;
        if (r > 0 && !changed[r & 1]) { settled = 1; break; }
    }
    if (nsub == 0 && empty_settles) settled = 1;
    scan_exclusive(nsub, cnt, part, [&](uint32_t i) { return cnt[i]; });
    if (t == 0) meta->rounds = rounds, meta->settled = settled, meta->nsub = nsub;
}

// One workgroup per file: (Ri > 0) every interval's first subsequence, then the settle stage (the write stage takes the interval's own
// first count off a subsequence's).
__global__ __launch_bounds__(DEC_THREADS) void jpegd_settle_kernel(const uint8_t* __restrict__ blobs, const uint32_t* __restrict__ stream, uint32_t cap_words,
                                                                   DecMeta* __restrict__ meta, uint2* __restrict__ state, uint32_t* __restrict__ count,
                                                                   uint32_t nsub_max, uint32_t chunk_bits, DecShape g, uint32_t* __restrict__ itab) {
    __shared__ FileTables ft;
    __shared__ uint32_t part[16];
    const size_t f = blockIdx.x;
    load_tables(&ft, blobs + f * sizeof(FileTables));
    const uint32_t* s = stream + f * cap_words;
    const uint32_t nbits = min(meta[f].ulen, (cap_words - 3) * 4) * 8;
    uint32_t* tab = itab ? itab + f * 2 * ((size_t)g.nint + 1) : nullptr;
    uint32_t nsub = (uint32_t)(((uint64_t)nbits + chunk_bits - 1) / chunk_bits);      // <= nsub_max
    if (tab) {
        // the table is whole only with nint - 1 markers in order: then its entries rise from 0 to the stream's length
        const bool whole = meta[f].nmark == g.nint - 1 && !meta[f].merr;
        const uint32_t total = scan_exclusive(whole ? g.nint : 0u, tab + g.nint + 1, part, [&](uint32_t k) {
            return (uint32_t)(((uint64_t)(tab[k + 1] - tab[k]) * 8 + chunk_bits - 1) / chunk_bits);
        });
        nsub = whole && total <= nsub_max ? total : 0u;
        if (threadIdx.x == 0) tab[2 * g.nint + 1] = nsub;
        __syncthreads();
    }
    // an empty stream is settled; a table that is not whole is not
    settle(state + f * 3 * nsub_max, count + f * nsub_max, nsub, nsub_max, !(tab && nbits), meta + f, part,
           [&](uint32_t i) {
               const DecInterval iv = interval_of(i, tab, g.nint, nbits);
               const uint32_t begin = iv.begin + (i - iv.sub0) * chunk_bits;
               return DecSpan{begin, (uint32_t)min(begin + chunk_bits, iv.stop), iv.stop, i == iv.sub0};
           },
           [&](const DecSpan& sp, uint2 in, uint32_t* nb) { return decode_span<false>(s, cap_words - 1, sp.end, sp.stop, in, ft, g, nb, nullptr, 0, 0, 0, nullptr); });
}

__global__ __launch_bounds__(256) void jpegd_write_kernel(const uint8_t* __restrict__ blobs, const uint32_t* __restrict__ stream, uint32_t cap_words,
                                                          DecMeta* __restrict__ meta, const uint2* __restrict__ state, const uint32_t* __restrict__ count,
                                                          uint32_t nsub_max, uint32_t chunk_bits, DecShape g, int16_t* __restrict__ coef,
                                                          const uint32_t* __restrict__ itab) {
    __shared__ FileTables ft;
    const size_t f = blockIdx.y;
    load_tables(&ft, blobs + f * sizeof(FileTables));
    const uint32_t nbits = min(meta[f].ulen, (cap_words - 3) * 4) * 8;
    const uint32_t nsub = meta[f].nsub;
    const uint32_t i = blockIdx.x * 256 + threadIdx.x;
    if (i >= nsub) return;
    const DecInterval iv = interval_of(i, itab ? itab + f * 2 * ((size_t)g.nint + 1) : nullptr, g.nint, nbits);
    const uint2* exit_state = state + f * 3 * nsub_max;         // both arrays hold the settled states
    const uint32_t begin = iv.begin + (i - iv.sub0) * chunk_bits;
    const uint2 in = i == iv.sub0 ? make_uint2(begin, 0u) : exit_state[i - 1];
    const uint32_t* cnt = count + f * nsub_max;
    const size_t mcu0 = (size_t)iv.k * g.ri, nmcu = g.nblk / g.bpm;
    const long long b_lo = (long long)(mcu0 * g.bpm), b_end = b_lo + (long long)(min((size_t)g.ri, nmcu - mcu0) * g.bpm);
    const long long b = b_lo + (long long)(cnt[i] - cnt[iv.sub0]) - ((in.y & 255) ? 1 : 0);       // a block under way was begun further left
    uint32_t nb;
    decode_span<true>(stream + f * cap_words, cap_words - 1, min(begin + chunk_bits, iv.stop), iv.stop, in, ft, g, &nb, coef + f * g.nblk * 64, b, b_lo, b_end,
                      meta + f);
}

// the segmented sum of the threads before this one, back to and with the nearest whose flag is set; part: 32 ints of LDS
__device__ __forceinline__ int decode_exclusive_segmented(int v, int flag, int* part) {
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    for (int d = 1; d < 64; d <<= 1) {
        const int uv = __shfl_up(v, d), uf = __shfl_up(flag, d);
        if (lane >= d) {
            if (!flag) v += uv;
            flag |= uf;
        }
    }
    __syncthreads();                                   // the previous pass has read part
    if (lane == 63) part[wv] = v, part[16 + wv] = flag;
    __syncthreads();
    int before = 0;                                    // of the waves below
    for (int k = 0; k < wv; ++k) before = part[16 + k] ? part[k] : before + part[k];
    const int ev = __shfl_up(v, 1), ef = __shfl_up(flag, 1);
    if (lane == 0) return before;
    return ef ? ev : before + ev;
}

// block i of component comp in the order of an interleaved scan -> its index in the MCU-ordered coefficient buffer
__device__ __forceinline__ size_t interleaved_block(const DecShape& g, int comp, size_t i) {
    const int hv = g.H * g.V;
    return comp == 0 ? (i / hv) * g.bpm + i % hv : i * g.bpm + hv + comp - 1;
}

// One workgroup per file: DC differences -> DC terms per component in scan order, from 0 at every interval's first MCU; then the record.
__global__ __launch_bounds__(DEC_THREADS) void jpegd_dc_kernel(int16_t* __restrict__ coef, const DecMeta* __restrict__ meta, DecShape g, int32_t* __restrict__ record) {
    __shared__ int part[32];
    __shared__ int range_err;
    const size_t f = blockIdx.x;
    const int t = threadIdx.x, hv = g.H * g.V;
    int16_t* fc = coef + f * g.nblk * 64;
    const size_t nmcu = g.nblk / g.bpm;
    if (t == 0) range_err = 0;
    int bad = 0;
    for (int comp = 0; comp < g.c; ++comp) {
        const size_t cnt = comp == 0 ? nmcu * hv : nmcu;
        const size_t per = (cnt + DEC_THREADS - 1) / DEC_THREADS;
        const size_t a = min((size_t)t * per, cnt), e = min(a + per, cnt);
        auto block_of = [&](size_t i) { return interleaved_block(g, comp, i); };
        auto restarts = [&](size_t i) { return comp == 0 ? i % ((size_t)g.ri * hv) == 0 : i % g.ri == 0; };      // an interval's first block of the component
        int sum = 0, flag = 0;
        for (size_t i = a; i < e; ++i) {
            if (restarts(i)) sum = 0, flag = 1;
            sum += fc[block_of(i) * 64];
        }
        int run = decode_exclusive_segmented(sum, flag, part);
        for (size_t i = a; i < e; ++i) {
            if (restarts(i)) run = 0;
            run += fc[block_of(i) * 64];
            if (run > 2047 || run < -2047) bad = 1;
            fc[block_of(i) * 64] = (int16_t)run;
        }
    }
    __syncthreads();
    if (bad) range_err = 1;
    __syncthreads();
    if (t == 0) {
        const DecMeta m = meta[f];
        const bool ok = m.settled && !m.err && !range_err && !m.merr && m.nmark + 1 == g.nint && m.done == g.nint;
        record[2 * f] = ok ? 0 : 1;
        record[2 * f + 1] = (int32_t)m.rounds;
    }
}

// The IDCT stage on natural-order coefficients, dequantised by the file's own tables.  blob_stride: bytes from one file's tables to the
// next file's (a progressive file has a blob per scan).
__global__ __launch_bounds__(IDCT_PER_WG * 8) void jpegd_idct_kernel(const int16_t* __restrict__ coef, const uint8_t* __restrict__ blobs, size_t blob_stride,
                                                                     uint8_t* __restrict__ planes, DecPlanes g) {
    __shared__ int samp[IDCT_PER_WG * 72];
    __shared__ int q[192];
    if (threadIdx.x < 192) q[threadIdx.x] = blobs[(size_t)blockIdx.y * blob_stride + offsetof(FileTables, q) + threadIdx.x];
    __syncthreads();
    idct_blocks(coef, planes, g, samp, [&](int* sb, uint32_t v, int i, int comp) {
        const int* qt = q + comp * 64 + 2 * i;
        int* p = sb + (i >> 2) * 9 + 2 * (i & 3);
        p[0] = (int)(int16_t)(v & 0xffff) * qt[0];
        p[1] = (int)(int16_t)(v >> 16) * qt[1];
    });
}

// One lane per pixel.  C = 1: the luma sample; C = 3: upsampling by the file's layout (g.H, g.V) and libjpeg's YCbCr -> RGB.
template <int C>
__global__ __launch_bounds__(256) void jpegd_pixels_kernel(const uint8_t* __restrict__ planes, DecPlanes g, int h, int w, uint8_t* __restrict__ dst) {
    const int x = blockIdx.x * 256 + threadIdx.x, y = blockIdx.y;
    if (x >= w) return;
    const uint8_t* fp = planes + (size_t)blockIdx.z * g.stride;
    uint8_t* d = dst + (((size_t)blockIdx.z * h + y) * w + x) * C;
    const int yy = fp[(size_t)y * g.yw + x];
    if (C == 1) { d[0] = (uint8_t)yy; return; }
    const int ch = g.V == 2 ? (h + 1) >> 1 : h, cw = g.H == 2 ? (w + 1) >> 1 : w;
    const int r = g.V == 2 ? y >> 1 : y, cc = g.H == 2 ? x >> 1 : x;
    int uv[2];
#pragma unroll
    for (int k = 0; k < 2; ++k) {
        const uint8_t* pl = fp + (k ? g.o_cr : g.o_cb);
        const uint8_t* a = pl + (size_t)r * g.cw;
        if (g.H == 1 || cw <= 2) {
            uv[k] = a[cc];                              // fullsize_upsample, or the narrow case: replication
        } else {
            const int cn = (x & 1) ? min(cc + 1, cw - 1) : max(cc - 1, 0);
            if (g.V == 2) {
                const int rn = (y & 1) ? min(r + 1, ch - 1) : max(r - 1, 0);
                const uint8_t* b = pl + (size_t)rn * g.cw;
                uv[k] = h2v2_sample(h2v2_column(a, b, cc), h2v2_column(a, b, cn), x & 1);
            } else {
                uv[k] = (3 * a[cc] + a[cn] + ((x & 1) ? 2 : 1)) >> 2;
            }
        }
    }
    ycc_to_rgb(yy, uv[0], uv[1], d);
}

// ---- the progressive file decoder: the scans of an SOF2 file -> the coefficient buffer of the file decoder above ---------------------------
constexpr int PROG_MAX_SCANS = 32;

struct ProgScan { int ncomp, comp, ss, se, ah, al; uint32_t bw, nblk; };       // comp: of a one-component scan; bw: its blocks per row; nblk: blocks the scan covers

// block sb of the scan's order -> its index in the MCU-ordered coefficient buffer
__device__ __forceinline__ size_t prog_block(const DecShape& g, const ProgScan& sc, int mw, uint32_t sb) {
    if (sc.ncomp == g.c) return sb;
    if (sc.comp > 0) return (size_t)sb * g.bpm + g.H * g.V + sc.comp - 1;
    const uint32_t by = sb / sc.bw, bx = sb - by * sc.bw;
    return ((size_t)(by / g.V) * mw + bx / g.H) * g.bpm + (by % g.V) * g.H + bx % g.H;
}

__device__ __forceinline__ uint32_t prog_bit(const uint32_t* __restrict__ s, uint32_t last_word, uint32_t pos, uint32_t stop) {
    return peek32(s, last_word, pos, stop) >> 31;
}

// a scan's last block ended at pos
__device__ __forceinline__ void prog_last_block(uint32_t pos, uint32_t stop, DecMeta* __restrict__ meta) {
    if (pos <= stop && pos + 8 > stop) atomicAdd(&meta->done, 1u); else meta->err = 1;
}

// One correction bit of an AC refinement for the coefficient at p
__device__ __forceinline__ void prog_correct(int16_t* p, int al) {
    const int v = *p, p1 = 1 << al;
    if ((v & p1) == 0) *p = (int16_t)(v >= 0 ? v + p1 : v - p1);
}

// Decodes a Huffman-coded scan from state st while position < end (and, KIND 2, block < sc.nblk); returns the exit state and counts the
// blocks begun.  KIND 0, DC first: st = (position, block in MCU); 1, AC first: (position, k); 2, AC refine: (position, block, run, k).
// WRITE: b is the scan-order index of the block current at st (KIND 2: st.y is); coefficients of the blocks below sc.nblk go to coef.
template <int KIND, bool WRITE>
__device__ __forceinline__ uint4 prog_span(const uint32_t* __restrict__ s, uint32_t last_word, uint32_t end, uint32_t stop, uint4 st, const FileTables& T_,
                                           const DecShape& g, const ProgScan& sc, int mw, const uint64_t* __restrict__ mask, uint32_t* begun,
                                           int16_t* __restrict__ coef, long long b, DecMeta* __restrict__ meta) {
    uint32_t pos = st.x, nb = 0;
    const int hv = g.H * g.V;
    if (KIND == 0) {
        const uint32_t bpm = sc.ncomp == g.c ? (uint32_t)g.bpm : 1u;
        uint32_t blk = st.y < bpm ? st.y : 0u;
        while (pos < end) {
            const int comp = sc.ncomp == g.c ? (g.c == 3 && (int)blk >= hv ? (int)blk - hv + 1 : 0) : sc.comp;
            const uint32_t bits = peek32(s, last_word, pos, stop);
            const bool live = WRITE && b >= 0 && b < (long long)sc.nblk;
            const uint32_t e = huff_symbol(T_.huff[T_.sel[comp] & 1], bits);
            if (e == 0) {
                pos += 1;
                if (live) meta->err = 1;
                continue;
            }
            const uint32_t len = e >> 8, sym = e & 255, sz = sym & 15;
            const uint32_t v = sz ? (bits << len) >> (32 - sz) : 0u;
            const int value = (sz == 0 || v >= (1u << (sz - 1))) ? (int)v : (int)v - (1 << sz) + 1;
            ++nb;
            pos += len + sz;
            if (live) {
                coef[prog_block(g, sc, mw, (uint32_t)b) * 64] = (int16_t)value;
                if (sym > 11) meta->err = 1;
                if (b == (long long)sc.nblk - 1) prog_last_block(pos, stop, meta);
            }
            blk = blk + 1 == bpm ? 0u : blk + 1;
            ++b;
        }
        *begun = nb;
        return make_uint4(pos, blk, 0u, 0u);
    } else if (KIND == 1) {
        const uint32_t ss = (uint32_t)sc.ss, se = (uint32_t)sc.se;
        uint32_t k = st.y >= ss && st.y <= se ? st.y : ss;
        const HuffTab& tab = T_.huff[2 + (T_.sel[3 + sc.comp] & 1)];
        const long long last = (long long)sc.nblk - 1;
        while (pos < end) {
            const uint32_t bits = peek32(s, last_word, pos, stop);
            const bool live = WRITE && b >= 0 && b <= last;
            const uint32_t e = huff_symbol(tab, bits);
            if (e == 0) {
                pos += 1;
                if (live) meta->err = 1;
                continue;
            }
            if (k == ss) ++nb;
            const uint32_t len = e >> 8, sym = e & 255, r = sym >> 4, sz = sym & 15;
            if (sz == 0 && r < 15) {
                const uint32_t run = (1u << r) + (r ? (bits << len) >> (32 - r) : 0u);      // len + r <= 30
                pos += len + r;
                nb += run - 1;
                if (live && b + (long long)run - 1 >= last) prog_last_block(pos, stop, meta);
                b += run, k = ss;
                continue;
            }
            if (sz == 0) {
                pos += len;
                k += 16;
                if (k > se && live) meta->err = 1;          // the index passed Se
            } else {
                const uint32_t v = (bits << len) >> (32 - sz);
                const int value = v >= (1u << (sz - 1)) ? (int)v : (int)v - (1 << sz) + 1;
                pos += len + sz;
                k += r;
                if (live) {
                    const int val = value * (1 << sc.al);
                    if (k <= se && val >= -32768 && val <= 32767) coef[prog_block(g, sc, mw, (uint32_t)b) * 64 + T.zigzag[k]] = (int16_t)val;
                    if (k > se || sz > 10 || val < -32768 || val > 32767) meta->err = 1;
                }
                k += 1;
            }
            if (k > se) {
                if (live && b == last) prog_last_block(pos, stop, meta);
                k = ss, ++b;
            }
        }
        *begun = nb;
        return make_uint4(pos, k, 0u, 0u);
    } else {
        const uint32_t ss = (uint32_t)sc.ss, se = (uint32_t)sc.se;
        uint32_t blk = min(st.y, sc.nblk), run = st.z & 0x7fffu, k = st.w >= ss && st.w <= se ? st.w : ss;
        const HuffTab& tab = T_.huff[2 + (T_.sel[3 + sc.comp] & 1)];
        while (blk < sc.nblk && (pos < end || (end == stop && run > 0 && pos <= stop))) {         // a run's blocks may take no bit: the stream's last subsequence ends them
            const uint64_t m = mask[blk];
            int16_t* bc = WRITE ? coef + prog_block(g, sc, mw, blk) * 64 : nullptr;
            bool ends = run > 0;                // the block is inside a run: its rest is walked and it ends
            if (!ends) {
                const uint32_t bits = peek32(s, last_word, pos, stop);
                const uint32_t e = huff_symbol(tab, bits);
                if (e == 0) {
                    pos += 1;
                    if (WRITE) meta->err = 1;
                    continue;
                }
                const uint32_t len = e >> 8, sym = e & 255, sz = sym & 15;
                uint32_t r = sym >> 4;
                if (sz == 0 && r < 15) {
                    run = (1u << r) + (r ? (bits << len) >> (32 - r) : 0u);
                    pos += len + r;
                    ends = true;
                } else {
                    pos += len;
                    int put = 0;
                    if (sz) {
                        if (WRITE && sz != 1) meta->err = 1;
                        put = prog_bit(s, last_word, pos, stop) ? (1 << sc.al) : -(1 << sc.al);
                        pos += 1;
                    }
                    while (k <= se) {
                        if ((m >> k) & 1) {
                            if (prog_bit(s, last_word, pos, stop) && WRITE) prog_correct(bc + T.zigzag[k], sc.al);
                            pos += 1;
                        } else {
                            if (r == 0) break;
                            --r;
                        }
                        ++k;
                    }
                    if (WRITE) {
                        if (k > se) meta->err = 1;          // the run passed Se (a ZRL included)
                        else if (put) bc[T.zigzag[k]] = (int16_t)put;
                    }
                    ++k;
                    if (k > se) {
                        ++blk, k = ss;
                        if (WRITE && blk == sc.nblk) prog_last_block(pos, stop, meta);
                    }
                }
            }
            if (ends) {
                for (; k <= se; ++k)
                    if ((m >> k) & 1) {
                        if (prog_bit(s, last_word, pos, stop) && WRITE) prog_correct(bc + T.zigzag[k], sc.al);
                        pos += 1;
                    }
                --run, ++blk, k = ss;
                if (WRITE && blk == sc.nblk) prog_last_block(pos, stop, meta);
            }
        }
        *begun = 0;
        return make_uint4(pos, blk, run, k);
    }
}

// One workgroup per file, one scan: the file decoder's settle stage on the scan's own stream.  Every subsequence enters round 0 from
// (its first bit, 0, 0, 0), which each kind reads as its start-of-block state.
template <int KIND>
__global__ __launch_bounds__(DEC_THREADS) void jpegp_settle_kernel(const uint8_t* __restrict__ blobs, const uint32_t* __restrict__ stream, uint32_t cap_words,
                                                                   DecMeta* __restrict__ meta, uint4* __restrict__ state, uint32_t* __restrict__ count,
                                                                   uint32_t nsub_max, uint32_t chunk_bits, DecShape g, ProgScan sc, int mw, int scan, int nscans,
                                                                   const uint64_t* __restrict__ mask) {
    __shared__ FileTables ft;
    __shared__ uint32_t part[16];
    const size_t f = blockIdx.x, fs = f * nscans + scan;
    load_tables(&ft, blobs + fs * sizeof(FileTables));
    const uint32_t* s = stream + fs * cap_words;
    const uint32_t nbits = min(meta[fs].ulen, (cap_words - 3) * 4) * 8;
    const uint32_t nsub = min((uint32_t)(((uint64_t)nbits + chunk_bits - 1) / chunk_bits), nsub_max);
    const uint64_t* fm = mask + f * g.nblk;
    settle(state + f * 3 * nsub_max, count + f * nsub_max, nsub, nsub_max, true, meta + fs, part,
           [&](uint32_t i) { return DecSpan{i * chunk_bits, (uint32_t)min(i * chunk_bits + chunk_bits, nbits), nbits, i == 0}; },
           [&](const DecSpan& sp, uint4 in, uint32_t* nb) { return prog_span<KIND, false>(s, cap_words - 1, sp.end, sp.stop, in, ft, g, sc, mw, fm, nb, nullptr, 0, nullptr); });
}

template <int KIND>
__global__ __launch_bounds__(256) void jpegp_write_kernel(const uint8_t* __restrict__ blobs, const uint32_t* __restrict__ stream, uint32_t cap_words,
                                                          DecMeta* __restrict__ meta, const uint4* __restrict__ state, const uint32_t* __restrict__ count,
                                                          uint32_t nsub_max, uint32_t chunk_bits, DecShape g, ProgScan sc, int mw, int scan, int nscans,
                                                          const uint64_t* __restrict__ mask, int16_t* __restrict__ coef) {
    __shared__ FileTables ft;
    const size_t f = blockIdx.y, fs = f * nscans + scan;
    load_tables(&ft, blobs + fs * sizeof(FileTables));
    const uint32_t nbits = min(meta[fs].ulen, (cap_words - 3) * 4) * 8;
    const uint32_t nsub = min(meta[fs].nsub, nsub_max);
    const uint32_t i = blockIdx.x * 256 + threadIdx.x;
    if (i >= nsub) return;
    const uint4* exit_state = state + f * 3 * nsub_max;
    const uint32_t begin = i * chunk_bits;
    const uint4 in = i == 0 ? make_uint4(0u, 0u, 0u, 0u) : exit_state[i - 1];
    long long b = (long long)count[f * nsub_max + i];
    if (KIND == 1 && in.y > (uint32_t)sc.ss && in.y <= (uint32_t)sc.se) b -= 1;          // a block under way was begun further left
    uint32_t nb;
    prog_span<KIND, true>(stream + fs * cap_words, cap_words - 1, min(begin + chunk_bits, nbits), nbits, in, ft, g, sc, mw, mask + f * g.nblk, &nb,
                          coef + f * g.nblk * 64, b, meta + fs);
}

// One workgroup per file: the DC differences of a DC-first scan -> (sum per component in scan order) << Al
__global__ __launch_bounds__(DEC_THREADS) void jpegp_dc_kernel(int16_t* __restrict__ coef, DecMeta* __restrict__ meta, DecShape g, ProgScan sc, int mw, int scan, int nscans) {
    __shared__ uint32_t part[16];
    const size_t f = blockIdx.x;
    const int t = threadIdx.x, hv = g.H * g.V;
    int16_t* fc = coef + f * g.nblk * 64;
    const size_t nmcu = g.nblk / g.bpm;
    const bool inter = sc.ncomp == g.c;
    int bad = 0;
    for (int ci = 0; ci < sc.ncomp; ++ci) {
        const int comp = inter ? ci : sc.comp;
        const size_t cnt = inter ? (comp == 0 ? nmcu * hv : nmcu) : (size_t)sc.nblk;
        const size_t per = (cnt + DEC_THREADS - 1) / DEC_THREADS;
        const size_t a = min((size_t)t * per, cnt), e = min(a + per, cnt);
        auto block_of = [&](size_t i) { return inter ? interleaved_block(g, comp, i) : prog_block(g, sc, mw, (uint32_t)i); };
        uint32_t sum = 0;
        for (size_t i = a; i < e; ++i) sum += (uint32_t)(int)fc[block_of(i) * 64];
        uint32_t run = workgroup_inclusive(sum, part) - sum;
        for (size_t i = a; i < e; ++i) {
            run += (uint32_t)(int)fc[block_of(i) * 64];
            const long long v = (long long)(int)run * (1 << sc.al);
            if (v < -32768 || v > 32767) bad = 1;
            fc[block_of(i) * 64] = (int16_t)v;
        }
    }
    if (bad) meta[f * nscans + scan].err = 1;
}

// A DC refinement: bit sb of the stream belongs to block sb of the scan
__global__ __launch_bounds__(256) void jpegp_dcrefine_kernel(const uint32_t* __restrict__ stream, uint32_t cap_words, DecMeta* __restrict__ meta, DecShape g, ProgScan sc,
                                                             int mw, int scan, int nscans, int16_t* __restrict__ coef) {
    const size_t f = blockIdx.y, fs = f * nscans + scan;
    const uint32_t nbits = min(meta[fs].ulen, (cap_words - 3) * 4) * 8;
    const uint32_t sb = blockIdx.x * 256 + threadIdx.x;
    if (sb == 0) {
        meta[fs].settled = 1;
        if (sc.nblk <= nbits && sc.nblk + 8 > nbits) meta[fs].done = 1; else meta[fs].err = 1;
    }
    if (sb >= sc.nblk || sb >= nbits) return;
    if (prog_bit(stream + fs * cap_words, cap_words - 1, sb, nbits)) {
        int16_t* p = coef + (f * g.nblk + prog_block(g, sc, mw, sb)) * 64;
        *p = (int16_t)(*p | (1 << sc.al));
    }
}

// The history of an AC refinement: bit k of mask[sb] is set when the coefficient at zigzag index k of the scan's block sb is not zero
__global__ __launch_bounds__(256) void jpegp_mask_kernel(const int16_t* __restrict__ coef, DecShape g, ProgScan sc, int mw, uint64_t* __restrict__ mask) {
    const size_t f = blockIdx.y;
    const uint32_t sb = blockIdx.x * 256 + threadIdx.x;
    if (sb >= sc.nblk) return;
    const int16_t* bc = coef + (f * g.nblk + prog_block(g, sc, mw, sb)) * 64;
    uint64_t m = 0;
    for (int k = 0; k < 64; ++k) m |= (uint64_t)(bc[T.zigzag[k]] != 0) << k;
    mask[f * g.nblk + sb] = m;
}

// One workgroup per file: the DC bound and the record
__global__ __launch_bounds__(DEC_THREADS) void jpegp_finish_kernel(const int16_t* __restrict__ coef, const DecMeta* __restrict__ meta, DecShape g, int nscans,
                                                                   int32_t* __restrict__ record) {
    __shared__ int range_err;
    const size_t f = blockIdx.x;
    if (threadIdx.x == 0) range_err = 0;
    __syncthreads();
    int bad = 0;
    for (size_t b = threadIdx.x; b < g.nblk; b += DEC_THREADS) {
        const int dc = coef[(f * g.nblk + b) * 64];
        if (dc > 2047 || dc < -2047) bad = 1;
    }
    if (bad) range_err = 1;
    __syncthreads();
    if (threadIdx.x == 0) {
        bool ok = !range_err;
        uint32_t rounds = 0;
        for (int k = 0; k < nscans; ++k) {
            const DecMeta m = meta[f * nscans + k];
            ok = ok && m.settled && !m.err && m.done == 1;
            rounds += m.rounds;
        }
        record[2 * f] = ok ? 0 : 1;
        record[2 * f + 1] = (int32_t)rounds;
    }
}

const char* check_progressive_scans(int c, int nscans, const int32_t* scans) {
    if (nscans < 1 || nscans > PROG_MAX_SCANS) return "nscans outside 1..32";
    for (int k = 0; k < nscans; ++k) {
        const int32_t* d = scans + 8 * k;
        const int ncomp = d[0], ss = d[4], se = d[5], ah = d[6], al = d[7];
        if (ncomp != 1 && ncomp != c) return "a scan with neither one component nor all of them";
        for (int i = 0; i < ncomp; ++i)
            if (d[1 + i] < 0 || d[1 + i] >= c || (ncomp > 1 && d[1 + i] != i)) return "a scan component outside the frame, or an interleaved scan out of frame order";
        if (ss < 0 || se < ss || se > 63) return "a band with Se < Ss or outside 0..63";
        if (ss == 0 && se != 0) return "a scan that mixes the DC term with AC coefficients";
        if (ss > 0 && ncomp != 1) return "an interleaved AC scan";
        if (ah < 0 || ah > 13 || al < 0 || al > 13) return "Ah or Al outside 0..13";
    }
    return nullptr;
}

// What both decoders do between their own argument checks and their first launch: the `streams` segments are held to `files`, the call is
// planned at the longest of them (scans, state_bytes, mask: as make_decode_plan) and its buffers are checked.  who: the entry's name.
int plan_decode(const char* who, size_t files_bytes, int n, int h, int w, int c, int sampling, int restart_interval, int chunk_bits, int scans, size_t state_bytes,
                bool mask, const uint64_t* seg_offsets, const uint32_t* seg_lengths, const int32_t* record, const void* workspace, size_t workspace_bytes, DecPlan* p) {
    size_t longest = 0;
    for (size_t i = 0; i < (size_t)n * scans; ++i) {
        if (seg_offsets[i] > files_bytes || seg_lengths[i] > files_bytes - seg_offsets[i]) {
            set_error("%s: segment %zu (%llu + %u bytes) leaves the %zu bytes of files", who, i, (unsigned long long)seg_offsets[i], seg_lengths[i], files_bytes);
            return ADAIN_EINVAL;
        }
        longest = seg_lengths[i] > longest ? seg_lengths[i] : longest;
    }
    const char* bad = check_decode_shape(n, h, w, c, sampling, restart_interval, longest, chunk_bits);
    if (bad) { set_error("%s: %s", who, bad); return ADAIN_EINVAL; }
    if ((uintptr_t)record % 4) { set_error("%s: the record must be 4-byte aligned", who); return ADAIN_EINVAL; }
    *p = make_decode_plan(n, h, w, c, sampling, restart_interval, longest, chunk_bits, scans, state_bytes, mask);
    return check_workspace(who, workspace, workspace_bytes, p->total, 8);
}

// The front of both decoders: the segment table, the unstuffed streams (`streams` of them; an interval table only where the plan has
// one) and the zero-filled coefficient buffer
int launch_decode_front(const char* who, const DecPlan& p, char* ws, const uint8_t* files, int n, size_t streams, const uint64_t* seg_offsets,
                        const uint32_t* seg_lengths, bool restart, hipStream_t s) {
    DecSeg* seg = (DecSeg*)(ws + p.o_seg);
    DecMeta* meta = (DecMeta*)(ws + p.o_meta);
    for (size_t first = 0; first < streams; first += DEC_SEG_BATCH) {
        DecSegBatch b{};
        const int count = streams - first < (size_t)DEC_SEG_BATCH ? (int)(streams - first) : DEC_SEG_BATCH;
        for (int i = 0; i < count; ++i) b.off[i] = seg_offsets[first + i], b.len[i] = seg_lengths[first + i];
        jpegd_table_kernel<<<1, DEC_SEG_BATCH, 0, s>>>(b, (int)first, count, seg, meta);
    }
    if (restart)
        jpegd_unstuff_kernel<true><<<(unsigned)streams, DEC_THREADS, 0, s>>>(files, seg, meta, (uint8_t*)(ws + p.o_stream), p.cap_words, (uint32_t*)(ws + p.o_itab), p.nint);
    else
        jpegd_unstuff_kernel<false><<<(unsigned)streams, DEC_THREADS, 0, s>>>(files, seg, meta, (uint8_t*)(ws + p.o_stream), p.cap_words, nullptr, p.nint);
    if (hipMemsetAsync(ws + p.o_coef, 0, (size_t)n * p.g.nblk * 64 * sizeof(int16_t), s) != hipSuccess) { set_error("%s: hipMemsetAsync failed", who); return ADAIN_EINVAL; }
    return 0;
}

// The back half of both decoders: coefficients -> planes -> pixels
int launch_decode_back(const char* who, const DecPlan& p, char* ws, const uint8_t* blobs, size_t blob_stride, int n, int h, int w, uint8_t* dst, hipStream_t s) {
    uint8_t* planes = (uint8_t*)(ws + p.o_planes);
    jpegd_idct_kernel<<<dim3((unsigned)((p.g.nblk + IDCT_PER_WG - 1) / IDCT_PER_WG), n), IDCT_PER_WG * 8, 0, s>>>((const int16_t*)(ws + p.o_coef), blobs, blob_stride, planes, p.g);
    const dim3 grid((w + 255) / 256, h, n);
    if (p.g.c == 3)
        jpegd_pixels_kernel<3><<<grid, 256, 0, s>>>(planes, p.g, h, w, dst);
    else
        jpegd_pixels_kernel<1><<<grid, 256, 0, s>>>(planes, p.g, h, w, dst);
    return check_launch(who);
}

}  // namespace

int jpeg_decode_bytes(int n, int h, int w, int c, int sampling, int restart_interval, size_t max_segment_bytes, int chunk_bits, size_t* workspace_bytes) {
    const char* bad = check_decode_shape(n, h, w, c, sampling, restart_interval, max_segment_bytes, chunk_bits);
    if (bad) {
        set_error("jpeg_decode_u8: %s (n %d, %d x %d x %d, sampling %d, restart_interval %d, segment %zu, chunk_bits %d)", bad, n, h, w, c, sampling, restart_interval,
                  max_segment_bytes, chunk_bits);
        return ADAIN_EINVAL;
    }
    if (workspace_bytes) *workspace_bytes = make_decode_plan(n, h, w, c, sampling, restart_interval, max_segment_bytes, chunk_bits, 1, sizeof(uint2), false).total;
    return 0;
}

int launch_jpeg_decode_u8(const uint8_t* files, size_t files_bytes, const uint8_t* blobs, int n, int h, int w, int c, int sampling, int restart_interval,
                          const uint64_t* seg_offsets, const uint32_t* seg_lengths, uint8_t* dst, int32_t* record, void* workspace, size_t workspace_bytes,
                          int chunk_bits, hipStream_t s) {
    const char* who = "jpeg_decode_u8";
    const char* bad = check_decode_shape(n, h, w, c, sampling, restart_interval, 0, chunk_bits);
    if (bad) {
        set_error("jpeg_decode_u8: %s (n %d, %d x %d x %d, sampling %d, restart_interval %d, chunk_bits %d)", bad, n, h, w, c, sampling, restart_interval, chunk_bits);
        return ADAIN_EINVAL;
    }
    DecPlan p{};
    if (plan_decode(who, files_bytes, n, h, w, c, sampling, restart_interval, chunk_bits, 1, sizeof(uint2), false, seg_offsets, seg_lengths, record, workspace,
                    workspace_bytes, &p))
        return ADAIN_EINVAL;
    if ((p.g.nblk + IDCT_PER_WG - 1) / IDCT_PER_WG > 0x7fffffffull) { set_error("jpeg_decode_u8: %d x %d: too many blocks for one launch", h, w); return ADAIN_EINVAL; }
    char* ws = (char*)workspace;
    DecMeta* meta = (DecMeta*)(ws + p.o_meta);
    const uint32_t* stream = (const uint32_t*)(ws + p.o_stream);
    uint2* state = (uint2*)(ws + p.o_state);
    uint32_t* count = (uint32_t*)(ws + p.o_count);
    int16_t* coef = (int16_t*)(ws + p.o_coef);
    uint32_t* itab = restart_interval ? (uint32_t*)(ws + p.o_itab) : nullptr;
    const DecShape g{p.g.H, p.g.V, p.g.bpm, p.g.c, p.g.nblk, p.ri, p.nint};
    if (launch_decode_front(who, p, ws, files, n, (size_t)n, seg_offsets, seg_lengths, restart_interval != 0, s)) return ADAIN_EINVAL;
    jpegd_settle_kernel<<<n, DEC_THREADS, 0, s>>>(blobs, stream, p.cap_words, meta, state, count, p.nsub_max, p.chunk_bits, g, itab);
    jpegd_write_kernel<<<dim3((p.nsub_max + 255) / 256, n), 256, 0, s>>>(blobs, stream, p.cap_words, meta, state, count, p.nsub_max, p.chunk_bits, g, coef, itab);
    jpegd_dc_kernel<<<n, DEC_THREADS, 0, s>>>(coef, meta, g, record);
    return launch_decode_back(who, p, ws, blobs, sizeof(FileTables), n, h, w, dst, s);
}

int jpeg_decode_progressive_bytes(int n, int h, int w, int c, int sampling, int nscans, size_t max_segment_bytes, int chunk_bits, size_t* workspace_bytes) {
    const char* bad = check_decode_shape(n, h, w, c, sampling, 0, max_segment_bytes, chunk_bits);
    if (!bad && (nscans < 1 || nscans > PROG_MAX_SCANS)) bad = "nscans outside 1..32";
    if (bad) {
        set_error("jpeg_decode_progressive_u8: %s (n %d, %d x %d x %d, sampling %d, %d scans, segment %zu, chunk_bits %d)", bad, n, h, w, c, sampling, nscans,
                  max_segment_bytes, chunk_bits);
        return ADAIN_EINVAL;
    }
    if (workspace_bytes) *workspace_bytes = make_decode_plan(n, h, w, c, sampling, 0, max_segment_bytes, chunk_bits, nscans, sizeof(uint4), true).total;
    return 0;
}

int launch_jpeg_decode_progressive_u8(const uint8_t* files, size_t files_bytes, const uint8_t* blobs, int n, int h, int w, int c, int sampling, int nscans,
                                      const int32_t* scans, const uint64_t* seg_offsets, const uint32_t* seg_lengths, uint8_t* dst, int32_t* record, void* workspace,
                                      size_t workspace_bytes, int chunk_bits, hipStream_t s) {
    const char* who = "jpeg_decode_progressive_u8";
    const char* bad = check_decode_shape(n, h, w, c, sampling, 0, 0, chunk_bits);
    if (!bad) bad = check_progressive_scans(c, nscans, scans);
    if (bad) {
        set_error("jpeg_decode_progressive_u8: %s (n %d, %d x %d x %d, sampling %d, %d scans, chunk_bits %d)", bad, n, h, w, c, sampling, nscans, chunk_bits);
        return ADAIN_EINVAL;
    }
    const size_t streams = (size_t)n * nscans;
    DecPlan p{};
    if (plan_decode(who, files_bytes, n, h, w, c, sampling, 0, chunk_bits, nscans, sizeof(uint4), true, seg_offsets, seg_lengths, record, workspace, workspace_bytes, &p))
        return ADAIN_EINVAL;
    const DecPlanes& pg = p.g;
    if ((pg.nblk + IDCT_PER_WG - 1) / IDCT_PER_WG > 0x7fffffffull || streams > 0x7fffffffull) {
        set_error("jpeg_decode_progressive_u8: %d x %d, %d files: too many blocks or streams for one launch", h, w, n);
        return ADAIN_EINVAL;
    }
    char* ws = (char*)workspace;
    DecMeta* meta = (DecMeta*)(ws + p.o_meta);
    const uint32_t* stream = (const uint32_t*)(ws + p.o_stream);
    uint4* state = (uint4*)(ws + p.o_state);
    uint32_t* count = (uint32_t*)(ws + p.o_count);
    uint64_t* mask = (uint64_t*)(ws + p.o_mask);
    int16_t* coef = (int16_t*)(ws + p.o_coef);
    const DecShape g{pg.H, pg.V, pg.bpm, pg.c, pg.nblk, p.ri, p.nint};
    if (launch_decode_front(who, p, ws, files, n, streams, seg_offsets, seg_lengths, false, s)) return ADAIN_EINVAL;
    const dim3 subs((p.nsub_max + 255) / 256, n);
    for (int k = 0; k < nscans; ++k) {
        const int32_t* d = scans + 8 * k;
        ProgScan sc{d[0], d[0] == 1 ? d[1] : 0, d[4], d[5], d[6], d[7], 0u, 0u};
        if (sc.ncomp == c) {
            sc.bw = (uint32_t)pg.mw * (c == 1 ? 1u : (uint32_t)pg.H), sc.nblk = (uint32_t)pg.nblk;
        } else {
            const uint32_t cw = sc.comp == 0 ? (uint32_t)w : (uint32_t)((w + pg.H - 1) / pg.H), chh = sc.comp == 0 ? (uint32_t)h : (uint32_t)((h + pg.V - 1) / pg.V);
            sc.bw = (cw + 7) / 8, sc.nblk = sc.bw * ((chh + 7) / 8);
        }
        const dim3 blocks((sc.nblk + 255) / 256, n);
#define JPEGP_SETTLE(KIND)                                                                                                                                      \
    jpegp_settle_kernel<KIND><<<n, DEC_THREADS, 0, s>>>(blobs, stream, p.cap_words, meta, state, count, p.nsub_max, p.chunk_bits, g, sc, pg.mw, k, nscans, mask); \
    jpegp_write_kernel<KIND><<<subs, 256, 0, s>>>(blobs, stream, p.cap_words, meta, state, count, p.nsub_max, p.chunk_bits, g, sc, pg.mw, k, nscans, mask, coef)
        if (sc.ss == 0 && sc.ah == 0) {
            JPEGP_SETTLE(0);
            jpegp_dc_kernel<<<n, DEC_THREADS, 0, s>>>(coef, meta, g, sc, pg.mw, k, nscans);
        } else if (sc.ss == 0) {
            jpegp_dcrefine_kernel<<<blocks, 256, 0, s>>>(stream, p.cap_words, meta, g, sc, pg.mw, k, nscans, coef);
        } else if (sc.ah == 0) {
            JPEGP_SETTLE(1);
        } else {
            jpegp_mask_kernel<<<blocks, 256, 0, s>>>(coef, g, sc, pg.mw, mask);
            JPEGP_SETTLE(2);
        }
#undef JPEGP_SETTLE
    }
    jpegp_finish_kernel<<<n, DEC_THREADS, 0, s>>>(coef, meta, g, nscans, record);
    return launch_decode_back(who, p, ws, blobs, (size_t)nscans * sizeof(FileTables), n, h, w, dst, s);
}

}  // namespace adain
