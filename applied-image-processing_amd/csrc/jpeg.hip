// Baseline JPEG encoder on the device: the file Pillow's default Image.save(f, format="JPEG") writes, byte for byte (libjpeg's
// integer "islow" DCT, h2v2 chroma, the Annex K quantisation tables scaled by the quality, the Annex K Huffman tables, a JFIF 1.01
// header).  All arithmetic is int32 / uint64; no floating point; a frame's bytes do not depend on the batch it is in.
// tests/jpeg_ref.py restates the same rules in NumPy and tests/test_jpeg_host.py holds that restatement to Pillow on the host.
//
// The rules
//   header   FFD8; APP0 "JFIF\0" 1.01, units 0, density 1 x 1, no thumbnail; one DQT per table (8 bit, zigzag order; 0 luma, 1 chroma);
//            SOF0 (precision 8, h, w, components (1, 0x22, 0) (2, 0x11, 1) (3, 0x11, 1)); DHT DC0, AC0, DC1, AC1; SOS (1, 0x00)
//            (2, 0x11) (3, 0x11), Ss 0, Se 63, Ah/Al 0.  No DRI.  623 bytes for RGB.  Greyscale: one DQT, component (1, 0x11, 0), DHT
//            DC0 and AC0, a one-component SOS: 328 bytes.
//   tables   q = clamp((base * s + 50) / 100, 1, 255) with s = 5000 / quality below 50 and 200 - 2 quality from 50 up.
//   colour   Y = (19595 R + 38470 G + 7471 B + 32768) >> 16; Cb = (-11059 R - 21709 G + 32768 B + (128 << 16) + 32767) >> 16;
//            Cr = (32768 R - 27439 G - 5329 B + (128 << 16) + 32767) >> 16.
//   padding  luma: edge replication to whole 8 x 8 blocks.  Chroma: the full-resolution planes are replicated to whole MCU columns and
//            to an EVEN number of rows only, downsampled as (a + b + c + d + bias) >> 2 with bias 1 on even output columns and 2 on odd
//            ones, and the downsampled rows are then replicated to whole blocks (replicating full-resolution rows further down and
//            downsampling those gives other bottom rows when the height is even).
//   dummies  the luma blocks of an MCU that lie outside the ceil(h/8) x ceil(w/8) block grid: all AC zero, the DC of the block before
//            them in the MCU, so their DC difference is 0.
//   DCT      jfdctint: CONST_BITS 13, PASS1_BITS 2, rows then columns, output scaled by 8.
//   quantise sign(c) * ((|c| + (8q >> 1)) / (8q)).
//   entropy  scan order Y00 Y01 Y10 Y11 Cb Cr per 16 x 16 MCU (greyscale: the blocks row-major); DC prediction per component over the
//            whole scan; category = bit_length(|v|); a negative value puts v - 1 in the low bits; runs above 15 emit ZRL (0xF0);
//            trailing zeros emit EOB; the last byte is padded with 1-bits; a 0x00 follows every 0xFF.
//
// The stages (8 launches per call, every one over all n frames)
//   transform  one workgroup per 8 MCUs (greyscale: 32 blocks): the strip goes through LDS with coalesced byte loads, colour conversion
//              and chroma downsample into per-block planes, the two DCT passes with one lane per row / column, quantisation, and the
//              zigzag-ordered int16 coefficients leave as one contiguous store
//   count      one wave64 per block, one lane per coefficient: __ballot gives the non-zero mask, the runs come from bit operations
//   emit       the same kernel behind the back half's scan and zero: each lane ORs its ZRLs, code and value bits into the big-endian bit
//              stream at block offset + in-block prefix; the bits of different lanes are disjoint, so atomicOr on 32-bit words is
//              order-independent
//   the back half ("the back half of every file"): scan, zero, ffcount, scan and the scatter's stuffed copy - from the blocks' bit counts to
//              the bytes behind the header - are written once for the one entropy-coded segment of this file and the scans of a
//              progressive one; the scatter also writes the header, FFD9 and lengths[i]
//
// The options (adain_jpeg_encode_opt_u8): Pillow's save with subsampling = 0 / 1 / 2 and optimize = False / True; (2, False) is the file
// above in the launches above.  tests/jpeg_options_ref.py restates the rules, tests/test_jpeg_options_host.py holds that to Pillow.
//   4:4:4    8 x 8 MCUs, blocks Y Cb Cr, SOF0 luma sampling 0x11; the chroma planes are edge-replicated to whole blocks, not downsampled
//   4:2:2    16 x 8 MCUs, blocks Y0 Y1 Cb Cr, 0x21; the full-resolution chroma columns are replicated to whole MCUs and downsampled as
//            (a + b + bias) >> 1 with bias 0 on even output columns and 1 on odd ones, the rows replicated to whole blocks; a luma
//            block beyond ceil(w/8) is a dummy as above
//   grey     ignores the subsampling: the file is the one Pillow writes for an L image without the keyword
//   optimize libjpeg's two-pass optimize_coding - the rule list stands in front of its kernels ("optimised tables"): the histogram and
//            table stages run between transform and count (10 launches and a memset), count and emit read the frame's own tables
//            from the workspace, and scatter writes a per-frame header with four (grey: two) DHT segments of only the symbols that occur
//
// Progressive files (adain_jpeg_encode_progressive_u8): Pillow's save with progressive = True, the same coefficients in libjpeg's simple
// progression; the rules and the stages stand in front of its kernels ("progressive files").
//
// The round trip (adain_jpeg_roundtrip_u8): the pixels Pillow decodes from that file, byte for byte, without the file.  Entropy coding is
// lossless, so they are a function of the quantised coefficients the transform stage leaves in the workspace; what follows it is the
// back half of libjpeg's decoder.  tests/jpeg_decode_ref.py restates it in NumPy, tests/test_jpeg_roundtrip_host.py holds that to Pillow.
//
// Its rules
//   dequantise  coef * q, the q of `tables` above, natural order.
//   IDCT        jidctint's jpeg_idct_islow: CONST_BITS 13, PASS1_BITS 2, COLUMNS then rows (the mirror of the encoder).  Per pass on d0..d7:
//               z1 = (d2 + d6) * 4433, tmp2 = z1 - d6 * 15137, tmp3 = z1 + d2 * 6270; tmp0 = (d0 + d4) << 13, tmp1 = (d0 - d4) << 13;
//               tmp10 = tmp0 + tmp3, tmp13 = tmp0 - tmp3, tmp11 = tmp1 + tmp2, tmp12 = tmp1 - tmp2; odd part from t0 = d7, t1 = d5, t2 = d3,
//               t3 = d1: z1 = t0 + t3, z2 = t1 + t2, z3 = t0 + t2, z4 = t1 + t3, z5 = (z3 + z4) * 9633; t0 *= 2446, t1 *= 16819, t2 *= 25172,
//               t3 *= 12299; z1 *= -7373, z2 *= -20995, z3 = z3 * -16069 + z5, z4 = z4 * -3196 + z5; t0 += z1 + z3, t1 += z2 + z4,
//               t2 += z2 + z3, t3 += z1 + z4.  Outputs 0..7: tmp10 + t3, tmp11 + t2, tmp12 + t1, tmp13 + t0, tmp13 - t0, tmp12 - t1,
//               tmp11 - t2, tmp10 - t3, each descaled as (x + (1 << (n - 1))) >> n with n = 11 in the column pass and 18 in the row pass.
//               The sample is range_limit[x & 0x3FF], libjpeg's table centred on 128: x + 128 clamped to 0..255 for x in -512..511,
//               wrapping beyond as the 1024-entry table does.
//   luma        the padded block grid cropped to h x w.  Greyscale: that plane is the output.
//   chroma      the planes are cropped to ch = ceil(h/2) rows and cw = ceil(w/2) columns BEFORE upsampling: context beyond the first and
//               last real row is that row replicated, the encoder's block padding is not used.  cw > 2: h2v2_fancy_upsample - for output
//               row 2r + v, s[c] = 3 C[r][c] + C[r - 1 if v == 0 else r + 1][c] (row clamped to 0..ch-1), out[2c] = (3 s[c] + s[c-1] + 8)
//               >> 4, out[2c+1] = (3 s[c] + s[c+1] + 7) >> 4, and at the ends out[0] = (4 s[0] + 8) >> 4, out[2cw-1] = (4 s[cw-1] + 7) >> 4
//               (the column clamped to 0..cw-1 says the same).  cw <= 2 (w <= 4): libjpeg leaves the fancy filter out and every chroma
//               sample is replicated 2 x 2.
//   colour      with cb, cr minus 128: R = Y + ((91881 cr + 32768) >> 16), G = Y + ((-22554 cb - 46802 cr + 32768) >> 16),
//               B = Y + ((116130 cb + 32768) >> 16); arithmetic shifts; each channel clamped to 0..255.
//
// Its stages (3 launches per call, every one over all n frames)
//   transform  the encoder's, unchanged
//   idct       8 lanes per block: the zigzag int16 coefficients are dequantised into LDS in natural order, a lane per column, then a lane per
//              row, and each lane stores its 8 samples as one 8-byte word into padded uint8 Y / Cb / Cr planes in the workspace
//   merge      one workgroup per 512 pixels of an output row, a lane per chroma column (two pixels): upsampling and colour conversion into an
//              LDS image of the row segment laid out at the destination's byte phase, which leaves as aligned dwords with byte stores at
//              its two ends only - any destination address and any 3 w row stride
//
// The file decoders (adain_jpeg_decode_u8, adain_jpeg_decode_restart_u8, adain_jpeg_decode_progressive_u8) are in jpeg_decode.hip; what
// they share with the round trip - the tables, the IDCT with its plane geometry, the colour arithmetic - is in jpeg_common.h.
#include "jpeg_common.h"

namespace adain {
namespace {

constexpr int MCUS_PER_WG = 8;          // RGB: 8 MCUs = 128 x 16 pixels = 48 blocks, 384 threads (one per block row)
constexpr int GREY_PER_WG = 32;         // L: 32 blocks = 256 x 8 pixels, 256 threads
constexpr int CHUNK = 1024;             // bytes of entropy-coded data per workgroup pass of the stuffing kernels (one word per thread)
constexpr int SCAN_THREADS = 1024;
constexpr int STREAM_GRID = 64;         // workgroups per frame of the grid-stride kernels (zero, ffcount, scatter)
constexpr int PSCANS = 10;              // scans of a colour progressive file; grey has 6

// ---- sizes -----------------------------------------------------------------------------------------------------------------------------
// A frame's entropy-coded segments, which the back half of every file walks: a baseline file has one, a progressive file one per scan.
// A segment's "entries" are the blocks it codes; its bits are scanned per entry, its stream is stuffed per CHUNK.  Passed by value.
struct Segment {
    size_t entry0, word0, chunk0;       // its first entry, stream word and stuffing chunk among the frame's
    uint32_t nentries;
};
struct Segments {
    int count;
    int totals;                                 // total_bits and fftotal hold this many per frame: [frame][totals]
    size_t entries, stream_words, chunks;       // per frame, of all its segments
    Segment s[PSCANS];
    // appends a segment of nblk blocks and at most max_bytes entropy-coded bytes before stuffing
    void add(size_t nblk, size_t max_bytes) {
        s[count++] = Segment{entries, stream_words, chunks, (uint32_t)nblk};
        entries += nblk;
        stream_words += (max_bytes + 3) / 4 + 4;
        chunks += (max_bytes + CHUNK - 1) / CHUNK;
    }
};

// A frame's own Huffman code of one table slot (DC0, AC0, DC1, AC1), built on the device for optimize = 1: what count and emit read in
// place of T.huff, and the slot's DHT payload for the header.
struct HuffSlot {
    uint16_t code[256];
    uint8_t len[256];        // 0: the symbol does not occur
    uint8_t bits[16];        // codes per length 1..16
    uint8_t vals[256];       // the first nvals: the symbols by code length, then by value
    uint32_t nvals;
};
constexpr int SLOTS = 4;                                    // per frame in the workspace, whatever c
constexpr int OPT_BLOCK_BITS = (16 + 11) + 63 * (16 + 10);  // every code of an optimal table may be 16 bits long
constexpr int HIST_GRID = 128;                              // workgroups per frame of the histogram stage

struct Plan {
    int c, hs, vs, mw, mh, bw, bh;      // hs x vs: luma blocks per MCU (RGB); mw x mh: MCUs
    size_t nblk;                  // blocks per frame in scan order, dummy blocks included
    size_t max_bytes;             // entropy-coded bytes of a frame before stuffing, at most
    Segments seg;                 // the one segment of the file
    size_t out_stride;
    size_t o_coef, o_bits, o_off, o_total, o_stream, o_ffcnt, o_ffoff, o_fftotal, total;      // workspace offsets (bytes) of the n-frame arrays
    size_t o_hist, o_huff;              // optimize only: uint64 [n][SLOTS][256] symbol counts, HuffSlot [n][SLOTS]
};

// sampling: 0 (4:4:4), 1 (4:2:2), 2 (4:2:0); greyscale has no MCUs and is planned as 2: (2, false) is the default file's plan
Plan make_plan(int n, int h, int w, int c, int sampling = 2, bool optimize = false) {
    Plan p{};
    p.c = c;
    p.hs = c == 3 && sampling == 0 ? 1 : 2, p.vs = c == 3 && sampling != 2 ? 1 : 2;
    p.bw = (w + 7) / 8, p.bh = (h + 7) / 8;
    p.mw = (w + 8 * p.hs - 1) / (8 * p.hs), p.mh = (h + 8 * p.vs - 1) / (8 * p.vs);
    p.nblk = c == 3 ? (size_t)p.mw * p.mh * (p.hs * p.vs + 2) : (size_t)p.bw * p.bh;
    p.max_bytes = (p.nblk * (optimize ? OPT_BLOCK_BITS : HOST_T.max_block_bits) + 7) / 8;
    p.seg.totals = 1;
    p.seg.add(p.nblk, p.max_bytes);
    p.out_stride = HOST_T.hdr_len[c == 3] + 2 * p.max_bytes + 2;
    const size_t N = (size_t)n;
    Carve ws;
    p.o_coef = ws.take(N * p.nblk * 64 * sizeof(int16_t));
    p.o_bits = ws.take(N * p.nblk * sizeof(uint32_t));
    p.o_off = ws.take(N * p.nblk * sizeof(uint64_t));
    p.o_total = ws.take(N * sizeof(uint64_t));
    p.o_stream = ws.take(N * p.seg.stream_words * sizeof(uint32_t));
    p.o_ffcnt = ws.take(N * p.seg.chunks * sizeof(uint32_t));
    p.o_ffoff = ws.take(N * p.seg.chunks * sizeof(uint32_t));
    p.o_fftotal = ws.take(N * sizeof(uint32_t));
    if (optimize) {
        p.o_hist = ws.take(N * SLOTS * 256 * sizeof(uint64_t));
        p.o_huff = ws.take(N * SLOTS * sizeof(HuffSlot));
    }
    p.total = ws.at;
    return p;
}

// ---- transform -------------------------------------------------------------------------------------------------------------------------
// One pass of jfdctint over 8 values p[0], p[S], ...: the first pass keeps PASS1_BITS of extra precision, the second removes them.
template <int S, bool FIRST>
__device__ __forceinline__ void fdct_pass(int* p) {
    constexpr int N = FIRST ? 11 : 15, R = 1 << (N - 1);
    const int d0 = p[0], d1 = p[S], d2 = p[2 * S], d3 = p[3 * S], d4 = p[4 * S], d5 = p[5 * S], d6 = p[6 * S], d7 = p[7 * S];
    int t0 = d0 + d7, t7 = d0 - d7, t1 = d1 + d6, t6 = d1 - d6, t2 = d2 + d5, t5 = d2 - d5, t3 = d3 + d4, t4 = d3 - d4;
    const int t10 = t0 + t3, t13 = t0 - t3, t11 = t1 + t2, t12 = t1 - t2;
    if (FIRST) {
        p[0] = (t10 + t11) * 4;
        p[4 * S] = (t10 - t11) * 4;
    } else {
        p[0] = (t10 + t11 + 2) >> 2;
        p[4 * S] = (t10 - t11 + 2) >> 2;
    }
    int z1 = (t12 + t13) * 4433;
    p[2 * S] = (z1 + t13 * 6270 + R) >> N;
    p[6 * S] = (z1 - t12 * 15137 + R) >> N;
    z1 = t4 + t7;
    int z2 = t5 + t6, z3 = t4 + t6, z4 = t5 + t7;
    const int z5 = (z3 + z4) * 9633;
    t4 *= 2446, t5 *= 16819, t6 *= 25172, t7 *= 12299;
    z1 *= -7373, z2 *= -20995;
    z3 = z3 * -16069 + z5, z4 = z4 * -3196 + z5;
    p[7 * S] = (t4 + z1 + z3 + R) >> N;
    p[5 * S] = (t5 + z2 + z4 + R) >> N;
    p[3 * S] = (t6 + z2 + z3 + R) >> N;
    p[S] = (t7 + z1 + z4 + R) >> N;
}

__device__ __forceinline__ int quant_entry(int table, int natural, int quality) {
    const int s = quality < 50 ? 5000 / quality : 200 - 2 * quality;
    const int q = (T.qbase[table][natural] * s + 50) / 100;
    return q < 1 ? 1 : q > 255 ? 255 : q;
}

// The DCT, quantisation and store shared by both layouts.  samp: NB blocks of level-shifted samples, 8 rows of 9 ints (72 per block: a
// lane per row, then a lane per column, both free of bank conflicts); q8: 8 q of both tables in natural order; zq: NB x 64 int16.
// Block j of the workgroup uses table table_of(j) and is all zero when dummy_of(j); the first `count` blocks go to dst.
template <int NB, class TableOf, class DummyOf>
__device__ __forceinline__ void dct_quantise_store(int* samp, const int* q8, int16_t* zq, int16_t* dst, int count, TableOf table_of, DummyOf dummy_of) {
    const int t = threadIdx.x, blk = t >> 3, k = t & 7;
    if (blk < NB) fdct_pass<1, true>(samp + blk * 72 + k * 9);
    __syncthreads();
    if (blk < NB) {
        int* p = samp + blk * 72 + k;
        fdct_pass<9, false>(p);
        const int* q = q8 + table_of(blk) * 64;
        const bool dummy = dummy_of(blk);
#pragma unroll
        for (int r = 0; r < 8; ++r) {
            const int v = p[r * 9], d = q[r * 8 + k];
            const int m = (int)(((unsigned)(v < 0 ? -v : v) + (unsigned)(d >> 1)) / (unsigned)d);
            zq[blk * 64 + T.zpos[r * 8 + k]] = dummy ? (int16_t)0 : (int16_t)(v < 0 ? -m : m);
        }
    }
    __syncthreads();
    uint32_t* d32 = (uint32_t*)dst;               // block starts are 128-byte aligned in the workspace
    const uint32_t* s32 = (const uint32_t*)zq;
    for (int i = t; i < count * 32; i += blockDim.x) d32[i] = s32[i];
}

__global__ __launch_bounds__(MCUS_PER_WG * 48) void jpeg_transform_rgb_kernel(const uint8_t* __restrict__ src, int h, int w, int quality, int16_t* __restrict__ coef,
                                                                              int mw, int bw, int bh, size_t nblk) {
    constexpr int NB = MCUS_PER_WG * 6, PX = MCUS_PER_WG * 16, THREADS = MCUS_PER_WG * 48;
    __shared__ uint8_t raw[16 * PX * 3];
    __shared__ int samp[NB * 72];
    __shared__ int q8[128];
    __shared__ __attribute__((aligned(16))) int16_t zq[NB * 64];
    const int t = threadIdx.x, my = blockIdx.y, mx0 = blockIdx.x * MCUS_PER_WG;
    const uint8_t* img = src + (size_t)blockIdx.z * h * w * 3;
    if (t < 128) q8[t] = 8 * quant_entry(t >> 6, t & 63, quality);
    for (int i = t; i < 16 * PX * 3; i += THREADS) {
        const int r = i / (PX * 3), j = i - r * (PX * 3), px = j / 3, ch = j - px * 3;
        const int gy = min(my * 16 + r, h - 1), gx = min(mx0 * 16 + px, w - 1);
        raw[i] = img[((size_t)gy * w + gx) * 3 + ch];
    }
    __syncthreads();
    const int ch2 = (h + 1) >> 1;
    for (int i = t; i < 16 * PX + 2 * 8 * (PX / 2); i += THREADS) {
        if (i < 16 * PX) {
            const int r = i / PX, c = i - r * PX;
            const uint8_t* p = raw + r * (PX * 3) + c * 3;
            const int y = (19595 * p[0] + 38470 * p[1] + 7471 * p[2] + 32768) >> 16;
            samp[((c >> 4) * 6 + ((r >> 3) << 1) + ((c >> 3) & 1)) * 72 + (r & 7) * 9 + (c & 7)] = y - 128;
        } else {
            const int j = i - 16 * PX, comp = j / (8 * (PX / 2)), jj = j - comp * (8 * (PX / 2)), crow = jj / (PX / 2), cc = jj - crow * (PX / 2);
            const int lr = min(my * 8 + crow, ch2 - 1) - my * 8;          // the downsampled ROW is what is replicated below the image
            int sum = 1 + (cc & 1);
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const uint8_t* p = raw + (2 * lr + (k >> 1)) * (PX * 3) + (2 * cc + (k & 1)) * 3;
                sum += comp == 0 ? (-11059 * p[0] - 21709 * p[1] + 32768 * p[2] + (128 << 16) + 32767) >> 16
                                 : (32768 * p[0] - 27439 * p[1] - 5329 * p[2] + (128 << 16) + 32767) >> 16;
            }
            samp[((cc >> 3) * 6 + 4 + comp) * 72 + crow * 9 + (cc & 7)] = (sum >> 2) - 128;
        }
    }
    __syncthreads();
    const int count = min(MCUS_PER_WG, mw - mx0) * 6;
    int16_t* dst = coef + ((size_t)blockIdx.z * nblk + ((size_t)my * mw + mx0) * 6) * 64;
    dct_quantise_store<NB>(samp, q8, zq, dst, count, [](int j) { return j % 6 >= 4 ? 1 : 0; },
                           [&](int j) { const int m = j / 6, k = j - m * 6; return k < 4 && !(2 * (mx0 + m) + (k & 1) < bw && 2 * my + (k >> 1) < bh); });
}

// 4:4:4 (HS = 1: 8 x 8 MCUs, blocks Y Cb Cr) and 4:2:2 (HS = 2: 16 x 8 MCUs, blocks Y0 Y1 Cb Cr): one workgroup per 128 x 8 pixel strip.
// Chroma: the full-resolution planes are edge-replicated to whole MCUs; 4:2:2 then averages column pairs as (a + b + bias) >> 1 with bias
// 0 on even output columns and 1 on odd ones.  The second luma block of a 4:2:2 MCU beyond ceil(w/8) is a dummy.
template <int HS>
__global__ __launch_bounds__((128 / (8 * HS)) * (HS + 2) * 8) void jpeg_transform_rgb_h_kernel(const uint8_t* __restrict__ src, int h, int w, int quality,
                                                                                               int16_t* __restrict__ coef, int mw, int bw, size_t nblk) {
    constexpr int PX = 128, BPM = HS + 2, MCUS = PX / (8 * HS), NB = MCUS * BPM, THREADS = NB * 8, CW = PX / HS;
    __shared__ uint8_t raw[8 * PX * 3];
    __shared__ int samp[NB * 72];
    __shared__ int q8[128];
    __shared__ __attribute__((aligned(16))) int16_t zq[NB * 64];
    const int t = threadIdx.x, my = blockIdx.y, mx0 = blockIdx.x * MCUS;
    const uint8_t* img = src + (size_t)blockIdx.z * h * w * 3;
    if (t < 128) q8[t] = 8 * quant_entry(t >> 6, t & 63, quality);
    for (int i = t; i < 8 * PX * 3; i += THREADS) {
        const int r = i / (PX * 3), j = i - r * (PX * 3), px = j / 3, ch = j - px * 3;
        const int gy = min(my * 8 + r, h - 1), gx = min(mx0 * 8 * HS + px, w - 1);
        raw[i] = img[((size_t)gy * w + gx) * 3 + ch];
    }
    __syncthreads();
    for (int i = t; i < 8 * PX + 2 * 8 * CW; i += THREADS) {
        if (i < 8 * PX) {
            const int r = i / PX, c = i - r * PX;
            const uint8_t* p = raw + r * (PX * 3) + c * 3;
            const int y = (19595 * p[0] + 38470 * p[1] + 7471 * p[2] + 32768) >> 16;
            samp[((c / (8 * HS)) * BPM + ((c >> 3) & (HS - 1))) * 72 + r * 9 + (c & 7)] = y - 128;
        } else {
            const int j = i - 8 * PX, comp = j / (8 * CW), jj = j - comp * (8 * CW), crow = jj / CW, cc = jj - crow * CW;
            int sum = HS == 2 ? (cc & 1) : 0;
#pragma unroll
            for (int k = 0; k < HS; ++k) {
                const uint8_t* p = raw + crow * (PX * 3) + (HS * cc + k) * 3;
                sum += comp == 0 ? (-11059 * p[0] - 21709 * p[1] + 32768 * p[2] + (128 << 16) + 32767) >> 16
                                 : (32768 * p[0] - 27439 * p[1] - 5329 * p[2] + (128 << 16) + 32767) >> 16;
            }
            samp[((cc >> 3) * BPM + HS + comp) * 72 + crow * 9 + (cc & 7)] = (sum >> (HS - 1)) - 128;
        }
    }
    __syncthreads();
    const int count = min(MCUS, mw - mx0) * BPM;
    int16_t* dst = coef + ((size_t)blockIdx.z * nblk + ((size_t)my * mw + mx0) * BPM) * 64;
    dct_quantise_store<NB>(samp, q8, zq, dst, count, [](int j) { return j % BPM >= HS ? 1 : 0; },
                           [&](int j) { const int m = j / BPM, k = j - m * BPM; return k < HS && !(HS * (mx0 + m) + k < bw); });
}

__global__ __launch_bounds__(GREY_PER_WG * 8) void jpeg_transform_grey_kernel(const uint8_t* __restrict__ src, int h, int w, int quality, int16_t* __restrict__ coef,
                                                                              int bw, size_t nblk) {
    constexpr int NB = GREY_PER_WG, PX = NB * 8, THREADS = NB * 8;
    __shared__ int samp[NB * 72];
    __shared__ int q8[128];
    __shared__ __attribute__((aligned(16))) int16_t zq[NB * 64];
    const int t = threadIdx.x, by = blockIdx.y, bx0 = blockIdx.x * NB;
    const uint8_t* img = src + (size_t)blockIdx.z * h * w;
    if (t < 128) q8[t] = 8 * quant_entry(t >> 6, t & 63, quality);
    for (int i = t; i < 8 * PX; i += THREADS) {
        const int r = i / PX, c = i - r * PX;
        const int gy = min(by * 8 + r, h - 1), gx = min(bx0 * 8 + c, w - 1);
        samp[(c >> 3) * 72 + r * 9 + (c & 7)] = (int)img[(size_t)gy * w + gx] - 128;
    }
    __syncthreads();
    int16_t* dst = coef + ((size_t)blockIdx.z * nblk + (size_t)by * bw + bx0) * 64;
    dct_quantise_store<NB>(samp, q8, zq, dst, min(NB, bw - bx0), [](int) { return 0; }, [](int) { return false; });
}

// ---- entropy coding: one wave64 per block, one lane per coefficient ------------------------------------------------------------------------
// The MCU layout is a template parameter of what follows: HS x VS luma blocks, then Cb and Cr (2 x 2: 4:2:0, 2 x 1: 4:2:2, 1 x 1: 4:4:4).
struct Geometry {
    int c, mw, bw, bh;
    size_t nblk;
};

template <int HS, int VS>
__device__ __forceinline__ bool luma_is_real(const Geometry& g, int mx, int my, int k) { return HS * mx + (k % HS) < g.bw && VS * my + (k / HS) < g.bh; }

// The DC difference of block b of a frame (wave-uniform).  The predictor of a real luma block is the last real block before it in the
// scan: the dummy blocks in between carry that block's DC.
template <int HS, int VS>
__device__ int dc_difference(const int16_t* __restrict__ coef, size_t b, const Geometry& g, int* table) {
    constexpr int NL = HS * VS, BPM = NL + 2;
    *table = 0;
    if (g.c != 3) return coef[b * 64] - (b ? coef[(b - 1) * 64] : 0);
    size_t m = b / BPM;
    int k = (int)(b - m * BPM);
    if (k >= NL) {
        *table = 1;
        return coef[b * 64] - (m ? coef[((m - 1) * BPM + k) * 64] : 0);
    }
    if (!luma_is_real<HS, VS>(g, (int)(m % g.mw), (int)(m / g.mw), k)) return 0;
    const int dc = coef[b * 64];
    if (k == 0) {
        if (m == 0) return dc;
        --m, k = NL - 1;
    } else {
        --k;
    }
    const int mx = (int)(m % g.mw), my = (int)(m / g.mw);
    while (!luma_is_real<HS, VS>(g, mx, my, k)) --k;      // block 0 of an MCU is always real
    return dc - coef[(m * BPM + k) * 64];
}

// What this lane puts into the stream: the ZRLs of its run, its code and its value bits, and the EOB when it is the last coded
// coefficient of a block that does not end at 63; right-aligned in *pattern.  Returns the number of bits (0: a zero).  Annex K's tables
// (OPT false) keep all of it within 63 bits.  A frame's own tables (OPT: `huff`, its SLOTS HuffSlot) may give ZRL and EOB 16 bits, 90 in
// all, so there the ZRLs go first into *zrl (at most 48 bits, *zrl_len) and the rest (at most 42) into *pattern.
template <bool OPT>
__device__ __forceinline__ int lane_bits(int lane, int v, int table, const HuffSlot* __restrict__ huff, uint64_t* pattern, uint64_t* zrl, int* zrl_len) {
    const uint64_t mask = __ballot(v != 0) | 1ull;        // the DC always codes
    *zrl = 0, *zrl_len = 0;
    if (!((mask >> lane) & 1)) { *pattern = 0; return 0; }
    const int a = v < 0 ? -v : v;
    const int size = 32 - __clz(a);
    const uint32_t value = (uint32_t)(v < 0 ? v - 1 : v) & ((1u << size) - 1);
    const HuffSlot* dc = huff + 2 * table;
    const HuffSlot* ac = dc + 1;
    auto ac_code = [&](int sym) { return OPT ? (int)ac->code[sym] : (int)T.huff.ac_code[table][sym]; };
    auto ac_len = [&](int sym) { return OPT ? (int)ac->len[sym] : (int)T.huff.ac_len[table][sym]; };
    uint64_t pat = 0;
    int len = 0;
    if (lane == 0) {
        pat = OPT ? dc->code[size] : T.huff.dc_code[table][size], len = OPT ? dc->len[size] : T.huff.dc_len[table][size];
    } else {
        const int prev = 63 - __clzll((long long)(mask & ((1ull << lane) - 1)));
        const int run = lane - prev - 1;
        const int zc = ac_code(0xf0), zl = ac_len(0xf0);
        for (int k = 0; k < (run >> 4); ++k) pat = (pat << zl) | zc, len += zl;
        if (OPT) *zrl = pat, *zrl_len = len, pat = 0, len = 0;
        const int sym = ((run & 15) << 4) | size;
        const int cl = ac_len(sym);
        pat = (pat << cl) | ac_code(sym), len += cl;
    }
    pat = (pat << size) | value, len += size;
    if (lane < 63 && lane == 63 - __clzll((long long)mask)) {
        const int el = ac_len(0);
        pat = (pat << el) | ac_code(0), len += el;
    }
    *pattern = pat;
    return len;
}

// ORs the `len` (1..64) right-aligned bits of pat into the big-endian bit stream at bit position pos.  A word is touched only where
// there are bits for it: never beyond the frame's last coded bit.
__device__ __forceinline__ void or_bits(uint32_t* __restrict__ stream, uint64_t pos, uint64_t pat, int len) {
    uint32_t* word = stream + (size_t)(pos >> 5);
    const int o = (int)(pos & 31);
    const uint64_t hi = pat << (64 - len);                // left-aligned; the 96-bit window starting at the word is hi >> o
    const uint32_t w0 = (uint32_t)((hi >> 32) >> o), w1 = (uint32_t)(hi >> o), w2 = o ? (uint32_t)hi << (32 - o) : 0u;
    if (w0) atomicOr(word, w0);
    if (w1) atomicOr(word + 1, w1);
    if (w2) atomicOr(word + 2, w2);
}

// count (EMIT false): bits[block] = the bits the block's lanes put into the stream.  emit: the lanes OR them into the frame's stream, from
// the block's offset off[block] on, each behind the lanes before it.
template <int HS, int VS, bool OPT, bool EMIT>
__global__ __launch_bounds__(256) void jpeg_code_kernel(const int16_t* __restrict__ coef, Geometry g, size_t total_blocks, const HuffSlot* __restrict__ huff,
                                                        uint32_t* __restrict__ bits, const uint64_t* __restrict__ off, uint32_t* __restrict__ stream,
                                                        size_t stream_words) {
    const size_t gw = (size_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (gw >= total_blocks) return;
    const int lane = threadIdx.x & 63;
    const size_t f = gw / g.nblk, b = gw - f * g.nblk;
    const int16_t* fc = coef + f * g.nblk * 64;
    int table;
    const int diff = dc_difference<HS, VS>(fc, b, g, &table);
    const int v = lane == 0 ? diff : fc[b * 64 + lane];
    uint64_t pat, zrl;
    int zrl_len;
    const int len = lane_bits<OPT>(lane, v, table, huff + f * SLOTS, &pat, &zrl, &zrl_len);
    if (!EMIT) {
        int sum = len + zrl_len;
        for (int d = 32; d >= 1; d >>= 1) sum += __shfl_xor(sum, d);
        if (lane == 0) bits[gw] = (uint32_t)sum;
        return;
    }
    int incl = len + zrl_len;
    for (int d = 1; d < 64; d <<= 1) {
        const int up = __shfl_up(incl, d);
        if (lane >= d) incl += up;
    }
    if (len == 0) return;
    const uint64_t pos = off[gw] + (uint64_t)(incl - len - zrl_len);
    if (OPT && zrl_len) or_bits(stream + f * stream_words, pos, zrl, zrl_len);
    or_bits(stream + f * stream_words, pos + zrl_len, pat, len);
}

// ---- optimised tables: libjpeg's two-pass optimize_coding --------------------------------------------------------------------------------
// histogram  the symbols emit will code, per frame and table slot: the DC category; per non-zero AC its run/size symbol and 0xF0 once per
//            ZRL; 0x00 per EOB.  A workgroup counts its blocks in LDS (at most 64 symbols per block and table, far below 2^32 for
//            the blocks one workgroup sees) and adds what it has to the frame's 64-bit counters: integer adds, any order, and no wrap
// table      one workgroup per (frame, slot), one thread per symbol plus the pseudo-symbol 256 of frequency 1 (so that no code is all
//            ones).  Merge until one tree is left: c1 = the smallest non-zero frequency, among equals the LARGEST symbol; c2 = the same
//            without c1; c1 takes both frequencies, c2 becomes 0, every member of both trees gets one bit longer and c2's tree joins
//            c1's.  Then the symbols are counted per length and limited to 16 as in Annex K.3 (from the longest down to 17: take two from
//            length i, give one to i - 1; take one from the largest j <= i - 2 that has any, give two to j + 1), the pseudo-symbol leaves
//            the longest length, and the symbols are listed by UNRESTRICTED length, then by value; codes count up per length.
template <int HS, int VS>
__global__ __launch_bounds__(256) void jpeg_histogram_kernel(const int16_t* __restrict__ coef, Geometry g, unsigned long long* __restrict__ hist) {
    __shared__ uint32_t cnt[SLOTS][256];
    const int lane = threadIdx.x & 63;
    const size_t f = blockIdx.y;
    for (int i = threadIdx.x; i < SLOTS * 256; i += 256) (&cnt[0][0])[i] = 0;
    __syncthreads();
    const int16_t* fc = coef + f * g.nblk * 64;
    for (size_t b = (size_t)blockIdx.x * 4 + (threadIdx.x >> 6); b < g.nblk; b += (size_t)gridDim.x * 4) {
        int table;
        const int diff = dc_difference<HS, VS>(fc, b, g, &table);
        const int v = lane == 0 ? diff : fc[b * 64 + lane];
        const uint64_t mask = __ballot(v != 0) | 1ull;
        if (!((mask >> lane) & 1)) continue;
        const int size = 32 - __clz(v < 0 ? -v : v);
        if (lane == 0) {
            atomicAdd(&cnt[2 * table][size], 1u);
        } else {
            const int run = lane - (63 - __clzll((long long)(mask & ((1ull << lane) - 1)))) - 1;
            if (run >> 4) atomicAdd(&cnt[2 * table + 1][0xf0], (uint32_t)(run >> 4));
            atomicAdd(&cnt[2 * table + 1][((run & 15) << 4) | size], 1u);
        }
        if (lane < 63 && lane == 63 - __clzll((long long)mask)) atomicAdd(&cnt[2 * table + 1][0], 1u);
    }
    __syncthreads();
    for (int k = 0; k < SLOTS; ++k) {
        const uint32_t c = cnt[k][threadIdx.x];
        if (c) atomicAdd(&hist[(f * SLOTS + k) * 256 + threadIdx.x], (unsigned long long)c);
    }
}

constexpr int TABLE_THREADS = 320;      // 5 waves: a thread per symbol 0..256, the rest idle

// The thread holding the smallest non-zero frequency (among equals the largest index) of those with `in`; -1: none.  Uniform over the
// workgroup.  part: one of two LDS buffers that successive calls alternate, so that one barrier per call is enough: a wave can write a
// buffer again only behind the barrier of the call in between, which every reader of the earlier contents has reached.
struct Least {
    unsigned long long f;
    int at;
};
__device__ __forceinline__ Least better(Least a, Least b) { return (b.at >= 0 && (a.at < 0 || b.f < a.f || (b.f == a.f && b.at > a.at))) ? b : a; }
__device__ __forceinline__ Least least_frequency(unsigned long long f, bool in, Least* part) {
    Least m{f, in && f ? (int)threadIdx.x : -1};
    for (int d = 32; d >= 1; d >>= 1) {
        Least o;
        o.f = ((unsigned long long)(uint32_t)__shfl_xor((int)(m.f >> 32), d) << 32) | (uint32_t)__shfl_xor((int)(uint32_t)m.f, d);
        o.at = __shfl_xor(m.at, d);
        m = better(m, o);
    }
    if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = m;
    __syncthreads();
    m = part[0];
    for (int k = 1; k < TABLE_THREADS / 64; ++k) m = better(m, part[k]);
    return m;
}

// slots: table slots per frame in hist and huff (blockIdx.y: the frame, blockIdx.x: its slot)
__global__ __launch_bounds__(TABLE_THREADS) void jpeg_table_kernel(const unsigned long long* __restrict__ hist, HuffSlot* __restrict__ huff, int slots) {
    __shared__ Least part[2][TABLE_THREADS / 64];
    __shared__ int size_of[256];                // the unrestricted code length per symbol
    __shared__ int bits[260];                   // symbols per code length; a chain of 257 symbols is at most 256 deep
    __shared__ int first[18], upto[18];         // per length 1..16: its first code; the symbols of shorter-or-equal length
    const int t = threadIdx.x;
    const size_t slot = (size_t)blockIdx.y * slots + blockIdx.x;
    unsigned long long f = t < 256 ? hist[slot * 256 + t] : t == 256 ? 1ull : 0ull;
    int tree = t, size = 0;
    for (int i = t; i < 260; i += TABLE_THREADS) bits[i] = 0;
    for (;;) {
        const Least c1 = least_frequency(f, true, part[0]);
        const Least c2 = least_frequency(f, t != c1.at, part[1]);
        if (c2.at < 0) break;
        if (t == c1.at) f += c2.f;
        if (t == c2.at) f = 0;
        if (tree == c1.at || tree == c2.at) ++size, tree = c1.at;
    }
    if (t < 256) size_of[t] = size;
    __syncthreads();
    if (t <= 256 && size) atomicAdd(&bits[size], 1);
    __syncthreads();
    if (t == 0) {
        for (int i = 256; i > 16; --i)
            while (bits[i] > 0) {
                int j = i - 2;
                while (j > 0 && bits[j] == 0) --j;
                bits[i] -= 2, bits[i - 1] += 1, bits[j + 1] += 2, bits[j] -= 1;
            }
        int i = 16;
        while (i > 1 && bits[i] == 0) --i;
        bits[i] -= 1;
        int code = 0, n = 0;
        upto[0] = 0;
        for (int len = 1; len <= 16; ++len) {
            first[len] = code, n += bits[len], upto[len] = n;
            code = (code + bits[len]) << 1;
            huff[slot].bits[len - 1] = (uint8_t)bits[len];
        }
        huff[slot].nvals = (uint32_t)n;
    }
    __syncthreads();
    if (t < 256) {
        int len = 0, code = 0;
        if (size) {
            int rank = 0;
            for (int s = 0; s < 256; ++s) {
                const int other = size_of[s];
                rank += (other && (other < size || (other == size && s < t))) ? 1 : 0;
            }
            len = 1;
            while (len < 16 && upto[len] <= rank) ++len;
            code = first[len] + rank - upto[len - 1];
            huff[slot].vals[rank] = (uint8_t)t;
        }
        huff[slot].code[t] = (uint16_t)code, huff[slot].len[t] = (uint8_t)len;
    }
}

// ---- the back half of every file: from the entries' bit counts to the stuffed bytes, per (frame, segment) ----------------------------------
//   scan       out = the exclusive scan of a segment's entries' bit counts (64-bit offsets), the sum to total_bits[frame][segment]
//   zero       the words of the bit stream the segment will use; count or emit of the file's kind then fills them
//   ffcount    the 0xFF bytes per CHUNK of the segment's stream, the 1-bit padding of its last byte applied
//   scan       of those counts over the chunks the segment's bits fill, the sum to fftotal[frame][segment]
//   stuffed copy   the scatter of the file's kind places each segment's bytes behind what it writes in front of them, a 0x00 after each 0xFF
// One workgroup per (frame, segment) scans; STREAM_GRID workgroups per frame walk the segments one after the other, a chunk per pass.
__device__ __forceinline__ size_t stream_bytes(uint64_t bits) { return (size_t)((bits + 7) >> 3); }
__device__ __forceinline__ size_t stream_chunks(uint64_t bits) { return (stream_bytes(bits) + CHUNK - 1) / CHUNK; }

// out[i] = in[0] + ... + in[i - 1] over `count` entries by the SCAN_THREADS threads of a workgroup; part: one entry of LDS per thread.
// Returns, in the last thread, the sum.
template <class In, class Out>
__device__ __forceinline__ Out exclusive_scan(const In* __restrict__ in, Out* __restrict__ out, size_t count, Out* part) {
    const int t = threadIdx.x;
    const size_t per = (count + SCAN_THREADS - 1) / SCAN_THREADS;
    const size_t a = min((size_t)t * per, count), b = min(a + per, count);
    Out sum = 0;
    for (size_t i = a; i < b; ++i) sum += in[i];
    part[t] = sum;
    __syncthreads();
    for (int d = 1; d < SCAN_THREADS; d <<= 1) {
        const Out add = t >= d ? part[t - d] : (Out)0;
        __syncthreads();
        part[t] += add;
        __syncthreads();
    }
    Out run = part[t] - sum;
    for (size_t i = a; i < b; ++i) {
        const Out v = in[i];
        out[i] = run;
        run += v;
    }
    return part[t];
}

// out = the exclusive scan of segment blockIdx.x of frame blockIdx.y - CHUNKS false: its entries; true: the chunks its count_bits coded bits
// fill - and the sum to total[frame][segment]
template <class In, class Out, bool CHUNKS>
__global__ __launch_bounds__(SCAN_THREADS) void jpeg_scan_kernel(const In* __restrict__ in, Out* __restrict__ out, Out* __restrict__ total, Segments S,
                                                                 const uint64_t* __restrict__ count_bits) {
    __shared__ Out part[SCAN_THREADS];
    const size_t f = blockIdx.y, slot = f * S.totals + blockIdx.x;
    const Segment& sg = S.s[blockIdx.x];
    const size_t at = CHUNKS ? f * S.chunks + sg.chunk0 : f * S.entries + sg.entry0;
    const Out sum = exclusive_scan(in + at, out + at, CHUNKS ? stream_chunks(count_bits[slot]) : (size_t)sg.nentries, part);
    if (threadIdx.x == SCAN_THREADS - 1) total[slot] = sum;
}

__global__ __launch_bounds__(256) void jpeg_zero_kernel(uint32_t* __restrict__ stream, Segments S, const uint64_t* __restrict__ total_bits) {
    const size_t f = blockIdx.y;
    int k = 0;
    do {          // a file has a segment: the first one's loads do not wait for count, as a baseline file's never did
        const size_t words = (size_t)((total_bits[f * S.totals + k] + 31) >> 5) + 2;          // the plan keeps 4 beyond each segment's bound
        uint32_t* s = stream + f * S.stream_words + S.s[k].word0;
        for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < words; i += (size_t)gridDim.x * 256) s[i] = 0;
    } while (++k < S.count);
}

// ---- byte stuffing -------------------------------------------------------------------------------------------------------------------------
// Word i of a frame's stream as its four bytes in file order (the first in the top byte), the 1-bit padding of the last byte applied;
// *valid = how many of them are part of the stream.
__device__ __forceinline__ uint32_t stream_word(const uint32_t* __restrict__ s, size_t i, uint64_t bits, int* valid) {
    const size_t nbytes = stream_bytes(bits);
    if (i * 4 >= nbytes) { *valid = 0; return 0; }
    uint32_t v = s[i];
    *valid = (int)min((size_t)4, nbytes - i * 4);
    if (i == (nbytes - 1) >> 2) {
        const int pad = (int)(nbytes * 8 - bits);
        v |= ((1u << pad) - 1) << (24 - 8 * (int)((nbytes - 1) & 3));
    }
    return v;
}

__device__ __forceinline__ int count_ff(uint32_t v, int valid) {
    int c = 0;
#pragma unroll
    for (int k = 0; k < 4; ++k) c += (k < valid && ((v >> (24 - 8 * k)) & 255) == 255) ? 1 : 0;
    return c;
}

__global__ __launch_bounds__(256) void jpeg_ffcount_kernel(const uint32_t* __restrict__ stream, Segments S, const uint64_t* __restrict__ total_bits,
                                                           uint32_t* __restrict__ ffcnt) {
    __shared__ int part[4];
    const size_t f = blockIdx.y;
    int k = 0;
    do {          // as in jpeg_zero_kernel
        const uint64_t bits = total_bits[f * S.totals + k];
        const uint32_t* s = stream + f * S.stream_words + S.s[k].word0;
        for (size_t ck = blockIdx.x; ck < stream_chunks(bits); ck += gridDim.x) {
            int valid;
            const uint32_t v = stream_word(s, ck * (CHUNK / 4) + threadIdx.x, bits, &valid);
            const int incl = workgroup_inclusive(count_ff(v, valid), part);
            if (threadIdx.x == 255) ffcnt[f * S.chunks + S.s[k].chunk0 + ck] = (uint32_t)incl;
        }
    } while (++k < S.count);
}

// The stuffed copy of one segment by the frame's workgroups: the `bits` coded bits of its stream s go to dst with a 0x00 after each 0xFF;
// ffoff: per chunk of the segment, the 0xFF bytes in front of it.  part: 4 ints of LDS.
__device__ __forceinline__ void stuffed_copy(const uint32_t* __restrict__ s, uint64_t bits, const uint32_t* __restrict__ ffoff, uint8_t* __restrict__ dst, int* part) {
    for (size_t ck = blockIdx.x; ck < stream_chunks(bits); ck += gridDim.x) {
        int valid;
        const uint32_t v = stream_word(s, ck * (CHUNK / 4) + threadIdx.x, bits, &valid);
        const int c = count_ff(v, valid);
        const int before = workgroup_inclusive(c, part) - c;
        uint8_t* d = dst + ck * CHUNK + ffoff[ck] + threadIdx.x * 4 + before;
        for (int k = 0; k < valid; ++k) {
            const uint8_t byte = (uint8_t)(v >> (24 - 8 * k));
            *d++ = byte;
            if (byte == 255) *d++ = 0;
        }
    }
}

// FFD9 behind the last segment's bytes, which end at `end`, and the file's length
__device__ __forceinline__ void end_file(uint8_t* __restrict__ file, size_t end, int32_t* __restrict__ length) {
    file[end] = 0xff, file[end + 1] = 0xd9;
    *length = (int32_t)(end + 2);
}

// Byte i of a frame's header.  luma: SOF0's sampling byte of component 1.  OPT: the DHT segments hold the frame's own tables (`huff`, its
// SLOTS HuffSlot; `slots` of them used), each with only the symbols that occur, so the header's length varies per frame: at[k] is
// where segment k starts, at[slots] where SOS does.
template <bool OPT>
__device__ __forceinline__ int header_byte(int i, int rgb, int h, int w, int quality, int luma, const HuffSlot* __restrict__ huff, const int* at, int slots) {
    if (OPT && i >= T.dht[rgb]) {
        if (i >= at[slots]) return T.hdr[rgb][T.sos[rgb] + i - at[slots]];
        int k = 0;
        while (i >= at[k + 1]) ++k;
        const int j = i - at[k], payload = 2 + 1 + 16 + (int)huff[k].nvals;
        return j == 0 ? 0xff : j == 1 ? 0xc4 : j == 2 ? payload >> 8 : j == 3 ? payload & 255 : j == 4 ? ((k & 1) << 4) | (k >> 1)
             : j < 21 ? huff[k].bits[j - 5] : huff[k].vals[j - 21];
    }
    int v = T.hdr[rgb][i];
    for (int k = 0; k <= rgb; ++k)
        if (i >= T.dqt[rgb][k] && i < T.dqt[rgb][k] + 64) v = quant_entry(k, T.zigzag[i - T.dqt[rgb][k]], quality);
    const int j = i - T.sof_hw[rgb];
    if (j >= 0 && j < 4) v = j == 0 ? h >> 8 : j == 1 ? h & 255 : j == 2 ? w >> 8 : w & 255;
    return i == T.sof_luma[rgb] ? luma : v;
}

// The baseline file of frame blockIdx.y: the header, its one segment's stuffed bytes, FFD9
template <bool OPT>
__global__ __launch_bounds__(256) void jpeg_scatter_kernel(const uint32_t* __restrict__ stream, size_t stream_words, const uint64_t* __restrict__ total_bits,
                                                           const uint32_t* __restrict__ ffoff, const uint32_t* __restrict__ fftotal, size_t chunks, int h, int w,
                                                           int rgb, int quality, int luma, const HuffSlot* __restrict__ huff, uint8_t* __restrict__ out,
                                                           size_t out_stride, int32_t* __restrict__ lengths) {
    __shared__ int part[4];
    const size_t f = blockIdx.y;
    const uint64_t bits = total_bits[f];
    uint8_t* file = out + f * out_stride;
    const int slots = rgb ? 4 : 2;
    int at[SLOTS + 1] = {}, hdr = T.hdr_len[rgb];
    if (OPT) {
        huff += f * SLOTS;
        at[0] = T.dht[rgb];
        for (int k = 0; k < slots; ++k) at[k + 1] = at[k] + 4 + 1 + 16 + (int)huff[k].nvals;
        hdr = at[slots] + T.hdr_len[rgb] - T.sos[rgb];
    }
    if (blockIdx.x == 0) {
        for (int i = threadIdx.x; i < hdr; i += 256) file[i] = (uint8_t)header_byte<OPT>(i, rgb, h, w, quality, luma, huff, at, slots);
        if (threadIdx.x == 0) end_file(file, hdr + stream_bytes(bits) + fftotal[f], lengths + f);
    }
    stuffed_copy(stream + f * stream_words, bits, ffoff + f * chunks, file + hdr, part);
}

// ---- progressive files: libjpeg's jpeg_simple_progression ------------------------------------------------------------------------------
// adain_jpeg_encode_progressive_u8: the file Pillow's save(progressive=True) writes.  The quantised coefficients are the baseline file's -
// the transform stage is used unchanged - and only the entropy coding differs.  tests/jpeg_progressive_encode_ref.py restates the rules,
// tests/test_jpeg_progressive_encode_host.py holds that to Pillow.
//
// The rules
//   header   the baseline file's up to the frame header, which is SOF2 (FFC2); no DHT there: every scan brings its own
//   scans    (Ss-Se, Ah, Al); colour, 10: DC of Y Cb Cr interleaved (0-0, 0, 1); Y (1-5, 0, 2); Cr (1-63, 0, 1); Cb (1-63, 0, 1); Y (6-63, 0, 2);
//            Y (1-63, 2, 1); DC again (0-0, 1, 0); Cr (1-63, 1, 0); Cb (1-63, 1, 0); Y (1-63, 1, 0).  Grey, 6: DC (0-0, 0, 1); (1-5, 0, 2);
//            (6-63, 0, 2); (1-63, 2, 1); DC (0-0, 1, 0); (1-63, 1, 0)
//   tables   libjpeg forces optimize_coding: every scan that codes symbols is preceded by the DHT of the optimal table of its own symbol
//            counts (the table stage above).  The first DC scan: class 0 id 0 (Y), then for colour class 0 id 1 (Cb and Cr counted
//            together); an AC scan: class 1, id 0 for Y and 1 for chroma; the second DC scan has none.  SOS names only the table in use
//   blocks   the DC scans are interleaved: MCU order, dummy luma blocks included, a dummy carrying the DC of the real block before it
//            in its MCU.  An AC scan holds one component: its own grid row-major - Y ceil(h/8) x ceil(w/8) without the dummies, chroma
//            the MCU grid.  No second copy of the coefficients: a scan's block index is mapped to the transform's block
//   DC       first: v = DC >> Al (arithmetic), the difference to the component's previous v coded as baseline codes a DC.  Again: one raw
//            bit per block, (DC >> Al) & 1
//   AC first t = |coef| >> Al over the band; zeros extend the run r; a non-zero t writes the pending end-of-band run, a ZRL (0xF0) per 16
//            of r, the symbol (r << 4) | bit_length(t) and t (a negative coefficient: ~t) in that many bits.  A block whose band ends in
//            zeros adds 1 to EOBRUN, which is written as the symbol n << 4, n = floor(log2(EOBRUN)), and the low n bits of EOBRUN: before
//            the next symbol, at the end of the scan, and at once when it reaches 0x7FFF
//   AC again a = |coef| >> Al; EOB = the last a == 1 of the band.  a == 0 extends r; at every non-zero a, while r > 15 and k <= EOB: the
//            pending run, a ZRL, then the correction bits buffered so far; a > 1 buffers its correction bit a & 1; a == 1 writes the pending
//            run, (r << 4) | 1, a sign bit (0 negative, 1 positive) and the buffered bits.  A block with anything behind its EOB adds 1 to
//            EOBRUN and its buffered bits to the run's; the run is written - symbol, count bits, then those bits - as above, and at once
//            when it holds more than 937 bits (MAX_CORR_BITS - DCTSIZE2 + 1)
//   data     every scan is padded to a byte with 1-bits and byte-stuffed on its own; FFD9 ends the file
//
// The stages (13 launches and a memset per call, every one over all n frames and all scans: a "unit" is one block of one scan)
//   transform  the baseline encoder's, unchanged
//   state      a wave per unit: does the block code a symbol, does it add to EOBRUN, how many correction bits does it leave to the run
//   walk       a run is delimited by the blocks that code a symbol, and its 0x7FFF cuts lie at fixed offsets from its start, but the 937-bit
//              cut is greedy in the bits gathered so far: no scan primitive places it.  So one wave per run walks its run from its first
//              block, 64 blocks a step (a prefix sum over the lanes finds the next cut), and leaves per block the bits buffered before
//              it and where its run is written, per written run its count and bits.  The walk is sequential in the steps: the worst
//              case is one wave over a frame without detail, all blocks of a scan - 33 124 for a 1456 x 1456 frame, 518 steps; frames
//              with detail have short runs and as many waves as runs
//   histogram / table   the symbols per (frame, slot), the runs' n << 4 included, and their optimal codes: the stages of `optimize`
//   count / emit   one kernel, as the baseline file's: the bits of a unit, then - behind the back half's scan and zero - the bits themselves;
//              emit also places a lane's buffered bit behind the symbol of the lane that flushes it, or in its run's tail
//   the back half  the baseline file's kernels ("the back half of every file") with a segment per scan; the scatter adds up the scans'
//              DHT, SOS and stuffed lengths, writes them and calls the stuffed copy per scan
constexpr int PSLOTS = 10;              // table slots per frame: 2 DC + 8 AC; grey uses 1 + 4
constexpr int EOBRUN_CAP = 0x7fff;
constexpr int CORR_CUT = 937;           // MAX_CORR_BITS - DCTSIZE2 + 1
// The most bits a block can put into a scan when every code may be 16 bits long.  A coefficient counts in every scan that can spend bits on
// it: a luma AC coefficient in three (first, and twice again), a chroma one in two.
//   DC first   a code and an 11-bit difference; DC again: 1 bit
//   run        the symbol and 14 count bits, at most once per block (the block that ends the run) and only when the band's last
//              coefficient is not newly coded - that one is then zero (no bits) or costs its correction bit
//   AC first   a code and 10 value bits per coefficient (a ZRL's 16 bits stand for 16 coefficients without any): m x 26, or (m - 1) x 26 + 30
//   AC again   a code and a sign bit per new coefficient, one bit per old one: m x 17, or (m - 1) x 17 + 1 + 30
constexpr int P_DC_FIRST_BITS = 16 + 11, P_RUN_BITS = 16 + 14;
constexpr int prog_ac_bits(int m, bool again) { return again ? (m - 1) * 17 + 1 + P_RUN_BITS : (m - 1) * 26 + P_RUN_BITS; }
constexpr int P_DHT_BYTES = 4 + 1 + 16 + 256;

struct PScan {
    int comp;                           // 0 Y, 1 Cb, 2 Cr; -1: every component, interleaved (the DC scans)
    int ss, se, ah, al;
    int slot;                           // the scan's table slot (first DC scan: Y's, the chroma one follows); -1: it codes no symbol
    uint32_t nblk;                      // blocks in the scan
};
struct PScript {
    int c, hs, vs, mw, bw, bh, nscans, nslots;
    size_t nblk;                        // coefficient blocks per frame
    PScan s[PSCANS];
    Segments seg;                       // scan i's units, stream and chunks: segment i; its entries are the frame's units
};
struct ProgPlan {
    Plan base;                          // the transform's geometry
    PScript P;
    size_t out_stride;
    size_t o_coef, o_state, o_pre, o_run_n, o_run_be, o_run_end, o_body, o_bits, o_off, o_total, o_stream, o_ffcnt, o_ffoff, o_fftotal, o_hist, o_huff, total;
};

ProgPlan make_prog_plan(int n, int h, int w, int c, int sampling) {
    static const int COLOUR[PSCANS][6] = {{-1, 0, 0, 0, 1, 0}, {0, 1, 5, 0, 2, 2}, {2, 1, 63, 0, 1, 3}, {1, 1, 63, 0, 1, 4}, {0, 6, 63, 0, 2, 5},
                                          {0, 1, 63, 2, 1, 6}, {-1, 0, 0, 1, 0, -1}, {2, 1, 63, 1, 0, 7}, {1, 1, 63, 1, 0, 8}, {0, 1, 63, 1, 0, 9}};
    static const int GREY[6][6] = {{-1, 0, 0, 0, 1, 0}, {0, 1, 5, 0, 2, 1}, {0, 6, 63, 0, 2, 2}, {0, 1, 63, 2, 1, 3}, {-1, 0, 0, 1, 0, -1}, {0, 1, 63, 1, 0, 4}};
    ProgPlan p{};
    p.base = make_plan(n, h, w, c, sampling, false);
    PScript& P = p.P;
    P.c = c, P.hs = p.base.hs, P.vs = p.base.vs, P.mw = p.base.mw, P.bw = p.base.bw, P.bh = p.base.bh;
    P.nscans = c == 3 ? PSCANS : 6, P.nslots = c == 3 ? PSLOTS : 5;
    P.nblk = p.base.nblk;
    P.seg.totals = PSCANS;
    p.out_stride = HOST_T.dht[c == 3] + 2;
    for (int i = 0; i < P.nscans; ++i) {
        const int* d = c == 3 ? COLOUR[i] : GREY[i];
        PScan& sc = P.s[i];
        sc.comp = d[0], sc.ss = d[1], sc.se = d[2], sc.ah = d[3], sc.al = d[4], sc.slot = d[5];
        const size_t nblk = sc.comp < 0 ? P.nblk : sc.comp == 0 ? (size_t)P.bw * P.bh : (size_t)P.mw * p.base.mh;
        const int block_bits = sc.ss ? prog_ac_bits(sc.se - sc.ss + 1, sc.ah != 0) : sc.ah ? 1 : P_DC_FIRST_BITS;
        const size_t max_bytes = (nblk * block_bits + 7) / 8;          // entropy-coded bytes before stuffing, at most
        sc.nblk = (uint32_t)nblk;
        P.seg.add(nblk, max_bytes);
        const int tables = sc.slot < 0 ? 0 : sc.ss == 0 && c == 3 ? 2 : 1, comps = sc.comp < 0 ? c : 1;
        p.out_stride += tables * P_DHT_BYTES + 8 + 2 * comps + 2 * max_bytes;
    }
    const size_t N = (size_t)n, units = P.seg.entries;
    Carve ws;
    p.o_coef = ws.take(N * P.nblk * 64 * sizeof(int16_t));
    p.o_state = ws.take(N * units * sizeof(uint8_t));
    p.o_pre = ws.take(N * units * sizeof(uint16_t));
    p.o_run_n = ws.take(N * units * sizeof(uint16_t));
    p.o_run_be = ws.take(N * units * sizeof(uint16_t));
    p.o_run_end = ws.take(N * units * sizeof(uint32_t));
    p.o_body = ws.take(N * units * sizeof(uint32_t));
    p.o_bits = ws.take(N * units * sizeof(uint32_t));
    p.o_off = ws.take(N * units * sizeof(uint64_t));
    p.o_total = ws.take(N * PSCANS * sizeof(uint64_t));
    p.o_stream = ws.take(N * P.seg.stream_words * sizeof(uint32_t));
    p.o_ffcnt = ws.take(N * P.seg.chunks * sizeof(uint32_t));
    p.o_ffoff = ws.take(N * P.seg.chunks * sizeof(uint32_t));
    p.o_fftotal = ws.take(N * PSCANS * sizeof(uint32_t));
    p.o_hist = ws.take(N * PSLOTS * 256 * sizeof(uint64_t));
    p.o_huff = ws.take(N * PSLOTS * sizeof(HuffSlot));
    p.total = ws.at;
    return p;
}

__device__ __forceinline__ uint64_t bits_upto(int p) { return p < 0 ? 0ull : p >= 63 ? ~0ull : (2ull << p) - 1; }          // bits 0..p
__device__ __forceinline__ int top_bit(uint64_t m) { return m ? 63 - __clzll((long long)m) : -1; }

// The scan a frame's unit is in; *first: that scan's first unit
__device__ __forceinline__ int prog_scan_of(const PScript& P, size_t unit, size_t* first) {
    int s = 0;
    *first = 0;
    while (s + 1 < P.nscans && unit >= P.seg.s[s + 1].entry0) *first = P.seg.s[++s].entry0;
    return s;
}

// Block bi of a scan's own grid -> the block of the transform's array (MCU order: hs x vs luma blocks, Cb, Cr)
__device__ __forceinline__ size_t prog_coef_block(const PScript& P, int comp, uint32_t bi) {
    if (P.c != 3 || comp < 0) return bi;
    const int nl = P.hs * P.vs, bpm = nl + 2;
    if (comp > 0) return (size_t)bi * bpm + nl + comp - 1;
    const uint32_t by = bi / (uint32_t)P.bw, bx = bi - by * (uint32_t)P.bw;
    return ((size_t)(by / P.vs) * P.mw + bx / P.hs) * bpm + (by % P.vs) * P.hs + bx % P.hs;
}

// The DC of block b (MCU order): the transform leaves 0 in a dummy luma block, which carries the DC of the real block before it in its MCU
__device__ int prog_dc(const int16_t* __restrict__ fc, const PScript& P, size_t b) {
    if (P.c != 3) return fc[b * 64];
    const int nl = P.hs * P.vs, bpm = nl + 2;
    const size_t m = b / bpm;
    int k = (int)(b - m * bpm);
    if (k >= nl) return fc[b * 64];
    const int mx = (int)(m % P.mw), my = (int)(m / P.mw);
    while (!(P.hs * mx + k % P.hs < P.bw && P.vs * my + k / P.hs < P.bh)) --k;          // block 0 of an MCU is always real
    return fc[(m * bpm + k) * 64];
}

// (DC >> al) minus the same of the component's block before b in the scan; *table: 0 luma, 1 chroma
__device__ int prog_dc_difference(const int16_t* __restrict__ fc, const PScript& P, size_t b, int al, int* table) {
    *table = 0;
    if (P.c != 3) return (prog_dc(fc, P, b) >> al) - (b ? prog_dc(fc, P, b - 1) >> al : 0);
    const int nl = P.hs * P.vs, bpm = nl + 2;
    const size_t m = b / bpm;
    const int k = (int)(b - m * bpm);
    *table = k >= nl;
    const bool none = k >= nl ? m == 0 : b == 0;
    const size_t before = k >= nl ? b - bpm : k ? b - 1 : b - 3;          // luma block 0 follows the last luma block of the MCU before
    return (prog_dc(fc, P, b) >> al) - (none ? 0 : prog_dc(fc, P, before) >> al);
}

// What lane k (coefficient k of a block) does in an AC scan.  "fresh": it codes a symbol - first scans: t != 0; later ones: a == 1.  "old":
// later scans, a > 1: one correction bit, which waits for the next lane that flushes (a fresh one, or an old one in front of EOB with ZRLs
// of its own) and follows that lane's first ZRL or, without one, its symbol and value bits; with no such lane it goes to the run's tail.
struct PLane {
    bool fresh, old;
    int nzrl, sym, size, eob;           // ZRLs in front of it; its symbol; its value bits; the block's last fresh lane (-1: none)
    uint32_t value, corr;
    int waiting;                        // a lane that flushes: the old lanes' bits buffered for it
    int flusher, rank;                  // an old lane: the lane that flushes its bit (-1: the run's tail) and its place among those bits
    uint64_t old_mask;
};

__device__ __forceinline__ PLane prog_lane(int lane, int v, const PScan& sc) {
    PLane L;
    const bool in = lane >= sc.ss && lane <= sc.se;
    const int a = in ? (v < 0 ? -v : v) >> sc.al : 0;
    L.fresh = sc.ah ? a == 1 : a != 0;
    L.old = sc.ah && a > 1;
    const uint64_t fm = __ballot(L.fresh), zm = __ballot(in && a == 0), below = (1ull << lane) - 1;
    L.old_mask = __ballot(L.old);
    const int pn = max(top_bit(fm & below), sc.ss - 1);          // the fresh lane before this one, or the band's start
    const uint64_t since = zm & ~bits_upto(pn);
    const int zeros = __popcll(since & below);
    const int pz = top_bit((fm | L.old_mask) & below);           // the non-zero lane before this one
    const int given = pz > pn ? __popcll(since & bits_upto(pz)) >> 4 : 0;          // ZRLs written by then
    L.eob = top_bit(fm);
    L.nzrl = (L.fresh || L.old) && lane <= L.eob ? (zeros >> 4) - given : 0;
    L.size = L.fresh ? 32 - __clz(a) : 0;
    L.sym = ((zeros & 15) << 4) | L.size;
    L.value = (uint32_t)(v < 0 ? ~a : a) & ((1u << L.size) - 1);
    L.corr = (uint32_t)a & 1u;
    const uint64_t flm = __ballot(L.fresh || L.nzrl > 0);
    const uint64_t later = flm & ~bits_upto(lane);
    L.flusher = later ? __ffsll((long long)later) - 1 : -1;
    // an old lane that flushes buffers its own bit after that: the bits waiting at a lane are the old lanes from the last flush on
    L.rank = __popcll(L.old_mask & below & ~bits_upto(top_bit(flm & bits_upto(lane)) - 1));
    L.waiting = __popcll(L.old_mask & below & ~bits_upto(top_bit(flm & below) - 1));
    return L;
}

// state: bit 0 - the block codes a symbol (which first writes the pending run); bit 1 - it adds to EOBRUN; bits 2..7 - the correction bits
// it leaves to the run (old lanes behind its EOB)
__global__ __launch_bounds__(256) void jpeg_prog_state_kernel(const int16_t* __restrict__ coef, PScript P, size_t total_units, uint8_t* __restrict__ state,
                                                              uint16_t* __restrict__ run_n) {
    const size_t gw = (size_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (gw >= total_units) return;
    const int lane = threadIdx.x & 63;
    const size_t f = gw / P.seg.entries, u = gw - f * P.seg.entries;
    size_t unit0;
    const PScan& sc = P.s[prog_scan_of(P, u, &unit0)];
    int st = 0;
    if (sc.ss) {
        const int v = coef[(f * P.nblk + prog_coef_block(P, sc.comp, (uint32_t)(u - unit0))) * 64 + lane];
        const PLane L = prog_lane(lane, v, sc);
        st = (L.eob >= 0 ? 1 : 0) | (L.eob != sc.se ? 2 : 0) | (__popcll(L.old_mask & ~bits_upto(L.eob)) << 2);
    }
    if (lane == 0) state[gw] = (uint8_t)st, run_n[gw] = 0;
}

// One wave per run, 64 blocks a step.  A run starts at a block that adds to EOBRUN and either codes a symbol (which wrote the run before
// it), is the scan's first, or follows a block that added nothing; it goes on through the blocks that code no symbol.  Within a step the
// bits gathered so far are a prefix sum over the lanes, and the next cut is the first lane at which they pass 937 or the count reaches
// 0x7FFF; the walk goes on behind it with an empty run.  pre: the run's correction bits in front of the block's; at the block where a run
// is written run_n, run_be: its count and correction bits; run_end: that block, for every block of the run.
__global__ __launch_bounds__(256) void jpeg_prog_walk_kernel(PScript P, size_t total_units, const uint8_t* __restrict__ state, uint16_t* __restrict__ pre,
                                                             uint16_t* __restrict__ run_n, uint16_t* __restrict__ run_be, uint32_t* __restrict__ run_end) {
    const size_t gw = (size_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (gw >= total_units) return;
    const int lane = threadIdx.x & 63;
    const size_t f = gw / P.seg.entries, u = gw - f * P.seg.entries;
    size_t unit0;
    const PScan& sc = P.s[prog_scan_of(P, u, &unit0)];
    if (sc.ss == 0) return;
    const uint32_t bi = (uint32_t)(u - unit0), s0 = state[gw];
    if (!(s0 & 2) || (bi && !(s0 & 1) && (state[gw - 1] & 2))) return;
    const size_t base = gw - bi;
    uint32_t first = bi, count = 0, be = 0;          // the open run: its first block, its blocks and correction bits so far
    auto write = [&](uint32_t e, uint32_t n, uint32_t bits) {
        if (lane == 0) run_n[base + e] = (uint16_t)n, run_be[base + e] = (uint16_t)bits;
        for (uint32_t i = first + lane; i <= e; i += 64) run_end[base + i] = e;
    };
    for (uint32_t j0 = bi;; j0 += 64) {
        const uint32_t j = j0 + lane;
        const uint32_t st = j < sc.nblk ? state[base + j] : 1u;          // the scan's end stops the run as a block that codes a symbol does
        const uint64_t stops = __ballot((st & 1) && j != bi);
        const int m = stops ? __ffsll((long long)stops) - 1 : 64;         // lanes 0..m-1 are blocks of the run
        const uint32_t brt = lane < m ? st >> 2 : 0u;
        uint32_t incl = brt;
        for (int d = 1; d < 64; d <<= 1) {
            const uint32_t up = __shfl_up(incl, d);
            if (lane >= d) incl += up;
        }
        uint32_t before = 0;          // the bits of the lanes in front of `from`
        for (int from = 0; from < m;) {
            const uint32_t after = be + incl - before;
            const uint64_t cuts = __ballot(lane >= from && lane < m && (after > CORR_CUT || count + lane - from + 1 == EOBRUN_CAP));
            const int c = cuts ? __ffsll((long long)cuts) - 1 : m - 1;
            if (lane >= from && lane <= c) pre[base + j] = (uint16_t)(after - brt);
            const uint32_t bits = __shfl(after, c), n = count + c - from + 1;
            if (cuts) {
                write(j0 + c, n, bits);
                first = j0 + c + 1, count = 0, be = 0;
            } else {
                count = n, be = bits;
            }
            before = __shfl(incl, c);
            from = c + 1;
        }
        if (m < 64) {
            if (count) write(j0 + m - 1, count, be);
            return;
        }
    }
}

__global__ __launch_bounds__(256) void jpeg_prog_histogram_kernel(const int16_t* __restrict__ coef, PScript P, const uint16_t* __restrict__ run_n,
                                                                  unsigned long long* __restrict__ hist) {
    __shared__ uint32_t cnt[PSLOTS][256];
    const int lane = threadIdx.x & 63;
    const size_t f = blockIdx.y;
    for (int i = threadIdx.x; i < PSLOTS * 256; i += 256) (&cnt[0][0])[i] = 0;
    __syncthreads();
    const int16_t* fc = coef + f * P.nblk * 64;
    for (size_t u = (size_t)blockIdx.x * 4 + (threadIdx.x >> 6); u < P.seg.entries; u += (size_t)gridDim.x * 4) {
        size_t unit0;
        const PScan& sc = P.s[prog_scan_of(P, u, &unit0)];
        if (sc.slot < 0) continue;
        const uint32_t bi = (uint32_t)(u - unit0);
        if (sc.ss == 0) {
            int table;
            const int diff = prog_dc_difference(fc, P, bi, sc.al, &table);
            if (lane == 0) atomicAdd(&cnt[sc.slot + table][32 - __clz(diff < 0 ? -diff : diff)], 1u);
            continue;
        }
        const PLane L = prog_lane(lane, fc[prog_coef_block(P, sc.comp, bi) * 64 + lane], sc);
        if (L.fresh) atomicAdd(&cnt[sc.slot][L.sym], 1u);
        if (L.nzrl) atomicAdd(&cnt[sc.slot][0xf0], (uint32_t)L.nzrl);
        const uint32_t rn = run_n[f * P.seg.entries + u];
        if (lane == 0 && rn) atomicAdd(&cnt[sc.slot][(31 - __clz(rn)) << 4], 1u);
    }
    __syncthreads();
    for (int k = 0; k < P.nslots; ++k) {
        const uint32_t c = cnt[k][threadIdx.x];
        if (c) atomicAdd(&hist[(f * PSLOTS + k) * 256 + threadIdx.x], (unsigned long long)c);
    }
}

// count (EMIT false): body[unit] = the bits of the block's own symbols and of the correction bits among them; bits[unit] = that plus, where
// a run is written, its symbol, count bits and correction bits.  emit: the same lanes OR their bits into the scan's stream.
template <bool EMIT>
__global__ __launch_bounds__(256) void jpeg_prog_code_kernel(const int16_t* __restrict__ coef, PScript P, size_t total_units, const HuffSlot* __restrict__ huff,
                                                             const uint16_t* __restrict__ pre, const uint16_t* __restrict__ run_n, const uint16_t* __restrict__ run_be,
                                                             const uint32_t* __restrict__ run_end, uint32_t* __restrict__ body, uint32_t* __restrict__ bits,
                                                             const uint64_t* __restrict__ off, uint32_t* __restrict__ stream) {
    const size_t gw = (size_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (gw >= total_units) return;
    const int lane = threadIdx.x & 63;
    const size_t f = gw / P.seg.entries, u = gw - f * P.seg.entries;
    size_t unit0;
    const int scan = prog_scan_of(P, u, &unit0);
    const PScan& sc = P.s[scan];
    const uint32_t bi = (uint32_t)(u - unit0);
    const int16_t* fc = coef + f * P.nblk * 64;
    uint32_t* st = stream + f * P.seg.stream_words + P.seg.s[scan].word0;
    const HuffSlot* tab = huff + f * PSLOTS + max(sc.slot, 0);
    if (sc.ss == 0) {
        uint64_t pat;
        int len;
        if (sc.ah) {
            pat = (uint64_t)((prog_dc(fc, P, bi) >> sc.al) & 1), len = 1;
        } else {
            int table;
            const int diff = prog_dc_difference(fc, P, bi, sc.al, &table);
            const int size = 32 - __clz(diff < 0 ? -diff : diff);
            tab += table;
            pat = ((uint64_t)tab->code[size] << size) | ((uint32_t)(diff < 0 ? diff - 1 : diff) & ((1u << size) - 1));
            len = tab->len[size] + size;
        }
        if (lane) return;
        if (!EMIT) body[gw] = bits[gw] = (uint32_t)len;
        else if (pat) or_bits(st, off[gw], pat, len);
        return;
    }
    const PLane L = prog_lane(lane, fc[prog_coef_block(P, sc.comp, bi) * 64 + lane], sc);
    const int zl = tab->len[0xf0], cl = L.fresh ? tab->len[L.sym] : 0;
    const bool inside = L.old && L.flusher >= 0;          // its correction bit is among the block's symbols
    const int len = L.nzrl * zl + cl + L.size + (inside ? 1 : 0);
    int incl = len;
    for (int d = 1; d < 64; d <<= 1) {
        const int up = __shfl_up(incl, d);
        if (lane >= d) incl += up;
    }
    const int total = __shfl(incl, 63);
    const uint32_t rn = run_n[gw];
    const int rk = rn ? 31 - __clz(rn) : 0, rl = rn ? tab->len[rk << 4] + rk : 0;
    if (!EMIT) {
        if (lane == 0) body[gw] = (uint32_t)total, bits[gw] = (uint32_t)(total + (rn ? rl + run_be[gw] : 0));
        return;
    }
    const uint64_t at = off[gw];
    // The lanes in front of a flushing lane that wait for it hold one bit each, so its group starts `waiting` bits before its own place.
    // With ZRLs: the first ZRL, the waiting bits, then the rest; without: the symbol and value bits, then the waiting bits.
    const int mine = incl - len, group = mine - L.waiting;
    const int tail = group + (L.nzrl > 0 ? zl : cl + L.size);
    const int tail_of = __shfl(tail, max(L.flusher, 0));
    const uint64_t zc = tab->code[0xf0];
    if (L.nzrl > 0) or_bits(st, at + group, zc, zl);
    uint64_t pat = 0;
    int plen = 0;
    for (int k = 1; k < L.nzrl; ++k) pat = (pat << zl) | zc, plen += zl;
    if (L.fresh) pat = (((pat << cl) | tab->code[L.sym]) << L.size) | L.value, plen += cl + L.size;
    if (plen) or_bits(st, at + (L.nzrl > 0 ? mine + zl : group), pat, plen);
    if (L.old && L.corr) {
        uint64_t pos = at + tail_of + L.rank;
        if (!inside) {          // the tail of the run the block is in: behind its symbol and count bits, in block order
            const size_t e = gw - bi + run_end[gw];
            const int ek = 31 - __clz((uint32_t)run_n[e]);
            pos = off[e] + body[e] + tab->len[ek << 4] + ek + pre[gw] + L.rank;
        }
        or_bits(st, pos, 1, 1);
    }
    if (lane == 0 && rn) or_bits(st, at + total, ((uint64_t)tab->code[rk << 4] << rk) | (rn & ((1u << rk) - 1)), rl);
}

// What stands in front of a scan's data: the DHT segment of each of its tables (only the symbols that occur), then SOS
__device__ __forceinline__ int prog_scan_tables(const PScript& P, const PScan& sc) { return sc.slot < 0 ? 0 : sc.ss == 0 && P.c == 3 ? 2 : 1; }
__device__ __forceinline__ int prog_scan_components(const PScript& P, const PScan& sc) { return sc.comp < 0 ? P.c : 1; }
__device__ int prog_scan_header_len(const PScript& P, const PScan& sc, const HuffSlot* __restrict__ huff) {
    int len = 8 + 2 * prog_scan_components(P, sc);
    for (int t = 0; t < prog_scan_tables(P, sc); ++t) len += 4 + 1 + 16 + (int)huff[sc.slot + t].nvals;
    return len;
}
__device__ int prog_scan_header_byte(const PScript& P, const PScan& sc, const HuffSlot* __restrict__ huff, int j) {
    for (int t = 0; t < prog_scan_tables(P, sc); ++t) {
        const HuffSlot& k = huff[sc.slot + t];
        const int payload = 2 + 1 + 16 + (int)k.nvals;
        if (j < payload + 2)
            return j == 0 ? 0xff : j == 1 ? 0xc4 : j == 2 ? payload >> 8 : j == 3 ? payload & 255 : j == 4 ? (sc.ss ? 0x10 | (sc.comp > 0) : t)
                 : j < 21 ? k.bits[j - 5] : k.vals[j - 21];
        j -= payload + 2;
    }
    const int comps = prog_scan_components(P, sc);
    if (j < 5) return j == 0 ? 0xff : j == 1 ? 0xda : j == 2 ? 0 : j == 3 ? 6 + 2 * comps : comps;
    j -= 5;
    if (j < 2 * comps) {
        const int i = j >> 1;
        if (!(j & 1)) return sc.comp < 0 ? i + 1 : sc.comp + 1;
        return sc.ss ? (sc.comp > 0 ? 0x01 : 0x00) : (sc.ah == 0 && i > 0 ? 0x10 : 0x00);
    }
    j -= 2 * comps;
    return j == 0 ? sc.ss : j == 1 ? sc.se : (sc.ah << 4) | sc.al;
}

__global__ __launch_bounds__(256) void jpeg_prog_scatter_kernel(const uint32_t* __restrict__ stream, PScript P, const uint64_t* __restrict__ total_bits,
                                                                const uint32_t* __restrict__ ffoff, const uint32_t* __restrict__ fftotal, int h, int w, int quality,
                                                                int luma, const HuffSlot* __restrict__ huff, uint8_t* __restrict__ out, size_t out_stride,
                                                                int32_t* __restrict__ lengths) {
    __shared__ int part[4];
    __shared__ size_t seg_at[PSCANS], data_at[PSCANS + 1];          // where each scan's DHT / SOS and its data start; [nscans]: FFD9
    const size_t f = blockIdx.y;
    const int rgb = P.c == 3;
    huff += f * PSLOTS;
    uint8_t* file = out + f * out_stride;
    if (threadIdx.x == 0) {
        size_t at = T.dht[rgb];
        for (int k = 0; k < P.nscans; ++k) {
            seg_at[k] = at, at += prog_scan_header_len(P, P.s[k], huff);
            data_at[k] = at, at += stream_bytes(total_bits[f * PSCANS + k]) + fftotal[f * PSCANS + k];
        }
        data_at[P.nscans] = at;
    }
    __syncthreads();
    if (blockIdx.x == 0) {
        for (int i = threadIdx.x; i < T.dht[rgb]; i += 256)
            file[i] = i == T.sof_hw[rgb] - 4 ? 0xc2 : (uint8_t)header_byte<false>(i, rgb, h, w, quality, luma, nullptr, nullptr, 0);          // SOF2 for SOF0
        for (int k = 0; k < P.nscans; ++k)
            for (int j = threadIdx.x; j < (int)(data_at[k] - seg_at[k]); j += 256) file[seg_at[k] + j] = (uint8_t)prog_scan_header_byte(P, P.s[k], huff, j);
        if (threadIdx.x == 0) end_file(file, data_at[P.nscans], lengths + f);
    }
    const Segments& S = P.seg;
    for (int k = 0; k < P.nscans; ++k)
        stuffed_copy(stream + f * S.stream_words + S.s[k].word0, total_bits[f * PSCANS + k], ffoff + f * S.chunks + S.s[k].chunk0, file + data_at[k], part);
}

// ---- the round trip: coefficients -> pixels ---------------------------------------------------------------------------------------------
constexpr int MERGE_PX = 512;           // pixels of one output row per workgroup of the merge, 2 per lane

// The file's MCUs are 2 x 2 luma blocks (grey: one block); the n-frame arrays of the workspace are the coefficients, then the planes
struct RoundtripPlan {
    DecPlanes g;
    size_t o_coef, o_planes, total;     // workspace offsets (bytes)
};

RoundtripPlan make_roundtrip_plan(int n, int h, int w, int c) {
    RoundtripPlan p{};
    p.g = make_planes(h, w, c, c == 3 ? 2 : 1, c == 3 ? 2 : 1);
    Carve ws;
    p.o_coef = ws.take((size_t)n * p.g.nblk * 64 * sizeof(int16_t));
    p.o_planes = ws.take((size_t)n * p.g.stride);
    p.total = ws.at;
    return p;
}

// The IDCT stage on the transform's zigzag-ordered coefficients, dequantised by the tables of `quality`
__global__ __launch_bounds__(IDCT_PER_WG * 8) void jpeg_idct_kernel(const int16_t* __restrict__ coef, int quality, uint8_t* __restrict__ planes, DecPlanes g) {
    __shared__ int samp[IDCT_PER_WG * 72];
    __shared__ int q[128];
    if (threadIdx.x < 128) q[threadIdx.x] = quant_entry(threadIdx.x >> 6, threadIdx.x & 63, quality);
    __syncthreads();
    idct_blocks(coef, planes, g, samp, [&](int* sb, uint32_t v, int i, int comp) {
        const int* qt = q + (comp ? 64 : 0);
        const int n0 = T.zigzag[2 * i], n1 = T.zigzag[2 * i + 1];
        sb[(n0 >> 3) * 9 + (n0 & 7)] = (int)(int16_t)(v & 0xffff) * qt[n0];
        sb[(n1 >> 3) * 9 + (n1 & 7)] = (int)(int16_t)(v >> 16) * qt[n1];
    });
}

// C = 3: the pixels (x, x + 1) of row y from their luma samples and chroma column x / 2; C = 1: the luma samples themselves.
template <int C>
__global__ __launch_bounds__(MERGE_PX / 2) void jpeg_merge_kernel(const uint8_t* __restrict__ planes, DecPlanes g, int h, int w, uint8_t* __restrict__ dst) {
    constexpr int THREADS = MERGE_PX / 2;
    __shared__ __attribute__((aligned(4))) uint8_t seg[MERGE_PX * C + 8];           // the row segment, shifted by the destination's byte phase
    const int t = threadIdx.x, y = blockIdx.y, x0 = blockIdx.x * MERGE_PX, x = x0 + 2 * t;
    const uint8_t* fp = planes + (size_t)blockIdx.z * g.stride;
    uint8_t* d = dst + (((size_t)blockIdx.z * h + y) * w + x0) * C;
    const int sh = (int)((uintptr_t)d & 3), total = min(MERGE_PX, w - x0) * C;
    if (x < w) {
        const uint8_t* yp = fp + (size_t)y * g.yw + x;                              // x + 1 <= yw - 1: the plane has whole blocks
        const int y0 = yp[0], y1 = yp[1];
        uint8_t* o = seg + sh + 2 * t * C;
        if (C == 1) {
            o[0] = (uint8_t)y0, o[1] = (uint8_t)y1;
        } else {
            const int ch = (h + 1) >> 1, cw = (w + 1) >> 1, r = y >> 1, cc = x >> 1;
            int cb[2], cr[2];
            if (cw <= 2) {
                cb[0] = cb[1] = fp[g.o_cb + (size_t)r * g.cw + cc];
                cr[0] = cr[1] = fp[g.o_cr + (size_t)r * g.cw + cc];
            } else {
                const int rn = (y & 1) ? min(r + 1, ch - 1) : max(r - 1, 0), cl = max(cc - 1, 0), cn = min(cc + 1, cw - 1);
                const uint8_t* a = fp + (size_t)r * g.cw;
                const uint8_t* b = fp + (size_t)rn * g.cw;
#pragma unroll
                for (int k = 0; k < 2; ++k) {
                    const size_t o_k = k ? g.o_cr : g.o_cb;
                    const int s = h2v2_column(a + o_k, b + o_k, cc);
                    (k ? cr : cb)[0] = h2v2_sample(s, h2v2_column(a + o_k, b + o_k, cl), false);
                    (k ? cr : cb)[1] = h2v2_sample(s, h2v2_column(a + o_k, b + o_k, cn), true);
                }
            }
            ycc_to_rgb(y0, cb[0], cr[0], o);
            ycc_to_rgb(y1, cb[1], cr[1], o + 3);
        }
    }
    __syncthreads();
    // seg[sh .. sh + total) goes to d[0 .. total): dword j of seg is the aligned dword j from d - sh on
    uint8_t* base = d - sh;
    for (int j = t; j < (sh + total + 3) >> 2; j += THREADS) {
        const int lo = max(4 * j, sh), hi = min(4 * j + 4, sh + total);
        if (hi - lo == 4) {
            ((uint32_t*)base)[j] = ((const uint32_t*)seg)[j];
        } else {
            for (int i = lo; i < hi; ++i) base[i] = seg[i];
        }
    }
}

const char* check_shape(int n, int h, int w, int c, int quality) {
    if (n < 1) return "n < 1";
    if (c != 1 && c != 3) return "channels other than 1 (L) and 3 (RGB)";
    if (h < 1 || h > 65535 || w < 1 || w > 65535) return "height or width outside 1..65535";
    if (quality < 1 || quality > 100) return "quality outside 1..100";
    return nullptr;
}

const char* check_options(int sampling, int optimize) {
    if (sampling < 0 || sampling > 2) return "sampling outside 0 (4:4:4), 1 (4:2:2), 2 (4:2:0)";
    if (optimize < 0 || optimize > 1) return "optimize outside 0..1";
    return nullptr;
}

// The arguments of an encode call, or (quality nullptr) of its size query, as both kinds of file check and name them; the progressive
// entry has no optimize (nullptr)
struct EncodeArgs {
    const char* who;
    int n, h, w, c;
    const int* quality;
    int sampling;
    const int* optimize;
    const char* check() const {
        const char* bad = check_shape(n, h, w, c, quality ? *quality : 75);
        return bad ? bad : check_options(sampling, optimize ? *optimize : 0);
    }
    int refuse(const char* bad) const {
        char q[32] = "", o[32] = "";
        if (quality) snprintf(q, sizeof q, " quality %d,", *quality);
        if (optimize) snprintf(o, sizeof o, ", optimize %d", *optimize);
        set_error("%s: %s (n %d, %d x %d x %d,%s sampling %d%s)", who, bad, n, h, w, c, q, sampling, o);
        return ADAIN_EINVAL;
    }
};

// The size query of either kind of file; make_the_plan is called for checked arguments only
template <class MakeThePlan>
int encode_bytes(const EncodeArgs& a, MakeThePlan make_the_plan, size_t* out_stride, size_t* workspace_bytes) {
    if (const char* bad = a.check()) return a.refuse(bad);
    const auto p = make_the_plan();
    if (p.out_stride > (size_t)INT32_MAX) return a.refuse("a worst-case file beyond 2^31 - 1 bytes (lengths are int32)");
    if (out_stride) *out_stride = p.out_stride;
    if (workspace_bytes) *workspace_bytes = p.total;
    return 0;
}

// What either launcher holds the buffers of a call with checked arguments to, in this order.  entries: the plan's blocks (progressive:
// units) per frame, which count and emit give a wave each
template <class AnyPlan>
int check_encode_buffers(const EncodeArgs& a, const AnyPlan& p, size_t entries, size_t out_stride, const int32_t* lengths, const void* workspace,
                         size_t workspace_bytes) {
    if (p.out_stride > (size_t)INT32_MAX) { set_error("%s: %d x %d x %d: a worst-case file beyond 2^31 - 1 bytes", a.who, a.h, a.w, a.c); return ADAIN_EINVAL; }
    if (out_stride < p.out_stride) { set_error("%s: out_stride %zu below the %zu of the size query", a.who, out_stride, p.out_stride); return ADAIN_EINVAL; }
    if (int rc = check_workspace(a.who, workspace, workspace_bytes, p.total, 8)) return rc;
    if ((uintptr_t)lengths % 4) { set_error("%s: lengths must be 4-byte aligned", a.who); return ADAIN_EINVAL; }
    // gridDim.y and .z are limited to 65535: h, w <= 65535 keep the block rows below that; the frames ride in y or z
    if (a.n > 65535 || ((size_t)a.n * entries + 3) / 4 > 0x7fffffffull) { set_error("%s: batch of %d frames too large for one call", a.who, a.n); return ADAIN_EINVAL; }
    return 0;
}

// histogram (stage 0, optimize only), count (1) and emit (2) of one MCU layout
template <int HS, int VS>
void launch_entropy_stage(int stage, bool optimize, unsigned grid, int n, const int16_t* coef, uint32_t* bits, const uint64_t* off, uint32_t* stream,
                          size_t stream_words, const Geometry& g, size_t blocks, unsigned long long* hist, const HuffSlot* huff, hipStream_t s) {
    if (stage == 0) {
        jpeg_histogram_kernel<HS, VS><<<dim3(HIST_GRID, n), 256, 0, s>>>(coef, g, hist);
        return;
    }
    const auto code = stage == 1 ? (optimize ? jpeg_code_kernel<HS, VS, true, false> : jpeg_code_kernel<HS, VS, false, false>)
                                 : (optimize ? jpeg_code_kernel<HS, VS, true, true> : jpeg_code_kernel<HS, VS, false, true>);
    code<<<grid, 256, 0, s>>>(coef, g, blocks, huff, bits, off, stream, stream_words);
}

// The transform stage of a plan's layout
void launch_transform(const Plan& p, const uint8_t* src, int n, int h, int w, int c, int quality, int16_t* coef, hipStream_t s) {
    if (c != 3)
        jpeg_transform_grey_kernel<<<dim3((p.bw + GREY_PER_WG - 1) / GREY_PER_WG, p.bh, n), GREY_PER_WG * 8, 0, s>>>(src, h, w, quality, coef, p.bw, p.nblk);
    else if (p.vs == 2)
        jpeg_transform_rgb_kernel<<<dim3((p.mw + MCUS_PER_WG - 1) / MCUS_PER_WG, p.mh, n), MCUS_PER_WG * 48, 0, s>>>(src, h, w, quality, coef, p.mw, p.bw, p.bh, p.nblk);
    else if (p.hs == 2)
        jpeg_transform_rgb_h_kernel<2><<<dim3((p.mw + 7) / 8, p.mh, n), 256, 0, s>>>(src, h, w, quality, coef, p.mw, p.bw, p.nblk);
    else
        jpeg_transform_rgb_h_kernel<1><<<dim3((p.mw + 15) / 16, p.mh, n), 384, 0, s>>>(src, h, w, quality, coef, p.mw, p.bw, p.nblk);
}

// The back half's arrays in a call's workspace, at the offsets of its plan (of either kind), and its four launches: those that place the
// entries in the stream, in front of emit, and those that place the chunks in the file, behind it
struct BackHalf {
    uint32_t* bits;
    uint64_t *off, *total;
    uint32_t *stream, *ffcnt, *ffoff, *fftotal;
    template <class AnyPlan>
    BackHalf(char* ws, const AnyPlan& p)
        : bits((uint32_t*)(ws + p.o_bits)), off((uint64_t*)(ws + p.o_off)), total((uint64_t*)(ws + p.o_total)), stream((uint32_t*)(ws + p.o_stream)),
          ffcnt((uint32_t*)(ws + p.o_ffcnt)), ffoff((uint32_t*)(ws + p.o_ffoff)), fftotal((uint32_t*)(ws + p.o_fftotal)) {}
    void place_entries(const Segments& S, int n, hipStream_t s) const {
        jpeg_scan_kernel<uint32_t, uint64_t, false><<<dim3(S.count, n), SCAN_THREADS, 0, s>>>(bits, off, total, S, nullptr);
        jpeg_zero_kernel<<<dim3(STREAM_GRID, n), 256, 0, s>>>(stream, S, total);
    }
    void place_chunks(const Segments& S, int n, hipStream_t s) const {
        jpeg_ffcount_kernel<<<dim3(STREAM_GRID, n), 256, 0, s>>>(stream, S, total, ffcnt);
        jpeg_scan_kernel<uint32_t, uint32_t, true><<<dim3(S.count, n), SCAN_THREADS, 0, s>>>(ffcnt, ffoff, fftotal, S, total);
    }
};

}  // namespace

int jpeg_encode_bytes(const char* who, int n, int h, int w, int c, int sampling, int optimize, size_t* out_stride, size_t* workspace_bytes) {
    return encode_bytes({who, n, h, w, c, nullptr, sampling, &optimize}, [&] { return make_plan(n, h, w, c, sampling, optimize); }, out_stride, workspace_bytes);
}

int jpeg_encode_progressive_bytes(int n, int h, int w, int c, int sampling, size_t* out_stride, size_t* workspace_bytes) {
    return encode_bytes({"jpeg_encode_progressive_u8", n, h, w, c, nullptr, sampling, nullptr}, [&] { return make_prog_plan(n, h, w, c, sampling); }, out_stride,
                        workspace_bytes);
}

// sampling 2, optimize 0: the default file, in 8 launches.  Other samplings change the transform and the scan order only; optimize adds
// the clearing of the counters (a memset), the histogram and the table stage in front of count: 10 launches, whatever n.
int launch_jpeg_encode_u8(const char* who, const uint8_t* src, int n, int h, int w, int c, int quality, int sampling, int optimize, uint8_t* out,
                          size_t out_stride, int32_t* lengths, void* workspace, size_t workspace_bytes, hipStream_t s) {
    const EncodeArgs a{who, n, h, w, c, &quality, sampling, &optimize};
    if (const char* bad = a.check()) return a.refuse(bad);
    const Plan p = make_plan(n, h, w, c, sampling, optimize);
    if (int rc = check_encode_buffers(a, p, p.nblk, out_stride, lengths, workspace, workspace_bytes)) return rc;
    char* ws = (char*)workspace;
    int16_t* coef = (int16_t*)(ws + p.o_coef);
    const BackHalf b(ws, p);
    unsigned long long* hist = optimize ? (unsigned long long*)(ws + p.o_hist) : nullptr;
    HuffSlot* huff = optimize ? (HuffSlot*)(ws + p.o_huff) : nullptr;
    const Geometry g{c, p.mw, p.bw, p.bh, p.nblk};
    const size_t blocks = (size_t)n * p.nblk;
    launch_transform(p, src, n, h, w, c, quality, coef, s);
    auto entropy = [&](int stage) {
        const unsigned grid = (unsigned)((blocks + 3) / 4);
        if (p.vs == 2) launch_entropy_stage<2, 2>(stage, optimize, grid, n, coef, b.bits, b.off, b.stream, p.seg.stream_words, g, blocks, hist, huff, s);
        else if (p.hs == 2) launch_entropy_stage<2, 1>(stage, optimize, grid, n, coef, b.bits, b.off, b.stream, p.seg.stream_words, g, blocks, hist, huff, s);
        else launch_entropy_stage<1, 1>(stage, optimize, grid, n, coef, b.bits, b.off, b.stream, p.seg.stream_words, g, blocks, hist, huff, s);
    };
    if (optimize) {
        if (hipMemsetAsync(hist, 0, (size_t)n * SLOTS * 256 * sizeof(uint64_t), s) != hipSuccess) { set_error("%s: hipMemsetAsync failed", who); return ADAIN_EINVAL; }
        entropy(0);
        jpeg_table_kernel<<<dim3(c == 3 ? 4 : 2, n), TABLE_THREADS, 0, s>>>(hist, huff, SLOTS);
    }
    entropy(1);
    b.place_entries(p.seg, n, s);
    entropy(2);
    b.place_chunks(p.seg, n, s);
    const int luma = c == 3 ? p.hs << 4 | p.vs : 0x11;
    const auto scatter = optimize ? jpeg_scatter_kernel<true> : jpeg_scatter_kernel<false>;
    scatter<<<dim3(STREAM_GRID, n), 256, 0, s>>>(b.stream, p.seg.stream_words, b.total, b.ffoff, b.fftotal, p.seg.chunks, h, w, c == 3, quality, luma, huff, out,
                                                 out_stride, lengths);
    return check_launch(who);
}

// 13 launches and a memset, whatever n: transform; state, walk; histogram, table; count, scan, zero, emit; ffcount, scan, scatter
int launch_jpeg_encode_progressive_u8(const uint8_t* src, int n, int h, int w, int c, int quality, int sampling, uint8_t* out, size_t out_stride, int32_t* lengths,
                                      void* workspace, size_t workspace_bytes, hipStream_t s) {
    const char* who = "jpeg_encode_progressive_u8";
    const EncodeArgs a{who, n, h, w, c, &quality, sampling, nullptr};
    if (const char* bad = a.check()) return a.refuse(bad);
    const ProgPlan p = make_prog_plan(n, h, w, c, sampling);
    const PScript& P = p.P;
    if (int rc = check_encode_buffers(a, p, P.seg.entries, out_stride, lengths, workspace, workspace_bytes)) return rc;
    const size_t units = (size_t)n * P.seg.entries;
    char* ws = (char*)workspace;
    int16_t* coef = (int16_t*)(ws + p.o_coef);
    uint8_t* state = (uint8_t*)(ws + p.o_state);
    uint16_t* pre = (uint16_t*)(ws + p.o_pre);
    uint16_t* run_n = (uint16_t*)(ws + p.o_run_n);
    uint16_t* run_be = (uint16_t*)(ws + p.o_run_be);
    uint32_t* run_end = (uint32_t*)(ws + p.o_run_end);
    uint32_t* body = (uint32_t*)(ws + p.o_body);
    const BackHalf b(ws, p);
    unsigned long long* hist = (unsigned long long*)(ws + p.o_hist);
    HuffSlot* huff = (HuffSlot*)(ws + p.o_huff);
    launch_transform(p.base, src, n, h, w, c, quality, coef, s);
    if (hipMemsetAsync(hist, 0, (size_t)n * PSLOTS * 256 * sizeof(uint64_t), s) != hipSuccess) { set_error("%s: hipMemsetAsync failed", who); return ADAIN_EINVAL; }
    const unsigned waves = (unsigned)((units + 3) / 4);
    jpeg_prog_state_kernel<<<waves, 256, 0, s>>>(coef, P, units, state, run_n);
    jpeg_prog_walk_kernel<<<waves, 256, 0, s>>>(P, units, state, pre, run_n, run_be, run_end);
    jpeg_prog_histogram_kernel<<<dim3(HIST_GRID, n), 256, 0, s>>>(coef, P, run_n, hist);
    jpeg_table_kernel<<<dim3(P.nslots, n), TABLE_THREADS, 0, s>>>(hist, huff, PSLOTS);
    jpeg_prog_code_kernel<false><<<waves, 256, 0, s>>>(coef, P, units, huff, pre, run_n, run_be, run_end, body, b.bits, b.off, b.stream);
    b.place_entries(P.seg, n, s);
    jpeg_prog_code_kernel<true><<<waves, 256, 0, s>>>(coef, P, units, huff, pre, run_n, run_be, run_end, body, b.bits, b.off, b.stream);
    b.place_chunks(P.seg, n, s);
    const int luma = c == 3 ? P.hs << 4 | P.vs : 0x11;
    jpeg_prog_scatter_kernel<<<dim3(STREAM_GRID, n), 256, 0, s>>>(b.stream, P, b.total, b.ffoff, b.fftotal, h, w, quality, luma, huff, out, out_stride, lengths);
    return check_launch(who);
}

int jpeg_roundtrip_bytes(int n, int h, int w, int c, size_t* workspace_bytes) {
    const char* bad = check_shape(n, h, w, c, 75);
    if (bad) { set_error("jpeg_roundtrip_u8: %s (n %d, %d x %d x %d)", bad, n, h, w, c); return ADAIN_EINVAL; }
    if (workspace_bytes) *workspace_bytes = make_roundtrip_plan(n, h, w, c).total;
    return 0;
}

int launch_jpeg_roundtrip_u8(const uint8_t* src, int n, int h, int w, int c, int quality, uint8_t* dst, void* workspace, size_t workspace_bytes, hipStream_t s) {
    const char* bad = check_shape(n, h, w, c, quality);
    if (bad) { set_error("jpeg_roundtrip_u8: %s (n %d, %d x %d x %d, quality %d)", bad, n, h, w, c, quality); return ADAIN_EINVAL; }
    const RoundtripPlan p = make_roundtrip_plan(n, h, w, c);
    if (int rc = check_workspace("jpeg_roundtrip_u8", workspace, workspace_bytes, p.total, 8)) return rc;
    const DecPlanes& g = p.g;
    // gridDim.y and .z are limited to 65535: h <= 65535 keeps the rows below that; the frames ride in y (idct) and z (transform, merge)
    if (n > 65535 || (g.nblk + IDCT_PER_WG - 1) / IDCT_PER_WG > 0x7fffffffull) { set_error("jpeg_roundtrip_u8: batch of %d frames too large for one call", n); return ADAIN_EINVAL; }
    int16_t* coef = (int16_t*)((char*)workspace + p.o_coef);
    uint8_t* planes = (uint8_t*)workspace + p.o_planes;
    launch_transform(make_plan(n, h, w, c), src, n, h, w, c, quality, coef, s);          // the default file's layout: g's blocks
    jpeg_idct_kernel<<<dim3((unsigned)((g.nblk + IDCT_PER_WG - 1) / IDCT_PER_WG), n), IDCT_PER_WG * 8, 0, s>>>(coef, quality, planes, g);
    const dim3 grid((w + MERGE_PX - 1) / MERGE_PX, h, n);
    if (c == 3)
        jpeg_merge_kernel<3><<<grid, MERGE_PX / 2, 0, s>>>(planes, g, h, w, dst);
    else
        jpeg_merge_kernel<1><<<grid, MERGE_PX / 2, 0, s>>>(planes, g, h, w, dst);
    return check_launch("jpeg_roundtrip_u8");
}

}  // namespace adain
