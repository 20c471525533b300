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
//   scan       exclusive scan of the blocks' bit counts per frame (64-bit offsets)
//   zero       the words of the bit stream the frame will use
//   emit       each lane ORs its ZRLs, code and value bits into the big-endian bit stream at block offset + in-block prefix; the bits of
//              different lanes are disjoint, so atomicOr on 32-bit words is order-independent
//   ffcount / scan / scatter   0xFF bytes per 1024-byte chunk, their scan, and the copy behind the header with a 0x00 after each 0xFF;
//              the scatter also writes the header, FFD9 and lengths[i]
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

// ---- sizes -----------------------------------------------------------------------------------------------------------------------------
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
    size_t stream_words;          // words of one frame's bit stream
    size_t chunks;                // CHUNK-byte pieces of max_bytes
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
    p.stream_words = (p.max_bytes + 3) / 4 + 4;
    p.chunks = (p.max_bytes + CHUNK - 1) / CHUNK;
    p.out_stride = HOST_T.hdr_len[c == 3] + 2 * p.max_bytes + 2;
    const size_t N = (size_t)n;
    Carve ws;
    p.o_coef = ws.take(N * p.nblk * 64 * sizeof(int16_t));
    p.o_bits = ws.take(N * p.nblk * sizeof(uint32_t));
    p.o_off = ws.take(N * p.nblk * sizeof(uint64_t));
    p.o_total = ws.take(N * sizeof(uint64_t));
    p.o_stream = ws.take(N * p.stream_words * sizeof(uint32_t));
    p.o_ffcnt = ws.take(N * p.chunks * sizeof(uint32_t));
    p.o_ffoff = ws.take(N * p.chunks * sizeof(uint32_t));
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

template <int HS, int VS, bool OPT>
__global__ __launch_bounds__(256) void jpeg_count_kernel(const int16_t* __restrict__ coef, uint32_t* __restrict__ bits, Geometry g, size_t total_blocks,
                                                         const HuffSlot* __restrict__ huff) {
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
    int len = lane_bits<OPT>(lane, v, table, huff + f * SLOTS, &pat, &zrl, &zrl_len);
    len += zrl_len;
    for (int d = 32; d >= 1; d >>= 1) len += __shfl_xor(len, d);
    if (lane == 0) bits[gw] = (uint32_t)len;
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

template <int HS, int VS, bool OPT>
__global__ __launch_bounds__(256) void jpeg_emit_kernel(const int16_t* __restrict__ coef, const uint64_t* __restrict__ off, uint32_t* __restrict__ stream,
                                                        size_t stream_words, Geometry g, size_t total_blocks, const HuffSlot* __restrict__ huff) {
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

__global__ __launch_bounds__(TABLE_THREADS) void jpeg_table_kernel(const unsigned long long* __restrict__ hist, HuffSlot* __restrict__ huff) {
    __shared__ Least part[2][TABLE_THREADS / 64];
    __shared__ int size_of[256];                // the unrestricted code length per symbol
    __shared__ int bits[260];                   // symbols per code length; a chain of 257 symbols is at most 256 deep
    __shared__ int first[18], upto[18];         // per length 1..16: its first code; the symbols of shorter-or-equal length
    const int t = threadIdx.x;
    const size_t slot = (size_t)blockIdx.y * SLOTS + blockIdx.x;
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

// ---- scans: one workgroup per frame ------------------------------------------------------------------------------------------------------
__device__ __forceinline__ size_t stream_bytes(uint64_t bits) { return (size_t)((bits + 7) >> 3); }
__device__ __forceinline__ size_t stream_chunks(uint64_t bits) { return (stream_bytes(bits) + CHUNK - 1) / CHUNK; }

// out[i] = in[0] + ... + in[i - 1] over a frame's `count` entries (count_bits != nullptr: the chunks of that many coded bits), the sum to total[frame]
template <class In, class Out>
__global__ __launch_bounds__(SCAN_THREADS) void jpeg_scan_kernel(const In* __restrict__ in, Out* __restrict__ out, Out* __restrict__ total, size_t stride, size_t count,
                                                                 const uint64_t* __restrict__ count_bits) {
    __shared__ Out part[SCAN_THREADS];
    const int t = threadIdx.x;
    const size_t f = blockIdx.x;
    if (count_bits) count = stream_chunks(count_bits[f]);
    in += f * stride, out += f * stride;
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
    if (t == SCAN_THREADS - 1) total[f] = part[t];
}

__global__ __launch_bounds__(256) void jpeg_zero_kernel(uint32_t* __restrict__ stream, size_t stream_words, const uint64_t* __restrict__ total_bits) {
    const size_t f = blockIdx.y;
    const size_t words = (size_t)((total_bits[f] + 31) >> 5) + 2;           // <= stream_words: the plan keeps 4 beyond the bound
    uint32_t* s = stream + f * stream_words;
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < words; i += (size_t)gridDim.x * 256) s[i] = 0;
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

__global__ __launch_bounds__(256) void jpeg_ffcount_kernel(const uint32_t* __restrict__ stream, size_t stream_words, const uint64_t* __restrict__ total_bits,
                                                           uint32_t* __restrict__ ffcnt, size_t chunks) {
    __shared__ int part[4];
    const size_t f = blockIdx.y;
    const uint64_t bits = total_bits[f];
    const uint32_t* s = stream + f * stream_words;
    for (size_t ck = blockIdx.x; ck < stream_chunks(bits); ck += gridDim.x) {
        int valid;
        const uint32_t v = stream_word(s, ck * (CHUNK / 4) + threadIdx.x, bits, &valid);
        const int incl = workgroup_inclusive(count_ff(v, valid), part);
        if (threadIdx.x == 255) ffcnt[f * chunks + ck] = (uint32_t)incl;
    }
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

template <bool OPT>
__global__ __launch_bounds__(256) void jpeg_scatter_kernel(const uint32_t* __restrict__ stream, size_t stream_words, const uint64_t* __restrict__ total_bits,
                                                           const uint32_t* __restrict__ ffoff, const uint32_t* __restrict__ fftotal, size_t chunks, int h, int w,
                                                           int rgb, int quality, int luma, const HuffSlot* __restrict__ huff, uint8_t* __restrict__ out,
                                                           size_t out_stride, int32_t* __restrict__ lengths) {
    __shared__ int part[4];
    const size_t f = blockIdx.y;
    const uint64_t bits = total_bits[f];
    const uint32_t* s = stream + f * stream_words;
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
        if (threadIdx.x == 0) {
            const size_t end = hdr + stream_bytes(bits) + fftotal[f];
            file[end] = 0xff, file[end + 1] = 0xd9;
            lengths[f] = (int32_t)(end + 2);
        }
    }
    for (size_t ck = blockIdx.x; ck < stream_chunks(bits); ck += gridDim.x) {
        int valid;
        const uint32_t v = stream_word(s, ck * (CHUNK / 4) + threadIdx.x, bits, &valid);
        const int c = count_ff(v, valid);
        const int before = workgroup_inclusive(c, part) - c;
        uint8_t* d = file + hdr + ck * CHUNK + ffoff[f * chunks + ck] + threadIdx.x * 4 + before;
        for (int k = 0; k < valid; ++k) {
            const uint8_t byte = (uint8_t)(v >> (24 - 8 * k));
            *d++ = byte;
            if (byte == 255) *d++ = 0;
        }
    }
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

}  // namespace

int jpeg_encode_bytes(const char* who, int n, int h, int w, int c, int sampling, int optimize, size_t* out_stride, size_t* workspace_bytes) {
    const char* bad = check_shape(n, h, w, c, 75);
    if (!bad) bad = check_options(sampling, optimize);
    if (!bad && make_plan(n, h, w, c, sampling, optimize).out_stride > (size_t)INT32_MAX) bad = "a worst-case file beyond 2^31 - 1 bytes (lengths are int32)";
    if (bad) { set_error("%s: %s (n %d, %d x %d x %d, sampling %d, optimize %d)", who, bad, n, h, w, c, sampling, optimize); return ADAIN_EINVAL; }
    const Plan p = make_plan(n, h, w, c, sampling, optimize);
    if (out_stride) *out_stride = p.out_stride;
    if (workspace_bytes) *workspace_bytes = p.total;
    return 0;
}

namespace {

// count, (optimize) histogram and emit of one MCU layout
template <int HS, int VS>
void launch_entropy_stage(int stage, bool optimize, unsigned grid, int n, const int16_t* coef, uint32_t* bits, const uint64_t* off, uint32_t* stream,
                          size_t stream_words, const Geometry& g, size_t blocks, unsigned long long* hist, const HuffSlot* huff, hipStream_t s) {
    if (stage == 0)
        jpeg_histogram_kernel<HS, VS><<<dim3(HIST_GRID, n), 256, 0, s>>>(coef, g, hist);
    else if (stage == 1 && optimize)
        jpeg_count_kernel<HS, VS, true><<<grid, 256, 0, s>>>(coef, bits, g, blocks, huff);
    else if (stage == 1)
        jpeg_count_kernel<HS, VS, false><<<grid, 256, 0, s>>>(coef, bits, g, blocks, huff);
    else if (optimize)
        jpeg_emit_kernel<HS, VS, true><<<grid, 256, 0, s>>>(coef, off, stream, stream_words, g, blocks, huff);
    else
        jpeg_emit_kernel<HS, VS, false><<<grid, 256, 0, s>>>(coef, off, stream, stream_words, g, blocks, huff);
}

}  // namespace

// sampling 2, optimize 0: the default file, in 8 launches.  Other samplings change the transform and the scan order only; optimize adds
// the clearing of the counters (a memset), the histogram and the table stage in front of count: 10 launches, whatever n.
int launch_jpeg_encode_u8(const char* who, const uint8_t* src, int n, int h, int w, int c, int quality, int sampling, int optimize, uint8_t* out,
                          size_t out_stride, int32_t* lengths, void* workspace, size_t workspace_bytes, hipStream_t s) {
    const char* bad = check_shape(n, h, w, c, quality);
    if (!bad) bad = check_options(sampling, optimize);
    if (bad) { set_error("%s: %s (n %d, %d x %d x %d, quality %d, sampling %d, optimize %d)", who, bad, n, h, w, c, quality, sampling, optimize); return ADAIN_EINVAL; }
    const Plan p = make_plan(n, h, w, c, sampling, optimize);
    if (p.out_stride > (size_t)INT32_MAX) { set_error("%s: %d x %d x %d: a worst-case file beyond 2^31 - 1 bytes", who, h, w, c); return ADAIN_EINVAL; }
    if (out_stride < p.out_stride) { set_error("%s: out_stride %zu below the %zu of the size query", who, out_stride, p.out_stride); return ADAIN_EINVAL; }
    if (int rc = check_workspace(who, workspace, workspace_bytes, p.total, 8)) return rc;
    if ((uintptr_t)lengths % 4) { set_error("%s: lengths must be 4-byte aligned", who); return ADAIN_EINVAL; }
    char* ws = (char*)workspace;
    int16_t* coef = (int16_t*)(ws + p.o_coef);
    uint32_t* bits = (uint32_t*)(ws + p.o_bits);
    uint64_t* off = (uint64_t*)(ws + p.o_off);
    uint64_t* total = (uint64_t*)(ws + p.o_total);
    uint32_t* stream = (uint32_t*)(ws + p.o_stream);
    uint32_t* ffcnt = (uint32_t*)(ws + p.o_ffcnt);
    uint32_t* ffoff = (uint32_t*)(ws + p.o_ffoff);
    uint32_t* fftotal = (uint32_t*)(ws + p.o_fftotal);
    unsigned long long* hist = optimize ? (unsigned long long*)(ws + p.o_hist) : nullptr;
    HuffSlot* huff = optimize ? (HuffSlot*)(ws + p.o_huff) : nullptr;
    const Geometry g{c, p.mw, p.bw, p.bh, p.nblk};
    const size_t blocks = (size_t)n * p.nblk;
    // gridDim.y and .z are limited to 65535: h, w <= 65535 keep the block rows below that; the frames ride in z
    if (n > 65535 || (blocks + 3) / 4 > 0x7fffffffull) { set_error("%s: batch of %d frames too large for one call", who, n); return ADAIN_EINVAL; }
    if (c != 3)
        jpeg_transform_grey_kernel<<<dim3((p.bw + GREY_PER_WG - 1) / GREY_PER_WG, p.bh, n), GREY_PER_WG * 8, 0, s>>>(src, h, w, quality, coef, p.bw, p.nblk);
    else if (p.vs == 2)
        jpeg_transform_rgb_kernel<<<dim3((p.mw + MCUS_PER_WG - 1) / MCUS_PER_WG, p.mh, n), MCUS_PER_WG * 48, 0, s>>>(src, h, w, quality, coef, p.mw, p.bw, p.bh, p.nblk);
    else if (p.hs == 2)
        jpeg_transform_rgb_h_kernel<2><<<dim3((p.mw + 7) / 8, p.mh, n), 256, 0, s>>>(src, h, w, quality, coef, p.mw, p.bw, p.nblk);
    else
        jpeg_transform_rgb_h_kernel<1><<<dim3((p.mw + 15) / 16, p.mh, n), 384, 0, s>>>(src, h, w, quality, coef, p.mw, p.bw, p.nblk);
    auto entropy = [&](int stage) {
        const unsigned grid = (unsigned)((blocks + 3) / 4);
        if (p.vs == 2) launch_entropy_stage<2, 2>(stage, optimize, grid, n, coef, bits, off, stream, p.stream_words, g, blocks, hist, huff, s);
        else if (p.hs == 2) launch_entropy_stage<2, 1>(stage, optimize, grid, n, coef, bits, off, stream, p.stream_words, g, blocks, hist, huff, s);
        else launch_entropy_stage<1, 1>(stage, optimize, grid, n, coef, bits, off, stream, p.stream_words, g, blocks, hist, huff, s);
    };
    if (optimize) {
        if (hipMemsetAsync(hist, 0, (size_t)n * SLOTS * 256 * sizeof(uint64_t), s) != hipSuccess) { set_error("%s: hipMemsetAsync failed", who); return ADAIN_EINVAL; }
        entropy(0);
        jpeg_table_kernel<<<dim3(c == 3 ? 4 : 2, n), TABLE_THREADS, 0, s>>>(hist, huff);
    }
    entropy(1);
    jpeg_scan_kernel<uint32_t, uint64_t><<<n, SCAN_THREADS, 0, s>>>(bits, off, total, p.nblk, p.nblk, nullptr);
    jpeg_zero_kernel<<<dim3(STREAM_GRID, n), 256, 0, s>>>(stream, p.stream_words, total);
    entropy(2);
    jpeg_ffcount_kernel<<<dim3(STREAM_GRID, n), 256, 0, s>>>(stream, p.stream_words, total, ffcnt, p.chunks);
    jpeg_scan_kernel<uint32_t, uint32_t><<<n, SCAN_THREADS, 0, s>>>(ffcnt, ffoff, fftotal, p.chunks, 0, total);
    const int luma = c == 3 ? p.hs << 4 | p.vs : 0x11;
    if (optimize)
        jpeg_scatter_kernel<true><<<dim3(STREAM_GRID, n), 256, 0, s>>>(stream, p.stream_words, total, ffoff, fftotal, p.chunks, h, w, c == 3, quality, luma, huff, out, out_stride, lengths);
    else
        jpeg_scatter_kernel<false><<<dim3(STREAM_GRID, n), 256, 0, s>>>(stream, p.stream_words, total, ffoff, fftotal, p.chunks, h, w, c == 3, quality, luma, huff, out, out_stride, lengths);
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
    const int bw = (w + 7) / 8, bh = (h + 7) / 8;
    // gridDim.y and .z are limited to 65535: h <= 65535 keeps the rows below that; the frames ride in y (idct) and z (transform, merge)
    if (n > 65535 || (g.nblk + IDCT_PER_WG - 1) / IDCT_PER_WG > 0x7fffffffull) { set_error("jpeg_roundtrip_u8: batch of %d frames too large for one call", n); return ADAIN_EINVAL; }
    int16_t* coef = (int16_t*)((char*)workspace + p.o_coef);
    uint8_t* planes = (uint8_t*)workspace + p.o_planes;
    if (c == 3)
        jpeg_transform_rgb_kernel<<<dim3((g.mw + MCUS_PER_WG - 1) / MCUS_PER_WG, g.mh, n), MCUS_PER_WG * 48, 0, s>>>(src, h, w, quality, coef, g.mw, bw, bh, g.nblk);
    else
        jpeg_transform_grey_kernel<<<dim3((bw + GREY_PER_WG - 1) / GREY_PER_WG, bh, n), GREY_PER_WG * 8, 0, s>>>(src, h, w, quality, coef, bw, g.nblk);
    jpeg_idct_kernel<<<dim3((unsigned)((g.nblk + IDCT_PER_WG - 1) / IDCT_PER_WG), n), IDCT_PER_WG * 8, 0, s>>>(coef, quality, planes, g);
    const dim3 grid((w + MERGE_PX - 1) / MERGE_PX, h, n);
    if (c == 3)
        jpeg_merge_kernel<3><<<grid, MERGE_PX / 2, 0, s>>>(planes, g, h, w, dst);
    else
        jpeg_merge_kernel<1><<<grid, MERGE_PX / 2, 0, s>>>(planes, g, h, w, dst);
    return check_launch("jpeg_roundtrip_u8");
}

}  // namespace adain
