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
// The file decoder (adain_jpeg_decode_u8, adain_jpeg_decode_restart_u8): a baseline file's entropy-coded segment -> the pixels Pillow decodes from the file.  Its rule list
// and its stages stand in front of its kernels below ("the file decoder"); in short
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
// script -> the same coefficient buffer, then the file decoder's back half unchanged.  Its rules, stages and launches per call stand in
// front of its kernels below ("the progressive file decoder"); in short: every scan's segment is unstuffed on its own, the scans apply in
// file order, every Huffman-coded scan goes through the fixed-point scheme above with a state of its kind, a DC refinement is one lane
// per block, and an AC refinement's state carries the block it is in because the bits a block takes depend on the coefficients before it
#include "common.h"

namespace adain {
namespace {

constexpr int MCUS_PER_WG = 8;          // RGB: 8 MCUs = 128 x 16 pixels = 48 blocks, 384 threads (one per block row)
constexpr int GREY_PER_WG = 32;         // L: 32 blocks = 256 x 8 pixels, 256 threads
constexpr int CHUNK = 1024;             // bytes of entropy-coded data per workgroup pass of the stuffing kernels (one word per thread)
constexpr int SCAN_THREADS = 1024;
constexpr int STREAM_GRID = 64;         // workgroups per frame of the grid-stride kernels (zero, ffcount, scatter)

struct Huff {
    uint16_t dc_code[2][12];
    uint8_t dc_len[2][12];
    uint16_t ac_code[2][256];
    uint8_t ac_len[2][256];
};
struct Tables {
    uint8_t zigzag[64];      // zigzag position -> natural index
    uint8_t zpos[64];        // natural index -> zigzag position
    uint8_t qbase[2][64];    // Annex K.1, natural order
    Huff huff;
    uint8_t hdr[2][640];     // [0]: greyscale, [1]: RGB; the DQT entries and SOF0's size are left 0
    int hdr_len[2], dqt[2][2], sof_hw[2];       // offsets of the 64 DQT entries per table and of SOF0's height
    int sof_luma[2], dht[2], sos[2];            // offsets of SOF0's luma sampling byte, of the first DHT and of SOS
    int max_block_bits;
};

constexpr uint8_t DC_BITS[2][16] = {{0, 1, 5, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0, 0, 0}, {0, 3, 1, 1, 1, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0}};
constexpr uint8_t AC_BITS[2][16] = {{0, 2, 1, 3, 3, 2, 4, 3, 5, 5, 4, 4, 0, 0, 1, 0x7d}, {0, 2, 1, 2, 4, 4, 3, 4, 7, 5, 4, 4, 0, 1, 2, 0x77}};
constexpr uint8_t AC_VALS[2][162] = {
    {0x01, 0x02, 0x03, 0x00, 0x04, 0x11, 0x05, 0x12, 0x21, 0x31, 0x41, 0x06, 0x13, 0x51, 0x61, 0x07, 0x22, 0x71, 0x14, 0x32, 0x81, 0x91, 0xa1,
     0x08, 0x23, 0x42, 0xb1, 0xc1, 0x15, 0x52, 0xd1, 0xf0, 0x24, 0x33, 0x62, 0x72, 0x82, 0x09, 0x0a, 0x16, 0x17, 0x18, 0x19, 0x1a, 0x25, 0x26,
     0x27, 0x28, 0x29, 0x2a, 0x34, 0x35, 0x36, 0x37, 0x38, 0x39, 0x3a, 0x43, 0x44, 0x45, 0x46, 0x47, 0x48, 0x49, 0x4a, 0x53, 0x54, 0x55, 0x56,
     0x57, 0x58, 0x59, 0x5a, 0x63, 0x64, 0x65, 0x66, 0x67, 0x68, 0x69, 0x6a, 0x73, 0x74, 0x75, 0x76, 0x77, 0x78, 0x79, 0x7a, 0x83, 0x84, 0x85,
     0x86, 0x87, 0x88, 0x89, 0x8a, 0x92, 0x93, 0x94, 0x95, 0x96, 0x97, 0x98, 0x99, 0x9a, 0xa2, 0xa3, 0xa4, 0xa5, 0xa6, 0xa7, 0xa8, 0xa9, 0xaa,
     0xb2, 0xb3, 0xb4, 0xb5, 0xb6, 0xb7, 0xb8, 0xb9, 0xba, 0xc2, 0xc3, 0xc4, 0xc5, 0xc6, 0xc7, 0xc8, 0xc9, 0xca, 0xd2, 0xd3, 0xd4, 0xd5, 0xd6,
     0xd7, 0xd8, 0xd9, 0xda, 0xe1, 0xe2, 0xe3, 0xe4, 0xe5, 0xe6, 0xe7, 0xe8, 0xe9, 0xea, 0xf1, 0xf2, 0xf3, 0xf4, 0xf5, 0xf6, 0xf7, 0xf8, 0xf9,
     0xfa},
    {0x00, 0x01, 0x02, 0x03, 0x11, 0x04, 0x05, 0x21, 0x31, 0x06, 0x12, 0x41, 0x51, 0x07, 0x61, 0x71, 0x13, 0x22, 0x32, 0x81, 0x08, 0x14, 0x42,
     0x91, 0xa1, 0xb1, 0xc1, 0x09, 0x23, 0x33, 0x52, 0xf0, 0x15, 0x62, 0x72, 0xd1, 0x0a, 0x16, 0x24, 0x34, 0xe1, 0x25, 0xf1, 0x17, 0x18, 0x19,
     0x1a, 0x26, 0x27, 0x28, 0x29, 0x2a, 0x35, 0x36, 0x37, 0x38, 0x39, 0x3a, 0x43, 0x44, 0x45, 0x46, 0x47, 0x48, 0x49, 0x4a, 0x53, 0x54, 0x55,
     0x56, 0x57, 0x58, 0x59, 0x5a, 0x63, 0x64, 0x65, 0x66, 0x67, 0x68, 0x69, 0x6a, 0x73, 0x74, 0x75, 0x76, 0x77, 0x78, 0x79, 0x7a, 0x82, 0x83,
     0x84, 0x85, 0x86, 0x87, 0x88, 0x89, 0x8a, 0x92, 0x93, 0x94, 0x95, 0x96, 0x97, 0x98, 0x99, 0x9a, 0xa2, 0xa3, 0xa4, 0xa5, 0xa6, 0xa7, 0xa8,
     0xa9, 0xaa, 0xb2, 0xb3, 0xb4, 0xb5, 0xb6, 0xb7, 0xb8, 0xb9, 0xba, 0xc2, 0xc3, 0xc4, 0xc5, 0xc6, 0xc7, 0xc8, 0xc9, 0xca, 0xd2, 0xd3, 0xd4,
     0xd5, 0xd6, 0xd7, 0xd8, 0xd9, 0xda, 0xe2, 0xe3, 0xe4, 0xe5, 0xe6, 0xe7, 0xe8, 0xe9, 0xea, 0xf2, 0xf3, 0xf4, 0xf5, 0xf6, 0xf7, 0xf8, 0xf9,
     0xfa}};

constexpr Tables make_tables() {
    Tables t{};
    const uint8_t zz[64] = {0,  1,  8,  16, 9,  2,  3,  10, 17, 24, 32, 25, 18, 11, 4,  5,  12, 19, 26, 33, 40, 48, 41, 34, 27, 20, 13, 6,  7,  14, 21, 28,
                            35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23, 30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63};
    const uint8_t ql[64] = {16, 11, 10, 16, 24, 40, 51, 61, 12, 12, 14, 19, 26, 58,  60,  55, 14, 13, 16, 24, 40,  57,  69,  56,  14, 17, 22, 29, 51,  87,  80,  62,
                            18, 22, 37, 56, 68, 109, 103, 77, 24, 35, 55, 64, 81, 104, 113, 92, 49, 64, 78, 87, 103, 121, 120, 101, 72, 92, 95, 98, 112, 100, 103, 99};
    const uint8_t qc[32] = {17, 18, 24, 47, 99, 99, 99, 99, 18, 21, 26, 66, 99, 99, 99, 99, 24, 26, 56, 99, 99, 99, 99, 99, 47, 66, 99, 99, 99, 99, 99, 99};
    for (int i = 0; i < 64; ++i) {
        t.zigzag[i] = zz[i];
        t.zpos[zz[i]] = (uint8_t)i;
        t.qbase[0][i] = ql[i];
        t.qbase[1][i] = i < 32 ? qc[i] : 99;
    }
    for (int k = 0; k < 2; ++k) {
        int code = 0, at = 0;
        for (int len = 1; len <= 16; ++len) {
            for (int i = 0; i < DC_BITS[k][len - 1]; ++i, ++at, ++code) { t.huff.dc_code[k][at] = (uint16_t)code; t.huff.dc_len[k][at] = (uint8_t)len; }
            code <<= 1;
        }
        code = 0, at = 0;
        for (int len = 1; len <= 16; ++len) {
            for (int i = 0; i < AC_BITS[k][len - 1]; ++i, ++at, ++code) { t.huff.ac_code[k][AC_VALS[k][at]] = (uint16_t)code; t.huff.ac_len[k][AC_VALS[k][at]] = (uint8_t)len; }
            code <<= 1;
        }
    }
    // the most bits one block can emit: an 11-bit DC difference and 63 AC coefficients of 10 bits, each with the longest code of its kind
    int dc = 0, ac = 0;
    for (int k = 0; k < 2; ++k) {
        for (int s = 0; s < 12; ++s) dc = t.huff.dc_len[k][s] + s > dc ? t.huff.dc_len[k][s] + s : dc;
        for (int r = 0; r < 16; ++r)
            for (int s = 1; s <= 10; ++s) ac = t.huff.ac_len[k][r * 16 + s] + s > ac ? t.huff.ac_len[k][r * 16 + s] + s : ac;
    }
    t.max_block_bits = dc + 63 * ac;
    for (int rgb = 0; rgb < 2; ++rgb) {
        uint8_t* b = t.hdr[rgb];
        int n = 0;
        auto put = [&](int v) { b[n++] = (uint8_t)v; };
        auto seg = [&](int marker, int payload) { put(0xff); put(marker); put((payload + 2) >> 8); put((payload + 2) & 255); };
        put(0xff); put(0xd8);
        seg(0xe0, 14);
        put('J'); put('F'); put('I'); put('F'); put(0); put(1); put(1); put(0); put(0); put(1); put(0); put(1); put(0); put(0);
        for (int k = 0; k <= rgb; ++k) {
            seg(0xdb, 65);
            put(k);
            t.dqt[rgb][k] = n;
            n += 64;
        }
        seg(0xc0, rgb ? 15 : 9);
        put(8);
        t.sof_hw[rgb] = n;
        n += 4;
        put(rgb ? 3 : 1);
        put(1);
        t.sof_luma[rgb] = n;
        put(rgb ? 0x22 : 0x11); put(0);
        if (rgb) { put(2); put(0x11); put(1); put(3); put(0x11); put(1); }
        t.dht[rgb] = n;
        for (int k = 0; k <= rgb; ++k) {
            seg(0xc4, 1 + 16 + 12);
            put(k);
            for (int i = 0; i < 16; ++i) put(DC_BITS[k][i]);
            for (int i = 0; i < 12; ++i) put(i);
            seg(0xc4, 1 + 16 + 162);
            put(0x10 | k);
            for (int i = 0; i < 16; ++i) put(AC_BITS[k][i]);
            for (int i = 0; i < 162; ++i) put(AC_VALS[k][i]);
        }
        t.sos[rgb] = n;
        seg(0xda, rgb ? 10 : 6);
        put(rgb ? 3 : 1);
        put(1); put(0x00);
        if (rgb) { put(2); put(0x11); put(3); put(0x11); }
        put(0); put(63); put(0);
        t.hdr_len[rgb] = n;
    }
    return t;
}

constexpr Tables HOST_T = make_tables();
static_assert(HOST_T.hdr_len[1] == 623 && HOST_T.max_block_bits == 1660, "the header and the per-block bound of include/adain_hip.h");
__constant__ const Tables T = make_tables();

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

size_t align256(size_t x) { return (x + 255) & ~(size_t)255; }

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
    size_t at = 0, N = (size_t)n;
    auto take = [&](size_t bytes) { size_t o = at; at = align256(at + bytes); return o; };
    p.o_coef = take(N * p.nblk * 64 * sizeof(int16_t));
    p.o_bits = take(N * p.nblk * sizeof(uint32_t));
    p.o_off = take(N * p.nblk * sizeof(uint64_t));
    p.o_total = take(N * sizeof(uint64_t));
    p.o_stream = take(N * p.stream_words * sizeof(uint32_t));
    p.o_ffcnt = take(N * p.chunks * sizeof(uint32_t));
    p.o_ffoff = take(N * p.chunks * sizeof(uint32_t));
    p.o_fftotal = take(N * sizeof(uint32_t));
    if (optimize) {
        p.o_hist = take(N * SLOTS * 256 * sizeof(uint64_t));
        p.o_huff = take(N * SLOTS * sizeof(HuffSlot));
    }
    p.total = at;
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

// inclusive sum over the 256 threads of a workgroup; part: 4 ints of LDS
__device__ __forceinline__ int workgroup_inclusive(int v, int* part) {
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    for (int d = 1; d < 64; d <<= 1) {
        const int up = __shfl_up(v, d);
        if (lane >= d) v += up;
    }
    __syncthreads();                                   // the previous pass has read part
    if (lane == 63) part[wv] = v;
    __syncthreads();
    for (int k = 0; k < wv; ++k) v += part[k];
    return v;
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
constexpr int IDCT_PER_WG = 32;         // blocks per workgroup of the IDCT, 8 lanes each
constexpr int MERGE_PX = 512;           // pixels of one output row per workgroup of the merge, 2 per lane

// Where the IDCT puts a frame's samples: uint8 planes of whole blocks, 64 bytes per block of the scan, Y [yh][yw] first, then (RGB)
// Cb and Cr [8 mh][cw].  Every plane starts at a multiple of 64 bytes and every row stride is a multiple of 8.
struct Planes {
    int c, mw, bw, yw, cw;
    size_t nblk, o_cb, o_cr, stride;
};

struct RoundtripPlan {
    Planes g;
    int mh, bh;
    size_t o_coef, o_planes, total;     // workspace offsets (bytes) of the n-frame arrays
};

RoundtripPlan make_roundtrip_plan(int n, int h, int w, int c) {
    RoundtripPlan p{};
    Planes& g = p.g;
    g.c = c;
    g.bw = (w + 7) / 8, p.bh = (h + 7) / 8;
    g.mw = (w + 15) / 16, p.mh = (h + 15) / 16;
    g.nblk = c == 3 ? (size_t)g.mw * p.mh * 6 : (size_t)g.bw * p.bh;
    g.yw = c == 3 ? 16 * g.mw : 8 * g.bw;
    g.cw = c == 3 ? 8 * g.mw : 0;
    g.o_cb = c == 3 ? (size_t)g.mw * p.mh * 256 : 0;
    g.o_cr = c == 3 ? g.o_cb + (size_t)g.mw * p.mh * 64 : 0;
    g.stride = g.nblk * 64;
    p.o_coef = 0;
    p.o_planes = align256((size_t)n * g.nblk * 64 * sizeof(int16_t));
    p.total = p.o_planes + align256((size_t)n * g.stride);
    return p;
}

// One pass of jidctint over 8 values p[0], p[S], ..., descaled by N bits.  int32 suffices for coefficients that come from 8-bit samples at
// any quality: a dequantised coefficient is within q / 2 <= 127.5 of the forward DCT's, which is at most 1024, so |d| <= 1152, and in the
// column pass even the sum of the absolute values of every term of the largest intermediate (an output: 169352 |d|) is 1.96e8 < 2^31.  For
// the row pass that crude sum is too weak and Parseval does the work: the block's 64 coefficients are an orthonormal DCT of samples in
// [-128, 127] (2-norm <= 8 * 128) plus a quantisation error (2-norm <= 8 * 127.5), the column pass is 4 sqrt(8) times an orthonormal
// transform, so the 8 inputs of a row have a 2-norm of at most 4 sqrt(8) * 2044 + rounding < 23200; every intermediate of the pass is a
// fixed linear form of them whose coefficient vector has a 2-norm below 30000 (the largest: z2, 20995 sqrt(2) = 29692; the outputs: 23200),
// so by Cauchy-Schwarz it stays below 30000 * 23200 = 6.96e8 < 2^31.
template <int S, int N>
__device__ __forceinline__ void idct_pass(int* p) {
    constexpr int R = 1 << (N - 1);
    const int d0 = p[0], d1 = p[S], d2 = p[2 * S], d3 = p[3 * S], d4 = p[4 * S], d5 = p[5 * S], d6 = p[6 * S], d7 = p[7 * S];
    int z1 = (d2 + d6) * 4433;
    const int tmp2 = z1 - d6 * 15137, tmp3 = z1 + d2 * 6270;
    const int tmp0 = (d0 + d4) * 8192, tmp1 = (d0 - d4) * 8192;
    const int tmp10 = tmp0 + tmp3, tmp13 = tmp0 - tmp3, tmp11 = tmp1 + tmp2, tmp12 = tmp1 - tmp2;
    int t0 = d7, t1 = d5, t2 = d3, t3 = d1;
    z1 = t0 + t3;
    int z2 = t1 + t2, z3 = t0 + t2, z4 = t1 + t3;
    const int z5 = (z3 + z4) * 9633;
    t0 *= 2446, t1 *= 16819, t2 *= 25172, t3 *= 12299;
    z1 *= -7373, z2 *= -20995;
    z3 = z3 * -16069 + z5, z4 = z4 * -3196 + z5;
    t0 += z1 + z3, t1 += z2 + z4, t2 += z2 + z3, t3 += z1 + z4;
    p[0] = (tmp10 + t3 + R) >> N;
    p[7 * S] = (tmp10 - t3 + R) >> N;
    p[S] = (tmp11 + t2 + R) >> N;
    p[6 * S] = (tmp11 - t2 + R) >> N;
    p[2 * S] = (tmp12 + t1 + R) >> N;
    p[5 * S] = (tmp12 - t1 + R) >> N;
    p[3 * S] = (tmp13 + t0 + R) >> N;
    p[4 * S] = (tmp13 - t0 + R) >> N;
}

__device__ __forceinline__ uint32_t range_limit(int x) {
    const int i = x & 0x3ff;
    return (uint32_t)(i < 512 ? min(i + 128, 255) : max(i - 896, 0));
}

__global__ __launch_bounds__(IDCT_PER_WG * 8) void jpeg_idct_kernel(const int16_t* __restrict__ coef, int quality, uint8_t* __restrict__ planes, Planes g) {
    constexpr int NB = IDCT_PER_WG, THREADS = NB * 8;
    __shared__ int samp[NB * 72];               // 8 rows of 9 ints per block, as in the forward transform
    __shared__ int q[128];
    const int t = threadIdx.x;
    const size_t f = blockIdx.y, b0 = (size_t)blockIdx.x * NB;
    const int count = (int)min((size_t)NB, g.nblk - b0);
    if (t < 128) q[t] = quant_entry(t >> 6, t & 63, quality);
    __syncthreads();
    const uint32_t* s32 = (const uint32_t*)(coef + (f * g.nblk + b0) * 64);          // block starts are 128-byte aligned in the workspace
    for (int i = t; i < count * 32; i += THREADS) {
        const uint32_t v = s32[i];
        const int blk = i >> 5, z = (i & 31) * 2;
        const int* qt = q + (g.c == 3 && (b0 + blk) % 6 >= 4 ? 64 : 0);
        const int n0 = T.zigzag[z], n1 = T.zigzag[z + 1];
        samp[blk * 72 + (n0 >> 3) * 9 + (n0 & 7)] = (int)(int16_t)(v & 0xffff) * qt[n0];
        samp[blk * 72 + (n1 >> 3) * 9 + (n1 & 7)] = (int)(int16_t)(v >> 16) * qt[n1];
    }
    __syncthreads();
    const int blk = t >> 3, k = t & 7;
    if (blk < count) idct_pass<9, 11>(samp + blk * 72 + k);
    __syncthreads();
    if (blk < count) {
        int* p = samp + blk * 72 + k * 9;
        idct_pass<1, 18>(p);
        uint2 out;
        out.x = range_limit(p[0]) | range_limit(p[1]) << 8 | range_limit(p[2]) << 16 | range_limit(p[3]) << 24;
        out.y = range_limit(p[4]) | range_limit(p[5]) << 8 | range_limit(p[6]) << 16 | range_limit(p[7]) << 24;
        const size_t b = b0 + blk;
        size_t at;                              // of row k of the block in the frame's planes
        if (g.c == 3) {
            const size_t m = b / 6, my = m / g.mw, mx = m - my * g.mw;
            const int j = (int)(b - m * 6);
            if (j < 4) at = ((2 * my + (j >> 1)) * 8 + k) * g.yw + (2 * mx + (j & 1)) * 8;
            else at = (j == 4 ? g.o_cb : g.o_cr) + (my * 8 + k) * g.cw + mx * 8;
        } else {
            const size_t by = b / g.bw, bx = b - by * g.bw;
            at = (by * 8 + k) * g.yw + bx * 8;
        }
        *(uint2*)(planes + f * g.stride + at) = out;
    }
}

__device__ __forceinline__ uint32_t clamp_u8(int v) { return (uint32_t)min(max(v, 0), 255); }

// C = 3: the pixels (x, x + 1) of row y from their luma samples and chroma column x / 2; C = 1: the luma samples themselves.
template <int C>
__global__ __launch_bounds__(MERGE_PX / 2) void jpeg_merge_kernel(const uint8_t* __restrict__ planes, Planes g, int h, int w, uint8_t* __restrict__ dst) {
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
                    const int s = 3 * a[o_k + cc] + b[o_k + cc], sl = 3 * a[o_k + cl] + b[o_k + cl], sn = 3 * a[o_k + cn] + b[o_k + cn];
                    (k ? cr : cb)[0] = (3 * s + sl + 8) >> 4;
                    (k ? cr : cb)[1] = (3 * s + sn + 7) >> 4;
                }
            }
#pragma unroll
            for (int k = 0; k < 2; ++k) {
                const int yy = k ? y1 : y0, u = cb[k] - 128, v = cr[k] - 128;
                o[3 * k] = (uint8_t)clamp_u8(yy + ((91881 * v + 32768) >> 16));
                o[3 * k + 1] = (uint8_t)clamp_u8(yy + ((-22554 * u - 46802 * v + 32768) >> 16));
                o[3 * k + 2] = (uint8_t)clamp_u8(yy + ((116130 * u + 32768) >> 16));
            }
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
//   samples   coefficient times the FILE's table entry of its component, then the IDCT of the round trip above, unchanged
//   chroma    cropped to the real samples first (ch x cw; 4:2:0: ceil(h/2) x ceil(w/2), 4:2:2: h x ceil(w/2), 4:4:4: h x w).
//             4:2:0: h2v2_fancy_upsample as in the round trip.  4:2:2: h2v1_fancy_upsample - out[2c] = (3 C[c] + C[c-1] + 1) >> 2,
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
//   idct / pixels   as in the round trip, with the file's tables and the three layouts
// Launches per call, whatever Ri: ceil(n / 64) table + unstuff + one memset + settle + write + dc + idct + pixels.
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

struct DecPlan {
    int c, H, V, bpm, mw, mh, yw, yh, cw, chh;        // luma blocks per MCU H x V; plane sizes in samples (whole blocks)
    size_t nblk, o_cb, o_cr, plane_stride;
    uint32_t cap_words, nsub_max, chunk_bits;
    uint32_t ri, nint;          // MCUs per interval (Ri, or all of them at Ri = 0) and intervals
    size_t o_seg, o_meta, o_stream, o_state, o_count, o_coef, o_planes, o_itab, total;          // itab: per file nint + 1 first stream bytes, nint + 1 first subsequences; none at Ri = 0
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

DecPlan make_decode_plan(int n, int h, int w, int c, int sampling, int restart_interval, size_t max_segment_bytes, int chunk_bits) {
    DecPlan p{};
    p.c = c;
    p.H = sampling >= 1 ? 2 : 1, p.V = sampling == 2 ? 2 : 1;
    p.bpm = c == 3 ? p.H * p.V + 2 : 1;
    p.mw = (w + 8 * p.H - 1) / (8 * p.H), p.mh = (h + 8 * p.V - 1) / (8 * p.V);
    p.nblk = (size_t)p.mw * p.mh * p.bpm;
    p.yw = p.mw * p.H * 8, p.yh = p.mh * p.V * 8;
    p.cw = c == 3 ? p.mw * 8 : 0, p.chh = c == 3 ? p.mh * 8 : 0;
    p.o_cb = (size_t)p.yw * p.yh;
    p.o_cr = p.o_cb + (size_t)p.cw * p.chh;
    p.plane_stride = p.nblk * 64;
    p.chunk_bits = chunk_bits ? (uint32_t)chunk_bits : (uint32_t)DEC_DEFAULT_CHUNK_BITS;
    p.cap_words = (uint32_t)((max_segment_bytes + 3) / 4 + 3);
    const uint32_t nmcu = (uint32_t)p.mw * (uint32_t)p.mh;
    p.ri = restart_interval ? (uint32_t)restart_interval : nmcu;
    p.nint = (nmcu + p.ri - 1) / p.ri;
    // every interval rounds its last subsequence up: the sum of ceil(bits_k / chunk_bits) is below ceil(bits / chunk_bits) + nint
    p.nsub_max = (uint32_t)((max_segment_bytes * 8 + p.chunk_bits - 1) / p.chunk_bits) + (restart_interval ? p.nint : 0u);
    if (p.nsub_max == 0) p.nsub_max = 1;
    size_t at = 0, N = (size_t)n;
    auto take = [&](size_t bytes) { size_t o = at; at = align256(at + bytes); return o; };
    p.o_seg = take(N * sizeof(DecSeg));
    p.o_meta = take(N * sizeof(DecMeta));
    p.o_stream = take(N * p.cap_words * sizeof(uint32_t));
    p.o_state = take(3 * N * p.nsub_max * sizeof(uint2));
    p.o_count = take(N * p.nsub_max * sizeof(uint32_t));
    p.o_coef = take(N * p.nblk * 64 * sizeof(int16_t));
    p.o_planes = take(N * p.plane_stride);
    p.o_itab = take(restart_interval ? N * 2 * ((size_t)p.nint + 1) * sizeof(uint32_t) : 0);
    p.total = at;
    return p;
}

__global__ void jpegd_table_kernel(DecSegBatch b, int first, int count, DecSeg* __restrict__ seg, DecMeta* __restrict__ meta) {
    const int i = threadIdx.x;
    if (i >= count) return;
    seg[first + i] = DecSeg{b.off[i], b.len[i], 0u};
    meta[first + i] = DecMeta{0u, 0u, 0u, 0u, 0u, 0u, 0u, 0u};
}

// inclusive sum over the DEC_THREADS threads of a workgroup; part: 16 uint32 of LDS
__device__ __forceinline__ uint32_t decode_inclusive(uint32_t v, uint32_t* part) {
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    for (int d = 1; d < 64; d <<= 1) {
        const uint32_t up = __shfl_up(v, d);
        if (lane >= d) v += up;
    }
    __syncthreads();                                   // the previous pass has read part
    if (lane == 63) part[wv] = v;
    __syncthreads();
    for (int k = 0; k < wv; ++k) v += part[k];
    return v;
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
        const uint32_t v = keep | (marks << 16);
        const uint32_t incl = decode_inclusive(v, part);
        uint32_t at = carry + ((incl - v) & 0xffffu), m = mcarry + ((incl - v) >> 16);
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            if (kept[k]) out[at++] = b[k + 1];
            if (mark[k]) {
                if (m + 1 < nint) tab[m + 1] = at;
                if ((b[k + 2] & 7u) != (m & 7u)) order = true;
                ++m;
            }
        }
        __syncthreads();
        if (threadIdx.x == DEC_THREADS - 1) part[15] = incl;          // wave 15's slot is read only by waves above it: none
        __syncthreads();
        carry += part[15] & 0xffffu, mcarry += part[15] >> 16;
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

// One workgroup per file: (Ri > 0) every interval's first subsequence, then the rounds, then the scan of the block counts (count[s] becomes
// the blocks begun before subsequence s in the file; the write stage takes the interval's own first count off it).
__global__ __launch_bounds__(DEC_THREADS) void jpegd_settle_kernel(const uint8_t* __restrict__ blobs, const uint32_t* __restrict__ stream, uint32_t cap_words,
                                                                   DecMeta* __restrict__ meta, uint2* __restrict__ state, uint32_t* __restrict__ count,
                                                                   uint32_t nsub_max, uint32_t chunk_bits, DecShape g, uint32_t* __restrict__ itab) {
    __shared__ FileTables ft;
    __shared__ uint32_t part[16];
    __shared__ int changed[2];
    const size_t f = blockIdx.x;
    const int t = threadIdx.x;
    load_tables(&ft, blobs + f * sizeof(FileTables));
    const uint32_t* s = stream + f * cap_words;
    const uint32_t nbits = min(meta[f].ulen, (cap_words - 3) * 4) * 8;
    uint32_t* tab = itab ? itab + f * 2 * ((size_t)g.nint + 1) : nullptr;
    uint32_t nsub = (uint32_t)(((uint64_t)nbits + chunk_bits - 1) / chunk_bits);      // <= nsub_max
    if (tab) {
        // the table is whole only with nint - 1 markers in order: then its entries rise from 0 to the stream's length
        const bool whole = meta[f].nmark == g.nint - 1 && !meta[f].merr;
        uint32_t carry = 0;
        for (uint32_t base = 0; base < g.nint && whole; base += DEC_THREADS) {
            const uint32_t k = base + t;
            const uint32_t v = k < g.nint ? (uint32_t)(((uint64_t)(tab[k + 1] - tab[k]) * 8 + chunk_bits - 1) / chunk_bits) : 0u;
            const uint32_t incl = decode_inclusive(v, part);
            if (k < g.nint) tab[g.nint + 1 + k] = carry + incl - v;
            __syncthreads();
            if (t == DEC_THREADS - 1) part[15] = incl;
            __syncthreads();
            carry += part[15];
        }
        nsub = whole && carry <= nsub_max ? carry : 0u;
        if (t == 0) tab[2 * g.nint + 1] = nsub;
        __syncthreads();
    }
    uint2* st[2] = {state + f * 3 * nsub_max, state + (f * 3 + 1) * nsub_max};
    uint2* last_in = state + (f * 3 + 2) * nsub_max;    // the state each subsequence was last decoded from: read and written by its lane only
    uint32_t* cnt = count + f * nsub_max;
    uint32_t rounds = 0, settled = 0;
    for (uint32_t r = 0; r <= nsub; ++r) {              // at most nsub + 1 rounds
        if (t == 0) changed[r & 1] = 0;
        __syncthreads();
        uint2* cur = st[r & 1];                         // written in this round, by lane i at i only
        const uint2* prev = st[(r & 1) ^ 1];            // the exit states of round r - 1: only read in this round
        int any = 0;
        for (uint32_t i = t; i < nsub; i += DEC_THREADS) {
            const DecInterval iv = interval_of(i, tab, g.nint, nbits);
            const uint32_t begin = iv.begin + (i - iv.sub0) * chunk_bits, end = min(begin + chunk_bits, iv.stop);
            const uint2 in = (r == 0 || i == iv.sub0) ? make_uint2(begin, 0u) : prev[i - 1];
            uint2 out;
            if (r > 0 && last_in[i].x == in.x && last_in[i].y == in.y) {
                out = prev[i];                          // the same input as last time: the same exit state
            } else {
                uint32_t nb = 0;
                out = decode_span<false>(s, cap_words - 1, end, iv.stop, in, ft, g, &nb, nullptr, 0, 0, 0, nullptr);
                cnt[i] = nb;
                last_in[i] = in;
                if (r > 0 && (out.x != prev[i].x || out.y != prev[i].y)) any = 1;
            }
            cur[i] = out;
        }
        if (any) changed[r & 1] = 1;
        __syncthreads();
        ++rounds;
        if (r > 0 && !changed[r & 1]) { settled = 1; break; }
    }
    if (nsub == 0 && !(tab && nbits)) settled = 1;      // an empty stream is settled; a table that is not whole is not
    // exclusive scan of the counts
    uint32_t carry = 0;
    for (uint32_t base = 0; base < nsub; base += DEC_THREADS) {
        const uint32_t i = base + t;
        const uint32_t v = i < nsub ? cnt[i] : 0u;
        const uint32_t incl = decode_inclusive(v, part);
        if (i < nsub) cnt[i] = carry + incl - v;
        __syncthreads();
        if (t == DEC_THREADS - 1) part[15] = incl;
        __syncthreads();
        carry += part[15];
    }
    if (t == 0) meta[f].rounds = rounds, meta[f].settled = settled, meta[f].nsub = nsub;
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
        auto block_of = [&](size_t i) { return comp == 0 ? (i / hv) * g.bpm + i % hv : i * g.bpm + hv + comp - 1; };
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

struct DecPlanes { int c, H, V, bpm, mw, yw, cw; size_t nblk, o_cb, o_cr, stride; };

// The round trip's IDCT stage on natural-order coefficients with the file's own tables; the planes are whole blocks, Y [8 V mh][8 H mw]
// first, then (colour) Cb and Cr [8 mh][8 mw].  blob_stride: bytes from one file's tables to the next file's (a progressive file has a blob per scan).
__global__ __launch_bounds__(IDCT_PER_WG * 8) void jpegd_idct_kernel(const int16_t* __restrict__ coef, const uint8_t* __restrict__ blobs, size_t blob_stride,
                                                                     uint8_t* __restrict__ planes, DecPlanes g) {
    constexpr int NB = IDCT_PER_WG, THREADS = NB * 8;
    __shared__ int samp[NB * 72];
    __shared__ int q[192];
    const int t = threadIdx.x, hv = g.H * g.V;
    const size_t f = blockIdx.y, b0 = (size_t)blockIdx.x * NB;
    const int count = (int)min((size_t)NB, g.nblk - b0);
    if (t < 192) q[t] = blobs[f * blob_stride + offsetof(FileTables, q) + t];
    __syncthreads();
    const uint32_t* s32 = (const uint32_t*)(coef + (f * g.nblk + b0) * 64);
    for (int i = t; i < count * 32; i += THREADS) {
        const uint32_t v = s32[i];
        const int blk = i >> 5, n0 = (i & 31) * 2;
        const int j = (int)((b0 + blk) % g.bpm);
        const int* qt = q + (j < hv ? 0 : j - hv + 1) * 64;
        int* p = samp + blk * 72 + (n0 >> 3) * 9 + (n0 & 7);
        p[0] = (int)(int16_t)(v & 0xffff) * qt[n0];
        p[1] = (int)(int16_t)(v >> 16) * qt[n0 + 1];
    }
    __syncthreads();
    const int blk = t >> 3, k = t & 7;
    if (blk < count) idct_pass<9, 11>(samp + blk * 72 + k);
    __syncthreads();
    if (blk < count) {
        int* p = samp + blk * 72 + k * 9;
        idct_pass<1, 18>(p);
        uint2 out;
        out.x = range_limit(p[0]) | range_limit(p[1]) << 8 | range_limit(p[2]) << 16 | range_limit(p[3]) << 24;
        out.y = range_limit(p[4]) | range_limit(p[5]) << 8 | range_limit(p[6]) << 16 | range_limit(p[7]) << 24;
        const size_t b = b0 + blk, m = b / g.bpm, my = m / g.mw, mx = m - my * g.mw;
        const int j = (int)(b - m * g.bpm);
        size_t at;
        if (j < hv) at = ((my * g.V + j / g.H) * 8 + k) * g.yw + (mx * g.H + j % g.H) * 8;
        else at = (j == hv ? g.o_cb : g.o_cr) + (my * 8 + k) * g.cw + mx * 8;
        *(uint2*)(planes + f * g.stride + at) = out;
    }
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
                uv[k] = (3 * (3 * a[cc] + b[cc]) + 3 * a[cn] + b[cn] + ((x & 1) ? 7 : 8)) >> 4;
            } else {
                uv[k] = (3 * a[cc] + a[cn] + ((x & 1) ? 2 : 1)) >> 2;
            }
        }
    }
    const int u = uv[0] - 128, v = uv[1] - 128;
    d[0] = (uint8_t)clamp_u8(yy + ((91881 * v + 32768) >> 16));
    d[1] = (uint8_t)clamp_u8(yy + ((-22554 * u - 46802 * v + 32768) >> 16));
    d[2] = (uint8_t)clamp_u8(yy + ((116130 * u + 32768) >> 16));
}

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

__device__ __forceinline__ bool prog_same(uint4 a, uint4 b) { return a.x == b.x && a.y == b.y && a.z == b.z && a.w == b.w; }

// One workgroup per file, one scan: the file decoder's settle stage on the scan's own stream.  Every subsequence enters round 0 from
// (its first bit, 0, 0, 0), which each kind reads as its start-of-block state.
template <int KIND>
__global__ __launch_bounds__(DEC_THREADS) void jpegp_settle_kernel(const uint8_t* __restrict__ blobs, const uint32_t* __restrict__ stream, uint32_t cap_words,
                                                                   DecMeta* __restrict__ meta, uint4* __restrict__ state, uint32_t* __restrict__ count,
                                                                   uint32_t nsub_max, uint32_t chunk_bits, DecShape g, ProgScan sc, int mw, int scan, int nscans,
                                                                   const uint64_t* __restrict__ mask) {
    __shared__ FileTables ft;
    __shared__ uint32_t part[16];
    __shared__ int changed[2];
    const size_t f = blockIdx.x, fs = f * nscans + scan;
    const int t = threadIdx.x;
    load_tables(&ft, blobs + fs * sizeof(FileTables));
    const uint32_t* s = stream + fs * cap_words;
    const uint32_t nbits = min(meta[fs].ulen, (cap_words - 3) * 4) * 8;
    const uint32_t nsub = min((uint32_t)(((uint64_t)nbits + chunk_bits - 1) / chunk_bits), nsub_max);
    uint4* st[2] = {state + f * 3 * nsub_max, state + (f * 3 + 1) * nsub_max};
    uint4* last_in = state + (f * 3 + 2) * nsub_max;
    uint32_t* cnt = count + f * nsub_max;
    const uint64_t* fm = mask + f * g.nblk;
    uint32_t rounds = 0, settled = 0;
    for (uint32_t r = 0; r <= nsub; ++r) {
        if (t == 0) changed[r & 1] = 0;
        __syncthreads();
        uint4* cur = st[r & 1];
        const uint4* prev = st[(r & 1) ^ 1];
        int any = 0;
        for (uint32_t i = t; i < nsub; i += DEC_THREADS) {
            const uint32_t begin = i * chunk_bits, end = min(begin + chunk_bits, nbits);
            const uint4 in = (r == 0 || i == 0) ? make_uint4(begin, 0u, 0u, 0u) : prev[i - 1];
            uint4 out;
            if (r > 0 && prog_same(last_in[i], in)) {
                out = prev[i];
            } else {
                uint32_t nb = 0;
                out = prog_span<KIND, false>(s, cap_words - 1, end, nbits, in, ft, g, sc, mw, fm, &nb, nullptr, 0, nullptr);
                cnt[i] = nb;
                last_in[i] = in;
                if (r > 0 && !prog_same(out, prev[i])) any = 1;
            }
            cur[i] = out;
        }
        if (any) changed[r & 1] = 1;
        __syncthreads();
        ++rounds;
        if (r > 0 && !changed[r & 1]) { settled = 1; break; }
    }
    if (nsub == 0) settled = 1;
    uint32_t carry = 0;
    for (uint32_t base = 0; base < nsub; base += DEC_THREADS) {
        const uint32_t i = base + t;
        const uint32_t v = i < nsub ? cnt[i] : 0u;
        const uint32_t incl = decode_inclusive(v, part);
        if (i < nsub) cnt[i] = carry + incl - v;
        __syncthreads();
        if (t == DEC_THREADS - 1) part[15] = incl;
        __syncthreads();
        carry += part[15];
    }
    if (t == 0) meta[fs].rounds = rounds, meta[fs].settled = settled, meta[fs].nsub = nsub;
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
        auto block_of = [&](size_t i) { return inter ? (comp == 0 ? (i / hv) * g.bpm + i % hv : i * g.bpm + hv + comp - 1) : prog_block(g, sc, mw, (uint32_t)i); };
        uint32_t sum = 0;
        for (size_t i = a; i < e; ++i) sum += (uint32_t)(int)fc[block_of(i) * 64];
        uint32_t run = decode_inclusive(sum, part) - sum;
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

struct ProgPlan {
    DecPlan d;          // the geometry; of its offsets only the ones below are used
    size_t o_seg, o_meta, o_stream, o_state, o_count, o_mask, o_coef, o_planes, total;
};

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

ProgPlan make_progressive_plan(int n, int h, int w, int c, int sampling, int nscans, size_t max_segment_bytes, int chunk_bits) {
    ProgPlan p{};
    p.d = make_decode_plan(n, h, w, c, sampling, 0, max_segment_bytes, chunk_bits);
    size_t at = 0, N = (size_t)n, S = (size_t)nscans;
    auto take = [&](size_t bytes) { size_t o = at; at = align256(at + bytes); return o; };
    p.o_seg = take(N * S * sizeof(DecSeg));
    p.o_meta = take(N * S * sizeof(DecMeta));
    p.o_stream = take(N * S * p.d.cap_words * sizeof(uint32_t));
    p.o_state = take(3 * N * p.d.nsub_max * sizeof(uint4));
    p.o_count = take(N * p.d.nsub_max * sizeof(uint32_t));
    p.o_mask = take(N * p.d.nblk * sizeof(uint64_t));
    p.o_coef = take(N * p.d.nblk * 64 * sizeof(int16_t));
    p.o_planes = take(N * p.d.plane_stride);
    p.total = at;
    return p;
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
    if (bad) { set_error("%s: %s (n %d, %d x %d x %d, sampling %d, optimize %d)", who, bad, n, h, w, c, sampling, optimize); return -1; }
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
                          size_t out_stride, int32_t* lengths, void* workspace, hipStream_t s) {
    const char* bad = check_shape(n, h, w, c, quality);
    if (!bad) bad = check_options(sampling, optimize);
    if (bad) { set_error("%s: %s (n %d, %d x %d x %d, quality %d, sampling %d, optimize %d)", who, bad, n, h, w, c, quality, sampling, optimize); return -1; }
    const Plan p = make_plan(n, h, w, c, sampling, optimize);
    if (p.out_stride > (size_t)INT32_MAX) { set_error("%s: %d x %d x %d: a worst-case file beyond 2^31 - 1 bytes", who, h, w, c); return -1; }
    if (out_stride < p.out_stride) { set_error("%s: out_stride %zu below the %zu of the size query", who, out_stride, p.out_stride); return -1; }
    if ((uintptr_t)workspace % 8 || (uintptr_t)lengths % 4) { set_error("%s: the workspace must be 8-byte and lengths 4-byte aligned", who); return -1; }
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
    if (n > 65535 || (blocks + 3) / 4 > 0x7fffffffull) { set_error("%s: batch of %d frames too large for one call", who, n); return -1; }
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
        if (hipMemsetAsync(hist, 0, (size_t)n * SLOTS * 256 * sizeof(uint64_t), s) != hipSuccess) { set_error("%s: hipMemsetAsync failed", who); return -1; }
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
    if (bad) { set_error("jpeg_roundtrip_u8: %s (n %d, %d x %d x %d)", bad, n, h, w, c); return -1; }
    if (workspace_bytes) *workspace_bytes = make_roundtrip_plan(n, h, w, c).total;
    return 0;
}

int launch_jpeg_roundtrip_u8(const uint8_t* src, int n, int h, int w, int c, int quality, uint8_t* dst, void* workspace, hipStream_t s) {
    const char* bad = check_shape(n, h, w, c, quality);
    if (bad) { set_error("jpeg_roundtrip_u8: %s (n %d, %d x %d x %d, quality %d)", bad, n, h, w, c, quality); return -1; }
    if ((uintptr_t)workspace % 8) { set_error("jpeg_roundtrip_u8: the workspace must be 8-byte aligned"); return -1; }
    const RoundtripPlan p = make_roundtrip_plan(n, h, w, c);
    const Planes& g = p.g;
    // gridDim.y and .z are limited to 65535: h <= 65535 keeps the rows below that; the frames ride in y (idct) and z (transform, merge)
    if (n > 65535 || (g.nblk + IDCT_PER_WG - 1) / IDCT_PER_WG > 0x7fffffffull) { set_error("jpeg_roundtrip_u8: batch of %d frames too large for one call", n); return -1; }
    int16_t* coef = (int16_t*)((char*)workspace + p.o_coef);
    uint8_t* planes = (uint8_t*)workspace + p.o_planes;
    if (c == 3)
        jpeg_transform_rgb_kernel<<<dim3((g.mw + MCUS_PER_WG - 1) / MCUS_PER_WG, p.mh, n), MCUS_PER_WG * 48, 0, s>>>(src, h, w, quality, coef, g.mw, g.bw, p.bh, g.nblk);
    else
        jpeg_transform_grey_kernel<<<dim3((g.bw + GREY_PER_WG - 1) / GREY_PER_WG, p.bh, n), GREY_PER_WG * 8, 0, s>>>(src, h, w, quality, coef, g.bw, g.nblk);
    jpeg_idct_kernel<<<dim3((unsigned)((g.nblk + IDCT_PER_WG - 1) / IDCT_PER_WG), n), IDCT_PER_WG * 8, 0, s>>>(coef, quality, planes, g);
    const dim3 grid((w + MERGE_PX - 1) / MERGE_PX, h, n);
    if (c == 3)
        jpeg_merge_kernel<3><<<grid, MERGE_PX / 2, 0, s>>>(planes, g, h, w, dst);
    else
        jpeg_merge_kernel<1><<<grid, MERGE_PX / 2, 0, s>>>(planes, g, h, w, dst);
    return check_launch("jpeg_roundtrip_u8");
}

int jpeg_decode_bytes(int n, int h, int w, int c, int sampling, int restart_interval, size_t max_segment_bytes, int chunk_bits, size_t* workspace_bytes) {
    const char* bad = check_decode_shape(n, h, w, c, sampling, restart_interval, max_segment_bytes, chunk_bits);
    if (bad) {
        set_error("jpeg_decode_u8: %s (n %d, %d x %d x %d, sampling %d, restart_interval %d, segment %zu, chunk_bits %d)", bad, n, h, w, c, sampling, restart_interval,
                  max_segment_bytes, chunk_bits);
        return -1;
    }
    if (workspace_bytes) *workspace_bytes = make_decode_plan(n, h, w, c, sampling, restart_interval, max_segment_bytes, chunk_bits).total;
    return 0;
}

int launch_jpeg_decode_u8(const uint8_t* files, size_t files_bytes, const uint8_t* blobs, int n, int h, int w, int c, int sampling, int restart_interval,
                          const uint64_t* seg_offsets, const uint32_t* seg_lengths, uint8_t* dst, int32_t* record, void* workspace, size_t workspace_bytes,
                          int chunk_bits, hipStream_t s) {
    const char* bad = check_decode_shape(n, h, w, c, sampling, restart_interval, 0, chunk_bits);
    if (bad) {
        set_error("jpeg_decode_u8: %s (n %d, %d x %d x %d, sampling %d, restart_interval %d, chunk_bits %d)", bad, n, h, w, c, sampling, restart_interval, chunk_bits);
        return -1;
    }
    size_t longest = 0;
    for (int i = 0; i < n; ++i) {
        if (seg_offsets[i] > files_bytes || seg_lengths[i] > files_bytes - seg_offsets[i]) {
            set_error("jpeg_decode_u8: segment %d (%llu + %u bytes) leaves the %zu bytes of files", i, (unsigned long long)seg_offsets[i], seg_lengths[i], files_bytes);
            return -1;
        }
        longest = seg_lengths[i] > longest ? seg_lengths[i] : longest;
    }
    if ((bad = check_decode_shape(n, h, w, c, sampling, restart_interval, longest, chunk_bits))) { set_error("jpeg_decode_u8: %s", bad); return -1; }
    if ((uintptr_t)workspace % 8 || (uintptr_t)record % 4) { set_error("jpeg_decode_u8: the workspace must be 8-byte and the record 4-byte aligned"); return -1; }
    const DecPlan p = make_decode_plan(n, h, w, c, sampling, restart_interval, longest, chunk_bits);
    if (workspace_bytes < p.total) { set_error("jpeg_decode_u8: workspace too small (%zu < %zu bytes)", workspace_bytes, p.total); return -1; }
    if ((p.nblk + IDCT_PER_WG - 1) / IDCT_PER_WG > 0x7fffffffull) { set_error("jpeg_decode_u8: %d x %d: too many blocks for one launch", h, w); return -1; }
    char* ws = (char*)workspace;
    DecSeg* seg = (DecSeg*)(ws + p.o_seg);
    DecMeta* meta = (DecMeta*)(ws + p.o_meta);
    uint32_t* stream = (uint32_t*)(ws + p.o_stream);
    uint2* state = (uint2*)(ws + p.o_state);
    uint32_t* count = (uint32_t*)(ws + p.o_count);
    int16_t* coef = (int16_t*)(ws + p.o_coef);
    uint8_t* planes = (uint8_t*)(ws + p.o_planes);
    uint32_t* itab = restart_interval ? (uint32_t*)(ws + p.o_itab) : nullptr;
    const DecShape g{p.H, p.V, p.bpm, p.c, p.nblk, p.ri, p.nint};
    const DecPlanes pg{p.c, p.H, p.V, p.bpm, p.mw, p.yw, p.cw, p.nblk, p.o_cb, p.o_cr, p.plane_stride};
    for (int first = 0; first < n; first += DEC_SEG_BATCH) {
        DecSegBatch b{};
        const int count_ = n - first < DEC_SEG_BATCH ? n - first : DEC_SEG_BATCH;
        for (int i = 0; i < count_; ++i) b.off[i] = seg_offsets[first + i], b.len[i] = seg_lengths[first + i];
        jpegd_table_kernel<<<1, DEC_SEG_BATCH, 0, s>>>(b, first, count_, seg, meta);
    }
    if (restart_interval)
        jpegd_unstuff_kernel<true><<<n, DEC_THREADS, 0, s>>>(files, seg, meta, (uint8_t*)stream, p.cap_words, itab, p.nint);
    else
        jpegd_unstuff_kernel<false><<<n, DEC_THREADS, 0, s>>>(files, seg, meta, (uint8_t*)stream, p.cap_words, nullptr, p.nint);
    if (hipMemsetAsync(coef, 0, (size_t)n * p.nblk * 64 * sizeof(int16_t), s) != hipSuccess) { set_error("jpeg_decode_u8: hipMemsetAsync failed"); return -1; }
    jpegd_settle_kernel<<<n, DEC_THREADS, 0, s>>>(blobs, stream, p.cap_words, meta, state, count, p.nsub_max, p.chunk_bits, g, itab);
    jpegd_write_kernel<<<dim3((p.nsub_max + 255) / 256, n), 256, 0, s>>>(blobs, stream, p.cap_words, meta, state, count, p.nsub_max, p.chunk_bits, g, coef, itab);
    jpegd_dc_kernel<<<n, DEC_THREADS, 0, s>>>(coef, meta, g, record);
    jpegd_idct_kernel<<<dim3((unsigned)((p.nblk + IDCT_PER_WG - 1) / IDCT_PER_WG), n), IDCT_PER_WG * 8, 0, s>>>(coef, blobs, sizeof(FileTables), planes, pg);
    const dim3 grid((w + 255) / 256, h, n);
    if (c == 3)
        jpegd_pixels_kernel<3><<<grid, 256, 0, s>>>(planes, pg, h, w, dst);
    else
        jpegd_pixels_kernel<1><<<grid, 256, 0, s>>>(planes, pg, h, w, dst);
    return check_launch("jpeg_decode_u8");
}

int jpeg_decode_progressive_bytes(int n, int h, int w, int c, int sampling, int nscans, size_t max_segment_bytes, int chunk_bits, size_t* workspace_bytes) {
    const char* bad = check_decode_shape(n, h, w, c, sampling, 0, max_segment_bytes, chunk_bits);
    if (!bad && (nscans < 1 || nscans > PROG_MAX_SCANS)) bad = "nscans outside 1..32";
    if (bad) {
        set_error("jpeg_decode_progressive_u8: %s (n %d, %d x %d x %d, sampling %d, %d scans, segment %zu, chunk_bits %d)", bad, n, h, w, c, sampling, nscans,
                  max_segment_bytes, chunk_bits);
        return -1;
    }
    if (workspace_bytes) *workspace_bytes = make_progressive_plan(n, h, w, c, sampling, nscans, max_segment_bytes, chunk_bits).total;
    return 0;
}

int launch_jpeg_decode_progressive_u8(const uint8_t* files, size_t files_bytes, const uint8_t* blobs, int n, int h, int w, int c, int sampling, int nscans,
                                      const int32_t* scans, const uint64_t* seg_offsets, const uint32_t* seg_lengths, uint8_t* dst, int32_t* record, void* workspace,
                                      size_t workspace_bytes, int chunk_bits, hipStream_t s) {
    const char* bad = check_decode_shape(n, h, w, c, sampling, 0, 0, chunk_bits);
    if (!bad) bad = check_progressive_scans(c, nscans, scans);
    if (bad) {
        set_error("jpeg_decode_progressive_u8: %s (n %d, %d x %d x %d, sampling %d, %d scans, chunk_bits %d)", bad, n, h, w, c, sampling, nscans, chunk_bits);
        return -1;
    }
    const size_t streams = (size_t)n * nscans;
    size_t longest = 0;
    for (size_t i = 0; i < streams; ++i) {
        if (seg_offsets[i] > files_bytes || seg_lengths[i] > files_bytes - seg_offsets[i]) {
            set_error("jpeg_decode_progressive_u8: segment %zu (%llu + %u bytes) leaves the %zu bytes of files", i, (unsigned long long)seg_offsets[i], seg_lengths[i],
                      files_bytes);
            return -1;
        }
        longest = seg_lengths[i] > longest ? seg_lengths[i] : longest;
    }
    if ((bad = check_decode_shape(n, h, w, c, sampling, 0, longest, chunk_bits))) { set_error("jpeg_decode_progressive_u8: %s", bad); return -1; }
    if ((uintptr_t)workspace % 8 || (uintptr_t)record % 4) { set_error("jpeg_decode_progressive_u8: the workspace must be 8-byte and the record 4-byte aligned"); return -1; }
    const ProgPlan pp = make_progressive_plan(n, h, w, c, sampling, nscans, longest, chunk_bits);
    const DecPlan& p = pp.d;
    if (workspace_bytes < pp.total) { set_error("jpeg_decode_progressive_u8: workspace too small (%zu < %zu bytes)", workspace_bytes, pp.total); return -1; }
    if ((p.nblk + IDCT_PER_WG - 1) / IDCT_PER_WG > 0x7fffffffull || streams > 0x7fffffffull) {
        set_error("jpeg_decode_progressive_u8: %d x %d, %d files: too many blocks or streams for one launch", h, w, n);
        return -1;
    }
    char* ws = (char*)workspace;
    DecSeg* seg = (DecSeg*)(ws + pp.o_seg);
    DecMeta* meta = (DecMeta*)(ws + pp.o_meta);
    uint32_t* stream = (uint32_t*)(ws + pp.o_stream);
    uint4* state = (uint4*)(ws + pp.o_state);
    uint32_t* count = (uint32_t*)(ws + pp.o_count);
    uint64_t* mask = (uint64_t*)(ws + pp.o_mask);
    int16_t* coef = (int16_t*)(ws + pp.o_coef);
    uint8_t* planes = (uint8_t*)(ws + pp.o_planes);
    const DecShape g{p.H, p.V, p.bpm, p.c, p.nblk, p.ri, p.nint};
    const DecPlanes pg{p.c, p.H, p.V, p.bpm, p.mw, p.yw, p.cw, p.nblk, p.o_cb, p.o_cr, p.plane_stride};
    for (size_t first = 0; first < streams; first += DEC_SEG_BATCH) {
        DecSegBatch b{};
        const int count_ = streams - first < (size_t)DEC_SEG_BATCH ? (int)(streams - first) : DEC_SEG_BATCH;
        for (int i = 0; i < count_; ++i) b.off[i] = seg_offsets[first + i], b.len[i] = seg_lengths[first + i];
        jpegd_table_kernel<<<1, DEC_SEG_BATCH, 0, s>>>(b, (int)first, count_, seg, meta);
    }
    jpegd_unstuff_kernel<false><<<(unsigned)streams, DEC_THREADS, 0, s>>>(files, seg, meta, (uint8_t*)stream, p.cap_words, nullptr, 1u);
    if (hipMemsetAsync(coef, 0, (size_t)n * p.nblk * 64 * sizeof(int16_t), s) != hipSuccess) { set_error("jpeg_decode_progressive_u8: hipMemsetAsync failed"); return -1; }
    const dim3 subs((p.nsub_max + 255) / 256, n);
    for (int k = 0; k < nscans; ++k) {
        const int32_t* d = scans + 8 * k;
        ProgScan sc{d[0], d[0] == 1 ? d[1] : 0, d[4], d[5], d[6], d[7], 0u, 0u};
        if (sc.ncomp == c) {
            sc.bw = (uint32_t)p.mw * (c == 1 ? 1u : (uint32_t)p.H), sc.nblk = (uint32_t)p.nblk;
        } else {
            const uint32_t cw = sc.comp == 0 ? (uint32_t)w : (uint32_t)((w + p.H - 1) / p.H), chh = sc.comp == 0 ? (uint32_t)h : (uint32_t)((h + p.V - 1) / p.V);
            sc.bw = (cw + 7) / 8, sc.nblk = sc.bw * ((chh + 7) / 8);
        }
        const dim3 blocks((sc.nblk + 255) / 256, n);
#define JPEGP_SETTLE(KIND)                                                                                                                                     \
    jpegp_settle_kernel<KIND><<<n, DEC_THREADS, 0, s>>>(blobs, stream, p.cap_words, meta, state, count, p.nsub_max, p.chunk_bits, g, sc, p.mw, k, nscans, mask); \
    jpegp_write_kernel<KIND><<<subs, 256, 0, s>>>(blobs, stream, p.cap_words, meta, state, count, p.nsub_max, p.chunk_bits, g, sc, p.mw, k, nscans, mask, coef)
        if (sc.ss == 0 && sc.ah == 0) {
            JPEGP_SETTLE(0);
            jpegp_dc_kernel<<<n, DEC_THREADS, 0, s>>>(coef, meta, g, sc, p.mw, k, nscans);
        } else if (sc.ss == 0) {
            jpegp_dcrefine_kernel<<<blocks, 256, 0, s>>>(stream, p.cap_words, meta, g, sc, p.mw, k, nscans, coef);
        } else if (sc.ah == 0) {
            JPEGP_SETTLE(1);
        } else {
            jpegp_mask_kernel<<<blocks, 256, 0, s>>>(coef, g, sc, p.mw, mask);
            JPEGP_SETTLE(2);
        }
#undef JPEGP_SETTLE
    }
    jpegp_finish_kernel<<<n, DEC_THREADS, 0, s>>>(coef, meta, g, nscans, record);
    jpegd_idct_kernel<<<dim3((unsigned)((p.nblk + IDCT_PER_WG - 1) / IDCT_PER_WG), n), IDCT_PER_WG * 8, 0, s>>>(coef, blobs, (size_t)nscans * sizeof(FileTables), planes, pg);
    const dim3 grid((w + 255) / 256, h, n);
    if (c == 3)
        jpegd_pixels_kernel<3><<<grid, 256, 0, s>>>(planes, pg, h, w, dst);
    else
        jpegd_pixels_kernel<1><<<grid, 256, 0, s>>>(planes, pg, h, w, dst);
    return check_launch("jpeg_decode_progressive_u8");
}

}  // namespace adain
