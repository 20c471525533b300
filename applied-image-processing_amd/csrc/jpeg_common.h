// What the device JPEG encoder and round trip (jpeg.hip) and the file decoders (jpeg_decode.hip) share: the constant tables, the inverse
// DCT with its plane geometry, the colour and upsampling arithmetic and the workgroup scan.  Everything here is in an anonymous namespace:
// each of the two translation units has its own copy, its own __constant__ T included, and no kernel is reached across them.
#pragma once
#include "common.h"

namespace adain {
namespace {

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

__device__ __forceinline__ uint32_t clamp_u8(int v) { return (uint32_t)min(max(v, 0), 255); }

// inclusive sum over the threads of a workgroup (a multiple of 64, up to 1024); part: one entry of LDS per wave
template <class V>
__device__ __forceinline__ V workgroup_inclusive(V v, V* part) {
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    for (int d = 1; d < 64; d <<= 1) {
        const V up = __shfl_up(v, d);
        if (lane >= d) v += up;
    }
    __syncthreads();                                   // the previous pass has read part
    if (lane == 63) part[wv] = v;
    __syncthreads();
    for (int k = 0; k < wv; ++k) v += part[k];
    return v;
}

// libjpeg's YCbCr -> RGB of one pixel
__device__ __forceinline__ void ycc_to_rgb(int yy, int cb, int cr, uint8_t* rgb) {
    const int u = cb - 128, v = cr - 128;
    rgb[0] = (uint8_t)clamp_u8(yy + ((91881 * v + 32768) >> 16));
    rgb[1] = (uint8_t)clamp_u8(yy + ((-22554 * u - 46802 * v + 32768) >> 16));
    rgb[2] = (uint8_t)clamp_u8(yy + ((116130 * u + 32768) >> 16));
}

// h2v2_fancy_upsample: the column sum s[c] = 3 C[r][c] + C[rn][c] of a row r and its vertical neighbour rn, and the output sample between
// column c and its horizontal neighbour `side` (the left one for an even output column, the right one for an odd one)
__device__ __forceinline__ int h2v2_column(const uint8_t* row, const uint8_t* neighbour, int c) { return 3 * row[c] + neighbour[c]; }
__device__ __forceinline__ int h2v2_sample(int s, int side, bool odd) { return (3 * s + side + (odd ? 7 : 8)) >> 4; }

// ---- the back half: coefficients -> sample planes -----------------------------------------------------------------------------------------
constexpr int IDCT_PER_WG = 32;         // blocks per workgroup of the IDCT, 8 lanes each

// A frame's blocks in scan order - per MCU the H x V luma blocks row-major, then (colour) Cb and Cr; grey: one block per MCU - and where
// the IDCT puts their samples: uint8 planes of whole blocks, 64 bytes per block of the scan, Y [8 V mh][yw] first, then (colour) Cb and
// Cr [8 mh][cw].  Every plane starts at a multiple of 64 bytes and every row stride is a multiple of 8.
struct DecPlanes { int c, H, V, bpm, mw, mh, yw, cw; size_t nblk, o_cb, o_cr, stride; };

DecPlanes make_planes(int h, int w, int c, int H, int V) {
    DecPlanes g{};
    g.c = c, g.H = H, g.V = V;
    g.bpm = c == 3 ? H * V + 2 : 1;
    g.mw = (w + 8 * H - 1) / (8 * H), g.mh = (h + 8 * V - 1) / (8 * V);
    g.nblk = (size_t)g.mw * g.mh * g.bpm;
    g.yw = g.mw * H * 8;
    g.cw = c == 3 ? g.mw * 8 : 0;
    g.o_cb = (size_t)g.yw * g.mh * V * 8;
    g.o_cr = g.o_cb + (size_t)g.cw * g.mh * 8;
    g.stride = g.nblk * 64;
    return g;
}

// The IDCT stage of IDCT_PER_WG blocks from b0 of frame blockIdx.y: 8 lanes per block, a lane per column, then a lane per row, and each
// lane stores its 8 samples as one 8-byte word.  samp: IDCT_PER_WG x 72 ints of LDS (8 rows of 9 per block, as in the forward transform).
// put(sb, v, i, comp): the dequantised coefficients 2 i and 2 i + 1 of a block of component comp, v = its int16 pair, into sb[row * 9 + column].
template <class Put>
__device__ __forceinline__ void idct_blocks(const int16_t* __restrict__ coef, uint8_t* __restrict__ planes, const DecPlanes& g, int* samp, Put put) {
    constexpr int NB = IDCT_PER_WG, THREADS = NB * 8;
    const int t = threadIdx.x, hv = g.H * g.V;
    const size_t f = blockIdx.y;
    const uint32_t b0 = blockIdx.x * NB;        // block indices fit 32 bits: at most 8192 x 8192 MCUs of 6 blocks
    const int count = (int)min((size_t)NB, g.nblk - b0);
    const uint32_t* s32 = (const uint32_t*)(coef + (f * g.nblk + b0) * 64);          // block starts are 128-byte aligned in the workspace
    for (int i = t; i < count * 32; i += THREADS) {
        const int blk = i >> 5, j = (int)((b0 + blk) % (uint32_t)g.bpm);
        put(samp + blk * 72, s32[i], i & 31, j < hv ? 0 : j - hv + 1);
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
        const uint32_t b = b0 + blk, m = b / (uint32_t)g.bpm;
        const size_t my = m / (uint32_t)g.mw, mx = m - my * g.mw;
        const int j = (int)(b - m * g.bpm);
        size_t at;                              // of row k of the block in the frame's planes
        if (j < hv) at = ((my * g.V + j / g.H) * 8 + k) * g.yw + (mx * g.H + j % g.H) * 8;
        else at = (j == hv ? g.o_cb : g.o_cr) + (my * 8 + k) * g.cw + mx * 8;
        *(uint2*)(planes + f * g.stride + at) = out;
    }
}

}  // namespace
}  // namespace adain
