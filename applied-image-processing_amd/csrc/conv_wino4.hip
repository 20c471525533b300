// Winograd F(4,3) x F(2,3) form of the 3x3 convolution, gfx950: 4 x 2 output tiles (4 rows, 2 columns) from 6 x 4 input
// patches, 24 multiplies per (cin, cout) pair and tile = 3 per output instead of 4 for F(2x2,3x3) and 9 for the direct form.
//
//   Y = A4^T [ sum_cin (G4 g G2^T) .* (B4^T d B2) ] A2          (rows: F(4,3), points 0, +-1, +-2, inf; columns: F(2,3))
//
// fp32 error of one layer ~ 1.2e-6 relative (F(2x2,3x3): 4.6e-7, direct: 2.3e-7), far inside the path's tolerance.
// F(4,3) is applied along the ROWS so that neighbouring lanes' patches stay 2 pixels apart in the LDS halo image (the
// conflict pattern of the F(2x2,3x3) kernels; 4 pixels apart would be a 4-way conflict for every 16-byte-aligned pixel stride).
//
// Mapping (that of the retired F(2x2,3x3) kernels - docs/HISTORY.md - with the roles of rows and columns swapped):
//   * block = 4 waves, tile = 32 Winograd tiles (2 tile rows x 16 tile columns = 8 x 32 output pixels) x 32 channels;
//   * the 24 transform positions xi = (r, j) are 24 GEMMs [32 tiles x cin] x [cin x 32]; wave j owns transform COLUMN j
//     (its 6 row positions r): 6 MFMA tiles of 32x32 = 96 accumulator registers (v_mfma_f32_32x32x2_f32, A = weights,
//     B = tiles, so that a lane holds 4 consecutive channels of one tile);
//   * A-side operand in registers: column j of d B2 needs two patch columns, so a lane reads 6 rows x 2 columns (b128,
//     4 channels) from the raw reflect-padded 10 x 34 halo image in LDS, combines them (24 adds) and applies B4^T down the
//     rows (48 fma/adds); fragments are updated in place (row r's fragment is dead once step r has issued);
//   * weights U = G4 g G2^T packed once as [cout/32][j][cin/8][r][lane][4], streamed into a 6-slot register ring (slot = r);
//   * the raw halo is staged 16 channels at a time (global -> registers -> LDS), one barrier per 48 MFMAs per wave;
//   * epilogue: P_j = A4^T M_j per wave (4 values), the four columns meet in LDS (64 KiB, XOR-swizzled b128), then
//     Y = P A2: bias, ReLU, optional 2x2 max-pool (a tile holds two pool windows), b128 buffer stores.
//
// Tried and measured without effect (tools/tune_conv.py, all 13 layer shapes, +-1 %): pixel-tile-fastest and grouped
// block -> tile orders (weights L2-resident), raised wave priority outside the main loop, halo loads spread differently,
// a 12-slot weight ring (512-register build).  See DESIGN.md 4(C) for what the probes say bounds the kernel.
#include <stdlib.h>
#include <type_traits>
#include <utility>

#include "common.h"
#include "device_utils.h"

namespace adain {

namespace {
constexpr int W4_KR = 16;                    // channels per raw stage = 2 chunks of 8
constexpr int W4_RSTR = W4_KR + 4;           // floats per halo pixel (80 B = 5 quads: an odd number of 16-byte bank quads)
constexpr int W4_RITEMS = 6;                 // staging items per thread: at most 340 halo pixels x 4 quads over 256 threads
// Tile geometry (template parameter GEO): the 32 Winograd tiles of a workgroup sit either 2 x 16 (GEO 0: 8 x 32 output pixels, a
// 10 x 34 halo - the tuned default) or 4 x 8 (GEO 1: 16 x 16 output pixels, an 18 x 18 halo).  One kernel, two layouts: the
// launcher picks per layer the one that pads the feature map less (W = 400 pads to 416 with 32-wide tiles but not with
// 16-wide ones; the reference's own video frames, 256 x 456, give maps 228 / 114 / 57 wide).
//
// LDS image of the raw halo, DE-INTERLEAVED by column parity: plane E holds the even halo columns, plane O the odd ones, each
// [HALO_H rows][HALO_W / 2 columns] pixels of 20 floats.  The tiles of a workgroup sit 2 pixels apart, i.e. 1 plane pixel = 5
// quads: the 16 lanes that one LDS cycle of a ds_read_b128 serves ({0-3,12-15,20-27} ..., MI355X_MICROARCH.md, LDS) must read
// 16 different quads of the 64 banks.  In one interleaved image (round 1: [10][34] pixels) neighbouring tiles are 10 quads apart
// and every patch read was a two-way bank conflict (SQ_LDS_BANK_CONFLICT = 49 % of SQ_LDS_IDX_ACTIVE).
//   GEO 0: lane li = tile (row li >> 4, column li & 15).  Row stride 88 quads (17 x 5 + 3): the second tile row, 4 halo rows
//          down, lands on the same quads modulo 16 as the first, so the columns 4-11 of one row and 0-3 / 12-15 of the other
//          (the hardware's lane groups) still cover all 16.
//   GEO 1: lane li = tile (row li >> 3, column li & 7).  A lane group reads columns 0-3 of tile rows 0 and 3 and columns 4-7 of
//          rows 1 and 2 (or the complement): columns 0-3 sit on quads {0,5,10,15}, columns 4-7 on {4,9,14,3} (mod 16), and the
//          two sets together with their shifts by 8 cover all 16 - so tile rows 1 and 3 must be shifted by 8 quads and row 2 by
//          0 (mod 16): 4 S = 8, 8 S = 0, 12 S = 8 (mod 16) for a row stride of S quads, i.e. S = 2 (mod 4): 46 = 9 x 5 + 1.
// Plane O starts 4 quads (mod 8) after plane E: the two neighbouring pixels that one 8-lane group of a staging ds_write_b128
// stores cover all 32 banks.
template <int GEO>
struct W4G {
    static constexpr int TROWS_LOG = GEO == 0 ? 1 : 2;             // Winograd-tile rows of a workgroup = 2 / 4
    static constexpr int TCOLS_LOG = 5 - TROWS_LOG;                // Winograd-tile columns = 16 / 8
    static constexpr int TILE_H = 4 << TROWS_LOG, TILE_W = 2 << TCOLS_LOG;        // output pixels: 8 x 32 / 16 x 16
    static constexpr int HALO_H = TILE_H + 2, HALO_W = TILE_W + 2;
    static constexpr int HALO = HALO_H * HALO_W;                   // 340 / 324 pixels
    static constexpr int PROW = (HALO_W / 2) * W4_RSTR + (GEO == 0 ? 12 : 4);      // 352 / 184 floats per plane row
    static constexpr int PLANE = HALO_H * PROW + (GEO == 0 ? 16 : 0);              // 3536 / 3312 floats per plane
    static constexpr int TAIL = 2 * PLANE;                         // staging items past the halo land here, never read
    static_assert(TAIL + (W4_RITEMS * 64 - HALO) * W4_RSTR <= 8192, "LDS layout");
    static_assert(PROW % 4 == 0 && (PLANE / 4) % 8 == 4, "bank layout");
    static_assert(GEO != 0 || (PROW / 4) % 16 == 8, "bank layout (2 x 16 tiles)");
    static_assert(GEO != 1 || (PROW / 4) % 4 == 2, "bank layout (4 x 8 tiles)");
    static_assert(HALO * 4 <= W4_RITEMS * 256, "staging items");
    static constexpr int RITEMS = W4_RITEMS, RBUF = 8192, CH1 = 8;      // staging items per thread; floats per halo buffer; chunk 1
};
// UP2X_POLY: a nearest-2x upsample + reflection pad + 3x3 conv is, per output phase (py, px) = pixels (2y + py, 2x + px), a 2 x 2
// convolution of the SOURCE map with a clamp pad (up[-1] reflects to up[1] = src[0], up[2W] to src[W-1]); along one axis the even
// phase applies (w0, w1 + w2) to src[i-1], src[i], the odd phase (w0 + w1, w2) to src[i], src[i+1].  F(5,2) uses the points of F(4,3)
// and F(3,2) those of F(2,3), so the input transform - patch 6 x 4, 24 positions, one column per wave - is the kernel's own.  A tile
// keeps 4 of the 5 rows F(5,2) yields (the fifth is the next tile's first; A5^T's rows 0-3 are A4^T's without the inf column, whose
// position then feeds nothing kept): 4 x 3 outputs of one phase instead of 4 x 2, 24 / 12 = 2 multiplies per output instead of 3.
// Tiles of 4 rows keep every tile boundary where the 3x3 kernel has one (multiples of 16 output rows): a frame and a band cut from it
// on such rows compute the rows they share with the same arithmetic (5-row tiles, 1.6 multiplies, would not: test_gpu_parity's
// 4k-frame bands).  An item is (tile group, channel tile, phase): the phase is folded into a VIRTUAL channel tile 4 ct + phase
// (weights [cout/32][phase][j][cin/8][r][lane][4]).  Two halo buffers = 65,664 B per workgroup.
// Tile group: 4 x 8 tiles = 16 x 24 outputs of the phase grid from an 18 x 25 source halo.  LDS image without per-pixel padding (the
// 80-byte pixels of W4G would leave no room for a second workgroup): halo pixel (hy, hx), channel quad q at quad
//   hy * 114 + q * 27 + (hx % 3) * 9 + hx / 3
// so that a patch column c of the lanes' patches (3 pixels apart) sits in one column-mod-3 sub-row at consecutive quads: lane
// (tile row tr = li >> 3, column tc = li & 7) reads quad 4 tr * 114 + tc + const; 456 = 8 (mod 16), so the four tile rows of a
// ds_read_b128 lane group ({0-3,12-15,20-27}: tr 0 / 3 columns 0-3, tr 1 / 2 columns 4-7) land on quads {0-3}, {8-11}, {12-15},
// {4-7} (mod 16) and those of the complement on {4-7}, {8-11}, {0-3}, {12-15}: all 16, conflict-free.  Staging stores hit at most
// 2-way on one bank per 8-lane group, which a ds_write_b128 absorbs (its transfer, not the LDS array, sets its cycles).
struct W4P {
    static constexpr int TCOLS_LOG = 3;
    static constexpr int TSTEP = 4;                                // output rows per tile (of the 5 F(5,2) yields)
    static constexpr int TILE_H = 4 * TSTEP, TILE_W = 24, HALO_H = TILE_H + 2, HALO_W = 25, HALO = HALO_H * HALO_W;
    static constexpr int RQ = 114, QQ = 27, SQ = 9;                // quads per halo row, per channel quad, per sub-row
    static constexpr int PROW = 4 * RQ, PLANE = 0, TAIL = 0;
    static constexpr int RITEMS = 8, RBUF = HALO_H * RQ * 4, CH1 = 2 * QQ * 4;
    static_assert(4 * QQ <= RQ && 3 * SQ <= QQ, "row layout");
    static_assert((TSTEP * RQ) % 16 == 8, "bank layout: tile rows 1 / 2 / 3 shifted by 8 / 0 / 8 quads against the column blocks");
    static_assert(HALO * 4 <= RITEMS * 256 && 2 * RBUF * 4 <= 80 * 1024, "LDS layout");
};
constexpr int W4_PEX = 4 * 4 * 32 * 32;                // [column j][a][tile][32 channels] floats = 64 KiB
static_assert(2 * W4G<0>::RBUF <= W4_PEX && 2 * W4G<1>::RBUF <= W4_PEX, "LDS layout");

// 128-bit buffer store.  The scalar offset operand is deliberately NOT exposed (always the literal 0): with an SGPR soffset LLVM
// models no hazard between a >64-bit MUBUF store and a following VALU write of its data registers and emits none of the wait states
// it emits for the literal form - and on gfx950, with two waves per SIMD queueing VMEM work, the store then reads data the next
// instruction has already overwritten (seen in round 2's F(2x2,3x3) kernel: the register allocator reused the first data register of
// one store as the address of the next; the .x lane values arrived as address bit patterns).  With the literal form the compiler
// inserts its `s_nop 1` and the stores are exact.
__device__ __forceinline__ void buf_store4(rsrc_t r, f32x4 v, int voff) {
    __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(u32x4, v), r, voff, 0, 0);
}
}  // namespace

// OIHW [cout][cin][3][3] -> U = G4 g G2^T packed as [cout/32][j 4][cin/8][r 6][lane 64][s 4]:
//   value = U[r][j][cout = 32 ct + (lane & 31)][cin = 8 chunk + 4 (lane >> 5) + s]
__global__ void pack_wino4_kernel(const float* __restrict__ w, float* __restrict__ p, int cin, int cout) {
    // transformed in double and rounded once: U carries half an ulp instead of the few ulp of nine fp32 products with 1/6, 1/12, 1/24
    // (a systematic, per-weight error; runs once per weight set)
    const double G2[4][3] = {{1., 0., 0.}, {0.5, 0.5, 0.5}, {0.5, -0.5, 0.5}, {0., 0., 1.}};
    const double G4[6][3] = {{0.25, 0., 0.},           {-1. / 6, -1. / 6, -1. / 6}, {-1. / 6, 1. / 6, -1. / 6},
                             {1. / 24, 1. / 12, 1. / 6}, {1. / 24, -1. / 12, 1. / 6}, {0., 0., 1.}};
    const size_t total = (size_t)cin * cout * 24;
    const int nch = cin / 8;
    for (size_t idx = blockIdx.x * (size_t)blockDim.x + threadIdx.x; idx < total; idx += (size_t)gridDim.x * blockDim.x) {
        size_t t = idx;
        const int s = t & 3; t >>= 2;
        const int lane = t & 63; t >>= 6;
        const int r = t % 6; t /= 6;
        const int chunk = t % nch; t /= nch;
        const int j = t & 3; t >>= 2;
        const int ct = (int)t;
        const int co = ct * 32 + (lane & 31), ci = chunk * 8 + 4 * (lane >> 5) + s;
        const float* g = w + ((size_t)co * cin + ci) * 9;
        double u = 0.;
#pragma unroll
        for (int a = 0; a < 3; ++a)
#pragma unroll
            for (int b = 0; b < 3; ++b) u += G4[r][a] * (double)g[a * 3 + b] * G2[j][b];
        p[idx] = (float)u;
    }
}

// UP2X_POLY: OIHW [cout][cin][3][3] -> per phase (py, px) the folded 2 x 2 filter h = F_py g F_px^T (even phase (w0, w1 + w2), odd
// phase (w0 + w1, w2) along each axis), then U = G5 h G3^T, packed as [cout/32][phase 2 py + px][j 4][cin/8][r 6][lane 64][s 4]
// (pack_wino4_kernel's layout with the phase beside the channel tile: the kernel streams it as virtual channel tile 4 ct + phase).
// Folded and transformed in double, rounded once.
__global__ void pack_up2x_poly_kernel(const float* __restrict__ w, float* __restrict__ p, int cin, int cout) {
    const double G3[4][2] = {{1., 0.}, {0.5, 0.5}, {0.5, -0.5}, {0., -1.}};
    const double G5[6][2] = {{0.25, 0.}, {-1. / 6, -1. / 6}, {-1. / 6, 1. / 6}, {1. / 24, 1. / 12}, {1. / 24, -1. / 12}, {0., 1.}};
    const size_t total = (size_t)cin * cout * 96;
    const int nch = cin / 8;
    for (size_t idx = blockIdx.x * (size_t)blockDim.x + threadIdx.x; idx < total; idx += (size_t)gridDim.x * blockDim.x) {
        size_t t = idx;
        const int s = t & 3; t >>= 2;
        const int lane = t & 63; t >>= 6;
        const int r = t % 6; t /= 6;
        const int chunk = t % nch; t /= nch;
        const int j = t & 3; t >>= 2;
        const int ph = t & 3; t >>= 2;
        const int ct = (int)t, py = ph >> 1, px = ph & 1;
        // fold: tap a of 2 takes taps {0} / {1, 2} of 3 (even phase) or {0, 1} / {2} (odd phase)
        auto fold = [](int odd, int a, int t3) { return (double)(odd ? (a ? t3 == 2 : t3 < 2) : (a ? t3 > 0 : t3 == 0)); };
        const int co = ct * 32 + (lane & 31), ci = chunk * 8 + 4 * (lane >> 5) + s;
        const float* g = w + ((size_t)co * cin + ci) * 9;
        double u = 0.;
#pragma unroll
        for (int a = 0; a < 2; ++a)
#pragma unroll
            for (int b = 0; b < 2; ++b) {
                double h = 0.;
#pragma unroll
                for (int ty = 0; ty < 3; ++ty)
#pragma unroll
                    for (int tx = 0; tx < 3; ++tx) h += fold(py, a, ty) * fold(px, b, tx) * (double)g[ty * 3 + tx];
                u += G5[r][a] * h * G3[j][b];
            }
        p[idx] = (float)u;
    }
}

// The stamp and timing-only ablation variants that measured this kernel (what its data movement costs, where its steps wait) are
// retired; docs/HISTORY.md keeps their numbers.
// PERSIST: a workgroup walks a list of tiles (grid = 2 per CU; XCD x owns a contiguous range of the tile list, channel tile
// fastest) instead of one: the next tile's first halo stage is loaded during the current tile's last stages and its first
// weight fragments replace the ring's run-off loads, so a tile starts with an LDS write + barrier + transform instead of a cold
// HBM round trip (tools/wino4_phase_probe.py: 3.4-4.1 us of prologue per one-tile workgroup; with cin = 64 both workgroups of a
// CU are inside their main loops only 22 % of the time).  The wave priority alternates per tile between the two halves of the
// grid: the SIMD arbiter prefers the older wave - the workgroup dispatched first ran its tiles ~1.4x faster than its CU partner and
// then sat idle at the end of the launch (static tile lists); alternating the priority per tile, in opposite phase for workgroups b
// and b + grid / 2 (they share a CU), evens the two out (round 2's persistent F(2x2,3x3) kernel: both in their main loops 71 % -> 84 %
// of the time).
// SEGMENTS (persistent form only): the tile list may run over up to four (source, output) tensor pairs of different sizes
// that share the layer's weights - the content batch and the style image of one encoder pass (reference test.py:57,63 encodes
// both through the same vgg) - so that the deep style-branch layers, too small to fill the chip on their own, ride in the
// content launch's list.  A tile's geometry (H, W, pointers) comes from its segment's descriptor, re-read from the kernel
// arguments at the two places that need it (the next tile's halo offsets, the epilogue's stores).
// BIG: per-tile buffer descriptors (any image size); the default form keeps one descriptor per image (tensors below 2 GiB)
template <int MODE, bool PERSIST = false, bool BIG = false, int GEO = 0>
__global__ __launch_bounds__(256, 2) void conv3x3_wino4_kernel(ConvArgs a, ConvSegs m, int items) {
    constexpr bool POLY = MODE == SRC_UP2X_POLY;      // UP2X_POLY: see W4P
    using G = std::conditional_t<POLY, W4P, W4G<GEO>>;
    constexpr int W4_HALO_W = G::HALO_W, W4_HALO_H = G::HALO_H, W4_HALO = G::HALO, W4_PROW = G::PROW, W4_PLANE = G::PLANE,
                  W4_TAIL = G::TAIL, TILE_W = G::TILE_W, TILE_H = G::TILE_H, TCL = G::TCOLS_LOG, TCM = (1 << G::TCOLS_LOG) - 1;
    constexpr int RI = G::RITEMS, W4_RBUF = G::RBUF, CH1 = G::CH1;
    __shared__ __attribute__((aligned(16))) float smem[POLY ? 2 * W4P::RBUF : W4_PEX];
    float* const Rs = smem;

    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wj = __builtin_amdgcn_readfirstlane(tid >> 6);      // transform column of this wave
    // the one lane constant kept live through the main loop; other lane-derived addresses are rebuilt from an opaque copy
    const int wvo = lane * 16;
    auto lane_now = [&]() {
        int w = wvo;
        asm volatile("" : "+v"(w));
        return w >> 4;
    };

    // block -> (channel tile fastest, pixel tile, image) inside a contiguous per-XCD range (halo reuse in L2)
    int tiles = a.tiles_x * a.tiles_y;
    const int nct = (POLY ? 4 : 1) * (a.cout / 32);   // POLY: virtual channel tiles 4 ct + phase
    int lid = blockIdx.x, ct, pt, img;
    // geometry of the tile being computed (gH, gW: conv output size; gWs: source row length) and of its tensors
    int gH = a.H, gW = a.W, gWs = a.Ws, gtx = a.tiles_x;
    int seg = 0;                                     // persistent form: segment of the current tile
    // CIN SPLIT (one-tile form only, launches too small to give every compute unit a tile: launch_conv3x3_wino4): workgroup
    // (tile, channel tile, ks) accumulates input channels [ks * cin_sub, (ks + 1) * cin_sub) only and writes its output-transformed
    // partial sums - no bias, no ReLU, no pool - into slab ks of a workspace; splitk_combine_kernel adds the slabs in the fixed
    // order ks = 0, 1, ... and finishes the layer.  The output transform is linear, so the split changes rounding only.
    int ks = 0;
    auto seg_of = [&](int it) {
        int si = 0;
        for (int k = 1; k < m.count; ++k)
            if (it >= m.s[k].item0) si = k;
        return si;
    };
    // persistent form: the tile list of this workgroup = items lo + slot, lo + slot + stride, ... below hi
    const int stride = gridDim.x >> 3;
    const int lo = (int)((long long)items * (blockIdx.x & 7) / 8), hi = (int)((long long)items * ((blockIdx.x & 7) + 1) / 8);
    int item = lo + (blockIdx.x >> 3);
    if constexpr (PERSIST) {
        if (item >= hi) return;
        seg = seg_of(item);
        lid = item - m.s[seg].item0;
        gH = m.s[seg].H; gW = m.s[seg].W; gWs = m.s[seg].Ws; gtx = m.s[seg].tiles_x;
        tiles = gtx * m.s[seg].tiles_y;
    } else if ((gridDim.x & 7) == 0) {
        lid = (lid & 7) * (gridDim.x >> 3) + (lid >> 3);
    }
    // Persistent walk: inside a segment the items are ordered (channel-tile GROUP, image, pixel tile, channel tile in the group),
    // group size m.ctg.  With ctg == nct (every channel tile in one group) consecutive items are the channel tiles of one pixel
    // tile: the 64 workgroups resident on an XCD share halos, but a layer whose transformed weights exceed the XCD's 4 MB L2
    // (256 -> 256: 6.3 MB) re-fetches them from the Infinity Cache once per group of 8 pixel tiles.  With a smaller group an
    // XCD's contiguous range stays inside ONE group for many pixel tiles: its weights (cin * 32 ctg * 96 B) stay in L2 and
    // the halos are fetched once per group instead.
    auto decode = [&](int li, int ntl, int nimgs, int& ct_, int& pt_, int& img_) {
        const int G = m.ctg;
        const int c = li % G, r = li / G;
        const int per = ntl * nimgs;
        const int g = r / per, pi = r - g * per;
        ct_ = g * G + c;
        img_ = pi / ntl;
        pt_ = pi - img_ * ntl;
    };
    if constexpr (PERSIST) {
        decode(lid, tiles, m.s[seg].n, ct, pt, img);
    } else {                         // channel tile fastest: the workgroups resident on an XCD share halos
        ct = lid % nct; lid /= nct;
        if (a.ksplit > 1) { ks = lid % a.ksplit; lid /= a.ksplit; }      // CIN SPLIT: then the cin ranges of one (pixel tile, channel tile)
        pt = lid % tiles;
        img = lid / tiles;
    }
    int tx0 = (pt % gtx) * TILE_W, ty0 = (pt / gtx) * TILE_H;
    const int nst = (PERSIST ? a.cin : a.cin_sub) / W4_KR;      // stages of this workgroup's cin range
    const int nch = a.cin / 8;

    // BIG: per-tile buffer descriptors.  The source descriptor starts at the first source row a tile's halo can touch, the output
    // descriptor (epilogue) at the tile's first output row, so every 32-bit offset stays inside a band of 10 source / 8 output
    // rows and an image may be of any size; the default form keeps one descriptor per image (row 0), which caps a tensor at
    // 2 GiB per image and costs 13 scalar registers less (same-box A/B: 0.4 % of the kernel's time).
    auto src_row0 = [&](int y0) {
        if constexpr (!BIG) return 0;
        const int r = max(y0 - 1, 0);                  // reflection never reaches above this row (row -1 maps to row 1)
        return MODE == SRC_UP2X ? r >> 1 : r;          // (POLY: y0 is a source row; the window starts at y0 - 1 + py, clamped)
    };
    auto src_of = [&](const float* base, int Hs, int Ws, int im, int y0) {
        if constexpr (!BIG) {
            const size_t per = (size_t)Hs * Ws * a.cin;
            return make_rsrc(base + im * per, (unsigned)(per * 4u));
        } else {
            const size_t row = (size_t)Ws * a.cin;
            const int r0 = src_row0(y0);
            const size_t left = (size_t)(Hs - r0) * row * 4;
            return make_rsrc(base + ((size_t)im * Hs + r0) * row, left < 0x7ffffff0ull ? (unsigned)left : 0x7ffffff0u);
        }
    };
    rsrc_t src = PERSIST ? src_of(m.s[seg].in, m.s[seg].Hs, m.s[seg].Ws, img, ty0) : src_of(a.in, a.Hs, a.Ws, img, ty0);
    const rsrc_t wsr = make_rsrc(a.wpk, (unsigned)a.cin * a.cout * (POLY ? 384u : 96u));

    // ---- raw halo staging: 340 pixels x 4 quads over 256 threads x 6 items ---------------------------------------------------
    // Per-lane byte offsets of the six staging items + a per-tile SCALAR base (the buffer load's soffset operand).  A tile whose
    // 10 x 34 halo lies inside the image needs no reflection (92 % of the tiles at 1024 x 1024), and then item k of a lane sits at
    // tile base + an offset that depends only on the lane and the segment's row pitch: the six registers are computed once per
    // segment (roff_seg remembers for which) and an interior tile costs scalar arithmetic only - round 2 recomputed them per
    // tile, 78 vector instructions of the ~560 a tile spends outside its main loop (they cost matrix-pipe time: DESIGN.md 4).
    // Tile origins are multiples of 8 / 32, so the nearest-2x source index splits the same way: (x0 + hx - 1) >> 1 =
    // (x0 / 2 - 1) + ((hx + 1) >> 1).  Tiles at the image border take the general path (reflection, base 0).
    int roff[RI];
    int tbase = 0, roff_seg = -1;
    auto halo_offsets = [&](int x0, int y0, int H, int W, int Ws, int sg, int vct) {
        const int t = PERSIST ? (lane_now() | (wj << 6)) : tid;        // persistent: recomputed per tile, nothing hoisted
        if constexpr (POLY) {           // window of phase (py, px) = vct & 3 at source (y0 - 1 + py, x0 - 1 + px), clamped
            const int Hs = H >> 1, wy = y0 - 1 + ((vct >> 1) & 1), wx = x0 - 1 + (vct & 1);
            const int r0 = src_row0(y0);
            if (PERSIST && wy >= 0 && wy + W4_HALO_H <= Hs && wx >= 0 && wx + W4_HALO_W <= Ws) {
                if (roff_seg != sg) {
#pragma unroll
                    for (int k = 0; k < RI; ++k) {
                        const int idx = t + k * 256;
                        const int hp = min(idx >> 2, W4_HALO - 1), q = idx & 3;
                        const int hy = hp / W4_HALO_W, hx = hp - hy * W4_HALO_W;
                        roff[k] = ((hy * Ws + hx) * a.cin + q * 4) * 4;
                    }
                    roff_seg = sg;
                }
                tbase = (((wy - r0) * Ws + wx) * a.cin) * 4;
            } else {
#pragma unroll
                for (int k = 0; k < RI; ++k) {
                    const int idx = t + k * 256;
                    const int hp = min(idx >> 2, W4_HALO - 1), q = idx & 3;
                    const int hy = hp / W4_HALO_W, hx = hp - hy * W4_HALO_W;
                    const int y = min(max(wy + hy, 0), Hs - 1) - r0, x = min(max(wx + hx, 0), Ws - 1);
                    roff[k] = ((y * Ws + x) * a.cin + q * 4) * 4;
                }
                roff_seg = -1;
                tbase = 0;
            }
            return;
        }
        const bool interior = PERSIST && y0 >= 1 && y0 + W4_HALO_H - 1 <= H && x0 >= 1 && x0 + W4_HALO_W - 1 <= W;
        [[maybe_unused]] const int r0 = src_row0(y0);  // BIG: rows are counted from the tile's source descriptor
        if (interior) {
            if (roff_seg != sg) {
#pragma unroll
                for (int k = 0; k < RI; ++k) {
                    const int idx = t + k * 256;
                    const int hp = min(idx >> 2, W4_HALO - 1), q = idx & 3;
                    const int hy = hp / W4_HALO_W, hx = hp - hy * W4_HALO_W;
                    const int yc = MODE == SRC_UP2X ? (hy + 1) >> 1 : hy, xc = MODE == SRC_UP2X ? (hx + 1) >> 1 : hx;
                    roff[k] = ((yc * Ws + xc) * a.cin + q * 4) * 4;
                }
                roff_seg = sg;
            }
            // source pixel of the halo's top-left corner; BIG: the tile's descriptor already starts at that row
            const int by = BIG ? 0 : (MODE == SRC_UP2X ? (y0 >> 1) - 1 : y0 - 1), bx = MODE == SRC_UP2X ? (x0 >> 1) - 1 : x0 - 1;
            tbase = ((by * Ws + bx) * a.cin) * 4;
        } else {
#pragma unroll
            for (int k = 0; k < RI; ++k) {
                const int idx = t + k * 256;
                const int hp = min(idx >> 2, W4_HALO - 1), q = idx & 3;
                const int hy = hp / W4_HALO_W, hx = hp - hy * W4_HALO_W;
                int y = reflect1(y0 + hy - 1, H), x = reflect1(x0 + hx - 1, W);
                if (MODE == SRC_UP2X) { y >>= 1; x >>= 1; }
                if constexpr (BIG) y -= r0;
                roff[k] = ((y * Ws + x) * a.cin + q * 4) * 4;
            }
            roff_seg = -1;
            tbase = PERSIST ? 0 : ks * a.cin_sub * 4;       // first channel of this workgroup's cin range
        }
    };
    halo_offsets(tx0, ty0, gH, gW, gWs, seg, ct);
    f32x4 rawreg[RI];
    auto raw_load = [&](int soff) {
#pragma unroll
        for (int k = 0; k < RI; ++k) rawreg[k] = buf_load4(src, roff[k], tbase + soff);
    };
    // LDS address (in BYTES from the start of a halo buffer) of staging item k of this thread: pixel (t >> 2) + 64 k of the halo,
    // quad t & 3; depends on the thread only, computed once.  Bytes, so that a store into a buffer whose place is known at compile
    // time is the register + an immediate offset (the persistent form's stage loop: no address arithmetic at all).
    int sa[RI];
    {
        const int t = tid;
#pragma unroll
        for (int k = 0; k < RI; ++k) {
            const int hp = (t >> 2) + 64 * k, q = t & 3;
            const int hy = hp / W4_HALO_W, hx = hp - hy * W4_HALO_W;
            if constexpr (POLY) {       // items past the halo repeat its last pixel (the same bytes to the same place)
                const int hc = min(hp, W4_HALO - 1), cy = hc / W4_HALO_W, cx = hc - cy * W4_HALO_W;
                sa[k] = 16 * (cy * W4P::RQ + q * W4P::QQ + (cx % 3) * W4P::SQ + cx / 3);
            } else {
                sa[k] = 4 * (hp < W4_HALO ? (hx & 1) * W4_PLANE + hy * W4_PROW + (hx >> 1) * W4_RSTR + q * 4
                                          : W4_TAIL + (hp - W4_HALO) * W4_RSTR + q * 4);
            }
            asm volatile("" : "+v"(sa[k]));      // held in a register: left alone the compiler recomputes it (8 vector
        }                                        // instructions per item and stage, and every one of them costs matrix-pipe time)
    }
    auto raw_store = [&](float* buf) {
#pragma unroll
        for (int k = 0; k < RI; ++k) *(f32x4*)((char*)buf + sa[k]) = rawreg[k];
    };

    // ---- weights: one b128 fragment per step (row position r), ring slot = r, loaded 5 steps ahead ---------------------------
    f32x4 bq[6];
    int wso = ((ct * 4 + wj) * nch + (PERSIST ? 0 : ks * (a.cin_sub >> 3))) * 6144;
#pragma unroll
    for (int r = 0; r < 4; ++r) bq[r] = buf_load4(wsr, wvo, wso + r * 1024);

    f32x16 acc[6];
    if constexpr (!PERSIST) {       // the persistent form starts every tile with MFMAs on a zero C operand
#pragma unroll
        for (int r = 0; r < 6; ++r)
#pragma unroll
            for (int e = 0; e < 16; ++e) acc[r][e] = 0.f;
    }

    // ---- epilogue (a lambda: the persistent form runs it inside the tile loop) ------------------------------------------------------
    // lane (li = tile, lh): acc[r][e16] = M[row r][column wj][channel 8 (e16 >> 2) + 4 lh + (e16 & 3)][tile li]
    auto epilogue = [&]() {
    {
        const int le = lane_now(), li = le & 31, lh = le >> 5;
        float* Pw = smem + (wj * 4) * (32 * 32) + li * 32;
        const int sw = (li >> 1) & 7;
#pragma unroll
        for (int rq = 0; rq < 4; ++rq) {
            f32x4 P0, P1, P2, P3;
            const int slot = ((2 * rq + lh) ^ sw) << 2;    // channel quad of the 32, XOR-swizzled: conflict-free both ways
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const int k = rq * 4 + e;
                const float s1 = acc[1][k] + acc[2][k], d1 = acc[1][k] - acc[2][k];
                const float s2 = acc[3][k] + acc[4][k], d2 = acc[3][k] - acc[4][k];
                P0[e] = acc[0][k] + s1 + s2;               // A4^T = (1,1,1,1,1,0) (0,1,-1,2,-2,0) (0,1,1,4,4,0) (0,1,-1,8,-8,1)
                P1[e] = d1 + 2.f * d2;
                P2[e] = s1 + 4.f * s2;
                P3[e] = d1 + 8.f * d2 + (POLY ? 0.f : acc[5][k]);      // POLY: rows 0-3 of A5^T (no inf column)
            }
            *(f32x4*)(Pw + slot) = P0;
            *(f32x4*)(Pw + 1 * 32 * 32 + slot) = P1;
            *(f32x4*)(Pw + 2 * 32 * 32 + slot) = P2;
            *(f32x4*)(Pw + 3 * 32 * 32 + slot) = P3;
        }
    }
    __syncthreads();
    if constexpr (POLY) {
        const int le = lane_now(), q8 = le & 7, tt = le >> 3;
        const int tl = wj * 8 + tt;
        const float* Pr = smem + tl * 32 + ((q8 ^ ((tl >> 1) & 7)) << 2);
        const int ctr = ct >> 2, py = (ct >> 1) & 1, px = ct & 1;       // real channel tile, phase
        const f32x4 bias4 = *(const f32x4*)(a.bias + ctr * 32 + 4 * q8);
        const int eH = PERSIST ? m.s[seg].H : a.H, eW = PERSIST ? m.s[seg].W : a.W, pH = eH >> 1, pW = eW >> 1;
        float* const eout = PERSIST ? m.s[seg].out : a.out;
        rsrc_t dst;
        if constexpr (!BIG) dst = make_rsrc(eout + (size_t)img * eH * eW * a.cout, (unsigned)(eH * eW * a.cout) * 4u);
        else dst = make_rsrc(eout + ((size_t)img * eH + 2 * ty0) * eW * a.cout, 0x7ffffff0u);      // stores masked per lane
        const int gy = ty0 + W4P::TSTEP * (tl >> TCL), gx = tx0 + 3 * (tl & TCM);     // the tile's first output in the phase grid
        const int ry = (BIG ? 2 * W4P::TSTEP * (tl >> TCL) : 2 * gy) + py, ox = 2 * gx + px;
        const int cbyte = (ctr * 32 + 4 * q8) * 4;
        const float relu_lo = a.relu ? 0.f : -__builtin_inff();
        f32x4 P[4][4];
#pragma unroll
        for (int ap = 0; ap < 4; ++ap)
#pragma unroll
            for (int j = 0; j < 4; ++j) P[ap][j] = *(const f32x4*)(Pr + (j * 4 + ap) * (32 * 32));
        if constexpr (PERSIST) {
            __syncthreads();                               // every wave has its P values: the LDS image is free again
            raw_store(Rs);                                 // the next tile's first halo stage (loaded during this tile)
        }
#pragma unroll
        for (int ap = 0; ap < 4; ++ap) {
            f32x4 y[3];
            y[0] = P[ap][0] + P[ap][1] + P[ap][2] + bias4;          // A3 = columns (1,1,1,0), (0,1,-1,0), (0,1,1,1)
            y[1] = P[ap][1] - P[ap][2] + bias4;
            y[2] = P[ap][1] + P[ap][2] + P[ap][3] + bias4;
            const int off = (((ry + 2 * ap) * eW + ox) * a.cout) * 4 + cbyte;
            const bool rowok = gy + ap < pH;
#pragma unroll
            for (int b = 0; b < 3; ++b) {
#pragma unroll
                for (int e = 0; e < 4; ++e) y[b][e] = __builtin_amdgcn_fmed3f(y[b][e], relu_lo, __builtin_inff());
                buf_store4(dst, y[b], (rowok && gx + b < pW) ? off + b * 2 * a.cout * 4 : 0x7fffffff);
            }
        }
    } else {
        const int le = lane_now(), q8 = le & 7, tt = le >> 3;
        const int tl = wj * 8 + tt;
        const float* Pr = smem + tl * 32 + ((q8 ^ ((tl >> 1) & 7)) << 2);
        f32x4 bias4 = {0.f, 0.f, 0.f, 0.f};
        if (PERSIST || a.ksplit <= 1) bias4 = *(const f32x4*)(a.bias + ct * 32 + 4 * q8);      // (a split launch's bias is the combine kernel's)
        const int eH = PERSIST ? m.s[seg].H : a.H, eW = PERSIST ? m.s[seg].W : a.W;
        float* const eout = PERSIST ? m.s[seg].out : a.out + (size_t)ks * a.slab_stride;         // slab_stride = 0 unless split
        const int Ho = a.pool_out ? (eH + 1) >> 1 : eH, Wo = a.pool_out ? (eW + 1) >> 1 : eW;
        rsrc_t dst;
        if constexpr (!BIG) {
            dst = make_rsrc(eout + (size_t)img * Ho * Wo * a.cout, (unsigned)(Ho * Wo * a.cout) * 4u);
        } else {                                                           // the tile's first output row is the descriptor's origin
            const int orow0 = a.pool_out ? ty0 >> 1 : ty0;
            dst = make_rsrc(eout + ((size_t)img * Ho + orow0) * Wo * a.cout, 0x7ffffff0u);      // stores are masked per lane, never range-checked
        }
        const int oy = ty0 + 4 * (tl >> TCL), ox = tx0 + 2 * (tl & TCM);
        const int ry = BIG ? 4 * (tl >> TCL) : oy;                         // row counted from the descriptor's origin
        const int cbyte = (ct * 32 + 4 * q8) * 4;
        const bool colok0 = ox < eW, colok1 = ox + 1 < eW;
        const float relu_lo = a.relu ? 0.f : -__builtin_inff();
        f32x4 y[4][2], P[4][4];
#pragma unroll
        for (int ap = 0; ap < 4; ++ap)
#pragma unroll
            for (int j = 0; j < 4; ++j) P[ap][j] = *(const f32x4*)(Pr + (j * 4 + ap) * (32 * 32));
        if constexpr (PERSIST) {
            __syncthreads();                               // every wave has its P values: the LDS image is free again
            raw_store(Rs);                                 // the next tile's first halo stage (loaded during this tile)
        }
#pragma unroll
        for (int ap = 0; ap < 4; ++ap) {
            y[ap][0] = P[ap][0] + P[ap][1] + P[ap][2] + bias4;          // A2 = columns (1,1,1,0), (0,1,-1,-1)
            y[ap][1] = P[ap][1] - P[ap][2] - P[ap][3] + bias4;
            // ReLU as ONE v_med3_f32 per element, max(y, lo) = med3(y, lo, +inf) with lo = 0 or -inf (no ReLU): fmaxf costs two
            // instructions here (a canonicalising v_max before the real one) and the branch around it a dozen register copies
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                y[ap][0][e] = __builtin_amdgcn_fmed3f(y[ap][0][e], relu_lo, __builtin_inff());
                y[ap][1][e] = __builtin_amdgcn_fmed3f(y[ap][1][e], relu_lo, __builtin_inff());
            }
        }
        if (a.pool_out) {
#pragma unroll
            for (int h2 = 0; h2 < 2; ++h2) {               // two pool windows per tile: rows (0,1) and (2,3)
                const int r0 = oy + 2 * h2;
                f32x4 v = y[2 * h2][0];
                if (colok1) v = max4(v, y[2 * h2][1]);
                if (r0 + 1 < eH) {
                    v = max4(v, y[2 * h2 + 1][0]);
                    if (colok1) v = max4(v, y[2 * h2 + 1][1]);
                }
                const int off = BIG ? ((((ry >> 1) + h2) * Wo + (ox >> 1)) * a.cout) * 4 + cbyte
                                    : (((r0 >> 1) * Wo + (ox >> 1)) * a.cout) * 4 + cbyte;
                buf_store4(dst, v, (r0 < eH && colok0) ? off : 0x7fffffff);
            }
        } else {
#pragma unroll
            for (int ap = 0; ap < 4; ++ap) {
                const int off = (((ry + ap) * eW + ox) * a.cout) * 4 + cbyte;
                const bool rowok = oy + ap < eH;
                buf_store4(dst, y[ap][0], (rowok && colok0) ? off : 0x7fffffff);
                buf_store4(dst, y[ap][1], (rowok && colok1) ? off + a.cout * 4 : 0x7fffffff);
            }
        }
    }
    };

    // the main loop is instantiated once per transform column (WJ a compile-time constant inside): with a run-time column the compiler
    // turns the sign selection of the column combine into scalar branches around every group of adds, which splits the MFMA steps into
    // many basic blocks and leaves the transform outside the matrix pipe's shadow (measured on round 1's F(2x2,3x3) kernel: 1200-1300
    // cycles for a step with the transform against 630 without, ideal 512)
    auto main_loop = [&](auto WJC) {
        constexpr int WJ = decltype(WJC)::value;
        constexpr int cA = WJ == 0 ? 0 : 1, cB = WJ == 3 ? 3 : 2;
        asm volatile("; transform column %0" ::"n"(WJ));
        // patch rows 0-2, then 3-5: column combine f[a] = d[a][cA] +- d[a][cB]
        f32x4 dA[3], dB[3], f[6], o4, o5;
        auto xf_cols = [&](int a0) {
#pragma unroll
            for (int k = 0; k < 3; ++k) {
                if constexpr (WJ == 1) f[a0 + k] = dA[k] + dB[k];
                else if constexpr (WJ == 2) f[a0 + k] = dB[k] - dA[k];
                else f[a0 + k] = dA[k] - dB[k];
            }
        };
        // B4^T down the rows: (4,0,-5,0,1,0) (0,-4,-4,1,1,0) (0,4,-4,-1,1,0) (0,-2,-1,2,1,0) (0,2,-1,-2,1,0) (0,4,0,-5,0,1)
        auto rows_012 = [&](f32x4 (&q)[6]) {
            q[0] = 4.f * f[0] + (f[4] - 5.f * f[2]);
            const f32x4 t1 = f[4] - 4.f * f[2], t2 = f[3] - 4.f * f[1];
            q[1] = t1 + t2;
            q[2] = t1 - t2;
        };
        auto rows_34 = [&](f32x4 (&q)[6]) {
            const f32x4 t3 = f[4] - f[2], d31 = f[3] - f[1];
            q[3] = t3 + 2.f * d31;
            o4 = t3 - 2.f * d31;
        };
        auto rows_5 = [&]() { o5 = 4.f * f[1] + (f[5] - 5.f * f[3]); };

        f32x4 aq[6], t1, t2, t3, d31;
        int xaddr = 0;          // this lane's patch origin in the halo image (floats): computed once, held in a register
        {
            const int li = lane & 31, lh = lane >> 5;
            if constexpr (POLY) xaddr = 4 * (W4P::TSTEP * (li >> TCL) * W4P::RQ + (li & TCM) + lh * W4P::QQ);
            else xaddr = (4 * (li >> TCL)) * W4_PROW + (li & TCM) * W4_RSTR + 4 * lh;
            asm volatile("" : "+v"(xaddr));
        }
        // patch pixel (row a, column c of the 6 x 4 patch) relative to xaddr: plane c & 1, plane column + (c >> 1)
        auto poff = [=](int a, int c) {
            if constexpr (POLY) return 4 * (a * W4P::RQ + (c % 3) * W4P::SQ + c / 3);
            else return (c & 1) * W4_PLANE + a * W4_PROW + (c >> 1) * W4_RSTR;
        };
        auto xf_read3 = [&](const float* rb, int a0) {
#pragma unroll
            for (int k = 0; k < 3; ++k) {
                dA[k] = *(const f32x4*)(rb + xaddr + poff(a0 + k, cA));
                dB[k] = *(const f32x4*)(rb + xaddr + poff(a0 + k, cB));
            }
        };
        // one patch read (read index i = 0..5 of rows a0..a0+2: i / 2 = row, i & 1 = column cA / cB)
        auto xf_read1 = [&](const float* rb, int a0, auto II) {
            constexpr int i = decltype(II)::value, k = i / 2;
            if constexpr ((i & 1) == 0) dA[k] = *(const f32x4*)(rb + xaddr + poff(a0 + k, cA));
            else dB[k] = *(const f32x4*)(rb + xaddr + poff(a0 + k, cB));
        };

        // One chunk of 8 channels = 24 MFMAs in 24 scheduling regions of ONE MFMA plus its share of the chunk's other work
        // (issued right behind it, in its 64-cycle shadow).  Regions alternate between the accumulators of row positions 2d
        // and 2d+1 (d = region / 8): four back-to-back MFMAs on one accumulator are a dependent chain (tools/wino4_probe.py:
        // 412 cycles per 4 instead of 256 + issue overheads), and left to itself the scheduler builds exactly those chains.
        // XF: transform the next chunk's patches meanwhile; ST: the last third also writes the staged halo registers to LDS;
        // LD: the halo loads two stages ahead.  Weight ring: slot = row position, refilled as soon as its MFMAs have issued.
        auto chunk = [&](const float* nsrc, auto XFC, auto STC, auto LDC, int raw_soff, float* store_to, int wnext, auto FIRSTC) {
            constexpr bool do_xf = decltype(XFC)::value, st = decltype(STC)::value, ld = decltype(LDC)::value;
            // FIRST: the tile's first chunk - every accumulator's first MFMA takes a zero C operand (an inline constant) instead of
            // a cleared register: no 96 v_mov per tile (vector instructions cost this kernel matrix-pipe time)
            constexpr bool first = decltype(FIRSTC)::value;
            // A plain fp32 vector instruction takes matrix-pipe time on gfx950 (tools/probes/mfma_valu_probe.hip: a bare stream of fp32
            // MFMAs with 5 v_fma_f32 each reaches 113-119 TFLOP/s alternating 1 : 5 and 126-129 in bursts of 4 : 20 or more), but in this
            // kernel a burst schedule (the eight MFMAs of a pair of row positions back to back, then their regions' work) measured 0.6 %
            // SLOWER (3.64 vs 3.62 ms per config-2 step): what counts is the NUMBER of vector instructions per MFMA (see `sa`, `xaddr`),
            // not their placement.
            auto mf = [&](auto HH) {
                constexpr int h = decltype(HH)::value, m = h / 2, b = h & 1, d = m / 4, sidx = m & 3, r = 2 * d + b;
                if constexpr (first && sidx == 0) {
                    constexpr f32x16 zero = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
                    acc[r] = __builtin_amdgcn_mfma_f32_32x32x2f32(bq[r][sidx], aq[r][sidx], zero, 0, 0, 0);
                } else {
                    acc[r] = __builtin_amdgcn_mfma_f32_32x32x2f32(bq[r][sidx], aq[r][sidx], acc[r], 0, 0, 0);
                }
            };
            auto work = [&](auto HH) {
                constexpr int h = decltype(HH)::value;          // 0..23: mini-step m = h / 2 (d = m / 4, s = m % 4), b = second MFMA
                constexpr int m = h / 2, b = h & 1;
                // ---- weight ring: (this chunk) slots 4, 5 at mini-steps 0, 1; (next chunk) slots 0, 1 at 4, 5; slots 2, 3 at 8, 9 ----
                if constexpr (b == 0) {
                    if constexpr (m == 0) bq[4] = buf_load4(wsr, wvo, wso + 4 * 1024);
                    if constexpr (m == 1) bq[5] = buf_load4(wsr, wvo, wso + 5 * 1024);
                    if constexpr (m == 4) bq[0] = buf_load4(wsr, wvo, wnext);
                    if constexpr (m == 5) bq[1] = buf_load4(wsr, wvo, wnext + 1024);
                    if constexpr (m == 8) bq[2] = buf_load4(wsr, wvo, wnext + 2 * 1024);
                    if constexpr (m == 9) bq[3] = buf_load4(wsr, wvo, wnext + 3 * 1024);
                }
                // ---- halo loads two stages ahead, in the odd regions from 5 (5..15; POLY's nine items 5..21) ----
                if constexpr (ld && b == 1 && h >= 5 && h < 5 + 2 * RI) {
                    constexpr int k = (h - 5) / 2;
                    rawreg[k] = buf_load4(src, roff[k], tbase + raw_soff);
                }
                // ---- input transform of the next chunk ----
                if constexpr (do_xf) {
                    if constexpr (h >= 1 && h <= 6) xf_read1(nsrc, 0, std::integral_constant<int, h - 1>{});
                    if constexpr (h == 10) xf_cols(0);
                    if constexpr (h >= 11 && h <= 16) xf_read1(nsrc, 3, std::integral_constant<int, h - 11>{});
                    if constexpr (h == 20) xf_cols(3);
                    if constexpr (h == 21) { aq[0] = 4.f * f[0] + (f[4] - 5.f * f[2]); t1 = f[4] - 4.f * f[2]; t2 = f[3] - 4.f * f[1]; }   // fragments 0..3: dead since region 15
                    if constexpr (h == 22) { aq[1] = t1 + t2; aq[2] = t1 - t2; t3 = f[4] - f[2]; d31 = f[3] - f[1]; }
                    if constexpr (h == 23) { aq[3] = t3 + 2.f * d31; o4 = t3 - 2.f * d31; o5 = 4.f * f[1] + (f[5] - 5.f * f[3]); }
                }
                // ---- halo store of the stage loaded one stage ago ----
                if constexpr (st && h >= 23 - RI && h <= 22) *(f32x4*)((char*)store_to + sa[h - (23 - RI)]) = rawreg[h - (23 - RI)];
                if constexpr (do_xf && h == 23) { aq[4] = o4; aq[5] = o5; }
            };
            auto region = [&](auto HH) {
                mf(HH);
                work(HH);
                __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);       // the MFMA first, everything else behind it
                __builtin_amdgcn_sched_barrier(0);
            };
            [&]<int... H>(std::integer_sequence<int, H...>) { (region(std::integral_constant<int, H>{}), ...); }(std::make_integer_sequence<int, 24>{});
            wso += 6144;
        };
        constexpr std::true_type T{};
        constexpr std::false_type F{};

        // ---- prologue --------------------------------------------------------------------------------------------------------------
        raw_load(0);
        raw_store(Rs);
        __syncthreads();
        raw_load(W4_KR * 4);                                // stages past the end read neighbouring data or zeros, never consumed
        xf_read3(Rs, 0); xf_cols(0);
        xf_read3(Rs, 3); xf_cols(3);
        rows_012(aq); rows_34(aq); rows_5();
        aq[4] = o4; aq[5] = o5;

        if constexpr (!PERSIST) {
            // stages in pairs (even stage: reads buffer 0, fills buffer 1; odd stage: the reverse): every LDS address of the loop is a
            // register + an immediate (see the persistent form); the last pair is its first half when nst is even
            for (int s = 0; s + 1 < nst; s += 2) {
                chunk(Rs + CH1, T, T, F, 0, Rs + W4_RBUF, wso + 6144, F);        // channels 0..7; prepares 8..15; writes the next stage's halo
                __syncthreads();
                chunk(Rs + W4_RBUF, T, F, T, (s + 2) * W4_KR * 4, nullptr, wso + 6144, F);      // channels 8..15; prepares the next stage; loads two stages ahead
                if (s + 2 < nst) {
                    chunk(Rs + W4_RBUF + CH1, T, T, F, 0, Rs, wso + 6144, F);
                    __syncthreads();
                    chunk(Rs, T, F, T, (s + 3) * W4_KR * 4, nullptr, wso + 6144, F);
                }
            }
            chunk(Rs + ((nst - 1) & 1) * W4_RBUF + CH1, T, F, F, 0, nullptr, wso + 6144, F);
            chunk(Rs, F, F, F, 0, nullptr, wso + 6144, F);
        } else {
            int ntile = 0;
            for (;;) {
                // the tile after this one (or this one again when the list is exhausted: its loads are then never consumed)
                const int nitem = item + stride < hi ? item + stride : item;
                const int nseg = seg_of(nitem);
                const int nli = nitem - m.s[nseg].item0, ngtx = m.s[nseg].tiles_x, ntiles = ngtx * m.s[nseg].tiles_y;
                int nct_, npt, nimg;
                decode(nli, ntiles, m.s[nseg].n, nct_, npt, nimg);
                const int ntx0 = (npt % ngtx) * TILE_W, nty0 = (npt / ngtx) * TILE_H;
                const int wso_next = ((nct_ * 4 + wj) * nch) * 6144;
                // wave priority alternating per tile, in opposite phase for the two halves of the grid (see PERSIST above)
                if ((ntile + (int)((blockIdx.x >> 3) >= (stride >> 1))) & 1) __builtin_amdgcn_s_setprio(1);
                else __builtin_amdgcn_s_setprio(0);
                ++ntile;
                // The halo loads run two stages ahead, and the staging offsets (six vector registers, the scalar tile base, the source
                // descriptor) switch to the next tile at ONE straight-line point: behind the stage loop, in front of the tile's last two
                // chunks, whose first then requests the next tile's first stage (it still has that chunk's tail, a whole chunk and the
                // epilogue's exchange to arrive).  Round 2 switched inside the loop ("if (s == nst - 3)", two more call sites for
                // nst = 2 / 3): the registers then were loop-carried values redefined on one path, and the compiler kept two copies of
                // them, 12 v_mov per stage (3 % of the stage's vector instructions - which cost matrix-pipe time here) besides three
                // inlined copies of the offset code.  The price: the stage that has nothing left to request re-requests the tile's
                // last stage (six loads per thread and tile that hit in L1 / L2 and are never stored).
                auto next_halo = [&]() {
                    halo_offsets(ntx0, nty0, m.s[nseg].H, m.s[nseg].W, m.s[nseg].Ws, nseg, nct_);
                    src = src_of(m.s[nseg].in, m.s[nseg].Hs, m.s[nseg].Ws, nimg, nty0);
                };
                {   // stage 0, peeled: its first chunk starts the tile's accumulators (FIRST)
                    chunk(Rs + CH1, T, T, F, 0, Rs + W4_RBUF, wso + 6144, T);
                    __syncthreads();
                    chunk(Rs + W4_RBUF, T, F, T, min(2, nst - 1) * W4_KR * 4, nullptr, wso + 6144, F);
                }
                // stages 1 .. nst-2 in pairs (odd stage: reads buffer 1, fills buffer 0; even stage: the reverse), so that every LDS
                // address of the loop is a register + an immediate: with the buffer a run-time value the loop spent 8 vector
                // instructions per stage on `base + offset` (of 152; every one costs matrix-pipe time).  cin a multiple of 32 gives
                // whole pairs; otherwise the last pair is its first half.
                for (int s = 1; s + 1 < nst; s += 2) {
                    chunk(Rs + W4_RBUF + CH1, T, T, F, 0, Rs, wso + 6144, F);
                    __syncthreads();
                    chunk(Rs, T, F, T, min(s + 2, nst - 1) * W4_KR * 4, nullptr, wso + 6144, F);
                    if (s + 2 < nst) {
                        chunk(Rs + CH1, T, T, F, 0, Rs + W4_RBUF, wso + 6144, F);
                        __syncthreads();
                        chunk(Rs + W4_RBUF, T, F, T, min(s + 3, nst - 1) * W4_KR * 4, nullptr, wso + 6144, F);
                    }
                }
                next_halo();
                chunk(Rs + ((nst - 1) & 1) * W4_RBUF + CH1, T, F, T, 0, nullptr, wso + 6144, F);      // + the next tile's first halo stage
                chunk(Rs, F, F, F, 0, nullptr, wso_next, F);      // the ring's look-ahead continues in the next tile's weights
                wso = wso_next;
                __syncthreads();
                epilogue();                                     // of (ct, img, tx0, ty0); also writes the next tile's first halo stage
                if (item + stride >= hi) break;
                item += stride;
                ct = nct_; img = nimg; tx0 = ntx0; ty0 = nty0; seg = nseg;
                __syncthreads();                                // (the accumulators are not cleared: see FIRST)
                raw_load(W4_KR * 4);
                xf_read3(Rs, 0); xf_cols(0);
                xf_read3(Rs, 3); xf_cols(3);
                rows_012(aq); rows_34(aq); rows_5();
                aq[4] = o4; aq[5] = o5;
            }
        }
    };
    if (wj == 0) main_loop(std::integral_constant<int, 0>{});
    else if (wj == 1) main_loop(std::integral_constant<int, 1>{});
    else if (wj == 2) main_loop(std::integral_constant<int, 2>{});
    else main_loop(std::integral_constant<int, 3>{});
    if constexpr (PERSIST) return;
    __syncthreads();
    epilogue();
}

// Second half of a cin-split layer: out = [pool](relu(slab 0 + slab 1 + ... + bias)), the slabs added in that fixed order (bitwise
// reproducible; no atomics).  One thread per output pixel and channel quad; slabs and out are NHWC, the slabs at the conv's
// own size H x W, out at the pooled size when `pool` (MaxPool2d(2, 2, ceil_mode=True): windows clipped at the border).
__global__ __launch_bounds__(256) void splitk_combine_kernel(const float* __restrict__ slabs, size_t slab_stride, int S,
                                                             const float* __restrict__ bias, int relu, int pool, float* __restrict__ out,
                                                             int n, int H, int W, int cout) {
    const int Ho = pool ? (H + 1) >> 1 : H, Wo = pool ? (W + 1) >> 1 : W;
    const int cq = cout >> 2;
    const size_t total = (size_t)n * Ho * Wo * cq;
    const float lo = relu ? 0.f : -__builtin_inff();
    for (size_t idx = blockIdx.x * (size_t)blockDim.x + threadIdx.x; idx < total; idx += (size_t)gridDim.x * blockDim.x) {
        size_t t = idx;
        const int c4 = (int)(t % cq); t /= cq;
        const int xo = (int)(t % Wo); t /= Wo;
        const int yo = (int)(t % Ho);
        const int img = (int)(t / Ho);
        const f32x4 b4 = *(const f32x4*)(bias + 4 * c4);
        auto at = [&](int y, int x) {
            const float* p = slabs + (((size_t)img * H + y) * W + x) * cout + 4 * c4;
            f32x4 v = *(const f32x4*)p;
            for (int k = 1; k < S; ++k) v += *(const f32x4*)(p + (size_t)k * slab_stride);
            v += b4;
#pragma unroll
            for (int e = 0; e < 4; ++e) v[e] = __builtin_amdgcn_fmed3f(v[e], lo, __builtin_inff());
            return v;
        };
        f32x4 r;
        if (pool) {
            const int y0 = 2 * yo, x0 = 2 * xo;
            r = at(y0, x0);
            if (x0 + 1 < W) r = max4(r, at(y0, x0 + 1));
            if (y0 + 1 < H) {
                r = max4(r, at(y0 + 1, x0));
                if (x0 + 1 < W) r = max4(r, at(y0 + 1, x0 + 1));
            }
        } else {
            r = at(yo, xo);
        }
        *(f32x4*)(out + idx * 4) = r;
    }
}

int launch_pack_wino4(const float* w, float* p, int cin, int cout, hipStream_t s) {
    if (cin % 8 || cout % 32) { set_error("pack_wino4: cin %% 8 or cout %% 32 != 0 (%d, %d)", cin, cout); return ADAIN_EINVAL; }
    const size_t total = (size_t)cin * cout * 24;
    const int blocks = (int)((total + 255) / 256 < 4096 ? (total + 255) / 256 : 4096);
    hipLaunchKernelGGL(pack_wino4_kernel, dim3(blocks), dim3(256), 0, s, w, p, cin, cout);
    return check_launch("pack_wino4");
}

int launch_pack_up2x_poly(const float* w, float* p, int cin, int cout, hipStream_t s) {
    if (cin % 8 || cout % 32 || cin < 8 || cout < 32) { set_error("pack_up2x_poly: cin %% 8 or cout %% 32 != 0 (%d, %d)", cin, cout); return ADAIN_EINVAL; }
    const size_t total = (size_t)cin * cout * 96;
    const int blocks = (int)((total + 255) / 256 < 4096 ? (total + 255) / 256 : 4096);
    hipLaunchKernelGGL(pack_up2x_poly_kernel, dim3(blocks), dim3(256), 0, s, w, p, cin, cout);
    return check_launch("pack_up2x_poly");
}

// a per-image source or output tensor of 2 GiB or more needs the per-tile descriptors (BIG instantiations)
static bool wino4_big(const ConvArgs& a) {
    return (size_t)a.Hs * a.Ws * a.cin * 4 >= 0x7ffffff0ULL || (size_t)a.H * a.W * a.cout * 4 >= 0x7ffffff0ULL;
}

static int check_wino4_shape(const ConvArgs& a, int src_mode) {
    if (a.cin % W4_KR || a.cin < W4_KR) { set_error("conv3x3_wino4: cin %d not a multiple of 16", a.cin); return ADAIN_EINVAL; }
    if (a.cout % 32) { set_error("conv3x3_wino4: cout %d not a multiple of 32", a.cout); return ADAIN_EINVAL; }
    if (a.H < 2 || a.W < 2 || a.n < 1) { set_error("conv3x3_wino4: H, W must be >= 2, got %dx%d", a.H, a.W); return ADAIN_EINVAL; }
    // 32-bit offsets address a band of at most 18 source / 16 output rows (the taller tile geometry) from a per-tile descriptor: the
    // image itself may be of any size
    if ((size_t)a.Ws * a.cin * 4 * 18 >= 0x7ffffff0ULL || (size_t)a.W * a.cout * 4 * 16 >= 0x7ffffff0ULL) {
        set_error("conv3x3_wino4: a band of eighteen %d-channel source rows or sixteen %d-channel output rows of width %d reaches 2 GiB",
                  a.cin, a.cout, a.W);
        return ADAIN_EINVAL;
    }
    if ((size_t)a.cin * a.cout * 96 >= 0xffffffffULL) { set_error("conv3x3_wino4: packed weights must stay below 4 GiB"); return ADAIN_EINVAL; }
    if (src_mode == SRC_DIRECT) {
        if (a.Hs != a.H || a.Ws != a.W) { set_error("conv3x3_wino4: direct mode needs Hs==H, Ws==W"); return ADAIN_EINVAL; }
    } else if (src_mode == SRC_UP2X) {
        if (a.H != 2 * a.Hs || a.W != 2 * a.Ws) { set_error("conv3x3_wino4: up2x mode needs H==2Hs, W==2Ws"); return ADAIN_EINVAL; }
    } else {
        set_error("conv3x3_wino4: unsupported src_mode %d", src_mode);
        return ADAIN_EINVAL;
    }
    return 0;
}

// Channel tiles per group of the persistent walk: the largest divisor of cout / 32 whose transformed weights (cin x 32 G x 24
// floats) fit W4_L2_WEIGHT_BYTES of an XCD's 4 MB L2 (the rest is left to the halos and outputs streaming through).
constexpr size_t W4_L2_WEIGHT_BYTES = 3u << 20;
static int walk_group(int cin, int cout) {
    const int nct = cout / 32;
    int g = nct;
    while (g > 1 && (size_t)cin * 32 * g * 96 > W4_L2_WEIGHT_BYTES) --g;
    while (nct % g) --g;
    return g;
}

static long long persistent_grid() {
    const int cus = device_cu_count();
    if (cus <= 0) return 0;
    const long long pgrid = 2LL * cus;
    return pgrid - pgrid % 8;
}

// Tile geometry of a launch: 0 = 8 x 32 output pixels per workgroup tile (the tuned default), 1 = 16 x 16.  Both cost the same per
// tile, so the one that covers the launch's feature maps with fewer tiles wins; the default keeps ties and near-ties (1 %).
static int tile_h(int geo) { return geo ? 16 : 8; }
static int tile_w(int geo) { return geo ? 16 : 32; }
static long long geo_tiles(int geo, int n, int H, int W) {
    return (long long)n * ((H + tile_h(geo) - 1) / tile_h(geo)) * ((W + tile_w(geo) - 1) / tile_w(geo));
}
static int pick_geo(const ConvSeg* segs, int count) {
    long long t0 = 0, t1 = 0;
    for (int i = 0; i < count; ++i) {
        t0 += geo_tiles(0, segs[i].n, segs[i].H, segs[i].W);
        t1 += geo_tiles(1, segs[i].n, segs[i].H, segs[i].W);
    }
    return t1 * 101 < t0 * 100 ? 1 : 0;
}

// Rounds of the persistent grid that ONE image of a layer is worth: tiles of the geometry its launch would pick x channel tiles over
// the resident workgroups.  The encoder / decoder schedules (api.hip) use it to decide which layers of a batch of large frames run
// frame by frame and which over the whole batch.
double wino4_rounds_per_image(int H, int W, int cout) {
    const long long pgrid = persistent_grid();
    if (pgrid <= 0 || H < 1 || W < 1) return 0.0;
    ConvSeg s{};
    s.n = 1; s.H = H; s.W = W;
    const int geo = pick_geo(&s, 1);
    return (double)geo_tiles(geo, 1, H, W) * (cout / 32) / (double)pgrid;
}

// The 12 instantiations the generic layers launch: source mode DIRECT or UP2X, persistent or one-tile, and geometry 0, 1 or (BIG: per-tile
// descriptors for tensors of 2 GiB and more) 0 - the BIG build exists for the default geometry only (see w4_list).
template <int MODE, bool PERSIST>
static void w4_launch_mode(bool big, int geo, dim3 grid, hipStream_t s, const ConvArgs& a, const ConvSegs& m, int items) {
    if (big) hipLaunchKernelGGL((conv3x3_wino4_kernel<MODE, PERSIST, true, 0>), grid, dim3(256), 0, s, a, m, items);
    else if (geo) hipLaunchKernelGGL((conv3x3_wino4_kernel<MODE, PERSIST, false, 1>), grid, dim3(256), 0, s, a, m, items);
    else hipLaunchKernelGGL((conv3x3_wino4_kernel<MODE, PERSIST, false, 0>), grid, dim3(256), 0, s, a, m, items);
}
template <bool PERSIST>
static void w4_launch(int src_mode, bool big, int geo, dim3 grid, hipStream_t s, const ConvArgs& a, const ConvSegs& m, int items) {
    if (src_mode == SRC_UP2X) w4_launch_mode<SRC_UP2X, PERSIST>(big, geo, grid, s, a, m, items);
    else w4_launch_mode<SRC_DIRECT, PERSIST>(big, geo, grid, s, a, m, items);
}

// Cin split of a small launch.  A one-tile workgroup walks its whole cin loop alone (about 1.5 us per 16 channels, 8 us of launch,
// prologue and epilogue around it: tools/probes/small_frame_trace.py), and a workgroup's vector and matrix instructions share the
// SIMD's issue, so a second workgroup on a compute unit buys nothing: what a split can win is the compute units a launch leaves
// EMPTY.  S = the largest power of two with items x S <= compute units and at least 64 channels (4 stages) per workgroup.
static int wino4_ksplit(long long items, int cin) {
    const int cus = device_cu_count();
    int S = 1;
    while (S < 8 && items * (2 * S) <= cus && cin % (2 * S * W4_KR) == 0 && cin / (2 * S) >= 64) S *= 2;
    return S;
}
static long long wino4_items(int n, int H, int W, int cout, int* geo_out) {
    ConvSeg sg{};
    sg.n = n; sg.H = H; sg.W = W;
    const int geo = pick_geo(&sg, 1);
    if (geo_out) *geo_out = geo;
    return geo_tiles(geo, n, H, W) * (cout / 32);
}
// The slab workspace is S equal slabs of one output tensor each, nothing else: it has no layout value of its own, and its size is the
// kernel's (not rounded to 256 bytes; the networks round the block they keep it in, api.hip's net_plan).
size_t wino4_split_floats(int n, int H, int W, int cin, int cout) {
    if (n < 1 || H < 2 || W < 2 || cin % W4_KR || cout % 32) return 0;
    const int S = wino4_ksplit(wino4_items(n, H, W, cout, nullptr), cin);
    return S > 1 ? (size_t)S * n * H * W * cout : 0;
}

// The tile list of one launch of a layer over `count` segments: every segment's shape checked (ConvArgs `layer` with the segment's
// sizes), one tile geometry for all of them - the one with fewer tiles over all segments, or the default when any tensor reaches
// 2 GiB (the BIG build exists for that geometry only) - and each segment's tiles and first item.  `a` = `layer` with segment 0's
// geometry; `items` = tiles x channel tiles over all segments.
struct W4List {
    ConvArgs a;
    ConvSegs m;
    bool big;
    int geo;
    long long items;
};
static void set_seg(ConvArgs& a, const ConvSeg& g) {
    a.in = g.in; a.out = g.out; a.n = g.n; a.H = g.H; a.W = g.W; a.Hs = g.Hs; a.Ws = g.Ws;
}
static int w4_list(const ConvArgs& layer, const ConvSeg* segs, int count, int src_mode, W4List& t) {
    t.a = layer;
    t.m = ConvSegs{};
    t.m.count = count;
    t.m.ctg = walk_group(layer.cin, layer.cout);
    t.big = false;
    for (int i = 0; i < count; ++i) {
        set_seg(t.a, segs[i]);
        if (check_wino4_shape(t.a, src_mode)) return ADAIN_EINVAL;
        t.big = t.big || wino4_big(t.a);
    }
    t.geo = t.big ? 0 : pick_geo(segs, count);
    t.items = 0;
    for (int i = 0; i < count; ++i) {
        ConvSeg& g = t.m.s[i];
        g = segs[i];
        g.tiles_x = (g.W + tile_w(t.geo) - 1) / tile_w(t.geo);
        g.tiles_y = (g.H + tile_h(t.geo) - 1) / tile_h(t.geo);
        g.item0 = (int)t.items;
        t.items += (long long)g.tiles_x * g.tiles_y * (layer.cout / 32) * g.n;
    }
    set_seg(t.a, t.m.s[0]);
    t.a.tiles_x = t.m.s[0].tiles_x;
    t.a.tiles_y = t.m.s[0].tiles_y;
    return 0;
}

int launch_conv3x3_wino4(const ConvArgs& a0, int src_mode, hipStream_t s, SplitWs split) {
    ConvArgs layer = a0;
    layer.ksplit = 1; layer.cin_sub = layer.cin; layer.slab_stride = 0;
    const ConvSeg seg{layer.in, layer.out, layer.n, layer.H, layer.W, layer.Hs, layer.Ws, 0, 0, 0};
    W4List t;
    if (w4_list(layer, &seg, 1, src_mode, t)) return ADAIN_EINVAL;
    const ConvArgs& a = t.a;
    const long long blocks = t.items;
    if (blocks <= 0 || blocks > 0x7fffffffLL) { set_error("conv3x3_wino4: bad grid %lld", blocks); return ADAIN_EINVAL; }
    // persistent form whenever the launch has at least two tiles per resident workgroup (and cin is at most 2^20): +2-3 % on most
    // layer shapes, +1.1 % on the config-2 step
    const long long pgrid = persistent_grid();
    if (pgrid <= 0) { set_error("conv3x3_wino4: device query failed"); return ADAIN_EINVAL; }
    const bool persist = a.cin <= (1 << 20) && a.cin >= 2 * W4_KR && pgrid >= 8 && blocks >= 2 * pgrid;
    const int items = (int)blocks;
    if (persist) {
        w4_launch<true>(src_mode, t.big, t.geo, dim3((unsigned)pgrid), s, a, t.m, items);
        return check_launch("conv3x3_wino4");
    }
    const int S = (split.slab && !t.big) ? wino4_ksplit(blocks, a.cin) : 1;
    if (S > 1) {
        const size_t slab = (size_t)a.n * a.H * a.W * a.cout;
        if (int rc = check_workspace("conv3x3_wino4 (cin split)", split.slab, split.floats * sizeof(float), (size_t)S * slab * sizeof(float), 1)) return rc;
        ConvArgs p = a;                  // first half: S workgroups per (tile, channel tile), partial sums into the slabs
        p.ksplit = S; p.cin_sub = a.cin / S; p.slab_stride = slab;
        p.out = split.slab; p.relu = 0; p.pool_out = 0;
        w4_launch<false>(src_mode, false, t.geo, dim3((unsigned)(blocks * S)), s, p, t.m, items * S);
        if (int r = check_launch("conv3x3_wino4(split)")) return r;
        const int Ho = a.pool_out ? (a.H + 1) / 2 : a.H, Wo = a.pool_out ? (a.W + 1) / 2 : a.W;
        const size_t total = (size_t)a.n * Ho * Wo * (a.cout / 4);
        const unsigned cb = (unsigned)((total + 255) / 256 < 4096 ? (total + 255) / 256 : 4096);
        hipLaunchKernelGGL(splitk_combine_kernel, dim3(cb), dim3(256), 0, s, (const float*)split.slab, slab, S, a.bias, a.relu, a.pool_out, a.out,
                           a.n, a.H, a.W, a.cout);
        return check_launch("conv3x3_wino4(combine)");
    }
    w4_launch<false>(src_mode, t.big, t.geo, dim3((unsigned)blocks), s, a, t.m, items);
    return check_launch("conv3x3_wino4");
}

int launch_conv3x3_wino4_multi(const ConvArgs& layer, const ConvSeg* segs, int count, int src_mode, hipStream_t s, const SplitWs* split) {
    if (count < 1 || count > MAX_CONV_SEGS) { set_error("conv3x3_wino4_multi: 1..%d segments, got %d", MAX_CONV_SEGS, count); return ADAIN_EINVAL; }
    for (int i = 0; i < count; ++i)
        if (!segs[i].in || !segs[i].out) { set_error("conv3x3_wino4_multi: null pointer in segment %d", i); return ADAIN_EINVAL; }
    W4List t;
    if (w4_list(layer, segs, count, src_mode, t)) return ADAIN_EINVAL;
    if (t.items > 0x7fffffffLL) { set_error("conv3x3_wino4_multi: too many tiles"); return ADAIN_EINVAL; }
    const long long pgrid = persistent_grid();
    if (pgrid <= 0) { set_error("conv3x3_wino4: device query failed"); return ADAIN_EINVAL; }
    if (count == 1 || layer.cin < 2 * W4_KR || pgrid < 8 || t.items < 2 * pgrid) {
        // not enough work for a shared persistent list (or a single segment): one launch per segment
        ConvArgs a = layer;
        for (int i = 0; i < count; ++i) {
            set_seg(a, segs[i]);
            if (int r = launch_conv3x3_wino4(a, src_mode, s, split ? split[i] : SplitWs{nullptr, 0})) return r;
        }
        return 0;
    }
    // the kernel reads its geometry from the segments; the ConvArgs copy carries the layer (weights, bias, cin, cout, flags)
    w4_launch<true>(src_mode, t.big, t.geo, dim3((unsigned)pgrid), s, t.a, t.m, (int)t.items);
    return check_launch("conv3x3_wino4(multi)");
}

}  // namespace adain

namespace adain {
// The decoder's up layers (nearest 2x upsample + reflection pad + 3x3 conv) as four phase convolutions of the source (W4P): weights
// from launch_pack_up2x_poly; (a.H, a.W) = 2 (a.Hs, a.Ws).  Never split along cin (the latency schedule runs these layers whole).
int launch_conv3x3_up2x_poly(const ConvArgs& a0, hipStream_t s) {
    ConvArgs a = a0;
    a.ksplit = 1; a.cin_sub = a.cin; a.slab_stride = 0;
    if (a.cin % W4_KR || a.cin < W4_KR) { set_error("conv3x3_up2x_poly: cin %d not a multiple of 16", a.cin); return ADAIN_EINVAL; }
    if (a.cout % 32 || a.cout < 32) { set_error("conv3x3_up2x_poly: cout %d not a multiple of 32", a.cout); return ADAIN_EINVAL; }
    if (a.n < 1 || a.Hs < 1 || a.Ws < 1 || a.H != 2 * a.Hs || a.W != 2 * a.Ws) {
        set_error("conv3x3_up2x_poly: needs n >= 1, a source of at least 1x1 and H == 2 Hs, W == 2 Ws (got %d: %dx%d -> %dx%d)", a.n, a.Hs, a.Ws, a.H, a.W);
        return ADAIN_EINVAL;
    }
    if (a.pool_out) { set_error("conv3x3_up2x_poly: no fused output pool"); return ADAIN_EINVAL; }
    // per-tile descriptors address a band of 19 source / 32 output rows with 32-bit offsets
    if ((size_t)a.Ws * a.cin * 4 * 19 >= 0x7ffffff0ULL || (size_t)a.W * a.cout * 4 * 32 >= 0x7ffffff0ULL) {
        set_error("conv3x3_up2x_poly: a band of 19 source or 32 output rows reaches 2 GiB");
        return ADAIN_EINVAL;
    }
    if ((size_t)a.cin * a.cout * 384 >= 0xffffffffULL) { set_error("conv3x3_up2x_poly: packed weights must stay below 4 GiB"); return ADAIN_EINVAL; }
    const bool big = wino4_big(a);
    a.tiles_x = (a.Ws + W4P::TILE_W - 1) / W4P::TILE_W;
    a.tiles_y = (a.Hs + W4P::TILE_H - 1) / W4P::TILE_H;
    ConvSegs m{};
    m.count = 1;
    m.s[0] = ConvSeg{a.in, a.out, a.n, a.H, a.W, a.Hs, a.Ws, a.tiles_x, a.tiles_y, 0};
    m.ctg = walk_group(a.cin, 4 * a.cout);           // virtual channel tiles 4 ct + phase: the phases of a channel tile share halos
    const long long blocks = (long long)a.tiles_x * a.tiles_y * (4 * a.cout / 32) * a.n;
    if (blocks <= 0 || blocks > 0x7fffffffLL) { set_error("conv3x3_up2x_poly: bad grid %lld", blocks); return ADAIN_EINVAL; }
    // One tile per workgroup: the persistent form's loop-carried next-tile state does not fit beside nine staging items per thread
    // (the build spills; the one-tile form holds 246 registers and no scratch).
    const dim3 g((unsigned)blocks);
    if (big) hipLaunchKernelGGL((conv3x3_wino4_kernel<SRC_UP2X_POLY, false, true>), g, dim3(256), 0, s, a, m, (int)blocks);
    else hipLaunchKernelGGL((conv3x3_wino4_kernel<SRC_UP2X_POLY, false, false>), g, dim3(256), 0, s, a, m, (int)blocks);
    return check_launch("conv3x3_up2x_poly");
}
}  // namespace adain
