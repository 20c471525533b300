// A palette of at most 256 colours chosen on the device (gfx950) from the frames themselves: the stage in front of csrc/palette.hip and
// csrc/gif.hip for a full-colour clip (Style_3DGS/render.py:29-33 create_gif hands Pillow RGB renders, and Pillow quantises every frame
// to an adaptive palette).  NOT Pillow's palette: a median cut of its own whose result is a function of the pixels alone.  The rules,
// restated in tests/quantize_ref.py:
//
//   1. Cells.  A pixel (r, g, b) falls into cell (r >> 3, g >> 3, b >> 3) of a 32 x 32 x 32 grid.  A cell has five integer moments: the
//      count w, Sr, Sg, Sb and Q = sum of r^2 + g^2 + b^2.  One grid for the whole call (ADAIN_QUANTIZE_GLOBAL: one palette for the n
//      frames) or one per frame (ADAIN_QUANTIZE_PER_FRAME).
//   2. Boxes are inclusive cell ranges and always tight: each of the six faces touches a non-empty cell.  Box 0 is the tight bound of all
//      non-empty cells.  A box's moments are the sums over its cells; its error is E = Q - (Sr^2 + Sg^2 + Sb^2) / w, an exact rational.
//   3. Loop while there are fewer than K boxes.  Candidates are the boxes with more than one cell along some axis; without one the loop
//      stops and used < K.  The candidate with the largest E is split, compared exactly: E_i > E_j as (w_i Q_i - |S_i|^2) w_j against
//      (w_j Q_j - |S_j|^2) w_i, 128-bit unsigned products (numerators below 2^82, products below 2^114); no 128-bit division.  The
//      lowest box index wins a tie.
//   4. Split axis: the longest side in cells; among equal sides g, then r, then b.
//   5. Cut position: with the slab counts m[lo..hi] along that axis, k is the smallest t with m[lo] + ... + m[t] >= ceil(w / 2), then
//      k = min(k, hi - 1).  [lo..k] keeps the box's index, [k + 1..hi] is appended; both are tightened.
//   6. Entry i is (2 S_c + w) / (2 w), rounded down, per channel, for box i in index order; entries used..255 are zero; used is the number
//      of boxes.
// Two colours in one cell are merged, so a frame with fewer than K non-empty cells gets used < K from these rules however many colours
// it has; the rounds of k-means a call may ask for behind them (rules 7-11, csrc/quantize_refine.hip, mode's ADAIN_QUANTIZE_REFINE bits)
// move the entries to their pixels' centres and fill the unused ones.
//
// Stages (a memset and 3 launches, whatever n; nothing allocates or waits):
//   hist : the frames' bytes once.  A thread takes 16 pixels from three 16-byte loads (the pixels in front of the first 16-byte
//          boundary and behind the last whole 48 bytes go one to a thread), merges runs of equal consecutive cells in registers, a wave
//          whose lanes all hold one cell sums them by lane shuffles, and what is left goes into the workgroup's LDS table: a hash of cell
//          -> five accumulators, open addressing with a bounded probe.  The table is added to the grid - integer atomics, so the sums do
//          not depend on the order - when it is three quarters full, before a 32-bit accumulator could overflow, and at the end; a run
//          that finds no slot within the probe bound goes to the grid directly.  No float atomics, no spin-wait, no flags.
//   sat  : inclusive prefix sums of every plane over (r, g, b) in place, a workgroup per plane and palette, three passes of 1024 lines.
//          Then a box's moments are 8 reads a plane and a slab count is 8 reads.
//   cut  : a workgroup per palette, K - 1 sequential steps with barriers inside the workgroup only: the choice is a tree reduction over
//          the boxes' keys in LDS, the marginal one slab count per thread, the two tightenings one slab count per thread (2 boxes x 3
//          axes x 32 positions), the moments one plane per thread.  The rule functions are quantize_cut.h's, shared with the host.
#include "common.h"
#include "quantize_refine.h"

namespace adain {
namespace {

using quant::Box;
using quant::Grid;
using quant::Key;
typedef unsigned long long ull;

// ---- hist ---------------------------------------------------------------------------------------------------------------------------------
constexpr int HIST_THREADS = 256;
constexpr int GROUP = 16;                                  // pixels a thread takes at once: 48 bytes, three aligned 16-byte loads
constexpr int TILE = HIST_THREADS * GROUP;                 // pixels a workgroup takes between two looks at its table
constexpr int SLOTS = 1024;                                // 28 KiB of LDS: five workgroups to a CU
constexpr int PROBES = 8;
constexpr uint32_t FLUSH_AT = SLOTS * 3 / 4;
constexpr int FLUSH_TILES = 1024;                          // 2^22 pixels: 255 x 2^22 stays below 2^32 in a slot's 32-bit sums
constexpr uint32_t NO_CELL = 0xffffffffu;
constexpr int MAX_HIST_GROUPS = 1024;                      // workgroups of a launch, over all palettes, about

struct HistShared {
    uint32_t key[SLOTS], w[SLOTS], s[3][SLOTS];
    ull q[SLOTS];
    uint32_t filled;
};

// a run of `cnt` pixels of one cell
struct Run {
    uint32_t cell, cnt, s[3], q;
};

__device__ __forceinline__ void add_to_grid(const Grid& g, uint32_t cell, uint32_t cnt, uint32_t s0, uint32_t s1, uint32_t s2, ull q) {
    atomicAdd(&g.w[cell], cnt);
    atomicAdd((ull*)&g.s[0][cell], (ull)s0);
    atomicAdd((ull*)&g.s[1][cell], (ull)s1);
    atomicAdd((ull*)&g.s[2][cell], (ull)s2);
    atomicAdd((ull*)&g.q[cell], q);
}

__device__ __forceinline__ void add_run(HistShared& sh, const Grid& g, const Run& r) {
    uint32_t slot = (r.cell * 2654435761u) >> 22;          // 10 bits
    for (int probe = 0; probe < PROBES; ++probe, slot = (slot + 1) & (SLOTS - 1)) {
        uint32_t held = *(volatile uint32_t*)&sh.key[slot];          // a slot's key stays until the table is flushed, behind a barrier
        if (held != r.cell) {
            if (held != NO_CELL) continue;
            held = atomicCAS(&sh.key[slot], NO_CELL, r.cell);
            if (held == NO_CELL) atomicAdd(&sh.filled, 1u);
            else if (held != r.cell) continue;
        }
        atomicAdd(&sh.w[slot], r.cnt);
        atomicAdd(&sh.s[0][slot], r.s[0]);
        atomicAdd(&sh.s[1][slot], r.s[1]);
        atomicAdd(&sh.s[2][slot], r.s[2]);
        atomicAdd(&sh.q[slot], (ull)r.q);
        return;
    }
    add_to_grid(g, r.cell, r.cnt, r.s[0], r.s[1], r.s[2], r.q);
}

__device__ __forceinline__ void take_pixel(HistShared& sh, const Grid& g, Run& run, uint32_t r, uint32_t gr, uint32_t b) {
    const uint32_t cell = quant::cell_of(r, gr, b);
    if (run.cnt && cell != run.cell) {
        add_run(sh, g, run);
        run.cnt = 0;
    }
    if (!run.cnt) run.cell = cell, run.s[0] = run.s[1] = run.s[2] = run.q = 0;
    ++run.cnt;
    run.s[0] += r, run.s[1] += gr, run.s[2] += b;
    run.q += r * r + gr * gr + b * b;
}

// The run every thread is left with (cnt 0: none; at most GROUP pixels).  Every lane of the wave calls it.
__device__ __forceinline__ void add_last_run(HistShared& sh, const Grid& g, Run run) {
    const ull have = __ballot(run.cnt > 0);
    if (!have) return;
    const uint32_t first = (uint32_t)__shfl((int)run.cell, __builtin_ctzll(have));
    if (__all(run.cnt == 0 || run.cell == first)) {          // a flat stretch: one addition for the wave
        if (run.cnt == 0) run.s[0] = run.s[1] = run.s[2] = run.q = 0;
        for (int d = 32; d > 0; d >>= 1) {
            run.cnt += (uint32_t)__shfl_xor((int)run.cnt, d);
            run.s[0] += (uint32_t)__shfl_xor((int)run.s[0], d);
            run.s[1] += (uint32_t)__shfl_xor((int)run.s[1], d);
            run.s[2] += (uint32_t)__shfl_xor((int)run.s[2], d);
            run.q += (uint32_t)__shfl_xor((int)run.q, d);          // 64 x 16 x 195075 is below 2^32
        }
        run.cell = first;
        if ((threadIdx.x & 63) == 0) add_run(sh, g, run);
    } else if (run.cnt) {
        add_run(sh, g, run);
    }
}

__device__ __forceinline__ void flush_table(HistShared& sh, const Grid& g) {
    for (int i = threadIdx.x; i < SLOTS; i += HIST_THREADS) {
        const uint32_t cell = sh.key[i];
        if (cell == NO_CELL) continue;
        add_to_grid(g, cell, sh.w[i], sh.s[0][i], sh.s[1][i], sh.s[2][i], sh.q[i]);
        sh.key[i] = NO_CELL, sh.w[i] = sh.s[0][i] = sh.s[1][i] = sh.s[2][i] = 0, sh.q[i] = 0;
    }
    if (threadIdx.x == 0) sh.filled = 0;
}

// grid (workgroups, P).  Palette p's pixels: `pixels` of them from src + p * pixels * 3, at any byte address.  The grids are zero on entry.
__global__ __launch_bounds__(HIST_THREADS) void quantize_hist_kernel(const uint8_t* __restrict__ src, size_t pixels, void* workspace) {
    __shared__ HistShared sh;
    const int t = threadIdx.x;
    const Grid g = quant::grid_at(workspace, blockIdx.y);
    const uint8_t* base = src + (size_t)blockIdx.y * pixels * 3;
    for (int i = t; i < SLOTS; i += HIST_THREADS) sh.key[i] = NO_CELL, sh.w[i] = sh.s[0][i] = sh.s[1][i] = sh.s[2][i] = 0, sh.q[i] = 0;
    if (t == 0) sh.filled = 0;
    __syncthreads();
    // pixel p starts at base + 3 p: the first one on a 16-byte boundary is p = -base * 11 mod 16 (3 * 11 = 33 = 1 mod 16)
    const size_t head = min(pixels, (size_t)(((0 - (uintptr_t)base) * 11) & 15));
    const size_t groups = (pixels - head) / GROUP, tail0 = head + groups * GROUP;
    Run run;
    run.cnt = 0;
    if (blockIdx.x == 0) {          // the pixels outside the aligned body, fewer than 16 at either end
        size_t p = pixels;
        if ((size_t)t < head) p = t;
        else if (t >= 16 && tail0 + (t - 16) < pixels) p = tail0 + (t - 16);
        if (p < pixels) take_pixel(sh, g, run, base[3 * p], base[3 * p + 1], base[3 * p + 2]);
        add_last_run(sh, g, run);
        run.cnt = 0;
    }
    const size_t tiles = (groups + HIST_THREADS - 1) / HIST_THREADS;
    int since = 0;
    for (size_t tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
        const size_t group = tile * HIST_THREADS + t;
        if (group < groups) {
            const uint4* p = (const uint4*)(base + 3 * (head + group * GROUP));
            const uint4 a = p[0], b = p[1], c = p[2];
            const uint32_t word[12] = {a.x, a.y, a.z, a.w, b.x, b.y, b.z, b.w, c.x, c.y, c.z, c.w};
#pragma unroll
            for (int i = 0; i < GROUP; ++i) {
                const int e = 3 * i;
                take_pixel(sh, g, run, (word[e >> 2] >> (8 * (e & 3))) & 255u, (word[(e + 1) >> 2] >> (8 * ((e + 1) & 3))) & 255u,
                           (word[(e + 2) >> 2] >> (8 * ((e + 2) & 3))) & 255u);
            }
        }
        add_last_run(sh, g, run);
        run.cnt = 0;
        __syncthreads();
        const bool flush = sh.filled >= FLUSH_AT || ++since >= FLUSH_TILES;          // the same answer in every thread
        __syncthreads();
        if (flush) {
            flush_table(sh, g);
            since = 0;
            __syncthreads();
        }
    }
    __syncthreads();
    flush_table(sh, g);
}

// ---- sat ----------------------------------------------------------------------------------------------------------------------------------
// grid (5, P), 1024 threads: plane blockIdx.x of palette blockIdx.y.  A workgroup's own stores are visible to it behind a barrier.
__global__ __launch_bounds__(1024) void quantize_sat_kernel(void* workspace) {
    const Grid g = quant::grid_at(workspace, blockIdx.y);
    const int plane = blockIdx.x;
    for (int pass = 0; pass < 3; ++pass) {
        if (plane == 0) quant::scan_pass(g.w, pass, (int)threadIdx.x);
        else quant::scan_pass(plane == 4 ? g.q : g.s[plane - 1], pass, (int)threadIdx.x);
        __syncthreads();
    }
}

// ---- cut ----------------------------------------------------------------------------------------------------------------------------------
constexpr int CUT_THREADS = 256;
static_assert(CUT_THREADS == quant::MAX_COLOURS && CUT_THREADS >= 2 * 3 * quant::SIDE, "a thread per box and per slab of two boxes");

struct CutShared {
    Key key[CUT_THREADS];
    uint64_t s[3][CUT_THREADS];
    Box box[CUT_THREADS];
    int pick[CUT_THREADS];
    uint32_t m[quant::SIDE];
    uint32_t mask[2][3];
    uint64_t moment[2][5];
    Box loose[2];
};

// `count` loose boxes in sh.loose (each holds a pixel) become the tight boxes sh.box[dest0], sh.box[dest1] with their keys.  sh.mask is
// zero on entry and on return.  Every thread calls it.
__device__ __forceinline__ void settle(CutShared& sh, const Grid& g, int count, int dest0, int dest1) {
    const int t = threadIdx.x;
    if (t < count * 3 * quant::SIDE) {
        const int b = t / (3 * quant::SIDE), a = t / quant::SIDE % 3, pos = t % quant::SIDE;
        const Box x = sh.loose[b];
        if (pos >= x.lo[a] && pos <= x.hi[a] && quant::slab_count(g.w, x, a, pos)) atomicOr(&sh.mask[b][a], 1u << pos);
    }
    __syncthreads();
    if (t < count * 5) {
        const int b = t / 5, plane = t % 5;
        Box x;
        for (int a = 0; a < 3; ++a) quant::tight_range(sh.mask[b][a], &x.lo[a], &x.hi[a]);
        sh.moment[b][plane] = plane == 0 ? quant::box_sum(g.w, x) : quant::box_sum(plane == 4 ? g.q : g.s[plane - 1], x);
    }
    __syncthreads();
    if (t < count) {
        const int dest = t ? dest1 : dest0;
        Box x;
        for (int a = 0; a < 3; ++a) quant::tight_range(sh.mask[t][a], &x.lo[a], &x.hi[a]), sh.mask[t][a] = 0;
        quant::Moments mo;
        mo.w = sh.moment[t][0], mo.s[0] = sh.moment[t][1], mo.s[1] = sh.moment[t][2], mo.s[2] = sh.moment[t][3], mo.q = sh.moment[t][4];
        sh.box[dest] = x;
        for (int c = 0; c < 3; ++c) sh.s[c][dest] = mo.s[c];
        Key k;
        k.num = quant::error_numerator(mo), k.w = mo.w, k.splittable = quant::splittable(x);
        sh.key[dest] = k;
    }
    __syncthreads();
}

// grid P.  palettes: [P][256][3]; used: [P]
__global__ __launch_bounds__(CUT_THREADS) void quantize_cut_kernel(void* workspace, int K, uint8_t* __restrict__ palettes, int32_t* __restrict__ used) {
    __shared__ CutShared sh;
    const int t = threadIdx.x;
    const Grid g = quant::grid_at(workspace, blockIdx.x);
    if (t < 6) sh.mask[t / 3][t % 3] = 0;
    if (t == 0) sh.loose[0] = Box{{0, 0, 0}, {quant::SIDE - 1, quant::SIDE - 1, quant::SIDE - 1}};
    __syncthreads();
    settle(sh, g, 1, 0, 0);
    int boxes = 1;
    while (boxes < K) {
        // the box to split: a tree over the boxes' indices; an index from `boxes` on stands for no box
        sh.pick[t] = t;
        __syncthreads();
        for (int step = CUT_THREADS / 2; step > 0; step >>= 1) {
            if (t < step) {
                const int a = sh.pick[t], b = sh.pick[t + step];
                if (b < boxes && (a >= boxes || quant::chosen_over(sh.key[b], b, sh.key[a], a))) sh.pick[t] = b;
            }
            __syncthreads();
        }
        const int best = sh.pick[0];          // below `boxes`: box 0 exists
        if (!sh.key[best].splittable) break;          // the same in every thread
        const Box x = sh.box[best];
        const int axis = quant::split_axis(x), lo = x.lo[axis], hi = x.hi[axis];
        if (t < quant::SIDE) sh.m[t] = t >= lo && t <= hi ? (uint32_t)quant::slab_count(g.w, x, axis, t) : 0u;
        __syncthreads();
        if (t == 0) {
            const int k = quant::cut_position(sh.m, lo, hi, sh.key[best].w);
            sh.loose[0] = sh.loose[1] = x;
            sh.loose[0].hi[axis] = (int8_t)k, sh.loose[1].lo[axis] = (int8_t)(k + 1);
        }
        __syncthreads();
        settle(sh, g, 2, best, boxes);
        ++boxes;
    }
    __syncthreads();
    uint8_t* pal = palettes + (size_t)blockIdx.x * quant::MAX_COLOURS * 3;
    for (int c = 0; c < 3; ++c) pal[3 * t + c] = t < boxes ? quant::entry(sh.s[c][t], sh.key[t].w) : (uint8_t)0;
    if (t == 0) used[blockIdx.x] = boxes;
}

// ---- the call -----------------------------------------------------------------------------------------------------------------------------
struct QuantPlan {
    size_t palettes, pixels;          // pixels per palette
    unsigned hist_groups;             // workgroups per palette
    int rounds;                       // of refinement (csrc/quantize_refine.hip): mode >> 8
    unsigned assign_groups;
    size_t o_grids, o_refine, total;
    size_t clear_bytes;               // from o_grids: the grids and, behind them, the refinement's accumulators
};

// mode = ADAIN_QUANTIZE_GLOBAL or _PER_FRAME in its low byte, or-ed with ADAIN_QUANTIZE_REFINE(rounds)
const char* check_quantize_shape(int n, int h, int w, int mode) {
    static_assert(ADAIN_QUANTIZE_REFINE_MAX == 64, "the text below names the bound");
    const int rounds = mode >> 8, which = mode & 0xff;
    if (mode < 0 || rounds > ADAIN_QUANTIZE_REFINE_MAX || (which != ADAIN_QUANTIZE_GLOBAL && which != ADAIN_QUANTIZE_PER_FRAME))
        return "mode other than ADAIN_QUANTIZE_GLOBAL (0) and ADAIN_QUANTIZE_PER_FRAME (1), or-ed with ADAIN_QUANTIZE_REFINE(0..64)";
    mode = which;
    if (n < 1 || n > 65535) return "n outside 1..65535";
    if (h < 1 || w < 1) return "empty frames: height or width below 1";
    const uint64_t frame = (uint64_t)h * (uint64_t)w;          // below 2^62
    if (frame >> 32 || (mode == ADAIN_QUANTIZE_GLOBAL && (frame * (uint64_t)n) >> 32)) return "2^32 or more pixels for one palette (the counts are 32 bits)";
    return nullptr;
}

// The one layout of a call
QuantPlan make_quant_plan(int n, int h, int w, int mode) {
    QuantPlan p{};
    p.rounds = mode >> 8;
    mode &= 0xff;
    p.palettes = mode == ADAIN_QUANTIZE_GLOBAL ? 1 : (size_t)n;
    p.pixels = (size_t)h * w * (mode == ADAIN_QUANTIZE_GLOBAL ? (size_t)n : 1);
    // a workgroup clears and flushes a table of SLOTS: it takes two tiles at least where there are two
    const size_t tiles = (p.pixels + TILE - 1) / TILE, share = max((size_t)1, MAX_HIST_GROUPS / p.palettes);
    p.hist_groups = (unsigned)max((size_t)1, min((tiles + 1) / 2, share));
    Carve ws;
    p.o_grids = ws.take(p.palettes * quant::GRID_BYTES);
    p.clear_bytes = p.palettes * quant::GRID_BYTES;
    if (p.rounds) {          // without rounds the layout is the median cut's alone
        p.assign_groups = quantize_refine_groups(p.palettes, p.pixels);
        p.o_refine = ws.take(p.palettes * quant::REFINE_BYTES);
        p.clear_bytes = p.o_refine + p.palettes * quant::REFINE_BYTES - p.o_grids;
    }
    p.total = ws.at;
    return p;
}

bool overlaps(const void* a, size_t a_bytes, const void* b, size_t b_bytes) {
    return (uintptr_t)a < (uintptr_t)b + b_bytes && (uintptr_t)b < (uintptr_t)a + a_bytes;
}

}  // namespace

int quantize_palette_bytes(int n, int h, int w, int mode, size_t* workspace_bytes) {
    if (const char* bad = check_quantize_shape(n, h, w, mode)) { set_error("quantize_palette_u8: %s (n %d, %d x %d, mode %d)", bad, n, h, w, mode); return ADAIN_EINVAL; }
    if (workspace_bytes) *workspace_bytes = make_quant_plan(n, h, w, mode).total;
    return 0;
}

int launch_quantize_palette_u8(const uint8_t* src, int n, int h, int w, int K, int mode, uint8_t* palettes, int32_t* used, void* workspace, size_t workspace_bytes,
                               hipStream_t s) {
    const char* who = "quantize_palette_u8";
    if (!src) { set_error("%s: src is a null pointer", who); return ADAIN_EINVAL; }
    if (!palettes) { set_error("%s: palettes is a null pointer", who); return ADAIN_EINVAL; }
    if (!used) { set_error("%s: used is a null pointer", who); return ADAIN_EINVAL; }
    const char* bad = check_quantize_shape(n, h, w, mode);
    if (!bad && (K < 1 || K > 256)) bad = "K outside 1..256";
    if (bad) { set_error("%s: %s (n %d, %d x %d, K %d, mode %d)", who, bad, n, h, w, K, mode); return ADAIN_EINVAL; }
    const QuantPlan p = make_quant_plan(n, h, w, mode);
    if (int rc = check_workspace(who, workspace, workspace_bytes, p.total, 8)) return rc;
    if ((uintptr_t)used % 4) { set_error("%s: used must be 4-byte aligned", who); return ADAIN_EINVAL; }
    const size_t src_bytes = (size_t)n * h * w * 3, pal_bytes = p.palettes * quant::MAX_COLOURS * 3, used_bytes = p.palettes * sizeof(int32_t);
    if (overlaps(palettes, pal_bytes, src, src_bytes)) { set_error("%s: palettes overlaps src", who); return ADAIN_EINVAL; }
    if (overlaps(used, used_bytes, src, src_bytes)) { set_error("%s: used overlaps src", who); return ADAIN_EINVAL; }
    if (overlaps(workspace, p.total, src, src_bytes)) { set_error("%s: the workspace overlaps src", who); return ADAIN_EINVAL; }
    char* grids = (char*)workspace + p.o_grids;
    if (hipMemsetAsync(grids, 0, p.clear_bytes, s) != hipSuccess) { set_error("%s: hipMemsetAsync failed", who); return ADAIN_ELAUNCH; }
    quantize_hist_kernel<<<dim3(p.hist_groups, (unsigned)p.palettes), HIST_THREADS, 0, s>>>(src, p.pixels, grids);
    quantize_sat_kernel<<<dim3(5, (unsigned)p.palettes), 1024, 0, s>>>(grids);
    quantize_cut_kernel<<<(unsigned)p.palettes, CUT_THREADS, 0, s>>>(grids, K, palettes, used);
    if (p.rounds) launch_quantize_refine(src, p.palettes, p.pixels, p.assign_groups, K, p.rounds, palettes, used, (char*)workspace + p.o_refine, s);
    return check_launch(who);
}

}  // namespace adain
