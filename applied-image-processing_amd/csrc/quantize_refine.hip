// k-means refinement of the palette csrc/quantize.hip chooses (gfx950): T rounds behind its median cut, asked for by
// ADAIN_QUANTIZE_REFINE(T) in the call's mode.  Integers only; restated in tests/quantize_refine_ref.py.  Rules 1-6 (top of quantize.hip)
// give the start, a palette P[0..255] and used = u.  Then, for each round:
//
//   7.  Assign.  Every pixel x of the palette's frames goes to the entry j = argmin over i < u of |x - P_i|^2, the squared Euclidean
//       distance in ints; the lowest i wins a tie (csrc/palette.hip's "nearest" rule).
//   8.  Moments.  Per entry i, over its pixels: the count n_i, the sums S_i[c], and the far key F_i = max((d << 24) | (0xFFFFFF -
//       (r << 16 | g << 8 | b))) with d the pixel's distance to P_i, at most 195 075.  The key is a function of the colour, never of the
//       position: the farthest colour wins, among equally far colours the one with the smallest r, g, b value.
//   9.  Centres.  n_i > 0: P'_i[c] = (2 S_i[c] + n_i) / (2 n_i), rounded down (rule 6's rounding).  n_i == 0: P'_i = P_i.
//   10. Fill.  The free slots are the indices i < K with n_i == 0 in ascending order: every i >= u, and any live entry that got no
//       pixel.  The donors are the entries with n_i > 0 and F_i >> 24 > 0, ordered by that distance descending, then by index ascending.
//       The m-th free slot takes the m-th donor's far colour as long as both lists last; u' = max(u, 1 + the highest slot filled).  A
//       donor gives at most one colour a round, so a palette can at most double per round.  A free slot without a donor keeps what it held.
//   11. P, u <- P', u'.  After the last round entries u..255 are zero, as in rule 6.
//
// The result is a function of the multiset of the pixels, K, T and the mode alone.  A round that changes nothing is a fixed point.
//
// Stages (2 launches a round, whatever n; nothing allocates or waits; the accumulators are zero on entry - the call's one memset - and
// every round leaves them zero).  The working palette lives in the call's `palettes` and `used`: entries behind `used` are zero after
// the cut and stay so, since the free slots fill in ascending order.
//   assign : the frames' bytes once, read as hist reads them.  The palette sits in LDS and is walked one entry at a time, every lane
//            reading the same word (a broadcast), 16 pixels a thread in registers.  A thread merges runs of consecutive pixels of one
//            entry, a wave whose lanes all hold one entry sums them by lane shuffles (a flat frame: one addition a wave), the rest goes
//            to the workgroup's accumulators in LDS and from there, at the end, to the palette's in the workspace: integer atomicAdd
//            and atomicMax on 64-bit words, so the sums do not depend on the order.  No float atomics, no spin-wait, no flags.
//            No accumulator can overflow: they are 64 bits wide in LDS and in the workspace, a palette has fewer than 2^32 pixels, so
//            n < 2^32, S <= 255 n < 2^40 and F < 2^42; a thread's run is at most 16 pixels and a wave's 1024, whose sums (at most
//            255 x 1024) fit the 32 bits they are shuffled in.
//   update : a workgroup per palette, a thread per entry.  Rule 9, then rule 10: a donor's rank is the number of donors that give
//            before it (no equal keys: distance, then index), a free slot's the number of free slots below it.  Clears the accumulators.
#include "common.h"
#include "quantize_refine.h"

namespace adain {
namespace {

using quant::Acc;
typedef unsigned long long ull;

// ---- assign -------------------------------------------------------------------------------------------------------------------------------
constexpr int ASSIGN_THREADS = 256;
constexpr int GROUP = 16;                                  // pixels a thread takes at once: 48 bytes, three aligned 16-byte loads
constexpr int TILE = ASSIGN_THREADS * GROUP;
constexpr int MAX_ASSIGN_GROUPS = 2048;                    // workgroups of a launch, over all palettes, about

struct AssignShared {
    uint32_t colour[quant::MAX_COLOURS];
    ull n[quant::MAX_COLOURS], s[3][quant::MAX_COLOURS], f[quant::MAX_COLOURS];
};

// a run of `cnt` pixels of entry j
struct Run {
    uint32_t j, cnt, s[3];
    ull f;
};

__device__ __forceinline__ void add_run(AssignShared& sh, const Run& r) {
    atomicAdd(&sh.n[r.j], (ull)r.cnt);
    atomicAdd(&sh.s[0][r.j], (ull)r.s[0]);
    atomicAdd(&sh.s[1][r.j], (ull)r.s[1]);
    atomicAdd(&sh.s[2][r.j], (ull)r.s[2]);
    atomicMax(&sh.f[r.j], r.f);
}

// pixel (r, g, b), whose nearest entry's key is `key` (quant::nearest_key)
__device__ __forceinline__ void take_pixel(AssignShared& sh, Run& run, uint32_t r, uint32_t g, uint32_t b, uint32_t key) {
    const uint32_t j = key & 255u;
    if (run.cnt && j != run.j) {
        add_run(sh, run);
        run.cnt = 0;
    }
    if (!run.cnt) run.j = j, run.s[0] = run.s[1] = run.s[2] = 0, run.f = 0;
    ++run.cnt;
    run.s[0] += r, run.s[1] += g, run.s[2] += b;
    const ull f = quant::far_key(key >> 8, quant::rgb_of(r, g, b));
    run.f = f > run.f ? f : run.f;
}

// The run every thread is left with (cnt 0: none; at most GROUP pixels).  Every lane of the wave calls it.
__device__ __forceinline__ void add_last_run(AssignShared& sh, Run run) {
    const ull have = __ballot(run.cnt > 0);
    if (!have) return;
    const uint32_t first = (uint32_t)__shfl((int)run.j, __builtin_ctzll(have));
    if (__all(run.cnt == 0 || run.j == first)) {          // a flat stretch: one addition for the wave
        if (run.cnt == 0) run.s[0] = run.s[1] = run.s[2] = 0, run.f = 0;
        for (int d = 32; d > 0; d >>= 1) {
            run.cnt += (uint32_t)__shfl_xor((int)run.cnt, d);
            run.s[0] += (uint32_t)__shfl_xor((int)run.s[0], d);          // 64 x 16 x 255 is below 2^32
            run.s[1] += (uint32_t)__shfl_xor((int)run.s[1], d);
            run.s[2] += (uint32_t)__shfl_xor((int)run.s[2], d);
            const ull other = (ull)(uint32_t)__shfl_xor((int)(uint32_t)(run.f >> 32), d) << 32 | (ull)(uint32_t)__shfl_xor((int)(uint32_t)run.f, d);
            run.f = other > run.f ? other : run.f;
        }
        run.j = first;
        if ((threadIdx.x & 63) == 0) add_run(sh, run);
    } else if (run.cnt) {
        add_run(sh, run);
    }
}

// grid (workgroups, P).  Palette p's pixels: `pixels` of them from src + p * pixels * 3, at any byte address; its entries palettes[p]
// [0..used[p]).  Adds into palette p's accumulators.
__global__ __launch_bounds__(ASSIGN_THREADS) void quantize_assign_kernel(const uint8_t* __restrict__ src, size_t pixels, const uint8_t* __restrict__ palettes,
                                                                         const int32_t* __restrict__ used, void* accumulators) {
    __shared__ AssignShared sh;
    const int t = threadIdx.x;
    const uint8_t* base = src + (size_t)blockIdx.y * pixels * 3;
    const uint8_t* pal = palettes + (size_t)blockIdx.y * quant::MAX_COLOURS * 3;
    const int u = min(max(used[blockIdx.y], 1), quant::MAX_COLOURS);          // 1..256 by rules 3 and 10; the bound keeps the walk inside sh.colour
    sh.colour[t] = quant::rgb_of(pal[3 * t], pal[3 * t + 1], pal[3 * t + 2]);
    sh.n[t] = sh.s[0][t] = sh.s[1][t] = sh.s[2][t] = sh.f[t] = 0;
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
        if (p < pixels) {
            const uint32_t r = base[3 * p], g = base[3 * p + 1], b = base[3 * p + 2];
            uint32_t best = 0xffffffffu;
            for (int i = 0; i < u; ++i) best = min(best, quant::nearest_key(quant::distance(r, g, b, sh.colour[i]), (uint32_t)i));
            take_pixel(sh, run, r, g, b, best);
        }
        add_last_run(sh, run);
        run.cnt = 0;
    }
    const size_t tiles = (groups + ASSIGN_THREADS - 1) / ASSIGN_THREADS;
    for (size_t tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
        const size_t group = tile * ASSIGN_THREADS + t;
        if (group < groups) {
            const uint4* p = (const uint4*)(base + 3 * (head + group * GROUP));
            const uint4 a = p[0], b = p[1], c = p[2];
            const uint32_t word[12] = {a.x, a.y, a.z, a.w, b.x, b.y, b.z, b.w, c.x, c.y, c.z, c.w};
            uint32_t v[GROUP][3], best[GROUP];
#pragma unroll
            for (int i = 0; i < GROUP; ++i) {
                best[i] = 0xffffffffu;
#pragma unroll
                for (int ch = 0; ch < 3; ++ch) {
                    const int e = 3 * i + ch;
                    v[i][ch] = (word[e >> 2] >> (8 * (e & 3))) & 255u;
                }
            }
            for (int i = 0; i < u; ++i) {
                const uint32_t entry = sh.colour[i];          // one word for the wave
#pragma unroll
                for (int k = 0; k < GROUP; ++k) best[k] = min(best[k], quant::nearest_key(quant::distance(v[k][0], v[k][1], v[k][2], entry), (uint32_t)i));
            }
#pragma unroll
            for (int k = 0; k < GROUP; ++k) take_pixel(sh, run, v[k][0], v[k][1], v[k][2], best[k]);
        }
        add_last_run(sh, run);
        run.cnt = 0;
    }
    __syncthreads();
    if (sh.n[t]) {          // a thread per entry
        const Acc acc = quant::acc_at(accumulators, blockIdx.y);
        atomicAdd((ull*)&acc.n[t], sh.n[t]);
        for (int ch = 0; ch < 3; ++ch) atomicAdd((ull*)&acc.s[ch][t], sh.s[ch][t]);
        atomicMax((ull*)&acc.f[t], sh.f[t]);
    }
}

// ---- update -------------------------------------------------------------------------------------------------------------------------------
constexpr int UPDATE_THREADS = 256;
static_assert(UPDATE_THREADS == quant::MAX_COLOURS && ASSIGN_THREADS == quant::MAX_COLOURS, "a thread per entry");

struct UpdateShared {
    ull f[quant::MAX_COLOURS];                 // a donor's far key, 0 for an entry that is none (a donor's distance is above 0)
    uint32_t gift[quant::MAX_COLOURS];         // the far colours in the order they are given
    uint32_t is_free[quant::MAX_COLOURS];
    int donors, next_used;
};

// grid P.  palettes: [P][256][3]; used: [P]: rules 9 to 11 on palette blockIdx.x, whose accumulators are cleared
__global__ __launch_bounds__(UPDATE_THREADS) void quantize_update_kernel(void* accumulators, int K, uint8_t* palettes, int32_t* used) {
    __shared__ UpdateShared sh;
    const int t = threadIdx.x;
    const Acc acc = quant::acc_at(accumulators, blockIdx.x);
    const uint64_t n = acc.n[t], s0 = acc.s[0][t], s1 = acc.s[1][t], s2 = acc.s[2][t], f = acc.f[t];
    acc.n[t] = acc.s[0][t] = acc.s[1][t] = acc.s[2][t] = acc.f[t] = 0;
    uint8_t* pal = palettes + (size_t)blockIdx.x * quant::MAX_COLOURS * 3;
    const uint32_t old = quant::rgb_of(pal[3 * t], pal[3 * t + 1], pal[3 * t + 2]);
    const bool donor = quant::is_donor(n, f), free_slot = quant::is_free(n, t, K);
    sh.f[t] = donor ? f : 0;
    sh.is_free[t] = free_slot;
    if (t == 0) sh.donors = 0, sh.next_used = used[blockIdx.x];
    __syncthreads();
    if (donor) {
        int rank = 0;
        for (int o = 0; o < quant::MAX_COLOURS; ++o) rank += sh.f[o] && quant::gives_before(sh.f[o], o, f, t);          // not itself: t < t is false
        sh.gift[rank] = quant::far_colour(f);
        atomicAdd(&sh.donors, 1);
    }
    int below = 0;
    if (free_slot)
        for (int o = 0; o < t; ++o) below += (int)sh.is_free[o];
    __syncthreads();
    uint32_t colour = quant::centre(n, s0, s1, s2, old);
    if (free_slot && below < sh.donors) {
        colour = sh.gift[below];
        atomicMax(&sh.next_used, t + 1);
    }
    pal[3 * t] = (uint8_t)(colour >> 16), pal[3 * t + 1] = (uint8_t)(colour >> 8), pal[3 * t + 2] = (uint8_t)colour;
    __syncthreads();
    if (t == 0) used[blockIdx.x] = sh.next_used;
}

}  // namespace

unsigned quantize_refine_groups(size_t palettes, size_t pixels) {
    const size_t tiles = (pixels + TILE - 1) / TILE, share = max((size_t)1, MAX_ASSIGN_GROUPS / palettes);
    return (unsigned)max((size_t)1, min(tiles, share));
}

// `rounds` rounds on the palettes the cut kernel left in `palettes` and `used`; the accumulators (palettes x quant::REFINE_BYTES) are zero
void launch_quantize_refine(const uint8_t* src, size_t palettes_n, size_t pixels, unsigned groups, int K, int rounds, uint8_t* palettes, int32_t* used,
                            void* accumulators, hipStream_t s) {
    for (int round = 0; round < rounds; ++round) {
        quantize_assign_kernel<<<dim3(groups, (unsigned)palettes_n), ASSIGN_THREADS, 0, s>>>(src, pixels, palettes, used, accumulators);
        quantize_update_kernel<<<(unsigned)palettes_n, UPDATE_THREADS, 0, s>>>(accumulators, K, palettes, used);
    }
}

}  // namespace adain
