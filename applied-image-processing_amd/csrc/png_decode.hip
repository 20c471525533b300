// PNG input files on the device (gfx950): pixel for pixel what Pillow's Image.open gives.  Replaces the host's Image.open of a .png path
// (train.py:86-115's guide loop, test.py's content image, video/utils.py's frames).  The host walks the chunks (png_file.py) and hands
// over the IDAT payloads joined; the rules of what follows are RFC 1950 / 1951 and the PNG specification, restated in
// tests/png_decode_ref.py.  The cores live in png_inflate.h, which also compiles for the host (tools/png_decode_check.cpp).
//
// Stages (3 launches and one more per 64 files, whatever the files hold; nothing allocates or waits):
//   table   : the host's stream offsets into the workspace
//   inflate : a wave per file.  Lane 0 reads a block header and builds its tables, or decodes up to 64 tokens, from 1 KiB of the stream
//             staged in LDS; the wave then writes the stored bytes, the literals and, one after the other, the matches - into a 64 KiB ring
//             in LDS, which is the window that matches read, and into the filtered stream h (w c + 1) in the workspace - and keeps the
//             Adler-32 of what it wrote, which is compared with the stream's trailer
//   unfilter: a wave per file walks bands of 64 rows as a diagonal wavefront and writes the pixels in c_out channels (pack is fused)
// A damaged file ends with its status in the record (ADAIN_PNGD_*); the bounds argument is at the top of png_inflate.h.
#include "common.h"
#include "png_inflate.h"

namespace adain {
namespace {

constexpr int OFFSET_BATCH = 64;

struct PngdMeta {
    int32_t status, blocks;
};
struct OffsetBatch {
    uint64_t at[OFFSET_BATCH];
};

struct PngdPlan {
    size_t S, o_offsets, o_meta, o_filt, total;
};

// The one layout of a call
PngdPlan make_pngd_plan(int n, int h, int w, int c) {
    PngdPlan p{};
    p.S = ((size_t)w * c + 1) * h;
    Carve ws;
    p.o_offsets = ws.take(((size_t)n + 1) * sizeof(uint64_t));
    p.o_meta = ws.take((size_t)n * sizeof(PngdMeta));
    p.o_filt = ws.take((size_t)n * p.S);
    p.total = ws.at;
    return p;
}

const char* check_pngd_shape(int n, int h, int w, int c_file, size_t max_stream_bytes) {
    if (n < 1 || n > 65535) return "n outside 1..65535";
    if (c_file != 1 && c_file != 3 && c_file != 4) return "channels of the file other than 1 (grey), 3 (RGB) and 4 (RGBA)";
    if (h < 1 || w < 1) return "height or width below 1";
    if (((uint64_t)w * c_file + 1) * (uint64_t)h >= (1ull << 31)) return "a filtered stream h (w c + 1) of 2^31 bytes or more";
    if (max_stream_bytes >= ((size_t)1 << 31)) return "a stream of 2^31 bytes or more";
    return nullptr;
}

__global__ void pngd_table_kernel(OffsetBatch b, int first, int count, uint64_t* __restrict__ offsets) {
    if ((int)threadIdx.x < count) offsets[first + threadIdx.x] = b.at[threadIdx.x];
}

// grid n, one wave each
__global__ __launch_bounds__(64) void pngd_inflate_kernel(const uint8_t* __restrict__ streams, const uint64_t* __restrict__ offsets, size_t S, uint8_t* __restrict__ filt,
                                                          PngdMeta* __restrict__ meta) {
    __shared__ pngd::State st;
    __shared__ pngd::Tables tb;
    __shared__ uint8_t ring[pngd::RING];
    __shared__ uint8_t stage[pngd::STAGE];
    const int lane = threadIdx.x;
    const size_t f = blockIdx.x;
    const uint8_t* in = streams + offsets[f];
    const size_t in_len = (size_t)(offsets[f + 1] - offsets[f]);
    uint8_t* out = filt + f * S;
    if (lane == 0) pngd::start(st, in_len, S);
    __syncthreads();
    pngd::AdlerPart acc{0, 0};
    const uint64_t steps = pngd::max_steps(in_len);
    bool more = st.status == 0;
    for (uint64_t i = 0; more && i < steps; ++i) {
        const size_t base = st.next;
        for (int k = lane; k < pngd::STAGE; k += 64) stage[k] = base + k < in_len ? in[base + k] : 0;
        __syncthreads();
        if (lane == 0) pngd::step(st, tb, stage, true);
        __syncthreads();
        if (st.status == 0) {
            if (st.stored_len) pngd::write_stored(st, lane, 64, in, ring, out, acc);
            pngd::write_literals(st, lane, 64, ring, out, acc);
            __syncthreads();
            const int count = st.count;
            for (int k = 0; k < count; ++k) {
                if (!pngd::is_match(st, k)) continue;
                pngd::write_match(st, k, lane, 64, ring, out, acc);
                __syncthreads();
            }
            pngd::settle(acc);
        }
        more = st.status == 0 && st.mode != pngd::MODE_DONE;
        __syncthreads();                        // before lane 0 steps on: everyone has read the State
    }
    uint64_t a = acc.a % pngd::ADLER_MOD, b = acc.b % pngd::ADLER_MOD;
    for (int d = 32; d > 0; d >>= 1) a += __shfl_down(a, d), b += __shfl_down(b, d);
    if (lane == 0) {
        int status = st.status;
        if (!status && st.mode != pngd::MODE_DONE) status = ADAIN_PNGD_TRUNCATED;           // the step bound, which no stream reaches
        if (!status && pngd::adler_of(a, b, S) != st.adler) status = ADAIN_PNGD_ADLER;
        meta[f].status = status, meta[f].blocks = st.blocks;
    }
}

// grid n, one wave each
__global__ __launch_bounds__(64) void pngd_unfilter_kernel(uint8_t* __restrict__ filt, size_t S, const PngdMeta* __restrict__ meta, int h, int w, int c, int c_out,
                                                           uint8_t* __restrict__ out, int32_t* __restrict__ record) {
    const size_t f = blockIdx.x;
    const int lane = threadIdx.x;
    int status = meta[f].status;
    if (!status) {
        bool bad = false;
        for (int r0 = 0; r0 < h; r0 += pngd::BAND) {
            bad |= pngd::unfilter_band<1>(filt + f * S, h, w, c, c_out, r0, out + f * (size_t)h * w * c_out, lane);
            __syncthreads();                    // the band's last row, written back in place, is the next band's `up`
        }
        if (__any(bad)) status = ADAIN_PNGD_FILTER;
    }
    if (lane == 0) record[2 * f] = status, record[2 * f + 1] = meta[f].blocks;
}

}  // namespace

int png_decode_bytes(int n, int h, int w, int c_file, size_t max_stream_bytes, size_t* workspace_bytes) {
    if (const char* bad = check_pngd_shape(n, h, w, c_file, max_stream_bytes)) {
        set_error("png_decode_u8: %s (n %d, %d x %d x %d, streams of up to %zu bytes)", bad, n, h, w, c_file, max_stream_bytes);
        return ADAIN_EINVAL;
    }
    if (workspace_bytes) *workspace_bytes = make_pngd_plan(n, h, w, c_file).total;
    return 0;
}

int launch_png_decode_u8(const uint8_t* streams, size_t streams_bytes, const uint64_t* offsets, int n, int h, int w, int c_file, int c_out, uint8_t* out,
                         int32_t* record, void* workspace, size_t workspace_bytes, hipStream_t s) {
    const char* who = "png_decode_u8";
    if (!streams || !offsets || !out || !record) { set_error("%s: null pointer", who); return ADAIN_EINVAL; }
    const char* bad = check_pngd_shape(n, h, w, c_file, 0);
    if (!bad && c_out != c_file && c_out != 3) bad = "c_out that is neither the file's channels nor 3";
    if (bad) { set_error("%s: %s (n %d, %d x %d x %d -> %d)", who, bad, n, h, w, c_file, c_out); return ADAIN_EINVAL; }
    for (int i = 0; i < n; ++i)
        if (offsets[i] > offsets[i + 1] || offsets[i + 1] > streams_bytes || offsets[i + 1] - offsets[i] >= (1ull << 31)) {
            set_error("%s: stream %d (%llu..%llu) leaves the %zu bytes of streams, runs backwards or has 2^31 bytes or more", who, i, (unsigned long long)offsets[i],
                      (unsigned long long)offsets[i + 1], streams_bytes);
            return ADAIN_EINVAL;
        }
    if ((uintptr_t)record % 4) { set_error("%s: the record must be 4-byte aligned", who); return ADAIN_EINVAL; }
    const PngdPlan p = make_pngd_plan(n, h, w, c_file);
    if (int rc = check_workspace(who, workspace, workspace_bytes, p.total, 8)) return rc;
    char* ws = (char*)workspace;
    uint64_t* dev_offsets = (uint64_t*)(ws + p.o_offsets);
    PngdMeta* meta = (PngdMeta*)(ws + p.o_meta);
    uint8_t* filt = (uint8_t*)(ws + p.o_filt);
    for (int first = 0; first <= n; first += OFFSET_BATCH) {
        OffsetBatch b{};
        const int count = n + 1 - first < OFFSET_BATCH ? n + 1 - first : OFFSET_BATCH;
        for (int i = 0; i < count; ++i) b.at[i] = offsets[first + i];
        pngd_table_kernel<<<1, OFFSET_BATCH, 0, s>>>(b, first, count, dev_offsets);
    }
    pngd_inflate_kernel<<<n, 64, 0, s>>>(streams, dev_offsets, p.S, filt, meta);
    pngd_unfilter_kernel<<<n, 64, 0, s>>>(filt, p.S, meta, h, w, c_file, c_out, out, record);
    return check_launch(who);
}

}  // namespace adain
