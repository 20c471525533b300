// Animated GIF clips on the device (gfx950): pixel for pixel what Pillow 12.2 gives for
//     [np.asarray(f.convert("RGB")) for f in ImageSequence.Iterator(Image.open(io.BytesIO(data)))]
// under its default LOADING_STRATEGY (RGB_AFTER_FIRST).  The counterpart of gif.hip, and of the reference's video_to_frames
// (video/utils.py:24-42) for the one clip container this package reads without cv2.  The host walks the file (gif_file.parse) and hands
// over the colour tables and every frame's data sub-blocks joined; include/adain_gif_decode.h has the table of frames and says why these
// calls have a header and a library of their own.  The cores live in gif_unlzw.h, which also compiles for the host
// (tools/gif_decode_check.cpp).
//
// THE RULES (PIL/GifImagePlugin.py: _seek, load_prepare, load_end; restated in tests/gif_decode_ref.py):
//   1. Frame 0 is a palette image.  Outside its rectangle the screen holds the frame's transparent index, or index 0 without one; a
//      pixel shows the colour of its index in the frame's table - its own, else the global one - and the transparent index shows its
//      table colour like any other.  A table is padded to 256 entries with zeros: an index at or above its size is black, not damage.
//   2. A later frame is pasted into the running RGB canvas inside its rectangle; pixels of its transparent index are skipped.
//   3. Before a frame is drawn the disposal of the frame before it is carried out inside THAT frame's rectangle.  The method in force
//      is the last non-zero one: a frame with method 0, or without a graphic control extension, inherits it.  0 and 1 leave the canvas.
//   4. Disposal 2 refills the rectangle, "transparency first, else background": with the colour of the frame's transparent index in
//      the frame's own table, or without one of the screen's background index (0 in a file without a global table).  For frame 0 the
//      index is looked up as a pixel is (rule 1: black at or above the table's size); for a later frame an index at or above the
//      table's size is taken as index 0.
//   5. Disposal 3 restores what the rectangle held before the frame was drawn, after rule 3.  Frame 0 has nothing to restore: with a
//      transparent index its rectangle is refilled with that index's colour, without one nothing happens.
//   6. The rows of an interlaced frame are stored in four passes: rows 0, 8, ...; 4, 12, ...; 2, 6, ...; 1, 3, ....
//   7. Alpha is dropped at the end: the canvas's alpha never reaches a pixel, so none is kept.
//   LZW (Pillow's GifDecode.c): codes of (minimum code size + 1) bits, least significant bit first; the width grows when the entry
//   2^width - 1 is made, up to 12; CLEAR resets width and table, several in a row too; the first code behind a CLEAR - and the first of
//   the stream, which needs no CLEAR - must be a root (ADAIN_GIFD_BAD_FIRST) and makes no entry; a code may be the entry being made
//   (KwKwK) and no higher (ADAIN_GIFD_BAD_CODE); once 4096 entries are made nothing is added and codes stay 12 bits; everything behind
//   the rectangle's last pixel is ignored, damage included; data that ends sooner is ADAIN_GIFD_TRUNCATED, the end code sooner
//   ADAIN_GIFD_EOI (Pillow reads on behind the data there; the caller lets it).
//
// Stages (2 launches, whatever the clip holds; nothing allocates or waits; no wave waits for another):
//   unlzw  : a wave per frame, frames side by side.  The simple form shipped: lane 0 parses up to 64 codes from 128 staged bytes into
//            (position, source, length) tokens against a table of (start, length) strings in LDS, 24 KiB a wave; the wave then writes the
//            literals and the copies from before the batch together, and the copies that read the batch's own output (KwKwK among them)
//            one after the other.  A copy reads bytes other lanes of the wave stored: every such read is behind a __syncthreads(), which
//            orders the workgroup's global stores before its loads.  The frame's indices land in its plane of the workspace in stored
//            row order.
//   compose: a thread per screen pixel walks the frames in order with the canvas, the pending fill and the method in force in
//            registers (gifd::walk_frame) and writes out[i][y][x] at every step; interlace is a row mapping on the read.
#include "common.h"
#include "gif_unlzw.h"

#include <stdarg.h>
#include <stdio.h>

namespace adain {

// This library's own text (adain_gif_decode_last_error): common.h's helpers report through set_error
static thread_local char g_gifd_err[512] = "";
void set_error(const char* fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_gifd_err, sizeof(g_gifd_err), fmt, ap);
    va_end(ap);
}

namespace {

const char* check_gifd_shape(int n, int H, int W) {
    if (n < 1 || n > 65535) return "n outside 1..65535";
    if (H < 1 || H > 65535 || W < 1 || W > 65535) return "a screen side outside 1..65535";
    return nullptr;
}

// The one layout of a call: n planes of `slot` indices
size_t gifd_slot(int n, int H, int W, size_t workspace_bytes) {
    size_t slot = workspace_bytes / (size_t)n;
    const size_t screen = (size_t)H * W, cap = ((size_t)1 << 31) - 1;
    if (slot > screen) slot = screen;
    return slot > cap ? cap : slot;
}

// grid n, one wave each
__global__ __launch_bounds__(64) void gifd_unlzw_kernel(const uint8_t* __restrict__ blob, size_t blob_bytes, const uint64_t* __restrict__ frames, int H, int W,
                                                        size_t slot, uint8_t* planes, int32_t* __restrict__ record) {
    __shared__ gifd::State st;
    __shared__ gifd::Table tb;
    __shared__ gifd::Tokens tk;
    __shared__ uint8_t stage[gifd::STAGE];
    const int lane = threadIdx.x;
    const size_t f = blockIdx.x;
    const uint64_t* words = frames + f * ADAIN_GIFD_ROW_WORDS;
    const gifd::Row r = gifd::read_row(words);
    if (!gifd::row_ok(r, words, (uint32_t)H, (uint32_t)W, slot, blob_bytes)) {           // the same for every lane
        if (lane == 0) record[2 * f] = ADAIN_GIFD_ROW, record[2 * f + 1] = 0;
        return;
    }
    const uint8_t* in = blob + r.data_at;
    const uint64_t in_len = r.data_len;
    uint8_t* out = planes + f * slot;
    if (lane == 0) gifd::start(st, in_len, r.w * r.h, r.code_size);
    __syncthreads();
    const uint64_t steps = gifd::max_batches(in_len);
    bool more = true;
    for (uint64_t i = 0; more && i < steps; ++i) {
        const uint64_t base = st.bitpos >> 3;
        for (int k = lane; k < gifd::STAGE; k += 64) stage[k] = base + k < in_len ? in[base + k] : 0;
        __syncthreads();
        if (lane == 0) gifd::parse(st, tb, tk, stage);
        __syncthreads();
        gifd::write_independent(st, tk, lane, 64, out);
        const int ndep = st.ndep;
        for (int j = 0; j < ndep; ++j) {
            __syncthreads();                    // what token j reads - the batch so far, other lanes' stores - is visible
            gifd::write_dependent(tk, j, lane, 64, out);
        }
        more = st.status == 0 && !st.done;
        __syncthreads();                        // before lane 0 parses on: everyone has read the State and the tokens, and the stores are visible
    }
    if (lane == 0) {
        int status = st.status;
        if (!status && !st.done) status = ADAIN_GIFD_TRUNCATED;            // the step bound, which no stream reaches
        record[2 * f] = status, record[2 * f + 1] = st.codes;
    }
}

__global__ __launch_bounds__(256) void gifd_compose_kernel(const uint8_t* __restrict__ blob, size_t blob_bytes, const uint64_t* __restrict__ frames, int n, int H, int W,
                                                           size_t slot, const uint8_t* __restrict__ planes, const int32_t* __restrict__ record,
                                                           uint8_t* __restrict__ out) {
    const size_t pixels = (size_t)H * W;
    const size_t p = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (p >= pixels) return;
    const uint32_t y = (uint32_t)(p / (size_t)W), x = (uint32_t)(p % (size_t)W);
    gifd::Walk walk;
    for (int k = 0; k < n; ++k) {
        const uint64_t* words = frames + (size_t)k * ADAIN_GIFD_ROW_WORDS;
        gifd::Rgb c = walk.canvas;
        if (record[2 * (size_t)k] == ADAIN_GIFD_OK) {                          // a refused row is never followed, a plane that is not full never read
            const gifd::Row r = gifd::read_row(words);
            c = gifd::walk_frame(walk, k, r, blob, planes + (size_t)k * slot, y, x);
        }
        uint8_t* o = out + ((size_t)k * pixels + p) * 3;
        o[0] = c.r, o[1] = c.g, o[2] = c.b;
    }
}

}  // namespace
}  // namespace adain

using namespace adain;

extern "C" {

const char* adain_gif_decode_last_error(void) { return g_gifd_err; }

int adain_gif_decode_u8_bytes(int n, int H, int W, size_t max_frame_pixels, size_t* workspace_bytes) {
    const char* bad = check_gifd_shape(n, H, W);
    if (!bad && (max_frame_pixels < 1 || max_frame_pixels > (size_t)H * W)) bad = "max_frame_pixels outside 1..H W";
    if (!bad && max_frame_pixels >= ((size_t)1 << 31)) bad = "a frame of 2^31 pixels or more";
    if (bad) {
        set_error("gif_decode_u8: %s (n %d, screen %d x %d, frames of up to %zu pixels)", bad, n, H, W, max_frame_pixels);
        return ADAIN_EINVAL;
    }
    if (workspace_bytes) *workspace_bytes = (size_t)n * max_frame_pixels;
    return ADAIN_OK;
}

int adain_gif_decode_u8(const uint8_t* blob, size_t blob_bytes, const uint64_t* frames, int n, int H, int W, uint8_t* out, int32_t* record, void* workspace,
                        size_t workspace_bytes, adain_stream_t stream) {
    const char* who = "gif_decode_u8";
    hipStream_t s = (hipStream_t)stream;
    if (!blob || !frames || !out || !record) { set_error("%s: null pointer", who); return ADAIN_EINVAL; }
    if (const char* bad = check_gifd_shape(n, H, W)) { set_error("%s: %s (n %d, screen %d x %d)", who, bad, n, H, W); return ADAIN_EINVAL; }
    if ((uintptr_t)frames % 8 || (uintptr_t)record % 4) { set_error("%s: the table must be 8-byte and the record 4-byte aligned", who); return ADAIN_EINVAL; }
    if (int rc = check_workspace(who, workspace, workspace_bytes, (size_t)n, 1)) return rc;          // a pixel a frame at the least
    const size_t slot = gifd_slot(n, H, W, workspace_bytes);
    uint8_t* planes = (uint8_t*)workspace;
    gifd_unlzw_kernel<<<n, 64, 0, s>>>(blob, blob_bytes, frames, H, W, slot, planes, record);
    const size_t pixels = (size_t)H * W;
    gifd_compose_kernel<<<(unsigned)((pixels + 255) / 256), 256, 0, s>>>(blob, blob_bytes, frames, n, H, W, slot, planes, record, out);
    return check_launch(who);
}

}  // extern "C"
