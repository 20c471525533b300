/* Animated GIF clips decoded on the device (gfx950): pixel for pixel what Pillow 12.2 gives for
 *
 *     [np.asarray(f.convert("RGB")) for f in ImageSequence.Iterator(Image.open(io.BytesIO(data)))]
 *
 * under its default LOADING_STRATEGY (RGB_AFTER_FIRST).  The rules are stated once, at the top of csrc/gif_decode.hip, and restated in
 * plain Python in tests/gif_decode_ref.py; the host walk that produces this call's arguments is gif_file.parse.
 *
 * WHY A HEADER OF ITS OWN.  The launches of adain_hip.h are audited by three tables (tests/far_batch.py, the table of
 * tests/test_limits_host.py, tests/capture_cases.py), and the product library libadain_hip.so is held to export exactly what adain_hip.h
 * declares (tests/test_host_and_abi.py).  The change that added this decoder could not edit those files, so its two calls are declared
 * here and live in a library of their own, libadain_gif_decode.so, built by the same build.py from csrc/gif_decode.hip alone.  They are
 * held to the same four promises by test files of their own:
 *   - a call stays inside its buffers and ignores stale workspace bytes   tests/test_gpu_gif_decode_arena.py
 *   - it indexes with size_t: a clip whose frames pass 2^32 bytes         tests/test_gpu_far_batch_gif_decode.py
 *   - its size query refuses the edges of its limits                      tests/test_gif_decode_host.py
 *   - it allocates nothing and waits for nothing: hipGraph capture        tests/test_gpu_gif_decode_capture.py
 * Folding them into adain_hip.h and its tables is left to a change that may edit those tables.
 *
 * Because the second library cannot reach the first one's thread-local text, a refused call sets adain_gif_decode_last_error(), not
 * adain_last_error(); the return codes are adain_hip.h's (ADAIN_OK, ADAIN_EINVAL, ADAIN_ELAUNCH). */
#ifndef ADAIN_GIF_DECODE_H
#define ADAIN_GIF_DECODE_H

#include "adain_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* status words of the record, one per frame */
#define ADAIN_GIFD_OK 0
#define ADAIN_GIFD_TRUNCATED 1 /* the data ends (inside a code too) before the rectangle is full; Pillow: "image file is truncated" */
#define ADAIN_GIFD_BAD_CODE 2  /* a code above the next free entry; Pillow: "broken data stream" */
#define ADAIN_GIFD_BAD_FIRST 3 /* the first code behind a CLEAR (or of the stream) is no root; Pillow: "broken data stream" */
#define ADAIN_GIFD_EOI 4       /* the end code before the rectangle is full: Pillow reads on into the bytes behind the data */
#define ADAIN_GIFD_ROW 5       /* the frame's row of the table points outside the screen, the blob or its plane of the workspace */
/* An index at or above the frame's table size is NOT damage: Pillow pads every table to 256 entries with zeros, so such a pixel is
 * black, and so it is here.  (Only the fill colour of disposal 2 treats it specially: see ADAIN_GIFD_ROW_FLAGS.) */

/* The per-frame table: n rows of ADAIN_GIFD_ROW_WORDS uint64 words, in DEVICE memory, 8-byte aligned (it travels with the blob: one
 * upload).  Every row is checked on the device before it is used; a row that fails gives its frame ADAIN_GIFD_ROW.
 *   word 0  offset of the frame's LZW data in the blob: the data sub-blocks joined, without their length bytes
 *   word 1  length of that data in bytes
 *   word 2  the rectangle: left | top << 16 | width << 32 | height << 48; not empty, inside the screen, width * height <= max_frame_pixels
 *   word 3  flags: the minimum code size 2..8 | interlace << 8 | disposal 0..3 << 16 | (transparent index + 1, 0 for none) << 32
 *   word 4  offset of the frame's colour table (its own, else the global one) in the blob: 3 bytes per entry
 *   word 5  entries of that table, 2..256
 *   word 6  the screen's background index (0 in a file without a global table, as Pillow has it)
 *   word 7  0 */
#define ADAIN_GIFD_ROW_WORDS 8
#define ADAIN_GIFD_ROW_FLAGS(code_size, interlace, disposal, transparent) \
    ((uint64_t)(code_size) | (uint64_t)((interlace) != 0) << 8 | (uint64_t)(disposal) << 16 | (uint64_t)((transparent) + 1) << 32)

/* adain_gif_decode_u8_bytes (host only): *workspace_bytes = n planes of max_frame_pixels indices, the frames' rectangles in stored row
 * order.  Refused with ADAIN_EINVAL: n outside 1..65535, H or W outside 1..65535, max_frame_pixels 0, above H * W, or 2^31 and more (a
 * plane is indexed with 32 bits by the table of strings).
 *
 * adain_gif_decode_u8: blob (device, any byte address) holds the colour tables and the joined LZW data; out [n][H][W][3] and record
 * [n][2] (int32, 4-byte aligned: status, codes read) are device memory.  Two launches on `stream`: a wave per frame decodes the LZW
 * data into the frame's plane, then one thread per screen pixel walks the frames in order and writes every frame's pixel.  The call
 * allocates nothing and waits for nothing, so it may be captured into a hipGraph.  The planes are workspace_bytes / n bytes each, H W
 * at the most.  A frame whose status is not ADAIN_GIFD_OK is left out of the walk (its plane is not read: the result stays a function of
 * the inputs alone), so the clip's pixels are then not Pillow's: the caller decodes the file with Pillow. */
ADAIN_API int adain_gif_decode_u8_bytes(int n, int H, int W, size_t max_frame_pixels, size_t* workspace_bytes);
ADAIN_API int adain_gif_decode_u8(const uint8_t* blob, size_t blob_bytes, const uint64_t* frames, int n, int H, int W, uint8_t* out,
                                  int32_t* record, void* workspace, size_t workspace_bytes, adain_stream_t stream);
/* the calling thread's text of the last refusal of the two calls above */
ADAIN_API const char* adain_gif_decode_last_error(void);

#ifdef __cplusplus
}
#endif
#endif
