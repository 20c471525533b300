"""The size limits of DESIGN.md's table at their edge: for every row the FIRST refused value returns ADAIN_EINVAL with a message that
names the call, and ``n = 65536`` is refused where ``n`` is capped.  No device is needed: a refusal comes before anything is
launched or dereferenced, so the pointers are made-up addresses (distinct, far apart, 256-byte aligned).  On a machine without a
GPU a missed refusal ends as a launch error (another return code), never on a device.  The module is collected on a machine with a
GPU as well, where a refusal missed in the future would launch a kernel on these made-up addresses: that is why the rows hold first
refused values only, why every row was first run without a device, and why a new row must be.

The largest admitted values themselves are launched nowhere: those frames are 2 GiB each and a wrong index there is out of
bounds.  What stands for them is the audit behind the table (every index a live or an idle lane forms, every grid size and every
grid-stride sum fits its type at the largest admitted value) and these refusals one step further.

The table is held to the header: every launch of include/adain_hip.h (tests/abi_launches.py) is the call of a row here, or a key of
``NO_ROW`` with the reason it has none."""
import ctypes

import pytest

import applied_image_processing_amd.runtime as rt

EINVAL = -1
A, B, C, D, E = (k << 40 for k in range(1, 6))          # made-up device addresses
BIG = 1 << 62                                           # a workspace or stride "large enough"
M31 = 0x7fffffff                                        # 2^31 - 1
THIRD = M31 // 3 + 1                                    # 715 827 883: the first h w with 3 h w > 2^31 - 1
M30 = 0x40000000                                        # 2^30: the first pixel count CORAL and the colour transfer refuse


S24 = 1 << 24                                           # the first side the PIL resizes refuse
OFF64 = ctypes.POINTER(ctypes.c_uint64)
LEN32 = ctypes.POINTER(ctypes.c_uint32)
# host tables of the decoders: one JPEG segment of 2^28 bytes at offset 0; one PNG stream of 2^31 bytes
SEG_OFF, SEG_LEN = ctypes.cast((ctypes.c_uint64 * 2)(0, 1 << 28), OFF64), ctypes.cast((ctypes.c_uint32 * 1)(1 << 28), LEN32)
PNG_OFF = ctypes.cast((ctypes.c_uint64 * 2)(0, 1 << 31), OFF64)
SCANS = ctypes.cast((ctypes.c_int32 * 8)(3, 0, 1, 2, 0, 0, 0, 0), ctypes.POINTER(ctypes.c_int32))          # one scan: the DC terms of all three components
TABLES = (C, D, 5, E, E + (1 << 30), 5)                 # resize_pil_u8's tap tables: x bounds, x taps, ksize, y bounds, y taps, ksize (BICUBIC at scale 1: 5 taps)
WS = A + (1 << 39)
# host tables of adain_encode_multi: one batch of one image of 9 x 2^20 pixels, its image and feature pointers made up like the rest
PTRS = ctypes.POINTER(ctypes.c_void_p)
INTS = ctypes.POINTER(ctypes.c_int)
ONE_IMAGE, ONE_FEAT = ctypes.cast((ctypes.c_void_p * 1)(A), PTRS), ctypes.cast((ctypes.c_void_p * 1)(B), PTRS)
ONE_N, NINE_ROWS, WIDE = (ctypes.cast((ctypes.c_int * 1)(v), INTS) for v in (1, 9, 1 << 20))


def tv_params():
    from applied_image_processing_amd import tvl1

    return tvl1.check_params()


# (row of DESIGN.md's table, call, arguments in front of the stream, what the message holds)
ROWS = [
    ("quantize_u8: h w c", "adain_quantize_u8", (A, B, 1, 1, 1, M31), "quantize_u8: image too large"),
    ("quantize_u8: h w c, three channels", "adain_quantize_u8", (A, B, 1, 3, 1, THIRD), "quantize_u8: image too large"),
    ("quantize_u8: n", "adain_quantize_u8", (A, B, 65536, 3, 4, 4), "batch > 65535"),
    ("u8_to_f32: h w c", "adain_u8_to_f32", (A, B, 1, 1, M31, 1), "u8_to_f32: image too large"),
    ("u8_to_f32: n", "adain_u8_to_f32", (A, B, 65536, 3, 4, 4), "batch > 65535"),
    ("warp_blend_u8: h w c", "adain_warp_blend_u8", (A, B, C, D, 1, M31, 1, 0.5, 0.5), "warp_blend_u8: frame too large"),
    ("warp_blend_u8: h w c, three channels", "adain_warp_blend_u8", (A, B, C, D, THIRD, 1, 3, 0.5, 0.5), "warp_blend_u8: frame too large"),
    ("resize_bilinear: source plane", "adain_resize_bilinear", (A, B, 1, 1, M31, 4, 4), "resize_bilinear: a plane must stay below 2^31 pixels"),
    ("resize_bilinear: result plane", "adain_resize_bilinear", (A, B, 1, 4, 4, 1, M31), "resize_bilinear: a plane must stay below 2^31 pixels"),
    ("resize_bilinear: rows", "adain_resize_bilinear", (A, B, 1, 4, 4, 262141, 1), "more than 262140 rows or 65535 planes"),
    ("resize_bilinear: planes", "adain_resize_bilinear", (A, B, 65536, 4, 4, 4, 4), "more than 262140 rows or 65535 planes"),
    ("resize_nearest: source plane", "adain_resize_nearest", (A, B, 1, M31, 1, 4, 4), "resize_nearest: a plane must stay below 2^31 pixels"),
    ("resize_nearest: result plane", "adain_resize_nearest", (A, B, 1, 4, 4, 1, M31), "resize_nearest: a plane must stay below 2^31 pixels"),
    ("resize_nearest: planes", "adain_resize_nearest", (A, B, 65536, 4, 4, 4, 4), "more than 262140 rows or 65535 planes"),
    ("mask_composite: planes", "adain_mask_composite", (A, B, C, 1, 1, D, 21846, 3, 16), "mask_composite: more than 65535 planes"),
    ("resize_area_u8: frame", "adain_resize_area_u8", (A, B, 1, 1, M31, 1, 1, 4), "resize_area_u8: frame (2^31 - 1 bytes)"),
    ("resize_area_u8: n", "adain_resize_area_u8", (A, B, 65536, 8, 8, 3, 4, 4), "batch (65535)"),
    ("resize_area_u8: output rows", "adain_resize_area_u8", (A, B, 1, 8, 8, 1, 262141, 8), "output height (262140)"),
    ("resize_area_u8: output rows that wrap an int", "adain_resize_area_u8", (A, B, 1, 8, 8, 1, M31, 8), "output height (262140)"),
    ("strength_map: result", "adain_strength_map", (A, 4, 4, 1, M31, 0.15, 20.0, B, C, BIG), "strength_map: map too large"),
    ("strength_map: source", "adain_strength_map", (A, M31, 1, 4, 4, 0.15, 20.0, B, C, BIG), "strength_map: map too large"),
    ("nchw_to_nhwc: tiles", "adain_nchw_to_nhwc", (A, B, 1, 32 * 4096, 32 * 4096), "nchw_to_nhwc: grid too large"),
    ("nchw_to_nhwc: n", "adain_nchw_to_nhwc", (A, B, 65536, 3, 16), "nchw_to_nhwc: grid too large"),
    ("nhwc_to_nchw: tiles", "adain_nhwc_to_nchw", (A, B, 1, 1, M31), "nhwc_to_nchw: grid too large"),
    ("nhwc_to_nchw: n", "adain_nhwc_to_nchw", (A, B, 65536, 3, 16), "nhwc_to_nchw: grid too large"),
    ("flow_gray_u8: n", "adain_flow_gray_u8", (A, 65536, 8, 8, B, 8, 8), "flow_gray_u8: bad frame count 65536"),
    ("flow_gray_u8: frame", "adain_flow_gray_u8", (A, 1, 8, 8, B, 1, 429496730), "flow_gray_u8: bad frame size"),
    ("flow_gray_u8: rows", "adain_flow_gray_u8", (A, 1, 65536, 1, B, 8, 8), "flow_gray_u8: bad frame size"),
    ("palette_map_u8: n", "adain_palette_map_u8", (A, 65536, 4, 4, B, 16, 1, None, 0, C, None), "palette_map_u8: n outside 1..65535"),
    ("palette_map_u8: frame", "adain_palette_map_u8", (A, 1, 1, THIRD, B, 16, 1, None, 0, C, None), "a frame beyond 2^31 - 1 bytes"),
    ("tone_u8: n", "adain_tone_u8", (A, 65536, 4, 4, None, 1, B), "tone_u8: n outside 1..65535"),
    ("tone_u8: frame", "adain_tone_u8", (A, 1, THIRD, 1, None, 1, B), "a frame beyond 2^31 - 1 bytes"),
    ("palette_dither_u8: n", "adain_palette_dither_u8", (A, 65536, 4, 4, B, 16, None, 0, C, None, D, BIG), "palette_dither_u8: n outside 1..65535"),
    ("palette_dither_u8: frame", "adain_palette_dither_u8", (A, 1, 1, THIRD, B, 16, None, 0, C, None, D, BIG), "a frame beyond 2^31 - 1 bytes"),
    ("quantize_palette_u8: n", "adain_quantize_palette_u8", (A, 65536, 4, 4, 16, 1, B, C, D, BIG), "quantize_palette_u8: n outside"),
    ("quantize_palette_u8: pixels of a frame", "adain_quantize_palette_u8", (A, 1, 65536, 65536, 16, 1, B, C, D, BIG), "2^32 or more pixels for one palette"),
    ("quantize_palette_u8: pixels of a clip", "adain_quantize_palette_u8", (A, 16, 16384, 16384, 16, 0, B, C, D, BIG), "2^32 or more pixels for one palette"),
    ("image_metrics_u8: n", "adain_image_metrics_u8", (A, B, 65536, 4, 4, 3, C, None, D, BIG), "image_metrics_u8: n outside 1..65535"),
    ("image_metrics_u8: frame", "adain_image_metrics_u8", (A, B, 1, 1, THIRD, 3, C, None, D, BIG), "a frame beyond 2^31 - 1 samples"),
    ("image_metrics_f32: n", "adain_image_metrics_f32", (A, B, 65536, 3, 4, 4, C, None, D, BIG), "image_metrics_f32: n outside 1..65535"),
    ("image_metrics_f32: frame", "adain_image_metrics_f32", (A, B, 1, 1, 32768, 65536, C, None, D, BIG), "a frame beyond 2^31 - 1 samples"),
    ("coral: n", "adain_coral", (A, 1, 1, 4, 4, B, 1, 65536, 4, 4, C, D, BIG), "coral: unsupported shape"),
    ("coral: style pixels", "adain_coral", (A, 1, 1, 1, M30, B, 1, 1, 4, 4, C, D, BIG), "at most 65535 pairs, 2^30 - 1 pixels"),
    ("coral: content pixels", "adain_coral", (A, 1, 1, 4, 4, B, 1, 1, M30, 1, C, D, BIG), "at most 65535 pairs, 2^30 - 1 pixels"),
    ("colour_transfer_u8: pixels", "adain_colour_transfer_u8", (A, B, C, 32768, 32768, D), "colour_transfer_u8: unsupported size"),
    ("mean_std: elements", "adain_mean_std", (A, 0, 1, 1, M31, 1e-5, B, C, D, BIG), "more than 2^31 elements per call"),
    ("blend_alpha: elements", "adain_blend_alpha", (A, 0, 4, 1, 536870912, B, C, D, E, 1, 0.7, 0.3, A + (1 << 36)), "more than 2^31 elements per call"),
    ("jpeg_encode_u8: side", "adain_jpeg_encode_u8", (A, 1, 65536, 8, 3, 75, B, BIG, C, D, BIG), "height or width outside 1..65535"),
    ("jpeg_encode_u8: n", "adain_jpeg_encode_u8", (A, 65536, 8, 8, 3, 75, B, BIG, C, D, BIG), "batch of 65536 frames too large"),
    ("png_encode_u8: side", "adain_png_encode_u8", (A, 1, 8, 65536, 3, -1, B, BIG, C, D, BIG), "height or width outside 1..65535"),
    ("png_encode_u8: n", "adain_png_encode_u8", (A, 65536, 8, 8, 3, -1, B, BIG, C, D, BIG), "n outside 1..65535"),
    ("gif_encode_u8: side", "adain_gif_encode_u8", (A, 1, 65536, 8, 16, 5, B, BIG, C, D, BIG), "height or width outside 1..65535"),
    ("gif_encode_u8: n", "adain_gif_encode_u8", (A, 65536, 8, 8, 16, 5, B, BIG, C, D, BIG), "n outside 1..65535"),
    ("jpeg_roundtrip_u8: side", "adain_jpeg_roundtrip_u8", (A, 1, 8, 65536, 3, 75, B, C, BIG), "height or width outside 1..65535"),
    ("jpeg_roundtrip_u8: n", "adain_jpeg_roundtrip_u8", (A, 65536, 8, 8, 3, 75, B, C, BIG), "batch of 65536 frames too large"),
    ("mean_std: images (NHWC)", "adain_mean_std", (A, 1, 65536, 4, 4, 1e-5, B, C, D, BIG), "more than 65535 images (NHWC) or 16777215 planes (NCHW)"),
    ("mean_std: planes (NCHW)", "adain_mean_std", (A, 0, 16777216, 1, 4, 1e-5, B, C, D, BIG), "more than 65535 images (NHWC) or 16777215 planes (NCHW)"),
    ("blend_pmap: elements", "adain_blend_pmap", (A, 0, 4, 1, 536870912, B, C, D, E, 1, A + (1 << 36), 1, A + (1 << 37)), "more than 2^31 elements per call"),
    ("blend_mix: elements", "adain_blend_mix", (A, 0, 4, 1, 536870912, B, C, D, E, 2, A + (1 << 36), 1, 1, 0.5, 0.5, None, 1, A + (1 << 37)),
     "adain_blend_mix: more than 2^31 elements per call"),
    ("localized_combine_u8: pixels", "adain_localized_combine_u8", (A, B, C, D, 32768, 32768, E), "localized_combine_u8: unsupported size"),
    ("flow_gray_u8: result rows", "adain_flow_gray_u8", (A, 1, 8, 8, B, 65536, 1), "flow_gray_u8: bad frame size 1 x 65536"),
    ("flow_gray_u8: result frame", "adain_flow_gray_u8", (A, 1, 8, 8, B, 1, 429496730), "flow_gray_u8: bad frame size 429496730 x 1"),
    ("resize_pil_bilinear_u8: n", "adain_resize_pil_bilinear_u8", (A, 3, 65536, 8, 8, B, 8, 8, 0, 0, 8, 8, C, BIG), "resize_pil_bilinear_u8: grid too large"),
    ("resize_pil_bilinear_u8: result rows", "adain_resize_pil_bilinear_u8", (A, 3, 1, 262141, 8, B, 262141, 8, 0, 0, 262141, 8, C, BIG),
     "resize_pil_bilinear_u8: grid too large"),
    ("resize_pil_bilinear_u8: shrink factor", "adain_resize_pil_bilinear_u8", (A, 3, 1, 257, 8, B, 1, 8, 0, 0, 1, 8, C, BIG), "shrink factor above 256"),
    ("resize_pil_bilinear_u8: side", "adain_resize_pil_bilinear_u8", (A, 3, 1, 8, S24, B, 8, S24, 0, 0, 8, 8, C, BIG), "every side must be in [1, 2^24)"),
    ("resize_pil_u8: n", "adain_resize_pil_u8", (A, 3, 65536, 8, 8, B, 8, 8, 3) + TABLES + (0, 0, 8, 8, WS, BIG), "resize_pil_u8: grid too large"),
    ("resize_pil_u8: result rows", "adain_resize_pil_u8", (A, 3, 1, 262141, 8, B, 262141, 8, 3) + TABLES + (0, 0, 262141, 8, WS, BIG), "resize_pil_u8: grid too large"),
    ("resize_pil_u8: shrink factor", "adain_resize_pil_u8", (A, 3, 1, 257, 8, B, 1, 8, 3) + TABLES + (0, 0, 1, 8, WS, BIG), "shrink factor above 256"),
    ("resize_pil_u8: side", "adain_resize_pil_u8", (A, 3, 1, 8, S24, B, 8, S24, 3) + TABLES + (0, 0, 8, 8, WS, BIG), "every side must be in [1, 2^24)"),
    ("jpeg_decode_u8: n", "adain_jpeg_decode_u8", (A, BIG, B, 65536, 8, 8, 3, 2, SEG_OFF, SEG_LEN, C, D, E, BIG, 0), "jpeg_decode_u8: n outside 1..65535"),
    ("jpeg_decode_u8: side", "adain_jpeg_decode_u8", (A, BIG, B, 1, 65536, 8, 3, 2, SEG_OFF, SEG_LEN, C, D, E, BIG, 0), "height or width outside 1..65535"),
    ("jpeg_decode_u8: segment", "adain_jpeg_decode_u8", (A, BIG, B, 1, 8, 8, 3, 2, SEG_OFF, SEG_LEN, C, D, E, BIG, 0), "a segment of 2^28 bytes or more"),
    ("jpeg_decode_restart_u8: n", "adain_jpeg_decode_restart_u8", (A, BIG, B, 65536, 8, 8, 3, 2, 1, SEG_OFF, SEG_LEN, C, D, E, BIG, 0), "n outside 1..65535"),
    ("jpeg_decode_restart_u8: segment", "adain_jpeg_decode_restart_u8", (A, BIG, B, 1, 8, 8, 3, 2, 1, SEG_OFF, SEG_LEN, C, D, E, BIG, 0),
     "a segment of 2^28 bytes or more"),
    ("jpeg_decode_progressive_u8: n", "adain_jpeg_decode_progressive_u8", (A, BIG, B, 65536, 8, 8, 3, 2, 1, SCANS, SEG_OFF, SEG_LEN, C, D, E, BIG, 0),
     "jpeg_decode_progressive_u8: n outside 1..65535"),
    ("jpeg_decode_progressive_u8: side", "adain_jpeg_decode_progressive_u8", (A, BIG, B, 1, 8, 65536, 3, 2, 1, SCANS, SEG_OFF, SEG_LEN, C, D, E, BIG, 0),
     "height or width outside 1..65535"),
    ("jpeg_decode_progressive_u8: segment", "adain_jpeg_decode_progressive_u8", (A, BIG, B, 1, 8, 8, 3, 2, 1, SCANS, SEG_OFF, SEG_LEN, C, D, E, BIG, 0),
     "a segment of 2^28 bytes or more"),
    ("png_decode_u8: n", "adain_png_decode_u8", (A, BIG, PNG_OFF, 65536, 8, 8, 3, 3, B, C, D, BIG), "png_decode_u8: n outside 1..65535"),
    ("png_decode_u8: stream", "adain_png_decode_u8", (A, BIG, PNG_OFF, 1, 8, 8, 3, 3, B, C, D, BIG), "has 2^31 bytes or more"),
    ("png_decode_u8: filtered frame", "adain_png_decode_u8", (A, BIG, PNG_OFF, 1, 32768, 65535, 1, 1, B, C, D, BIG), "a filtered stream h (w c + 1) of 2^31 bytes or more"),
    # 2^32 - 255 = 401 x 10 710 641: the first uint8 mask stylize_u8 refuses (mask_to_f32 runs a thread per element)
    ("stylize_u8: uint8 mask elements", "adain_stylize_u8_ex", (A, 1, 16, 16, B, C, D, E, 1, 0.5, 0.5, None, None, None, 0.0, 0.0, A + (1 << 37), 0, 1, 1, 401, 10710641,
                                                               A + (1 << 38), WS, BIG), "stylize_u8: a uint8 mask of more than 2^32 - 256 elements"),
    ("jpeg_encode_opt_u8: side", "adain_jpeg_encode_opt_u8", (A, 1, 65536, 8, 3, 75, 0, 1, B, BIG, C, D, BIG), "height or width outside 1..65535"),
    ("jpeg_encode_opt_u8: n", "adain_jpeg_encode_opt_u8", (A, 65536, 8, 8, 3, 75, 0, 1, B, BIG, C, D, BIG), "batch of 65536 frames too large"),
    ("jpeg_encode_progressive_u8: side", "adain_jpeg_encode_progressive_u8", (A, 1, 8, 65536, 3, 75, 2, B, BIG, C, D, BIG), "height or width outside 1..65535"),
    ("jpeg_encode_progressive_u8: n", "adain_jpeg_encode_progressive_u8", (A, 65536, 8, 8, 3, 75, 2, B, BIG, C, D, BIG), "batch of 65536 frames too large"),
    # the 3DGS loss calls: a, b, n, c, h, w, weights, grad_a, grad_b, workspace / image, guide, n, h, w, gh, gw, ...
    ("image_metrics_grad_f32: n", "adain_image_metrics_grad_f32", (A, B, 65536, 3, 4, 4, C, D, None, WS, BIG), "image_metrics_grad_f32: n outside 1..65535"),
    ("image_metrics_grad_f32: frame", "adain_image_metrics_grad_f32", (A, B, 1, 1, 32768, 65536, C, D, None, WS, BIG), "a frame beyond 2^31 - 1 samples"),
    ("image_metrics_grad_f32: frame, three planes", "adain_image_metrics_grad_f32", (A, B, 1, 3, 1, THIRD, C, D, None, WS, BIG), "a frame beyond 2^31 - 1 samples"),
    ("image_metrics_grad_f32: frame, with grad_b", "adain_image_metrics_grad_f32", (A, B, 1, 3, THIRD, 1, C, D, E, WS, BIG), "a frame beyond 2^31 - 1 samples"),
    ("guide_l1_f32: n", "adain_guide_l1_f32", (A, B, 65536, 4, 4, 4, 4, C, D, WS, BIG), "guide_l1_f32: n outside 1..65535"),
    ("guide_l1_f32: render", "adain_guide_l1_f32", (A, B, 1, 1, THIRD, 4, 4, C, D, WS, BIG), "guide_l1_f32: a frame beyond 2^31 - 1 samples"),
    ("guide_l1_f32: guide", "adain_guide_l1_f32", (A, B, 1, 4, 4, THIRD, 1, C, D, WS, BIG), "guide_l1_f32: a guide beyond 2^31 - 1 samples"),
    ("guide_l1_grad_f32: n", "adain_guide_l1_grad_f32", (A, B, 65536, 4, 4, 4, 4, C, D), "guide_l1_grad_f32: n outside 1..65535"),
    ("guide_l1_grad_f32: render", "adain_guide_l1_grad_f32", (A, B, 1, THIRD, 1, 4, 4, C, D), "guide_l1_grad_f32: a frame beyond 2^31 - 1 samples"),
    ("guide_l1_grad_f32: guide", "adain_guide_l1_grad_f32", (A, B, 1, 4, 4, 1, THIRD, C, D), "guide_l1_grad_f32: a guide beyond 2^31 - 1 samples"),
    # stylize_u8_ex's uint8-mask row for its two siblings (one launcher, stylize_impl)
    ("stylize_u8: uint8 mask elements, one style", "adain_stylize_u8", (A, 1, 16, 16, B, C, D, E, 0.5, 0.5, None, None, None, 0.0, 0.0, A + (1 << 37), 0, 1, 1, 401, 10710641,
                                                                         A + (1 << 38), WS, BIG), "stylize_u8: a uint8 mask of more than 2^32 - 256 elements"),
    ("stylize_u8_mix: uint8 mask elements", "adain_stylize_u8_mix", (A, 1, 16, 16, B, C, D, E, 2, A + (1 << 36), 1, 1, 0.5, 0.5, None, None, None, 0.0, 0.0, A + (1 << 37), 0,
                                                                     1, 1, 401, 10710641, A + (1 << 38), WS, BIG), "stylize_u8: a uint8 mask of more than 2^32 - 256 elements"),
    # the networks' frame limits (Data layout in HBM): eight 64-channel rows and three float planes of an image below 2 GiB in the
    # first layer, a band of eighteen source or sixteen output rows below 2 GiB in a 3 x 3 layer (32 output rows in the polyphase up layer)
    ("encode_relu1_1: eight rows of relu1_1", "adain_encode_relu1_1", (A, 0, B, C, 1, 2, 1 << 20), "conv_first: eight 64-channel rows of width 1048576 reach 2 GiB"),
    # 215 x 832 358 = 178 956 970 pixels, the first count with 12 h w >= 2^31 - 16
    ("encode_relu1_1: three float planes", "adain_encode_relu1_1", (A, 0, B, C, 1, 215, 832358), "reaches 2 GiB as three float planes"),
    ("encode: eight rows of relu1_1", "adain_encode", (A, B, C, WS, BIG, 1, 9, 1 << 20, None), "conv_first: eight 64-channel rows of width 1048576 reach 2 GiB"),
    ("encode_u8: eight rows of relu1_1", "adain_encode_u8", (A, B, C, WS, BIG, 1, 9, 1 << 20, None), "conv_first: eight 64-channel rows of width 1048576 reach 2 GiB"),
    ("encode_multi: eight rows of relu1_1", "adain_encode_multi", (1, ONE_IMAGE, ONE_FEAT, ONE_N, NINE_ROWS, WIDE, C, WS, BIG, None),
     "conv_first: eight 64-channel rows of width 1048576 reach 2 GiB"),
    # the decoder's first layer has 512 input channels: 18 x 2048 x 58 255 bytes is the first band of 2^31 - 16 bytes or more
    ("decode: a band of source rows", "adain_decode", (A, B, C, WS, BIG, 1, 2, 58255, None), "conv3x3_wino4: a band of eighteen 512-channel source rows"),
    ("conv3x3_wino: a band of output rows", "adain_conv3x3_wino", (A, B, C, D, 1, 2, 1 << 20, 2, 1 << 20, 16, 32, 0, 1, 0, 5), "of width 1048576 reaches 2 GiB"),
    ("conv3x3_wino4_split: a band of output rows", "adain_conv3x3_wino4_split", (A, B, C, D, 1, 2, 1 << 20, 2, 1 << 20, 16, 32, 0, 1, 0, None, 0),
     "of width 1048576 reaches 2 GiB"),
    ("conv3x3_up2x_poly: a band of output rows", "adain_conv3x3_up2x_poly", (A, B, C, D, 1, 1, 1 << 18, 16, 32, 1), "a band of 19 source or 32 output rows reaches 2 GiB"),
    # the flow estimators: h; 5 h w (Farneback); pairs, h, w and 4 h w (TV-L1, the limits of tvl1_prepare)
    ("farneback_expand: rows", "adain_farneback_expand", (A, 65536, 1, 0.5, 3, 5, 1.1, B, WS, BIG), "farneback_expand: bad frame size 1 x 65536"),
    ("farneback_expand: frame", "adain_farneback_expand", (A, 1, 429496730, 0.5, 3, 5, 1.1, B, WS, BIG), "farneback_expand: bad frame size 429496730 x 1"),
    ("farneback_flow: rows", "adain_farneback_flow", (A, B, 65536, 1, 0.5, 3, 15, 3, 0, C, WS, BIG), "farneback_flow: bad frame size 1 x 65536"),
    ("farneback_flow: frame", "adain_farneback_flow", (A, B, 1, 429496730, 0.5, 3, 15, 3, 0, C, WS, BIG), "farneback_flow: bad frame size 429496730 x 1"),
]

# A launch of include/adain_hip.h without a row, a test of FILES or test_tvl1_prepare_caps_n_and_the_frame / test_tvl1_flow_caps_the_pairs_and_the_frame:
# where its limit is enforced, or why it has none.  test_every_launch_of_the_header_has_a_row_or_a_reason holds this to the header.
NO_ROW = {
    "adain_encoder_pack": "no size argument: the ten layers of the one encoder, sizes fixed at compile time",
    "adain_decoder_pack": "no size argument: the nine layers of the one decoder, sizes fixed at compile time",
    "adain_conv3x3_wino4_pack": "refuses no size: a grid-stride walk of at most 4096 workgroups over cin cout 24 floats, counted in size_t; the layer that "
                                "reads the weights refuses cin cout 96 >= 2^32 - 1 (adain_conv3x3_wino's launcher)",
    "adain_conv3x3_up2x_poly_pack": "refuses no size: the same walk over cin cout 96 floats; adain_conv3x3_up2x_poly refuses cin cout 384 >= 2^32 - 1",
}


@pytest.fixture(scope="module")
def lib():
    return rt.lib()


@pytest.mark.parametrize("row", ROWS, ids=[r[0] for r in ROWS])
def test_the_first_refused_value_is_einval_with_a_message(lib, row):
    what, call, args, text = row
    rc = getattr(lib, call)(*args, None)
    message = lib.adain_last_error().decode()
    assert rc == EINVAL, (what, rc, message)
    assert text in message and ": " in message, (what, message)


def test_tvl1_prepare_caps_n_and_the_frame(lib):
    P = tv_params()
    for args, text in (((A, 65536, 36, 64, ctypes.addressof(P), B), "tvl1_prepare: bad frame count 65536"),
                       ((A, 1, 65536, 64, ctypes.addressof(P), B), "bad frame size"), ((A, 1, 64, 65536, ctypes.addressof(P), B), "bad frame size"),
                       # 4 h w: 23171^2 is the first square past (2^31 - 2) / 4, with both sides far below 65535
                       ((A, 1, 23171, 23171, ctypes.addressof(P), B), "bad frame size 23171 x 23171")):
        assert lib.adain_tvl1_prepare(*args, None) == EINVAL
        assert text in lib.adain_last_error().decode()


def test_tvl1_flow_caps_the_pairs_and_the_frame(lib):
    """The frame limits are tvl1_prepare's (tv_check, in front of everything else); the pairs are capped like its n."""
    P = tv_params()
    for args, text in (((A, B, 65536, 36, 64, ctypes.addressof(P), C, None, WS, BIG), "tvl1_flow: bad pair count 65536"),
                       ((A, B, 1, 65536, 64, ctypes.addressof(P), C, None, WS, BIG), "tvl1_flow: bad frame size"),
                       ((A, B, 1, 64, 65536, ctypes.addressof(P), C, None, WS, BIG), "tvl1_flow: bad frame size"),
                       ((A, B, 1, 23171, 23171, ctypes.addressof(P), C, None, WS, BIG), "tvl1_flow: bad frame size 23171 x 23171")):
        assert lib.adain_tvl1_flow(*args, None) == EINVAL
        assert text in lib.adain_last_error().decode()


def test_every_launch_of_the_header_has_a_row_or_a_reason():
    """The tables cannot fall behind the header: a declaration of include/adain_hip.h that ends in ``adain_stream_t stream`` is the call
    of a row of ROWS or FILES or of one of the two TV-L1 tests, or a key of NO_ROW with its reason - never both."""
    import abi_launches

    tested = {r[1] for r in ROWS} | {f[0] for f in FILES} | {"adain_tvl1_prepare", "adain_tvl1_flow"}
    abi_launches.audit(tested, NO_ROW, "tests/test_limits_host.py")
    assert len({r[0] for r in ROWS}) == len(ROWS), "two rows have one id"


# (call, its size query, arguments of the query after n, h, w; arguments of the call after src, n, h, w)
FILES = [
    ("adain_jpeg_encode_u8", "adain_jpeg_encode_u8_bytes", (3,), (3, 75, B, BIG, C, D, BIG)),
    ("adain_jpeg_encode_opt_u8", "adain_jpeg_encode_opt_u8_bytes", (3, 0, 1), (3, 75, 0, 1, B, BIG, C, D, BIG)),
    ("adain_jpeg_encode_progressive_u8", "adain_jpeg_encode_progressive_u8_bytes", (3, 2), (3, 75, 2, B, BIG, C, D, BIG)),
    ("adain_png_encode_u8", "adain_png_encode_u8_bytes", (3,), (3, -1, B, BIG, C, D, BIG)),
    ("adain_gif_encode_u8", "adain_gif_encode_u8_bytes", (16,), (16, 5, B, BIG, C, D, BIG)),
]


@pytest.mark.parametrize("call,query,qargs,cargs", FILES, ids=[f[0] for f in FILES])
def test_the_first_worst_case_file_beyond_int32_is_refused(lib, call, query, qargs, cargs):
    """The encoders' third limit, a worst-case file of 2^31 - 1 bytes (lengths are int32): at w = 65535 the first h whose worst case
    is larger is found by bisection over the host-only size query; the query admits h - 1 with a stride of at most 2^31 - 1, and the
    query and the call refuse h with the message."""
    stride, ws = ctypes.c_size_t(), ctypes.c_size_t()
    ok = lambda h: getattr(lib, query)(1, h, 65535, *qargs, ctypes.byref(stride), ctypes.byref(ws)) == 0
    lo, hi = 1, 65535
    assert ok(lo) and not ok(hi)
    while hi - lo > 1:
        mid = (lo + hi) // 2
        lo, hi = (mid, hi) if ok(mid) else (lo, mid)
    assert ok(lo) and stride.value <= M31, (lo, stride.value)
    assert not ok(hi) and "beyond 2^31 - 1 bytes (lengths are int32)" in lib.adain_last_error().decode()
    assert getattr(lib, call)(A, 1, hi, 65535, *cargs, None) == EINVAL
    assert "beyond 2^31 - 1 bytes" in lib.adain_last_error().decode(), (hi, lib.adain_last_error())


def test_the_size_queries_refuse_what_the_calls_refuse(lib):
    size = ctypes.c_size_t()
    two = (ctypes.byref(size), ctypes.byref(ctypes.c_size_t()))
    for call, args in (("adain_png_encode_u8_bytes", (65536, 8, 8, 3) + two), ("adain_gif_encode_u8_bytes", (65536, 8, 8, 16) + two),
                       ("adain_png_encode_u8_bytes", (1, 65536, 8, 3) + two), ("adain_gif_encode_u8_bytes", (1, 8, 65536, 16) + two),
                       ("adain_image_metrics_u8_bytes", (65536, 4, 4, 3, ctypes.byref(size))), ("adain_image_metrics_u8_bytes", (1, 1, THIRD, 3, ctypes.byref(size))),
                       ("adain_quantize_palette_u8_bytes", (65536, 4, 4, 1, ctypes.byref(size))), ("adain_palette_dither_u8_bytes", (65536, 4, 4, ctypes.byref(size))),
                       ("adain_palette_dither_u8_bytes", (1, 1, THIRD, ctypes.byref(size))),
                       ("adain_jpeg_decode_u8_bytes", (1, 8, 8, 3, 2, 1 << 28, 0, ctypes.byref(size))), ("adain_jpeg_decode_u8_bytes", (65536, 8, 8, 3, 2, 64, 0, ctypes.byref(size))),
                       ("adain_jpeg_decode_progressive_u8_bytes", (1, 8, 8, 3, 2, 1, 1 << 28, 0, ctypes.byref(size))),
                       ("adain_png_decode_u8_bytes", (1, 8, 8, 3, 1 << 31, ctypes.byref(size))), ("adain_png_decode_u8_bytes", (65536, 8, 8, 3, 64, ctypes.byref(size))),
                       ("adain_resize_pil_u8_bytes", (1, 257, 8, 1, 8, 3, 3, 0, 0, 1, 8, ctypes.byref(size))),
                       ("adain_resize_pil_u8_bytes", (1, 8, S24, 8, S24, 3, 3, 0, 0, 8, 8, ctypes.byref(size))),
                       ("adain_image_metrics_f32_bytes", (65536, 3, 4, 4, ctypes.byref(size))), ("adain_image_metrics_f32_bytes", (1, 1, 32768, 65536, ctypes.byref(size))),
                       ("adain_image_metrics_grad_f32_bytes", (65536, 3, 4, 4, 0, ctypes.byref(size))),
                       ("adain_image_metrics_grad_f32_bytes", (1, 1, 32768, 65536, 0, ctypes.byref(size))),
                       ("adain_image_metrics_grad_f32_bytes", (1, 3, 1, THIRD, 1, ctypes.byref(size))),
                       ("adain_guide_l1_f32_bytes", (65536, 4, 4, ctypes.byref(size))), ("adain_guide_l1_f32_bytes", (1, 1, THIRD, ctypes.byref(size)))):
        assert getattr(lib, call)(*args) == EINVAL, (call, args)
        assert lib.adain_last_error()
    assert lib.adain_coral_workspace_bytes(65536, 1, 4, 4, 4, 4) == 0 and lib.adain_coral_workspace_bytes(1, 1, 1, M30, 4, 4) == 0
    assert lib.adain_colour_transfer_workspace_bytes(32768, 32768) == 0 and lib.adain_strength_map_workspace_bytes(4, 4) > 0


def test_the_largest_admitted_values_pass_the_size_queries(lib):
    """One step inside the limits the host-only queries answer: the refusals above are the limits', not the harness's."""
    size = ctypes.c_size_t()
    for call, args in (("adain_image_metrics_u8_bytes", (65535, 1, THIRD - 1, 3)), ("adain_image_metrics_f32_bytes", (1, 1, 1, M31)),
                       ("adain_quantize_palette_u8_bytes", (65535, 65535, 65537, 1)), ("adain_quantize_palette_u8_bytes", (65535, 256, 256, 0)),
                       ("adain_palette_dither_u8_bytes", (65535, 1, THIRD - 1)), ("adain_jpeg_decode_u8_bytes", (65535, 8, 8, 3, 2, (1 << 28) - 1, 0)),
                       ("adain_png_decode_u8_bytes", (65535, 8, 8, 3, (1 << 31) - 1)), ("adain_resize_pil_u8_bytes", (65535, 256, 8, 1, 8, 3, 3, 0, 0, 1, 8))):
        assert getattr(lib, call)(*args, ctypes.byref(size)) == 0, (call, args, lib.adain_last_error())
    assert lib.adain_coral_workspace_bytes(65535, 1, 1, M30 - 1, 32767, 32768) > 0
    # the 3DGS loss calls, and here the answer too: the tile counts of a plane of 2^31 - 1 samples are formed from sizes within 64 of
    # INT_MAX (ceil(Wp / 64), ceil(H / 16)), the planes and partials of 65535 such frames in size_t
    up256 = lambda v: -(-v // 256) * 256
    for call, args, want in (("adain_image_metrics_f32_bytes", (1, 1, 1, M31), up256(24 << 25)), ("adain_image_metrics_f32_bytes", (1, 1, M31, 1), up256(24 << 27)),
                             ("adain_image_metrics_u8_bytes", (1, 1, THIRD - 1, 3), up256(24 * -(-3 * (THIRD - 1) // 64))),
                             ("adain_image_metrics_grad_f32_bytes", (1, 1, 1, M31, 0), 3 * up256(4 * M31)),
                             ("adain_image_metrics_grad_f32_bytes", (1, 1, 1, M31, 1), 5 * up256(4 * M31)),
                             ("adain_image_metrics_grad_f32_bytes", (1, 1, M31, 1, 1), 5 * up256(4 * M31)),
                             ("adain_image_metrics_grad_f32_bytes", (65535, 3, 1, THIRD - 1, 0), 3 * up256(65535 * 3 * (THIRD - 1) * 4)),
                             ("adain_guide_l1_f32_bytes", (65535, 1, THIRD - 1), up256(65535 * 8 * -(-(-(-(THIRD - 1) // 4)) // 256))),
                             ("adain_guide_l1_f32_bytes", (1, THIRD - 1, 1), up256(8 * -(-(THIRD - 1) // 256)))):
        assert getattr(lib, call)(*args, ctypes.byref(size)) == 0, (call, args, lib.adain_last_error())
        assert size.value == want, (call, args, size.value, want)
