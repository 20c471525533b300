"""ctypes binding of ``libadain_hip.so`` (the C ABI declared in include/adain_hip.h).

PyTorch is used only for device memory, streams and (elsewhere) ``torch.distributed``: every
compute call below hands raw device pointers (``tensor.data_ptr()``) and the current HIP stream to a
hand-written gfx950 kernel.  There is NO fallback: if the shared library is missing or the tensors
are not on a GPU, these functions raise.
"""
import collections
import contextlib
import ctypes
import os
import threading

import torch

from . import jpeg_file, png_file

_PKG = os.path.dirname(os.path.abspath(__file__))
# The product library.  Nothing in the environment can swap it: another build is loaded only by an explicit ``use_library(path)``
# call (bench.py --lib: same-box A/B runs).
LIB_PATH = os.path.join(_PKG, "libadain_hip.so")

SRC_DIRECT, SRC_UP2X, SRC_POOL2 = 0, 1, 2
SCHEDULE_BATCH, SCHEDULE_LATENCY = 0, 1      # ADAIN_SCHEDULE_*: see adain_set_schedule in include/adain_hip.h
ABI_VERSION = 4          # ADAIN_ABI_VERSION of include/adain_hip.h this binding was written against

_c_int, _c_float, _c_size_t, _c_void_p = ctypes.c_int, ctypes.c_float, ctypes.c_size_t, ctypes.c_void_p
_PP = ctypes.POINTER(ctypes.c_void_p)

# name -> (restype, argtypes); mirrors include/adain_hip.h one to one
SIGNATURES = {
    "adain_abi_version": (_c_int, []),
    "adain_last_error": (ctypes.c_char_p, []),
    "adain_set_schedule": (_c_int, [_c_int]),
    "adain_get_schedule": (_c_int, []),
    "adain_encoder_packed_floats": (_c_size_t, []),
    "adain_decoder_packed_floats": (_c_size_t, []),
    "adain_encoder_pack": (_c_int, [_PP, _PP, _c_void_p, _c_void_p]),
    "adain_decoder_pack": (_c_int, [_PP, _PP, _c_void_p, _c_void_p]),
    "adain_encoded_size": (None, [_c_int, _c_int, ctypes.POINTER(_c_int), ctypes.POINTER(_c_int)]),
    "adain_encode_workspace_bytes": (_c_size_t, [_c_int, _c_int, _c_int]),
    "adain_encode": (_c_int, [_c_void_p, _c_void_p, _c_void_p, _c_void_p, _c_size_t, _c_int, _c_int, _c_int, _PP, _c_void_p]),
    "adain_encode_u8": (_c_int, [_c_void_p, _c_void_p, _c_void_p, _c_void_p, _c_size_t, _c_int, _c_int, _c_int, _PP, _c_void_p]),
    "adain_encode_relu1_1": (_c_int, [_c_void_p, _c_int, _c_void_p, _c_void_p, _c_int, _c_int, _c_int, _c_void_p]),
    "adain_encode_multi_workspace_bytes": (_c_size_t, [_c_int, ctypes.POINTER(_c_int), ctypes.POINTER(_c_int), ctypes.POINTER(_c_int)]),
    "adain_encode_multi": (_c_int, [_c_int, _PP, _PP, ctypes.POINTER(_c_int), ctypes.POINTER(_c_int), ctypes.POINTER(_c_int), _c_void_p,
                                    _c_void_p, _c_size_t, _PP, _c_void_p]),
    "adain_decode_workspace_bytes": (_c_size_t, [_c_int, _c_int, _c_int]),
    "adain_decode": (_c_int, [_c_void_p, _c_void_p, _c_void_p, _c_void_p, _c_size_t, _c_int, _c_int, _c_int, _PP, _c_void_p]),
    "adain_mean_std_workspace_bytes": (_c_size_t, [_c_int, _c_int, _c_int, _c_int]),
    "adain_mean_std": (_c_int, [_c_void_p, _c_int, _c_int, _c_int, _c_int, _c_float, _c_void_p, _c_void_p, _c_void_p, _c_size_t, _c_void_p]),
    "adain_blend_alpha": (_c_int, [_c_void_p, _c_int, _c_int, _c_int, _c_int, _c_void_p, _c_void_p, _c_void_p, _c_void_p, _c_int,
                                   _c_float, _c_float, _c_void_p, _c_void_p]),
    "adain_blend_pmap": (_c_int, [_c_void_p, _c_int, _c_int, _c_int, _c_int, _c_void_p, _c_void_p, _c_void_p, _c_void_p, _c_int,
                                  _c_void_p, _c_int, _c_void_p, _c_void_p]),
    "adain_blend_mix": (_c_int, [_c_void_p, _c_int, _c_int, _c_int, _c_int, _c_void_p, _c_void_p, _c_void_p, _c_void_p, _c_int, _c_void_p, _c_int,
                                 _c_int, _c_float, _c_float, _c_void_p, _c_int, _c_void_p, _c_void_p]),
    "adain_strength_map_workspace_bytes": (_c_size_t, [_c_int, _c_int]),
    "adain_strength_map": (_c_int, [_c_void_p, _c_int, _c_int, _c_int, _c_int, _c_float, _c_float, _c_void_p, _c_void_p, _c_size_t, _c_void_p]),
    "adain_resize_bilinear": (_c_int, [_c_void_p, _c_void_p, _c_int, _c_int, _c_int, _c_int, _c_int, _c_void_p]),
    "adain_resize_nearest": (_c_int, [_c_void_p, _c_void_p, _c_int, _c_int, _c_int, _c_int, _c_int, _c_void_p]),
    "adain_mask_composite": (_c_int, [_c_void_p, _c_void_p, _c_void_p, _c_int, _c_int, _c_void_p, _c_int, _c_int, _c_int, _c_void_p]),
    "adain_quantize_u8": (_c_int, [_c_void_p, _c_void_p, _c_int, _c_int, _c_int, _c_int, _c_void_p]),
    "adain_u8_to_f32": (_c_int, [_c_void_p, _c_void_p, _c_int, _c_int, _c_int, _c_int, _c_void_p]),
    "adain_warp_blend_u8": (_c_int, [_c_void_p, _c_void_p, _c_void_p, _c_void_p, _c_int, _c_int, _c_int, _c_float, _c_float, _c_void_p]),
    "adain_resize_area_u8": (_c_int, [_c_void_p, _c_void_p] + [_c_int] * 6 + [_c_void_p]),
    "adain_flow_gray_u8": (_c_int, [_c_void_p, _c_int, _c_int, _c_int, _c_void_p, _c_int, _c_int, _c_void_p]),
    "adain_farneback_levels": (_c_int, [_c_int, _c_int, ctypes.c_double, _c_int, ctypes.POINTER(_c_int), ctypes.POINTER(_c_int),
                                        ctypes.POINTER(_c_int), ctypes.POINTER(ctypes.c_double)]),
    "adain_farneback_pyramid_bytes": (_c_size_t, [_c_int, _c_int, ctypes.c_double, _c_int]),
    "adain_farneback_workspace_bytes": (_c_size_t, [_c_int, _c_int]),
    "adain_farneback_expand": (_c_int, [_c_void_p, _c_int, _c_int, ctypes.c_double, _c_int, _c_int, ctypes.c_double, _c_void_p, _c_void_p,
                                        _c_size_t, _c_void_p]),
    "adain_farneback_flow": (_c_int, [_c_void_p, _c_void_p, _c_int, _c_int, ctypes.c_double, _c_int, _c_int, _c_int, _c_int, _c_void_p,
                                      _c_void_p, _c_size_t, _c_void_p]),
    "adain_tvl1_scales": (_c_int, [_c_int, _c_int, _c_void_p, ctypes.POINTER(_c_int), ctypes.POINTER(_c_int)]),
    "adain_tvl1_frame_bytes": (_c_size_t, [_c_int, _c_int, _c_void_p]),
    "adain_tvl1_prepare": (_c_int, [_c_void_p, _c_int, _c_int, _c_int, _c_void_p, _c_void_p, _c_void_p]),
    "adain_tvl1_workspace_bytes": (_c_size_t, [_c_int, _c_int, _c_int, _c_void_p]),
    "adain_tvl1_flow": (_c_int, [_c_void_p, _c_void_p, _c_int, _c_int, _c_int, _c_void_p, _c_void_p, _c_void_p, _c_void_p, _c_size_t,
                                 _c_void_p]),
    "adain_colour_transfer_workspace_bytes": (_c_size_t, [_c_int, _c_int]),
    "adain_colour_transfer_u8": (_c_int, [_c_void_p, _c_void_p, _c_void_p, _c_int, _c_int, _c_void_p, _c_void_p]),
    "adain_localized_combine_u8": (_c_int, [_c_void_p, _c_void_p, _c_void_p, _c_void_p, _c_int, _c_int, _c_void_p, _c_void_p]),
    "adain_coral_workspace_bytes": (_c_size_t, [_c_int] * 6),
    "adain_coral": (_c_int, [_c_void_p, _c_int, _c_int, _c_int, _c_int, _c_void_p, _c_int, _c_int, _c_int, _c_int, _c_void_p, _c_void_p, _c_size_t,
                             _c_void_p]),
    "adain_resize_pil_bilinear_u8_workspace_bytes": (_c_size_t, [_c_int] * 4),
    "adain_resize_pil_bilinear_u8": (_c_int, [_c_void_p, _c_int, _c_int, _c_int, _c_int, _c_void_p] + [_c_int] * 6 + [_c_void_p, _c_size_t, _c_void_p]),
    "adain_pil_resize_taps_bytes": (_c_int, [_c_int] * 3 + [ctypes.POINTER(_c_int), ctypes.POINTER(_c_size_t)]),
    "adain_pil_resize_taps": (_c_int, [_c_int] * 3 + [_c_void_p, _c_void_p]),
    "adain_resize_pil_u8_bytes": (_c_int, [_c_int] * 11 + [ctypes.POINTER(_c_size_t)]),
    "adain_resize_pil_u8": (_c_int, [_c_void_p, _c_int, _c_int, _c_int, _c_int, _c_void_p, _c_int, _c_int, _c_int, _c_void_p, _c_void_p, _c_int, _c_void_p,
                                     _c_void_p, _c_int] + [_c_int] * 4 + [_c_void_p, _c_size_t, _c_void_p]),
    "adain_stylize_u8_workspace_bytes": (_c_size_t, [_c_int] * 9),
    "adain_stylize_u8_out_size": (None, [_c_int, _c_int, _c_int, ctypes.POINTER(_c_int), ctypes.POINTER(_c_int)]),
    "adain_stylize_u8": (_c_int, [_c_void_p, _c_int, _c_int, _c_int, _c_void_p, _c_void_p, _c_void_p, _c_void_p, _c_float, _c_float, _PP,
                                  ctypes.POINTER(_c_int), ctypes.POINTER(_c_int), _c_float, _c_float, _c_void_p, _c_int, _c_int, _c_int, _c_int,
                                  _c_int, _c_void_p, _c_void_p, _c_size_t, _c_void_p]),
    "adain_stylize_u8_ex_workspace_bytes": (_c_size_t, [_c_int] * 9),
    "adain_stylize_u8_ex": (_c_int, [_c_void_p, _c_int, _c_int, _c_int, _c_void_p, _c_void_p, _c_void_p, _c_void_p, _c_int, _c_float, _c_float, _PP,
                                     ctypes.POINTER(_c_int), ctypes.POINTER(_c_int), _c_float, _c_float, _c_void_p, _c_int, _c_int, _c_int, _c_int,
                                     _c_int, _c_void_p, _c_void_p, _c_size_t, _c_void_p]),
    "adain_stylize_u8_mix_workspace_bytes": (_c_size_t, [_c_int] * 9),
    "adain_stylize_u8_mix": (_c_int, [_c_void_p, _c_int, _c_int, _c_int, _c_void_p, _c_void_p, _c_void_p, _c_void_p, _c_int, _c_void_p, _c_int, _c_int,
                                      _c_float, _c_float, _PP, ctypes.POINTER(_c_int), ctypes.POINTER(_c_int), _c_float, _c_float, _c_void_p, _c_int,
                                      _c_int, _c_int, _c_int, _c_int, _c_void_p, _c_void_p, _c_size_t, _c_void_p]),
    "adain_jpeg_encode_u8_bytes": (_c_int, [_c_int] * 4 + [ctypes.POINTER(_c_size_t), ctypes.POINTER(_c_size_t)]),
    "adain_jpeg_encode_u8": (_c_int, [_c_void_p] + [_c_int] * 5 + [_c_void_p, _c_size_t, _c_void_p, _c_void_p, _c_size_t, _c_void_p]),
    "adain_png_encode_u8_bytes": (_c_int, [_c_int] * 4 + [ctypes.POINTER(_c_size_t), ctypes.POINTER(_c_size_t)]),
    "adain_png_encode_u8": (_c_int, [_c_void_p] + [_c_int] * 5 + [_c_void_p, _c_size_t, _c_void_p, _c_void_p, _c_size_t, _c_void_p]),
    "adain_png_decode_u8_bytes": (_c_int, [_c_int] * 4 + [_c_size_t, ctypes.POINTER(_c_size_t)]),
    "adain_png_decode_u8": (_c_int, [_c_void_p, _c_size_t, ctypes.POINTER(ctypes.c_uint64)] + [_c_int] * 5 + [_c_void_p, _c_void_p, _c_void_p, _c_size_t, _c_void_p]),
    "adain_palette_map_u8": (_c_int, [_c_void_p] + [_c_int] * 3 + [_c_void_p, _c_int, _c_int, _c_void_p, _c_int, _c_void_p, _c_void_p, _c_void_p]),
    "adain_tone_u8": (_c_int, [_c_void_p] + [_c_int] * 3 + [_c_void_p, _c_int, _c_void_p, _c_void_p]),
    "adain_palette_dither_u8_bytes": (_c_int, [_c_int] * 3 + [ctypes.POINTER(_c_size_t)]),
    "adain_palette_dither_u8": (_c_int, [_c_void_p] + [_c_int] * 3 + [_c_void_p, _c_int, _c_void_p, _c_int, _c_void_p, _c_void_p, _c_void_p, _c_size_t, _c_void_p]),
    "adain_gif_encode_u8_bytes": (_c_int, [_c_int] * 4 + [ctypes.POINTER(_c_size_t), ctypes.POINTER(_c_size_t)]),
    "adain_gif_encode_u8": (_c_int, [_c_void_p] + [_c_int] * 5 + [_c_void_p, _c_size_t, _c_void_p, _c_void_p, _c_size_t, _c_void_p]),
    "adain_quantize_palette_u8_bytes": (_c_int, [_c_int] * 4 + [ctypes.POINTER(_c_size_t)]),
    "adain_quantize_palette_u8": (_c_int, [_c_void_p] + [_c_int] * 5 + [_c_void_p, _c_void_p, _c_void_p, _c_size_t, _c_void_p]),
    "adain_image_metrics_u8_bytes": (_c_int, [_c_int] * 4 + [ctypes.POINTER(_c_size_t)]),
    "adain_image_metrics_u8": (_c_int, [_c_void_p, _c_void_p] + [_c_int] * 4 + [_c_void_p, _c_void_p, _c_void_p, _c_size_t, _c_void_p]),
    "adain_image_metrics_f32_bytes": (_c_int, [_c_int] * 4 + [ctypes.POINTER(_c_size_t)]),
    "adain_image_metrics_f32": (_c_int, [_c_void_p, _c_void_p] + [_c_int] * 4 + [_c_void_p, _c_void_p, _c_void_p, _c_size_t, _c_void_p]),
    "adain_ssim_window": (_c_int, [ctypes.POINTER(_c_float)]),
    "adain_image_metrics_grad_f32_bytes": (_c_int, [_c_int] * 5 + [ctypes.POINTER(_c_size_t)]),
    "adain_image_metrics_grad_f32": (_c_int, [_c_void_p, _c_void_p] + [_c_int] * 4 + [_c_void_p, _c_void_p, _c_void_p, _c_void_p, _c_size_t, _c_void_p]),
    "adain_guide_l1_f32_bytes": (_c_int, [_c_int] * 3 + [ctypes.POINTER(_c_size_t)]),
    "adain_guide_l1_f32": (_c_int, [_c_void_p, _c_void_p] + [_c_int] * 5 + [_c_void_p, _c_void_p, _c_void_p, _c_size_t, _c_void_p]),
    "adain_guide_l1_grad_f32": (_c_int, [_c_void_p, _c_void_p] + [_c_int] * 5 + [_c_void_p, _c_void_p, _c_void_p]),
    "adain_jpeg_encode_opt_u8_bytes": (_c_int, [_c_int] * 6 + [ctypes.POINTER(_c_size_t), ctypes.POINTER(_c_size_t)]),
    "adain_jpeg_encode_opt_u8": (_c_int, [_c_void_p] + [_c_int] * 7 + [_c_void_p, _c_size_t, _c_void_p, _c_void_p, _c_size_t, _c_void_p]),
    "adain_jpeg_encode_progressive_u8_bytes": (_c_int, [_c_int] * 5 + [ctypes.POINTER(_c_size_t), ctypes.POINTER(_c_size_t)]),
    "adain_jpeg_encode_progressive_u8": (_c_int, [_c_void_p] + [_c_int] * 6 + [_c_void_p, _c_size_t, _c_void_p, _c_void_p, _c_size_t, _c_void_p]),
    "adain_jpeg_roundtrip_u8_bytes": (_c_int, [_c_int] * 4 + [ctypes.POINTER(_c_size_t)]),
    "adain_jpeg_roundtrip_u8": (_c_int, [_c_void_p] + [_c_int] * 5 + [_c_void_p, _c_void_p, _c_size_t, _c_void_p]),
    "adain_jpeg_decode_u8_bytes": (_c_int, [_c_int] * 5 + [_c_size_t, _c_int, ctypes.POINTER(_c_size_t)]),
    "adain_jpeg_decode_u8": (_c_int, [_c_void_p, _c_size_t, _c_void_p] + [_c_int] * 5 + [ctypes.POINTER(ctypes.c_uint64), ctypes.POINTER(ctypes.c_uint32),
                                      _c_void_p, _c_void_p, _c_void_p, _c_size_t, _c_int, _c_void_p]),
    "adain_jpeg_decode_restart_u8_bytes": (_c_int, [_c_int] * 6 + [_c_size_t, _c_int, ctypes.POINTER(_c_size_t)]),
    "adain_jpeg_decode_restart_u8": (_c_int, [_c_void_p, _c_size_t, _c_void_p] + [_c_int] * 6 + [ctypes.POINTER(ctypes.c_uint64), ctypes.POINTER(ctypes.c_uint32),
                                              _c_void_p, _c_void_p, _c_void_p, _c_size_t, _c_int, _c_void_p]),
    "adain_jpeg_decode_progressive_u8_bytes": (_c_int, [_c_int] * 6 + [_c_size_t, _c_int, ctypes.POINTER(_c_size_t)]),
    "adain_jpeg_decode_progressive_u8": (_c_int, [_c_void_p, _c_size_t, _c_void_p] + [_c_int] * 6 + [ctypes.POINTER(ctypes.c_int32), ctypes.POINTER(ctypes.c_uint64),
                                                  ctypes.POINTER(ctypes.c_uint32), _c_void_p, _c_void_p, _c_void_p, _c_size_t, _c_int, _c_void_p]),
    "adain_nhwc_to_nchw": (_c_int, [_c_void_p, _c_void_p, _c_int, _c_int, _c_int, _c_void_p]),
    "adain_nchw_to_nhwc": (_c_int, [_c_void_p, _c_void_p, _c_int, _c_int, _c_int, _c_void_p]),
    "adain_conv3x3_wino4_packed_floats": (_c_size_t, [_c_int, _c_int]),
    "adain_conv3x3_wino4_pack": (_c_int, [_c_void_p, _c_void_p, _c_int, _c_int, _c_void_p]),
    "adain_conv3x3_wino": (_c_int, [_c_void_p, _c_void_p, _c_void_p, _c_void_p] + [_c_int] * 11 + [_c_void_p]),
    "adain_conv3x3_wino4_split_workspace_bytes": (_c_size_t, [_c_int] * 5),
    "adain_conv3x3_up2x_poly_packed_floats": (_c_size_t, [_c_int, _c_int]),
    "adain_conv3x3_up2x_poly_pack": (_c_int, [_c_void_p, _c_void_p, _c_int, _c_int, _c_void_p]),
    "adain_conv3x3_up2x_poly": (_c_int, [_c_void_p, _c_void_p, _c_void_p, _c_void_p] + [_c_int] * 6 + [_c_void_p]),
    "adain_conv3x3_wino4_split": (_c_int, [_c_void_p, _c_void_p, _c_void_p, _c_void_p] + [_c_int] * 10 + [_c_void_p, _c_size_t, _c_void_p]),
}

# The GIF decoder's calls: include/adain_gif_decode.h, a header and a library of their own (the header says why).  name -> (restype,
# argtypes), one to one as above; ``_entry`` finds a name's function in the library that has it, so ``call`` launches both alike.
GIF_DECODE_LIB_PATH = os.path.join(_PKG, "libadain_gif_decode.so")
GIF_DECODE_SIGNATURES = {
    "adain_gif_decode_last_error": (ctypes.c_char_p, []),
    "adain_gif_decode_u8_bytes": (_c_int, [_c_int] * 3 + [_c_size_t, ctypes.POINTER(_c_size_t)]),
    "adain_gif_decode_u8": (_c_int, [_c_void_p, _c_size_t, _c_void_p] + [_c_int] * 3 + [_c_void_p, _c_void_p, _c_void_p, _c_size_t, _c_void_p]),
}

_lib = None
_gif_decode_lib = None
_lock = threading.Lock()


class AdainHipError(RuntimeError):
    pass


def lib():
    """Loads the shared library once.  Raises if it has not been built (``__graft_entry__.build()``)."""
    global _lib
    if _lib is None:
        with _lock:
            if _lib is None:
                if not os.path.exists(LIB_PATH):
                    raise AdainHipError(
                        f"{LIB_PATH} is missing: build it with `python applied-image-processing_amd/build.py` "
                        "(there is no CPU / PyTorch fallback for the AdaIN path)"
                    )
                l = ctypes.CDLL(LIB_PATH)
                for name, (res, args) in SIGNATURES.items():
                    f = getattr(l, name)
                    f.restype, f.argtypes = res, args
                if l.adain_abi_version() != ABI_VERSION:
                    raise AdainHipError(f"{LIB_PATH}: ABI version {l.adain_abi_version()}, this binding needs {ABI_VERSION} "
                                        "(rebuild: python applied-image-processing_amd/build.py)")
                _lib = l
    return _lib


def gif_decode_lib():
    """Loads the GIF decoder's library once.  Raises if it has not been built: a missing kernel is an error, never a fall-back."""
    global _gif_decode_lib
    if _gif_decode_lib is None:
        with _lock:
            if _gif_decode_lib is None:
                if not os.path.exists(GIF_DECODE_LIB_PATH):
                    raise AdainHipError(f"{GIF_DECODE_LIB_PATH} is missing: build it with `python applied-image-processing_amd/build.py`")
                l = ctypes.CDLL(GIF_DECODE_LIB_PATH)
                for name, (res, args) in GIF_DECODE_SIGNATURES.items():
                    f = getattr(l, name)
                    f.restype, f.argtypes = res, args
                _gif_decode_lib = l
    return _gif_decode_lib


def _entry(name):
    """The C function ``name`` of whichever library declares it."""
    return getattr(gif_decode_lib() if name in GIF_DECODE_SIGNATURES else lib(), name)


def use_library(path):
    """Switches the process to another build of the library (bench.py --lib: a same-box A/B against another build of the
    product library).  The product path always runs ``LIB_PATH``."""
    global _lib, LIB_PATH
    with _lock:
        _lib, LIB_PATH = None, path
    return lib()


ABI_CALLS = [0]          # compute calls made through the C ABI by this process (jobs report it per frame)


def _failure(what, rc):
    text = gif_decode_lib().adain_gif_decode_last_error() if what in GIF_DECODE_SIGNATURES else lib().adain_last_error()
    return AdainHipError(f"{what} failed ({rc}): {text.decode()}")


def _check(rc, what):
    ABI_CALLS[0] += 1
    if rc != 0:
        raise _failure(what, rc)


class schedule:
    """``with runtime.schedule(runtime.SCHEDULE_LATENCY): ...`` - the launch schedule of the calling thread for the C-ABI calls
    inside (adain_set_schedule: under LATENCY a generic 3x3 layer whose launch leaves compute units without a tile is split along
    cin; results then differ from the batch schedule's in the last bits and depend on the launch's batch size).  Restored on exit."""

    def __init__(self, value):
        self.value = int(value)

    def __enter__(self):
        self.prev = set_schedule(self.value)
        return self

    def __exit__(self, *exc):
        set_schedule(self.prev)
        return False


def set_schedule(value):
    """Sets the calling thread's schedule; returns the previous one."""
    prev = lib().adain_set_schedule(int(value))
    if prev < 0:
        raise _failure("adain_set_schedule", prev)
    return prev


def get_schedule():
    return lib().adain_get_schedule()


def _stream():
    return torch.cuda.current_stream().cuda_stream


def device_tensor(t, name, dtype=torch.float32):
    """``t`` contiguous, or AdainHipError when it is not a GPU tensor of ``dtype``."""
    if not isinstance(t, torch.Tensor) or not t.is_cuda:
        raise AdainHipError(f"{name}: expected a GPU tensor (the AdaIN path has no CPU fallback)")
    if t.dtype != dtype:
        raise AdainHipError(f"{name}: expected dtype {dtype}, got {t.dtype}")
    return t.contiguous()


def check_buffer(t, name, dtype, device, shape=None, numel=None, min_numel=None, align=None, distinct=()):
    """Refuses a caller-supplied buffer that a kernel could not be handed as it is: not a contiguous ``dtype`` GPU tensor on
    ``device``, not of ``shape`` / ``numel`` / at least ``min_numel`` elements, not ``align``-byte aligned, or starting where one
    of the ``distinct`` inputs starts.  AdainHipError("<name> must be ...") before anything is launched."""
    ok = (isinstance(t, torch.Tensor) and t.is_cuda and t.device == device and t.dtype == dtype and t.is_contiguous()
          and (shape is None or tuple(t.shape) == tuple(shape)) and (numel is None or t.numel() == numel)
          and (min_numel is None or t.numel() >= min_numel) and (align is None or t.data_ptr() % align == 0)
          and t.data_ptr() not in [d.data_ptr() for d in distinct])
    if not ok:
        size = (f"[{','.join(map(str, shape))}]" if shape is not None else f"{numel}-element" if numel is not None
                else f"at least {min_numel}-element" if min_numel is not None else "")
        raise AdainHipError(f"{name} must be a contiguous{f', {align}-byte aligned' if align else ''} {str(dtype)[6:]} {size} tensor "
                            f"on {device if device.type == 'cuda' else 'a GPU'}{', distinct from its inputs' if distinct else ''}")
    return t


def _ptr_array(tensors):
    arr = (ctypes.c_void_p * len(tensors))(*[t.data_ptr() for t in tensors])
    return ctypes.cast(arr, _PP), arr


# --- workspaces: one growing scratch buffer per (device, stream, tag) -----------------------------------------
# (keyed by stream so that independent frames can be in flight on different HIP streams)
_ws = {}


def workspace(device, tag, nbytes):
    key = (device.index if device.index is not None else torch.cuda.current_device(), torch.cuda.current_stream(device).cuda_stream, tag)
    buf = _ws.get(key)
    if buf is None or buf.numel() < nbytes:
        buf = None
        _ws.pop(key, None)
        buf = torch.empty(max(int(nbytes), 256), dtype=torch.uint8, device=device)
        _ws[key] = buf
    return buf


def free_workspaces():
    _ws.clear()


# --- the call path -----------------------------------------------------------------------------------------------
# THE RULE: a library function whose answer depends on the device that is current on the calling thread is called only inside
# call() or scratch(), which make the tensors' device current first.  Those functions are every launch (whatever takes a stream)
# and the size queries that count the device's compute units for the cin split: adain_encode_workspace_bytes,
# adain_encode_multi_workspace_bytes, adain_decode_workspace_bytes, adain_stylize_u8_workspace_bytes (and its _ex twin) and
# adain_conv3x3_wino4_split_workspace_bytes.  Asked elsewhere, such a query sizes the slabs for another device's compute units
# (the launch then refuses them as too small, with the layers before it already queued) and opens a HIP context on a GPU the
# caller never meant to touch.
def _launch(name, *args):
    """``lib().<name>(*args, stream)`` on the device that is current, with its current stream: counted in ABI_CALLS,
    AdainHipError("<name> failed (<rc>): <last error>") on a non-zero return."""
    _check(_entry(name)(*args, _stream()), name)


def call(name, device, *args):
    """One compute call of the C ABI: ``_launch`` with ``device`` current."""
    with torch.cuda.device(device):
        _launch(name, *args)


@contextlib.contextmanager
def scratch(device, tag, query, *dims, refuse=None):
    """``with scratch(device, tag, "adain_x_workspace_bytes", *dims) as ws: _launch(...)`` - the calling stream's ``tag`` workspace
    of ``device``, of the size ``lib().<query>(*dims)`` (or a callable's ``query(*dims)``) answers with ``device`` current; the body
    runs with it current too, so a wrapper enters the device once for its query and its launch.  ``refuse``: the AdainHipError
    text of a 0 answer, for the queries that refuse a size that way."""
    with torch.cuda.device(device):
        nbytes = getattr(lib(), query)(*dims) if isinstance(query, str) else query(*dims)
        if nbytes == 0 and refuse is not None:
            raise AdainHipError(refuse)
        yield workspace(device, tag, nbytes)


# --- weights ------------------------------------------------------------------------------------------------
ENC_KEYS = [0, 2, 5, 9, 12, 16, 19, 22, 25, 29]
DEC_KEYS = [1, 5, 8, 11, 14, 18, 21, 25, 28]


def _pack(net, keys, state_dict, device):
    ws = [device_tensor(state_dict[f"{k}.weight"].to(device=device, dtype=torch.float32), "weight") for k in keys]
    bs = [device_tensor(state_dict[f"{k}.bias"].to(device=device, dtype=torch.float32), "bias") for k in keys]
    packed = torch.empty(getattr(lib(), f"adain_{net}_packed_floats")(), dtype=torch.float32, device=device)
    wp, _k1 = _ptr_array(ws)
    bp, _k2 = _ptr_array(bs)
    call(f"adain_{net}_pack", packed.device, wp, bp, packed.data_ptr())
    torch.cuda.current_stream(packed.device).synchronize()   # the source tensors may be freed after return
    return packed


def pack_encoder(state_dict, device):
    """state_dict with reference keys ("0.weight", "2.weight", ... ) -> packed device buffer."""
    return _pack("encoder", ENC_KEYS, state_dict, device)


def pack_decoder(state_dict, device):
    return _pack("decoder", DEC_KEYS, state_dict, device)


# --- encoder / decoder -----------------------------------------------------------------------------------
def encoded_size(h, w):
    hc, wc = ctypes.c_int(), ctypes.c_int()
    lib().adain_encoded_size(h, w, ctypes.byref(hc), ctypes.byref(wc))
    return hc.value, wc.value


def _event_array(events):
    if events is None:
        return None, None
    arr = (ctypes.c_void_p * len(events))(*[e.cuda_event for e in events])
    return ctypes.cast(arr, _PP), arr


def _image_dims(x, refuse):
    """(n, h, w) of an image batch, uint8 NHWC [n,h,w,3] or float NCHW [n,3,h,w]; AdainHipError("<refuse>, got <shape>") for any other."""
    u8 = x.dtype == torch.uint8
    if x.dim() != 4 or x.shape[3 if u8 else 1] != 3:
        raise AdainHipError(f"{refuse}, got {tuple(x.shape)}")
    return (x.shape[0], x.shape[1], x.shape[2]) if u8 else (x.shape[0], x.shape[2], x.shape[3])


def _encode(name, x, u8, packed, events):
    x = device_tensor(x, "frames" if u8 else "image", torch.uint8 if u8 else torch.float32)
    n, h, w = _image_dims(x, f"{name}: expected {'uint8 [n,h,w,3]' if u8 else '[n,3,h,w]'}")
    hc, wc = encoded_size(h, w)
    feat = torch.empty((n, hc, wc, 512), dtype=torch.float32, device=x.device)
    ev, _keep = _event_array(events)
    with scratch(x.device, "conv", "adain_encode_workspace_bytes", n, h, w) as ws:
        _launch(f"adain_{name}", x.data_ptr(), feat.data_ptr(), packed.data_ptr(), ws.data_ptr(), ws.numel(), n, h, w, ev)
    return feat


def encode(image, packed, events=None):
    """image NCHW [n,3,h,w] -> relu4_1 features NHWC [n,hc,wc,512]."""
    return _encode("encode", image, False, packed, events)


def encode_u8(frames_u8, packed, events=None):
    """Decoded frames HWC uint8 [n,h,w,3] -> relu4_1 features NHWC [n,hc,wc,512]; ToTensor (v / 255) happens inside the first
    layer's kernel: bit-identical to ``encode(u8_to_f32(frames_u8))``."""
    return _encode("encode_u8", frames_u8, True, packed, events)


def encode_relu1_1(image, packed):
    """vgg[:4] (conv0 -> pad -> conv1_1 -> relu, net.py:39-42) as the one folded layer the encoder starts with: image NCHW float
    [n,3,h,w] or decoded uint8 frames [n,h,w,3] -> relu1_1 NHWC [n,h,w,64]."""
    u8 = isinstance(image, torch.Tensor) and image.dtype == torch.uint8
    x = device_tensor(image, "image", torch.uint8 if u8 else torch.float32)
    n, h, w = _image_dims(x, "encode_relu1_1: expected float [n,3,h,w] or uint8 [n,h,w,3]")
    out = torch.empty((n, h, w, 64), dtype=torch.float32, device=x.device)
    call("adain_encode_relu1_1", x.device, x.data_ptr(), 1 if u8 else 0, out.data_ptr(), packed.data_ptr(), n, h, w)
    return out


def encode_multi(images, packed, events=None):
    """Several image batches [n_i,3,h_i,w_i] of different sizes through the encoder in one pass (the content batch and the
    style image of one style_transfer call) -> list of relu4_1 features NHWC; bit-identical to ``encode`` per batch."""
    images = [device_tensor(x, "image") for x in images]
    for x in images:
        if x.dim() != 4 or x.shape[1] != 3:
            raise AdainHipError(f"encode: expected [n,3,h,w], got {tuple(x.shape)}")
        if x.device != images[0].device:
            raise AdainHipError("encode_multi: all image batches must be on one device")
    k = len(images)
    IntArr = _c_int * k
    n, h, w = IntArr(*[x.shape[0] for x in images]), IntArr(*[x.shape[2] for x in images]), IntArr(*[x.shape[3] for x in images])
    feats = []
    for x in images:
        hc, wc = encoded_size(x.shape[2], x.shape[3])
        feats.append(torch.empty((x.shape[0], hc, wc, 512), dtype=torch.float32, device=x.device))
    ip, _k1 = _ptr_array(images)
    fp, _k2 = _ptr_array(feats)
    ev, _keep = _event_array(events)
    with scratch(images[0].device, "conv", "adain_encode_multi_workspace_bytes", k, n, h, w,
                 refuse=f"encode_multi: 1..4 image batches per call, got {k}") as ws:
        _launch("adain_encode_multi", k, ip, fp, n, h, w, packed.data_ptr(), ws.data_ptr(), ws.numel(), ev)
    return feats


def decode(feat, packed, events=None):
    """features NHWC [n,hc,wc,512] -> image NCHW [n,3,8hc,8wc]."""
    feat = device_tensor(feat, "feat")
    if feat.dim() != 4 or feat.shape[3] != 512:
        raise AdainHipError(f"decode: expected NHWC [n,hc,wc,512], got {tuple(feat.shape)}")
    n, hc, wc, _ = feat.shape
    img = torch.empty((n, 3, 8 * hc, 8 * wc), dtype=torch.float32, device=feat.device)
    ev, _keep = _event_array(events)
    with scratch(feat.device, "conv", "adain_decode_workspace_bytes", n, hc, wc) as ws:
        _launch("adain_decode", feat.data_ptr(), img.data_ptr(), packed.data_ptr(), ws.data_ptr(), ws.numel(), n, hc, wc, ev)
    return img


# --- statistics and blend ------------------------------------------------------------------------------
def _feat_dims(x, nhwc):
    """(n, c, h * w) of a feature tensor NHWC [n,h,w,c] (nhwc) or NCHW [n,c,h,w]."""
    if nhwc:
        n, h, w, c = x.shape
    else:
        n, c, h, w = x.shape
    return n, c, h * w


def mean_std(feat, nhwc, eps=1e-5):
    """feat NHWC [n,h,w,c] (nhwc=True) or NCHW [n,c,h,w] -> (mean [n,c], std [n,c])."""
    feat = device_tensor(feat, "feat")
    assert feat.dim() == 4
    n, c, hw = _feat_dims(feat, nhwc)
    mean = torch.empty((n, c), dtype=torch.float32, device=feat.device)
    std = torch.empty_like(mean)
    with scratch(feat.device, "stats", "adain_mean_std_workspace_bytes", int(nhwc), n, c, hw) as ws:
        _launch("adain_mean_std", feat.data_ptr(), int(nhwc), n, c, hw, eps, mean.data_ptr(), std.data_ptr(), ws.data_ptr(), ws.numel())
    return mean, std


def _blend(name, x, nhwc, c_mean, c_std, term):
    """The blends' common call: ``term(x, n, c, hw)`` checks and returns the arguments between ``c_std`` and ``out`` (tensors as they
    are, so that they live until the call is made)."""
    x = device_tensor(x, "content_feat")
    if x.dim() != 4:
        raise AdainHipError(f"{name}: expected a 4-D feature tensor, got {tuple(x.shape)}")
    n, c, hw = _feat_dims(x, nhwc)
    args = term(x, n, c, hw)
    out = torch.empty_like(x)
    call("adain_" + name, x.device, x.data_ptr(), int(nhwc), n, c, hw, c_mean.data_ptr(), c_std.data_ptr(),
         *(a.data_ptr() if isinstance(a, torch.Tensor) else a for a in args), out.data_ptr())
    return out


def blend_alpha(x, nhwc, c_mean, c_std, s_mean, s_std, alpha):
    """AdaIN(x) * alpha + x * (1 - alpha);  alpha = 1 gives plain adaptive_instance_normalization."""
    return _blend("blend_alpha", x, nhwc, c_mean, c_std, lambda x, n, c, hw: (s_mean, s_std, s_mean.shape[0], float(alpha), float(1 - alpha)))


def _pmap(pmap, hw, what):
    """(the strength maps P [pn,hc,wc] contiguous on the device, pn) for feature maps of ``hw`` pixels."""
    pmap = device_tensor(pmap, "pmap")
    pn = pmap.numel() // hw
    if pn * hw != pmap.numel():
        raise AdainHipError(f"{what}: strength map size does not match the feature map")
    return pmap, pn


def blend_pmap(x, nhwc, c_mean, c_std, s_mean, s_std, pmap):
    """AdaIN(x) * (1 - P) + x * P with P [pn, hc, wc] (pn in {1, n})."""
    return _blend("blend_pmap", x, nhwc, c_mean, c_std, lambda x, n, c, hw: (s_mean, s_std, s_mean.shape[0]) + _pmap(pmap, hw, "blend_pmap"))


MIX_MAX_STYLES = 16          # ADAIN_MIX_MAX_STYLES


def mix_weights(weights, n, k, hc, wc, device, what):
    """Style-mix weights as the C ABI takes them: ``weights`` float32 on ``device`` shaped [k], [n,k], [k,hc,wc] or [n,k,hc,wc]
    (a row for all frames or one per frame; scalars or maps at feature resolution) -> (contiguous tensor, weights_n, weights_hw).
    The values are handed over as they are: nothing normalises them."""
    weights = device_tensor(weights, f"{what}: style weights")
    shapes = {(k,): (1, 1), (n, k): (n, 1), (k, hc, wc): (1, hc * wc), (n, k, hc, wc): (n, hc * wc)}
    if weights.device != device or tuple(weights.shape) not in shapes:
        raise AdainHipError(f"{what}: style weights must be [{k}], [{n},{k}], [{k},{hc},{wc}] or [{n},{k},{hc},{wc}] on the features' device, "
                            f"got {tuple(weights.shape)}")
    return (weights,) + shapes[tuple(weights.shape)]


def blend_mix(x, nhwc, c_mean, c_std, s_mean, s_std, weights, alpha=None, pmap=None):
    """The blend of a weighted mix of K styles (``adain_blend_mix``; test_video.py:36-44): feat = sum_k w_k (nrm * s_std[k] +
    s_mean[k]) accumulated in style order, then feat * alpha + x * (1 - alpha), or feat * (1 - P) + x * P when ``pmap`` [1|n,...] is
    given.  s_mean / s_std [K,c]: one set of styles for the batch; ``weights`` [K], [n,K], [K,hc,wc] or [n,K,hc,wc] on the device,
    used as given.  Exactly one of ``alpha`` and ``pmap``."""
    if (alpha is None) == (pmap is None):
        raise AdainHipError("blend_mix: exactly one of alpha and pmap")

    def term(x, n, c, hw):
        hc, wc = (x.shape[1], x.shape[2]) if nhwc else (x.shape[2], x.shape[3])
        sm, sd = device_tensor(s_mean, "s_mean"), device_tensor(s_std, "s_std")
        k = sm.numel() // c
        if not 1 <= k <= MIX_MAX_STYLES or sm.numel() != k * c or sd.numel() != k * c:
            raise AdainHipError(f"blend_mix: style statistics must be [K,{c}] each with 1 <= K <= {MIX_MAX_STYLES}, got {tuple(sm.shape)}, "
                                f"{tuple(sd.shape)}")
        a = 0.0 if alpha is None else float(alpha)
        return (sm, sd, k) + mix_weights(weights, n, k, hc, wc, x.device, "blend_mix") + (a, float(1 - a)) + (
            (None, 1) if pmap is None else _pmap(pmap, hw, "blend_mix"))

    return _blend("blend_mix", x, nhwc, c_mean, c_std, term)


def strength_map(depth, hc, wc, offset, prominence):
    """depth [h0,w0] -> P [1,1,hc,wc]."""
    depth = device_tensor(depth, "depth_map")
    if depth.dim() != 2:
        raise AdainHipError(f"strength_map: expected a 2-D depth map, got {tuple(depth.shape)}")
    h0, w0 = depth.shape
    p = torch.empty((1, 1, hc, wc), dtype=torch.float32, device=depth.device)
    with scratch(depth.device, "pmap", "adain_strength_map_workspace_bytes", hc, wc) as ws:
        _launch("adain_strength_map", depth.data_ptr(), h0, w0, hc, wc, float(offset), float(prominence), p.data_ptr(), ws.data_ptr(),
                ws.numel())
    return p


# --- pixel kernels -----------------------------------------------------------------------------------------
def _map(name, x, shape, *dims, dtype=torch.float32):
    """A call that reads ``x`` and writes a new ``dtype`` tensor of ``shape``: ``lib().<name>(x, out, *dims, stream)``."""
    out = torch.empty(shape, dtype=dtype, device=x.device)
    call(name, x.device, x.data_ptr(), out.data_ptr(), *dims)
    return out


def _resize(name, x, size):
    x = device_tensor(x, name)
    assert x.dim() == 4
    n, c, hi, wi = x.shape
    ho, wo = size
    return _map(name, x, (n, c, ho, wo), n * c, hi, wi, ho, wo)


def resize_bilinear(x, size):
    return _resize("adain_resize_bilinear", x, size)


def resize_nearest(x, size):
    return _resize("adain_resize_nearest", x, size)


def mask_composite(content, stylized, mask):
    """content, stylized NCHW [n,c,h,w]; mask [mn,mc,h,w] float -> content*(1-m) + stylized*m."""
    content, stylized, mask = device_tensor(content, "content"), device_tensor(stylized, "stylized"), device_tensor(mask, "mask")
    n, c, h, w = content.shape
    if stylized.shape != content.shape or mask.shape[-2:] != content.shape[-2:]:
        raise AdainHipError("mask_composite: shape mismatch")
    out = torch.empty_like(content)
    call("adain_mask_composite", content.device, content.data_ptr(), stylized.data_ptr(), mask.data_ptr(), mask.shape[1], mask.shape[0],
         out.data_ptr(), n, c, h * w)
    return out


def quantize_u8(img, out=None):
    """NCHW float [n,c,h,w] -> NHWC uint8 [n,h,w,c] (x*255 + 0.5, clamp, truncate); ``out``: a contiguous uint8 [n,h,w,c] GPU
    tensor to write into (a slice of a job's frame block)."""
    img = device_tensor(img, "image")
    n, c, h, w = img.shape
    if out is None:
        out = torch.empty((n, h, w, c), dtype=torch.uint8, device=img.device)
    else:
        check_buffer(out, "quantize_u8: out", torch.uint8, img.device, shape=(n, h, w, c))
    call("adain_quantize_u8", img.device, img.data_ptr(), out.data_ptr(), n, c, h, w)
    return out


def _stylize_u8_styles(x, s_mean, s_std, style_n, style_weights):
    """(the entry point of a ``stylize_u8`` call of the frames ``x``, what it takes between ``s_std`` and ``alpha``): adain_stylize_u8 (),
    _ex (style_n,) or _mix (K, weights, weights_n, weights_hw) - with the statistics checked for the rows that form takes."""
    n, h, w, _ = x.shape
    mixing = style_weights is not None
    if mixing and style_n is not None:
        raise AdainHipError("stylize_u8: style_weights mixes one set of styles for the batch; style_n does not apply")
    rows = s_mean.numel() // 512 if mixing else 1 if style_n is None else int(style_n)
    if mixing and not 1 <= rows <= MIX_MAX_STYLES:
        raise AdainHipError(f"stylize_u8: a style mix needs statistics [K,512] each, 1 <= K <= {MIX_MAX_STYLES}, got {tuple(s_mean.shape)}")
    if not mixing and rows not in (1, n):
        raise AdainHipError(f"stylize_u8: style_n must be 1 or {n}, got {rows}")
    if s_mean.numel() != rows * 512 or s_std.numel() != rows * 512 or s_mean.device != x.device or s_std.device != x.device:
        raise AdainHipError(f"stylize_u8: the style statistics must be [{rows},512] each on the frames' device, got {tuple(s_mean.shape)}, "
                            f"{tuple(s_std.shape)}")
    if mixing:
        weights, wn, whw = mix_weights(style_weights, n, rows, *encoded_size(h, w), x.device, "stylize_u8")
        return "adain_stylize_u8_mix", (rows, weights.data_ptr(), wn, whw)
    return ("adain_stylize_u8", ()) if style_n is None else ("adain_stylize_u8_ex", (rows,))


def stylize_u8(frames_u8, enc_packed, dec_packed, s_mean, s_std, alpha=0.5, depth_maps=None, depth_offset=0.15, depth_prominence=20,
               mask=None, out=None, style_n=None, style_weights=None):
    """One sub-batch of decoded frames through the whole path in ONE call of the C ABI (``adain_stylize_u8``: ToTensor + encoder,
    statistics, AdaIN blend - the alpha form, or the depth-aware form when ``depth_maps`` (one [h0,w0] float GPU tensor per frame)
    are given - decoder, mask composite, uint8 quantiser); the bytes the separate calls give.  frames_u8 uint8 [n,h,w,3]; s_mean /
    s_std [1,512]; mask [1|n, 1|3, hm, wm] uint8 / bool / float32 on the GPU.  Returns uint8 [n,oh,ow,3] (``out`` if given).
    ``style_n`` (1 or n): the call goes through ``adain_stylize_u8_ex`` with s_mean / s_std [style_n,512], one style per frame when
    it is n (the colour-preserving path: every frame has its own recoloured style).
    ``style_weights`` ([K], [n,K], [K,hc,wc] or [n,K,hc,wc] on the device, used as given): the call goes through
    ``adain_stylize_u8_mix`` with s_mean / s_std [K,512], every frame styled with the weighted mix of the K styles (``blend_mix``)."""
    x = device_tensor(frames_u8, "frames", torch.uint8)
    if x.dim() != 4 or x.shape[3] != 3:
        raise AdainHipError(f"stylize_u8: expected uint8 [n,h,w,3], got {tuple(x.shape)}")
    n, h, w, _ = x.shape
    dev = x.device
    s_mean, s_std = device_tensor(s_mean, "s_mean"), device_tensor(s_std, "s_std")
    if style_weights is not None:
        style_weights = device_tensor(style_weights, "stylize_u8: style weights")      # held here until the launch
    name, styles = _stylize_u8_styles(x, s_mean, s_std, style_n, style_weights)
    mn = mc = mh = mw = 0
    m_float, m_ptr = 0, None
    if mask is not None:
        if not isinstance(mask, torch.Tensor) or not mask.is_cuda or mask.dim() != 4:
            raise AdainHipError("stylize_u8: mask must be a GPU tensor [1|n, 1|3, hm, wm]")
        if mask.dtype == torch.float32:
            m_float = 1
        elif mask.dtype not in (torch.uint8, torch.bool):
            raise AdainHipError(f"stylize_u8: mask dtype {mask.dtype} (uint8, bool or float32)")
        mask = mask.contiguous()
        mn, mc, mh, mw = mask.shape
        m_ptr = mask.data_ptr()
    dp = dh = dw = None
    if depth_maps is not None:
        depth_maps = [device_tensor(d, "depth_map") for d in depth_maps]
        if len(depth_maps) != n or any(d.dim() != 2 for d in depth_maps):
            raise AdainHipError(f"stylize_u8: need {n} depth maps [h0,w0], one per frame")
        dp, _keep = _ptr_array(depth_maps)
        dh = (_c_int * n)(*[d.shape[0] for d in depth_maps])
        dw = (_c_int * n)(*[d.shape[1] for d in depth_maps])
    oh, ow = ctypes.c_int(), ctypes.c_int()
    lib().adain_stylize_u8_out_size(h, w, int(mask is not None), ctypes.byref(oh), ctypes.byref(ow))
    shape = (n, oh.value, ow.value, 3)
    if out is None:
        out = torch.empty(shape, dtype=torch.uint8, device=dev)
    else:
        check_buffer(out, "stylize_u8: out", torch.uint8, dev, shape=shape)
    with scratch(dev, "stylize", f"{name}_workspace_bytes", n, h, w, int(depth_maps is not None), mn, mc, mh, mw, m_float) as ws:
        _launch(name, x.data_ptr(), n, h, w, enc_packed.data_ptr(), dec_packed.data_ptr(), s_mean.data_ptr(), s_std.data_ptr(), *styles,
                float(alpha), float(1 - alpha), dp, dh, dw, float(depth_offset), float(depth_prominence), m_ptr, m_float, mn, mc, mh, mw,
                out.data_ptr(), ws.data_ptr(), ws.numel())
    return out


def u8_to_f32(frames_u8):
    """torchvision ToTensor on the device: NHWC uint8 [n,h,w,c] -> NCHW float [n,c,h,w] = v / 255 (bit for bit the host's)."""
    x = device_tensor(frames_u8, "frames", torch.uint8)
    if x.dim() != 4:
        raise AdainHipError(f"u8_to_f32: expected uint8 [n,h,w,c], got {tuple(x.shape)}")
    n, h, w, c = x.shape
    return _map("adain_u8_to_f32", x, (n, c, h, w), n, c, h, w)


def warp_blend_u8(cur, prev, flow, alpha, out=None):
    """Video post-pass: cur, prev uint8 [h,w,c]; flow float32 [2,h,w] -> blended uint8 [h,w,c] (written into ``out`` when given: a
    contiguous uint8 [h,w,c] GPU tensor that is neither ``cur`` nor ``prev`` - a row of the clip's result block)."""
    cur, prev, flow = device_tensor(cur, "cur", torch.uint8), device_tensor(prev, "prev", torch.uint8), device_tensor(flow, "flow")
    h, w, c = cur.shape
    if prev.shape != cur.shape or tuple(flow.shape) != (2, h, w):
        raise AdainHipError("warp_blend_u8: shape mismatch")
    if out is None:
        out = torch.empty_like(cur)
    else:
        check_buffer(out, "warp_blend_u8: out", torch.uint8, cur.device, shape=cur.shape, distinct=(cur, prev))
    call("adain_warp_blend_u8", cur.device, cur.data_ptr(), prev.data_ptr(), flow.data_ptr(), out.data_ptr(), h, w, c, float(alpha),
         float(1 - alpha))
    return out


# --- the localized pipeline's colour transfer (adain_colour_transfer_u8 / adain_localized_combine_u8) ---------------------------
COLOUR_FG_EMPTY, COLOUR_BG_EMPTY, COLOUR_FG_SINGLE, COLOUR_BG_SINGLE = 1, 2, 4, 8      # ADAIN_COLOUR_*: adain_colour_record.status


class _ColourRegion(ctypes.Structure):
    _fields_ = [("n", ctypes.c_int64), ("mean", ctypes.c_double * 3), ("component", ctypes.c_double * 3), ("explained_variance", ctypes.c_double)]


class _ColourRecord(ctypes.Structure):        # adain_colour_record of include/adain_hip.h
    _fields_ = [("fg", _ColourRegion), ("bg", _ColourRegion), ("status", ctypes.c_int32), ("reserved", ctypes.c_int32)]


COLOUR_RECORD_BYTES = ctypes.sizeof(_ColourRecord)


def colour_record(record):
    """The device record a colour call returned (uint8 [COLOUR_RECORD_BYTES]) as a dict: ``status`` and per region (``fg``, ``bg``)
    ``n``, ``mean``, ``component``, ``explained_variance``.  One fixed-size copy to the host, which waits for the call's stream."""
    raw = _ColourRecord.from_buffer_copy(record.cpu().numpy().tobytes())
    region = lambda r: dict(n=int(r.n), mean=list(r.mean), component=list(r.component), explained_variance=float(r.explained_variance))
    return dict(status=int(raw.status), fg=region(raw.fg), bg=region(raw.bg))


def _colour_call(name, images, out):
    h, w, c = images[0].shape
    dev = images[0].device
    if out is None:
        out = torch.empty((h, w, 3), dtype=torch.uint8, device=dev)
    else:
        check_buffer(out, f"{name}: out", torch.uint8, dev, shape=(h, w, 3), distinct=images)
    with scratch(dev, "colour", "adain_colour_transfer_workspace_bytes", h, w, refuse=f"{name}: unsupported size {h} x {w}") as ws:
        _launch(f"adain_{name}", *[t.data_ptr() for t in images], out.data_ptr(), h, w, ws.data_ptr())
        record = ws[:COLOUR_RECORD_BYTES].clone()        # the workspace is the stream's: the next call overwrites it
    return out, record


def colour_transfer_u8(fg, bg, out=None):
    """color_transfer_foreground (Style_3DGS/localized_style_transfer.py:128-168) on the device: fg, bg uint8 [h,w,3] -> (adjusted
    foreground uint8 [h,w,3], device record for ``colour_record``).  Nothing is copied to the host: an empty or one-pixel region leaves
    a copy of ``fg`` and a non-zero status in the record."""
    fg, bg = device_tensor(fg, "fg", torch.uint8), device_tensor(bg, "bg", torch.uint8)
    if fg.dim() != 3 or fg.shape[2] != 3 or bg.shape != fg.shape or bg.device != fg.device:
        raise AdainHipError(f"colour_transfer_u8: expected two uint8 [h,w,3] images of one size on one device, got {tuple(fg.shape)} and {tuple(bg.shape)}")
    return _colour_call("colour_transfer_u8", (fg, bg), out)


def localized_combine_u8(content, stylised, mask, out=None):
    """The composite of run_localized_style_transfer (:232-238) with the colour transfer inside: content, stylised uint8 [h,w,3], mask
    uint8 [h,w] holding 0 and 1 only (1 = background; NOT checked here, that would wait for the device) -> (uint8 [h,w,3], record)."""
    content, stylised, mask = (device_tensor(content, "content", torch.uint8), device_tensor(stylised, "stylised", torch.uint8),
                               device_tensor(mask, "mask", torch.uint8))
    if (content.dim() != 3 or content.shape[2] != 3 or stylised.shape != content.shape or tuple(mask.shape) != tuple(content.shape[:2])
            or stylised.device != content.device or mask.device != content.device):
        raise AdainHipError(f"localized_combine_u8: expected uint8 [h,w,3], [h,w,3] and [h,w] on one device, got {tuple(content.shape)}, "
                            f"{tuple(stylised.shape)} and {tuple(mask.shape)}")
    return _colour_call("localized_combine_u8", (content, stylised, mask), out)


# --- colour preservation (adain_coral) ------------------------------------------------------------------------------------------
CORAL_STYLE_FLAT, CORAL_CONTENT_FLAT, CORAL_STYLE_SINGLE, CORAL_CONTENT_SINGLE = 1, 2, 4, 8      # ADAIN_CORAL_*: adain_coral_record.status


class _CoralSide(ctypes.Structure):
    _fields_ = [("n", ctypes.c_int64), ("sum", ctypes.c_int64 * 3), ("sum2", ctypes.c_int64 * 6), ("mean", ctypes.c_double * 3),
                ("std", ctypes.c_double * 3)]


class _CoralRecord(ctypes.Structure):         # adain_coral_record of include/adain_hip.h
    _fields_ = [("A", ctypes.c_double * 9), ("b", ctypes.c_double * 3), ("style", _CoralSide), ("content", _CoralSide),
                ("status", ctypes.c_int32), ("reserved", ctypes.c_int32)]


CORAL_RECORD_BYTES = ctypes.sizeof(_CoralRecord)


def coral_record(record):
    """The device records a ``coral`` call returned (uint8 [n, CORAL_RECORD_BYTES]) as a list of dicts, one per pair: ``status``,
    ``A`` (3 x 3 nested lists), ``b`` and per side (``style``, ``content``) ``n``, ``sum``, ``sum2``, ``mean``, ``std``.  One copy to
    the host, which waits for the call's stream."""
    raw = record.cpu().numpy().tobytes()
    side = lambda s: dict(n=int(s.n), sum=list(s.sum), sum2=list(s.sum2), mean=list(s.mean), std=list(s.std))
    out = []
    for i in range(len(raw) // CORAL_RECORD_BYTES):
        r = _CoralRecord.from_buffer_copy(raw, i * CORAL_RECORD_BYTES)
        out.append(dict(status=int(r.status), A=[list(r.A[3 * k:3 * k + 3]) for k in range(3)], b=list(r.b), style=side(r.style),
                        content=side(r.content)))
    return out


def _coral_side(t, name):
    """(contiguous tensor, is_u8, k, h, w) of one side of ``coral``: uint8 [k,h,w,3] or float32 [k,3,h,w] on a GPU."""
    if not isinstance(t, torch.Tensor) or not t.is_cuda or t.dtype not in (torch.uint8, torch.float32) or t.dim() != 4:
        raise AdainHipError(f"coral: {name} must be a GPU tensor, uint8 [k,h,w,3] or float32 [k,3,h,w]")
    return (t.contiguous(), int(t.dtype == torch.uint8)) + _image_dims(t, f"coral: {name} must be uint8 [k,h,w,3] or float32 [k,3,h,w]")


def coral(style, content, out=None):
    """``coral(style_i, content_i)`` of the reference (function.py:26-67) for n contents and 1 or n styles on the device
    (``adain_coral``): each side uint8 [k,h,w,3] or float32 [k,3,h,w], sizes independent -> (float32 [n,3,hs,ws], ready for ``encode``
    and not clamped; device records uint8 [n, CORAL_RECORD_BYTES] for ``coral_record``).  Nothing is copied to the host: a degenerate
    pair (a flat channel, a single pixel) gets a copy of its style and a non-zero status in its record."""
    s, s_u8, sn, hs, ws_ = _coral_side(style, "style")
    c, c_u8, n, hc, wc = _coral_side(content, "content")
    if c.device != s.device or sn not in (1, n):
        raise AdainHipError(f"coral: {sn} style image(s) for {n} content image(s) (1 or one per content, on one device)")
    dev = c.device
    if out is None:
        out = torch.empty((n, 3, hs, ws_), dtype=torch.float32, device=dev)
    else:
        check_buffer(out, "coral: out", torch.float32, dev, shape=(n, 3, hs, ws_), distinct=(s, c))
    with scratch(dev, "coral", "adain_coral_workspace_bytes", n, sn, hs, ws_, hc, wc,
                 refuse=f"coral: unsupported shape ({sn} x {hs} x {ws_} style, {n} x {hc} x {wc} content)") as ws:
        _launch("adain_coral", s.data_ptr(), s_u8, sn, hs, ws_, c.data_ptr(), c_u8, n, hc, wc, out.data_ptr(), ws.data_ptr(), ws.numel())
        record = ws[:n * CORAL_RECORD_BYTES].clone().view(n, CORAL_RECORD_BYTES)      # the workspace is the stream's: the next call overwrites it
    return out, record


def resize_area_u8(frames, dsize):
    """cv2.resize(frame, dsize, interpolation=cv2.INTER_AREA) on uint8 HWC frames: [h,w,c] or a batch [n,h,w,c];
    ``dsize`` = (width, height) as in cv2 (reference video/utils.py:352-353): the true-area branch when both axes shrink
    or stay, OpenCV's fixed-point linear emulation when one is enlarged."""
    frames = device_tensor(frames, "frames", torch.uint8)
    single = frames.dim() == 3
    if single:
        frames = frames.unsqueeze(0)
    if frames.dim() != 4:
        raise AdainHipError(f"resize_area_u8: expected [h,w,c] or [n,h,w,c] uint8, got {tuple(frames.shape)}")
    n, hi, wi, c = frames.shape
    wo, ho = int(dsize[0]), int(dsize[1])
    out = _map("adain_resize_area_u8", frames, (n, ho, wo, c), n, hi, wi, c, ho, wo, dtype=torch.uint8)
    return out[0] if single else out


_pil_lock = threading.Lock()


def resize_pil_bilinear_u8(frames, size, crop=None, out=None):
    """``PIL.Image.resize(size, BILINEAR)`` of uint8 images on the device, bit for bit (test.py:16-24's Resize on a PIL image).
    frames: uint8 [n,h,w,3] (packed RGB) or [n,h,w,4] (Pillow's RGBX storage); ``size`` = (width, height) as PIL takes it;
    ``crop`` = (top, left, height, width) window of the result (CenterCrop), default all of it.  Returns packed RGB uint8 [n,ch,cw,3]."""
    x = device_tensor(frames, "frames", torch.uint8)
    if x.dim() != 4 or x.shape[3] not in (3, 4):
        raise AdainHipError(f"resize_pil_bilinear_u8: expected uint8 [n,h,w,3|4], got {tuple(x.shape)}")
    n, hi, wi, pix = x.shape
    wo, ho = int(size[0]), int(size[1])
    y0, x0, ch, cw = (0, 0, ho, wo) if crop is None else [int(v) for v in crop]
    if out is None:
        out = torch.empty((n, max(ch, 0), max(cw, 0), 3), dtype=torch.uint8, device=x.device)
    else:
        check_buffer(out, "resize_pil_bilinear_u8: out", torch.uint8, x.device, shape=(n, ch, cw, 3))
    # the tap tables live in the stream's workspace between the call's two launches: calls from several threads (the job feeders'
    # fetch pool) on one stream must not interleave
    with _pil_lock, scratch(x.device, "pil", "adain_resize_pil_bilinear_u8_workspace_bytes", hi, wi, ho, wo) as ws:
        _launch("adain_resize_pil_bilinear_u8", x.data_ptr(), pix, n, hi, wi, out.data_ptr(), ho, wo, y0, x0, ch, cw, ws.data_ptr(), ws.numel())
    return out


# --- PIL.Image.resize for all six filters (adain_resize_pil_u8) ---------------------------------------------------------------------------
PIL_NEAREST, PIL_LANCZOS, PIL_BILINEAR, PIL_BICUBIC, PIL_BOX, PIL_HAMMING = 0, 1, 2, 3, 4, 5          # PIL.Image.Resampling
PIL_FILTERS = {"NEAREST": PIL_NEAREST, "BOX": PIL_BOX, "BILINEAR": PIL_BILINEAR, "HAMMING": PIL_HAMMING, "BICUBIC": PIL_BICUBIC, "LANCZOS": PIL_LANCZOS}
PIL_MAX_SHRINK = 256          # in / out per axis beyond which adain_resize_pil_u8 refuses
PIL_TABLES_KEPT = 32          # axes whose device tables are kept, least recently used first out
PIL_TABLE_STATS = {"hits": 0, "uploads": 0}          # per axis of a call: found in the cache / built on the host and uploaded
_pil_tables = collections.OrderedDict()          # (device index, filter, in, out) -> (ksize, int32 device tensor: bounds, then taps, its stream)


def pil_filter(resample):
    """Pillow's integer code of ``resample``: an ``Image.Resampling`` member, its code, or its name."""
    code = PIL_FILTERS.get(resample.upper()) if isinstance(resample, str) else int(resample)
    if code not in PIL_FILTERS.values():
        raise AdainHipError(f"resize_pil_u8: unknown resampling filter {resample!r} (one of {', '.join(PIL_FILTERS)})")
    return code


def _pil_taps_host(code, in_size, out_size):
    """-> (ksize, one int32 array: bounds [out,2], then taps [out,ksize]) as adain_pil_resize_taps builds them.  Host only."""
    import numpy as np

    ksize, nbytes = _c_int(), _c_size_t()
    rc = lib().adain_pil_resize_taps_bytes(code, int(in_size), int(out_size), ctypes.byref(ksize), ctypes.byref(nbytes))
    if rc != 0:
        raise _failure("adain_pil_resize_taps_bytes", rc)
    table = np.empty(nbytes.value // 4, np.int32)
    rc = lib().adain_pil_resize_taps(code, int(in_size), int(out_size), table.ctypes.data, table.ctypes.data + 8 * out_size if ksize.value else None)
    if rc != 0:
        raise _failure("adain_pil_resize_taps", rc)
    return ksize.value, table


def pil_resize_taps(resample, in_size, out_size):
    """The tables of one axis as ``adain_pil_resize_taps`` builds them on the host (no device needed) ->
    (ksize, bounds int32 [out,2], taps int32 [out,ksize]) as NumPy arrays."""
    ksize, table = _pil_taps_host(pil_filter(resample), in_size, out_size)
    return ksize, table[:2 * out_size].reshape(out_size, 2), table[2 * out_size:].reshape(out_size, ksize)


def _pil_axis_tables(device, code, in_size, out_size, stream):
    """(ksize, device table) of one axis from the cache, built and uploaded when it is not there.  Called under ``_pil_lock`` with
    ``device`` current; ``stream``: the calling stream's handle."""
    key = (device.index if device.index is not None else torch.cuda.current_device(), code, in_size, out_size)
    hit = _pil_tables.get(key)
    if hit is not None:
        _pil_tables.move_to_end(key)
        PIL_TABLE_STATS["hits"] += 1
        if hit[2] != stream:          # it may leave the cache while this stream still reads it
            hit[1].record_stream(torch.cuda.current_stream(device))
        return hit[:2]
    ksize, host = _pil_taps_host(code, in_size, out_size)
    # a copy from pageable memory has arrived when .to() returns: any stream may read the table afterwards
    table = torch.from_numpy(host).to(device)
    PIL_TABLE_STATS["uploads"] += 1
    _pil_tables[key] = (ksize, table, stream)
    while len(_pil_tables) > PIL_TABLES_KEPT:
        _pil_tables.popitem(last=False)
    return ksize, table


def free_pil_tables():
    with _pil_lock:
        _pil_tables.clear()


def resize_pil_u8(frames, size, resample=PIL_BILINEAR, crop=None, out=None):
    """``PIL.Image.resize(size, resample)`` of uint8 images on the device for Pillow's six filters (NEAREST, BOX, BILINEAR, HAMMING,
    BICUBIC, LANCZOS: ``Image.Resampling`` members, their codes or names), bit for bit; no ``box=``, no ``reducing_gap``.
    frames: uint8 [n,h,w,3] (packed RGB), [n,h,w,4] (Pillow's RGBX storage), [n,h,w,1] or [n,h,w] (L); ``size`` = (width, height) as PIL
    takes it; ``crop`` = (top, left, height, width) window of the result, default all of it.  Returns packed RGB [n,ch,cw,3], or L in
    the source's rank.  The tap tables come from the host (``pil_resize_taps``) and stay on the device in a small LRU cache per
    (device, filter, in, out): a clip's second frame costs the two launches and no upload.  An unchanged size gives a copy."""
    x = device_tensor(frames, "frames", torch.uint8)
    flat = x.dim() == 3
    if flat:
        x = x.unsqueeze(3)
    if x.dim() != 4 or x.shape[3] not in (1, 3, 4):
        raise AdainHipError(f"resize_pil_u8: expected uint8 [n,h,w,3|4|1] or [n,h,w], got {tuple(frames.shape)}")
    code = pil_filter(resample)
    n, hi, wi, pix = x.shape
    c = 1 if pix == 1 else 3
    wo, ho = int(size[0]), int(size[1])
    y0, x0, ch, cw = (0, 0, ho, wo) if crop is None else [int(v) for v in crop]
    shape = (n, max(ch, 0), max(cw, 0)) + (() if flat else (c,))
    if out is None:
        out = torch.empty(shape, dtype=torch.uint8, device=x.device)
    else:
        check_buffer(out, "resize_pil_u8: out", torch.uint8, x.device, shape=shape, distinct=(x,))
    # the intermediate lives in the stream's workspace between the call's two launches: calls from several threads on one stream
    # must not interleave; the same lock guards the table cache
    with _pil_lock, scratch(x.device, "pil_filters", lambda *d: _size_query("adain_resize_pil_u8_bytes", *d)[0], n, hi, wi, ho, wo, pix, code, y0, x0, ch,
                            cw) as ws:
        stream = _stream()
        kx, tx = _pil_axis_tables(x.device, code, wi, wo, stream)
        ky, ty = _pil_axis_tables(x.device, code, hi, ho, stream)
        _launch("adain_resize_pil_u8", x.data_ptr(), pix, n, hi, wi, out.data_ptr(), ho, wo, code, tx.data_ptr(), tx.data_ptr() + 8 * wo, kx, ty.data_ptr(),
                ty.data_ptr() + 8 * ho, ky, y0, x0, ch, cw, ws.data_ptr(), ws.numel())
    return out


# --- output files (adain_jpeg_encode_u8) ---------------------------------------------------------------------------------------------
JPEG_DEFAULT_QUALITY = 75          # Pillow's


def _size_query(name, *dims, results=1):
    """The size query ``name`` of the C ABI on the integers ``dims`` -> its size_t results.  Host only.  AdainHipError for a refused shape."""
    out = [_c_size_t() for _ in range(results)]
    rc = _entry(name)(*(int(d) for d in dims), *(ctypes.byref(o) for o in out))
    if rc != 0:
        raise _failure(name, rc)
    return [o.value for o in out]


def _u8_frames(u8, what):
    """The input forms the file encoders share: frames uint8 [n,h,w,3|1], one frame [h,w,3|1] or [h,w] -> contiguous [n,h,w,c]."""
    x = device_tensor(u8, "frames", torch.uint8)
    if x.dim() == 2:
        x = x[None, :, :, None]
    elif x.dim() == 3:
        x = x[None]
    if x.dim() != 4 or x.shape[3] not in (1, 3) or x.shape[0] < 1:
        raise AdainHipError(f"{what}: expected uint8 [n,h,w,3|1], [h,w,3|1] or [h,w], got {tuple(u8.shape)}")
    return x


def _jpeg_frames(u8, what, quality):
    """``_u8_frames`` behind the JPEG calls' check of ``quality``."""
    if isinstance(quality, bool) or not isinstance(quality, int) or not 1 <= quality <= 100:
        raise AdainHipError(f"{what}: quality must be an int in 1..100, got {quality!r}")
    return _u8_frames(u8, what)


JPEG_SUBSAMPLING = {"4:4:4": 0, "4:2:2": 1, "4:2:0": 2}          # Pillow's strings -> its numbers, which are the C ABI's `sampling`


def jpeg_subsampling(subsampling, what="jpeg_encode_u8"):
    """Pillow's ``subsampling`` keyword as the C ABI's number: 0 / "4:4:4", 1 / "4:2:2", 2 / "4:2:0".  Anything else (-1 and "keep"
    included: they mean "whatever the source file had", and a frame has no source file) raises AdainHipError."""
    if isinstance(subsampling, str) and subsampling in JPEG_SUBSAMPLING:
        return JPEG_SUBSAMPLING[subsampling]
    if isinstance(subsampling, bool) or not isinstance(subsampling, int) or not 0 <= subsampling <= 2:
        raise AdainHipError(f"{what}: subsampling must be 0, 1, 2 or '4:4:4', '4:2:2', '4:2:0', got {subsampling!r}")
    return subsampling


def _jpeg_flag(value, what, name):
    if isinstance(value, int) and value in (0, 1):          # bool is an int
        return int(value)
    raise AdainHipError(f"{what}: {name} must be False or True, got {value!r}")


def is_jpeg_path(path):
    return str(path).lower().endswith((".jpg", ".jpeg"))


class _Value:
    """What the immutable values below share: their fields are their ``__slots__``, set once in ``__init__`` (``_set``); equality, hash
    and repr go by value; ``replace(**changes)`` gives a changed copy."""
    __slots__ = ()

    def _set(self, **fields):
        for name, value in fields.items():
            object.__setattr__(self, name, value)

    def __setattr__(self, name, value):
        raise AttributeError(f"{type(self).__name__} is immutable")

    def _key(self):
        return tuple(getattr(self, name) for name in self.__slots__)

    @classmethod
    def of(cls, value):
        """None -> the defaults; an instance -> itself; a dict of keywords -> the value."""
        if value is None:
            return cls()
        if isinstance(value, cls) or type(value).__name__ == cls.__name__:          # (a reloaded module's class is another object)
            return value
        if isinstance(value, dict):
            return cls(**value)
        raise AdainHipError(f"expected {cls.__name__}, a dict or None, got {value!r}")

    def replace(self, **changes):
        return type(self)(**{**dict(zip(self.__slots__, self._key())), **changes})

    def __eq__(self, other):
        return type(other).__name__ == type(self).__name__ and self._key() == other._key()

    def __hash__(self):
        return hash(self._key())

    def __repr__(self):
        return f"{type(self).__name__}({', '.join(f'{name}={value!r}' for name, value in zip(self.__slots__, self._key()))})"


class JpegOptions(_Value):
    """How to save a JPEG: Pillow's ``quality`` (1..100, default 75), ``subsampling`` (0 / "4:4:4", 1 / "4:2:2", 2 / "4:2:0", default
    4:2:0), ``optimize`` (the file's own optimal Huffman tables, default off) and ``progressive`` (libjpeg's simple progression, every
    scan under its own optimal table, default off; ``optimize`` has no effect with it, as in Pillow) - the keywords the device encoder
    covers.  The defaults are Pillow's default save.  One value for both routes of a caller: ``encode`` is the device's (``jpeg_encode_u8``), ``save`` the
    host's (``Image.save`` with the same keywords), and the files are the same.  An L image ignores ``subsampling`` on both routes: its
    file is the one Pillow writes without the keyword.  ``repr`` and ``save_kwargs`` name ``progressive`` only when it is set.  What
    stays with Pillow alone: ``qtables=``, ``quality="keep"``, EXIF / ICC / comments / DPI, restart markers, CMYK, arithmetic coding,
    scan scripts other than libjpeg's simple progression.  AdainHipError for a value outside these."""
    __slots__ = ("quality", "subsampling", "optimize", "progressive")

    def __init__(self, quality=JPEG_DEFAULT_QUALITY, subsampling=2, optimize=False, progressive=False):
        if isinstance(quality, bool) or not isinstance(quality, int) or not 1 <= quality <= 100:
            raise AdainHipError(f"JpegOptions: quality must be an int in 1..100, got {quality!r}")
        self._set(quality=quality, subsampling=jpeg_subsampling(subsampling, "JpegOptions"), optimize=bool(_jpeg_flag(optimize, "JpegOptions", "optimize")),
                  progressive=bool(_jpeg_flag(progressive, "JpegOptions", "progressive")))

    @classmethod
    def of(cls, value):
        """None -> the defaults; a JpegOptions -> itself; a (quality, subsampling, optimize[, progressive]) tuple or a dict of keywords -> the
        value."""
        if isinstance(value, (tuple, list)):
            return cls(*value)
        if value is None or isinstance(value, dict) or type(value).__name__ == cls.__name__:
            return super().of(value)
        raise AdainHipError(f"jpeg_options: expected JpegOptions, a (quality, subsampling, optimize[, progressive]) tuple, a dict or None, got {value!r}")

    @property
    def is_default(self):
        return self._key() == (JPEG_DEFAULT_QUALITY, 2, False, False)

    def __repr__(self):
        fields = [(name, value) for name, value in zip(self.__slots__, self._key()) if name != "progressive" or value]
        return f"JpegOptions({', '.join(f'{name}={value!r}' for name, value in fields)})"

    def save_kwargs(self, mode="RGB"):
        """The keywords of ``Image.save`` for an image of ``mode``: none at the defaults (today's call), no ``subsampling`` for L."""
        if self.is_default:
            return {}
        kw = {"quality": self.quality, "optimize": self.optimize}
        if mode != "L":
            kw["subsampling"] = self.subsampling
        if self.progressive:
            kw["progressive"] = True
        return kw

    def save(self, img, path):
        """The host route: ``img.save(path)``, with these keywords for a .jpg / .jpeg path only - other extensions never see them.
        Pillow sizes its encoder buffer for ``optimize`` or ``progressive`` at width x height bytes and fails ("broken data stream") on a frame whose file
        is larger, which a noisy 4:4:4 frame is: ImageFile.MAXBLOCK, Pillow's knob for it, is raised to the worst case first."""
        kw = self.save_kwargs(img.mode) if is_jpeg_path(path) else {}
        if kw.get("optimize") or kw.get("progressive"):
            from PIL import ImageFile

            ImageFile.MAXBLOCK = max(ImageFile.MAXBLOCK, 4 * img.size[0] * img.size[1] * len(img.getbands()) + 4096)
        img.save(str(path), **kw)

    def encode(self, u8):
        """The device route: ``jpeg_encode_u8`` with these options -> (files, lengths) on the device."""
        return jpeg_encode_u8(u8, self.quality, self.subsampling, self.optimize, self.progressive)


class JpegRoutes(_Value):
    """Which of a call's JPEG work the device does and how its files are saved - one value for every caller (``AdaIN.test``'s setters, the
    video entry points, ``jobs.FileSink``, the localized pipeline).  ``encode_on_device``: .jpg / .jpeg outputs are encoded on the device
    instead of by PIL, the same files; ``decode_on_device``: .jpg / .jpeg inputs are decoded there, the same pixels;
    ``decode_progressive``: progressive inputs too - only with ``decode_on_device``, False without it (this is the one place that says
    so); ``options``: a ``JpegOptions`` (or what ``JpegOptions.of`` takes), how an output is saved on either route.  The defaults:
    everything off, Pillow's default save."""
    __slots__ = ("encode_on_device", "decode_on_device", "decode_progressive", "options")

    def __init__(self, encode_on_device=False, decode_on_device=False, decode_progressive=False, options=None):
        self._set(encode_on_device=bool(encode_on_device), decode_on_device=bool(decode_on_device),
                  decode_progressive=bool(decode_on_device and decode_progressive), options=JpegOptions.of(options))

    def encodes(self, paths):
        """Does the device encode the file(s) at ``paths`` (one, or a list)?  With ``encode_on_device``, when every path is .jpg / .jpeg."""
        paths = paths if isinstance(paths, (list, tuple)) else [paths]
        return self.encode_on_device and len(paths) > 0 and all(is_jpeg_path(p) for p in paths)

    def write(self, u8, path, mark=None):
        """``OutputRoutes.write`` with the .png route off: the device's file of a .jpg / .jpeg frame it holds, ``options.save`` for every other."""
        OutputRoutes(jpeg=self).write(u8, path, mark)

    def read_rgb(self, path, device):
        """``jpeg_decode_rgb_file(path, device)`` with ``decode_on_device`` - the frame on the device, or None: the caller decodes with PIL."""
        return jpeg_decode_rgb_file(path, device, self.decode_progressive) if self.decode_on_device else None


def _encode_files(x, tag, sizes, launch):
    """What the file encoders share: frames [n,h,w,c] -> (files uint8 [n, stride], lengths int32 [n]) on their device.  ``sizes()`` answers
    (out_stride, workspace_bytes), one query for both; ``launch(out, stride, lengths, ws)`` runs the encoder on the ``tag`` workspace."""
    n, stride = x.shape[0], 0

    def workspace_bytes():
        nonlocal stride
        stride, nbytes = sizes()
        return nbytes

    with scratch(x.device, tag, workspace_bytes) as ws:
        out = torch.empty((n, stride), dtype=torch.uint8, device=x.device)
        lengths = torch.empty((n,), dtype=torch.int32, device=x.device)
        launch(out, stride, lengths, ws)
    return out, lengths


def jpeg_encode_sizes(n, h, w, c, subsampling=2, optimize=False, progressive=False):
    """(out_stride, workspace_bytes) of adain_jpeg_encode_opt_u8_bytes (at the defaults: adain_jpeg_encode_u8_bytes' values; with
    ``progressive``: adain_jpeg_encode_progressive_u8_bytes', whatever ``optimize``): the largest file a frame of this shape can have
    and the scratch of an n-frame call.  Host only.  AdainHipError for a refused shape."""
    sampling, optimize = jpeg_subsampling(subsampling, "jpeg_encode_sizes"), _jpeg_flag(optimize, "jpeg_encode_sizes", "optimize")
    if _jpeg_flag(progressive, "jpeg_encode_sizes", "progressive"):
        return tuple(_size_query("adain_jpeg_encode_progressive_u8_bytes", n, h, w, c, sampling, results=2))
    return tuple(_size_query("adain_jpeg_encode_opt_u8_bytes", n, h, w, c, sampling, optimize, results=2))


def jpeg_encode_u8(u8, quality=JPEG_DEFAULT_QUALITY, subsampling=2, optimize=False, progressive=False):
    """Frames uint8 [n,h,w,c] (c = 3: RGB, 1: L; or one frame [h,w,c] / [h,w]) -> (files uint8 [n, stride], lengths int32 [n]), both on the
    device: row i starts with frame i's JPEG file, ``lengths[i]`` bytes, byte for byte what ``PIL.Image.fromarray(frame).save(f,
    format="JPEG", quality=quality, subsampling=subsampling, optimize=optimize)`` writes; the rest of the row is not written.
    ``subsampling``: 0 / "4:4:4", 1 / "4:2:2", 2 / "4:2:0" (the default, Pillow's own); L frames ignore it and get the file Pillow writes
    without the keyword.  ``optimize``: the frame's own optimal Huffman tables.  The defaults give Pillow's default file
    (adain_jpeg_encode_u8).  ``progressive``: the file of ``save(..., progressive=True)`` (adain_jpeg_encode_progressive_u8), on which
    ``optimize`` has no effect, as in Pillow.  Nothing is copied to the host and nothing waits."""
    sampling, optimize = jpeg_subsampling(subsampling), _jpeg_flag(optimize, "jpeg_encode_u8", "optimize")
    progressive = _jpeg_flag(progressive, "jpeg_encode_u8", "progressive")
    x = _jpeg_frames(u8, "jpeg_encode_u8", quality)
    n, h, w, c = x.shape

    def launch(out, stride, lengths, ws):
        tail = (out.data_ptr(), stride, lengths.data_ptr(), ws.data_ptr(), ws.numel())
        if progressive:
            _launch("adain_jpeg_encode_progressive_u8", x.data_ptr(), n, h, w, c, quality, sampling, *tail)
        elif (sampling, optimize) == (2, 0):
            _launch("adain_jpeg_encode_u8", x.data_ptr(), n, h, w, c, quality, *tail)
        else:
            _launch("adain_jpeg_encode_opt_u8", x.data_ptr(), n, h, w, c, quality, sampling, optimize, *tail)

    return _encode_files(x, "jpeg", lambda: jpeg_encode_sizes(n, h, w, c, sampling, optimize, progressive), launch)


def jpeg_files(out, lengths):
    """The files of a ``jpeg_encode_u8`` result as a list of ``bytes``: the lengths first, then exactly that many bytes per frame (waits for
    the device)."""
    ln = lengths.cpu().tolist()
    return [out[i, :k].cpu().numpy().tobytes() for i, k in enumerate(ln)]


# --- .png output files (adain_png_encode_u8) ------------------------------------------------------------------------------------------
def is_png_path(path):
    return str(path).lower().endswith(".png")


def _png_filter(filter, what):
    """None (every row's filter by libpng's minimum sum of magnitudes) -> -1; 0..4 (None, Sub, Up, Average, Paeth on every row) -> itself."""
    if filter is None:
        return -1
    if isinstance(filter, bool) or not isinstance(filter, int) or not 0 <= filter <= 4:
        raise AdainHipError(f"{what}: filter must be None or an int in 0..4, got {filter!r}")
    return filter


def png_encode_sizes(n, h, w, c):
    """(out_stride, workspace_bytes) of adain_png_encode_u8_bytes: the largest file a frame of this shape can have and the scratch of an
    n-frame call.  Host only.  AdainHipError for a refused shape."""
    return tuple(_size_query("adain_png_encode_u8_bytes", n, h, w, c, results=2))


def png_encode_u8(u8, filter=None):
    """Frames uint8 [n,h,w,c] (c = 3: RGB, 1: L; or one frame [h,w,c] / [h,w]) -> (files uint8 [n, stride], lengths int32 [n]), both on the
    device: row i starts with frame i's PNG file, ``lengths[i]`` bytes - 8-bit, non-interlaced, IHDR / IDAT / IEND - which any reader
    decodes to the frame's pixels; the rest of the row is not written.  The bytes are not Pillow's: they follow the rules of
    csrc/png.hip (tests/png_ref.py) and depend on the frame and ``filter`` alone.  ``filter``: None chooses every row's filter as libpng
    does, 0..4 forces one.  16-bit, palette, RGBA, interlace, ancillary chunks, ``compress_level`` and ``optimize`` stay with Pillow.
    Nothing is copied to the host and nothing waits."""
    filt = _png_filter(filter, "png_encode_u8")
    x = _u8_frames(u8, "png_encode_u8")
    n, h, w, c = x.shape

    def launch(out, stride, lengths, ws):
        _launch("adain_png_encode_u8", x.data_ptr(), n, h, w, c, filt, out.data_ptr(), stride, lengths.data_ptr(), ws.data_ptr(), ws.numel())

    return _encode_files(x, "png", lambda: png_encode_sizes(n, h, w, c), launch)


png_files = jpeg_files          # the files of a ``png_encode_u8`` result as a list of ``bytes`` (waits for the device)


# --- palette control (adain_palette_map_u8, adain_tone_u8, adain_palette_dither_u8) --------------------------------------------------------
PALETTE_DITHER_BAND = 1024          # ADAIN_PALETTE_DITHER_BAND: the rows one workgroup of adain_palette_dither_u8 holds at once
PALETTE_METRICS = {"rgb": 0, "nearest": 1}          # ADAIN_PALETTE_METRIC_*


def _rgb_frames(u8, what):
    """uint8 [n,h,w,3] or one frame [h,w,3] on the device -> contiguous [n,h,w,3]."""
    x = device_tensor(u8, what + ": frames", torch.uint8)
    if x.dim() == 3:
        x = x[None]
    if x.dim() != 4 or x.shape[3] != 3 or x.numel() == 0:
        raise AdainHipError(f"{what}: expected uint8 [n,h,w,3] or [h,w,3], got {tuple(u8.shape)}")
    return x


def palette_tensor(palette, device, what="palette"):
    """A palette - a uint8 tensor [K,3] or a sequence of K RGB triples, 1 <= K <= 256 - as a contiguous uint8 [K,3] on ``device``."""
    if isinstance(palette, torch.Tensor):
        if palette.dtype != torch.uint8:
            raise AdainHipError(f"{what}: a palette tensor must be uint8, got {palette.dtype}")
        p = palette
    else:
        rows = [[int(v) for v in c] for c in palette]
        if any(len(c) != 3 or min(c) < 0 or max(c) > 255 for c in rows):
            raise AdainHipError(f"{what}: expected RGB triples of 0..255")
        p = torch.tensor(rows, dtype=torch.uint8).reshape(-1, 3)
    if p.dim() != 2 or p.shape[1] != 3 or not 1 <= p.shape[0] <= 256:
        raise AdainHipError(f"{what}: expected [K,3] with 1 <= K <= 256, got {tuple(p.shape)}")
    return p.to(device).contiguous()


def _tone_args(lut, grey, device, what):
    """(lut tensor or None, its pointer or None, grey as int).  ``lut``: None, or uint8 [256] (one table for the three channels) or [3,256]."""
    if lut is None:
        return None, None, int(bool(grey))
    t = lut if isinstance(lut, torch.Tensor) else torch.as_tensor(lut)
    if t.dtype != torch.uint8 or tuple(t.shape) not in ((256,), (3, 256)):
        raise AdainHipError(f"{what}: lut must be uint8 [256] or [3,256], got {t.dtype} {tuple(t.shape)}")
    t = t.expand(3, 256).to(device).contiguous()
    return t, t.data_ptr(), int(bool(grey))


def _index_plane(x, index):
    return torch.empty(x.shape[:3], dtype=torch.uint8, device=x.device) if index else None


def palette_map_u8(u8, palette, metric="nearest", lut=None, grey=False, index=False):
    """Frames uint8 [n,h,w,3] (or [h,w,3]) on the device -> every pixel replaced by its palette entry (adain_palette_map_u8), in the
    input's shape; with ``index`` a pair (frames, uint8 [n,h,w] or [h,w] of the chosen entries).  ``metric``: "rgb", the reference's
    ``_recolor_image`` with its uint8 differences that wrap modulo 256, or "nearest", the true nearest colour (``_recolor_image_kd``);
    the lowest index wins a tie.  ``grey`` / ``lut``: the tone step in front (``tone_u8``).  Nothing is copied to the host and nothing waits."""
    what = "palette_map_u8"
    if metric not in PALETTE_METRICS:
        raise AdainHipError(f"{what}: metric must be one of {sorted(PALETTE_METRICS)}, got {metric!r}")
    x = _rgb_frames(u8, what)
    n, h, w, _ = x.shape
    pal = palette_tensor(palette, x.device, what + ": palette")
    keep, lut_ptr, grey = _tone_args(lut, grey, x.device, what)
    out, idx = torch.empty_like(x), _index_plane(x, index)
    call("adain_palette_map_u8", x.device, x.data_ptr(), n, h, w, pal.data_ptr(), pal.shape[0], PALETTE_METRICS[metric], lut_ptr, grey, out.data_ptr(),
         idx.data_ptr() if index else None)
    out = out.reshape(u8.shape)
    return (out, idx.reshape(u8.shape[:-1])) if index else out


def tone_u8(u8, lut=None, grey=False, out=None):
    """Frames uint8 [n,h,w,3] (or [h,w,3]) -> the tone step alone (adain_tone_u8): ``grey``, Pillow's ``convert("L").convert("RGB")``,
    then ``lut`` (uint8 [256] or [3,256]: channel c becomes lut[c][value]).  ``out``: the frames themselves for in place, or None."""
    what = "tone_u8"
    x = _rgb_frames(u8, what)
    n, h, w, _ = x.shape
    keep, lut_ptr, grey = _tone_args(lut, grey, x.device, what)
    if out is None:
        res = torch.empty_like(x)
    else:
        res = check_buffer(out, "tone_u8: out", torch.uint8, x.device, numel=x.numel())
    call("adain_tone_u8", x.device, x.data_ptr(), n, h, w, lut_ptr, grey, res.data_ptr())
    return res.reshape(u8.shape)


def palette_dither_sizes(n, h, w):
    """workspace_bytes of adain_palette_dither_u8_bytes.  Host only.  AdainHipError for a refused shape."""
    return _size_query("adain_palette_dither_u8_bytes", n, h, w)[0]


def palette_dither_u8(u8, palette, lut=None, grey=False, index=False):
    """Frames uint8 [n,h,w,3] (or [h,w,3]) on the device -> Floyd-Steinberg error diffusion onto the palette (adain_palette_dither_u8): the
    loop the reference's ``_recolor_image_floyd`` spells out, float32, bit for bit tests/palette_ref.py's sequential form.  Returns as
    ``palette_map_u8`` does.  Nothing is copied to the host and nothing waits."""
    what = "palette_dither_u8"
    x = _rgb_frames(u8, what)
    n, h, w, _ = x.shape
    pal = palette_tensor(palette, x.device, what + ": palette")
    keep, lut_ptr, grey = _tone_args(lut, grey, x.device, what)
    out, idx = torch.empty_like(x), _index_plane(x, index)
    with scratch(x.device, "palette", palette_dither_sizes, n, h, w) as ws:
        _launch("adain_palette_dither_u8", x.data_ptr(), n, h, w, pal.data_ptr(), pal.shape[0], lut_ptr, grey, out.data_ptr(), idx.data_ptr() if index else None,
                ws.data_ptr(), ws.numel())
    out = out.reshape(u8.shape)
    return (out, idx.reshape(u8.shape[:-1])) if index else out


# --- animated GIF frame records (adain_gif_encode_u8) -----------------------------------------------------------------------------------
GIF_SEGMENT = 2048          # ADAIN_GIF_SEGMENT: the pixels coded from one CLEAR to the next


def gif_encode_sizes(n, h, w, K):
    """(out_stride, workspace_bytes) of adain_gif_encode_u8_bytes: the largest record a frame of this shape and palette size can have and
    the scratch of an n-frame call.  Host only.  AdainHipError for a refused shape."""
    return tuple(_size_query("adain_gif_encode_u8_bytes", n, h, w, K, results=2))


def gif_encode_u8(index, K, delay_cs):
    """Palette index planes uint8 [n,h,w] (or one, [h,w]) on the device, every index below ``K`` -> (records uint8 [n, stride], lengths
    int32 [n]), both on the device: row i starts with frame i's GIF record - graphic control extension with ``delay_cs`` centiseconds,
    image descriptor, LZW data - ``lengths[i]`` bytes; the rest of the row is not written.  ``gif_file.assemble`` makes the file.  The
    bytes follow the rules of csrc/gif.hip (tests/gif_ref.py), not Pillow's, and depend on the indices, ``K`` and ``delay_cs`` alone.
    A frame with an index >= K has length 0 (``gif_file.assemble`` raises).  Nothing is copied to the host and nothing waits."""
    what = "gif_encode_u8"
    for name, v, lo, hi in (("K", K, 1, 256), ("delay_cs", delay_cs, 0, 65535)):
        if isinstance(v, bool) or not isinstance(v, int) or not lo <= v <= hi:
            raise AdainHipError(f"{what}: {name} must be an int in {lo}..{hi}, got {v!r}")
    x = device_tensor(index, what + ": index", torch.uint8)
    if x.dim() == 2:
        x = x[None]
    if x.dim() != 3 or x.numel() == 0:
        raise AdainHipError(f"{what}: expected uint8 [n,h,w] or [h,w], got {tuple(index.shape)}")
    n, h, w = x.shape

    def launch(out, stride, lengths, ws):
        _launch("adain_gif_encode_u8", x.data_ptr(), n, h, w, K, delay_cs, out.data_ptr(), stride, lengths.data_ptr(), ws.data_ptr(), ws.numel())

    return _encode_files(x, "gif", lambda: gif_encode_sizes(n, h, w, K), launch)


# --- a palette chosen from the frames (adain_quantize_palette_u8) -------------------------------------------------------------------------
QUANTIZE_GLOBAL, QUANTIZE_PER_FRAME = 0, 1          # ADAIN_QUANTIZE_*
QUANTIZE_REFINE_MAX = 64                            # ADAIN_QUANTIZE_REFINE_MAX


def quantize_mode(per_frame=False, refine=0):
    """The call's ``mode``: ADAIN_QUANTIZE_GLOBAL or _PER_FRAME, or-ed with ADAIN_QUANTIZE_REFINE(refine).  ValueError for a ``refine``
    that is not an int in 0..64."""
    if isinstance(refine, bool) or not isinstance(refine, int) or not 0 <= refine <= QUANTIZE_REFINE_MAX:
        raise ValueError(f"quantize_palette_u8: refine must be an int in 0..{QUANTIZE_REFINE_MAX}, got {refine!r}")
    return (QUANTIZE_PER_FRAME if per_frame else QUANTIZE_GLOBAL) | refine << 8


def quantize_palette_sizes(n, h, w, per_frame=False, refine=0):
    """workspace_bytes of adain_quantize_palette_u8_bytes.  Host only.  AdainHipError for a refused shape."""
    return _size_query("adain_quantize_palette_u8_bytes", n, h, w, quantize_mode(per_frame, refine))[0]


def quantize_palette_u8(frames, K=256, per_frame=False, refine=0):
    """Frames uint8 [n,h,w,3] (or [h,w,3]) on the device -> (palettes uint8 [P,256,3], used int32 [P]), both on the device: at most ``K``
    colours chosen from the frames themselves, one palette for all of them (P = 1) or with ``per_frame`` one each (P = n).  Palette p's
    colours are its first ``used[p]`` entries, the rest is zero.  A median cut over 32 x 32 x 32 cells by the rules of csrc/quantize.hip
    (tests/quantize_ref.py), not Pillow's palette; a function of the pixels, ``K`` and ``per_frame`` alone.  ``refine`` = T in 1..64: T
    rounds of k-means behind the cut, in integers (rules 7-11, csrc/quantize_refine.hip, tests/quantize_refine_ref.py): the entries move
    to their pixels' centres and the unused ones take the farthest colours, so a frame with fewer than ``K`` non-empty cells still gets
    ``K`` colours where it has them; ValueError outside 0..64.  ``palette_map_u8`` /
    ``palette_dither_u8`` take ``palettes[p, :used[p]]``.  (``quantize_u8`` is the float -> uint8 quantiser of ``save_image``.)  Nothing is
    copied to the host and nothing waits."""
    what = "quantize_palette_u8"
    if isinstance(K, bool) or not isinstance(K, int) or not 1 <= K <= 256:
        raise AdainHipError(f"{what}: K must be an int in 1..256, got {K!r}")
    mode = quantize_mode(per_frame, refine)
    x = _rgb_frames(frames, what)
    n, h, w, _ = x.shape
    P = n if per_frame else 1
    palettes = torch.empty((P, 256, 3), dtype=torch.uint8, device=x.device)
    used = torch.empty((P,), dtype=torch.int32, device=x.device)
    with scratch(x.device, "quantize", quantize_palette_sizes, n, h, w, bool(per_frame), refine) as ws:
        _launch("adain_quantize_palette_u8", x.data_ptr(), n, h, w, K, mode, palettes.data_ptr(), used.data_ptr(), ws.data_ptr(), ws.numel())
    return palettes, used


# --- image quality metrics (adain_image_metrics_u8 / adain_image_metrics_f32) ---------------------------------------------------------------
METRICS_TILE = (16, 64)          # ADAIN_METRICS_TILE_Y, ADAIN_METRICS_TILE_X: rows x samples a workgroup takes


class ImageMetrics:
    """What ``image_metrics`` returns: ``ssim``, ``mse``, ``l1`` and ``psnr`` as float64 [n] device tensors (views of ``records``, the
    call's float64 [n,4]) and ``ssim_map``, float32 of the inputs' shape, or None when it was not asked for."""
    __slots__ = ("records", "ssim_map")

    def __init__(self, records, ssim_map=None):
        self.records, self.ssim_map = records, ssim_map

    ssim = property(lambda self: self.records[:, 0])
    mse = property(lambda self: self.records[:, 1])
    l1 = property(lambda self: self.records[:, 2])
    psnr = property(lambda self: self.records[:, 3])


def image_metrics_sizes(n, h, w, c, u8=True):
    """workspace_bytes of adain_image_metrics_u8_bytes (``u8``) or adain_image_metrics_f32_bytes.  Host only.  AdainHipError for a
    refused shape."""
    return _size_query("adain_image_metrics_u8_bytes", n, h, w, c)[0] if u8 else _size_query("adain_image_metrics_f32_bytes", n, c, h, w)[0]


def image_metrics(a, b, ssim_map=False):
    """Two clips on the device -> their per-frame scores, an ``ImageMetrics``: the reference's ``ssim`` (window 11), ``mse``, ``l1`` and
    ``psnr`` (Style_3DGS utils/loss_utils.py, utils/image_utils.py) as float64 [n] device tensors, and with ``ssim_map`` the per-element
    map.  uint8 [n,h,w,c] or [h,w,c] with c = 1 or 3 takes adain_image_metrics_u8 (scaled as ``to_tensor`` does, x / 255); float32
    [n,c,h,w] or [c,h,w] with c in 1..4 takes adain_image_metrics_f32, values as given.  Equal frames score ssim 1, mse 0, l1 0 and
    psnr +inf exactly; the uint8 mse and l1 are exact.  Nothing is copied to the host and nothing waits."""
    what = "image_metrics"
    if not isinstance(a, torch.Tensor) or not isinstance(b, torch.Tensor) or a.dtype not in (torch.uint8, torch.float32):
        raise AdainHipError(f"{what}: expected two uint8 or two float32 GPU tensors")
    u8 = a.dtype == torch.uint8
    x, y = device_tensor(a, what + ": a", a.dtype), device_tensor(b, what + ": b", a.dtype)
    if x.shape != y.shape or x.device != y.device:
        raise AdainHipError(f"{what}: a and b must have one shape and one device, got {tuple(a.shape)} and {tuple(b.shape)}")
    if x.dim() == 3:
        x, y = x[None], y[None]
    if x.dim() != 4 or x.numel() == 0 or (x.shape[3] not in (1, 3) if u8 else not 1 <= x.shape[1] <= 4):
        raise AdainHipError(f"{what}: expected uint8 [n,h,w,1|3] / [h,w,1|3] or float32 [n,1..4,h,w] / [c,h,w], got {tuple(a.shape)}")
    n = x.shape[0]
    (h, w, c) = x.shape[1:] if u8 else (x.shape[2], x.shape[3], x.shape[1])
    records = torch.empty((n, 4), dtype=torch.float64, device=x.device)
    smap = torch.empty(x.shape, dtype=torch.float32, device=x.device) if ssim_map else None
    with scratch(x.device, "metrics", image_metrics_sizes, n, h, w, c, u8) as ws:
        dims = (n, h, w, c) if u8 else (n, c, h, w)
        _launch("adain_image_metrics_u8" if u8 else "adain_image_metrics_f32", x.data_ptr(), y.data_ptr(), *dims, records.data_ptr(),
                smap.data_ptr() if ssim_map else None, ws.data_ptr(), ws.numel())
    return ImageMetrics(records, smap.reshape(a.shape) if ssim_map else None)


def image_metrics_grad_sizes(n, c, h, w, grad_b=False):
    """workspace_bytes of adain_image_metrics_grad_f32_bytes: 3 planes of the clip's floats, 5 with ``grad_b``, each rounded up to 256
    bytes.  Host only.  AdainHipError for a refused shape."""
    return _size_query("adain_image_metrics_grad_f32_bytes", n, c, h, w, 1 if grad_b else 0)[0]


def image_metrics_grad(a, b, weights, grad_b=False):
    """The gradient of ``image_metrics``' float32 scores: ``a``, ``b`` float32 [n,c,h,w] or [c,h,w] with c in 1..4 on the device and
    ``weights`` float64 [n,3] (or [3] for one frame) there, row i the upstream gradient of frame i's {ssim, mse, l1} -> ``grad_a``,
    float32 of ``a``'s shape: weights[i,0] d ssim_i / d a + weights[i,1] 2 (a - b) / count + weights[i,2] sign(a - b) / count; with
    ``grad_b`` (grad_a, grad_b) (adain_image_metrics_grad_f32).  The window statistics are recomputed from ``a`` and ``b``; a frame's
    gradient is a function of its two frames and its three weights alone.  Nothing is copied to the host and nothing waits."""
    what = "image_metrics_grad"
    x, y = device_tensor(a, what + ": a"), device_tensor(b, what + ": b")
    if x.shape != y.shape or x.device != y.device:
        raise AdainHipError(f"{what}: a and b must have one shape and one device, got {tuple(a.shape)} and {tuple(b.shape)}")
    if x.dim() == 3:
        x, y = x[None], y[None]
    if x.dim() != 4 or x.numel() == 0 or not 1 <= x.shape[1] <= 4:
        raise AdainHipError(f"{what}: expected float32 [n,1..4,h,w] / [c,h,w], got {tuple(a.shape)}")
    n, c, h, w = x.shape
    wts = device_tensor(weights, what + ": weights", torch.float64)
    if wts.device != x.device or wts.numel() != 3 * n or tuple(wts.shape) not in ((n, 3), (3,)):
        raise AdainHipError(f"{what}: weights must be float64 [{n},3] on {x.device}, got {tuple(weights.shape)} on {weights.device}")
    ga = torch.empty(x.shape, dtype=torch.float32, device=x.device)
    gb = torch.empty(x.shape, dtype=torch.float32, device=x.device) if grad_b else None
    with scratch(x.device, "metrics_grad", image_metrics_grad_sizes, n, c, h, w, bool(grad_b)) as ws:
        _launch("adain_image_metrics_grad_f32", x.data_ptr(), y.data_ptr(), n, c, h, w, wts.data_ptr(), ga.data_ptr(), gb.data_ptr() if grad_b else None,
                ws.data_ptr(), ws.numel())
    return (ga.reshape(a.shape), gb.reshape(a.shape)) if grad_b else ga.reshape(a.shape)


def ssim_window():
    """The eleven float32 weights of the SSIM kernel (adain_ssim_window): the reference's ``gaussian(11, 1.5)``.  Host only."""
    out = (_c_float * 11)()
    rc = lib().adain_ssim_window(out)
    if rc != 0:
        raise _failure("adain_ssim_window", rc)
    return list(out)


# --- the guide-view loss (adain_guide_l1_f32 / adain_guide_l1_grad_f32) -----------------------------------------------------------------------
class GuideL1:
    """What ``guide_l1`` returns: ``l1``, float64 [n] on the device (train.py's ``Ll1`` per frame), and ``resampled``, the guide at the
    render's size as float32 of the image's shape, or None when it was not asked for."""
    __slots__ = ("l1", "resampled")

    def __init__(self, l1, resampled=None):
        self.l1, self.resampled = l1, resampled


def guide_l1_sizes(n, h, w):
    """workspace_bytes of adain_guide_l1_f32_bytes: a float64 per workgroup of the n frames.  Host only.  AdainHipError for a refused
    shape."""
    return _size_query("adain_guide_l1_f32_bytes", n, h, w)[0]


def _guide_pair(image, guide, what):
    """The input forms of the guide calls: ``image`` float32 [n,3,h,w] or [3,h,w], ``guide`` uint8 [n,gh,gw,3] or [gh,gw,3] on the same
    device -> both contiguous with the batch dimension."""
    x, g = device_tensor(image, what + ": image"), device_tensor(guide, what + ": guide", torch.uint8)
    if x.dim() == 3:
        x = x[None]
    if g.dim() == 3:
        g = g[None]
    if x.dim() != 4 or g.dim() != 4 or x.shape[1] != 3 or g.shape[3] != 3 or x.numel() == 0 or g.numel() == 0 or x.shape[0] != g.shape[0] or x.device != g.device:
        raise AdainHipError(f"{what}: expected float32 [n,3,h,w] / [3,h,w] and uint8 [n,gh,gw,3] / [gh,gw,3] on one device, got {tuple(image.shape)} "
                            f"on {image.device} and {tuple(guide.shape)} on {guide.device}")
    return x, g


def guide_l1(image, guide, resampled=False):
    """A render float32 [n,3,h,w] (or [3,h,w]) and its guide views uint8 [n,gh,gw,3] (or [gh,gw,3]) on the device -> a ``GuideL1``: per
    frame ``l1_loss(image, F.interpolate(to_tensor(guide), size=(h, w), mode="bilinear", align_corners=False))`` of Style_3DGS/train.py as
    float64 [n], and with ``resampled`` the interpolated guide (adain_guide_l1_f32).  No float guide is written otherwise.  Nothing is
    copied to the host and nothing waits."""
    x, g = _guide_pair(image, guide, "guide_l1")
    n, _, h, w = x.shape
    out = torch.empty((n,), dtype=torch.float64, device=x.device)
    res = torch.empty(x.shape, dtype=torch.float32, device=x.device) if resampled else None
    with scratch(x.device, "guide_l1", guide_l1_sizes, n, h, w) as ws:
        _launch("adain_guide_l1_f32", x.data_ptr(), g.data_ptr(), n, h, w, g.shape[1], g.shape[2], out.data_ptr(), res.data_ptr() if resampled else None,
                ws.data_ptr(), ws.numel())
    return GuideL1(out, res.reshape(image.shape) if resampled else None)


def guide_l1_grad(image, guide, weights):
    """The gradient of ``guide_l1`` by the render: ``weights`` float64 [n] on the device, the upstream gradient of every frame's l1 ->
    float32 of ``image``'s shape, weights[i] / (3 h w) * sign(image - guide at the render's size), sign(0) = 0
    (adain_guide_l1_grad_f32).  The guide is resampled again; nothing of a forward call is taken.  Nothing is copied to the host and
    nothing waits."""
    what = "guide_l1_grad"
    x, g = _guide_pair(image, guide, what)
    n, _, h, w = x.shape
    wts = device_tensor(weights, what + ": weights", torch.float64)
    if wts.device != x.device or wts.numel() != n or wts.dim() > 1:
        raise AdainHipError(f"{what}: weights must be float64 [{n}] on {x.device}, got {tuple(weights.shape)} on {weights.device}")
    grad = torch.empty(x.shape, dtype=torch.float32, device=x.device)
    call("adain_guide_l1_grad_f32", x.device, x.data_ptr(), g.data_ptr(), n, h, w, g.shape[1], g.shape[2], wts.data_ptr(), grad.data_ptr())
    return grad.reshape(image.shape)


class PngRoute(_Value):
    """Which of a call's .png work the device does - the ``png`` of its ``OutputRoutes``.  ``encode_on_device``: ``png_encode_u8`` writes
    the .png outputs (the same pixels, not Pillow's bytes) and only the files cross to the host; ``filter``: its row filter, None for the
    adaptive choice; ``decode_on_device``: .png inputs are decoded on the device (``png_decode_u8``), the same pixels.  The default:
    everything off, Pillow's save and open.  ``repr`` names ``decode_on_device`` only when it is set."""
    __slots__ = ("encode_on_device", "filter", "decode_on_device")

    def __init__(self, encode_on_device=False, filter=None, decode_on_device=False):
        _png_filter(filter, "PngRoute")
        self._set(encode_on_device=bool(encode_on_device), filter=filter, decode_on_device=bool(decode_on_device))

    def __repr__(self):
        shown = [name for name in self.__slots__ if name != "decode_on_device" or self.decode_on_device]
        return f"PngRoute({', '.join(f'{name}={getattr(self, name)!r}' for name in shown)})"

    def read_rgb(self, path, device):
        """``png_decode_rgb_file(path, device)`` with ``decode_on_device`` - the frame on the device, or None: the caller decodes with PIL."""
        return png_decode_rgb_file(path, device) if self.decode_on_device else None

    def encodes(self, paths):
        """Does the device encode the file(s) at ``paths`` (one, or a list)?  With ``encode_on_device``, when every path is .png."""
        paths = paths if isinstance(paths, (list, tuple)) else [paths]
        return self.encode_on_device and len(paths) > 0 and all(is_png_path(p) for p in paths)

    def encode(self, u8):
        """The device route: ``png_encode_u8`` with this filter -> (files, lengths) on the device."""
        return png_encode_u8(u8, self.filter)


class OutputRoutes(_Value):
    """Who writes a call's output files - one value for every caller: ``jpeg``, a ``JpegRoutes``, and ``png``, a ``PngRoute``, each given as
    what its own ``of`` takes (None: everything off, Pillow's default save).  ``encoder`` alone decides between the device and Pillow."""
    __slots__ = ("jpeg", "png")

    def __init__(self, jpeg=None, png=None):
        self._set(jpeg=JpegRoutes.of(jpeg), png=PngRoute.of(png))

    def encoder(self, u8, paths):
        """The device encoder of the frames ``u8`` for the file(s) at ``paths`` (one, or a list), a callable u8 -> (files, lengths), or None:
        Pillow saves them.  The device takes a uint8 GPU tensor [n,h,w,c] or [h,w,c] with c = 1 or 3 whose paths are all .jpg / .jpeg with
        ``jpeg.encode_on_device`` or all .png with ``png.encode_on_device``; no host frame, RGBA, float, mixed or empty list, other extension."""
        if not (isinstance(u8, torch.Tensor) and u8.is_cuda and u8.dtype == torch.uint8 and u8.dim() in (3, 4) and u8.shape[-1] in (1, 3)):
            return None
        if self.jpeg.encodes(paths):
            return self.jpeg.options.encode
        return self.png.encode if self.png.encodes(paths) else None

    def read_rgb(self, path, device):
        """The file at ``path`` as ``np.asarray(Image.open(path).convert("RGB"))`` on ``device``, decoded there by the route that owns its
        extension (``png`` for .png, ``jpeg`` for everything else, which answers for .jpg / .jpeg) - or None: the caller decodes with PIL."""
        return self.png.read_rgb(path, device) if is_png_path(path) else self.jpeg.read_rgb(path, device)

    def decoder(self, path):
        """(the ``InputFormat`` that owns the extension of ``path``, the options its file routes parse with) when that format's
        ``decode_on_device`` is set - or None: PIL opens the file."""
        if self.png.decode_on_device and is_png_path(path):
            return PNG_INPUT, {}
        if self.jpeg.decode_on_device and is_jpeg_path(path):
            return JPEG_INPUT, {"restart": True, "progressive": self.jpeg.decode_progressive}
        return None

    def save(self, arr, path):
        """The host route: a numpy frame [h,w,c] (c = 1: mode L) -> the file ``jpeg.options.save`` writes (its keywords: .jpg / .jpeg only)."""
        from PIL import Image

        self.jpeg.options.save(Image.fromarray(arr[:, :, 0] if arr.shape[2] == 1 else arr), path)

    def write(self, u8, path, mark=None):
        """One uint8 frame [1,h,w,c] or [h,w,c] -> the file at ``path``: encoded where it is by ``encoder(u8, path)``, only the file coming over;
        without one downloaded (a numpy frame is taken as it is) and saved by ``save``.  ``mark()`` is called after each of the three steps:
        the launch, the wait for the device with the download, the write."""
        mark = mark or (lambda: None)
        encode = self.encoder(u8, path)
        if encode is not None:
            encoded = encode(u8)
            mark()
            data, = jpeg_files(*encoded)
            mark()
            with open(str(path), "wb") as f:
                f.write(data)
        else:
            mark()
            arr = u8.cpu().numpy() if isinstance(u8, torch.Tensor) else u8
            mark()
            self.save(arr[0] if arr.ndim == 4 else arr, path)
        mark()


def jpeg_roundtrip_sizes(n, h, w, c):
    """workspace_bytes of adain_jpeg_roundtrip_u8_bytes: the scratch of an n-frame call.  Host only.  AdainHipError for a refused shape."""
    return _size_query("adain_jpeg_roundtrip_u8_bytes", n, h, w, c)[0]


def jpeg_roundtrip_u8(u8, quality=JPEG_DEFAULT_QUALITY):
    """Frames uint8 [n,h,w,c] (c = 3: RGB, 1: L; or one frame [h,w,c] / [h,w]) -> a device tensor of the input's shape: per frame the
    pixels ``Image.open`` decodes (mode RGB / L) from the file ``PIL.Image.fromarray(frame).save(f, format="JPEG", quality=quality)``
    writes, byte for byte, computed on the device without the file (adain_jpeg_roundtrip_u8).  Nothing is copied to the host and
    nothing waits."""
    x = _jpeg_frames(u8, "jpeg_roundtrip_u8", quality)
    n, h, w, c = x.shape
    with scratch(x.device, "jpeg", jpeg_roundtrip_sizes, n, h, w, c) as ws:
        out = torch.empty_like(x)
        _launch("adain_jpeg_roundtrip_u8", x.data_ptr(), n, h, w, c, quality, out.data_ptr(), ws.data_ptr(), ws.numel())
    return out.reshape(u8.shape)


# --- input files: the doors to the C calls, the two formats, the one path over them, the public functions --------------------------------
# baseline .jpg / .jpeg (adain_jpeg_decode_restart_u8; at restart interval 0 that is adain_jpeg_decode_u8)
def jpeg_decode_sizes(n, h, w, c, sampling, max_segment_bytes, chunk_bits=0, restart_interval=0):
    """workspace_bytes of adain_jpeg_decode_restart_u8_bytes: the scratch of an n-file call whose longest entropy-coded segment has
    ``max_segment_bytes`` and whose files have ``restart_interval`` MCUs per restart interval (0: none).  Host only.  AdainHipError for
    a refused shape."""
    return _size_query("adain_jpeg_decode_restart_u8_bytes", n, h, w, c, sampling, restart_interval, max_segment_bytes, chunk_bits)[0]


_jpeg_decode_lock = threading.Lock()


def _jpeg_upload(streams, device, lead):
    """``streams``: per entropy-coded segment what describes it (``blob``, ``seg_offset``, ``seg_length``: a baseline file, or one scan of
    a progressive one) and the bytes of its file -> (device uint8 tensor: the blobs, ``lead`` spare bytes, the segments back to back;
    segment offsets behind the blobs; segment lengths)."""
    device = torch.device(device)
    if device.type != "cuda":
        raise AdainHipError("jpeg_decode_u8: expected a GPU device (the device decoder has no CPU form)")
    blobs = len(streams) * jpeg_file.BLOB_BYTES
    lengths = [s.seg_length for s, _ in streams]
    offsets, at = [], lead
    for ln in lengths:
        offsets.append(at)
        at += ln
    host = bytearray(blobs + at + 1)            # one spare byte: the pointer behind the blobs stays inside the tensor
    for i, (s, d) in enumerate(streams):
        host[i * jpeg_file.BLOB_BYTES:(i + 1) * jpeg_file.BLOB_BYTES] = s.blob
        host[blobs + offsets[i]:blobs + offsets[i] + lengths[i]] = d[s.seg_offset:s.seg_offset + s.seg_length]
    return torch.frombuffer(host, dtype=torch.uint8).to(device), offsets, lengths


def jpeg_decode_upload(parsed, datas, device, lead=0):
    """The one upload of a ``jpeg_decode_batch`` call: the table blobs of n files of ONE geometry and ONE restart interval, ``lead``
    spare bytes, then their entropy-coded segments (RSTn markers and all) back to back -> (device uint8 tensor, segment offsets behind
    the blobs, segment lengths)."""
    n = len(parsed)
    if n < 1 or any(p.geometry != parsed[0].geometry for p in parsed) or len(datas) != n:
        raise AdainHipError("jpeg_decode_batch: expected the files of one geometry")
    if any(p.restart_interval != parsed[0].restart_interval for p in parsed):
        raise AdainHipError("jpeg_decode_batch: expected the files of one restart interval")
    return _jpeg_upload(list(zip(parsed, datas)), device, lead)


def jpeg_decode_launch(up, offsets, lengths, geometry, chunk_bits=0, restart_interval=0):
    """adain_jpeg_decode_restart_u8 on an upload of ``jpeg_decode_upload`` whose files have ``restart_interval`` MCUs per restart
    interval (0: none) -> (frames uint8 [n,h,w,c], record int32 [n,2]) on its device."""
    n = len(lengths)
    h, w, c, sampling = geometry
    blobs = n * jpeg_file.BLOB_BYTES
    off = (ctypes.c_uint64 * n)(*offsets)
    ln = (ctypes.c_uint32 * n)(*lengths)
    # the workspace is shared per stream: calls from several threads (the video path's fetch pool) on one stream must not interleave
    with _jpeg_decode_lock, scratch(up.device, "jpeg_decode", jpeg_decode_sizes, n, h, w, c, sampling, max(lengths), chunk_bits,
                                    restart_interval) as ws:
        out = torch.empty((n, h, w, c), dtype=torch.uint8, device=up.device)
        record = torch.empty((n, 2), dtype=torch.int32, device=up.device)
        _launch("adain_jpeg_decode_restart_u8", up.data_ptr() + blobs, up.numel() - blobs, up.data_ptr(), n, h, w, c, sampling, int(restart_interval), off, ln,
                out.data_ptr(), record.data_ptr(), ws.data_ptr(), ws.numel(), int(chunk_bits))
    return out, record


def jpeg_decode_batch(parsed, datas, device, chunk_bits=0, lead=0):
    """``parsed``: jpeg_file.JpegFile of n files of ONE geometry and ONE restart interval (anything else is an error), ``datas``: their
    bytes -> (frames uint8 [n,h,w,c], record int32 [n,2]: status and rounds per file), both on ``device``.  One upload - the table
    blobs, ``lead`` spare bytes, then the entropy-coded segments back to back at whatever byte offsets that gives - and one call of
    adain_jpeg_decode_restart_u8; nothing comes back and nothing waits.  A frame whose status is not 0 is unspecified."""
    up, offsets, lengths = jpeg_decode_upload(parsed, datas, device, lead)
    return jpeg_decode_launch(up, offsets, lengths, parsed[0].geometry, chunk_bits, parsed[0].restart_interval)


# progressive .jpg / .jpeg (adain_jpeg_decode_progressive_u8)
def jpeg_decode_progressive_sizes(n, h, w, c, sampling, nscans, max_segment_bytes, chunk_bits=0):
    """workspace_bytes of adain_jpeg_decode_progressive_u8_bytes: the scratch of an n-file call of ``nscans`` scans whose longest scan
    segment has ``max_segment_bytes``.  Host only.  AdainHipError for a refused shape."""
    return _size_query("adain_jpeg_decode_progressive_u8_bytes", n, h, w, c, sampling, nscans, max_segment_bytes, chunk_bits)[0]


def jpeg_decode_progressive_upload(parsed, datas, device, lead=0):
    """The one upload of a ``jpeg_decode_progressive_batch`` call: the table blobs [n][scans] of n files of ONE geometry and ONE scan
    script, ``lead`` spare bytes, then every file's scan segments back to back -> (device uint8 tensor, segment offsets behind the
    blobs [n * scans], segment lengths [n * scans])."""
    n = len(parsed)
    if n < 1 or any(p.geometry != parsed[0].geometry for p in parsed) or len(datas) != n:
        raise AdainHipError("jpeg_decode_progressive_batch: expected the files of one geometry")
    if any(p.script != parsed[0].script for p in parsed):
        raise AdainHipError("jpeg_decode_progressive_batch: expected the files of one scan script")
    return _jpeg_upload([(sc, d) for p, d in zip(parsed, datas) for sc in p.scans], device, lead)


def jpeg_decode_progressive_launch(up, offsets, lengths, geometry, script, chunk_bits=0):
    """adain_jpeg_decode_progressive_u8 on an upload of ``jpeg_decode_progressive_upload`` whose files have the scan ``script``
    (ProgressiveJpegFile.script) -> (frames uint8 [n,h,w,c], record int32 [n,2]) on its device."""
    nscans = len(script)
    n = len(lengths) // max(nscans, 1)
    h, w, c, sampling = geometry
    blobs = n * nscans * jpeg_file.BLOB_BYTES
    desc = []
    for comps, ss, se, ah, al in script:
        desc += [len(comps)] + list(comps) + [0] * (3 - len(comps)) + [ss, se, ah, al]
    scans = (ctypes.c_int32 * max(len(desc), 1))(*desc)
    off = (ctypes.c_uint64 * max(len(offsets), 1))(*offsets)
    ln = (ctypes.c_uint32 * max(len(lengths), 1))(*lengths)
    # the workspace is shared per stream, as the baseline decoder's is
    with _jpeg_decode_lock, scratch(up.device, "jpeg_decode_progressive", jpeg_decode_progressive_sizes, n, h, w, c, sampling, nscans, max(lengths, default=0),
                                    chunk_bits) as ws:
        out = torch.empty((n, h, w, c), dtype=torch.uint8, device=up.device)
        record = torch.empty((n, 2), dtype=torch.int32, device=up.device)
        _launch("adain_jpeg_decode_progressive_u8", up.data_ptr() + blobs, up.numel() - blobs, up.data_ptr(), n, h, w, c, sampling, nscans, scans, off, ln,
                out.data_ptr(), record.data_ptr(), ws.data_ptr(), ws.numel(), int(chunk_bits))
    return out, record


def jpeg_decode_progressive_batch(parsed, datas, device, chunk_bits=0, lead=0):
    """``parsed``: jpeg_file.ProgressiveJpegFile of n files of ONE geometry and ONE scan script (anything else is an error), ``datas``:
    their bytes -> (frames uint8 [n,h,w,c], record int32 [n,2]: status, and the rounds summed over the Huffman-coded scans), both on
    ``device``.  One upload and one call of adain_jpeg_decode_progressive_u8; nothing comes back and nothing waits.  A frame whose
    status is not 0 is unspecified."""
    up, offsets, lengths = jpeg_decode_progressive_upload(parsed, datas, device, lead)
    return jpeg_decode_progressive_launch(up, offsets, lengths, parsed[0].geometry, parsed[0].script, chunk_bits)


def jpeg_decode_parsed(parsed, datas, device, chunk_bits=0, lead=0):
    """``jpeg_decode_progressive_batch`` or ``jpeg_decode_batch`` of files parsed alike, by what they were parsed as.  Every route to
    the device decoders goes through here and through those two names (looked up when called: tests count the decodes there)."""
    batch = jpeg_decode_progressive_batch if isinstance(parsed[0], jpeg_file.ProgressiveJpegFile) else jpeg_decode_batch
    return batch(parsed, datas, device, chunk_bits, lead)


# .png (adain_png_decode_u8)
def png_decode_sizes(n, h, w, c_file, max_stream_bytes):
    """workspace_bytes of adain_png_decode_u8_bytes: the scratch of an n-file call whose longest zlib stream has ``max_stream_bytes``.
    Host only.  AdainHipError for a refused shape."""
    return _size_query("adain_png_decode_u8_bytes", n, h, w, c_file, max_stream_bytes)[0]


_png_decode_lock = threading.Lock()


def png_decode_batch(parsed, datas, device, c_out=None):
    """``parsed``: png_file.PngFile of n files of ONE (h, w, colour type) (anything else is an error), ``datas``: their bytes, one per
    file, or None (``jpeg_decode_batch``'s signature; a PngFile already holds its stream, so only their number is checked) -> (frames uint8 [n,h,w,c_out], record int32 [n,2]:
    status and deflate blocks per file), both on ``device``.  ``c_out``: None for the file's channels, or 3 (grey replicated, alpha
    dropped).  One upload - the zlib streams back to back - and one call of adain_png_decode_u8; nothing comes back and nothing waits.
    A frame whose status is not 0 is unspecified.  The one door to the C call (looked up when called: tests count the decodes here)."""
    device = torch.device(device)
    if device.type != "cuda":
        raise AdainHipError("png_decode_batch: expected a GPU device (the device decoder has no CPU form)")
    n = len(parsed)
    if n < 1 or any(p.geometry != parsed[0].geometry for p in parsed) or (datas is not None and len(datas) != n):
        raise AdainHipError("png_decode_batch: expected the files of one height, width and colour type")
    h, w, c = parsed[0].h, parsed[0].w, parsed[0].c
    c_out = c if c_out is None else int(c_out)
    offsets = [0]
    for p in parsed:
        offsets.append(offsets[-1] + len(p.stream))
    up = torch.frombuffer(bytearray(b"".join(p.stream for p in parsed) + b"\0"), dtype=torch.uint8).to(device)
    off = (ctypes.c_uint64 * (n + 1))(*offsets)
    # Stream order is what keeps two calls off each other's workspace; the lock only keeps the size query, a growth of the stream's
    # workspace and the launch of one thread's call together, so that a second thread on the same stream cannot re-make the workspace between them
    with _png_decode_lock, scratch(device, "png_decode", png_decode_sizes, n, h, w, c, max(len(p.stream) for p in parsed)) as ws:
        out = torch.empty((n, h, w, c_out), dtype=torch.uint8, device=device)
        record = torch.empty((n, 2), dtype=torch.int32, device=device)
        _launch("adain_png_decode_u8", up.data_ptr(), offsets[-1], off, n, h, w, c, c_out, out.data_ptr(), record.data_ptr(), ws.data_ptr(), ws.numel())
    return out, record


# What the two input formats do differently; everything below is written once over the two values.  ``owns(path)``: is the extension
# the format's; ``parse(data, **options)``: the parsed file (the module's ``parse``, looked up when called: a test replaces it), or
# ``refused`` raised with why not (the report's "host: <why>"); ``colour(p)``: is the parsed file one that mode "L" leaves to the host;
# ``alike(p)``: what the files of one batch call share; ``launch(parsed, datas, device, mode, chunk_bits)``: one group's call ->
# (out, record), through the doors above, looked up when called; ``shape(out, k, p, mode)``: row k of ``out`` as the caller's frame;
# ``failure``: the host route's text for a non-zero ``status``; ``what``, ``count``: the public function's name in its errors and the
# report's key for the record's second column.
InputFormat = collections.namedtuple("InputFormat", "what owns parse refused colour alike launch shape failure count")
JPEG_INPUT = InputFormat(
    what="jpeg_decode_u8", owns=is_jpeg_path, count="rounds", failure="the entropy-coded data did not decode cleanly",
    parse=lambda data, **options: jpeg_file.parse(data, **options), refused=jpeg_file.UnsupportedJpeg, colour=lambda p: p.c == 3,
    alike=lambda p: (p.geometry, p.script if hasattr(p, "script") else p.restart_interval),
    launch=lambda parsed, datas, device, mode, chunk_bits: jpeg_decode_parsed(parsed, datas, device, chunk_bits),
    shape=lambda out, k, p, mode: out[k] if p.c == 3 else out[k, :, :, 0] if mode != "RGB" else out[k].expand(-1, -1, 3).contiguous())
PNG_INPUT = InputFormat(
    what="png_decode_u8", owns=is_png_path, count="blocks", failure="the zlib stream did not decode cleanly (status {status})",
    parse=lambda data, **options: png_file.parse(data, **options), refused=png_file.UnsupportedPng, colour=lambda p: p.c != 1,
    alike=lambda p: p.geometry,
    launch=lambda parsed, datas, device, mode, chunk_bits: png_decode_batch(parsed, datas, device, 3 if mode == "RGB" else None),
    shape=lambda out, k, p, mode: out[k, :, :, 0] if out.shape[3] == 1 else out[k])          # (the kernel replicated grey and dropped alpha)


def settle_decodes(fmt, items, device, mode=None, chunk_bits=0):
    """``items``: (key, parsed, data) per file that ``fmt.parse`` took -> yields (key, frame | None, status, count) per file, group by
    group: the files are grouped by ``fmt.alike``, EVERY group is launched (one upload and one call each) before anything is read, then
    each group's record is read once, in launch order (the read waits for the call).  ``frame``: ``fmt.shape``'s, on ``device``, or None
    for a non-zero status.  ``mode``: None or "RGB" (a grey file replicated, a .png's alpha dropped).  A generator: nothing is launched
    before the first result is asked for."""
    groups = {}
    for item in items:
        groups.setdefault(fmt.alike(item[1]), []).append(item)
    launched = [(members, fmt.launch([p for _, p, _ in members], [d for _, _, d in members], device, mode, chunk_bits)) for members in groups.values()]
    for members, (out, record) in launched:
        rec = record.cpu().tolist()                      # the one read of the record: waits for the call
        for k, (key, p, _) in enumerate(members):
            status, count = rec[k]
            yield key, fmt.shape(out, k, p, mode) if status == 0 else None, status, count


def read_input(fmt, path, **options):
    """The file at ``path``, read and parsed -> (the parsed file, its bytes), or None for a file ``fmt.parse`` refuses."""
    with open(str(path), "rb") as f:
        data = f.read()
    try:
        return fmt.parse(data, **options), data
    except fmt.refused:
        return None


def _pil_pixels(data, mode):
    import io

    import numpy as np
    from PIL import Image

    img = Image.open(io.BytesIO(data))
    return np.asarray(img.convert(mode) if mode is not None else img)


def _decode_files(fmt, files, device, mode, report, chunk_bits=0, **options):
    """``jpeg_decode_u8`` / ``png_decode_u8``: parse every file, settle what the device takes, PIL for the rest, the report."""
    single = isinstance(files, (bytes, bytearray, memoryview))
    datas = [bytes(files)] if single else [bytes(f) for f in files]
    device = torch.device(device if device is not None else f"cuda:{torch.cuda.current_device()}")
    if mode not in (None, "RGB", "L"):
        raise AdainHipError(f"{fmt.what}: mode must be None, 'RGB' or 'L', got {mode!r}")
    results, why, counts, items = [None] * len(datas), [None] * len(datas), [0] * len(datas), []
    for i, d in enumerate(datas):
        try:
            p = fmt.parse(d, **options)
        except fmt.refused as e:
            why[i] = str(e)
            continue
        if mode == "L" and fmt.colour(p):
            why[i] = "a colour file where grey is wanted"
        else:
            items.append((i, p, d))
    for i, frame, status, count in settle_decodes(fmt, items, device, mode, chunk_bits):
        results[i], counts[i] = frame, count
        if frame is None:
            why[i] = fmt.failure.format(status=status)
    for i, d in enumerate(datas):
        if results[i] is None:
            results[i] = torch.from_numpy(_pil_pixels(d, mode).copy()).to(device)
    if report is not None:
        report[:] = [{"path": "device" if w is None else "host: " + w, fmt.count: n} for w, n in zip(why, counts)]
    return results[0] if single else results


def _decode_rgb_file(fmt, path, device, **options):
    """``jpeg_decode_rgb_file`` / ``png_decode_rgb_file``: a file of another extension is not opened."""
    read = read_input(fmt, path, **options) if fmt.owns(path) and torch.device(device).type == "cuda" else None
    if read is None:
        return None
    (_, frame, _, _), = settle_decodes(fmt, [(path, *read)], device, "RGB")
    return frame


def jpeg_decode_u8(files, device=None, chunk_bits=0, mode=None, report=None, restart=False, progressive=False):
    """The bytes of image files (a list, or one ``bytes``) -> device uint8 tensors (a list, or one): per file the array
    ``np.asarray(Image.open(io.BytesIO(data)))`` gives - [h,w,3] for a colour file, [h,w] for a grey one - or, with ``mode`` "RGB" / "L",
    ``np.asarray(Image.open(...).convert(mode))`` (a grey file is replicated for "RGB"; "L" from a colour file goes to the host).  Baseline
    JPEG files are decoded on the device (adain_jpeg_decode_restart_u8; grouped by geometry and restart interval, one call and one
    upload per group, the record read once); whatever jpeg_file.parse refuses, and any file whose status comes back non-zero, is decoded
    by PIL on the host exactly as before and uploaded - PIL's exceptions pass through.  ``restart``: files with a restart interval (DRI,
    RSTn markers) are decoded on the device as well; False, the default, leaves them to PIL as before.  ``progressive``: 8-bit
    progressive Huffman (SOF2) files with a complete scan script are decoded on the device as well (adain_jpeg_decode_progressive_u8;
    grouped by geometry and scan script); False, the default, leaves them to PIL as before.  ``report`` (a list): per file "device" or
    "host: <why>", and the rounds (a progressive file's: summed over its Huffman-coded scans)."""
    return _decode_files(JPEG_INPUT, files, device, mode, report, chunk_bits, restart=restart, progressive=progressive)


def png_decode_u8(files, device=None, mode=None, report=None):
    """The bytes of PNG files (a list, or one ``bytes``) -> device uint8 tensors (a list, or one): per file the array
    ``np.asarray(Image.open(io.BytesIO(data)))`` gives - [h,w] for a grey file, [h,w,3] for RGB, [h,w,4] for RGBA - or, with ``mode``
    "RGB" / "L", ``np.asarray(Image.open(...).convert(mode))`` (grey is replicated and alpha dropped for "RGB"; "L" from a colour file
    goes to the host).  8-bit non-interlaced files of colour type 0, 2 or 6 are decoded on the device (adain_png_decode_u8; grouped by
    height, width and colour type, one upload and one call per group, the record read once); whatever png_file.parse refuses, and any
    file whose status comes back non-zero, is decoded by PIL on the host exactly as before and uploaded - PIL's exceptions pass through.
    ``report`` (a list): per file "device" or "host: <why>", and the deflate blocks the device read."""
    return _decode_files(PNG_INPUT, files, device, mode, report)


def jpeg_decode_rgb_file(path, device, progressive=False):
    """The frame ``np.asarray(Image.open(path).convert("RGB"))`` as a uint8 [h,w,3] tensor on ``device``, decoded there - or None when
    the file is not one the device decoder takes (not a .jpg / .jpeg name, refused by jpeg_file.parse, a non-zero status): the caller
    then decodes it with PIL as before.  Files with restart intervals are taken; progressive files only with ``progressive=True``.
    Reads the record once (waits for the call)."""
    return _decode_rgb_file(JPEG_INPUT, path, device, restart=True, progressive=progressive)


def png_decode_rgb_file(path, device):
    """The frame ``np.asarray(Image.open(path).convert("RGB"))`` as a uint8 [h,w,3] tensor on ``device``, decoded there - or None when
    the file is not one the device decoder takes (not a .png name, refused by png_file.parse, a non-zero status): the caller then
    decodes it with PIL as before.  Reads the record once (waits for the call)."""
    return _decode_rgb_file(PNG_INPUT, path, device)


# .gif (adain_gif_decode_u8, include/adain_gif_decode.h)
GIFD_ROW_WORDS = 8                      # ADAIN_GIFD_ROW_WORDS
GIFD_STATUS = {0: "ok", 1: "the data ends before the rectangle is full", 2: "a code above the next free entry", 3: "a first code behind a CLEAR that is no root",
               4: "the end code before the rectangle is full", 5: "a row of the frame table that leaves the screen, the blob or its plane"}


def gif_decode_sizes(n, H, W, max_frame_pixels):
    """workspace_bytes of adain_gif_decode_u8_bytes: the index planes of an n-frame clip on an H x W screen whose largest rectangle has
    ``max_frame_pixels`` pixels.  Host only.  AdainHipError for a refused shape."""
    return _size_query("adain_gif_decode_u8_bytes", n, H, W, max_frame_pixels)[0]


def gif_decode_table(clip, lead=0):
    """A ``gif_file.GifClip`` -> (the frame table as n x 8 Python ints, the blob ``bytes``): every colour table once, then every frame's
    data; ``lead`` bytes of zeros in front of all of it (the far-batch test's).  The rows: include/adain_gif_decode.h."""
    parts, at, tables, rows = [bytes(lead)] if lead else [], lead, {}, []
    for f in clip.frames:
        if f.table not in tables:
            tables[f.table] = at
            parts.append(f.table)
            at += len(f.table)
    for f in clip.frames:
        flags = f.code_size | int(f.interlace) << 8 | f.disposal << 16 | ((0 if f.transparent is None else f.transparent + 1) << 32)
        rows.append([at, len(f.data), f.left | f.top << 16 | f.w << 32 | f.h << 48, flags, tables[f.table], len(f.table) // 3, clip.background, 0])
        parts.append(f.data)
        at += len(f.data)
    return rows, b"".join(parts)


_gif_decode_lock = threading.Lock()


def gif_decode_clip(clip, device):
    """A ``gif_file.GifClip`` -> (frames uint8 [n,H,W,3], record int32 [n,2]: status and codes per frame), both on ``device``.  One upload
    - the frame table and the blob in one buffer - and one call of adain_gif_decode_u8; nothing comes back and nothing waits.  With any
    status not 0 the frames are unspecified.  The one door to the C call (looked up when called: tests count the decodes here)."""
    import numpy as np

    device = torch.device(device)
    if device.type != "cuda":
        raise AdainHipError("gif_decode_clip: expected a GPU device (the device decoder has no CPU form)")
    rows, blob = gif_decode_table(clip)
    n = len(rows)
    table = np.asarray(rows, dtype=np.uint64).tobytes()
    up = torch.frombuffer(bytearray(table + blob + b"\0"), dtype=torch.uint8).to(device)
    with _gif_decode_lock, scratch(device, "gif_decode", gif_decode_sizes, n, clip.h, clip.w, max(f.w * f.h for f in clip.frames)) as ws:
        out = torch.empty((n, clip.h, clip.w, 3), dtype=torch.uint8, device=device)
        record = torch.empty((n, 2), dtype=torch.int32, device=device)
        _launch("adain_gif_decode_u8", up.data_ptr() + len(table), len(blob), up.data_ptr(), n, clip.h, clip.w, out.data_ptr(), record.data_ptr(), ws.data_ptr(),
                ws.numel())
    return out, record


def gif_decode_u8(data, device=None, report=None):
    """The bytes of an animated GIF -> (frames uint8 [n,H,W,3] on the device, ``gif_file.GifInfo(durations, loop, size)``): per frame the
    array ``np.asarray(f.convert("RGB"))`` of Pillow's ``ImageSequence.Iterator``.  What gif_file.parse takes is decoded and composed on
    the device (adain_gif_decode_u8: one upload, one call, the record read once); a file it refuses, and a clip with any frame whose
    status comes back non-zero, is decoded whole by Pillow on the host and uploaded - Pillow's pixels, or Pillow's exception.  ``report``
    (a list): one entry, "device" or "host: <why>", and the LZW codes the device read."""
    from . import gif_file

    data = bytes(data)
    device = torch.device(device if device is not None else f"cuda:{torch.cuda.current_device()}")
    why, codes, frames, info = None, 0, None, None
    try:
        clip = gif_file.parse(data)
    except gif_file.UnsupportedGif as e:
        why = str(e)
    else:
        frames, record = gif_decode_clip(clip, device)
        rec = record.cpu().tolist()                      # the one read of the record: waits for the call
        codes = sum(c for _, c in rec)
        bad = [(k, s) for k, (s, _) in enumerate(rec) if s != 0]
        if bad:
            why, frames = f"frame {bad[0][0]}: {GIFD_STATUS.get(bad[0][1], bad[0][1])} (status {bad[0][1]})", None
        else:
            info = clip.info
    if frames is None:
        pixels, info = gif_file.pil_clip(data)
        frames = torch.from_numpy(pixels).to(device)
    if report is not None:
        report[:] = [{"path": "device" if why is None else "host: " + why, "codes": codes}]
    return frames, info


def nhwc_to_nchw(x):
    x = device_tensor(x, "x")
    n, h, w, c = x.shape
    return _map("adain_nhwc_to_nchw", x, (n, c, h, w), n, c, h * w)


def nchw_to_nhwc(x):
    x = device_tensor(x, "x")
    n, c, h, w = x.shape
    return _map("adain_nchw_to_nhwc", x, (n, h, w, c), n, c, h * w)


# --- single conv layer (tests / profiling) -------------------------------------------------------------------------------------
def _pack_layer(which, w_oihw):
    w = device_tensor(w_oihw, "weight")
    cout, cin = w.shape[:2]
    return _map(f"adain_conv3x3_{which}_pack", w, getattr(lib(), f"adain_conv3x3_{which}_packed_floats")(cin, cout), cin, cout)


def conv3x3_wino_pack(w_oihw, form=5):
    """Packed transformed weights U = G4 g G2^T for conv3x3_wino / conv3x3_wino4_split (24 floats per (cin, cout) pair)."""
    if form != 5:
        raise AdainHipError(f"conv3x3_wino_pack: form {form} is retired; the library runs form 5, F(4,3) x F(2,3)")
    return _pack_layer("wino4", w_oihw)


def conv3x3_up2x_poly_pack(w_oihw):
    """Packed weights of the polyphase up layer (adain_conv3x3_up2x_poly_pack): per output phase the folded 2 x 2 filter in
    Winograd F(5,2) x F(3,2), 96 floats per (cin, cout) pair."""
    return _pack_layer("up2x_poly", w_oihw)


def _conv_layer(x, cout, src_mode, pool_out):
    """A generic 3x3 layer over NHWC ``x``: ((n, h, w, hs, ws, cin), empty NHWC result) - h x w is the conv's own size, the source's
    hs x ws doubled under SRC_UP2X; the result is that, halved (rounding up) under ``pool_out``."""
    n, hs, ws_, cin = x.shape
    h, w = (2 * hs, 2 * ws_) if src_mode == SRC_UP2X else (hs, ws_)
    oh, ow = ((h + 1) // 2, (w + 1) // 2) if pool_out else (h, w)
    return (n, h, w, hs, ws_, cin), torch.empty((n, oh, ow, cout), dtype=torch.float32, device=x.device)


def conv3x3_wino(x_nhwc, packed_w, bias, cout, src_mode=SRC_DIRECT, relu=True, pool_out=False, m_tiles=5):
    """One generic 3x3 layer, ReflectionPad2d(1) + Conv2d [+ ReLU] [+ fused ceil-mode pool] on NHWC, in the form the schedules run
    (``m_tiles`` = the C ABI's `form`, 5 = F(4,3) x F(2,3); weights packed by conv3x3_wino_pack)."""
    x = device_tensor(x_nhwc, "x")
    dims, out = _conv_layer(x, cout, src_mode, pool_out)
    call("adain_conv3x3_wino", x.device, x.data_ptr(), out.data_ptr(), packed_w.data_ptr(), bias.data_ptr(), *dims, cout, src_mode, int(relu),
         int(pool_out), int(m_tiles))
    return out


def conv3x3_up2x_poly(x_nhwc, packed_w, bias, cout, relu=True):
    """The decoder's up layer as the schedules run it: nearest 2x upsample + ReflectionPad2d(1) + Conv2d [+ ReLU] on NHWC, as four
    phase convolutions of the source (weights packed by conv3x3_up2x_poly_pack)."""
    x = device_tensor(x_nhwc, "x")
    n, hs, ws_, cin = x.shape
    out = torch.empty((n, 2 * hs, 2 * ws_, cout), dtype=torch.float32, device=x.device)
    call("adain_conv3x3_up2x_poly", x.device, x.data_ptr(), out.data_ptr(), packed_w.data_ptr(), bias.data_ptr(), n, hs, ws_, cin, cout,
         int(relu))
    return out


def conv3x3_wino4_split_bytes(n, h, w, cin, cout):
    """Bytes of partial-sum slabs a launch of this layer needs to be split along cin; 0: it would not be split.  For the device
    that is current on the calling thread (its compute units decide the split)."""
    return lib().adain_conv3x3_wino4_split_workspace_bytes(int(n), int(h), int(w), int(cin), int(cout))


def conv3x3_wino4_split(x_nhwc, packed_w, bias, cout, src_mode=SRC_DIRECT, relu=True, pool_out=False):
    """The F(4,3) x F(2,3) layer as the latency schedule runs it: split along cin when the launch is smaller than the chip
    (adain_conv3x3_wino4_split; weights packed by conv3x3_wino_pack(form=5))."""
    x = device_tensor(x_nhwc, "x")
    dims, out = _conv_layer(x, cout, src_mode, pool_out)
    n, h, w, _hs, _ws, cin = dims
    # a launch that would not be split (a 0 answer) ignores the slabs it is handed
    with scratch(x.device, "conv_split", "adain_conv3x3_wino4_split_workspace_bytes", n, h, w, cin, cout) as ws:
        _launch("adain_conv3x3_wino4_split", x.data_ptr(), out.data_ptr(), packed_w.data_ptr(), bias.data_ptr(), *dims, cout, src_mode,
                int(relu), int(pool_out), ws.data_ptr(), ws.numel())
    return out
