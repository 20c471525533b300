"""Command-line front end of the MI355X AdaIN path with the flag set and defaults of the reference's
Style_3DGS/AdaIN/run_depth.py (:13-55), so existing invocations keep working:

    python -m applied_image_processing_amd.AdaIN.run_depth --content c.jpg --style s.jpg [--use_depth]

Extra flags make the depth-aware mode usable offline (the reference pulls MiDaS through torch.hub at run time):
``--depth_npy`` takes a precomputed proximity map, ``--vgg`` / ``--decoder`` the checkpoint paths; ``--jpeg_on_device`` encodes the
result's JPEG file on the GPU (the same bytes); ``--jpeg_quality``, ``--jpeg_subsampling`` (4:4:4, 4:2:2, 4:2:0), ``--jpeg_optimize`` and ``--jpeg_progressive``
are Pillow's save keywords for that file, on either route; ``--jpeg_decode_on_device`` decodes a baseline JPEG
content there too (the same pixels), ``--jpeg_decode_progressive`` (which implies it) a progressive one as well; ``--coral_on_device`` preserves the content's colours (``adain_inference``'s
``preserve_color``, which the reference's CLI does not expose) with CORAL computed on the GPU.

Style interpolation (the upstream AdaIN CLI's flag, Style_3DGS/AdaIN/test_video.py:77-79): ``--style a.jpg,b.jpg
--style_interpolation_weights 1,3`` styles the content with a mix of the styles.  The weights are divided by their sum (in double),
as the upstream CLI does; this is the only place where they are normalised.
"""
import argparse

import numpy as np
import torch

from .. import runtime as rt
from .test import adain_inference, output_routes, set_device_coral, set_output_routes

# (flag, argparse keyword arguments) — names and defaults as in the reference CLI
_REFERENCE_FLAGS = (
    ("--content", dict(type=str, required=True, help="content image file")),
    ("--style", dict(type=str, required=True, help="style image file (several, comma-separated, with --style_interpolation_weights)")),
    ("--output", dict(type=str, default="output", help="directory the result is written to")),
    ("--file_name", dict(type=str, default="stylized", help="result file name, extension excluded")),
    ("--depth_offset", dict(type=float, default=0.15, help="cap of the strength map is 1 - offset (depth-aware mode)")),
    ("--depth_prominence", dict(type=float, default=20, help="slope of the sigmoid applied to the proximity map")),
    ("--use_depth", dict(action="store_true", help="blend by the depth-proximity map instead of a global alpha")),
)
_EXTRA_FLAGS = (
    ("--style_interpolation_weights", dict(type=str, default="", help="comma-separated weights, one per --style file; divided by their sum")),
    ("--depth_npy", dict(type=str, default=None, help=".npy proximity map [H0,W0]; replaces the MiDaS estimate")),
    ("--vgg", dict(type=str, default="Style_3DGS/AdaIN/models/vgg_normalised.pth", help="encoder state_dict")),
    ("--decoder", dict(type=str, default="Style_3DGS/AdaIN/models/decoder.pth", help="decoder state_dict")),
    ("--jpeg_on_device", dict(action="store_true", help="encode the output JPEG on the GPU instead of in PIL (byte-identical file)")),
    ("--jpeg_quality", dict(type=int, default=75, help="Pillow's quality of the output JPEG, 1..100 (PIL or --jpeg_on_device: the same file)")),
    ("--jpeg_subsampling", dict(type=str, default="4:2:0", choices=["4:4:4", "4:2:2", "4:2:0"], help="chroma subsampling of the output JPEG")),
    ("--jpeg_optimize", dict(action="store_true", help="give the output JPEG its own optimal Huffman tables (Pillow's optimize=True)")),
    ("--jpeg_progressive", dict(action="store_true", help="write the output JPEG as a progressive file (Pillow's progressive=True)")),
    ("--coral_on_device", dict(action="store_true", help="preserve the content's colours (preserve_color) with CORAL computed on the GPU")),
    ("--jpeg_decode_on_device", dict(action="store_true", help="decode a baseline JPEG content on the GPU instead of in PIL (the same pixels)")),
    ("--jpeg_decode_progressive", dict(action="store_true", help="decode a progressive JPEG content on the GPU too (implies --jpeg_decode_on_device)")),
    ("--save_ext", dict(type=str, default=".jpg", help="extension of the result file (adain_inference's save_ext)")),
    ("--png_on_device", dict(action="store_true", help="encode a .png result on the GPU instead of in PIL (the same pixels, not Pillow's bytes)")),
    ("--png_decode_on_device", dict(action="store_true", help="decode an 8-bit RGB .png content on the GPU instead of in PIL (the same pixels)")),
)


def interpolation_weights(text, n_styles):
    """``--style_interpolation_weights 1,3`` -> [0.25, 0.75]: divided by their sum in double (the upstream CLI's convention)."""
    w = [float(v) for v in text.split(",")]
    if len(w) != n_styles:
        raise SystemExit(f"--style_interpolation_weights: {len(w)} weights for {n_styles} style files")
    total = sum(w)
    if not total > 0 or any(v < 0 for v in w):
        raise SystemExit("--style_interpolation_weights: the weights must be non-negative with a positive sum")
    return [v / total for v in w]


def main(argv=None):
    ap = argparse.ArgumentParser(description="AdaIN style transfer of one image on an MI355X.")
    for flag, kw in _REFERENCE_FLAGS + _EXTRA_FLAGS:
        ap.add_argument(flag, **kw)
    ns = ap.parse_args(argv)
    proximity = None
    if ns.depth_npy:
        proximity = torch.from_numpy(np.load(ns.depth_npy).astype(np.float32))
    jpeg = rt.JpegRoutes(ns.jpeg_on_device, ns.jpeg_decode_on_device or ns.jpeg_decode_progressive, ns.jpeg_decode_progressive,
                         (ns.jpeg_quality, ns.jpeg_subsampling, ns.jpeg_optimize, ns.jpeg_progressive))
    prev_routes = set_output_routes(rt.OutputRoutes(jpeg, output_routes().png.replace(encode_on_device=ns.png_on_device,
                                                                                      decode_on_device=ns.png_decode_on_device)))
    prev_coral = set_device_coral(ns.coral_on_device)
    style, mix = ns.style, {}
    if ns.style_interpolation_weights:
        style = ns.style.split(",")
        mix = {"style_interpolation_weights": interpolation_weights(ns.style_interpolation_weights, len(style))}
    elif "," in ns.style:
        raise SystemExit("--style: several files need --style_interpolation_weights")
    try:
        return adain_inference(ns.content, style, vgg_str=ns.vgg, decoder_str=ns.decoder, depth_offset=ns.depth_offset,
                               depth_prominence=ns.depth_prominence, output=ns.output, file_name=ns.file_name,
                               use_depth=ns.use_depth, depth_map=proximity, preserve_color=ns.coral_on_device, save_ext=ns.save_ext, **mix)
    finally:
        set_output_routes(prev_routes)
        set_device_coral(prev_coral)


if __name__ == "__main__":
    main()
