"""Command-line front end of the localized (semantic-mask) style transfer with the flag set and defaults of the reference's
Style_3DGS/run_semantic_segm.py (:12-44), so existing invocations keep working:

    python -m applied_image_processing_amd.run_semantic_segm --content c.jpg --style s.jpg [--use_depth]

It calls ``localized.run_localized_style_transfer`` (reference Style_3DGS/localized_style_transfer.py:191-245): background mask ->
``adain_inference(content_mask=..., alpha=1)`` on the MI355X kernels -> Reinhard / PCA / CDF colour transfer of the foreground ->
composite.  Extra flags make it usable offline (the reference downloads DeepLabV3 and MiDaS at run time): ``--mask_npy`` takes a
precomputed background mask ([1,H,W] or [H,W], 1 = background), ``--depth_npy`` a proximity map, ``--vgg`` / ``--decoder`` the
checkpoint paths, ``--colour_on_device`` moves the colour transfer and the composite to the GPU, ``--jpeg_on_device`` the JPEG encode of the intermediate
stylised file and of the final composite (the same bytes); ``--jpeg_quality``, ``--jpeg_subsampling``, ``--jpeg_optimize``, ``--jpeg_progressive`` are Pillow's
keywords for the final composite's file, on either route; ``--save_ext`` is the extension of the intermediate stylised file (the final composite
stays .jpg) and, with ``--save_ext .png``, ``--png_on_device`` encodes that file on the GPU (the same pixels).  Without ``--mask_npy`` a provider must have been registered (``localized.set_mask_provider``).
"""
import argparse

import numpy as np
import torch

from .AdaIN.test import output_routes, set_output_routes
from .localized import run_localized_style_transfer

# (flag, argparse keyword arguments) - names and defaults as in the reference CLI
_REFERENCE_FLAGS = (
    ("--content", dict(type=str, required=True, help="content image file")),
    ("--style", dict(type=str, required=True, help="style image file")),
    ("--output", dict(type=str, default="output", help="directory the results are written to")),
    ("--file_name", dict(type=str, default="stylized", help="name of the intermediate stylised file, extension excluded")),
    ("--use_depth", dict(action="store_true", help="depth-aware stylisation of the background")),
)
_EXTRA_FLAGS = (
    ("--mask_npy", dict(type=str, default=None, help=".npy background mask [1,H,W] or [H,W] (1 = background); replaces the DeepLabV3 estimate")),
    ("--depth_npy", dict(type=str, default=None, help=".npy proximity map [H0,W0]; replaces the MiDaS estimate")),
    ("--vgg", dict(type=str, default="Style_3DGS/AdaIN/models/vgg_normalised.pth", help="encoder state_dict")),
    ("--decoder", dict(type=str, default="Style_3DGS/AdaIN/models/decoder.pth", help="decoder state_dict")),
    ("--colour_on_device", dict(action="store_true", help="run the foreground colour transfer and the composite on the GPU instead of in numpy")),
    ("--jpeg_on_device", dict(action="store_true", help="encode the intermediate stylised JPEG and the final composite's on the GPU instead of in PIL (byte-identical files)")),
    ("--jpeg_quality", dict(type=int, default=75, help="Pillow's quality of the final composite's JPEG, 1..100")),
    ("--jpeg_subsampling", dict(type=str, default="4:2:0", choices=["4:4:4", "4:2:2", "4:2:0"], help="chroma subsampling of the final composite's JPEG")),
    ("--jpeg_optimize", dict(action="store_true", help="give the final composite's JPEG its own optimal Huffman tables (Pillow's optimize=True)")),
    ("--jpeg_progressive", dict(action="store_true", help="write the final composite's JPEG as a progressive file (Pillow's progressive=True)")),
    ("--save_ext", dict(type=str, default=".jpg", help="extension of the intermediate stylised file (adain_inference's save_ext); the final composite stays .jpg")),
    ("--png_on_device", dict(action="store_true", help="with --save_ext .png: encode the intermediate stylised file on the GPU instead of in PIL (the same pixels, not Pillow's bytes)")),
)


def main(argv=None):
    ap = argparse.ArgumentParser(description="Localized AdaIN style transfer (stylised background, colour-matched foreground) on an MI355X.")
    for flag, kw in _REFERENCE_FLAGS + _EXTRA_FLAGS:
        ap.add_argument(flag, **kw)
    ns = ap.parse_args(argv)
    mask = None
    if ns.mask_npy:
        mask = np.load(ns.mask_npy)
        mask = (mask[None] if mask.ndim == 2 else mask).astype(np.uint8)
    extra = dict(vgg_str=ns.vgg, decoder_str=ns.decoder, save_ext=ns.save_ext)
    if ns.depth_npy:
        extra["depth_map"] = torch.from_numpy(np.load(ns.depth_npy).astype(np.float32))
    now = output_routes()
    prev = set_output_routes(now.replace(jpeg=now.jpeg.replace(encode_on_device=ns.jpeg_on_device), png=now.png.replace(encode_on_device=ns.png_on_device)))
    try:
        return run_localized_style_transfer(content_img_path=ns.content, style_img_path=ns.style, output_path=ns.output, file_name=ns.file_name,
                                            use_depth=ns.use_depth, background_mask=mask, colour_on_device=ns.colour_on_device,
                                            jpeg_on_device=ns.jpeg_on_device, jpeg_options=(ns.jpeg_quality, ns.jpeg_subsampling, ns.jpeg_optimize, ns.jpeg_progressive),
                                            **extra)
    finally:
        set_output_routes(prev)


if __name__ == "__main__":
    main()
