"""Writes tests/golden/palette/: what the reference's palette page computes, by its own unmodified methods.

    python tests/golden/make_palette_golden.py /path/to/reference

Runs only where the reference tree exists.  gui/second_page.py is imported with stand-ins for the UI, graph and model modules it never
needs here; its working directory must be the reference root (it opens the palette list by a relative path).  The methods live in a
class nested in the function ``Pixelize``: their code objects are found in ``Pixelize.__code__.co_consts``, recursively, and
``types.FunctionType(code, module.__dict__)`` makes them callable with ``self=None`` (or, for ``_convert_image``, with a plain object
that carries the two attributes and the helpers it reads).  Nothing of the reference's text is copied.

Written: palettes.json - the three palettes the reference's README names, in the lospec list's format - and palette_golden.npz:
  gradient     uint8 [40,61,3]: a smooth gradient with noise; at most a few pixels lie at equal distance from two sweetie-16 entries
  ties         uint8 [24,37,3]: noise in 0..127 whose first pixels are designed ties of ``ties_palette``: between two entries, between
               three and more, at a duplicated entry, and a tie that exists only under the wrapping metric
  ties_palette uint8 [K,3], with one entry twice
  <frame>_rgb / _kd / _floyd        _recolor_image, _recolor_image_kd, _recolor_image_floyd (gradient: sweetie-16; ties: ties_palette)
  <frame>_tone<i>                   _adjust_brightness_and_contrast at TONES[i]
  convert<i>                        _convert_image on the gradient at CONVERTS[i]
"""
import importlib
import json
import os
import sys
import types

import numpy as np
from PIL import Image

HERE = os.path.dirname(os.path.abspath(__file__))
OUT = os.path.join(HERE, "palette")
NAMES = ("slso8", "sweetie-16", "borkfest")
TONES = ((0.25, 0), (0, -0.3), (-0.5, 0.8))
# (factor, resampling, grayscale, brightness, contrast, palette, reference method)
CONVERTS = ((1, Image.BILINEAR, False, 0, 0, "sweetie-16", "RGB"), (2, Image.BILINEAR, True, 0.25, 0, "slso8", "kd-tree"),
            (3, Image.NEAREST, False, -0.5, 0.8, "borkfest", "Floyd-Steinberg"), (2, Image.BICUBIC, True, 0, -0.3, None, "RGB"))
STUBS = ("pygame", "pygame.locals", "tkinter", "tkinter.filedialog", "cv2", "tensorflow", "tensorflow_hub", "utils.draw_helpers", "pixel_art.utils",
         "video.utils", "Style_3DGS", "networkx")


def gradient_frame():
    rng = np.random.default_rng(17)
    y, x = np.mgrid[0:40, 0:61]
    base = np.stack([x * 4.1, y * 6.2, (x + y) * 2.4], axis=-1)
    return np.clip(base + rng.normal(0, 6, base.shape), 0, 255).astype(np.uint8)


TIES_PALETTE = np.array([[0, 0, 0], [20, 0, 0], [0, 20, 0], [0, 0, 20], [20, 20, 20], [255, 255, 255], [255, 255, 255], [100, 50, 100], [100, 60, 100]], np.uint8)
DESIGNED = [[10, 0, 0], [0, 10, 0], [10, 10, 10], [30, 30, 0], [10, 10, 0], [255, 255, 255], [250, 250, 250], [100, 55, 100], [0, 10, 10], [10, 20, 10]]


def ties_frame():
    rng = np.random.default_rng(23)
    f = rng.integers(0, 128, (24, 37, 3), dtype=np.uint8)
    flat = f.reshape(-1, 3)
    for i in range(30):          # under 5 % of the frame: the nearest colour stays unique on the rest
        flat[i] = DESIGNED[i % len(DESIGNED)]
    return f


class _Anything:
    """What every attribute of a stand-in module is: callable, and with any attribute, to the same end."""

    def __call__(self, *args, **kwargs):
        return self

    def __getattr__(self, name):
        return self


def reference_methods(root):
    os.chdir(root)
    sys.path.insert(0, root)
    for name in STUBS:
        m = types.ModuleType(name)
        m.__path__ = []
        m.__getattr__ = lambda attr: _Anything()          # pygame.init(), pygame.font.SysFont(...), the names imported from the helpers
        sys.modules[name] = m
    sys.modules["pygame.locals"].__all__ = []
    mod = importlib.import_module("gui.second_page")

    found = {}

    def walk(code):
        for c in code.co_consts:
            if isinstance(c, types.CodeType):
                found[c.co_name] = c
                walk(c)

    walk(mod.Pixelize.__code__)
    return mod, {name: types.FunctionType(code, mod.__dict__) for name, code in found.items() if name.startswith("_") and not code.co_freevars}


def main(root):
    mod, fn = reference_methods(os.path.abspath(root))
    os.makedirs(OUT, exist_ok=True)
    palettes = {k: mod.PALETTES[k] for k in NAMES}
    with open(os.path.join(OUT, "palettes.json"), "w") as f:
        json.dump(palettes, f, indent=1, ensure_ascii=False)
    from PIL import ImageColor
    colours = {k: [ImageColor.getrgb(c) for c in v["colors"]] for k, v in palettes.items()}
    data = {"gradient": gradient_frame(), "ties": ties_frame(), "ties_palette": TIES_PALETTE}
    for name, cols in (("gradient", colours["sweetie-16"]), ("ties", [tuple(int(v) for v in c) for c in TIES_PALETTE])):
        img = Image.fromarray(data[name])
        data[name + "_rgb"] = np.asarray(fn["_recolor_image"](None, img, cols))
        data[name + "_kd"] = np.asarray(fn["_recolor_image_kd"](None, img, cols))
        data[name + "_floyd"] = np.asarray(fn["_recolor_image_floyd"](None, img, cols))
        for i, (b, c) in enumerate(TONES):
            data[f"{name}_tone{i}"] = np.asarray(fn["_adjust_brightness_and_contrast"](None, img, b, c))
    methods = ["RGB", "kd-tree", "LAB", "Floyd-Steinberg"]
    for i, (factor, mode, grey, b, c, pal, method) in enumerate(CONVERTS):
        me = types.SimpleNamespace(recolor_methods=methods, selected_recolor_method=methods.index(method))
        for helper in ("_downsample_image", "_adjust_brightness_and_contrast", "_recolor_image", "_recolor_image_kd", "_recolor_image_floyd"):
            setattr(me, helper, types.MethodType(fn[helper], me))
        out = fn["_convert_image"](me, Image.fromarray(data["gradient"]), factor, mode, grey, b, c, colours[pal] if pal else None)
        data[f"convert{i}"] = np.asarray(out)
    np.savez_compressed(os.path.join(OUT, "palette_golden.npz"), **data)
    print({k: v.shape for k, v in data.items()})


if __name__ == "__main__":
    main(sys.argv[1])
