"""Writes every sound and damaged file of tests/png_decode_cases.py into one binary file for tools/png_decode_check.cpp, the stand-alone
program that runs the decoder's cores on the CPU (under a sanitiser).  Per case: the name, h, w, c, the expected status, the zlib stream
that png_file.parse hands over and, for a sound file, the pixels (the case's own, or Pillow's for a fixture).  Little-endian uint32s.

    python tools/png_decode_dump_cases.py cases.bin
"""
import importlib.util
import io
import os
import struct
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))


def _png_file():
    spec = importlib.util.spec_from_file_location("png_file", os.path.join(ROOT, "applied-image-processing_amd", "png_file.py"))
    mod = importlib.util.module_from_spec(spec)
    sys.modules["png_file"] = mod
    spec.loader.exec_module(mod)
    return mod


def main(path):
    from PIL import Image

    import png_decode_cases as cases

    png_file = _png_file()
    out = []
    for c in cases.sound() + cases.damaged():
        p = png_file.parse(c.data)
        assert (p.h, p.w, p.c) == (c.h, c.w, c.c), c.name
        pixels = b""
        if c.status == 0:
            px = c.pixels if c.pixels is not None else np.asarray(Image.open(io.BytesIO(c.data)))
            pixels = np.ascontiguousarray(px, np.uint8).tobytes()
            assert len(pixels) == c.h * c.w * c.c, c.name
        name = c.name.encode()
        out.append(struct.pack("<I", len(name)) + name + struct.pack("<6I", c.h, c.w, c.c, c.status, len(p.stream), len(pixels)) + p.stream + pixels)
    with open(path, "wb") as f:
        f.write(struct.pack("<I", len(out)) + b"".join(out))
    print(f"{len(out)} cases -> {path}")


if __name__ == "__main__":
    main(sys.argv[1])
