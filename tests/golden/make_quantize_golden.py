"""Makes the palette chooser's quality fixtures: thumbnails of the modelled project's pictures under tests/golden/quantize/ and the
table tests/golden/quantize_quality.json.

    python tests/golden/make_quantize_golden.py REFERENCE_ROOT      # thumbnails and table
    python tests/golden/make_quantize_golden.py                     # the table alone, from the thumbnails that are there

A thumbnail is the picture as RGB, ``Image.thumbnail((160, 160), LANCZOS)``, saved as PNG.  The table holds, per picture and K in 2, 4, 16,
64, 256, the PSNR of the picture against its nearest-colour map onto three palettes: tests/quantize_ref.py's ("ours", with ``used``),
Pillow's ``quantize(K, method=MEDIANCUT, dither=NONE)`` and its ``FASTOCTREE``; Pillow's own maps are what it is credited with.
"""
import json
import os
import sys

import numpy as np
from PIL import Image

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))

import quantize_ref as Q  # noqa: E402

SOURCES = ["assets/readme/brad_pitt.jpg", "assets/readme/brushstrokes.jpg", "assets/readme/cat.jpg", "assets/readme/munch.jpg", "assets/readme/oil_painting.jpg",
           "assets/readme/sailboat.jpg", "assets/readme/pixel_art/st.png", "assets/readme/pixel_art/orig.png", "input/3dgs/bathtub_0121/images/000.png"]
KS = (2, 4, 16, 64, 256)
DIR = os.path.join(HERE, "quantize")
TABLE = os.path.join(HERE, "quantize_quality.json")


def fixture_name(source):
    return os.path.splitext(source)[0].replace("/", "_") + ".png"


def thumbnails(root):
    os.makedirs(DIR, exist_ok=True)
    for source in SOURCES:
        im = Image.open(os.path.join(root, source)).convert("RGB")
        im.thumbnail((160, 160), Image.LANCZOS)
        im.save(os.path.join(DIR, fixture_name(source)), optimize=True)


def ours(a, K):
    pal, used = Q.palette(a, K)
    return Q.psnr(a, pal[:used][Q.nearest(a, pal[:used])]), used


def pillow(a, K, method):
    return Q.psnr(a, np.asarray(Image.fromarray(a).quantize(K, method=method, dither=Image.Dither.NONE).convert("RGB")))


def table():
    out = {}
    for source in SOURCES:
        a = np.asarray(Image.open(os.path.join(DIR, fixture_name(source))).convert("RGB"))
        rows = {}
        for K in KS:
            value, used = ours(a, K)
            rows[str(K)] = {"ours": value, "used": used, "mediancut": pillow(a, K, Image.Quantize.MEDIANCUT), "fastoctree": pillow(a, K, Image.Quantize.FASTOCTREE)}
        out[fixture_name(source)] = rows
    return out


if __name__ == "__main__":
    if len(sys.argv) > 1:
        thumbnails(sys.argv[1])
    t = table()
    with open(TABLE, "w") as f:
        json.dump({"pillow": __import__("PIL").__version__, "psnr_db": t}, f, indent=1, sort_keys=True)
    for name, rows in t.items():
        print(name, {K: (round(r["ours"], 2), r["used"], round(r["mediancut"], 2), round(r["fastoctree"], 2)) for K, r in rows.items()})
