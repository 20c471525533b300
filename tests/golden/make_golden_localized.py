"""Generates tests/golden/case_h.npz: the REFERENCE's own localized colour transfer (Style_3DGS/localized_style_transfer.py:99-168 and
the composite :232-238, imported unmodified through oracle/ref_loader.load_localized(), scikit-learn's PCA included) on seeded
synthetic inputs chosen so that every branch of match_cdf and np.interp's tie rule are exercised.

Run in the build container only (needs the reference tree):
    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_localized.py
The file holds data only: inputs are rebuilt from seeds by ``case_inputs`` (which the tests import), outputs are stored.
"""
import os
import sys

sys.dont_write_bytecode = True
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import numpy as np

import applied_image_processing_amd.synth as synth

OUT = os.path.dirname(os.path.abspath(__file__))
SAMPLE_STRIDE = 64       # every 64th sorted projection / matched value is stored

# name -> (h, w, content seed, stylised seed, mask kind, 16-level quantisation)
CASES = {
    "disc_96x128": (96, 128, 71, 72, "disc", False),         # foreground smaller than background; swapped: the other resample branch
    "disc_250x333": (250, 333, 73, 74, "disc", False),       # the odd size
    "halves_64x96": (64, 96, 75, 76, "halves", False),       # equal region sizes: no resampling
    "ties_96x128": (96, 128, 71, 72, "disc", True),          # 16 levels per channel: thousands of pixels share a colour
    "two_pixels_40x56": (40, 56, 77, 78, "two", False),      # a foreground region of exactly 2 pixels among black ones
}


def case_inputs(name):
    """(content, stylised, background mask [H,W] of 0 / 1) of a case, uint8, as run_localized_style_transfer meets them (:218-234):
    foreground = content * (1 - mask), background = stylised * mask.  Pixels are kept off exact black (max(., 1)) except where a
    case wants black pixels inside the foreground's area."""
    h, w, cseed, sseed, kind, quantise = CASES[name]
    a = (synth.image(cseed, 1, h, w)[0].transpose(1, 2, 0) * np.float32(255)).astype(np.uint8)
    b = (synth.image(sseed, 1, h, w)[0].transpose(1, 2, 0) * np.float32([200, 120, 90]) + np.float32([30, 60, 20])).astype(np.uint8)
    if quantise:
        a, b = (a // 16) * 16 + 1, (b // 16) * 16 + 1
    a, b = np.maximum(a, 1), np.maximum(b, 1)
    yy, xx = np.mgrid[:h, :w]
    if kind == "disc":
        m = (((yy - 0.45 * h) ** 2 + (xx - 0.55 * w) ** 2) >= (0.3 * min(h, w)) ** 2).astype(np.uint8)
    elif kind == "halves":
        m = (xx >= w // 2).astype(np.uint8)
    else:                                   # a 5 x 7 foreground window whose content is black but for two pixels
        m = np.ones((h, w), np.uint8)
        m[10:15, 20:27] = 0
        keep = np.zeros((h, w), bool)
        keep[11, 22] = keep[13, 25] = True
        a = np.where(((m == 0) & ~keep)[..., None], 0, a).astype(np.uint8)
    return a, b, m


def regions(name):
    """(foreground, background) uint8 images of a case: what the composite hands to color_transfer_foreground."""
    content, stylised, m = case_inputs(name)
    return content * (1 - m)[..., None], stylised * m[..., None]


def within_bar(got, want):
    """The project's bar for this truncating cast (tests/test_oracle_golden.py, case E): no channel off by more than one level, share
    of differing channel values below 1e-3."""
    d = np.abs(got.astype(int) - want.astype(int))
    return got.dtype == np.uint8 and got.shape == want.shape and d.max() <= 1 and (d > 0).mean() < 1e-3


def main():
    from applied_image_processing_amd import localized as L
    from oracle import ref_loader

    loc = ref_loader.load_localized()
    arrays = {}
    for name in CASES:
        content, stylised, m = case_inputs(name)
        fg, bg = regions(name)
        adjusted = loc.color_transfer_foreground(fg, bg)
        swapped = loc.color_transfer_foreground(bg, fg)
        fgm = 1 - m
        combined = (adjusted * fgm[..., None] + bg).astype(np.uint8)                                   # :232-241
        fg_proj, fg_pca = loc.apply_pca(loc.rgb_to_lab_pixels(fg[fg.sum(-1) > 0]))
        bg_proj, bg_pca = loc.apply_pca(loc.rgb_to_lab_pixels(bg[bg.sum(-1) > 0]))
        matched = loc.match_cdf(fg_proj, bg_proj)
        for key, val in (("adjusted", adjusted), ("adjusted_swapped", swapped), ("combined", combined),
                         ("n", np.array([len(fg_proj), len(bg_proj)], np.int64)),
                         ("comp_f", fg_pca.components_[0]), ("mean_f", fg_pca.mean_), ("comp_b", bg_pca.components_[0]), ("mean_b", bg_pca.mean_),
                         ("proj_f_sorted", np.sort(fg_proj.ravel())[::SAMPLE_STRIDE]), ("proj_b_sorted", np.sort(bg_proj.ravel())[::SAMPLE_STRIDE]),
                         ("matched", matched.ravel()[::SAMPLE_STRIDE])):
            arrays[f"{name}/{key}"] = val
        # the fixtures are only worth something if this repository's host path stays inside the bar on them by itself
        host = (L.color_transfer_foreground(fg, bg), L.color_transfer_foreground(bg, fg), L.combine_localized(content, stylised, m))
        for tag, got, want in zip(("adjusted", "swapped", "combined"), host, (adjusted, swapped, combined)):
            d = np.abs(got.astype(int) - want.astype(int))
            print(f"{name:18s} {tag:9s} n = {len(fg_proj):6d} / {len(bg_proj):6d}  host path vs reference: max {d.max()}  differing {(d > 0).sum()} of {d.size}")
            assert within_bar(got, want), (name, tag)
    path = os.path.join(OUT, "case_h.npz")
    np.savez_compressed(path, **arrays)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
