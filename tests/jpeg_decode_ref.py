"""NumPy restatement of the back half of a baseline JPEG round trip: the pixels ``Image.open(BytesIO(saved))`` gives for the file Pillow's
``Image.save(f, format="JPEG", quality=q)`` wrote (mode RGB for [h, w, 3], mode L for [h, w]) - the rules csrc/jpeg.hip runs on the
device behind its transform stage.  Entropy coding is lossless, so the decoded pixels are a function of the quantised coefficients
alone: the front half (colour conversion, chroma downsample, padding, forward DCT, quantisation) is tests/jpeg_ref.py's, imported;
this file adds dequantisation, libjpeg's integer "islow" inverse DCT, its chroma upsampling and its YCbCr -> RGB map.  Integer
arithmetic throughout: the target is the same bytes, not a tolerance.  tests/test_jpeg_roundtrip_host.py holds this to Pillow.
"""
import numpy as np

import jpeg_ref as J
from jpeg_ref import DEFAULT_QUALITY, Q_CHROMA, Q_LUMA, _blocks, _pad_edge, fdct, quant_table, quantise

# the shapes of the round trip's tests: the encoder's, then narrow and odd ones; (9, 4) and (9, 5) straddle the narrow-width rule
SHAPES = J.SHAPES + [(9, 1), (9, 2), (9, 4), (9, 5), (33, 4), (33, 5), (1, 5), (3, 6), (15, 31), (31, 15), (16, 16)]


def _idct_pass(d, n):
    """One pass of libjpeg's jidctint (jpeg_idct_islow: CONST_BITS 13, PASS1_BITS 2) along the last axis, descaled by n bits."""
    d = [d[..., k] for k in range(8)]
    z1 = (d[2] + d[6]) * 4433
    tmp2, tmp3 = z1 - d[6] * 15137, z1 + d[2] * 6270
    tmp0, tmp1 = (d[0] + d[4]) << 13, (d[0] - d[4]) << 13
    tmp10, tmp13, tmp11, tmp12 = tmp0 + tmp3, tmp0 - tmp3, tmp1 + tmp2, tmp1 - tmp2
    t0, t1, t2, t3 = d[7], d[5], d[3], d[1]
    z1, z2, z3, z4 = t0 + t3, t1 + t2, t0 + t2, t1 + t3
    z5 = (z3 + z4) * 9633
    t0, t1, t2, t3 = t0 * 2446, t1 * 16819, t2 * 25172, t3 * 12299
    z1, z2, z3, z4 = z1 * -7373, z2 * -20995, z3 * -16069 + z5, z4 * -3196 + z5
    t0, t1, t2, t3 = t0 + z1 + z3, t1 + z2 + z4, t2 + z2 + z3, t3 + z1 + z4
    o = [tmp10 + t3, tmp11 + t2, tmp12 + t1, tmp13 + t0, tmp13 - t0, tmp12 - t1, tmp11 - t2, tmp10 - t3]
    return np.stack([(x + (1 << (n - 1))) >> n for x in o], axis=-1)


def range_limit(x):
    """libjpeg's 1024-entry table centred on 128, indexed by x & 0x3FF: x + 128 clamped to 0..255 for x in -512..511, wrapping beyond."""
    i = x & 0x3FF
    return np.where(i < 512, np.minimum(i + 128, 255), np.maximum(i - 896, 0))


def idct(coef):
    """coef [..., 8, 8] dequantised, natural order -> samples 0..255: columns first (11 bits), then rows (18 bits)."""
    x = np.swapaxes(_idct_pass(np.swapaxes(coef.astype(np.int64), -1, -2), 11), -1, -2)
    return range_limit(_idct_pass(x, 18))


def _plane(p, table):
    """A plane padded to whole blocks, level-shifted -> the samples the decoder gives for it, same size."""
    q = quantise(fdct(_blocks(p)), table)                                  # [bh, bw, 8, 8], natural order
    s = idct(q * table.reshape(8, 8))
    return s.swapaxes(1, 2).reshape(p.shape)


def upsample(c, h, w):
    """A chroma plane (any size from ceil(h/2) x ceil(w/2) up) -> [h, w]: cropped to the real samples first, then libjpeg's
    h2v2_fancy_upsample with the first and last real row replicated as context - or, from 2 columns down, plain 2 x 2 replication."""
    ch, cw = -(-h // 2), -(-w // 2)
    c = c[:ch, :cw].astype(np.int64)
    if cw <= 2:
        return np.repeat(np.repeat(c, 2, axis=0), 2, axis=1)[:h, :w]
    up, down = np.concatenate([c[:1], c[:-1]]), np.concatenate([c[1:], c[-1:]])
    out = np.empty((2 * ch, 2 * cw), np.int64)
    for v, near in ((0, up), (1, down)):
        s = 3 * c + near
        left, right = np.concatenate([s[:, :1], s[:, :-1]], axis=1), np.concatenate([s[:, 1:], s[:, -1:]], axis=1)
        out[v::2, 0::2] = (3 * s + left + 8) >> 4
        out[v::2, 1::2] = (3 * s + right + 7) >> 4
    return out[:h, :w]


def roundtrip(img, quality=DEFAULT_QUALITY):
    """uint8 [h, w, 3] (RGB), [h, w] or [h, w, 1] (L) -> the uint8 array of the same shape Pillow decodes from the file it saved."""
    img = np.asarray(img)
    assert img.dtype == np.uint8 and img.ndim in (2, 3) and (img.ndim == 2 or img.shape[2] in (1, 3))
    h, w = img.shape[:2]
    ql, qc = quant_table(Q_LUMA, quality), quant_table(Q_CHROMA, quality)
    bh, bw = -(-h // 8), -(-w // 8)
    if img.ndim == 2 or img.shape[2] == 1:
        y = _plane(_pad_edge(img.reshape(h, w).astype(np.int64), 8 * bh, 8 * bw) - 128, ql)[:h, :w]
        return y.astype(np.uint8).reshape(img.shape)
    r, g, b = (img[..., k].astype(np.int64) for k in range(3))
    y = (19595 * r + 38470 * g + 7471 * b + 32768) >> 16
    cb = (-11059 * r - 21709 * g + 32768 * b + (128 << 16) + 32767) >> 16
    cr = (32768 * r - 27439 * g - 5329 * b + (128 << 16) + 32767) >> 16
    mh, mw = -(-h // 16), -(-w // 16)
    y = _plane(_pad_edge(y, 8 * bh, 8 * bw) - 128, ql)[:h, :w]
    bias = np.tile(np.array([1, 2]), 8 * mw // 2)
    chroma = []
    for p in (cb, cr):                                                     # the encoder's padding and downsample (jpeg_ref.scan_blocks)
        p = _pad_edge(p, h + (h & 1), 16 * mw)
        d = (p[0::2, 0::2] + p[0::2, 1::2] + p[1::2, 0::2] + p[1::2, 1::2] + bias) >> 2
        chroma.append(upsample(_plane(_pad_edge(d, 8 * mh, 8 * mw) - 128, qc), h, w) - 128)
    cb, cr = chroma
    rgb = [y + ((91881 * cr + 32768) >> 16), y + ((-22554 * cb - 46802 * cr + 32768) >> 16), y + ((116130 * cb + 32768) >> 16)]
    return np.clip(np.stack(rgb, axis=-1), 0, 255).astype(np.uint8)
