"""Independent restatements of the palette rules (csrc/palette.hip, include/adain_hip.h "pixel-art palette control"), in NumPy, written
from the rules and not from the kernels or from pixelize.py's host route:

- ``map_index`` / ``map_frame``: the integer rules of both metrics, lowest index among equals
- ``tone_lut``: ``_adjust_brightness_and_contrast`` as a table over the 256 channel values
- ``grey``: Pillow's L formula, replicated
- ``dither_push``: the diffused loop, sequential, NumPy float32, with ``np.linalg.norm(P - v, axis=1)`` itself
- ``dither_pull``: a scalar emulation of the pull form the kernel runs - every pixel gathers its four incoming terms in the order the
  sequential loop adds them - with the explicit ``sqrt((s0 + s1) + s2)``
"""
import numpy as np

BAND = 1024          # ADAIN_PALETTE_DITHER_BAND (tests/test_palette_host.py holds it against the header and the binding)
F = np.float32


def map_index(frames, palette, metric):
    """uint8 [..., 3], uint8 [K,3] -> the chosen entry per pixel.  metric "rgb": sum ((p - P) & 255)^2; "nearest": sum (p - P)^2."""
    assert metric in ("rgb", "nearest")
    d = frames[..., None, :].astype(np.int32) - palette.astype(np.int32)          # [..., K, 3]
    if metric == "rgb":
        d = d & 255
    return (d * d).sum(axis=-1).argmin(axis=-1)          # argmin: the first minimum


def map_frame(frames, palette, metric):
    return palette[map_index(frames, palette, metric)]


def min_distance_count(frames, palette):
    """Per pixel, how many palette entries lie at the smallest true squared distance (1: no tie)."""
    d = frames[..., None, :].astype(np.int32) - palette.astype(np.int32)
    s = (d * d).sum(axis=-1)
    return (s == s.min(axis=-1, keepdims=True)).sum(axis=-1), s


def tone_lut(brightness, contrast):
    v = np.arange(256, dtype=np.uint8)
    a = np.asarray(v) / 255          # float64, as uint8 / 255 is
    if brightness != 0:
        a = a + brightness
    if contrast != 0:
        a = (a - 0.5) * np.tan((0.5 + contrast) * np.pi / 4) + 0.5
    return (np.clip(a, 0, 1) * 255).astype(np.uint8)


def grey(frames):
    r, g, b = (frames[..., c].astype(np.int64) for c in range(3))
    L = (19595 * r + 38470 * g + 7471 * b + 0x8000) >> 16
    return np.stack([L, L, L], axis=-1).astype(np.uint8)


def tone(frames, lut=None, grey_first=False):
    """grey, then lut (uint8 [256] or [3,256])."""
    a = grey(frames) if grey_first else frames
    if lut is not None:
        lut = np.broadcast_to(lut, (3, 256))
        a = np.stack([lut[c][a[..., c]] for c in range(3)], axis=-1)
    return a


def norm_rule(P, v):
    """t_k = sqrt((d0 d0 + d1 d1) + d2 d2) in float32, d = P_k - v."""
    d = (P - v).astype(F)
    s = d * d
    return np.sqrt((s[:, 0] + s[:, 1]) + s[:, 2])


def dither_push(frame, palette):
    """The loop ``_recolor_image_floyd`` spells out, with the error copied before the pixel is overwritten.  -> (frame, index)."""
    img = frame.astype(F)
    h, w, _ = img.shape
    out = np.empty((h, w, 3), np.uint8)
    idx = np.empty((h, w), np.uint8)
    for y in range(h):
        for x in range(w):
            v = img[y, x].copy()
            k = int(np.argmin(np.linalg.norm(palette - v, axis=1)))
            out[y, x], idx[y, x] = palette[k], k
            e = v - palette[k]
            if x < w - 1:
                img[y, x + 1] += e * (7 / 16)
            if y < h - 1 and x > 0:
                img[y + 1, x - 1] += e * (3 / 16)
            if y < h - 1:
                img[y + 1, x] += e * (5 / 16)
            if y < h - 1 and x < w - 1:
                img[y + 1, x + 1] += e * (1 / 16)
    return out, idx


def dither_pull(frame, palette):
    """Every pixel gathers: v = ((((p + e[y-1][x-1] 1/16) + e[y-1][x] 5/16) + e[y-1][x+1] 3/16) + e[y][x-1] 7/16), each product rounded
    to float32 before its add, terms outside the frame skipped; scalar float32 throughout.  -> (frame, index)."""
    h, w, _ = frame.shape
    P = [[F(c) for c in row] for row in palette]
    E = np.zeros((h, w, 3), F)
    out = np.empty((h, w, 3), np.uint8)
    idx = np.empty((h, w), np.uint8)
    w1, w3, w5, w7 = F(1 / 16), F(3 / 16), F(5 / 16), F(7 / 16)
    for y in range(h):
        for x in range(w):
            v = [F(frame[y, x, c]) for c in range(3)]
            for c in range(3):
                if y > 0 and x > 0:
                    v[c] = F(v[c] + F(E[y - 1, x - 1, c] * w1))
                if y > 0:
                    v[c] = F(v[c] + F(E[y - 1, x, c] * w5))
                if y > 0 and x < w - 1:
                    v[c] = F(v[c] + F(E[y - 1, x + 1, c] * w3))
                if x > 0:
                    v[c] = F(v[c] + F(E[y, x - 1, c] * w7))
            best, kb = None, 0
            for k, pk in enumerate(P):
                d = [F(pk[c] - v[c]) for c in range(3)]
                t = np.sqrt(F(F(F(d[0] * d[0]) + F(d[1] * d[1])) + F(d[2] * d[2])))
                if best is None or t < best:
                    best, kb = t, k
            for c in range(3):
                E[y, x, c] = F(v[c] - P[kb][c])
            out[y, x], idx[y, x] = palette[kb], kb
    return out, idx


def dither(frames, palette, lut=None, grey_first=False):
    """The device call's answer for uint8 [n,h,w,3] or [h,w,3]: tone, then ``dither_push`` per frame.  -> (frames, index)."""
    a = tone(frames, lut, grey_first)
    flat = a.reshape((-1,) + a.shape[-3:])
    res = [dither_push(f, palette) for f in flat]
    return np.stack([r[0] for r in res]).reshape(a.shape), np.stack([r[1] for r in res]).reshape(a.shape[:-1])
