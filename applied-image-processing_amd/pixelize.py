"""Pixel-art palette control: the reference's palette page (gui/second_page.py, ``MainWindow._convert_image`` and its helpers) without
its UI - downsample, grey, brightness / contrast, recolour onto a palette - on frames that stay on the device.

The recolouring methods, by the bytes the reference's code produces (tests/palette_ref.py restates them, tests/golden/palette/ holds
the reference's own outputs):

``"rgb"``                       ``_recolor_image``: it subtracts uint8 from uint8, so every channel difference wraps modulo 256 before
                                the norm; the entry minimises sum_c ((p_c - P_kc) & 255)^2.  Rarely the nearest colour - and what the
                                page shows, so it is kept byte for byte.
``"kd-tree"``                   ``_recolor_image_kd``: the nearest colour, sum_c (p_c - P_kc)^2, lowest index among equals.
``"floyd-steinberg"``           ``_recolor_image_floyd`` as it runs: it takes the pixel as a view, overwrites it with the new colour and
                                only then forms the error, which is therefore zero - nothing is diffused and the result is the nearest
                                colour.  Runs the same kernel as ``"kd-tree"``.
``"floyd-steinberg-diffused"``  the loop as its lines describe it (the error taken before the pixel is overwritten): Floyd-Steinberg
                                error diffusion in float32.
``"LAB"``                       not available: it needs cv2's COLOR_RGB2LAB on uint8, which nothing here can be pinned to.

``extract_palette`` chooses a palette from the image itself (the reference's gui/seven_page.py does it with sklearn's k-means in LAB; here
a median cut in RGB by the rules at the top of csrc/quantize.hip): ``runtime.quantize_palette_u8`` on the device, the same rules in NumPy
without one, the same palette either way; ``refine=T`` adds T rounds of k-means in RGB behind the cut (csrc/quantize_refine.hip), which
also fill the entries the cut left unused.  ``--palette adaptive --colors N --refine T`` on the command line.

With a GPU the work is done by csrc/palette.hip (``runtime.palette_map_u8`` / ``tone_u8`` / ``palette_dither_u8``).  Without one
(``device="cpu"``, or ``device=None`` on a machine that has none) the same rules run in NumPy on the host: slow for the diffused
method, a Python loop over every pixel, and meant for machines without a device, not as a substitute when a kernel fails.
"""
import json

import numpy as np

METHODS = ("rgb", "kd-tree", "floyd-steinberg", "floyd-steinberg-diffused")
_METRIC = {"rgb": "rgb", "kd-tree": "nearest", "floyd-steinberg": "nearest"}
BILINEAR = 2          # PIL.Image.BILINEAR
RESAMPLING = {"NEAREST": 0, "BOX": 4, "BILINEAR": 2, "HAMMING": 5, "BICUBIC": 3, "LANCZOS": 1}          # PIL.Image.Resampling, the page's cycle


def _method(method):
    if str(method).upper() == "LAB":
        raise NotImplementedError('recolouring method "LAB" needs cv2 (cv2.COLOR_RGB2LAB on uint8), which is not available: it stays on the host')
    if method not in METHODS:
        raise ValueError(f"recolouring method must be one of {METHODS}, got {method!r}")
    return method


# --- palettes -----------------------------------------------------------------------------------------------------------------------
def parse_palette(colors):
    """``"#rrggbb"`` strings (as the lospec list has them; ``"rrggbb"`` too) or RGB triples, or a mix -> uint8 [K,3], 1 <= K <= 256."""
    rows = []
    for c in colors:
        if isinstance(c, str):
            t = c.strip().lstrip("#")
            if len(t) != 6:
                raise ValueError(f"palette colour {c!r} is not #rrggbb")
            rows.append([int(t[i:i + 2], 16) for i in (0, 2, 4)])
        else:
            v = [int(x) for x in c]
            if len(v) != 3 or min(v) < 0 or max(v) > 255:
                raise ValueError(f"palette colour {c!r} is not an RGB triple of 0..255")
            rows.append(v)
    if not 1 <= len(rows) <= 256:
        raise ValueError(f"a palette has 1..256 colours, got {len(rows)}")
    return np.asarray(rows, dtype=np.uint8).reshape(-1, 3)


def load_palettes(path):
    """A JSON file in the lospec list's format, ``{key: {"name": ..., "author": ..., "colors": ["#rrggbb", ...]}}`` -> {key: uint8 [K,3]}."""
    with open(path) as f:
        data = json.load(f)
    return {key: parse_palette(entry["colors"]) for key, entry in data.items()}


# --- the tone step --------------------------------------------------------------------------------------------------------------------
def tone_lut(brightness, contrast):
    """``_adjust_brightness_and_contrast`` as a table: its float64 arithmetic is a function of the channel value alone, so the
    expression evaluated on 0..255 is the whole method.  uint8 [256], or None when both adjustments are zero (the reference skips the step)."""
    if brightness == 0 and contrast == 0:
        return None
    a = np.arange(256) / 255
    if brightness != 0:
        a += brightness
    if contrast != 0:
        a = (a - 0.5) * np.tan((0.5 + contrast) * np.pi / 4) + 0.5
    return (a.clip(0, 1) * 255).astype(np.uint8)


def _grey_host(a):
    """Pillow's convert("L").convert("RGB") (ImagingConvert's rgb2l, Pillow 12.2.0)."""
    v = a.astype(np.uint32)
    L = ((19595 * v[..., 0] + 38470 * v[..., 1] + 7471 * v[..., 2] + 0x8000) >> 16).astype(np.uint8)
    return np.repeat(L[..., None], 3, axis=-1)


def _tone_host(a, lut, grey):
    if grey:
        a = _grey_host(a)
    if lut is not None:
        a = lut[a]
    return a


# --- the host route (no GPU) -----------------------------------------------------------------------------------------------------------
def _map_host(a, pal, metric):
    best = np.full(a.shape[:-1], np.iinfo(np.int64).max, dtype=np.int64)
    idx = np.zeros(a.shape[:-1], dtype=np.intp)
    p = a.astype(np.int64)
    for k in range(len(pal)):
        d = p - pal[k].astype(np.int64)
        if metric == "rgb":
            d &= 255
        s = (d * d).sum(axis=-1)
        better = s < best
        best[better] = s[better]
        idx[better] = k
    return pal[idx]


def _dither_host(frame, pal):
    img = frame.astype(np.float32)
    h, w, _ = img.shape
    P = pal.astype(np.float32)
    out = np.empty_like(frame)
    for y in range(h):
        for x in range(w):
            v = img[y, x].copy()
            d = P - v
            s = d * d
            k = int(np.argmin(np.sqrt((s[:, 0] + s[:, 1]) + s[:, 2])))
            out[y, x] = pal[k]
            e = v - P[k]
            if x < w - 1:
                img[y, x + 1] += e * np.float32(7 / 16)
            if y < h - 1 and x > 0:
                img[y + 1, x - 1] += e * np.float32(3 / 16)
            if y < h - 1:
                img[y + 1, x] += e * np.float32(5 / 16)
            if y < h - 1 and x < w - 1:
                img[y + 1, x + 1] += e * np.float32(1 / 16)
    return out


def _run_host(a, pal, method, lut, grey):
    a = _tone_host(a, lut, grey)
    if pal is None:
        return a
    if method == "floyd-steinberg-diffused":
        return np.stack([_dither_host(f, pal) for f in a.reshape((-1,) + a.shape[-3:])]).reshape(a.shape)
    return _map_host(a, pal, _METRIC[method])


# --- a palette chosen from the image (csrc/quantize.hip's rules on the host) -----------------------------------------------------------------
ADAPTIVE = "adaptive"          # --palette adaptive: the image's own colours, ``extract_palette``


def _quantize_host(pixels, K, refine=0):
    """The rules at the top of csrc/quantize.hip in NumPy, for machines without a GPU: ``pixels`` uint8 [N,3], all of one palette ->
    (uint8 [256,3] with zeros behind the colours, used), then ``refine`` rounds of ``_refine_host``.  The same palette as
    ``runtime.quantize_palette_u8``'s."""
    px = np.ascontiguousarray(pixels).reshape(-1, 3)
    if len(px) < 1 or len(px) >= 1 << 32:
        raise ValueError(f"extract_palette: a palette needs 1..2^32 - 1 pixels, got {len(px)}")
    v = px.astype(np.int64)
    cell = ((v[:, 0] >> 3) << 10) | ((v[:, 1] >> 3) << 5) | (v[:, 2] >> 3)
    # five planes of integer moments; bincount sums in float64, exact below 2^53 (Q stays below 2^50)
    planes = [np.bincount(cell, minlength=32768).astype(np.int64)]
    planes += [np.bincount(cell, weights=v[:, c], minlength=32768).astype(np.int64) for c in range(3)]
    planes.append(np.bincount(cell, weights=(v * v).sum(axis=1), minlength=32768).astype(np.int64))
    planes = [p.reshape(32, 32, 32) for p in planes]

    def settle(lo, hi):
        """The tight box inside cells lo..hi (inclusive, per axis) as (lo, hi, [w, Sr, Sg, Sb, Q] as Python ints)."""
        sub = planes[0][lo[0]:hi[0] + 1, lo[1]:hi[1] + 1, lo[2]:hi[2] + 1]
        lo, hi = list(lo), list(hi)
        for a in range(3):
            at = np.flatnonzero(sub.sum(axis=tuple(i for i in range(3) if i != a)))
            lo[a], hi[a] = lo[a] + int(at[0]), lo[a] + int(at[-1])
        where = tuple(slice(lo[a], hi[a] + 1) for a in range(3))
        return lo, hi, [int(p[where].sum()) for p in planes]

    def numerator(m):
        return m[0] * m[4] - (m[1] ** 2 + m[2] ** 2 + m[3] ** 2)          # w E, a Python int

    boxes = [settle([0, 0, 0], [31, 31, 31])]
    while len(boxes) < K:
        best = None
        for i, (lo, hi, m) in enumerate(boxes):
            if lo == hi:
                continue
            # E_i > E_best, exactly
            if best is None or numerator(m) * boxes[best][2][0] > numerator(boxes[best][2]) * m[0]:
                best = i
        if best is None:
            break
        lo, hi, m = boxes[best]
        side = [hi[a] - lo[a] for a in range(3)]
        axis = next(a for a in (1, 0, 2) if side[a] == max(side))
        sub = planes[0][lo[0]:hi[0] + 1, lo[1]:hi[1] + 1, lo[2]:hi[2] + 1]
        cum = np.cumsum(sub.sum(axis=tuple(i for i in range(3) if i != axis)))
        k = min(lo[axis] + int(np.searchsorted(cum, (m[0] + 1) // 2)), hi[axis] - 1)
        low_hi, high_lo = list(hi), list(lo)
        low_hi[axis], high_lo[axis] = k, k + 1
        boxes[best] = settle(lo, low_hi)
        boxes.append(settle(high_lo, hi))
    pal = np.zeros((256, 3), dtype=np.uint8)
    for i, (_, _, m) in enumerate(boxes):
        pal[i] = [(2 * m[1 + c] + m[0]) // (2 * m[0]) for c in range(3)]
    if refine:
        return _refine_host(v, pal, len(boxes), K, refine)
    return pal, len(boxes)


REFINE_MAX = 64          # ADAIN_QUANTIZE_REFINE_MAX


def _refine(refine):
    if isinstance(refine, bool) or not isinstance(refine, (int, np.integer)) or not 0 <= refine <= REFINE_MAX:
        raise ValueError(f"refine must be an int in 0..{REFINE_MAX} (rounds of k-means behind the median cut), got {refine!r}")
    return int(refine)


def _refine_host(v, pal, used, K, rounds):
    """Rules 7-11 (top of csrc/quantize_refine.hip) in NumPy: ``rounds`` rounds of k-means on the palette ``pal`` uint8 [256,3] with
    ``used`` colours, over the pixels ``v`` int64 [N,3] -> (uint8 [256,3], used).  The rules see the multiset of the pixels only, so the
    work is done on the distinct colours and their counts."""
    code, weight = np.unique((v[:, 0] << 16) | (v[:, 1] << 8) | v[:, 2], return_counts=True)
    col = np.stack([code >> 16, (code >> 8) & 255, code & 255], axis=1)
    P, u = pal.astype(np.int64), int(used)
    step = 8192          # colours at a time: a [step, 256] table of distances
    for _ in range(rounds):
        j, d = np.empty(len(col), dtype=np.int64), np.empty(len(col), dtype=np.int64)
        for at in range(0, len(col), step):
            c = col[at:at + step]
            dist = sum((c[:, ch, None] - P[None, :u, ch]) ** 2 for ch in range(3))
            near = dist.argmin(axis=1)          # the first of equal minima: the lowest index
            j[at:at + step], d[at:at + step] = near, dist[np.arange(len(c)), near]
        # bincount sums in float64, exact below 2^53 (255 x 2^32 is below 2^40)
        n = np.bincount(j, weights=weight, minlength=256).astype(np.int64)
        S = np.stack([np.bincount(j, weights=weight * col[:, ch], minlength=256).astype(np.int64) for ch in range(3)], axis=1)
        F = np.zeros(256, dtype=np.int64)
        np.maximum.at(F, j, (d << 24) | (0xFFFFFF - code))
        live = n > 0
        new = P.copy()
        new[live] = (2 * S[live] + n[live, None]) // (2 * n[live, None])
        free = np.flatnonzero(n[:K] == 0)
        donors = np.flatnonzero(live & ((F >> 24) > 0))
        donors = donors[np.lexsort((donors, -(F[donors] >> 24)))]          # the distance descending, then the index ascending
        m = min(len(free), len(donors))
        if m:
            far = 0xFFFFFF - (F[donors[:m]] & 0xFFFFFF)
            new[free[:m]] = np.stack([far >> 16, (far >> 8) & 255, far & 255], axis=1)
            u = max(u, int(free[m - 1]) + 1)
        P = new
    return P.astype(np.uint8), u


def quantize_palettes(frames, K=256, per_frame=False, device=None, refine=0):
    """``frames`` uint8 [n,h,w,3], a NumPy array or a tensor -> (palettes uint8 [P,256,3], used: a list of P ints) as NumPy, chosen on the
    device the frames are on (an array goes to the current GPU when there is one; ``device="cpu"``: never) by ``runtime.quantize_palette_u8``,
    on the host by the same rules in NumPy.  ``refine``: rounds of k-means behind the median cut, 0..64.  Waits for the device."""
    if isinstance(K, bool) or not isinstance(K, (int, np.integer)) or not 1 <= K <= 256:
        raise ValueError(f"a palette has 1..256 colours, got {K!r}")
    refine = _refine(refine)
    torch = _torch()
    dev = _device(device, frames, "tensor" if isinstance(frames, torch.Tensor) else "numpy")
    if dev is None:
        a = frames.cpu().numpy() if isinstance(frames, torch.Tensor) else np.asarray(frames)
        parts = [_quantize_host(f, int(K), refine) for f in a] if per_frame else [_quantize_host(a, int(K), refine)]
        return np.stack([p for p, _ in parts]), [u for _, u in parts]
    from . import runtime as rt
    pals, used = rt.quantize_palette_u8(_tensor(frames).to(dev), int(K), per_frame, refine)
    return pals.cpu().numpy(), used.cpu().tolist()


def extract_palette(image, K, per_frame=False, device=None, refine=0):
    """At most ``K`` colours chosen from ``image`` itself - a PIL image, a uint8 NumPy array or a uint8 tensor, [h,w,3] or [n,h,w,3] - as
    uint8 [used,3] (the reference's gui/seven_page.py ``extract_palette`` takes ``num_colors`` by k-means in LAB; this is a median cut in
    RGB, the rules at the top of csrc/quantize.hip, with ``refine`` rounds of k-means in RGB behind it, 0..64: csrc/quantize_refine.hip).
    One palette for all frames, or with ``per_frame`` a list of one per frame.  With a
    GPU the palette is chosen there, without one (or ``device="cpu"``) by the same rules in NumPy: the same palette.  Without ``refine``
    ``used`` is below ``K`` when the image has fewer than ``K`` non-empty cells of 8 x 8 x 8 colours; the rounds fill the unused entries
    with the image's farthest colours, up to twice as many a round."""
    _, frames = _open(image)
    if frames.ndim == 3:
        frames = frames[None]
    pals, used = quantize_palettes(frames, K, per_frame, device, refine)
    out = [pals[i, :u].copy() for i, u in enumerate(used)]
    return out if per_frame else out[0]


# --- inputs: a PIL image, a NumPy array or a GPU tensor; the result comes back as the same kind -----------------------------------------
def _torch():
    import torch
    return torch


def _open(image):
    """-> (kind, frames): kind "pil" | "numpy" | "tensor"; frames uint8 [h,w,3] or [n,h,w,3], a NumPy array or (kind "tensor") a tensor."""
    if hasattr(image, "convert") and hasattr(image, "size"):
        return "pil", np.asarray(image if image.mode == "RGB" else image.convert("RGB"))
    if isinstance(image, np.ndarray):
        a = image
        kind = "numpy"
    else:
        a, kind = image, "tensor"
    if str(a.dtype).split(".")[-1] != "uint8" or a.ndim not in (3, 4) or a.shape[-1] != 3:
        raise ValueError(f"expected a PIL image or uint8 [h,w,3] / [n,h,w,3], got {a.dtype} {tuple(a.shape)}")
    return kind, a


def _tensor(frames):
    torch = _torch()
    if isinstance(frames, torch.Tensor):
        return frames
    a = np.ascontiguousarray(frames)
    return torch.from_numpy(a if a.flags.writeable else a.copy())          # np.asarray of a PIL image is read-only


def _device(device, frames, kind):
    """The device the work runs on: a torch.device of type cuda, or None for the host route."""
    torch = _torch()
    if kind == "tensor" and frames.is_cuda:
        return frames.device
    if device is None:
        return torch.device("cuda", torch.cuda.current_device()) if torch.cuda.is_available() else None
    d = torch.device(device)
    return None if d.type == "cpu" else d


def _close(kind, out):
    torch = _torch()
    if kind == "tensor":
        return _tensor(out)
    a = out.cpu().numpy() if isinstance(out, torch.Tensor) else out
    if kind == "pil":
        from PIL import Image
        return Image.fromarray(a)
    return a


def _run(frames, pal, method, lut, grey, dev):
    """Tone and recolour ``frames`` (NumPy or tensor) on ``dev`` (None: the host route); pal None: the tone step alone."""
    torch = _torch()
    if dev is None:
        a = frames.cpu().numpy() if isinstance(frames, torch.Tensor) else frames
        return _run_host(a, pal, method, lut, grey)
    from . import runtime as rt
    x = _tensor(frames)
    x = x.to(dev)
    if pal is None:
        return rt.tone_u8(x, lut, grey) if (grey or lut is not None) else x
    if method == "floyd-steinberg-diffused":
        return rt.palette_dither_u8(x, pal, lut, grey)
    return rt.palette_map_u8(x, pal, _METRIC[method], lut, grey)


def _palette(colors):
    if colors is None or len(colors) == 0:
        return None
    torch = _torch()
    if isinstance(colors, torch.Tensor):
        colors = colors.cpu().numpy()
    if isinstance(colors, np.ndarray) and colors.dtype == np.uint8 and colors.ndim == 2 and colors.shape[1] == 3 and 1 <= len(colors) <= 256:
        return colors
    return parse_palette(colors)


def recolor(image, colors, method="rgb", device=None):
    """``image`` - a PIL image, a uint8 NumPy array or a uint8 tensor, [h,w,3] or [n,h,w,3] - with every pixel replaced by an entry of the
    palette ``colors`` (``parse_palette``'s forms, or a uint8 [K,3] array / tensor), returned as the same kind (a GPU tensor stays one).

    ``method``: see the module's text.  ``"kd-tree"`` and ``"floyd-steinberg"`` both run the nearest-colour kernel: the reference's
    Floyd-Steinberg loop reads its error through a view of the pixel it has just overwritten, so the error is zero and it diffuses
    nothing.  ``"floyd-steinberg-diffused"`` is the loop as its lines describe it.  ``"LAB"`` raises NotImplementedError (cv2)."""
    method = _method(method)
    pal = _palette(colors)
    if pal is None:
        raise ValueError("recolor: an empty palette")
    kind, frames = _open(image)
    return _close(kind, _run(frames, pal, method, None, False, _device(device, frames, kind)))


def convert_image(image, downsampling_factor=1, resampling_mode=BILINEAR, grayscale=False, brightness=0, contrast=0, colors=None, method="rgb",
                  device=None):
    """``_convert_image`` in its order and under its conditions: downsample to (w // f, h // f) when the factor is above 1; grey
    (Pillow's convert("L").convert("RGB")) when ``grayscale``; brightness / contrast when either is non-zero; recolour when ``colors``
    are given.  Grey, tone and recolouring are one kernel launch.

    Every ``resampling_mode`` of ``Image.Resampling`` (the page cycles through all six) is downsampled on the device through the
    Pillow-exact resizes: ``BILINEAR`` by ``runtime.resize_pil_bilinear_u8``, the others by ``runtime.resize_pil_u8``; a factor beyond the
    device calls' limit of 256 raises.  On the host route Pillow resizes.  Input kinds and ``device`` as in ``recolor``."""
    method = _method(method)
    pal = _palette(colors)
    kind, frames = _open(image)
    dev = _device(device, frames, kind)
    torch = _torch()
    f = int(downsampling_factor)
    if f > 1:
        h, w = frames.shape[-3], frames.shape[-2]
        size = (w // f, h // f)
        if dev is not None:
            frames = _downsample_device(frames, size, int(resampling_mode), dev)
        else:
            from PIL import Image
            a = frames.cpu().numpy() if isinstance(frames, torch.Tensor) else frames
            small = [np.asarray(Image.fromarray(fr).resize(size, resample=resampling_mode)) for fr in a.reshape((-1,) + a.shape[-3:])]
            frames = np.stack(small).reshape(a.shape[:-3] + (size[1], size[0], 3))
    return _close(kind, _run(frames, pal, method, tone_lut(brightness, contrast), bool(grayscale), dev))


def _downsample_device(frames, size, mode, dev):
    """``_downsample_image`` on ``dev``: frames [..., h, w, 3] (NumPy or tensor) -> a tensor [..., size[1], size[0], 3] there."""
    from . import runtime as rt
    x = _tensor(frames)
    x = x.to(dev)
    flat = x.reshape((-1,) + tuple(x.shape[-3:]))
    small = rt.resize_pil_bilinear_u8(flat, size) if mode == BILINEAR else rt.resize_pil_u8(flat, size, mode)
    return small.reshape(tuple(x.shape[:-3]) + (size[1], size[0], 3))


def frames_post(colors, method="rgb", grayscale=False, brightness=0, contrast=0, downsampling_factor=1, resampling_mode=BILINEAR):
    """An ``f(u8_block) -> u8_block`` for ``stylize_frames_sharded(post=...)``: every stylised sub-batch [n,h,w,3] leaves its rank already
    downsampled (``downsampling_factor`` above 1: to (w // f, h // f) with ``resampling_mode``, as ``convert_image`` does; the default
    keeps the frame's size) / grey / toned / recoloured, on the device, and can go straight to the device PNG or JPEG writer."""
    method = _method(method)
    pal = _palette(colors)
    lut = tone_lut(brightness, contrast)
    grey = bool(grayscale)
    f, mode = int(downsampling_factor), int(resampling_mode)

    def post(u8):
        if f > 1:
            u8 = _downsample_device(u8, (u8.shape[-2] // f, u8.shape[-3] // f), mode, u8.device)
        return _run(u8, pal, method, lut, grey, u8.device)

    return post


def main(argv=None):
    import argparse

    from PIL import Image

    ap = argparse.ArgumentParser(prog="python -m applied_image_processing_amd.pixelize", description="Recolour an image onto a palette (the reference's palette page).")
    ap.add_argument("input")
    ap.add_argument("output")
    ap.add_argument("--palette", required=True, help="a name in --palettes, #hex,#hex,... or adaptive (--colors colours chosen from the image)")
    ap.add_argument("--palettes", help="a JSON file in the lospec list's format")
    ap.add_argument("--colors", type=int, default=256, help="the colours of --palette adaptive, 1..256 (default 256)")
    ap.add_argument("--refine", type=int, default=0, metavar="T", help="rounds of k-means behind --palette adaptive's median cut, 0..64 (default 0)")
    ap.add_argument("--method", default="rgb", choices=METHODS + ("LAB",))
    ap.add_argument("--factor", type=int, default=1)
    ap.add_argument("--resampling", default="BILINEAR", type=str.upper, choices=tuple(RESAMPLING), metavar="NAME",
                    help="the downsampling filter of --factor, a member of PIL.Image.Resampling: " + ", ".join(RESAMPLING) + " (default BILINEAR)")
    ap.add_argument("--grayscale", action="store_true")
    ap.add_argument("--brightness", type=float, default=0)
    ap.add_argument("--contrast", type=float, default=0)
    a = ap.parse_args(argv)
    image = Image.open(a.input).convert("RGB")
    if a.palette == ADAPTIVE:
        if not 1 <= a.colors <= 256:
            ap.error("--colors must be in 1..256")
        if not 0 <= a.refine <= REFINE_MAX:
            ap.error(f"--refine must be in 0..{REFINE_MAX}")
        # of the image as the recolouring sees it: downsampled and toned, not yet recoloured
        colors = extract_palette(convert_image(image, a.factor, RESAMPLING[a.resampling], a.grayscale, a.brightness, a.contrast), a.colors, refine=a.refine)
    elif a.palette.startswith("#"):
        colors = parse_palette(a.palette.split(","))
    else:
        if not a.palettes:
            ap.error("a palette name needs --palettes FILE")
        palettes = load_palettes(a.palettes)
        if a.palette not in palettes:
            ap.error(f"no palette {a.palette!r} in {a.palettes}")
        colors = palettes[a.palette]
    out = convert_image(image, a.factor, RESAMPLING[a.resampling], a.grayscale, a.brightness, a.contrast, colors, a.method)
    out.save(a.output)
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
