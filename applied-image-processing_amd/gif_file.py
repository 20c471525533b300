"""Animated GIF clips: the file the reference shows its video and pixel-art results as (Style_3DGS/render.py:29-33 ``create_gif``,
Pillow's ``save(save_all=True, duration=, loop=0)``; assets/readme/video/*.gif), written from frames that are already on the device.

A palette clip is at most 256 colours and already indexed on the device (csrc/palette.hip): the index planes are coded there
(csrc/gif.hip, ``runtime.gif_encode_u8``: one record per frame) and only the records cross to the host, which puts the file around them:

    GIF89a | logical screen descriptor: w, h, flags 0x80 | 0x70 | (g - 1) with g = max(1, ceil(log2 K)), background 0, aspect 0
    | global colour table: 3 * 2^g bytes, the palette and then zeros | NETSCAPE2.0 loop extension (more than one frame, or an explicit
    count) | the records, back to back | 3B

The records are not Pillow's bytes: the indices are cut into segments of 2048 pixels that each start with a CLEAR code, so that the
segments are coded side by side (the rules: top of csrc/gif.hip, tests/gif_ref.py); every reader decodes them to the same pixels.  Every
frame is a full frame on the global table.  Not built: frame differencing and transparency, local colour tables, interlace, choosing a
palette from the clip (Pillow's ``quantize``), reading GIFs.

Without a GPU the same indices go through Pillow's own ``save(save_all=True)``: other bytes, the same decoded pixels.
"""
import struct

import numpy as np

from . import pixelize

WEB = "web"          # the 6 x 6 x 6 colour cube, for clips that are not pixel art; it goes with "floyd-steinberg-diffused"


def web_palette():
    """uint8 [216,3]: every channel one of 0, 51, ..., 255; red slowest."""
    v = np.arange(6, dtype=np.uint8) * 51
    return np.stack(np.meshgrid(v, v, v, indexing="ij"), axis=-1).reshape(-1, 3)


def default_method(palette):
    """The method a caller that names none gets: error diffusion onto the cube, the nearest colour onto a pixel-art palette."""
    return "floyd-steinberg-diffused" if isinstance(palette, str) and palette == WEB else "kd-tree"


def _palette(palette):
    if isinstance(palette, str) and palette == WEB:
        return web_palette()
    pal = pixelize._palette(palette)
    if pal is None:
        raise ValueError("gif: an empty palette")
    return np.ascontiguousarray(pal)


def _u16(v, what):
    if isinstance(v, bool) or not isinstance(v, (int, np.integer)) or not 0 <= v <= 65535:
        raise ValueError(f"gif: {what} must be an int in 0..65535, got {v!r}")
    return int(v)


def header(size, palette, loop=None):
    """Everything in front of the first record.  ``size``: (w, h); ``palette``: ``"web"`` or 1..256 colours (``pixelize.parse_palette``'s
    forms or uint8 [K,3]); ``loop``: None for no NETSCAPE2.0 extension, or the loop count (0: for ever)."""
    pal = _palette(palette)
    w, h = (_u16(v, "a frame side") for v in size)
    if w < 1 or h < 1:
        raise ValueError(f"gif: an empty frame {size!r}")
    g = 1
    while (1 << g) < len(pal):
        g += 1
    out = b"GIF89a" + struct.pack("<HHBBB", w, h, 0x80 | 0x70 | (g - 1), 0, 0) + pal.tobytes() + bytes(3 * ((1 << g) - len(pal)))
    if loop is not None:
        out += b"\x21\xff\x0bNETSCAPE2.0\x03\x01" + struct.pack("<H", _u16(loop, "loop")) + b"\x00"
    return out


def records_bytes(records, lengths):
    """The records of a ``runtime.gif_encode_u8`` result back to back: the lengths first, then only the bytes that are records (waits for
    the device).  ValueError for a frame the device refused (length 0: an index that is not below K)."""
    ln = [int(v) for v in (lengths.cpu().tolist() if hasattr(lengths, "cpu") else np.asarray(lengths).tolist())]
    bad = [i for i, k in enumerate(ln) if k <= 0]
    if bad:
        raise ValueError(f"gif: frame(s) {bad} hold an index that is not below the palette's size")
    rows = records[:, :max(ln)]
    rows = rows.cpu().numpy() if hasattr(rows, "cpu") else np.asarray(rows)
    return b"".join(rows[i, :k].tobytes() for i, k in enumerate(ln))


def assemble(header, records, lengths):
    """``header(...)``, the records [n, stride] with their ``lengths`` (device tensors or arrays) and the trailer -> the file's ``bytes``."""
    return header + records_bytes(records, lengths) + b"\x3b"


def delay_of(fps):
    """Centiseconds per frame: round(100 / fps)."""
    if not fps > 0:
        raise ValueError(f"gif: fps must be positive, got {fps!r}")
    return _u16(int(round(100 / fps)), "the delay of this fps, in centiseconds,")


def _index_host(recoloured, pal):
    """The lowest palette index of every pixel's colour; ``recoloured`` [..., 3] holds palette colours only."""
    key = lambda a: (a[..., 0].astype(np.int64) << 16) | (a[..., 1].astype(np.int64) << 8) | a[..., 2].astype(np.int64)
    keys = key(pal)
    order = np.argsort(keys, kind="stable")
    return order[np.searchsorted(keys[order], key(recoloured))].astype(np.uint8)


def _cuda(frames):
    import torch

    if isinstance(frames, torch.Tensor):
        return frames.device if frames.is_cuda else None
    return torch.device("cuda", torch.cuda.current_device()) if torch.cuda.is_available() else None


def index_planes(frames, palette, method="kd-tree"):
    """uint8 [n,h,w,3] frames -> their palette indices uint8 [n,h,w] by ``method`` (``pixelize.METHODS``): on the device the frames are
    on (a NumPy array goes to the current GPU when there is one, a host tensor stays on the host) through ``runtime.palette_map_u8`` / ``palette_dither_u8``, a tensor;
    without a GPU by pixelize's host route, an array.  A frame ``pixelize.frames_post`` recoloured onto the palette maps to itself."""
    method = pixelize._method(method)
    pal = _palette(palette)
    dev = _cuda(frames)
    if dev is None:
        a = frames.numpy() if hasattr(frames, "numpy") else np.asarray(frames)
        return _index_host(pixelize._run_host(a, pal, method, None, False), pal)
    from . import runtime as rt
    x = pixelize._tensor(frames).to(dev)
    if method == "floyd-steinberg-diffused":
        return rt.palette_dither_u8(x, pal, index=True)[1]
    return rt.palette_map_u8(x, pal, pixelize._METRIC[method], index=True)[1]


def write_gif(frames, path, palette, fps=20, method="kd-tree", loop=0, sub_batch=None):
    """``frames`` - uint8 [N,h,w,3], a GPU tensor or a NumPy array - as an animated GIF at ``path``: mapped (``method`` "rgb", "kd-tree",
    "floyd-steinberg") or dithered ("floyd-steinberg-diffused"; None: ``default_method``) onto ``palette`` (``header``'s forms), ``round(100 / fps)`` centiseconds a
    frame, ``loop`` times (0: for ever; None: no loop extension for a single frame).  With a GPU the frames are indexed and coded there,
    ``sub_batch`` frames to a call (default: about 32 MiB of pixels), and only the records are downloaded; without one Pillow writes the
    same indices.  Returns ``path``."""
    pal = _palette(palette)
    method = default_method(palette) if method is None else method
    delay = delay_of(fps)
    if getattr(frames, "ndim", 0) != 4 or frames.shape[3] != 3 or frames.shape[0] < 1 or str(frames.dtype).split(".")[-1] != "uint8":
        raise ValueError(f"write_gif: expected uint8 [N,h,w,3], got {getattr(frames, 'dtype', None)} {tuple(getattr(frames, 'shape', ()))}")
    n, h, w, _ = frames.shape
    if loop is None and n > 1:
        loop = 0
    step = int(sub_batch) if sub_batch else max(1, min(n, (32 << 20) // (h * w)))
    if step < 1:
        raise ValueError(f"write_gif: sub_batch must be positive, got {sub_batch!r}")
    if _cuda(frames) is None:
        from PIL import Image

        idx = index_planes(frames, pal, method)
        images = [Image.frombytes("P", (w, h), f.tobytes()) for f in idx]
        for im in images:
            im.putpalette(pal.tobytes())
        extra = {} if loop is None else {"loop": loop}
        images[0].save(path, format="GIF", save_all=True, append_images=images[1:], duration=delay * 10, disposal=1, optimize=False, **extra)
        return path
    from . import runtime as rt
    parts = [header((w, h), pal, loop)]
    pending = None          # the batch before: its records are downloaded while the next one is being coded
    for i in range(0, n, step):
        coded = rt.gif_encode_u8(index_planes(frames[i:i + step], pal, method), len(pal), delay)
        if pending is not None:
            parts.append(records_bytes(*pending))
        pending = coded
    parts.append(records_bytes(*pending))
    parts.append(b"\x3b")
    with open(path, "wb") as f:
        f.write(b"".join(parts))
    return path


def main(argv=None):
    import argparse

    ap = argparse.ArgumentParser(prog="python -m applied_image_processing_amd.gif_file", description="Write a directory of frames as an animated GIF on a palette.")
    ap.add_argument("frames_dir")
    ap.add_argument("output")
    ap.add_argument("--palette", required=True, help="a name in --palettes, #hex,#hex,... or web (the 6x6x6 cube)")
    ap.add_argument("--palettes", help="a JSON file in the lospec list's format")
    ap.add_argument("--method", default=None, choices=pixelize.METHODS, help="default: kd-tree; floyd-steinberg-diffused for web")
    ap.add_argument("--fps", type=float, default=20)
    a = ap.parse_args(argv)
    if a.palette == WEB:
        colors = WEB
    elif a.palette.startswith("#"):
        colors = pixelize.parse_palette(a.palette.split(","))
    else:
        if not a.palettes:
            ap.error("a palette name needs --palettes FILE")
        palettes = pixelize.load_palettes(a.palettes)
        if a.palette not in palettes:
            ap.error(f"no palette {a.palette!r} in {a.palettes}")
        colors = palettes[a.palette]
    from . import video

    video.frames_to_gif(a.frames_dir, a.output, fps=a.fps, palette=colors, method=a.method)
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
