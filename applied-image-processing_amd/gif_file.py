"""Animated GIF clips: the file the reference shows its video and pixel-art results as (Style_3DGS/render.py:29-33 ``create_gif``,
Pillow's ``save(save_all=True, duration=, loop=0)``; assets/readme/video/*.gif), written from frames that are already on the device.

A palette clip is at most 256 colours and already indexed on the device (csrc/palette.hip): the index planes are coded there
(csrc/gif.hip, ``runtime.gif_encode_u8``: one record per frame) and only the records cross to the host, which puts the file around them:

    GIF89a | logical screen descriptor: w, h, flags 0x80 | 0x70 | (g - 1) with g = max(1, ceil(log2 K)), background 0, aspect 0
    | global colour table: 3 * 2^g bytes, the palette and then zeros | NETSCAPE2.0 loop extension (more than one frame, or an explicit
    count) | the records, back to back | 3B

The records are not Pillow's bytes: the indices are cut into segments of 2048 pixels that each start with a CLEAR code, so that the
segments are coded side by side (the rules: top of csrc/gif.hip, tests/gif_ref.py); every reader decodes them to the same pixels.  Every
frame is a full frame.

A full-colour clip brings no palette.  ``palette="adaptive"`` chooses one of 256 colours for the whole clip from its frames,
``"adaptive-local"`` one per frame - what Pillow writes for the reference's ``create_gif``, which hands it RGB frames - and
``adaptive(colors, local, refine)`` names either with another count, and with ``refine`` = T rounds of k-means behind the cut
(``"adaptive:N:rT"``; Pillow's ``quantize(kmeans=)`` is the like).  The colours are chosen on the device (csrc/quantize.hip,
csrc/quantize_refine.hip, ``runtime.quantize_palette_u8``: a median cut of its own, not Pillow's palette).  A frame's own table is spliced into its record on the
host: the descriptor's flag byte (offset 17 of the record) becomes 0x80 | (g - 1) and 3 * 2^g table bytes follow it, the palette and then
zeros, g = max(1, ceil(log2 colors)); the header then has no global table (flags 0x70).  Both go with the nearest colour: Pillow's
``convert("P", palette=ADAPTIVE)`` does not dither.

Not built: frame differencing and transparency, interlace.

Reading (``parse``, ``read_gif``): the host walks the file - header, screen, colour tables, extensions, descriptors, the data sub-blocks of
every frame joined - and the device decodes and composes the clip (csrc/gif_decode.hip, ``runtime.gif_decode_u8``): the frames Pillow's
``ImageSequence.Iterator`` + ``convert("RGB")`` gives, pixel for pixel.  Taken: ``GIF87a`` / ``GIF89a``; a screen of 1..65535 a side; a
global table or none; per frame at most one graphic control extension (delay, disposal 0..3, transparent index) and a descriptor whose
rectangle is not empty and lies inside the screen, a local table or none (some table there must be), the interlace flag, a minimum code
size of 2..8, data sub-blocks of any lengths; the NETSCAPE2.0 loop count in front of the first frame; comment, plain-text and unknown
application extensions, skipped; 1..65535 frames; the trailer.  Everything else is refused (``UnsupportedGif``, the reason in words) and
stays with Pillow: a frame that leaves the screen (Pillow grows the screen), no table, code size 1 or above 8, disposal 4..7, a block that
passes the end of the file, a missing trailer, junk between blocks, a second graphic control extension in front of one frame, and a colour
table that is the grey ramp 0, 1, 2, ... (Pillow opens such a frame in mode "L").  The parser never makes a caller fail: every caller
catches ``UnsupportedGif`` and takes Pillow.

Without a GPU the same indices go through Pillow's own ``save(save_all=True)``: other bytes, the same decoded pixels.
"""
import collections
import struct
from dataclasses import dataclass

import numpy as np

from . import pixelize

WEB = "web"          # the 6 x 6 x 6 colour cube, for clips that are not pixel art; it goes with "floyd-steinberg-diffused"
ADAPTIVE = "adaptive"                   # one palette chosen from the whole clip, the global table
ADAPTIVE_LOCAL = "adaptive-local"       # one palette chosen from every frame, a local table each


def web_palette():
    """uint8 [216,3]: every channel one of 0, 51, ..., 255; red slowest."""
    v = np.arange(6, dtype=np.uint8) * 51
    return np.stack(np.meshgrid(v, v, v, indexing="ij"), axis=-1).reshape(-1, 3)


def default_method(palette):
    """The method a caller that names none gets: error diffusion onto the cube, the nearest colour onto a pixel-art palette and onto the
    adaptive ones (Pillow's ``convert("P", palette=ADAPTIVE)`` does not dither)."""
    return "floyd-steinberg-diffused" if isinstance(palette, str) and palette == WEB else "kd-tree"


def adaptive(colors=256, local=False, refine=0):
    """The ``palette`` of a clip that brings none: ``"adaptive"`` / ``"adaptive-local"``, which stand for 256 colours, or with another
    count ``"adaptive:N"`` / ``"adaptive-local:N"``; with ``refine`` = T rounds of k-means behind the median cut (1..64,
    ``runtime.quantize_palette_u8``'s) ``"adaptive:N:rT"`` / ``"adaptive-local:N:rT"``: the count rides in the string, as the colours do."""
    name = ADAPTIVE_LOCAL if local else ADAPTIVE
    if pixelize._refine(refine):
        return f"{name}:{_colors(colors)}:r{int(refine)}"
    return name if _colors(colors) == 256 else f"{name}:{colors}"


def _parse(palette):
    """(local, colors, refine) of ``adaptive``'s strings, None for any other palette; ValueError for a count outside 1..256 or rounds
    outside 0..64."""
    if not isinstance(palette, str):
        return None
    name, _, rest = palette.partition(":")
    count, _, rounds = rest.partition(":")
    if name not in (ADAPTIVE, ADAPTIVE_LOCAL) or (count and not count.isdigit()):
        return None
    if rounds and not (count and rounds[0] == "r" and rounds[1:].isdigit()):
        return None
    return name == ADAPTIVE_LOCAL, _colors(int(count)) if count else 256, pixelize._refine(int(rounds[1:])) if rounds else 0


def parse_adaptive(palette):
    """(local, colors) of ``adaptive``'s strings, None for any other palette; ValueError for a count outside 1..256."""
    chosen = _parse(palette)
    return None if chosen is None else chosen[:2]


def parse_refine(palette):
    """The rounds T of ``adaptive``'s ``":rT"`` strings, 0 for the strings without and for any other palette."""
    chosen = _parse(palette)
    return 0 if chosen is None else chosen[2]


def is_adaptive(palette):
    return parse_adaptive(palette) is not None


def check_palette(palette):
    """ValueError for a palette ``write_gif`` would refuse."""
    if not is_adaptive(palette):
        header((1, 1), palette)


def _colors(colors):
    if isinstance(colors, bool) or not isinstance(colors, (int, np.integer)) or not 1 <= colors <= 256:
        raise ValueError(f"gif: colors must be an int in 1..256, got {colors!r}")
    return int(colors)


def table_bits(colors):
    """g: a colour table of 2^g entries holds ``colors`` of them, g = max(1, ceil(log2 colors))."""
    g = 1
    while (1 << g) < colors:
        g += 1
    return g


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
    forms or uint8 [K,3]), or None for a file without a global table (flags 0x70: every record brings its own, ``local_records``);
    ``loop``: None for no NETSCAPE2.0 extension, or the loop count (0: for ever)."""
    pal = None if palette is None else _palette(palette)
    w, h = (_u16(v, "a frame side") for v in size)
    if w < 1 or h < 1:
        raise ValueError(f"gif: an empty frame {size!r}")
    if pal is None:
        out = b"GIF89a" + struct.pack("<HHBBB", w, h, 0x70, 0, 0)
    else:
        g = table_bits(len(pal))
        out = b"GIF89a" + struct.pack("<HHBBB", w, h, 0x80 | 0x70 | (g - 1), 0, 0) + pal.tobytes() + bytes(3 * ((1 << g) - len(pal)))
    if loop is not None:
        out += b"\x21\xff\x0bNETSCAPE2.0\x03\x01" + struct.pack("<H", _u16(loop, "loop")) + b"\x00"
    return out


FLAGS_AT = 17          # of a record: 8 bytes of graphic control extension, then 2C, left, top, width, height and the flag byte


def records_bytes(records, lengths, tables=None, colors=None):
    """The records of a ``runtime.gif_encode_u8`` result back to back: the lengths first, then only the bytes that are records (waits for
    the device).  ValueError for a frame the device refused (length 0: an index that is not below K).  ``tables``: per frame its own
    colours uint8 [k,3], k <= ``colors``, spliced in as a local table of 2^g entries, g = ``table_bits(colors)``: the flag byte becomes
    0x80 | (g - 1) and the table - the colours, then zeros - follows it."""
    ln = [int(v) for v in (lengths.cpu().tolist() if hasattr(lengths, "cpu") else np.asarray(lengths).tolist())]
    bad = [i for i, k in enumerate(ln) if k <= 0]
    if bad:
        raise ValueError(f"gif: frame(s) {bad} hold an index that is not below the palette's size")
    rows = records[:, :max(ln)]
    rows = rows.cpu().numpy() if hasattr(rows, "cpu") else np.asarray(rows)
    if tables is None:
        return b"".join(rows[i, :k].tobytes() for i, k in enumerate(ln))
    g = table_bits(colors)
    parts = []
    for i, k in enumerate(ln):
        rec, pal = rows[i, :k].tobytes(), np.ascontiguousarray(tables[i], dtype=np.uint8)
        parts += [rec[:FLAGS_AT], bytes([0x80 | (g - 1)]), pal.tobytes(), bytes(3 * ((1 << g) - len(pal))), rec[FLAGS_AT + 1:]]
    return b"".join(parts)


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


def _write_adaptive(frames, path, local, colors, refine, delay, method, loop, step):
    """``write_gif`` for the two adaptive palettes: the colours come from the frames (``pixelize.quantize_palettes``: on the device when
    there is one; ``refine`` rounds of k-means), a frame is indexed onto its palette's ``used`` colours and coded with K = ``colors``."""
    n, h, w, _ = frames.shape
    pals, used = pixelize.quantize_palettes(frames, colors, per_frame=local, device=None if _cuda(frames) is not None else "cpu", refine=refine)
    tables = [pals[i, :u] for i, u in enumerate(used)]          # one, or one per frame
    if _cuda(frames) is None:
        from PIL import Image

        images = []
        for i in range(n):
            pal = tables[i if local else 0]
            im = Image.frombytes("P", (w, h), index_planes(frames[i:i + 1], pal, method)[0].tobytes())
            im.putpalette(pal.tobytes())
            images.append(im)
        extra = {} if loop is None else {"loop": loop}
        images[0].save(path, format="GIF", save_all=True, append_images=images[1:], duration=delay * 10, disposal=1, optimize=False, **extra)
        return path
    from . import runtime as rt
    import torch

    parts = [header((w, h), None if local else tables[0], loop)]
    pending = None
    for i in range(0, n, step):
        block = frames[i:i + step]
        if local:          # a palette each: a map per frame, one coding call for the block
            idx = torch.stack([index_planes(block[j:j + 1], tables[i + j], method)[0] for j in range(len(block))])
        else:
            idx = index_planes(block, tables[0], method)
        coded = rt.gif_encode_u8(idx, colors, delay) + ((tables[i:i + len(block)], colors) if local else ())
        if pending is not None:
            parts.append(records_bytes(*pending))
        pending = coded
    parts.append(records_bytes(*pending))
    parts.append(b"\x3b")
    with open(path, "wb") as f:
        f.write(b"".join(parts))
    return path


def write_gif(frames, path, palette, fps=20, method="kd-tree", loop=0, sub_batch=None):
    """``frames`` - uint8 [N,h,w,3], a GPU tensor or a NumPy array - as an animated GIF at ``path``: mapped (``method`` "rgb", "kd-tree",
    "floyd-steinberg") or dithered ("floyd-steinberg-diffused"; None: ``default_method``) onto ``palette`` (``header``'s forms), ``round(100 / fps)`` centiseconds a
    frame, ``loop`` times (0: for ever; None: no loop extension for a single frame).  With a GPU the frames are indexed and coded there,
    ``sub_batch`` frames to a call (default: about 32 MiB of pixels), and only the records are downloaded; without one Pillow writes the
    same indices.  ``palette="adaptive"``: at most 256 colours chosen from the whole clip, the global table; ``"adaptive-local"``: chosen
    from every frame, a local table each (the module's text); ``adaptive(colors, local, refine)`` names another count and rounds of
    k-means behind the median cut.  Returns ``path``."""
    chosen = _parse(palette)
    pal = None if chosen else _palette(palette)
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
    if chosen:
        return _write_adaptive(frames, path, *chosen, delay, method, loop, step)
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


# ---- reading -------------------------------------------------------------------------------------------------------------------------
MAX_FRAMES = 65535
DEFAULT_FPS = 20                       # ``write_gif``'s default, and ``clip_fps``'s answer for a clip of zero delays

# durations: milliseconds per frame, as Pillow's ``info["duration"]`` (0 for a frame without a graphic control extension); loop: the
# NETSCAPE2.0 count (0: for ever) or None for a file without one; size: (w, h) of the screen
GifInfo = collections.namedtuple("GifInfo", "durations loop size")


class UnsupportedGif(Exception):
    """The file is not one the device decoder takes; str(e) says why.  Callers fall back to Pillow."""


@dataclass
class GifFrame:
    left: int
    top: int
    w: int
    h: int
    interlace: bool
    code_size: int              # the minimum code size, 2..8
    disposal: int               # 0..3, as the file has it (0 inherits the method in force: csrc/gif_decode.hip, rule 3)
    transparent: object         # the transparent index, or None
    delay_cs: int               # centiseconds; 0 without a graphic control extension
    table: bytes                # the frame's colour table, its own or the global one: 3 bytes an entry
    local: bool                 # the table is the frame's own
    data: bytes                 # the LZW data: the sub-blocks joined


@dataclass
class GifClip:
    w: int
    h: int
    background: int             # the screen's background index; 0 in a file without a global table, as Pillow has it
    loop: object                # the NETSCAPE2.0 count, or None
    frames: list

    @property
    def durations(self):
        return [10 * f.delay_cs for f in self.frames]

    @property
    def info(self):
        return GifInfo(self.durations, self.loop, (self.w, self.h))


def _grey_ramp(table):
    return all(table[3 * i] == table[3 * i + 1] == table[3 * i + 2] == i for i in range(len(table) // 3))


def _blocks(data, at, what):
    """The sub-blocks from ``at`` on -> (their list, the offset behind the terminator)."""
    out = []
    while True:
        if at >= len(data):
            raise UnsupportedGif(f"{what}: a block that passes the end of the file")
        size = data[at]
        at += 1
        if size == 0:
            return out, at
        if at + size > len(data):
            raise UnsupportedGif(f"{what}: a block that passes the end of the file")
        out.append(data[at:at + size])
        at += size


def parse(data):
    """bytes of a file -> GifClip, or UnsupportedGif (the module's text lists what is taken)."""
    data = bytes(data)
    n = len(data)
    if data[:6] not in (b"GIF87a", b"GIF89a"):
        raise UnsupportedGif("not a GIF file (no signature)")
    if n < 13:
        raise UnsupportedGif("truncated inside the logical screen descriptor")
    w, h, flags, background, _ = struct.unpack_from("<HHBBB", data, 6)
    if w < 1 or h < 1:
        raise UnsupportedGif(f"an empty screen ({w} x {h})")
    at = 13
    global_table = None
    if flags & 0x80:
        size = 3 << ((flags & 7) + 1)
        if at + size > n:
            raise UnsupportedGif("the global colour table passes the end of the file")
        global_table = data[at:at + size]
        at += size
        if _grey_ramp(global_table):
            raise UnsupportedGif("a global colour table that is the grey ramp (Pillow opens it in mode L)")
    else:
        background = 0
    loop, frames, control = None, [], None
    while True:
        if at >= n:
            raise UnsupportedGif("no trailer")
        kind = data[at]
        at += 1
        if kind == 0x3B:
            break
        if kind == 0x21:
            if at >= n:
                raise UnsupportedGif("truncated inside an extension")
            label = data[at]
            blocks, at = _blocks(data, at + 1, f"extension {label:#04x}")
            if label == 0xF9:
                if control is not None:
                    raise UnsupportedGif("two graphic control extensions in front of one frame")
                if len(blocks) != 1 or len(blocks[0]) != 4:
                    raise UnsupportedGif("a graphic control extension that is not one block of 4 bytes")
                packed, delay, index = struct.unpack("<BHB", blocks[0])
                disposal = packed >> 2 & 7
                if disposal > 3:
                    raise UnsupportedGif(f"disposal method {disposal}")
                control = (disposal, index if packed & 1 else None, delay)
            elif label == 0xFF and not frames and blocks and blocks[0].startswith(b"NETSCAPE2.0"):
                if len(blocks) > 1 and len(blocks[1]) >= 3 and blocks[1][0] == 1:
                    loop = blocks[1][1] | blocks[1][2] << 8
            continue                    # comment, plain text, other applications: skipped
        if kind != 0x2C:
            raise UnsupportedGif(f"byte {kind:#04x} at {at - 1} where a block should start")
        if at + 9 > n:
            raise UnsupportedGif("truncated inside an image descriptor")
        left, top, fw, fh, fl = struct.unpack_from("<HHHHB", data, at)
        at += 9
        k = len(frames)
        if fw < 1 or fh < 1:
            raise UnsupportedGif(f"frame {k}: an empty rectangle")
        if left + fw > w or top + fh > h:
            raise UnsupportedGif(f"frame {k}: the rectangle {fw} x {fh} at ({left}, {top}) leaves the {w} x {h} screen")
        if fw * fh >= 1 << 31:
            raise UnsupportedGif(f"frame {k}: 2^31 pixels or more")
        table, local = global_table, False
        if fl & 0x80:
            size = 3 << ((fl & 7) + 1)
            if at + size > n:
                raise UnsupportedGif(f"frame {k}: the local colour table passes the end of the file")
            table, local = data[at:at + size], True
            at += size
            if _grey_ramp(table):
                raise UnsupportedGif(f"frame {k}: a local colour table that is the grey ramp (Pillow opens it in mode L)")
        if table is None:
            raise UnsupportedGif(f"frame {k}: no colour table, neither its own nor a global one")
        if at >= n:
            raise UnsupportedGif(f"frame {k}: truncated in front of the code size")
        code_size = data[at]
        if not 2 <= code_size <= 8:
            raise UnsupportedGif(f"frame {k}: minimum code size {code_size}")
        blocks, at = _blocks(data, at + 1, f"frame {k}")
        if k >= MAX_FRAMES:
            raise UnsupportedGif(f"more than {MAX_FRAMES} frames")
        disposal, transparent, delay = control if control is not None else (0, None, 0)
        control = None
        frames.append(GifFrame(left, top, fw, fh, bool(fl & 0x40), code_size, disposal, transparent, delay, table, local, b"".join(blocks)))
    if not frames:
        raise UnsupportedGif("no frames")
    return GifClip(w, h, background, loop, frames)


def pil_clip(data):
    """Pillow's clip: (uint8 [n,H,W,3] array, GifInfo); its exceptions pass through."""
    import io

    from PIL import Image, ImageSequence

    im = Image.open(io.BytesIO(bytes(data)))
    frames, durations = [], []
    for f in ImageSequence.Iterator(im):
        frames.append(np.asarray(f.convert("RGB")))
        durations.append(f.info.get("duration", 0))
    return np.stack(frames), GifInfo(durations, im.info.get("loop"), im.size)


def read_gif(path_or_bytes, device=None):
    """The counterpart of ``write_gif``: a file's path or its bytes -> (frames uint8 [n,H,W,3], GifInfo).  With a GPU the clip is decoded
    there (``runtime.gif_decode_u8``; ``device``: default the current one) and the frames are a tensor on it; without one, or with
    ``device="cpu"``, Pillow decodes and the same frames come as a NumPy array."""
    if isinstance(path_or_bytes, (bytes, bytearray, memoryview)):
        data = bytes(path_or_bytes)
    else:
        with open(str(path_or_bytes), "rb") as f:
            data = f.read()
    import torch

    if str(device) == "cpu" or not torch.cuda.is_available():
        return pil_clip(data)
    from . import runtime as rt
    return rt.gif_decode_u8(data, device)


def clip_fps(info):
    """The frames per second ``write_gif`` would give the clip's pace back with: 100 / round(mean delay in centiseconds);
    ``DEFAULT_FPS`` for a clip of zero delays."""
    durations = list(info.durations)
    cs = int(round(sum(durations) / (10 * len(durations)))) if durations else 0
    return 100 / cs if cs > 0 else float(DEFAULT_FPS)


def main(argv=None):
    import argparse

    ap = argparse.ArgumentParser(prog="python -m applied_image_processing_amd.gif_file", description="Write a directory of frames as an animated GIF on a palette.")
    ap.add_argument("frames_dir", help="the directory of frames; with --extract the GIF to read")
    ap.add_argument("output", help="the GIF to write; with --extract the directory the frames go to")
    ap.add_argument("--extract", action="store_true", help="the other way round: write the frames of the GIF FRAMES_DIR into the directory OUTPUT "
                    "as frame_0000.png, ... (video.gif_to_frames)")
    ap.add_argument("--palette", help="a name in --palettes, #hex,#hex,..., web (the 6x6x6 cube), adaptive (--colors colours chosen from "
                    "the clip) or adaptive-local (chosen from every frame, a local colour table each)")
    ap.add_argument("--colors", type=int, default=256, help="the colours of --palette adaptive / adaptive-local, 1..256 (default 256)")
    ap.add_argument("--refine", type=int, default=0, metavar="T", help="rounds of k-means behind the median cut of --palette adaptive / adaptive-local, 0..64 (default 0)")
    ap.add_argument("--palettes", help="a JSON file in the lospec list's format")
    ap.add_argument("--method", default=None, choices=pixelize.METHODS, help="default: kd-tree; floyd-steinberg-diffused for web")
    ap.add_argument("--fps", type=float, default=20)
    a = ap.parse_args(argv)
    if a.extract:
        from . import video

        info = video.gif_to_frames(a.frames_dir, a.output)
        print(f"{len(info.durations)} frames of {info.size[0]} x {info.size[1]}, {clip_fps(info):g} fps")
        return 0
    if a.palette is None:
        ap.error("the following arguments are required: --palette")
    if a.palette in (ADAPTIVE, ADAPTIVE_LOCAL):
        if not 1 <= a.colors <= 256:
            ap.error("--colors must be in 1..256")
        if not 0 <= a.refine <= pixelize.REFINE_MAX:
            ap.error(f"--refine must be in 0..{pixelize.REFINE_MAX}")
        colors = adaptive(a.colors, a.palette == ADAPTIVE_LOCAL, a.refine)
    elif a.palette == WEB:
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
