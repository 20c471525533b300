"""The GIF reader of csrc/gif_decode.hip restated in plain Python, with no Pillow inside: the walk over the file, LZW, and the composition
of the clip.  tests/test_gif_decode_host.py pins it to Pillow 12.2 over every file of tests/gif_decode_cases.py; the device tests then
hold the kernels to it.  The rules are numbered as at the top of csrc/gif_decode.hip.

``walk`` is a reader of its own, not gif_file.parse: it takes only what the designed files hold and asserts the rest.
"""
import struct

import numpy as np

OK, TRUNCATED, BAD_CODE, BAD_FIRST, EOI = 0, 1, 2, 3, 4          # ADAIN_GIFD_* of include/adain_gif_decode.h


def walk(data):
    """bytes -> dict(w, h, background, loop, frames=[dict(rect, interlace, code_size, disposal, transparent, delay, table, data)])."""
    assert data[:6] in (b"GIF87a", b"GIF89a")
    w, h, flags, background, _ = struct.unpack_from("<HHBBB", data, 6)
    at = 13
    global_table = None
    if flags & 0x80:
        size = 3 << ((flags & 7) + 1)
        global_table, at = data[at:at + size], at + size
    else:
        background = 0

    def blocks(at):
        out = []
        while data[at]:
            out.append(data[at + 1:at + 1 + data[at]])
            at += 1 + data[at]
        return out, at + 1

    loop, frames, control = None, [], (0, None, 0)
    while data[at] != 0x3B:
        kind = data[at]
        at += 1
        if kind == 0x21:
            label = data[at]
            body, at = blocks(at + 1)
            if label == 0xF9:
                packed, delay, index = struct.unpack("<BHB", body[0])
                control = (packed >> 2 & 7, index if packed & 1 else None, delay)
            elif label == 0xFF and not frames and body[0].startswith(b"NETSCAPE2.0") and len(body) > 1 and len(body[1]) >= 3 and body[1][0] == 1:
                loop = body[1][1] | body[1][2] << 8
            continue
        assert kind == 0x2C, kind
        left, top, fw, fh, fl = struct.unpack_from("<HHHHB", data, at)
        at += 9
        table = global_table
        if fl & 0x80:
            size = 3 << ((fl & 7) + 1)
            table, at = data[at:at + size], at + size
        code_size = data[at]
        body, at = blocks(at + 1)
        frames.append(dict(rect=(left, top, fw, fh), interlace=bool(fl & 0x40), code_size=code_size, disposal=control[0], transparent=control[1],
                           delay=control[2], table=table, data=b"".join(body)))
        control = (0, None, 0)
    return dict(w=w, h=h, background=background, loop=loop, frames=frames)


def unlzw(data, code_size, total):
    """The first ``total`` indices of an LZW stream -> (status, list of indices, codes read).  Strings are kept as strings here, not as
    places in the output: another construction than the kernel's."""
    clear, end = 1 << code_size, (1 << code_size) + 1
    bits = int.from_bytes(data, "little")
    have, at = 8 * len(data), 0
    out, codes = [], 0
    table, width, prev = {}, code_size + 1, None          # prev None: the next code is the first behind a CLEAR, or of the stream
    nxt = clear + 2
    while len(out) < total:
        if at + width > have:
            return TRUNCATED, out, codes
        c = bits >> at & ((1 << width) - 1)
        at += width
        codes += 1
        if c == clear:
            table, width, prev, nxt = {}, code_size + 1, None, clear + 2
            continue
        if c == end:
            return EOI, out, codes
        if prev is None:
            if c > clear:
                return BAD_FIRST, out, codes
            string = [c]
        else:
            if c > nxt:
                return BAD_CODE, out, codes
            if c < clear:
                string = [c]
            elif c == nxt:
                string = prev + [prev[0]]
            else:
                string = table[c]
            if nxt < 4096:
                table[nxt] = prev + [string[0]]
                if nxt == (1 << width) - 1 and width < 12:
                    width += 1
                nxt += 1
        out += string
        prev = string
    return OK, out[:total], codes


def interlaced_rows(h):
    """The screen row of every stored row: rule 6."""
    return [y for start, step in ((0, 8), (4, 8), (2, 4), (1, 2)) for y in range(start, h, step)]


def colour(table, index):
    """Rule 1: a table is padded to 256 entries with zeros."""
    return tuple(table[3 * index:3 * index + 3]) if 3 * index + 3 <= len(table) else (0, 0, 0)


def compose(clip):
    """-> (statuses, frames uint8 [n,H,W,3]); the frames mean something only when every status is OK."""
    H, W = clip["h"], clip["w"]
    canvas = np.zeros((H, W, 3), np.uint8)
    out, statuses = [], []
    method, pending = 0, None                   # pending: (rectangle, what to put there) left by the frame before
    for k, f in enumerate(clip["frames"]):
        left, top, fw, fh = f["rect"]
        status, indices, _ = unlzw(f["data"], f["code_size"], fw * fh)
        statuses.append(status)
        indices = np.asarray(indices + [0] * (fw * fh - len(indices)), np.int64).reshape(fh, fw)
        if f["interlace"]:
            plane = np.zeros_like(indices)
            plane[interlaced_rows(fh)] = indices
            indices = plane
        if pending is not None:                 # rule 3
            (pl, pt, pw, ph), what = pending
            canvas[pt:pt + ph, pl:pl + pw] = what
            pending = None
        if f["disposal"]:
            method = f["disposal"]
        t, table = f["transparent"], f["table"]
        if method == 2:                         # rule 4
            index = t if t is not None else clip["background"]
            if k > 0 and 3 * index + 3 > len(table):
                index = 0
            pending = (f["rect"], np.asarray(colour(table, index), np.uint8))
        elif method == 3:                       # rule 5
            if k > 0:
                pending = (f["rect"], canvas[top:top + fh, left:left + fw].copy())
            elif t is not None:
                pending = (f["rect"], np.asarray(colour(table, t), np.uint8))
        lut = np.zeros((256, 3), np.uint8)
        lut[:len(table) // 3] = np.frombuffer(table, np.uint8).reshape(-1, 3)
        if k == 0:                              # rule 1
            canvas[:] = lut[t if t is not None else 0]
            canvas[top:top + fh, left:left + fw] = lut[indices]
        else:                                   # rule 2
            keep = indices != t if t is not None else np.ones_like(indices, bool)
            region = canvas[top:top + fh, left:left + fw]
            region[keep] = lut[indices][keep]
        out.append(canvas.copy())
    return statuses, np.stack(out)


def decode(data):
    return compose(walk(data))
