"""Designed GIF files for the reader (csrc/gif_decode.hip, gif_file.parse): built by a small writer of their own that places chosen codes,
not by Pillow's encoder, so that each thing a case is named for is certain to occur.  ``CASES``: name -> bytes of files Pillow loads;
``DAMAGED``: name -> (bytes, the status the decoder must report); ``REFUSED``: name -> (bytes, a word of gif_file.parse's reason);
``pillow_clips()``: the committed clips Pillow's own encoder made (tests/golden/gif_decode/, written by ``python tests/gif_decode_cases.py``).
"""
import itertools
import os
import struct

import numpy as np

import gif_decode_ref as R
import gif_ref

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "gif_decode")


class Coder:
    """Places codes at the widths a decoder reads them with: it follows the decoder's table count, nothing else."""

    def __init__(self, m):
        self.m, self.clear, self.end = m, 1 << m, (1 << m) + 1
        self.width, self.next, self.fresh = m + 1, self.clear + 2, True
        self.codes = []

    def emit(self, c):
        self.codes.append((c, self.width))
        if c == self.clear:
            self.width, self.next, self.fresh = self.m + 1, self.clear + 2, True
        elif c == self.end:
            pass
        elif self.fresh:
            self.fresh = False
        elif self.next < 4096:
            if self.next == (1 << self.width) - 1 and self.width < 12:
                self.width += 1
            self.next += 1
        return self

    def data(self):
        return gif_ref.pack(self.codes)


def greedy(indices, m, leading_clear=True, at_full="defer", eoi=True):
    """Greedy LZW over the whole frame.  at_full: "defer" - the table fills and is never cleared, "clear" - CLEAR the moment it fills."""
    px = [int(v) for v in np.asarray(indices).reshape(-1)]
    co = Coder(m)
    if leading_clear:
        co.emit(co.clear)
    table, nxt, cur = {}, co.clear + 2, px[0]
    for v in px[1:]:
        hit = table.get((cur, v))
        if hit is not None:
            cur = hit
            continue
        co.emit(cur)
        if nxt < 4096:
            table[(cur, v)] = nxt
            nxt += 1
        if nxt == 4096 and at_full == "clear":
            co.emit(co.clear)
            table, nxt = {}, co.clear + 2
        cur = v
    co.emit(cur)
    if eoi:
        co.emit(co.end)
    return co


def sub_blocks(data, size=255):
    out = bytearray()
    for i in range(0, len(data), size):
        out += bytes([len(data[i:i + size])]) + data[i:i + size]
    return bytes(out) + b"\0"


def table_of(colours, entries=None):
    colours = np.asarray(colours, np.uint8).reshape(-1, 3)
    g = gif_ref.table_bits(entries or len(colours))
    return colours.tobytes() + bytes(3 * ((1 << g) - len(colours)))


def frame(indices, m=None, rect=None, gce=None, local=None, interlace=False, data=None, block=255, **lzw):
    """One frame's bytes.  indices [h,w]; gce: (disposal, transparent index or None, delay) or None for no extension; local: a table's
    bytes; data: LZW bytes instead of ``greedy(indices, m, **lzw)``."""
    indices = np.asarray(indices)
    h, w = indices.shape
    left, top = rect or (0, 0)
    if m is None:
        m = max(2, int(indices.max()).bit_length())
    stored = indices[R.interlaced_rows(h)] if interlace else indices
    out = b""
    if gce is not None:
        disposal, t, delay = gce
        out += b"\x21\xf9\x04" + struct.pack("<BHB", disposal << 2 | (t is not None), delay, t or 0) + b"\0"
    flags = (0x40 if interlace else 0) | ((0x80 | (len(local) // 3).bit_length() - 2) if local else 0)
    out += b"\x2c" + struct.pack("<HHHHB", left, top, w, h, flags) + (local or b"")
    return out + bytes([m]) + sub_blocks(greedy(stored, m, **lzw).data() if data is None else data, block)


def gif(size, table, frames, background=0, loop=None, version=b"GIF89a", extras=b""):
    """size: (w, h); table: the global table's bytes or None."""
    flags = 0x70 | ((0x80 | (len(table) // 3).bit_length() - 2) if table else 0)
    out = version + struct.pack("<HHBBB", size[0], size[1], flags, background, 0) + (table or b"")
    if loop is not None:
        out += b"\x21\xff\x0bNETSCAPE2.0\x03\x01" + struct.pack("<H", loop) + b"\0"
    return out + extras + b"".join(frames) + b"\x3b"


def _rng(seed):
    return np.random.default_rng(seed)


def _colours(k, seed=1):
    c = _rng(seed).integers(0, 256, (k, 3))
    c[0] = (11, 22, 33)          # never the grey ramp's first entry
    return c


def build():
    cases = {}
    pal4, pal256 = table_of(_colours(4)), table_of(_colours(256))
    cases["1x1"] = gif((1, 1), pal4, [frame([[3]], 2)])
    for m in range(2, 9):
        cases[f"code_size_{m}_5x7"] = gif((5, 7), table_of(_colours(1 << m)), [frame(_rng(m).integers(0, 1 << m, (7, 5)), m)])
    # every pixel its own root: the width steps at each power of two up to 12 bits, then the full table
    cases["width_steps_roots"] = gif((90, 50), pal4, [frame(np.arange(4500).reshape(50, 90) % 3 + (np.arange(4500).reshape(50, 90) % 7 == 0), 2,
                                                            data=_roots(np.arange(4500) % 3 + (np.arange(4500) % 7 == 0), 2))])
    cases["one_colour_64x3"] = gif((64, 3), pal4, [frame(np.full((3, 64), 1), 2)])
    cases["one_colour_70x70"] = gif((70, 70), pal4, [frame(np.full((70, 70), 2), 2)])
    noise = _rng(7).integers(0, 256, (80, 96))
    cases["table_full_deferred"] = gif((96, 80), pal256, [frame(noise, 8)])
    cases["table_full_no_leading_clear"] = gif((96, 80), pal256, [frame(noise, 8, leading_clear=False)])
    cases["table_full_clear_when_full"] = gif((96, 80), pal256, [frame(noise, 8, at_full="clear")])
    for K in (2, 8, 256):
        own = _rng(K).integers(0, K, (3, 41, 50))
        cases[f"own_records_K{K}"] = gif_ref.file(own, _colours(K), 5)
    # data that ends at the edges of the sub-blocks (zeros behind the end code, which nobody reads), and other block sizes
    base = greedy(_rng(3).integers(0, 16, (12, 20)), 4).data()
    for length in (254, 255, 256, 510):
        assert len(base) <= 254
        cases[f"data_length_{length}"] = gif((20, 12), table_of(_colours(16)), [frame(np.zeros((12, 20), int), 4, data=base + bytes(length - len(base)))])
    for block in (1, 7):
        cases[f"sub_blocks_of_{block}"] = gif((20, 12), table_of(_colours(16)), [frame(_rng(3).integers(0, 16, (12, 20)), 4, block=block)])
    extra = greedy(_rng(4).integers(0, 4, (5, 6)), 2, eoi=False)
    for c in (1, 2, 3, 300 & 7, extra.end):          # codes behind the last pixel, a wild one among them
        extra.emit(c)
    cases["excess_data"] = gif((6, 5), pal4, [frame(np.zeros((5, 6), int), 2, data=extra.data() + b"\xff\xff")])
    # rectangles
    back = _rng(5).integers(0, 4, (9, 11))
    for name, rect, hw in (("top_left", (0, 0), (3, 4)), ("top_right", (7, 0), (3, 4)), ("bottom_left", (0, 6), (3, 4)), ("bottom_right", (7, 6), (3, 4)),
                           ("1x1_inside", (5, 4), (1, 1)), ("1x1_corner", (10, 8), (1, 1)), ("whole_screen", (0, 0), (9, 11))):
        cases[f"rect_{name}"] = gif((11, 9), pal4, [frame(back, 2, gce=(1, None, 4)), frame(_rng(6).integers(0, 4, hw), 2, rect=rect, gce=(1, None, 4))])
    cases["frame0_smaller_than_screen"] = gif((11, 9), pal4, [frame(_rng(6).integers(1, 4, (3, 4)), 2, rect=(2, 3))])
    cases["frame0_smaller_transparent"] = gif((11, 9), pal4, [frame(_rng(6).integers(0, 4, (3, 4)), 2, rect=(2, 3), gce=(0, 2, 0)),
                                                              frame(_rng(8).integers(0, 4, (5, 5)), 2, rect=(1, 1), gce=(0, 2, 0))])
    cases["transparency_frame0"] = gif((6, 5), pal4, [frame(_rng(9).integers(0, 4, (5, 6)), 2, gce=(1, 1, 3)), frame(_rng(10).integers(0, 4, (5, 6)), 2, gce=(1, None, 3))])
    cases["transparency_later"] = gif((6, 5), pal4, [frame(_rng(9).integers(0, 4, (5, 6)), 2, gce=(1, None, 3))]
                                      + [frame(_rng(10 + i).integers(0, 4, (4, 4)), 2, rect=(i, 1), gce=(1, i, 3)) for i in (1, 2)])
    cases["transparent_index_beyond_table"] = gif((6, 5), table_of(_colours(2)), [frame(_rng(9).integers(0, 2, (5, 6)), 2, gce=(2, None, 3)),
                                                                                 frame(_rng(10).integers(0, 4, (4, 4)), 2, rect=(1, 1), gce=(2, 3, 3)),
                                                                                 frame(_rng(11).integers(0, 2, (2, 2)), 2, rect=(0, 0), gce=(1, None, 3))])
    # disposal: every method on every position of a 4-frame clip, with and without a transparent index
    rects = [((0, 0), (5, 6)), ((1, 1), (3, 3)), ((2, 0), (4, 3)), ((0, 2), (3, 5))]
    for keyed in (False, True):
        for ds in itertools.product(range(4), repeat=4):
            frames = [frame(_rng(20 + i).integers(0, 4, hw), 2, rect=at, gce=(d, (i + 1) % 4 if keyed else None, 2)) for i, ((at, hw), d) in enumerate(zip(rects, ds))]
            cases[f"disposal_{''.join(map(str, ds))}{'_keyed' if keyed else ''}"] = gif((6, 5), pal4, frames, background=2)
    cases["disposal_3_after_3"] = gif((6, 5), pal4, [frame(_rng(30).integers(0, 4, (5, 6)), 2, gce=(1, None, 2))]
                                      + [frame(_rng(31 + i).integers(0, 4, (3, 3)), 2, rect=(i, i), gce=(3, None, 2)) for i in range(3)])
    cases["disposal_3_on_frame0_keyed_small"] = gif((6, 5), pal4, [frame(_rng(30).integers(0, 4, (3, 3)), 2, rect=(1, 1), gce=(3, 1, 2)),
                                                                 frame(_rng(31).integers(0, 4, (2, 2)), 2, rect=(0, 0), gce=(1, None, 2))])
    for bg in (1, 5, 255):                   # 5 and 255: at or beyond the 4 entries of the table
        cases[f"disposal_2_background_{bg}"] = gif((6, 5), pal4, [frame(_rng(30).integers(0, 4, (3, 3)), 2, rect=(1, 1), gce=(2, None, 2)),
                                                                   frame(_rng(31).integers(0, 4, (2, 2)), 2, rect=(3, 2), gce=(2, None, 2)),
                                                                   frame(_rng(32).integers(0, 4, (2, 2)), 2, rect=(0, 0), gce=(1, None, 2))], background=bg)
    cases["no_gce_inherits_disposal"] = gif((6, 5), pal4, [frame(_rng(30).integers(0, 4, (5, 6)), 2, gce=(2, None, 2)), frame(_rng(31).integers(0, 4, (2, 2)), 2, rect=(1, 1)),
                                                           frame(_rng(32).integers(0, 4, (2, 2)), 2, rect=(3, 3))], background=3)
    for h in list(range(1, 10)) + [17]:
        cases[f"interlaced_h{h}"] = gif((7, h), table_of(_colours(16)), [frame(_rng(40 + h).integers(0, 16, (h, 7)), 4, interlace=True)])
    cases["interlaced_later_frame"] = gif((7, 9), table_of(_colours(16)), [frame(_rng(50).integers(0, 16, (9, 7)), 4),
                                                                          frame(_rng(51).integers(0, 16, (6, 5)), 4, rect=(1, 2), gce=(1, 3, 1), interlace=True)])
    local2, local256 = table_of(_colours(2, 2)), table_of(_colours(256, 3))
    cases["local_tables"] = gif((6, 5), pal4, [frame(_rng(60).integers(0, 2, (5, 6)), 2, local=local2, gce=(2, None, 1)), frame(_rng(61).integers(0, 256, (4, 4)), 8, rect=(1, 1), local=local256, gce=(2, 200, 1)),
                                               frame(_rng(62).integers(0, 4, (3, 3)), 2, rect=(0, 0), gce=(1, None, 1))], background=3)
    cases["no_global_table"] = gif((6, 5), None, [frame(_rng(60).integers(0, 2, (5, 6)), 2, local=local2, gce=(2, None, 1)),
                                                  frame(_rng(61).integers(0, 256, (4, 4)), 8, rect=(1, 1), local=local256, gce=(1, None, 1))], background=1)
    cases["zero_delays"] = gif((6, 5), pal4, [frame(_rng(70 + i).integers(0, 4, (5, 6)), 2, gce=(1, None, 0)) for i in range(3)])
    for loop in (None, 0, 3):
        cases[f"loop_{loop}"] = gif((6, 5), pal4, [frame(_rng(70 + i).integers(0, 4, (5, 6)), 2, gce=(1, None, 7)) for i in range(2)], loop=loop)
    cases["gif87a_and_skipped_extensions"] = gif((6, 5), pal4, [frame(_rng(70).integers(0, 4, (5, 6)), 2), b"\x21\xfe\x05hello\0",
                                                                b"\x21\x01\x0c" + bytes(12) + b"\x02hi\0", b"\x21\xff\x0bUNKNOWN_1.0\x02ab\0",
                                                                frame(_rng(71).integers(0, 4, (5, 6)), 2, gce=(1, None, 9))], version=b"GIF87a")
    return cases


def _roots(px, m):
    co = Coder(m).emit(1 << m)
    for v in px:
        co.emit(int(v))
    return co.emit(co.end).data()


def build_damaged():
    pal256, pal4 = table_of(_colours(256)), table_of(_colours(4))
    noise = _rng(7).integers(0, 256, (80, 96))
    whole = greedy(noise, 8).data()
    out = {"cut_at_1000_bytes": (gif((96, 80), pal256, [frame(noise, 8, data=whole[:1000])]), R.TRUNCATED)}
    co = Coder(2).emit(4).emit(1).emit(2)                     # 9 bits: the third code needs the second byte, which is cut
    out["cut_inside_a_code"] = (gif((6, 5), pal4, [frame(np.zeros((5, 6), int), 2, data=co.data()[:1])]), R.TRUNCATED)
    co = Coder(8).emit(256).emit(1).emit(2).emit(300)
    for _ in range(40):
        co.emit(3)
    out["code_300_as_the_third"] = (gif((6, 5), pal256, [frame(np.zeros((5, 6), int), 8, data=co.emit(co.end).data())]), R.BAD_CODE)
    co = Coder(2).emit(4).emit(1).emit(2).emit(4).emit(6)
    for _ in range(40):
        co.emit(3)
    out["non_root_behind_a_clear"] = (gif((6, 5), pal4, [frame(np.zeros((5, 6), int), 2, data=co.emit(co.end).data())]), R.BAD_FIRST)
    out["eoi_before_the_rectangle_is_full"] = (gif((6, 5), pal4, [frame(np.zeros((5, 6), int), 2, data=greedy(np.ones((4, 6), int), 2).data())]), R.EOI)
    return out


def build_refused():
    pal4 = table_of(_colours(4))
    ok = frame(np.ones((5, 6), int), 2)
    grey = bytes(v for i in range(4) for v in (i, i, i))
    return {
        "frame_outside_the_screen": (gif((6, 5), pal4, [frame(np.ones((5, 6), int), 2, rect=(1, 0))]), "leaves"),
        "no_table": (gif((6, 5), None, [ok]), "no colour table"),
        "code_size_1": (gif((6, 5), pal4, [ok[:10] + b"\x01" + ok[11:]]), "code size 1"),
        "code_size_9": (gif((6, 5), pal4, [ok[:10] + b"\x09" + ok[11:]]), "code size 9"),
        "disposal_5": (gif((6, 5), pal4, [frame(np.ones((5, 6), int), 2, gce=(5, None, 1))]), "disposal method 5"),
        "block_passes_the_end": (gif((6, 5), pal4, [ok])[:-4], "passes the end"),
        "no_trailer": (gif((6, 5), pal4, [ok])[:-1], "no trailer"),
        "empty_rectangle": (gif((6, 5), pal4, [b"\x2c" + struct.pack("<HHHHB", 0, 0, 0, 5, 0) + ok[10:]]), "empty rectangle"),
        "grey_ramp_table": (gif((6, 5), grey, [ok]), "grey ramp"),
        "not_a_gif": (b"\x89PNG\r\n\x1a\n" + bytes(20), "signature"),
        "no_frames": (gif((6, 5), pal4, []), "no frames"),
        "two_graphic_controls": (gif((6, 5), pal4, [b"\x21\xf9\x04\x04\x01\x00\x00\x00" + frame(np.ones((5, 6), int), 2, gce=(1, None, 1))]), "two graphic control"),
    }


def make_pillow_clips():
    """The clips Pillow's own encoder writes for a 50 x 40 six-frame clip with a moving block: sub-rectangles, and transparency where it helps."""
    import io

    from PIL import Image

    out = {}
    rng = _rng(99)
    back = rng.integers(0, 256, (40, 50, 3)).astype(np.uint8) // 64 * 64
    for d in range(4):
        frames = []
        for i in range(6):
            a = back.copy()
            a[5 + 4 * i:15 + 4 * i, 3 + 6 * i:15 + 6 * i] = (250, 10 + 40 * i, 30)
            frames.append(Image.fromarray(a).quantize(32) if i == 0 else Image.fromarray(a).quantize(palette=frames[0]))          # one palette: the frames differ in the block alone
        buf = io.BytesIO()
        frames[0].save(buf, format="GIF", save_all=True, append_images=frames[1:], optimize=True, disposal=d, duration=[30, 40, 50, 60, 70, 80], loop=2)
        out[f"pillow_disposal_{d}"] = buf.getvalue()
    return out


def pillow_clips():
    return {name[:-4]: open(os.path.join(GOLDEN, name), "rb").read() for name in sorted(os.listdir(GOLDEN)) if name.endswith(".gif")}


CASES = build()
DAMAGED = build_damaged()
REFUSED = build_refused()


if __name__ == "__main__":
    os.makedirs(GOLDEN, exist_ok=True)
    for name, data in make_pillow_clips().items():
        with open(os.path.join(GOLDEN, name + ".gif"), "wb") as f:
            f.write(data)
        print(name, len(data))
