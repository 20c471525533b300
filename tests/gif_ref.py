"""The GIF writer of csrc/gif.hip and gif_file.py restated in plain Python: the frame record and the file around the records.

The record of one frame - a function of its indices, K and the delay alone:
  GCE        : 21 F9 04 04 dl dh 00 00 - disposal 1, no transparency, the delay in centiseconds, little endian.
  descriptor : 2C 00 00 00 00 wl wh hl hh 00 - the full frame, no local table, not interlaced.
  code size  : m = max(2, ceil(log2 K)); CLEAR = 2^m, EOI = CLEAR + 1, the first dictionary code is CLEAR + 2.
  segments   : the h w indices in raster order, SEGMENT = 2048 to a segment, the last one may be shorter.  A segment is CLEAR, then
               plain greedy LZW from an empty dictionary: the longest known string, one new entry per emitted code except the segment's
               last.  EOI behind the last segment's codes.
  widths     : the k-th code behind a CLEAR (k = 1, 2, ...) has w(k) bits, the smallest w >= m + 1 with 2^m + 1 + k <= 2^w.  A segment
               of c codes is closed by the next CLEAR, or by EOI, as its code number c + 1 with w(c + 1) bits; the frame's first CLEAR
               has m + 1.
  packing    : codes LSB first, the last byte zero-padded; the data bytes in sub-blocks of 255, each behind its length byte, the last
               one may be shorter; a 00 terminator.
The file: GIF89a; the logical screen descriptor w, h, flags 0x80 | 0x70 | (g - 1) with g = max(1, ceil(log2 K)), background 0, aspect
0; the global colour table, 3 * 2^g bytes, the palette and then zeros; for more than one frame or an explicit loop count the
NETSCAPE2.0 application extension; the records back to back; 3B.

FAULTS: names of single deviations a test switches on to show that its checks notice them.
"""
import struct

import numpy as np

SEGMENT = 2048
FAULTS = set()          # "width_off_by_one": w(k) by 2^m + 1 + k < 2^w; "msb_first"; "no_clear": segments not opened with CLEAR


def min_code_size(K):
    m = 2
    while (1 << m) < K:
        m += 1
    return m


def table_bits(K):
    g = 1
    while (1 << g) < K:
        g += 1
    return g


def code_width(k, m):
    w = m + 1
    while ((1 << m) + 1 + k >= (1 << w)) if "width_off_by_one" in FAULTS else ((1 << m) + 1 + k > (1 << w)):
        w += 1
    return w


def code_bits(c, m):
    """W(c) = w(1) + ... + w(c)"""
    return sum(code_width(k, m) for k in range(1, c + 1))


def lzw_segment(px, m):
    """The codes of one segment (without its CLEAR): greedy LZW from an empty dictionary."""
    table = {}
    nxt = (1 << m) + 2
    cur = px[0]
    out = []
    for v in px[1:]:
        hit = table.get((cur, v))
        if hit is not None:
            cur = hit
            continue
        out.append(cur)
        table[(cur, v)] = nxt
        nxt += 1
        cur = v
    out.append(cur)
    return out


def frame_codes(index, K):
    """[(value, bits)] of a frame's code stream."""
    flat = [int(v) for v in np.asarray(index, np.uint8).reshape(-1)]
    assert flat and max(flat) < K <= 256
    m = min_code_size(K)
    clear = 1 << m
    out = [(clear, m + 1)]
    for s in range(0, len(flat), SEGMENT):
        codes = lzw_segment(flat[s:s + SEGMENT], m)
        out += [(c, code_width(k + 1, m)) for k, c in enumerate(codes)]
        last = s + SEGMENT >= len(flat)
        if last or "no_clear" not in FAULTS:
            out.append((clear + 1 if last else clear, code_width(len(codes) + 1, m)))
    return out


def pack(codes):
    acc = have = 0
    out = bytearray()
    for value, bits in codes:
        if "msb_first" in FAULTS:
            value = int(format(value, f"0{bits}b")[::-1], 2)
        acc |= value << have
        have += bits
        while have >= 8:
            out.append(acc & 255)
            acc >>= 8
            have -= 8
    if have:
        out.append(acc & 255)
    return bytes(out)


def frame_data(index, K):
    """The data bytes of a frame, before they are cut into sub-blocks."""
    return pack(frame_codes(index, K))


def sub_blocks(data):
    out = bytearray()
    for i in range(0, len(data), 255):
        piece = data[i:i + 255]
        out.append(len(piece))
        out += piece
    out.append(0)
    return bytes(out)


def record(index, K, delay_cs):
    """One frame's record: ``index`` uint8 [h,w]."""
    h, w = np.asarray(index).shape
    return (b"\x21\xf9\x04\x04" + struct.pack("<H", delay_cs) + b"\x00\x00" + b"\x2c" + struct.pack("<HHHH", 0, 0, w, h) + b"\x00"
            + bytes([min_code_size(K)]) + sub_blocks(frame_data(index, K)))


def header(size, palette, loop=None):
    """``size``: (w, h); ``palette``: uint8 [K,3]; ``loop``: None (no NETSCAPE2.0 extension) or the loop count, 0 for ever."""
    pal = np.asarray(palette, np.uint8).reshape(-1, 3)
    g = table_bits(len(pal))
    out = b"GIF89a" + struct.pack("<HHBBB", size[0], size[1], 0x80 | 0x70 | (g - 1), 0, 0) + pal.tobytes() + bytes(3 * ((1 << g) - len(pal)))
    if loop is not None:
        out += b"\x21\xff\x0bNETSCAPE2.0\x03\x01" + struct.pack("<H", loop) + b"\x00"
    return out


def file(indices, palette, delay_cs, loop=None):
    """The whole file of ``indices`` uint8 [n,h,w].  ``loop``: a count (0: for ever) is written; None writes 0 when n > 1 and nothing for one frame."""
    indices = np.asarray(indices, np.uint8)
    n, h, w = indices.shape
    K = len(np.asarray(palette).reshape(-1, 3))
    if loop is None and n > 1:
        loop = 0
    return header((w, h), palette, loop) + b"".join(record(f, K, delay_cs) for f in indices) + b"\x3b"


def out_stride(h, w, K):
    """The bound of adain_gif_encode_u8_bytes: a segment of p pixels costs at most W(p + 1) bits."""
    m = min_code_size(K)
    full, rest = divmod(h * w, SEGMENT)
    bits = (m + 1) + full * code_bits(SEGMENT + 1, m) + (code_bits(rest + 1, m) if rest else 0)
    D = (bits + 7) // 8
    return 20 + D + (D + 254) // 255
