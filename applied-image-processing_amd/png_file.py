"""Reading a PNG file on the host for the device decoder (csrc/png_decode.hip, adain_png_decode_u8): a walk over the file's chunks that
returns the frame's shape and its IDAT payloads joined, or raises ``UnsupportedPng`` with the reason in words.  The counterpart of
jpeg_file.py.

Taken: the signature and IHDR first; bit depth 8; colour type 0 (grey, c = 1), 2 (RGB, c = 3) or 6 (RGBA, c = 4); compression 0, filter
method 0, interlace 0; one or more CONSECUTIVE IDAT chunks of any lengths, 0 included, split anywhere (inside the zlib header too); IEND;
any ancillary chunks except tRNS, which are skipped.  Of the zlib header the walk checks CM = 8, CINFO <= 7, FCHECK and FDICT = 0; the
deflate data and the Adler-32 are the device's to check.  Everything else is refused and stays with PIL: palette, grey + alpha, 1 / 2 /
4 / 16-bit and interlaced files, tRNS, IDAT chunks that are not consecutive, a missing IEND, a chunk length that passes the end of the
file, APNG (acTL), an unknown critical chunk, a filtered stream h (w c + 1) of 2^31 bytes or more.  CRCs are not verified: Pillow 12.2
does not verify IDAT's (a flipped CRC byte still loads), and a wrong Adler-32, which Pillow does refuse, is found on the device.  The
parser never makes a caller fail: every caller catches ``UnsupportedPng`` and takes the PIL path.
"""
from dataclasses import dataclass

SIGNATURE = b"\x89PNG\r\n\x1a\n"
CHANNELS = {0: 1, 2: 3, 6: 4}                  # colour type -> channels
_COLOUR_REFUSED = {3: "a palette", 4: "grey with alpha"}


class UnsupportedPng(Exception):
    """The file is not one the device decoder takes; str(e) says why.  Callers fall back to PIL."""


@dataclass
class PngFile:
    h: int
    w: int
    colour_type: int            # 0, 2 or 6
    c: int                      # channels: 1, 3 or 4
    stream: bytes               # the IDAT payloads joined: a zlib stream

    @property
    def geometry(self):
        return (self.h, self.w, self.colour_type)


def parse(data):
    """bytes of a file -> PngFile, or UnsupportedPng."""
    data = bytes(data)
    n = len(data)
    if data[:8] != SIGNATURE:
        raise UnsupportedPng("not a PNG file (no signature)")
    at = 8
    header = None
    pieces = []
    state = 0                   # 0: before IDAT, 1: inside the run of IDATs, 2: behind it
    ended = False
    while at < n:
        if at + 8 > n:
            raise UnsupportedPng("truncated inside a chunk header")
        length = int.from_bytes(data[at:at + 4], "big")
        kind = data[at + 4:at + 8]
        if at + 12 + length > n:
            raise UnsupportedPng(f"chunk {kind!r} of length {length} at {at} passes the end of the file")
        body = data[at + 8:at + 8 + length]
        at += 12 + length
        if header is None:
            if kind != b"IHDR" or length != 13:
                raise UnsupportedPng("the first chunk is not a 13-byte IHDR")
            w, h = int.from_bytes(body[0:4], "big"), int.from_bytes(body[4:8], "big")
            depth, colour, compression, method, interlace = body[8:13]
            if w < 1 or h < 1 or w >= 1 << 31 or h >= 1 << 31:
                raise UnsupportedPng(f"a width or height outside 1..2^31 - 1 ({w} x {h})")
            if colour in _COLOUR_REFUSED:
                raise UnsupportedPng(f"{_COLOUR_REFUSED[colour]} (colour type {colour})")
            if colour not in CHANNELS:
                raise UnsupportedPng(f"colour type {colour}")
            if depth != 8:
                raise UnsupportedPng(f"{depth}-bit samples")
            if compression != 0 or method != 0:
                raise UnsupportedPng(f"compression method {compression}, filter method {method}")
            if interlace != 0:
                raise UnsupportedPng("an interlaced file")
            if h * (w * CHANNELS[colour] + 1) >= 1 << 31:
                raise UnsupportedPng("a filtered stream h (w c + 1) of 2^31 bytes or more")
            header = (h, w, colour)
            continue
        if kind == b"IHDR":
            raise UnsupportedPng("a second IHDR")
        if kind == b"IDAT":
            if state == 2:
                raise UnsupportedPng("IDAT chunks that are not consecutive")
            state = 1
            pieces.append(body)
            continue
        if state == 1:
            state = 2
        if kind == b"IEND":
            ended = True
            break
        if kind == b"tRNS":
            raise UnsupportedPng("a tRNS chunk")
        if kind == b"acTL":
            raise UnsupportedPng("an animated file (acTL)")
        if not kind[0] & 0x20:
            raise UnsupportedPng(f"critical chunk {kind!r}")
    if header is None:
        raise UnsupportedPng("no IHDR")
    if not ended:
        raise UnsupportedPng("no IEND")
    if state == 0:
        raise UnsupportedPng("no IDAT")
    stream = b"".join(pieces)
    if len(stream) < 2:
        raise UnsupportedPng("a zlib stream shorter than its header")
    cmf, flg = stream[0], stream[1]
    if cmf & 15 != 8:
        raise UnsupportedPng(f"zlib compression method {cmf & 15}")
    if cmf >> 4 > 7:
        raise UnsupportedPng(f"a zlib window of 2^{(cmf >> 4) + 8} bytes")
    if (cmf << 8 | flg) % 31:
        raise UnsupportedPng("a zlib header whose check bits are wrong")
    if flg & 0x20:
        raise UnsupportedPng("a zlib preset dictionary")
    if len(stream) >= 1 << 31:
        raise UnsupportedPng("a zlib stream of 2^31 bytes or more")
    h, w, colour = header
    return PngFile(h, w, colour, CHANNELS[colour], stream)
