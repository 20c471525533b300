"""Reading a baseline JPEG file on the host for the device decoder (csrc/jpeg_decode.hip, adain_jpeg_decode_u8 / adain_jpeg_decode_restart_u8):
a walk over the file's markers that returns a description of the file and packs its tables into one small blob, or raises
``UnsupportedJpeg`` with the reason in words.

Taken: 8-bit baseline (SOF0) and extended sequential Huffman (SOF1) files with ONE interleaved scan, one component (grey, sampled 1 x 1)
or three with JFIF's ids 1, 2, 3, chroma sampled 1 x 1 and luma 1 x 1 (4:4:4), 2 x 1 (4:2:2) or 2 x 2 (4:2:0), 8-bit quantisation tables,
Huffman tables 0 and 1 of either class, the entropy-coded segment followed by EOI.  A restart interval (DRI other than 0) is taken with
``parse(data, restart=True)``: the walk then passes the RSTn markers inside the scan, which stay in the segment - the device removes
them - and must be ceil(MCUs / Ri) - 1 in number, numbered D0..D7 in turn, with no fill byte in front of any; ``restart_interval`` is
the file's Ri.  By default such a file is refused as before.  Everything else is refused and stays with PIL: progressive, arithmetic,
lossless and 12-bit files, several scans, non-interleaved scans, CMYK / YCCK or an Adobe APP14 segment with transform 0, other
component ids, any other sampling (4:4:0 and 4:1:1 included), DNL, restart markers that are missing, surplus or out of order (no
resynchronisation is tried), and truncated or inconsistent segments.  EXIF orientation is ignored, as PIL ignores it.  The parser never
makes a caller fail: every caller catches ``UnsupportedJpeg`` and takes the PIL path.

Progressive files (SOF2, 8-bit, Huffman) are taken with ``parse(data, progressive=True)`` and come back as a ``ProgressiveJpegFile``
(adain_jpeg_decode_progressive_u8): the frame rules above, no DRI other than 0, between scans nothing but DHT, APPn and COM, table ids
of at most 1, 1..``MAX_SCANS`` scans, a DC scan (Ss = Se = 0) with all components in frame order or exactly one, an AC scan with
1 <= Ss <= Se <= 63 and one component, Al <= 13, a component's AC scans behind its first DC scan, a coefficient's first scan at Ah = 0,
every later one at Ah = its current Al with Al = Ah - 1, one history per band, and a COMPLETE script: at EOI every coefficient of every
component stands at Al = 0 (on an incomplete one libjpeg smooths between blocks and the pixels are no longer a function of the
coefficients).  Every scan keeps its own segment (up to the next marker) and a blob with the Huffman tables in force at its SOS; files
are batched by ``(geometry, script)``.  By default such a file is refused as before.

The blob (``BLOB_BYTES`` per file, the layout csrc/jpeg_decode.hip's ``FileTables`` reads):
  4 Huffman tables in the order DC0, DC1, AC0, AC1, 912 bytes each - look[256] uint16: for the next 8 bits of the stream, (code length
    << 8) | symbol of the code of at most 8 bits that starts there, 0 when none; maxcode[18] int32: the largest code of each length 1..16,
    -1 where the length has none (index 0 unused, index 17 = -1); valoff[18] int32: index into val of the first symbol of that length
    minus its smallest code; val[256] uint8: HUFFVAL, zero padded
  q[3][64] uint8: the quantisation table of each component in NATURAL order
  sel[8] uint8: the DC table (0, 1) of components 0..2, then the AC table (0, 1) of components 0..2, two zero bytes
"""
from dataclasses import dataclass

import numpy as np

ZIGZAG = (0, 1, 8, 16, 9, 2, 3, 10, 17, 24, 32, 25, 18, 11, 4, 5, 12, 19, 26, 33, 40, 48, 41, 34, 27, 20, 13, 6, 7, 14, 21, 28,
          35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23, 30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63)
HUFF_BYTES = 912
BLOB_BYTES = 4 * HUFF_BYTES + 3 * 64 + 8
MAX_SCANS = 32                             # of a progressive file (adain_jpeg_decode_progressive_u8)
MAX_SEGMENT_BYTES = (1 << 28) - 1          # the device decoder's bit positions are uint32
SAMPLINGS = {(1, 1): 0, (2, 1): 1, (2, 2): 2}          # luma h x v -> Pillow's subsampling number


class UnsupportedJpeg(Exception):
    """The file is not one the device decoder takes; str(e) says why.  Callers fall back to PIL."""


@dataclass
class JpegFile:
    h: int
    w: int
    c: int                      # components: 1 (grey) or 3 (YCbCr)
    sampling: int               # 0: luma 1 x 1 (4:4:4, grey), 1: 2 x 1 (4:2:2), 2: 2 x 2 (4:2:0)
    qtables: np.ndarray         # uint8 [c, 64], natural order, per component
    huffman: dict               # (class, id) -> (bits [16], huffval bytes), class 0 DC, 1 AC; the tables the scan uses
    dc_sel: tuple               # per component
    ac_sel: tuple
    restart_interval: int       # MCUs per restart interval; 0: none (always, unless parsed with restart=True)
    seg_offset: int             # of the entropy-coded segment in the file
    seg_length: int             # up to EOI, RSTn markers included
    blob: bytes                 # BLOB_BYTES

    @property
    def geometry(self):
        return (self.h, self.w, self.c, self.sampling)


@dataclass
class ProgressiveScan:
    comps: tuple                # indices of the scan's components in the frame
    ss: int
    se: int
    ah: int
    al: int
    seg_offset: int             # of the scan's entropy-coded segment in the file
    seg_length: int             # up to the next marker
    blob: bytes                 # BLOB_BYTES: the Huffman tables in force at this SOS (and the frame's quantisation tables)

    @property
    def key(self):
        return (self.comps, self.ss, self.se, self.ah, self.al)


@dataclass
class ProgressiveJpegFile:
    """An 8-bit progressive Huffman (SOF2) file whose scan script is complete: parse(data, progressive=True)."""
    h: int
    w: int
    c: int
    sampling: int
    qtables: np.ndarray         # uint8 [c, 64], natural order, per component
    scans: tuple                # of ProgressiveScan, in file order

    @property
    def geometry(self):
        return (self.h, self.w, self.c, self.sampling)

    @property
    def script(self):
        """The scans without offsets and blobs: files are batched by (geometry, script)."""
        return tuple(sc.key for sc in self.scans)


def huffman_lookup(bits, vals):
    """(BITS[16], HUFFVAL) -> (look uint16 [256], maxcode int32 [18], valoff int32 [18], val uint8 [256]): libjpeg's derived table."""
    look = np.zeros(256, np.uint16)
    maxcode = np.full(18, -1, np.int32)
    valoff = np.zeros(18, np.int32)
    val = np.zeros(256, np.uint8)
    val[:len(vals)] = np.frombuffer(bytes(vals), np.uint8)
    code = k = 0
    for ln in range(1, 17):
        if bits[ln - 1]:
            valoff[ln] = k - code
            for _ in range(bits[ln - 1]):
                if ln <= 8:
                    look[code << (8 - ln):(code + 1) << (8 - ln)] = (ln << 8) | vals[k]
                code += 1
                k += 1
            maxcode[ln] = code - 1
        code <<= 1
    return look, maxcode, valoff, val


def _pack_blob(c, qtables, huffman, dc_sel, ac_sel):
    out = bytearray()
    for key in ((0, 0), (0, 1), (1, 0), (1, 1)):
        if key in huffman:
            look, maxcode, valoff, val = huffman_lookup(*huffman[key])
            out += look.astype("<u2").tobytes() + maxcode.astype("<i4").tobytes() + valoff.astype("<i4").tobytes() + val.tobytes()
        else:
            out += (np.zeros(256, "<u2").tobytes() + np.full(18, -1, "<i4").tobytes() + bytes(72 + 256))          # no code at all
    q = np.zeros((3, 64), np.uint8)
    q[:c] = qtables
    out += q.tobytes() + bytes(list(dc_sel) + [0] * (3 - c) + list(ac_sel) + [0] * (3 - c) + [0, 0])
    assert len(out) == BLOB_BYTES
    return bytes(out)


_SOF_REFUSED = {0xC2: "progressive (SOF2)", 0xC3: "lossless (SOF3)", 0xC5: "differential sequential (SOF5)", 0xC6: "differential progressive (SOF6)",
                0xC7: "differential lossless (SOF7)", 0xC9: "arithmetic coding (SOF9)", 0xCA: "arithmetic coding (SOF10)", 0xCB: "arithmetic coding (SOF11)",
                0xCD: "arithmetic coding (SOF13)", 0xCE: "arithmetic coding (SOF14)", 0xCF: "arithmetic coding (SOF15)"}


def _segment_end(data, seg):
    """Index of the first FF behind ``seg`` that is not followed by a stuffed 00: the marker that ends the entropy-coded segment."""
    end = seg
    while True:
        end = data.find(b"\xff", end)
        if end < 0 or end + 1 >= len(data):
            raise UnsupportedJpeg("truncated: no marker behind the entropy-coded segment")
        if data[end + 1] != 0:
            return end
        end += 2


def _progressive_scan(body, frame, huff, state):
    """The SOS ``body`` of a progressive file -> (comps, ss, se, ah, al, dc_sel, ac_sel), checked against the script so far.
    ``state``: per component the current Al of each of the 64 coefficients, -1 before its first scan."""
    h, w, nc, comps = frame
    ns = body[0]
    ids = [x[0] for x in comps]
    sel = [(body[1 + 2 * i], body[2 + 2 * i] >> 4, body[2 + 2 * i] & 15) for i in range(ns)]
    if any(s_[0] not in ids for s_ in sel):
        raise UnsupportedJpeg("a scan component that is not in the frame")
    cis = tuple(ids.index(s_[0]) for s_ in sel)
    ss, se, ah, al = body[-3], body[-2], body[-1] >> 4, body[-1] & 15
    if ss == 0:
        if se != 0:
            raise UnsupportedJpeg("a progressive scan that mixes the DC term with AC coefficients")
        if ns != 1 and cis != tuple(range(nc)):
            raise UnsupportedJpeg("a DC scan with neither one component nor all of them in frame order")
    else:
        if not 1 <= ss <= se <= 63:
            raise UnsupportedJpeg(f"a band {ss}..{se}")
        if ns != 1:
            raise UnsupportedJpeg("an interleaved AC scan")
    if al > 13:
        raise UnsupportedJpeg(f"a point transform Al of {al}")
    for ci in cis:
        band = state[ci][ss:se + 1]
        if ss > 0 and state[ci][0] < 0:
            raise UnsupportedJpeg("an AC scan before the component's first DC scan")
        if len(set(band)) != 1:
            raise UnsupportedJpeg(f"a band {ss}..{se} whose coefficients do not share one history")
        if band[0] < 0:
            if ah != 0:
                raise UnsupportedJpeg(f"a first scan of a coefficient with Ah = {ah}")
        elif ah != band[0] or al != ah - 1:
            raise UnsupportedJpeg(f"a refinement with Ah = {ah}, Al = {al} of coefficients that stand at Al = {band[0]}")
        state[ci][ss:se + 1] = [al] * (se + 1 - ss)
    dc_sel, ac_sel = [0] * nc, [0] * nc
    for ci, (_, d, a) in zip(cis, sel):
        if d > 1 or a > 1:
            raise UnsupportedJpeg("Huffman table ids above 1")
        if ss == 0 and ah == 0 and (0, d) not in huff:
            raise UnsupportedJpeg("a missing Huffman table")
        if ss > 0 and (1, a) not in huff:
            raise UnsupportedJpeg("a missing Huffman table")
        dc_sel[ci], ac_sel[ci] = d, a
    return cis, ss, se, ah, al, tuple(dc_sel), tuple(ac_sel)


def _parse_progressive(data, at, frame, qt, huff, restart_interval, adobe_transform):
    """The scans of an SOF2 file from its first SOS segment (marker at ``at`` - 2) to EOI -> ProgressiveJpegFile."""
    n = len(data)
    h, w, nc, comps = frame
    if adobe_transform == 0 and nc == 3:
        raise UnsupportedJpeg("an Adobe APP14 segment with transform 0 (RGB, not YCbCr)")
    if restart_interval != 0:
        raise UnsupportedJpeg(f"a progressive file with a restart interval ({restart_interval} MCUs)")
    for x in comps:
        if x[3] not in qt:
            raise UnsupportedJpeg("a missing quantisation table")
    q = np.stack([qt[x[3]] for x in comps])
    state = [[-1] * 64 for _ in range(nc)]
    scans = []
    m = 0xDA
    while True:
        if at + 2 > n:
            raise UnsupportedJpeg("truncated inside a segment length")
        ln = (data[at] << 8) | data[at + 1]
        if ln < 2 or at + ln > n:
            raise UnsupportedJpeg(f"truncated or inconsistent: segment FF{m:02X} of length {ln} at {at - 2} passes the end of the file")
        body = data[at + 2:at + ln]
        if m == 0xDA:
            if len(body) < 1 or not 1 <= body[0] <= 3 or len(body) != 4 + 2 * body[0]:
                raise UnsupportedJpeg("inconsistent: SOS length")
            if len(scans) == MAX_SCANS:
                raise UnsupportedJpeg(f"more than {MAX_SCANS} scans")
            cis, ss, se, ah, al, dc_sel, ac_sel = _progressive_scan(body, frame, huff, state)
            seg = at + ln
            end = _segment_end(data, seg)
            if end - seg > MAX_SEGMENT_BYTES:
                raise UnsupportedJpeg("an entropy-coded segment of 2^28 bytes or more")
            scans.append(ProgressiveScan(cis, ss, se, ah, al, seg, end - seg, _pack_blob(nc, q, dict(huff), dc_sel, ac_sel)))
            at = end
        elif m == 0xC4:
            _read_dht(body, huff)
            at += ln
        elif 0xE0 <= m <= 0xEF or m == 0xFE:
            at += ln
        else:
            raise UnsupportedJpeg(f"marker FF{m:02X} behind the first scan of a progressive file (only DHT, APPn and COM may stand between scans)")
        while True:                      # the next marker, fill bytes passed
            if at + 2 > n:
                raise UnsupportedJpeg("truncated: no EOI")
            if data[at] != 0xFF:
                raise UnsupportedJpeg(f"inconsistent: byte {data[at]:#04x} at {at} where a marker is due")
            if data[at + 1] != 0xFF:
                break
            at += 1
        m = data[at + 1]
        at += 2
        if m == 0xD9:
            break
    if any(a != 0 for st in state for a in st):
        raise UnsupportedJpeg("an incomplete progressive script (a coefficient that no scan brings to full precision)")
    return ProgressiveJpegFile(h, w, nc, SAMPLINGS[(comps[0][1], comps[0][2])], q, tuple(scans))


def _read_dht(body, huff):
    p = 0
    while p < len(body):
        if p + 17 > len(body):
            raise UnsupportedJpeg("inconsistent: DHT too short")
        tc, th = body[p] >> 4, body[p] & 15
        bits = list(body[p + 1:p + 17])
        total = sum(bits)
        if tc > 1 or th > 3:
            raise UnsupportedJpeg("inconsistent: DHT class or id")
        if total > 256:
            raise UnsupportedJpeg(f"inconsistent: a DHT whose BITS sum to {total}")
        if p + 17 + total > len(body):
            raise UnsupportedJpeg("inconsistent: DHT shorter than its BITS say")
        c_ = 0               # more codes of a length than the length has
        for i, b in enumerate(bits):
            c_ += b
            if c_ > (1 << (i + 1)):
                raise UnsupportedJpeg("inconsistent: a DHT with more codes than its lengths allow")
            c_ <<= 1
        huff[(tc, th)] = (bits, bytes(body[p + 17:p + 17 + total]))
        p += 17 + total


def parse(data, restart=False, progressive=False):
    """bytes of a file -> JpegFile, or UnsupportedJpeg.  ``restart``: take files with a restart interval too.  ``progressive``: take
    8-bit progressive Huffman (SOF2) files with a complete scan script too, as a ProgressiveJpegFile."""
    data = bytes(data)
    n = len(data)
    if n < 4 or data[:2] != b"\xff\xd8":
        raise UnsupportedJpeg("not a JPEG file (no SOI)")
    qt, huff = {}, {}
    frame = None
    restart_interval = 0
    adobe_transform = None
    is_progressive = False
    at = 2
    while True:
        if at + 2 > n:
            raise UnsupportedJpeg("truncated: the file ends before a scan")
        if data[at] != 0xFF:
            raise UnsupportedJpeg(f"inconsistent: byte {data[at]:#04x} at {at} where a marker is due")
        m = data[at + 1]
        if m == 0xFF:                    # fill byte
            at += 1
            continue
        at += 2
        if m == 0xD8 or m == 0x01 or 0xD0 <= m <= 0xD7:
            raise UnsupportedJpeg(f"inconsistent: marker FF{m:02X} in the header")
        if m == 0xD9:
            raise UnsupportedJpeg("no scan before EOI")
        if at + 2 > n:
            raise UnsupportedJpeg("truncated inside a segment length")
        ln = (data[at] << 8) | data[at + 1]
        if ln < 2 or at + ln > n:
            raise UnsupportedJpeg(f"truncated or inconsistent: segment FF{m:02X} of length {ln} at {at - 2} passes the end of the file")
        body = data[at + 2:at + ln]
        if m in _SOF_REFUSED and not (progressive and m == 0xC2):
            raise UnsupportedJpeg(_SOF_REFUSED[m])
        if m == 0xDC:
            raise UnsupportedJpeg("a DNL marker")
        if m in (0xC0, 0xC1, 0xC2):
            if frame is not None:
                raise UnsupportedJpeg("more than one frame header")
            if len(body) < 6:
                raise UnsupportedJpeg("inconsistent: SOF too short")
            prec, h, w, nc = body[0], (body[1] << 8) | body[2], (body[3] << 8) | body[4], body[5]
            if prec != 8:
                raise UnsupportedJpeg(f"{prec}-bit samples")
            if h == 0 or w == 0:
                raise UnsupportedJpeg("a height or width of 0 (DNL)")
            if nc == 4:
                raise UnsupportedJpeg("four components (CMYK / YCCK)")
            if nc not in (1, 3):
                raise UnsupportedJpeg(f"{nc} components")
            if len(body) != 6 + 3 * nc:
                raise UnsupportedJpeg("inconsistent: SOF length")
            comps = [(body[6 + 3 * i], body[7 + 3 * i] >> 4, body[7 + 3 * i] & 15, body[8 + 3 * i]) for i in range(nc)]
            if [x[0] for x in comps] != list(range(1, nc + 1)):
                raise UnsupportedJpeg(f"component ids {[x[0] for x in comps]} are not JFIF's")
            if any((x[1], x[2]) != (1, 1) for x in comps[1:]) or (comps[0][1], comps[0][2]) not in SAMPLINGS or (nc == 1 and (comps[0][1], comps[0][2]) != (1, 1)):
                raise UnsupportedJpeg(f"sampling factors {[(x[1], x[2]) for x in comps]}")
            frame = (h, w, nc, comps)
            is_progressive = m == 0xC2
        elif m == 0xDB:
            p = 0
            while p < len(body):
                pq, tq = body[p] >> 4, body[p] & 15
                if pq != 0:
                    raise UnsupportedJpeg("a 16-bit quantisation table")
                if tq > 3 or p + 65 > len(body):
                    raise UnsupportedJpeg("inconsistent: DQT")
                t = np.zeros(64, np.uint8)
                t[list(ZIGZAG)] = np.frombuffer(body[p + 1:p + 65], np.uint8)
                qt[tq] = t
                p += 65
        elif m == 0xC4:
            _read_dht(body, huff)
        elif m == 0xDD:
            if len(body) != 2:
                raise UnsupportedJpeg("inconsistent: DRI length")
            restart_interval = (body[0] << 8) | body[1]
        elif m == 0xEE:
            if body[:5] == b"Adobe" and len(body) >= 12:
                adobe_transform = body[11]
        elif m == 0xDA:
            if frame is None:
                raise UnsupportedJpeg("a scan before the frame header")
            if is_progressive:
                return _parse_progressive(data, at, frame, qt, huff, restart_interval, adobe_transform)
            h, w, nc, comps = frame
            if adobe_transform == 0 and nc == 3:
                raise UnsupportedJpeg("an Adobe APP14 segment with transform 0 (RGB, not YCbCr)")
            if len(body) < 1 or len(body) != 4 + 2 * body[0]:
                raise UnsupportedJpeg("inconsistent: SOS length")
            if body[0] != nc:
                raise UnsupportedJpeg("a non-interleaved scan (more than one scan)")
            sel = [(body[1 + 2 * i], body[2 + 2 * i] >> 4, body[2 + 2 * i] & 15) for i in range(nc)]
            if [s[0] for s in sel] != [x[0] for x in comps]:
                raise UnsupportedJpeg("scan components out of order")
            if tuple(body[-3:]) != (0, 63, 0):
                raise UnsupportedJpeg("a scan that is not the whole spectrum at full precision")
            if restart_interval != 0 and not restart:
                raise UnsupportedJpeg(f"a restart interval ({restart_interval} MCUs)")
            for _, d, a in sel:
                if d > 1 or a > 1:
                    raise UnsupportedJpeg("Huffman table ids above 1")
                if (0, d) not in huff or (1, a) not in huff:
                    raise UnsupportedJpeg("a missing Huffman table")
            for x in comps:
                if x[3] not in qt:
                    raise UnsupportedJpeg("a missing quantisation table")
            seg = at + ln
            end = seg
            markers = 0
            while True:                  # the segment ends at the first marker that is neither a stuffed FF 00 nor (restart) the RSTn that is due
                end = data.find(b"\xff", end)
                if end < 0 or end + 1 >= n:
                    raise UnsupportedJpeg("truncated: no marker behind the entropy-coded segment")
                if data[end + 1] == 0:
                    end += 2
                    continue
                if restart_interval != 0 and 0xD0 <= data[end + 1] <= 0xD7:
                    if data[end + 1] != 0xD0 + markers % 8:
                        raise UnsupportedJpeg(f"restart marker {markers} is FF{data[end + 1]:02X}, not FF{0xD0 + markers % 8:02X}")
                    markers += 1
                    end += 2
                    continue
                if restart_interval != 0 and data[end + 1] == 0xFF:
                    raise UnsupportedJpeg("a fill byte in front of a marker in a scan with restart intervals")
                break
            if data[end + 1] != 0xD9:
                raise UnsupportedJpeg(f"marker FF{data[end + 1]:02X} behind the scan (more than one scan, restart markers or damage)")
            if end - seg > MAX_SEGMENT_BYTES:
                raise UnsupportedJpeg("an entropy-coded segment of 2^28 bytes or more")
            if restart_interval != 0:
                hh, vv = comps[0][1], comps[0][2]
                nmcu = -(-w // (8 * hh)) * -(-h // (8 * vv))
                if markers != -(-nmcu // restart_interval) - 1:
                    raise UnsupportedJpeg(f"{markers} restart markers where {nmcu} MCUs in intervals of {restart_interval} have {-(-nmcu // restart_interval) - 1}")
            used = {(0, d) for _, d, _ in sel} | {(1, a) for _, _, a in sel}
            tables = {k: v for k, v in huff.items() if k in used}
            q = np.stack([qt[x[3]] for x in comps])
            dc_sel, ac_sel = tuple(s[1] for s in sel), tuple(s[2] for s in sel)
            return JpegFile(h, w, nc, SAMPLINGS[(comps[0][1], comps[0][2])], q, tables, dc_sel, ac_sel, restart_interval, seg, end - seg,
                            _pack_blob(nc, q, tables, dc_sel, ac_sel))
        at += ln
