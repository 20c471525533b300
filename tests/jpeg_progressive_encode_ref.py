"""NumPy / Python restatement of the progressive JPEG file ``Image.fromarray(frame).save(f, format="JPEG", quality=q, subsampling=s,
progressive=True)`` writes - the rules the device encoder's progressive path (csrc/jpeg.hip, adain_jpeg_encode_progressive_u8) runs.
The quantised coefficients are the baseline file's (jpeg_options_ref.scan_blocks); what differs is the entropy coding: libjpeg's
``jpeg_simple_progression`` script, one optimal Huffman table per scan, end-of-band runs across blocks and buffered correction bits.
tests/test_jpeg_progressive_encode_host.py holds this to Pillow on the host.

The scans, as (components, Ss, Se, Ah, Al); component 0 Y, 1 Cb, 2 Cr.  Cr comes before Cb.
"""
import numpy as np

import jpeg_options_ref as O
import jpeg_ref as J

COLOUR_SCRIPT = [((0, 1, 2), 0, 0, 0, 1), ((0,), 1, 5, 0, 2), ((2,), 1, 63, 0, 1), ((1,), 1, 63, 0, 1), ((0,), 6, 63, 0, 2),
                 ((0,), 1, 63, 2, 1), ((0, 1, 2), 0, 0, 1, 0), ((2,), 1, 63, 1, 0), ((1,), 1, 63, 1, 0), ((0,), 1, 63, 1, 0)]
GREY_SCRIPT = [((0,), 0, 0, 0, 1), ((0,), 1, 5, 0, 2), ((0,), 6, 63, 0, 2), ((0,), 1, 63, 2, 1), ((0,), 0, 0, 1, 0), ((0,), 1, 63, 1, 0)]

EOBRUN_CAP = 0x7FFF
MAX_CORR_BITS = 1000
CORR_CUT = MAX_CORR_BITS - 64 + 1          # a run is written once its buffer holds MORE than this many correction bits


def script(c):
    return COLOUR_SCRIPT if c == 3 else GREY_SCRIPT


def components(img, quality=J.DEFAULT_QUALITY, subsampling=2):
    """The frame's quantised coefficients per component, zigzag order with the TRUE DC at 0 (a dummy luma block carries the DC of the block
    before it): (mcu [blocks, 64] in the interleaved order of the DC scans with the component per block, grids: per component its own
    row-major block grid [rows, cols, 64] - Y cropped to ceil(h/8) x ceil(w/8), chroma the MCU grid)."""
    img = np.asarray(img)
    if img.ndim == 3 and img.shape[2] == 1:
        img = img[..., 0]
    h, w = img.shape[:2]
    bh, bw = -(-h // 8), -(-w // 8)
    z, tbl = O.scan_blocks(img, quality, subsampling)
    z = z.copy()
    if img.ndim == 2:
        z[:, 0] = np.cumsum(z[:, 0])
        return z, np.zeros(len(z), np.int64), [z.reshape(bh, bw, 64)]
    hs, vs = O.SUBSAMPLING[subsampling]
    bpm = hs * vs + 2
    mh, mw = -(-h // (8 * vs)), -(-w // (8 * hs))
    comp = np.tile(np.array([0] * (hs * vs) + [1, 2]), mh * mw)
    for k in range(3):
        z[comp == k, 0] = np.cumsum(z[comp == k, 0])
    m = z.reshape(mh, mw, bpm, 64)
    y = m[:, :, :hs * vs].reshape(mh, mw, vs, hs, 64).swapaxes(1, 2).reshape(vs * mh, hs * mw, 64)[:bh, :bw]
    return z, comp, [y, m[:, :, hs * vs], m[:, :, hs * vs + 1]]


class _Events:
    """What a scan puts into its stream, in order: Huffman symbols (of table 0 or 1 of the scan) and raw bits."""

    def __init__(self):
        self.sym, self.val, self.len = [], [], []

    def symbol(self, s, table=0):
        self.sym.append(s + 256 * table)
        self.val.append(0)
        self.len.append(0)

    def bits(self, value, n):
        if n:
            self.sym.append(-1)
            self.val.append(value & ((1 << n) - 1))
            self.len.append(n)


def _dc_first(mcu, comp, al, ev):
    v = mcu[:, 0] >> al
    last = [0, 0, 0]
    for x, k in zip(v.tolist(), comp.tolist()):
        d = x - last[k]
        last[k] = x
        n = abs(d).bit_length()
        ev.symbol(n, 1 if k else 0)
        ev.bits(d if d >= 0 else d - 1, n)


def _dc_refine(mcu, al, ev):
    for x in ((mcu[:, 0] >> al) & 1).tolist():
        ev.bits(x, 1)


class _Run:
    """The pending end-of-band run of an AC scan, with the correction bits buffered behind it."""

    def __init__(self, ev, cuts):
        self.ev, self.cuts, self.n, self.corr = ev, cuts, 0, []

    def write(self):
        if self.n:
            k = self.n.bit_length() - 1
            self.ev.symbol(k << 4)
            self.ev.bits(self.n, k)
            self.n = 0
        for b in self.corr:
            self.ev.bits(b, 1)
        self.corr = []

    def add(self, corr):
        self.n += 1
        self.corr += corr
        if self.n == EOBRUN_CAP:
            self.cuts["cap"] += 1
            self.write()
        elif len(self.corr) > CORR_CUT:
            self.cuts["corr"] += 1
            self.write()


def _ac_first(blocks, ss, se, al, ev, cuts):
    run = _Run(ev, cuts)
    band = blocks[:, ss:se + 1]
    empty = ~((np.abs(band) >> al) != 0).any(axis=1)
    for blk, none in zip(band.tolist(), empty.tolist()):
        if none:
            run.add([])
            continue
        r = 0
        for c in blk:
            t = abs(c) >> al
            if t == 0:
                r += 1
                continue
            run.write()
            while r > 15:
                ev.symbol(0xF0)
                r -= 16
            n = t.bit_length()
            ev.symbol((r << 4) | n)
            ev.bits(t if c >= 0 else ~t, n)
            r = 0
        if r > 0:
            run.add([])
    run.write()


def _ac_refine(blocks, ss, se, al, ev, cuts):
    run = _Run(ev, cuts)
    band = blocks[:, ss:se + 1]
    empty = ~((np.abs(band) >> al) != 0).any(axis=1)
    for blk, none in zip(band.tolist(), empty.tolist()):
        if none:
            run.add([])
            continue
        a = [abs(c) >> al for c in blk]
        eob = max((k for k, x in enumerate(a) if x == 1), default=-1)
        r, corr = 0, []
        for k, x in enumerate(a):
            if x == 0:
                r += 1
                continue
            while r > 15 and k <= eob:
                run.write()
                ev.symbol(0xF0)
                r -= 16
                for b in corr:
                    ev.bits(b, 1)
                corr = []
            if x > 1:
                corr.append(x & 1)
                continue
            run.write()
            ev.symbol((r << 4) | 1)
            ev.bits(0 if blk[k] < 0 else 1, 1)
            for b in corr:
                ev.bits(b, 1)
            corr = []
            r = 0
        if r > 0 or corr:
            run.add(corr)
    run.write()


def scan_events(mcu, comp, grids, scan):
    """(events, cuts) of one scan: cuts = {"cap": runs cut by the 0x7FFF cap, "corr": runs cut by the correction-bit rule}."""
    comps, ss, se, ah, al = scan
    ev, cuts = _Events(), {"cap": 0, "corr": 0}
    if ss == 0:
        if ah == 0:
            _dc_first(mcu, comp, al, ev)
        else:
            _dc_refine(mcu, al, ev)
    else:
        blocks = grids[comps[0]].reshape(-1, 64)
        (_ac_first if ah == 0 else _ac_refine)(blocks, ss, se, al, ev, cuts)
    return ev, cuts


def scan_segment(ev, scan, c):
    """The DHT segment(s), the SOS and the stuffed entropy-coded data of one scan."""
    comps, ss, se, ah, al = scan
    sym, val, ln = np.array(ev.sym, np.int64), np.array(ev.val, np.uint64), np.array(ev.len, np.int64)
    out = b""
    coded = sym >= 0
    if coded.any():
        tables = [0, 1][:2 if (ss == 0 and c == 3) else 1]
        ident = (1 if comps[0] else 0) if ss else None
        for t in tables:
            m = coded & (sym >> 8 == t)
            spec = O.optimal_table(np.bincount(sym[m] & 255, minlength=256))
            code, length = J.huff_codes(spec)
            val[m], ln[m] = code[sym[m] & 255], length[sym[m] & 255]
            out += O.dht_segments([spec], ids=[(0x10 | ident) if ss else t])
    if ss == 0:
        sel = [(k + 1, (0x10 if k else 0x00) if ah == 0 else 0x00) for k in comps]
    else:
        sel = [(comps[0] + 1, 0x01 if comps[0] else 0x00)]
    return out + O.sos_segment(sel, ss, se, ah, al) + J.pack_bits(val, ln)


def encode(img, quality=J.DEFAULT_QUALITY, subsampling=2, report=None):
    """uint8 [h, w, 3] (RGB), [h, w] or [h, w, 1] (L) -> the bytes of the file.  L ignores ``subsampling``, as Pillow does.  ``report``: a
    list that receives, per scan, (scan, {"cap": ..., "corr": ...}) - how many of its end-of-band runs each rule cut."""
    img = np.asarray(img)
    assert img.dtype == np.uint8 and img.ndim in (2, 3) and (img.ndim == 2 or img.shape[2] in (1, 3))
    assert subsampling in O.SUBSAMPLING
    h, w = img.shape[:2]
    c = 3 if img.ndim == 3 and img.shape[2] == 3 else 1
    mcu, comp, grids = components(img, quality, subsampling)
    out = O.header(h, w, c, quality, subsampling if c == 3 else 0, [], sof=0xC2, sos=False)
    for scan in script(c):
        ev, cuts = scan_events(mcu, comp, grids, scan)
        if report is not None:
            report.append((scan, cuts))
        out += scan_segment(ev, scan, c)
    return out + b"\xff\xd9"


def stripes(size=256):
    """The frame whose refinement scans buffer more than 937 correction bits in one run: every 8 x 8 block the row
    round(128 + 60 cos((2 (x mod 8) + 1) pi / 16)), uint8 [size, size]."""
    row = np.rint(128 + 60 * np.cos((2 * (np.arange(size) % 8) + 1) * np.pi / 16)).astype(np.uint8)
    return np.ascontiguousarray(np.broadcast_to(row, (size, size)))


def flat(size=1456, value=77):
    """The frame whose end-of-band runs pass the 0x7FFF cap: (size / 8)^2 blocks with no AC coefficient at all."""
    return np.full((size, size), value, np.uint8)


