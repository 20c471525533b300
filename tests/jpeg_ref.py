"""NumPy restatement of the baseline JPEG file Pillow's default ``Image.save(f, format="JPEG")`` writes (libjpeg's integer "islow"
DCT, h2v2 chroma, the Annex K tables scaled by the quality, fixed Huffman tables, JFIF 1.01 header) - the rules csrc/jpeg.hip runs on
the device.  Integer arithmetic throughout: the target is the same bytes, not a tolerance.  Every table is written out here, none is
read from a file Pillow wrote, so that the header is pinned as well.  tests/test_jpeg_host.py holds this to Pillow on the host.
"""
import numpy as np

# zigzag position k -> index in the natural (row-major) 8 x 8 order
ZIGZAG = np.array([0, 1, 8, 16, 9, 2, 3, 10, 17, 24, 32, 25, 18, 11, 4, 5, 12, 19, 26, 33, 40, 48, 41, 34, 27, 20, 13, 6, 7, 14, 21, 28,
                   35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23, 30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63])

# Annex K.1 quantisation tables, natural order
Q_LUMA = np.array([16, 11, 10, 16, 24, 40, 51, 61, 12, 12, 14, 19, 26, 58, 60, 55, 14, 13, 16, 24, 40, 57, 69, 56, 14, 17, 22, 29, 51, 87, 80, 62,
                   18, 22, 37, 56, 68, 109, 103, 77, 24, 35, 55, 64, 81, 104, 113, 92, 49, 64, 78, 87, 103, 121, 120, 101, 72, 92, 95, 98, 112, 100, 103, 99])
Q_CHROMA = np.array([17, 18, 24, 47, 99, 99, 99, 99, 18, 21, 26, 66, 99, 99, 99, 99, 24, 26, 56, 99, 99, 99, 99, 99, 47, 66, 99, 99, 99, 99, 99, 99]
                    + [99] * 32)

# Annex K.3 Huffman tables: codes per length 1..16, then the symbols in code order
DC_LUMA = ([0, 1, 5, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0, 0, 0], list(range(12)))
DC_CHROMA = ([0, 3, 1, 1, 1, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0], list(range(12)))
AC_LUMA = ([0, 2, 1, 3, 3, 2, 4, 3, 5, 5, 4, 4, 0, 0, 1, 0x7D], [
    0x01, 0x02, 0x03, 0x00, 0x04, 0x11, 0x05, 0x12, 0x21, 0x31, 0x41, 0x06, 0x13, 0x51, 0x61, 0x07, 0x22, 0x71, 0x14, 0x32, 0x81, 0x91, 0xA1, 0x08,
    0x23, 0x42, 0xB1, 0xC1, 0x15, 0x52, 0xD1, 0xF0, 0x24, 0x33, 0x62, 0x72, 0x82, 0x09, 0x0A, 0x16, 0x17, 0x18, 0x19, 0x1A, 0x25, 0x26, 0x27, 0x28,
    0x29, 0x2A, 0x34, 0x35, 0x36, 0x37, 0x38, 0x39, 0x3A, 0x43, 0x44, 0x45, 0x46, 0x47, 0x48, 0x49, 0x4A, 0x53, 0x54, 0x55, 0x56, 0x57, 0x58, 0x59,
    0x5A, 0x63, 0x64, 0x65, 0x66, 0x67, 0x68, 0x69, 0x6A, 0x73, 0x74, 0x75, 0x76, 0x77, 0x78, 0x79, 0x7A, 0x83, 0x84, 0x85, 0x86, 0x87, 0x88, 0x89,
    0x8A, 0x92, 0x93, 0x94, 0x95, 0x96, 0x97, 0x98, 0x99, 0x9A, 0xA2, 0xA3, 0xA4, 0xA5, 0xA6, 0xA7, 0xA8, 0xA9, 0xAA, 0xB2, 0xB3, 0xB4, 0xB5, 0xB6,
    0xB7, 0xB8, 0xB9, 0xBA, 0xC2, 0xC3, 0xC4, 0xC5, 0xC6, 0xC7, 0xC8, 0xC9, 0xCA, 0xD2, 0xD3, 0xD4, 0xD5, 0xD6, 0xD7, 0xD8, 0xD9, 0xDA, 0xE1, 0xE2,
    0xE3, 0xE4, 0xE5, 0xE6, 0xE7, 0xE8, 0xE9, 0xEA, 0xF1, 0xF2, 0xF3, 0xF4, 0xF5, 0xF6, 0xF7, 0xF8, 0xF9, 0xFA])
AC_CHROMA = ([0, 2, 1, 2, 4, 4, 3, 4, 7, 5, 4, 4, 0, 1, 2, 0x77], [
    0x00, 0x01, 0x02, 0x03, 0x11, 0x04, 0x05, 0x21, 0x31, 0x06, 0x12, 0x41, 0x51, 0x07, 0x61, 0x71, 0x13, 0x22, 0x32, 0x81, 0x08, 0x14, 0x42, 0x91,
    0xA1, 0xB1, 0xC1, 0x09, 0x23, 0x33, 0x52, 0xF0, 0x15, 0x62, 0x72, 0xD1, 0x0A, 0x16, 0x24, 0x34, 0xE1, 0x25, 0xF1, 0x17, 0x18, 0x19, 0x1A, 0x26,
    0x27, 0x28, 0x29, 0x2A, 0x35, 0x36, 0x37, 0x38, 0x39, 0x3A, 0x43, 0x44, 0x45, 0x46, 0x47, 0x48, 0x49, 0x4A, 0x53, 0x54, 0x55, 0x56, 0x57, 0x58,
    0x59, 0x5A, 0x63, 0x64, 0x65, 0x66, 0x67, 0x68, 0x69, 0x6A, 0x73, 0x74, 0x75, 0x76, 0x77, 0x78, 0x79, 0x7A, 0x82, 0x83, 0x84, 0x85, 0x86, 0x87,
    0x88, 0x89, 0x8A, 0x92, 0x93, 0x94, 0x95, 0x96, 0x97, 0x98, 0x99, 0x9A, 0xA2, 0xA3, 0xA4, 0xA5, 0xA6, 0xA7, 0xA8, 0xA9, 0xAA, 0xB2, 0xB3, 0xB4,
    0xB5, 0xB6, 0xB7, 0xB8, 0xB9, 0xBA, 0xC2, 0xC3, 0xC4, 0xC5, 0xC6, 0xC7, 0xC8, 0xC9, 0xCA, 0xD2, 0xD3, 0xD4, 0xD5, 0xD6, 0xD7, 0xD8, 0xD9, 0xDA,
    0xE2, 0xE3, 0xE4, 0xE5, 0xE6, 0xE7, 0xE8, 0xE9, 0xEA, 0xF2, 0xF3, 0xF4, 0xF5, 0xF6, 0xF7, 0xF8, 0xF9, 0xFA])

DEFAULT_QUALITY = 75


def quant_table(base, quality):
    """The Annex K table at a quality (natural order): scale 5000/q below 50, 200 - 2q from 50 up; (base * s + 50) / 100 in 1..255."""
    s = 5000 // quality if quality < 50 else 200 - 2 * quality
    return np.clip((base.astype(np.int64) * s + 50) // 100, 1, 255)


def huff_codes(spec):
    """(bits, vals) -> (code[256], length[256]) by symbol; length 0: no code."""
    bits, vals = spec
    code = np.zeros(256, np.uint64)
    length = np.zeros(256, np.int64)
    c, k = 0, 0
    for ln in range(1, 17):
        for _ in range(bits[ln - 1]):
            code[vals[k]], length[vals[k]] = c, ln
            c += 1
            k += 1
        c <<= 1
    return code, length


def _segment(marker, payload):
    return bytes([0xFF, marker]) + (len(payload) + 2).to_bytes(2, "big") + payload


def header(h, w, c, quality=DEFAULT_QUALITY):
    """Everything in front of the entropy-coded data: SOI, APP0, DQT per table, SOF0, DHT per table, SOS."""
    out = b"\xff\xd8" + _segment(0xE0, b"JFIF\0" + bytes([1, 1, 0, 0, 1, 0, 1, 0, 0]))
    tables = [Q_LUMA, Q_CHROMA][:2 if c == 3 else 1]
    for i, t in enumerate(tables):
        out += _segment(0xDB, bytes([i]) + bytes(quant_table(t, quality)[ZIGZAG].astype(np.uint8).tolist()))
    comps = [(1, 0x22, 0), (2, 0x11, 1), (3, 0x11, 1)] if c == 3 else [(1, 0x11, 0)]
    out += _segment(0xC0, bytes([8]) + h.to_bytes(2, "big") + w.to_bytes(2, "big") + bytes([len(comps)]) + b"".join(bytes(x) for x in comps))
    dht = [(0x00, DC_LUMA), (0x10, AC_LUMA), (0x01, DC_CHROMA), (0x11, AC_CHROMA)][:4 if c == 3 else 2]
    for tc_th, (bits, vals) in dht:
        out += _segment(0xC4, bytes([tc_th]) + bytes(bits) + bytes(vals))
    sel = [(1, 0x00), (2, 0x11), (3, 0x11)] if c == 3 else [(1, 0x00)]
    out += _segment(0xDA, bytes([len(sel)]) + b"".join(bytes(x) for x in sel) + bytes([0, 63, 0]))
    return out


def _descale(x, n):
    return (x + (1 << (n - 1))) >> n


def _fdct_pass(d, first):
    """One pass of libjpeg's jfdctint (CONST_BITS 13, PASS1_BITS 2) along the last axis."""
    d = [d[..., k] for k in range(8)]
    t0, t7, t1, t6 = d[0] + d[7], d[0] - d[7], d[1] + d[6], d[1] - d[6]
    t2, t5, t3, t4 = d[2] + d[5], d[2] - d[5], d[3] + d[4], d[3] - d[4]
    t10, t13, t11, t12 = t0 + t3, t0 - t3, t1 + t2, t1 - t2
    n = 11 if first else 15
    o = [None] * 8
    if first:
        o[0], o[4] = (t10 + t11) << 2, (t10 - t11) << 2
    else:
        o[0], o[4] = _descale(t10 + t11, 2), _descale(t10 - t11, 2)
    z1 = (t12 + t13) * 4433
    o[2] = _descale(z1 + t13 * 6270, n)
    o[6] = _descale(z1 - t12 * 15137, n)
    z1, z2, z3, z4 = t4 + t7, t5 + t6, t4 + t6, t5 + t7
    z5 = (z3 + z4) * 9633
    t4, t5, t6, t7 = t4 * 2446, t5 * 16819, t6 * 25172, t7 * 12299
    z1, z2, z3, z4 = z1 * -7373, z2 * -20995, z3 * -16069 + z5, z4 * -3196 + z5
    o[7], o[5], o[3], o[1] = _descale(t4 + z1 + z3, n), _descale(t5 + z2 + z4, n), _descale(t6 + z2 + z3, n), _descale(t7 + z1 + z4, n)
    return np.stack(o, axis=-1)


def fdct(blocks):
    """blocks [..., 8, 8] level-shifted samples -> coefficients scaled by 8: rows first, then columns."""
    x = _fdct_pass(blocks.astype(np.int64), True)
    return np.swapaxes(_fdct_pass(np.swapaxes(x, -1, -2), False), -1, -2)


def quantise(coef, table):
    """coef [..., 8, 8] (scaled by 8), table [64] natural order -> sign(c) * ((|c| + (8q >> 1)) / (8q))."""
    q8 = (table.reshape(8, 8) * 8).astype(np.int64)
    return np.sign(coef) * ((np.abs(coef) + (q8 >> 1)) // q8)


def _pad_edge(p, rows, cols):
    return np.pad(p, ((0, rows - p.shape[0]), (0, cols - p.shape[1])), mode="edge")


def _blocks(p):
    """[8 bh, 8 bw] -> [bh, bw, 8, 8]."""
    return p.reshape(p.shape[0] // 8, 8, p.shape[1] // 8, 8).swapaxes(1, 2)


def _zz(q):
    return q.reshape(q.shape[:-2] + (64,))[..., ZIGZAG]


def scan_blocks(img, quality=DEFAULT_QUALITY):
    """img uint8 [h, w, 3] or [h, w] -> (coefficients int64 [blocks, 64] in zigzag order with the DC DIFFERENCE at 0, table index per
    block [blocks]) in scan order: Y00 Y01 Y10 Y11 Cb Cr per 16 x 16 MCU, dummy blocks included; greyscale: the blocks row-major."""
    img = np.asarray(img)
    if img.ndim == 3 and img.shape[2] == 1:
        img = img[..., 0]
    h, w = img.shape[:2]
    bh, bw = -(-h // 8), -(-w // 8)
    ql, qc = quant_table(Q_LUMA, quality), quant_table(Q_CHROMA, quality)
    if img.ndim == 2:
        y = _pad_edge(img.astype(np.int64), 8 * bh, 8 * bw) - 128
        z = _zz(quantise(fdct(_blocks(y)), ql)).reshape(-1, 64)
        z[:, 0] = np.diff(z[:, 0], prepend=0)
        return z, np.zeros(len(z), np.int64)
    r, g, b = (img[..., k].astype(np.int64) for k in range(3))
    y = (19595 * r + 38470 * g + 7471 * b + 32768) >> 16
    cb = (-11059 * r - 21709 * g + 32768 * b + (128 << 16) + 32767) >> 16
    cr = (32768 * r - 27439 * g - 5329 * b + (128 << 16) + 32767) >> 16
    mh, mw = -(-h // 16), -(-w // 16)
    zy = _zz(quantise(fdct(_blocks(_pad_edge(y, 8 * bh, 8 * bw) - 128)), ql))                    # [bh, bw, 64]
    real = np.zeros((2 * mh, 2 * mw), bool)
    real[:bh, :bw] = True
    full = np.zeros((2 * mh, 2 * mw, 64), np.int64)
    full[:bh, :bw] = zy
    # luma in MCU order [mh, mw, 2, 2]; a dummy block is all zero with the DC of the block before it in its MCU: its difference is 0
    order = lambda a: a.reshape((mh, 2, mw, 2) + a.shape[2:]).swapaxes(1, 2)
    zl = order(full).reshape(-1, 64)
    rl = order(real).reshape(-1)
    idx = np.maximum.accumulate(np.where(rl, np.arange(len(rl)), 0))          # the last real block at or before each (block 0 is real)
    dc = zl[idx, 0]
    zl[:, 0] = np.diff(dc, prepend=0)
    chroma = []
    bias = np.tile(np.array([1, 2]), 8 * mw // 2)
    for p in (cb, cr):
        p = _pad_edge(p, h + (h & 1), 16 * mw)                                # columns to the MCU grid, rows to an even count ONLY
        d = (p[0::2, 0::2] + p[0::2, 1::2] + p[1::2, 0::2] + p[1::2, 1::2] + bias) >> 2
        d = _pad_edge(d, 8 * mh, 8 * mw)                                      # the rows of whole blocks are replicated AFTER the downsample
        z = _zz(quantise(fdct(_blocks(d - 128)), qc)).reshape(-1, 64)
        z[:, 0] = np.diff(z[:, 0], prepend=0)
        chroma.append(z)
    z = np.concatenate([zl.reshape(mh * mw, 4, 64), chroma[0][:, None], chroma[1][:, None]], axis=1).reshape(-1, 64)
    return z, np.tile(np.array([0, 0, 0, 0, 1, 1]), mh * mw)


_TABLES = None


def _huff():
    global _TABLES
    if _TABLES is None:
        dc = [huff_codes(DC_LUMA), huff_codes(DC_CHROMA)]
        ac = [huff_codes(AC_LUMA), huff_codes(AC_CHROMA)]
        _TABLES = (np.stack([t[0] for t in dc]), np.stack([t[1] for t in dc]), np.stack([t[0] for t in ac]), np.stack([t[1] for t in ac]))
    return _TABLES


def run_sizes(z):
    """Per coefficient of z [blocks, 64] (DC difference at 0): (coded bool - the DC and every non-zero AC; run - the zeros between it and
    the coded coefficient before it, 0..62, 0 at the DC; size - bit_length(|v|); last - the last coded position at or before each)."""
    nb = len(z)
    pos = np.arange(64)
    nz = z != 0
    nz[:, 0] = True
    last = np.maximum.accumulate(np.where(nz, pos, 0), axis=1)                # the last coded position at or before each
    run = pos[None, :] - np.concatenate([np.zeros((nb, 1), np.int64), last[:, :-1]], axis=1) - 1
    run[:, 0] = 0
    a = np.abs(z)
    size = sum((a >> k) > 0 for k in range(12)).astype(np.int64)              # bit_length(|v|)
    return nz, run, size, last


def entropy_bits(z, tbl):
    """Per coefficient of z [blocks, 64] (DC difference at 0) the bits it puts into the stream as (pattern uint64, right-aligned; length):
    a non-zero AC coefficient carries the ZRLs of its run, its run/size code and its value bits; the DC always codes; the last coded
    coefficient of a block that does not end at 63 carries the EOB as well.  Length 0: nothing."""
    dcc, dcl, acc, acl = _huff()
    u = np.uint64
    pos = np.arange(64)
    nz, run, size, last = run_sizes(z)
    val = (np.where(z < 0, z - 1, z) & ((1 << size) - 1)).astype(u)
    t = tbl[:, None]
    sym = np.where(nz, ((run & 15) << 4) | size, 0)
    code = np.where(pos[None, :] == 0, dcc[t, np.minimum(size, 11)], acc[t, sym])
    clen = np.where(pos[None, :] == 0, dcl[t, np.minimum(size, 11)], acl[t, sym])
    pat = (code << size.astype(u)) | val
    ln = clen + size
    zrl_c, zrl_l = acc[t, 0xF0], acl[t, 0xF0]
    for k in (1, 2, 3):
        m = (run >> 4) >= k
        pat = np.where(m, pat | (zrl_c << ln.astype(u)), pat)
        ln = np.where(m, ln + zrl_l, ln)
    eob = nz & (last[:, -1:] == pos[None, :]) & (pos[None, :] < 63)
    eob_l = acl[t, 0]
    pat = np.where(eob, (pat << eob_l.astype(u)) | acc[t, 0], pat)
    ln = np.where(eob, ln + eob_l, ln)
    return pat.astype(u), np.where(nz, ln, 0)


def pack_bits(pat, ln):
    """The coded bits in order, the last byte padded with 1-bits, then a 0x00 stuffed behind every 0xFF."""
    pat, ln = pat.reshape(-1), ln.reshape(-1)
    keep = ln > 0
    pat, ln = pat[keep], ln[keep]
    shifts = np.arange(63, -1, -1, dtype=np.uint64)
    parts = []
    for a in range(0, len(pat), 1 << 16):
        p, l = pat[a:a + (1 << 16)], ln[a:a + (1 << 16)]
        left = p << (64 - l).astype(np.uint64)
        bits = ((left[:, None] >> shifts[None, :]) & np.uint64(1)).astype(np.uint8)
        parts.append(bits[np.arange(64)[None, :] < l[:, None]])
    bits = np.concatenate(parts) if parts else np.zeros(0, np.uint8)
    bits = np.concatenate([bits, np.ones(-len(bits) % 8, np.uint8)])
    data = np.packbits(bits)
    ff = np.nonzero(data == 0xFF)[0]
    return np.insert(data, ff + 1, 0).tobytes()


def encode(img, quality=DEFAULT_QUALITY):
    """uint8 [h, w, 3] (RGB), [h, w] or [h, w, 1] (L) -> the bytes of the file."""
    img = np.asarray(img)
    assert img.dtype == np.uint8 and img.ndim in (2, 3) and (img.ndim == 2 or img.shape[2] in (1, 3))
    h, w = img.shape[:2]
    c = 3 if img.ndim == 3 and img.shape[2] == 3 else 1
    z, tbl = scan_blocks(img, quality)
    return header(h, w, c, quality) + pack_bits(*entropy_bits(z, tbl)) + b"\xff\xd9"


def max_block_bits():
    """The most bits one block can put into the stream with these tables: a DC difference of 11 bits and 63 AC coefficients of 10."""
    _, dcl, _, acl = _huff()
    dc = max(int(dcl[t, s]) + s for t in range(2) for s in range(12))
    ac = max(int(acl[t, (r << 4) | s]) + s for t in range(2) for r in range(16) for s in range(1, 11))
    return dc + 63 * ac


# ---- the test content of the issue: shapes, modes and kinds of content ------------------------------------------------------------------
SHAPES = [(1, 1), (8, 8), (17, 9), (24, 40), (37, 53), (40, 72), (64, 64), (250, 333), (256, 456)]
CONTENTS = ["noise", "smooth", "binary", "white", "black"]


def content(kind, h, w, c, seed=0):
    """uint8 [h, w, 3] or [h, w]: uniform noise, a smooth field, random 0/255, constant 255, constant 0."""
    rng = np.random.default_rng(seed + 1000 * h + w + (7 if c == 3 else 0))
    shape = (h, w, 3) if c == 3 else (h, w)
    if kind == "noise":
        return rng.integers(0, 256, shape, dtype=np.uint8)
    if kind == "binary":
        return (rng.integers(0, 2, shape, dtype=np.uint8) * 255).astype(np.uint8)
    if kind == "white":
        return np.full(shape, 255, np.uint8)
    if kind == "black":
        return np.zeros(shape, np.uint8)
    assert kind == "smooth"
    yy, xx = np.mgrid[0:h, 0:w].astype(np.float64)
    planes = [127.5 + 100 * np.sin(xx / (11.0 + 3 * k) + k) * np.cos(yy / (17.0 - 2 * k)) + rng.normal(0, 2.0, (h, w)) for k in range(3)]
    a = np.clip(np.rint(np.stack(planes, axis=-1)), 0, 255).astype(np.uint8)
    return a if c == 3 else np.ascontiguousarray(a[..., 0])
