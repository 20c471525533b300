"""NumPy restatement of the baseline JPEG file ``Image.fromarray(frame).save(f, format="JPEG", quality=q, subsampling=s, optimize=o)``
writes for s in 0 (4:4:4), 1 (4:2:2), 2 (4:2:0) and o in False / True - the rules the device encoder's option path (csrc/jpeg.hip,
adain_jpeg_encode_opt_u8) runs.  It reuses the pieces of tests/jpeg_ref.py (colour map, DCT, quantiser, bit packing, the 4:2:0 scan)
and adds the two other MCU geometries and libjpeg's two-pass ``optimize_coding``: the symbol histogram of the scan and the optimal
length-limited Huffman code per table slot.  Integer arithmetic throughout: the target is the same bytes, not a tolerance.
tests/test_jpeg_options_host.py holds this to Pillow on the host.
"""
import numpy as np

import jpeg_ref as J

SUBSAMPLING = {0: (1, 1), 1: (2, 1), 2: (2, 2)}          # Pillow's number -> luma sampling factors (horizontal, vertical)
SLOTS = ["DC0", "AC0", "DC1", "AC1"]                      # the order of the DHT segments in the file


def scan_blocks(img, quality=J.DEFAULT_QUALITY, subsampling=2):
    """jpeg_ref.scan_blocks for the three chroma layouts: (coefficients [blocks, 64] in zigzag order with the DC DIFFERENCE at 0, table
    index per block) in scan order.  4:4:4: Y Cb Cr per 8 x 8 MCU, the chroma planes edge-replicated to whole blocks.  4:2:2: Y0 Y1 Cb
    Cr per 16 x 8 MCU; the chroma columns are replicated to the MCU grid at full resolution and downsampled as (a + b + bias) >> 1 with
    bias 0 on even output columns and 1 on odd ones; a luma block beyond ceil(w/8) is a dummy (AC zero, the DC of the block before it)."""
    img = np.asarray(img)
    if img.ndim == 3 and img.shape[2] == 1:
        img = img[..., 0]
    if img.ndim == 2 or subsampling == 2:
        return J.scan_blocks(img, quality)
    hs = SUBSAMPLING[subsampling][0]
    h, w = img.shape[:2]
    bh, bw = -(-h // 8), -(-w // 8)
    mh, mw = bh, -(-w // (8 * hs))
    ql, qc = J.quant_table(J.Q_LUMA, quality), J.quant_table(J.Q_CHROMA, quality)
    r, g, b = (img[..., k].astype(np.int64) for k in range(3))
    y = (19595 * r + 38470 * g + 7471 * b + 32768) >> 16
    cb = (-11059 * r - 21709 * g + 32768 * b + (128 << 16) + 32767) >> 16
    cr = (32768 * r - 27439 * g - 5329 * b + (128 << 16) + 32767) >> 16
    full = np.zeros((bh, hs * mw, 64), np.int64)
    full[:, :bw] = J._zz(J.quantise(J.fdct(J._blocks(J._pad_edge(y, 8 * bh, 8 * bw) - 128)), ql))
    real = np.zeros((bh, hs * mw), bool)
    real[:, :bw] = True
    zl, rl = full.reshape(-1, 64), real.reshape(-1)          # the luma blocks of an MCU are neighbours in a block row: row-major IS MCU order
    idx = np.maximum.accumulate(np.where(rl, np.arange(len(rl)), 0))
    zl[:, 0] = np.diff(zl[idx, 0], prepend=0)
    chroma = []
    for p in (cb, cr):
        p = J._pad_edge(p, h, 8 * hs * mw)
        if hs == 2:
            p = (p[:, 0::2] + p[:, 1::2] + np.tile(np.array([0, 1]), 4 * mw)) >> 1
        z = J._zz(J.quantise(J.fdct(J._blocks(J._pad_edge(p, 8 * mh, 8 * mw) - 128)), qc)).reshape(-1, 64)
        z[:, 0] = np.diff(z[:, 0], prepend=0)
        chroma.append(z)
    z = np.concatenate([zl.reshape(mh * mw, hs, 64), chroma[0][:, None], chroma[1][:, None]], axis=1).reshape(-1, 64)
    return z, np.tile(np.array([0] * hs + [1, 1]), mh * mw)


def symbol_counts(z, tbl):
    """The symbols the entropy coder emits for z [blocks, 64] (DC difference at 0), counted per table slot: int64 [4, 256] in the order
    DC0, AC0, DC1, AC1.  DC: the category.  AC: the run/size symbol of every non-zero coefficient, 0xF0 once per ZRL, 0x00 per EOB."""
    counts = np.zeros((4, 256), np.int64)
    nz, run, size, last = J.run_sizes(z)
    for t in (0, 1):
        m = tbl == t
        if not m.any():
            continue
        counts[2 * t] += np.bincount(size[m, 0], minlength=256)
        ac = nz[m, 1:]
        counts[2 * t + 1] += np.bincount((((run[m, 1:] & 15) << 4) | size[m, 1:])[ac], minlength=256)
        counts[2 * t + 1, 0xF0] += int((run[m, 1:] >> 4)[ac].sum())
        counts[2 * t + 1, 0x00] += int((last[m, -1] < 63).sum())
    return counts


def code_sizes(freq):
    """libjpeg's jpeg_gen_optimal_table, first half: the UNRESTRICTED Huffman code length of each of the 256 symbols and of the
    pseudo-symbol 256 (frequency 1, so that no real symbol gets the all-ones code); 0: the symbol does not occur.  Merge until one tree
    is left: c1 = the smallest non-zero frequency, among equals the largest index; c2 = the same without c1."""
    f = [int(x) for x in freq] + [1]
    assert len(f) == 257 and min(f) >= 0
    size = [0] * 257
    others = [-1] * 257

    def smallest(skip):
        best = -1
        for i in range(257):
            if f[i] and i != skip and (best < 0 or f[i] <= f[best]):
                best = i
        return best

    while True:
        c1 = smallest(-1)
        c2 = smallest(c1)
        if c2 < 0:
            return size
        f[c1] += f[c2]
        f[c2] = 0
        size[c1] += 1
        while others[c1] >= 0:
            c1 = others[c1]
            size[c1] += 1
        others[c1] = c2
        size[c2] += 1
        while others[c2] >= 0:
            c2 = others[c2]
            size[c2] += 1


def optimal_table(freq):
    """freq [256] -> (bits [16], vals): the DHT of libjpeg's optimal table.  The code lengths of ``code_sizes`` are counted per length,
    limited to 16 as in Annex K.3 (from the longest down to 17: take two from length i, give one to i - 1; take one from the largest
    j <= i - 2 that has any, give two to j + 1), the pseudo-symbol leaves the longest length, and the symbols are listed by unrestricted
    length, then by value."""
    size = code_sizes(freq)
    top = max(max(size), 32)
    bits = [0] * (top + 1)
    for s in size:
        if s:
            bits[s] += 1
    for i in range(top, 16, -1):
        while bits[i] > 0:
            j = i - 2
            while bits[j] == 0:
                j -= 1
            bits[i] -= 2
            bits[i - 1] += 1
            bits[j + 1] += 2
            bits[j] -= 1
    i = 16
    while bits[i] == 0:
        i -= 1
    bits[i] -= 1
    vals = [s for ln in range(1, top + 1) for s in range(256) if size[s] == ln]
    assert sum(bits[1:17]) == len(vals)
    return bits[1:17], vals


def dht_segments(dht, ids=(0x00, 0x10, 0x01, 0x11), one_segment=False):
    """The DHT segment(s) of the (bits, vals) tables ``dht`` under the class / id bytes ``ids``: one segment each, or all in one."""
    parts = [bytes([tc_th]) + bytes(bits) + bytes(vals) for tc_th, (bits, vals) in zip(ids, dht)]
    if one_segment:
        return J._segment(0xC4, b"".join(parts)) if parts else b""
    return b"".join(J._segment(0xC4, p) for p in parts)


def sos_segment(sel, ss=0, se=63, ah=0, al=0):
    """The SOS segment of a scan of the components ``sel``: (component id, DC table << 4 | AC table) each."""
    return J._segment(0xDA, bytes([len(sel)]) + b"".join(bytes(x) for x in sel) + bytes([ss, se, ah << 4 | al]))


def header(h, w, c, quality, subsampling, dht, *, qtables=None, qsel=None, dht_ids=(0x00, 0x10, 0x01, 0x11), one_dht=False, sel=None, sof=0xC0, ri=0,
           fill=False, sos=True):
    """jpeg_ref.header with the luma sampling factors of the layout and the four (two for L) given (bits, vals) tables.  The keywords
    write the headers other encoders write: ``qtables`` [(id, natural-order table)] in place of the quality's two, ``qsel`` the table
    id per component, ``dht_ids`` the class / id byte of each table of ``dht`` (any number, an id may come twice: the later definition
    holds), ``one_dht`` all of them in one segment, ``sel`` DC << 4 | AC per component, ``sof`` the frame marker, ``ri`` a DRI segment,
    ``fill`` an FF fill byte in front of the frame header's marker, ``sos`` False: no SOS segment (a progressive file writes its own)."""
    out = b"\xff\xd8" + J._segment(0xE0, b"JFIF\0" + bytes([1, 1, 0, 0, 1, 0, 1, 0, 0]))
    if qtables is None:
        qtables = list(enumerate(J.quant_table(t, quality) for t in [J.Q_LUMA, J.Q_CHROMA][:2 if c == 3 else 1]))
    for i, t in qtables:
        out += J._segment(0xDB, bytes([i]) + bytes(np.asarray(t)[J.ZIGZAG].astype(np.uint8).tolist()))
    hs, vs = SUBSAMPLING[subsampling]
    qsel = qsel or (0, 1, 1)
    comps = [(1, hs << 4 | vs, qsel[0]), (2, 0x11, qsel[1]), (3, 0x11, qsel[2])] if c == 3 else [(1, 0x11, qsel[0])]
    out += b"\xff" * bool(fill)
    out += J._segment(sof, bytes([8]) + h.to_bytes(2, "big") + w.to_bytes(2, "big") + bytes([len(comps)]) + b"".join(bytes(x) for x in comps))
    if ri:
        out += J._segment(0xDD, ri.to_bytes(2, "big"))
    out += dht_segments(dht, dht_ids, one_dht)
    sel = sel or (0x00, 0x11, 0x11)
    return out + sos_segment([(i + 1, sel[i]) for i in range(c)]) if sos else out


def entropy_data(z, tbl, dht):
    """The entropy-coded segment of z [blocks, 64] under the tables ``dht`` (slot order): jpeg_ref.entropy_bits for any tables.  An
    optimal code may give ZRL and EOB 16 bits, so a coefficient's contribution no longer fits one 64-bit pattern: its (up to three) ZRLs,
    its code with the value bits and the EOB are packed as parts of their own."""
    u = np.uint64
    codes = [J.huff_codes(spec) for spec in dht]
    dcc, dcl, acc, acl = (np.stack([codes[2 * k + ac][i] for k in range(len(codes) // 2)]) for ac in (0, 1) for i in (0, 1))          # [tables, 256]
    shifts = np.arange(63, -1, -1, dtype=u)
    chunks = []
    for a in range(0, len(z), 1 << 14):
        zz = z[a:a + (1 << 14)]
        nz, run, size, last = J.run_sizes(zz)
        blk, pos = np.nonzero(nz)                                  # the coded coefficients, in stream order
        v, run, size, t = zz[blk, pos], run[blk, pos], size[blk, pos], tbl[a:a + (1 << 14)][blk]
        val = (np.where(v < 0, v - 1, v) & ((1 << size) - 1)).astype(u)
        sym = ((run & 15) << 4) | size
        code = np.where(pos == 0, dcc[t, np.minimum(size, 255)], acc[t, sym])
        clen = np.where(pos == 0, dcl[t, np.minimum(size, 255)], acl[t, sym])
        assert bool((clen > 0).all()), "a symbol without a code"
        pat = np.zeros((len(v), 5), u)
        ln = np.zeros((len(v), 5), np.int64)
        for k in (1, 2, 3):
            m = (pos > 0) & ((run >> 4) >= k)
            pat[:, k - 1] = np.where(m, acc[t, 0xF0], 0)
            ln[:, k - 1] = np.where(m, acl[t, 0xF0], 0)
        pat[:, 3] = (code << size.astype(u)) | val
        ln[:, 3] = clen + size
        eob = (last[blk, -1] == pos) & (pos < 63)
        pat[:, 4] = np.where(eob, acc[t, 0], 0)
        ln[:, 4] = np.where(eob, acl[t, 0], 0)
        pat, ln = pat.reshape(-1), ln.reshape(-1)
        keep = ln > 0
        pat, ln = pat[keep], ln[keep]
        left = pat << (64 - ln).astype(u)
        for b in range(0, len(pat), 1 << 16):
            bits = ((left[b:b + (1 << 16), None] >> shifts[None, :]) & u(1)).astype(np.uint8)
            chunks.append(bits[np.arange(64)[None, :] < ln[b:b + (1 << 16), None]])
    bits = np.concatenate(chunks) if chunks else np.zeros(0, np.uint8)
    data = np.packbits(np.concatenate([bits, np.ones(-len(bits) % 8, np.uint8)]))
    return np.insert(data, np.nonzero(data == 0xFF)[0] + 1, 0).tobytes()


STANDARD = [J.DC_LUMA, J.AC_LUMA, J.DC_CHROMA, J.AC_CHROMA]


def tables_for(z, tbl, c, optimize):
    """The (bits, vals) of the file's DHT segments in slot order: Annex K's, or the optimal ones of the scan's own symbol counts."""
    slots = 4 if c == 3 else 2
    if not optimize:
        return STANDARD[:slots]
    return [optimal_table(f) for f in symbol_counts(z, tbl)[:slots]]


def encode(img, quality=J.DEFAULT_QUALITY, subsampling=2, optimize=False):
    """uint8 [h, w, 3] (RGB), [h, w] or [h, w, 1] (L) -> the bytes of the file.  L ignores ``subsampling``, as Pillow does."""
    img = np.asarray(img)
    assert img.dtype == np.uint8 and img.ndim in (2, 3) and (img.ndim == 2 or img.shape[2] in (1, 3))
    assert subsampling in SUBSAMPLING
    h, w = img.shape[:2]
    c = 3 if img.ndim == 3 and img.shape[2] == 3 else 1
    z, tbl = scan_blocks(img, quality, subsampling)
    dht = tables_for(z, tbl, c, optimize)
    return header(h, w, c, quality, subsampling if c == 3 else 0, dht) + entropy_data(z, tbl, dht) + b"\xff\xd9"


def max_block_bits(optimize):
    """The most bits one block can put into the stream: jpeg_ref's bound for Annex K's tables; for an optimal table every code may be 16
    bits long, so (16 + 11) for the DC difference and 63 x (16 + 10) for the AC coefficients."""
    return (16 + 11) + 63 * (16 + 10) if optimize else J.max_block_bits()


# ---- fixture A: a frame whose AC table needs the length-limiting step ------------------------------------------------------------------
FIXTURE_A_QUALITY = 50
FIXTURE_A_COUNTS = [1, 1] + [1 << k for k in range(1, 18)]          # blocks per run/size symbol: 19 symbols, 2^18 blocks


def _single_coefficient_blocks():
    """8 x 8 uint8 blocks 128 + amp * (one DCT basis function) that quantise, at quality 50 with this file's FDCT and quantiser, to DC 0
    and exactly one non-zero AC at zigzag position k <= 16 with value 1, 2, 4 or 8: {(k, value): block}, found by search over amp."""
    q = J.quant_table(J.Q_LUMA, FIXTURE_A_QUALITY)
    n = np.arange(8)
    cos = np.cos((2 * n[None, :] + 1) * n[:, None] * np.pi / 16)          # [frequency, sample]
    found = {}
    for k in range(1, 17):
        u, v = divmod(int(J.ZIGZAG[k]), 8)
        basis = cos[u][:, None] * cos[v][None, :]
        amps = np.arange(1, 255) * 0.5
        blocks = np.clip(np.rint(128 + amps[:, None, None] * basis[None]), 0, 255).astype(np.int64)
        z = J._zz(J.quantise(J.fdct(blocks - 128), q))
        for value in (1, 2, 4, 8):
            want = np.zeros(64, np.int64)
            want[k] = value
            hit = np.nonzero((z == want[None]).all(axis=1))[0]
            if len(hit):
                found[(k, value)] = blocks[hit[0]].astype(np.uint8)
    return found


def fixture_a():
    """(frame uint8 [4096, 4096], counts) - 2^18 blocks, 19 distinct run/size symbols with the block counts of FIXTURE_A_COUNTS (rarest
    first in ``counts``: {symbol: blocks}); every block also codes DC category 0 and an EOB.  The AC table's unrestricted tree is a chain
    deeper than 16."""
    found = _single_coefficient_blocks()
    keys = sorted(found)[:len(FIXTURE_A_COUNTS)]
    assert len(keys) == len(FIXTURE_A_COUNTS), "too few single-coefficient blocks found"
    which = np.repeat(np.arange(len(keys)), FIXTURE_A_COUNTS)
    blocks = np.stack([found[k] for k in keys])[which].reshape(512, 512, 8, 8)
    frame = np.ascontiguousarray(blocks.swapaxes(1, 2).reshape(4096, 4096))
    counts = {((k - 1) << 4) | int(value).bit_length(): n for (k, value), n in zip(keys, FIXTURE_A_COUNTS)}
    return frame, counts
