"""Plain NumPy / Python restatement of the device JPEG file decoder (csrc/jpeg_decode.hip, adain_jpeg_decode_u8): the marker walk, a sequential
Huffman decoder, the DC sums and the back half (dequantisation with the file's tables, libjpeg's islow IDCT, its three upsamplers, its
YCbCr -> RGB map) - and the fixed-point scheme the device uses to decode a stream in parallel, simulated lane by lane.  The IDCT and
the h2v2 upsampler are tests/jpeg_decode_ref.py's, imported.  tests/test_jpeg_file_host.py holds all of it to Pillow.

The entropy decoder's rules (the ones the device shares, so that garbage decodes the same way on both sides)
  stream   the segment with the 00 behind every FF removed; bits big-endian; past its end the reader returns 1-bits
  symbol   the shortest code of the component's table that matches; no code of 1..16 bits matches: ONE bit is consumed, nothing else changes
  DC       zigzag index 0: symbol = size s (low 4 bits), then s bits v, difference = v if v >= 2^(s-1) else v - 2^s + 1; index becomes 1
  AC       symbol = run r << 4 | size s.  s = 0: r = 15 skips 16 positions, any other r ends the block.  s > 0: r zeros, then the
           coefficient at index + r (a position past 63 is not written) and the index moves behind it.  An index of 64 or more ends the block
  blocks   per MCU h*v luma blocks row-major, then Cb, Cr (grey: one block); a finished block moves on to the next, modulo the MCU
  damage   (only in blocks below the expected count) a missing code, a DC size above 11, an AC size above 10 or a coefficient past 63
           marks the file; so does a DC sum outside -2047..2047, a block count below the expected one and a last block that does not
           end inside the last byte.  A marked file has a non-zero status.
"""
import numpy as np

import jpeg_decode_ref as D
from jpeg_ref import ZIGZAG

LUMA_HV = {0: (1, 1), 1: (2, 1), 2: (2, 2)}


class Refused(Exception):
    pass


# ---- the marker walk ---------------------------------------------------------------------------------------------------------------------
def parse(data):
    """bytes -> dict(h, w, c, sampling, q [c,64] natural, huff {(class, id): (bits, vals)}, dc, ac, seg (offset, length)) or Refused."""
    if data[:2] != b"\xff\xd8":
        raise Refused("no SOI")
    q, huff, frame, at, adobe = {}, {}, None, 2, None
    while True:
        if at + 4 > len(data) or data[at] != 0xFF:
            raise Refused("truncated or no marker")
        m = data[at + 1]
        if m == 0xFF:
            at += 1
            continue
        ln = int.from_bytes(data[at + 2:at + 4], "big")
        if ln < 2 or at + 2 + ln > len(data):
            raise Refused("segment past the end")
        body = data[at + 4:at + 2 + ln]
        if m in (0xC0, 0xC1):
            if frame is not None or body[0] != 8 or body[5] not in (1, 3) or len(body) != 6 + 3 * body[5]:
                raise Refused("frame header")
            comps = [(body[6 + 3 * i], body[7 + 3 * i] >> 4, body[7 + 3 * i] & 15, body[8 + 3 * i]) for i in range(body[5])]
            hv = (comps[0][1], comps[0][2])
            ok = [c[0] for c in comps] == list(range(1, len(comps) + 1)) and all(c[1:3] == (1, 1) for c in comps[1:])
            ok = ok and (hv in ((1, 1), (2, 1), (2, 2)) if len(comps) == 3 else hv == (1, 1))
            h, w = int.from_bytes(body[1:3], "big"), int.from_bytes(body[3:5], "big")
            if not ok or h == 0 or w == 0:
                raise Refused("components or sampling")
            frame = (h, w, comps)
        elif 0xC0 <= m <= 0xCF and m not in (0xC4, 0xC8, 0xCC) or m in (0xDC, 0xD8, 0xD9, 0x01) or 0xD0 <= m <= 0xD7:
            raise Refused(f"marker {m:02X}")
        elif m == 0xDB:
            for p in range(0, len(body), 65):
                if body[p] > 3 or p + 65 > len(body):
                    raise Refused("DQT")
                t = np.zeros(64, np.int64)
                t[ZIGZAG] = list(body[p + 1:p + 65])
                q[body[p]] = t
        elif m == 0xC4:
            p = 0
            while p < len(body):
                bits = list(body[p + 1:p + 17])
                if len(bits) < 16 or body[p] >> 4 > 1 or body[p] & 15 > 3 or sum(bits) > 256 or p + 17 + sum(bits) > len(body):
                    raise Refused("DHT")
                c_ = 0
                for i, b in enumerate(bits):
                    c_ += b
                    if c_ > 1 << (i + 1):
                        raise Refused("DHT: too many codes")
                    c_ <<= 1
                huff[(body[p] >> 4, body[p] & 15)] = (bits, list(body[p + 17:p + 17 + sum(bits)]))
                p += 17 + sum(bits)
        elif m == 0xDD:
            if int.from_bytes(body, "big") != 0:
                raise Refused("restart interval")
        elif m == 0xEE and body[:5] == b"Adobe" and len(body) >= 12:
            adobe = body[11]
        elif m == 0xDA:
            if frame is None:
                raise Refused("scan before frame")
            h, w, comps = frame
            if len(body) != 4 + 2 * len(comps) or body[0] != len(comps) or tuple(body[-3:]) != (0, 63, 0) or (adobe == 0 and len(comps) == 3):
                raise Refused("scan header")
            sel = [(body[1 + 2 * i], body[2 + 2 * i] >> 4, body[2 + 2 * i] & 15) for i in range(len(comps))]
            if [s[0] for s in sel] != [c[0] for c in comps] or any(d > 1 or a > 1 or (0, d) not in huff or (1, a) not in huff for _, d, a in sel):
                raise Refused("scan tables")
            if any(c[3] not in q for c in comps):
                raise Refused("quantisation table")
            seg = end = at + 2 + ln
            while True:
                end = data.find(b"\xff", end)
                if end < 0 or end + 1 >= len(data):
                    raise Refused("no EOI")
                if data[end + 1] != 0:
                    break
                end += 2
            if data[end + 1] != 0xD9:
                raise Refused("a marker other than EOI behind the scan")
            return dict(h=h, w=w, c=len(comps), sampling={(1, 1): 0, (2, 1): 1, (2, 2): 2}[comps[0][1:3]], q=np.stack([q[c[3]] for c in comps]),
                        huff=huff, dc=[s[1] for s in sel], ac=[s[2] for s in sel], seg=(seg, end - seg))
        at += 2 + ln


# ---- the entropy decoder -------------------------------------------------------------------------------------------------------------------
def code_table(bits, vals):
    """BITS / HUFFVAL -> a list over the next 16 bits of the stream: (symbol, code length) of the code that starts there, or None."""
    out, code, k = [None] * 65536, 0, 0
    for ln in range(1, 17):
        for _ in range(bits[ln - 1]):
            out[code << (16 - ln):(code + 1) << (16 - ln)] = [(vals[k], ln)] * (1 << (16 - ln))
            code += 1
            k += 1
        code <<= 1
    return out


def unstuff(seg):
    return bytes(seg).replace(b"\xff\x00", b"\xff")


class Stream:
    trace = None             # an object whose symbol(kind, table id, symbol, code length, position, size, value bits) takes the write pass's walk

    def __init__(self, info, data):
        self.dc_id, self.ac_id = list(info["dc"]), list(info["ac"])
        off, ln = info["seg"]
        self.bytes = unstuff(data[off:off + ln])
        self.nbits = 8 * len(self.bytes)
        self.padded = self.bytes + b"\xff" * 16
        hh, vv = LUMA_HV[info["sampling"]]
        self.comp_of = [0] * (hh * vv) + [1, 2] if info["c"] == 3 else [0]
        self.bpm = len(self.comp_of)
        self.dc = [code_table(*info["huff"][(0, t)]) for t in info["dc"]]
        self.ac = [code_table(*info["huff"][(1, t)]) for t in info["ac"]]
        mw, mh = -(-info["w"] // (8 * hh)), -(-info["h"] // (8 * vv))
        self.nblk = mw * mh * self.bpm

    def peek(self, pos, n):
        """n <= 32 bits at pos <= nbits; 1-bits past the end."""
        at = pos >> 3
        return (int.from_bytes(self.padded[at:at + 8], "big") >> (64 - (pos & 7) - n)) & ((1 << n) - 1)

    def symbol(self, table, pos):
        """(symbol, code length) of the shortest code that matches at pos, or (None, 1)."""
        return table[self.peek(pos, 16)] or (None, 1)


def decode_span(st, state, end, sink=None, block=0):
    """Decodes from ``state`` = (pos, block in MCU, zigzag index) while pos < end -> (exit state, blocks begun).  ``sink(b, k, value)``
    takes the coefficients (zigzag index k; k = -1: damage; k = 64: block b ended at ``value``), ``block``: the index of the block that is
    current at ``state`` (the one under way, or the next to begin)."""
    pos, blk, zz = state
    begun = 0
    b = block
    while pos < end:
        comp = st.comp_of[blk]
        if zz == 0:
            sym, ln = st.symbol(st.dc[comp], pos)
            if sym is None:
                pos += 1
                if sink:
                    sink(b, -1, 0)
                continue
            begun += 1
            s = sym & 15
            v = st.peek(pos + ln, s) if s else 0
            if sink and st.trace and 0 <= b < sink.nblk:
                st.trace.symbol("DC", st.dc_id[comp], sym, ln, pos, s, v)
            pos += ln + s
            if sink:
                sink(b, 0, v if s == 0 or v >= 1 << (s - 1) else v - (1 << s) + 1)
                if sym > 11:
                    sink(b, -1, 0)
            zz = 1
        else:
            sym, ln = st.symbol(st.ac[comp], pos)
            if sym is None:
                pos += 1
                if sink:
                    sink(b, -1, 0)
                continue
            r, s = sym >> 4, sym & 15
            if sink and st.trace and 0 <= b < sink.nblk:
                st.trace.symbol("AC", st.ac_id[comp], sym, ln, pos, s, st.peek(pos + ln, s) if s else 0, zz)
            if s == 0:
                pos += ln
                zz = zz + 16 if r == 15 else 64
            else:
                v = st.peek(pos + ln, s)
                pos += ln + s
                k = zz + r
                if sink:
                    if k <= 63 and s <= 10:
                        sink(b, k, v if v >= 1 << (s - 1) else v - (1 << s) + 1)
                    else:
                        sink(b, -1, 0)
                        if k <= 63:
                            sink(b, k, v if v >= 1 << (s - 1) else v - (1 << s) + 1)
                zz = k + 1
        if zz >= 64:
            if sink:
                sink(b, 64, pos)
            zz, blk, b = 0, (blk + 1) % st.bpm, b + 1
    return (pos, blk, zz), begun


class Sink:
    """Coefficients [nblk, 64] in zigzag order, DC as differences; damage and the end of the last block."""

    def __init__(self, nblk):
        self.coef = np.zeros((nblk, 64), np.int64)
        self.damage, self.end, self.nblk = False, None, nblk

    def __call__(self, b, k, v):
        if b >= self.nblk or b < 0:
            return
        if k == -1:
            self.damage = True
        elif k == 64:
            if b == self.nblk - 1:
                self.end = v
        else:
            self.coef[b, k] = v

    def status(self, st):
        return int(self.damage or self.end is None or not st.nbits - 8 < self.end <= st.nbits)


def decode_sequential(st):
    """The whole stream in one go -> Sink."""
    sink = Sink(st.nblk)
    decode_span(st, (0, 0, 0), st.nbits, sink, 0)
    return sink


def decode_lanes(st, chunk_bits):
    """The device's scheme: subsequences of chunk_bits bits, round 0 from the all-zero state at each one's first bit, every later round
    from the left neighbour's exit state, until a round changes no exit state -> (Sink, rounds run, round 0 and the last one included)."""
    assert chunk_bits >= 32 and chunk_bits % 32 == 0
    nsub = -(-st.nbits // chunk_bits)
    ends = [min((s + 1) * chunk_bits, st.nbits) for s in range(nsub)]
    out = [decode_span(st, (s * chunk_bits, 0, 0), ends[s]) for s in range(nsub)]
    prev_in = [(s * chunk_bits, 0, 0) for s in range(nsub)]
    rounds = 1
    while rounds < nsub + 1:
        ins = [(0, 0, 0)] + [o[0] for o in out[:-1]]
        new = [out[s] if ins[s] == prev_in[s] else decode_span(st, ins[s], ends[s]) for s in range(nsub)]
        rounds += 1
        changed = any(a[0] != b[0] for a, b in zip(new, out))
        out, prev_in = new, ins
        if not changed:
            break
    first = np.concatenate([[0], np.cumsum([o[1] for o in out])])
    sink = Sink(st.nblk)
    for s in range(nsub):
        state = (0, 0, 0) if s == 0 else out[s - 1][0]
        decode_span(st, state, ends[s], sink, int(first[s]) - (1 if state[2] else 0))
    return sink, rounds


# ---- the back half ---------------------------------------------------------------------------------------------------------------------------
def upsample_h2v1(c, w):
    """libjpeg's h2v1_fancy_upsample of the ceil(w/2) real columns; from 2 columns down plain replication (h2v1_upsample)."""
    cw = -(-w // 2)
    c = c[:, :cw].astype(np.int64)
    if cw <= 2:
        return np.repeat(c, 2, axis=1)[:, :w]
    left, right = np.concatenate([c[:, :1], c[:, :-1]], axis=1), np.concatenate([c[:, 1:], c[:, -1:]], axis=1)
    out = np.empty((c.shape[0], 2 * cw), np.int64)
    out[:, 0::2] = (3 * c + left + 1) >> 2
    out[:, 1::2] = (3 * c + right + 2) >> 2
    return out[:, :w]


def pixels(info, sink):
    """The decoded coefficients -> uint8 [h, w, 3] or [h, w]; the DC sums run per component over the scan."""
    h, w, c = info["h"], info["w"], info["c"]
    hh, vv = LUMA_HV[info["sampling"]]
    mw, mh = -(-w // (8 * hh)), -(-h // (8 * vv))
    bpm = hh * vv + 2 if c == 3 else 1
    z = sink.coef.reshape(mh * mw, bpm, 64).copy()
    damage = False
    planes = []
    for comp in range(c):
        js = list(range(hh * vv)) if comp == 0 else [hh * vv + comp - 1]
        part = z[:, js]                                                  # [mcus, blocks, 64]
        dc = np.cumsum(part[..., 0].reshape(-1)).reshape(part.shape[:2])
        damage |= bool(np.any(np.abs(dc) > 2047))
        part[..., 0] = ((dc + 32768) & 0xFFFF) - 32768                  # int16, as the coefficient buffer holds it
        nat = np.zeros_like(part)
        nat[..., ZIGZAG] = part
        s = D.idct((nat * info["q"][comp]).reshape(part.shape[:2] + (8, 8)))
        bv, bh_ = (vv, hh) if comp == 0 else (1, 1)
        planes.append(s.reshape(mh, mw, bv, bh_, 8, 8).transpose(0, 2, 4, 1, 3, 5).reshape(mh * bv * 8, mw * bh_ * 8))
    y = planes[0][:h, :w]
    if c == 1:
        return y.astype(np.uint8), damage
    if info["sampling"] == 2:
        cb, cr = (D.upsample(p, h, w) - 128 for p in planes[1:])
    elif info["sampling"] == 1:
        cb, cr = (upsample_h2v1(p[:h], w) - 128 for p in planes[1:])
    else:
        cb, cr = (p[:h, :w].astype(np.int64) - 128 for p in planes[1:])
    rgb = [y + ((91881 * cr + 32768) >> 16), y + ((-22554 * cb - 46802 * cr + 32768) >> 16), y + ((116130 * cb + 32768) >> 16)]
    return np.clip(np.stack(rgb, axis=-1), 0, 255).astype(np.uint8), damage


def decode(data, chunk_bits=None):
    """bytes of a file -> (pixels uint8, status, rounds): sequentially, or (chunk_bits) by the device's scheme."""
    info = parse(data)
    st = Stream(info, data)
    sink, rounds = (decode_sequential(st), 0) if chunk_bits is None else decode_lanes(st, chunk_bits)
    px, damage = pixels(info, sink)
    return px, int(bool(sink.status(st)) or damage), rounds
