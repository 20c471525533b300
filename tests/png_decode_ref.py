"""A plain Python / NumPy restatement of the device PNG decoder (csrc/png_inflate.h, csrc/png_decode.hip), written from RFC 1950 / 1951 and
the PNG specification: inflate with the decoder's statuses, looked for in the decoder's order, the five row filters, and a trace of what
a stream holds (block types, tokens, symbols, code lengths, repeat codes).  Also a tiny LSB-first bit writer and the helpers that
assemble deflate streams and PNG files by hand.  Not a test module.
"""
import struct
import zlib

import numpy as np

OK, TRUNCATED, BLOCK_TYPE, STORED_LEN, OVERSUBSCRIBED, INCOMPLETE, REPEAT, NO_END_OF_BLOCK, BAD_SYMBOL, FAR_DISTANCE, TOO_MUCH, TOO_LITTLE, \
    TRAILING, ADLER, FILTER, UNUSED_CODE, TOO_MANY_SYMBOLS = range(17)
STATUS_NAMES = ["OK", "TRUNCATED", "BLOCK_TYPE", "STORED_LEN", "OVERSUBSCRIBED", "INCOMPLETE", "REPEAT", "NO_END_OF_BLOCK", "BAD_SYMBOL", "FAR_DISTANCE",
                "TOO_MUCH", "TOO_LITTLE", "TRAILING", "ADLER", "FILTER", "UNUSED_CODE", "TOO_MANY_SYMBOLS"]
CL_ORDER = (16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15)
LENGTH_BASE = (3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 17, 19, 23, 27, 31, 35, 43, 51, 59, 67, 83, 99, 115, 131, 163, 195, 227, 258)
LENGTH_EXTRA = (0, 0, 0, 0, 0, 0, 0, 0, 1, 1, 1, 1, 2, 2, 2, 2, 3, 3, 3, 3, 4, 4, 4, 4, 5, 5, 5, 5, 0)
DIST_BASE = (1, 2, 3, 4, 5, 7, 9, 13, 17, 25, 33, 49, 65, 97, 129, 193, 257, 385, 513, 769, 1025, 1537, 2049, 3073, 4097, 6145, 8193, 12289, 16385, 24577)
DIST_EXTRA = (0, 0, 0, 0, 1, 1, 2, 2, 3, 3, 4, 4, 5, 5, 6, 6, 7, 7, 8, 8, 9, 9, 10, 10, 11, 11, 12, 12, 13, 13)
FIXED_LL = [8] * 144 + [9] * 112 + [7] * 24 + [8] * 8
FIXED_D = [5] * 32
BAND = 64               # rows the device's unfilter handles at once


class Damaged(Exception):
    def __init__(self, status):
        super().__init__(STATUS_NAMES[status])
        self.status = status


class Trace:
    def __init__(self):
        self.blocks = []            # BTYPE of every block
        self.tokens = []            # (byte,) for a literal, (length, distance) for a match
        self.length_symbols = set()
        self.dist_symbols = set()
        self.code_lengths = []      # per dynamic block (literal/length lengths, distance lengths)
        self.repeats = []           # per repeat code (symbol, lengths read before it, lengths it gives, HLIT)
        self.stored = []            # LEN of every stored block


class _Bits:
    def __init__(self, data, at):
        self.data = data
        self.pos = 8 * at
        self.end = 8 * len(data)

    def left(self):
        return self.end - self.pos

    def peek(self):
        """At least 32 bits from the position on, zeros behind the end."""
        at = self.pos >> 3
        return int.from_bytes(self.data[at:at + 5], "little") >> (self.pos & 7)

    def take(self, n):
        if self.left() < n:
            raise Damaged(TRUNCATED)
        v = self.peek() & ((1 << n) - 1)
        self.pos += n
        return v

    def align(self):
        self.pos = (self.pos + 7) & ~7


class _Huff:
    """Canonical code of the lengths; ``one_code_ok``: zlib's exception for a single code of one bit.  A set without codes is taken."""

    def __init__(self, lens, one_code_ok):
        count = [0] * 16
        for ln in lens:
            count[ln] += 1
        self.count = count
        self.symbol = [s for ln in range(1, 16) for s, k in enumerate(lens) if k == ln]
        if count[0] == len(lens):
            return
        left, longest = 1, 0
        for ln in range(1, 16):
            left = (left << 1) - count[ln]
            if left < 0:
                raise Damaged(OVERSUBSCRIBED)
            if count[ln]:
                longest = ln
        if left > 0 and not (one_code_ok and longest == 1):
            raise Damaged(INCOMPLETE)

    def decode(self, b):
        bits = b.peek()                                      # behind the end: zeros
        code = first = index = 0
        for ln in range(1, 16):
            code |= bits & 1
            bits >>= 1
            k = self.count[ln]
            if code - k < first:
                if ln > b.left():
                    raise Damaged(TRUNCATED)
                b.pos += ln
                return self.symbol[index + code - first], ln
            index += k
            first = (first + k) << 1
            code <<= 1
        raise Damaged(TRUNCATED if b.left() < 15 else UNUSED_CODE)


def _dynamic(b, trace):
    head = b.take(14)
    nlen, ndist, ncode = (head & 31) + 257, (head >> 5 & 31) + 1, (head >> 10 & 15) + 4
    if nlen > 286 or ndist > 30:
        raise Damaged(TOO_MANY_SYMBOLS)
    cl = [0] * 19
    for i in range(ncode):
        cl[CL_ORDER[i]] = b.take(3)
    code = _Huff(cl, False)
    lens = []
    while len(lens) < nlen + ndist:
        sym, _ = code.decode(b)
        if sym < 16:
            lens.append(sym)
            continue
        prev = 0
        if sym == 16:
            if not lens:
                raise Damaged(REPEAT)
            prev = lens[-1]
            copy = 3 + b.take(2)
        elif sym == 17:
            copy = 3 + b.take(3)
        else:
            copy = 11 + b.take(7)
        if len(lens) + copy > nlen + ndist:
            raise Damaged(REPEAT)
        trace.repeats.append((sym, len(lens), copy, nlen))
        lens += [prev] * copy
    if lens[256] == 0:
        raise Damaged(NO_END_OF_BLOCK)
    trace.code_lengths.append((lens[:nlen], lens[nlen:]))
    ll = _Huff(lens[:nlen], True)
    return ll, _Huff(lens[nlen:], True)


def inflate(stream, size):
    """The zlib stream of a file whose filtered stream has ``size`` bytes -> (bytes, status, Trace).  The two header bytes are the host
    parser's to check and are skipped.  With a non-zero status the bytes are what was written before it."""
    stream = bytes(stream)
    out = bytearray()
    trace = Trace()
    try:
        if len(stream) < 2:
            raise Damaged(TRUNCATED)
        b = _Bits(stream, 2)
        final = 0
        while not final:
            head = b.take(3)
            final, btype = head & 1, head >> 1
            trace.blocks.append(btype)
            if btype == 3:
                raise Damaged(BLOCK_TYPE)
            if btype == 0:
                b.align()
                v = b.take(32)
                ln, nln = v & 0xffff, v >> 16
                if ln != nln ^ 0xffff:
                    raise Damaged(STORED_LEN)
                src = b.pos // 8
                if ln > len(stream) - src:
                    raise Damaged(TRUNCATED)
                if ln > size - len(out):
                    raise Damaged(TOO_MUCH)
                out += stream[src:src + ln]
                b.pos += 8 * ln
                trace.stored.append(ln)
                continue
            ll, d = (_Huff(FIXED_LL, False), _Huff(FIXED_D, False)) if btype == 1 else _dynamic(b, trace)
            while True:
                sym, _ = ll.decode(b)
                if sym < 256:
                    if size - len(out) < 1:
                        raise Damaged(TOO_MUCH)
                    out.append(sym)
                    trace.tokens.append((sym,))
                    continue
                if sym == 256:
                    break
                sym -= 257
                if sym >= 29:
                    raise Damaged(BAD_SYMBOL)
                ln = LENGTH_BASE[sym] + b.take(LENGTH_EXTRA[sym])
                dsym, _ = d.decode(b)
                if dsym >= 30:
                    raise Damaged(BAD_SYMBOL)
                dist = DIST_BASE[dsym] + b.take(DIST_EXTRA[dsym])
                if dist > len(out):
                    raise Damaged(FAR_DISTANCE)
                if ln > size - len(out):
                    raise Damaged(TOO_MUCH)
                trace.length_symbols.add(257 + sym)
                trace.dist_symbols.add(dsym)
                trace.tokens.append((ln, dist))
                if dist >= ln:
                    out += out[len(out) - dist:len(out) - dist + ln]
                else:
                    for _ in range(ln):
                        out.append(out[-dist])
        b.align()
        left = len(stream) - b.pos // 8
        if left < 4:
            raise Damaged(TRUNCATED)
        if len(out) < size:
            raise Damaged(TOO_LITTLE)
        if left > 4:
            raise Damaged(TRAILING)
        if int.from_bytes(stream[-4:], "big") != adler32(out):
            raise Damaged(ADLER)
    except Damaged as e:
        return bytes(out), e.status, trace
    return bytes(out), OK, trace


def adler32(data):
    """RFC 1950's checksum, from its definition (NumPy: both sums over blocks that cannot overflow)."""
    a, b = 1, 0
    arr = np.frombuffer(bytes(data), np.uint8).astype(np.uint64)
    for i in range(0, len(arr), 4096):
        blk = arr[i:i + 4096]
        n = len(blk)
        b = (b + n * a + int((np.arange(n, 0, -1, dtype=np.uint64) * blk).sum())) % 65521
        a = (a + int(blk.sum())) % 65521
    return b << 16 | a


def _paeth(a, b, c):
    p = a + b - c
    pa, pb, pc = abs(p - a), abs(p - b), abs(p - c)
    return a if pa <= pb and pa <= pc else b if pb <= pc else c


def unfilter(filtered, h, w, c):
    """The filtered stream h x (w c + 1) -> (pixels uint8 [h,w,c], status): filters 0..4 of the PNG specification, 9.2."""
    rb = w * c
    rows = np.frombuffer(bytes(filtered), np.uint8).reshape(h, rb + 1)
    if (rows[:, 0] > 4).any():
        return None, FILTER
    out = np.zeros((h, rb), np.uint8)
    prev = [0] * rb
    for y in range(h):
        ft, raw = int(rows[y, 0]), rows[y, 1:].tolist()
        if ft == 0:
            cur = raw
        elif ft == 2:
            cur = [(x + b) & 255 for x, b in zip(raw, prev)]
        else:
            cur = [0] * rb
            for i in range(rb):
                a = cur[i - c] if i >= c else 0
                if ft == 1:
                    pred = a
                elif ft == 3:
                    pred = (a + prev[i]) >> 1
                else:
                    pred = _paeth(a, prev[i], prev[i - c] if i >= c else 0)
                cur[i] = (raw[i] + pred) & 255
        out[y] = cur
        prev = cur
    return out.reshape(h, w, c), OK


def decode(stream, h, w, c, c_out=None):
    """What adain_png_decode_u8 answers for one file: (pixels uint8 [h,w,c_out] or None, status, Trace)."""
    data, status, trace = inflate(stream, h * (w * c + 1))
    if status:
        return None, status, trace
    px, status = unfilter(data, h, w, c)
    if status:
        return None, status, trace
    if c_out is not None and c_out != c:
        px = np.repeat(px, 3, axis=2) if c == 1 else px[:, :, :3]
    return np.ascontiguousarray(px), OK, trace


# ---- writing streams and files by hand -----------------------------------------------------------------------------------------------------
class BitWriter:
    """LSB-first bits, as deflate packs them.  ``code`` puts a Huffman code, whose bits go most significant first."""

    def __init__(self):
        self.out = bytearray()
        self.v = 0              # the bits of the byte being filled, and those behind it
        self.n = 0              # all bits written

    def bits(self, value, count):
        assert 0 <= value < 1 << count
        self.v |= value << (self.n & 7)
        self.n += count
        while len(self.out) < self.n >> 3:
            self.out.append(self.v & 255)
            self.v >>= 8
        return self

    def code(self, code, length):
        for i in range(length - 1, -1, -1):
            self.bits(code >> i & 1, 1)
        return self

    def align(self):
        return self.bits(0, -self.n & 7)

    def raw(self, data):
        assert self.n % 8 == 0
        for byte in bytes(data):
            self.bits(byte, 8)
        return self

    def done(self):
        return bytes(self.out) + (bytes([self.v & 255]) if self.n & 7 else b"")


def canonical(lens):
    """lengths -> {symbol: (code, length)} by RFC 1951 3.2.2 (whatever the set: the caller may ask for a damaged one)."""
    count = [0] * 16
    for ln in lens:
        count[ln] += 1
    count[0] = 0
    nxt, code = [0] * 16, 0
    for ln in range(1, 16):
        code = (code + count[ln - 1]) << 1
        nxt[ln] = code
    out = {}
    for s, ln in enumerate(lens):
        if ln:
            out[s] = (nxt[ln], ln)
            nxt[ln] += 1
    return out


def length_symbol(length):
    s = max(i for i in range(29) if LENGTH_BASE[i] <= length) if length < 258 else 28
    return 257 + s, length - LENGTH_BASE[s], LENGTH_EXTRA[s]


def dist_symbol(dist):
    s = max(i for i in range(30) if DIST_BASE[i] <= dist)
    return s, dist - DIST_BASE[s], DIST_EXTRA[s]


def put_tokens(bw, tokens, ll, d):
    """tokens: ints (literals) and (length, distance) pairs, then the end-of-block code; ll, d: ``canonical`` codes."""
    for t in tokens:
        if isinstance(t, int):
            bw.code(*ll[t])
            continue
        s, ev, eb = length_symbol(t[0])
        bw.code(*ll[s]).bits(ev, eb)
        s, ev, eb = dist_symbol(t[1])
        bw.code(*d[s]).bits(ev, eb)
    bw.code(*ll[256])


def put_dynamic_header(bw, final, ll_lens, d_lens, cl_lens, items):
    """BFINAL, BTYPE 2, HLIT, HDIST, HCLEN (all 19), the code-length code ``cl_lens`` and the ``items`` that spell the lengths: a length
    0..15, or (16, extra), (17, extra), (18, extra)."""
    bw.bits(final, 1).bits(2, 2).bits(len(ll_lens) - 257, 5).bits(len(d_lens) - 1, 5).bits(15, 4)
    for s in CL_ORDER:
        bw.bits(cl_lens[s], 3)
    cl = canonical(cl_lens)
    for it in items:
        if isinstance(it, int):
            bw.code(*cl[it])
        else:
            bw.code(*cl[it[0]]).bits(it[1], {16: 2, 17: 3, 18: 7}[it[0]])


def zlib_wrap(deflate, filtered, header=b"\x78\x01"):
    return header + deflate + struct.pack(">I", zlib.adler32(bytes(filtered)))


def chunk(kind, body):
    return struct.pack(">I", len(body)) + kind + body + struct.pack(">I", zlib.crc32(kind + body))


def png_file(h, w, colour_type, pieces, before=(), after=(), depth=8, interlace=0):
    """A PNG file around the IDAT payloads ``pieces`` (a list of bytes; one bytes is one IDAT); before / after: (kind, body) chunks in
    front of and behind the IDATs."""
    pieces = [pieces] if isinstance(pieces, (bytes, bytearray)) else pieces
    out = b"\x89PNG\r\n\x1a\n" + chunk(b"IHDR", struct.pack(">IIBBBBB", w, h, depth, colour_type, 0, 0, interlace))
    out += b"".join(chunk(k, v) for k, v in before)
    out += b"".join(chunk(b"IDAT", bytes(p)) for p in pieces)
    out += b"".join(chunk(k, v) for k, v in after)
    return out + chunk(b"IEND", b"")


def filter_rows(px, filters):
    """pixels uint8 [h,w,c] and a filter 0..4 per row -> the filtered stream (the inverse of ``unfilter``)."""
    h, w, c = px.shape
    rb = w * c
    rows = px.reshape(h, rb).astype(np.int64)
    out = bytearray()
    prev = np.zeros(rb, np.int64)
    for y in range(h):
        cur = rows[y]
        a = np.concatenate([np.zeros(c, np.int64), cur[:-c]]) if rb > c else np.zeros(rb, np.int64)
        cc = np.concatenate([np.zeros(c, np.int64), prev[:-c]]) if rb > c else np.zeros(rb, np.int64)
        ft = filters[y]
        if ft == 0:
            pred = np.zeros(rb, np.int64)
        elif ft == 1:
            pred = a
        elif ft == 2:
            pred = prev
        elif ft == 3:
            pred = (a + prev) >> 1
        else:
            pred = np.array([_paeth(int(x), int(y_), int(z)) for x, y_, z in zip(a, prev, cc)], np.int64)
        out.append(ft)
        out += ((cur - pred) & 255).astype(np.uint8).tobytes()
        prev = cur
    return bytes(out)
