"""The device PNG writer's rules (csrc/png.hip) in NumPy / Python, byte for byte the device's file.  Host only.

The file: signature, IHDR, one IDAT, IEND; 8-bit, colour type 2 (c = 3) or 0 (c = 1), non-interlaced.
  * rows    : filter -1 tries all five filters on the raw previous row and keeps the one whose filtered bytes have the smallest sum of
              magnitudes (b < 128 ? b : 256 - b), ties to the lowest number; filter 0..4 forces one.  The filtered stream is, per row,
              the filter's number and the w * c filtered bytes: stride = w * c + 1.
  * blocks  : BLOCK filtered bytes each (the last one shorter).  A block is a dynamic-Huffman block or a fixed-Huffman one, whichever
              has fewer bits, ties to fixed.  BFINAL on the last, which is zero-padded to a byte.
  * matches : at every position the longest match among the distances {1, 2, 3, 4, 6, stride - c, stride, stride + c} (those in
              1..32768, and never a source before the stream's start), ties to the smallest distance, at most 258 bytes and never past the
              block's end; then a greedy parse from the block's start that takes matches of MIN_MATCH bytes or more.
  * lengths : Huffman by the two-queue merge over the symbols sorted by (count, symbol), a leaf before an internal node of the same
              weight; a tree deeper than the limit (15; 7 for the code-length alphabet) is rebuilt with every count halved, rounding up.
              One used symbol gets one bit; a block without matches sends distance symbol 0 with one bit.
  * header  : the code lengths of both alphabets as one sequence, run-length coded greedily: zeros by 18 (11..138) while 11 or more remain,
              then 17 (3..10), then singly; another length once, then 16 (3..6) while 3 or more remain, then singly.
  * wrapper : zlib header 78 01, Adler-32 of the filtered stream, CRC-32 on every chunk.
FAULTS names single deliberate mistakes, for the tests that show the host checks would catch them."""
import struct
import zlib

import numpy as np

BLOCK = 32768
MIN_MATCH = 4
MAX_MATCH = 258
MAX_DIST = 32768
SIGNATURE = b"\x89PNG\r\n\x1a\n"
FAULTS = set()          # of: "paeth_tie", "cross_block", "msb_first", "hlit", "adler"
STATS = {"halved": {15: 0, 7: 0}}          # how often a tree had to be rebuilt for its limit: the tests' proof that a case reaches the rule

LEN_BASE = [3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 17, 19, 23, 27, 31, 35, 43, 51, 59, 67, 83, 99, 115, 131, 163, 195, 227, 258]
LEN_EXTRA = [0, 0, 0, 0, 0, 0, 0, 0, 1, 1, 1, 1, 2, 2, 2, 2, 3, 3, 3, 3, 4, 4, 4, 4, 5, 5, 5, 5, 0]
DIST_BASE = [1, 2, 3, 4, 5, 7, 9, 13, 17, 25, 33, 49, 65, 97, 129, 193, 257, 385, 513, 769, 1025, 1537, 2049, 3073, 4097, 6145, 8193, 12289,
             16385, 24577]
DIST_EXTRA = [0, 0, 0, 0, 1, 1, 2, 2, 3, 3, 4, 4, 5, 5, 6, 6, 7, 7, 8, 8, 9, 9, 10, 10, 11, 11, 12, 12, 13, 13]
CL_ORDER = [16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15]
FIXED_LL = [8] * 144 + [9] * 112 + [7] * 24 + [8] * 8          # 288 lengths; symbols 286, 287 never occur
FIXED_D = [5] * 30


def length_symbol(length):
    """(symbol - 257, extra bits' value) of a match length 3..258."""
    k = max(i for i in range(29) if LEN_BASE[i] <= length) if length < 258 else 28
    return k, length - LEN_BASE[k]


def dist_symbol(dist):
    k = max(i for i in range(30) if DIST_BASE[i] <= dist)
    return k, dist - DIST_BASE[k]


def stride_of(w, c):
    return w * c + 1


def distances(w, c):
    """The candidate distances of a frame, ascending, without repeats."""
    s = stride_of(w, c)
    return sorted({d for d in (1, 2, 3, 4, 6, s - c, s, s + c) if 1 <= d <= MAX_DIST})


def out_stride(h, w, c):
    """The derived bound of include/adain_hip.h: a literal costs at most 9 bits, a match no more than its literals, a block 10 more."""
    n = h * stride_of(w, c)
    blocks = (n + BLOCK - 1) // BLOCK
    return 57 + 6 + (9 * n + 10 * blocks + 7) // 8


# ---- rows ---------------------------------------------------------------------------------------------------------------------------------
def filter_rows(frame, filt=None):
    """frame uint8 [h, w, c] -> (the filtered stream uint8 [h * (w * c + 1)], the filter of every row)."""
    h, w, c = frame.shape
    raw = frame.reshape(h, w * c).astype(np.int32)
    up = np.vstack([np.zeros((1, w * c), np.int32), raw[:-1]])
    left = np.hstack([np.zeros((h, c), np.int32), raw[:, :-c]]) if w * c > c else np.zeros_like(raw)
    ul = np.hstack([np.zeros((h, c), np.int32), up[:, :-c]]) if w * c > c else np.zeros_like(raw)
    p = left + up - ul
    pa, pb, pc = np.abs(p - left), np.abs(p - up), np.abs(p - ul)
    if "paeth_tie" in FAULTS:
        paeth = np.where((pa <= pb) & (pa <= pc), left, np.where(pb < pc, up, ul))          # (pa == pb happens only where left == up)
    else:
        paeth = np.where((pa <= pb) & (pa <= pc), left, np.where(pb <= pc, up, ul))
    cand = np.stack([raw, raw - left, raw - up, raw - ((left + up) >> 1), raw - paeth]) & 255        # [5, h, w * c]
    cost = np.where(cand < 128, cand, 256 - cand).sum(axis=2)                                           # [5, h]
    which = np.argmin(cost, axis=0) if filt is None or filt < 0 else np.full(h, filt)
    rows = cand[which, np.arange(h)]
    return np.hstack([which[:, None], rows]).astype(np.uint8).reshape(-1), which


# ---- matches ------------------------------------------------------------------------------------------------------------------------------
def best_matches(f, dists):
    """(length, distance index) of the best candidate at every position of the filtered stream f; length 0: none."""
    n = len(f)
    pos = np.arange(n)
    cap = np.minimum(MAX_MATCH, (pos // BLOCK + 1) * BLOCK - pos)
    cap = np.minimum(cap, n - pos)
    if "cross_block" in FAULTS:
        cap = np.minimum(MAX_MATCH, n - pos)
    best = np.zeros(n, np.int64)
    which = np.zeros(n, np.int64)
    for k, d in enumerate(dists):
        if d >= n:
            continue
        differs = np.ones(n + 1, bool)
        differs[d:n] = f[d:] != f[:-d]
        nxt = np.where(differs, np.arange(n + 1), n)
        nxt = np.minimum.accumulate(nxt[::-1])[::-1]          # the first differing position at or after each one
        run = np.minimum(nxt[:n] - pos, cap)
        better = run > best
        best[better], which[better] = run[better], k
    return best, which


def parse(best):
    """The greedy parse: the token starts (positions) of every block."""
    n = len(best)
    starts = []
    lens = best.tolist()
    for b0 in range(0, n, BLOCK):
        p, end = b0, min(b0 + BLOCK, n)
        while p < end:
            starts.append(p)
            p += lens[p] if lens[p] >= MIN_MATCH else 1
    return np.array(starts, np.int64)


# ---- code lengths -------------------------------------------------------------------------------------------------------------------------
def code_lengths(freq, limit):
    n = len(freq)
    f = list(freq)
    used = [i for i in range(n) if f[i] > 0]
    lens = [0] * n
    if len(used) == 1:
        lens[used[0]] = 1
    if len(used) < 2:
        return lens
    m = len(used)
    while True:
        leaves = sorted(used, key=lambda i: (f[i], i))
        wt = [f[i] for i in leaves]
        iw, pl, pi = [0] * (m - 1), [0] * m, [0] * (m - 1)
        li = ii = 0
        for k in range(m - 1):
            total = 0
            for _ in range(2):
                if li < m and (ii >= k or wt[li] <= iw[ii]):
                    total += wt[li]
                    pl[li] = k
                    li += 1
                else:
                    total += iw[ii]
                    pi[ii] = k
                    ii += 1
            iw[k] = total
        depth = [0] * (m - 1)
        for k in range(m - 3, -1, -1):
            depth[k] = depth[pi[k]] + 1
        for j, i in enumerate(leaves):
            lens[i] = depth[pl[j]] + 1
        if max(lens) <= limit:
            return lens
        STATS["halved"][limit] += 1
        for i in used:
            f[i] = (f[i] + 1) >> 1


def canonical_codes(lens):
    """RFC 1951 3.2.2: the codes of the lengths, MSB first as integers."""
    count = [0] * 17
    for v in lens:
        count[v] += 1
    count[0] = 0
    nxt, code = [0] * 17, 0
    for bits in range(1, 16):
        code = (code + count[bits - 1]) << 1
        nxt[bits] = code
    codes = [0] * len(lens)
    for i, v in enumerate(lens):
        if v:
            codes[i] = nxt[v]
            nxt[v] += 1
    return codes


def reverse_bits(code, nbits):
    r = 0
    for _ in range(nbits):
        r = r << 1 | (code & 1)
        code >>= 1
    return r


def run_length(seq):
    """The code-length sequence as (symbol, extra value) pairs."""
    out, i, n = [], 0, len(seq)
    while i < n:
        v, r = seq[i], 1
        while i + r < n and seq[i + r] == v:
            r += 1
        i += r
        if v == 0:
            while r >= 11:
                k = min(r, 138)
                out.append((18, k - 11))
                r -= k
            if r >= 3:
                out.append((17, r - 3))
                r = 0
        else:
            out.append((v, 0))
            r -= 1
            while r >= 3:
                k = min(r, 6)
                out.append((16, k - 3))
                r -= k
        out += [(v, 0)] * r
    return out


CL_EXTRA = {16: 2, 17: 3, 18: 7}


class Bits:
    """(value, bit count) pairs, packed LSB first at the end."""

    def __init__(self):
        self.values, self.counts = [], []

    def put(self, value, count):
        self.values.append(np.atleast_1d(np.asarray(value, np.int64)))
        self.counts.append(np.atleast_1d(np.asarray(count, np.int64)))

    def pack(self):
        v, c = np.concatenate(self.values), np.concatenate(self.counts)
        v, c = v[c > 0], c[c > 0]
        total = int(c.sum())
        start = np.cumsum(c) - c
        item = np.repeat(np.arange(len(c)), c)
        j = np.arange(total) - start[item]
        bits = ((v[item] >> j) & 1).astype(np.uint8)
        if "msb_first" in FAULTS:
            return np.packbits(bits, bitorder="big").tobytes()
        return np.packbits(bits, bitorder="little").tobytes()


def block_plan(ll_freq, d_freq, extra_bits):
    """The choice of one block: (dynamic?, ll lengths, d lengths, header as (value, count) pairs behind BFINAL, bits without BFINAL's,
    (dynamic bits, fixed bits))."""
    ll_len = code_lengths(ll_freq, 15)
    d_len = code_lengths(d_freq, 15)
    if not any(d_len):
        d_len[0] = 1
    hlit = max(i for i in range(286) if ll_len[i]) + 1
    hdist = max(i for i in range(30) if d_len[i]) + 1
    rle = run_length(ll_len[:hlit] + d_len[:hdist])
    cl_freq = [0] * 19
    for s, _ in rle:
        cl_freq[s] += 1
    cl_len = code_lengths(cl_freq, 7)
    hclen = max(i for i in range(19) if cl_len[CL_ORDER[i]]) + 1
    hclen = max(hclen, 4)
    body = lambda ll, d: sum(a * b for a, b in zip(ll_freq, ll)) + sum(a * b for a, b in zip(d_freq, d)) + extra_bits
    dyn = 2 + 14 + 3 * hclen + sum(cl_len[s] + CL_EXTRA.get(s, 0) for s, _ in rle) + body(ll_len, d_len)
    fixed = 2 + body(FIXED_LL, FIXED_D)
    if dyn >= fixed:
        return False, FIXED_LL, FIXED_D, [(1, 2)], fixed, (dyn, fixed)
    cl_code = canonical_codes(cl_len)
    header = [(2, 2), (hlit - 257 + ("hlit" in FAULTS), 5), (hdist - 1, 5), (hclen - 4, 4)] + [(cl_len[CL_ORDER[i]], 3) for i in range(hclen)]
    for s, e in rle:
        header.append((reverse_bits(cl_code[s], cl_len[s]), cl_len[s]))
        if s >= 16:
            header.append((e, CL_EXTRA[s]))
    return True, ll_len, d_len, header, dyn, (dyn, fixed)


LEN_SYM = np.array([0, 0, 0] + [length_symbol(v)[0] for v in range(3, 259)])
DIST_SYM = np.array([0] + [dist_symbol(v)[0] for v in range(1, MAX_DIST + 1)])


def deflate(f, dists, report=None):
    """The deflate stream (bytes) of the filtered stream f.  report: a list that receives one dict per block."""
    n = len(f)
    best, which = best_matches(f, dists)
    starts = parse(best)
    length = best[starts]
    is_match = length >= MIN_MATCH
    dist = np.array(dists, np.int64)[which[starts]]
    lsym = np.where(is_match, LEN_SYM[np.where(is_match, length, 3)], 0)
    dsym = np.where(is_match, DIST_SYM[np.where(is_match, dist, 1)], 0)
    lextra_n = np.where(is_match, np.array(LEN_EXTRA)[lsym], 0)
    dextra_n = np.where(is_match, np.array(DIST_EXTRA)[dsym], 0)
    lextra = np.where(is_match, length - np.array(LEN_BASE)[lsym], 0)
    dextra = np.where(is_match, dist - np.array(DIST_BASE)[dsym], 0)
    symbol = np.where(is_match, 257 + lsym, f[starts].astype(np.int64))
    block_of = starts // BLOCK
    nblocks = (n + BLOCK - 1) // BLOCK
    out = Bits()
    for b in range(nblocks):
        sel = block_of == b
        ll_freq = np.bincount(symbol[sel], minlength=286).tolist()
        ll_freq[256] = 1
        d_freq = np.bincount(dsym[sel][is_match[sel]], minlength=30).tolist()
        dynamic, ll_len, d_len, header, bits, both = block_plan(ll_freq, d_freq, int(lextra_n[sel].sum() + dextra_n[sel].sum()))
        if report is not None:
            report.append({"dynamic": dynamic, "ll_len": list(ll_len), "d_len": list(d_len), "bits": bits + 1, "ll_freq": ll_freq, "d_freq": d_freq,
                           "header": header, "dynamic_bits": both[0], "fixed_bits": both[1]})
        out.put(int(b == nblocks - 1), 1)
        for value, count in header:
            out.put(value, count)
        ll_code = np.array([reverse_bits(v, k) for v, k in zip(canonical_codes(list(ll_len)), ll_len)], np.int64)
        d_code = np.array([reverse_bits(v, k) for v, k in zip(canonical_codes(list(d_len)), d_len)], np.int64)
        ll_len, d_len = np.array(ll_len, np.int64), np.array(d_len, np.int64)
        m = is_match[sel]
        fields = np.stack([ll_code[symbol[sel]], lextra[sel], d_code[dsym[sel]], dextra[sel]], axis=1)
        counts = np.stack([ll_len[symbol[sel]], lextra_n[sel], np.where(m, d_len[dsym[sel]], 0), dextra_n[sel]], axis=1)
        out.put(fields.reshape(-1), counts.reshape(-1))
        out.put(int(ll_code[256]), int(ll_len[256]))
    return out.pack()


def adler32(f):
    """Adler-32 by the device's sums: a = 1 + sum of the bytes, b = N + sum of (N - j) * byte j."""
    n = len(f)
    v = f.astype(object)
    a = (1 + int(v.sum())) % 65521
    b = (n + int((v * np.arange(n, 0, -1).astype(object)).sum())) % 65521
    if "adler" in FAULTS:
        b = (b + n) % 65521
    return b << 16 | a


def chunk(kind, data):
    return struct.pack(">I", len(data)) + kind + data + struct.pack(">I", zlib.crc32(kind + data))


def zlib_stream(f, dists, report=None):
    return b"\x78\x01" + deflate(f, dists, report) + struct.pack(">I", adler32(f))


def encode(frame, filt=None, report=None):
    """frame uint8 [h, w, c] (c 1 or 3) or [h, w] -> the PNG file (bytes)."""
    frame = np.asarray(frame)
    if frame.ndim == 2:
        frame = frame[:, :, None]
    h, w, c = frame.shape
    assert frame.dtype == np.uint8 and c in (1, 3)
    f, _ = filter_rows(frame, filt)
    ihdr = struct.pack(">IIBBBBB", w, h, 8, 2 if c == 3 else 0, 0, 0, 0)
    return SIGNATURE + chunk(b"IHDR", ihdr) + chunk(b"IDAT", zlib_stream(f, distances(w, c), report)) + chunk(b"IEND", b"")
