"""JPEG files built from chosen coefficients, for the three device decoders (csrc/jpeg_decode.hip: adain_jpeg_decode_u8, adain_jpeg_decode_restart_u8,
adain_jpeg_decode_progressive_u8).  Files an encoder derives from pixels reach only part of what a decoder must take; here the
coefficients, the Huffman tables, the header fields and the scan script are chosen, and ``coverage`` counts from the restatements' own
walk (tests/jpeg_file_ref.py, jpeg_restart_ref.py, jpeg_progressive_ref.py) what a file makes a decoder do.  NumPy only, deterministic,
nothing is read from a file.  tests/test_jpeg_designed_host.py holds every file to Pillow on the host, tests/test_gpu_jpeg_designed.py
decodes them on the device.

Coefficients are int64 [blocks, 64]: the blocks in MCU order (per MCU the H x V luma blocks row-major, then Cb, Cr), each in zigzag
order with the DC VALUE at 0; the writers make the differences.  ``geometry`` is (h, w, c, sampling) as jpeg_file.parse gives it.

The range condition.  "Pixel for pixel Pillow's" holds while the IDCT's centred sample (before the + 128) lies in -512..511: libjpeg's C
range-limit table, which the device follows, is a clamp only there and wraps beyond, and the SIMD build inside Pillow saturates instead.
Every good file here keeps ``centred_range`` inside that interval, and the host test asserts it per file: the quantisation tables are
all ones where sizes 8..10 are aimed at, steps of 2 and 3 stand only at zigzag indices 58..63, where the content keeps |value| <= 127,
and a block's sum of |coefficient| x step stays under ``BUDGET`` (a sample is at most sum |AC| step / 4 + |DC| step / 8).

Every-length tables.  A prefix code with a code of EVERY length 1..16 is a chain: the lengths 1..15 leave room for two codes of 16 bits,
so such a table has at most 17 symbols.  No table can carry the 162 AC symbols and every length at once, and a DC table reaches 16
lengths only with symbols a good file never uses.  ``chain_table`` is that chain over 16 symbols (the all-ones code left out, as
libjpeg's encoder leaves it out); the B-lengths set runs it forwards and backwards over 16 chosen symbols per slot, so that every symbol
of them meets a short and a long code, and adds ``tail_table`` (every size-10 and size-11 symbol on a 16-bit code, everything else on 8
bits) and ``spread_table`` (libjpeg's optimal table of geometric counts, lengths limited to 16 by Annex K.3) over all symbols.
"""
import collections
import functools
import itertools

import numpy as np

import jpeg_decode_ref as D
import jpeg_file_ref as R
import jpeg_options_ref as O
import jpeg_progressive_ref as P
import jpeg_ref as J
import jpeg_restart_ref as RR

EOI = b"\xff\xd9"
BUDGET = 1900
DC_SYMBOLS = list(range(12))
AC_SYMBOLS = [0x00, 0xF0] + [r << 4 | s for r in range(16) for s in range(1, 11)]
# the 14 run/size symbols of the chain tables (with EOB and ZRL: 16): every size 1..10, runs 0, 1, 2, 3, 5, 7, 9, 14, 15
CHAIN_AC = [0x00, 0xF0, 0x01, 0x02, 0x11, 0x0A, 0xFA, 0x23, 0x05, 0x37, 0x79, 0xF1, 0xEA, 0x54, 0x08, 0x96]
PATTERNS = ("100..0", "111..1", "000..0", "011..1")          # the value bits of the four extreme values of a size


def extremes(s):
    """The values of size s whose bits are 100..0, 111..1, 000..0 and 011..1 (size 1: two values)."""
    return list(dict.fromkeys([1 << (s - 1), (1 << s) - 1, -((1 << s) - 1), -(1 << (s - 1))])) if s else [0]


# ---- geometry ------------------------------------------------------------------------------------------------------------------------------
def layout(geometry):
    """-> (H, V, MCU rows, MCU columns, the component of each block of an MCU)."""
    h, w, c, sampling = geometry
    H, V = R.LUMA_HV[sampling] if c == 3 else (1, 1)
    return H, V, -(-h // (8 * V)), -(-w // (8 * H)), ([0] * (H * V) + [1, 2] if c == 3 else [0])


def scan_order(geometry, comps):
    """The blocks a scan of the components ``comps`` codes, in its order: indices into the MCU-ordered array, and each one's component.
    An interleaved scan walks the MCU grid; a one-component scan walks the component's own raster, which leaves the dummy luma blocks
    of partial MCUs out."""
    h, w, c, _ = geometry
    H, V, mh, mw, comp_of = layout(geometry)
    bpm = len(comp_of)
    if len(comps) == c:
        return list(range(mh * mw * bpm)), comp_of * (mh * mw)
    k = comps[0]
    if k > 0:
        return [m * bpm + H * V + k - 1 for m in range(mh * mw)], [k] * (mh * mw)
    bh, bw = -(-h // 8), -(-w // 8)
    return [((by // V) * mw + bx // H) * bpm + (by % V) * H + bx % H for by in range(bh) for bx in range(bw)], [0] * (bh * bw)


def real_blocks(geometry):
    """bool [blocks]: False for the dummy luma blocks of partial MCUs, which only interleaved scans code."""
    H, V, mh, mw, comp_of = layout(geometry)
    real = np.zeros(mh * mw * len(comp_of), bool)
    for k in range(geometry[2]):
        real[scan_order(geometry, (k,) if geometry[2] == 3 else (0,))[0]] = True
    return real


def assemble(geometry, per_comp):
    """Per component its blocks in scan order -> the MCU-ordered array."""
    H, V, mh, mw, comp_of = layout(geometry)
    n = mh * mw
    parts = [per_comp[0][:n * H * V].reshape(n, H * V, 64)] + [p[:n].reshape(n, 1, 64) for p in per_comp[1:]]
    return np.concatenate(parts, axis=1).reshape(-1, 64)


# ---- quantisation tables and the range condition ------------------------------------------------------------------------------------------
def qtable(step):
    """Natural order: ones, and ``step`` at the zigzag indices 58..63."""
    z = np.ones(64, np.int64)
    z[58:] = step
    t = np.zeros(64, np.int64)
    t[J.ZIGZAG] = z
    return t


Q1, Q2, Q3 = qtable(1), qtable(2), qtable(3)


def centred_range(coef, geometry, q):
    """(min, max) of the unclamped, centred IDCT samples of the coefficients under the per-component tables q [c, 64] natural: libjpeg's
    two islow passes (tests/jpeg_decode_ref.py) without the range limit."""
    comp = np.tile(layout(geometry)[4], len(coef) // len(layout(geometry)[4]))
    nat = np.zeros_like(coef)
    nat[:, J.ZIGZAG] = coef
    x = (nat * np.asarray(q)[comp]).reshape(-1, 8, 8)
    x = np.swapaxes(D._idct_pass(np.swapaxes(x, -1, -2), 11), -1, -2)
    s = D._idct_pass(x, 18)
    return int(s.min()), int(s.max())


def intended_pixels(coef, geometry, q):
    """tests/jpeg_decode_ref.py's IDCT and upsampling (through jpeg_file_ref.pixels, which adds the 4:2:2 upsampler and the colour map)
    of the coefficients as intended: no entropy decoder has touched them."""
    h, w, c, sampling = geometry
    comp = np.tile(layout(geometry)[4], len(coef) // len(layout(geometry)[4]))
    sink = R.Sink(len(coef))
    sink.coef = coef.astype(np.int64).copy()
    for k in range(c):
        sink.coef[comp == k, 0] = np.diff(coef[comp == k, 0], prepend=0)
    px, damage = R.pixels(dict(h=h, w=w, c=c, sampling=sampling, q=np.asarray(q)), sink)
    assert not damage
    return px


# ---- Huffman tables ----------------------------------------------------------------------------------------------------------------------------
def chain_table(symbols):
    """(bits, vals): the i-th symbol on the one code of length i + 1 - 0, 10, 110, ... - for up to 16 symbols; the all-ones code stays free."""
    assert len(symbols) <= 16 and len(set(symbols)) == len(symbols)
    return [1] * len(symbols) + [0] * (16 - len(symbols)), list(symbols)


def tail_table(symbols, long):
    """(bits, vals): the symbols of ``long`` on 16-bit codes, every other one of ``symbols`` on an 8-bit code."""
    short = [s for s in symbols if s not in long]
    assert len(short) <= 255
    bits = [0] * 16
    bits[7], bits[15] = len(short), len(long)
    return bits, short + list(long)


def spread_table(symbols, seed):
    """(bits, vals): libjpeg's optimal table of geometric counts over a seeded order of the symbols - an unrestricted tree deeper than
    16, limited as in Annex K.3 (jpeg_options_ref.optimal_table, as its FIXTURE_A_COUNTS does)."""
    order = np.random.default_rng(seed).permutation(len(symbols))
    freq = np.zeros(256, np.int64)
    for i, j in enumerate(order):
        freq[symbols[j]] = 1 << max(0, 24 - i)
    return O.optimal_table(freq)


def code_lengths(spec):
    return {ln + 1 for ln, n in enumerate(spec[0]) if n}


# ---- bits ------------------------------------------------------------------------------------------------------------------------------------
def pack(tokens, specs):
    """tokens (table index or -1, symbol, extra bits, their number) -> the entropy-coded segment: each symbol's code under
    ``specs[table]`` followed by its extra bits, index -1: the extra bits alone; padded with ones and stuffed (jpeg_ref.pack_bits)."""
    codes = [J.huff_codes(s) if s is not None else None for s in specs]
    pat, ln = [], []
    for t, sym, extra, n in tokens:
        assert 0 <= extra < 1 << n
        if t >= 0:
            code, length = int(codes[t][0][sym]), int(codes[t][1][sym])
            assert length > 0, f"symbol {sym:#04x} has no code"
            pat.append(code << n | extra)
            ln.append(length + n)
        elif n:
            pat.append(extra)
            ln.append(n)
    return J.pack_bits(np.array(pat, np.uint64), np.array(ln, np.int64))


# ---- the baseline writer -----------------------------------------------------------------------------------------------------------------------
DHT_IDS = (0x00, 0x10, 0x01, 0x11)
SEL = (0x00, 0x11, 0x11)


def coding_tables(c, dht, dht_ids=DHT_IDS, sel=SEL):
    """Per component its (DC, AC) tables as the header says: of an id defined twice the LATER definition holds."""
    def table(cls, ident):
        at = [i for i, x in enumerate(dht_ids[:len(dht)]) if x == cls << 4 | ident]
        assert at, f"table {cls}/{ident} is not defined"
        return dht[at[-1]]

    return [t for k in range(c) for t in (table(0, sel[k] >> 4), table(1, sel[k] & 15))]


def baseline(coef, geometry, dht, q=None, ri=0, code_with=None, **hdr):
    """A sequential file of the coefficients: jpeg_options_ref.header (``hdr``: its keywords - qsel, dht_ids, one_dht, sel, sof, fill)
    and jpeg_options_ref.entropy_data per restart interval of ``ri`` MCUs (0: one), the DC differences restarting with each, every
    interval padded with ones to a byte, RSTn markers numbered in turn.  ``q``: [(id, natural table)], default table 0 all ones for
    luma, table 1 with steps of 2 at 58..63 for chroma.  ``code_with``: the tables to code with where they are NOT the header's (a
    file whose header declares another symbol for a code: the status files)."""
    h, w, c, sampling = geometry
    H, V, mh, mw, comp_of = layout(geometry)
    bpm = len(comp_of)
    assert coef.shape == (mh * mw * bpm, 64)
    q = q or [(0, Q1), (1, Q2)][:2 if c == 3 else 1]
    pairs = code_with or coding_tables(c, dht, hdr.get("dht_ids", DHT_IDS), hdr.get("sel", SEL))
    comp = np.tile(comp_of, mh * mw)
    step = (ri or mh * mw) * bpm
    parts = []
    for a in range(0, len(coef), step):
        z, cm = coef[a:a + step].astype(np.int64).copy(), comp[a:a + step]
        for k in range(c):
            z[cm == k, 0] = np.diff(z[cm == k, 0], prepend=0)
        parts.append(O.entropy_data(z, cm, pairs))
    body = b"".join(p + (bytes([0xFF, 0xD0 + i % 8]) if i + 1 < len(parts) else b"") for i, p in enumerate(parts))
    return O.header(h, w, c, 100, sampling if c == 3 else 0, dht, qtables=q, ri=ri, **hdr) + body + EOI


# ---- the progressive writer --------------------------------------------------------------------------------------------------------------------
def _dc_first(vals, comps, al):
    pred, tokens = {}, []
    for v, k in zip(vals, comps):
        v >>= al
        d = v - pred.get(k, 0)
        pred[k] = v
        s = abs(d).bit_length()
        tokens.append((min(k, 1), s, (d if d >= 0 else d - 1) & ((1 << s) - 1), s))
    return tokens


class _Runs:
    """libjpeg's EOBRUN and its buffered correction bits (jcphuff.c): blocks that end in zeros are counted, and the count goes out as one
    EOBn symbol with its extra bits, followed by the correction bits those blocks left, before the next symbol of another kind - or
    when the count reaches the caller's limit (``limits``, taken in turn, each at most 32 767) or the bit buffer runs full."""

    def __init__(self, tokens, t, limits):
        self.tokens, self.t, self.limits = tokens, t, limits
        self.run, self.bits, self.limit = 0, [], next(limits)

    def flush(self):
        if self.run:
            n = self.run.bit_length() - 1
            self.tokens.append((self.t, n << 4, self.run & ((1 << n) - 1), n))
            self.run, self.limit = 0, next(self.limits)
        self.tokens.extend((-1, 0, b, 1) for b in self.bits)
        self.bits = []

    def block_ends(self, bits=()):
        self.run += 1
        self.bits += bits
        if self.run >= min(self.limit, 0x7FFF) or len(self.bits) > 1000 - 64 + 1:
            self.flush()


def _ac_first(rows, t, ss, se, al, limits):
    tokens = []
    runs = _Runs(tokens, t, limits)
    for row in rows:
        r = 0
        for k in range(ss, se + 1):
            v = row[k]
            a = abs(v) >> al
            if a == 0:
                r += 1
                continue
            runs.flush()
            while r > 15:
                tokens.append((t, 0xF0, 0, 0))
                r -= 16
            s = a.bit_length()
            tokens.append((t, r << 4 | s, (a if v > 0 else ~a) & ((1 << s) - 1), s))
            r = 0
        if r > 0:
            runs.block_ends()
    runs.flush()
    return tokens


def _ac_refine(rows, t, ss, se, al, limits):
    """libjpeg's encode_mcu_AC_refine: a coefficient that is 1 after the shift is new and goes out as run/1 and a sign bit, one that
    is larger leaves a correction bit; the correction bits passed on the way to a new coefficient or over a ZRL follow that symbol,
    those behind a block's last new coefficient wait with the end-of-band run."""
    tokens = []
    runs = _Runs(tokens, t, limits)
    for row in rows:
        a = [abs(v) >> al for v in row]
        eob = max([k for k in range(ss, se + 1) if a[k] == 1], default=-1)
        r, br = 0, []
        for k in range(ss, se + 1):
            if a[k] == 0:
                r += 1
                continue
            while r > 15 and k <= eob:
                runs.flush()
                tokens.append((t, 0xF0, 0, 0))
                r -= 16
                tokens.extend((-1, 0, b, 1) for b in br)
                br = []
            if a[k] > 1:
                br.append(a[k] & 1)
                continue
            runs.flush()
            tokens.append((t, r << 4 | 1, 0 if row[k] < 0 else 1, 1))
            tokens.extend((-1, 0, b, 1) for b in br)
            r, br = 0, []
        if r > 0 or br:
            runs.block_ends(br)
    runs.flush()
    return tokens


def scan_tokens(coef, geometry, scan, limits):
    """The tokens (``pack``) of one scan (components, Ss, Se, Ah, Al) of the coefficients; ``limits``: an iterator of end-of-band run limits."""
    comps, ss, se, ah, al = scan
    order, comp = scan_order(geometry, comps)
    if ss == 0 and ah == 0:
        return _dc_first([int(coef[b, 0]) for b in order], comp, al)
    if ss == 0:
        return [(-1, 0, int(coef[b, 0]) >> al & 1, 1) for b in order]
    return (_ac_refine if ah else _ac_first)(coef[order].tolist(), min(comps[0], 1), ss, se, al, limits)


def scan_tables(tokens, given=None):
    """[table 0, table 1] for the tokens: the given one, else libjpeg's optimal table of the tokens' own symbol counts; None: unused."""
    specs = [None, None]
    for k in sorted({tok[0] for tok in tokens if tok[0] >= 0}):
        specs[k] = (given or {}).get(k) or O.optimal_table(np.bincount([tok[1] for tok in tokens if tok[0] == k], minlength=256))
    return specs


def token_bits(tokens, specs):
    lengths = [J.huff_codes(s)[1] if s is not None else None for s in specs]
    return sum((int(lengths[t][sym]) if t >= 0 else 0) + n for t, sym, _, n in tokens)


def progressive(coef, geometry, script, q=None, qsel=None, tables=None, eob_limits=(0x7FFF,), **hdr):
    """An SOF2 file of the coefficients under the scan ``script`` [(components, Ss, Se, Ah, Al)] - anything jpeg_file.parse(progressive=True)
    takes: DC first and refine, AC first, AC refine.  Luma uses table id 0, chroma id 1; ``tables`` {scan index: {id: (bits, vals)}}
    gives a scan's tables, every other scan gets libjpeg's optimal table of its own symbol counts.  ``eob_limits``: the longest
    end-of-band run to merge, taken in turn per run written and repeated (1: one EOB0 per block); a dict {scan index: such a sequence} sets them per scan."""
    h, w, c, sampling = geometry
    q = q or [(0, Q1), (1, Q2)][:2 if c == 3 else 1]
    out = O.header(h, w, c, 100, sampling if c == 3 else 0, [], qtables=q, qsel=qsel, sof=0xC2, sos=False, **hdr)
    shared = None if isinstance(eob_limits, dict) else itertools.cycle(eob_limits)
    for i, scan in enumerate(script):
        comps, ss, se, ah, al = scan
        tokens = scan_tokens(coef, geometry, scan, shared or itertools.cycle(eob_limits.get(i, (0x7FFF,))))
        specs = scan_tables(tokens, (tables or {}).get(i, {}))
        cls = 0 if ss == 0 else 1
        used = [k for k in (0, 1) if specs[k] is not None]
        out += O.dht_segments([specs[k] for k in used], [cls << 4 | k for k in used])
        out += O.sos_segment([(k + 1, min(k, 1) * 0x11) for k in comps], ss, se, ah, al) + pack(tokens, specs)
    return out + EOI


# ---- coverage ------------------------------------------------------------------------------------------------------------------------------------
class Coverage:
    """What the restatements' write pass met, counted through their ``trace`` hooks."""

    def __init__(self):
        self.kind = "sequential"
        self.symbols = collections.defaultdict(collections.Counter)          # (scan kind, class, table id) -> symbol -> count
        self.lengths = collections.defaultdict(set)                            # (scan kind, class, table id) -> code lengths
        self.long_phase = set()                                                # (code length >= 9, bit position mod 32)
        self.long_values = set()                                               # (class, size) of the value bits behind a 16-bit code
        self.values = collections.defaultdict(set)                             # (class, size) -> PATTERNS met
        self.straddle = collections.Counter()                                  # "code" / "value": cut by a multiple of 32 bits
        self.straddle_codes, self.straddle_values = set(), set()               # the code lengths and the (class, size) of those
        self.eob = collections.defaultdict(set)                                # scan kind -> (r, "0" / "1": the extra bits all that)
        self.eob_to_the_end = collections.Counter()                            # scan kind -> runs that end on the scan's last block
        self.steps = collections.defaultdict(set)                              # "zrl" / "run" -> 0, 1, 2 (several) history coefficients passed
        self.corrections = set()                                               # (bit, sign, Al, "first" / "refine": the scan kind that made the coefficient)
        self.run_blocks = collections.Counter()                                # blocks inside a run: ("bits" / "no bit", "before the end" / "at the end" of the stream)
        self.born = {}

    def symbol(self, cls, tid, sym, ln, pos, s, v, k=None):
        key = (self.kind, cls, tid)
        self.symbols[key][sym] += 1
        self.lengths[key].add(ln)
        if ln >= 9:
            self.long_phase.add((ln, pos % 32))
        if pos // 32 != (pos + ln - 1) // 32:
            self.straddle["code"] += 1
            self.straddle_codes.add(ln)
        if s and self.kind != "AC refine":
            if ln == 16:
                self.long_values.add((cls, s))
            if (pos + ln) // 32 != (pos + ln + s - 1) // 32:
                self.straddle["value"] += 1
                self.straddle_values.add((cls, s))
            for name, x in zip(PATTERNS, (1 << (s - 1), (1 << s) - 1, 0, (1 << (s - 1)) - 1)):
                if v == x:
                    self.values[(cls, s)].add(name)

    def end_of_band(self, kind, r, extra, pos, to_the_end):
        name = {1: "AC first", 2: "AC refine"}[kind]
        if extra == 0:
            self.eob[name].add((r, "0"))
        if extra == (1 << r) - 1:
            self.eob[name].add((r, "1"))
        self.eob_to_the_end[name] += bool(to_the_end)

    def put(self, b, k, al, refine):
        self.born[(b, k)] = "refine" if refine else "first"

    def step(self, what, r, passed):
        self.steps[what].add(min(passed, 2))

    def correction(self, bit, v, al, b, k):
        self.corrections.add((bit, "+" if v > 0 else "-", al, self.born[(b, k)]))

    def run_block(self, takes_bits, at_the_end):
        self.run_blocks[("bits" if takes_bits else "no bit", "at the end" if at_the_end else "before the end")] += 1

    def add(self, other):
        for name in ("symbols", "lengths", "values", "eob", "steps"):
            mine = getattr(self, name)
            for key, v in getattr(other, name).items():
                mine[key] = mine[key] + v if isinstance(v, collections.Counter) else mine[key] | v
        for name in ("long_phase", "long_values", "corrections", "straddle_codes", "straddle_values"):
            setattr(self, name, getattr(self, name) | getattr(other, name))
        for name in ("straddle", "eob_to_the_end", "run_blocks"):
            getattr(self, name).update(getattr(other, name))
        return self


def is_progressive(data):
    return any(m == 0xC2 for m in _markers(data))


def _markers(data):
    at = 2
    while data[at + 1] != 0xDA:
        if data[at + 1] == 0xFF:
            at += 1
            continue
        yield data[at + 1]
        at += 2 + int.from_bytes(data[at + 2:at + 4], "big")


def coverage(data):
    """The file walked once, sequentially, by the restatement of its kind -> Coverage.  The status must come out 0."""
    cov = Coverage()
    if is_progressive(data):
        info = P.parse(data)
        H, V = R.LUMA_HV[info["sampling"]]
        coef = np.zeros((-(-info["w"] // (8 * H)) * -(-info["h"] // (8 * V)) * (H * V + 2 if info["c"] == 3 else 1), 64), np.int64)
        for sc in info["scans"]:
            S, out = P.Scan(info, sc, data), P.Out(coef)
            S.trace, cov.kind = cov, ("DC first", "AC first", "AC refine", "DC refine")[S.kind]
            P.decode_scan(S, out)
            assert not out.err and out.done == 1
        return cov
    info = RR.parse(data)
    sts, _ = RR.intervals(info, data)
    for st in sts:
        st.trace = cov
    assert RR.merge(info, sts, RR.decode_sequential(sts))[1] == 0
    return cov


# ---- content ---------------------------------------------------------------------------------------------------------------------------------------
def random_blocks(seed, n, qz=None, symbols=None, stops=(0.02, 0.1, 0.3, 1.0)):
    """n blocks of seeded coefficients whose run/size symbols come from ``symbols`` (default: all 160, and ZRL), half of the values one of
    the four extremes of their size, every block inside BUDGET under the zigzag-order steps ``qz``; DC values in -40..40, three in ten in -1000..1000."""
    rng = np.random.default_rng(seed)
    qz = np.ones(64, np.int64) if qz is None else qz
    allowed = [s for s in (symbols or AC_SYMBOLS) if s & 15]
    zrl = symbols is None or 0xF0 in symbols
    out = np.zeros((n, 64), np.int64)
    for b in range(n):
        out[b, 0] = rng.integers(-40, 41) if rng.random() < 0.7 else rng.integers(-1000, 1001)
        k, left, misses, stop = 1, BUDGET - abs(int(out[b, 0])) // 2 - 20, 0, stops[rng.integers(len(stops))]
        while k <= 63 and misses < 4 and rng.random() >= stop:
            sym = allowed[rng.integers(len(allowed))]
            r, s = (sym >> 4) + (16 * int(rng.integers(1, 4)) if zrl and rng.random() < 0.1 else 0), sym & 15
            if k + r > 63:
                misses += 1
                continue
            v = extremes(s)[rng.integers(len(extremes(s)))] if rng.random() < 0.5 else int(rng.integers(1 << (s - 1), 1 << s)) * (1 if rng.random() < 0.5 else -1)
            if abs(v) * qz[k + r] > left or (k + r >= 58 and abs(v) > 127):
                misses += 1
                continue
            out[b, k + r] = v
            left -= abs(v) * qz[k + r]
            k += r + 1
    return out


def symbol_blocks():
    """One component's designed blocks, in its scan order (about 900):
      a  every run/size symbol (16 runs x 10 sizes) at the four extreme values, from the DC term or behind a leading coefficient
      b  ZRL chains of 1, 2 and 3 that end at index 63 (no EOB), 62 and 60 (EOB), with runs 16 n + 0, 7, 15
      c  an EOB at every index: dense +-1 up to k, and one coefficient alone at k, for k = 0..62
      d  per DC category 0..11 the four extreme differences, as pairs of blocks without AC whose DC values stay inside +-1024
    The DC values outside d cycle through -3..3."""
    blocks = []

    def block(dc=None, **at):
        z = np.zeros(64, np.int64)
        z[0] = len(blocks) * 5 % 7 - 3 if dc is None else dc
        for k, v in at.items():
            z[int(k[1:])] = v
        blocks.append(z)

    for r in range(16):
        for s in range(1, 11):
            for i, v in enumerate((extremes(s) * 2)[:4]):
                lead = 0 if i % 2 == 0 else (r * 7 + s) % 40 + 1
                block(**({f"k{lead}": 1 if s % 2 else -1} if lead else {}), **{f"k{lead + 1 + r}": v})
    n = 0
    for nz in (1, 2, 3):
        for end in (63, 62, 60):
            for rr in (0, 7, 15):
                first = end - (16 * nz + rr) - 1
                if first < 0:
                    continue
                s = n % 7 + 1
                v = (extremes(s) * 2)[n % 4]
                n += 1
                block(**({f"k{first}": -1} if first else {}), **{f"k{end}": v})
    for k in range(63):
        block(**{f"k{j}": 1 if (j + k) % 3 else -1 for j in range(1, k + 1)})
        if k:
            block(**{f"k{k}": 2 if k % 2 else -3})
    for s in range(12):
        for d in extremes(s):
            block(dc=-(d // 2))
            block(dc=-(d // 2) + d)
    return np.stack(blocks)


def dc_blocks():
    """Part d of ``symbol_blocks`` alone: blocks without AC."""
    base = symbol_blocks()
    return base[~base[:, 1:].any(axis=1) & (np.abs(base[:, 0]) > 3)]


def component_content(n, roll, seed, qz=None, symbols=None):
    """n blocks for one component: the designed blocks rolled by ``roll`` (between 250 and 600, so that the cut falls between two
    blocks of part a), again while they fit, the rest seeded noise blocks.  ``symbols``: the AC symbols the file's table has, where it
    has not all - then the DC pairs of part d and seeded noise blocks of those symbols."""
    if symbols is not None:
        base = dc_blocks()
        return np.concatenate([base, random_blocks(seed, n - len(base), qz, symbols)]) if n >= len(base) else random_blocks(seed, n, qz, symbols)
    base = symbol_blocks()
    parts, left = [], n
    while left >= len(base):
        parts.append(np.roll(base, roll + 4 * len(parts), axis=0))
        left -= len(base)
    parts.append(random_blocks(seed, left, qz))
    return np.concatenate(parts)


def designed_coefficients(geometry, seed=0, steps=(1, 2, 2), symbols=None, progressive=False):
    """The MCU-ordered coefficients of a file of the geometry: ``component_content`` per component (steps: the quantisation step of each
    at 58..63).  ``progressive``: the dummy luma blocks of partial MCUs are zero, as one-component scans leave them."""
    H, V, mh, mw, comp_of = layout(geometry)
    per = []
    for k in range(geometry[2]):
        qz = np.ones(64, np.int64)
        qz[58:] = steps[k]
        per.append(component_content(mh * mw * (H * V if k == 0 else 1), 260 + 100 * k, seed * 10 + k, qz, symbols[k] if symbols else None))
    coef = assemble(geometry, per)
    if progressive:
        coef[~real_blocks(geometry)] = 0
    return coef


# ---- the designed sets ---------------------------------------------------------------------------------------------------------------------------
Designed = collections.namedtuple("Designed", "data coef geometry q twin")          # q [c, 64] natural per component; twin: a progressive file's baseline twin

GREY, C444, C422, C420 = (237, 235, 1, 0), (237, 235, 3, 0), (237, 475, 3, 1), (475, 477, 3, 2)          # 30 x 30 MCUs each, the last row and column partial
SMALL = [(33, 17, 3, 2), (17, 33, 3, 2), (33, 17, 3, 1), (17, 33, 3, 1)]
# Under the chain tables every bit string is a row of valid codes and all components share one code, so a lane that starts inside a block
# never finds the block's place in the MCU again: the rounds grow with the stream.  The colour files under those tables are 30 MCUs.
# The same holds under the tables whose codes are all 8 or 16 bits long, and the streams of deep refinements settle slowly as well: those
# colour files are 64 and 128 MCUs, which keeps the lane simulation of every file within seconds.
CHAIN_420, MID_420, MID_422 = (75, 91, 3, 2), (123, 125, 3, 2), (61, 251, 3, 1)
LAYOUT_NAME = {GREY: "grey", C444: "4:4:4", C422: "4:2:2", C420: "4:2:0", CHAIN_420: "4:2:0", MID_420: "4:2:0", MID_422: "4:2:2"}
DC_UP, DC_DOWN = list(range(16)), [12, 13, 14, 15] + list(range(12))          # sizes 12..15: symbols no good file uses, there to make the chain
SIZE_10 = [r << 4 | 10 for r in range(16)]
STD_Q = {1: [Q1], 3: [Q1, Q2, Q2]}


def _slots(c, dc, ac):
    return [dc, ac, dc, ac][:4 if c == 3 else 2]


def _baseline(geometry, dht, symbols=None, seed=0, q=None, qsel=None, **kw):
    c = geometry[2]
    tables = dict(q) if q else {0: Q1, 1: Q2}
    per = [tables[i] for i in (qsel or (0, 1, 1))[:c]]
    coef = designed_coefficients(geometry, seed, [int(t[63]) for t in per] + [1, 1], [symbols] * 3 if symbols else None)
    hdr = dict(kw, **({"qsel": qsel} if qsel else {}))
    return Designed(baseline(coef, geometry, dht, q, **hdr), coef, geometry, np.stack(per), None)


def _decoy(cls):
    """A table that is in the file and must not be used: every code of it means a symbol the content does not have."""
    return chain_table([12, 13, 14, 15]) if cls == 0 else chain_table([0x0B, 0x1B, 0x2B])


def _variants():
    std = O.STANDARD
    tail = [tail_table(DC_SYMBOLS, [10, 11]), tail_table(AC_SYMBOLS, SIZE_10)]
    mixed = [std[0], tail[1], tail[0], std[3]]
    return {
        "B-lengths swapped selectors, one DHT segment, SOF1 4:2:2": lambda: _baseline(C422, mixed, seed=11, sel=(0x11, 0x00, 0x00), one_dht=True, sof=0xC1),
        "B-lengths Cb and Cr on different tables, three DQTs with ids up to 3, a fill byte 4:4:4":
            lambda: _baseline(C444, mixed, seed=12, sel=(0x00, 0x10, 0x01), q=[(0, Q1), (3, Q2), (2, Q3)], qsel=(0, 3, 2), fill=True),
        "B-lengths a table defined twice, unused tables 2 and 3 4:2:0":
            lambda: _baseline(C420, [_decoy(1), std[0], mixed[1], _decoy(0), mixed[2], std[3], _decoy(1), _decoy(0)], seed=13,
                              dht_ids=(0x10, 0x00, 0x10, 0x01, 0x01, 0x11, 0x13, 0x02)),
        "B-lengths SOF1, a table defined twice, quantisation table 3 grey":
            lambda: _baseline(GREY, [_decoy(0), tail[0], tail[1]], seed=14, dht_ids=(0x00, 0x00, 0x10), sof=0xC1, q=[(3, Q1)], qsel=(3,)),
    }


def _baseline_sets():
    out = {}
    for g in (GREY, C444, C422, C420):
        out[f"B-symbols {LAYOUT_NAME[g]}"] = functools.partial(_baseline, g, O.STANDARD[:4 if g[2] == 3 else 2])
    for g in SMALL:
        out[f"B-symbols {g[0]}x{g[1]} sampling {g[3]}"] = functools.partial(_baseline, g, O.STANDARD, seed=g[0] + g[3])
    for g in (GREY, CHAIN_420):
        c = g[2]
        out[f"B-lengths chain up {LAYOUT_NAME[g]}"] = functools.partial(_baseline, g, _slots(c, chain_table(DC_UP), chain_table(CHAIN_AC)), CHAIN_AC, 1)
        out[f"B-lengths chain down {LAYOUT_NAME[g]}"] = functools.partial(_baseline, g, _slots(c, chain_table(DC_DOWN), chain_table(CHAIN_AC[::-1])), CHAIN_AC, 2)
        out[f"B-lengths 16-bit codes for sizes 10 and 11 {LAYOUT_NAME[g]}"] = functools.partial(
            _baseline, MID_420 if c == 3 else g, _slots(c, tail_table(DC_SYMBOLS, [10, 11]), tail_table(AC_SYMBOLS, SIZE_10)), None, 3)
    out["B-lengths optimal tables of geometric counts 4:4:4"] = functools.partial(
        _baseline, C444, [spread_table(DC_SYMBOLS, 1), spread_table(AC_SYMBOLS, 2), spread_table(DC_SYMBOLS, 3), spread_table(AC_SYMBOLS, 4)], None, 4)
    out.update(_variants())
    for g, ri in ((GREY, 1), (GREY, 7), (GREY, 13), (C444, 1), (C420, 7), (C422, 13)):
        out[f"B-restart Ri {ri} {LAYOUT_NAME[g]}"] = functools.partial(_baseline, g, O.STANDARD[:4 if g[2] == 3 else 2], None, 20 + ri, ri=ri)
    return out


def _all(c, *bands):
    """Script pieces: every component in turn through the AC scans (Ss, Se, Ah, Al) of ``bands``."""
    return [((k,), *b) for k in range(c) for b in bands]


def scripts(c):
    everyone = tuple(range(c))
    out = {
        "spectral selection": [(everyone, 0, 0, 0, 0)] + _all(c, (1, 1, 0, 0), (2, 5, 0, 0), (6, 62, 0, 0), (63, 63, 0, 0)),
        "deep approximation": [(everyone, 0, 0, 0, 4)] + [(everyone, 0, 0, a, a - 1) for a in (4, 3, 2, 1)]
                              + _all(c, (1, 63, 0, 3), (1, 63, 3, 2), (1, 63, 2, 1), (1, 63, 1, 0)),
        "one-component DC scans": [((k,), 0, 0, 0, 1) for k in range(c)] + _all(c, (1, 63, 0, 0)) + [((k,), 0, 0, 1, 0) for k in reversed(range(c))],
    }
    if c == 1:
        out["Pillow's script"] = [((0,), 0, 0, 0, 1), ((0,), 1, 5, 0, 2), ((0,), 6, 63, 0, 2), ((0,), 1, 63, 2, 1), ((0,), 0, 0, 1, 0), ((0,), 1, 63, 1, 0)]
    else:
        out["Pillow's script"] = [(everyone, 0, 0, 0, 1), ((0,), 1, 5, 0, 2), ((2,), 1, 63, 0, 1), ((1,), 1, 63, 0, 1), ((0,), 6, 63, 0, 2), ((0,), 1, 63, 2, 1),
                                  (everyone, 0, 0, 1, 0), ((2,), 1, 63, 1, 0), ((1,), 1, 63, 1, 0), ((0,), 1, 63, 1, 0)]
    return out


PROGRESSIVE_AC_SYMBOLS = AC_SYMBOLS + [r << 4 for r in range(1, 15)]


def _progressive(geometry, script, seed, eob_limits=(0x7FFF,), tables=None):
    c = geometry[2]
    if tables == "16-bit codes":
        tables = {i: {0: tail_table(DC_SYMBOLS, [10, 11]) if sc[1] == 0 else tail_table(PROGRESSIVE_AC_SYMBOLS, SIZE_10)} for i, sc in enumerate(scripts(c)[script])}
    coef = designed_coefficients(geometry, seed, (1, 2, 2), progressive=True)
    q = np.stack(STD_Q[c])
    return Designed(progressive(coef, geometry, scripts(c)[script], eob_limits=eob_limits, tables=tables), coef, geometry, q,
                    baseline(coef, geometry, O.STANDARD[:4 if c == 3 else 2]))


RUN_LENGTHS = [n for r in range(15) for n in (1 << r, (2 << r) - 1)]          # per r = 0..14: the extra bits all 0, then all 1
RUN_GEOMETRY = (2512, 2512, 1, 0)                                             # 314 x 314 blocks: the runs and 310 blocks between them
RUN_SCRIPTS = {"AC first": [((0,), 0, 0, 0, 0), ((0,), 1, 63, 0, 0)],
               "AC refine": [((0,), 0, 0, 0, 0), ((0,), 1, 5, 0, 1), ((0,), 6, 63, 0, 0), ((0,), 1, 5, 1, 0)]}


def _runs(kind):
    """One grey file whose ``kind`` scan holds an end-of-band run of every length of RUN_LENGTHS, in that order with the longest last, so
    that it ends on the scan's last block; ten or eleven blocks that end at Se stand in front of each.  AC first: a run's first block
    ends behind a coefficient at index 3 on every second run.  AC refine (band 1..5, from Al 1): about nine blocks of a run have a
    coefficient with history (2, 3, -2, -3 at index 2: a correction bit 0 or 1), the others none, and the last run has none at all:
    its blocks take no bit, and the stream ends behind the run's extra bits with no pad bit: the decoder stands AT the stream's end with
    32 766 blocks to go."""
    nblk = (RUN_GEOMETRY[0] // 8) * (RUN_GEOMETRY[1] // 8)
    coef = np.zeros((nblk, 64), np.int64)
    coef[:, 0] = np.arange(nblk) % 9 - 4
    spare = nblk - sum(RUN_LENGTHS)
    at = 0
    for i, n in enumerate(RUN_LENGTHS):
        between = spare // len(RUN_LENGTHS) + (i < spare % len(RUN_LENGTHS))
        coef[at:at + between, 63 if kind == "AC first" else 5] = 1 - 2 * (i % 2)
        at += between
        if kind == "AC first":
            coef[at, 3] = (i % 2) * (5 - i)
        elif i + 1 < len(RUN_LENGTHS):
            marked = np.arange(at, at + n, max(1, n // 8))
            coef[marked, 2] = np.array([2, 3, -2, -3])[(np.arange(len(marked)) + i) % 4]
        at += n
    assert at == nblk
    script = RUN_SCRIPTS[kind]
    scan = len(script) - 1
    if kind == "AC refine":          # every further coefficient with history adds one correction bit: as many as end the scan on a byte
        tokens = scan_tokens(coef, RUN_GEOMETRY, script[scan], itertools.cycle(RUN_LENGTHS))
        coef[nblk - n - 100:nblk - n - 100 + -token_bits(tokens, scan_tables(tokens)) % 8, 4] = 2
    data = progressive(coef, RUN_GEOMETRY, script, eob_limits={scan: RUN_LENGTHS})
    return Designed(data, coef, RUN_GEOMETRY, np.stack([Q1]), baseline(coef, RUN_GEOMETRY, O.STANDARD[:2]))


def _progressive_sets():
    out = {}
    for name, g, script, seed, limits in (("P-scripts spectral selection, 16-bit codes for sizes 10 and 11, grey", GREY, "spectral selection", 31, (1,)),
                                          ("P-scripts spectral selection 4:4:4", C444, "spectral selection", 32, (1, 2, 3, 5, 0x7FFF)),
                                          ("P-scripts deep approximation grey", GREY, "deep approximation", 33, (0x7FFF,)),
                                          ("P-scripts deep approximation 4:2:0", MID_420, "deep approximation", 34, (1, 4, 0x7FFF)),
                                          ("P-scripts one-component DC scans 4:2:0", C420, "one-component DC scans", 35, (0x7FFF,)),
                                          ("P-scripts one-component DC scans 4:2:2", C422, "one-component DC scans", 36, (2, 0x7FFF)),
                                          ("P-scripts Pillow's script grey", GREY, "Pillow's script", 37, (0x7FFF,)),
                                          ("P-scripts Pillow's script 4:2:2", MID_422, "Pillow's script", 38, (0x7FFF,))):
        out[name] = functools.partial(_progressive, g, script, seed, limits, "16-bit codes" if "16-bit" in name else None)
    for g in SMALL[:2] + SMALL[3:]:
        out[f"P-scripts one-component DC scans {g[0]}x{g[1]} sampling {g[3]}"] = functools.partial(_progressive, g, "one-component DC scans", 40 + g[0] + g[3])
    for kind in RUN_SCRIPTS:
        out[f"P-runs {kind}"] = functools.partial(_runs, kind)
    return out


BASELINE = _baseline_sets()
PROGRESSIVE = _progressive_sets()
GOOD = {**BASELINE, **PROGRESSIVE}


@functools.lru_cache(maxsize=None)
def good(name):
    """The file ``name`` of GOOD: built once, shared by every test."""
    d = GOOD[name]()
    d.coef.setflags(write=False)
    return d


# ---- the status files: structurally legal, one designed rule break each -----------------------------------------------------------------------
def _grey_scans(h, w, scans, sof=0xC2):
    """A grey file written token by token: scans of (Ss, Se, Ah, Al, the scan's one table or None, tokens)."""
    out = O.header(h, w, 1, 100, 0, [], qtables=[(0, Q1)], sof=sof, sos=False)
    for ss, se, ah, al, spec, tokens in scans:
        if spec is not None:
            out += O.dht_segments([spec], [0x00 if ss == 0 else 0x10])
        out += O.sos_segment([(1, 0x00)], ss, se, ah, al) + pack(tokens, [spec])
    return out + EOI


def _dc_zero(n, al=0):
    return (0, 0, 0, al, chain_table([0, 1, 2]), [(0, 0, 0, 0)] * n)


def _eob_run(ss, se, ah, al, r):
    return (ss, se, ah, al, chain_table([r << 4]), [(0, r << 4, 0, r)])


def _status_files():
    four = (8, 32, 1, 0)
    dc12 = np.zeros((4, 64), np.int64)
    dc12[:, 0] = [-1024, 1024, 0, 5]
    ac11 = np.zeros((4, 64), np.int64)
    ac11[1, 1] = 1024
    high = np.zeros((4, 64), np.int64)
    high[:, 0] = [1024, 2048, 1030, 5]
    std = O.STANDARD[:2]
    past63 = [(0, 0, 0, 0)] + [(1, 0xF0, 0, 0)] * 3 + [(1, 0xB1, 1, 1), (1, 0x51, 1, 1), (0, 0, 0, 0), (1, 0x00, 0, 0)]          # index 1 + 48 + 11 = 60, then 61 + 5 = 66
    return {
        "baseline: DC size 12": lambda: baseline(dc12, four, [tail_table(list(range(13)), [12]), std[1]]),
        "baseline: AC size 11": lambda: baseline(ac11, four, [std[0], tail_table(AC_SYMBOLS + [0x0B], [0x0B])]),
        "baseline: a run that puts the index past 63": lambda: O.header(8, 16, 1, 100, 0, std, qtables=[(0, Q1)]) + pack(past63, std) + EOI,
        "baseline: a DC sum of +2048": lambda: baseline(high, four, std),
        "baseline: a DC sum of -2048": lambda: baseline(-high, four, std),
        "progressive: ZRL past Se": lambda: _grey_scans(8, 16, [_dc_zero(2), (1, 5, 0, 0, chain_table([0x00, 0xF0]), [(0, 0xF0, 0, 0), (0, 0x00, 0, 0)]),
                                                               _eob_run(6, 63, 0, 0, 1)]),
        "progressive: an index past Se": lambda: _grey_scans(8, 16, [_dc_zero(2), (1, 5, 0, 0, chain_table([0x00, 0x61]), [(0, 0x61, 1, 1), (0, 0x00, 0, 0)]),
                                                                    _eob_run(6, 63, 0, 0, 1)]),
        "progressive: refinement size 2": lambda: _grey_scans(8, 16, [_dc_zero(2), _eob_run(1, 63, 0, 1, 1),
                                                                     (1, 63, 1, 0, chain_table([0x00, 0x02]), [(0, 0x02, 1, 1), (0, 0x00, 0, 0), (0, 0x00, 0, 0)])]),
        "progressive: AC first, size 10 at Al = 6": lambda: _grey_scans(8, 16, [_dc_zero(2), (1, 63, 0, 6, chain_table([0x00, 0x0A]),
                                                                                            [(0, 0x0A, 1023, 10), (0, 0x00, 0, 0), (0, 0x00, 0, 0)])]
                                                                       + [_eob_run(1, 63, a, a - 1, 1) for a in range(6, 0, -1)]),
        "progressive: a DC-refine stream one byte short": lambda: _grey_scans(8, 128, [_dc_zero(16, 1), (0, 0, 1, 0, None, [(-1, 0, 0, 1)] * 8), _eob_run(1, 63, 0, 0, 4)]),
    }


STATUS = _status_files()


@functools.lru_cache(maxsize=None)
def status_file(name):
    return STATUS[name]()
