"""Plain Python restatement of the device decoder for progressive JPEG files (csrc/jpeg_decode.hip, adain_jpeg_decode_progressive_u8): a marker
walk of its own (not the package's parser), a sequential decoder of the four scan kinds, and the device's scheme - every Huffman-coded
scan cut into subsequences whose exit states are iterated to the fixed point - simulated lane by lane, which predicts the device's round
count.  The back half (dequantisation, IDCT, upsampling, colour) is tests/jpeg_file_ref.py's.  Every index formed here is asserted to be
in range, so a damaged file can be walked on the CPU before a device sees it.  tests/test_jpeg_progressive_host.py holds all of it to Pillow.

The rules (the ones the device shares)
  streams    every scan's segment runs from behind its SOS to the next marker that is not a stuffed FF 00; the 00 behind every FF is
             removed; bits big-endian; past the end the reader returns 1-bits
  blocks     an interleaved scan covers the MCU grid (per MCU the H x V luma blocks row-major, then Cb, Cr); a one-component scan covers
             the component's own raster of ceil(ceil(w Hi / Hmax) / 8) by ceil(ceil(h Vi / Vmax) / 8) blocks, row-major; block (by, bx)
             of it is block (by % V) H + bx % H of MCU (by / V) mw + bx / H.  Blocks no scan codes stay zero
  symbol     the shortest code of the table that matches; none of 1..16 bits: ONE bit is consumed, and that is damage
  DC first   symbol & 15 = size s, s bits v, difference = v if v >= 2^(s-1) else v - 2^s + 1; summed per component in SCAN order; the DC
             term is the sum << Al.  State: (position, block in MCU)
  DC refine  bit i of the stream belongs to block i of the scan; a set bit ORs 1 << Al into the DC term
  AC first   at zigzag index k (Ss at a block's start) symbol = r << 4 | s.  s > 0: k += r, the coefficient there = value << Al, k += 1.
             s = 0, r = 15: k += 16.  s = 0, r < 15: run = 2^r + the next r bits; this block ends and run - 1 more blocks are empty, all
             in this one step.  k > Se ends the block.  State: (position, k)
  AC refine  outside a run: symbol r << 4 | s; s > 0: one sign bit at once; s = 0, r < 15: run = 2^r + r bits and the rest of the block is
             walked as inside a run; else walk from k: a coefficient with history (non-zero BEFORE this scan) reads a correction bit, one
             without counts r down, the walk stops at the first such one met at r = 0; s > 0 puts +-(1 << Al) there; k moves behind it.
             Inside a run: one correction bit per coefficient with history from k to Se, the block ends, the run is one shorter.  A set
             correction bit adds 1 << Al away from zero where (coefficient & (1 << Al)) == 0.  Decoding stops at the scan's last block;
             the blocks of a run may take no bit at all, so the stream's last subsequence goes on while a run is under way and the position has not passed the end.
             State: (position, block, run, k)
  damage     in a block the scan covers: no code, DC size > 11, AC-first size > 10, refinement size > 1, an index past Se, a value or DC
             sum << Al that is no int16; a scan whose last block does not end inside the stream's last byte or is never reached; a final
             DC term outside -2047..2047
"""
import numpy as np

import jpeg_file_ref as R
from jpeg_file_ref import Refused, code_table, unstuff
from jpeg_ref import ZIGZAG

MAX_SCANS = 32


# ---- the marker walk -----------------------------------------------------------------------------------------------------------------------
def parse(data):
    """bytes -> dict(h, w, c, sampling, q [c,64] natural, scans [dict(comps, ss, se, ah, al, seg, huff, dc, ac)]) or Refused."""
    data = bytes(data)
    if data[:2] != b"\xff\xd8":
        raise Refused("no SOI")
    q, huff, frame, at, scans = {}, {}, None, 2, []
    while True:
        if at + 2 > len(data) or data[at] != 0xFF:
            raise Refused("truncated or no marker")
        m = data[at + 1]
        if m == 0xFF:
            at += 1
            continue
        if m == 0xD9:
            break
        if at + 4 > len(data):
            raise Refused("truncated")
        ln = int.from_bytes(data[at + 2:at + 4], "big")
        if ln < 2 or at + 2 + ln > len(data):
            raise Refused("segment past the end")
        body = data[at + 4:at + 2 + ln]
        at += 2 + ln
        if m == 0xC2:
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
        elif m == 0xDB:
            if scans:
                raise Refused("DQT behind a scan")
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
                huff[(body[p] >> 4, body[p] & 15)] = (bits, list(body[p + 17:p + 17 + sum(bits)]))
                p += 17 + sum(bits)
        elif m == 0xDD:
            if int.from_bytes(body, "big") != 0 or scans:
                raise Refused("restart interval")
        elif 0xE0 <= m <= 0xEF or m == 0xFE:
            pass
        elif m == 0xDA:
            if frame is None or len(scans) == MAX_SCANS:
                raise Refused("scan before frame, or too many")
            h, w, comps = frame
            ids = [c[0] for c in comps]
            ns = body[0]
            if len(body) != 4 + 2 * ns or any(body[1 + 2 * i] not in ids for i in range(ns)):
                raise Refused("scan header")
            cis = [ids.index(body[1 + 2 * i]) for i in range(ns)]
            dc, ac = [0] * len(comps), [0] * len(comps)
            for i, ci in enumerate(cis):
                dc[ci], ac[ci] = body[2 + 2 * i] >> 4, body[2 + 2 * i] & 15
            ss, se, ah, al = body[-3], body[-2], body[-1] >> 4, body[-1] & 15
            if not (ss == se == 0 and (ns == 1 or cis == list(range(len(comps)))) or 1 <= ss <= se <= 63 and ns == 1) or al > 13 or max(dc + ac) > 1:
                raise Refused("scan parameters")
            end = at
            while True:
                end = data.find(b"\xff", end)
                if end < 0 or end + 1 >= len(data):
                    raise Refused("no marker behind the scan")
                if data[end + 1] != 0:
                    break
                end += 2
            scans.append(dict(comps=cis, ss=ss, se=se, ah=ah, al=al, seg=(at, end - at), huff=dict(huff), dc=dc, ac=ac))
            at = end
        else:
            raise Refused(f"marker {m:02X}")
    if frame is None or not scans or any(c[3] not in q for c in frame[2]):
        raise Refused("no frame, no scan or no quantisation table")
    h, w, comps = frame
    # the script: first scans at Ah = 0, refinements one bit at a time, complete at EOI
    al_of = [[-1] * 64 for _ in comps]
    for sc in scans:
        for ci in sc["comps"]:
            band = set(al_of[ci][sc["ss"]:sc["se"] + 1])
            if len(band) != 1 or (sc["ss"] > 0 and al_of[ci][0] < 0):
                raise Refused("script: mixed histories, or AC before DC")
            was = band.pop()
            if (was < 0 and sc["ah"] != 0) or (was >= 0 and (sc["ah"] != was or sc["al"] != was - 1)):
                raise Refused("script: Ah / Al")
            al_of[ci][sc["ss"]:sc["se"] + 1] = [sc["al"]] * (sc["se"] + 1 - sc["ss"])
    if any(a != 0 for c in al_of for a in c):
        raise Refused("script: incomplete")
    return dict(h=h, w=w, c=len(comps), sampling={(1, 1): 0, (2, 1): 1, (2, 2): 2}[comps[0][1:3]], q=np.stack([q[c[3]] for c in comps]), scans=scans)


# ---- one scan --------------------------------------------------------------------------------------------------------------------------------
class Scan:
    """A scan's stream, tables and block geometry."""
    trace = None             # an object that takes the write pass's walk: symbol(), end_of_band(), step(), correction(), put(), run_block()

    def __init__(self, info, sc, data):
        self.dc_id, self.ac_id = list(sc["dc"]), list(sc["ac"])
        off, ln = sc["seg"]
        self.bytes = unstuff(data[off:off + ln])
        self.nbits = 8 * len(self.bytes)
        self.padded = self.bytes + b"\xff" * 16
        self.H, self.V = R.LUMA_HV[info["sampling"]]
        self.c, self.ss, self.se, self.ah, self.al = info["c"], sc["ss"], sc["se"], sc["ah"], sc["al"]
        self.bpm_frame = self.H * self.V + 2 if self.c == 3 else 1
        self.mw, self.mh = -(-info["w"] // (8 * self.H)), -(-info["h"] // (8 * self.V))
        self.frame_blocks = self.mw * self.mh * self.bpm_frame
        self.inter = len(sc["comps"]) == self.c
        self.comp = sc["comps"][0]
        if self.inter:
            self.comp_of = [0] * (self.H * self.V) + [1, 2] if self.c == 3 else [0]
            self.nblk = self.frame_blocks
        else:
            self.comp_of = [self.comp]
            cw = info["w"] if self.comp == 0 else -(-info["w"] // self.H)
            ch = info["h"] if self.comp == 0 else -(-info["h"] // self.V)
            self.bw = -(-cw // 8)
            self.nblk = self.bw * -(-ch // 8)
        self.bpm = len(self.comp_of)
        self.kind = (0 if self.ah == 0 else 3) if self.ss == 0 else (1 if self.ah == 0 else 2)
        empty = ([0] * 16, [])
        self.dc = [code_table(*sc["huff"].get((0, t), empty)) for t in sc["dc"]]
        self.ac = [code_table(*sc["huff"].get((1, t), empty)) for t in sc["ac"]]

    def peek(self, pos, n):
        assert 0 <= pos <= self.nbits + 128 and 0 <= n <= 32
        at = min(pos >> 3, len(self.bytes))
        return (int.from_bytes(self.padded[at:at + 8], "big") >> (64 - (pos & 7) - n)) & ((1 << n) - 1) if pos < self.nbits else (1 << n) - 1

    def symbol(self, table, pos):
        return table[self.peek(pos, 16)] or (None, 1)

    def block(self, sb):
        """Scan-order block -> its index in the MCU-ordered coefficient buffer."""
        assert 0 <= sb < self.nblk
        if self.inter:
            b = sb
        elif self.comp > 0:
            b = sb * self.bpm_frame + self.H * self.V + self.comp - 1
        else:
            by, bx = divmod(sb, self.bw)
            b = ((by // self.V) * self.mw + bx // self.H) * self.bpm_frame + (by % self.V) * self.H + bx % self.H
        assert 0 <= b < self.frame_blocks
        return b


class Out:
    """What a write pass leaves: the coefficients (zigzag order, MCU-ordered blocks), damage, whether the last block ended, the runs read."""

    def __init__(self, coef):
        self.coef, self.err, self.done, self.runs = coef, False, 0, []

    def last_block(self, S, pos):
        if S.nbits - 8 < pos <= S.nbits:
            self.done += 1
        else:
            self.err = True


def extend(v, s):
    return v if s == 0 or v >= 1 << (s - 1) else v - (1 << s) + 1


def fits(v):
    return -32768 <= v <= 32767


def correct(out, b, k, al):
    v = int(out.coef[b, k])
    if v & (1 << al) == 0:
        out.coef[b, k] = v + (1 << al) if v >= 0 else v - (1 << al)


def span(S, state, end, mask=None, out=None, b=0):
    """Decodes scan S from ``state`` while position < end -> (exit state, blocks begun).  ``out``: an Out that takes the coefficients,
    ``b``: the scan-order index of the block current at ``state``; ``mask[sb]``: the history of block sb (AC refine)."""
    nb = 0
    if S.kind == 0:
        pos, blk = state
        while pos < end:
            live = out is not None and 0 <= b < S.nblk
            sym, ln = S.symbol(S.dc[S.comp_of[blk]], pos)
            if sym is None:
                pos += 1
                if live:
                    out.err = True
                continue
            s = sym & 15
            value = extend(S.peek(pos + ln, s), s)
            nb += 1
            if live and S.trace:
                S.trace.symbol("DC", S.dc_id[S.comp_of[blk]], sym, ln, pos, s, S.peek(pos + ln, s))
            pos += ln + s
            if live:
                out.coef[S.block(b), 0] = value
                out.err |= sym > 11
                if b == S.nblk - 1:
                    out.last_block(S, pos)
            blk, b = (blk + 1) % S.bpm, b + 1
        return (pos, blk), nb
    if S.kind == 1:
        pos, k = state
        table, last = S.ac[S.comp], S.nblk - 1
        while pos < end:
            live = out is not None and 0 <= b <= last
            sym, ln = S.symbol(table, pos)
            if sym is None:
                pos += 1
                if live:
                    out.err = True
                continue
            if k == S.ss:
                nb += 1
            r, s = sym >> 4, sym & 15
            if live and S.trace:
                S.trace.symbol("AC", S.ac_id[S.comp], sym, ln, pos, s, S.peek(pos + ln, s), k)
            if s == 0 and r < 15:
                run = (1 << r) + S.peek(pos + ln, r)
                if live and S.trace:
                    S.trace.end_of_band(1, r, S.peek(pos + ln, r), pos + ln, b + run - 1 == last)
                pos += ln + r
                nb += run - 1
                if live:
                    out.runs.append(run)
                    if b + run - 1 >= last:
                        out.last_block(S, pos)
                b, k = b + run, S.ss
                continue
            if s == 0:
                pos += ln
                k += 16
                if k > S.se and live:
                    out.err = True
            else:
                value = extend(S.peek(pos + ln, s), s)
                pos += ln + s
                k += r
                if live:
                    val = value << S.al
                    if k <= S.se and fits(val):
                        out.coef[S.block(b), k] = val
                        if S.trace:
                            S.trace.put(S.block(b), k, S.al, False)
                    out.err |= k > S.se or s > 10 or not fits(val)
                k += 1
            if k > S.se:
                if live and b == last:
                    out.last_block(S, pos)
                k, b = S.ss, b + 1
        return (pos, k), nb
    assert S.kind == 2
    pos, blk, run, k = state
    table = S.ac[S.comp]
    while blk < S.nblk and (pos < end or (end == S.nbits and run > 0 and pos <= end)):           # a run's blocks may take no bit: the last subsequence ends them
        assert 0 <= blk < len(mask) and S.ss <= k <= S.se and 0 <= run <= 32767
        m = mask[blk]
        bc = S.block(blk)
        ends = run > 0
        T = S.trace if out is not None else None
        if T and ends:
            T.run_block(bool((m >> k) & ((1 << (S.se + 1 - k)) - 1)), pos >= end)
        if not ends:
            sym, ln = S.symbol(table, pos)
            if sym is None:
                pos += 1
                if out is not None:
                    out.err = True
                continue
            r, s = sym >> 4, sym & 15
            if T:
                T.symbol("AC", S.ac_id[S.comp], sym, ln, pos, s, S.peek(pos + ln, s), k)
            if s == 0 and r < 15:
                run = (1 << r) + S.peek(pos + ln, r)
                if T:
                    T.end_of_band(2, r, S.peek(pos + ln, r), pos + ln, blk + run == S.nblk)
                pos += ln + r
                ends = True
                if out is not None:
                    out.runs.append(run)
            else:
                pos += ln
                put = 0
                stepped = 0
                if s:
                    if out is not None and s != 1:
                        out.err = True
                    put = (1 << S.al) if S.peek(pos, 1) else -(1 << S.al)
                    pos += 1
                while k <= S.se:
                    if m >> k & 1:
                        if T:
                            T.correction(S.peek(pos, 1), int(out.coef[bc, k]), S.al, bc, k)
                        if S.peek(pos, 1) and out is not None:
                            correct(out, bc, k, S.al)
                        pos += 1
                        stepped += 1
                    else:
                        if r == 0:
                            break
                        r -= 1
                    k += 1
                if T:
                    T.step("run" if s else "zrl", sym >> 4, stepped)
                if out is not None:
                    if k > S.se:
                        out.err = True
                    elif put:
                        out.coef[bc, k] = put
                        if T:
                            T.put(bc, k, S.al, True)
                k += 1
                if k > S.se:
                    blk, k = blk + 1, S.ss
                    if out is not None and blk == S.nblk:
                        out.last_block(S, pos)
        if ends:
            while k <= S.se:
                if m >> k & 1:
                    if T:
                        T.correction(S.peek(pos, 1), int(out.coef[bc, k]), S.al, bc, k)
                    if S.peek(pos, 1) and out is not None:
                        correct(out, bc, k, S.al)
                    pos += 1
                k += 1
            run, blk, k = run - 1, blk + 1, S.ss
            if out is not None and blk == S.nblk:
                out.last_block(S, pos)
    return (pos, blk, run, k), 0


def start(S, pos):
    """The state every subsequence enters round 0 from, and the scan's true start at position 0."""
    return {0: (pos, 0), 1: (pos, S.ss), 2: (pos, 0, 0, S.ss)}[S.kind]


def history(S, coef):
    nz = (coef[[S.block(sb) for sb in range(S.nblk)]] != 0).astype(np.uint64)
    return (nz << np.arange(64, dtype=np.uint64)).sum(axis=1, dtype=np.uint64).tolist()


def dc_refine(S, out):
    if not (S.nbits - 8 < S.nblk <= S.nbits):
        out.err = True
    else:
        out.done += 1
    for sb in range(min(S.nblk, S.nbits)):
        if S.peek(sb, 1):
            out.coef[S.block(sb), 0] |= 1 << S.al


def dc_sums(S, out):
    """The differences of a DC-first scan -> (sum per component in scan order) << Al."""
    run = [0] * 3
    for sb in range(S.nblk):
        comp = S.comp_of[sb % S.bpm]
        run[comp] += int(out.coef[S.block(sb), 0])
        v = run[comp] << S.al
        out.err |= not fits(v)
        out.coef[S.block(sb), 0] = ((v + 32768) & 0xFFFF) - 32768


def decode_scan(S, out, chunk_bits=None):
    """Applies scan S to out.coef -> rounds (0: sequential, or a scan without a Huffman code)."""
    if S.kind == 3:
        dc_refine(S, out)
        return 0
    mask = history(S, out.coef) if S.kind == 2 else None
    rounds = 0
    if chunk_bits is None:
        span(S, start(S, 0), S.nbits, mask, out, 0)
    else:
        assert chunk_bits >= 32 and chunk_bits % 32 == 0
        nsub = -(-S.nbits // chunk_bits)
        ends = [min((i + 1) * chunk_bits, S.nbits) for i in range(nsub)]
        prev_in = [start(S, i * chunk_bits) for i in range(nsub)]
        res = [span(S, prev_in[i], ends[i], mask) for i in range(nsub)]
        rounds = 1 if nsub else 0
        while nsub and rounds < nsub + 1:
            ins = [start(S, 0)] + [r[0] for r in res[:-1]]
            new = [res[i] if ins[i] == prev_in[i] else span(S, ins[i], ends[i], mask) for i in range(nsub)]
            rounds += 1
            changed = any(a[0] != b[0] for a, b in zip(new, res))
            res, prev_in = new, ins
            if not changed:
                break
        if nsub == 0:
            rounds = 1              # the device's loop runs once on an empty stream
        first = np.concatenate([[0], np.cumsum([r[1] for r in res])]) if nsub else [0]
        for i in range(nsub):
            state = start(S, 0) if i == 0 else res[i - 1][0]
            b = int(first[i]) - (1 if S.kind == 1 and state[1] != S.ss else 0)
            span(S, state, ends[i], mask, out, b)
    if S.kind == 0:
        dc_sums(S, out)
    return rounds


def coefficients(data, chunk_bits=None, info=None):
    """bytes -> (info, coefficients [blocks, 64] zigzag with final DC terms, status, rounds, per scan the end-of-band runs read).
    ``info``: the file's description when it is not to be parsed from ``data`` (a test that hands a scan another scan's tables)."""
    info = info or parse(data)
    H, V = R.LUMA_HV[info["sampling"]]
    nblk = -(-info["w"] // (8 * H)) * -(-info["h"] // (8 * V)) * (H * V + 2 if info["c"] == 3 else 1)
    coef = np.zeros((nblk, 64), np.int64)
    bad, rounds, runs = False, 0, []
    for sc in info["scans"]:
        S, out = Scan(info, sc, data), Out(coef)
        rounds += decode_scan(S, out, chunk_bits)
        bad |= out.err or out.done != 1
        runs.append(out.runs)
    return info, coef, int(bad), rounds, runs


def decode(data, chunk_bits=None, info=None):
    """bytes of a progressive file -> (pixels uint8, status, rounds): sequentially, or (chunk_bits) by the device's scheme."""
    info, coef, status, rounds, _ = coefficients(data, chunk_bits, info)
    # jpeg_file_ref.pixels sums DC differences per component in MCU order: hand it the differences of the final terms
    H, V = R.LUMA_HV[info["sampling"]]
    bpm = H * V + 2 if info["c"] == 3 else 1
    z = coef.reshape(-1, bpm, 64).copy()
    for comp in range(info["c"]):
        js = list(range(H * V)) if comp == 0 else [H * V + comp - 1]
        dc = z[:, js, 0].reshape(-1)
        z[:, js, 0] = np.diff(dc, prepend=0).reshape(-1, len(js))
    sink = R.Sink(coef.shape[0])
    sink.coef = z.reshape(-1, 64)
    px, damage = R.pixels(info, sink)
    return px, int(bool(status) or damage), rounds
