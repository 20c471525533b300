"""Plain Python restatement of the device JPEG file decoder's restart-interval rules (csrc/jpeg_decode.hip, adain_jpeg_decode_restart_u8), on top
of tests/jpeg_file_ref.py: that file's entropy decoder, ``Sink``, ``decode_lanes`` and ``pixels`` are imported and run per interval; this
one adds the marker walk, the per-interval streams, the sequential decoder per interval and the lane scheme per interval.
tests/test_jpeg_restart_host.py holds all of it to Pillow.

The rules (the ones csrc/jpeg_decode.hip lists under "restart"; Ri > 0 MCUs, nmcu = mw mh, nint = ceil(nmcu / Ri), interval k holds the MCUs
k Ri .. min((k+1) Ri, nmcu) - 1 and expects bpm min(Ri, nmcu - k Ri) blocks)
  segment  from behind SOS to EOI; it holds FF D0..D7 pairs, and as unstuffed entropy data cannot, each such pair is a marker.  Byte by
           byte: dropped are a 00 behind an FF, an FF in front of a D0..D7 that is still in the segment, and a D0..D7 behind an FF
  stream   the kept bytes.  Marker m (0-based) ends interval m, interval m + 1 begins at the stream byte behind it, interval 0 at byte 0
  reader   inside interval k the bits at or beyond the interval's end read as 1; decoding never continues into the next interval; pad
           bits (at most 7 ones) complete no code, so they begin no block
  grid     interval k is cut into subsequences of chunk_bits bits from its own first bit, the last one shorter; in every round an
           interval's first subsequence enters from (its first bit, block 0, index 0), every other one from its left neighbour's exit
           state of the round before; the loop ends after the first round that changed no exit state in any interval - the largest
           round count any interval needs on its own
  blocks   a block's index is k Ri bpm plus the blocks begun before it in interval k; blocks at or above the interval's expected count
           are written by nobody and are not damage
  DC       the running sum per component restarts at 0 at every interval's first MCU
  status   non-zero when, in some interval: damage inside an expected block, a DC sum outside -2047..2047, fewer blocks than expected or
           a last expected block that does not end inside the interval's last byte; when the markers found are not nint - 1 or marker m
           is not FF D(m mod 8) (the entropy decode is then skipped: all coefficients zero); when the decode did not settle
With Ri = 0 the whole stream is one interval and nothing is removed but the stuffed zeros: tests/jpeg_file_ref.py's decoder.
"""
import copy

import numpy as np

import jpeg_file_ref as R
from jpeg_file_ref import Refused, Sink, decode_lanes as lanes_of_one, decode_span, pixels


# ---- the marker walk -------------------------------------------------------------------------------------------------------------------
def parse(data):
    """bytes -> jpeg_file_ref.parse's dict with ``ri`` (the DRI's value, 0 without one) and ``seg`` = (offset, length) of everything
    between SOS and EOI, restart markers included; Refused as there, and for an FF in the scan that is followed by neither 00, D0..D7
    nor D9."""
    data = bytes(data)
    at, ri, dri_at = 2, 0, None
    while True:                              # to SOS: the DRI's place, nothing else (the header is jpeg_file_ref.parse's to judge)
        if at + 4 > len(data) or data[at] != 0xFF:
            raise Refused("truncated or no marker")
        m, ln = data[at + 1], int.from_bytes(data[at + 2:at + 4], "big")
        if m == 0xFF:
            at += 1
            continue
        if m == 0xDD and ln == 4:
            ri, dri_at = int.from_bytes(data[at + 4:at + 6], "big"), at + 4
        if m == 0xDA:
            seg = at + 2 + ln
            break
        if ln < 2 or m in (0xD8, 0xD9):
            raise Refused("header")
        at += 2 + ln
    header = bytearray(data[:seg])
    if dri_at is not None:
        header[dri_at:dri_at + 2] = b"\0\0"
    info = R.parse(bytes(header) + b"\xff\xd9")          # the same file without its restart interval and with an empty scan
    end = seg
    while True:
        end = data.find(b"\xff", end)
        if end < 0 or end + 1 >= len(data):
            raise Refused("no EOI")
        if data[end + 1] == 0 or (ri and 0xD0 <= data[end + 1] <= 0xD7):
            end += 2
            continue
        break
    if data[end + 1] != 0xD9:
        raise Refused("a marker other than EOI or RSTn behind the scan")
    return dict(info, ri=ri, seg=(seg, end - seg))


def split(seg, restart=True):
    """The segment -> (stream bytes, the stream byte each marker stands in front of, each marker's low three bits)."""
    keep, at, numbers = bytearray(), [], []
    for i, c in enumerate(seg):
        behind_ff = i >= 1 and seg[i - 1] == 0xFF
        if behind_ff and c == 0:
            continue
        if restart and c == 0xFF and i + 1 < len(seg) and seg[i + 1] & 0xF8 == 0xD0:
            at.append(len(keep))
            numbers.append(seg[i + 1] & 7)
            continue
        if restart and behind_ff and c & 0xF8 == 0xD0:
            continue
        keep.append(c)
    return bytes(keep), at, numbers


# ---- the per-interval streams ------------------------------------------------------------------------------------------------------------
def intervals(info, data):
    """-> (one jpeg_file_ref.Stream per interval - its own bytes, its own end, ``nblk`` = the blocks it expects, ``first`` = the index of
    its first block - or None when the markers are not nint - 1 in number and D0..D7 in turn, the stream's length in bits)."""
    off, ln = info["seg"]
    base = R.Stream(dict(info, seg=(off, 0)), data)              # the tables, built once
    nmcu = base.nblk // base.bpm
    ri = info["ri"] or nmcu
    nint = -(-nmcu // ri)
    stream, at, numbers = split(data[off:off + ln], restart=info["ri"] > 0)
    if len(at) != nint - 1 or numbers != [m % 8 for m in range(len(at))]:
        return None, 8 * len(stream)
    bounds = [0] + at + [len(stream)]
    out = []
    for k in range(nint):
        st = copy.copy(base)
        st.bytes = stream[bounds[k]:bounds[k + 1]]
        st.nbits = 8 * len(st.bytes)
        st.padded = st.bytes + b"\xff" * 16
        st.nblk = base.bpm * min(ri, nmcu - k * ri)
        st.first = base.bpm * k * ri
        out.append(st)
    return out, 8 * len(stream)


# ---- the decoders ------------------------------------------------------------------------------------------------------------------------
def decode_sequential(sts):
    """Every interval in one go from its first bit -> one Sink per interval."""
    sinks = []
    for st in sts:
        sink = Sink(st.nblk)
        decode_span(st, (0, 0, 0), st.nbits, sink, 0)
        sinks.append(sink)
    return sinks


def decode_lanes(sts, chunk_bits):
    """The device's scheme, interval by interval (no subsequence straddles an interval start, and an interval's first subsequence always
    enters from the known state, so the intervals do not touch each other) -> (Sinks, rounds: the most any interval took)."""
    done = [lanes_of_one(st, chunk_bits) for st in sts]
    return [d[0] for d in done], max(d[1] for d in done)


def merge(info, sts, sinks):
    """-> (one Sink over the file whose DC differences sum, over the whole scan, to the per-interval sums; status of the entropy decode)."""
    whole = Sink(sum(st.nblk for st in sts))
    whole.coef = np.concatenate([s.coef for s in sinks])
    status = int(any(s.status(st) for s, st in zip(sinks, sts)))
    bpm = sts[0].bpm
    comp_of = np.array(sts[0].comp_of)
    for k in range(1, len(sts)):                                   # take the previous interval's final DC sums off this one's first blocks
        prev = sinks[k - 1].coef[:, 0].reshape(-1, bpm)
        for comp in range(info["c"]):
            js = np.flatnonzero(comp_of == comp)
            whole.coef[sts[k].first + js[0], 0] -= prev[:, js].sum()
    return whole, status


def decode(data, chunk_bits=None):
    """bytes of a file -> (pixels uint8, status, rounds): sequentially, or (chunk_bits) by the device's scheme."""
    info = parse(data)
    sts, _ = intervals(info, data)
    if sts is None:                                                 # the markers are wrong: nothing is decoded
        nblk = R.Stream(dict(info, seg=(info["seg"][0], 0)), data).nblk
        return pixels(info, Sink(nblk))[0], 1, 0
    sinks, rounds = (decode_sequential(sts), 0) if chunk_bits is None else decode_lanes(sts, chunk_bits)
    whole, status = merge(info, sts, sinks)
    px, damage = pixels(info, whole)
    return px, int(bool(status) or damage), rounds
