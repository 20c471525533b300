"""Restart intervals in the device JPEG file decoder (adain_jpeg_decode_restart_u8), settled on the host: the Python restatement of the
restart rules (tests/jpeg_restart_ref.py, on top of tests/jpeg_file_ref.py) against Pillow on files Pillow writes with restart markers
and on one file another encoder wrote (tests/golden/jpeg_restart/), the per-interval lane scheme simulated against the sequential
decoder, the rounds it may take, and what ``jpeg_file.parse(data, restart=True)`` takes and refuses.  Exact equality throughout.  No GPU."""
import functools
import io
import os

import numpy as np
import pytest
from PIL import Image

import jpeg_file_ref as R
import jpeg_ref as J
import jpeg_restart_ref as RR
from conftest import ROOT
from test_jpeg_file_host import LAYOUTS, SHAPES, assert_same, pillow, save

import applied_image_processing_amd.jpeg_file as F

GOLDEN_RESTART = os.path.join(ROOT, "tests", "golden", "jpeg_restart", "the_resevoir_at_poitiers.jpg")
# Pillow's keywords: restart_marker_blocks = Ri in MCUs, restart_marker_rows = Ri in MCU rows
SETTINGS = [("blocks 1", dict(restart_marker_blocks=1), 75), ("blocks 3", dict(restart_marker_blocks=3), 75), ("rows 1", dict(restart_marker_rows=1), 75),
            ("blocks 9 optimize", dict(restart_marker_blocks=9, optimize=True), 75), ("rows 1 q100", dict(restart_marker_rows=1), 100)]


def mcus(h, w, layout):
    hh, vv = {0: (1, 1), 1: (2, 1), 2: (2, 2), "L": (1, 1)}[layout]
    return -(-w // (8 * hh)), -(-h // (8 * vv))


@functools.lru_cache(maxsize=None)
def restart_files(h, w):
    """(name, bytes, layout, Ri) of every case of one shape: contents x layouts x restart settings."""
    out = []
    for kind in J.CONTENTS:
        for layout in LAYOUTS:
            a = J.content(kind, h, w, 1 if layout == "L" else 3)
            mw, _ = mcus(h, w, layout)
            for name, kw, q in SETTINGS:
                ri = kw.get("restart_marker_blocks") or kw["restart_marker_rows"] * mw
                out.append((f"{kind} {h}x{w} layout {layout} {name}", save(a, q, layout, **kw), layout, ri))
    return tuple(out)


def markers_in(data):
    """The RSTn markers of the scan, by the plainest reading: FF D0..D7 behind SOS."""
    scan = data[data.index(b"\xff\xda"):]
    return sum(scan.count(bytes([0xFF, 0xD0 + k])) for k in range(8))


@pytest.mark.parametrize("h,w", SHAPES)
def test_restatement_equals_pillow_on_pillows_restart_files(h, w):
    """Every content, layout and restart setting: the restatement's pixels are Pillow's, status 0, and the parser describes the file."""
    for what, data, layout, ri in restart_files(h, w):
        got, status, _ = RR.decode(data)
        assert status == 0, what
        assert_same(got, pillow(data), what)
        f = F.parse(data, restart=True)
        assert f.restart_interval == ri, what
        assert f.geometry == (h, w, 1 if layout == "L" else 3, 0 if layout == "L" else layout), what
        assert data[f.seg_offset + f.seg_length:] == b"\xff\xd9", what
        info = RR.parse(data)
        mw, mh = mcus(h, w, layout)
        assert (f.seg_offset, f.seg_length) == info["seg"] and info["ri"] == ri and markers_in(data) == -(-mw * mh // ri) - 1, what
        with pytest.raises(F.UnsupportedJpeg, match="restart interval"):
            F.parse(data)


def test_the_cases_hold_files_with_a_dri_and_no_marker():
    one = [c for c in restart_files(1, 1)]
    assert one and all(b"\xff\xdd" in d and markers_in(d) == 0 for _, d, _, _ in one)
    six = [(d, layout, ri) for _, d, layout, ri in restart_files(17, 33) if ri == 9 and mcus(17, 33, layout) == (3, 2)]
    assert six and all(b"\xff\xdd" in d and markers_in(d) == 0 and F.parse(d, restart=True).restart_interval == 9 for d, _, _ in six)
    assert any(markers_in(d) > 8 for _, d, _, _ in restart_files(48, 64)), "the marker numbers should wrap past D7 somewhere"
    # blocks 3: intervals that straddle MCU rows and a short last one
    assert any(ri == 3 and mw > 1 and mw % 3 and mw * mh > 3 and (mw * mh) % 3 for h, w in SHAPES for _, _, layout, ri in restart_files(h, w)
               for mw, mh in [mcus(h, w, layout)])


def test_the_golden_restart_file():
    data = open(GOLDEN_RESTART, "rb").read()
    assert os.path.getsize(GOLDEN_RESTART) < (1 << 20)
    got, status, _ = RR.decode(data)
    assert status == 0
    assert_same(got, pillow(data), "the_resevoir_at_poitiers.jpg")
    f = F.parse(data, restart=True)
    assert f.restart_interval == 100 and f.geometry == (662, 800, 3, 0)
    with pytest.raises(F.UnsupportedJpeg, match="restart interval"):
        F.parse(data)


def test_files_without_a_restart_interval_parse_the_same_either_way():
    data = save(J.content("smooth", 33, 17, 3))
    a, b = F.parse(data, restart=True), F.parse(data)
    assert (a.geometry, a.restart_interval, a.seg_offset, a.seg_length, a.blob) == (b.geometry, 0, b.seg_offset, b.seg_length, b.blob)
    got, status, _ = RR.decode(data)
    assert status == 0
    assert_same(got, R.decode(data)[0], "Ri = 0")


LANE_FILES = {
    "noise 48x64 q100 4:4:4 rows 1": lambda: save(J.content("noise", 48, 64, 3), 100, 0, restart_marker_rows=1),           # intervals of about 16.5 kbit
    "smooth 64x64 4:2:0 blocks 5": lambda: save(J.content("smooth", 64, 64, 3), 75, 2, restart_marker_blocks=5),
    "constant white 64x64 4:2:0 rows 2": lambda: save(J.content("white", 64, 64, 3), 75, 2, restart_marker_rows=2),
    "constant grey 64x64 optimize blocks 7": lambda: save(J.content("white", 64, 64, 1), 75, "L", optimize=True, restart_marker_blocks=7),   # intervals of 16-24 bits
}


@pytest.mark.parametrize("name", LANE_FILES)
@pytest.mark.parametrize("chunk_bits", [32, 64, 1024])
def test_lane_scheme_per_interval_reaches_the_sequential_decoder(name, chunk_bits):
    """The device's scheme simulated per interval: the coefficients, the status and the pixels of the sequential decoder, whatever the
    chunk size.  The rounds are derived, not measured: interval k settles within ceil(bits_k / chunk_bits) + 1 rounds (its first
    subsequence is right from round 0, each round makes one more right, one more round sees no change), the file takes the most any
    interval does, and where every interval fits in one chunk that is round 0 and the one round that changes nothing."""
    data = LANE_FILES[name]()
    info = RR.parse(data)
    sts, _ = RR.intervals(info, data)
    assert sts is not None and len(sts) > 1
    want, want_status = RR.merge(info, sts, RR.decode_sequential(sts))
    sinks, rounds = RR.decode_lanes(sts, chunk_bits)
    got, got_status = RR.merge(info, sts, sinks)
    bits = [st.nbits for st in sts]
    print(f"{name}: {len(sts)} intervals of {min(bits)}..{max(bits)} bits, chunks of {chunk_bits}, {rounds} rounds")
    assert np.array_equal(got.coef, want.coef) and got_status == want_status == 0
    assert 2 <= rounds <= max(-(-b // chunk_bits) for b in bits) + 1
    if all(b <= chunk_bits for b in bits):
        assert rounds == 2
    assert_same(RR.pixels(info, got)[0], pillow(data), name)
    assert RR.decode(data, chunk_bits)[1:] == (0, rounds)


def test_the_lane_files_are_what_they_are_meant_to_be():
    bits = {}
    for name, make in LANE_FILES.items():
        data = make()
        bits[name] = [st.nbits for st in RR.intervals(RR.parse(data), data)[0]]
    assert all(15000 < b < 18000 for b in bits["noise 48x64 q100 4:4:4 rows 1"])
    assert all(16 <= b <= 24 for b in bits["constant grey 64x64 optimize blocks 7"]), bits["constant grey 64x64 optimize blocks 7"]
    assert len(bits["smooth 64x64 4:2:0 blocks 5"]) == 4 and len(bits["constant white 64x64 4:2:0 rows 2"]) == 2


# ---- more intervals than a per-file workgroup has threads ------------------------------------------------------------------------------
MANY_KINDS = ["smooth", "noise"]


@functools.lru_cache(maxsize=None)
def many_intervals_file(kind):
    """A grey 264 x 264 frame, 33 x 33 = 1089 MCUs, one MCU per restart interval: more intervals than the 1024 threads of the device's
    per-file workgroups, so its scans over the interval table and over the subsequences' block counts take a second pass and carry."""
    return save(J.content(kind, 264, 264, 1), 75, "L", restart_marker_blocks=1)


@pytest.mark.parametrize("kind", MANY_KINDS)
def test_more_intervals_than_threads(kind):
    """The restatement is Pillow, sequentially and by the device's scheme at chunks of 32 and 1024 bits."""
    data = many_intervals_file(kind)
    f = F.parse(data, restart=True)
    assert f.restart_interval == 1 and f.geometry == (264, 264, 1, 0) and markers_in(data) == 1088
    want = pillow(data)
    for chunk_bits in (None, 32, 1024):
        got, status, _ = RR.decode(data, chunk_bits)
        assert status == 0, chunk_bits
        assert_same(got, want, f"{kind}, chunks of {chunk_bits}")


# ---- what the parser refuses with restart=True ----------------------------------------------------------------------------------------
def _with_markers():
    data = save(J.content("noise", 33, 17, 3), 90, 0, restart_marker_blocks=2)
    f = F.parse(data, restart=True)
    assert markers_in(data) == 7 and f.restart_interval == 2
    return data, data.index(b"\xff\xd2", f.seg_offset)


def renumbered():
    data, at = _with_markers()
    return data[:at] + b"\xff\xd5" + data[at + 2:]


def removed():
    data, _ = _with_markers()
    at = data.rindex(b"\xff\xd6")               # the last one: the others stay in order
    return data[:at] + data[at + 2:]


def fill_byte():
    data, at = _with_markers()
    first = data.index(b"\xff\xd0", F.parse(data, restart=True).seg_offset)
    return data[:first] + b"\xff" + data[first:]


def progressive_with_dri():
    buf = io.BytesIO()
    Image.fromarray(J.content("smooth", 33, 17, 3)).save(buf, format="JPEG", progressive=True, restart_marker_blocks=2)
    assert b"\xff\xdd" in buf.getvalue()
    return buf.getvalue()


@pytest.mark.parametrize("make,why", [(renumbered, "restart marker 2 is FFD5"), (removed, "6 restart markers where"), (fill_byte, "fill byte"),
                                      (progressive_with_dri, "progressive")], ids=["renumbered", "removed", "fill", "progressive"])
def test_parser_refuses_with_restart(make, why):
    data = make()
    with pytest.raises(F.UnsupportedJpeg, match=why):
        F.parse(data, restart=True)


def test_the_restatement_marks_wrong_markers():
    """A marker renumbered or removed: a non-zero status, as the device gives (the entropy decode is skipped)."""
    for data in (renumbered(), removed()):
        assert RR.decode(data)[1] != 0
