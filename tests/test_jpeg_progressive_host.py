"""The pixel-identity contract of the device decoder for progressive JPEG files (adain_jpeg_decode_progressive_u8), settled on the host:
the Python restatement of its rules (tests/jpeg_progressive_ref.py) against Pillow on progressive files Pillow writes and on three files
of other encoders with three scan scripts (tests/golden/jpeg_progressive/), end-of-band runs at their longest, the fixed-point scheme of
the parallel entropy decode simulated lane by lane against the sequential decoder, the two damaged inputs of the GPU test walked on the
CPU first, and what the parser (applied_image_processing_amd.jpeg_file) takes and refuses.  No GPU."""
import functools
import os

import numpy as np
import pytest

import jpeg_progressive_ref as P
import jpeg_ref as J
from conftest import ROOT
from test_jpeg_file_host import LAYOUTS, SHAPES, assert_same, pillow, save

import applied_image_processing_amd.jpeg_file as F

QUALITIES = [1, 75, 100]
KINDS = ["smooth", "noise"]
GOLDEN_DIR = os.path.join(ROOT, "tests", "golden", "jpeg_progressive")
# the scripts of the golden files: (components, Ss, Se, Ah, Al) per scan
GOLDEN = {
    "munch.jpg": dict(bytes=57415, geometry=(750, 594, 3, 2),
                      script=(((0, 1, 2), 0, 0, 0, 0), ((0,), 1, 5, 0, 0), ((0,), 6, 63, 0, 0), ((1,), 1, 8, 0, 0), ((1,), 9, 63, 0, 0), ((2,), 1, 8, 0, 0),
                              ((2,), 9, 63, 0, 0))),
    "cat.jpg": dict(bytes=94456, geometry=(485, 728, 3, 1),
                    script=(((0,), 0, 0, 0, 0), ((1,), 0, 0, 0, 0), ((2,), 0, 0, 0, 0), ((0,), 1, 8, 0, 1), ((0,), 9, 63, 0, 1), ((0,), 1, 63, 1, 0),
                            ((1,), 1, 5, 0, 0), ((1,), 6, 63, 0, 0), ((2,), 1, 5, 0, 0), ((2,), 6, 63, 0, 0))),
    "modern.jpg": dict(bytes=81622, geometry=(564, 564, 3, 2),
                       script=(((0, 1, 2), 0, 0, 0, 1), ((0,), 1, 5, 0, 2), ((2,), 1, 63, 0, 1), ((1,), 1, 63, 0, 1), ((0,), 6, 63, 0, 2), ((0,), 1, 63, 2, 1),
                               ((0, 1, 2), 0, 0, 1, 0), ((2,), 1, 63, 1, 0), ((1,), 1, 63, 1, 0), ((0,), 1, 63, 1, 0))),
}


def golden(name):
    with open(os.path.join(GOLDEN_DIR, name), "rb") as f:
        return f.read()


@functools.lru_cache(maxsize=None)
def files_of(h, w):
    """(name, bytes) of every progressive case of one shape: contents x layouts x qualities, and one with optimize=False."""
    out = []
    for kind in KINDS:
        for layout in LAYOUTS:
            a = J.content(kind, h, w, 1 if layout == "L" else 3)
            out += [(f"{kind} {h}x{w} layout {layout} q{q}", save(a, q, layout, progressive=True)) for q in QUALITIES]
    out.append((f"noise {h}x{w} layout 2 optimize=False", save(J.content("noise", h, w, 3), 75, 2, progressive=True, optimize=False)))
    return tuple(out)


@functools.lru_cache(maxsize=None)
def uniform_grey():
    """33 124 blocks of nothing but DC: the encoder must split the end-of-band run at 32 767."""
    return save(np.full((1456, 1456), 100, np.uint8), 75, "L", progressive=True)


@functools.lru_cache(maxsize=None)
def uniform_colour():
    return save(np.full((256, 456, 3), (90, 160, 200), np.uint8), 75, 2, progressive=True)


@functools.lru_cache(maxsize=None)
def restatement(data):
    """Computed once per file, shared by the tests (the GPU tests included) and never written to."""
    px, status, _ = P.decode(data)
    assert status == 0
    px.setflags(write=False)
    return px


def noise_48x64():
    return save(J.content("noise", 48, 64, 3), 100, 0, progressive=True)


# ---- the two damaged inputs of the GPU test --------------------------------------------------------------------------------------------------
def damaged_file():
    return save(J.content("noise", 40, 56, 3), 90, 2, progressive=True)


def damaged_short():
    """Scan 1 (the first luma band) loses the last 16 bytes of its segment: the file's bytes with them cut out."""
    data = damaged_file()
    sc = F.parse(data, progressive=True).scans[1]
    assert sc.seg_length > 32
    end = sc.seg_offset + sc.seg_length
    return data[:end - 16] + data[end:]


def damaged_swap(parsed):
    """The description ``parsed`` with the table blobs of scans 1 (luma, 1..5) and 2 (Cr, 1..63) exchanged."""
    a, b = parsed.scans[1], parsed.scans[2]
    assert a.blob != b.blob
    scans = list(parsed.scans)
    scans[1] = F.ProgressiveScan(**{**a.__dict__, "blob": b.blob})
    scans[2] = F.ProgressiveScan(**{**b.__dict__, "blob": a.blob})
    return F.ProgressiveJpegFile(**{**parsed.__dict__, "scans": tuple(scans)})


# ---- the restatement against Pillow ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("h,w", SHAPES)
def test_restatement_equals_pillow_on_pillows_progressive_files(h, w):
    for what, data in files_of(h, w):
        assert b"\xff\xc2" in data, what
        got, status, _ = P.decode(data)
        assert status == 0, what
        assert_same(got, pillow(data), what)


@pytest.mark.parametrize("name", GOLDEN)
def test_restatement_equals_pillow_on_the_golden_files(name):
    data = golden(name)
    assert_same(restatement(data), pillow(data), name)


@pytest.mark.parametrize("name", GOLDEN)
def test_the_golden_files_have_the_scripts_listed(name):
    data, want = golden(name), GOLDEN[name]
    assert len(data) == want["bytes"]
    f = F.parse(data, progressive=True)
    assert f.geometry == want["geometry"] and f.script == want["script"]
    info = P.parse(data)
    assert tuple((tuple(s["comps"]), s["ss"], s["se"], s["ah"], s["al"]) for s in info["scans"]) == want["script"]
    assert [(s.seg_offset, s.seg_length) for s in f.scans] == [s["seg"] for s in info["scans"]]


def test_a_uniform_grey_frame_splits_its_run_at_32767():
    data = uniform_grey()
    info, coef, status, _, runs = P.coefficients(data)
    assert status == 0 and coef.shape[0] == 33124 and not coef[:, 1:].any()
    assert any(32767 in r for r in runs), runs
    for sc, r in zip(info["scans"], runs):
        if sc["ss"] > 0:
            assert sum(r) == 33124, (sc["ss"], sc["se"], sc["ah"], r)
    assert_same(restatement(data), pillow(data), "uniform grey 1456 x 1456")


def test_a_uniform_colour_frame_is_one_run_per_ac_scan():
    data = uniform_colour()
    info, coef, status, _, runs = P.coefficients(data)
    assert status == 0 and not coef[:, 1:].any()
    luma, chroma = 32 * 57, 16 * 29
    for sc, r in zip(info["scans"], runs):
        assert r == ([] if sc["ss"] == 0 else [luma if sc["comps"] == [0] else chroma]), (sc["comps"], sc["ss"], sc["se"], sc["ah"], r)
    assert_same(restatement(data), pillow(data), "uniform colour 256 x 456")


# ---- the lane simulation ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["noise q100 4:4:4 48x64", "munch.jpg"])
def test_the_lanes_reach_the_sequential_decoders_coefficients(name):
    data = golden(name) if name.endswith(".jpg") else noise_48x64()
    _, want, status, _, _ = P.coefficients(data)
    assert status == 0
    for chunk_bits in (32, 64, 256, 1024):
        info, got, status, rounds, _ = P.coefficients(data, chunk_bits)
        assert status == 0 and np.array_equal(got, want), (name, chunk_bits)
        coded = sum(1 for s in info["scans"] if not (s["ss"] == 0 and s["ah"] > 0))
        assert rounds >= 2 * coded, (name, chunk_bits, rounds)          # at least 2 rounds on each Huffman-coded scan
        print(f"{name} at {chunk_bits} bits: {rounds} rounds over {coded} Huffman-coded scans")


# ---- damage, walked here before a device sees it -------------------------------------------------------------------------------------------
def test_a_shortened_scan_is_damage():
    bad = damaged_short()
    _, status, _ = P.decode(bad)
    assert status != 0
    for chunk_bits in (32, 1024):
        assert P.decode(bad, chunk_bits)[1] != 0
    assert F.parse(bad, progressive=True).script == F.parse(damaged_file(), progressive=True).script


def test_a_scan_with_another_scans_tables_is_damage():
    data = damaged_file()
    info = P.parse(data)
    a, b = info["scans"][1], info["scans"][2]
    for key in ("huff", "dc", "ac"):
        a[key], b[key] = b[key], a[key]
    # the tables travel with the scan's selectors per frame component: scan 1 now reads luma through Cr's blob and the other way round
    _, status, _ = P.decode(data, info=info)
    assert status != 0
    for chunk_bits in (32, 1024):
        assert P.decode(data, chunk_bits, info=P.parse(data) | {"scans": info["scans"]})[1] != 0
    swapped = damaged_swap(F.parse(data, progressive=True))
    assert swapped.scans[1].blob == F.parse(data, progressive=True).scans[2].blob


# ---- the parser --------------------------------------------------------------------------------------------------------------------------------
def segments(data):
    """[(marker, start, end)] of a file: every marker segment with its entropy-coded data (for SOS) up to the next marker."""
    out, at = [(0xD8, 0, 2)], 2
    while data[at + 1] != 0xD9:
        m = data[at + 1]
        end = at + 2 + int.from_bytes(data[at + 2:at + 4], "big")
        if m == 0xDA:
            while True:
                end = data.index(b"\xff", end)
                if data[end + 1] != 0:
                    break
                end += 2
        out.append((m, at, end))
        at = end
    return out + [(0xD9, at, at + 2)]


def test_the_parser_takes_progressive_files_only_with_the_keyword():
    datas = [d for h, w in ((17, 33), (48, 64)) for _, d in files_of(h, w)] + [golden(n) for n in GOLDEN] + [uniform_grey(), uniform_colour()]
    for data in datas:
        with pytest.raises(F.UnsupportedJpeg, match=r"^progressive \(SOF2\)$"):
            F.parse(data)
        with pytest.raises(F.UnsupportedJpeg, match=r"^progressive \(SOF2\)$"):
            F.parse(data, restart=True)
        f = F.parse(data, progressive=True)
        assert isinstance(f, F.ProgressiveJpegFile) and 1 <= len(f.scans) <= F.MAX_SCANS == 32
        assert all(len(sc.blob) == F.BLOB_BYTES for sc in f.scans) and f.script == tuple(sc.key for sc in f.scans)
        assert f.geometry[:2] == pillow(data).shape[:2]
        assert data[f.scans[-1].seg_offset + f.scans[-1].seg_length:] == b"\xff\xd9"


def test_the_tables_in_force_travel_with_each_scan():
    """Pillow optimises the tables of every scan and redefines them between scans: the blobs of two AC scans of one component differ."""
    f = F.parse(noise_48x64(), progressive=True)
    luma = [sc.blob for sc in f.scans if sc.comps == (0,) and sc.ss > 0]
    assert len(luma) >= 3 and len(set(luma)) > 1


def test_the_parser_refuses_a_progressive_file_with_restart_intervals():
    data = save(J.content("noise", 33, 17, 3), 75, 2, progressive=True, restart_marker_blocks=1)
    assert b"\xff\xdd" in data
    with pytest.raises(F.UnsupportedJpeg, match="a progressive file with a restart interval"):
        F.parse(data, progressive=True)
    with pytest.raises(F.UnsupportedJpeg, match="a progressive file with a restart interval"):
        F.parse(data, restart=True, progressive=True)
    with pytest.raises(P.Refused):
        P.parse(data)


def test_the_parser_refuses_broken_scripts():
    data = save(J.content("noise", 33, 17, 3), 75, 2, progressive=True)
    segs = segments(data)
    scans = [s for s in segs if s[0] == 0xDA]
    assert len(scans) == 10
    # the last scan deleted: the luma band never reaches full precision
    cut = data[:scans[-1][1]] + b"\xff\xd9"
    with pytest.raises(F.UnsupportedJpeg, match="incomplete"):
        F.parse(cut, progressive=True)
    with pytest.raises(P.Refused):
        P.parse(cut)
    # a refinement's Ah patched: scan 5 refines luma 1..63 from Al 2 to 1
    _, at, _ = scans[5]
    ln = int.from_bytes(data[at + 2:at + 4], "big")
    assert data[at + 1 + ln] == 0x21
    patched = data[:at + 1 + ln] + b"\x31" + data[at + 2 + ln:]
    with pytest.raises(F.UnsupportedJpeg, match="a refinement with Ah = 3"):
        F.parse(patched, progressive=True)
    with pytest.raises(P.Refused):
        P.parse(patched)
    # a DQT behind the first scan, moved or repeated
    dqt = [s for s in segs if s[0] == 0xDB]
    assert dqt and dqt[-1][2] <= scans[0][1]
    tables = b"".join(data[a:b] for _, a, b in dqt)
    moved = data[:dqt[0][1]] + data[dqt[-1][2]:scans[0][2]] + tables + data[scans[0][2]:]
    repeated = data[:scans[0][2]] + tables + data[scans[0][2]:]
    with pytest.raises(F.UnsupportedJpeg):
        F.parse(moved, progressive=True)
    with pytest.raises(F.UnsupportedJpeg, match="FFDB behind the first scan"):
        F.parse(repeated, progressive=True)
    with pytest.raises(P.Refused):
        P.parse(repeated)


def test_the_parser_refuses_33_scans():
    """A grey 8 x 8 constant block: every AC scan is one EOB, so the first one's bytes serve any band - 32 bands after the DC scan."""
    data = save(np.full((8, 8), 100, np.uint8), 75, "L", progressive=True)
    segs = segments(data)
    first_ac = next(i for i, s in enumerate(segs) if s[0] == 0xDA and data[s[1] + 7] > 0)
    head = data[:segs[first_ac][1]]
    _, a, b = segs[first_ac]
    assert data[a + 4] == 1 and data[a + 7:a + 10] == b"\x01\x05\x02"            # one component; Ss 1, Se 5, Ah 0 Al 2

    def band(k):
        return data[a:a + 7] + bytes([k, k, 0]) + data[a + 10:b]

    ok = head + b"".join(band(k) for k in range(1, 32)) + b"\xff\xd9"          # 32 scans, then incomplete: the count is not the reason
    with pytest.raises(F.UnsupportedJpeg, match="incomplete"):
        F.parse(ok, progressive=True)
    many = head + b"".join(band(k) for k in range(1, 33)) + b"\xff\xd9"
    with pytest.raises(F.UnsupportedJpeg, match="more than 32 scans"):
        F.parse(many, progressive=True)
    with pytest.raises(P.Refused):
        P.parse(many)


def test_baseline_files_parse_the_same_with_the_keyword():
    for layout in LAYOUTS:
        a = J.content("smooth", 33, 17, 1 if layout == "L" else 3)
        for kw, restart in ((dict(), False), (dict(optimize=True), False), (dict(restart_marker_blocks=2), True)):
            data = save(a, 75, layout, **kw)
            off, on = F.parse(data, restart=restart), F.parse(data, restart=restart, progressive=True)
            assert isinstance(on, F.JpegFile) and off.__dict__.keys() == on.__dict__.keys()
            for key, v in off.__dict__.items():
                assert np.array_equal(v, on.__dict__[key]) if isinstance(v, np.ndarray) else v == on.__dict__[key], key
