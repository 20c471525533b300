"""The PNG decoder's restatement (tests/png_decode_ref.py) held to zlib and Pillow on the files of tests/png_decode_cases.py; what every
designed file was designed for, shown by the trace; the statuses of the damaged files with Pillow's outcome beside them; what
``png_file.parse`` takes and refuses; and the ``PngRoute`` / ``OutputRoutes`` additions.  No GPU.  Every check is an equality."""
import io
import struct
import zlib

import numpy as np
import pytest
from PIL import Image

import applied_image_processing_amd.png_file as png_file
import applied_image_processing_amd.runtime as rt
import png_decode_cases as C
import png_decode_ref as R


@pytest.fixture(scope="module")
def decoded():
    """Per sound case (parsed file, restatement's pixels, status, trace), computed once."""
    out = {}
    for c in C.sound():
        p = png_file.parse(c.data)
        out[c.name] = (p,) + R.decode(p.stream, p.h, p.w, p.c)
    return out


def case_of(name):
    return next(c for c in C.sound() if c.name == name)


@pytest.mark.parametrize("name", [c.name for c in C.sound()])
def test_the_restatement_is_zlib_and_pillow_on_every_sound_file(decoded, name):
    case = case_of(name)
    p, px, status, trace = decoded[name]
    assert (p.h, p.w, p.c, png_file.CHANNELS[p.colour_type]) == (case.h, case.w, case.c, case.c)
    assert status == 0
    filtered, st, _ = R.inflate(p.stream, p.h * (p.w * p.c + 1)) if case.h * case.w < 70000 else (zlib.decompress(p.stream), 0, None)
    assert st == 0 and filtered == zlib.decompress(p.stream)
    img = Image.open(io.BytesIO(case.data))
    pil = np.asarray(img)
    assert np.array_equal(px.reshape(pil.shape), pil)
    if case.pixels is not None:
        assert np.array_equal(px, case.pixels)
    three = R.decode(p.stream, p.h, p.w, p.c, 3)[0] if case.h * case.w < 70000 else (np.repeat(px, 3, 2) if p.c == 1 else px[:, :, :3])
    assert np.array_equal(three, np.asarray(img.convert("RGB")))         # grey replicated, alpha dropped


def test_each_designed_file_holds_what_it_was_designed_for(decoded):
    tr = {name: d[3] for name, d in decoded.items()}
    assert tr["zlib_stored"].blocks == [0] and tr["zlib_stored_two"].blocks == [0, 0] and sum(tr["zlib_stored_two"].stored) == 150 * 451 > 65535
    assert tr["zlib_fixed"].blocks == [1] and tr["zlib_default"].blocks == [2] and tr["zlib_level9"].blocks == [2] and tr["zlib_wbits9"].blocks == [2]
    assert tr["zlib_huffman_only"].blocks == [2] and all(len(t) == 1 for t in tr["zlib_huffman_only"].tokens)
    rle = [t for t in tr["zlib_rle"].tokens if len(t) == 2]
    assert rle and all(d == 1 for _, d in rle) and max(n for n, _ in rle) == 258          # copies that overlap their own output
    assert tr["zlib_sync_flush"].blocks == [2, 0, 2] and tr["zlib_sync_flush"].stored == [0]
    assert decoded["zlib_wbits9"][0].stream[:2] == b"\x18\x95"
    assert (258, 32768) in tr["window_32768"].tokens and max(t[1] for t in tr["window_32768"].tokens if len(t) == 2) == 32768
    assert max(tr["hand_15bit"].code_lengths[0][0]) == 15
    for name, sym in (("hand_repeat16", 16), ("hand_repeat17", 17), ("hand_repeat18", 18)):
        assert any(s == sym and before < hlit < before + count for s, before, count, hlit in tr[name].repeats), name
    assert tr["hand_one_distance"].code_lengths[0][1] == [1] and tr["hand_one_distance"].dist_symbols == {0}
    assert {281, 284, 285} <= tr["hand_far"].length_symbols and 29 in tr["hand_far"].dist_symbols
    assert (162, 8192) in tr["hand_far"].tokens and (257, 30000) in tr["hand_far"].tokens          # 5 extra bits at 31 and 30, 13 extra bits
    assert tr["hand_blocks"].blocks == [2, 2, 2]
    # the filters: every one forced, the first row included; all five in one file; 9-bit sums; every tie of Paeth
    for ft in range(5):
        p = decoded[f"filter_{ft}"][0]
        assert set(zlib.decompress(p.stream)[::p.w * p.c + 1]) == {ft}
    p = decoded["filter_mixed_rgba"][0]
    assert set(zlib.decompress(p.stream)[::p.w * p.c + 1]) == {0, 1, 2, 3, 4}
    px = decoded["filter_average_noise"][1][:, :, 0].astype(int)
    assert (px[1:, :-1] + px[:-1, 1:]).max() > 255
    t = C.paeth_ties()[:, :, 0].astype(int)
    ties = set()
    for x in (1, 3, 5):
        a, b, c = t[1, x - 1], t[0, x], t[0, x - 1]
        pa, pb, pc = abs(b - c), abs(a - c), abs(a + b - 2 * c)
        ties.add("ab" if pa == pb < pc else "ac" if pa == pc < pb else "bc" if pb == pc < pa else "")
    assert ties == {"ab", "ac", "bc"}
    # heights around the unfilter's band, row bytes off the 4-byte grid
    assert {c.h for c in C.sound() if c.name.startswith("height_")} == {R.BAND - 1, R.BAND, R.BAND + 1, 2 * R.BAND + 1}
    assert {c.w * c.c for c in C.sound() if c.name.startswith("rowbytes_")} == {1, 3, 5, 7}
    # the IDAT splits and the fixtures
    kinds = lambda data: [data[at + 4:at + 8] for at in chunk_starts(data)]
    assert kinds(case_of("idat_1_rest").data).count(b"IDAT") == 2 and len(chunk_body(case_of("idat_1_rest").data, 1)) == 1
    every = case_of("idat_every_byte").data
    assert kinds(every).count(b"IDAT") == len(decoded["idat_every_byte"][0].stream) > 100
    assert any(len(chunk_body(case_of("idat_empty_between").data, k)) == 0 for k in (1, 2))
    assert kinds(case_of("idat_ancillary").data)[1:3] == [b"tEXt", b"pHYs"] and kinds(case_of("idat_ancillary").data)[-2] == b"tIME"
    view, conv = case_of("fixture_view_800.png"), case_of("fixture_conv_1.png")
    assert (view.h, view.w, view.c) == (800, 800, 3) and kinds(view.data).count(b"IDAT") == 21 and kinds(view.data).count(b"tEXt") == 7 and b"pHYs" in kinds(view.data)
    assert (conv.h, conv.w, conv.c) == (642, 673, 4) and {b"sRGB", b"gAMA"} <= set(kinds(conv.data))


def chunk_starts(data):
    at = 8
    while at < len(data):
        yield at
        at += 12 + int.from_bytes(data[at:at + 4], "big")


def chunk_body(data, k):
    at = list(chunk_starts(data))[k]
    return data[at + 8:at + 8 + int.from_bytes(data[at:at + 4], "big")]


PILLOW_ON_DAMAGED = {}          # name -> "pixels" or the exception's name: recorded beside the status, not asserted on


@pytest.mark.parametrize("name", [c.name for c in C.damaged()])
def test_the_restatement_gives_every_damaged_file_its_status(name):
    case = next(c for c in C.damaged() if c.name == name)
    p = png_file.parse(case.data)                   # the parser takes them all: the damage is the device's to find
    px, status, _ = R.decode(p.stream, p.h, p.w, p.c)
    assert px is None and status == case.status != 0, f"{name}: {R.STATUS_NAMES[status]}, expected {R.STATUS_NAMES[case.status]}"
    try:
        np.asarray(Image.open(io.BytesIO(case.data)))
        PILLOW_ON_DAMAGED[name] = "pixels"
    except Exception as e:          # noqa: BLE001 - whatever Pillow raises is what the caller would see
        PILLOW_ON_DAMAGED[name] = type(e).__name__
    print(f"{name}: {R.STATUS_NAMES[status]}; Pillow: {PILLOW_ON_DAMAGED[name]}")


def test_every_status_has_a_damaged_file():
    assert {c.status for c in C.damaged()} == set(range(1, 17))
    cuts = [c.name for c in C.damaged() if c.status == R.TRUNCATED]
    assert cuts == ["cut_at_zlib_header", "cut_in_dynamic_header", "cut_in_stored", "cut_before_adler_end"]
    bad = next(c for c in C.damaged() if c.name == "adler")
    with pytest.raises(OSError):                    # Pillow refuses a wrong Adler-32 ...
        np.asarray(Image.open(io.BytesIO(bad.data)))
    good = bytearray(C.file_of(C.gradient(2, 4, 1, 60), [1, 2]))
    good[-13] ^= 1                                  # ... and does not look at IDAT's CRC
    assert np.array_equal(np.asarray(Image.open(io.BytesIO(bytes(good)))), C.gradient(2, 4, 1, 60)[:, :, 0])
    assert png_file.parse(bytes(good)).stream == png_file.parse(C.file_of(C.gradient(2, 4, 1, 60), [1, 2])).stream


# ---- png_file.parse ---------------------------------------------------------------------------------------------------------------------
def saved(img, **kw):
    f = io.BytesIO()
    img.save(f, format="PNG", **kw)
    return f.getvalue()


def test_parse_takes_what_the_decoder_takes():
    rng = np.random.default_rng(0)
    for mode, c, colour in (("L", 1, 0), ("RGB", 3, 2), ("RGBA", 4, 6)):
        arr = rng.integers(0, 256, (5, 7) + ((c,) if c > 1 else ()), dtype=np.uint8)
        img = Image.fromarray(arr)
        assert img.mode == mode
        p = png_file.parse(saved(img))
        assert (p.h, p.w, p.colour_type, p.c, p.geometry) == (5, 7, colour, c, (5, 7, colour))
        assert np.array_equal(R.decode(p.stream, 5, 7, c)[0].reshape(arr.shape), arr)
    px = C.gradient(2, 4, 1, 60)
    stream = C.deflate(R.filter_rows(px, [1, 2]))
    for pieces in ([stream[:1], stream[1:]], [b"", stream[:1], b"", stream[1:2], stream[2:], b""], [bytes([b]) for b in stream]):
        assert png_file.parse(R.png_file(2, 4, 0, pieces)).stream == stream           # split anywhere, inside the zlib header too
    anc = ((b"gAMA", bytes(4)), (b"tEXt", b"a\0b"), (b"zzZz", b"private"))
    assert png_file.parse(R.png_file(2, 4, 0, stream, anc, anc)).stream == stream
    assert png_file.parse(bytearray(R.png_file(2, 4, 0, stream))).stream == stream


def test_parse_refuses_the_rest_and_says_why():
    rng = np.random.default_rng(1)
    grey = rng.integers(0, 256, (6, 6), dtype=np.uint8)
    px = C.gradient(2, 4, 1, 60)
    stream = C.deflate(R.filter_rows(px, [1, 2]))
    good = R.png_file(2, 4, 0, stream)
    with_dict = zlib.compressobj(zdict=b"abc")
    fdict = with_dict.compress(R.filter_rows(px, [1, 2])) + with_dict.flush()
    assert fdict[1] & 0x20
    refused = {
        "a palette": saved(Image.fromarray(grey).convert("P")),
        "grey with alpha": saved(Image.fromarray(grey).convert("LA")),
        "16-bit": saved(Image.fromarray(grey.astype(np.uint16) * 257)),
        "1-bit": saved(Image.fromarray(grey > 128)),
        "interlaced": R.png_file(2, 4, 0, stream, interlace=1),
        "2-bit": R.png_file(2, 4, 0, stream, depth=2),
        "4-bit": R.png_file(2, 4, 0, stream, depth=4),
        "tRNS": R.png_file(2, 4, 0, stream, before=((b"tRNS", bytes(2)),)),
        "acTL": R.png_file(2, 4, 0, stream, before=((b"acTL", bytes(8)),)),
        "not consecutive": R.png_file(2, 4, 0, stream[:5], after=((b"tEXt", b"a\0b"), (b"IDAT", stream[5:]))),
        "no IEND": good[:-12],
        "chunk passes the end": good[:-14],
        "length passes the end": good[:33] + struct.pack(">I", 1 << 20) + good[37:],
        "no IDAT": R.png_file(2, 4, 0, []),
        "FDICT": R.png_file(2, 4, 0, fdict),
        "FCHECK": R.png_file(2, 4, 0, stream[:1] + bytes([stream[1] ^ 1]) + stream[2:]),
        "CM": R.png_file(2, 4, 0, b"\x77" + stream[1:]),
        "CINFO": R.png_file(2, 4, 0, b"\x88\x1c" + stream[2:]),
        "one stream byte": R.png_file(2, 4, 0, stream[:1]),
        "no signature": b"\x89PNX" + good[4:],
        "IHDR second": good[:8] + R.chunk(b"tEXt", b"a\0b") + good[8:],
        "colour type 5": R.png_file(2, 4, 5, stream),
        "critical chunk": R.png_file(2, 4, 0, stream, before=((b"PLTE", bytes(3)),)),
        "2^31": R.png_file(1 << 16, 1 << 15, 0, stream),
        "empty": b"",
    }
    assert saved(Image.fromarray(grey > 128))[24] == 1 and saved(Image.fromarray(grey.astype(np.uint16) * 257))[24] == 16
    for why, data in refused.items():
        with pytest.raises(png_file.UnsupportedPng) as e:
            png_file.parse(data)
        assert str(e.value), why
    assert (1 << 16) * ((1 << 15) + 1) >= 1 << 31 and png_file.parse(R.png_file((1 << 16) - 2, 1 << 15, 0, stream)).h == 65534


# ---- the routes -------------------------------------------------------------------------------------------------------------------------
def test_png_route_gains_decode_on_device_behind_filter():
    assert rt.PngRoute.__slots__ == ("encode_on_device", "filter", "decode_on_device")
    d = rt.PngRoute()
    assert (d.encode_on_device, d.filter, d.decode_on_device) == (False, None, False)
    assert repr(d) == "PngRoute(encode_on_device=False, filter=None)" and repr(rt.PngRoute(True, 2)) == "PngRoute(encode_on_device=True, filter=2)"
    assert rt.PngRoute(True, 2) == rt.PngRoute(encode_on_device=True, filter=2, decode_on_device=False)
    on = rt.PngRoute(False, None, True)
    assert on.decode_on_device is True and repr(on) == "PngRoute(encode_on_device=False, filter=None, decode_on_device=True)"
    assert on != d and hash(on) != hash(d) and on == rt.PngRoute(decode_on_device=1)
    assert d.replace(decode_on_device=True) == on and on.replace(decode_on_device=False) == d and on.replace(filter=3) == rt.PngRoute(False, 3, True)
    assert rt.PngRoute.of({"decode_on_device": True}) == on and rt.PngRoute.of(None) == d and rt.PngRoute.of(on) is on
    assert rt.OutputRoutes.of({"png": {"decode_on_device": True}}).png == on
    assert repr(rt.OutputRoutes(png=on)).endswith("png=PngRoute(encode_on_device=False, filter=None, decode_on_device=True))")
    with pytest.raises(AttributeError):
        on.decode_on_device = False


def test_read_rgb_asks_the_route_that_owns_the_extension(monkeypatch):
    asked = []
    monkeypatch.setattr(rt, "png_decode_rgb_file", lambda path, device: asked.append(("png", str(path))) or "png frame")
    monkeypatch.setattr(rt, "jpeg_decode_rgb_file", lambda path, device, progressive=False: asked.append(("jpeg", str(path), progressive)) or "jpeg frame")
    off, on = rt.OutputRoutes(), rt.OutputRoutes(rt.JpegRoutes(False, True, True), rt.PngRoute(False, None, True))
    for path in ("a.png", "a.PNG", "a.jpg", "a.jpeg", "a.bmp"):
        assert off.read_rgb(path, "cuda:0") is None
    assert asked == []
    assert on.read_rgb("a.png", "cuda:0") == "png frame" and on.read_rgb("b.PNG", "cuda:0") == "png frame"
    assert on.read_rgb("a.jpg", "cuda:0") == "jpeg frame" and on.read_rgb("a.bmp", "cuda:0") == "jpeg frame"
    assert asked == [("png", "a.png"), ("png", "b.PNG"), ("jpeg", "a.jpg", True), ("jpeg", "a.bmp", True)]
    assert on.png.read_rgb("a.png", "cuda:0") == "png frame" and rt.PngRoute().read_rgb("a.png", "cuda:0") is None
    only_png = rt.OutputRoutes(png=rt.PngRoute(decode_on_device=True))
    assert only_png.read_rgb("a.jpg", "cuda:0") is None and only_png.read_rgb("a.png", "cuda:0") == "png frame"


def test_png_decode_rgb_file_leaves_other_files_and_devices_to_the_caller(tmp_path):
    path = tmp_path / "a.png"
    path.write_bytes(C.file_of(C.gradient(2, 4, 3, 1), [1, 2]))
    assert rt.png_decode_rgb_file(path, "cpu") is None
    assert rt.png_decode_rgb_file(tmp_path / "a.jpg", "cuda:0") is None          # not read at all: the file does not exist
    with pytest.raises(rt.AdainHipError, match="mode"):
        rt.png_decode_u8(b"", device="cpu", mode="RGBA")


def test_the_callers_take_the_switch():
    import inspect

    from applied_image_processing_amd import jobs, video
    from applied_image_processing_amd.AdaIN import run_depth
    from applied_image_processing_amd.AdaIN import test as t

    for fn in (video.apply_style_transfer_ada, video.apply_style_transfer_multi_ada, jobs.precompute_guides_sharded):
        assert inspect.signature(fn).parameters["png_decode_on_device"].default is False
    assert dict(run_depth._EXTRA_FLAGS)["--png_decode_on_device"]["action"] == "store_true"
    before = t.output_routes()
    try:
        assert t.set_device_png_decode(True) is False and t.output_routes() == before.replace(png=before.png.replace(decode_on_device=True))
        assert t.set_device_png_decode(False) is True and t.output_routes() == before
    finally:
        t.set_output_routes(before)
