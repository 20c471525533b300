"""Restart intervals in the device JPEG file decoder (csrc/jpeg_decode.hip, adain_jpeg_decode_restart_u8) and its callers.  Element-for-element
equality everywhere: the device's pixels against Pillow's for the same bytes and against the Python restatement
(tests/jpeg_restart_ref.py), with no file allowed to fall back to the host.  Then markers on the unstuff stage's piece and thread
boundaries, the chunk size and the rounds, batches, the memory contract through the guard-band arena (tests/abi_arena.py) with stale
workspaces of another restart interval and of none, refusals, the Ri = 0 path against the old entry, damaged marker structure, and the
callers that now keep restart files on the device."""
import ctypes
import functools
import io
import re

import numpy as np
import pytest
import torch
from PIL import Image

import abi_arena as A
import jpeg_ref as J
import jpeg_restart_ref as RR
from test_gpu_jpeg_decode import Counter, first_difference, pil_outcome, u8img
from test_jpeg_file_host import LAYOUTS, SHAPES, pillow, save
from test_jpeg_restart_host import GOLDEN_RESTART, LANE_FILES, MANY_KINDS, many_intervals_file, markers_in, restart_files

import applied_image_processing_amd.jpeg_file as F
import applied_image_processing_amd.synth as synth

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
_arena_passed = set()


@pytest.fixture(scope="module")
def rt():
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    import applied_image_processing_amd.runtime as rt

    rt.lib()
    torch.cuda.set_device(0)
    return rt


@functools.lru_cache(maxsize=None)
def restatement(data):
    """Computed once per file, shared by the tests and never written to."""
    px, status, _ = RR.decode(data)
    assert status == 0
    px.setflags(write=False)
    return px


def device_pixels(rt, datas, **kw):
    """The frames of the files as numpy arrays, every one decoded ON THE DEVICE (a fallback to PIL fails the test), and the rounds."""
    report = []
    out = rt.jpeg_decode_u8(list(datas), DEV, report=report, restart=True, **kw)
    assert [r["path"] for r in report] == ["device"] * len(datas), report
    assert all(o.is_cuda and o.dtype == torch.uint8 for o in out)
    return [o.cpu().numpy() for o in out], [r["rounds"] for r in report]


@pytest.mark.parametrize("h,w", SHAPES)
def test_device_pixels_are_pillows_and_the_restatements(rt, h, w):
    """Every host case of the shape in ONE call (it goes out grouped by layout and restart interval): none left to the host."""
    names, datas = zip(*[(name, data) for name, data, _, _ in restart_files(h, w)])
    got, _ = device_pixels(rt, datas)
    for name, data, g in zip(names, datas, got):
        bad = first_difference(g, pillow(data))
        assert bad is None, f"{name} against Pillow: {bad}"
        bad = first_difference(g, restatement(data))
        assert bad is None, f"{name} against the restatement: {bad}"


def test_the_golden_restart_file(rt):
    data = open(GOLDEN_RESTART, "rb").read()
    (got,), (rounds,) = device_pixels(rt, [data])
    bad = first_difference(got, pillow(data))
    assert bad is None, bad
    bad = first_difference(got, restatement(data))
    assert bad is None, bad
    assert rounds >= 2


def test_without_the_keyword_a_restart_file_stays_on_the_host(rt):
    data = save(J.content("smooth", 33, 17, 3), restart_marker_blocks=1)
    report = []
    out = rt.jpeg_decode_u8(data, DEV, report=report)
    assert report[0]["path"].startswith("host: a restart interval"), report
    assert first_difference(out.cpu().numpy(), pillow(data)) is None


@pytest.mark.parametrize("kind", MANY_KINDS)
def test_more_intervals_than_threads(rt, kind):
    """1089 intervals of one MCU: the settle stage's scans over the interval table and over the block counts run past one pass of the
    workgroup's 1024 threads and carry into a second; the noise file is also longer than ten pieces of the unstuff stage."""
    data = many_intervals_file(kind)
    p = F.parse(data, restart=True)
    assert p.restart_interval == 1 and markers_in(data) == 1088
    assert kind != "noise" or p.seg_length > 10 * 4096
    frames, record = rt.jpeg_decode_batch([p], [data], DEV)
    assert record.cpu().tolist()[0][0] == 0, record
    (got,), _ = device_pixels(rt, [data])                       # through the caller: not left to the host
    assert np.array_equal(frames[0, :, :, 0].cpu().numpy(), got)
    bad = first_difference(got, pillow(data))
    assert bad is None, f"against Pillow: {bad}"
    bad = first_difference(got, restatement(data))
    assert bad is None, f"against the restatement: {bad}"


# ---- markers on the unstuff stage's boundaries ---------------------------------------------------------------------------------------------
def marker_offsets(data):
    p = F.parse(data, restart=True)
    return [m.start() for m in re.finditer(rb"\xff[\xd0-\xd7]", data[p.seg_offset:p.seg_offset + p.seg_length])]


def test_markers_on_piece_boundaries(rt):
    """The unstuff stage works in pieces of 4096 bytes, four bytes a thread.  Files with a marker whose FF is the last byte of a piece
    (the Dn in the next), whose Dn is, and whose FF is the first byte of a piece are searched among seeded noise frames, with one MCU per
    interval, so that markers also fall on every position of a thread's four bytes; a stuffed FF 00 stands directly in front of a marker."""
    found = {}
    for s in range(2000):
        data = save(J.content("noise", 48, 64, 3, seed=s), 100, 0, restart_marker_blocks=1)
        for r in {o % 4096 for o in marker_offsets(data)} & {4095, 4094, 0}:
            found.setdefault(r, data)
        if len(found) == 3:
            break
    assert sorted(found) == [0, 4094, 4095], f"no file found for {sorted({0, 4094, 4095} - set(found))}"
    datas = list(dict.fromkeys(found.values()))
    assert any(re.search(rb"\xff\x00\xff[\xd0-\xd7]", d) for d in datas)
    assert {o % 4 for d in datas for o in marker_offsets(d)} == {0, 1, 2, 3}
    got, _ = device_pixels(rt, datas)
    for d, g in zip(datas, got):
        bad = first_difference(g, pillow(d))
        assert bad is None, bad


# ---- chunk_bits and the rounds ---------------------------------------------------------------------------------------------------------------
def test_pixels_do_not_depend_on_chunk_bits(rt):
    data = LANE_FILES["noise 48x64 q100 4:4:4 rows 1"]()
    want = pillow(data)
    for chunk_bits in (32, 64, 256, 0):
        (got,), (rounds,) = device_pixels(rt, [data], chunk_bits=chunk_bits)
        bad = first_difference(got, want)
        assert bad is None, f"chunk_bits {chunk_bits}: {bad}"
        assert rounds >= 2


def test_rounds_are_the_simulations(rt):
    """The device runs the per-interval scheme tests/jpeg_restart_ref.py simulates: the same number of rounds."""
    for name in ("noise 48x64 q100 4:4:4 rows 1", "smooth 64x64 4:2:0 blocks 5"):
        data = LANE_FILES[name]()
        for chunk_bits in (32, 256):
            _, (rounds,) = device_pixels(rt, [data], chunk_bits=chunk_bits)
            assert rounds == RR.decode(data, chunk_bits)[2], (name, chunk_bits)


def test_two_rounds_where_every_interval_fits_in_one_chunk(rt):
    """Intervals of 16 to 24 bits: round 0 decodes every one from its known state, round 1 changes nothing."""
    data = LANE_FILES["constant grey 64x64 optimize blocks 7"]()
    for chunk_bits in (32, 0):
        (got,), (rounds,) = device_pixels(rt, [data], chunk_bits=chunk_bits)
        assert rounds == 2
        assert first_difference(got, pillow(data)) is None


# ---- batches ------------------------------------------------------------------------------------------------------------------------------
def batch_of_four():
    h, w, kw = 37, 53, dict(restart_marker_blocks=3)
    return [save(J.content("noise", h, w, 3), 50, **kw), save(J.content("smooth", h, w, 3), 75, optimize=True, **kw), save(J.content("white", h, w, 3), 95, **kw),
            save(J.content("binary", h, w, 3), 100, optimize=True, **kw)]


@pytest.mark.parametrize("lead", [0, 1, 3])
def test_a_batch_of_four_equals_four_single_calls(rt, lead):
    """One geometry, one restart interval, four contents, four sets of tables, the segments at whatever byte offsets they fall on."""
    datas = batch_of_four()
    parsed = [F.parse(d, restart=True) for d in datas]
    assert len({p.geometry for p in parsed}) == 1 and {p.restart_interval for p in parsed} == {3} and len({p.blob for p in parsed}) == 4
    out, record = rt.jpeg_decode_batch(parsed, datas, DEV, lead=lead)
    assert record[:, 0].cpu().tolist() == [0, 0, 0, 0]
    batch = out.cpu().numpy()
    for i, d in enumerate(datas):
        single, rec = rt.jpeg_decode_batch(parsed[i:i + 1], [d], DEV)
        assert rec[0, 0].item() == 0
        bad = first_difference(batch[i], single[0].cpu().numpy())
        assert bad is None, f"file {i}: {bad}"
        bad = first_difference(batch[i], pillow(d))
        assert bad is None, f"file {i}: {bad}"


def test_two_restart_intervals_go_out_as_two_groups(rt, monkeypatch):
    a = J.content("smooth", 33, 17, 3)
    datas = [save(a, restart_marker_blocks=1), save(a, restart_marker_blocks=2), save(a, 90, restart_marker_blocks=1)]
    parsed = [F.parse(d, restart=True) for d in datas]
    with pytest.raises(rt.AdainHipError, match="one restart interval"):
        rt.jpeg_decode_batch(parsed, datas, DEV)
    entry = Counter(rt.jpeg_decode_batch)
    monkeypatch.setattr(rt, "jpeg_decode_batch", entry)
    got, _ = device_pixels(rt, datas)
    assert entry.calls == 2
    for d, g in zip(datas, got):
        assert first_difference(g, pillow(d)) is None


# ---- the memory contract, through the guard-band arena ----------------------------------------------------------------------------------
def abi_case(rt, datas, parsed=None, chunk_bits=0, restart_interval=None):
    """(specs, setup, call, geometry) of one direct call of adain_jpeg_decode_restart_u8 on the files ``datas`` (``parsed``: their
    descriptions, when the bytes are damaged and must not be parsed again; ``restart_interval``: another one than the files')."""
    parsed = parsed or [F.parse(d, restart=True) for d in datas]
    ri = parsed[0].restart_interval if restart_interval is None else restart_interval
    n = len(datas)
    h, w, c, sampling = parsed[0].geometry
    segs = [d[p.seg_offset:p.seg_offset + p.seg_length] for d, p in zip(datas, parsed)]
    lengths = [len(s) for s in segs]
    offsets = [3 + sum(lengths[:i]) for i in range(n)]
    files = b"\xa5\xa5\xa5" + b"".join(segs)
    blobs = b"".join(p.blob for p in parsed)
    nbytes = rt.jpeg_decode_sizes(n, h, w, c, sampling, max(lengths), chunk_bits, ri)
    specs = [("files", len(files), "in", 1), ("blobs", len(blobs), "in", 1), ("dst", n * h * w * c, "out", 1), ("record", 8 * n, "out", 4),
             ("workspace", nbytes, "ws", 8)]
    off, ln = (ctypes.c_uint64 * n)(*offsets), (ctypes.c_uint32 * n)(*lengths)
    stream = torch.cuda.current_stream().cuda_stream

    def setup(arena):
        arena.put("files", torch.frombuffer(bytearray(files), dtype=torch.uint8))
        arena.put("blobs", torch.frombuffer(bytearray(blobs), dtype=torch.uint8))

    def call(arena):
        rc = rt.lib().adain_jpeg_decode_restart_u8(arena.ptr("files"), len(files), arena.ptr("blobs"), n, h, w, c, sampling, ri, off, ln, arena.ptr("dst"),
                                                   arena.ptr("record"), arena.ptr("workspace"), arena.nbytes("workspace"), chunk_bits, stream)
        assert rc == 0, rt.lib().adain_last_error().decode()

    return specs, setup, call, (n, h, w, c)


ARENA_CASES = {
    "two 4:2:0 17x9 at Ri 1": lambda: [save(J.content("noise", 17, 9, 3, seed=i), 90, 2, restart_marker_blocks=1) for i in range(2)],
    "two 4:2:2 33x17 at Ri 3, one optimised": lambda: [save(J.content("smooth", 33, 17, 3), 75, 1, restart_marker_blocks=3),
                                                        save(J.content("noise", 33, 17, 3), 75, 1, optimize=True, restart_marker_blocks=3)],
    "4:4:4 16x16 at one row": lambda: [save(J.content("binary", 16, 16, 3), 75, 0, restart_marker_rows=1)],
    "two grey 64x64 at Ri 7": lambda: [save(J.content("binary", 64, 64, 1, seed=i), 75, "L", restart_marker_blocks=7) for i in range(2)],
}
HISTORIES = {"another Ri": dict(restart_marker_blocks=4), "Ri 0": {}}            # of a grey 8 x 40 file: 5 MCUs in intervals of 4 and 1


@pytest.mark.parametrize("past", HISTORIES)
@pytest.mark.parametrize("name", ARENA_CASES)
def test_the_call_stays_in_its_buffers_and_ignores_stale_bytes(rt, name, past):
    """dst, the record and the workspace start as 0xFF bytes and as a non-zero pattern: the pixels and the record are the same, no byte
    outside the three regions changes; then a call on another file through the same workspace - one with another restart interval, or
    with none - and the call again: stale streams, interval tables, states, coefficients and planes."""
    datas = ARENA_CASES[name]()
    specs, setup, call, (n, h, w, c) = abi_case(rt, datas)
    other = [save(J.content("noise", 8, 40, 1), 75, "L", **HISTORIES[past])]
    op = F.parse(other[0], restart=True)
    assert op.restart_interval == (4 if HISTORIES[past] else 0) != F.parse(datas[0], restart=True).restart_interval
    ospecs, _, _, (on, oh, ow, oc) = abi_case(rt, other, chunk_bits=32)
    assert ospecs[4][1] <= specs[4][1] and on * oh * ow * oc <= n * h * w * c
    up = torch.frombuffer(bytearray(op.blob + other[0][op.seg_offset:op.seg_offset + op.seg_length]), dtype=torch.uint8).to(DEV)

    def history(arena):
        off, ln = (ctypes.c_uint64 * 1)(0), (ctypes.c_uint32 * 1)(op.seg_length)
        rc = rt.lib().adain_jpeg_decode_restart_u8(up.data_ptr() + F.BLOB_BYTES, op.seg_length, up.data_ptr(), 1, oh, ow, oc, op.sampling, op.restart_interval, off, ln,
                                                   arena.ptr("dst"), arena.ptr("record"), arena.ptr("workspace"), arena.nbytes("workspace"), 32,
                                                   torch.cuda.current_stream().cuda_stream)
        assert rc == 0, rt.lib().adain_last_error().decode()

    outs = A.run_case(specs, call, DEV, torch.cuda.synchronize, history=history, setup=setup)
    record = outs["record"].cpu().numpy().view(np.int32).reshape(n, 2)
    assert record[:, 0].tolist() == [0] * n and (record[:, 1] >= 2).all()
    got = outs["dst"].cpu().numpy().reshape(n, h, w, c)
    for i, d in enumerate(datas):
        want = pillow(d)
        bad = first_difference(got[i].reshape(want.shape), want)
        assert bad is None, f"file {i}: {bad}"
    _arena_passed.add((name, past))


def test_refusals_come_before_any_launch(rt):
    data = save(J.content("smooth", 16, 16, 3), restart_marker_blocks=1)
    p = F.parse(data, restart=True)
    L = rt.lib()
    up = torch.frombuffer(bytearray(p.blob + data), dtype=torch.uint8).to(DEV)
    dst = torch.zeros(16 * 16 * 3, dtype=torch.uint8, device=DEV)
    record = torch.full((2,), 77, dtype=torch.int32, device=DEV)
    nbytes = rt.jpeg_decode_sizes(1, 16, 16, 3, 2, p.seg_length, 0, 1)
    assert nbytes > rt.jpeg_decode_sizes(1, 16, 16, 3, 2, p.seg_length), "the interval table takes room"
    ws = torch.empty(nbytes, dtype=torch.uint8, device=DEV)
    stream = torch.cuda.current_stream().cuda_stream

    def call(n=1, h=16, w=16, c=3, sampling=2, ri=1, offset=p.seg_offset, length=p.seg_length, files_bytes=len(data), nbytes=nbytes, chunk_bits=0, ws_ptr=ws.data_ptr()):
        off, ln = (ctypes.c_uint64 * 1)(offset), (ctypes.c_uint32 * 1)(length)
        return L.adain_jpeg_decode_restart_u8(up.data_ptr() + F.BLOB_BYTES, files_bytes, up.data_ptr(), n, h, w, c, sampling, ri, off, ln, dst.data_ptr(),
                                              record.data_ptr(), ws_ptr, nbytes, chunk_bits, stream)

    for kw in (dict(ri=-1), dict(ri=65536), dict(nbytes=nbytes - 1),
               dict(n=0), dict(c=2), dict(sampling=3), dict(c=1, sampling=2), dict(h=0), dict(w=65536), dict(chunk_bits=31), dict(chunk_bits=48), dict(chunk_bits=-32),
               dict(offset=len(data)), dict(length=len(data)), dict(ws_ptr=ws.data_ptr() + 4)):
        assert call(**kw) == -1 and L.adain_last_error().startswith(b"jpeg_decode_u8"), kw
    torch.cuda.synchronize()
    assert record.cpu().tolist() == [77, 77] and int(dst.sum()) == 0
    assert call() == 0
    torch.cuda.synchronize()
    assert record[0].item() == 0 and first_difference(dst.cpu().numpy().reshape(16, 16, 3), pillow(data)) is None
    size = ctypes.c_size_t()
    for ri in (-1, 65536):
        assert L.adain_jpeg_decode_restart_u8_bytes(1, 16, 16, 3, 2, ri, p.seg_length, 0, ctypes.byref(size)) == -1
        with pytest.raises(rt.AdainHipError):
            rt.jpeg_decode_sizes(1, 16, 16, 3, 2, p.seg_length, 0, ri)


@pytest.mark.parametrize("layout", LAYOUTS, ids=str)
def test_restart_interval_0_is_the_old_entry(rt, layout):
    """adain_jpeg_decode_restart_u8 at 0 and adain_jpeg_decode_u8: the same workspace size, the same dst and record, byte for byte."""
    data = save(J.content("noise", 33, 40, 1 if layout == "L" else 3), 90, layout)
    p = F.parse(data)
    h, w, c, sampling = p.geometry
    L = rt.lib()
    a, b = ctypes.c_size_t(), ctypes.c_size_t()
    assert L.adain_jpeg_decode_u8_bytes(1, h, w, c, sampling, p.seg_length, 32, ctypes.byref(a)) == 0
    assert L.adain_jpeg_decode_restart_u8_bytes(1, h, w, c, sampling, 0, p.seg_length, 32, ctypes.byref(b)) == 0
    assert a.value == b.value
    up = torch.frombuffer(bytearray(p.blob + data), dtype=torch.uint8).to(DEV)
    off, ln = (ctypes.c_uint64 * 1)(p.seg_offset), (ctypes.c_uint32 * 1)(p.seg_length)
    stream = torch.cuda.current_stream().cuda_stream
    outs = []
    for new in (False, True):
        dst = torch.zeros(h * w * c, dtype=torch.uint8, device=DEV)
        record = torch.full((2,), 77, dtype=torch.int32, device=DEV)
        ws = torch.full((a.value,), 0x5A, dtype=torch.uint8, device=DEV)
        args = [up.data_ptr() + F.BLOB_BYTES, len(data), up.data_ptr(), 1, h, w, c, sampling] + ([0] if new else []) + [off, ln, dst.data_ptr(), record.data_ptr(),
                                                                                                             ws.data_ptr(), a.value, 32, stream]
        assert (L.adain_jpeg_decode_restart_u8 if new else L.adain_jpeg_decode_u8)(*args) == 0, L.adain_last_error().decode()
        torch.cuda.synchronize()
        outs.append((dst.cpu().numpy(), record.cpu().tolist()))
    assert outs[0][1] == outs[1][1] and outs[0][1][0] == 0 and outs[0][1][1] >= 2
    assert np.array_equal(outs[0][0], outs[1][0])
    assert first_difference(outs[1][0].reshape(pillow(data).shape), pillow(data)) is None


# ---- damaged marker structure ----------------------------------------------------------------------------------------------------------------
def damaged(kind):
    """(bytes, description, the restart interval declared to the call)."""
    data = save(J.content("noise", 33, 17, 3), 90, 0, restart_marker_blocks=2)
    p = F.parse(data, restart=True)
    if kind == "declared Ri off by one":
        return data, p, 3
    at = data.index(b"\xff\xd2", p.seg_offset)
    bad = data[:at] + (b"\xff\xd5" if kind == "renumbered" else b"") + data[at + 2:]
    return bad, F.JpegFile(**{**p.__dict__, "seg_length": p.seg_length - (0 if kind == "renumbered" else 2)}), 2


@pytest.mark.parametrize("kind", ["renumbered", "removed", "declared Ri off by one"])
def test_damaged_marker_structure(rt, kind):
    """One marker renumbered, one removed, or a call that declares another interval than the file has: the status is non-zero or the
    pixels are Pillow's for those bytes, the guard bands are intact either way, and the wrapper returns what PIL returns."""
    if _arena_passed != {(name, past) for name in ARENA_CASES for past in HISTORIES}:
        pytest.fail("runs only after the arena tests of valid files have passed")
    bad, q, ri = damaged(kind)
    specs, setup, call, (n, h, w, c) = abi_case(rt, [bad], [q], chunk_bits=32, restart_interval=ri)
    outs = A.run_case(specs, call, DEV, torch.cuda.synchronize, setup=setup)
    status = int(outs["record"].cpu().numpy().view(np.int32)[0])
    want, error = pil_outcome(bad)
    print(f"{kind}: status {status}, PIL {'raises ' + error.__name__ if error else 'decodes'}")
    if status == 0:
        assert error is None, f"status 0 for bytes PIL refuses with {error.__name__}"
        diff = first_difference(outs["dst"].cpu().numpy().reshape(h, w, c), want)
        assert diff is None, f"status 0, but {diff}"
    if error is not None:
        with pytest.raises(error):
            rt.jpeg_decode_u8(bad, DEV, restart=True)
    else:
        report = []
        got = rt.jpeg_decode_u8(bad, DEV, report=report, restart=True).cpu().numpy()
        assert first_difference(got, want) is None, report


# ---- the callers ------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def ckpt(tmp_path_factory):
    d = tmp_path_factory.mktemp("ckpt")
    torch.save(synth.to_torch(synth.vgg_state_dict(0, full=True)), d / "vgg.pth")
    torch.save(synth.to_torch(synth.decoder_state_dict(0)), d / "dec.pth")
    return dict(vgg_str=str(d / "vgg.pth"), decoder_str=str(d / "dec.pth"))


@pytest.fixture
def t():
    from applied_image_processing_amd.AdaIN import test as t

    t.clear_style_cache()
    yield t
    t.set_device_jpeg_decode(False)
    t.clear_style_cache()


def test_adain_inference_keeps_a_restart_content_on_the_device(rt, t, ckpt, tmp_path, monkeypatch):
    """A 48 x 64 content with one restart interval per MCU row, given as a path, and the golden restart file as the style: byte-identical
    output with the switch off and on, and with it on the content is decoded by the device decoder."""
    content = tmp_path / "content.jpg"
    Image.fromarray(u8img(900, 48, 64)).save(content, quality=90, restart_marker_rows=1)
    assert F.parse(content.read_bytes(), restart=True).restart_interval == 4          # 4:2:0: four MCUs a row
    style = Image.open(GOLDEN_RESTART)
    entry = Counter(rt.jpeg_decode_batch)
    monkeypatch.setattr(rt, "jpeg_decode_batch", entry)
    files = {}
    for on in (False, True):
        t.set_device_jpeg_decode(on)
        p = t.adain_inference(str(content), style, content_size=32, style_size=32, output=str(tmp_path / f"out_{int(on)}"), file_name="x", **ckpt)
        files[on] = p.read_bytes()
        assert entry.calls == (1 if on else 0)
    assert files[True] == files[False]


def test_jpeg_decode_rgb_file_takes_restart_files(rt, tmp_path):
    path = tmp_path / "frame.jpg"
    Image.fromarray(u8img(901, 40, 56)).save(path, quality=85, restart_marker_blocks=2)
    got = rt.jpeg_decode_rgb_file(str(path), DEV)
    assert got is not None and got.is_cuda
    assert first_difference(got.cpu().numpy(), np.asarray(Image.open(path).convert("RGB"))) is None
    got = rt.jpeg_decode_rgb_file(GOLDEN_RESTART, DEV)
    assert got is not None and first_difference(got.cpu().numpy(), np.asarray(Image.open(GOLDEN_RESTART).convert("RGB"))) is None
