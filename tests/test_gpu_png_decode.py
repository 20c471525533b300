"""The device PNG decoder (csrc/png_decode.hip, adain_png_decode_u8): its pixels against the restatement (tests/png_decode_ref.py) and
against Pillow on the files of tests/png_decode_cases.py, in the file's channels and in 3; the statuses of the damaged files; batches,
also of sound and damaged files mixed; the device writer's own files; a side stream; the size query and every refusal.
tests/test_png_decode_host.py holds the restatement itself to zlib and Pillow on the same files.  Every check is an equality."""
import ctypes
import io

import numpy as np
import pytest
import torch
from PIL import Image

import png_cases
import png_decode_cases as C
import png_decode_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


@pytest.fixture(scope="module")
def rt():
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    import applied_image_processing_amd.runtime as rt

    rt.lib()
    torch.cuda.set_device(0)
    return rt


@pytest.fixture(scope="module")
def png_file():
    import applied_image_processing_amd.png_file as png_file

    return png_file


@pytest.fixture(scope="module")
def want():
    """Per sound case the restatement's pixels (Pillow's for the two large fixtures, which the host test holds the restatement to)."""
    out = {}
    for c in C.sound():
        out[c.name] = c.pixels if c.pixels is not None else np.asarray(Image.open(io.BytesIO(c.data)))
    return out


def decode(rt, png_file, datas, c_out=None):
    parsed = [png_file.parse(d) for d in datas]
    out, record = rt.png_decode_batch(parsed, datas, DEV, c_out)
    return out.cpu().numpy(), record.cpu().numpy()


def in_three(px):
    return np.repeat(px, 3, axis=2) if px.shape[2] == 1 else px[:, :, :3]


@pytest.mark.parametrize("name", [c.name for c in C.sound()])
def test_device_pixels_are_the_restatements_and_pillows(rt, png_file, want, name):
    case = next(c for c in C.sound() if c.name == name)
    pil = Image.open(io.BytesIO(case.data))
    for c_out in (None, 3):
        out, record = decode(rt, png_file, [case.data], c_out)
        assert record[0, 0] == 0, f"{name}: status {R.STATUS_NAMES[record[0, 0]]}"
        px = want[name].reshape(case.h, case.w, case.c)
        assert np.array_equal(out[0], px if c_out is None else in_three(px)), f"{name}, c_out {c_out}"
        assert np.array_equal(out[0].reshape(np.asarray(pil).shape) if c_out is None else out[0], np.asarray(pil if c_out is None else pil.convert("RGB")))
    if case.pixels is not None and case.h * case.w < 70000:
        assert record[0, 1] == len(R.inflate(png_file.parse(case.data).stream, case.h * (case.w * case.c + 1))[2].blocks)


def test_damaged_files_report_their_status(rt, png_file):
    """Every damaged file as an ordinary input, once, each alone in its call."""
    for case in C.damaged():
        _, record = decode(rt, png_file, [case.data])
        assert record[0, 0] == case.status, f"{case.name}: {R.STATUS_NAMES[record[0, 0]]}, expected {R.STATUS_NAMES[case.status]}"


def test_a_batch_is_its_files_alone_also_beside_damaged_ones(rt, png_file, want):
    px = C.gradient(2, 4, 1, 60)
    sound = [C.file_of(px, [1, 2]), C.file_of(C.noise(2, 4, 1, 7), [3, 4], level=0), C.file_of(C.noise(2, 4, 1, 8), [4, 0], strategy=2)]
    frames = [px, C.noise(2, 4, 1, 7), C.noise(2, 4, 1, 8)]
    damaged = [c for c in C.damaged() if (c.h, c.w, c.c) == (2, 4, 1)]
    assert len(damaged) >= 18
    datas, expect = [], []
    for i, d in enumerate(damaged):                 # a sound file between every two damaged ones
        datas += [d.data, sound[i % 3]]
        expect += [(d.status, None), (0, frames[i % 3])]
    out, record = decode(rt, png_file, datas)
    for k, (status, frame) in enumerate(expect):
        assert record[k, 0] == status, f"file {k}"
        if frame is not None:
            assert np.array_equal(out[k], frame), f"file {k}"
    same = [c for c in C.sound() if c.name.startswith(("zlib_", "idat_")) and (c.h, c.w, c.c) == (40, 33, 3)]
    assert len(same) >= 8
    out, record = decode(rt, png_file, [c.data for c in same], 3)
    assert not record[:, 0].any()
    for k, c in enumerate(same):
        alone, _ = decode(rt, png_file, [c.data], 3)
        assert np.array_equal(out[k], alone[0]) and np.array_equal(out[k], want[c.name])


def test_the_device_writers_own_files_decode_to_the_frame_without_a_download(rt, png_file):
    for name, frame, filt in png_cases.cases():
        x =torch.from_numpy(np.ascontiguousarray(frame)).to(DEV)
        files, lengths = rt.png_encode_u8(x, filt)
        n = int(lengths[0].item())
        h, w, c = frame.shape
        data = files[0, :n]
        # what png_file.parse would hand over, taken on the device: one IDAT behind the 41 bytes of signature, IHDR and IDAT's head
        stream = data[41:n - 16].contiguous()
        out = torch.empty((1, h, w, c), dtype=torch.uint8, device=DEV)
        record = torch.empty((1, 2), dtype=torch.int32, device=DEV)
        nbytes = rt.png_decode_sizes(1, h, w, c, stream.numel())
        ws = torch.empty(nbytes, dtype=torch.uint8, device=DEV)
        off = (ctypes.c_uint64 * 2)(0, stream.numel())
        rc = rt.lib().adain_png_decode_u8(stream.data_ptr(), stream.numel(), off, 1, h, w, c, c, out.data_ptr(), record.data_ptr(), ws.data_ptr(), nbytes,
                                          torch.cuda.current_stream().cuda_stream)
        assert rc == 0, rt.lib().adain_last_error().decode()
        assert record[0, 0].item() == 0, name
        assert torch.equal(out[0], x), name
        assert png_file.parse(bytes(data.cpu().numpy())).stream == bytes(stream.cpu().numpy())


def test_on_a_side_stream(rt, png_file, want):
    case = next(c for c in C.sound() if c.name == "height_129")
    side = torch.cuda.Stream(DEV)
    with torch.cuda.stream(side):
        parsed = png_file.parse(case.data)
        out, record = rt.png_decode_batch([parsed], [case.data], DEV)
    side.synchronize()
    assert record[0, 0].item() == 0 and np.array_equal(out[0].cpu().numpy(), want["height_129"])


def test_the_size_query_matches_the_launch_and_refuses_bad_shapes(rt, png_file):
    lib = rt.lib()
    case = next(c for c in C.sound() if c.name == "height_65")
    p = png_file.parse(case.data)
    n, h, w, c = 2, p.h, p.w, p.c
    nbytes = rt.png_decode_sizes(n, h, w, c, len(p.stream))
    assert nbytes >= n * h * (w * c + 1) and nbytes % 256 == 0
    up = torch.frombuffer(bytearray(p.stream * 2), dtype=torch.uint8).to(DEV)
    out = torch.empty((n, h, w, c), dtype=torch.uint8, device=DEV)
    record = torch.empty((n, 2), dtype=torch.int32, device=DEV)
    ws = torch.empty(nbytes, dtype=torch.uint8, device=DEV)
    off = (ctypes.c_uint64 * 3)(0, len(p.stream), 2 * len(p.stream))
    stream = torch.cuda.current_stream().cuda_stream

    def call(n=n, h=h, w=w, c=c, c_out=c, off=off, nbytes=nbytes, ws_ptr=None, record_ptr=None, streams_bytes=up.numel()):
        return lib.adain_png_decode_u8(up.data_ptr(), streams_bytes, off, n, h, w, c, c_out, out.data_ptr(), record.data_ptr() if record_ptr is None else record_ptr,
                                       ws.data_ptr() if ws_ptr is None else ws_ptr, nbytes, stream)

    assert call() == 0, lib.adain_last_error().decode()         # exactly the query's bytes are enough
    assert record[:, 0].tolist() == [0, 0] and np.array_equal(out[1].cpu().numpy(), case.pixels)
    assert call(nbytes=nbytes - 1) != 0 and b"workspace too small" in lib.adain_last_error()
    assert call(ws_ptr=ws.data_ptr() + 4) != 0
    assert call(record_ptr=record.data_ptr() + 2) != 0
    assert call(c_out=1) != 0 and call(c_out=4) != 0 and call(c=2, c_out=2) != 0
    assert call(n=0) != 0 and call(h=0) != 0 and call(w=0) != 0
    assert call(off=(ctypes.c_uint64 * 3)(0, 2 * len(p.stream), len(p.stream))) != 0
    assert call(streams_bytes=up.numel() - 1) != 0
    size = ctypes.c_size_t()
    for bad in ((0, 4, 4, 3, 10), (1, 0, 4, 3, 10), (1, 4, 0, 3, 10), (1, 4, 4, 2, 10), (1, 4, 4, 5, 10), (70000, 4, 4, 3, 10), (1, 32768, 21846, 3, 10), (1, 4, 4, 3, 1 << 31)):
        assert lib.adain_png_decode_u8_bytes(*bad, ctypes.byref(size)) != 0, bad
    assert lib.adain_png_decode_u8_bytes(1, 32768, 21845, 3, 10, ctypes.byref(size)) != 0          # h (w c + 1) = 2^31
    assert lib.adain_png_decode_u8_bytes(1, 32768, 21844, 3, 10, ctypes.byref(size)) == 0
    assert lib.adain_png_decode_u8_bytes(1, 4, 4, 4, 10, None) == 0
