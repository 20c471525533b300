"""The device PNG writer (csrc/png.hip, adain_png_encode_u8): its files against the NumPy restatement (tests/png_ref.py), byte for byte,
on the cases of tests/png_cases.py - the smallest frames that reach every rule; tests/test_png_host.py holds the restatement itself to
zlib and Pillow on the same cases.  Then batches, a side stream, buffers off the 4-byte grid, and every refusal."""
import ctypes

import numpy as np
import pytest
import torch

import png_cases as C
import png_ref as P

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
def want():
    """The restatement's file of every case, computed once."""
    return {name: P.encode(frame, filt) for name, frame, filt in C.cases()}


def device_files(rt, frames, filt=None):
    out, lengths = rt.png_encode_u8(torch.from_numpy(np.ascontiguousarray(frames)).to(DEV), filt)
    files = rt.png_files(out, lengths)
    assert all(len(f) <= out.shape[1] for f in files)
    return files


def first_difference(got, want):
    k = next((i for i in range(min(len(got), len(want))) if got[i] != want[i]), min(len(got), len(want)))
    return f"{len(got)} bytes against {len(want)}, first difference at {k}"


@pytest.mark.parametrize("name", [name for name, _, _ in C.cases()])
def test_device_file_is_the_restatements(rt, want, name):
    frame, filt = next((f, k) for n, f, k in C.cases() if n == name)
    got, = device_files(rt, frame[None], filt)
    assert got == want[name], f"{name}: {first_difference(got, want[name])}"


@pytest.mark.parametrize("n", [2, 3])
def test_a_batch_is_its_frames_alone(rt, n):
    rng = np.random.default_rng(n)
    frames = np.stack([C.noisy_gradient(37, 53, 10 + i) if i != 1 else rng.integers(0, 256, (37, 53, 3), dtype=np.uint8) for i in range(n)])
    got = device_files(rt, frames)
    for i in range(n):
        alone, = device_files(rt, frames[i:i + 1])
        assert got[i] == alone == P.encode(frames[i]), f"frame {i} of {n}"
    grey = device_files(rt, frames[:, :, :, :1], 4)
    assert grey == [P.encode(f[:, :, :1], 4) for f in frames]


def test_on_a_side_stream(rt, want):
    frame = next(f for n, f, _ in C.cases() if n == "gradient_128x228")
    side = torch.cuda.Stream(DEV)
    with torch.cuda.stream(side):
        got, = device_files(rt, frame[None])
    side.synchronize()
    assert got == want["gradient_128x228"]


def test_src_and_out_off_the_word_grid(rt):
    frame = C.noisy_gradient(19, 23, 3)
    h, w, c = frame.shape
    stride, nbytes = rt.png_encode_sizes(2, h, w, c)
    src = torch.zeros(2 * frame.size + 8, dtype=torch.uint8, device=DEV)
    src[1:1 + 2 * frame.size] = torch.from_numpy(np.stack([frame, frame[::-1]]).reshape(-1)).to(DEV)
    out = torch.zeros(2 * (stride + 1) + 8, dtype=torch.uint8, device=DEV)
    lengths = torch.zeros(2, dtype=torch.int32, device=DEV)
    ws = torch.empty(nbytes, dtype=torch.uint8, device=DEV)
    assert (src.data_ptr() + 1) % 4 and (out.data_ptr() + 3) % 4
    rc = rt.lib().adain_png_encode_u8(src.data_ptr() + 1, 2, h, w, c, -1, out.data_ptr() + 3, stride + 1, lengths.data_ptr(), ws.data_ptr(), nbytes,
                                      torch.cuda.current_stream().cuda_stream)
    assert rc == 0, rt.lib().adain_last_error()
    host, ln = out.cpu().numpy(), lengths.cpu().tolist()
    for i, f in enumerate((frame, np.ascontiguousarray(frame[::-1]))):
        at = 3 + i * (stride + 1)
        assert host[at:at + ln[i]].tobytes() == P.encode(f)
    assert not host[:3].any()


def test_noise_and_a_stylised_frame_stay_within_out_stride(rt):
    for name in ("noise_64x96", "stylised_256x456"):
        frame = next(f for n, f, _ in C.cases() if n == name)
        out, lengths = rt.png_encode_u8(torch.from_numpy(frame[None]).to(DEV))
        assert out.shape[1] == P.out_stride(*frame.shape) and 0 < int(lengths[0]) <= out.shape[1]


def test_refusals(rt):
    L = rt.lib()
    s, b = ctypes.c_size_t(), ctypes.c_size_t()
    assert L.adain_png_encode_u8_bytes(2, 8, 9, 3, ctypes.byref(s), ctypes.byref(b)) == 0
    buf = torch.zeros(b.value + s.value * 2 + 4096, dtype=torch.uint8, device=DEV)
    p = buf.data_ptr()
    assert p % 8 == 0

    def call(src=p, n=2, h=8, w=9, c=3, filt=-1, out=p, stride=None, lengths=p, ws=p, ws_bytes=None):
        return L.adain_png_encode_u8(src, n, h, w, c, filt, out, s.value if stride is None else stride, lengths, ws, b.value if ws_bytes is None else ws_bytes, None)

    refused = [dict(src=None), dict(out=None), dict(lengths=None), dict(ws=None), dict(c=2), dict(c=4), dict(h=0), dict(h=65536), dict(w=0), dict(w=65536),
               dict(n=0), dict(n=65536), dict(filt=-2), dict(filt=5), dict(stride=s.value - 1), dict(ws_bytes=b.value - 1), dict(ws=p + 4), dict(lengths=p + 2),
               dict(h=65535, w=65535)]
    for kw in refused:
        assert call(**kw) == -1 and L.adain_last_error(), kw
    for dims in ((0, 8, 8, 3), (65536, 8, 8, 3), (1, 8, 8, 2), (1, 0, 8, 3), (1, 8, 65536, 3), (1, 65535, 65535, 3)):
        assert L.adain_png_encode_u8_bytes(*dims, ctypes.byref(s), ctypes.byref(b)) == -1 and L.adain_last_error(), dims
    torch.cuda.synchronize()
    assert not buf.any(), "a refused call wrote to its buffers"
    with pytest.raises(rt.AdainHipError):
        rt.png_encode_u8(torch.zeros(4, 4, 3, dtype=torch.uint8, device=DEV), filter=5)
    with pytest.raises(rt.AdainHipError):
        rt.png_encode_u8(torch.zeros(4, 4, 4, dtype=torch.uint8, device=DEV))
