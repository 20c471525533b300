"""The device JPEG encoder and round trip (csrc/jpeg.hip) on the designed frames of tests/jpeg_symbols.py: every run/size symbol of both
Huffman tables, every DC category, one to three ZRLs in front of every size, blocks that end at coefficient 63, lane patterns up to
the 63 bits a lane can build, at every bit offset (tests/test_jpeg_symbols_host.py asserts that the frames hold all this).  Byte and
element equality throughout: against the NumPy restatements and, in tests of their own, against Pillow - a failure of the first kind
says the kernel moved, of the second kind alone that the environment's Pillow / libjpeg did.  Then uneven batches, and the densest
frame through the guard-band arena (tests/abi_arena.py)."""
import functools
import io

import numpy as np
import pytest
import torch
from PIL import Image

import abi_arena as A
import jpeg_decode_ref as D
import jpeg_ref as J
import jpeg_symbols as S

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
MODES = ["L", "RGB"]


@pytest.fixture(scope="module")
def rt():
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    import applied_image_processing_amd.runtime as rt

    rt.lib()
    torch.cuda.set_device(0)
    return rt


def nhwc(img):
    return img[None, :, :, None] if img.ndim == 2 else img[None]


_device = {}


def device_file(rt, name, quality, img):
    """The device's file of a designed frame in a call of its own; one call per frame for the whole module."""
    if name not in _device:
        out, lengths = rt.jpeg_encode_u8(torch.from_numpy(np.array(nhwc(img))).to(DEV), quality)
        _device[name] = rt.jpeg_files(out, lengths)[0]
    return _device[name]


_pixels = {}


def device_pixels(rt, name, quality, img):
    if name not in _pixels:
        _pixels[name] = rt.jpeg_roundtrip_u8(torch.from_numpy(np.array(img)).to(DEV), quality).cpu().numpy()
    return _pixels[name]


@functools.lru_cache(maxsize=None)
def restatement_file(mode, name):
    """Computed once per frame, shared by the tests."""
    quality, img = next((f[1], f[2]) for f in S.frames(mode) if f[0] == name)
    return J.encode(img, quality)


@functools.lru_cache(maxsize=None)
def pillow_file(mode, name):
    quality, img = next((f[1], f[2]) for f in S.frames(mode) if f[0] == name)
    f = io.BytesIO()
    Image.fromarray(img).save(f, format="JPEG", quality=quality)
    return f.getvalue()


def first_difference(got, want):
    k = next((i for i in range(min(len(got), len(want))) if got[i] != want[i]), min(len(got), len(want)))
    return f"{len(got)} bytes against {len(want)}, first difference at {k}"


def first_pixel_difference(got, want):
    assert got.shape == want.shape and got.dtype == want.dtype == np.uint8, f"{got.shape} {got.dtype} against {want.shape} {want.dtype}"
    at = np.argwhere(got != want)
    if len(at) == 0:
        return None
    i = tuple(int(v) for v in at[0])
    return f"{len(at)} of {got.size} elements differ; the first at pixel (row {i[0]}, column {i[1]}), channel {i[2] if len(i) > 2 else 0}: {got[i]} against {want[i]}"


@pytest.mark.parametrize("mode", MODES)
def test_device_bytes_are_the_restatements(rt, mode):
    for name, quality, img in S.frames(mode):
        got, want = device_file(rt, name, quality, img), restatement_file(mode, name)
        assert got == want, f"{name}: {first_difference(got, want)}"


@pytest.mark.parametrize("mode", MODES)
def test_device_bytes_are_pillows(rt, mode):
    for name, quality, img in S.frames(mode):
        got, want = device_file(rt, name, quality, img), pillow_file(mode, name)
        assert got == want, f"{name}: {first_difference(got, want)}"


@pytest.mark.parametrize("mode", MODES)
def test_device_pixels_are_the_restatements(rt, mode):
    for name, quality, img in S.frames(mode):
        bad = first_pixel_difference(device_pixels(rt, name, quality, img), D.roundtrip(img, quality))
        assert bad is None, f"{name}: {bad}"


@pytest.mark.parametrize("mode", MODES)
def test_device_pixels_are_pillows(rt, mode):
    for name, quality, img in S.frames(mode):
        want = np.asarray(Image.open(io.BytesIO(pillow_file(mode, name))).convert(mode))
        bad = first_pixel_difference(device_pixels(rt, name, quality, img), want)
        assert bad is None, f"{name}: {bad}"


@pytest.mark.parametrize("mode", MODES)
def test_a_batch_of_uneven_frames_equals_the_single_calls(rt, mode):
    """All designed frames of one quality (they have one shape) in one call: files from 2 KB to 190 KB side by side at quality 100, so
    the per-frame 64-bit offsets, the zeroing and the stuffing scan see very different totals.  The encoder and the round trip."""
    fr = S.frames(mode)
    for quality in S.QUALITIES:
        group = [f for f in fr if f[1] == quality]
        assert len(group) >= 2
        x = torch.from_numpy(np.concatenate([nhwc(f[2]) for f in group])).to(DEV)
        out, lengths = rt.jpeg_encode_u8(x, quality)
        batch = rt.jpeg_files(out, lengths)
        assert len({len(b) for b in batch}) == len(batch)
        pixels = rt.jpeg_roundtrip_u8(x, quality).cpu().numpy()
        for i, (name, _, img) in enumerate(group):
            single = device_file(rt, name, quality, img)
            assert batch[i] == single, f"{name} as frame {i} of {len(group)}: {first_difference(batch[i], single)}"
            bad = first_pixel_difference(pixels[i].reshape(img.shape), device_pixels(rt, name, quality, img))
            assert bad is None, f"{name} as frame {i} of {len(group)}: {bad}"


@pytest.mark.parametrize("mode", MODES)
def test_the_densest_frame_stays_in_its_buffers(rt, mode, capsys):
    """The designed frame with the most bits per block, alone, with out, lengths and the workspace starting as 0xFF bytes and as a
    non-zero pattern: the length is exact, the file is the restatement's, no byte outside the three regions changes and none behind the
    file inside `out`; then a smaller call through the same buffers and the call again.  An in-bounds check of jpeg_encode_sizes on a
    stream of 936.0 (L) and 775.6 (RGB) bits per block, computed on the host and printed here; 0 / 255 noise at quality 75, the densest
    content of tests/test_gpu_jpeg.py's arena cases, has 348 and 260; the size query allows max_block_bits = 1660."""
    name, quality, img = S.densest(mode)
    density = S.bits_per_block(img, quality)
    with capsys.disabled():
        print(f"\n{name}: {density:.1f} bits per block, max_block_bits {J.max_block_bits()}")
    assert density <= J.max_block_bits()
    frames = nhwc(img)
    n, h, w, c = frames.shape
    stride, nbytes = rt.jpeg_encode_sizes(n, h, w, c)
    specs = [("src", frames.size, "in", 1), ("out", n * stride, "ws", 1), ("lengths", 4 * n, "out", 4), ("workspace", nbytes, "ws", 8)]
    src = torch.from_numpy(np.array(frames))
    stream = torch.cuda.current_stream().cuda_stream
    want = restatement_file(mode, name)

    def call(arena, shape=(n, h, w, c)):
        rc = rt.lib().adain_jpeg_encode_u8(arena.ptr("src"), *shape, quality, arena.ptr("out"), stride, arena.ptr("lengths"), arena.ptr("workspace"),
                                           nbytes, stream)
        assert rc == 0, rt.lib().adain_last_error().decode()

    def files(arena):
        """The file as an output; behind it, the row still holds the arena's fill."""
        k, = arena.bytes("lengths").view(torch.int32).tolist()
        assert 0 < k <= stride
        row = arena.bytes("out")[:stride]
        a, b = arena.region("out").offset + k, arena.region("out").offset + stride
        assert bool((row[k:] == arena._expected(a, b)).all()), f"bytes behind the file's {k} changed"
        return {"files": row[:k].clone()}

    outs = A.run_case(specs, call, DEV, torch.cuda.synchronize, history=lambda arena: call(arena, (1, h // 8, w // 8, c)),
                      setup=lambda arena: arena.put("src", src), extra=files)
    got = outs["files"].cpu().numpy().tobytes()
    assert int(outs["lengths"].view(torch.int32)[0]) == len(want)
    assert got == want, f"{name}: {first_difference(got, want)}"
