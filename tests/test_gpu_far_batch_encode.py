"""Far-batch tests of the file encoders (csrc/jpeg.hip: adain_jpeg_encode_u8, _opt_u8, _progressive_u8, adain_jpeg_roundtrip_u8;
csrc/png.hip; csrc/gif.hip): one call whose frames, file rows and workspace pass 2^32 bytes (the case table says which, per call),
``lengths`` and the first ``lengths[i]`` bytes of every row compared with the file of the frame's pattern - Pillow's own bytes for
the JPEG calls, png_ref's and gif_ref's for the other two: equality, as in the calls' own tests.  The rest of a row stays 0xA5.
tests/far_batch.py states the design and holds the cases.  Run with ``-m gpu``.

Out of scope here as everywhere in the far-batch tests: the whole-network calls, adain_tvl1_flow / adain_farneback_*, and the
single-frame calls.

Measured on an MI355X, seconds per test (fill, call and comparison):
png_encode_u8 1.10, gif_encode_u8 0.81, jpeg_encode_u8 0.32, jpeg_encode_progressive_u8 0.16, jpeg_encode_opt_u8 0.08,
jpeg_roundtrip_u8 0.05."""
import numpy as np
import pytest
import torch

import far_batch as B

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


@pytest.fixture(scope="module")
def rt():
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    import applied_image_processing_amd.runtime as rt

    rt.lib()
    torch.cuda.set_device(0)
    return rt


def run_files(rt, case, args):
    """``args(src, rows, stride, lengths, ws, ws_bytes) -> the C arguments`` of an encoder; rows, lengths and workspace poisoned."""
    B.reserve(case, DEV)
    (frames,), (files,) = case.make()
    sizes = dict((b[0], b[2]) for b in case.buffers())
    stride = sizes["rows"] // case.n
    assert stride * case.n == sizes["rows"] and max(len(f) for f in files) <= stride
    src = B.tile(frames, case.n, DEV)
    rows = B.poisoned((case.n, stride), torch.uint8, DEV)
    lengths = B.poisoned((case.n,), torch.int32, DEV)
    ws = B.poisoned((sizes["workspace"],), torch.uint8, DEV)
    try:
        assert src.numel() == sizes["src"]
        rt.call(case.call, torch.device(DEV), *args(src, rows, stride, lengths, ws, ws.numel()))
        torch.cuda.synchronize()
        want_len = np.asarray([len(f) for f in files], dtype=np.int32)
        B.assert_frames(case.id + ": lengths", lengths.view(case.n, 1), want_len.reshape(B.P, 1))
        padded = np.zeros((B.P, stride), dtype=np.uint8)
        for k, f in enumerate(files):
            padded[k, :len(f)] = np.frombuffer(f, np.uint8)
        B.assert_frames(case.id + ": files", rows, padded, lengths=want_len)
        # behind its file a row is not written
        for k in range(B.P):
            tail = rows[k::B.P, int(want_len[k]):]
            step = max(1, B.PIECE // max(1, tail.shape[1]))
            assert all(bool((tail[r:r + step] == 0xA5).all()) for r in range(0, tail.shape[0], step)), f"{case.id}: bytes behind a file of pattern {k} were written"
        B.assert_frames(case.id + ": the frames changed", src, frames)
    finally:
        del src, rows, lengths, ws
        B.release()


def test_jpeg_encode_u8(rt):
    case = B.BY_ID["jpeg_encode_u8"]
    run_files(rt, case, lambda src, rows, stride, lengths, ws, nbytes: (src.data_ptr(), case.n, B.H, B.W, 3, 75, rows.data_ptr(), stride, lengths.data_ptr(), ws.data_ptr(), nbytes))


def test_jpeg_encode_opt_u8(rt):
    case = B.BY_ID["jpeg_encode_opt_u8"]
    run_files(rt, case, lambda src, rows, stride, lengths, ws, nbytes: (src.data_ptr(), case.n, B.H, B.W, 3, 75, 0, 1, rows.data_ptr(), stride, lengths.data_ptr(), ws.data_ptr(), nbytes))


def test_jpeg_encode_progressive_u8(rt):
    case = B.BY_ID["jpeg_encode_progressive_u8"]
    run_files(rt, case, lambda src, rows, stride, lengths, ws, nbytes: (src.data_ptr(), case.n, B.H, B.W, 3, 75, 2, rows.data_ptr(), stride, lengths.data_ptr(), ws.data_ptr(), nbytes))


def test_png_encode_u8(rt):
    case = B.BY_ID["png_encode_u8"]
    run_files(rt, case, lambda src, rows, stride, lengths, ws, nbytes: (src.data_ptr(), case.n, B.H, B.W, 3, -1, rows.data_ptr(), stride, lengths.data_ptr(), ws.data_ptr(), nbytes))


def test_gif_encode_u8(rt):
    case = B.BY_ID["gif_encode_u8"]
    _p, h, w = case.make()[0][0].shape
    run_files(rt, case, lambda src, rows, stride, lengths, ws, nbytes: (src.data_ptr(), case.n, h, w, 16, 5, rows.data_ptr(), stride, lengths.data_ptr(), ws.data_ptr(), nbytes))


def test_jpeg_roundtrip_u8(rt):
    case = B.BY_ID["jpeg_roundtrip_u8"]
    sizes = dict((b[0], b[2]) for b in case.buffers())
    B.run_equal(rt, case, DEV, [((B.H, B.W, 3), torch.uint8)],
                lambda src, dst, ws: (src.data_ptr(), case.n, B.H, B.W, 3, 75, dst.data_ptr(), ws.data_ptr(), ws.numel()), workspace=sizes["workspace"])
