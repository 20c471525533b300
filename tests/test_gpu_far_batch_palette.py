"""Far-batch tests of palette control (csrc/palette.hip: adain_palette_map_u8, adain_tone_u8, adain_palette_dither_u8) and the palette
chooser (csrc/quantize.hip: adain_quantize_palette_u8, per frame and global): one call whose buffers pass 2^32 bytes (the case table
says which, per call), every frame compared with palette_ref's / quantize_ref's result for its pattern - equality, the bar of the
calls' own tests.  The global chooser makes ONE palette over 65535 frames, 4.12 GiB inside one palette: the expected palette is
quantize_ref's over the P patterns with their multiplicities (``palette_weighted``, pinned in test_quantize_host.py).
tests/far_batch.py states the design and holds the cases.  Run with ``-m gpu``.

Out of scope here as everywhere in the far-batch tests: the whole-network calls, adain_tvl1_flow / adain_farneback_*, and the
single-frame calls.

Measured on an MI355X, seconds per test (fill, call and comparison):
palette_dither_u8/index 3.94 (28.7 GiB), palette_dither_u8/wide 3.13 (65535 workgroups of 5469 sequential steps), palette_dither_u8 1.41, quantize global 0.83,
palette_map_u8 0.38, palette_map_u8/index 0.3, quantize per frame 0.30, per frame of 66 MB 0.30, tone_u8 0.02."""
import numpy as np
import pytest
import torch

import far_batch as B

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
K = B.PALETTE_K


@pytest.fixture(scope="module")
def rt():
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    import applied_image_processing_amd.runtime as rt

    rt.lib()
    torch.cuda.set_device(0)
    return rt


@pytest.mark.parametrize("id,metric", [("palette_map_u8", 1), ("palette_map_u8/index", 0)])
def test_palette_map_u8(rt, id, metric):
    case = B.BY_ID[id]
    _p, h, w, _c = case.make()[0][0].shape
    B.run_equal(rt, case, DEV, [((h, w, 3), torch.uint8), ((h, w), torch.uint8)],
                lambda src, pal, out, idx: (src.data_ptr(), case.n, h, w, pal.data_ptr(), K, metric, None, 0, out.data_ptr(), idx.data_ptr()), shared=1)


def test_tone_u8(rt):
    case = B.BY_ID["tone_u8"]
    B.run_equal(rt, case, DEV, [((B.H, B.W, 3), torch.uint8)], lambda src, lut, out: (src.data_ptr(), case.n, B.H, B.W, lut.data_ptr(), 1, out.data_ptr()), shared=1)


@pytest.mark.parametrize("id", ["palette_dither_u8", "palette_dither_u8/wide", "palette_dither_u8/index"])
def test_palette_dither_u8(rt, id):
    case = B.BY_ID[id]
    _p, h, w, _c = case.make()[0][0].shape
    sizes = dict((b[0], b[2]) for b in case.buffers())
    B.run_equal(rt, case, DEV, [((h, w, 3), torch.uint8), ((h, w), torch.uint8)],
                lambda src, pal, out, idx, ws: (src.data_ptr(), case.n, h, w, pal.data_ptr(), K, None, 0, out.data_ptr(), idx.data_ptr(), ws.data_ptr(), ws.numel()),
                workspace=sizes["workspace"], shared=1)


def test_quantize_palette_per_frame(rt):
    case = B.BY_ID["quantize_palette_u8/per_frame"]
    sizes = dict((b[0], b[2]) for b in case.buffers())
    B.run_equal(rt, case, DEV, [((256, 3), torch.uint8), ((), torch.int32)],
                lambda src, pals, used, ws: (src.data_ptr(), case.n, B.H, B.W, K, 1, pals.data_ptr(), used.data_ptr(), ws.data_ptr(), ws.numel()),
                workspace=sizes["workspace"])


def test_quantize_palette_per_frame_of_66_mb(rt):
    """Frames of 66 MB, so that 70 of them pass 2^32 bytes: each is its 128 x 176 pattern 977 times one below the other."""
    case = B.BY_ID["quantize_palette_u8/per_frame_source"]
    (frames,), (pals, used) = case.make()
    sizes = dict((b[0], b[2]) for b in case.buffers())
    B.reserve(case, DEV)
    p = B.upload(frames, DEV)
    src = torch.empty((case.n, B.TALL, B.H, B.W, 3), dtype=torch.uint8, device=DEV)
    for k in range(B.P):
        src[k::B.P] = p[k]
    out_p, out_u = B.poisoned((case.n, 256, 3), torch.uint8, DEV), B.poisoned((case.n,), torch.int32, DEV)
    ws = B.poisoned((sizes["workspace"],), torch.uint8, DEV)
    try:
        assert src.numel() == sizes["src"] and src.numel() > B.TWO32
        rt.call(case.call, torch.device(DEV), src.data_ptr(), case.n, B.TALL * B.H, B.W, K, 1, out_p.data_ptr(), out_u.data_ptr(), ws.data_ptr(), ws.numel())
        torch.cuda.synchronize()
        B.assert_frames(case.id + ": palettes", out_p, pals)
        B.assert_frames(case.id + ": used", out_u.view(case.n, 1), used.reshape(B.P, 1))
        B.assert_frames(case.id + ": the frames changed", src.view(case.n, B.TALL, -1)[:, 0], frames.reshape(B.P, -1))
        B.assert_frames(case.id + ": the frames changed", src.view(case.n, B.TALL, -1)[:, B.TALL - 1], frames.reshape(B.P, -1))
    finally:
        del src, out_p, out_u, ws
        B.release()


def test_quantize_palette_global(rt):
    case = B.BY_ID["quantize_palette_u8/global"]
    (frames,), (pal, used) = case.make()
    sizes = dict((b[0], b[2]) for b in case.buffers())
    B.reserve(case, DEV)
    src = B.tile(frames, case.n, DEV)
    out_p, out_u = B.poisoned((256, 3), torch.uint8, DEV), B.poisoned((1,), torch.int32, DEV)
    ws = B.poisoned((sizes["workspace"],), torch.uint8, DEV)
    try:
        assert src.numel() == sizes["src"] and src.numel() > B.TWO32
        rt.call(case.call, torch.device(DEV), src.data_ptr(), case.n, B.H, B.W, 256, 0, out_p.data_ptr(), out_u.data_ptr(), ws.data_ptr(), ws.numel())
        torch.cuda.synchronize()
        assert out_u.cpu().tolist() == used[0].tolist()
        got = out_p.cpu().numpy()
        assert np.array_equal(got, pal[0]), f"entries {np.flatnonzero((got != pal[0]).any(axis=1))[:8].tolist()} differ from the weighted restatement's"
        B.assert_frames(case.id + ": the frames changed", src, frames)
    finally:
        del src, out_p, out_u, ws
        B.release()
