"""Far-batch tests of the pixel kernels (csrc/pixel.hip) and the flow estimators' frame preparation (csrc/flow.hip, csrc/tvl1.hip): one
call over a batch whose buffers pass 2^32 bytes, every frame compared with the restatement's result for its pattern.
tests/far_batch.py states the design and holds the cases; pixel_ref, the oracle and farneback_ref are the references the kernels'
own tests use, and the bar is theirs: equality.  adain_tvl1_prepare's bar is a tolerance (test_gpu_tvl1.py), so its P frames alone
are held to it and the batch to those P device results, bit for bit.  Run with ``-m gpu``.

Out of scope here as everywhere in the far-batch tests: the whole-network calls, adain_tvl1_flow / adain_farneback_*, and the
single-frame calls (adain_strength_map, adain_warp_blend_u8, adain_colour_transfer_u8, adain_localized_combine_u8).

Measured on an MI355X, seconds per test (fill, call and comparison; the host references are computed once per process):
quantize_u8 rgb4 0.46, generic 0.03; u8_to_f32 0.02 and 0.03; resize_bilinear 0.02, resize_nearest 2.81; mask_composite 0.02;
resize_area_u8 linear 0.04, 2x2_rgb4 0.05, tab_rgbw 0.04; flow_gray_u8 0.05; tvl1_prepare 0.05.  Filling and comparing 4 to 20 GiB takes tens of
milliseconds at this chip's bandwidth; a test that happens to make the process's first allocation of that size pays 1 to 5 s for it
(resize_nearest here, another test in another run)."""
import ctypes

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


@pytest.mark.parametrize("id", ["quantize_u8/rgb4", "quantize_u8/generic"])
def test_quantize_u8(rt, id):
    case = B.BY_ID[id]
    n, c, h, w = (case.n,) + case.make()[0][0].shape[1:]
    B.run_equal(rt, case, DEV, [((h, w, c), torch.uint8)], lambda x, out: (x.data_ptr(), out.data_ptr(), n, c, h, w))


@pytest.mark.parametrize("id", ["u8_to_f32/rgb4", "u8_to_f32/generic"])
def test_u8_to_f32(rt, id):
    case = B.BY_ID[id]
    n, h, w, c = (case.n,) + case.make()[0][0].shape[1:]
    B.run_equal(rt, case, DEV, [((c, h, w), torch.float32)], lambda x, out: (x.data_ptr(), out.data_ptr(), n, c, h, w))


@pytest.mark.parametrize("id", ["resize_bilinear", "resize_nearest"])
def test_resize(rt, id):
    case = B.BY_ID[id]
    (x,), (want,) = case.make()
    hi, wi, ho, wo = x.shape[2:] + want.shape[2:]
    B.run_equal(rt, case, DEV, [((1, ho, wo), torch.float32)], lambda xd, out: (xd.data_ptr(), out.data_ptr(), case.n, hi, wi, ho, wo))


def test_mask_composite(rt):
    case = B.BY_ID["mask_composite"]
    hw = case.make()[0][0].shape[-1]
    assert case.n % 3 == 0
    B.run_equal(rt, case, DEV, [((1, 1, hw), torch.float32)],
                lambda a, b, m, out: (a.data_ptr(), b.data_ptr(), m.data_ptr(), 3, case.n // 3, out.data_ptr(), case.n // 3, 3, hw))


@pytest.mark.parametrize("id", ["resize_area_u8/linear", "resize_area_u8/2x2_rgb4", "resize_area_u8/tab_rgbw"])
def test_resize_area_u8(rt, id):
    import pixel_ref as R

    case = B.BY_ID[id]
    (x,), (want,) = case.make()
    _p, hi, wi, c = x.shape
    _p, ho, wo, _c = want.shape
    assert R.select_resize_area_u8(hi, wi, c, ho, wo) == id
    B.run_equal(rt, case, DEV, [((ho, wo, c), torch.uint8)], lambda xd, out: (xd.data_ptr(), out.data_ptr(), case.n, hi, wi, c, ho, wo))


def test_flow_gray_u8(rt):
    case = B.BY_ID["flow_gray_u8"]
    (rgb,), (want,) = case.make()
    _p, hi, wi, _c = rgb.shape
    _p, ho, wo = want.shape
    B.run_equal(rt, case, DEV, [((ho, wo), torch.uint8)], lambda x, out: (x.data_ptr(), case.n, hi, wi, out.data_ptr(), ho, wo))


def test_tvl1_prepare(rt):
    import applied_image_processing_amd.tvl1 as tvl1
    import tvl1_ref as TV

    case = B.BY_ID["tvl1_prepare"]
    (gray,), (want,) = case.make()
    _p, h, w = gray.shape
    t = tvl1.TVL1(h, w)
    B.reserve(case, DEV)
    # the P frames alone, held to test_gpu_tvl1.py's bar: rel L2 within max(1e-6, twice the float32 restatement's own)
    small = t.prepare(B.upload(gray, DEV))
    rel = lambda a, b: float(np.linalg.norm(a.astype(np.float64) - b) / max(np.linalg.norm(b), 1e-30))
    for k in range(B.P):
        got = [[x.cpu().numpy() for x in s] for s in t.prepared_views(small[k])]
        r64, r32 = TV.prepare(gray[k]), TV.prepare(gray[k], dtype=np.float32)
        for g, r, f in zip(got, r64, r32):
            for c in range(3):
                assert rel(g[c], r[c]) <= max(1e-6, 2 * rel(f[c], r[c])), (k, c)
    src = B.tile(gray, case.n, DEV)
    out = B.poisoned((case.n, t.frame_floats), torch.float32, DEV)
    try:
        assert src.numel() + out.numel() * 4 == case.total_bytes()
        rt.call("adain_tvl1_prepare", torch.device(DEV), src.data_ptr(), case.n, h, w, ctypes.addressof(t.P), out.data_ptr())
        torch.cuda.synchronize()
        # the padding behind a frame's 256-byte aligned scale blocks is not written: compare the blocks
        off = 0
        for ws_, hs_ in t.scales:
            block = slice(off, off + 4 * ws_ * hs_)
            B.assert_frames(f"tvl1_prepare scale {ws_} x {hs_}", out[:, block], small[:, block].contiguous())
            pad = slice(block.stop, (block.stop + 63) // 64 * 64)
            assert bool((out[:, pad].contiguous().view(torch.uint8) == 0xA5).all()), "the padding behind a scale block was written"
            off = pad.stop
        assert off == t.frame_floats
        B.assert_frames("tvl1_prepare: the gray frames changed", src, gray)
    finally:
        del src, out, small
        B.release()
