"""One far-batch case of the palette refinement (csrc/quantize_refine.hip): adain_quantize_palette_u8 in global mode with
ADAIN_QUANTIZE_REFINE(1), K = 16, on the source of tests/far_batch.py's quantize_palette_u8/global - 65535 frames of 128 x 176 whose frame
i holds pattern i % 7: 1.48 G pixels, 4.12 GiB, inside one palette.  What can go wrong there is a 32-bit pixel index or byte offset in the
assign kernel, or a 32-bit count or sum in its accumulators.  The expected palette is the restatement's over the seven patterns' colours
with their multiplicities (tests/quantize_refine_ref.py ``palette_weighted``, pinned to the built-out clip in
test_quantize_refine_host.py): equality, as everywhere in this feature.  far_batch.py's helpers are imported; it gains no row."""
import numpy as np
import pytest
import torch

import far_batch as B
import quantize_refine_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
K, T = 16, 1


@pytest.fixture(scope="module")
def rt():
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    import applied_image_processing_amd.runtime as rt

    rt.lib()
    torch.cuda.set_device(0)
    return rt


def test_quantize_palette_global_refined(rt):
    case = B.BY_ID["quantize_palette_u8/global"]
    (frames,), _ = case.make()
    n = case.n
    weights = [n // B.P + (1 if k < n % B.P else 0) for k in range(B.P)]
    pal, used = R.palette_weighted(frames, weights, K, T)
    before, _ = R.palette_weighted(frames, weights, K, 0)
    assert not np.array_equal(pal, before), "the round is meant to move the palette"
    src_bytes = n * 3 * B.H * B.W
    nbytes = rt.quantize_palette_sizes(n, B.H, B.W, False, T)
    assert src_bytes > B.TWO32 and n * B.H * B.W < B.TWO32 and src_bytes + nbytes + 2 * B.PIECE <= B.CAP
    torch.cuda.empty_cache()
    free, _total = torch.cuda.mem_get_info(DEV)
    assert free >= src_bytes + nbytes + 2 * B.PIECE, f"needs {(src_bytes + nbytes + 2 * B.PIECE) >> 20} MiB of device memory, {free >> 20} MiB are free"
    src = B.tile(frames, n, DEV)
    out_p, out_u = B.poisoned((256, 3), torch.uint8, DEV), B.poisoned((1,), torch.int32, DEV)
    ws = B.poisoned((nbytes,), torch.uint8, DEV)
    try:
        assert src.numel() == src_bytes
        rt.call(case.call, torch.device(DEV), src.data_ptr(), n, B.H, B.W, K, 0 | T << 8, out_p.data_ptr(), out_u.data_ptr(), ws.data_ptr(), ws.numel())
        torch.cuda.synchronize()
        assert out_u.cpu().tolist() == [used]
        got = out_p.cpu().numpy()
        assert np.array_equal(got, pal), f"entries {np.flatnonzero((got != pal).any(axis=1))[:8].tolist()} differ from the weighted restatement's"
        B.assert_frames("the frames changed", src, frames)
    finally:
        del src, out_p, out_u, ws
        B.release()
