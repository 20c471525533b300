"""Far-batch tests of the two PIL resizes (csrc/resample.hip: adain_resize_pil_bilinear_u8; csrc/resample_filters.hip:
adain_resize_pil_u8): one call over 65535 frames whose source, uint8 intermediate (the workspace) and result each pass 2^32 bytes,
every frame compared with Pillow's own ``Image.resize`` of its pattern - equality, the bar of test_gpu_resize_filters.py and
test_gpu_resize_pil.py.  tests/far_batch.py states the design and holds the cases.  Run with ``-m gpu``.

Out of scope here as everywhere in the far-batch tests: the whole-network calls, adain_tvl1_flow / adain_farneback_*, and the
single-frame calls.

Measured on an MI355X, seconds per test (fill, call and comparison):
resize_pil_u8 bicubic_rgb 0.21 (4.88 when it makes the process's first large allocations), lanczos_l 0.16, hamming_rgbx 0.04,
nearest_rgb 0.03; resize_pil_bilinear_u8 0.03."""
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


FILTERS = {"resize_pil_u8/bicubic_rgb": "BICUBIC", "resize_pil_u8/nearest_rgb": "NEAREST", "resize_pil_u8/lanczos_l": "LANCZOS",
           "resize_pil_u8/hamming_rgbx": "HAMMING"}


@pytest.mark.parametrize("id", sorted(FILTERS))
def test_resize_pil_u8(rt, id):
    """Through the C call itself, with the tables ``rt.pil_resize_taps`` builds on the host and a workspace of the query's size."""
    case = B.BY_ID[id]
    (src,), (want,) = case.make()
    _p, hi, wi, pix = src.shape
    _p, ho, wo, c = want.shape
    code = rt.pil_filter(FILTERS[id])
    sizes = dict((b[0], b[2]) for b in case.buffers())
    tables = []
    for a, b in ((wi, wo), (hi, ho)):
        k, bounds, taps = rt.pil_resize_taps(code, a, b)
        tables.append((k, torch.from_numpy(bounds.copy()).to(DEV), torch.from_numpy(taps.copy()).to(DEV) if k else None))
    (kx, bx, tx), (ky, by, ty) = tables
    ptr = lambda t: t.data_ptr() if t is not None else None

    def args(x, out, ws=None):
        return (x.data_ptr(), pix, case.n, hi, wi, out.data_ptr(), ho, wo, code, bx.data_ptr(), ptr(tx), kx, by.data_ptr(), ptr(ty), ky, 0, 0, ho, wo,
                ptr(ws), sizes.get("workspace", 0))

    B.run_equal(rt, case, DEV, [((ho, wo, c), torch.uint8)], args, workspace=sizes["workspace"])


def test_resize_pil_bilinear_u8(rt):
    case = B.BY_ID["resize_pil_bilinear_u8"]
    (src,), (want,) = case.make()
    _p, hi, wi, pix = src.shape
    _p, ho, wo, _c = want.shape
    nbytes = rt.lib().adain_resize_pil_bilinear_u8_workspace_bytes(hi, wi, ho, wo)          # the tap tables: no term in n
    ws = torch.empty(nbytes, dtype=torch.uint8, device=DEV)
    try:
        B.run_equal(rt, case, DEV, [((ho, wo, 3), torch.uint8)],
                    lambda x, out: (x.data_ptr(), pix, case.n, hi, wi, out.data_ptr(), ho, wo, 0, 0, ho, wo, ws.data_ptr(), nbytes))
    finally:
        del ws
        B.release()
