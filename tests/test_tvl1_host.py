"""CPU tests of the Dual TV-L1 optical-flow feature (csrc/tvl1.hip, tvl1.py, video.device_flow_provider_all): the host-only scale
list against hand-derived tables, the new C-ABI symbols, the refused parameters, and the NumPy restatement's own rules
(tests/tvl1_ref.py)."""
import ctypes
import os

import numpy as np
import pytest

from conftest import ROOT

import tvl1_ref as T

import applied_image_processing_amd.runtime as rt

NEW_SYMBOLS = ["adain_tvl1_scales", "adain_tvl1_frame_bytes", "adain_tvl1_prepare", "adain_tvl1_workspace_bytes", "adain_tvl1_flow"]

# (w, h) -> [(w_s, h_s)] with the defaults (nscales 5, scaleStep 0.8): cvRound half to even of the previous level's size * 0.8
SCALES = {
    (64, 36): [(64, 36), (51, 29), (41, 23), (33, 18)],
    (256, 256): [(256, 256), (205, 205), (164, 164), (131, 131), (105, 105)],
    (1920, 1080): [(1920, 1080), (1536, 864), (1229, 691), (983, 553), (786, 442)],
    (16, 16): [(16, 16)],
}


def _lib():
    if not os.path.exists(rt.LIB_PATH):
        import __graft_entry__ as g

        g.build()
    return rt.lib()


@pytest.mark.parametrize("wh", sorted(SCALES))
def test_scale_list_matches_the_worked_examples(wh):
    from applied_image_processing_amd import tvl1

    _lib()
    w, h = wh
    assert tvl1.scales(h, w) == SCALES[wh]
    assert T.scales(h, w) == SCALES[wh]
    P = tvl1.check_params()
    assert rt.lib().adain_tvl1_frame_bytes(h, w, ctypes.addressof(P)) == 4 * sum((4 * x * y + 63) // 64 * 64 for x, y in SCALES[wh])
    assert tvl1.scales(h, w, nscales=2) == SCALES[wh][:2]
    assert tvl1.scales(h, w, nscales=1) == SCALES[wh][:1]


def test_new_symbols_are_exported_and_bound():
    lib = _lib()
    header = open(os.path.join(ROOT, "include", "adain_hip.h")).read()
    for name in NEW_SYMBOLS:
        assert f"{name}(" in header and name in rt.SIGNATURES and hasattr(lib, name)
    assert "typedef struct adain_tvl1_params" in header
    assert lib.adain_abi_version() == 4


REFUSED = [(dict(gamma=0.1), "gamma"), (dict(useInitialFlow=True), "useInitialFlow"), (dict(medianFiltering=2), "medianFiltering"),
           (dict(medianFiltering=7), "medianFiltering"), (dict(medianFiltering=4), "medianFiltering"), (dict(nscales=0), "nscales"),
           (dict(warps=-1), "warps"), (dict(innerIterations=-1), "innerIterations"), (dict(scaleStep=1.5), "scaleStep"),
           (dict(scaleStep=0.0), "scaleStep")]


@pytest.mark.parametrize("bad,word", REFUSED)
def test_refused_parameters_python_and_c_abi(bad, word):
    import torch

    from applied_image_processing_amd import flow, tvl1

    lib = _lib()
    with pytest.raises(ValueError, match=word):
        tvl1.check_params(**bad)
    with pytest.raises(ValueError, match=word):
        flow.DualTVL1OpticalFlow_create(**bad)
    with pytest.raises(ValueError, match=word):
        tvl1.TVL1Sequence(**bad)
    # the C ABI refuses the same values on its own, before any launch (no device needed)
    ok = tvl1.check_params()
    P = tvl1.Params(*[getattr(ok, f) for f, _ in tvl1.Params._fields_])
    for k, v in bad.items():
        setattr(P, k, int(v) if isinstance(v, bool) else v)
    ws = 1 << 30
    assert lib.adain_tvl1_flow(8, 8, 1, 36, 64, ctypes.addressof(P), 8, None, 8, ws, None) == -1
    assert word.encode() in lib.adain_last_error()
    assert lib.adain_tvl1_prepare(8, 1, 36, 64, ctypes.addressof(P), 8, None) == -1
    assert word.encode() in lib.adain_last_error()
    assert lib.adain_tvl1_workspace_bytes(36, 64, 1, ctypes.addressof(P)) == 0
    assert lib.adain_tvl1_frame_bytes(36, 64, ctypes.addressof(P)) == 0
    g = torch.zeros(36, 64, dtype=torch.uint8)
    with pytest.raises(ValueError, match="flow=None"):
        flow.DualTVL1OpticalFlow_create().calc(g, g, torch.zeros(36, 64, 2))


def test_c_abi_checks_sizes_and_workspace():
    from applied_image_processing_amd import tvl1

    lib = _lib()
    P = tvl1.check_params()
    need = lib.adain_tvl1_workspace_bytes(36, 64, 3, ctypes.addressof(P))
    assert need > 3 * 16 * 36 * 64 * 4
    assert lib.adain_tvl1_flow(8, 8, 3, 36, 64, ctypes.addressof(P), 8, None, 8, need - 1, None) == -1
    assert b"workspace" in lib.adain_last_error()
    assert lib.adain_tvl1_flow(8, 8, 0, 36, 64, ctypes.addressof(P), 8, None, 8, need, None) == -1
    assert lib.adain_tvl1_scales(2, 64, ctypes.addressof(P), None, None) == -1
    assert b"frame size" in lib.adain_last_error()
    assert lib.adain_tvl1_flow(8, 8, 1, 36, 64, None, 8, None, 8, need, None) == -1


def test_restatement_divergence_and_forward_gradient_borders():
    v1 = np.array([[1., 2., 4.], [8., 16., 32.]])
    v2 = np.array([[3., 5., 7.], [11., 13., 17.]])
    d = T.divergence(v1, v2)
    assert d[0, 0] == 1 + 3                               # corner: the values themselves
    assert d[0, 1] == (2 - 1) + 5 and d[0, 2] == (4 - 2) + 7     # row 0: p2 itself
    assert d[1, 0] == (8 + 11) - 3                        # column 0: p1 itself
    assert d[1, 2] == (32 - 16) + (17 - 7)
    dx, dy = T.forward_gradient(v1)
    assert (dx[:, -1] == 0).all() and (dy[-1, :] == 0).all()
    assert dx[0, 0] == 1 and dx[1, 1] == 16 and dy[0, 2] == 28


def test_restatement_cubic_taps():
    assert T.CUBIC.dtype == np.float32 and T.CUBIC.shape == (32, 4)
    assert T.CUBIC[0].tolist() == [0.0, 1.0, 0.0, 0.0]
    assert np.allclose(T.CUBIC.sum(axis=1), 1.0, rtol=0, atol=1e-6)
    assert np.allclose(T.CUBIC[16], [-0.09375, 0.59375, 0.59375, -0.09375], atol=1e-7)   # Keys A = -0.75 at 1/2
    # at zero flow the remap is the identity, bit for bit
    I = T.texture(20, 24, seed=1).astype(np.float32)
    ys, xs = np.mgrid[0:20, 0:24].astype(np.float32)
    assert np.array_equal(T.remap_cubic([I], xs, ys, np.float32)[0], I)


def test_restatement_replicate_median():
    rng = np.random.default_rng(0)
    u = rng.standard_normal((9, 11))
    m = T.median(u, 5)
    pad = np.pad(u, 2, mode="edge")
    for y in range(9):
        for x in range(11):
            assert m[y, x] == np.sort(pad[y:y + 5, x:x + 5].ravel())[12]
    assert np.array_equal(T.median(u, 3)[4, 5], np.sort(u[3:6, 4:7].ravel())[4])


def test_restatement_identical_and_constant_frames_give_zero_flow():
    a = T.texture(36, 64, seed=3)
    for f, dt in [(a, np.float64), (a, np.float32), (np.full((36, 64), 77, np.uint8), np.float64)]:
        flow, iters, _ = T.tvl1(f, f, dtype=dt)
        assert np.count_nonzero(flow) == 0
        assert (iters == 1).all()                         # the first step's error is 0: every warp stops at once


def test_device_flow_provider_all_refuses_an_unknown_method():
    from applied_image_processing_amd import video

    with pytest.raises(ValueError, match="unknown optical-flow method"):
        video.device_flow_provider_all("a.png", "b.png", (64, 36), "lucas-kanade")


def test_unknown_method_is_refused_before_any_frame_is_stylised(tmp_path):
    """With device_flow_provider_all installed, an unknown flow_method stops the job in its status word, before the engine is built
    or a frame is stylised: the checkpoint paths here do not exist and no GPU is needed."""
    from PIL import Image

    from applied_image_processing_amd import video

    cdir, sdir = tmp_path / "frames", tmp_path / "styles"
    cdir.mkdir(); sdir.mkdir()
    for i in range(2):
        Image.fromarray(np.full((8, 8, 3), 40 * i, np.uint8)).save(cdir / f"frame_{i}.png")
    Image.fromarray(np.zeros((8, 8, 3), np.uint8)).save(sdir / "style.png")
    video.set_flow_provider(video.device_flow_provider_all)
    try:
        with pytest.raises(ValueError, match="unknown optical-flow method"):
            video.apply_style_transfer_multi_ada(str(cdir), str(sdir), str(tmp_path / "out"), flow_method="lucas-kanade",
                                                 vgg_str=str(tmp_path / "missing_vgg.pth"), decoder_str=str(tmp_path / "missing_dec.pth"))
    finally:
        video.set_flow_provider(None)
    assert not list((tmp_path / "out").glob("*.png"))


def test_farneback_provider_refuses_dualtvl1_before_any_frame_is_stylised(tmp_path):
    """device_flow_provider serves 'farneback' only: 'dualtvl1' stops the job in its status word, as an unknown method does with
    device_flow_provider_all, before the engine is built."""
    from PIL import Image

    from applied_image_processing_amd import video

    cdir, sdir = tmp_path / "frames", tmp_path / "styles"
    cdir.mkdir(); sdir.mkdir()
    for i in range(2):
        Image.fromarray(np.full((8, 8, 3), 40 * i, np.uint8)).save(cdir / f"frame_{i}.png")
    Image.fromarray(np.zeros((8, 8, 3), np.uint8)).save(sdir / "style.png")
    video.set_flow_provider(video.device_flow_provider)
    try:
        with pytest.raises(ValueError, match="DualTV-L1"):
            video.apply_style_transfer_multi_ada(str(cdir), str(sdir), str(tmp_path / "out"), flow_method="dualtvl1",
                                                 vgg_str=str(tmp_path / "missing_vgg.pth"), decoder_str=str(tmp_path / "missing_dec.pth"))
    finally:
        video.set_flow_provider(None)
    assert not list((tmp_path / "out").glob("*.png"))
