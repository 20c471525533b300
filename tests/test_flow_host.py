"""CPU tests of the Farneback optical-flow feature (csrc/flow.hip, flow.py): the host-only level schedule against hand-derived
tables, the new C-ABI symbols, the parameter checks, and the NumPy restatement's own known answers (tests/farneback_ref.py)."""
import os

import numpy as np
import pytest

from conftest import ROOT

import farneback_ref as F

import applied_image_processing_amd.runtime as rt

NEW_SYMBOLS = ["adain_flow_gray_u8", "adain_farneback_levels", "adain_farneback_pyramid_bytes", "adain_farneback_workspace_bytes",
               "adain_farneback_expand", "adain_farneback_flow"]

# (w, h, ksize, sigma) coarse to fine: the reference's video size, 1080p, the existing video test's size
TABLES = {
    (256, 256): [(32, 32, 19, 3.5), (64, 64, 9, 1.5), (128, 128, 3, 0.5), (256, 256, 3, 0.0)],
    (1920, 1080): [(60, 34, 79, 15.5), (120, 68, 39, 7.5), (240, 135, 19, 3.5), (480, 270, 9, 1.5), (960, 540, 3, 0.5),
                   (1920, 1080, 3, 0.0)],
    (64, 36): [(64, 36, 3, 0.0)],
    # odd sizes: cvRound's half-to-even (127.5 -> 128, 165.5 -> 166, 82.75 -> 83); 33 and 31 fall below 32 at the first halving
    (255, 331): [(64, 83, 9, 1.5), (128, 166, 3, 0.5), (255, 331, 3, 0.0)],
    (33, 33): [(33, 33, 3, 0.0)],
    (31, 100): [(31, 100, 3, 0.0)],
}


def _lib():
    if not os.path.exists(rt.LIB_PATH):
        import __graft_entry__ as g

        g.build()
    return rt.lib()


@pytest.mark.parametrize("wh", sorted(TABLES))
def test_level_schedule_matches_the_hand_derived_table(wh):
    from applied_image_processing_amd import flow

    _lib()
    w, h = wh
    got = flow.level_schedule(h, w, 0.5, 5)[::-1]
    assert [(a, b, c) for a, b, c, _ in got] == [(a, b, c) for a, b, c, _ in TABLES[wh]]
    assert np.allclose([s for *_, s in got], [s for *_, s in TABLES[wh]], rtol=0, atol=1e-12)
    assert [t[:3] for t in F.level_schedule(h, w)[::-1]] == [t[:3] for t in TABLES[wh]]
    assert flow.pyramid_bytes(h, w) == 4 * sum((x * y + 63) // 64 * 64 + (5 * x * y + 63) // 64 * 64 for x, y, *_ in TABLES[wh])


def test_levels_parameter_edge_cases():
    from applied_image_processing_amd import flow

    _lib()
    assert len(flow.level_schedule(1080, 1920, 0.5, 0)) == 1          # levels=0: the full-size level only
    assert len(flow.level_schedule(1080, 1920, 0.5, 2)) == 3          # capped by the request, not by the size
    assert [t[:2] for t in flow.level_schedule(100, 100, 0.8, 5)] == [(100, 100), (80, 80), (64, 64), (51, 51), (41, 41), (33, 33)]
    with pytest.raises(ValueError):
        flow.level_schedule(100, 100, 1.0, 5)


def test_new_symbols_are_exported_and_bound():
    lib = _lib()
    header = open(os.path.join(ROOT, "include", "adain_hip.h")).read()
    for name in NEW_SYMBOLS:
        assert f"{name}(" in header and name in rt.SIGNATURES and hasattr(lib, name)
    assert lib.adain_abi_version() == 4
    assert lib.adain_farneback_workspace_bytes(1080, 1920) == 14 * 1080 * 1920 * 4
    assert lib.adain_farneback_pyramid_bytes(256, 256, 1.5, 5) == 0


def test_flow_module_imports_and_refuses_what_is_not_built():
    from applied_image_processing_amd import flow, video

    _lib()
    ok = dict(flow.DEFAULTS)
    flow.check_params(**ok)
    for bad in (dict(flags=flow.OPTFLOW_FARNEBACK_GAUSSIAN), dict(flags=flow.OPTFLOW_USE_INITIAL_FLOW), dict(pyr_scale=1.0),
                dict(pyr_scale=0.0), dict(poly_n=3), dict(poly_n=6), dict(winsize=1), dict(winsize=64), dict(iterations=0)):
        with pytest.raises(ValueError):
            flow.check_params(**{**ok, **bad})
        with pytest.raises(ValueError):
            flow.FlowSequence(**{**ok, **bad})
    import torch

    g = torch.zeros(36, 64, dtype=torch.uint8)
    with pytest.raises(ValueError, match="flow=None"):
        flow.calc_optical_flow_farneback(g, g, torch.zeros(36, 64, 2))
    with pytest.raises(ValueError, match="flags"):
        flow.calc_optical_flow_farneback(g, g, None, 0.5, 5, 15, 3, 7, 1.5, 256)
    with pytest.raises(ValueError, match="DualTV-L1"):
        video.device_flow_provider("a.png", "b.png", (64, 36), "dualtvl1")
    # the C ABI refuses the same values on its own (no device needed: checked before any launch)
    lib = _lib()
    ws = rt.lib().adain_farneback_workspace_bytes(36, 64)
    assert lib.adain_farneback_flow(8, 8, 36, 64, 0.5, 5, 15, 3, 256, 8, 8, ws, None) == -1
    assert b"flags" in lib.adain_last_error()
    assert lib.adain_farneback_expand(8, 36, 64, 0.5, 5, 6, 1.5, 8, 8, ws, None) == -1
    assert b"poly_n" in lib.adain_last_error()
    assert lib.adain_farneback_flow(8, 8, 36, 64, 1.0, 5, 15, 3, 0, 8, 8, ws, None) == -1
    assert b"pyr_scale" in lib.adain_last_error()
    assert lib.adain_farneback_flow(8, 8, 36, 64, 0.5, 5, 15, 3, 0, 8, 8, ws - 1, None) == -1
    assert b"workspace" in lib.adain_last_error()


@pytest.mark.parametrize("hw", [(64, 64), (96, 128)])
def test_restatement_known_answers(hw):
    """The float64 restatement: identical constant frames give a flow of exactly 0; identical textured frames give a flow that is
    not exactly 0 - OpenCV's "else" branch of the matrix update (floor(x+dx) = w-1 or floor(y+dy) = h-1: the last column and row at
    zero flow) leaves a residual there that the box blur and the iterations carry inwards - but small; a band-limited texture
    translated by a sub-pixel amount gives that translation in the interior."""
    h, w = hw
    c = np.full((h, w), 97, np.uint8)
    assert np.abs(F.farneback(c, c)).max() == 0.0 and np.abs(F.farneback(c, c, dtype=np.float32)).max() == 0.0
    a = F.texture(h, w, seed=3)
    e = F.endpoint_error(F.farneback(a, a), np.zeros((2, h, w)))
    assert np.median(e) < 1e-4 and e.max() < 0.2
    for shift in [(0.6, -0.3), (1.7, 1.2)]:
        f = F.farneback(a, F.texture(h, w, shift, seed=3))
        e = F.endpoint_error(f, np.array(shift)[:, None, None])[16:-16, 16:-16]
        assert np.median(e) < 0.05 and np.percentile(e, 95) < 0.15, (shift, np.median(e), np.percentile(e, 95))
    # float32 mode: the noise floor of a float implementation, far below the method's own error
    b = F.texture(h, w, (0.6, -0.3), seed=3)
    d = F.endpoint_error(F.farneback(a, b, dtype=np.float32), F.farneback(a, b))
    assert np.median(d) < 1e-4


def test_restatement_frame_to_gray_integer_rules():
    rng = np.random.default_rng(0)
    rgb = rng.integers(0, 256, (20, 30, 3), dtype=np.uint8)
    g = F.frame_to_gray(rgb, 30, 20)                                        # equal size: the conversion alone
    v = rgb.astype(np.int64)
    want = (4899 * v[..., 2] + 9617 * v[..., 1] + 1868 * v[..., 0] + 8192) >> 14
    assert np.array_equal(g, want)
    half = F.resize_linear_u8(rgb, 15, 10)                                  # exact 2x: INTER_AREA's 2x2 mean
    assert np.array_equal(half, (rgb[0::2, 0::2].astype(int) + rgb[0::2, 1::2] + rgb[1::2, 0::2] + rgb[1::2, 1::2] + 2) >> 2)
    flat = np.full((20, 30, 3), 77, np.uint8)                               # constant frames stay constant in the fixed point
    for wo, ho in [(17, 9), (64, 36), (31, 20)]:
        assert (F.resize_linear_u8(flat, wo, ho) == 77).all()
