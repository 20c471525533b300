"""runtime.image_metrics (csrc/metrics.hip) against the float64 restatement tests/metrics_ref.py: the per-frame SSIM within bar_frame and
every map element within bar_map of tests/golden/metrics/noise.json, the uint8 mse and l1 equal to the exact integer ratios, equal frames
scoring exactly 1 / 0 / 0 / +inf, and the records the same bits with the map and without it.  Both entries, c = 1 and c = 3, the golden
cases and seeded shapes around the kernel's tile."""
import json
import math
import os

import numpy as np
import pytest
import torch

import metrics_cases as C
import metrics_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
F32_REL = 8 * 2.0 ** -24          # float-input mse, l1: one float32 rounding of the difference, squared, with room to spare
# psnr = 20 log10(1 / sqrt(mse)) in float64 from an mse that is within `rel` of the restatement's: 10 / ln 10 times rel, and a few ulps of
# the device's log10 at up to 2^7 dB
PSNR_OF_REL = 10 / math.log(10)
PSNR_ULPS = 8 * 2.0 ** -46


@pytest.fixture(scope="module")
def rt():
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    import applied_image_processing_amd.runtime as rt

    rt.lib()
    torch.cuda.set_device(0)
    return rt


@pytest.fixture(scope="module")
def bars():
    with open(os.path.join(C.GOLDEN, "noise.json")) as f:
        return json.load(f)


@pytest.fixture(scope="module")
def z():
    return C.load_golden()


def records(got):
    torch.cuda.synchronize()
    return got.records.cpu().numpy()


def check_u8(rt, bars, a, b):
    """Both calls (with the map, without it) of the uint8 entry on a, b [n,h,w,c] against the restatement."""
    want = R.metrics_u8(a, b)
    x, y = torch.from_numpy(a).to(DEV), torch.from_numpy(b).to(DEV)
    with_map, without = rt.image_metrics(x, y, ssim_map=True), rt.image_metrics(x, y)
    got, smap = records(with_map), with_map.ssim_map.cpu().numpy()
    assert without.ssim_map is None and smap.shape == a.shape and smap.dtype == np.float32
    assert np.array_equal(got.view(np.uint64), records(without).view(np.uint64)), "the records differ between the call with the map and the call without"
    print("ssim", np.abs(got[:, 0] - want["ssim"]).max(), "map", np.abs(smap - want["map"]).max())
    assert np.abs(got[:, 0] - want["ssim"]).max() <= bars["bar_frame"]
    assert np.abs(smap.astype(np.float64) - want["map"]).max() <= bars["bar_map"]
    assert got[:, 1].tolist() == want["mse"].tolist() and got[:, 2].tolist() == want["l1"].tolist()          # exact
    for g, w in zip(got[:, 3], want["psnr"]):
        assert g == w if math.isinf(w) else abs(g - w) <= PSNR_ULPS * 128, (g, w)
    # the map's float64 mean is the record's ssim
    assert np.abs(smap.astype(np.float64).reshape(len(a), -1).mean(axis=1) - got[:, 0]).max() <= 1e-12


def check_f32(rt, bars, a, b):
    """The float32 entry on a, b float32 [n,c,h,w]."""
    want = R.metrics_f32(a, b)
    x, y = torch.from_numpy(a).to(DEV), torch.from_numpy(b).to(DEV)
    with_map, without = rt.image_metrics(x, y, ssim_map=True), rt.image_metrics(x, y)
    got, smap = records(with_map), with_map.ssim_map.cpu().numpy()
    assert smap.shape == a.shape and np.array_equal(got.view(np.uint64), records(without).view(np.uint64))
    print("ssim", np.abs(got[:, 0] - want["ssim"]).max(), "map", np.abs(smap - want["map"]).max())
    assert np.abs(got[:, 0] - want["ssim"]).max() <= bars["bar_frame"]
    assert np.abs(smap.astype(np.float64) - want["map"]).max() <= bars["bar_map"]
    for col, key in ((1, "mse"), (2, "l1")):
        assert np.all(np.abs(got[:, col] - want[key]) <= F32_REL * want[key]), key
    for g, w in zip(got[:, 3], want["psnr"]):
        assert g == w if math.isinf(w) else abs(g - w) <= PSNR_OF_REL * F32_REL + PSNR_ULPS * 128, (g, w)


@pytest.mark.parametrize("name", C.golden_names())
def test_the_golden_cases_through_both_entries(rt, bars, z, name):
    a, b = C.golden_pair(z, name)
    check_u8(rt, bars, a, b)
    check_f32(rt, bars, C.to_nchw_f32(a), C.to_nchw_f32(b))


@pytest.mark.parametrize("c", [1, 3])
@pytest.mark.parametrize("family,h,w", C.TILE_SHAPES, ids=[f"{f}-{h}x{w}" for f, h, w in C.TILE_SHAPES])
def test_three_pairs_of_shapes_around_the_tile(rt, bars, family, h, w, c):
    a, b = C.pair(family, 3, h, w, c, seed=1)
    check_u8(rt, bars, a, b)
    # the float entry sees w samples a row where the packed entry saw w c, and unscaled, unclamped values
    fa, fb = C.to_nchw_f32(a), C.to_nchw_f32(b)
    check_f32(rt, bars, fa, fb)


def test_four_channels_and_values_outside_the_unit_range(rt, bars):
    a, b = C.pair("near", 2, 17, 66, 1, seed=2)
    rng = np.random.default_rng(3)
    fa = np.ascontiguousarray(np.concatenate([C.to_nchw_f32(a)] * 4, axis=1) + rng.uniform(-0.5, 0.5, (2, 4, 17, 66)).astype(np.float32))
    fb = np.ascontiguousarray(fa + rng.uniform(-0.02, 0.02, fa.shape).astype(np.float32))
    check_f32(rt, bars, fa, fb)


@pytest.mark.parametrize("family", ["noise", "ramp", "flat"])
@pytest.mark.parametrize("c", [1, 3])
def test_a_frame_against_itself_scores_exactly(rt, family, c):
    a, _ = C.pair(family, 2, 2 * C.TILE_Y + 3, C.TILE_X + 9, c, seed=4)
    for frames in (a, C.to_nchw_f32(a)):
        x = torch.from_numpy(frames).to(DEV)
        for y in (x, x.clone()):
            got = rt.image_metrics(x, y, ssim_map=True)
            rec = records(got)
            assert rec[:, 0].tolist() == [1.0, 1.0] and rec[:, 1].tolist() == [0.0, 0.0] and rec[:, 2].tolist() == [0.0, 0.0]
            assert rec[:, 3].tolist() == [math.inf, math.inf]
            assert bool((got.ssim_map == 1.0).all())


def test_the_value_and_the_refused_inputs(rt):
    a, b = C.pair("near", 2, 9, 12, 3)
    x, y = torch.from_numpy(a).to(DEV), torch.from_numpy(b).to(DEV)
    got = rt.image_metrics(x, y)
    assert all(t.shape == (2,) and t.dtype == torch.float64 and t.is_cuda for t in (got.ssim, got.mse, got.l1, got.psnr))
    one = rt.image_metrics(x[0], y[0], ssim_map=True)
    assert one.ssim.shape == (1,) and one.ssim_map.shape == (9, 12, 3) and torch.equal(one.records[0], got.records[0])
    for bad in ((x.cpu(), y.cpu()), (x, y[:1]), (x[..., :2], y[..., :2]), (x.to(torch.float16), y.to(torch.float16)), (x.float(), y),
                (torch.zeros(1, 5, 4, 4, device=DEV), torch.zeros(1, 5, 4, 4, device=DEV))):
        with pytest.raises(rt.AdainHipError):
            rt.image_metrics(*bad)
