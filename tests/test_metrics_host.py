"""The image metrics without a GPU: the float64 restatement (tests/metrics_ref.py) held to the reference's recorded float32 results
(tests/golden/metrics/cases.npz) within the recorded bars (noise.json), the bars shown to discriminate, the library's window and entries,
the refusals that need no device, and the CPU surface of ``applied_image_processing_amd.metrics``."""
import ctypes
import json
import math
import os
import re

import numpy as np
import pytest
import torch
from PIL import Image

import metrics_cases as C
import metrics_ref as R

NAMES = C.golden_names()
ENTRIES = ("adain_image_metrics_u8_bytes", "adain_image_metrics_u8", "adain_image_metrics_f32_bytes", "adain_image_metrics_f32", "adain_ssim_window")


@pytest.fixture(scope="module")
def z():
    return C.load_golden()


@pytest.fixture(scope="module")
def bars():
    with open(os.path.join(C.GOLDEN, "noise.json")) as f:
        return json.load(f)


@pytest.fixture(scope="module")
def restated(z):
    """name -> tests/metrics_ref.py on the case, computed once."""
    return {name: R.metrics_u8(*C.golden_pair(z, name)) for name in NAMES}


def worst(z, name, got):
    """(per-image, per-element) distance of a restatement's result from the reference's float32 outputs on one case."""
    return (float(np.abs(got["ssim"] - z[name + "_ssim"].astype(np.float64)).max()),
            float(np.abs(got["map"].transpose(0, 3, 1, 2) - z[name + "_map"].astype(np.float64)).max()))


def test_the_fixtures_are_the_cases_and_the_bars_are_the_rule(z, bars):
    assert len(NAMES) == 40
    for family in C.FAMILIES:
        for h, w in C.GOLDEN_SIZES:
            a, b = C.pair(family, 2, h, w, 3)
            assert np.array_equal(z[f"{family}_{h}x{w}_c3_a"], a) and np.array_equal(z[f"{family}_{h}x{w}_c3_b"], b)
    assert all(bars[k] > 0 for k in ("R_frame", "R_map", "S_frame", "S_map"))
    assert bars["bar_frame"] == 2 * max(bars["R_frame"], bars["S_frame"]) and bars["bar_map"] == 2 * max(bars["R_map"], bars["S_map"])
    assert z["window"].dtype == np.float32 and z["window"].view(np.uint32).tolist() == list(R.WINDOW_BITS)


@pytest.mark.parametrize("name", NAMES)
def test_the_restatement_is_within_the_bar_of_the_reference(z, bars, restated, name):
    frame, element = worst(z, name, restated[name])
    print(name, frame, element)
    assert frame <= bars["bar_frame"] and element <= bars["bar_map"]
    # psnr: the reference's float32 mean of n <= 2^13 squares is within (3 + log2 n) 2^-24 of the exact one, relatively; psnr moves by
    # 10 / ln 10 times that, and its own float32 rounding adds half an ulp of at most 128 dB
    want, got = z[name + "_psnr"].astype(np.float64), restated[name]["psnr"]
    for w_, g_ in zip(want, got):
        assert (math.isinf(w_) and math.isinf(g_)) or abs(w_ - g_) <= 4.343 * 16 * 2.0 ** -24 + 2.0 ** -17, (name, w_, g_)


def test_the_bars_discriminate(z, bars):
    """Reflect padding in place of zeros, and the window one tap off centre: each must miss the reference by more than the bar."""
    for kw in (dict(pad="reflect"), dict(shift=1)):
        frame = element = 0.0
        for name in NAMES:
            f, e = worst(z, name, R.metrics_u8(*C.golden_pair(z, name), **kw))
            frame, element = max(frame, f), max(element, e)
        print(kw, frame, element)
        assert frame > bars["bar_frame"] and element > bars["bar_map"], kw


def separable_f32(a, b):
    """The device's form in NumPy float32: a row pass and a column pass of 11 taps, taps in index order, zero padding."""
    g = R.window()
    x, y = (np.pad((v.astype(np.float32) / np.float32(255.0)).transpose(0, 3, 1, 2), [(0, 0), (0, 0), (5, 5), (5, 5)]) for v in (a, b))
    h, w = a.shape[1:3]

    def blur(t):
        rows = np.zeros(t.shape[:3] + (w,), dtype=np.float32)
        for k in range(11):
            rows = rows + g[k] * t[..., k:k + w]
        out = np.zeros(t.shape[:2] + (h, w), dtype=np.float32)
        for k in range(11):
            out = out + g[k] * rows[..., k:k + h, :]
        return out

    c1, c2 = np.float32(R.C1), np.float32(R.C2)
    mu1, mu2 = blur(x), blur(y)
    s1, s2, s12 = blur(x * x) - mu1 * mu1, blur(y * y) - mu2 * mu2, blur(x * y) - mu1 * mu2
    m = ((np.float32(2) * (mu1 * mu2) + c1) * (np.float32(2) * s12 + c2)) / ((mu1 * mu1 + mu2 * mu2 + c1) * (s1 + s2 + c2))
    assert m.dtype == np.float32
    return m.transpose(0, 2, 3, 1)


def test_the_separable_float32_form_stays_inside_the_bars(z, bars, restated):
    frame = element = 0.0
    for name in NAMES:
        a, b = C.golden_pair(z, name)
        m = separable_f32(a, b).astype(np.float64)
        frame = max(frame, float(np.abs(m.mean(axis=(1, 2, 3)) - restated[name]["ssim"]).max()))
        element = max(element, float(np.abs(m - restated[name]["map"]).max()))
        if name.startswith(("noise", "ramp")):          # equal frames run equal operations: exactly 1
            assert np.all(separable_f32(a, a) == np.float32(1.0))
    print(frame, element)
    assert frame <= bars["bar_frame"] and element <= bars["bar_map"]


# ---- the built library and the package, without a GPU ---------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def rt():
    import applied_image_processing_amd.runtime as rt

    rt.lib()
    return rt


def test_the_entries_are_declared_bound_and_exported(rt):
    header = open(os.path.join(os.path.dirname(C.GOLDEN), os.pardir, os.pardir, "include", "adain_hip.h")).read()
    for name in ENTRIES:
        assert re.search(rf"ADAIN_API int {name}\(", header) and name in rt.SIGNATURES and hasattr(rt.lib(), name), name
    assert f"#define ADAIN_METRICS_TILE_X {C.TILE_X}\n" in header and f"#define ADAIN_METRICS_TILE_Y {C.TILE_Y}\n" in header
    assert rt.METRICS_TILE == (C.TILE_Y, C.TILE_X)
    assert rt.lib().adain_abi_version() == 4


def test_the_window_is_the_references_bit_for_bit(rt, z):
    got = np.array(rt.ssim_window(), dtype=np.float32)
    assert got.view(np.uint32).tolist() == z["window"].view(np.uint32).tolist()
    assert rt.lib().adain_ssim_window(None) == -1 and b"ssim_window" in rt.lib().adain_last_error()


def test_the_size_queries_and_the_refusals_that_need_no_device(rt):
    L = rt.lib()
    b = ctypes.c_size_t()
    # 24 bytes per tile, rounded up to 256: 130 x 97 x 3 is 9 x 5 tiles a frame, 97 x 130 x 3 planes is 7 x 3 x 3
    assert rt.image_metrics_sizes(3, 130, 97, 3) == (3 * 9 * 5 * 24 + 255) // 256 * 256
    assert rt.image_metrics_sizes(2, 97, 130, 3, u8=False) == (2 * 3 * 7 * 3 * 24 + 255) // 256 * 256
    assert L.adain_image_metrics_u8_bytes(1, 8, 8, 3, None) == 0 and L.adain_image_metrics_f32_bytes(1, 4, 8, 8, None) == 0
    for dims, word in (((0, 8, 8, 3), b"n "), ((65536, 8, 8, 3), b"n "), ((1, 0, 8, 3), b"h "), ((1, 8, 0, 3), b"w "), ((1, 8, 8, 2), b"c "), ((1, 8, 8, 4), b"c "),
                       ((1, 65536, 65536, 1), b"2^31")):
        assert L.adain_image_metrics_u8_bytes(*dims, ctypes.byref(b)) == -1 and b"image_metrics_u8" in L.adain_last_error() and word in L.adain_last_error(), dims
    for dims, word in (((1, 0, 8, 8), b"c "), ((1, 5, 8, 8), b"c "), ((0, 3, 8, 8), b"n "), ((1, 3, 0, 8), b"h "), ((1, 3, 8, -1), b"w "), ((1, 4, 32768, 32768), b"2^31")):
        assert L.adain_image_metrics_f32_bytes(*dims, ctypes.byref(b)) == -1 and b"image_metrics_f32" in L.adain_last_error() and word in L.adain_last_error(), dims
    buf = ctypes.create_string_buffer(4096)
    p = (ctypes.addressof(buf) + 15) & ~15
    src, out, smap, ws, size = p, p + 1024, p + 2048, p + 3072, rt.image_metrics_sizes(1, 8, 8, 3)
    call = lambda a=src, b=src, n=1, h=8, w=8, c=3, out=out, smap=None, ws=ws, size=size: L.adain_image_metrics_u8(a, b, n, h, w, c, out, smap, ws, size, None)
    for kw, word in ((dict(a=None), b"a is a null"), (dict(b=None), b"b is a null"), (dict(out=None), b"out is a null"), (dict(ws=None), b"workspace"),
                     (dict(c=2), b"c "), (dict(n=0), b"n "), (dict(h=0), b"h "), (dict(w=0), b"w "), (dict(size=size - 1), b"workspace too small"),
                     (dict(ws=ws + 4), b"workspace must be 8-byte aligned"), (dict(out=out + 4), b"out must be 8-byte aligned"), (dict(smap=smap + 2), b"ssim_map must be 4-byte aligned"),
                     (dict(out=src + 8), b"out overlaps a"), (dict(smap=src + 128), b"ssim_map overlaps a"), (dict(ws=src + 8), b"workspace overlaps a"),
                     (dict(b=src + 512, out=src + 512 + 184), b"out overlaps b")):
        assert call(**kw) == -1 and word in L.adain_last_error(), (kw, L.adain_last_error())
    f32 = lambda a=src, b=src, out=out: L.adain_image_metrics_f32(a, b, 1, 3, 4, 4, out, None, ws, size, None)
    for kw, word in ((dict(a=src + 2), b"a must be 4-byte aligned"), (dict(b=src + 1), b"b must be 4-byte aligned"), (dict(out=src + 184), b"out overlaps a")):
        assert f32(**kw) == -1 and b"image_metrics_f32" in L.adain_last_error() and word in L.adain_last_error(), (kw, L.adain_last_error())


# ---- applied_image_processing_amd.metrics on the CPU ------------------------------------------------------------------------------------------
def torch_expression(x, y, window_size=11):
    """The reference's expressions, written out here: (the map [N,C,H,W], psnr [N,1])."""
    g = torch.tensor([math.exp(-(i - window_size // 2) ** 2 / float(2 * 1.5 ** 2)) for i in range(window_size)], dtype=torch.float32)
    g = (g / g.sum()).unsqueeze(1)
    c = x.shape[-3]
    win = g.mm(g.t()).float()[None, None].expand(c, 1, window_size, window_size).contiguous()
    conv = lambda t: torch.nn.functional.conv2d(t, win, padding=window_size // 2, groups=c)
    mu1, mu2 = conv(x), conv(y)
    s1, s2, s12 = conv(x * x) - mu1.pow(2), conv(y * y) - mu2.pow(2), conv(x * y) - mu1 * mu2
    m = ((2 * mu1 * mu2 + 0.01 ** 2) * (2 * s12 + 0.03 ** 2)) / ((mu1.pow(2) + mu2.pow(2) + 0.01 ** 2) * (s1 + s2 + 0.03 ** 2))
    return m, 20 * torch.log10(1.0 / torch.sqrt(((x - y) ** 2).view(x.shape[0], -1).mean(1, keepdim=True)))


@pytest.mark.parametrize("name", [n for n in NAMES if "_12x33_" in n or "_1x1_" in n])
def test_the_cpu_surface_is_torchs_expression(z, name):
    import applied_image_processing_amd.metrics as M

    a, b = C.golden_pair(z, name)
    x, y = torch.from_numpy(C.to_nchw_f32(a)), torch.from_numpy(C.to_nchw_f32(b))
    want_m, want_p = torch_expression(x, y)
    want_s = want_m.mean(1).mean(1).mean(1)
    assert torch.equal(M.ssim(x, y, size_average=False), want_s) and torch.equal(M.ssim(x, y), want_m.mean()) and M.ssim(x, y).dtype == torch.float32
    assert torch.equal(M.psnr(x, y), want_p) and M.psnr(x, y).shape == (2, 1)
    assert torch.equal(M.ssim(x[0], y[0]), torch_expression(x[0], y[0])[0].mean())
    assert torch.equal(M.ssim(x, y, 7, False), torch_expression(x, y, 7)[0].mean(1).mean(1).mean(1))
    assert torch.equal(M.mse(x, y), ((x - y) ** 2).view(2, -1).mean(1, keepdim=True))
    assert torch.equal(M.l1_loss(x, y), (x - y).abs().mean()) and torch.equal(M.l2_loss(x, y), ((x - y) ** 2).mean())
    # and the recorded reference values, to float32's last bits (the recording machine's torch may order a sum differently)
    assert np.allclose(want_s.numpy(), z[name + "_ssim"], rtol=0, atol=1e-6)


def make_scene(root, views=2):
    """root/test/ours_7/{renders,gt}/0000i.png, 23 x 31 noise against itself +-3."""
    a, b = C.pair("near", views, 23, 31, 3, seed=5)
    for sub, frames in (("renders", a), ("gt", b)):
        d = os.path.join(root, "test", "ours_7", sub)
        os.makedirs(d)
        for i, f in enumerate(frames):
            Image.fromarray(f).save(os.path.join(d, f"{i:05d}.png"))
    return a, b


def test_evaluate_writes_the_references_two_files(tmp_path):
    import applied_image_processing_amd.metrics as M

    scene = str(tmp_path / "scene")
    a, b = make_scene(scene)
    M.evaluate([scene], device="cpu")
    results, per_view = json.load(open(os.path.join(scene, "results.json"))), json.load(open(os.path.join(scene, "per_view.json")))
    assert list(results) == ["ours_7"] and sorted(results["ours_7"]) == ["PSNR", "SSIM"]
    assert list(per_view) == ["ours_7"] and sorted(per_view["ours_7"]) == ["PSNR", "SSIM"]
    assert sorted(per_view["ours_7"]["SSIM"]) == sorted(per_view["ours_7"]["PSNR"]) == ["00000.png", "00001.png"]
    want_m, want_p = torch_expression(torch.from_numpy(C.to_nchw_f32(a)), torch.from_numpy(C.to_nchw_f32(b)))
    want_s = want_m.mean(1).mean(1).mean(1)
    assert [per_view["ours_7"]["SSIM"][f"{i:05d}.png"] for i in range(2)] == want_s.tolist()
    assert [per_view["ours_7"]["PSNR"][f"{i:05d}.png"] for i in range(2)] == want_p.reshape(-1).tolist()
    assert results["ours_7"]["SSIM"] == want_s.mean().item() and results["ours_7"]["PSNR"] == want_p.mean().item()
    # a provider adds the third key, and is handed [1,3,h,w] in [0,1]
    seen = []
    M.evaluate([scene], lpips_fn=lambda r, g: seen.append((tuple(r.shape), float(r.max()) <= 1.0)) or 0.25, device="cpu")
    results, per_view = json.load(open(os.path.join(scene, "results.json"))), json.load(open(os.path.join(scene, "per_view.json")))
    assert sorted(results["ours_7"]) == ["LPIPS", "PSNR", "SSIM"] and results["ours_7"]["LPIPS"] == 0.25
    assert per_view["ours_7"]["LPIPS"] == {"00000.png": 0.25, "00001.png": 0.25} and seen == [((1, 3, 23, 31), True)] * 2


def test_the_command_line_runs_the_evaluation(tmp_path):
    import applied_image_processing_amd.metrics as M

    scene = str(tmp_path / "scene")
    make_scene(scene, views=1)
    assert M.main(["-m", scene, "--device", "cpu"]) == 0
    assert sorted(json.load(open(os.path.join(scene, "results.json")))["ours_7"]) == ["PSNR", "SSIM"]
