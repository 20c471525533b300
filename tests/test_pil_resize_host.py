"""Host tests of the six-filter Pillow resize (no GPU): tests/pil_resize_ref.py - the rules in plain Python - equals ``Image.resize``;
the library's ``adain_pil_resize_taps``, in a process that sees no device, returns exactly the restatement's tables; the refusals and a
handful of answers of the two size queries are pinned."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest
from PIL import Image

import pil_resize_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NO_DEVICE = {"HIP_VISIBLE_DEVICES": "-1", "CUDA_VISIBLE_DEVICES": "-1"}
FILTERS = list(R.FILTERS.items())
IDS = [name for name, _ in FILTERS]
# in -> out: one pixel, from one, to one, a factor-99 shrink whose windows clamp at both ends, unchanged, enlarging, the largest shrink
AXES = [(1, 1), (1, 7), (7, 1), (640, 6), (300, 300), (100, 333), (3000, 12), (256, 1)]
# (h, w) -> (width, height): the GPU test's named shapes
NAMED = [((1, 1), (1, 1)), ((1, 1), (3, 5)), ((7, 5), (1, 1)), ((31, 57), (20, 31)), ((31, 57), (57, 9)), ((64, 48), (123, 200)),
         ((270, 480), (455, 256)), ((200, 300), (3, 2)), ((3, 3000), (12, 3))]


@pytest.fixture(scope="module")
def rt():
    import applied_image_processing_amd.runtime as rt

    rt.lib()
    return rt


def pil_resize(a, size, f):
    return np.asarray(Image.fromarray(a).resize(size, f))


def test_the_codes_are_pillows():
    assert {name: int(getattr(Image.Resampling, name)) for name in R.FILTERS} == R.FILTERS
    assert sorted(R.FILTERS.values()) == list(range(6))


@pytest.mark.parametrize("name,f", FILTERS, ids=IDS)
def test_the_restatement_is_pillow_on_the_named_shapes(name, f):
    for hw, size in NAMED:
        a = R.picture(5, *hw)
        assert np.array_equal(R.resize(a, size, f), pil_resize(a, size, f)), (hw, size)
        grey = np.ascontiguousarray(a[..., 2])
        assert np.array_equal(R.resize(grey, size, f), pil_resize(grey, size, f)), (hw, size, "L")


@pytest.mark.parametrize("name,f", FILTERS, ids=IDS)
def test_the_restatement_is_pillow_on_300_random_pairs(name, f):
    g = np.random.default_rng(20261020 + f)
    bad = []
    for case in range(300):
        hi, wi, ho, wo = (int(v) for v in g.integers(1, 130, 4))
        if case % 4 == 0:          # shrinks down to 1/20
            ho, wo = max(1, int(hi / g.uniform(1.0, 20.0))), max(1, int(wi / g.uniform(1.0, 20.0)))
        elif case % 4 == 1:        # one axis unchanged
            ho, wo = (hi, wo) if case % 8 == 1 else (ho, wi)
        a = R.picture(case, hi, wi)
        if case % 3 == 2:
            a = np.ascontiguousarray(a[..., 0])
        if not np.array_equal(R.resize(a, (wo, ho), f), pil_resize(a, (wo, ho), f)):
            bad.append((hi, wi, ho, wo, a.ndim))
    assert not bad, (len(bad), bad[:10])


def test_the_hamming_window_constants_are_floats():
    """Resample.c writes the window as 0.54f + 0.46f * cos(x): floats, widened to double.  With the doubles 0.54 and 0.46 the centre tap
    of 9 -> 3 is one unit of 2^-22 higher, and this row - 255 under that tap, the sum just under a rounding step - comes out 168 where
    Pillow, and the float constants, give 167."""
    row = np.array([[0, 0, 219, 62, 255, 137, 109, 204, 0]], np.uint8)
    _, bounds, kk = R.taps(R.HAMMING, 9, 3)
    assert bounds[1].tolist() == [2, 6] and kk[1, :6].tolist() == [212512, 1055706, 1657868, 1055706, 212512, 0]
    saved = R._F32_054, R._F32_046
    try:
        R._F32_054, R._F32_046 = 0.54, 0.46
        assert R.taps(R.HAMMING, 9, 3)[2][1, 2] == 1657869 and R.resize(row, (3, 1), R.HAMMING)[0, 1] == 168
    finally:
        R._F32_054, R._F32_046 = saved
    assert R.resize(row, (3, 1), R.HAMMING)[0, 1] == 167 == pil_resize(row, (3, 1), R.HAMMING)[0, 1]


def _tables_without_a_device(tmp_path):
    """{(filter, in, out): (ksize, bounds, taps)} from the library, asked in a process of its own that finds no device."""
    path = str(tmp_path / "tables.npz")
    prog = ("import sys, numpy as np\n"
            f"sys.path.insert(0, {ROOT!r})\n"
            "sys.dont_write_bytecode = True\n"
            "import applied_image_processing_amd.runtime as rt\n"
            "import torch\n"
            "assert not torch.cuda.is_available()\n"
            "out = {}\n"
            f"for f in range(6):\n    for a, b in {AXES!r}:\n"
            "        k, bounds, taps = rt.pil_resize_taps(f, a, b)\n"
            "        out[f'{f}_{a}_{b}_k'] = np.int64(k); out[f'{f}_{a}_{b}_b'] = bounds; out[f'{f}_{a}_{b}_t'] = taps\n"
            f"np.savez({path!r}, **out)\n")
    run = subprocess.run([sys.executable] + (["-s"] if sys.flags.no_user_site else []) + ["-c", prog], capture_output=True, text=True,
                         env={**os.environ, **NO_DEVICE})
    assert run.returncode == 0, run.stderr[-2000:]
    return np.load(path)


def test_the_librarys_tables_are_the_restatements(tmp_path):
    got = _tables_without_a_device(tmp_path)
    for name, f in FILTERS:
        for a, b in AXES:
            ksize, bounds, taps = R.taps(f, a, b)
            key = f"{f}_{a}_{b}"
            assert int(got[key + "_k"]) == ksize, (name, a, b)
            assert got[key + "_b"].dtype == np.int32 and np.array_equal(got[key + "_b"], bounds), (name, a, b)
            assert got[key + "_t"].shape == (b, ksize) and np.array_equal(got[key + "_t"], taps), (name, a, b)
    # what the tables look like: the factor-99 shrink clamps its first and last windows, NEAREST has no taps
    _, bounds, _ = R.taps(R.LANCZOS, 640, 6)
    assert bounds[0, 0] == 0 and bounds[-1].sum() == 640 and int(got[f"{R.LANCZOS}_640_6_k"]) == 2 * 320 + 1
    assert int(got[f"{R.NEAREST}_640_6_k"]) == 0 and got[f"{R.NEAREST}_100_333_b"][:, 1].all()
    assert (got[f"{R.BICUBIC}_100_333_t"] < 0).any() and (got[f"{R.LANCZOS}_640_6_t"] < 0).any()          # the negative branch of the rounding is live


def _taps_bytes(rt, f, a, b):
    ksize, nbytes = ctypes.c_int(-7), ctypes.c_size_t(12345)
    rc = rt.lib().adain_pil_resize_taps_bytes(f, a, b, ctypes.byref(ksize), ctypes.byref(nbytes))
    return rc, ksize.value, nbytes.value, rt.lib().adain_last_error().decode()


def test_the_taps_query_answers_and_refusals(rt):
    assert _taps_bytes(rt, R.NEAREST, 640, 6)[:3] == (0, 0, 6 * 2 * 4)
    assert _taps_bytes(rt, R.BOX, 640, 6)[:3] == (0, 109, 6 * 111 * 4)                    # ceil(0.5 * 106.67) * 2 + 1
    assert _taps_bytes(rt, R.BILINEAR, 1920, 455)[:3] == (0, 11, 455 * 13 * 4)
    assert _taps_bytes(rt, R.HAMMING, 100, 333)[:3] == (0, 3, 333 * 5 * 4)
    assert _taps_bytes(rt, R.BICUBIC, 300, 300)[:3] == (0, 5, 300 * 7 * 4)
    assert _taps_bytes(rt, R.LANCZOS, 256, 1)[:3] == (0, 1537, 1539 * 4)                  # the most taps an accepted axis has
    assert _taps_bytes(rt, R.LANCZOS, (1 << 24) - 1, 1 << 16)[:2] == (0, 1537)
    for args, text in (((6, 8, 8), "unknown filter"), ((-1, 8, 8), "unknown filter"), ((R.BOX, 0, 8), "bad size"), ((R.BOX, 8, 0), "bad size"),
                       ((R.BOX, 1 << 24, 1 << 24), "bad size"), ((R.BOX, 8, -3), "bad size"), ((R.NEAREST, 257, 1), "shrink factor"),
                       ((R.LANCZOS, 3000, 10), "shrink factor")):
        rc, ksize, nbytes, err = _taps_bytes(rt, *args)
        assert rc == -1 and text in err and (ksize, nbytes) == (-7, 12345), args
    assert rt.lib().adain_pil_resize_taps_bytes(R.BOX, 8, 8, None, None) == -1
    table = np.zeros(64, np.int32)
    assert rt.lib().adain_pil_resize_taps(R.BOX, 8, 4, None, table.ctypes.data) == -1 and b"null" in rt.lib().adain_last_error()
    assert rt.lib().adain_pil_resize_taps(R.BOX, 8, 4, table.ctypes.data, None) == -1
    assert rt.lib().adain_pil_resize_taps(R.BOX, 2000, 4, table.ctypes.data, table.ctypes.data) == -1 and b"shrink factor" in rt.lib().adain_last_error()
    assert not table.any()
    assert rt.lib().adain_pil_resize_taps(R.NEAREST, 8, 4, table.ctypes.data, None) == 0 and table[:8].tolist() == [1, 1, 3, 1, 5, 1, 7, 1]
    with pytest.raises(rt.AdainHipError, match="unknown resampling filter"):
        rt.pil_resize_taps("CUBIC", 8, 8)


def _ws(rt, *args):
    nbytes = ctypes.c_size_t(12345)
    rc = rt.lib().adain_resize_pil_u8_bytes(*args, ctypes.byref(nbytes))
    return rc, nbytes.value, rt.lib().adain_last_error().decode()


def test_the_workspace_query_answers_and_refusals(rt):
    # n, hi, wi, ho, wo, channels, filter, y0, x0, ch, cw: the intermediate is n x (source rows the window's taps reach) x cw x (1 | 3) bytes
    assert _ws(rt, 1, 1080, 1920, 256, 455, 3, R.LANCZOS, 0, 0, 256, 455)[:2] == (0, 1080 * 455 * 3)
    assert _ws(rt, 2, 1080, 1920, 256, 455, 4, R.BILINEAR, 0, 0, 256, 455)[:2] == (0, 2 * 1080 * 455 * 3)          # RGBX in, RGB between the passes
    assert _ws(rt, 3, 1080, 1920, 256, 455, 1, R.BOX, 0, 0, 256, 455)[:2] == (0, 3 * 1080 * 455)
    for f in (R.BOX, R.BICUBIC, R.LANCZOS):          # a band of the result needs a band of the intermediate
        _, bounds, _ = R.taps(f, 1080, 256)
        rows = int(bounds[109].sum() - bounds[100, 0])
        assert 0 < rows < 120
        assert _ws(rt, 1, 1080, 1920, 256, 455, 3, f, 100, 7, 10, 64)[:2] == (0, rows * 64 * 3)
    assert _ws(rt, 1, 1080, 1920, 256, 455, 3, R.BICUBIC, 100, 7, 1, 1)[:2] == (0, 16 * 3)          # one pixel: its 16 taps' rows, 416 .. 431
    # a skipped pass, NEAREST and an unchanged size need no intermediate
    assert _ws(rt, 1, 31, 57, 31, 20, 3, R.LANCZOS, 0, 0, 31, 20)[:2] == (0, 0)
    assert _ws(rt, 1, 31, 57, 9, 57, 3, R.LANCZOS, 0, 0, 9, 57)[:2] == (0, 0)
    assert _ws(rt, 1, 1080, 1920, 256, 455, 3, R.NEAREST, 0, 0, 256, 455)[:2] == (0, 0)
    assert _ws(rt, 1, 31, 57, 31, 57, 3, R.HAMMING, 0, 0, 31, 57)[:2] == (0, 0)
    base = [1, 270, 480, 256, 455, 3, R.LANCZOS, 0, 0, 256, 455]
    for at, value, text in ((0, 0, "n must be"), (1, 0, "bad size"), (2, 1 << 24, "bad size"), (3, 0, "bad size"), (4, -1, "bad size"), (5, 2, "pixels of"),
                            (5, 0, "pixels of"), (6, 6, "unknown filter"), (3, 1, "shrink factor"), (4, 1, "shrink factor"), (7, -1, "crop window"),
                            (8, 455, "crop window"), (9, 0, "crop window"), (9, 257, "crop window"), (10, 456, "crop window")):
        args = list(base)
        args[at] = value
        if at in (3, 4) and value == 1:          # keep the window inside the one-pixel side
            args[9 if at == 3 else 10] = 1
        rc, nbytes, err = _ws(rt, *args)
        assert rc == -1 and text in err and nbytes == 12345, (at, value, err)
    assert rt.lib().adain_resize_pil_u8_bytes(*base, None) == -1
