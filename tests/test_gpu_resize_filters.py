"""GPU tests of ``adain_resize_pil_u8`` / ``runtime.resize_pil_u8``: ``PIL.Image.resize(size, resample)`` of uint8 L and RGB images on
the device for Pillow's six filters.  The Pillow installed next to the tests is the reference, and every comparison is for equality
(``torch.equal`` / ``np.array_equal``).  The pictures saturate: noise over a ramp with patches of 0 and 255 and a black / white
checker, so that the negative lobes of BICUBIC and LANCZOS reach clip8 at both ends in both passes.  Run with ``-m gpu``."""
import threading

import numpy as np
import pytest
import torch
from PIL import Image

import pil_resize_ref as R

pytestmark = pytest.mark.gpu
FILTERS = list(R.FILTERS.items())          # NEAREST, BOX, BILINEAR, HAMMING, BICUBIC, LANCZOS
IDS = [name for name, _ in FILTERS]


@pytest.fixture(scope="module")
def rt():
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    import applied_image_processing_amd.runtime as rt

    rt.lib()
    torch.cuda.set_device(0)
    return rt


def pil_resize(a, size, f):
    return np.asarray(Image.fromarray(a).resize(size, f))


def gpu(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


# (h, w) -> (width, height)
NAMED = [((1, 1), (1, 1)),
         ((1, 1), (3, 5)),           # 1x1 -> 5x3
         ((7, 5), (1, 1)),
         ((31, 57), (20, 31)),       # the vertical pass is skipped
         ((31, 57), (57, 9)),        # the horizontal pass is skipped
         ((64, 48), (123, 200)),     # enlarging
         ((270, 480), (455, 256)),
         ((200, 300), (3, 2)),       # the palette page at factor 99: more taps than source pixels
         ((3, 3000), (12, 3))]       # a 250 x shrink, the largest side of the limit of 256


@pytest.mark.parametrize("name,f", FILTERS, ids=IDS)
@pytest.mark.parametrize("hw,size", NAMED)
def test_named_sizes_are_pillows_bytes(rt, hw, size, name, f):
    a = R.picture(5, *hw)
    want = pil_resize(a, size, f)
    got = rt.resize_pil_u8(gpu(a[None]), size, f)
    assert got.shape == (1, size[1], size[0], 3)
    assert torch.equal(got[0].cpu(), torch.from_numpy(want.copy()))


@pytest.mark.parametrize("name,f", FILTERS, ids=IDS)
def test_a_shrink_factor_above_256_is_refused_with_a_message(rt, name, f):
    x = gpu(R.picture(8, 3, 3000)[None])
    with pytest.raises(rt.AdainHipError, match="shrink factor"):
        rt.resize_pil_u8(x, (10, 3), f)


@pytest.mark.parametrize("name,f", FILTERS, ids=IDS)
def test_batch_rgbx_and_l(rt, name, f):
    frames = np.stack([R.picture(300 + k, 45, 70) for k in range(3)])
    size = (33, 52)
    want = np.stack([pil_resize(fr, size, f) for fr in frames])
    assert torch.equal(rt.resize_pil_u8(gpu(frames), size, f).cpu(), torch.from_numpy(want))
    # Pillow's own 4-byte storage (Image.tobytes("raw", "RGBX")) as the source
    x4 = np.stack([np.frombuffer(Image.fromarray(fr).tobytes("raw", "RGBX"), np.uint8).reshape(45, 70, 4) for fr in frames])
    assert torch.equal(rt.resize_pil_u8(gpu(x4), size, f).cpu(), torch.from_numpy(want))
    # L, with and without the channel axis
    grey = np.ascontiguousarray(frames[..., 1])
    want_l = np.stack([pil_resize(g, size, f) for g in grey])
    got = rt.resize_pil_u8(gpu(grey), size, f)
    assert got.shape == (3, 52, 33) and torch.equal(got.cpu(), torch.from_numpy(want_l))
    got = rt.resize_pil_u8(gpu(grey[..., None]), size, f)
    assert got.shape == (3, 52, 33, 1) and torch.equal(got[..., 0].cpu(), torch.from_numpy(want_l))
    # an unchanged size is a copy, as Pillow's is
    same = rt.resize_pil_u8(gpu(frames), (70, 45), f)
    assert torch.equal(same.cpu(), torch.from_numpy(frames))
    assert torch.equal(rt.resize_pil_u8(gpu(x4), (70, 45), f).cpu(), torch.from_numpy(frames))


@pytest.mark.parametrize("name,f", FILTERS, ids=IDS)
def test_crop_windows_and_out(rt, name, f):
    frames = np.stack([R.picture(400 + k, 120, 90) for k in range(2)])
    x = gpu(frames)
    for size in ((40, 23), (90, 23), (40, 120), (131, 170)):          # both passes, each pass alone, enlarging
        full = np.stack([pil_resize(fr, size, f) for fr in frames])
        wo, ho = size
        # a band of rows (a band of the intermediate), a band of columns, one pixel in a corner and one inside
        for y0, x0, ch, cw in ((ho // 2, 0, 3, wo), (0, wo // 3, ho, 5), (ho - 1, wo - 1, 1, 1), (ho // 3, wo // 2, 1, 1)):
            got = rt.resize_pil_u8(x, size, f, crop=(y0, x0, ch, cw))
            assert torch.equal(got.cpu(), torch.from_numpy(full[:, y0:y0 + ch, x0:x0 + cw].copy())), (size, y0, x0, ch, cw)
    full = np.stack([pil_resize(fr, (40, 23), f) for fr in frames])
    out = torch.zeros((2, 10, 7, 3), dtype=torch.uint8, device="cuda")
    assert rt.resize_pil_u8(x, (40, 23), f, crop=(5, 30, 10, 7), out=out) is out
    assert torch.equal(out.cpu(), torch.from_numpy(full[:, 5:15, 30:37].copy()))
    with pytest.raises(rt.AdainHipError, match="crop window"):
        rt.resize_pil_u8(x, (40, 23), f, crop=(20, 0, 10, 10))
    with pytest.raises(rt.AdainHipError):
        rt.resize_pil_u8(x, (40, 23), f, out=out)                               # out of another shape
    with pytest.raises(rt.AdainHipError):
        rt.resize_pil_u8(x.cpu(), (40, 23), f)                                  # no CPU fallback
    with pytest.raises(rt.AdainHipError):
        rt.resize_pil_u8(x[..., :2].contiguous(), (40, 23), f)                  # L, RGB or RGBX only


@pytest.mark.parametrize("name,f", FILTERS, ids=IDS)
def test_150_random_size_pairs(rt, name, f):
    g = np.random.default_rng(20261020)
    bad = []
    for case in range(150):
        hi, wi = int(g.integers(1, 200)), int(g.integers(1, 200))
        if case % 3 == 0:      # shrink, up to 20 x
            ho, wo = max(1, int(hi / g.uniform(1.0, 20.0))), max(1, int(wi / g.uniform(1.0, 20.0)))
        elif case % 3 == 1:    # enlarge (kept below 200)
            ho, wo = min(199, int(hi * g.uniform(1.0, 4.0)) + 1), min(199, int(wi * g.uniform(1.0, 4.0)) + 1)
        else:                  # anything
            ho, wo = int(g.integers(1, 200)), int(g.integers(1, 200))
        a = R.picture(100 + case, hi, wi)
        if case % 5 == 4:
            a = np.ascontiguousarray(a[..., 0])
        got = rt.resize_pil_u8(gpu(a[None]), (wo, ho), f)[0].cpu().numpy()
        want = pil_resize(a, (wo, ho), f)
        if not np.array_equal(got, want):
            bad.append((hi, wi, ho, wo, a.ndim, int(np.abs(got.astype(int) - want.astype(int)).max())))
    assert not bad, (len(bad), bad[:10])


@pytest.mark.parametrize("name,f", FILTERS, ids=IDS)
def test_a_1080p_frame(rt, name, f):
    a = R.picture(9, 1080, 1920)
    got = rt.resize_pil_u8(gpu(a[None]), (455, 256), f)[0].cpu().numpy()
    assert np.array_equal(got, pil_resize(a, (455, 256), f))


def test_bilinear_equals_the_one_pass_call(rt):
    for hw, size in (((270, 480), (455, 256)), ((64, 48), (123, 200)), ((31, 57), (20, 31)), ((200, 300), (3, 2))):
        x = gpu(R.picture(21, *hw)[None])
        assert torch.equal(rt.resize_pil_u8(x, size, rt.PIL_BILINEAR), rt.resize_pil_bilinear_u8(x, size))
        wo, ho = size
        crop = (ho // 2, wo // 3, ho - ho // 2, wo - wo // 3)
        assert torch.equal(rt.resize_pil_u8(x, size, "bilinear", crop=crop), rt.resize_pil_bilinear_u8(x, size, crop=crop))


def test_filter_names_codes_and_members(rt):
    x = gpu(R.picture(22, 20, 30)[None])
    want = rt.resize_pil_u8(x, (7, 9), Image.Resampling.LANCZOS)
    assert torch.equal(rt.resize_pil_u8(x, (7, 9), "LANCZOS"), want) and torch.equal(rt.resize_pil_u8(x, (7, 9), 1), want)
    for bad in (6, -1, "CUBIC"):
        with pytest.raises(rt.AdainHipError, match="unknown resampling filter"):
            rt.resize_pil_u8(x, (7, 9), bad)


def test_the_second_call_of_a_geometry_uploads_nothing(rt):
    """The counter on the table cache, not a clock: the first call of a geometry builds and uploads one table per axis, the second finds
    both; a square resize shares one table between its axes; the cache forgets the least recently used axis beyond its bound."""
    rt.free_pil_tables()
    x = gpu(R.picture(23, 40, 60)[None])
    stats = rt.PIL_TABLE_STATS
    before = dict(stats)
    first = rt.resize_pil_u8(x, (25, 17), rt.PIL_LANCZOS)
    assert (stats["uploads"] - before["uploads"], stats["hits"] - before["hits"]) == (2, 0)
    second = rt.resize_pil_u8(x, (25, 17), rt.PIL_LANCZOS)
    assert (stats["uploads"] - before["uploads"], stats["hits"] - before["hits"]) == (2, 2) and torch.equal(first, second)
    rt.resize_pil_u8(x, (25, 17), rt.PIL_BICUBIC)                                   # another filter: other tables
    assert stats["uploads"] - before["uploads"] == 4
    sq = gpu(R.picture(24, 30, 30)[None])
    rt.resize_pil_u8(sq, (11, 11), rt.PIL_BOX)
    assert (stats["uploads"] - before["uploads"], stats["hits"] - before["hits"]) == (5, 3)
    for k in range(rt.PIL_TABLES_KEPT):                                             # push the first geometry out
        rt.resize_pil_u8(sq, (31 + k, 30), rt.PIL_BOX)
    assert len(rt._pil_tables) == rt.PIL_TABLES_KEPT
    mark = stats["uploads"]
    assert torch.equal(rt.resize_pil_u8(x, (25, 17), rt.PIL_LANCZOS), first) and stats["uploads"] - mark == 2


def test_concurrent_calls_with_different_filters(rt):
    """Four threads on one stream, each with its own filter and sizes: the intermediate in the stream's workspace belongs to one call
    at a time."""
    jobs = []
    for k, (name, f) in enumerate(FILTERS[2:]):          # BILINEAR, HAMMING, BICUBIC, LANCZOS
        a = R.picture(600 + k, 90 + 7 * k, 130 - 11 * k)
        jobs.append((a, (41 + 5 * k, 37 - 3 * k), f))
    want = [[pil_resize(a, size, f)] * 6 for a, size, f in jobs]
    got = [[] for _ in jobs]

    def work(i):
        a, size, f = jobs[i]
        x = gpu(a[None])
        for _ in range(6):
            got[i].append(rt.resize_pil_u8(x, size, f))

    threads = [threading.Thread(target=work, args=(i,)) for i in range(len(jobs))]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    torch.cuda.synchronize()
    for i in range(len(jobs)):
        assert len(got[i]) == 6
        for g, w in zip(got[i], want[i]):
            assert np.array_equal(g[0].cpu().numpy(), w), i
