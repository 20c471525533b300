"""adain_palette_map_u8, adain_tone_u8 and adain_palette_dither_u8 against tests/palette_ref.py: every comparison is exact."""
import ctypes
import os

import numpy as np
import pytest
import torch
from PIL import Image

import palette_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "palette")
TONES = ((0.25, 0), (0, -0.3), (-0.5, 0.8))
SWEETIE = np.array([[0x1a, 0x1c, 0x2c], [0x5d, 0x27, 0x5d], [0xb1, 0x3e, 0x53], [0xef, 0x7d, 0x57], [0xff, 0xcd, 0x75], [0xa7, 0xf0, 0x70], [0x38, 0xb7, 0x64],
                    [0x25, 0x71, 0x79], [0x29, 0x36, 0x6f], [0x3b, 0x5d, 0xc9], [0x41, 0xa6, 0xf6], [0x73, 0xef, 0xf7], [0xf4, 0xf4, 0xf4], [0x94, 0xb0, 0xc2],
                    [0x56, 0x6c, 0x86], [0x33, 0x3c, 0x57]], np.uint8)


@pytest.fixture(scope="module")
def rt():
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    import applied_image_processing_amd.runtime as rt

    rt.lib()
    torch.cuda.set_device(0)
    return rt


@pytest.fixture(scope="module")
def G():
    return dict(np.load(os.path.join(GOLDEN, "palette_golden.npz")))


def T(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def noise(seed, *shape):
    return np.random.default_rng(seed).integers(0, 256, shape, dtype=np.uint8)


def noisy_gradient(h, w, seed):
    rng = np.random.default_rng(seed)
    y, x = np.mgrid[0:h, 0:w]
    base = np.stack([x * (250.0 / max(w - 1, 1)), y * (250.0 / max(h - 1, 1)), (x + y) * (250.0 / max(h + w - 2, 1))], axis=-1)
    return np.clip(base + rng.normal(0, 6, base.shape), 0, 255).astype(np.uint8)


def palette_of(K, seed=1):
    if K == 16:
        return SWEETIE
    return noise(seed + K, K, 3)


def same(t, a):
    return torch.equal(t.cpu(), torch.from_numpy(np.ascontiguousarray(a)))


# ---- map -----------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("metric", ["rgb", "nearest"])
@pytest.mark.parametrize("K", [1, 2, 16, 256])
def test_map_is_the_integer_rule(rt, metric, K):
    frame, pal = noise(K, 33, 45, 3), palette_of(K)
    out, idx = rt.palette_map_u8(T(frame), T(pal), metric, index=True)
    want = R.map_index(frame, pal, metric)
    assert same(idx, want.astype(np.uint8)) and same(out, pal[want])
    assert torch.equal(rt.palette_map_u8(T(frame), pal.tolist(), metric), out)          # a sequence of triples, no index plane


@pytest.mark.parametrize("metric", ["rgb", "nearest"])
@pytest.mark.parametrize("h,w", [(1, 1), (1, 67), (67, 1), (4, 4), (32, 40)])
def test_map_frame_shapes(rt, metric, h, w):
    frame = noise(h * 7 + w, h, w, 3)          # 4 x 4, 32 x 40: the four-pixels-per-thread form; the others: one pixel per thread
    out, idx = rt.palette_map_u8(T(frame), T(SWEETIE), metric, index=True)
    want = R.map_index(frame, SWEETIE, metric)
    assert same(idx, want.astype(np.uint8)) and same(out, SWEETIE[want])


@pytest.mark.parametrize("metric", ["rgb", "nearest"])
def test_map_ties_go_to_the_lowest_index(rt, G, metric):
    frame, pal = G["ties"], G["ties_palette"]          # duplicate entries, pixels exactly between two and more entries
    out, idx = rt.palette_map_u8(T(frame), T(pal), metric, index=True)
    want = R.map_index(frame, pal, metric)
    assert same(idx, want.astype(np.uint8)) and same(out, pal[want])
    assert same(out, G["ties_rgb" if metric == "rgb" else "ties_floyd"])          # the reference's own bytes
    between = np.array([[[10, 0, 0], [0, 10, 0], [250, 250, 250], [255, 255, 255]]], np.uint8)
    _, i = rt.palette_map_u8(T(between), T(pal), "nearest", index=True)
    assert i.cpu().tolist() == [[0, 0, 5, 5]]


def test_map_batch_equals_alone(rt):
    frames = noise(9, 3, 33, 45, 3)
    for metric in ("rgb", "nearest"):
        out, idx = rt.palette_map_u8(T(frames), T(SWEETIE), metric, index=True)
        for i in range(3):
            o1, i1 = rt.palette_map_u8(T(frames[i]), T(SWEETIE), metric, index=True)
            assert torch.equal(out[i], o1) and torch.equal(idx[i], i1)


@pytest.mark.parametrize("metric", [0, 1])
def test_map_at_odd_byte_offsets(rt, metric):
    frame = noise(4, 2, 12, 10, 3)
    nbytes = frame.size
    src, out, idx = (torch.full((nbytes + 8,), 0xAA, dtype=torch.uint8, device=DEV) for _ in range(3))
    src[1:1 + nbytes] = T(frame).reshape(-1)
    pal = T(SWEETIE)
    rt.call("adain_palette_map_u8", src.device, src.data_ptr() + 1, 2, 12, 10, pal.data_ptr(), 16, metric, None, 0, out.data_ptr() + 3, idx.data_ptr() + 1)
    want = R.map_index(frame, SWEETIE, "nearest" if metric else "rgb")
    assert same(out[3:3 + nbytes].reshape(frame.shape), SWEETIE[want]) and same(idx[1:1 + nbytes // 3].reshape(want.shape), want.astype(np.uint8))
    for buf, a, b in ((out, 3, 3 + nbytes), (idx, 1, 1 + nbytes // 3)):          # nothing before or behind
        assert bool((buf[:a] == 0xAA).all()) and bool((buf[b:] == 0xAA).all())


def test_map_with_the_tone_step_in_front(rt, G):
    frame, lut = G["gradient"], R.tone_lut(*TONES[2])
    out = rt.palette_map_u8(T(frame), T(SWEETIE), "rgb", lut=T(lut), grey=True)
    assert same(out, R.map_frame(R.tone(frame, lut, True), SWEETIE, "rgb"))


# ---- tone ----------------------------------------------------------------------------------------------------------------------------------
def test_tone_identity_and_in_place(rt, G):
    x = T(G["gradient"])
    assert torch.equal(rt.tone_u8(x, lut=torch.arange(256, dtype=torch.uint8)), x)
    assert torch.equal(rt.tone_u8(x), x)
    y = x.clone()
    assert rt.tone_u8(y, lut=T(R.tone_lut(*TONES[0])), out=y).data_ptr() == y.data_ptr() and same(y, G["gradient_tone0"])


@pytest.mark.parametrize("i", range(3))
@pytest.mark.parametrize("name", ["gradient", "ties"])
def test_tone_is_the_reference_adjustment(rt, G, name, i):
    assert same(rt.tone_u8(T(G[name]), lut=T(R.tone_lut(*TONES[i]))), G[f"{name}_tone{i}"])


@pytest.mark.parametrize("with_lut", [False, True])
def test_grey_is_pillows(rt, with_lut):
    frames = noise(12, 2, 31, 43, 3)
    lut = np.stack([R.tone_lut(*TONES[c]) for c in range(3)]) if with_lut else None          # a table per channel
    out = rt.tone_u8(T(frames), lut=None if lut is None else T(lut), grey=True)
    pil = np.stack([np.asarray(Image.fromarray(f).convert("L").convert("RGB")) for f in frames])
    assert same(out, R.tone(pil, lut))
    assert same(rt.tone_u8(T(frames), lut=None if lut is None else T(lut), grey=False), R.tone(frames, lut))


# ---- dither --------------------------------------------------------------------------------------------------------------------------------
B = R.BAND
DITHER_SHAPES = [(1, 1), (1, 9), (9, 1), (2, 3), (3, 2), (70, 33), (B - 1, 5), (B, 5), (B + 1, 5), (2 * B + 1, 5)]


@pytest.mark.parametrize("h,w", DITHER_SHAPES)
def test_dither_is_the_sequential_loop(rt, h, w):
    frame = noisy_gradient(h, w, h * 100 + w)
    out, idx = rt.palette_dither_u8(T(frame), T(SWEETIE), index=True)
    want, widx = R.dither_push(frame, SWEETIE)
    assert same(idx, widx) and same(out, want)


@pytest.fixture(scope="module")
def frame_40x61():
    return noisy_gradient(40, 61, 5)


def test_dither_with_every_option(rt, frame_40x61):
    lut = R.tone_lut(*TONES[1])
    out, idx = rt.palette_dither_u8(T(frame_40x61), T(SWEETIE), lut=T(lut), grey=True, index=True)
    want, widx = R.dither(frame_40x61, SWEETIE, lut, True)
    assert same(idx, widx) and same(out, want)


def test_dither_diffuses(rt, frame_40x61):
    x = T(frame_40x61)
    differ = (rt.palette_dither_u8(x, T(SWEETIE)) != rt.palette_map_u8(x, T(SWEETIE), "nearest")).any(dim=-1).float().mean().item()
    assert differ > 0.10, differ


def test_dither_batch_equals_alone(rt):
    frames = np.stack([noisy_gradient(37, 29, s) for s in (1, 2, 3)])
    pal = palette_of(8)
    out, idx = rt.palette_dither_u8(T(frames), T(pal), index=True)
    for i in range(3):
        o1, i1 = rt.palette_dither_u8(T(frames[i]), T(pal), index=True)
        assert torch.equal(out[i], o1) and torch.equal(idx[i], i1)
    assert same(out[1], R.dither_push(frames[1], pal)[0])


# ---- refusals ------------------------------------------------------------------------------------------------------------------------------
def refusal_cases():
    # (entry, the argument to spoil, its value, a word of the message)
    yield "map", "src", None, "src"
    yield "map", "palette", None, "palette"
    yield "map", "out", None, "out"
    yield "map", "K", 0, "K"
    yield "map", "K", 257, "K"
    yield "map", "metric", 2, "metric"
    yield "map", "metric", -1, "metric"
    yield "map", "h", 0, "height"
    yield "map", "w", 0, "width"
    yield "map", "n", 0, "n outside"
    yield "map", "n", 65536, "n outside"
    yield "tone", "src", None, "src"
    yield "tone", "out", None, "out"
    yield "tone", "h", 0, "height"
    yield "tone", "n", 65536, "n outside"
    yield "dither", "src", None, "src"
    yield "dither", "palette", None, "palette"
    yield "dither", "out", None, "out"
    yield "dither", "K", 0, "K"
    yield "dither", "K", 257, "K"
    yield "dither", "h", 0, "height"
    yield "dither", "w", -1, "width"
    yield "dither", "n", 0, "n outside"
    yield "dither", "n", 65536, "n outside"
    yield "dither", "workspace", None, "workspace"
    yield "dither", "workspace_bytes", "short", "workspace too small"
    yield "dither", "workspace", "misaligned", "aligned"


@pytest.mark.parametrize("entry,arg,value,word", list(refusal_cases()))
def test_refusals_come_before_any_launch(rt, entry, arg, value, word):
    n, h, w = 2, 6, 7
    src, pal = T(noise(1, n, h, w, 3)), T(SWEETIE)
    out = torch.full((n * h * w * 3,), 0x5A, dtype=torch.uint8, device=DEV)
    need = rt.palette_dither_sizes(n, h, w)
    ws = torch.full((need + 16,), 0x5A, dtype=torch.uint8, device=DEV)
    a = dict(src=src.data_ptr(), n=n, h=h, w=w, palette=pal.data_ptr(), K=16, metric=1, lut=None, grey=0, out=out.data_ptr(), index=None, workspace=ws.data_ptr(),
             workspace_bytes=need)
    assert ws.data_ptr() % 8 == 0
    if value == "short":
        a[arg] = need - 1
    elif value == "misaligned":
        a[arg] = ws.data_ptr() + 4
    else:
        a[arg] = value
    order = {"map": ("src", "n", "h", "w", "palette", "K", "metric", "lut", "grey", "out", "index"), "tone": ("src", "n", "h", "w", "lut", "grey", "out"),
             "dither": ("src", "n", "h", "w", "palette", "K", "lut", "grey", "out", "index", "workspace", "workspace_bytes")}[entry]
    name = {"map": "adain_palette_map_u8", "tone": "adain_tone_u8", "dither": "adain_palette_dither_u8"}[entry]
    with pytest.raises(rt.AdainHipError, match=r"failed \(-1\)") as e:
        rt.call(name, src.device, *(a[k] for k in order))
    assert word in str(e.value), str(e.value)
    torch.cuda.synchronize()
    assert bool((out == 0x5A).all()) and bool((ws == 0x5A).all())


def test_the_size_query_refuses_and_answers(rt):
    assert rt.palette_dither_sizes(3, 10, 7) >= 3 * 7 * 3 * 4
    out = ctypes.c_size_t(123)
    assert rt.lib().adain_palette_dither_u8_bytes(1, 0, 5, ctypes.byref(out)) == -1 and out.value == 123
    assert rt.lib().adain_palette_dither_u8_bytes(1, 4, 5, None) == 0
