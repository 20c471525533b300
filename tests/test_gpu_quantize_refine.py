"""runtime.quantize_palette_u8(..., refine=T) (csrc/quantize_refine.hip) against the rules restated in tests/quantize_refine_ref.py: every
result - palettes and used - is compared for equality, there is no tolerance.  The rules, behind the median cut's rules 1-6, per round:
(7) a pixel goes to the nearest entry below `used`, squared Euclidean distance in ints, the lowest index among equals; (8) per entry the
count, the sums and the far key max((d << 24) | (0xFFFFFF - rgb)); (9) an entry with pixels becomes (2 S + n) // (2 n), one without stays;
(10) the free slots - i < K without a pixel, ascending - take the far colours of the donors - by distance descending, then index
ascending - and `used` grows to the highest slot filled; (11) entries from `used` on are zero.

The shapes are the smallest at which the stages can go wrong: one pixel, fewer pixels than a 16-byte load, two small clips (a palette
per frame on the grid's second axis), more slots than a cell has colours, the hand cases that fill a slot and that have no donor, one pixel
below, at and above a workgroup's tile of 4096, and a clip whose one palette is spread over several workgroups."""
import functools

import numpy as np
import pytest
import torch

import quantize_refine_cases as RC
import quantize_refine_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


@pytest.fixture(scope="module")
def rt():
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    import applied_image_processing_amd.runtime as rt

    rt.lib()
    torch.cuda.set_device(0)
    return rt


FRAMES = dict(RC.device_frames())
FRAMES["several workgroups"] = RC.several_workgroups()


@functools.lru_cache(maxsize=None)
def traced(name, K, frame):
    """[(palette, used)] after 0..8 rounds of the restatement (frame None: the whole clip), computed once and never written to."""
    out = R.trace(FRAMES[name] if frame is None else FRAMES[name][frame], K, max(RC.TS))
    for pal, _ in out:
        pal.setflags(write=False)
    return out


def reference(name, K, per_frame, T):
    parts = [traced(name, K, i)[T] for i in range(len(FRAMES[name]))] if per_frame and len(FRAMES[name]) > 1 else [traced(name, K, None)[T]]
    return np.stack([p for p, _ in parts]), [u for _, u in parts]


def device(rt, frames, K, per_frame=False, refine=0):
    pals, used = rt.quantize_palette_u8(torch.from_numpy(np.ascontiguousarray(frames)).to(DEV), K, per_frame, refine)
    assert pals.dtype == torch.uint8 and used.dtype == torch.int32 and pals.is_cuda and used.is_cuda
    return pals.cpu().numpy(), used.cpu().tolist()


def check(got, want, what=""):
    assert got[1] == list(want[1]), what
    assert np.array_equal(got[0], want[0]), what


@pytest.mark.parametrize("name,frames,K,T,entries", RC.HAND, ids=[c[0] for c in RC.HAND])
def test_hand_computed_cases(rt, name, frames, K, T, entries):
    pal, used = RC.expected(entries)
    check(device(rt, frames, K, refine=T), (pal[None], [used]))
    check(device(rt, frames, K, per_frame=True, refine=T), (pal[None], [used]))


@pytest.mark.parametrize("K", RC.DEVICE_KS)
@pytest.mark.parametrize("per_frame", [False, True], ids=["global", "per-frame"])
@pytest.mark.parametrize("T", RC.TS)
@pytest.mark.parametrize("name", [n for n, _ in RC.device_frames()])
def test_frames(rt, name, T, per_frame, K):
    check(device(rt, FRAMES[name], K, per_frame, T), reference(name, K, per_frame, T))


@pytest.mark.parametrize("K", RC.DEVICE_KS)
@pytest.mark.parametrize("T", RC.TS)
def test_one_palette_over_several_workgroups(rt, T, K):
    frames = FRAMES["several workgroups"]
    assert frames.shape == (3, 96, 97, 3) and frames.shape[0] * 96 * 97 > 2 * 4096
    check(device(rt, frames, K, False, T), reference("several workgroups", K, False, T))


def test_two_calls_give_the_same_bits(rt):
    for name, per_frame in (("several workgroups", False), ("noise 2x16x24", True)):
        x = torch.from_numpy(FRAMES[name]).to(DEV)
        a = rt.quantize_palette_u8(x, 256, per_frame, 8)
        b = rt.quantize_palette_u8(x, 256, per_frame, 8)
        assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])


@pytest.mark.parametrize("K", [16, 256])
def test_the_clip_split_into_frames_two_ways(rt, K):
    frames = FRAMES["several workgroups"]
    want = reference("several workgroups", K, False, 2)
    for shape in ((3, 96, 97, 3), (1, 288, 97, 3), (97, 3, 96, 3), (3 * 96 * 97, 1, 1, 3)):
        check(device(rt, frames.reshape(shape), K, False, 2), want, shape)


def test_no_rounds_is_the_call_without_the_argument(rt):
    for name in ("several workgroups", "noise 2x16x24", "two colours in one cell"):
        x = torch.from_numpy(FRAMES[name]).to(DEV)
        for per_frame in (False, True):
            a = rt.quantize_palette_u8(x, 256, per_frame)
            b = rt.quantize_palette_u8(x, 256, per_frame, 0)
            assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
            n, h, w, _ = x.shape
            assert rt.quantize_palette_sizes(n, h, w, per_frame, 0) == rt.quantize_palette_sizes(n, h, w, per_frame)


def test_wrapper_refusals(rt):
    x = torch.zeros((2, 4, 4, 3), dtype=torch.uint8, device=DEV)
    for bad in (-1, 65, True, 2.0, None):
        with pytest.raises(ValueError, match="refine must be"):
            rt.quantize_palette_u8(x, 4, False, bad)
        with pytest.raises(ValueError, match="refine must be"):
            rt.quantize_palette_sizes(2, 4, 4, False, bad)
