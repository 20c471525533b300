"""The memory contract of adain_quantize_palette_u8 with ADAIN_QUANTIZE_REFINE(T) in its mode, through the guard-band arena
(tests/abi_arena.py): sources at every byte offset of a 16-byte line, no byte outside `palettes`, `used` and a workspace of exactly the
queried size changes, a workspace of 0x00 and of 0xFF stale bytes gives the same palettes, and a refused call writes nothing.  Every
result is the restatement's (tests/quantize_refine_ref.py), bit for bit."""
import functools

import numpy as np
import pytest
import torch

import abi_arena as A
import quantize_cases as C
import quantize_refine_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
EINVAL = -1
FRAMES = C.gradient(3, 37, 53, 20)          # 5883 pixels: two tiles for one palette, a ragged head and tail at most offsets
FRAMES.setflags(write=False)
K, T = 16, 2


def mode_of(per_frame, rounds):
    return (1 if per_frame else 0) | rounds << 8          # ADAIN_QUANTIZE_PER_FRAME | ADAIN_QUANTIZE_REFINE(rounds)


@pytest.fixture(scope="module")
def rt():
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    import applied_image_processing_amd.runtime as rt

    rt.lib()
    torch.cuda.set_device(0)
    return rt


@functools.lru_cache(maxsize=None)
def wanted(per_frame):
    pals, used = R.palettes(FRAMES, K, per_frame, T)
    pals.setflags(write=False)
    return pals, used.tolist()


def specs_of(rt, frames, per_frame, rounds, pad=0):
    n, h, w, _ = frames.shape
    P = n if per_frame else 1
    nbytes = rt.quantize_palette_sizes(n, h, w, per_frame, rounds)
    return [("src", frames.size + pad, "in", 16 if pad else 1), ("palettes", P * 768, "out", 1), ("used", 4 * P, "out", 4), ("workspace", nbytes, "ws", 8)], nbytes


def test_the_workspace_term(rt):
    """Per palette the accumulators of rule 8, 256 x 5 x 8 bytes, behind the grids; none without rounds."""
    for per_frame, P in ((False, 1), (True, 3)):
        plain = rt.quantize_palette_sizes(3, 37, 53, per_frame)
        assert rt.quantize_palette_sizes(3, 37, 53, per_frame, 0) == plain
        for rounds in (1, 8, 64):
            assert rt.quantize_palette_sizes(3, 37, 53, per_frame, rounds) == plain + P * 256 * 5 * 8


# the source at every offset behind a 16-byte boundary: the ragged head is 0..15 pixels long
@pytest.mark.parametrize("offset", range(16))
@pytest.mark.parametrize("per_frame", [False, True], ids=["global", "per-frame"])
def test_the_call_stays_in_its_buffers_and_ignores_stale_bytes(rt, offset, per_frame):
    n, h, w, _ = FRAMES.shape
    specs, nbytes = specs_of(rt, FRAMES, per_frame, T, pad=15)
    flat = torch.cat([torch.full((offset,), 0x5A, dtype=torch.uint8), torch.from_numpy(FRAMES.copy()).reshape(-1), torch.full((15 - offset,), 0x5A, dtype=torch.uint8)])
    stream = torch.cuda.current_stream().cuda_stream

    def call(arena):
        assert (arena.ptr("src") + offset) % 16 == offset
        rc = rt.lib().adain_quantize_palette_u8(arena.ptr("src") + offset, n, h, w, K, mode_of(per_frame, T), arena.ptr("palettes"), arena.ptr("used"),
                                                arena.ptr("workspace"), nbytes, stream)
        assert rc == 0, rt.lib().adain_last_error().decode()

    def stale(arena):          # what a call leaves in the workspace is not zero: the next call must not build on it
        arena.bytes("workspace").fill_(0xA5)

    outs = A.run_case(specs, call, DEV, torch.cuda.synchronize, history=stale, setup=lambda arena: arena.put("src", flat))
    pals, used = wanted(per_frame)
    assert outs["used"].view(torch.int32).tolist() == used
    assert np.array_equal(outs["palettes"].cpu().numpy().reshape(-1, 256, 3), pals)


@pytest.mark.parametrize("per_frame", [False, True], ids=["global", "per-frame"])
def test_stale_bytes_of_0x00_and_0xff(rt, per_frame):
    n, h, w, _ = FRAMES.shape
    specs, nbytes = specs_of(rt, FRAMES, per_frame, T)
    stream = torch.cuda.current_stream().cuda_stream
    pals, used = wanted(per_frame)
    arena = A.Arena(specs, "A", DEV)
    arena.put("src", torch.from_numpy(FRAMES.copy()))
    for stale in (0x00, 0xFF):
        arena.bytes("workspace").fill_(stale)
        arena.bytes("palettes").fill_(stale)
        arena.bytes("used").fill_(stale)
        rc = rt.lib().adain_quantize_palette_u8(arena.ptr("src"), n, h, w, K, mode_of(per_frame, T), arena.ptr("palettes"), arena.ptr("used"), arena.ptr("workspace"),
                                                nbytes, stream)
        assert rc == 0, rt.lib().adain_last_error().decode()
        torch.cuda.synchronize()
        arena.check()
        assert arena.bytes("used").view(torch.int32).tolist() == used, hex(stale)
        assert np.array_equal(arena.bytes("palettes").cpu().numpy().reshape(-1, 256, 3), pals), hex(stale)


def test_every_refusal_is_einval_and_writes_nothing(rt):
    frames = C.gradient(2, 9, 11, 1)
    n, h, w, _ = frames.shape
    specs, nbytes = specs_of(rt, frames, True, T)
    plain = rt.quantize_palette_sizes(n, h, w, True)
    assert plain < nbytes
    arena = A.Arena(specs, "B", DEV)
    arena.put("src", torch.from_numpy(frames))
    src, pal, used, ws = (arena.ptr(k) for k in ("src", "palettes", "used", "workspace"))
    stream = torch.cuda.current_stream().cuda_stream
    good = dict(src=src, n=n, h=h, w=w, K=16, mode=mode_of(True, T), palettes=pal, used=used, workspace=ws, workspace_bytes=nbytes)
    refusals = [          # (what adain_last_error names, the argument that is wrong)
        ("mode other than", dict(mode=mode_of(True, 65))), ("mode other than", dict(mode=2 | 1 << 8)), ("mode other than", dict(mode=mode_of(False, 1 << 20))),
        ("mode other than", dict(mode=-1)), ("mode other than", dict(mode=-(1 << 8))), ("mode other than", dict(mode=2)), ("mode other than", dict(mode=5)),
        ("workspace too small", dict(workspace_bytes=nbytes - 1)), ("workspace too small", dict(workspace_bytes=plain)),
        ("src is a null", dict(src=None)), ("palettes is a null", dict(palettes=None)), ("used is a null", dict(used=None)),
        ("workspace is a null", dict(workspace=None)), ("K outside 1..256", dict(K=0)), ("K outside 1..256", dict(K=257)),
        ("n outside", dict(n=0)), ("n outside", dict(n=65536)), ("empty frames", dict(h=0)), ("empty frames", dict(w=-3)),
        ("pixels for one palette", dict(h=65536, w=65536, workspace_bytes=1 << 62)),
        ("workspace must be 8-byte aligned", dict(workspace=ws + 4)), ("used must be 4-byte aligned", dict(used=used + 2)),
        ("palettes overlaps src", dict(palettes=src + 5)), ("used overlaps src", dict(used=src + (4 - src % 4))),
        ("workspace overlaps src", dict(workspace=src - src % 8)),
    ]
    for text, change in refusals:
        a = dict(good, **change)
        rc = rt.lib().adain_quantize_palette_u8(a["src"], a["n"], a["h"], a["w"], a["K"], a["mode"], a["palettes"], a["used"], a["workspace"], a["workspace_bytes"], stream)
        message = rt.lib().adain_last_error().decode()
        assert rc == EINVAL, (text, change, rc)
        assert message.startswith("quantize_palette_u8: ") and text in message, (text, message)
    for query in ((1, 4, 4, mode_of(False, 65)), (1, 4, 4, 2 | 1 << 8), (1, 4, 4, -1), (0, 4, 4, mode_of(False, 1)), (1, 65536, 65536, mode_of(True, 1))):
        assert rt.lib().adain_quantize_palette_u8_bytes(*query, None) == EINVAL
    assert rt.lib().adain_quantize_palette_u8_bytes(1, 4, 4, mode_of(True, 64), None) == 0
    torch.cuda.synchronize()
    arena.check()
    for name in ("palettes", "used", "workspace"):
        r = arena.region(name)
        assert bool((arena.bytes(name) == arena._expected(r.offset, r.offset + r.nbytes)).all()), f"a refused call wrote into {name}"
