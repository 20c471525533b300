"""The memory contract of the palette calls through the guard-band arena (tests/abi_arena.py): no byte outside `out`, `index` and the
workspace changes, and a workspace of stale bytes - 0xFF, a pattern, another call's error rows - gives the same frames."""
import numpy as np
import pytest
import torch

import abi_arena as A
import palette_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
PAL = np.array([[13, 43, 69], [32, 60, 86], [84, 78, 104], [141, 105, 122], [208, 129, 89], [255, 170, 94], [255, 212, 163], [255, 236, 214]], np.uint8)


@pytest.fixture(scope="module")
def rt():
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    import applied_image_processing_amd.runtime as rt

    rt.lib()
    torch.cuda.set_device(0)
    return rt


def frames_of(n, h, w):
    rng = np.random.default_rng(h * w + n)
    y, x = np.mgrid[0:h, 0:w]
    base = np.stack([x * (250.0 / max(w - 1, 1)), y * (250.0 / max(h - 1, 1)), (x + y) * (250.0 / max(h + w - 2, 1))], axis=-1)
    return np.stack([np.clip(base + rng.normal(0, 8, base.shape), 0, 255).astype(np.uint8) for _ in range(n)])


# one row, one column, a band that never fills, a batch, more than one band (the carry row in the workspace is read back)
DITHER_CASES = [(1, 1, 1, True), (1, 1, 9, False), (2, 9, 1, True), (3, 37, 29, True), (1, R.BAND + 3, 6, True), (2, 2 * R.BAND + 1, 3, False)]


@pytest.mark.parametrize("n,h,w,with_index", DITHER_CASES)
def test_dither_stays_in_its_buffers_and_ignores_stale_bytes(rt, n, h, w, with_index):
    frames = frames_of(n, h, w)
    nbytes = rt.palette_dither_sizes(n, h, w)
    specs = [("src", frames.size, "in", 1), ("palette", PAL.size, "in", 1), ("out", frames.size, "out", 1), ("workspace", nbytes, "ws", 8)]
    if with_index:
        specs.insert(3, ("index", n * h * w, "out", 1))
    stream = torch.cuda.current_stream().cuda_stream

    def call(arena, shape=(n, h, w)):
        rc = rt.lib().adain_palette_dither_u8(arena.ptr("src"), *shape, arena.ptr("palette"), len(PAL), None, 0, arena.ptr("out"),
                                              arena.ptr("index") if with_index else None, arena.ptr("workspace"), nbytes, stream)
        assert rc == 0, rt.lib().adain_last_error().decode()

    def setup(arena):
        arena.put("src", torch.from_numpy(frames))
        arena.put("palette", torch.from_numpy(PAL))

    # a shorter frame through the same workspace and outputs first, then the call again: stale error rows of another shape
    history = (lambda arena: call(arena, (1, h // 2, w))) if h >= 4 else None
    outs = A.run_case(specs, call, DEV, torch.cuda.synchronize, history=history, setup=setup)
    want = [R.dither_push(f, PAL) for f in frames]
    assert outs["out"].cpu().numpy().tobytes() == np.stack([o for o, _ in want]).tobytes()
    if with_index:
        assert outs["index"].cpu().numpy().tobytes() == np.stack([i for _, i in want]).tobytes()


@pytest.mark.parametrize("n,h,w,metric", [(1, 1, 1, 0), (3, 33, 45, 1), (2, 16, 24, 0)])
def test_map_and_tone_stay_in_their_buffers(rt, n, h, w, metric):
    frames = frames_of(n, h, w)
    lut = np.stack([R.tone_lut(0.25, 0), R.tone_lut(0, -0.3), R.tone_lut(-0.5, 0.8)])
    specs = [("src", frames.size, "in", 1), ("palette", PAL.size, "in", 1), ("lut", 768, "in", 1), ("out", frames.size, "out", 1), ("index", n * h * w, "out", 1),
             ("toned", frames.size, "out", 1)]
    stream = torch.cuda.current_stream().cuda_stream

    def call(arena):
        rc = rt.lib().adain_palette_map_u8(arena.ptr("src"), n, h, w, arena.ptr("palette"), len(PAL), metric, arena.ptr("lut"), 1, arena.ptr("out"), arena.ptr("index"),
                                           stream)
        assert rc == 0, rt.lib().adain_last_error().decode()
        rc = rt.lib().adain_tone_u8(arena.ptr("src"), n, h, w, arena.ptr("lut"), 1, arena.ptr("toned"), stream)
        assert rc == 0, rt.lib().adain_last_error().decode()

    def setup(arena):
        arena.put("src", torch.from_numpy(frames))
        arena.put("palette", torch.from_numpy(PAL))
        arena.put("lut", torch.from_numpy(lut))

    outs = A.run_case(specs, call, DEV, torch.cuda.synchronize, setup=setup)
    toned = R.tone(frames, lut, True)
    idx = R.map_index(toned, PAL, "rgb" if metric == 0 else "nearest")
    assert outs["toned"].cpu().numpy().tobytes() == toned.tobytes()
    assert outs["index"].cpu().numpy().tobytes() == idx.astype(np.uint8).tobytes() and outs["out"].cpu().numpy().tobytes() == PAL[idx].tobytes()
