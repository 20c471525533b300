"""The memory contract of adain_png_encode_u8 through the guard-band arena (tests/abi_arena.py): no byte outside `out`, `lengths` and the
workspace changes, none behind a file inside `out` either, and a workspace of stale bytes gives the same files."""
import numpy as np
import pytest
import torch

import abi_arena as A
import png_cases as C
import png_ref as P

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


@pytest.fixture(scope="module")
def rt():
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    import applied_image_processing_amd.runtime as rt

    rt.lib()
    torch.cuda.set_device(0)
    return rt


def frames_of(kind, n, h, w, c):
    rng = np.random.default_rng(h * w + n)
    if kind == "noise":                      # the longest files: the in-bounds check of out_stride
        return rng.integers(0, 256, (n, h, w, c), dtype=np.uint8)
    if kind == "zeros":                      # the shortest: almost all of `out` and the stream stay untouched
        return np.zeros((n, h, w, c), np.uint8)
    return np.stack([C.noisy_gradient(h, w, 20 + i)[:, :, :c] for i in range(n)])


# one block and less, several blocks with a short last one, a batch, grey, forced filters
ARENA_CASES = [(1, 1, 1, 3, "noise", -1), (1, 17, 9, 3, "smooth", -1), (3, 37, 53, 3, "noise", -1), (2, 40, 72, 1, "smooth", 4), (1, 150, 333, 3, "noise", -1),
               (2, 120, 200, 3, "smooth", -1), (1, 64, 100, 3, "zeros", 0)]


@pytest.mark.parametrize("n,h,w,c,kind,filt", ARENA_CASES)
def test_the_call_stays_in_its_buffers_and_ignores_stale_bytes(rt, n, h, w, c, kind, filt):
    frames = frames_of(kind, n, h, w, c)
    stride, nbytes = rt.png_encode_sizes(n, h, w, c)
    specs = [("src", frames.size, "in", 1), ("out", n * stride, "ws", 1), ("lengths", 4 * n, "out", 4), ("workspace", nbytes, "ws", 8)]
    src = torch.from_numpy(frames)
    stream = torch.cuda.current_stream().cuda_stream

    def call(arena, shape=(n, h, w, c)):
        rc = rt.lib().adain_png_encode_u8(arena.ptr("src"), *shape, filt, arena.ptr("out"), stride, arena.ptr("lengths"), arena.ptr("workspace"), nbytes, stream)
        assert rc == 0, rt.lib().adain_last_error().decode()

    def files(arena):
        """The files as one output; behind each, the row still holds the arena's fill."""
        ln = arena.bytes("lengths").view(torch.int32).tolist()
        region = arena.region("out")
        parts = []
        for i, k in enumerate(ln):
            assert 0 < k <= stride
            row = arena.bytes("out")[i * stride:(i + 1) * stride]
            parts.append(row[:k].clone())
            a, b = region.offset + i * stride + k, region.offset + (i + 1) * stride
            assert bool((row[k:] == arena._expected(a, b)).all()), f"frame {i}: bytes behind the file's {k} changed"
        return {"files": torch.cat(parts)}

    # a much smaller shape through the same workspace and `out`, then the call again: stale tokens, tables, offsets and stream words
    history = (lambda arena: call(arena, (1, h // 8, w // 8, c))) if h >= 16 else None
    outs = A.run_case(specs, call, DEV, torch.cuda.synchronize, history=history, setup=lambda arena: arena.put("src", src), extra=files)
    want = b"".join(P.encode(f, None if filt < 0 else filt) for f in frames)
    assert outs["files"].cpu().numpy().tobytes() == want
