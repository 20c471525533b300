"""The memory contract of adain_png_decode_u8 through the guard-band arena (tests/abi_arena.py): guard bytes around every buffer, the
streams and the frames at odd addresses, a workspace of stale bytes.  No byte outside `out`, `record` and the workspace changes, the
streams are only read, and the frames do not depend on what the workspace held - also when damaged files ride in the same call."""
import ctypes

import numpy as np
import pytest
import torch

import abi_arena as A
import png_decode_cases as C

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


@pytest.fixture(scope="module")
def rt():
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    import applied_image_processing_amd.runtime as rt

    rt.lib()
    torch.cuda.set_device(0)
    return rt


def streams_of(datas):
    import applied_image_processing_amd.png_file as png_file

    parsed = [png_file.parse(d) for d in datas]
    assert len({p.geometry for p in parsed}) == 1
    offsets = [0]
    for p in parsed:
        offsets.append(offsets[-1] + len(p.stream))
    return parsed[0], b"".join(p.stream for p in parsed), offsets


def sound(name):
    return next(c for c in C.sound() if c.name == name)


def run(rt, datas, c_out, compare_out=True, history_of=None):
    """The call on ``datas`` in the arena -> (frames [n,h,w,c_out] uint8, record [n,2])."""
    p, streams, offsets = streams_of(datas)
    n, h, w, c = len(datas), p.h, p.w, p.c
    nbytes = rt.png_decode_sizes(n, h, w, c, max(b - a for a, b in zip(offsets, offsets[1:])))
    specs = [("streams", len(streams), "in", 1), ("out", n * h * w * c_out, "out" if compare_out else "ws", 1), ("record", 8 * n, "out", 4),
             ("workspace", nbytes, "ws", 8)]
    stream = torch.cuda.current_stream().cuda_stream

    def call(arena, n=n, h=h, w=w, off=offsets):
        rc = rt.lib().adain_png_decode_u8(arena.ptr("streams"), len(streams), (ctypes.c_uint64 * (n + 1))(*off[:n + 1]), n, h, w, c, c_out, arena.ptr("out"),
                                          arena.ptr("record"), arena.ptr("workspace"), nbytes, stream)
        assert rc == 0, rt.lib().adain_last_error().decode()

    kept = {}

    def extra(arena):
        kept["out"] = arena.bytes("out").clone()
        return {}

    # one file of the batch alone through the same workspace, then the call again: stale offsets, statuses and filtered rows
    history = (lambda arena: call(arena, n=1)) if n > 1 else None
    outs = A.run_case(specs, call, DEV, torch.cuda.synchronize, history=history, setup=lambda arena: arena.put("streams", torch.frombuffer(bytearray(streams), dtype=torch.uint8)),
                      extra=extra)
    record = outs["record"].cpu().view(torch.int32).reshape(n, 2).numpy()
    return kept["out"].cpu().numpy().reshape(n, h, w, c_out), record


@pytest.mark.parametrize("names,c_out", [(["1x1_RGB"], 3), (["rowbytes_5"], 1), (["height_65", "height_65"], 3), (["filter_mixed_rgba"], 3), (["filter_mixed_rgba"], 4),
                                         (["zlib_stored", "zlib_fixed", "zlib_default", "zlib_sync_flush", "idat_every_byte"], 3), (["hand_far"], 3),
                                         (["zlib_stored_two"], 3)])
def test_the_call_stays_in_its_buffers_and_ignores_stale_bytes(rt, names, c_out):
    cases = [sound(nm) for nm in names]
    out, record = run(rt, [c.data for c in cases], c_out)
    assert not record[:, 0].any()
    for k, c in enumerate(cases):
        want = c.pixels if c_out == c.c else np.repeat(c.pixels, 3, 2) if c.c == 1 else c.pixels[:, :, :3]
        assert np.array_equal(out[k], want), names[k]


def test_damaged_files_in_the_call_stay_in_their_own_frame(rt):
    px = C.gradient(2, 4, 1, 60)
    good = C.file_of(px, [1, 2])
    damaged = [c for c in C.damaged() if (c.h, c.w, c.c) == (2, 4, 1)]
    datas = [good]
    for d in damaged:
        datas += [d.data, good]
    out, record = run(rt, datas, 1, compare_out=False)          # a damaged file's frame is unspecified: `out` may differ between the fills there
    assert record[0::2, 0].tolist() == [0] * (len(damaged) + 1) and record[1::2, 0].tolist() == [d.status for d in damaged]
    for k in range(0, len(datas), 2):
        assert np.array_equal(out[k], px), f"file {k}"
