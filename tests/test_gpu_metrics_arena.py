"""The memory contract of adain_image_metrics_u8 / adain_image_metrics_f32 through the guard-band arena (tests/abi_arena.py): sources at
every byte offset, no byte outside `out`, the map and the workspace changes, the inputs stay as they were, stale workspace bytes and a
previous call of another shape change nothing, every refusal is ADAIN_EINVAL and writes nothing; and a frame's record does not depend on
the batch it is in or on the stream."""
import json
import os

import numpy as np
import pytest
import torch

import abi_arena as A
import metrics_cases as C
import metrics_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
EINVAL = -1


@pytest.fixture(scope="module")
def rt():
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    import applied_image_processing_amd.runtime as rt

    rt.lib()
    torch.cuda.set_device(0)
    assert rt.lib().adain_image_metrics_u8(None, None, 1, 1, 1, 1, None, None, None, 0, None) == EINVAL          # ADAIN_EINVAL is what a null gets
    return rt


SHAPE = (2, 19, 23, 3)          # n, h, w, c: two tiles down, two across (69 samples a row)
PAIR = C.pair("near", *SHAPE, seed=6)
WANT = R.metrics_u8(*PAIR)
with open(os.path.join(C.GOLDEN, "noise.json")) as _f:
    BARS = json.load(_f)


def padded(frames, offset, pad):
    flat = torch.from_numpy(frames).reshape(-1)
    return torch.cat([torch.full((offset,), 0x5A, dtype=torch.uint8), flat, torch.full((pad - offset,), 0x5A, dtype=torch.uint8)])


# a at `offset` bytes behind a 16-byte boundary and b at another one: every offset 0..15 for either
@pytest.mark.parametrize("offset", range(16))
def test_the_u8_call_stays_in_its_buffers_at_every_source_offset(rt, offset):
    a, b = PAIR
    n, h, w, c = SHAPE
    off_a, off_b = offset, (5 * offset + 3) % 16
    nbytes = rt.image_metrics_sizes(n, h, w, c)
    with_map = offset % 2 == 0
    specs = [("a", a.size + 15, "in", 16), ("b", b.size + 15, "in", 16), ("out", n * 32, "out", 8), ("map", a.size * 4, "out" if with_map else "in", 4),
             ("workspace", nbytes, "ws", 8)]
    stream = torch.cuda.current_stream().cuda_stream

    def call(arena, shape=SHAPE):
        rc = rt.lib().adain_image_metrics_u8(arena.ptr("a") + off_a, arena.ptr("b") + off_b, *shape, arena.ptr("out"), arena.ptr("map") if with_map else None,
                                             arena.ptr("workspace"), nbytes, stream)
        assert rc == 0, rt.lib().adain_last_error().decode()

    def history(arena):          # a call of another shape leaves its partial records, then the workspace is poisoned behind them
        call(arena, (1, 37, 11, 3))
        arena.bytes("workspace")[nbytes // 2:].fill_(0xA5)

    def setup(arena):
        arena.put("a", padded(a, off_a, 15)), arena.put("b", padded(b, off_b, 15))

    outs = A.run_case(specs, call, DEV, torch.cuda.synchronize, history=history, setup=setup)
    got = outs["out"].cpu().numpy().view(np.float64).reshape(n, 4)
    assert got[:, 1].tolist() == WANT["mse"].tolist() and got[:, 2].tolist() == WANT["l1"].tolist()
    assert np.abs(got[:, 0] - WANT["ssim"]).max() <= BARS["bar_frame"]
    if with_map:
        assert np.abs(outs["map"].cpu().numpy().view(np.float32).reshape(a.shape) - WANT["map"]).max() <= BARS["bar_map"]


@pytest.mark.parametrize("offset", [0, 4, 8, 12])
def test_the_f32_call_stays_in_its_buffers(rt, offset):
    fa, fb = C.to_nchw_f32(PAIR[0]), C.to_nchw_f32(PAIR[1])
    n, h, w, c = SHAPE
    nbytes = rt.image_metrics_sizes(n, h, w, c, u8=False)
    specs = [("a", fa.nbytes + 12, "in", 16), ("b", fb.nbytes + 12, "in", 16), ("out", n * 32, "out", 8), ("map", fa.nbytes, "out", 4), ("workspace", nbytes, "ws", 8)]
    stream = torch.cuda.current_stream().cuda_stream
    off_b = (offset + 8) % 16

    def call(arena, shape=(n, c, h, w)):
        rc = rt.lib().adain_image_metrics_f32(arena.ptr("a") + offset, arena.ptr("b") + off_b, *shape, arena.ptr("out"), arena.ptr("map"), arena.ptr("workspace"), nbytes,
                                              stream)
        assert rc == 0, rt.lib().adain_last_error().decode()

    def history(arena):
        call(arena, (1, 2, 40, 9))
        arena.bytes("workspace").fill_(0xA5)

    def setup(arena):
        arena.put("a", padded(fa.view(np.uint8), offset, 12)), arena.put("b", padded(fb.view(np.uint8), off_b, 12))

    outs = A.run_case(specs, call, DEV, torch.cuda.synchronize, history=history, setup=setup)
    got = outs["out"].cpu().numpy().view(np.float64).reshape(n, 4)
    want_map = WANT["map"].transpose(0, 3, 1, 2)
    assert np.abs(got[:, 0] - WANT["ssim"]).max() <= BARS["bar_frame"] and np.abs(outs["map"].cpu().numpy().view(np.float32).reshape(fa.shape) - want_map).max() <= BARS["bar_map"]
    assert np.allclose(got[:, 1], R.metrics_f32(fa, fb)["mse"], rtol=8 * 2.0 ** -24, atol=0)


def test_every_refusal_is_einval_and_writes_nothing(rt):
    a, b = C.pair("near", 2, 9, 11, 3)
    n, h, w, c = a.shape
    nbytes = rt.image_metrics_sizes(n, h, w, c)
    specs = [("a", a.size, "in", 4), ("b", b.size, "in", 4), ("out", n * 32, "out", 8), ("map", a.size * 4, "out", 4), ("workspace", nbytes, "ws", 8)]
    arena = A.Arena(specs, "B", DEV)
    arena.put("a", torch.from_numpy(a)), arena.put("b", torch.from_numpy(b))
    pa, pb, out, smap, ws = (arena.ptr(k) for k in ("a", "b", "out", "map", "workspace"))
    stream = torch.cuda.current_stream().cuda_stream
    good = dict(a=pa, b=pb, n=n, h=h, w=w, c=c, out=out, map=smap, workspace=ws, workspace_bytes=nbytes)
    refusals = [          # (what adain_last_error names, the argument that is wrong)
        ("a is a null", dict(a=None)), ("b is a null", dict(b=None)), ("out is a null", dict(out=None)), ("workspace is a null", dict(workspace=None)),
        ("c other than 1 and 3", dict(c=2)), ("c other than 1 and 3", dict(c=4)), ("n outside", dict(n=0)), ("n outside", dict(n=65536)), ("h below 1", dict(h=0)),
        ("w below 1", dict(w=-2)), ("2^31 - 1 samples", dict(h=65536, w=65536, workspace_bytes=1 << 62)), ("workspace too small", dict(workspace_bytes=nbytes - 1)),
        ("workspace must be 8-byte aligned", dict(workspace=ws + 4)), ("out must be 8-byte aligned", dict(out=out + 4)), ("ssim_map must be 4-byte aligned", dict(map=smap + 2)),
        ("out overlaps a", dict(out=pa + 8 - pa % 8)), ("out overlaps b", dict(out=pb + 8 - pb % 8)), ("ssim_map overlaps a", dict(map=pa + 4)),
        ("ssim_map overlaps b", dict(map=pb - 4 * a.size + 4)), ("workspace overlaps a", dict(workspace=pa - pa % 8)), ("workspace overlaps b", dict(workspace=pb + 8 - pb % 8)),
    ]
    for entry, who in ((rt.lib().adain_image_metrics_u8, "image_metrics_u8"), (rt.lib().adain_image_metrics_f32, "image_metrics_f32")):
        for text, change in refusals:
            v = dict(good, **change)
            dims = (v["n"], v["h"], v["w"], v["c"]) if who.endswith("u8") else (v["n"], v["c"], v["h"], v["w"])
            if not who.endswith("u8"):
                if text.startswith("c other"):
                    text, dims = "c outside 1..4", (v["n"], 5 if v["c"] == 4 else 0, v["h"], v["w"])
            rc = entry(v["a"], v["b"], *dims, v["out"], v["map"], v["workspace"], v["workspace_bytes"], stream)
            message = rt.lib().adain_last_error().decode()
            assert rc == EINVAL, (who, text, rc)
            assert message.startswith(who + ": ") and text in message, (who, text, message)
    assert rt.lib().adain_image_metrics_f32(pa + 2, pb, 1, 1, 4, 4, out, None, ws, nbytes, stream) == EINVAL and "a must be 4-byte aligned" in rt.lib().adain_last_error().decode()
    assert rt.lib().adain_image_metrics_f32(pa, pb + 1, 1, 1, 4, 4, out, None, ws, nbytes, stream) == EINVAL and "b must be 4-byte aligned" in rt.lib().adain_last_error().decode()
    for query in ((0, 4, 4, 3), (1, 0, 4, 3), (1, 4, 4, 2), (1, 65536, 65536, 1)):
        assert rt.lib().adain_image_metrics_u8_bytes(*query, None) == EINVAL
    torch.cuda.synchronize()
    arena.check()
    for name in ("out", "map", "workspace"):
        r = arena.region(name)
        assert bool((arena.bytes(name) == arena._expected(r.offset, r.offset + r.nbytes)).all()), f"a refused call wrote into {name}"


@pytest.mark.parametrize("stream", ["default", "side"])
def test_a_frame_scores_the_same_alone_and_in_a_batch(rt, stream):
    a, b = C.pair("near", 5, 33, 45, 3, seed=7)
    fa, fb = C.to_nchw_f32(a), C.to_nchw_f32(b)
    side = torch.cuda.Stream() if stream == "side" else torch.cuda.current_stream()
    for x, y in ((torch.from_numpy(a).to(DEV), torch.from_numpy(b).to(DEV)), (torch.from_numpy(fa).to(DEV), torch.from_numpy(fb).to(DEV))):
        torch.cuda.synchronize()
        with torch.cuda.stream(side):
            whole = rt.image_metrics(x, y, ssim_map=True)
            alone = [rt.image_metrics(x[i:i + 1], y[i:i + 1], ssim_map=True) for i in range(5)]
        side.synchronize()
        for i in range(5):
            assert torch.equal(whole.records[i].view(torch.int64), alone[i].records[0].view(torch.int64)), i
            assert torch.equal(whole.ssim_map[i], alone[i].ssim_map[0]), i
