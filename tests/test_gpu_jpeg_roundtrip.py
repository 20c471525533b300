"""The device JPEG round trip (csrc/jpeg.hip, adain_jpeg_roundtrip_u8) and its callers.  Everything here is element-for-element equality:
the device's pixels against the NumPy restatement (tests/jpeg_decode_ref.py) and, in tests of their own, against Pillow's
decode(encode(frame)) - a failure of the first kind says the kernel moved, of the second kind alone that the environment's Pillow /
libjpeg did.  Then batch independence, misaligned buffers, the memory contract through the guard-band arena (tests/abi_arena.py), and
the callers: the engine method against ``video._jpeg_roundtrip`` and the video path with ``intermediate_jpeg`` on both routes."""
import functools
import io

import numpy as np
import pytest
import torch
from PIL import Image

import abi_arena as A
import jpeg_decode_ref as D
import jpeg_ref as J

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
OTHER_QUALITIES = [1, 100]
OTHER_SHAPES = [(17, 9), (37, 53), (9, 5)]


@pytest.fixture(scope="module")
def rt():
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    import applied_image_processing_amd.runtime as rt

    rt.lib()
    torch.cuda.set_device(0)
    return rt


@functools.lru_cache(maxsize=None)
def restatement(kind, h, w, c, quality=75):
    """Computed once per case, shared by the tests and never written to."""
    a = D.roundtrip(J.content(kind, h, w, c), quality)
    a.setflags(write=False)
    return a


def pillow_roundtrip(a, quality=75):
    f = io.BytesIO()
    Image.fromarray(a).save(f, format="JPEG", quality=quality)
    return np.asarray(Image.open(io.BytesIO(f.getvalue())).convert("RGB" if a.ndim == 3 else "L"))


def device_roundtrip(rt, a, quality=75):
    """A frame [h,w,3] or [h,w], or a batch [n,h,w,c], as the device returns it (same shape)."""
    return rt.jpeg_roundtrip_u8(torch.from_numpy(np.ascontiguousarray(a)).to(DEV), quality).cpu().numpy()


def first_difference(got, want):
    """Names the first differing pixel (row, column) and channel of two frames [h,w,3] / [h,w]."""
    assert got.shape == want.shape and got.dtype == want.dtype == np.uint8, f"{got.shape} {got.dtype} against {want.shape} {want.dtype}"
    at = np.argwhere(got != want)
    if len(at) == 0:
        return None
    i = tuple(int(v) for v in at[0])
    return (f"{len(at)} of {got.size} elements differ; the first at pixel (row {i[0]}, column {i[1]}), channel {i[2] if len(i) > 2 else 0}: "
            f"{got[i]} against {want[i]}")


def check(rt, want_of, cases):
    for (h, w, c, kind, quality) in cases:
        a = J.content(kind, h, w, c)
        bad = first_difference(device_roundtrip(rt, a, quality), want_of(a, kind, h, w, c, quality))
        assert bad is None, f"{h}x{w} c={c} {kind} q{quality}: {bad}"


def default_cases(h, w):
    return [(h, w, c, kind, 75) for c in (3, 1) for kind in J.CONTENTS]


def other_cases(quality):
    return [(h, w, c, kind, quality) for (h, w) in OTHER_SHAPES for c in (3, 1) for kind in J.CONTENTS]


from_restatement = lambda a, kind, h, w, c, quality: restatement(kind, h, w, c, quality)
from_pillow = lambda a, kind, h, w, c, quality: pillow_roundtrip(a, quality)


@pytest.mark.parametrize("h,w", D.SHAPES)
def test_device_pixels_are_the_restatements(rt, h, w):
    check(rt, from_restatement, default_cases(h, w))


@pytest.mark.parametrize("quality", OTHER_QUALITIES)
def test_other_qualities_against_the_restatement(rt, quality):
    check(rt, from_restatement, other_cases(quality))


@pytest.mark.parametrize("h,w", D.SHAPES)
def test_device_pixels_are_pillows(rt, h, w):
    check(rt, from_pillow, default_cases(h, w))


@pytest.mark.parametrize("quality", OTHER_QUALITIES)
def test_other_qualities_against_pillow(rt, quality):
    check(rt, from_pillow, other_cases(quality))


def test_input_forms_and_the_default_quality(rt):
    a = J.content("smooth", 37, 53, 3)
    want = restatement("smooth", 37, 53, 3)
    x = torch.from_numpy(a).to(DEV)
    for form, back in ((x, lambda y: y), (x[None], lambda y: y[0])):
        y = rt.jpeg_roundtrip_u8(form)
        assert y.is_cuda and y.dtype == torch.uint8 and y.shape == form.shape and y.data_ptr() != form.data_ptr()
        assert np.array_equal(back(y).cpu().numpy(), want)
    g = J.content("smooth", 37, 53, 1)
    xg = torch.from_numpy(g).to(DEV)
    for form in (xg, xg[..., None], xg[None, ..., None]):
        y = rt.jpeg_roundtrip_u8(form)
        assert y.shape == form.shape and np.array_equal(y.cpu().numpy().reshape(37, 53), restatement("smooth", 37, 53, 1))
    assert bool((x == torch.from_numpy(a).to(DEV)).all())            # the input is left alone


@pytest.mark.parametrize("h,w", [(37, 53), (40, 72)])
@pytest.mark.parametrize("c", [3, 1], ids=["RGB", "L"])
def test_a_batch_of_three_equals_three_single_calls(rt, h, w, c):
    """The middle frame is white: constant, so anything it borrowed from its neighbours' planes or coefficients would show."""
    kinds = ["noise", "white", "binary"]
    frames = np.stack([J.content(kind, h, w, c) for kind in kinds]).reshape(3, h, w, c)
    batch = device_roundtrip(rt, frames)
    for i, kind in enumerate(kinds):
        single = device_roundtrip(rt, frames[i:i + 1])[0]
        bad = first_difference(batch[i], single)
        assert bad is None, f"frame {i} ({kind}): {bad}"
        assert first_difference(single.reshape(J.content(kind, h, w, c).shape), restatement(kind, h, w, c)) is None
    assert len({batch[i].tobytes() for i in range(3)}) == 3


@pytest.mark.parametrize("h,w", [(17, 9), (24, 40)])
@pytest.mark.parametrize("c", [3, 1], ids=["RGB", "L"])
def test_misaligned_buffers(rt, h, w, c):
    """src starts 1 byte and dst 3 bytes into their allocations (torch's are 256-byte aligned at least); two frames, so the second one's
    rows start at yet another phase.  The bytes around dst keep their fill."""
    n, size = 2, 2 * h * w * c
    kinds = ["noise", "smooth"]
    frames = np.stack([J.content(kind, h, w, c) for kind in kinds]).reshape(-1)
    sbuf = torch.zeros(size + 16, dtype=torch.uint8, device=DEV)
    dbuf = torch.full((size + 16,), 0xA5, dtype=torch.uint8, device=DEV)
    assert sbuf.data_ptr() % 4 == 0 and dbuf.data_ptr() % 4 == 0
    sbuf[1:1 + size] = torch.from_numpy(frames).to(DEV)
    nbytes = rt.jpeg_roundtrip_sizes(n, h, w, c)
    ws = torch.empty(nbytes, dtype=torch.uint8, device=DEV)
    rc = rt.lib().adain_jpeg_roundtrip_u8(sbuf.data_ptr() + 1, n, h, w, c, 75, dbuf.data_ptr() + 3, ws.data_ptr(), nbytes,
                                          torch.cuda.current_stream().cuda_stream)
    assert rc == 0, rt.lib().adain_last_error().decode()
    torch.cuda.synchronize()
    got = dbuf.cpu().numpy()
    assert (got[:3] == 0xA5).all() and (got[3 + size:] == 0xA5).all(), "bytes around dst changed"
    out = got[3:3 + size].reshape(n, *J.content("noise", h, w, c).shape)
    for i, kind in enumerate(kinds):
        bad = first_difference(out[i], restatement(kind, h, w, c))
        assert bad is None, f"frame {i} ({kind}): {bad}"


# ---- the memory contract, through the guard-band arena ----------------------------------------------------------------------------------
@pytest.mark.parametrize("n,h,w,c,kind", [(2, 17, 9, 3, "noise"), (2, 64, 64, 1, "binary")])
def test_the_call_stays_in_its_buffers_and_ignores_stale_bytes(rt, n, h, w, c, kind):
    """dst and the workspace start as 0xFF bytes and as a non-zero pattern: the pixels are the same, no byte outside the two regions
    changes; then a smaller call through the same dst and workspace, and the call again: stale coefficients and planes."""
    frames = np.stack([J.content(kind, h, w, c, seed=i) for i in range(n)]).reshape(n, h, w, c)
    nbytes = rt.jpeg_roundtrip_sizes(n, h, w, c)
    specs = [("src", frames.size, "in", 1), ("dst", frames.size, "out", 1), ("workspace", nbytes, "ws", 8)]
    src = torch.from_numpy(frames)
    stream = torch.cuda.current_stream().cuda_stream

    def call(arena, shape=(n, h, w, c)):
        rc = rt.lib().adain_jpeg_roundtrip_u8(arena.ptr("src"), *shape, 75, arena.ptr("dst"), arena.ptr("workspace"), nbytes, stream)
        assert rc == 0, rt.lib().adain_last_error().decode()

    outs = A.run_case(specs, call, DEV, torch.cuda.synchronize, history=lambda arena: call(arena, (1, h // 2, w // 2 + 1, c)),
                      setup=lambda arena: arena.put("src", src))
    got = outs["dst"].cpu().numpy().reshape(n, h, w, c)
    for i in range(n):
        want = D.roundtrip(frames[i] if c == 3 else frames[i, :, :, 0])
        bad = first_difference(got[i].reshape(want.shape), want)
        assert bad is None, f"frame {i}: {bad}"


# ---- the callers ------------------------------------------------------------------------------------------------------------------------
import applied_image_processing_amd.synth as synth


def T(a):
    return torch.from_numpy(np.ascontiguousarray(a))


def u8img(seed, h, w, c=3):
    return (synth.image(seed, 1, h, w, c=c)[0].transpose(1, 2, 0) * 255).astype(np.uint8)


@pytest.fixture(scope="module")
def engine(rt, weights):
    from applied_image_processing_amd.engine import AdaINEngine

    return AdaINEngine(weights[0], weights[1], DEV)


def test_engine_equals_the_host_round_trip(rt, engine):
    from applied_image_processing_amd import video

    frames = np.stack([J.content(kind, 40, 72, 3) for kind in ("noise", "smooth", "binary")])
    got = engine.jpeg_roundtrip_u8(T(frames).to(DEV))
    assert got.is_cuda and got.dtype == torch.uint8 and tuple(got.shape) == (3, 40, 72, 3)
    want = video._jpeg_roundtrip(frames)
    for i in range(3):
        bad = first_difference(got[i].cpu().numpy(), want[i])
        assert bad is None, f"frame {i}: {bad}"
    q90 = engine.jpeg_roundtrip_u8(T(frames).to(DEV), quality=90).cpu().numpy()
    assert all(first_difference(q90[i], pillow_roundtrip(frames[i], 90)) is None for i in range(3))


@pytest.fixture
def clip(tmp_path):
    cdir = tmp_path / "frames"
    cdir.mkdir()
    n = 3
    for i in range(n):
        Image.fromarray(u8img(700 + i, 64, 96)).save(cdir / f"frame_{i:04d}.jpg", quality=95)
    Image.fromarray(u8img(750, 96, 96)).save(tmp_path / "style.png")
    depth_maps = [synth.smooth_depth(480 + i, 64, 96) for i in range(n)]
    return cdir, tmp_path / "style.png", depth_maps, n


def a_flow_provider(prev_frame_path, frame_path, target_resolution, method):
    """A caller's own provider: a smooth, frame-independent displacement field at the target resolution."""
    w, h = target_resolution
    yy, xx = np.mgrid[0:h, 0:w].astype(np.float32)
    return np.stack([1.5 * np.sin(yy / 7.0), 0.75 * np.cos(xx / 5.0)]).astype(np.float32)


class Counter:
    def __init__(self, fn):
        self.fn, self.calls = fn, 0

    def __call__(self, *args, **kwargs):
        self.calls += 1
        return self.fn(*args, **kwargs)


def run_clip(engine, clip, odir, **kw):
    from applied_image_processing_amd import video

    cdir, style, depth_maps, n = clip
    video.set_flow_provider(a_flow_provider)
    try:
        video.apply_style_transfer_ada(str(cdir), str(style), str(odir), alpha=0.7, target_resolution=(96, 64), engine=engine,
                                       depth_maps=depth_maps, **kw)
    finally:
        video.set_flow_provider(None)
    return [(odir / f"frame_{i:04d}.jpg").read_bytes() for i in range(n)]


def test_the_video_path_writes_the_same_files_on_both_routes(rt, engine, clip, tmp_path, monkeypatch):
    from applied_image_processing_amd import video

    device_entry = Counter(rt.jpeg_roundtrip_u8)
    host_route = Counter(video._jpeg_roundtrip)
    monkeypatch.setattr(rt, "jpeg_roundtrip_u8", device_entry)
    monkeypatch.setattr(video, "_jpeg_roundtrip", host_route)
    on = run_clip(engine, clip, tmp_path / "on", intermediate_jpeg=True, jpeg_on_device=True)
    assert device_entry.calls > 0 and host_route.calls == 0
    calls = device_entry.calls
    off = run_clip(engine, clip, tmp_path / "off", intermediate_jpeg=True, jpeg_on_device=False)
    assert device_entry.calls == calls and host_route.calls > 0
    assert on == off
    assert on[0][:2] == b"\xff\xd8" and Image.open(io.BytesIO(on[0])).size == (96, 64)


def test_without_intermediate_jpeg_nothing_changes(rt, engine, clip, tmp_path, monkeypatch):
    from applied_image_processing_amd import video

    device_entry = Counter(rt.jpeg_roundtrip_u8)
    host_route = Counter(video._jpeg_roundtrip)
    monkeypatch.setattr(rt, "jpeg_roundtrip_u8", device_entry)
    monkeypatch.setattr(video, "_jpeg_roundtrip", host_route)
    plain = {on: run_clip(engine, clip, tmp_path / f"plain_{int(on)}", intermediate_jpeg=False, jpeg_on_device=on) for on in (False, True)}
    assert device_entry.calls == 0 and host_route.calls == 0
    assert plain[True] == plain[False]
    lossy = run_clip(engine, clip, tmp_path / "lossy", intermediate_jpeg=True, jpeg_on_device=True)
    assert device_entry.calls > 0 and lossy != plain[True]           # the round trip is not a no-op on these frames
