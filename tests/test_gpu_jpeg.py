"""The device JPEG encoder (csrc/jpeg.hip, adain_jpeg_encode_u8) and its callers.  Everything here is byte equality: the device's
files against the NumPy restatement (tests/jpeg_ref.py) and, in tests of their own, against Pillow's - a failure of the first kind says
the kernel moved, of the second kind alone that the environment's Pillow / libjpeg did.  Then the memory contract through the
guard-band arena (tests/abi_arena.py), and every caller that gained ``jpeg_on_device``: the files written with it on are the files
written with it off."""
import io

import numpy as np
import pytest
import torch
from PIL import Image

import abi_arena as A
import jpeg_ref as J

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
BIG = [(1080, 1920), (1200, 1600)]


@pytest.fixture(scope="module")
def rt():
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    import applied_image_processing_amd.runtime as rt

    rt.lib()
    torch.cuda.set_device(0)
    return rt


def pillow_bytes(a, quality=None):
    f = io.BytesIO()
    Image.fromarray(a).save(f, format="JPEG", **({} if quality is None else {"quality": quality}))
    return f.getvalue()


def device_files(rt, frames, quality=75):
    out, lengths = rt.jpeg_encode_u8(torch.from_numpy(np.ascontiguousarray(frames)).to(DEV), quality)
    return rt.jpeg_files(out, lengths)


def cases(shapes):
    return [(h, w, c, kind) for (h, w) in shapes for c in (3, 1) for kind in J.CONTENTS]


def first_difference(got, want):
    k = next((i for i in range(min(len(got), len(want))) if got[i] != want[i]), min(len(got), len(want)))
    return f"{len(got)} bytes against {len(want)}, first difference at {k}"


@pytest.mark.parametrize("h,w", J.SHAPES + BIG)
def test_device_bytes_are_the_restatements(rt, h, w):
    for c in (3, 1):
        for kind in J.CONTENTS:
            a = J.content(kind, h, w, c)
            got, = device_files(rt, a[None] if c == 3 else a[None, :, :, None])
            want = J.encode(a)
            assert got == want, f"{h}x{w} c={c} {kind}: {first_difference(got, want)}"


@pytest.mark.parametrize("h,w", J.SHAPES + BIG)
def test_device_bytes_are_pillows(rt, h, w):
    for c in (3, 1):
        for kind in J.CONTENTS:
            a = J.content(kind, h, w, c)
            got, = device_files(rt, a[None] if c == 3 else a[None, :, :, None])
            want = pillow_bytes(a)
            assert got == want, f"{h}x{w} c={c} {kind}: {first_difference(got, want)}"


@pytest.mark.parametrize("quality", [1, 30, 50, 90, 95, 100])
def test_other_qualities(rt, quality):
    for (h, w) in [(17, 9), (37, 53), (250, 333)]:
        for c in (3, 1):
            for kind in ("noise", "smooth", "binary"):
                a = J.content(kind, h, w, c)
                got, = device_files(rt, a[None] if c == 3 else a[None, :, :, None], quality)
                assert got == J.encode(a, quality), f"q{quality} {h}x{w} c={c} {kind}: restatement"
                assert got == pillow_bytes(a, quality), f"q{quality} {h}x{w} c={c} {kind}: Pillow"


@pytest.mark.parametrize("h,w,c", [(37, 53, 3), (250, 333, 3), (40, 72, 1)])
def test_batch_of_five_equals_five_single_calls(rt, h, w, c):
    frames = np.stack([J.content(kind, h, w, c, seed=i) for i, kind in enumerate(["noise", "smooth", "binary", "white", "noise"])])
    if c == 1:
        frames = frames[..., None]
    batch = device_files(rt, frames)
    singles = [device_files(rt, frames[i:i + 1])[0] for i in range(5)]
    assert batch == singles
    assert len({len(b) for b in batch}) > 1          # files of different lengths share the call


def test_lengths_are_exact_and_the_rest_of_a_row_is_untouched(rt):
    a = J.content("smooth", 64, 64, 3)
    x = torch.from_numpy(a[None]).to(DEV)
    stride, nbytes = rt.jpeg_encode_sizes(1, 64, 64, 3)
    want = J.encode(a)
    for fill in (0xFF, 0x5A):
        out = torch.full((1, stride), fill, dtype=torch.uint8, device=DEV)
        lengths = torch.full((1,), -1, dtype=torch.int32, device=DEV)
        ws = torch.full((nbytes,), fill, dtype=torch.uint8, device=DEV)
        rc = rt.lib().adain_jpeg_encode_u8(x.data_ptr(), 1, 64, 64, 3, 75, out.data_ptr(), stride, lengths.data_ptr(), ws.data_ptr(), nbytes,
                                           torch.cuda.current_stream().cuda_stream)
        assert rc == 0, rt.lib().adain_last_error().decode()
        torch.cuda.synchronize()
        n = int(lengths[0])
        assert n == len(want) and out[0, :n].cpu().numpy().tobytes() == want
        assert bool((out[0, n:] == fill).all())


def test_refusals_reach_the_caller(rt):
    x = torch.zeros((1, 8, 8, 3), dtype=torch.uint8, device=DEV)
    for bad in (0, 101, 75.0, True):
        with pytest.raises(rt.AdainHipError):
            rt.jpeg_encode_u8(x, bad)
    with pytest.raises(rt.AdainHipError):
        rt.jpeg_encode_u8(torch.zeros((1, 8, 8, 2), dtype=torch.uint8, device=DEV))
    with pytest.raises(rt.AdainHipError):
        rt.jpeg_encode_u8(torch.zeros((1, 8, 8, 3), dtype=torch.uint8))          # a host tensor: no fallback
    stride, nbytes = rt.jpeg_encode_sizes(1, 8, 8, 3)
    out = torch.empty((1, stride), dtype=torch.uint8, device=DEV)
    lengths = torch.empty((1,), dtype=torch.int32, device=DEV)
    ws = torch.empty((nbytes,), dtype=torch.uint8, device=DEV)
    call = lambda s, b: rt.lib().adain_jpeg_encode_u8(x.data_ptr(), 1, 8, 8, 3, 75, out.data_ptr(), s, lengths.data_ptr(), ws.data_ptr(), b, None)
    assert call(stride - 1, nbytes) == -1 and b"out_stride" in rt.lib().adain_last_error()
    assert call(stride, nbytes - 1) == -1 and b"workspace" in rt.lib().adain_last_error()
    assert call(stride, nbytes) == 0
    torch.cuda.synchronize()


# ---- the memory contract, through the guard-band arena ----------------------------------------------------------------------------------
ARENA_CASES = [(1, 1, 1, 3, "noise"), (1, 17, 9, 3, "binary"), (3, 37, 53, 3, "noise"), (2, 40, 72, 1, "binary"), (1, 250, 333, 3, "binary"),
               (1, 256, 456, 3, "smooth"), (1, 1080, 1920, 3, "binary")]


@pytest.mark.parametrize("n,h,w,c,kind", ARENA_CASES)
def test_the_call_stays_in_its_buffers_and_ignores_stale_bytes(rt, n, h, w, c, kind):
    """out, lengths and the workspace start as 0xFF bytes and as a non-zero pattern: the files and lengths are the same, no byte outside
    the three regions changes, none behind a file inside `out` either.  The 0/255 frames are the densest streams these tables give: an
    in-bounds check of the size bound."""
    frames = np.stack([J.content(kind, h, w, c, seed=i) for i in range(n)]).reshape(n, h, w, c)
    stride, nbytes = rt.jpeg_encode_sizes(n, h, w, c)
    specs = [("src", frames.size, "in", 1), ("out", n * stride, "ws", 1), ("lengths", 4 * n, "out", 4), ("workspace", nbytes, "ws", 8)]
    src = torch.from_numpy(frames)
    stream = torch.cuda.current_stream().cuda_stream

    def call(arena, shape=(n, h, w, c)):
        rc = rt.lib().adain_jpeg_encode_u8(arena.ptr("src"), *shape, 75, arena.ptr("out"), stride, arena.ptr("lengths"), arena.ptr("workspace"),
                                           nbytes, stream)
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

    # a much smaller shape (its file is shorter than any of this case's) through the same workspace and `out`, then the call again:
    # stale coefficients, offsets and stream words
    history = (lambda arena: call(arena, (1, h // 8, w // 8, c))) if h >= 16 else None
    outs = A.run_case(specs, call, DEV, torch.cuda.synchronize, history=history, setup=lambda arena: arena.put("src", src), extra=files)
    want = b"".join(J.encode(f if c == 3 else f[..., 0]) for f in frames)
    assert outs["files"].cpu().numpy().tobytes() == want


# ---- the callers ------------------------------------------------------------------------------------------------------------------------
import applied_image_processing_amd.synth as synth


def T(a):
    return torch.from_numpy(np.ascontiguousarray(a))


def u8img(seed, h, w, c=3):
    return (synth.image(seed, 1, h, w, c=c)[0].transpose(1, 2, 0) * 255).astype(np.uint8)


@pytest.fixture(scope="module")
def ckpt(tmp_path_factory):
    d = tmp_path_factory.mktemp("ckpt")
    torch.save(synth.to_torch(synth.vgg_state_dict(0, full=True)), d / "vgg.pth")
    torch.save(synth.to_torch(synth.decoder_state_dict(0)), d / "dec.pth")
    return dict(vgg_str=str(d / "vgg.pth"), decoder_str=str(d / "dec.pth"))


@pytest.fixture(scope="module")
def engine(rt, weights):
    from applied_image_processing_amd.engine import AdaINEngine

    return AdaINEngine(weights[0], weights[1], DEV)


@pytest.fixture
def t():
    from applied_image_processing_amd.AdaIN import test as t

    t.clear_style_cache()
    yield t
    t.set_device_jpeg(False)
    t.set_style_cache(True)
    t.clear_style_cache()


def test_engine_returns_the_files_as_bytes(rt, engine):
    frames = np.stack([J.content(kind, 40, 72, 3) for kind in ("noise", "smooth")])
    got = engine.jpeg_encode_u8(T(frames).to(DEV))
    assert isinstance(got, list) and all(isinstance(b, bytes) for b in got)
    assert got == [pillow_bytes(f) for f in frames]
    assert engine.jpeg_encode_u8(T(frames).to(DEV), 90) == [pillow_bytes(f, 90) for f in frames]


@pytest.mark.parametrize("style_cache", [True, False])
def test_adain_inference_writes_the_same_files_with_the_device_encoder(t, ckpt, tmp_path, style_cache):
    """The plain, depth and masked variants at the sizes of tests/test_gpu_per_call.py, through the cached per-call path and (style cache
    off) the call-by-call path that ends in save_image."""
    style = Image.fromarray(u8img(950, 300, 400))
    frame = u8img(900, 270, 480)
    view = u8img(970, 160, 208)
    view[T(synth.uniform01(2000, 160 * 208).reshape(160, 208) < 0.3).numpy()] = 0
    depth = T(synth.smooth_depth(6, 270, 480))
    variants = {
        "plain": dict(content_img=Image.fromarray(frame), content_size=256),
        "depth": dict(content_img=Image.fromarray(frame), content_size=256, depth_offset=0.30, depth_prominence=20, use_depth=True, depth_map=depth),
        "masked": dict(content_img=Image.fromarray(view), content_size=128, style_size=128, content_mask=view.transpose(2, 0, 1) > 0),
    }
    t.set_style_cache(style_cache)
    for name, kw in variants.items():
        files = {}
        for on in (False, True):
            t.set_device_jpeg(on)
            p = t.adain_inference(style_img=style, output=str(tmp_path / f"{name}_{int(on)}"), file_name=name, **kw, **ckpt)
            assert p.suffix == ".jpg"
            files[on] = p.read_bytes()
        t.set_device_jpeg(False)
        assert files[True] == files[False], f"{name}: {first_difference(files[True], files[False])}"
        assert files[True][:2] == b"\xff\xd8" and files[True][-2:] == b"\xff\xd9"
    # another extension is PIL's as before
    t.set_device_jpeg(True)
    p = t.adain_inference(style_img=style, output=str(tmp_path / "png"), file_name="v", save_ext=".png", **variants["plain"], **ckpt)
    assert Image.open(p).format == "PNG"


def test_precompute_guides_sharded_writes_the_same_files(rt, engine, tmp_path):
    from applied_image_processing_amd import jobs

    pil = [Image.fromarray(u8img(300 + k, 96, 144)) for k in range(5)]
    names = [f"r_{k}" for k in range(5)]
    style = T(synth.image(310, 1, 64, 64))
    masks = [np.asarray(p.resize((72, 48))).transpose(2, 0, 1) > 60 for p in pil]
    for write in ("dst", "local"):
        got = {}
        for on in (False, True):
            paths, info = jobs.precompute_guides_sharded(engine, pil, names, tmp_path / f"{write}_{int(on)}", style, masks=masks, content_size=48,
                                                         write=write, sub_batch=2, jpeg_on_device=on)
            assert [paths[n].name for n in names] == [f"r_{k}.jpg" for k in range(5)]
            got[on] = ([paths[n].read_bytes() for n in names], info["d2h_bytes"])
        assert got[True][0] == got[False][0]
        raw = 5 * 48 * 72 * 3
        assert got[False][1] >= raw and got[True][1] < raw          # the files crossed, not the frames
        assert got[True][1] == sum(len(b) for b in got[True][0]) + 4 * 5


def test_a_png_path_falls_back_to_the_host_encoder(rt, tmp_path):
    from applied_image_processing_amd import jobs

    frames = np.stack([J.content("smooth", 40, 72, 3, seed=i) for i in range(3)])
    block = T(frames).to(DEV)
    sink = jobs.FileSink(torch.device(DEV), jpeg_on_device=True)
    sink.write(block, [tmp_path / "a.jpg", tmp_path / "b.JPEG", tmp_path / "c.jpeg"])
    sink.close()
    on_device = sink.d2h_bytes
    want = [pillow_bytes(f) for f in frames]
    assert [(tmp_path / n).read_bytes() for n in ("a.jpg", "b.JPEG", "c.jpeg")] == want
    assert on_device == sum(len(b) for b in want) + 12 and on_device < frames.size
    sink = jobs.FileSink(torch.device(DEV), jpeg_on_device=True)
    sink.write(block, [tmp_path / "d.jpg", tmp_path / "e.png", tmp_path / "f.jpg"])          # one .png: the whole block goes the old way
    sink.close()
    assert sink.d2h_bytes == frames.size
    assert (tmp_path / "d.jpg").read_bytes() == want[0] and (tmp_path / "f.jpg").read_bytes() == want[2]
    assert Image.open(tmp_path / "e.png").format == "PNG" and np.array_equal(np.asarray(Image.open(tmp_path / "e.png")), frames[1])
    # greyscale blocks
    grey = np.stack([J.content("noise", 17, 9, 1, seed=i) for i in range(2)])
    sink = jobs.FileSink(torch.device(DEV), jpeg_on_device=True)
    sink.write(T(grey[..., None]).to(DEV), [tmp_path / "g0.jpg", tmp_path / "g1.jpg"])
    sink.close()
    assert [(tmp_path / n).read_bytes() for n in ("g0.jpg", "g1.jpg")] == [pillow_bytes(g) for g in grey]


def test_a_short_clip_writes_the_same_files(rt, engine, t, tmp_path):
    from applied_image_processing_amd import video

    cdir = tmp_path / "frames"
    cdir.mkdir()
    n = 4
    for i in range(n):
        Image.fromarray(u8img(700 + i, 72, 128)).save(cdir / f"frame_{i:04d}.jpg", quality=95)
    Image.fromarray(u8img(750, 96, 96)).save(tmp_path / "style.png")
    t.set_depth_provider(lambda img: T(synth.smooth_depth(480 + img.size[0] % 7, img.size[1], img.size[0])))
    video.set_flow_provider(video.device_flow_provider)
    try:
        outs = {}
        for on in (False, True):
            odir = tmp_path / f"out_{int(on)}"
            video.apply_style_transfer_ada(str(cdir), str(tmp_path / "style.png"), str(odir), alpha=0.7, target_resolution=(64, 36), engine=engine,
                                           jpeg_on_device=on)
            outs[on] = [(odir / f"frame_{i:04d}.jpg").read_bytes() for i in range(n)]
    finally:
        t.set_depth_provider(None)
        video.set_flow_provider(None)
    assert outs[True] == outs[False]
    assert Image.open(io.BytesIO(outs[True][0])).size == (64, 36)
