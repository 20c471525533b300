"""The device JPEG encoder's option path (csrc/jpeg.hip, adain_jpeg_encode_opt_u8): Pillow's ``subsampling`` (4:4:4, 4:2:2, 4:2:0) and
``optimize`` keywords.  Everything here is byte equality.  The device's files against the NumPy restatement (tests/jpeg_options_ref.py)
and, in tests of their own, against Pillow's - a failure of the first kind says the kernel moved, of the second kind alone that the
environment's Pillow / libjpeg did.  Then the defaults (the old entry's bytes), batches, the memory contract through the guard-band
arena (tests/abi_arena.py), the refusals, and every caller that takes ``jpeg_options``: the files written with ``jpeg_on_device`` on
are the files written with it off.  An L frame ignores ``subsampling``: its file is the one Pillow writes without the keyword."""
import io

import numpy as np
import pytest
import torch
from PIL import Image, ImageFile

import abi_arena as A
import jpeg_options_ref as R
import jpeg_ref as J

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SHAPES = J.SHAPES + [(9, 17), (15, 31), (16, 33), (1, 2), (2, 1)]
COMBOS = [(s, o) for s in (0, 1, 2) for o in (0, 1)]


@pytest.fixture(scope="module")
def rt():
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    import applied_image_processing_amd.runtime as rt

    rt.lib()
    torch.cuda.set_device(0)
    return rt


def pillow_bytes(a, quality=75, subsampling=2, optimize=False):
    """Pillow's file.  Its encoder buffer for optimize is w * h bytes, which a noise frame at 4:4:4 overruns ("broken data stream"):
    ImageFile.MAXBLOCK, Pillow's documented knob, is raised for the call."""
    kw = dict(quality=quality, optimize=bool(optimize))
    if a.ndim == 3:
        kw["subsampling"] = subsampling
    f = io.BytesIO()
    old, ImageFile.MAXBLOCK = ImageFile.MAXBLOCK, max(ImageFile.MAXBLOCK, 4 * a.size + 4096)
    try:
        Image.fromarray(a).save(f, format="JPEG", **kw)
    finally:
        ImageFile.MAXBLOCK = old
    return f.getvalue()


def nhwc(a):
    return a[None] if a.ndim == 3 else a[None, :, :, None]


def device_files(rt, frames, quality=75, subsampling=2, optimize=0):
    out, lengths = rt.jpeg_encode_u8(torch.from_numpy(np.ascontiguousarray(frames)).to(DEV), quality, subsampling, bool(optimize))
    return rt.jpeg_files(out, lengths)


def first_difference(got, want):
    k = next((i for i in range(min(len(got), len(want))) if got[i] != want[i]), min(len(got), len(want)))
    return f"{len(got)} bytes against {len(want)}, first difference at {k}"


def grid(h, w):
    """(c, subsampling, optimize) of a shape: RGB x sampling x optimize, L x optimize (at a sampling that must be ignored)."""
    return [(3, s, o) for (s, o) in COMBOS] + [(1, 1, 0), (1, 0, 1)]


@pytest.mark.parametrize("h,w", SHAPES)
def test_device_bytes_are_the_restatements(rt, h, w):
    for kind in J.CONTENTS:
        for (c, s, o) in grid(h, w):
            a = J.content(kind, h, w, c)
            got, = device_files(rt, nhwc(a), 75, s, o)
            want = R.encode(a, 75, s, bool(o))
            assert got == want, f"{h}x{w} c={c} {kind} sampling {s} optimize {o}: {first_difference(got, want)}"


@pytest.mark.parametrize("h,w", SHAPES)
def test_device_bytes_are_pillows(rt, h, w):
    for kind in J.CONTENTS:
        for (c, s, o) in grid(h, w):
            a = J.content(kind, h, w, c)
            got, = device_files(rt, nhwc(a), 75, s, o)
            want = pillow_bytes(a, 75, s, o)
            assert got == want, f"{h}x{w} c={c} {kind} sampling {s} optimize {o}: {first_difference(got, want)}"


@pytest.mark.parametrize("quality", [1, 50, 95, 100])
def test_other_qualities(rt, quality):
    for (h, w) in [(17, 9), (37, 53), (250, 333)]:
        for kind in J.CONTENTS:
            for (c, s, o) in grid(h, w):
                a = J.content(kind, h, w, c)
                got, = device_files(rt, nhwc(a), quality, s, o)
                assert got == R.encode(a, quality, s, bool(o)), f"q{quality} {h}x{w} c={c} {kind} sampling {s} optimize {o}: restatement"
                assert got == pillow_bytes(a, quality, s, o), f"q{quality} {h}x{w} c={c} {kind} sampling {s} optimize {o}: Pillow"


@pytest.mark.parametrize("s,o", COMBOS)
def test_a_1080p_frame_is_the_restatements(rt, s, o):
    for kind in ("noise", "smooth"):
        a = J.content(kind, 1080, 1920, 3)
        got, = device_files(rt, a[None], 75, s, o)
        want = R.encode(a, 75, s, bool(o))
        assert got == want, f"{kind}: {first_difference(got, want)}"


@pytest.mark.parametrize("s,o", COMBOS)
def test_a_1080p_frame_is_pillows(rt, s, o):
    for kind in ("noise", "smooth"):
        a = J.content(kind, 1080, 1920, 3)
        got, = device_files(rt, a[None], 75, s, o)
        want = pillow_bytes(a, 75, s, o)
        assert got == want, f"{kind}: {first_difference(got, want)}"


def test_the_length_limited_table_is_pillows(rt):
    """Fixture A: the AC table's unrestricted tree is deeper than 16, so the table stage's Annex K.3 step runs."""
    frame, counts = R.fixture_a()
    freq = np.zeros(256, np.int64)
    freq[0] = frame.size // 64
    for sym, n in counts.items():
        freq[sym] = n
    assert max(R.code_sizes(freq)) > 16
    got, = device_files(rt, frame[None, :, :, None], R.FIXTURE_A_QUALITY, 2, 1)
    want = pillow_bytes(frame, R.FIXTURE_A_QUALITY, 2, True)
    assert got == want, first_difference(got, want)
    at = want.index(b"\xff\xc4", want.index(b"\xff\xc4") + 2)          # the second DHT: AC0
    assert list(want[at + 5:at + 21]) == [1] * 13 + [0, 0, 7]


@pytest.mark.parametrize("h,w", J.SHAPES)
def test_the_defaults_are_the_old_entry(rt, h, w):
    """adain_jpeg_encode_opt_u8 at (4:2:0, no optimize) through its own size query = adain_jpeg_encode_u8, sizes included."""
    L = rt.lib()
    stream = torch.cuda.current_stream().cuda_stream
    for c in (3, 1):
        frames = np.stack([J.content(kind, h, w, c) for kind in J.CONTENTS]).reshape(5, h, w, c)
        x = torch.from_numpy(frames).to(DEV)
        stride, nbytes = rt.jpeg_encode_sizes(5, h, w, c, 2, False)
        old_stride, old_bytes = A_sizes(rt, 5, h, w, c)
        assert (stride, nbytes) == (old_stride, old_bytes)
        results = []
        for opt in (True, False):
            out = torch.zeros((5, stride), dtype=torch.uint8, device=DEV)
            lengths = torch.zeros((5,), dtype=torch.int32, device=DEV)
            ws = torch.empty((nbytes,), dtype=torch.uint8, device=DEV)
            if opt:
                rc = L.adain_jpeg_encode_opt_u8(x.data_ptr(), 5, h, w, c, 75, 2, 0, out.data_ptr(), stride, lengths.data_ptr(), ws.data_ptr(), nbytes, stream)
            else:
                rc = L.adain_jpeg_encode_u8(x.data_ptr(), 5, h, w, c, 75, out.data_ptr(), stride, lengths.data_ptr(), ws.data_ptr(), nbytes, stream)
            assert rc == 0, L.adain_last_error().decode()
            results.append(rt.jpeg_files(out, lengths))
        assert results[0] == results[1]
        assert results[0] == [J.encode(f if c == 3 else f[..., 0]) for f in frames]


def A_sizes(rt, n, h, w, c):
    import ctypes

    s, b = ctypes.c_size_t(), ctypes.c_size_t()
    assert rt.lib().adain_jpeg_encode_u8_bytes(n, h, w, c, ctypes.byref(s), ctypes.byref(b)) == 0
    return s.value, b.value


def dht_segments(data):
    """The DHT segments of a file's header, in order."""
    segs, at = [], 2
    while data[at + 1] != 0xDA:
        n = int.from_bytes(data[at + 2:at + 4], "big")
        if data[at + 1] == 0xC4:
            segs.append(data[at:at + 2 + n])
        at += 2 + n
    return segs, at


@pytest.mark.parametrize("s,o", [(0, 1), (1, 1)])
@pytest.mark.parametrize("h,w,c", [(37, 53, 3), (250, 333, 3), (40, 72, 1)])
def test_batch_of_five_equals_five_single_calls(rt, h, w, c, s, o):
    frames = np.stack([J.content(kind, h, w, c, seed=i) for i, kind in enumerate(["noise", "smooth", "binary", "white", "noise"])]).reshape(5, h, w, c)
    batch = device_files(rt, frames, 75, s, o)
    singles = [device_files(rt, frames[i:i + 1], 75, s, o)[0] for i in range(5)]
    assert batch == singles
    assert batch == [pillow_bytes(f if c == 3 else f[..., 0], 75, s, o) for f in frames]
    headers = [dht_segments(b) for b in batch]
    assert len({tuple(segs) for segs, _ in headers}) == 5          # five different sets of optimal tables
    assert len({sos for _, sos in headers}) > 1                     # and header lengths that differ inside one call


# ---- the memory contract, through the guard-band arena ----------------------------------------------------------------------------------
ARENA_SHAPES = [(1, 1, 1, 3, "noise"), (1, 17, 9, 3, "binary"), (3, 37, 53, 3, "noise"), (2, 37, 53, 1, "binary"), (1, 250, 333, 3, "binary"),
                (1, 1080, 1920, 3, "binary")]


@pytest.mark.parametrize("s,o", [(0, 1), (1, 0), (2, 1)])
@pytest.mark.parametrize("n,h,w,c,kind", ARENA_SHAPES)
def test_the_call_stays_in_its_buffers_and_ignores_stale_bytes(rt, n, h, w, c, kind, s, o):
    """out, lengths and the workspace start as 0xFF bytes and as a non-zero pattern: the files and lengths are the same, no byte outside
    the three regions changes, none behind a file inside `out` either; a smaller call through the same workspace in between (stale
    coefficients, symbol counts and code tables) changes nothing.  The 0/255 frames are the densest streams: an in-bounds check of the
    size bound."""
    frames = np.stack([J.content(kind, h, w, c, seed=i) for i in range(n)]).reshape(n, h, w, c)
    stride, nbytes = rt.jpeg_encode_sizes(n, h, w, c, s, bool(o))
    specs = [("src", frames.size, "in", 1), ("out", n * stride, "ws", 1), ("lengths", 4 * n, "out", 4), ("workspace", nbytes, "ws", 8)]
    src = torch.from_numpy(frames)
    stream = torch.cuda.current_stream().cuda_stream

    def call(arena, shape=(n, h, w, c)):
        rc = rt.lib().adain_jpeg_encode_opt_u8(arena.ptr("src"), *shape, 75, s, o, arena.ptr("out"), stride, arena.ptr("lengths"),
                                               arena.ptr("workspace"), nbytes, stream)
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

    history = (lambda arena: call(arena, (1, h // 8, w // 8, c))) if h >= 16 else None
    outs = A.run_case(specs, call, DEV, torch.cuda.synchronize, history=history, setup=lambda arena: arena.put("src", src), extra=files)
    want = [pillow_bytes(f if c == 3 else f[..., 0], 75, s, o) for f in frames]
    assert outs["files"].cpu().numpy().tobytes() == b"".join(want)
    assert outs["lengths"].view(torch.int32).tolist() == [len(b) for b in want]


def test_refusals_reach_the_caller(rt):
    L = rt.lib()
    x = torch.zeros((1, 8, 8, 3), dtype=torch.uint8, device=DEV)
    for bad in ("keep", -1, 3, "4:1:1", None, True, 1.0):
        with pytest.raises(rt.AdainHipError, match="subsampling"):
            rt.jpeg_encode_u8(x, 75, bad)
    for bad in (2, -1, "yes", None, 1.0):
        with pytest.raises(rt.AdainHipError, match="optimize"):
            rt.jpeg_encode_u8(x, 75, 0, bad)
    with pytest.raises(rt.AdainHipError, match="quality"):
        rt.jpeg_encode_u8(x, True, 0, True)
    with pytest.raises(rt.AdainHipError, match="GPU tensor"):
        rt.jpeg_encode_u8(torch.zeros((1, 8, 8, 3), dtype=torch.uint8), 75, "4:4:4", True)          # a host tensor: no fallback
    stride, nbytes = rt.jpeg_encode_sizes(1, 8, 8, 3, 0, True)
    out = torch.full((1, 2 * stride), 0x5A, dtype=torch.uint8, device=DEV)
    lengths = torch.full((1,), -1, dtype=torch.int32, device=DEV)
    ws = torch.empty((2 * nbytes,), dtype=torch.uint8, device=DEV)
    call = lambda sampling, optimize, st, b: L.adain_jpeg_encode_opt_u8(x.data_ptr(), 1, 8, 8, 3, 75, sampling, optimize, out.data_ptr(), st,
                                                                        lengths.data_ptr(), ws.data_ptr(), b, None)
    for sampling, optimize, what in [(3, 0, b"sampling"), (-1, 0, b"sampling"), (0, 2, b"optimize"), (0, -1, b"optimize")]:
        assert call(sampling, optimize, stride, nbytes) == -1 and what in L.adain_last_error() and L.adain_last_error().startswith(b"jpeg_encode_opt_u8")
    assert call(0, 1, stride - 1, nbytes) == -1 and b"out_stride" in L.adain_last_error()
    assert call(0, 1, stride, nbytes - 1) == -1 and b"workspace" in L.adain_last_error()
    # the old entry's sizes are below this query's at (4:2:0, optimize): they are refused too
    old_stride, old_bytes = A_sizes(rt, 1, 8, 8, 3)
    big_stride, big_bytes = rt.jpeg_encode_sizes(1, 8, 8, 3, 2, True)
    assert old_stride < big_stride <= stride * 2 and old_bytes < big_bytes <= nbytes * 2
    assert call(2, 1, old_stride, big_bytes) == -1 and call(2, 1, big_stride, old_bytes) == -1
    torch.cuda.synchronize()
    assert bool((out == 0x5A).all()) and int(lengths[0]) == -1          # nothing was launched
    assert call(0, 1, stride, nbytes) == 0
    torch.cuda.synchronize()
    assert int(lengths[0]) == 283                                        # a constant 8 x 8 RGB frame: four single-code tables, 3 blocks
    assert call(2, 1, big_stride, big_bytes) == 0
    torch.cuda.synchronize()
    assert int(lengths[0]) == 285                                        # 6 blocks


# ---- the callers: one JpegOptions, two routes, the same files ------------------------------------------------------------------------------
import applied_image_processing_amd.synth as synth

OPTIONS = [(95, "4:4:4", True), (75, 1, False)]


def T(a):
    return torch.from_numpy(np.ascontiguousarray(a))


def u8img(seed, h, w, c=3):
    return (synth.image(seed, 1, h, w, c=c)[0].transpose(1, 2, 0) * 255).astype(np.uint8)


def shows(data, options, rt):
    """The file's header up to its first DHT is the one of these options (quality in the DQTs, the layout in SOF0), and its tables are
    Annex K's exactly when optimize is off."""
    o = rt.JpegOptions.of(options)
    img = Image.open(io.BytesIO(data))
    c = 3 if img.mode == "RGB" else 1
    want = R.header(img.size[1], img.size[0], c, o.quality, o.subsampling if c == 3 else 0, R.STANDARD[:4 if c == 3 else 2])
    cut = want.index(b"\xff\xc4")
    return data[:cut] == want[:cut] and (data[:len(want)] == want) == (not o.optimize)


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
    t.set_jpeg_save_options()
    t.set_style_cache(True)
    t.clear_style_cache()


def test_engine_returns_the_files_as_bytes(rt, engine):
    frames = np.stack([J.content(kind, 40, 72, 3) for kind in ("noise", "smooth")])
    got = engine.jpeg_encode_u8(T(frames).to(DEV), 95, "4:4:4", True)
    assert got == [pillow_bytes(f, 95, 0, True) for f in frames]
    assert engine.jpeg_encode_u8(T(frames).to(DEV), subsampling=1) == [pillow_bytes(f, 75, 1, False) for f in frames]
    assert engine.jpeg_encode_u8(T(frames).to(DEV)) == [J.encode(f) for f in frames]


@pytest.mark.parametrize("options", OPTIONS + [None])
def test_file_sink_writes_the_same_files_on_both_routes(rt, tmp_path, options):
    from applied_image_processing_amd import jobs

    o = rt.JpegOptions.of(options)
    frames = np.stack([J.content("smooth", 40, 72, 3, seed=i) for i in range(3)])
    grey = np.stack([J.content("noise", 17, 9, 1, seed=i) for i in range(2)])
    files = {}
    for on in (False, True):
        d = tmp_path / f"on{int(on)}"
        d.mkdir()
        sink = jobs.FileSink(torch.device(DEV), jpeg_on_device=on, jpeg_options=options)
        sink.write(T(frames).to(DEV), [d / "a.jpg", d / "b.JPEG", d / "c.jpeg"])
        sink.close()
        encoded = sink.d2h_bytes
        sink = jobs.FileSink(torch.device(DEV), jpeg_on_device=on, jpeg_options=options)
        sink.write(T(frames).to(DEV), [d / "d.jpg", d / "e.png", d / "f.jpg"])          # one .png: the whole block goes the old way
        sink.write(T(grey[..., None]).to(DEV), [d / "g0.jpg", d / "g1.jpg"])
        sink.close()
        files[on] = {p.name: p.read_bytes() for p in sorted(d.iterdir())}
        if on:
            assert encoded == sum(len(files[on][n]) for n in ("a.jpg", "b.JPEG", "c.jpeg")) + 12          # the files crossed, not the frames
        else:
            assert encoded == frames.size
    assert files[True] == files[False]
    want = [pillow_bytes(f, o.quality, o.subsampling, o.optimize) for f in frames]
    assert [files[True][n] for n in ("a.jpg", "b.JPEG", "c.jpeg", "d.jpg", "f.jpg")] == want + [want[0], want[2]]
    assert [files[True][n] for n in ("g0.jpg", "g1.jpg")] == [pillow_bytes(g, o.quality, 0, o.optimize) for g in grey]
    plain = io.BytesIO()
    Image.fromarray(frames[1]).save(plain, format="PNG")
    assert files[True]["e.png"] == plain.getvalue()                                      # the .png never sees the options
    if options is None:
        assert want == [J.encode(f) for f in frames]                                     # no options: today's bytes


@pytest.mark.parametrize("options", OPTIONS + [None])
def test_precompute_guides_sharded_writes_the_same_files(rt, engine, tmp_path, options):
    from applied_image_processing_amd import jobs

    pil = [Image.fromarray(u8img(300 + k, 96, 144)) for k in range(5)]
    names = [f"r_{k}" for k in range(5)]
    style = T(synth.image(310, 1, 64, 64))
    masks = [np.asarray(p.resize((72, 48))).transpose(2, 0, 1) > 60 for p in pil]
    got = {}
    for on in (False, True):
        paths, info = jobs.precompute_guides_sharded(engine, pil, names, tmp_path / f"on{int(on)}", style, masks=masks, content_size=48, write="local",
                                                     sub_batch=2, jpeg_on_device=on, jpeg_options=options)
        got[on] = [paths[n].read_bytes() for n in names]
    assert got[True] == got[False]
    assert all(shows(b, options, rt) and Image.open(io.BytesIO(b)).size == (72, 48) for b in got[True])
    if options is None:          # no options: the bytes of a call that does not know the keyword
        paths, _ = jobs.precompute_guides_sharded(engine, pil, names, tmp_path / "plain", style, masks=masks, content_size=48, write="local", sub_batch=2)
        assert [paths[n].read_bytes() for n in names] == got[True]


@pytest.mark.parametrize("options", OPTIONS + [None])
def test_a_short_clip_writes_the_same_files(rt, engine, t, tmp_path, options):
    from applied_image_processing_amd import video

    cdir = tmp_path / "frames"
    cdir.mkdir()
    n = 3
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
                                           jpeg_on_device=on, jpeg_options=options)
            outs[on] = [(odir / f"frame_{i:04d}.jpg").read_bytes() for i in range(n)]
    finally:
        t.set_depth_provider(None)
        video.set_flow_provider(None)
    assert outs[True] == outs[False]
    assert all(shows(b, options, rt) and Image.open(io.BytesIO(b)).size == (64, 36) for b in outs[True])


@pytest.mark.parametrize("style_cache", [True, False])
def test_adain_inference_honours_the_save_options_on_both_routes(rt, t, ckpt, tmp_path, style_cache):
    """Through the cached per-call path and (style cache off) the call-by-call path that ends in save_image."""
    style = Image.fromarray(u8img(950, 300, 400))
    frame = Image.fromarray(u8img(900, 270, 480))
    t.set_style_cache(style_cache)
    for k, options in enumerate(OPTIONS + [None]):
        o = rt.JpegOptions.of(options)
        assert isinstance(t.set_jpeg_save_options(o.quality, o.subsampling, o.optimize), rt.JpegOptions)
        files = {}
        for on in (False, True):
            t.set_device_jpeg(on)
            p = t.adain_inference(content_img=frame, style_img=style, content_size=256, output=str(tmp_path / f"{k}_{int(on)}"), file_name="v", **ckpt)
            files[on] = p.read_bytes()
        t.set_device_jpeg(False)
        assert files[True] == files[False], f"{options}: {first_difference(files[True], files[False])}"
        assert shows(files[True], options, rt)
    # another extension never sees the options
    t.set_jpeg_save_options(95, "4:4:4", True)
    t.set_device_jpeg(True)
    p = t.adain_inference(content_img=frame, style_img=style, content_size=256, output=str(tmp_path / "png"), file_name="v", save_ext=".png", **ckpt)
    assert Image.open(p).format == "PNG"


@pytest.mark.parametrize("options", OPTIONS + [None])
def test_the_localized_pipeline_saves_its_composite_on_the_device(rt, weights, tmp_path, options):
    from applied_image_processing_amd import localized as L

    torch.save(synth.to_torch(synth.vgg_state_dict(0, full=True)), tmp_path / "vgg.pth")
    torch.save(weights[1], tmp_path / "dec.pth")
    Image.fromarray(u8img(430, 64, 96)).save(tmp_path / "c.png")
    Image.fromarray(u8img(431, 64, 64)).save(tmp_path / "s.png")
    yy, xx = np.mgrid[:64, :96]
    bgmask = (((yy - 30) ** 2 + (xx - 50) ** 2) > 300).astype(np.uint8)[None]
    kw = dict(file_name="loc", vgg_str=str(tmp_path / "vgg.pth"), decoder_str=str(tmp_path / "dec.pth"), content_size=0, save_ext=".png",
              background_mask=bgmask, colour_on_device=True)
    files = {}
    for on in (False, True):
        p = L.run_localized_style_transfer(str(tmp_path / "c.png"), str(tmp_path / "s.png"), output_path=str(tmp_path / f"on{int(on)}"), jpeg_on_device=on,
                                           jpeg_options=options, **kw)
        assert p == f"{tmp_path / f'on{int(on)}'}/localized_style_transfer_result.jpg"
        files[on] = open(p, "rb").read()
    assert files[True] == files[False] and shows(files[True], options, rt)
    if options is None:
        p = L.run_localized_style_transfer(str(tmp_path / "c.png"), str(tmp_path / "s.png"), output_path=str(tmp_path / "plain"), **kw)
        assert open(p, "rb").read() == files[True]
    # the host composite (colour_on_device off) goes up for the encode: the same file as PIL's from that composite
    kw["colour_on_device"] = False
    both = [open(L.run_localized_style_transfer(str(tmp_path / "c.png"), str(tmp_path / "s.png"), output_path=str(tmp_path / f"h{int(on)}"),
                                                jpeg_on_device=on, jpeg_options=options, **kw), "rb").read() for on in (False, True)]
    assert both[0] == both[1]
