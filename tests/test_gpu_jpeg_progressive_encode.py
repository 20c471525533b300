"""The device JPEG encoder's progressive files (csrc/jpeg.hip, adain_jpeg_encode_progressive_u8), held to Pillow's ``save(...,
progressive=True)`` directly: lengths and bytes, no tolerance (tests/test_jpeg_progressive_encode_host.py holds the restatement of the
rules to the same files on the host).  Shapes from one block up, 17 x 23 among them - at 4:2:0 the smallest frame whose luma scans run
over another grid (3 x 3 blocks) than the MCU order (4 x 4) - the two designed frames that reach the cuts of an end-of-band run, batches,
a misaligned source, scans longer than the stuffing kernels' grid (through the baseline and optimize entries too, which share those
kernels), the memory contract, the device's own progressive decoder, and a caller.  An L frame ignores ``subsampling``."""
import io

import numpy as np
import pytest
import torch
from PIL import Image, ImageFile

import abi_arena as A
import jpeg_progressive_encode_ref as R
import jpeg_ref as J

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SHAPES = [(1, 1), (8, 8), (17, 23), (37, 53), (40, 72), (256, 456)]
CONTENTS = ["noise", "smooth", "black", "white"]
MODES = [(3, 0), (3, 1), (3, 2), (1, 1)]          # L at a sampling that must be ignored


@pytest.fixture(scope="module")
def rt():
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    import applied_image_processing_amd.runtime as rt

    rt.lib()
    torch.cuda.set_device(0)
    return rt


def pillow_file(a, quality, subsampling, **kw):
    """Pillow's file under further keywords (ImageFile.MAXBLOCK raised for the call: its buffer is w * h bytes, which a noise frame overruns)."""
    kw["quality"] = quality
    if a.ndim == 3:
        kw["subsampling"] = subsampling
    f = io.BytesIO()
    old, ImageFile.MAXBLOCK = ImageFile.MAXBLOCK, max(ImageFile.MAXBLOCK, 4 * a.size + 4096)
    try:
        Image.fromarray(a).save(f, format="JPEG", **kw)
    finally:
        ImageFile.MAXBLOCK = old
    return f.getvalue()


def pillow_bytes(a, quality=75, subsampling=2):
    """Pillow's progressive file."""
    return pillow_file(a, quality, subsampling, progressive=True)


def nhwc(a):
    return a[None] if a.ndim == 3 else a[None, :, :, None]


def device_files(rt, frames, quality=75, subsampling=2):
    out, lengths = rt.jpeg_encode_u8(torch.from_numpy(np.ascontiguousarray(frames)).to(DEV), quality, subsampling, progressive=True)
    files = rt.jpeg_files(out, lengths)
    assert lengths.cpu().tolist() == [len(f) for f in files]
    return files


def first_difference(got, want):
    k = next((i for i in range(min(len(got), len(want))) if got[i] != want[i]), min(len(got), len(want)))
    return f"{len(got)} bytes against {len(want)}, first difference at {k}"


@pytest.mark.parametrize("h,w", SHAPES)
def test_device_files_are_pillows(rt, h, w):
    for kind in CONTENTS:
        for (c, s) in MODES:
            a = J.content(kind, h, w, c)
            got, = device_files(rt, nhwc(a), 75, s)
            want = pillow_bytes(a, 75, s)
            assert got == want, f"{h}x{w} c={c} {kind} sampling {s}: {first_difference(got, want)}"


@pytest.mark.parametrize("quality", [30, 95, 100])
def test_other_qualities(rt, quality):
    for (h, w) in [(17, 23), (37, 53), (40, 72)]:
        for kind in CONTENTS:
            for (c, s) in MODES:
                a = J.content(kind, h, w, c)
                got, = device_files(rt, nhwc(a), quality, s)
                want = pillow_bytes(a, quality, s)
                assert got == want, f"q{quality} {h}x{w} c={c} {kind} sampling {s}: {first_difference(got, want)}"


def test_optimize_has_no_effect(rt):
    a = J.content("smooth", 37, 53, 3)
    x = torch.from_numpy(a[None]).to(DEV)
    both = [rt.jpeg_files(*rt.jpeg_encode_u8(x, 75, 0, o, True)) for o in (False, True)]
    assert both[0] == both[1] == [pillow_bytes(a, 75, 0)]


@pytest.mark.parametrize("rgb", [False, True], ids=["L", "RGB"])
def test_stripes_cut_a_run_by_its_correction_bits(rt, rgb):
    a = R.stripes()
    a = np.stack([a] * 3, axis=-1) if rgb else a
    got, = device_files(rt, nhwc(a))
    want = pillow_bytes(a)
    assert got == want, first_difference(got, want)


@pytest.mark.parametrize("rgb", [False, True], ids=["L", "RGB"])
def test_a_flat_frame_cuts_its_runs_at_the_cap(rt, rgb):
    a = R.flat()
    a = np.stack([a] * 3, axis=-1) if rgb else a
    got, = device_files(rt, nhwc(a))
    want = pillow_bytes(a)
    assert got == want, first_difference(got, want)


@pytest.mark.parametrize("h,w,c,s", [(37, 53, 3, 2), (17, 23, 3, 1), (40, 72, 1, 2)])
def test_batch_of_three_equals_three_single_calls(rt, h, w, c, s):
    frames = np.stack([J.content(kind, h, w, c, seed=i) for i, kind in enumerate(["noise", "smooth", "white"])]).reshape(3, h, w, c)
    batch = device_files(rt, frames, 75, s)
    assert batch == [device_files(rt, frames[i:i + 1], 75, s)[0] for i in range(3)]
    assert batch == [pillow_bytes(f if c == 3 else f[..., 0], 75, s) for f in frames]


def test_a_source_at_an_odd_address(rt):
    for c in (3, 1):
        a = J.content("noise", 37, 53, c)
        flat = torch.zeros((a.size + 3,), dtype=torch.uint8, device=DEV)
        for shift in (1, 3):
            flat[shift:shift + a.size] = torch.from_numpy(a.reshape(-1)).to(DEV)
            x = flat[shift:shift + a.size].view(1, 37, 53, c)
            assert x.data_ptr() % 4 == (flat.data_ptr() + shift) % 4
            got, = rt.jpeg_files(*rt.jpeg_encode_u8(x, 75, 2, progressive=True))
            assert got == pillow_bytes(a)


# ---- scans longer than the stuffing kernels' grid ---------------------------------------------------------------------------------------
# The back half walks a segment's stream in 1024-byte chunks, 64 workgroups per frame: a workgroup takes a second chunk only in a segment
# beyond 64 x 1024 bytes.  Noise at quality 100 and 4:4:4 is the smallest convenient frame with such scans (128 x 200 stays at 21 KB);
# its progressive file also has scans below one chunk, and its baseline files are one segment of several grids.
LONG = dict(h=256, w=456, quality=100, subsampling=0)
GRID_BYTES = 64 * 1024
ENTRIES = {"baseline": {}, "optimize": {"optimize": True}, "progressive": {"progressive": True}}


def long_frames(n):
    return np.stack([J.content("noise", LONG["h"], LONG["w"], 3, seed=i) for i in range(n)])


def scan_segment_bytes(data):
    """The stuffed bytes of each entropy-coded segment of a JPEG file without restart markers."""
    sizes, at = [], 2
    while data[at + 1] != 0xD9:
        assert data[at] == 0xFF
        marker, at = data[at + 1], at + 2 + int.from_bytes(data[at + 2:at + 4], "big")
        if marker == 0xDA:
            end = at
            while not (data[end] == 0xFF and data[end + 1] != 0x00):
                end += 1
            sizes.append(end - at)
            at = end
    return sizes


@pytest.fixture(scope="module")
def long_pillow():
    """{entry: Pillow's files of long_frames(2)}: computed once."""
    frames = long_frames(2)
    return {name: [pillow_file(f, LONG["quality"], LONG["subsampling"], **kw) for f in frames] for name, kw in ENTRIES.items()}


def test_scans_longer_than_the_stream_grid(rt, long_pillow):
    want = long_pillow["progressive"][0]
    sizes = scan_segment_bytes(want)
    print("stuffed bytes per scan:", sizes)
    assert len(sizes) == 10 and max(sizes) > GRID_BYTES and min(sizes) < 1024, sizes          # the case wraps the grid, and not in every scan
    got, = device_files(rt, long_frames(1), LONG["quality"], LONG["subsampling"])
    assert got == want, first_difference(got, want)


@pytest.mark.parametrize("entry", list(ENTRIES))
def test_a_batch_of_long_segments_through_every_entry(rt, long_pillow, entry):
    """The second frame's chunks lie behind the first frame's in the workspace: more than one grid of them in every entry."""
    frames = long_frames(2)
    want = long_pillow[entry]
    assert all(max(scan_segment_bytes(f)) > GRID_BYTES for f in want)

    def files(x):
        out, lengths = rt.jpeg_encode_u8(torch.from_numpy(x).to(DEV), LONG["quality"], LONG["subsampling"], **ENTRIES[entry])
        return rt.jpeg_files(out, lengths)

    batch = files(frames)
    assert batch == [files(frames[i:i + 1])[0] for i in range(2)]
    assert batch == want, [first_difference(g, w) for g, w in zip(batch, want)]


# ---- the memory contract, through the guard-band arena ----------------------------------------------------------------------------------
@pytest.mark.parametrize("n,h,w,c,s,kind", [(1, 1, 1, 3, 2, "noise"), (3, 37, 53, 3, 2, "noise"), (2, 17, 23, 3, 0, "binary"), (2, 40, 72, 1, 2, "binary"),
                                            (1, 256, 256, 1, 2, "stripes")])
def test_the_call_stays_in_its_buffers_and_ignores_stale_bytes(rt, n, h, w, c, s, kind):
    """out, lengths and the workspace start as 0xFF bytes and as a non-zero pattern: the files and lengths are the same, no byte outside
    the three regions changes, none behind a file inside `out` either; a smaller call through the same workspace in between (stale
    coefficients, run states, symbol counts and code tables) changes nothing."""
    memory_contract(rt, n, h, w, c, s, kind, 75)


def test_the_call_stays_in_its_buffers_with_scans_longer_than_the_grid(rt):
    """The same contract where the stuffing kernels' workgroups take more than one chunk of a scan, in both frames of a batch."""
    memory_contract(rt, 2, LONG["h"], LONG["w"], 3, LONG["subsampling"], "noise", LONG["quality"])


def memory_contract(rt, n, h, w, c, s, kind, quality):
    frames = (np.stack([R.stripes()] * n) if kind == "stripes" else np.stack([J.content(kind, h, w, c, seed=i) for i in range(n)])).reshape(n, h, w, c)
    stride, nbytes = rt.jpeg_encode_sizes(n, h, w, c, s, progressive=True)
    specs = [("src", frames.size, "in", 1), ("out", n * stride, "ws", 1), ("lengths", 4 * n, "out", 4), ("workspace", nbytes, "ws", 8)]
    src = torch.from_numpy(frames)
    stream = torch.cuda.current_stream().cuda_stream

    def call(arena, shape=(n, h, w, c)):
        rc = rt.lib().adain_jpeg_encode_progressive_u8(arena.ptr("src"), *shape, quality, s, arena.ptr("out"), stride, arena.ptr("lengths"),
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

    history = (lambda arena: call(arena, (1, h // 2, w // 2, c))) if h >= 16 else None
    outs = A.run_case(specs, call, DEV, torch.cuda.synchronize, history=history, setup=lambda arena: arena.put("src", src), extra=files)
    want = [pillow_bytes(f if c == 3 else f[..., 0], quality, s) for f in frames]
    assert outs["files"].cpu().numpy().tobytes() == b"".join(want)
    assert outs["lengths"].view(torch.int32).tolist() == [len(b) for b in want]


def test_refusals_launch_nothing(rt):
    L = rt.lib()
    x = torch.zeros((1, 8, 8, 3), dtype=torch.uint8, device=DEV)
    stride, nbytes = rt.jpeg_encode_sizes(1, 8, 8, 3, 0, progressive=True)
    out = torch.full((1, stride), 0x5A, dtype=torch.uint8, device=DEV)
    lengths = torch.full((1,), -1, dtype=torch.int32, device=DEV)
    ws = torch.empty((nbytes,), dtype=torch.uint8, device=DEV)
    call = lambda q, sampling, st, b: L.adain_jpeg_encode_progressive_u8(x.data_ptr(), 1, 8, 8, 3, q, sampling, out.data_ptr(), st, lengths.data_ptr(),
                                                                         ws.data_ptr(), b, None)
    for q, sampling, st, b, what in [(75, 3, stride, nbytes, b"sampling"), (0, 0, stride, nbytes, b"quality"), (75, 0, stride - 1, nbytes, b"out_stride"),
                                     (75, 0, stride, nbytes - 1, b"workspace")]:
        assert call(q, sampling, st, b) == -1 and what in L.adain_last_error() and L.adain_last_error().startswith(b"jpeg_encode_progressive_u8")
    torch.cuda.synchronize()
    assert bool((out == 0x5A).all()) and int(lengths[0]) == -1
    assert call(75, 0, stride, nbytes) == 0
    torch.cuda.synchronize()
    assert out[0, :int(lengths[0])].cpu().numpy().tobytes() == pillow_bytes(np.zeros((8, 8, 3), np.uint8), 75, 0)


# ---- closure without Pillow, and a caller -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("h,w", [(17, 23), (40, 72), (256, 456)])
def test_the_devices_progressive_decoder_reads_the_file_back(rt, h, w):
    for kind in ("noise", "smooth"):
        a = J.content(kind, h, w, 3)
        x = torch.from_numpy(a[None]).to(DEV)
        for quality in (75, 95):
            data, = rt.jpeg_files(*rt.jpeg_encode_u8(x, quality, progressive=True))
            report = []
            back = rt.jpeg_decode_u8(data, DEV, progressive=True, report=report)
            assert report[0]["path"] == "device", report                      # the device's decoder, not PIL's
            assert torch.equal(back[None], rt.jpeg_roundtrip_u8(x, quality)), (kind, quality)


def test_a_caller_writes_the_same_file_on_both_routes(rt, tmp_path):
    from applied_image_processing_amd import jobs

    options = {"quality": 95, "subsampling": "4:2:2", "progressive": True}
    a = J.content("smooth", 40, 72, 3)
    x = torch.from_numpy(a[None]).to(DEV)
    routes = rt.JpegRoutes(encode_on_device=True, options=options)
    routes.write(x, tmp_path / "device.jpg")
    routes.options.save(Image.fromarray(a), tmp_path / "host.jpg")
    assert (tmp_path / "device.jpg").read_bytes() == (tmp_path / "host.jpg").read_bytes() == pillow_bytes(a, 95, 1)
    frames = np.stack([J.content("noise", 40, 72, 3, seed=i) for i in range(2)])
    files = {}
    for on in (False, True):
        d = tmp_path / f"on{int(on)}"
        d.mkdir()
        sink = jobs.FileSink(torch.device(DEV), jpeg_on_device=on, jpeg_options=options)
        sink.write(torch.from_numpy(frames).to(DEV), [d / "a.jpg", d / "b.jpeg"])
        sink.close()
        files[on] = [(d / name).read_bytes() for name in ("a.jpg", "b.jpeg")]
    assert files[True] == files[False] == [pillow_bytes(f, 95, 1) for f in frames]
