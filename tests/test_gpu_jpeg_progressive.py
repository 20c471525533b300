"""The device decoder for progressive JPEG files (csrc/jpeg_decode.hip, adain_jpeg_decode_progressive_u8) and its callers.  Everything here is
element-for-element equality: the device's pixels against Pillow's ``np.asarray(Image.open(...))`` and against the Python restatement
(tests/jpeg_progressive_ref.py), whose lane simulation also predicts the rounds.  Then end-of-band runs at their longest, the chunk size
of the parallel entropy decode, batches, the memory contract through the guard-band arena (tests/abi_arena.py) with stale workspaces
left by a baseline call and by a call with another scan script, refusals, two damaged inputs (walked on the CPU first by
tests/test_jpeg_progressive_host.py), and the callers with their opt-ins."""
import ctypes
import io

import numpy as np
import pytest
import torch
from PIL import Image

import abi_arena as A
import jpeg_progressive_ref as P
import jpeg_ref as J
from test_gpu_jpeg_decode import Counter, a_flow_provider, first_difference, u8img
from test_jpeg_file_host import SHAPES, pillow, save
from test_jpeg_progressive_host import (GOLDEN, damaged_file, damaged_short, damaged_swap, files_of, golden, noise_48x64, restatement, uniform_colour,
                                        uniform_grey)

import applied_image_processing_amd.jpeg_file as F
import applied_image_processing_amd.synth as synth

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


@pytest.fixture(scope="module")
def rt():
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    import applied_image_processing_amd.runtime as rt

    rt.lib()
    torch.cuda.set_device(0)
    return rt


def device_pixels(rt, datas, **kw):
    """The frames of the files as numpy arrays, every one decoded ON THE DEVICE (a fallback to PIL fails the test), and the rounds."""
    report = []
    out = rt.jpeg_decode_u8(list(datas), DEV, report=report, progressive=True, **kw)
    assert [r["path"] for r in report] == ["device"] * len(datas), report
    assert all(o.is_cuda and o.dtype == torch.uint8 for o in out)
    return [o.cpu().numpy() for o in out], [r["rounds"] for r in report]


@pytest.mark.parametrize("h,w", SHAPES)
def test_device_pixels_are_pillows_and_the_restatements(rt, h, w):
    names, datas = zip(*files_of(h, w))
    got, _ = device_pixels(rt, datas)
    for name, data, g in zip(names, datas, got):
        bad = first_difference(g, pillow(data))
        assert bad is None, f"{name} against Pillow: {bad}"
        bad = first_difference(g, restatement(data))
        assert bad is None, f"{name} against the restatement: {bad}"


@pytest.mark.parametrize("name", GOLDEN)
def test_other_encoders_files(rt, name):
    data = golden(name)
    (got,), (rounds,) = device_pixels(rt, [data])
    print(f"{name}: {rounds} rounds")
    bad = first_difference(got, pillow(data))
    assert bad is None, f"{name} against Pillow: {bad}"
    bad = first_difference(got, restatement(data))
    assert bad is None, f"{name} against the restatement: {bad}"


@pytest.mark.parametrize("which", ["grey 1456x1456", "colour 256x456"])
def test_uniform_frames(rt, which):
    """End-of-band runs of 32 767 blocks and of a whole scan: one step of one lane begins them all."""
    data = uniform_grey() if which.startswith("grey") else uniform_colour()
    (got,), _ = device_pixels(rt, [data])
    bad = first_difference(got, pillow(data))
    assert bad is None, bad


# ---- the parallel entropy decode -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["noise q100 4:4:4 48x64", "munch.jpg"])
def test_pixels_do_not_depend_on_chunk_bits(rt, name):
    data = golden(name) if name.endswith(".jpg") else noise_48x64()
    want = pillow(data)
    for chunk_bits in (32, 64, 256, 0):
        (got,), (rounds,) = device_pixels(rt, [data], chunk_bits=chunk_bits)
        bad = first_difference(got, want)
        assert bad is None, f"{name} at chunk_bits {chunk_bits}: {bad}"
        assert rounds >= 2


ROUND_FILES = {
    "noise 17x33 4:2:0": lambda: save(J.content("noise", 17, 33, 3), 75, 2, progressive=True),
    "smooth 33x17 4:2:2": lambda: save(J.content("smooth", 33, 17, 3), 95, 1, progressive=True),
    "grey noise 40x24": lambda: save(J.content("noise", 40, 24, 1), 90, "L", progressive=True),
}


@pytest.mark.parametrize("name", ROUND_FILES)
def test_rounds_are_the_simulations(rt, name):
    """The device runs the scheme tests/jpeg_progressive_ref.py simulates: the same rounds, summed over the Huffman-coded scans."""
    data = ROUND_FILES[name]()
    for chunk_bits in (32, 64, 256, 0):
        _, (rounds,) = device_pixels(rt, [data], chunk_bits=chunk_bits)
        assert rounds == P.decode(data, chunk_bits or 1024)[2], (name, chunk_bits)


# ---- batches ------------------------------------------------------------------------------------------------------------------------------
def batch_of_four():
    h, w = 37, 53
    return [save(J.content("noise", h, w, 3), 50, progressive=True), save(J.content("smooth", h, w, 3), 75, progressive=True),
            save(J.content("white", h, w, 3), 95, progressive=True), save(J.content("binary", h, w, 3), 100, progressive=True)]


@pytest.mark.parametrize("lead", [0, 1, 3])
def test_a_batch_of_four_equals_four_single_calls(rt, lead):
    datas = batch_of_four()
    parsed = [F.parse(d, progressive=True) for d in datas]
    assert len({(p.geometry, p.script) for p in parsed}) == 1
    out, record = rt.jpeg_decode_progressive_batch(parsed, datas, DEV, lead=lead)
    assert record[:, 0].cpu().tolist() == [0, 0, 0, 0]
    batch = out.cpu().numpy()
    for i, d in enumerate(datas):
        single, rec = rt.jpeg_decode_progressive_batch(parsed[i:i + 1], [d], DEV)
        assert rec[0, 0].item() == 0 and rec[0, 1].item() == record[i, 1].item()
        bad = first_difference(batch[i], single[0].cpu().numpy())
        assert bad is None, f"file {i}: {bad}"
        bad = first_difference(batch[i], pillow(d))
        assert bad is None, f"file {i}: {bad}"


def test_two_scripts_go_out_as_two_groups(rt, monkeypatch):
    a, b = J.content("noise", 40, 56, 3), J.content("smooth", 40, 56, 3)
    datas = [save(a, 75, 2, progressive=True), save(a[..., 0], 75, "L", progressive=True), save(b, 90, 2, progressive=True)]
    assert len({F.parse(d, progressive=True).script for d in datas}) == 2
    entry = Counter(rt.jpeg_decode_progressive_batch)
    monkeypatch.setattr(rt, "jpeg_decode_progressive_batch", entry)
    got, _ = device_pixels(rt, datas)
    assert entry.calls == 2
    for d, g in zip(datas, got):
        assert first_difference(g, pillow(d)) is None


def test_a_mixed_list(rt):
    a = J.content("smooth", 33, 17, 3)
    datas = [save(a), save(a, restart_marker_blocks=1), save(a, progressive=True), save(a[..., 1], 75, "L", progressive=True), save(a, 75, 1)]
    report = []
    out = rt.jpeg_decode_u8(datas, DEV, report=report, restart=True, progressive=True)
    assert [r["path"] for r in report] == ["device"] * 5, report
    for d, o in zip(datas, out):
        assert first_difference(o.cpu().numpy(), pillow(d)) is None


def test_without_the_keyword_progressive_files_stay_with_pil(rt, monkeypatch):
    data = save(J.content("noise", 33, 17, 3), 75, 2, progressive=True)
    entry = Counter(rt.jpeg_decode_progressive_batch)
    monkeypatch.setattr(rt, "jpeg_decode_progressive_batch", entry)
    for kw in (dict(), dict(restart=True)):
        report = []
        out = rt.jpeg_decode_u8(data, DEV, report=report, **kw)
        assert report[0]["path"].startswith("host: progressive"), report
        assert first_difference(out.cpu().numpy(), pillow(data)) is None
    assert entry.calls == 0


# ---- the memory contract, through the guard-band arena ----------------------------------------------------------------------------------
def abi_case(rt, datas, parsed=None, chunk_bits=0):
    """(specs, setup, call, geometry) of one direct call of the C ABI on the progressive files ``datas``."""
    parsed = parsed or [F.parse(d, progressive=True) for d in datas]
    n, nscans = len(datas), len(parsed[0].scans)
    h, w, c, sampling = parsed[0].geometry
    segs = [d[sc.seg_offset:sc.seg_offset + sc.seg_length] for d, p in zip(datas, parsed) for sc in p.scans]
    lengths = [len(s) for s in segs]
    offsets = [3 + sum(lengths[:i]) for i in range(len(segs))]
    files = b"\xa5\xa5\xa5" + b"".join(segs)
    blobs = b"".join(sc.blob for p in parsed for sc in p.scans)
    desc = []
    for comps, ss, se, ah, al in parsed[0].script:
        desc += [len(comps)] + list(comps) + [0] * (3 - len(comps)) + [ss, se, ah, al]
    nbytes = rt.jpeg_decode_progressive_sizes(n, h, w, c, sampling, nscans, max(lengths), chunk_bits)
    specs = [("files", len(files), "in", 1), ("blobs", len(blobs), "in", 1), ("dst", n * h * w * c, "out", 1), ("record", 8 * n, "out", 4),
             ("workspace", nbytes, "ws", 8)]
    scans = (ctypes.c_int32 * len(desc))(*desc)
    off, ln = (ctypes.c_uint64 * len(segs))(*offsets), (ctypes.c_uint32 * len(segs))(*lengths)

    def setup(arena):
        arena.put("files", torch.frombuffer(bytearray(files), dtype=torch.uint8))
        arena.put("blobs", torch.frombuffer(bytearray(blobs), dtype=torch.uint8))

    def call(arena):
        rc = rt.lib().adain_jpeg_decode_progressive_u8(arena.ptr("files"), len(files), arena.ptr("blobs"), n, h, w, c, sampling, nscans, scans, off, ln,
                                                       arena.ptr("dst"), arena.ptr("record"), arena.ptr("workspace"), arena.nbytes("workspace"), chunk_bits,
                                                       torch.cuda.current_stream().cuda_stream)
        assert rc == 0, rt.lib().adain_last_error().decode()

    return specs, setup, call, (n, h, w, c)


ARENA_CASES = {
    "two grey 8x40": lambda: [save(J.content("noise", 8, 40, 1, seed=i), 90, "L", progressive=True) for i in range(2)],
    "two 4:2:0 17x33": lambda: [save(J.content("noise", 17, 33, 3, seed=i), 90, 2, progressive=True) for i in range(2)],
}


@pytest.mark.parametrize("stale", ["a baseline call", "another script"])
@pytest.mark.parametrize("name", ARENA_CASES)
def test_the_call_stays_in_its_buffers_and_ignores_stale_bytes(rt, name, stale):
    """dst, the record and the workspace start as 0xFF bytes and as a non-zero pattern: the same pixels and record, no byte outside the
    three regions changes; then another call through the same workspace - the baseline decoder's, or this one with another scan script -
    and the call again: stale streams, states, masks, coefficients and planes."""
    datas = ARENA_CASES[name]()
    specs, setup, call, (n, h, w, c) = abi_case(rt, datas)
    stream = torch.cuda.current_stream().cuda_stream
    if stale == "a baseline call":
        other = save(J.content("noise", 8, 8, 3), 75, 2)
        op = F.parse(other)
        up = torch.frombuffer(bytearray(op.blob + other[op.seg_offset:op.seg_offset + op.seg_length]), dtype=torch.uint8).to(DEV)
        assert rt.jpeg_decode_sizes(1, 8, 8, 3, 2, op.seg_length, 32) <= specs[4][1] and 8 * 8 * 3 <= n * h * w * c

        def history(arena):
            off, ln = (ctypes.c_uint64 * 1)(0), (ctypes.c_uint32 * 1)(op.seg_length)
            rc = rt.lib().adain_jpeg_decode_u8(up.data_ptr() + F.BLOB_BYTES, op.seg_length, up.data_ptr(), 1, 8, 8, 3, 2, off, ln, arena.ptr("dst"),
                                               arena.ptr("record"), arena.ptr("workspace"), arena.nbytes("workspace"), 32, stream)
            assert rc == 0, rt.lib().adain_last_error().decode()
    else:
        other = [save(J.content("noise", 8, 8, 3), 75, 0, progressive=True)] if c == 1 else [save(J.content("noise", 8, 16, 1), 75, "L", progressive=True)]
        ospecs, osetup, ocall, (on, oh, ow, oc) = abi_case(rt, other, chunk_bits=32)
        assert ospecs[4][1] <= specs[4][1] and on * oh * ow * oc <= n * h * w * c
        assert F.parse(other[0], progressive=True).script != F.parse(datas[0], progressive=True).script
        oarena = A.Arena(ospecs[:2], "A", DEV)
        osetup(oarena)

        class Both:             # the other call's inputs from its own arena, its outputs and workspace in the arena under test
            def __init__(self, arena):
                self.arena = arena

            def ptr(self, name):
                return (oarena if name in ("files", "blobs") else self.arena).ptr(name)

            def nbytes(self, name):
                return self.arena.nbytes(name)

        def history(arena):
            ocall(Both(arena))

    outs = A.run_case(specs, call, DEV, torch.cuda.synchronize, history=history, setup=setup)
    record = outs["record"].cpu().numpy().view(np.int32).reshape(n, 2)
    assert record[:, 0].tolist() == [0] * n and (record[:, 1] >= 2).all()
    got = outs["dst"].cpu().numpy().reshape(n, h, w, c)
    for i, d in enumerate(datas):
        want = pillow(d)
        bad = first_difference(got[i].reshape(want.shape), want)
        assert bad is None, f"file {i}: {bad}"


def test_refusals_come_before_any_launch(rt):
    data = save(J.content("smooth", 16, 16, 3), 75, 2, progressive=True)
    p = F.parse(data, progressive=True)
    L = rt.lib()
    nscans = len(p.scans)
    up = torch.frombuffer(bytearray(b"".join(sc.blob for sc in p.scans) + data), dtype=torch.uint8).to(DEV)
    blobs = nscans * F.BLOB_BYTES
    dst = torch.zeros(16 * 16 * 3, dtype=torch.uint8, device=DEV)
    record = torch.full((2,), 77, dtype=torch.int32, device=DEV)
    longest = max(sc.seg_length for sc in p.scans)
    nbytes = rt.jpeg_decode_progressive_sizes(1, 16, 16, 3, 2, nscans, longest)
    ws = torch.empty(nbytes, dtype=torch.uint8, device=DEV)
    stream = torch.cuda.current_stream().cuda_stream
    script = [[len(comps)] + list(comps) + [0] * (3 - len(comps)) + [ss, se, ah, al] for comps, ss, se, ah, al in p.script]

    def call(n=1, h=16, w=16, c=3, sampling=2, nscans=nscans, script=script, offset=None, files_bytes=len(data), nbytes=nbytes, chunk_bits=0, ws_ptr=ws.data_ptr()):
        flat = [v for d in script for v in d] + [0] * 8 * 40
        scans = (ctypes.c_int32 * len(flat))(*flat)
        offs = [sc.seg_offset for sc in p.scans] + [0] * 40
        if offset is not None:
            offs[0] = offset
        lens = [sc.seg_length for sc in p.scans] + [0] * 40
        off, ln = (ctypes.c_uint64 * len(offs))(*offs), (ctypes.c_uint32 * len(lens))(*lens)
        return L.adain_jpeg_decode_progressive_u8(up.data_ptr() + blobs, files_bytes, up.data_ptr(), n, h, w, c, sampling, nscans, scans, off, ln, dst.data_ptr(),
                                                  record.data_ptr(), ws_ptr, nbytes, chunk_bits, stream)

    def patched(k, **kw):
        names = ["ncomp", "c0", "c1", "c2", "ss", "se", "ah", "al"]
        out = [list(d) for d in script]
        for key, v in kw.items():
            out[k][names.index(key)] = v
        return out

    for kw in (dict(nscans=0), dict(nscans=33), dict(script=patched(1, ss=5, se=4)), dict(script=patched(1, se=64)), dict(script=patched(1, ncomp=3)),
               dict(script=patched(0, se=5)), dict(script=patched(1, c0=3)), dict(script=patched(2, al=14)), dict(nbytes=nbytes - 1),
               dict(n=0), dict(c=2), dict(sampling=3), dict(c=1, sampling=2), dict(h=0), dict(w=65536), dict(chunk_bits=31), dict(chunk_bits=48),
               dict(offset=len(data)), dict(ws_ptr=ws.data_ptr() + 4)):
        assert call(**kw) == -1 and L.adain_last_error().startswith(b"jpeg_decode_progressive_u8"), kw
    size = ctypes.c_size_t()
    for bad in (0, 33):
        assert L.adain_jpeg_decode_progressive_u8_bytes(1, 16, 16, 3, 2, bad, longest, 0, ctypes.byref(size)) == -1
    torch.cuda.synchronize()
    assert record.cpu().tolist() == [77, 77] and int(dst.sum()) == 0
    assert call() == 0
    torch.cuda.synchronize()
    assert record[0].item() == 0 and first_difference(dst.cpu().numpy().reshape(16, 16, 3), pillow(data)) is None
    with pytest.raises(rt.AdainHipError):
        rt.jpeg_decode_progressive_sizes(1, 16, 16, 3, 2, nscans, 1 << 28)


# ---- damage: two fixed inputs, walked on the CPU by tests/test_jpeg_progressive_host.py ---------------------------------------------------------
def pil_outcome(data):
    try:
        with Image.open(io.BytesIO(data)) as img:
            return np.asarray(img), None
    except Exception as e:                       # whatever PIL raises for these bytes
        return None, type(e)


@pytest.mark.parametrize("kind", ["a shortened scan", "another scan's tables"])
def test_damaged_scans(rt, kind, monkeypatch):
    data = damaged_short() if kind == "a shortened scan" else damaged_file()
    parsed = F.parse(data, progressive=True)
    if kind != "a shortened scan":
        parsed = damaged_swap(parsed)
    _, record = rt.jpeg_decode_progressive_batch([parsed], [data], DEV, chunk_bits=32)
    assert record[0, 0].item() != 0
    _, record = rt.jpeg_decode_progressive_batch([parsed], [data], DEV)
    assert record[0, 0].item() != 0
    monkeypatch.setattr(F, "parse", lambda d, restart=False, progressive=False: parsed)
    want, error = pil_outcome(data)
    if error is not None:
        with pytest.raises(error):
            rt.jpeg_decode_u8(data, DEV, progressive=True)
        return
    report = []
    got = rt.jpeg_decode_u8(data, DEV, report=report, progressive=True).cpu().numpy()
    assert report[0]["path"].startswith("host:"), report
    assert first_difference(got, want) is None


# ---- the callers ------------------------------------------------------------------------------------------------------------------------
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
    t.set_device_jpeg_decode(False)
    t.clear_style_cache()


def test_adain_inference_decodes_a_progressive_content_on_the_device(rt, t, ckpt, tmp_path, monkeypatch):
    content = tmp_path / "content.jpg"
    Image.fromarray(u8img(900, 48, 64)).save(content, quality=90, progressive=True)
    style = Image.fromarray(u8img(950, 40, 56))
    new, old = Counter(rt.jpeg_decode_progressive_batch), Counter(rt.jpeg_decode_batch)
    monkeypatch.setattr(rt, "jpeg_decode_progressive_batch", new)
    monkeypatch.setattr(rt, "jpeg_decode_batch", old)
    files = {}
    for on in (False, True):
        assert t.set_device_jpeg_decode(on, progressive=on) is False
        p = t.adain_inference(str(content), style, content_size=32, style_size=32, output=str(tmp_path / f"out_{int(on)}"), file_name="x", **ckpt)
        files[on] = p.read_bytes()
        assert (new.calls, old.calls) == (1 if on else 0, 0)
        assert t.set_device_jpeg_decode(False) is on
    assert files[True] == files[False]
    # today's switch alone keeps the file with PIL
    t.set_device_jpeg_decode(True)
    p = t.adain_inference(str(content), style, content_size=32, style_size=32, output=str(tmp_path / "out_plain"), file_name="x", **ckpt)
    assert (new.calls, old.calls) == (1, 0) and p.read_bytes() == files[False]
    assert t.set_device_jpeg_decode(False) is True


def test_the_video_path_writes_the_same_frames(rt, engine, tmp_path, monkeypatch):
    from applied_image_processing_amd import video

    cdir = tmp_path / "frames"
    cdir.mkdir()
    Image.fromarray(u8img(700, 64, 96)).save(cdir / "frame_0000.jpg", quality=95)
    Image.fromarray(u8img(701, 64, 96)).save(cdir / "frame_0001.jpg", quality=95, progressive=True)
    Image.fromarray(u8img(702, 64, 96)).save(cdir / "frame_0002.jpg", quality=95)
    Image.fromarray(u8img(750, 96, 96)).save(tmp_path / "style.png")
    depth_maps = [synth.smooth_depth(480 + i, 64, 96) for i in range(3)]
    new, old = Counter(rt.jpeg_decode_progressive_batch), Counter(rt.jpeg_decode_batch)
    monkeypatch.setattr(rt, "jpeg_decode_progressive_batch", new)
    monkeypatch.setattr(rt, "jpeg_decode_batch", old)
    out = {}
    for on in (False, True):
        video.set_flow_provider(a_flow_provider)
        try:
            video.apply_style_transfer_ada(str(cdir), str(tmp_path / "style.png"), str(tmp_path / f"out_{int(on)}"), alpha=0.7, target_resolution=(96, 64),
                                           engine=engine, depth_maps=depth_maps, jpeg_decode_on_device=on, jpeg_decode_progressive=on)
        finally:
            video.set_flow_provider(None)
        out[on] = [(tmp_path / f"out_{int(on)}" / f"frame_{i:04d}.jpg").read_bytes() for i in range(3)]
        assert (new.calls, old.calls) == ((1, 2) if on else (0, 0))
    assert out[True] == out[False]
    assert video._routes.get() == rt.JpegRoutes()          # the clip's routes are call-scoped: the default again afterwards


def test_jpeg_decode_rgb_file_takes_a_progressive_file_only_with_the_keyword(rt, tmp_path):
    path = tmp_path / "p.jpg"
    Image.fromarray(u8img(5, 33, 47)).save(path, quality=85, progressive=True)
    assert rt.jpeg_decode_rgb_file(str(path), DEV) is None
    got = rt.jpeg_decode_rgb_file(str(path), DEV, progressive=True)
    assert first_difference(got.cpu().numpy(), np.asarray(Image.open(path).convert("RGB"))) is None
    grey = tmp_path / "g.jpg"
    Image.fromarray(u8img(6, 33, 47)[..., 0]).save(grey, quality=85, progressive=True)
    got = rt.jpeg_decode_rgb_file(str(grey), DEV, progressive=True)
    assert first_difference(got.cpu().numpy(), np.asarray(Image.open(grey).convert("RGB"))) is None
