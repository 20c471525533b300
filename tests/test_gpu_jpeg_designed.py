"""The three device JPEG decoders (csrc/jpeg_decode.hip: adain_jpeg_decode_u8, adain_jpeg_decode_restart_u8, adain_jpeg_decode_progressive_u8) on
the designed files of tests/jpeg_designed.py, which tests/test_jpeg_designed_host.py has settled against Pillow on the host.  Everything is
element-for-element equality (``first_difference(...) is None``): the device's pixels against Pillow's and the restatement's, its rounds
against the lane simulation's, at chunk_bits 32 and at the default; a batch of two designed files per decoder against the two single
calls; and the status files - one designed rule break each, walked on the CPU first - through the guard-band arena (tests/abi_arena.py):
a non-zero status, the guard bands intact, and a good file decoded afterwards in the same workspace gives Pillow's pixels.  Nothing is
asserted about a damaged frame's pixels.

Wall time on an MI355X: the 61 tests of this file take 19 s together; the slowest are the two P-runs files (98 596 blocks each) at 3.3 s
(AC refine) and 1.7 s (AC first), then two 4:2:0 / 4:4:4 files at 1.6 and 1.3 s, every other one under 1 s.  Most of it is the host's share
(Pillow, the restatement and the lane simulation, computed once per file and shared), not the device's."""
import ctypes

import numpy as np
import pytest
import torch

import abi_arena as A
import jpeg_designed as Z
import jpeg_options_ref as O
from test_gpu_jpeg_decode import first_difference
from test_jpeg_designed_host import lanes, restatement
from test_jpeg_file_host import pillow

import applied_image_processing_amd.jpeg_file as F

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


@pytest.fixture(scope="module")
def rt():
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    import applied_image_processing_amd.runtime as rt

    rt.lib()
    torch.cuda.set_device(0)
    return rt


def device_pixels(rt, data, chunk_bits):
    """(pixels, rounds) of one file decoded ON THE DEVICE: a fallback to PIL, which a non-zero status causes too, fails the test."""
    report = []
    out = rt.jpeg_decode_u8([data], DEV, report=report, restart=True, progressive=True, chunk_bits=chunk_bits)
    assert [r["path"] for r in report] == ["device"], report
    return out[0].cpu().numpy(), report[0]["rounds"]


@pytest.mark.parametrize("name", Z.GOOD)
def test_a_designed_file_decodes_to_pillows_pixels_in_the_simulations_rounds(rt, name):
    d = Z.good(name)
    want, ours = pillow(d.data), restatement(name)[0]
    for chunk_bits in ((0,) if name.startswith("P-runs") else (32, 0)):
        got, rounds = device_pixels(rt, d.data, chunk_bits)
        bad = first_difference(got, want)
        assert bad is None, f"{name} at chunk_bits {chunk_bits} against Pillow: {bad}"
        bad = first_difference(got, ours)
        assert bad is None, f"{name} at chunk_bits {chunk_bits} against the restatement: {bad}"
        assert rounds == lanes(name, chunk_bits or 1024)[2], (name, chunk_bits)


# ---- batches: two designed files of one geometry with different tables ---------------------------------------------------------------------------
def pairs():
    tail = [Z.tail_table(Z.DC_SYMBOLS, [10, 11]), Z.tail_table(Z.AC_SYMBOLS, Z.SIZE_10)]
    return {
        "baseline": (dict(), [Z.good("B-symbols grey").data, Z.good("B-lengths chain down grey").data]),
        "restart": (dict(restart=True), [Z.good("B-restart Ri 7 grey").data, Z._baseline(Z.GREY, tail, None, 5, ri=7).data]),
        "progressive": (dict(progressive=True), [Z.good("P-scripts deep approximation grey").data, Z._progressive(Z.GREY, "deep approximation", 99, (3,)).data]),
    }


@pytest.mark.parametrize("decoder", ["baseline", "restart", "progressive"])
def test_a_batch_of_two_equals_two_single_calls(rt, decoder):
    kw, datas = pairs()[decoder]
    parsed = [F.parse(d, **kw) for d in datas]
    assert parsed[0].geometry == parsed[1].geometry
    if decoder == "progressive":
        assert parsed[0].script == parsed[1].script and all(a.blob != b.blob for a, b in zip(parsed[0].scans, parsed[1].scans) if a.ss or not a.ah)
    else:
        assert parsed[0].blob != parsed[1].blob
    entry = rt.jpeg_decode_progressive_batch if decoder == "progressive" else rt.jpeg_decode_batch
    out, record = entry(parsed, datas, DEV)
    assert record[:, 0].cpu().tolist() == [0, 0]
    batch = out.cpu().numpy()
    for i, d in enumerate(datas):
        single, rec = entry(parsed[i:i + 1], [d], DEV)
        assert rec[0].cpu().tolist() == record[i].cpu().tolist()
        bad = first_difference(batch[i], single[0].cpu().numpy())
        assert bad is None, f"file {i} against its single call: {bad}"
        want = pillow(d)
        bad = first_difference(batch[i].reshape(want.shape), want)
        assert bad is None, f"file {i} against Pillow: {bad}"


# ---- the status files, through the guard-band arena ---------------------------------------------------------------------------------------------------
def call_of(rt, data, chunk_bits=0):
    """(files bytes, blobs bytes, workspace bytes, dst bytes, call(arena, prefix)) of one direct call of the C ABI on one file."""
    progressive = Z.is_progressive(data)
    p = F.parse(data, progressive=progressive)
    h, w, c, sampling = p.geometry
    scans = p.scans if progressive else [p]
    segs = [data[s.seg_offset:s.seg_offset + s.seg_length] for s in scans]
    lengths = [len(s) for s in segs]
    offsets = [3 + sum(lengths[:i]) for i in range(len(segs))]
    files, blobs = b"\xa5\xa5\xa5" + b"".join(segs), b"".join(s.blob for s in scans)
    off, ln = (ctypes.c_uint64 * len(segs))(*offsets), (ctypes.c_uint32 * len(segs))(*lengths)
    if progressive:
        desc = []
        for comps, ss, se, ah, al in p.script:
            desc += [len(comps)] + list(comps) + [0] * (3 - len(comps)) + [ss, se, ah, al]
        script = (ctypes.c_int32 * len(desc))(*desc)
        nbytes = rt.jpeg_decode_progressive_sizes(1, h, w, c, sampling, len(scans), max(lengths), chunk_bits)
    else:
        nbytes = rt.jpeg_decode_sizes(1, h, w, c, sampling, max(lengths), chunk_bits, 0)

    def call(arena, prefix):
        stream = torch.cuda.current_stream().cuda_stream
        head = (arena.ptr(prefix + "files"), len(files), arena.ptr(prefix + "blobs"), 1, h, w, c, sampling)
        tail = (arena.ptr("dst"), arena.ptr("record"), arena.ptr("workspace"), arena.nbytes("workspace"), chunk_bits, stream)
        if progressive:
            rc = rt.lib().adain_jpeg_decode_progressive_u8(*head, len(scans), script, off, ln, *tail)
        else:
            rc = rt.lib().adain_jpeg_decode_restart_u8(*head, 0, off, ln, *tail)
        assert rc == 0, rt.lib().adain_last_error().decode()
        torch.cuda.synchronize()
        arena.check()

    return files, blobs, nbytes, h * w * c, call


def good_twin(data):
    """A good file of the damaged file's kind and geometry."""
    progressive = Z.is_progressive(data)
    g = F.parse(data, progressive=progressive).geometry
    coef = Z.random_blocks(7, (g[0] // 8) * (g[1] // 8))
    if progressive:
        return Z.progressive(coef, g, Z.scripts(1)["Pillow's script"], q=[(0, Z.Q1)])
    return Z.baseline(coef, g, O.STANDARD[:2], [(0, Z.Q1)])


@pytest.mark.parametrize("chunk_bits", [32, 0])
@pytest.mark.parametrize("name", Z.STATUS)
def test_a_status_file_gives_a_status_and_stays_in_its_buffers(rt, name, chunk_bits):
    bad, good = Z.status_file(name), good_twin(Z.status_file(name))
    bfiles, bblobs, bws, bdst, bcall = call_of(rt, bad, chunk_bits)
    gfiles, gblobs, gws, gdst, gcall = call_of(rt, good, chunk_bits)
    assert bdst == gdst
    specs = [("bad files", len(bfiles), "in", 1), ("bad blobs", len(bblobs), "in", 1), ("good files", len(gfiles), "in", 1), ("good blobs", len(gblobs), "in", 1),
             ("dst", bdst, "out", 1), ("record", 8, "out", 4), ("workspace", max(bws, gws), "ws", 8)]
    want = pillow(good)
    for fill in A.FILLS:
        arena = A.Arena(specs, fill, DEV)
        for region, content in (("bad files", bfiles), ("bad blobs", bblobs), ("good files", gfiles), ("good blobs", gblobs)):
            arena.put(region, torch.frombuffer(bytearray(content), dtype=torch.uint8))
        bcall(arena, "bad ")
        status = arena.outputs()["record"].cpu().numpy().view(np.int32)[0]
        assert status != 0, f"{name}: status 0 for a file that breaks the rule (fill {fill})"
        gcall(arena, "good ")
        outs = arena.outputs()
        assert outs["record"].cpu().numpy().view(np.int32)[0] == 0
        diff = first_difference(outs["dst"].cpu().numpy().reshape(want.shape), want)
        assert diff is None, f"{name}: the good file decoded behind it in the same workspace (fill {fill}): {diff}"
