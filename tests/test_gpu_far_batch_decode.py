"""Far-batch tests of the file decoders (csrc/jpeg_decode.hip: adain_jpeg_decode_u8, _restart_u8, _progressive_u8; csrc/png_decode.hip:
adain_png_decode_u8): one call of 65535 files whose segments lie behind a lead of more than 2^32 bytes - every ``uint64`` offset of
the host tables is past 2^32 - and whose ``dst`` and workspace pass 2^32 bytes.  The P = 7 parsed files' segments are tiled on the
device group by group and the offsets are computed arithmetically (far_batch.decode_tables); nothing is parsed 65535 times.  Every
status must be 0 and every frame the restatement's pixels for its pattern (jpeg_file_ref, jpeg_restart_ref, jpeg_progressive_ref,
png_decode_ref: equality, the bar of the decoders' own tests); the record's second column (rounds, deflate blocks) must be what the
device reports for the P files alone through runtime.jpeg_decode_parsed / png_decode_batch.  The lead is filled with 0xA5: a segment
read at an offset cut to 32 bits is not a file.  tests/far_batch.py states the design and holds the cases.  Run with ``-m gpu``.

Out of scope here as everywhere in the far-batch tests: the whole-network calls, adain_tvl1_flow / adain_farneback_*, and the
single-frame calls.

Measured on an MI355X, seconds per test (fill, call and comparison):
jpeg_decode/progressive 5.33 (655 350 segments), png_decode 4.59, jpeg_decode/jpeg 1.29, jpeg_decode/restart 0.83."""
import ctypes

import numpy as np
import pytest
import torch

import far_batch as B

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
U64, U32, I32 = ctypes.POINTER(ctypes.c_uint64), ctypes.POINTER(ctypes.c_uint32), ctypes.POINTER(ctypes.c_int32)


@pytest.fixture(scope="module")
def rt():
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    import applied_image_processing_amd.runtime as rt

    rt.lib()
    torch.cuda.set_device(0)
    return rt


def tiled_segments(d, n, group, groups):
    """uint8 [LEAD + groups * group + 1]: 0xA5 in the lead, then the P files' segments group after group."""
    files = B.poisoned((B.LEAD + groups * group + 1,), torch.uint8, DEV)
    one = torch.frombuffer(bytearray(b"".join(d["segments"])), dtype=torch.uint8).to(DEV)
    assert one.numel() == group
    files[B.LEAD:B.LEAD + groups * group].view(groups, group)[:] = one
    return files


@pytest.mark.parametrize("kind", ["jpeg", "restart", "progressive", "png"])
def test_decode(rt, kind):
    case = B.BY_ID["png_decode" if kind == "png" else f"jpeg_decode/{kind}"]
    d = B.decode_files(kind)
    n, h, w = case.n, B.H, B.W
    sizes = dict((b[0], b[2]) for b in case.buffers())
    B.reserve(case, DEV)
    # the P files alone, through the wrapper's door: the restatement's pixels, status 0
    small, small_rec = rt.png_decode_batch(d["parsed"], None, DEV) if kind == "png" else rt.jpeg_decode_parsed(d["parsed"], d["datas"], DEV)
    torch.cuda.synchronize()
    assert np.array_equal(small.cpu().numpy(), d["expected"]) and not small_rec[:, 0].any().item()
    off, ln, group, groups = B.decode_tables(kind, n)
    assert int(off.min()) > B.TWO32
    files = tiled_segments(d, n, group, groups)
    blobs = None if kind == "png" else B.tile(d["blobs"], n, DEV)
    dst = B.poisoned((n, h, w, 3), torch.uint8, DEV)
    record = B.poisoned((n, 2), torch.int32, DEV)
    ws = B.poisoned((sizes["workspace"],), torch.uint8, DEV)
    try:
        assert sum(t.numel() * t.element_size() for t in (files, blobs, dst, record, ws) if t is not None) == case.total_bytes()
        tail = (dst.data_ptr(), record.data_ptr(), ws.data_ptr(), ws.numel())
        streams_bytes = files.numel() - 1
        if kind == "png":
            args = (files.data_ptr(), streams_bytes, off.ctypes.data_as(U64), n, h, w, 3, 3) + tail
        else:
            p = d["parsed"][0]
            tables = (off.ctypes.data_as(U64), ln.ctypes.data_as(U32))
            front = (files.data_ptr(), streams_bytes, blobs.data_ptr(), n, h, w, 3, 2)
            if kind == "progressive":
                desc = []
                for comps, ss, se, ah, al in p.script:
                    desc += [len(comps)] + list(comps) + [0] * (3 - len(comps)) + [ss, se, ah, al]
                scans = np.array(desc, dtype=np.int32)
                args = front + (len(p.script), scans.ctypes.data_as(I32)) + tables + tail + (0,)
            elif kind == "restart":
                args = front + (p.restart_interval,) + tables + tail + (0,)
            else:
                args = front + tables + tail + (0,)
        rt.call(case.call, torch.device(DEV), *args)
        torch.cuda.synchronize()
        failed = torch.nonzero(record[:, 0]).flatten()[:8].tolist()
        assert not failed, f"{case.id}: files {failed} have the statuses {record[failed, 0].tolist()}"
        B.assert_frames(case.id + ": dst", dst, d["expected"])
        B.assert_frames(case.id + ": record", record, small_rec)
        for at in range(0, B.LEAD, B.PIECE):
            assert bool((files[at:min(at + B.PIECE, B.LEAD)] == 0xA5).all()), "the lead changed"
        B.assert_frames(case.id + ": the segments changed", files[B.LEAD:B.LEAD + groups * group].view(groups, group),
                        np.broadcast_to(np.frombuffer(b"".join(d["segments"]), np.uint8), (B.P, group)))
        if blobs is not None:
            B.assert_frames(case.id + ": the tables changed", blobs, d["blobs"])
    finally:
        del files, blobs, dst, record, ws, small, small_rec
        rt.free_workspaces()
        B.release()
