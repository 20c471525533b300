"""adain_gif_encode_u8 on the device: the records are byte for byte the restatement's (tests/gif_ref.py) on the cases of
tests/gif_cases.py, alone and inside a batch, at odd addresses; a frame with an index that is not below K gets length 0 and leaves its
neighbours alone; the assembled file plays in Pillow as the frames."""
import functools
import io

import numpy as np
import pytest
import torch
from PIL import Image

import gif_cases as C
import gif_ref as G

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


@pytest.fixture(scope="module")
def rt():
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    import applied_image_processing_amd.runtime as rt

    rt.lib()
    torch.cuda.set_device(0)
    return rt


@functools.lru_cache(maxsize=None)
def want(kind, K, h, w, seed, delay):
    return G.record(C.indices(kind, K, h, w, seed), K, delay)


def records(rt, idx, K, delay):
    """[bytes] of a call through the Python wrapper; the row behind every record is checked to be within the stride."""
    out, lengths = rt.gif_encode_u8(torch.from_numpy(np.ascontiguousarray(idx)).to(DEV), K, delay)
    stride = rt.gif_encode_sizes(idx.shape[0], *idx.shape[1:], K)[0]
    assert out.shape == (idx.shape[0], stride) and lengths.dtype == torch.int32
    ln = lengths.cpu().tolist()
    assert all(0 < k <= stride for k in ln)
    host = out.cpu().numpy()
    return [host[i, :k].tobytes() for i, k in enumerate(ln)]


@pytest.mark.parametrize("h,w", C.SHAPES)
@pytest.mark.parametrize("K", C.KS)
def test_records_are_the_restatements_alone_and_in_a_batch(rt, K, h, w):
    """Batch 3: the flat, the run and the noise frame of this K and shape in one call; batch 1: each of them alone - the same bytes."""
    delay = 5 + K
    frames = np.stack([C.indices(kind, K, h, w) for kind in C.KINDS])
    expect = [want(kind, K, h, w, 0, delay) for kind in C.KINDS]
    assert records(rt, frames, K, delay) == expect
    for i in range(3):
        assert records(rt, frames[i:i + 1], K, delay) == expect[i:i + 1], C.KINDS[i]


@pytest.mark.parametrize("K,h,w,seed,D", C.EDGES)
def test_the_sub_block_edges(rt, K, h, w, seed, D):
    expect = want("noise", K, h, w, seed, 0)
    assert len(expect) == 20 + D + (D + 254) // 255
    assert records(rt, C.indices("noise", K, h, w, seed)[None], K, 0) == [expect]
    frames = np.stack([C.indices("noise", K, h, w, s) for s in (7, seed, 8)])
    assert records(rt, frames, K, 0) == [want("noise", K, h, w, s, 0) for s in (7, seed, 8)]


def test_the_delay_and_the_frame_size_are_little_endian(rt):
    idx = C.indices("run", 5, 2, 300)
    rec, = records(rt, idx[None], 5, 0x1234)
    assert rec == G.record(idx, 5, 0x1234) and rec[4:6] == b"\x34\x12" and rec[13:17] == b"\x2c\x01\x02\x00"


@pytest.mark.parametrize("off_index,off_out", [(1, 1), (3, 0), (0, 5)])
def test_index_and_out_at_odd_addresses(rt, off_index, off_out):
    n, K, h, w = 2, 129, 17, 241
    idx = C.clip(n, K, h, w)
    stride, nbytes = rt.gif_encode_sizes(n, h, w, K)
    src = torch.zeros(idx.size + 8, dtype=torch.uint8, device=DEV)
    src[off_index:off_index + idx.size] = torch.from_numpy(idx.reshape(-1)).to(DEV)
    out = torch.full((n * stride + 8,), 0xa5, dtype=torch.uint8, device=DEV)
    lengths = torch.zeros(n, dtype=torch.int32, device=DEV)
    ws = torch.empty(nbytes, dtype=torch.uint8, device=DEV)
    assert (src.data_ptr() + off_index) % 2 == off_index % 2 and ws.data_ptr() % 8 == 0
    rc = rt.lib().adain_gif_encode_u8(src.data_ptr() + off_index, n, h, w, K, 9, out.data_ptr() + off_out, stride, lengths.data_ptr(), ws.data_ptr(), nbytes,
                                      torch.cuda.current_stream().cuda_stream)
    assert rc == 0, rt.lib().adain_last_error().decode()
    torch.cuda.synchronize()
    host, ln = out.cpu().numpy(), lengths.cpu().tolist()
    for i in range(n):
        row = host[off_out + i * stride:off_out + (i + 1) * stride]
        assert row[:ln[i]].tobytes() == G.record(idx[i], K, 9)
        assert (row[ln[i]:] == 0xa5).all(), "bytes behind the record were written"
    assert (host[:off_out] == 0xa5).all() and (host[off_out + n * stride:] == 0xa5).all()


def test_an_index_that_is_not_below_K_gives_length_zero_and_spares_the_neighbours(rt):
    from applied_image_processing_amd import gif_file

    n, K, h, w = 3, 5, 17, 241
    idx = C.clip(n, K, h, w)
    good = [G.record(f, K, 4) for f in idx]
    for where, value in ((0, 5), (h * w - 1, 255), (2048, 8)):          # the first and the last pixel, a segment's first; K, the largest byte, CLEAR
        bad = idx.copy()
        bad[1].reshape(-1)[where] = value
        out, lengths = rt.gif_encode_u8(torch.from_numpy(bad).to(DEV), K, 4)
        ln = lengths.cpu().tolist()
        assert ln == [len(good[0]), 0, len(good[2])]
        host = out.cpu().numpy()
        assert host[0, :ln[0]].tobytes() == good[0] and host[2, :ln[2]].tobytes() == good[2]
        with pytest.raises(ValueError, match=r"frame\(s\) \[1\]"):
            gif_file.assemble(gif_file.header((w, h), C.palette(K)), out, lengths)
    # the refused frame's row is not written
    stride, nbytes = rt.gif_encode_sizes(n, h, w, K)
    out = torch.full((n, stride), 0xa5, dtype=torch.uint8, device=DEV)
    lengths = torch.full((n,), -1, dtype=torch.int32, device=DEV)
    ws = torch.empty(nbytes, dtype=torch.uint8, device=DEV)
    src = torch.from_numpy(bad).to(DEV)
    rc = rt.lib().adain_gif_encode_u8(src.data_ptr(), n, h, w, K, 4, out.data_ptr(), stride, lengths.data_ptr(), ws.data_ptr(), nbytes,
                                      torch.cuda.current_stream().cuda_stream)
    assert rc == 0, rt.lib().adain_last_error().decode()
    torch.cuda.synchronize()
    assert lengths.cpu().tolist()[1] == 0 and bool((out[1] == 0xa5).all())


@pytest.mark.parametrize("n,K,h,w,kind,loop", [(1, 2, 23, 89, "run", None), (3, 16, 17, 241, "noise", 0), (4, 256, 45, 91, "noise", 2), (2, 129, 64, 100, "flat", 0)])
def test_the_assembled_file_plays_in_pillow_as_the_frames(rt, n, K, h, w, kind, loop):
    from applied_image_processing_amd import gif_file
    from applied_image_processing_amd.engine import AdaINEngine

    idx, pal = C.clip(n, K, h, w, kind), C.palette(K)
    recs, lengths = AdaINEngine.gif_encode_u8(None, torch.from_numpy(idx).to(DEV), K, 5)
    data = gif_file.assemble(gif_file.header((w, h), pal, loop), recs, lengths)
    assert data == G.file(idx, pal, 5, loop)
    im = Image.open(io.BytesIO(data))
    assert im.n_frames == n and im.size == (w, h)
    for i in range(n):
        im.seek(i)
        assert np.array_equal(np.asarray(im.convert("RGB")), pal[idx[i]]) and im.info["duration"] == 50
    assert im.info.get("loop") == loop
