"""adain_gif_decode_u8 indexes with size_t: one clip whose frames pass 2^32 bytes.  n = 65535 full-frame records of 128 x 176 on 7
patterns, tiled on the device with tests/far_batch.py's helpers (the table there gains no row); the colour table and every frame's data
sit behind a lead of more than 2^32 bytes, so every offset of the frame table is past 2^32.  The memory it needs is asserted first: the
test fails, it does not skip, when the device is short.  Run with ``-m gpu``."""
import numpy as np
import pytest
import torch

import far_batch as F
import gif_decode_cases as C
import gif_decode_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
H, W, K = 128, 176, 16
STRIDE = 8192                    # bytes of data per frame: every pattern's stream, padded


def test_a_clip_whose_frames_pass_4_gib():
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    import applied_image_processing_amd.runtime as rt

    torch.cuda.set_device(0)
    lib = rt.gif_decode_lib()
    n, lead = F.N, F.LEAD
    rng = np.random.default_rng(11)
    # blocks of 8 x 8 pixels of one colour: streams of a few KiB with long strings
    index = np.stack([np.kron(rng.integers(0, K, (H // 8, W // 8)), np.ones((8, 8), int)) for _ in range(F.P)])
    table = C.table_of(C._colours(K))
    streams = [C.greedy(index[k], 4).data() for k in range(F.P)]
    assert max(len(s) for s in streams) <= STRIDE
    expected = np.stack([np.frombuffer(table, np.uint8).reshape(-1, 3)[index[k]] for k in range(F.P)])
    assert F.distinct(expected)
    for k in range(F.P):                                  # the patterns are what the restatement decodes
        status, got, _ = R.unlzw(streams[k], 4, H * W)
        assert status == 0 and got == index[k].reshape(-1).tolist()
    out_bytes, ws_bytes = n * H * W * 3, rt.gif_decode_sizes(n, H, W, H * W)
    blob_bytes = lead + len(table) + n * STRIDE
    assert out_bytes > F.TWO32 and lead > F.TWO32 and ws_bytes == n * H * W
    need = out_bytes + ws_bytes + blob_bytes + n * 72 + 2 * F.PIECE
    assert need <= F.CAP
    torch.cuda.empty_cache()
    free, _ = torch.cuda.mem_get_info(DEV)
    assert free >= need, f"needs {need >> 20} MiB of device memory, {free >> 20} MiB are free"
    blob = torch.zeros(blob_bytes, dtype=torch.uint8, device=DEV)
    blob[lead:lead + len(table)] = torch.from_numpy(np.frombuffer(table, np.uint8).copy()).to(DEV)
    data = np.zeros((F.P, STRIDE), np.uint8)
    for k, s in enumerate(streams):
        data[k, :len(s)] = np.frombuffer(s, np.uint8)
    blob[lead + len(table):].view(n, STRIDE).copy_(F.tile(data, n, DEV))
    i = torch.arange(n, dtype=torch.int64, device=DEV)
    rows = torch.zeros((n, 8), dtype=torch.int64, device=DEV)
    rows[:, 0] = lead + len(table) + i * STRIDE
    rows[:, 1] = torch.from_numpy(np.array([len(s) for s in streams])).to(DEV)[i % F.P]
    rows[:, 2] = W << 32 | H << 48
    rows[:, 3] = 4 | 1 << 16          # code size 4, disposal 1, opaque
    rows[:, 4] = lead
    rows[:, 5] = len(table) // 3
    out = F.poisoned((n, H, W, 3), torch.uint8, DEV)
    record = F.poisoned((n, 2), torch.int32, DEV)
    ws = F.poisoned((ws_bytes,), torch.uint8, DEV)
    rc = lib.adain_gif_decode_u8(blob.data_ptr(), blob_bytes, rows.data_ptr(), n, H, W, out.data_ptr(), record.data_ptr(), ws.data_ptr(), ws_bytes,
                                 torch.cuda.current_stream().cuda_stream)
    assert rc == 0, lib.adain_gif_decode_last_error().decode()
    torch.cuda.synchronize()
    assert int((record[:, 0] != 0).sum()) == 0
    F.assert_frames("gif_decode_u8", out, expected)
    del out, ws, blob
    F.release()
