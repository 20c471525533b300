"""What the device tests of the GIF decoder share: a parsed clip as the raw call's arguments inside a guard-band arena (tests/abi_arena.py)
- the frame table, the blob at a chosen byte address, out, record and a workspace of exactly the queried size - and the restatement's
answer for every designed file, computed once."""
import functools

import numpy as np
import torch

import abi_arena as A
import gif_decode_cases as C
import gif_decode_ref as R


@functools.lru_cache(maxsize=None)
def expected(name):
    """(statuses, frames) of tests/gif_decode_ref.py for a file of CASES, DAMAGED or the Pillow-made clips: computed once, never changed."""
    statuses, frames = R.decode(data_of(name))
    frames.setflags(write=False)
    return tuple(statuses), frames


@functools.lru_cache(maxsize=None)
def _pillow():
    return C.pillow_clips()


def data_of(name):
    return C.CASES[name] if name in C.CASES else C.DAMAGED[name][0] if name in C.DAMAGED else _pillow()[name]


class Plan:
    """The call on one clip.  ``shift``: the blob starts ``shift`` bytes behind a 4-byte aligned address that is no multiple of 8."""

    def __init__(self, rt, data, shift=0, slack=0):
        from applied_image_processing_amd import gif_file

        self.rt, self.clip, self.shift = rt, gif_file.parse(data), shift
        rows, blob = rt.gif_decode_table(self.clip)
        self.n, self.H, self.W = len(rows), self.clip.h, self.clip.w
        self.rows, self.blob = np.asarray(rows, dtype=np.uint64), blob
        self.ws_bytes = rt.gif_decode_sizes(self.n, self.H, self.W, max(f.w * f.h for f in self.clip.frames)) + slack
        self.specs = [("table", self.n * 64, "in", 8), ("blob", shift + len(blob), "in", 4, [(0, shift)]), ("out", self.n * self.H * self.W * 3, "out", 1),
                      ("record", self.n * 8, "out", 4), ("ws", self.ws_bytes, "ws", 1)]

    def setup(self, arena):
        arena.put("table", torch.from_numpy(self.rows.view(np.uint8).copy()))
        arena.put("blob", torch.from_numpy(np.frombuffer(bytes(self.shift) + self.blob, np.uint8).copy()))

    def call(self, arena):
        """The raw C call on the current stream -> its return value."""
        lib = self.rt.gif_decode_lib()
        return lib.adain_gif_decode_u8(arena.ptr("blob") + self.shift, len(self.blob), arena.ptr("table"), self.n, self.H, self.W, arena.ptr("out"), arena.ptr("record"),
                                       arena.ptr("ws"), self.ws_bytes, torch.cuda.current_stream().cuda_stream)

    def checked_call(self, arena):
        rc = self.call(arena)
        assert rc == 0, self.rt.gif_decode_lib().adain_gif_decode_last_error().decode()

    def results(self, outs):
        """(statuses, frames [n,H,W,3]) of an arena's outputs."""
        record = outs["record"].cpu().view(torch.int32).reshape(self.n, 2)
        return tuple(record[:, 0].tolist()), outs["out"].cpu().numpy().reshape(self.n, self.H, self.W, 3)
