"""include/adain_gif_decode.h: "the call allocates nothing and waits for nothing, so it may be captured into a hipGraph".  The call is
captured alone on one side stream and replayed the way tests/test_gpu_graph_capture.py does for the rows of tests/capture_cases.py
(tests/abi_arena.run_captured; the table gains no row): on the clip it was captured with, on a second clip of the same shapes put into
the same buffers, and once more on the workspace the second replay left - each time the eager call's bytes, and the restatement's.  Run
with ``-m gpu``."""
import numpy as np
import pytest
import torch

import abi_arena as A
import gif_decode_cases as C
import gif_decode_gpu as G
import gif_decode_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _clip(seed):
    """Two clips of one shape - the same table, rectangles, flags and data lengths are not needed: only the byte counts of the regions
    must agree, so the data are padded to one length."""
    rng = np.random.default_rng(seed)
    pal = C.table_of(C._colours(16))
    frames = []
    for i, (at, hw, gce) in enumerate((((0, 0), (9, 12), (1, None, 3)), ((2, 1), (6, 7), (3, 5, 3)), ((1, 3), (5, 9), (2, None, 3)), ((0, 0), (9, 12), (1, 2, 3)))):
        data = C.greedy(rng.integers(0, 16, hw), 4).data()
        frames.append(C.frame(np.zeros(hw, int), 4, rect=at, gce=gce, data=data + bytes(200 - len(data))))
    return C.gif((12, 9), pal, frames, background=3)


def test_the_call_captured_alone_replays_the_eager_results():
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    import applied_image_processing_amd.runtime as rt

    torch.cuda.set_device(0)
    lib = rt.gif_decode_lib()
    last_error = lambda: lib.adain_gif_decode_last_error().decode()
    plans = {"A": G.Plan(rt, _clip(1)), "B": G.Plan(rt, _clip(2))}
    assert plans["A"].specs == plans["B"].specs
    ea, eb = A.run_captured(plans["A"].specs, plans["A"].call, DEV, torch.cuda.synchronize, {k: p.setup for k, p in plans.items()}, A.hip_graph(last_error),
                            differs=("out",), last_error=last_error)
    assert not torch.cuda.is_current_stream_capturing()
    for plan, e, seed in ((plans["A"], ea, 1), (plans["B"], eb, 2)):
        statuses, want = R.decode(_clip(seed))
        got_status, got = plan.results(e)
        assert list(got_status) == statuses == [0, 0, 0, 0] and np.array_equal(got, want)
