"""Times the device Farneback estimator with HIP events (flow.py / csrc/flow.hip): one pair pair-by-pair (two expansions + the
flow) and the flow alone at 256^2 and 1080p, and FlowSequence over a 1080p clip (one expansion + one flow per frame).  Prints one
JSON line.
The timing loops, the statistic and the verdict's rule are tools/benchkit.py's.
Usage: python tools/flow_bench.py [--frames 32] [--reps 20]"""
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "tests"))
import farneback_ref as F  # noqa: E402
from benchkit import arguments, emit, event_mean_ms  # noqa: E402

from applied_image_processing_amd import flow  # noqa: E402


def main():
    ap = arguments(__doc__)
    ap.add_argument("--frames", type=int, default=32)
    ap.set_defaults(reps=20)
    args = ap.parse_args()
    torch.cuda.set_device(0)
    res = {}
    for h, w in [(256, 256), (1080, 1920)]:
        a, b = torch.from_numpy(F.texture(h, w, seed=1)).cuda(), torch.from_numpy(F.texture(h, w, (2.5, -1.5), seed=1)).cuda()
        fb = flow.Farneback(h, w)
        pa, pb = fb.expand(a), fb.expand(b)
        out = torch.empty(2, h, w, device="cuda")
        res[f"{w}x{h}"] = {
            "pair_ms": round(event_mean_ms(lambda: flow.calc_optical_flow_farneback(a, b), args.reps), 4),
            "expand_ms": round(event_mean_ms(lambda: fb.expand(a, out=pa), args.reps), 4),
            "flow_ms": round(event_mean_ms(lambda: fb.flow(pa, pb, out=out), args.reps), 4),
        }
    clip = [torch.from_numpy(F.texture(1080, 1920, (0.8 * i, 0.3 * i), seed=2)).cuda() for i in range(args.frames)]
    out = torch.empty(args.frames - 1, 2, 1080, 1920, device="cuda")
    seq = flow.FlowSequence()
    ms = event_mean_ms(lambda: seq.batch(clip, out=out), 3)
    res["sequence_1080p"] = {"frames": args.frames, "ms": round(ms, 3), "fps": round(args.frames * 1000.0 / ms, 1)}
    emit(res, args.out)


if __name__ == "__main__":
    main()
