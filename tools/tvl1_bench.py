"""Times the device Dual TV-L1 estimator with HIP events (tvl1.py / csrc/tvl1.hip), create()'s defaults: one pair at 256^2 and at
1080p (preparation of both frames + the flow), a 256^2 clip through TVL1Sequence.batch (pairs/s), the inner steps each (scale, warp)
executed for those inputs, the time per executed step, and the cost of the host's stop reads (two runs with the same launches,
with and without the reads).  Prints one JSON line; the GPU's clock and power are read with amd-smi
when it is there.  No cv2 baseline exists on any machine of this project.
The timing loops, the statistic and the verdict's rule are tools/benchkit.py's.
Usage: python tools/tvl1_bench.py [--frames 64] [--reps 3]"""
import json
import os
import subprocess
import sys

import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "tests"))
import farneback_ref as F  # noqa: E402
from benchkit import arguments, emit, event_mean_ms  # noqa: E402

from applied_image_processing_amd import tvl1  # noqa: E402


def clock_power():
    try:
        out = subprocess.run(["amd-smi", "metric", "-g", "0", "-c", "-p", "--json"], capture_output=True, text=True, timeout=20).stdout
        return json.loads(out) if out.strip().startswith(("[", "{")) else None
    except Exception:
        return None


def main():
    ap = arguments(__doc__)
    ap.add_argument("--frames", type=int, default=64)
    ap.set_defaults(reps=3)
    args = ap.parse_args()
    torch.cuda.set_device(0)
    res = {}
    for h, w in [(256, 256), (1080, 1920)]:
        a = torch.from_numpy(F.texture(h, w, seed=1)).cuda()
        b = torch.from_numpy(F.texture(h, w, (2.5, -1.5), seed=1)).cuda()
        t = tvl1.TVL1(h, w)
        pa, pb = t.prepare(a), t.prepare(b)
        it = torch.zeros((1, len(t.scales), t.P.warps), dtype=torch.int32, device="cuda")
        out = torch.empty(1, 2, h, w, device="cuda")
        calc = tvl1.DualTVL1OpticalFlow_create().calc
        pair_ms = event_mean_ms(lambda: calc(a, b), args.reps)
        flow_ms = event_mean_ms(lambda: t.flows([pa], [pb], out=out, iters_out=it), args.reps)
        steps = int(it.sum().item())
        res[f"{w}x{h}"] = {"pair_ms": round(pair_ms, 3), "flow_ms": round(flow_ms, 3), "inner_steps": steps,
                           "us_per_step": round(1000 * flow_ms / max(steps, 1), 2), "iters": it[0].cpu().tolist()}
    n = args.frames
    clip = [torch.from_numpy(F.texture(256, 256, (0.8 * i, 0.3 * i), seed=2)).cuda() for i in range(n)]
    out = torch.empty(n - 1, 2, 256, 256, device="cuda")
    seq = tvl1.TVL1Sequence()
    ms = event_mean_ms(lambda: seq.batch(clip, out=out), 1)
    t = tvl1.TVL1(256, 256)
    m = min(t.default_max_pairs(), n - 1)
    prep = t.prepare(torch.stack(clip[:m + 1]))
    it = torch.zeros((m, len(t.scales), t.P.warps), dtype=torch.int32, device="cuda")
    t.flows([prep[j] for j in range(m)], [prep[j + 1] for j in range(m)], out=out[:m], iters_out=it)
    per_pair = it.sum(dim=(1, 2)).cpu()
    res["clip_256"] = {"frames": n, "max_pairs": m, "ms": round(ms, 2), "pairs_per_s": round((n - 1) * 1000.0 / ms, 1),
                       "inner_steps_per_pair_mean": round(float(per_pair.float().mean()), 1),
                       "inner_steps_per_pair_max": int(per_pair.max()), "iters_max_per_scale_warp": it.max(dim=0).values.cpu().tolist()}
    # the host's stop reads: two runs with the same launches (epsilon 0: no pair ever stops, no median), 30 inner steps per warp
    # as 10 outer passes of 3 (9 reads per warp) or 1 outer pass of 30 (no read); the difference over the reads is their cost
    reads = {}
    for npairs in (1, 63):
        ts = {}
        for outer, inner in ((10, 3), (1, 30)):
            tr = tvl1.TVL1(256, 256, epsilon=0.0, medianFiltering=1, outerIterations=outer, innerIterations=inner)
            pr = tr.prepare(torch.stack(clip[:npairs + 1]))
            o = torch.empty(npairs, 2, 256, 256, device="cuda")
            ts[outer] = event_mean_ms(lambda: tr.flows([pr[j] for j in range(npairs)], [pr[j + 1] for j in range(npairs)], out=o), args.reps)
        nreads = len(tr.scales) * tr.P.warps * 9
        reads[f"pairs_{npairs}"] = {"ms_with_reads": round(ts[10], 3), "ms_without": round(ts[1], 3), "reads": nreads,
                                    "us_per_read": round(1000 * (ts[10] - ts[1]) / nreads, 2)}
    res["stop_reads_256"] = reads
    res["gpu"] = clock_power()
    emit(res, args.out)


if __name__ == "__main__":
    main()
