"""Times the palette's k-means refinement (csrc/quantize_refine.hip) on the inputs of tools/quantize_bench.py: what a round costs on top of
the median cut, and Pillow's own refinement beside it.  Medians and interquartile ranges over --reps calls (>= 200) after warm-up.
  frames : one 1080 x 1920 frame - a stylised synthetic frame (seed-0 weights), uniform noise, flat white
  clips  : 64 stylised frames of 135 x 240, one palette for the clip and one per frame
each at K = 16 and 256 and T = 1 and 8 rounds.  Per cell:
  call_ms       adain_quantize_palette_u8 with ADAIN_QUANTIZE_REFINE(T) on device-resident frames, HIP events around the call
  cut_ms        the same call at T = 0: the median cut alone, what the call cost before there were rounds
  round_ms      (call_ms - cut_ms) / T of the medians
  stage_ms      the two kernels of a round (assign, update), per launch, from the profiler's kernel records of a run of their own;
                null where the profiler gives no kernel records
  used          the palette's entries after the rounds (and used_cut: after the cut alone)
  pillow_ms     Image.quantize(K, MEDIANCUT, kmeans=T, dither=NONE) of the same frame(s) on one host thread, over up to --pillow_reps
                calls (``calls`` records how many): neither the code under test nor a yardstick for its result - Pillow's palette is
                another one - and slow: a refined 1080p noise frame takes Pillow about a minute.  --pillow_budget_s bounds the seconds all
                of Pillow's calls may take together; the clips go first, and a cell the budget does not reach says "not recorded yet"
``faster`` / ``slower``: one median sits below the other by more than both interquartile ranges (benchkit's rule); null where Pillow was
called once.  The record is rewritten after every cell.  The timing loops, the statistic and the verdict's rule are tools/benchkit.py's.
(This tool's name does not end in _bench.py: tests/test_benchkit_host.py counts those.)
Usage: python tools/quantize_refine_timing.py [--reps 200] [--pillow_reps 20] [--pillow_budget_s 600] [--out profiles/quantize_refine_bench.json]"""
import json
import os
import sys
import time

import PIL
from PIL import Image

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))

import applied_image_processing_amd.runtime as rt  # noqa: E402
from benchkit import arguments, below, event_ms, gpu_setup, header, spread, write  # noqa: E402

KS = (16, 256)
TS = (1, 8)
STAGES = {"assign": "quantize_assign_kernel", "update": "quantize_update_kernel"}
NOT_RECORDED = "not recorded yet"


class PillowBudget:
    def __init__(self, seconds):
        self.left = float(seconds)

    def time(self, frames, K, T, reps):
        """{median, iqr, calls} in ms of Pillow's refined median cut over the frames, one after another; NOT_RECORDED once the budget is spent."""
        if self.left <= 0:
            return NOT_RECORDED
        images = [Image.fromarray(f) for f in frames]
        times = []
        while len(times) < reps and self.left > 0:
            t = time.perf_counter()
            for im in images:
                im.quantize(K, method=Image.Quantize.MEDIANCUT, kmeans=T, dither=Image.Dither.NONE)
            times.append((time.perf_counter() - t) * 1e3)
            self.left -= times[-1] / 1e3
        return dict(spread(times), calls=len(times))


def verdicts(r):
    """``below`` both ways for a cell's call_ms against cut_ms and pillow_ms."""
    r["slower_than_cut"] = below(r["cut_ms"], r["call_ms"])
    p = r["pillow_ms"]
    known = isinstance(p, dict) and p["iqr"] is not None
    r["faster_than_pillow"] = below(r["call_ms"], p) if known else None
    r["slower_than_pillow"] = below(p, r["call_ms"]) if known else None


def device_cells(x, per_frame, reps, stage_ms):
    out = {}
    for K in KS:
        cut = lambda: rt.quantize_palette_u8(x, K, per_frame)
        used_cut = cut()[1].cpu().tolist()
        cut_ms = event_ms(cut, reps, 20)
        for T in TS:
            call = lambda: rt.quantize_palette_u8(x, K, per_frame, T)
            used = call()[1].cpu().tolist()
            r = {"used": used if len(used) < 4 else [min(used), max(used)], "used_cut": used_cut if len(used_cut) < 4 else [min(used_cut), max(used_cut)],
                 "call_ms": event_ms(call, reps, 20), "cut_ms": cut_ms, "stage_ms": stage_ms(call, max(2, reps // T), STAGES), "pillow_ms": NOT_RECORDED}
            r["round_ms"] = round((r["call_ms"]["median"] - cut_ms["median"]) / T, 4)
            verdicts(r)
            out[f"K{K}_T{T}"] = r
    return out


def main():
    ap = arguments(__doc__)
    ap.add_argument("--pillow_reps", type=int, default=20)
    ap.add_argument("--pillow_budget_s", type=float, default=600)
    args = ap.parse_args()
    dev = gpu_setup("quantize_refine_timing")
    from quantize_bench import inputs, stage_ms

    reps = max(args.reps, 200)
    sources, clip = inputs(dev)
    res = header(reps=reps, pillow_reps=args.pillow_reps, pillow_budget_s=args.pillow_budget_s, pillow=PIL.__version__, frames={}, clips={})
    rows = [("clips", "global", clip, False), ("clips", "per_frame", clip, True)] + [("frames", kind, x, False) for kind, x in sources.items()]
    for group, name, x, per_frame in rows:
        res[group][name] = device_cells(x, per_frame, reps, stage_ms)
        print(name, json.dumps(res[group][name]), file=sys.stderr, flush=True)
        write(json.dumps(res), args.out)
    flat, noise = (res["frames"][k]["K256_T8"]["stage_ms"] for k in ("flat", "noise"))
    if flat and noise:
        res["assign_flat_over_noise_K256"] = round(flat["assign"]["median"] / noise["assign"]["median"], 3)
    budget = PillowBudget(args.pillow_budget_s)
    for group, name, x, per_frame in rows:          # Pillow's side, the small inputs first
        host = x.cpu().numpy()
        for K in KS:
            for T in TS:
                r = res[group][name][f"K{K}_T{T}"]
                r["pillow_ms"] = budget.time(host, K, T, args.pillow_reps)
                verdicts(r)
                write(json.dumps(res), args.out)
    line = json.dumps(res)
    print(line)
    write(line, args.out)


if __name__ == "__main__":
    main()
