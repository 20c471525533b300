"""Times the device palette chooser (csrc/quantize.hip) against Pillow's quantisers on the same machine.  Medians and interquartile ranges
over --reps calls (>= 200) after warm-up; Pillow's over --pillow_reps (the number used is recorded), on one thread.
  frames : one 1080 x 1920 frame - a stylised synthetic frame (seed-0 weights), uniform noise, flat white - at K = 16 and 256
  clips  : 64 stylised frames of 135 x 240, one palette for the clip and one per frame, at K = 16 and 256
  call_ms      adain_quantize_palette_u8 on device-resident frames, HIP events around the call
  stage_ms     the three kernels of that call (hist, sat, cut) from the profiler's kernel records of the same calls - the C call has no
               seam to put an event in; null where the profiler gives no kernel records
  cut_step_us  the cut kernel's median over the used - 1 steps it ran
  mediancut_ms / fastoctree_ms   Image.quantize(K, method, dither=NONE) of the same frame(s), one after another
  gif    : gif_file.write_gif(frames, path, "adaptive-local") from the device clip to the file (a temporary file, read back) against
           Pillow's save(save_all=True) of the same RGB frames to BytesIO - what the reference's create_gif does - with both files' sizes
``faster`` / ``slower``: one median sits below the other by more than both interquartile ranges.  Prints one JSON line; --out writes it.
The timing loops, the statistic and the verdict's rule are tools/benchkit.py's.
Usage: python tools/quantize_bench.py [--reps 200] [--pillow_reps 20] [--out profiles/quantize_bench.json]"""
import io
import json
import os
import sys
import tempfile

import numpy as np
import PIL
import torch
from PIL import Image

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))

import applied_image_processing_amd.runtime as rt  # noqa: E402
import applied_image_processing_amd.synth as synth  # noqa: E402
from applied_image_processing_amd import gif_file  # noqa: E402
from applied_image_processing_amd.engine import AdaINEngine  # noqa: E402
from benchkit import arguments, below, emit, event_ms, gpu_setup, header, spread, wall_ms  # noqa: E402

KS = (16, 256)
STAGES = {"hist": "quantize_hist_kernel", "sat": "quantize_sat_kernel", "cut": "quantize_cut_kernel"}


def stage_ms(fn, reps, stages=STAGES):
    """{stage: spread} from the profiler's kernel records of ``reps`` calls, or None.  ``stages``: {stage: its kernel's name}; a stage's
    figure is per launch."""
    try:
        from torch.profiler import ProfilerActivity, profile

        torch.cuda.synchronize()
        with profile(activities=[ProfilerActivity.CUDA]) as prof:
            for _ in range(reps):
                fn()
            torch.cuda.synchronize()
        times = {k: [] for k in stages}
        for e in prof.events():
            for k, kernel in stages.items():
                if kernel in e.name:
                    times[k].append(getattr(e, "device_time", None) or getattr(e, "cuda_time", 0.0))
        if any(len(v) < reps for v in times.values()):
            return None
        return {k: {s: round(x / 1e3, 4) for s, x in spread(v).items()} for k, v in times.items()}
    except Exception as e:          # the figures are optional: the whole call's are not
        print(f"no stage figures: {e!r}", file=sys.stderr)
        return None


def pillow_ms(frames, K, method, reps):
    images = [Image.fromarray(f) for f in frames]
    return wall_ms(lambda: [im.quantize(K, method=method, dither=Image.Dither.NONE) for im in images], reps, 1, "none")


def chooser(x, host, per_frame, reps, pillow_reps):
    out = {}
    for K in KS:
        call = lambda: rt.quantize_palette_u8(x, K, per_frame)
        used = call()[1].cpu().tolist()
        r = {"used": used if len(used) < 4 else [min(used), max(used)], "call_ms": event_ms(call, reps, 20), "stage_ms": stage_ms(call, reps),
             "mediancut_ms": pillow_ms(host, K, Image.Quantize.MEDIANCUT, pillow_reps), "fastoctree_ms": pillow_ms(host, K, Image.Quantize.FASTOCTREE, pillow_reps)}
        if r["stage_ms"] and not per_frame and used[0] > 1:
            r["cut_step_us"] = round(1e3 * r["stage_ms"]["cut"]["median"] / (used[0] - 1), 3)
        for name in ("mediancut", "fastoctree"):
            r[f"faster_than_{name}"], r[f"slower_than_{name}"] = below(r["call_ms"], r[name + "_ms"]), below(r[name + "_ms"], r["call_ms"])
        out[f"K{K}"] = r
    return out


def gif(x, host, reps, pillow_reps):
    with tempfile.TemporaryDirectory() as tmp:
        path = os.path.join(tmp, "clip.gif")

        def ours():
            gif_file.write_gif(x, path, "adaptive-local", fps=20)
            with open(path, "rb") as f:
                return f.read()

        def pillows():
            images = [Image.fromarray(f) for f in host]
            f = io.BytesIO()
            images[0].save(f, format="GIF", save_all=True, append_images=images[1:], duration=50, loop=0)
            return f.getvalue()

        a, b = wall_ms(ours, reps, 3, "before"), wall_ms(pillows, pillow_reps, 1, "none")
        data = ours()
        im = Image.open(io.BytesIO(data))
        return {"frames": len(host), "device_ms": a, "pillow_ms": b, "file_bytes": len(data), "pillow_file_bytes": len(pillows()), "frames_in_file": im.n_frames,
                "faster_than_pillow": below(a, b), "slower_than_pillow": below(b, a)}


def inputs(dev):
    """({kind: one 1080 x 1920 frame uint8 [1,h,w,3] on ``dev``}, the 64-frame 135 x 240 clip): what this tool and
    tools/quantize_refine_timing.py time."""
    engine = AdaINEngine(synth.to_torch(synth.vgg_state_dict(0, full=False)), synth.to_torch(synth.decoder_state_dict(0)), dev)
    engine.set_style(torch.from_numpy(synth.image(4, 1, 512, 512)).to(dev))

    def stylised(n, h, w):
        parts = []
        for i in range(0, n, 16):
            k = min(16, n - i)
            source = torch.from_numpy((synth.image(7 + i, k, h, w).transpose(0, 2, 3, 1) * np.float32(255)).astype(np.uint8)).to(dev)
            parts.append(engine.stylize_u8(source, alpha=0.5).contiguous())
        return torch.cat(parts).contiguous()

    h, w = 1080, 1920
    sources = {"stylised": stylised(1, h, w), "noise": torch.from_numpy(np.random.default_rng(5).integers(0, 256, (1, h, w, 3), dtype=np.uint8)).to(dev),
               "flat": torch.full((1, h, w, 3), 255, dtype=torch.uint8, device=dev)}
    return sources, stylised(64, 135, 240)


def main():
    ap = arguments(__doc__)
    ap.add_argument("--pillow_reps", type=int, default=20)
    args = ap.parse_args()
    dev = gpu_setup("quantize_bench")
    reps, pillow_reps = max(args.reps, 200), max(4, args.pillow_reps)
    sources, clip = inputs(dev)
    res = header(reps=reps, pillow_reps=pillow_reps, pillow=PIL.__version__, frames={}, clips={})
    for kind, x in sources.items():
        res["frames"][kind] = chooser(x, x.cpu().numpy(), False, reps, pillow_reps)
        print(kind, json.dumps(res["frames"][kind]), file=sys.stderr, flush=True)
    hist = lambda kind: (res["frames"][kind]["K256"]["stage_ms"] or {}).get("hist")
    if hist("flat") and hist("noise"):
        res["hist_flat_over_noise"] = round(hist("flat")["median"] / hist("noise")["median"], 3)
    host = clip.cpu().numpy()
    for mode, per_frame in (("global", False), ("per_frame", True)):
        res["clips"][mode] = chooser(clip, host, per_frame, reps, pillow_reps)
        print(mode, json.dumps(res["clips"][mode]), file=sys.stderr, flush=True)
    res["gif_adaptive_local"] = gif(clip, host, reps, pillow_reps)
    emit(res, args.out)


if __name__ == "__main__":
    main()
