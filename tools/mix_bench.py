"""Times the style-interpolation blend (csrc/stats.hip, ``adain_blend_mix``) at the relu4_1 shapes of a 256 x 456 frame (32 x 57), a
1080 x 1920 frame (135 x 240) and a batch of 8 such frames, NHWC with 512 channels, on seeded synthetic features:
  (a) blend_alpha          ``adain_blend_alpha``, one style: the single-style blend the mix has to keep up with
  (b) mix_scalar_K         ``adain_blend_mix`` at K = 1, 2, 4, 16 with one scalar weight per style
  (c) mix_maps_K           the same K with a weight map per style at feature resolution
  (d) emulation_K          what a caller could do before the kernel existed: K ``blend_alpha(alpha=1)`` calls combined with torch
                           ``mul`` / ``add`` and a last blend in torch (each pass reads and writes the feature map again)
Expected from the bytes moved, not measured: (b) moves the 8 bytes per element of (a) whatever K is ((c) adds 4 K bytes per PIXEL,
1/512 of that per element), (d) about (3 K + 2) / 2 times as many.
HIP events around each call, medians and interquartile ranges of --reps calls after 20 warm-up calls; shader clock and power over each
shape's window; each row also carries the sha256 of its last call's output bytes, so that two builds of the library (--lib PATH: that
build in place of the package's own) can be held to the same bytes as well as the same time.  Prints one JSON line and, with --out,
writes it to a file.
The timing loops, the statistic and the verdict's rule are tools/benchkit.py's.
Usage: python tools/mix_bench.py [--reps 200] [--lib PATH] [--out profiles/mix_bench.json]"""
import hashlib
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))

import applied_image_processing_amd.runtime as rt  # noqa: E402
from applied_image_processing_amd.telemetry import GpuTelemetry  # noqa: E402
from benchkit import arguments, emit, event_times  # noqa: E402

SHAPES = [("256x456", 1, 32, 57), ("1080x1920", 1, 135, 240), ("8x1080x1920", 8, 135, 240)]
KS = [1, 2, 4, 16]
C = 512


def summary(times, out):
    """This record's own shape: the quartiles themselves, and the sha256 of the last call's output."""
    q = statistics.quantiles(times, n=4)
    return {"median_ms": round(statistics.median(times), 4), "iqr_ms": [round(q[0], 4), round(q[2], 4)],
            "sha256": hashlib.sha256(out.cpu().numpy().tobytes()).hexdigest()}


def form_ms(fn, reps, warmup=20):
    return summary(*event_times(fn, reps, warmup))


def emulation(x, cm, cs, sm, ss, w, alpha):
    feat = None
    for k in range(sm.shape[0]):
        t = rt.blend_alpha(x, True, cm, cs, sm[k:k + 1], ss[k:k + 1], 1.0).mul_(w[k])
        feat = t if feat is None else feat.add_(t)
    return feat.mul_(alpha).add_(x, alpha=1 - alpha)


def iqr(s):
    return s["iqr_ms"][1] - s["iqr_ms"][0]


def main():
    args = arguments(__doc__, lib=True).parse_args()
    if args.lib:
        rt.use_library(os.path.abspath(args.lib))
    assert torch.cuda.is_available(), "mix_bench needs a GPU"
    torch.cuda.set_device(0)          # its own setup and header: the record has no CPU counts, and the host's threads are left as they are
    reps = max(args.reps, 8)
    g = torch.Generator().manual_seed(0)
    rand = lambda *s: torch.rand(*s, generator=g).cuda()
    tel = GpuTelemetry(0).start()
    res = {"device": torch.cuda.get_device_name(0), "reps": reps, "lib": os.path.relpath(rt.LIB_PATH), "channels": C, "shapes": {}}
    for name, n, hc, wc in SHAPES:
        x = (rand(n, hc, wc, C) * 4 - 2).contiguous()
        cm, cs = rand(n, C), rand(n, C) + 0.5
        sm, ss = rand(max(KS), C), rand(max(KS), C) + 0.5
        t0 = time.perf_counter()
        row = {"elements": x.numel(), "blend_alpha": form_ms(lambda: rt.blend_alpha(x, True, cm, cs, sm[:1], ss[:1], 0.6), reps)}
        for k in KS:
            w = (rand(k) / k).contiguous()
            maps = (rand(n, k, hc, wc) / k).contiguous()
            smk, ssk = sm[:k].contiguous(), ss[:k].contiguous()
            row[f"mix_scalar_{k}"] = form_ms(lambda: rt.blend_mix(x, True, cm, cs, smk, ssk, w, alpha=0.6), reps)
            row[f"mix_maps_{k}"] = form_ms(lambda: rt.blend_mix(x, True, cm, cs, smk, ssk, maps, alpha=0.6), reps)
            wl = [float(v) for v in w.cpu()]
            row[f"emulation_{k}"] = form_ms(lambda: emulation(x, cm, cs, smk, ssk, wl, 0.6), reps)
        tel.window(name, t0, time.perf_counter())
        a, b4 = row["blend_alpha"], row["mix_scalar_4"]
        row["mix_scalar_4_within_both_iqrs_of_blend_alpha"] = bool(abs(b4["median_ms"] - a["median_ms"]) <= iqr(a) + iqr(b4))
        for k in KS:
            b, d = row[f"mix_scalar_{k}"], row[f"emulation_{k}"]
            row[f"mix_scalar_{k}_below_emulation_by_more_than_both_iqrs"] = bool(d["median_ms"] - b["median_ms"] > iqr(b) + iqr(d))
            row[f"mix_scalar_{k}_gb_per_s"] = round(8 * x.numel() / (b["median_ms"] * 1e-3) / 1e9, 1)
        row["blend_alpha_gb_per_s"] = round(8 * x.numel() / (a["median_ms"] * 1e-3) / 1e9, 1)
        res["shapes"][name] = row
    res["telemetry"] = tel.stop()
    emit(res, args.out)


if __name__ == "__main__":
    main()
