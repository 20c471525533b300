"""Times the colour-preserving path's CORAL transform (csrc/coral.hip) at the two operating points of the per-call callers, a 256 x 456
frame and a 1080 x 1920 frame, each with a 512 x 512 style, on seeded synthetic images:
  kernel_ms   runtime.coral on device-resident uint8 inputs (moments, matrix, apply: 4 launches), HIP events
  host_ms     the host ``coral`` of AdaIN/function.py (float32 torch on ONE thread) on the same machine and pixels
  call_off_ms one adain_inference(preserve_color=True) call with set_device_coral(False): the call-by-call path, host clock
  call_on_ms  the same call with set_device_coral(True): the cached one-call path with CORAL on the device, host clock
Medians and interquartile ranges of --reps calls after warm-up (20 calls of the kernel, so that the clock has ramped; 3 of the others);
shader clock and power over each kernel window.  Seeded synthetic weights, JPEG output (PIL) to a temporary directory.  Prints one JSON line and,
with --out, writes it to a file.
The timing loops, the statistic and the verdict's rule are tools/benchkit.py's.
Usage: python tools/coral_bench.py [--reps 200] [--out profiles/coral_bench.json]"""
import contextlib
import io
import os
import statistics
import sys
import tempfile
import time

import numpy as np
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))

import applied_image_processing_amd.runtime as rt  # noqa: E402
import applied_image_processing_amd.synth as synth  # noqa: E402
from applied_image_processing_amd.AdaIN import test as adain  # noqa: E402
from applied_image_processing_amd.AdaIN.function import coral as host_coral  # noqa: E402
from applied_image_processing_amd.telemetry import GpuTelemetry  # noqa: E402
from benchkit import arguments, emit, event_times, wall_times  # noqa: E402

SIZES = [(256, 456), (1080, 1920)]
STYLE = (512, 512)


def u8(seed, h, w):
    return np.ascontiguousarray((synth.image(seed, 1, h, w)[0].transpose(1, 2, 0) * np.float32(255)).astype(np.uint8))


def summary(times):
    """This record's own shape: the quartiles themselves, not their distance."""
    q = statistics.quantiles(times, n=4)
    return {"median_ms": round(statistics.median(times), 4), "iqr_ms": [round(q[0], 4), round(q[2], 4)]}


def main():
    from PIL import Image

    args = arguments(__doc__).parse_args()
    assert torch.cuda.is_available(), "coral_bench needs a GPU"
    torch.cuda.set_device(0)          # its own setup and header: the calls run on the host's threads as they are, and the record names no library
    reps = max(args.reps, 8)
    tel = GpuTelemetry(0).start()
    res = {"device": torch.cuda.get_device_name(0), "cpus_usable": len(os.sched_getaffinity(0)), "cpus_machine": os.cpu_count(),
           "reps": reps, "style": f"{STYLE[0]}x{STYLE[1]}", "sizes": {}}
    style = u8(7, *STYLE)
    d_style = torch.from_numpy(style)[None].cuda()
    s_host = torch.from_numpy(style).permute(2, 0, 1).float().div(255)
    with tempfile.TemporaryDirectory() as tmp:
        torch.save(synth.to_torch(synth.vgg_state_dict(0, full=True)), os.path.join(tmp, "vgg.pth"))
        torch.save(synth.to_torch(synth.decoder_state_dict(0)), os.path.join(tmp, "dec.pth"))
        pil_style = Image.fromarray(style)
        for h, w in SIZES:
            frame = u8(100 + h, h, w)
            d_frame = torch.from_numpy(frame)[None].cuda()
            out = torch.empty((1, 3) + STYLE, dtype=torch.float32, device="cuda")
            t0 = time.perf_counter()
            kernel = summary(event_times(lambda: rt.coral(d_style, d_frame, out=out), reps, 20)[0])
            tel.window(f"kernel_{h}x{w}", t0, time.perf_counter())
            c_host = torch.from_numpy(frame).permute(2, 0, 1).float().div(255)
            threads = torch.get_num_threads()
            torch.set_num_threads(1)
            host = summary(wall_times(lambda: host_coral(s_host, c_host), reps, 3, "both")[0])
            torch.set_num_threads(threads)
            want = host_coral(s_host, c_host)
            err = float((out[0].cpu() - want).norm() / want.norm())
            pil_frame = Image.fromarray(frame)
            kw = dict(vgg_str=os.path.join(tmp, "vgg.pth"), decoder_str=os.path.join(tmp, "dec.pth"), content_size=h, style_size=STYLE[0],
                      output=tmp, file_name="bench", save_ext=".jpg", preserve_color=True)
            calls = {}
            for name, flag in (("call_off_ms", False), ("call_on_ms", True)):
                prev = adain.set_device_coral(flag)
                with contextlib.redirect_stdout(io.StringIO()):          # adain_inference prints the path it saved
                    calls[name] = summary(wall_times(lambda: adain.adain_inference(pil_frame, pil_style, **kw), reps, 3, "both")[0])
                adain.set_device_coral(prev)
            gap = calls["call_off_ms"]["median_ms"] - calls["call_on_ms"]["median_ms"]
            spread = max(b - a for a, b in (calls["call_off_ms"]["iqr_ms"], calls["call_on_ms"]["iqr_ms"]))
            res["sizes"][f"{h}x{w}"] = {"kernel_ms": kernel, "host_ms": host, "host_over_kernel": round(host["median_ms"] / kernel["median_ms"], 1),
                                        "relative_l2_against_host": float(f"{err:.3e}"), **calls,
                                        "device_call_below_host_call_by_more_than_both_iqrs": bool(gap > spread)}
    res["telemetry"] = tel.stop()          # shader clock and power over each size's kernel timing (sysfs reads)
    emit(res, args.out)


if __name__ == "__main__":
    main()
