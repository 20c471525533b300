"""Times the localized pipeline's colour transfer + composite (localized.py / csrc/colour.hip) at 250 x 333, 512 x 512 and 1080 x 1920 with
a disc foreground covering about a third of the frame, on seeded synthetic images:
  kernel_ms  adain_localized_combine_u8 on device-resident inputs, HIP events, median
  device_ms  wall time of combine_localized_device from numpy inputs (uploads, the call, the record read, the download), median
  host_ms    wall time of the host combine_localized (numpy, unchanged by the device path) on the same machine and inputs, median
Warm-up calls are excluded (20 of the kernel, so that the clock has ramped); each median is over at least 20 calls.  Prints one JSON
line and, with --out, writes it to a file.
The timing loops, the statistic and the verdict's rule are tools/benchkit.py's.
Usage: python tools/localized_bench.py [--reps 200] [--host_reps 5] [--out profiles/localized_bench.json]"""
import os
import statistics
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))

import applied_image_processing_amd.runtime as rt  # noqa: E402
import applied_image_processing_amd.synth as synth  # noqa: E402
from applied_image_processing_amd import localized as L  # noqa: E402
from applied_image_processing_amd.telemetry import GpuTelemetry  # noqa: E402
from benchkit import arguments, emit, event_times, wall_times  # noqa: E402

SIZES = [(250, 333), (512, 512), (1080, 1920)]


def inputs(h, w, seed):
    content = np.maximum((synth.image(seed, 1, h, w)[0].transpose(1, 2, 0) * np.float32(255)).astype(np.uint8), 1)
    stylised = (synth.image(seed + 1, 1, h, w)[0].transpose(1, 2, 0) * np.float32([200, 120, 90]) + np.float32([30, 60, 20])).astype(np.uint8)
    yy, xx = np.mgrid[:h, :w]
    r2 = h * w / (3 * np.pi)                                       # disc area = a third of the frame (clipped by the frame's edge at 1080p)
    mask = (((yy - h / 2) ** 2 + (xx - w / 2) ** 2) >= r2).astype(np.uint8)
    return np.ascontiguousarray(content), np.ascontiguousarray(stylised), mask


def median(timed):
    """This record's own shape: the bare median of a kit loop's (times, result)."""
    return statistics.median(timed[0])


def main():
    ap = arguments(__doc__)
    ap.add_argument("--host_reps", type=int, default=5)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "localized_bench needs a GPU"
    torch.cuda.set_device(0)          # its own setup and header: the host's threads are left as they are (omp_num_threads is recorded), and the record names no library
    tel = GpuTelemetry(0).start()
    res = {"device": torch.cuda.get_device_name(0), "cpus_usable": len(os.sched_getaffinity(0)), "cpus_machine": os.cpu_count(),
           "omp_num_threads": os.environ.get("OMP_NUM_THREADS"), "reps": args.reps, "host_reps": args.host_reps, "sizes": {}}
    for h, w in SIZES:
        content, stylised, mask = inputs(h, w, 100 + h)
        dc, ds, dm = (torch.from_numpy(a).cuda() for a in (content, stylised, mask))
        out = torch.empty((h, w, 3), dtype=torch.uint8, device=dc.device)
        t0 = time.perf_counter()
        kernel = median(event_times(lambda: rt.localized_combine_u8(dc, ds, dm, out=out), max(args.reps, 20), 20))
        tel.window(f"kernel_{h}x{w}", t0, time.perf_counter())
        device = median(wall_times(lambda: L.combine_localized_device(content, stylised, mask), max(args.reps, 20), 3, "both"))
        host = median(wall_times(lambda: L.combine_localized(content, stylised, mask), args.host_reps, 1, "both"))
        same = int(np.abs(L.combine_localized_device(content, stylised, mask).astype(int) - L.combine_localized(content, stylised, mask).astype(int)).max())
        res["sizes"][f"{h}x{w}"] = {"foreground_pixels": int((mask == 0).sum()), "kernel_ms": round(kernel, 4), "device_ms": round(device, 3),
                                    "host_ms": round(host, 2), "host_over_device": round(host / device, 1), "max_level_difference": same}
    res["telemetry"] = tel.stop()          # shader clock and power over each size's kernel timing (sysfs reads)
    emit(res, args.out)


if __name__ == "__main__":
    main()
