"""Times the video path's intermediate JPEG round trip (``intermediate_jpeg=True``) on the device (csrc/jpeg.hip,
adain_jpeg_roundtrip_u8) against the host route through Pillow on the same machine, at 256 x 456 and 1080 x 1920, on a stylised
synthetic frame (seed-0 weights) and on uniform noise.  Per call on a batch of --batch frames, median and interquartile range over
--reps calls (>= 200) after warm-up:
  kernel_ms  adain_jpeg_roundtrip_u8 on device-resident frames, HIP events
  device_ms  wall clock of the ``post`` hook with ``jpeg_on_device=True``: device tensor in, device tensor out, synchronised
  host_ms    the ``post`` hook without it: download, ``video._jpeg_roundtrip`` (Pillow, one thread), upload, synchronised
and whether the two give the same bytes.  ``device_is_faster``: device_ms sits below host_ms by more than the two interquartile ranges
combined.  Every kernel_ms also carries the sha256 of its last call's output bytes, so that two builds of the library
(--lib PATH: that build in place of the package's own) can be held to the same bytes as well as the same time.  Prints one JSON line and, with --out, writes it to a file.
The timing loops, the statistic and the verdict's rule are tools/benchkit.py's.
Usage: python tools/jpeg_roundtrip_bench.py [--reps 200] [--batch 1] [--lib PATH] [--out profiles/jpeg_roundtrip_bench.json]"""
import hashlib
import os
import sys
import time

import numpy as np
import PIL
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))

import applied_image_processing_amd.runtime as rt  # noqa: E402
import applied_image_processing_amd.synth as synth  # noqa: E402
from applied_image_processing_amd import video  # noqa: E402
from applied_image_processing_amd.engine import AdaINEngine  # noqa: E402
from applied_image_processing_amd.telemetry import GpuTelemetry  # noqa: E402
from benchkit import arguments, below, emit, event_times, gpu_setup, header, spread, wall_ms  # noqa: E402

SIZES = [(256, 456), (1080, 1920)]


def sha256(out):
    return hashlib.sha256(out.cpu().numpy().tobytes()).hexdigest()


def hashed_event_ms(fn, reps, warmup):
    """The kit's event_ms with the sha256 of the last call's frames beside it."""
    times, out = event_times(fn, reps, warmup)
    return dict(spread(times), sha256=sha256(out))


def host_post(u8):
    """The ``post`` hook of video._run without ``jpeg_on_device``."""
    return torch.from_numpy(video._jpeg_roundtrip(u8.cpu().numpy())).to(u8.device)


def main():
    ap = arguments(__doc__, lib=True)
    ap.add_argument("--batch", type=int, default=1)
    args = ap.parse_args()
    dev = gpu_setup("jpeg_roundtrip_bench", args.lib)
    reps, n = max(args.reps, 200), max(args.batch, 1)
    engine = AdaINEngine(synth.to_torch(synth.vgg_state_dict(0, full=False)), synth.to_torch(synth.decoder_state_dict(0)), dev)
    engine.set_style(torch.from_numpy(synth.image(4, 1, 512, 512)).to(dev))
    tel = GpuTelemetry(0).start()
    res = header(reps=reps, batch=n, pillow=PIL.__version__, sizes={})
    for h, w in SIZES:
        source = torch.from_numpy((synth.image(7, 1, h, w)[0].transpose(1, 2, 0) * np.float32(255)).astype(np.uint8)[None]).to(dev)
        frames = {"stylised": engine.stylize_u8(source, alpha=0.5).contiguous().expand(n, -1, -1, -1).contiguous(),
                  "noise": torch.from_numpy(np.random.default_rng(0).integers(0, 256, (n, h, w, 3), dtype=np.uint8)).to(dev)}
        for kind, x in frames.items():
            t0 = time.perf_counter()
            kernel = hashed_event_ms(lambda: rt.jpeg_roundtrip_u8(x), reps, 20)
            tel.window(f"kernel_{kind}_{h}x{w}", t0, time.perf_counter())
            device = wall_ms(lambda: engine.jpeg_roundtrip_u8(x), reps, 5, "both")          # both routes end on the device
            host = wall_ms(lambda: host_post(x), reps, 3, "both")
            res["sizes"][f"{kind}_{h}x{w}"] = {"frame_bytes": int(x[0].numel()), "same_bytes_as_host": bool(torch.equal(engine.jpeg_roundtrip_u8(x), host_post(x))),
                                               "kernel_ms": kernel, "device_ms": device, "host_ms": host,
                                               "host_over_device": round(host["median"] / device["median"], 2),
                                               "device_is_faster": below(device, host)}
    res["telemetry"] = tel.stop()          # shader clock and power over each kernel timing window (sysfs reads)
    emit(res, args.out)


if __name__ == "__main__":
    main()
