"""Times the device JPEG encoder (csrc/jpeg.hip) against Pillow's on the same machine, at 256 x 456, 1080 x 1920 and 1200 x 1600, on a
stylised synthetic frame (seed-0 weights) and on uniform noise.  Per frame, median and interquartile range over --reps calls (>= 200)
after warm-up:
  kernel_ms  adain_jpeg_encode_u8 on a device-resident frame, HIP events
  device_ms  wall clock from the device uint8 frame to host ``bytes``: the call, the length read, the copy of exactly that many bytes
  pillow_ms  Image.fromarray(frame).save(BytesIO, format="JPEG") of the same frame on this machine's CPU, one thread
and whether the two files are the same bytes.  ``passes_1080p``: device_ms sits below pillow_ms by more than the two interquartile
ranges combined.  ``options``: the same three figures at 1080 x 1920 per option set of OPTION_SETS (quality, subsampling, optimize), under a
key of its own, Pillow given the same keywords; ``faster_than_pillow`` there by the same rule.  ``progressive``: the same three figures for
``JpegOptions(progressive=True)`` at every size and kind, against Pillow's ``save(progressive=True)`` on one thread, and beside them this
encoder's own ``optimize=True`` file of the same frame (``optimize_kernel_ms``, ``optimize_device_ms``); ``faster_than_pillow`` only where the
device median is below Pillow's by more than both interquartile ranges.  --only KEY measures one of sizes / options / progressive and, with
--out, replaces that key alone in an existing file.  With --job, a 64-view 1200 x 1600 precompute_guides_sharded into a temporary directory with jpeg_on_device off and on:
wall time, the sink's wait and the bytes that crossed to the host.  Every kernel_ms also carries the sha256 of its last call's output bytes, so that two builds of the library
(--lib PATH: that build in place of the package's own) can be held to the same bytes as well as the same time.  Prints one JSON line and, with --out, writes it to a file.
The timing loops, the statistic and the verdict's rule are tools/benchkit.py's.
Usage: python tools/jpeg_bench.py [--reps 200] [--job] [--only KEY] [--lib PATH] [--out profiles/jpeg_bench.json]"""
import hashlib
import io
import json
import os
import sys
import tempfile
import time

import numpy as np
import PIL
import torch
from PIL import Image, ImageFile

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))

import applied_image_processing_amd.runtime as rt  # noqa: E402
import applied_image_processing_amd.synth as synth  # noqa: E402
from applied_image_processing_amd import jobs  # noqa: E402
from applied_image_processing_amd.engine import AdaINEngine  # noqa: E402
from applied_image_processing_amd.telemetry import GpuTelemetry  # noqa: E402
from benchkit import arguments, below, emit, event_times, gpu_setup, header, spread, wall_ms  # noqa: E402

SIZES = [(256, 456), (1080, 1920), (1200, 1600)]
OPTION_SETS = {"q95_444_optimize": (95, "4:4:4", True), "q75_420_optimize": (75, "4:2:0", True), "q75_422": (75, "4:2:2", False)}


def sha256(out):
    """Of the files of an encode's (files, lengths)."""
    return hashlib.sha256(b"".join(rt.jpeg_files(*out))).hexdigest()


def hashed_event_ms(fn, reps, warmup):
    """The kit's event_ms with the sha256 of the last call's files beside it."""
    times, out = event_times(fn, reps, warmup)
    return dict(spread(times), sha256=sha256(out))


def pillow_bytes(a, options=None):
    f = io.BytesIO()
    if options is None:
        Image.fromarray(a).save(f, format="JPEG")
    else:
        ImageFile.MAXBLOCK = max(ImageFile.MAXBLOCK, 4 * a.size)          # Pillow's optimize buffer is w * h bytes: too small for noise
        Image.fromarray(a).save(f, format="JPEG", **options.save_kwargs())
    return f.getvalue()


def compare(x, options, reps, tel=None, label=None):
    """kernel_ms, device_ms, pillow_ms of one device frame x [1,h,w,3] under ``options`` (None: the default entry, no keywords)."""
    encode = (lambda: rt.jpeg_encode_u8(x)) if options is None else (lambda: options.encode(x))
    host = x[0].cpu().numpy()
    t0 = time.perf_counter()
    kernel = hashed_event_ms(encode, reps, 20)
    if tel is not None:
        tel.window(label, t0, time.perf_counter())
    device = wall_ms(lambda: rt.jpeg_files(*encode()), reps, 5, "before")
    pillow = wall_ms(lambda: pillow_bytes(host, options), reps, 3, "none")
    data, = rt.jpeg_files(*encode())
    return {"frame_bytes": int(x.numel()), "file_bytes": len(data), "same_bytes_as_pillow": data == pillow_bytes(host, options),
            "kernel_ms": kernel, "device_ms": device, "pillow_ms": pillow, "pillow_over_device": round(pillow["median"] / device["median"], 2),
            "faster_than_pillow": below(device, pillow)}


def guide_job(engine, on, views, style, sub_batch):
    names = [f"view_{k:03d}" for k in range(len(views))]
    with tempfile.TemporaryDirectory() as d:
        torch.cuda.synchronize()
        t = time.perf_counter()
        paths, info = jobs.precompute_guides_sharded(engine, views, names, d, style, content_size=0, sub_batch=sub_batch, jpeg_on_device=on)
        wall = time.perf_counter() - t
        size = sum(os.path.getsize(p) for p in paths.values())
    return {"wall_s": round(wall, 3), "sink_wait_s": round(info["sink_wait_s"], 3), "write_s": round(info["write_s"], 3), "d2h_bytes": int(info["d2h_bytes"]),
            "file_bytes": size}


def main():
    ap = arguments(__doc__, lib=True)
    ap.add_argument("--job", action="store_true")
    ap.add_argument("--views", type=int, default=64)
    ap.add_argument("--only", type=str, default=None, choices=["sizes", "options", "progressive"])
    args = ap.parse_args()
    dev = gpu_setup("jpeg_bench", args.lib)
    reps = max(args.reps, 200)
    engine = AdaINEngine(synth.to_torch(synth.vgg_state_dict(0, full=False)), synth.to_torch(synth.decoder_state_dict(0)), dev)
    engine.set_style(torch.from_numpy(synth.image(4, 1, 512, 512)).to(dev))
    tel = GpuTelemetry(0).start()
    res = header(reps=reps, pillow=PIL.__version__, sizes={}, options={}, progressive={})
    want = lambda key: args.only in (None, key)
    for h, w in SIZES:
        source = torch.from_numpy((synth.image(7, 1, h, w)[0].transpose(1, 2, 0) * np.float32(255)).astype(np.uint8)[None]).to(dev)
        frames = {"stylised": engine.stylize_u8(source, alpha=0.5).contiguous(),
                  "noise": torch.from_numpy(np.random.default_rng(0).integers(0, 256, (1, h, w, 3), dtype=np.uint8)).to(dev)}
        for kind, x in frames.items():
            if want("sizes"):
                res["sizes"][f"{kind}_{h}x{w}"] = compare(x, None, reps, tel, f"kernel_{kind}_{h}x{w}")
            if want("progressive"):
                entry = compare(x, rt.JpegOptions(progressive=True), reps)
                optimised = compare(x, rt.JpegOptions(optimize=True), reps)
                entry.update(optimize_file_bytes=optimised["file_bytes"], optimize_kernel_ms=optimised["kernel_ms"], optimize_device_ms=optimised["device_ms"])
                res["progressive"][f"{kind}_{h}x{w}"] = entry
            if want("options") and (h, w) == (1080, 1920):
                for name, o in OPTION_SETS.items():
                    res["options"].setdefault(name, {"quality": o[0], "subsampling": o[1], "optimize": o[2]})[f"{kind}_{h}x{w}"] = compare(
                        x, rt.JpegOptions(*o), reps)
    if want("sizes"):
        res["passes_1080p"] = all(below(v["device_ms"], v["pillow_ms"]) for k, v in res["sizes"].items() if k.endswith("1080x1920"))
    if args.job:
        base = [(synth.image(100 + k, 1, 1200, 1600)[0].transpose(1, 2, 0) * np.float32(255)).astype(np.uint8) for k in range(8)]
        views = [Image.fromarray(np.roll(base[k % 8], 16 * (k // 8), axis=1)) for k in range(args.views)]       # PIL views, as the 3DGS caller holds them
        style = torch.from_numpy(synth.image(4, 1, 512, 512))
        guide_job(engine, False, views[:8], style, 4)                     # warm-up: workspaces, pinned buffers, clocks
        guide_job(engine, True, views[:8], style, 4)
        res["guide_job_64x1200x1600"] = {"views": len(views), "off": guide_job(engine, False, views, style, 4), "on": guide_job(engine, True, views, style, 4)}
    res["telemetry"] = tel.stop()          # shader clock and power over each kernel timing window (sysfs reads)
    if args.only:
        res = {args.only: dict(res[args.only], reps=reps, pillow=res["pillow"], device=res["device"])}
        if args.out and os.path.exists(args.out):
            res = dict(json.load(open(args.out)), **res)
    emit(res, args.out)


if __name__ == "__main__":
    main()
