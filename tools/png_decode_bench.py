"""Times the device PNG file decoder (csrc/png_decode.hip, adain_png_decode_u8) against the host route through Pillow on the same machine:
the 800 x 800 fixture view (tests/golden/png/view_800.png) alone and as a batch of 64 copies, and a stylised 1080 x 1920 frame (seed-0
weights) written by Pillow and by the device encoder.  Median and interquartile range over --reps calls (>= 200; the batch rows over
--batch-reps, which the row records) after warm-up:
  kernel_ms  adain_png_decode_u8 itself on streams, output and workspace that are already on the device, HIP events around the C call
  stage_ms   its table, inflate and unfilter kernels one by one, from the profiler's kernel records of 20 of those calls (the C ABI has
             no entry per stage); {"error": ...} where the profiler gives none
  device_ms  wall clock from ``bytes`` to frames on the device with ``rt.png_decode_u8(mode="RGB")``: chunk walk, upload, decode, the record read
  host_ms    the route without it on one thread: ``Image.open(...).convert("RGB")`` + ``np.asarray`` + upload, synchronised
with the deflate blocks the device read, whether the two give the same pixels, and ``device_is_faster``: device_ms sits below host_ms by
more than the two interquartile ranges combined.  With --job, a 64-view ``precompute_guides_sharded`` from .png paths (copies of the
fixture view) with ``png_decode_on_device`` off and on: wall, the time the compute loop waited for the feeder, and the bytes that went
to the device (the feeder's uploads, and with the switch on the files).  Prints one JSON line and, with --out, writes it.
The timing loops, the statistic and the verdict's rule are tools/benchkit.py's.
Usage: python tools/png_decode_bench.py [--reps 200] [--batch-reps 200] [--job] [--out profiles/png_decode_bench.json]"""
import ctypes
import io
import json
import os
import shutil
import sys
import tempfile
import threading
import time

import numpy as np
import PIL
import torch
from PIL import Image

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)

import applied_image_processing_amd.png_file as png_file  # noqa: E402
import applied_image_processing_amd.runtime as rt  # noqa: E402
import applied_image_processing_amd.synth as synth  # noqa: E402
from applied_image_processing_amd import jobs  # noqa: E402
from applied_image_processing_amd.AdaIN import test as adain_test  # noqa: E402
from applied_image_processing_amd.engine import AdaINEngine  # noqa: E402
from benchkit import arguments, below, emit, event_ms, gpu_setup, header, spread, wall_ms  # noqa: E402

FIXTURE = os.path.join(ROOT, "tests", "golden", "png", "view_800.png")


def host_route(datas, dev):
    """The route without the decoder for the same bytes: PIL decode on one thread, then the pixels go up."""
    return [torch.from_numpy(np.asarray(Image.open(io.BytesIO(d)).convert("RGB")).copy()).to(dev) for d in datas]


def resident_call(parsed, dev):
    """adain_png_decode_u8 itself on streams, output, record and workspace that are already on the device: nothing but the C call's launches."""
    n, (h, w, c) = len(parsed), (parsed[0].h, parsed[0].w, parsed[0].c)
    offsets = [0]
    for p in parsed:
        offsets.append(offsets[-1] + len(p.stream))
    up = torch.frombuffer(bytearray(b"".join(p.stream for p in parsed)), dtype=torch.uint8).to(dev)
    off = (ctypes.c_uint64 * (n + 1))(*offsets)
    nbytes = rt.png_decode_sizes(n, h, w, c, max(len(p.stream) for p in parsed))
    ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    out = torch.empty((n, h, w, 3), dtype=torch.uint8, device=dev)
    record = torch.empty((n, 2), dtype=torch.int32, device=dev)

    def launch():
        rc = rt.lib().adain_png_decode_u8(up.data_ptr(), up.numel(), off, n, h, w, c, 3, out.data_ptr(), record.data_ptr(), ws.data_ptr(), nbytes,
                                          torch.cuda.current_stream().cuda_stream)
        assert rc == 0, rt.lib().adain_last_error().decode()

    launch()
    assert not record[:, 0].any().item()
    return launch


def stage_ms(launch, reps):
    """The call's kernels one by one, from the profiler's kernel records of ``reps`` calls: median and interquartile range per kernel name
    (the table kernel's launches of a call summed).  {"error": ...} where the profiler gives no kernel records."""
    try:
        from torch.profiler import ProfilerActivity, profile

        launch()
        torch.cuda.synchronize()
        per_call = []
        for _ in range(reps):
            with profile(activities=[ProfilerActivity.CUDA]) as prof:
                launch()
                torch.cuda.synchronize()
            sums = {}
            for e in prof.events():
                stage = next((s for s in ("table", "inflate", "unfilter") if f"pngd_{s}_kernel" in e.name), None)
                if stage is not None:
                    sums[stage] = sums.get(stage, 0.0) + float(getattr(e, "device_time", None) or getattr(e, "cuda_time", 0.0)) / 1e3
            per_call.append(sums)
        stages = {s for c in per_call for s in c}
        if stages != {"table", "inflate", "unfilter"}:
            return {"error": f"kernel records of {sorted(stages)} only"}
        return {s: spread([c[s] for c in per_call]) for s in ("table", "inflate", "unfilter")}
    except Exception as e:          # noqa: BLE001 - the figure is then missing, and says why
        return {"error": f"{type(e).__name__}: {e}"[:200]}


def row(datas, reps, dev):
    parsed = [png_file.parse(d) for d in datas]
    report = []
    got = rt.png_decode_u8(datas, dev, mode="RGB", report=report)
    same = all(bool(torch.equal(g, w)) for g, w in zip(got, host_route(datas, dev)))
    launch = resident_call(parsed, dev)
    kernel = event_ms(launch, reps, 5)
    stages = stage_ms(launch, min(reps, 20))
    device = wall_ms(lambda: rt.png_decode_u8(datas, dev, mode="RGB"), reps, 3, "both")          # both routes end on the device
    host = wall_ms(lambda: host_route(datas, dev), reps, 2, "both")
    return {"files": len(datas), "file_bytes": sum(len(d) for d in datas), "frame_bytes": sum(int(g.numel()) for g in got), "reps": reps,
            "path": report[0]["path"], "blocks": report[0]["blocks"], "same_pixels_as_host": same, "kernel_ms": kernel, "stage_ms": stages, "device_ms": device, "host_ms": host,
            "host_over_device": round(host["median"] / device["median"], 2), "device_is_faster": below(device, host), "device_is_slower": below(host, device)}


def guide_job(engine, on, views, style, sub_batch):
    names = [f"view_{k:03d}" for k in range(len(views))]
    frames = [0]                 # bytes of the decoded frames that the host route uploads itself (AdaIN.test._upload_rgb), which the feeder does not count
    upload = adain_test._upload_rgb

    lock = threading.Lock()

    def counting(img, device, mark=None):
        with lock:               # the feeder fetches on several threads
            frames[0] += img.size[0] * img.size[1] * 3
        return upload(img, device, mark)

    adain_test._upload_rgb = counting
    try:
        with tempfile.TemporaryDirectory() as d:
            torch.cuda.synchronize()
            t = time.perf_counter()
            _, info = jobs.precompute_guides_sharded(engine, views, names, d, style, content_size=0, sub_batch=sub_batch, png_decode_on_device=on)
            wall = time.perf_counter() - t
    finally:
        adain_test._upload_rgb = upload
    files = sum(os.path.getsize(v) for v in views) if on else 0
    return {"wall_s": round(wall, 3), "feeder_wait_s": round(info["fetch_s"], 3), "h2d_bytes": int(info["h2d_bytes"]) + frames[0] + files}


def main():
    ap = arguments(__doc__)
    ap.add_argument("--batch-reps", type=int, default=200)
    ap.add_argument("--large-reps", type=int, default=200, help="calls of the 1080 x 1920 rows")
    ap.add_argument("--job", action="store_true")
    ap.add_argument("--views", type=int, default=64)
    args = ap.parse_args()
    dev = gpu_setup("png_decode_bench")
    reps = max(args.reps, 200)
    engine = AdaINEngine(synth.to_torch(synth.vgg_state_dict(0, full=False)), synth.to_torch(synth.decoder_state_dict(0)), dev)
    engine.set_style(torch.from_numpy(synth.image(4, 1, 512, 512)).to(dev))
    with open(FIXTURE, "rb") as f:
        view = f.read()
    source = torch.from_numpy((synth.image(7, 1, 1080, 1920)[0].transpose(1, 2, 0) * np.float32(255)).astype(np.uint8)[None]).to(dev)
    stylised = engine.stylize_u8(source, alpha=0.5).contiguous()
    by_pillow = io.BytesIO()
    Image.fromarray(stylised[0].cpu().numpy()).save(by_pillow, format="PNG")
    by_device, = rt.png_files(*rt.png_encode_u8(stylised))
    res = header(pillow=PIL.__version__, rows={})
    for name, datas, n in (("view_800x800", [view], reps), ("view_800x800_x64", [view] * 64, max(args.batch_reps, 8)),
                           ("stylised_1080x1920_pillow", [by_pillow.getvalue()], max(args.large_reps, 8)),
                           ("stylised_1080x1920_device", [by_device], max(args.large_reps, 8))):
        res["rows"][name] = row(datas, n, dev)
        print(f"{name}: {json.dumps(res['rows'][name])}", file=sys.stderr, flush=True)
    if args.job:
        with tempfile.TemporaryDirectory() as d:
            views = []
            for k in range(args.views):
                views.append(os.path.join(d, f"view_{k:03d}.png"))
                shutil.copyfile(FIXTURE, views[-1])
            style = torch.from_numpy(synth.image(4, 1, 512, 512))
            for on in (False, True):
                guide_job(engine, on, views[:8], style, 8)                   # warm-up: workspaces, pinned buffers, clocks
            res["job"] = {"views": args.views, "sub_batch": 8, "off": [guide_job(engine, False, views, style, 8) for _ in range(3)],
                          "on": [guide_job(engine, True, views, style, 8) for _ in range(3)]}
    emit(res, args.out)


if __name__ == "__main__":
    main()
