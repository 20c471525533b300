"""Times the device PNG writer (csrc/png.hip) against Pillow's on the same machine, at 256 x 456, 1080 x 1920 and 1200 x 1600, on a stylised
synthetic frame (seed-0 weights), a noisy gradient and a masked view (an object on black).  Per frame, median and interquartile range
over --reps calls (>= 200) after warm-up:
  kernel_ms     adain_png_encode_u8 on a device-resident frame, HIP events
  device_ms     wall clock from the device uint8 frame to host ``bytes``: the call, the length read, the copy of exactly that many bytes
  pillow_ms     Image.fromarray(frame).save(BytesIO, format="PNG") of the same frame on this machine's CPU, one thread
  pillow_l1_ms  the same with compress_level=1, Pillow's fast setting
with the three files' sizes beside the times, and whether the device's file decodes to the frame.  Pillow's two figures are medians of
--pillow_reps calls (default: --reps; a 1080p save takes about half a second, so a short run lowers it - the number used is recorded).
``faster_than_pillow`` / ``faster_than_pillow_l1``: the device median sits below Pillow's by more than both interquartile ranges.
With --job, a 64-view 1200 x 1600 precompute_guides_sharded(save_ext=".png") into a temporary directory with png_on_device off and on:
wall time, the sink's wait and the bytes that crossed to the host.  Prints one JSON line and, with --out, writes it to a file.
The timing loops, the statistic and the verdict's rule are tools/benchkit.py's.
Usage: python tools/png_bench.py [--reps 200] [--pillow_reps N] [--job] [--out profiles/png_bench.json]"""
import io
import json
import os
import sys
import tempfile
import time

import numpy as np
import PIL
import torch
from PIL import Image

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))

import applied_image_processing_amd.runtime as rt  # noqa: E402
import applied_image_processing_amd.synth as synth  # noqa: E402
from applied_image_processing_amd import jobs  # noqa: E402
from applied_image_processing_amd.engine import AdaINEngine  # noqa: E402
from benchkit import arguments, below, emit, event_ms, gpu_setup, header, wall_ms  # noqa: E402

SIZES = [(256, 456), (1080, 1920), (1200, 1600)]


def pillow_bytes(a, **kw):
    f = io.BytesIO()
    Image.fromarray(a).save(f, format="PNG", **kw)
    return f.getvalue()


def noisy_gradient(h, w, seed=1):
    rng = np.random.default_rng(seed)
    y, x = np.mgrid[0:h, 0:w]
    g = np.stack([x * 255 // w, y * 255 // h, (x + y) * 255 // (w + h)], 2) + rng.integers(-6, 7, (h, w, 3))
    return np.clip(g, 0, 255).astype(np.uint8)


def compare(x, reps, pillow_reps):
    """The figures of one device frame x [1,h,w,3]."""
    encode = lambda: rt.png_encode_u8(x)
    host = x[0].cpu().numpy()
    kernel = event_ms(encode, reps, 20)
    device = wall_ms(lambda: rt.png_files(*encode()), reps, 5, "before")
    pillow = wall_ms(lambda: pillow_bytes(host), pillow_reps, 1, "none")
    fast = wall_ms(lambda: pillow_bytes(host, compress_level=1), pillow_reps, 1, "none")
    data, = rt.png_files(*encode())
    return {"frame_bytes": int(x.numel()), "file_bytes": len(data), "pillow_file_bytes": len(pillow_bytes(host)),
            "pillow_l1_file_bytes": len(pillow_bytes(host, compress_level=1)), "decodes_to_the_frame": bool(np.array_equal(np.asarray(Image.open(io.BytesIO(data))), host)),
            "kernel_ms": kernel, "device_ms": device, "pillow_ms": pillow, "pillow_l1_ms": fast, "pillow_reps": pillow_reps,
            "faster_than_pillow": below(device, pillow), "faster_than_pillow_l1": below(device, fast)}


def guide_job(engine, on, views, style, sub_batch):
    names = [f"view_{k:03d}" for k in range(len(views))]
    with tempfile.TemporaryDirectory() as d:
        torch.cuda.synchronize()
        t = time.perf_counter()
        paths, info = jobs.precompute_guides_sharded(engine, views, names, d, style, content_size=0, sub_batch=sub_batch, save_ext=".png", png_on_device=on)
        wall = time.perf_counter() - t
        size = sum(os.path.getsize(p) for p in paths.values())
    return {"wall_s": round(wall, 3), "sink_wait_s": round(info["sink_wait_s"], 3), "write_s": round(info["write_s"], 3), "d2h_bytes": int(info["d2h_bytes"]),
            "file_bytes": size}


def main():
    ap = arguments(__doc__)
    ap.add_argument("--pillow_reps", type=int, default=None)
    ap.add_argument("--job", action="store_true")
    ap.add_argument("--views", type=int, default=64)
    args = ap.parse_args()
    dev = gpu_setup("png_bench")
    reps = max(args.reps, 200)
    pillow_reps = max(4, args.pillow_reps or reps)
    engine = AdaINEngine(synth.to_torch(synth.vgg_state_dict(0, full=False)), synth.to_torch(synth.decoder_state_dict(0)), dev)
    engine.set_style(torch.from_numpy(synth.image(4, 1, 512, 512)).to(dev))
    res = header(reps=reps, pillow=PIL.__version__, sizes={})
    for h, w in SIZES:
        source = torch.from_numpy((synth.image(7, 1, h, w)[0].transpose(1, 2, 0) * np.float32(255)).astype(np.uint8)[None]).to(dev)
        gradient = noisy_gradient(h, w)
        y, x = np.mgrid[0:h, 0:w]
        inside = ((y - h / 2) ** 2 + (x - w / 2) ** 2) < (min(h, w) / 3) ** 2
        frames = {"stylised": engine.stylize_u8(source, alpha=0.5).contiguous(), "gradient": torch.from_numpy(gradient[None]).to(dev),
                  "masked": torch.from_numpy((gradient * inside[:, :, None].astype(np.uint8))[None]).to(dev)}
        for kind, frame in frames.items():
            res["sizes"][f"{kind}_{h}x{w}"] = compare(frame, reps, pillow_reps)
            print(f"{kind}_{h}x{w}", json.dumps(res["sizes"][f"{kind}_{h}x{w}"]), file=sys.stderr, flush=True)
    if args.job:
        base = [(synth.image(100 + k, 1, 1200, 1600)[0].transpose(1, 2, 0) * np.float32(255)).astype(np.uint8) for k in range(8)]
        views = [Image.fromarray(np.roll(base[k % 8], 16 * (k // 8), axis=1)) for k in range(args.views)]       # PIL views, as the 3DGS caller holds them
        style = torch.from_numpy(synth.image(4, 1, 512, 512))
        guide_job(engine, False, views[:4], style, 4)                     # warm-up: workspaces, pinned buffers, clocks
        guide_job(engine, True, views[:4], style, 4)
        res["guide_job_64x1200x1600"] = {"views": len(views), "off": guide_job(engine, False, views, style, 4), "on": guide_job(engine, True, views, style, 4)}
    emit(res, args.out)


if __name__ == "__main__":
    main()
