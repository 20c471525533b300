"""Times the device GIF reader (csrc/gif_decode.hip, adain_gif_decode_u8) against Pillow on the same machine: file bytes in host memory ->
frames uint8 [n,H,W,3] on the device.  Medians and interquartile ranges over --reps calls (>= 200) after warm-up, by tools/benchkit.py's
rules; a cell stops early once --budget_s seconds of calls are spent (``calls`` records how many were made).  Per clip:
  pillow_ms  [np.asarray(f.convert("RGB")) for f in ImageSequence.Iterator(Image.open(...))] on one host thread, stacked and uploaded
  device_ms  wall clock of ``rt.gif_decode_u8``: the host walk, one upload, the call, the record read
  kernel_ms  adain_gif_decode_u8 itself on a table, blob, output and workspace that are already on the device, HIP events around the C call
  stage_ms   its two kernels, unlzw and compose, from the profiler's kernel records of a run of their own; null where it gives none
``faster`` / ``slower``: device_ms' median sits below / above pillow_ms' by more than both interquartile ranges.
The clips: the package's own writer's 64-frame slso8 clips at 256 x 456 and 1080 x 1920 (``gif_file.write_gif``: full frames, a CLEAR
every 2048 pixels), a 16-frame clip of noise on 256 colours at 256 x 456, a 32-frame clip Pillow's encoder optimised (sub-rectangles and
transparency), and with --file PATH any clip named on the command line.  Nothing outside this repository is read by default.
(This tool's name does not end in _bench.py: tests/test_benchkit_host.py counts those.)
Usage: python tools/gif_decode_timing.py [--reps 200] [--budget_s 25] [--file clip.gif ...] [--out profiles/gif_decode_bench.json]"""
import io
import json
import os
import sys
import time

import numpy as np
import PIL
import torch
from PIL import Image

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))

import applied_image_processing_amd.runtime as rt  # noqa: E402
import applied_image_processing_amd.synth as synth  # noqa: E402
from applied_image_processing_amd import gif_file  # noqa: E402
from benchkit import arguments, below, gpu_setup, header, spread, write  # noqa: E402

SLSO8 = ["#0d2b45", "#203c56", "#544e68", "#8d697a", "#d08159", "#ffaa5e", "#ffd4a3", "#ffecd6"]
STAGES = {"unlzw": "gifd_unlzw_kernel", "compose": "gifd_compose_kernel"}


def own_clip(dev, h, w, n, tmp):
    """The package's writer on a synthetic frame that drifts: n full frames on slso8."""
    base = torch.from_numpy((synth.image(5, 1, h, w)[0].transpose(1, 2, 0) * 255).astype(np.uint8)).to(dev)
    frames = torch.stack([torch.roll(base, shifts=(3 * i, 5 * i), dims=(0, 1)) for i in range(n)])
    gif_file.write_gif(frames, tmp, SLSO8, fps=20)
    with open(tmp, "rb") as f:
        return f.read()


def noise_clip(dev, h, w, n, tmp):
    rng = np.random.default_rng(3)
    palette = rng.integers(0, 256, (256, 3)).astype(np.uint8)
    frames = torch.from_numpy(palette[rng.integers(0, 256, (n, h, w))]).to(dev)
    gif_file.write_gif(frames, tmp, palette, fps=20, method="rgb")
    with open(tmp, "rb") as f:
        return f.read()


def pillow_optimised_clip(h, w, n):
    rng = np.random.default_rng(4)
    back = (rng.integers(0, 4, (h // 8, w // 8, 3)) * 64).astype(np.uint8).repeat(8, 0).repeat(8, 1)
    images = []
    for i in range(n):
        a = back.copy()
        a[20 + 5 * i:80 + 5 * i, 30 + 9 * i:120 + 9 * i] = (250, 10 + 7 * i, 30)
        images.append(Image.fromarray(a).quantize(64) if i == 0 else Image.fromarray(a).quantize(palette=images[0]))
    buf = io.BytesIO()
    images[0].save(buf, format="GIF", save_all=True, append_images=images[1:], optimize=True, disposal=1, duration=50, loop=0)
    return buf.getvalue()


def budgeted(fn, reps, warmup, budget_s, sync, events=False):
    """benchkit's wall_times / event_times with a budget: {median, iqr, calls}."""
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    times, spent = [], 0.0
    while len(times) < reps and spent < budget_s:
        t = time.perf_counter()
        if events:
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            fn()
            b.record()
            b.synchronize()
            times.append(a.elapsed_time(b))
        else:
            fn()
            if sync:
                torch.cuda.synchronize()
            times.append((time.perf_counter() - t) * 1e3)
        spent += time.perf_counter() - t
    return dict(spread(times), calls=len(times))


def stage_ms(fn, reps):
    """{stage: {median, iqr}} of the call's kernels from torch's profiler, or None where it records no kernels."""
    try:
        from torch.profiler import ProfilerActivity, profile

        with profile(activities=[ProfilerActivity.CUDA]) as prof:
            for _ in range(reps):
                fn()
            torch.cuda.synchronize()
        out = {}
        for stage, kernel in STAGES.items():
            times = [e.device_time_total / 1e3 for e in prof.events() if kernel in e.name]
            if len(times) < 2:
                return None
            out[stage] = spread(times)
        return out
    except Exception:
        return None


def cell(data, dev, reps, budget_s):
    clip = gif_file.parse(data)
    report = []
    got, info = rt.gif_decode_u8(data, dev, report=report)
    want, _ = gif_file.pil_clip(data)
    assert report[0]["path"] == "device" and np.array_equal(got.cpu().numpy(), want), "the device's frames are not Pillow's"
    rows, blob = rt.gif_decode_table(clip)
    n = len(rows)
    table = np.asarray(rows, dtype=np.uint64).tobytes()
    up = torch.frombuffer(bytearray(table + blob + b"\0"), dtype=torch.uint8).to(dev)
    nbytes = rt.gif_decode_sizes(n, clip.h, clip.w, max(f.w * f.h for f in clip.frames))
    ws = torch.empty(max(nbytes, 256), dtype=torch.uint8, device=dev)
    out = torch.empty((n, clip.h, clip.w, 3), dtype=torch.uint8, device=dev)
    record = torch.empty((n, 2), dtype=torch.int32, device=dev)
    del got

    def kernel():
        rt.call("adain_gif_decode_u8", dev, up.data_ptr() + len(table), len(blob), up.data_ptr(), n, clip.h, clip.w, out.data_ptr(), record.data_ptr(), ws.data_ptr(), nbytes)

    r = {"frames": n, "screen": [clip.h, clip.w], "file_bytes": len(data), "codes": report[0]["codes"],
         "sub_rectangles": sum((f.w, f.h) != (clip.w, clip.h) for f in clip.frames), "transparent_frames": sum(f.transparent is not None for f in clip.frames),
         "kernel_ms": budgeted(kernel, reps, 3, budget_s, True, events=True), "stage_ms": stage_ms(kernel, 5),
         "device_ms": budgeted(lambda: rt.gif_decode_u8(data, dev), reps, 2, budget_s, True),
         "pillow_ms": budgeted(lambda: torch.from_numpy(gif_file.pil_clip(data)[0]).to(dev), reps, 1, budget_s, True)}
    known = r["device_ms"]["iqr"] is not None and r["pillow_ms"]["iqr"] is not None
    r["faster"] = below(r["device_ms"], r["pillow_ms"]) if known else None
    r["slower"] = below(r["pillow_ms"], r["device_ms"]) if known else None
    if r["stage_ms"]:
        r["unlzw_share"] = round(r["stage_ms"]["unlzw"]["median"] / (r["stage_ms"]["unlzw"]["median"] + r["stage_ms"]["compose"]["median"]), 3)
    return r


def main():
    ap = arguments(__doc__)
    ap.add_argument("--budget_s", type=float, default=25)
    ap.add_argument("--file", action="append", default=[])
    ap.add_argument("--only", action="append", default=[], help="run only the named built-in clips")
    args = ap.parse_args()
    dev = gpu_setup("gif_decode_timing")
    import tempfile

    reps = max(args.reps, 200)
    res = header(reps=reps, budget_s=args.budget_s, pillow=PIL.__version__, gif_decode_lib=os.path.relpath(rt.GIF_DECODE_LIB_PATH), clips={})
    with tempfile.TemporaryDirectory() as tmp:
        path = os.path.join(tmp, "clip.gif")
        makers = {"own_slso8_256x456_x64": lambda: own_clip(dev, 256, 456, 64, path), "own_slso8_1080x1920_x64": lambda: own_clip(dev, 1080, 1920, 64, path),
                  "noise_K256_256x456_x16": lambda: noise_clip(dev, 256, 456, 16, path), "pillow_optimised_256x456_x32": lambda: pillow_optimised_clip(256, 456, 32)}
        for name, make in makers.items():
            if args.only and name not in args.only:
                continue
            res["clips"][name] = cell(make(), dev, reps, args.budget_s)
            print(name, json.dumps(res["clips"][name]), file=sys.stderr, flush=True)
            write(json.dumps(res), args.out)
    for path in args.file:
        with open(path, "rb") as f:
            res["clips"][os.path.basename(path)] = cell(f.read(), dev, reps, args.budget_s)
        write(json.dumps(res), args.out)
    line = json.dumps(res)
    print(line)
    write(line, args.out)


if __name__ == "__main__":
    main()
