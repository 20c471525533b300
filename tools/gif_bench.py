"""Times the device GIF writer (csrc/gif.hip) against Pillow's on the same machine, on three clips - one 1080 x 1920 frame, one 256 x 456
frame and 64 frames of 135 x 240 - each as a stylised synthetic clip (seed-0 weights) mapped onto the 8-colour palette slso8 and as
K = 256 uniform noise.  Per clip, median and interquartile range over --reps calls (>= 200) after warm-up:
  kernel_ms   adain_gif_encode_u8 on device-resident index planes, HIP events
  device_ms   wall clock from the device index planes to the file as host ``bytes``: the call, the lengths read, the copy of the records,
              the header and the trailer (gif_file.assemble)
  pillow_ms   Image.save(BytesIO, format="GIF", save_all=True) of the same P-mode frames on this machine's CPU, one thread
with the two files' sizes beside the times, and whether the device's file plays as the frames.  Pillow's figure is the median of
--pillow_reps calls (default: --reps; the number used is recorded).  ``faster_than_pillow`` / ``slower_than_pillow``: one median sits
below the other by more than both interquartile ranges.  Prints one JSON line and, with --out, writes it to a file.
The timing loops, the statistic and the verdict's rule are tools/benchkit.py's.
Usage: python tools/gif_bench.py [--reps 200] [--pillow_reps N] [--out profiles/gif_bench.json]"""
import io
import json
import os
import sys

import numpy as np
import PIL
import torch
from PIL import Image

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))

import applied_image_processing_amd.runtime as rt  # noqa: E402
import applied_image_processing_amd.synth as synth  # noqa: E402
from applied_image_processing_amd import gif_file, pixelize  # noqa: E402
from applied_image_processing_amd.engine import AdaINEngine  # noqa: E402
from benchkit import arguments, below, emit, event_ms, gpu_setup, header, wall_ms  # noqa: E402

CLIPS = [(1, 1080, 1920), (1, 256, 456), (64, 135, 240)]
SLSO8 = ["#0d2b45", "#203c56", "#544e68", "#8d697a", "#d08159", "#ffaa5e", "#ffd4a3", "#ffecd6"]          # lospec's slso8
DELAY = 5


def pillow_bytes(idx, pal):
    images = [Image.frombytes("P", (f.shape[1], f.shape[0]), f.tobytes()) for f in idx]
    for im in images:
        im.putpalette(pal.tobytes())
    f = io.BytesIO()
    images[0].save(f, format="GIF", save_all=True, append_images=images[1:], duration=DELAY * 10, loop=0)
    return f.getvalue()


def plays_as(data, want):
    im = Image.open(io.BytesIO(data))
    if im.n_frames != len(want):
        return False
    for i, frame in enumerate(want):
        im.seek(i)
        if not np.array_equal(np.asarray(im.convert("RGB")), frame):
            return False
    return True


def compare(idx, pal, reps, pillow_reps):
    """The figures of one clip: idx uint8 [n,h,w] on the device, pal uint8 [K,3]."""
    n, h, w = idx.shape
    K = len(pal)
    head = gif_file.header((w, h), pal, 0)
    encode = lambda: rt.gif_encode_u8(idx, K, DELAY)
    host = idx.cpu().numpy()
    kernel = event_ms(encode, reps, 20)
    device = wall_ms(lambda: gif_file.assemble(head, *encode()), reps, 5, "before")
    pillow = wall_ms(lambda: pillow_bytes(host, pal), pillow_reps, 1, "none")
    data = gif_file.assemble(head, *encode())
    return {"frames": n, "index_bytes": int(idx.numel()), "file_bytes": len(data), "pillow_file_bytes": len(pillow_bytes(host, pal)),
            "plays_as_the_frames": plays_as(data, pal[host]), "kernel_ms": kernel, "device_ms": device, "pillow_ms": pillow, "pillow_reps": pillow_reps,
            "faster_than_pillow": below(device, pillow), "slower_than_pillow": below(pillow, device)}


def main():
    ap = arguments(__doc__)
    ap.add_argument("--pillow_reps", type=int, default=None)
    args = ap.parse_args()
    dev = gpu_setup("gif_bench")
    reps = max(args.reps, 200)
    pillow_reps = max(4, args.pillow_reps or reps)
    engine = AdaINEngine(synth.to_torch(synth.vgg_state_dict(0, full=False)), synth.to_torch(synth.decoder_state_dict(0)), dev)
    engine.set_style(torch.from_numpy(synth.image(4, 1, 512, 512)).to(dev))
    slso8 = pixelize.parse_palette(SLSO8)
    grey = np.repeat(np.arange(256, dtype=np.uint8)[:, None], 3, axis=1)
    res = header(reps=reps, pillow=PIL.__version__, segment=rt.GIF_SEGMENT, clips={})
    for n, h, w in CLIPS:
        planes = []
        for i in range(0, n, 16):
            k = min(16, n - i)
            source = torch.from_numpy((synth.image(7 + i, k, h, w).transpose(0, 2, 3, 1) * np.float32(255)).astype(np.uint8)).to(dev)
            planes.append(rt.palette_map_u8(engine.stylize_u8(source, alpha=0.5).contiguous(), slso8, "nearest", index=True)[1])
        noise = torch.from_numpy(np.random.default_rng(n * h * w).integers(0, 256, (n, h, w), dtype=np.uint8)).to(dev)
        for kind, idx, pal in (("stylised_slso8", torch.cat(planes).contiguous(), slso8), ("noise_256", noise, grey)):
            key = f"{kind}_{n}x{h}x{w}"
            res["clips"][key] = compare(idx, pal, reps, pillow_reps)
            print(key, json.dumps(res["clips"][key]), file=sys.stderr, flush=True)
    emit(res, args.out)


if __name__ == "__main__":
    main()
