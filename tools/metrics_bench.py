"""Times the device image metrics (csrc/metrics.hip) against the modelled project's own expressions on the same machine, on four clips
of uniform noise against itself +-3 - one frame of 256 x 456, of 1080 x 1920 and of 1200 x 1600, and 64 frames of 135 x 240, RGB.  Per
clip, median and interquartile range over --reps calls (>= 200) after warm-up, from device-resident frames to the records:
  device_u8_ms, device_u8_map_ms      adain_image_metrics_u8 on the uint8 frames without and with the map, HIP events
  device_f32_ms, device_f32_map_ms    adain_image_metrics_f32 on the float32 NCHW tensors of the same frames, HIP events
  torch_gpu_ms   utils/loss_utils.py ssim (per image) and utils/image_utils.py psnr as the reference writes them - five depthwise 11 x 11
                 convolutions and the elementwise passes - restated below, not imported, run by PyTorch-ROCm on the same float32 tensors on
                 the same GPU, HIP events; the window is made once outside the timed region, which the reference does per call
  torch_cpu_ms   the same expressions on one host thread, wall clock, --cpu_reps calls (the number used is recorded)
Neither baseline is the code under test.  ``faster_than_torch_gpu`` / ``slower_than_torch_gpu`` (and ``..._torch_cpu``): device_f32_ms -
the same input as the baseline's - has its median below (above) the other by more than both interquartile ranges.  Prints one JSON line
and, with --out, writes it to a file.
The timing loops, the statistic and the verdict's rule are tools/benchkit.py's.
Usage: python tools/metrics_bench.py [--reps 200] [--cpu_reps 5] [--out profiles/metrics_bench.json]"""
import json
import math
import os
import sys

import numpy as np
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))

import applied_image_processing_amd.runtime as rt  # noqa: E402
from benchkit import arguments, below, emit, event_ms, gpu_setup, header, wall_ms  # noqa: E402

CLIPS = [(1, 256, 456), (1, 1080, 1920), (1, 1200, 1600), (64, 135, 240)]


def window(channel, device):
    g = torch.tensor([math.exp(-(x - 5) ** 2 / float(2 * 1.5 ** 2)) for x in range(11)], dtype=torch.float32)
    g = (g / g.sum()).unsqueeze(1)
    return g.mm(g.t()).float()[None, None].expand(channel, 1, 11, 11).contiguous().to(device)


def torch_scores(x, y, win):
    """The reference's ssim(size_average=False) and psnr on [n,c,h,w] float32, torch on whatever device the tensors are on."""
    c = x.shape[1]
    mu1, mu2 = F.conv2d(x, win, padding=5, groups=c), F.conv2d(y, win, padding=5, groups=c)
    mu1_sq, mu2_sq, mu1_mu2 = mu1.pow(2), mu2.pow(2), mu1 * mu2
    s1 = F.conv2d(x * x, win, padding=5, groups=c) - mu1_sq
    s2 = F.conv2d(y * y, win, padding=5, groups=c) - mu2_sq
    s12 = F.conv2d(x * y, win, padding=5, groups=c) - mu1_mu2
    m = ((2 * mu1_mu2 + 0.01 ** 2) * (2 * s12 + 0.03 ** 2)) / ((mu1_sq + mu2_sq + 0.01 ** 2) * (s1 + s2 + 0.03 ** 2))
    mse = ((x - y) ** 2).view(x.shape[0], -1).mean(1, keepdim=True)
    return m.mean(1).mean(1).mean(1), 20 * torch.log10(1.0 / torch.sqrt(mse))


def main():
    ap = arguments(__doc__)
    ap.add_argument("--cpu_reps", type=int, default=5)
    args = ap.parse_args()
    dev = gpu_setup("metrics_bench")
    reps, cpu_reps = max(args.reps, 200), max(3, args.cpu_reps)
    res = header(reps=reps, cpu_reps=cpu_reps, torch=torch.__version__, tile=list(rt.METRICS_TILE), clips={})
    for n, h, w in CLIPS:
        rng = np.random.default_rng(n * h * w)
        a = rng.integers(0, 256, (n, h, w, 3), dtype=np.uint8)
        b = np.clip(a.astype(np.int16) + rng.integers(-3, 4, a.shape), 0, 255).astype(np.uint8)
        ua, ub = torch.from_numpy(a).to(dev), torch.from_numpy(b).to(dev)
        fa, fb = (t.permute(0, 3, 1, 2).contiguous().to(torch.float32) / 255.0 for t in (ua, ub))
        ca, cb, win_gpu, win_cpu = fa.cpu(), fb.cpu(), window(3, dev), window(3, "cpu")
        row = {"frames": n, "samples": int(ua.numel()),
               "device_u8_ms": event_ms(lambda: rt.image_metrics(ua, ub), reps, 20), "device_u8_map_ms": event_ms(lambda: rt.image_metrics(ua, ub, True), reps, 20),
               "device_f32_ms": event_ms(lambda: rt.image_metrics(fa, fb), reps, 20), "device_f32_map_ms": event_ms(lambda: rt.image_metrics(fa, fb, True), reps, 20),
               "torch_gpu_ms": event_ms(lambda: torch_scores(fa, fb, win_gpu), reps, 20), "torch_cpu_ms": wall_ms(lambda: torch_scores(ca, cb, win_cpu), cpu_reps, 1, "none")}
        got, (want_s, want_p) = rt.image_metrics(fa, fb), torch_scores(fa, fb, win_gpu)
        row["ssim_distance_from_torch_gpu"] = float((got.ssim - want_s.double()).abs().max())
        row["psnr_distance_from_torch_gpu"] = float((got.psnr - want_p.double().reshape(-1)).abs().max())
        for other in ("torch_gpu", "torch_cpu"):
            row["faster_than_" + other], row["slower_than_" + other] = below(row["device_f32_ms"], row[other + "_ms"]), below(row[other + "_ms"], row["device_f32_ms"])
        key = f"near_{n}x{h}x{w}"
        res["clips"][key] = row
        print(key, json.dumps(row), file=sys.stderr, flush=True)
    emit(res, args.out)


if __name__ == "__main__":
    main()
