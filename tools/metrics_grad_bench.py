"""Times the device gradient of the image metrics (csrc/metrics.hip, adain_image_metrics_grad_f32) against the modelled project's training
loss under PyTorch-ROCm on the same machine, on four float32 RGB clips of uniform noise against itself +-3 - one frame of 256 x 456, of
1080 x 1920 and of 1200 x 1600 (the guide views), and 64 frames of 135 x 240.  Per clip, median and interquartile range over --reps calls
(>= 200) after warm-up, HIP events, device-resident tensors:
  device_backward_ms    ``runtime.image_metrics_grad`` alone (the gradient of a), weights {-0.2 / n, 0, 0.8 / n}
  device_loss_ms        ``metrics.dssim_loss(image, gt).backward()`` with the device route on: one forward call and one backward call
  torch_loss_ms         Style_3DGS/train.py's ``0.8 * l1_loss(image, gt) + 0.2 * (1 - ssim(image, gt))`` and its ``backward()`` as
                        utils/loss_utils.py writes them - five depthwise 11 x 11 convolutions, the elementwise passes, autograd - restated
                        below, not imported, on the same tensors; the window is made once outside the timed region
  kernels               the two kernels of device_backward_ms one by one, from the profiler's kernel records (torch.profiler, a run of
                        its own: no counters, nothing else timed meanwhile), microseconds
The baseline is not the code under test.  ``device_faster`` / ``device_slower``: device_loss_ms has its median below (above)
torch_loss_ms by more than both interquartile ranges.  Prints one JSON line and, with --out, writes it to a file.
The timing loops, the statistic and the verdict's rule are tools/benchkit.py's.
Usage: python tools/metrics_grad_bench.py [--reps 200] [--out profiles/metrics_grad_bench.json]"""
import json
import math
import os
import sys

import numpy as np
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))

import applied_image_processing_amd.metrics as M  # noqa: E402
import applied_image_processing_amd.runtime as rt  # noqa: E402
from benchkit import arguments, below, emit, event_ms, spread  # noqa: E402

CLIPS = [(1, 256, 456), (1, 1080, 1920), (1, 1200, 1600), (64, 135, 240)]
KERNELS = ("metrics_tile_kernel", "metrics_combine_kernel")


def window(channel, device):
    g = torch.tensor([math.exp(-(x - 5) ** 2 / float(2 * 1.5 ** 2)) for x in range(11)], dtype=torch.float32)
    g = (g / g.sum()).unsqueeze(1)
    return g.mm(g.t()).float()[None, None].expand(channel, 1, 11, 11).contiguous().to(device)


def torch_loss(x, y, win, lam=0.2):
    """train.py's loss from the reference's l1_loss and ssim expressions, torch on whatever device the tensors are on."""
    c = x.shape[1]
    mu1, mu2 = F.conv2d(x, win, padding=5, groups=c), F.conv2d(y, win, padding=5, groups=c)
    mu1_sq, mu2_sq, mu1_mu2 = mu1.pow(2), mu2.pow(2), mu1 * mu2
    s1 = F.conv2d(x * x, win, padding=5, groups=c) - mu1_sq
    s2 = F.conv2d(y * y, win, padding=5, groups=c) - mu2_sq
    s12 = F.conv2d(x * y, win, padding=5, groups=c) - mu1_mu2
    m = ((2 * mu1_mu2 + 0.01 ** 2) * (2 * s12 + 0.03 ** 2)) / ((mu1_sq + mu2_sq + 0.01 ** 2) * (s1 + s2 + 0.03 ** 2))
    return (1.0 - lam) * torch.abs(x - y).mean() + lam * (1.0 - m.mean())


def kernel_records(fn, reps):
    """The device time of each kernel of KERNELS over ``reps`` calls of ``fn``, from the profiler's kernel records."""
    from torch.profiler import ProfilerActivity, profile

    torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CUDA]) as prof:
        for _ in range(reps):
            fn()
        torch.cuda.synchronize()
    out = {}
    for key in KERNELS:
        times = [float(e.device_time_total) for e in prof.events() if key in e.name and e.device_time_total > 0]
        out[key + "_us"] = dict(spread(times, 2), records=len(times)) if len(times) >= 2 else {"records": len(times)}
    return out


def main():
    args = arguments(__doc__).parse_args()
    assert torch.cuda.is_available(), "metrics_grad_bench needs a GPU"
    torch.cuda.set_device(0)          # its own setup and header: the record has no CPU counts, and the host's threads are left as they are
    reps = max(args.reps, 200)
    dev = torch.device("cuda:0")
    res = {"device": torch.cuda.get_device_name(0), "reps": reps, "torch": torch.__version__, "lib": os.path.relpath(rt.LIB_PATH), "tile": list(rt.METRICS_TILE),
           "clips": {}}
    M.set_device_backward(True)
    for n, h, w in CLIPS:
        rng = np.random.default_rng(n * h * w)
        a = rng.integers(0, 256, (n, h, w, 3), dtype=np.uint8)
        b = np.clip(a.astype(np.int16) + rng.integers(-3, 4, a.shape), 0, 255).astype(np.uint8)
        fa, fb = (torch.from_numpy(t).to(dev).permute(0, 3, 1, 2).contiguous().to(torch.float32) / 255.0 for t in (a, b))
        weights = torch.tensor([[-0.2 / n, 0.0, 0.8 / n]] * n, dtype=torch.float64, device=dev)
        win = window(3, dev)
        x = fa.clone().requires_grad_()

        def device_loss():
            x.grad = None
            M.dssim_loss(x, fb).backward()

        def baseline():
            x.grad = None
            torch_loss(x, fb, win).backward()

        row = {"frames": n, "samples": int(fa.numel()),
               "device_backward_ms": event_ms(lambda: rt.image_metrics_grad(fa, fb, weights), reps, 20),
               "device_loss_ms": event_ms(device_loss, reps, 20), "torch_loss_ms": event_ms(baseline, reps, 20)}
        row["device_faster"], row["device_slower"] = below(row["device_loss_ms"], row["torch_loss_ms"]), below(row["torch_loss_ms"], row["device_loss_ms"])
        device_loss()
        got = x.grad.clone()
        baseline()
        row["grad_distance_from_torch"] = float((got - x.grad).abs().max() / x.grad.abs().max())
        try:
            row["kernels"] = kernel_records(lambda: rt.image_metrics_grad(fa, fb, weights), reps)
        except Exception as e:          # a profiler that cannot run costs the kernel figures, not the timings above
            row["kernels"] = {"error": f"{type(e).__name__}: {e}"}
        key = f"near_{n}x{h}x{w}"
        res["clips"][key] = row
        print(key, json.dumps(row), file=sys.stderr, flush=True)
    M.set_device_backward(False)
    emit(res, args.out)


if __name__ == "__main__":
    main()
