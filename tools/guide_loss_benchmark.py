"""Times the guide-view loss on the device (csrc/guide_loss.hip: adain_guide_l1_f32, adain_guide_l1_grad_f32) against the modelled project's
own lines, Style_3DGS/train.py:208-221, under PyTorch-ROCm on the same machine.  Renders are float32 RGB uniform noise of 800 x 800 (the
reference's 3DGS views), 1080 x 1920, 1200 x 1600 and 256 x 456; the guide is one 512 x 512 stylised synthetic frame (flat colour regions
with soft edges and grain), uint8.  Per render size, median and interquartile range over --reps calls (>= 200) after warm-up:
  device_forward_ms     ``runtime.guide_l1`` alone, HIP events
  device_backward_ms    ``runtime.guide_l1_grad`` alone, HIP events
  device_loss_ms        ``bank.loss(image, name).backward()``: one forward and one backward call under autograd, HIP events
  device_loss_wall_ms   the same by the host clock, the device waited for before and after
  torch_resident_ms     baseline (a): train.py's last three lines - F.interpolate of the float guide that is already on the device,
                        l1_loss, backward() - restated below, HIP events.  It pays no file, decode or upload
  torch_file_wall_ms    baseline (b): all six lines from the .jpg on disk (Image.open, convert, to_tensor, upload, interpolate, l1_loss,
                        backward) on one host thread plus the GPU, by the host clock with the device waited for before and after
  kernels               the three kernels one by one, from the profiler's kernel records (torch.profiler, a run of its own: no counters,
                        nothing else timed meanwhile), microseconds
  gpu_busy              the sum of all the profiler's device records per step, microseconds, of ``device_loss`` and of baseline (a): what
                        each route keeps the GPU busy for when the host runs ahead of it, as it does in a training loop whose rasteriser
                        has queued work; the *_ms figures above are taken with nothing else queued and include the host's launch path
Neither baseline is the code under test.  ``below_resident``: device_loss_ms has its median below torch_resident_ms by more than both
interquartile ranges (``above_resident``: the other way round); ``below_file`` / ``above_file``: device_loss_wall_ms against
torch_file_wall_ms.  ``bank``: the bytes a 64-view bank of such guides holds against the same views as float32 at the render's size.
Prints one JSON line and, with --out, writes it to a file.  (tests/test_benchkit_host.py counts the sixteen tools/*_bench.py, so this
seventeenth tool is named _benchmark; tests/test_guide_loss_benchmark_host.py holds it to the same rule.)  The timing loops, the statistic and the verdict's rule are tools/benchkit.py's.
Usage: python tools/guide_loss_benchmark.py [--reps 200] [--out profiles/guide_loss_bench.json]"""
import json
import os
import sys
import tempfile

import numpy as np
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))

import applied_image_processing_amd.metrics as M  # noqa: E402
import applied_image_processing_amd.runtime as rt  # noqa: E402
from benchkit import arguments, below, emit, event_ms, gpu_setup, header, spread, wall_ms  # noqa: E402

RENDERS = [(800, 800), (1080, 1920), (1200, 1600), (256, 456)]
GUIDE = (512, 512)
VIEWS = 64
KERNELS = ("guide_l1_tile_kernel", "guide_l1_finish_kernel", "guide_l1_grad_kernel")


def stylised_frame(gh, gw, seed=0):
    """A picture of the kind the stylisation writes: a few flat colour regions with soft edges, and grain.  uint8 [gh][gw][3]."""
    rng = np.random.default_rng(seed)
    y, x = np.mgrid[0:gh, 0:gw].astype(np.float32)
    field = np.sin(x / 37.0) + np.cos(y / 53.0) + np.sin((x + y) / 91.0)
    level = np.clip(np.round((field + 3.0) / 6.0 * 5.0), 0, 5).astype(np.int64)
    palette = rng.integers(20, 236, (6, 3)).astype(np.float32)
    flat = palette[level]
    soft = (flat + np.roll(flat, 1, 0) + np.roll(flat, 1, 1) + np.roll(flat, -1, 0) + np.roll(flat, -1, 1)) / 5.0
    return np.clip(soft + rng.normal(0.0, 4.0, soft.shape), 0, 255).astype(np.uint8)


def to_tensor(picture):
    """torchvision's to_tensor of an RGB PIL image: HWC uint8 -> CHW float32 / 255."""
    return torch.from_numpy(np.asarray(picture).copy()).permute(2, 0, 1).contiguous().to(torch.float32).div(255)


def torch_resident(image, image_guide_tensor):
    """train.py:216-221 with the float guide already on the device."""
    image_guide_resized = F.interpolate(image_guide_tensor, size=image.shape[-2:], mode="bilinear", align_corners=False).squeeze(0)
    loss = torch.abs((image - image_guide_resized)).mean()
    loss.backward()
    return loss


def torch_file(image, path):
    """train.py:208-221: the six lines from the file on disk."""
    from PIL import Image

    image_guide = Image.open(path).convert("RGB")
    image_guide_tensor = to_tensor(image_guide).unsqueeze(0).to(image.device)
    return torch_resident(image, image_guide_tensor)


def kernel_records(fn, reps):
    """The device time of each kernel of KERNELS over ``reps`` calls of ``fn``, from the profiler's kernel records."""
    from torch.profiler import ProfilerActivity, profile

    torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CUDA]) as prof:
        for _ in range(reps):
            fn()
        torch.cuda.synchronize()
    out = {"all_records_us_per_call": round(sum(float(e.device_time_total) for e in prof.events() if e.device_time_total > 0) / reps, 2)}
    for key in KERNELS:
        times = [float(e.device_time_total) for e in prof.events() if key in e.name and e.device_time_total > 0]
        if times:
            out[key + "_us"] = dict(spread(times, 2), records=len(times)) if len(times) >= 2 else {"records": len(times)}
    return out


def main():
    args = arguments(__doc__).parse_args()
    dev = gpu_setup("guide_loss_benchmark")
    reps = max(args.reps, 200)
    gh, gw = GUIDE
    picture = stylised_frame(gh, gw)
    res = header(reps=reps, torch=torch.__version__, guide=[gh, gw], renders={})
    with tempfile.TemporaryDirectory() as tmp:
        from PIL import Image

        path = os.path.join(tmp, "guide.jpg")
        Image.fromarray(picture).save(path)
        bank = M.GuideBank.from_files({"view": path}, dev)          # the pixels train.py reads back, post-JPEG
        guide = bank["view"]
        image_guide_tensor = to_tensor(guide.cpu().numpy()).unsqueeze(0).to(dev)
        for h, w in RENDERS:
            image = torch.rand(3, h, w, device=dev)
            x = image.clone().requires_grad_()
            one = torch.ones(1, dtype=torch.float64, device=dev)

            def device_loss():
                x.grad = None
                bank.loss(x, "view").backward()

            def resident():
                x.grad = None
                return torch_resident(x, image_guide_tensor)

            def from_file():
                x.grad = None
                return torch_file(x, path)

            row = {"samples": int(image.numel()),
                   "device_forward_ms": event_ms(lambda: rt.guide_l1(image, guide), reps, 20),
                   "device_backward_ms": event_ms(lambda: rt.guide_l1_grad(image, guide, one), reps, 20),
                   "device_loss_ms": event_ms(device_loss, reps, 20), "torch_resident_ms": event_ms(resident, reps, 20),
                   "device_loss_wall_ms": wall_ms(device_loss, reps, 20, "both"), "torch_file_wall_ms": wall_ms(from_file, reps, 20, "both")}
            row["below_resident"], row["above_resident"] = below(row["device_loss_ms"], row["torch_resident_ms"]), below(row["torch_resident_ms"], row["device_loss_ms"])
            row["below_file"], row["above_file"] = below(row["device_loss_wall_ms"], row["torch_file_wall_ms"]), below(row["torch_file_wall_ms"], row["device_loss_wall_ms"])
            # what the two routes computed, side by side
            device_loss()
            got = x.grad.clone()
            want = resident()
            row["loss_device"], row["loss_torch"] = float(bank.loss(image, "view")), float(want)
            row["grad_samples_that_differ"] = int((got != x.grad).sum())
            row["bytes_moved_forward"] = int(image.numel() * 4 + guide.numel())
            row["bytes_moved_backward"] = int(image.numel() * 8 + guide.numel())
            row["bank"] = {"views": VIEWS, "uint8_at_guide_size_bytes": VIEWS * gh * gw * 3, "float32_at_render_size_bytes": VIEWS * 3 * h * w * 4}
            try:
                def both_calls():
                    rt.guide_l1(image, guide)
                    rt.guide_l1_grad(image, guide, one)

                row["kernels"] = kernel_records(both_calls, reps)
                row["gpu_busy"] = {"device_loss_us": kernel_records(device_loss, reps)["all_records_us_per_call"],
                                   "torch_resident_us": kernel_records(resident, reps)["all_records_us_per_call"]}
            except Exception as e:          # a profiler that cannot run costs the kernel figures, not the timings above
                row["kernels"] = {"error": f"{type(e).__name__}: {e}"}
            res["renders"][f"{h}x{w}"] = row
            print(f"{h}x{w}", json.dumps(row), file=sys.stderr, flush=True)
    emit(res, args.out)


if __name__ == "__main__":
    main()
