"""Times the device palette kernels (csrc/palette.hip) against their host forms on the same machine, at 256 x 456 and 1080 x 1920 with
palettes of K = 8 and K = 16 colours, on a noisy gradient.  Per cell (method, size, K), median and interquartile range:
  device_ms   device frame -> device frame, HIP events, --reps calls (>= 200) after warm-up:
              "rgb" / "nearest": adain_palette_map_u8; "diffused": adain_palette_dither_u8
  host_ms     one thread on this machine's CPU:
              "rgb" / "nearest": the restatement's vectorised NumPy form (tests/palette_ref.py, map_frame: an H x W x K x 3 array)
              "diffused": the sequential loop (tests/palette_ref.py, dither_push)
              --reps calls where a call takes under a second; --slow_reps (default 20) where it takes seconds (on the machine of
              profiles/palette_bench.json: the diffused loop at 1080p, 14.5 s a call); --slowest_reps (default: --slow_reps) where it takes
              more than 20 s.  ``host_calls`` records the number used.
``device_faster``: the device median sits below the host's by more than both interquartile ranges; ``same_bytes``: both gave the same frame.
Prints one JSON line and, with --out, writes it to a file after every cell.  --skip_host / --methods / --sizes / --ks narrow a run; a cell
that was not run is absent.  --merge starts from the cells --out already holds (the host loops make a full run long: it may be made in parts).
The timing loops, the statistic and the verdict's rule are tools/benchkit.py's.
Usage: python tools/palette_bench.py [--reps 200] [--slow_reps 20] [--slowest_reps N] [--merge] [--out profiles/palette_bench.json]"""
import os

for _v in ("OMP_NUM_THREADS", "OPENBLAS_NUM_THREADS", "MKL_NUM_THREADS"):          # before NumPy loads: the host form runs on one thread
    os.environ[_v] = "1"

import json  # noqa: E402
import sys  # noqa: E402
import time  # noqa: E402

import numpy as np  # noqa: E402
import torch  # noqa: E402

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import applied_image_processing_amd.runtime as rt  # noqa: E402
import palette_ref as R  # noqa: E402
from benchkit import arguments, below, emit, event_ms, gpu_setup, header, spread, write  # noqa: E402

SIZES = {"256x456": (256, 456), "1080x1920": (1080, 1920)}
PALETTES = {8: ["#0d2b45", "#203c56", "#544e68", "#8d697a", "#d08159", "#ffaa5e", "#ffd4a3", "#ffecd6"],
            16: ["#1a1c2c", "#5d275d", "#b13e53", "#ef7d57", "#ffcd75", "#a7f070", "#38b764", "#257179", "#29366f", "#3b5dc9", "#41a6f6", "#73eff7", "#f4f4f4",
                 "#94b0c2", "#566c86", "#333c57"]}
METHODS = ("rgb", "nearest", "diffused")


def host_ms(fn, reps, label):
    """A loop of its own: no warm-up call (the caller's sizing call is it), and a progress line for every call over 5 s."""
    times = []
    for i in range(reps):
        t = time.perf_counter()
        fn()
        times.append((time.perf_counter() - t) * 1e3)
        if times[-1] > 5e3:
            print(f"{label}: host call {i + 1} of {reps}: {times[-1] / 1e3:.1f} s", file=sys.stderr, flush=True)
    return spread(times)


def noisy_gradient(h, w, seed=1):
    rng = np.random.default_rng(seed)
    y, x = np.mgrid[0:h, 0:w]
    g = np.stack([x * 255 // w, y * 255 // h, (x + y) * 255 // (w + h)], 2) + rng.integers(-6, 7, (h, w, 3))
    return np.clip(g, 0, 255).astype(np.uint8)


def main():
    ap = arguments(__doc__)
    ap.add_argument("--slow_reps", type=int, default=20)
    ap.add_argument("--slowest_reps", type=int, default=None)
    ap.add_argument("--skip_host", action="store_true")
    ap.add_argument("--methods", default=",".join(METHODS))
    ap.add_argument("--sizes", default=",".join(SIZES))
    ap.add_argument("--ks", default=",".join(str(k) for k in PALETTES))
    ap.add_argument("--merge", action="store_true")
    args = ap.parse_args()
    dev = gpu_setup("palette_bench")
    reps = max(args.reps, 200)
    slowest = args.slowest_reps or args.slow_reps
    res = header(numpy=np.__version__, reps=reps, slow_reps=args.slow_reps, slowest_reps=slowest, band=rt.PALETTE_DITHER_BAND, cells={})
    if args.merge and args.out and os.path.exists(args.out):
        with open(args.out) as f:
            res["cells"] = json.load(f)["cells"]
    from applied_image_processing_amd.pixelize import parse_palette
    for size in args.sizes.split(","):
        h, w = SIZES[size]
        frame = noisy_gradient(h, w)
        x = torch.from_numpy(frame[None]).to(dev)
        for K in (int(k) for k in args.ks.split(",")):
            pal = parse_palette(PALETTES[K])
            p = torch.from_numpy(pal).to(dev)
            for method in args.methods.split(","):
                label = f"{method}_{size}_K{K}"
                if method == "diffused":
                    device, host = (lambda: rt.palette_dither_u8(x, p)), (lambda: R.dither_push(frame, pal)[0])
                else:
                    device, host = (lambda: rt.palette_map_u8(x, p, method)), (lambda: R.map_frame(frame, pal, method))
                cell = {"device_ms": event_ms(device, reps, 5)}
                if not args.skip_host:
                    t = time.perf_counter()
                    want = host()          # the warm-up call sizes the run and checks the bytes
                    first = time.perf_counter() - t
                    calls = reps if first < 1 else args.slow_reps if first < 20 else slowest
                    cell["same_bytes"] = bool(np.array_equal(device().cpu().numpy()[0], want))
                    cell["host_ms"], cell["host_calls"] = host_ms(host, calls, label), calls
                    d, o = cell["device_ms"], cell["host_ms"]
                    cell["device_faster"] = None if o["iqr"] is None else below(d, o)          # a one-sample host run gives no verdict
                res["cells"][label] = cell
                print(label, json.dumps(cell), file=sys.stderr, flush=True)
                write(json.dumps(res), args.out)          # a run that is cut short keeps the cells it finished
    emit(res, args.out)


if __name__ == "__main__":
    main()
