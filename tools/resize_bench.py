"""Times the six-filter device resize (csrc/resample_filters.hip, ``runtime.resize_pil_u8``) against ``PIL.Image.resize`` on one thread of
the same machine, for every filter at the callers' sizes: a 1080p frame to 455 x 256 (the video size), to 960 x 540, to 1080p // 8 and
1080p // 99 (the palette page), and a 256 x 456 frame up to 1080p.  Per cell (filter, size), median and interquartile range of --reps
calls (>= 200):
  kernels_ms    device frame -> device frame with the tap tables in the cache: HIP events around the call (its one or two launches)
  cold_ms       the same call with the table cache emptied first: the host builds both tables, they are uploaded, the launches run;
                wall clock around the call and a stream synchronize
  host_ms       ``Image.fromarray(frame).resize(size, filter)`` of the same frame, wall clock
  one_pass_ms   BILINEAR only: ``runtime.resize_pil_bilinear_u8`` (the one-pass kernel of csrc/resample.hip, its tables built on the device) at
                the same sizes, HIP events
``same_bytes``: the device frame is Pillow's.  ``device_faster`` / ``cold_device_faster``: the device median sits below the host's by more than
both interquartile ranges; ``host_faster``: the other way round; ``two_pass_faster`` / ``one_pass_faster`` likewise between the two BILINEAR
kernels.  Prints one JSON line and, with --out, writes it to a file after every cell.  --filters / --sizes narrow a run.
The timing loops, the statistic and the verdict's rule are tools/benchkit.py's.
Usage: python tools/resize_bench.py [--reps 200] [--out profiles/resize_bench.json]"""
import os

for _v in ("OMP_NUM_THREADS", "OPENBLAS_NUM_THREADS", "MKL_NUM_THREADS"):          # before NumPy loads: the host form runs on one thread
    os.environ[_v] = "1"

import json  # noqa: E402
import sys  # noqa: E402

import numpy as np  # noqa: E402
import PIL  # noqa: E402
import torch  # noqa: E402
from PIL import Image  # noqa: E402

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import applied_image_processing_amd.runtime as rt  # noqa: E402
import pil_resize_ref as R  # noqa: E402
from benchkit import arguments, below, emit, event_ms, gpu_setup, header, wall_ms, write  # noqa: E402

# name -> ((h, w) of the source, (width, height) asked for)
SIZES = {"1080p_to_455x256": ((1080, 1920), (455, 256)), "1080p_to_960x540": ((1080, 1920), (960, 540)), "1080p_div8": ((1080, 1920), (240, 135)),
         "1080p_div99": ((1080, 1920), (19, 10)), "256x456_to_1080p": ((256, 456), (1920, 1080))}


def main():
    ap = arguments(__doc__)
    ap.add_argument("--filters", default=",".join(R.FILTERS))
    ap.add_argument("--sizes", default=",".join(SIZES))
    args = ap.parse_args()
    dev = gpu_setup("resize_bench")
    reps = max(args.reps, 200)
    res = header(pillow=PIL.__version__, reps=reps, cells={})
    for size_name in args.sizes.split(","):
        hw, size = SIZES[size_name]
        frame = R.picture(1, *hw)
        image = Image.fromarray(frame)
        x = torch.from_numpy(frame[None]).to(dev)
        for name in args.filters.split(","):
            f = R.FILTERS[name]
            label = f"{name}_{size_name}"

            def cold():
                rt.free_pil_tables()
                rt.resize_pil_u8(x, size, f)
                torch.cuda.synchronize()

            want = np.asarray(image.resize(size, f))
            cell = {"same_bytes": bool(np.array_equal(rt.resize_pil_u8(x, size, f)[0].cpu().numpy(), want))}
            cell["kernels_ms"] = event_ms(lambda: rt.resize_pil_u8(x, size, f), reps, 5)
            cell["cold_ms"] = wall_ms(cold, reps, 3, "none")          # cold() ends with its own synchronise
            cell["host_ms"] = wall_ms(lambda: image.resize(size, f), reps, 3, "none")
            cell["device_faster"], cell["host_faster"] = below(cell["kernels_ms"], cell["host_ms"]), below(cell["host_ms"], cell["kernels_ms"])
            cell["cold_device_faster"] = below(cell["cold_ms"], cell["host_ms"])
            if f == R.BILINEAR:
                cell["one_pass_ms"] = event_ms(lambda: rt.resize_pil_bilinear_u8(x, size), reps, 5)
                cell["two_pass_faster"], cell["one_pass_faster"] = below(cell["kernels_ms"], cell["one_pass_ms"]), below(cell["one_pass_ms"], cell["kernels_ms"])
            res["cells"][label] = cell
            print(label, json.dumps(cell), file=sys.stderr, flush=True)
            write(json.dumps(res), args.out)          # a run that is cut short keeps the cells it finished
    emit(res, args.out)


if __name__ == "__main__":
    main()
