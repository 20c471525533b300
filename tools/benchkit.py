"""The timing kit of the per-feature benchmarks (tools/*_bench.py): the loops, the statistic, the verdict, the record's header and its
tail, once.  The rules every ``profiles/*_bench.json`` figure follows:
  event_times   HIP events around each call: ``warmup`` calls, one synchronise, then per call a fresh event pair
  wall_times    the host clock around each call; ``sync`` says where the device is waited for: "none" (host work: torch.cuda is never
                touched), "before" (before the clock starts: fn itself ends on the host) or "both" (and again before it stops: fn
                leaves work on the device)
  event_mean_ms one event pair around ``reps`` calls after one warm-up call: the mean
  spread        median and interquartile range (exclusive quartiles), rounded
  below         a's median sits below b's by more than both interquartile ranges
Plain functions; a tool with a loop or a record shape of its own formats the raw times these return."""
import argparse
import json
import os
import statistics
import time

import torch

SYNC = ("none", "before", "both")


def event_times(fn, reps, warmup):
    """(times in ms, the last call's result)."""
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    times, r = [], None
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        r = fn()
        b.record()
        b.synchronize()
        times.append(a.elapsed_time(b))
    return times, r


def wall_times(fn, reps, warmup, sync):
    """(times in ms, the last call's result)."""
    if sync not in SYNC:
        raise ValueError(f"sync is one of {SYNC}, not {sync!r}")
    for _ in range(warmup):
        fn()
    times, r = [], None
    for _ in range(reps):
        if sync != "none":
            torch.cuda.synchronize()
        t = time.perf_counter()
        r = fn()
        if sync == "both":
            torch.cuda.synchronize()
        times.append((time.perf_counter() - t) * 1e3)
    return times, r


def event_mean_ms(fn, reps):
    fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / reps


def spread(times, digits=4):
    if len(times) < 2:
        return {"median": round(times[0], digits), "iqr": None}
    q = statistics.quantiles(times, n=4)
    return {"median": round(statistics.median(times), digits), "iqr": round(q[2] - q[0], digits)}


def event_ms(fn, reps, warmup):
    return spread(event_times(fn, reps, warmup)[0])


def wall_ms(fn, reps, warmup, sync):
    return spread(wall_times(fn, reps, warmup, sync)[0])


def below(a, b):
    return bool(a["median"] + a["iqr"] + b["iqr"] < b["median"])


def gpu_setup(name, lib=None):
    """Device 0, one host thread.  ``lib``: a --lib PATH, that build of the library in place of the package's own."""
    if lib:
        import applied_image_processing_amd.runtime as rt

        rt.use_library(os.path.abspath(lib))
    assert torch.cuda.is_available(), f"{name} needs a GPU"
    torch.cuda.set_device(0)
    torch.set_num_threads(1)
    return torch.device("cuda:0")


def header(**extra):
    import applied_image_processing_amd.runtime as rt

    return {"device": torch.cuda.get_device_name(0) if torch.cuda.is_available() else None, "cpus_usable": len(os.sched_getaffinity(0)),
            "cpus_machine": os.cpu_count(), "lib": os.path.relpath(rt.LIB_PATH), **extra}


def arguments(doc, lib=False):
    ap = argparse.ArgumentParser(description=doc.replace("%", "%%"), formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--out", type=str, default=None)
    if lib:
        ap.add_argument("--lib", type=str, default=None)
    return ap


def write(line, out):
    if out:
        with open(out, "w") as f:
            f.write(line + "\n")


def emit(res, out):
    """Prints the record as one JSON line and, with ``out``, writes that line to the file."""
    line = json.dumps(res)
    print(line)
    write(line, out)
