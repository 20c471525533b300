"""Times the device JPEG file decoder (csrc/jpeg_decode.hip, adain_jpeg_decode_u8) against the host route through Pillow on the same machine,
one file per call: files at 256 x 456 and 1080 x 1920, saved by Pillow at its default settings (quality 75, 4:2:0) and at quality 95,
of a stylised synthetic frame (seed-0 weights) and of uniform noise, each also with one restart interval per MCU row (Pillow's
``restart_marker_rows=1``, the ``_restart`` rows: adain_jpeg_decode_restart_u8) and as a progressive file (Pillow's ``progressive=True``:
adain_jpeg_decode_progressive_u8; those rows stand under a key of their own, ``progressive``, with the same fields and no chunk sweep).
Median and interquartile range over --reps calls (>= 200) after warm-up:
  kernel_ms  adain_jpeg_decode_u8 on bytes that are already on the device, HIP events
  device_ms  wall clock from ``bytes`` to a device frame with ``rt.jpeg_decode_u8``: marker walk, upload, decode, the record read
  host_ms    the route without it on one thread: ``Image.open`` + ``np.asarray`` + upload, synchronised
with the rounds the entropy decode took, whether the two give the same pixels, and ``device_is_faster``: device_ms sits below host_ms
by more than the two interquartile ranges combined.  ``chunk_bits``: kernel_ms of the 1080p files at 256, 512, 1024 and 2048 bits per
subsequence over --sweep-reps calls (the library's default is the best of them on the stylised frames; dense noise needs thousands of
rounds at the small sizes, which is why the sweep makes fewer calls).  Progress goes to stderr.  ``per_call``: ``adain_inference`` on a 256 x 456 JPEG content (style cached,
``bench.py --per-call video``'s call) with ``set_device_jpeg_decode`` off and on.  Every kernel_ms also carries the sha256 of its last call's output bytes, so that two builds of the library
(--lib PATH: that build in place of the package's own) can be held to the same bytes as well as the same time.  Prints one JSON line and, with --out,
writes it.
The timing loops, the statistic and the verdict's rule are tools/benchkit.py's.
Usage: python tools/jpeg_decode_bench.py [--reps 200] [--lib PATH] [--out profiles/jpeg_decode_bench.json]"""
import hashlib
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

import applied_image_processing_amd.jpeg_file as jpeg_file  # noqa: E402
import applied_image_processing_amd.runtime as rt  # noqa: E402
import applied_image_processing_amd.synth as synth  # noqa: E402
from applied_image_processing_amd.AdaIN import test as adain_test  # noqa: E402
from applied_image_processing_amd.engine import AdaINEngine  # noqa: E402
from applied_image_processing_amd.telemetry import GpuTelemetry  # noqa: E402
from benchkit import arguments, below, emit, event_times, gpu_setup, header, spread, wall_ms  # noqa: E402

SIZES = [(256, 456), (1080, 1920)]
CHUNKS = [256, 512, 1024, 2048]


def sha256(out):
    """Of a launch's (frames, record)."""
    return hashlib.sha256(b"".join(t.cpu().numpy().tobytes() for t in out)).hexdigest()


def hashed_event_ms(fn, reps, warmup):
    """The kit's event_ms with the sha256 of the last call's (frames, record) beside it."""
    times, out = event_times(fn, reps, warmup)
    return dict(spread(times), sha256=sha256(out))


def host_route(data, dev):
    """The parent's route for the same bytes: PIL decode on one thread, then the pixels go up."""
    return torch.from_numpy(np.asarray(Image.open(io.BytesIO(data))).copy()).to(dev)


def jpeg_bytes(frame, **kw):
    buf = io.BytesIO()
    Image.fromarray(frame).save(buf, format="JPEG", **kw)
    return buf.getvalue()


def per_call(reps, dev):
    """adain_inference(content path, cached style, content_size 256) with the switch off and on: wall clock per call."""
    out = {}
    with tempfile.TemporaryDirectory() as d:
        torch.save(synth.to_torch(synth.vgg_state_dict(0, full=True)), os.path.join(d, "vgg.pth"))
        torch.save(synth.to_torch(synth.decoder_state_dict(0)), os.path.join(d, "dec.pth"))
        content = os.path.join(d, "content.jpg")
        Image.fromarray((synth.image(7, 1, 256, 456)[0].transpose(1, 2, 0) * np.float32(255)).astype(np.uint8)).save(content)
        style = Image.fromarray((synth.image(4, 1, 512, 512)[0].transpose(1, 2, 0) * np.float32(255)).astype(np.uint8))
        call = lambda: adain_test.adain_inference(content, style, vgg_str=os.path.join(d, "vgg.pth"), decoder_str=os.path.join(d, "dec.pth"), content_size=256,
                                                  output=os.path.join(d, "out"), file_name="x")
        files = {}
        with open(os.devnull, "w") as null:
            stdout, sys.stdout = sys.stdout, null
            try:
                for on in (False, True):
                    adain_test.set_device_jpeg_decode(on)
                    out["on" if on else "off"] = wall_ms(call, reps, 10, "both")
                    files[on] = open(os.path.join(d, "out", "x.jpg"), "rb").read()
            finally:
                sys.stdout = stdout
                adain_test.set_device_jpeg_decode(False)
        out["same_file"] = files[True] == files[False]
    return out


def row(name, data, launch, restart_interval, kw, reps, dev, tel):
    """One file's row: kernel_ms of ``launch`` (bytes already on the device), device_ms of ``rt.jpeg_decode_u8(data, **kw)``, host_ms."""
    t0 = time.perf_counter()
    kernel = hashed_event_ms(launch, reps, 20)
    tel.window(f"kernel_{name}", t0, time.perf_counter())
    report = []
    same = bool(torch.equal(rt.jpeg_decode_u8(data, dev, report=report, **kw), host_route(data, dev)))
    device = wall_ms(lambda: rt.jpeg_decode_u8(data, dev, **kw), reps, 5, "both")          # both routes end on the device
    host = wall_ms(lambda: host_route(data, dev), reps, 3, "both")
    return {"file_bytes": len(data), "restart_interval": restart_interval, "path": report[0]["path"], "rounds": report[0]["rounds"], "same_pixels_as_host": same,
            "kernel_ms": kernel, "device_ms": device, "host_ms": host, "host_over_device": round(host["median"] / device["median"], 2),
            "device_is_faster": below(device, host)}


def main():
    ap = arguments(__doc__, lib=True)
    ap.add_argument("--sweep-reps", type=int, default=40)
    args = ap.parse_args()
    dev = gpu_setup("jpeg_decode_bench", args.lib)
    reps = max(args.reps, 200)
    engine = AdaINEngine(synth.to_torch(synth.vgg_state_dict(0, full=False)), synth.to_torch(synth.decoder_state_dict(0)), dev)
    engine.set_style(torch.from_numpy(synth.image(4, 1, 512, 512)).to(dev))
    tel = GpuTelemetry(0).start()
    res = header(reps=reps, pillow=PIL.__version__, sizes={}, chunk_bits={}, progressive={})
    for h, w in SIZES:
        source = torch.from_numpy((synth.image(7, 1, h, w)[0].transpose(1, 2, 0) * np.float32(255)).astype(np.uint8)[None]).to(dev)
        frames = {"stylised": engine.stylize_u8(source, alpha=0.5)[0].cpu().numpy(), "noise": np.random.default_rng(0).integers(0, 256, (h, w, 3), dtype=np.uint8)}
        for kind, frame in frames.items():
            for label, kw in (("default", {}), ("q95", {"quality": 95}), ("default_restart", {"restart_marker_rows": 1}),
                              ("q95_restart", {"quality": 95, "restart_marker_rows": 1})):
                data = jpeg_bytes(frame, **kw)
                parsed = jpeg_file.parse(data, restart=True)
                up, offsets, lengths = rt.jpeg_decode_upload([parsed], [data], dev)
                launch = lambda chunk_bits=0: rt.jpeg_decode_launch(up, offsets, lengths, parsed.geometry, chunk_bits, parsed.restart_interval)
                name = f"{kind}_{label}_{h}x{w}"
                res["sizes"][name] = row(name, data, launch, parsed.restart_interval, dict(restart=True), reps, dev, tel)
                if h == 1080:
                    res["chunk_bits"][name] = {}
                    for cb in CHUNKS:
                        rounds = int(launch(cb)[1][0, 1].item())
                        res["chunk_bits"][name][str(cb)] = dict(hashed_event_ms(lambda: launch(cb), max(args.sweep_reps, 8), 3), rounds=rounds, reps=max(args.sweep_reps, 8))
                print(f"{name}: {json.dumps(res['sizes'][name])} {json.dumps(res['chunk_bits'].get(name))}", file=sys.stderr, flush=True)
            for label, kw in (("default_progressive", {"progressive": True}), ("q95_progressive", {"quality": 95, "progressive": True})):
                data = jpeg_bytes(frame, **kw)
                prog = jpeg_file.parse(data, progressive=True)
                pup, poffsets, plengths = rt.jpeg_decode_progressive_upload([prog], [data], dev)
                name = f"{kind}_{label}_{h}x{w}"
                res["progressive"][name] = row(name, data, lambda: rt.jpeg_decode_progressive_launch(pup, poffsets, plengths, prog.geometry, prog.script), 0,
                                               dict(progressive=True), reps, dev, tel)
                res["progressive"][name]["scans"] = len(prog.scans)
                print(f"{name}: {json.dumps(res['progressive'][name])}", file=sys.stderr, flush=True)
    res["per_call"] = per_call(reps, dev)
    res["telemetry"] = tel.stop()          # shader clock and power over each kernel timing window (sysfs reads)
    emit(res, args.out)


if __name__ == "__main__":
    main()
