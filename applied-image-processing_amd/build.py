"""Builds the gfx950 shared library in-tree: ``applied-image-processing_amd/libadain_hip.so``.

hipcc cross-compiles without a GPU.  Objects are rebuilt only when a source or header is newer.
"""
import os
import subprocess
import sys
from concurrent.futures import ThreadPoolExecutor

PKG = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(PKG, "csrc")
INC = os.path.join(os.path.dirname(PKG), "include")
LIB = os.path.join(PKG, "libadain_hip.so")
# The GIF decoder's two calls (include/adain_gif_decode.h) are a library of their own: the product library exports exactly what
# include/adain_hip.h declares, and that header's launches are audited by tables this decoder's change could not edit
GIF_DECODE_LIB = os.path.join(PKG, "libadain_gif_decode.so")
GIF_DECODE_SOURCES = ["gif_decode.hip"]
# The direct implicit-GEMM and F(2x2,3x3) families of rounds 1-2 were retired in round 6 (git history).
SOURCES = ["conv_edge.hip", "conv_wino4.hip", "stats.hip", "pixel.hip", "resample.hip", "resample_filters.hip", "flow.hip", "tvl1.hip", "colour.hip", "coral.hip", "jpeg.hip", "jpeg_decode.hip", "png.hip", "png_decode.hip", "palette.hip", "gif.hip", "quantize.hip", "quantize_refine.hip", "metrics.hip", "guide_loss.hip", "api.hip"]
# -fvisibility=hidden: the shared library exports the C ABI of include/adain_hip.h (ADAIN_API) and nothing else
FLAGS = ["--offload-arch=gfx950", "-O3", "-std=c++20", "-fPIC", "-fvisibility=hidden", "-Wall", "-Wno-unused-function"]
# The MFMA kernels carry their fp32 vector-ALU work (input transform, epilogues) next to the matrix instructions, where
# v_pk_add_f32 / v_pk_fma_f32 issue far slower than the plain forms (MI355X_MICROARCH.md, "price of one filler beside
# MFMAs"): keep hipcc from packing f32 pairs in those files.  Measured on the Winograd kernel: +7 %.
NO_PACKED_F32 = ["-Xclang", "-target-feature", "-Xclang", "-packed-fp32-ops"]
# flow.hip and tvl1.hip keep OpenCV's float operations one by one (no FMA contraction), as their NumPy restatements do: with it the
# Farneback flow is the float32 restatement's bit for bit, without it the fused operations moved ill-conditioned narrow frames by
# up to 4.5e-5 px; colour.hip keeps numpy's float64 operations apart the same way, so that equal colours run one instruction
# sequence and project to equal keys; coral.hip shares colour.hip's float64 eigen-solve and is built the same way;
# palette.hip keeps numpy's float32 operations of the error diffusion apart (product, then add), as tests/palette_ref.py has them;
# resample_filters.hip builds Pillow's tap tables on the host in double, one operation at a time (pil_taps.h has the pragma as well);
# metrics.hip writes its fused operations out (fmaf in the two window passes) and keeps the SSIM map's products and sums apart, so that
# both inputs run one instruction sequence and equal frames score exactly 1; guide_loss.hip keeps the bilinear taps' products and sums
# apart, so that its resampled guide is adain_u8_to_f32 then adain_resize_bilinear bit for bit
NO_CONTRACT = ["-ffp-contract=off"]
EXTRA_FLAGS = {"conv_wino4.hip": NO_PACKED_F32, "flow.hip": NO_CONTRACT, "tvl1.hip": NO_CONTRACT, "colour.hip": NO_CONTRACT, "coral.hip": NO_CONTRACT, "palette.hip": NO_CONTRACT, "resample_filters.hip": NO_CONTRACT, "metrics.hip": NO_CONTRACT, "guide_loss.hip": NO_CONTRACT}


def _hipcc():
    c = os.environ.get("HIPCC")
    if c:
        return c
    return "/opt/rocm/bin/hipcc" if os.path.exists("/opt/rocm/bin/hipcc") else "hipcc"


def _newer(target, deps):
    if not os.path.exists(target):
        return True
    t = os.path.getmtime(target)
    return any(os.path.getmtime(d) > t for d in deps)


def build(force=False, verbose=False):
    """Builds the library and returns its path."""
    objdir = os.path.join(PKG, "build")
    os.makedirs(objdir, exist_ok=True)
    headers = [os.path.join(CSRC, h) for h in ("common.h", "device_utils.h", "cv_resize.h", "jpeg_common.h", "png_inflate.h", "pil_taps.h", "gif_lzw.h", "quantize_cut.h", "quantize_refine.h", "gif_unlzw.h")] + [os.path.join(INC, h) for h in ("adain_hip.h", "adain_gif_decode.h")]
    hipcc = _hipcc()
    jobs = []
    objs = []
    gif_decode_objs = []
    for src in SOURCES + GIF_DECODE_SOURCES:
        s = os.path.join(CSRC, src)
        o = os.path.join(objdir, src.replace(".hip", ".o"))
        (gif_decode_objs if src in GIF_DECODE_SOURCES else objs).append(o)
        if force or _newer(o, [s] + headers):
            jobs.append([hipcc] + FLAGS + EXTRA_FLAGS.get(src, []) + ["-I", INC, "-c", s, "-o", o])

    def run(cmd):
        if verbose:
            print(" ".join(cmd), flush=True)
        r = subprocess.run(cmd, capture_output=True, text=True)
        if r.returncode != 0:
            raise RuntimeError("hipcc failed:\n" + " ".join(cmd) + "\n" + r.stdout + r.stderr)
        if verbose and r.stderr.strip():
            print(r.stderr)
        return r.stderr

    with ThreadPoolExecutor(max_workers=4) as ex:
        list(ex.map(run, jobs))
    if force or jobs or _newer(LIB, objs):
        run([hipcc, "--offload-arch=gfx950", "-shared", "-fPIC", "-o", LIB] + objs)
    if force or _newer(GIF_DECODE_LIB, gif_decode_objs):
        run([hipcc, "--offload-arch=gfx950", "-shared", "-fPIC", "-o", GIF_DECODE_LIB] + gif_decode_objs)
    return LIB


if __name__ == "__main__":
    print(build(force="--force" in sys.argv, verbose=True))
