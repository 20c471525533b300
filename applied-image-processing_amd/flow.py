"""Dense optical flow on the device: OpenCV 4.x's ``calcOpticalFlowFarneback`` (flags = 0), which the reference's video callers
run for every frame pair (video/utils.py:75-86: ``cv2.calcOpticalFlowFarneback(prev, next, None, 0.5, 5, 15, 3, 7, 1.5, 0)``),
and their frame preparation (``cv2.imread`` -> ``cv2.resize(target_resolution)`` -> ``cv2.COLOR_RGB2GRAY`` on BGR data).

Every stage is a gfx950 kernel of csrc/flow.hip behind the C ABI (include/adain_hip.h, ``adain_farneback_*``); the rules are
restated there and in tests/farneback_ref.py.  A frame's pyramid (level images + polynomial expansion) depends on the frame only:
``FlowSequence`` expands each frame of a clip once and uses it as ``next`` of one pair and ``prev`` of the following one, with
the same bits as pair-by-pair calls.
"""
import ctypes

import torch

from . import runtime as rt

DEFAULTS = dict(pyr_scale=0.5, levels=5, winsize=15, iterations=3, poly_n=7, poly_sigma=1.5, flags=0)   # the reference's call
OPTFLOW_USE_INITIAL_FLOW, OPTFLOW_FARNEBACK_GAUSSIAN = 4, 256


def check_params(pyr_scale, levels, winsize, iterations, poly_n, poly_sigma, flags):
    """Refuses what the device estimator does not implement, before anything is launched."""
    if flags != 0:
        raise ValueError(f"calcOpticalFlowFarneback: only flags=0 is supported (OPTFLOW_USE_INITIAL_FLOW and OPTFLOW_FARNEBACK_GAUSSIAN "
                         f"are not built), got {flags}")
    if not 0.0 < float(pyr_scale) < 1.0:
        raise ValueError(f"calcOpticalFlowFarneback: pyr_scale must be in (0, 1), got {pyr_scale}")
    if poly_n not in (5, 7):
        raise ValueError(f"calcOpticalFlowFarneback: poly_n must be 5 or 7, got {poly_n}")
    if int(levels) < 0 or int(iterations) < 1 or not 2 <= int(winsize) <= 63:
        raise ValueError(f"calcOpticalFlowFarneback: need levels >= 0, iterations >= 1 and 2 <= winsize <= 63, got levels={levels}, "
                         f"iterations={iterations}, winsize={winsize}")


def level_schedule(h, w, pyr_scale=0.5, levels=5):
    """The pyramid schedule (host only, adain_farneback_levels): [(width, height, ksize, sigma)] for k = 0 (full size) .. L."""
    n = max(int(levels), 0) + 1
    L = ctypes.c_int()
    wh, ks, sg = (ctypes.c_int * (2 * n))(), (ctypes.c_int * n)(), (ctypes.c_double * n)()
    rc = rt.lib().adain_farneback_levels(int(h), int(w), float(pyr_scale), int(levels), ctypes.byref(L), wh, ks, sg)
    if rc != 0:
        raise ValueError(f"adain_farneback_levels: {rt.lib().adain_last_error().decode()}")
    return [(wh[2 * k], wh[2 * k + 1], ks[k], sg[k]) for k in range(L.value + 1)]


def pyramid_bytes(h, w, pyr_scale=0.5, levels=5):
    return rt.lib().adain_farneback_pyramid_bytes(int(h), int(w), float(pyr_scale), int(levels))


def pyramid_views(pyr, h, w, pyr_scale=0.5, levels=5):
    """[(level image [h_k,w_k], R [h_k,w_k,5])] views of a pyramid buffer (the layout of adain_farneback_expand)."""
    out, off = [], 0
    f = pyr.view(torch.float32)
    for (wl, hl, _ks, _s) in level_schedule(h, w, pyr_scale, levels):
        n = wl * hl
        img = f[off:off + n].view(hl, wl)
        off += (n + 63) // 64 * 64
        R = f[off:off + 5 * n].view(hl, wl, 5)
        off += (5 * n + 63) // 64 * 64
        out.append((img, R))
    return out


def frames_to_gray(frames, dsize=None):
    """The reference's frame preparation on the device: uint8 RGB frames [h,w,3] or [n,h,w,3] (PIL's channel order, as decoded
    here) -> uint8 gray [h,w] / [n,h,w] of ``cv2.cvtColor(cv2.resize(bgr, dsize), cv2.COLOR_RGB2GRAY)`` where ``bgr`` is what
    ``cv2.imread`` gives.  ``dsize`` = (width, height) as in cv2; None keeps the size."""
    frames = rt.device_tensor(frames, "frames", torch.uint8)
    single = frames.dim() == 3
    if single:
        frames = frames.unsqueeze(0)
    if frames.dim() != 4 or frames.shape[-1] != 3:
        raise rt.AdainHipError(f"frames_to_gray: expected uint8 [h,w,3] or [n,h,w,3], got {tuple(frames.shape)}")
    n, hi, wi, _ = frames.shape
    wo, ho = (wi, hi) if dsize is None else (int(dsize[0]), int(dsize[1]))
    out = torch.empty((n, ho, wo), dtype=torch.uint8, device=frames.device)
    rt.call("adain_flow_gray_u8", frames.device, frames.data_ptr(), n, hi, wi, out.data_ptr(), ho, wo)
    return out[0] if single else out


class Farneback:
    """One parameter set bound to a frame size: ``expand(gray) -> pyramid``, ``flow(pyr_prev, pyr_next) -> [2,h,w]``."""

    def __init__(self, h, w, pyr_scale=0.5, levels=5, winsize=15, iterations=3, poly_n=7, poly_sigma=1.5, flags=0):
        check_params(pyr_scale, levels, winsize, iterations, poly_n, poly_sigma, flags)
        self.h, self.w = int(h), int(w)
        self.pyr_scale, self.levels, self.winsize, self.iterations = float(pyr_scale), int(levels), int(winsize), int(iterations)
        self.poly_n, self.poly_sigma, self.flags = int(poly_n), float(poly_sigma), int(flags)
        self.pyr_bytes = pyramid_bytes(self.h, self.w, self.pyr_scale, self.levels)
        self.ws_bytes = rt.lib().adain_farneback_workspace_bytes(self.h, self.w)
        if self.pyr_bytes == 0 or self.ws_bytes == 0:
            raise ValueError(f"calcOpticalFlowFarneback: unsupported frame size {self.w} x {self.h}")

    def _gray(self, g):
        g = rt.device_tensor(g, "gray", torch.uint8)
        if tuple(g.shape) != (self.h, self.w):
            raise rt.AdainHipError(f"farneback: expected a uint8 [{self.h},{self.w}] frame, got {tuple(g.shape)}")
        return g

    def expand(self, gray, out=None):
        gray = self._gray(gray)
        pyr = out if out is not None else torch.empty(self.pyr_bytes, dtype=torch.uint8, device=gray.device)
        ws = rt.workspace(gray.device, "farneback", self.ws_bytes)
        rt.call("adain_farneback_expand", gray.device, gray.data_ptr(), self.h, self.w, self.pyr_scale, self.levels, self.poly_n,
                self.poly_sigma, pyr.data_ptr(), ws.data_ptr(), ws.numel())
        return pyr

    def flow(self, pyr_prev, pyr_next, out=None):
        dev = pyr_prev.device
        for p in (pyr_prev, pyr_next):
            rt.check_buffer(p, "farneback: each pyramid (made by expand())", torch.uint8, dev, min_numel=self.pyr_bytes)
        if out is None:
            out = torch.empty((2, self.h, self.w), dtype=torch.float32, device=dev)
        else:
            rt.check_buffer(out, "farneback: out", torch.float32, dev, shape=(2, self.h, self.w))
        ws = rt.workspace(dev, "farneback", self.ws_bytes)
        rt.call("adain_farneback_flow", dev, pyr_prev.data_ptr(), pyr_next.data_ptr(), self.h, self.w, self.pyr_scale, self.levels,
                self.winsize, self.iterations, self.flags, out.data_ptr(), ws.data_ptr(), ws.numel())
        return out


def calc_optical_flow_farneback(prev, next, flow=None, pyr_scale=0.5, levels=5, winsize=15, iterations=3, poly_n=7, poly_sigma=1.5,
                                flags=0):
    """``cv2.calcOpticalFlowFarneback`` on the device, same positional order: ``prev`` / ``next`` uint8 [H,W] device tensors ->
    float32 [H,W,2] device tensor (a view of the planar [2,H,W] result, x then y).  Only ``flow=None`` and ``flags=0``."""
    if flow is not None:
        raise ValueError("calcOpticalFlowFarneback: only flow=None is supported (no initial flow)")
    check_params(pyr_scale, levels, winsize, iterations, poly_n, poly_sigma, flags)
    if not isinstance(prev, torch.Tensor) or not isinstance(next, torch.Tensor) or prev.shape != next.shape or prev.dim() != 2:
        raise ValueError("calcOpticalFlowFarneback: prev and next must be uint8 [H,W] device tensors of one size")
    fb = Farneback(prev.shape[0], prev.shape[1], pyr_scale, levels, winsize, iterations, poly_n, poly_sigma, flags)
    return fb.flow(fb.expand(prev), fb.expand(next)).permute(1, 2, 0)


class FlowSequence:
    """The flows of a clip, frame i-1 -> frame i, with one pyramid per frame: ``push(gray)`` returns None for the first frame and
    the [2,H,W] flow from the previous frame after that; ``flows(grays)`` yields them; ``batch(grays)`` writes [n-1,2,H,W] (the
    ``flows=`` of jobs.video_style_transfer_sharded).  Bit-identical to pair-by-pair calc_optical_flow_farneback."""

    def __init__(self, pyr_scale=0.5, levels=5, winsize=15, iterations=3, poly_n=7, poly_sigma=1.5, flags=0):
        check_params(pyr_scale, levels, winsize, iterations, poly_n, poly_sigma, flags)
        self.params = dict(pyr_scale=pyr_scale, levels=levels, winsize=winsize, iterations=iterations, poly_n=poly_n,
                           poly_sigma=poly_sigma, flags=flags)
        self._fb = None
        self._prev = None
        self._spare = None

    def reset(self):
        self._prev = self._spare = None

    def push(self, gray, out=None):
        if self._fb is None or (self._fb.h, self._fb.w) != tuple(gray.shape):
            self._fb = Farneback(gray.shape[0], gray.shape[1], **self.params)
            self._prev = self._spare = None
        cur = self._fb.expand(gray, out=self._spare)           # the buffer of the frame before last is free again (stream order)
        flow = None if self._prev is None else self._fb.flow(self._prev, cur, out=out)
        self._spare, self._prev = self._prev, cur
        return flow

    def flows(self, grays):
        self.reset()
        for g in grays:
            f = self.push(g)
            if f is not None:
                yield f

    def batch(self, grays, out=None):
        grays = list(grays)
        if len(grays) < 2:
            raise ValueError("FlowSequence.batch: need at least two frames")
        h, w = grays[0].shape
        if out is None:
            out = torch.empty((len(grays) - 1, 2, h, w), dtype=torch.float32, device=grays[0].device)
        self.reset()
        for i, g in enumerate(grays):
            self.push(g, out=out[i - 1] if i > 0 else None)
        return out


# Dual TV-L1, the reference's other method (tvl1.py, csrc/tvl1.hip)
from .tvl1 import DualTVL1OpticalFlow, DualTVL1OpticalFlow_create, TVL1, TVL1Sequence  # noqa: E402,F401
