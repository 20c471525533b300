"""Dense optical flow on the device: OpenCV 4.x's contrib ``DualTVL1OpticalFlow`` (optflow module, CPU path), the reference's second
flow method (video/utils.py:75-86: ``cv2.optflow.DualTVL1OpticalFlow_create().calc(prev, next, None)``; its driver's choice, :416).

Every stage is a gfx950 kernel of csrc/tvl1.hip behind the C ABI (include/adain_hip.h, ``adain_tvl1_*``); the rules are restated
there and in tests/tvl1_ref.py.  A frame's preparation (float conversion, scale images, centred gradients) depends on the frame
only, and the flow call runs any number of pairs of one size together, each with its own stop rule: ``TVL1Sequence.batch`` prepares
each frame of a clip once and computes its n-1 flows in chunks, with the same bits as pair-by-pair ``calc``.  Re-exported by flow.py.
"""
import ctypes

import torch

from . import runtime as rt

DEFAULTS = dict(tau=0.25, lambda_=0.15, theta=0.3, nscales=5, warps=5, epsilon=0.01, innerIterations=30, outerIterations=10,
                scaleStep=0.8, gamma=0.0, medianFiltering=5, useInitialFlow=False)      # DualTVL1OpticalFlow_create()'s defaults


class Params(ctypes.Structure):
    """``adain_tvl1_params`` of include/adain_hip.h (``lambda`` is a Python keyword: ``lambda_``)."""
    _fields_ = [("tau", ctypes.c_double), ("lambda_", ctypes.c_double), ("theta", ctypes.c_double), ("nscales", ctypes.c_int),
                ("warps", ctypes.c_int), ("epsilon", ctypes.c_double), ("innerIterations", ctypes.c_int),
                ("outerIterations", ctypes.c_int), ("scaleStep", ctypes.c_double), ("gamma", ctypes.c_double),
                ("medianFiltering", ctypes.c_int), ("useInitialFlow", ctypes.c_int)]


def check_params(tau=0.25, lambda_=0.15, theta=0.3, nscales=5, warps=5, epsilon=0.01, innerIterations=30, outerIterations=10,
                 scaleStep=0.8, gamma=0.0, medianFiltering=5, useInitialFlow=False):
    """Refuses what the device estimator does not implement (the C ABI refuses the same), before anything is launched; returns the
    parameters as the C struct."""
    if float(gamma) != 0.0:
        raise ValueError(f"DualTVL1OpticalFlow: gamma != 0 is not supported, got {gamma}")
    if useInitialFlow:
        raise ValueError("DualTVL1OpticalFlow: useInitialFlow is not supported")
    if int(medianFiltering) > 1 and int(medianFiltering) not in (3, 5):
        raise ValueError(f"DualTVL1OpticalFlow: medianFiltering must be <= 1 (off), 3 or 5 (medianBlur on float data), got {medianFiltering}")
    if int(nscales) < 1:
        raise ValueError(f"DualTVL1OpticalFlow: nscales must be >= 1, got {nscales}")
    if min(int(warps), int(innerIterations), int(outerIterations)) < 0:
        raise ValueError("DualTVL1OpticalFlow: warps, innerIterations and outerIterations must be >= 0")
    if not 0.0 < float(scaleStep) <= 1.0:
        raise ValueError(f"DualTVL1OpticalFlow: scaleStep must be in (0, 1], got {scaleStep}")
    return Params(float(tau), float(lambda_), float(theta), int(nscales), int(warps), float(epsilon), int(innerIterations),
                  int(outerIterations), float(scaleStep), float(gamma), int(medianFiltering), int(bool(useInitialFlow)))


def _err(name):
    return ValueError(f"{name}: {rt.lib().adain_last_error().decode()}")


def scales(h, w, **params):
    """The scale list (host only, adain_tvl1_scales): [(width, height)] for s = 0 (full size) .. coarsest."""
    P = check_params(**params)
    n = ctypes.c_int()
    wh = (ctypes.c_int * (2 * max(P.nscales, 1)))()
    if rt.lib().adain_tvl1_scales(int(h), int(w), ctypes.addressof(P), ctypes.byref(n), wh) != 0:
        raise _err("adain_tvl1_scales")
    return [(wh[2 * s], wh[2 * s + 1]) for s in range(n.value)]


class TVL1:
    """One parameter set bound to a frame size: ``prepare(gray) -> prepared frame(s)``, ``flows(prev_list, next_list) -> [n,2,h,w]``."""

    def __init__(self, h, w, **params):
        self.params = dict(DEFAULTS, **params)
        self.P = check_params(**self.params)
        self.h, self.w = int(h), int(w)
        self.scales = scales(self.h, self.w, **self.params)
        self.frame_bytes = rt.lib().adain_tvl1_frame_bytes(self.h, self.w, ctypes.addressof(self.P))
        if self.frame_bytes == 0:
            raise _err("adain_tvl1_frame_bytes")
        self.frame_floats = self.frame_bytes // 4

    def workspace_bytes(self, npairs):
        return rt.lib().adain_tvl1_workspace_bytes(self.h, self.w, int(npairs), ctypes.addressof(self.P))

    def prepare(self, gray, out=None):
        """uint8 gray [h,w] -> float32 [frame_floats]; [n,h,w] -> [n, frame_floats]."""
        g = rt.device_tensor(gray, "gray", torch.uint8)
        single = g.dim() == 2
        if single:
            g = g.unsqueeze(0)
        if g.dim() != 3 or tuple(g.shape[1:]) != (self.h, self.w):
            raise rt.AdainHipError(f"tvl1: expected uint8 [{self.h},{self.w}] or [n,{self.h},{self.w}] frames, got {tuple(gray.shape)}")
        n = g.shape[0]
        if out is None:
            out = torch.empty((n, self.frame_floats), dtype=torch.float32, device=g.device)
        else:
            rt.check_buffer(out, "tvl1: out", torch.float32, g.device, numel=n * self.frame_floats, align=256)
        rt.call("adain_tvl1_prepare", g.device, g.data_ptr(), n, self.h, self.w, ctypes.addressof(self.P), out.data_ptr())
        return out.view(self.frame_floats) if single else out.view(n, self.frame_floats)

    def prepared_views(self, prep):
        """[(I, I_x, I_y)] per scale: views of one prepared frame (the layout of adain_tvl1_prepare)."""
        out, off = [], 0
        for (ws, hs) in self.scales:
            v = prep[off:off + 4 * ws * hs].view(hs, ws, 4)
            out.append((v[..., 0], v[..., 1], v[..., 2]))
            off += (4 * ws * hs + 63) // 64 * 64
        return out

    def flows(self, prev_list, next_list, out=None, iters_out=None):
        """The flows of pairs (prev_list[i] -> next_list[i], prepared frames) -> float32 [n,2,h,w]; ``iters_out`` (int32
        [n, nscales, warps]) receives the inner steps each (scale, warp) executed.  ``out`` and ``iters_out`` must be device tensors
        on the frames' device.  The host waits on the current stream after every outer pass but the last of each warp (the stop
        reads of adain_tvl1_flow); the last launches are still in flight when this returns."""
        n = len(prev_list)
        if n < 1 or len(next_list) != n:
            raise ValueError("tvl1: prev_list and next_list must be non-empty lists of one length")
        dev = prev_list[0].device
        for t in list(prev_list) + list(next_list):
            # prepare() writes each frame 256-byte aligned; the kernels read it as float4 at 256-byte aligned scale offsets
            rt.check_buffer(t, "tvl1: each of the prepared frames (made by prepare())", torch.float32, dev, min_numel=self.frame_floats,
                            align=256)
        if out is None:
            out = torch.empty((n, 2, self.h, self.w), dtype=torch.float32, device=dev)
        else:
            rt.check_buffer(out, "tvl1: out", torch.float32, dev, shape=(n, 2, self.h, self.w))
        if iters_out is not None:
            rt.check_buffer(iters_out, "tvl1: iters_out", torch.int32, dev, shape=(n, len(self.scales), self.P.warps))
        ptrs = torch.tensor([t.data_ptr() for t in prev_list] + [t.data_ptr() for t in next_list], dtype=torch.int64).to(dev)
        ws = rt.workspace(dev, "tvl1", self.workspace_bytes(n))
        rt.call("adain_tvl1_flow", dev, ptrs.data_ptr(), ptrs.data_ptr() + 8 * n, n, self.h, self.w, ctypes.addressof(self.P), out.data_ptr(),
                iters_out.data_ptr() if iters_out is not None else None, ws.data_ptr(), ws.numel())
        return out

    def default_max_pairs(self, budget=512 << 20):
        """The pairs per flow call of a clip: as many as a ``budget`` of workspace + prepared frames holds (1..64)."""
        per = self.workspace_bytes(2) - self.workspace_bytes(1) + self.frame_bytes
        return max(1, min(64, budget // max(per, 1)))


class DualTVL1OpticalFlow:
    """What ``cv2.optflow.DualTVL1OpticalFlow_create(...)`` returns, for device tensors: ``calc(I0, I1, None)`` with uint8 [H,W] device
    frames -> float32 [H,W,2] device tensor (a view of the planar [2,H,W] result, x then y)."""

    def __init__(self, **params):
        self.params = dict(DEFAULTS, **params)
        check_params(**self.params)
        self._tv = None

    def calc(self, I0, I1, flow=None):
        if flow is not None:
            raise ValueError("DualTVL1OpticalFlow.calc: only flow=None is supported (no initial flow)")
        if not isinstance(I0, torch.Tensor) or not isinstance(I1, torch.Tensor) or I0.shape != I1.shape or I0.dim() != 2:
            raise ValueError("DualTVL1OpticalFlow.calc: I0 and I1 must be uint8 [H,W] device tensors of one size")
        if self._tv is None or (self._tv.h, self._tv.w) != tuple(I0.shape):
            self._tv = TVL1(I0.shape[0], I0.shape[1], **self.params)
        tv = self._tv
        return tv.flows([tv.prepare(I0)], [tv.prepare(I1)])[0].permute(1, 2, 0)


def DualTVL1OpticalFlow_create(tau=0.25, lambda_=0.15, theta=0.3, nscales=5, warps=5, epsilon=0.01, innerIterations=30,
                               outerIterations=10, scaleStep=0.8, gamma=0.0, medianFiltering=5, useInitialFlow=False):
    """``cv2.optflow.DualTVL1OpticalFlow_create`` with its defaults (``lambda`` spelled ``lambda_``)."""
    return DualTVL1OpticalFlow(tau=tau, lambda_=lambda_, theta=theta, nscales=nscales, warps=warps, epsilon=epsilon,
                               innerIterations=innerIterations, outerIterations=outerIterations, scaleStep=scaleStep, gamma=gamma,
                               medianFiltering=medianFiltering, useInitialFlow=useInitialFlow)


class TVL1Sequence:
    """The TV-L1 flows of a clip, frame i-1 -> frame i, each frame prepared once: ``push(gray)`` returns None for the first frame and
    the [2,H,W] flow from the previous frame after that; ``flows(grays)`` yields them; ``batch(grays)`` writes [n-1,2,H,W] (the
    ``flows=`` of jobs.video_style_transfer_sharded), running up to ``max_pairs`` pairs per flow call.  Bit-identical to pair-by-pair
    ``DualTVL1OpticalFlow.calc``."""

    def __init__(self, **params):
        self.params = dict(DEFAULTS, **params)
        check_params(**self.params)
        self._tv = None
        self._prev = None

    def _bind(self, shape):
        if self._tv is None or (self._tv.h, self._tv.w) != tuple(shape):
            self._tv = TVL1(shape[0], shape[1], **self.params)
            self._prev = None
        return self._tv

    def reset(self):
        self._prev = None

    def push(self, gray, out=None):
        tv = self._bind(gray.shape)
        cur = tv.prepare(gray)
        flow = None
        if self._prev is not None:
            flow = tv.flows([self._prev], [cur], out=None if out is None else out.unsqueeze(0))[0]
        self._prev = cur
        return flow

    def flows(self, grays):
        self.reset()
        for g in grays:
            f = self.push(g)
            if f is not None:
                yield f

    def batch(self, grays, out=None, max_pairs=None, cancel=None):
        """[n-1,2,H,W] flows of n frames.  Frames live in a ring of max_pairs + 1 prepared slots; each chunk prepares its new frames
        and runs its pairs in one call.  ``cancel`` (an object with ``is_set()``) is checked between chunks: None is returned when set."""
        grays = list(grays)
        if len(grays) < 2:
            raise ValueError("TVL1Sequence.batch: need at least two frames")
        tv = self._bind(grays[0].shape)
        h, w = tv.h, tv.w
        n = len(grays)
        m = int(max_pairs) if max_pairs is not None else tv.default_max_pairs()
        m = max(1, min(m, n - 1))
        if out is None:
            out = torch.empty((n - 1, 2, h, w), dtype=torch.float32, device=grays[0].device)
        else:
            rt.check_buffer(out, "TVL1Sequence.batch: out", torch.float32, grays[0].device, shape=(n - 1, 2, h, w))
        ring = torch.empty((m + 1, tv.frame_floats), dtype=torch.float32, device=grays[0].device)

        def prepare(a, b):                  # frames a..b-1 into their slots, in contiguous runs of the ring
            while a < b:
                s = a % (m + 1)
                e = min(b, a + (m + 1 - s))
                tv.prepare(torch.stack([grays[j] for j in range(a, e)]), out=ring[s:s + e - a])
                a = e

        prepare(0, 1)
        for i in range(0, n - 1, m):
            if cancel is not None and cancel.is_set():
                return None
            k = min(m, n - 1 - i)
            prepare(i + 1, i + 1 + k)
            tv.flows([ring[j % (m + 1)] for j in range(i, i + k)], [ring[(j + 1) % (m + 1)] for j in range(i, i + k)], out=out[i:i + k])
        self._prev = None
        return out
