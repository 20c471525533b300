"""Sharded job drivers: the reference's two batch callers of the AdaIN path, cut across the GPUs of one node.

* ``video_style_transfer_sharded`` — reference video/utils.py:297-369 (``apply_style_transfer_multi_ada`` / ``_ada``): one
  ``adain_inference`` per frame (each reloads the weights and re-encodes the style), INTER_AREA resize to the target
  resolution, then the flow-warp / blend recurrence over the frames and one file per frame.
* ``precompute_guides_sharded`` — reference Style_3DGS/train.py:86-115: one ``adain_inference`` per training camera with
  the mask ``gt_image_np > 0`` and ``<model_path>/stylized/<image_name>.jpg`` as output.

Both sit on ``stylize_frames_sharded``: the frame index is cut into contiguous blocks (``sharding.shard_range``), every
rank (one process per GPU) runs the batched engine on its block against replicated weights and style statistics, and the
finished uint8 frames meet on ``dst`` in ONE gather (RCCL over xGMI when the process group's CUDA backend is ``nccl``).
There is no other collective on the data path, and nothing inside the frame loop synchronises the device or talks to another
rank: one one-word status all_reduce per job (``sharding.agree_geometry``: every rank learns whether all blocks finished and
what a finished frame looks like) precedes the gather, one device synchronisation ends the job.  What is sequential in the
reference stays on ``dst`` after the gather: the frame-to-frame warp / blend recurrence and (by default) the file writes.

Host side of a job (the reference goes file -> PIL -> tensor -> device per frame, test.py:190-204): ``FrameFeeder`` decodes /
fetches the frames of the next sub-batches on a worker thread, stages them in pinned buffers and uploads them on a copy stream
while the compute stream works on the current sub-batch.  Decoded frames travel as uint8 HWC (3 bytes per pixel; ToTensor runs
on the device, bit-identical to the host's ``/ 255``); ``FileSink`` brings finished uint8 frames back with asynchronous copies
and writes the image files on worker threads.

The engine is passed in (``engine.AdaINEngine`` on a GPU); the drivers only use its methods, so the multi-process logic is
exercised on CPU under ``gloo`` with a stand-in engine (tests/test_distributed_gloo.py).
"""
import queue
import threading
import time
from concurrent.futures import ThreadPoolExecutor
from pathlib import Path

import numpy as np
import torch
import torch.distributed as dist

from . import sharding as sh
from .runtime import JpegOptions, JpegRoutes, OutputRoutes, PngRoute


def style_schedule(n_frames, n_styles):
    """Style index per frame as the reference switches styles through a video (video/utils.py:311-337):
    ``frames_per_style = max(1, n_frames // n_styles)``; the index advances at every frame i > 0 with
    ``i % frames_per_style == 0`` and stops at the last style."""
    if n_styles < 1:
        raise ValueError("No style images found in the style directory.")      # video/utils.py:308
    per = max(1, n_frames // n_styles)
    out, idx = [], 0
    for i in range(n_frames):
        if i > 0 and i % per == 0:
            idx = min(idx + 1, n_styles - 1)
        out.append(idx)
    return out


def style_crossfade(n_frames, n_styles, fade):
    """Style-mix weights per frame, float32 [n_frames][n_styles], for a clip that cross-fades where ``style_schedule`` cuts: at every
    switch point s (the frame whose index advances from style a to a + 1) the ``fade`` frames s - fade // 2 .. s - fade // 2 + fade - 1
    ramp linearly, frame f of them (j = f - (s - fade // 2)) taking (j + 1) / (fade + 1) of style a + 1 and the rest of style a.
    The ramp is computed in double and rounded once; the two weights of a ramp frame are t and 1 - t rounded, every other frame is
    one-hot: rows sum to 1 (within one rounding).  ``fade=0``: one-hot rows at ``style_schedule``'s indices.  Ramps of neighbouring
    switch points must not overlap (``fade`` at most the frames per style), and a ramp is clipped at the ends of the clip."""
    idx = style_schedule(n_frames, n_styles)
    fade = int(fade)
    if fade < 0:
        raise ValueError("style_crossfade: fade must be >= 0")
    if fade > max(1, n_frames // n_styles):
        raise ValueError(f"style_crossfade: fade {fade} is longer than the {max(1, n_frames // n_styles)} frames a style is shown for")
    rows = np.zeros((n_frames, n_styles), dtype=np.float64)
    rows[np.arange(n_frames), idx] = 1.0
    for s in range(1, n_frames):
        if idx[s] == idx[s - 1]:
            continue
        a, first = idx[s - 1], s - fade // 2
        for j in range(fade):
            f = first + j
            if 0 <= f < n_frames:
                t = (j + 1) / (fade + 1)
                rows[f] = 0.0
                rows[f, a], rows[f, a + 1] = 1.0 - t, t
    return rows.astype(np.float32)


host_barrier = sh.host_barrier


# ---------------------------------------------------------------------------------------------------------------------------------
# frames on their way to the device
# ---------------------------------------------------------------------------------------------------------------------------------
def as_frame(x):
    """One frame in the form the drivers move it, and its kind: ``"u8"`` = a decoded frame uint8 [h,w,3] (an RGB PIL image,
    a numpy array or a tensor: what the reference holds BEFORE ToTensor, test.py:190-200; ToTensor then runs on the device) or
    ``"f32"`` = an already transformed float tensor [3,h,w] in [0,1] (a fourth channel is dropped)."""
    if not isinstance(x, (torch.Tensor, np.ndarray)):          # a PIL image
        if getattr(x, "mode", None) == "RGB":
            x = np.array(x)                                   # (a writable copy: np.asarray of a PIL image is read-only)
        else:
            from .AdaIN.test import _to_tensor

            x = _to_tensor(x)
    if isinstance(x, np.ndarray):
        x = np.ascontiguousarray(x)
        x = torch.from_numpy(x if x.flags.writeable else x.copy())
    if x.dtype == torch.uint8:
        if x.dim() != 3 or x.shape[2] != 3:
            raise ValueError(f"a uint8 frame must be [h,w,3], got {tuple(x.shape)}")
        return x, "u8"
    if x.dim() != 3 or x.shape[0] not in (3, 4):
        raise ValueError(f"a float frame must be [3,h,w] (or [4,h,w]), got {tuple(x.shape)}")
    return x[:3].to(torch.float32), "f32"


# sub_batch=None: frames per sub-batch chosen from the frame size, about three megapixels of content per sub-batch.  Measured on
# device-resident frames (tools/probes/small_frame_probe.py, frames/s at sub-batches of 1 / 2 / 4 / 8 / 16 / 32): 256 x 456 - the
# reference's own video shape, content_size = 256 - 1587 / 2164 / 2431 / 2570 / 2590 / 2579; 512 x 912: 611 / 646 / 670 / 671 / 659 /
# 651; 1080p: 154 / 153 / 151 / 148 / 146 / 145.  Small frames need company to fill the chip (a 256 x 456 frame is 960 tile items
# for 512 resident workgroups); large ones lose to the L2-miss traffic that grows faster than the batch.
AUTO_SUB_BATCH_PIXELS = 3.0e6
MAX_AUTO_SUB_BATCH = 32
# Frames of 1.5 - 3 megapixels (1080p, 1200 x 1600, 1408 x 1408): since round 4 the C schedules run the big layers of a batch of WIDE
# frames frame by frame and only its relu4-level layers over the whole batch (csrc/api.hip, BIG_FRAME_WIDTH / BIG_LAYER_ROUNDS), so a
# sub-batch no longer costs the mid-network layers anything and fills the last round of conv4_1 / dec1: per step 331.1 / 331.8 / 334.9
# Mpixels/s at 1 / 2 / 4 frames of 1080p, 324.1 / 326.1 / 328.2 at 1200 x 1600 (same box); narrower frames of that size always gained
# from a batch (1280 x 1280: 335.5 / 337.5 at 2 / 4).  Larger frames have no layer left that a batch would help.
LARGE_FRAME_PIXELS = (1.5e6, 3.0e6)
LARGE_FRAME_SUB_BATCH = 4
AUTO_FETCH_SUB_BATCH = 8           # the sub-batch the feeder's fetch window assumes while sub-batches are cut by frame size (sub_batch=None)
MAX_QUEUED_BATCHES = 6             # sub-batches enqueued ahead of the device (stylize_frames_sharded)


def auto_sub_batch(h, w):
    if LARGE_FRAME_PIXELS[0] <= h * w < LARGE_FRAME_PIXELS[1]:
        return LARGE_FRAME_SUB_BATCH
    return int(max(1, min(MAX_AUTO_SUB_BATCH, round(AUTO_SUB_BATCH_PIXELS / max(1, h * w)))))


def sleep_wait(event, period=2e-4):
    """Host wait for a HIP event that SLEEPS.  ``event.synchronize()`` - and ``torch.cuda.synchronize`` - spin a core for as long as
    the GPU is busy on this ROCm build, also for events created with ``blocking=True`` (measured: tools/probes/thread_cpu_probe.py:
    the waiting thread's CPU time equals the wall time); with eight ranks on one host that is eight cores doing nothing.  Polling
    ``query()`` with a short sleep costs nothing and at most ``period`` of latency, which none of the waits below is sensitive to."""
    while not event.query():
        time.sleep(period)


def _event(device, stream=None):
    """A HIP event recorded now on ``stream`` (default: the current stream of ``device``)."""
    e = torch.cuda.Event()
    e.record(stream if stream is not None else torch.cuda.current_stream(device))
    return e


class _Batch:
    __slots__ = ("i", "j", "content", "depth", "mask", "ready", "slot")

    def __init__(self, i, j, content, depth=None, mask=None, ready=None, slot=None):
        self.i, self.j, self.content, self.depth, self.mask, self.ready, self.slot = i, j, content, depth, mask, ready, slot


class FrameFeeder:
    """Feeds ``frames[lo:hi]`` to the compute loop as sub-batches that are already on the device.

    A feeder thread cuts sub-batches (at most ``sub_batch`` frames of one style, one size and one kind), copies them into a
    pinned staging slot and uploads the slot on a dedicated copy stream; the per-frame proximity maps and masks of the sub-batch
    ride along.  The frames themselves are fetched (``frames[k]`` may decode a file: it must be safe to call for different k
    from several threads) and copied into the pinned slot by a small pool of ``workers`` threads, a window of frames ahead of
    the cutter: PIL's decoders and numpy's memcpy release the interpreter lock, and ONE thread copying pageable frames into
    pinned memory was measured at 0.7-1.1 GB/s on the GPU box - a 1080p job needs 1 GB/s.  ``depth`` slots are in flight: the
    upload of sub-batch k+1 (and the decode of k+2 ...) overlaps the kernels of sub-batch k.  The consumer waits on the
    sub-batch's HIP event on ITS stream (no host synchronisation) and calls ``release`` once its last kernel reading the slot
    is enqueued.

    ``frames`` may offer ``block(i, j)`` -> a ready [j-i, ...] tensor of frames i..j-1 of one size (device-resident frame
    stores hand out views: no staging, no copy).  On a CPU engine (tests) the same thread and cutting logic run without
    pinned memory or streams."""

    def __init__(self, frames, lo, hi, style_of, sub_batch, device, depth_maps=None, masks=None, depth=4, cuts=(), workers=4):
        self.frames, self.lo, self.hi, self.style_of = frames, lo, hi, style_of
        self.auto = sub_batch is None          # frames per sub-batch from the frame size (auto_sub_batch), per run of equal-sized frames
        self.sub_batch = MAX_AUTO_SUB_BATCH if self.auto else max(1, int(sub_batch))
        self.cuts = set(cuts)              # frame indices at which a sub-batch must end (chunk borders of a chunked gather)
        self.device = torch.device(device)
        self.depth_maps, self.masks = depth_maps, masks
        self.cuda = self.device.type == "cuda"
        self.nslots = max(2, int(depth))
        self.q = queue.Queue()
        self.free = threading.Semaphore(self.nslots)
        self.stop = threading.Event()
        self.h2d_bytes = 0
        self.fetch_s = 0.0
        # where the worker thread's time goes (seconds): waiting for a free slot (= the consumer is the bottleneck, as it should
        # be), waiting for a slot's previous upload to leave its pinned buffer, copying frames into pinned memory
        self.stats = {"wait_slot_s": 0.0, "wait_h2d_s": 0.0, "stage_s": 0.0, "batches": 0}
        if self.cuda:
            self.copy_stream = torch.cuda.Stream(self.device)
            self.compute_stream = torch.cuda.current_stream(self.device)
            self.pinned, self.dev = {}, {}         # (slot, "content" | "mask" | "depth") -> staging buffers
            self.h2d_done = [None] * self.nslots
            self.consumed = [None] * self.nslots
        self.pool = ThreadPoolExecutor(max_workers=max(1, int(workers)), thread_name_prefix="adain-frame-fetch")
        self.window = max(2 * (AUTO_FETCH_SUB_BATCH if self.auto else self.sub_batch), 2 * max(1, int(workers)))      # frames fetched ahead of the cutter
        self.thread = threading.Thread(target=self._run, name="adain-frame-feeder", daemon=True)
        self.thread.start()

    # ---- worker thread ----------------------------------------------------------------------------------------------------------
    def _cut(self):
        """Yields (i, j, frames-or-block) for consecutive sub-batches of [lo, hi)."""
        k, carry = self.lo, None
        block = getattr(self.frames, "block", None)
        ahead, nxt = [], self.lo               # futures of frames nxt - len(ahead) .. nxt - 1, fetched by the pool in index order

        def fetch(idx):
            return as_frame(self.frames[idx])[0]

        def get(idx):
            nonlocal nxt
            while nxt < self.hi and len(ahead) < self.window and not self.stop.is_set():
                ahead.append(self.pool.submit(fetch, nxt))
                nxt += 1
            return ahead.pop(0).result()

        def size_of(t):                        # decoded frames are uint8 [.., h, w, 3], transformed ones float [.., 3, h, w]
            return (t.shape[-3], t.shape[-2]) if t.dtype == torch.uint8 else (t.shape[-2], t.shape[-1])

        while k < self.hi:
            i = k
            if block is not None:
                limit = self.sub_batch
                if self.auto:
                    limit = auto_sub_batch(*size_of(block(i, i + 1)))
                j = i + 1
                while j < self.hi and j - i < limit and self.style_of[j] == self.style_of[i] and j not in self.cuts:
                    j += 1
                yield i, j, block(i, j)
                k = j
                continue
            items = []
            limit = self.sub_batch
            while k < self.hi and len(items) < limit and self.style_of[k] == self.style_of[i] and not (items and k in self.cuts):
                fr = carry if carry is not None else get(k)
                carry = None
                if not items and self.auto:
                    limit = auto_sub_batch(*size_of(fr))
                if items and (fr.dtype != items[0].dtype or fr.shape != items[0].shape or fr.device != items[0].device):
                    carry = fr                # another size / kind: it opens the next sub-batch
                    break
                items.append(fr)
                k += 1
            yield i, k, items

    def _upload(self, host):
        """A one-off upload (shapes that do not fit the slot buffers): pinned copy + asynchronous H2D on the copy stream."""
        t = host if host.is_pinned() else host.pin_memory()
        d = t.to(self.device, non_blocking=True)
        d.record_stream(self.compute_stream)             # allocated under the copy stream, read by the compute stream
        self.h2d_bytes += host.numel() * host.element_size()
        return d

    def _stage(self, s, name, items):
        """Host tensors ``items`` (one shape, one dtype) -> the slot's pinned buffer ``name`` (one memcpy each, no intermediate
        stack) -> the slot's device buffer, asynchronously on the copy stream (the caller holds the stream context and has made
        the stream wait for the slot's previous consumers).  Returns the device view [len(items), ...]."""
        nb = len(items)
        # slot capacity: the fixed sub-batch size, or - automatic sub-batches - this batch's own length (constant over a run of
        # equal-sized frames; the buffers are re-made when a longer batch or another frame size comes)
        shape = (nb if self.auto else self.sub_batch,) + tuple(items[0].shape)
        key = (s, name)
        pin = self.pinned.get(key)
        if pin is None or tuple(pin.shape[1:]) != shape[1:] or pin.shape[0] < nb or pin.dtype != items[0].dtype:
            pin = self.pinned[key] = torch.empty(shape, dtype=items[0].dtype, pin_memory=True)
            self.dev[key] = torch.empty(shape, dtype=items[0].dtype, device=self.device)
        pin_np = pin.numpy()

        def put(q_, it):
            np.copyto(pin_np[q_], it.numpy())              # a plain memcpy outside the interpreter lock

        if nb > 1:
            list(self.pool.map(put, range(nb), items))
        else:
            put(0, items[0])
        self.dev[key][:nb].copy_(pin[:nb], non_blocking=True)
        self.h2d_bytes += nb * items[0].numel() * items[0].element_size()
        return self.dev[key][:nb]

    def _extras(self, i, j):
        """The sub-batch's proximity maps (float32 [h0,w0] each) and masks ([1|3,hm,wm] each; bool / uint8 / float) as host or
        device tensors, still one per frame."""
        depth = mask = None
        if self.depth_maps is not None:
            depth = [torch.as_tensor(self.depth_maps[k], dtype=torch.float32) for k in range(i, j)]
        if self.masks is not None:
            ms = [torch.as_tensor(self.masks[k]) for k in range(i, j)]
            mask = [m if m.dtype in (torch.uint8, torch.bool, torch.float32) else m.float() for m in ms]
        return depth, mask

    @staticmethod
    def _uniform(ts):
        return all(t.shape == ts[0].shape and t.dtype == ts[0].dtype and not t.is_cuda for t in ts)

    def _run(self):
        cpu0 = time.thread_time()
        try:
            self._run_inner()
        finally:
            self.stats["feeder_thread_cpu_s"] = time.thread_time() - cpu0

    def _run_inner(self):
        try:
            if self.cuda:
                torch.cuda.set_device(self.device)
            stage = self._stage_device if self.cuda else self._stage_host
            b = 0
            for i, j, items in self._cut():
                if self.stop.is_set():
                    return
                t0 = time.perf_counter()
                depth, mask = self._extras(i, j)
                t1 = time.perf_counter()
                self.fetch_s += t1 - t0
                self.free.acquire()
                self.stats["wait_slot_s"] += time.perf_counter() - t1
                self.stats["batches"] += 1
                if self.stop.is_set():
                    return
                self.q.put(stage(b % self.nslots, i, j, items, depth, mask))
                b += 1
            self.q.put(None)
        except BaseException as e:                                       # re-raised by the consumer
            self.q.put(e)

    def _stage_host(self, s, i, j, items, depth, mask):
        """The CPU stand-in: the sub-batch as stacked host tensors, no slot buffers and no streams."""
        content = items if isinstance(items, torch.Tensor) else torch.stack(items)
        if mask is not None and all(m.shape == mask[0].shape for m in mask):
            mask = torch.stack(mask)
        return _Batch(i, j, content, depth, mask, None, s)

    def _to_device(self, s, name, ts):
        """The tensors ``ts`` (one per frame) of slot ``s`` on their way up, on the copy stream: host tensors of one shape and
        dtype -> the slot's buffer ``name`` (a device view [len(ts), ...]), other host tensors -> one upload each (a list).
        Returns them and True - or, if all of them already are on the device, ``ts`` as it is and False: nothing left pinned
        memory, and it is the consumer that tells the allocator who reads them (``__iter__``)."""
        if all(t.is_cuda for t in ts):
            return ts, False
        if self._uniform(ts):
            return self._stage(s, name, ts), True
        return [t if t.is_cuda else self._upload(t) for t in ts], True

    def _stage_device(self, s, i, j, items, depth, mask):
        """Sub-batch i..j-1 into slot ``s``: its frames, proximity maps and masks uploaded on the copy stream, ordered behind
        the slot's previous use and ahead of the consumer (``ready``)."""
        t2 = time.perf_counter()
        if self.h2d_done[s] is not None:
            sleep_wait(self.h2d_done[s])                     # the slot's previous uploads have left its pinned buffers
        t3 = time.perf_counter()
        self.stats["wait_h2d_s"] += t3 - t2
        # device tensors handed over by the stores (a mask or depth map computed lazily in __getitem__, a frame made on the GPU)
        # were produced on the fetching threads' current stream, not on the copy stream: whatever reads them below - and the
        # consumer, through `ready` - is ordered behind an event recorded there now
        groups = [items if isinstance(items, list) else [items], depth or [], mask or []]
        fetched = _event(self.device) if any(t.is_cuda for g in groups for t in g) else None
        staged = False                                       # something was copied out of the slot's pinned buffers
        with torch.cuda.stream(self.copy_stream):
            if self.consumed[s] is not None:
                self.copy_stream.wait_event(self.consumed[s])      # the kernels that read this slot have finished
            if fetched is not None:
                self.copy_stream.wait_event(fetched)
            if isinstance(items, list):                      # (else a ready block of a device-resident store; a list of device
                items, staged = self._to_device(s, "content", items)         # tensors is stacked by the consumer on its own stream)
            if depth is not None:
                depth, up = self._to_device(s, "depth", depth)
                staged |= up
                if isinstance(depth, torch.Tensor):
                    depth = [depth[k] for k in range(j - i)]
            if mask is not None:
                mask, up = self._to_device(s, "mask", mask)  # (a list: masks of several sizes, composited per frame)
                staged |= up
                if not up:
                    mask = torch.stack(mask)
                    mask.record_stream(self.compute_stream)
            ready = None
            if staged or fetched is not None:                # `ready` carries the uploads' and `fetched`'s order on to the consumer
                ready = _event(self.device, self.copy_stream)
                if staged:                                   # only pinned buffers need the host to wait before reuse
                    self.h2d_done[s] = ready
        self.stats["stage_s"] += time.perf_counter() - t3
        return _Batch(i, j, items, depth, mask, ready, s)

    # ---- consumer ---------------------------------------------------------------------------------------------------------------
    def __iter__(self):
        while True:
            item = self.q.get()
            if item is None:
                return
            if isinstance(item, BaseException):
                raise item
            if item.ready is not None:
                torch.cuda.current_stream(self.device).wait_event(item.ready)
            if self.cuda:
                # Device tensors made on the fetch threads (device_transform_u8's resized frames, lazily computed depth maps) belong to
                # THEIR stream's allocator pool: once this batch drops them the block may be handed to the next fetch at once, while the
                # consumer's kernels - on another stream whenever the caller runs the job under `torch.cuda.stream(...)` - are still
                # queued.  Telling the allocator who reads them closes that (round-5 advisor finding).
                cur = torch.cuda.current_stream(self.device)
                for group in (item.content, item.depth, item.mask):
                    if isinstance(group, list):
                        for t in group:
                            if isinstance(t, torch.Tensor) and t.is_cuda:
                                t.record_stream(cur)
            if isinstance(item.content, list):                           # frames that already were device tensors
                item.content = torch.stack(item.content)
            yield item

    def release(self, batch):
        """The consumer has enqueued the last kernel that reads ``batch``'s slot."""
        if self.cuda and batch.slot is not None:
            self.consumed[batch.slot] = _event(self.device)
        self.free.release()

    def close(self):
        self.stop.set()
        for _ in range(self.nslots + 1):
            self.free.release()
        self.thread.join(30)
        self.pool.shutdown(wait=True, cancel_futures=True)


class HostCopier:
    """Asynchronous device -> pinned-host copies on a stream of their own: a finished block leaves the device while the next
    sub-batch's kernels run.  ``finish()`` waits for all of them."""

    def __init__(self, device):
        self.device = torch.device(device)
        self.cuda = self.device.type == "cuda"
        self.bytes = 0
        if self.cuda:
            self.stream = torch.cuda.Stream(self.device)

    def copy(self, dst_host, src):
        """dst_host.copy_(src) once the work enqueued so far on the current stream has finished.  Returns the event recorded
        behind the copy (None on a CPU device: the copy is done)."""
        self.bytes += src.numel() * src.element_size()
        if not self.cuda:
            dst_host.copy_(src)
            return None
        ready = _event(self.device)
        with torch.cuda.stream(self.stream):
            self.stream.wait_event(ready)
            dst_host.copy_(src, non_blocking=True)
            src.record_stream(self.stream)
            return _event(self.device, self.stream)

    def finish(self):
        if self.cuda:
            sleep_wait(_event(self.device, self.stream))


class FileSink:
    """Writes finished uint8 frames to image files off the compute path: the device -> host copy of a sub-batch runs on its own
    stream into a pinned buffer, a worker thread waits for it and encodes / saves the files (PIL), so the next sub-batch's
    kernels are already running.  ``close()`` waits for every file and re-raises the first error.  ``jpeg_options`` (``JpegOptions``, a
    (quality, subsampling, optimize) tuple or None for Pillow's defaults): how .jpg / .jpeg files are saved, on either route; files of
    other extensions never see them.  ``jpeg_on_device`` (default off): a block whose paths all end in .jpg / .jpeg is encoded on the
    compute stream (adain_jpeg_encode_u8: the bytes PIL would write); the copy stream then brings over the lengths and, on a second
    stream of the sink's own, exactly that many bytes per frame, and the worker only writes them.  (The files do not ride on the
    lengths' stream: by the time a worker knows its lengths, the launching thread may have queued later blocks' length copies there,
    each waiting for later kernels.)  ``png_on_device`` (default off): a block whose paths all end in .png goes the same way through
    adain_png_encode_u8 - files of the frames' pixels, not Pillow's bytes.  ``routes`` (a ``runtime.OutputRoutes``) gives all three.  A
    block of mixed extensions, and every block with the switches off, is saved by PIL as before."""

    def __init__(self, device, workers=4, max_in_flight=None, jpeg_on_device=False, jpeg_options=None, png_on_device=False, routes=None):
        self.copier = HostCopier(device)
        self.routes = OutputRoutes.of(routes) if routes is not None else OutputRoutes(JpegRoutes(jpeg_on_device, options=jpeg_options), PngRoute(png_on_device))
        self.file_stream = torch.cuda.Stream(self.copier.device) if (self.routes.jpeg.encode_on_device or self.routes.png.encode_on_device) and self.copier.cuda else None
        self.file_bytes = 0                # bytes of encoded files the workers copied (under spare_lock)
        self.pool = ThreadPoolExecutor(max_workers=workers, thread_name_prefix="adain-file-sink")
        self.futures = []
        # back-pressure: at most `max_in_flight` blocks (default 2 per writer) sit in pinned memory waiting for their encoder;
        # write() blocks when the writers fall behind instead of pinning the whole job.  The pinned buffers are reused.
        self.max_in_flight = max(1, int(max_in_flight if max_in_flight is not None else 2 * workers))
        self.slots = threading.Semaphore(self.max_in_flight)
        self.spare = {}                    # block shape -> idle pinned buffers
        self.spare_lock = threading.Lock()
        self.wait_s = 0.0                  # time write() spent blocked on the writers

    @property
    def d2h_bytes(self):
        with self.spare_lock:
            return self.copier.bytes + self.file_bytes

    def _pinned(self, shape):
        with self.spare_lock:
            idle = self.spare.get(shape)
            if idle:
                return idle.pop()
        return torch.empty(shape, dtype=torch.uint8, pin_memory=True)

    def _save(self, arr, path):             # the host job's seam: tests slow it down
        self.routes.save(arr, path)

    def _encoder(self, u8_block, paths):
        """The device encoder of a block (``OutputRoutes.encoder``; a sink on a GPU and a 4-D block only), or None: downloaded and saved by PIL."""
        return self.routes.encoder(u8_block, list(paths)) if self.copier.cuda and u8_block.dim() == 4 else None

    def _encodes(self, u8_block, paths):
        return self._encoder(u8_block, paths) is not None

    def _write_encoded(self, encode, u8_block, paths):
        """The device-encode form of ``write``: ``encode`` on the current stream, the lengths behind it on the copy stream; the worker
        waits for them, copies each frame's ``lengths[i]`` bytes into one pinned buffer on the copy stream and writes the files."""
        files, lengths = encode(u8_block)
        k = len(paths)
        lengths_host = torch.empty((k,), dtype=torch.int32, pin_memory=True)
        have_lengths = self.copier.copy(lengths_host, lengths)
        stream = self.file_stream          # the encode has finished once the lengths are here: nothing else to wait for

        def job():
            host = None
            try:
                sleep_wait(have_lengths)
                sizes = lengths_host.tolist()
                capacity = 1 << max(12, (sum(sizes) - 1).bit_length())       # pinned buffers are pooled by power-of-two size
                host = self._pinned((capacity,))
                with torch.cuda.stream(stream):
                    at = 0
                    for i, size in enumerate(sizes):
                        host[at:at + size].copy_(files[i, :size], non_blocking=True)
                        at += size
                    files.record_stream(stream)
                    done = _event(self.copier.device, stream)
                with self.spare_lock:
                    self.file_bytes += at
                sleep_wait(done)
                arr = host.numpy()
                at = 0
                for size, p in zip(sizes, paths):
                    with open(str(p), "wb") as f:
                        f.write(arr[at:at + size].tobytes())
                    at += size
            finally:
                if host is not None:
                    with self.spare_lock:
                        self.spare.setdefault(tuple(host.shape), []).append(host)
                self.slots.release()

        self.futures.append(self.pool.submit(job))

    def write(self, u8_block, paths):
        """u8_block [k,h,w,c] on the engine's device (finished on the current stream); paths: k file paths."""
        t0 = time.perf_counter()
        self.slots.acquire()
        self.wait_s += time.perf_counter() - t0
        encode = self._encoder(u8_block, paths)
        if encode is not None:
            try:
                return self._write_encoded(encode, u8_block.contiguous(), paths)
            except BaseException:
                self.slots.release()
                raise
        shape = tuple(u8_block.shape)
        if not self.copier.cuda:
            host, done = u8_block, None
        else:
            host = self._pinned(shape)
            done = self.copier.copy(host, u8_block)

        def job():
            try:
                if done is not None:
                    sleep_wait(done)                    # (a writer thread must not spin a core while the copy is on its way)
                arr = host.numpy()
                for k, p in enumerate(paths):
                    self._save(arr[k], p)
            finally:
                if done is not None:
                    with self.spare_lock:
                        self.spare.setdefault(shape, []).append(host)
                self.slots.release()

        self.futures.append(self.pool.submit(job))

    def close(self):
        err = None
        for f in self.futures:
            try:
                f.result()
            except BaseException as e:      # keep waiting for the others, report the first
                err = err or e
        self.pool.shutdown(wait=True)
        self.futures = []
        if err is not None:
            raise err


# ---------------------------------------------------------------------------------------------------------------------------------
def _mark(engine):
    m = getattr(engine, "mark", None)
    return m() if m is not None else time.perf_counter()


def _elapsed(engine, a, b):
    f = getattr(engine, "elapsed", None)
    return f(a, b) if f is not None else b - a


def _stylize_batch(engine, batch, alpha, depth_offset, depth_prominence, preserve_color=False, style_weights=None):
    """One sub-batch of the feeder on the engine -> the finished uint8 frames [k,H,W,3].  ``style_weights``: the sub-batch's rows of
    the job's style-mix weights, on the device."""
    content, dev = batch.content, engine.device
    how = {"preserve_color": True} if preserve_color else {}        # only named when asked for: engines without the keyword keep working
    if style_weights is not None:
        how["style_weights"] = style_weights
    one_call = getattr(engine, "stylize_u8", None)
    if (one_call is not None and content.dtype == torch.uint8 and content.dim() == 4 and content.shape[-1] == 3
            and not isinstance(batch.mask, list)):
        # decoded RGB frames with (at most) one mask tensor for the sub-batch: the whole chain in one C-ABI call
        return one_call(content, alpha=alpha, depth_maps=batch.depth, offset=depth_offset, prominence=depth_prominence, masks=batch.mask,
                        **how)
    if batch.depth is not None:
        out = engine.stylize_depth(content, [d.to(dev, torch.float32) for d in batch.depth], depth_offset, depth_prominence, **how)
    else:
        out = engine.stylize(content, alpha, **how)
    if isinstance(batch.mask, list):           # masks of different sizes inside one sub-batch: composite frame by frame
        out = torch.cat([engine.composite(content[k:k + 1], out[k:k + 1], m.to(dev).float().unsqueeze(0))
                         for k, m in enumerate(batch.mask)])
    elif batch.mask is not None:
        out = engine.composite(content, out, batch.mask.to(dev).float())
    return engine.to_u8(out)


class _StyleSwitch:
    """``ready(s)`` makes the engine ready for a frame whose style index is ``s``, with one lookup ``key -> maker``: ``s`` -> ``set_style``,
    ``("pixels", s)`` -> ``set_style_image`` (``preserve_color``), ``"mix"`` -> ``set_styles`` of the whole list (``mixing``).  A style is
    made once and kept in ``cache`` (the caller's ``style_cache``, or the job's own) as whatever ``engine.style_stats()`` returns."""
    def __init__(self, engine, style_list, cache, preserve_color=False, mixing=False):
        self.engine, self.cache, self.cur = engine, cache if cache is not None else {}, None
        self.key, self.make = ((lambda s: "mix", lambda s: engine.set_styles(style_list)) if mixing else
                               (lambda s: ("pixels", s), lambda s: engine.set_style_image(style_list[s])) if preserve_color else
                               (lambda s: s, lambda s: engine.set_style(style_list[s])))

    def ready(self, s):
        key = self.key(s)
        if key != self.cur:
            self.cur = key
            if key not in self.cache:
                self.cache[key] = self.make(s).style_stats()
            self.engine.use_style_stats(self.cache[key])


def _cat_blocks(blocks, geom, device):
    """The uint8 blocks as one [k,H,W,C] tensor; without blocks, an empty one of the frame geometry ``geom`` = (H, W, C)."""
    if blocks:
        return torch.cat(blocks) if len(blocks) > 1 else blocks[0]
    return torch.empty((0,) + tuple(geom), dtype=torch.uint8, device=device)


class _BlockGather:
    """The collectives of one job, the same sequence on every rank whatever happens to its block: pieces 0 .. k-2 of the
    block as soon as they are finished (``add``), then - ``finish`` - the status word and the last piece.  A single piece
    (k = 1) is the job's one gather after the status word.  The finished frames arrive on ``dst`` in frame order and, piece
    by piece, in ``host_out``."""

    def __init__(self, n, rank, world, dst, group, device, chunks, out_hw, info, copier=None, host_out=None):
        self.n, self.rank, self.world, self.dst, self.group, self.device = n, rank, world, dst, group, device
        self.chunks, self.out_hw, self.info, self.copier, self.host_out = chunks, out_hw, info, copier, host_out
        # pieces issued before the status word take the frame geometry from the caller
        self.piece_geom = tuple(out_hw) + (3,) if chunks > 1 else None
        self.first = [sh.shard_range(n, world, r)[0] for r in range(world)]
        # piece c of rank r = frames [first[r] + a, first[r] + b) with (a, b) = bounds[r][c]
        self.bounds = [sh.chunk_bounds(count, chunks) for count in sh.shard_counts(n, world)]
        self.blocks, self.shapes = [], set()   # finished sub-batches (i, j, u8) of this rank, their frame shapes
        self.issued = 0                        # pieces of this rank that have joined their gather
        self.pending, self.landed = [], []     # (piece, counts, finish closure) in flight; (first frame, rows) arrived on dst

    def cuts(self):
        """The frame indices at which a sub-batch of this rank must end: the borders of its pieces."""
        return [self.first[self.rank] + b for (_, b) in self.bounds[self.rank]]

    def add(self, i, j, u8):
        """Sub-batch (frames i..j-1) is finished: every in-loop piece that is now complete joins its gather."""
        self.blocks.append((i, j, u8))
        self.shapes.add(tuple(u8.shape[1:]))
        if self.chunks > 1 and tuple(u8.shape[1:3]) != tuple(self.out_hw):
            raise ValueError(f"stylize_frames_sharded: out_hw {tuple(self.out_hw)} but a finished frame is {tuple(u8.shape[1:3])}")
        while self.issued < self.chunks - 1 and self.first[self.rank] + self.bounds[self.rank][self.issued][1] <= j:
            self._issue(self.piece_geom)

    def _issue(self, geom, zeros=False):
        """The next piece of this rank's block joins its gather; ``zeros``: this rank has failed - it still takes part, with a
        zero-filled block of the agreed geometry, so that its peers (already inside the collective) are not left waiting; the
        status word after the last in-loop piece then raises on every rank."""
        c = self.issued
        self.issued += 1
        lo = self.first[self.rank]
        a, b = self.bounds[self.rank][c]
        if zeros:
            local = torch.zeros((b - a,) + geom, dtype=torch.uint8, device=self.device)
        else:
            local = _cat_blocks([u8 for (i, j, u8) in self.blocks if lo + a <= i and j <= lo + b], geom, self.device)
        cnts = [bd[c][1] - bd[c][0] for bd in self.bounds]
        self.info["gathers"] += 1
        self._land()                       # the previous piece has long arrived: hand it on before queueing the next
        self.pending.append((c, cnts, sh.gather_frames(local, self.n, dst=self.dst, group=self.group, async_op=True, counts=cnts)))

    def _land(self):
        """Waits (on the stream) for the gathered pieces issued so far and files them on dst: into the job's result and, piece
        by piece, into ``host_out``."""
        while self.pending:
            c, cnts, fin = self.pending.pop(0)
            got = fin()
            if self.rank != self.dst:
                continue
            # rank r's rows of the piece belong at frame first[r] + a; a job's only piece is the job in frame order: one run
            runs = [(0, self.n)] if self.chunks == 1 else [(self.first[r] + self.bounds[r][c][0], cnts[r]) for r in range(self.world)]
            at = 0
            for frame, k in runs:
                if k:
                    self.landed.append((frame, got[at:at + k]))
                    if self.copier is not None:
                        self.copier.copy(self.host_out[frame:frame + k], got[at:at + k])
                at += k

    def _drain(self):
        """An abandoned job: the pieces already issued are complete collectives (every rank took part) - wait for them so that
        nothing of this job is left in flight on the communicator, and drop the data."""
        while self.pending:
            try:
                self.pending.pop(0)[2]()
            except Exception:
                pass

    def finish(self, err):
        """The block is over, ``err`` = what ended it early (or None).  Returns the job's frames [n,H,W,C] on ``dst`` (None on
        the other ranks) - or raises, on EVERY rank, if any rank failed or the frames do not share one size."""
        # every rank issues every in-loop piece, whatever happened to its block: the collective sequence stays identical
        # (pieces 0 .. k-2, status word, last piece); a failed rank sends zeros and the status word raises everywhere
        try:
            while self.issued < self.chunks - 1:
                self._issue(self.piece_geom, zeros=err is not None)
        except Exception as e:
            err = err or e
        ok, geom, uniform = sh.agree_geometry(err is None, self.shapes, self.group, self.device)
        if err is not None or not ok:
            self._drain()
        if err is not None:
            raise err
        if not ok:
            raise RuntimeError("stylize_frames_sharded: another rank failed; job abandoned before the gather")
        if not uniform:
            raise ValueError("stylize_frames_sharded: the gather needs one frame size on every rank")
        if geom is not None and self.out_hw is not None and tuple(self.out_hw) != tuple(geom[:2]):
            raise ValueError(f"stylize_frames_sharded: out_hw {tuple(self.out_hw)} but the finished frames are {tuple(geom[:2])}")
        if geom is None:                       # an empty job: nothing to gather anywhere
            return torch.empty((0, 0, 0, 3), dtype=torch.uint8, device=self.device) if self.rank == self.dst else None
        self._issue(self.piece_geom or geom)   # (a job's only piece: a rank with an empty block learns the geometry from the status word)
        self._land()
        if self.rank != self.dst:
            return None
        if len(self.landed) == 1:              # one run holds every frame: it is the result
            return self.landed[0][1]
        out = torch.empty((self.n,) + tuple(geom), dtype=torch.uint8, device=self.device)
        for frame, rows in self.landed:
            out[frame:frame + rows.shape[0]].copy_(rows)
        return out


def stylize_frames_sharded(engine, frames, styles, *, style_of=None, alpha=0.5, depth_maps=None, depth_offset=0.15,
                           depth_prominence=20, masks=None, post=None, sub_batch=None, group=None, dst=0, gather=True,
                           require_transport=None, style_cache=None, out_hw=None, gather_chunks=1, sink=None,
                           prefetch=4, host_out=None, fetch_workers=4, preserve_color=False, style_weights=None):
    """Stylises ``frames`` (a sequence indexed lazily: a rank only ever touches its own block; an element is a decoded
    frame uint8 [h,w,3] / RGB PIL image, or a float tensor [3,h,w] in [0,1]) and returns ``(frames_u8, info)``: the uint8
    frames [n,H,W,3] in frame order on rank ``dst`` (None on the other ranks; with ``gather=False`` the local block — a
    list of per-size blocks if the frames have several sizes, None if a ``sink`` took them) and a dict with the shard, the
    timings and the transport.

    styles          one style tensor [1|.,3,hs,ws] or a list of them; ``style_of[i]`` picks the style of frame i
                    (``style_schedule``); every style image is encoded once per rank and call, its 2 x 512 statistics
                    are kept for the call (pass a dict as ``style_cache`` to keep them across calls with the SAME styles).
    depth_maps      optional sequence of [h0,w0] proximity maps, one per frame -> depth-aware blend (test.py:52-71) with
                    ``depth_offset`` / ``depth_prominence``; otherwise the ``alpha`` blend (test.py:74-81).
    masks           optional sequence of [1|3,hm,wm] masks -> content-mask composite (test.py:222-236).
    preserve_color  every frame is styled with ``coral(style, frame)`` instead of the style itself (adain_inference's
                    ``preserve_color``, test.py:201-202), on the device: each style's PIXELS stay resident next to its statistics
                    (``engine.set_style_image``; in ``style_cache`` under ``("pixels", index)``).  A frame's bytes do not depend on
                    the sub-batch or the shard it is in.
    style_weights   style interpolation: float32 rows [n][K] (``style_crossfade``), K = the number of ``styles``; frame i is styled with
                    the mix ``style_weights[i]`` of ALL the styles (``engine.set_styles``, once per call; in ``style_cache`` under
                    ``"mix"``) instead of the one style ``style_of[i]`` picks.  The rows go to the device once and every sub-batch takes
                    its slice; they are used as given.  A frame's bytes do not depend on the sub-batch or the shard it is in.  Not
                    with ``preserve_color`` or ``style_of``.
    sub_batch       frames per sub-batch; None (default) = chosen from the frame size, about three megapixels per sub-batch
                    (``auto_sub_batch``: 26 frames of 256 x 456, 6 of 512 x 912; 4 of 1080p or 1200 x 1600 - inside the measured optima).
    post            optional ``f(u8_block) -> u8_block`` applied per sub-batch on the owning rank BEFORE the gather
                    (frame-local work such as the INTER_AREA resize, so the gather moves the small frames).
    sink            optional ``f(i, j, u8_block)`` called with every finished sub-batch (frames i..j-1) on the owning rank.
    require_transport   e.g. "rccl": raise before any work if the gather would use another transport.
    out_hw          (H, W) of a finished frame, if the caller knows it: lets chunked gathers run with ranks whose block is empty.
    gather_chunks   1: ONE gather when every rank has finished (after the status word: an error anywhere raises everywhere).
                    k > 1 (needs ``out_hw``: ValueError without it): the block is gathered in k pieces, pieces 0 .. k-2
                    issued asynchronously as soon as they are finished so that they overlap the rest of the compute, then the
                    status word, then the last piece.  Every rank issues every piece whatever happens to its block - a rank that
                    fails (or whose frames are not ``out_hw``) sends zero-filled pieces - so the collective sequence is the same
                    on every rank and the status word still raises everywhere.
    host_out        a (pinned) uint8 host tensor [n,H,W,3]: finished frames are also copied into it, asynchronously on a copy
                    stream as they become available — per sub-batch on a single rank (or with ``gather=False``: every rank fills
                    the rows of its own block), per gathered piece on ``dst`` otherwise — and are all there when the call returns.

    The gather needs one frame size over the whole job; with ``gather=False`` sizes may differ from frame to frame (a
    sub-batch ends where the size changes).  Nothing in the frame loop synchronises the device or communicates."""
    rank, world = sh.rank_world(group)
    n = len(frames)
    lo, hi = sh.shard_range(n, world, rank)
    style_list = list(styles) if isinstance(styles, (list, tuple)) else [styles]
    if style_weights is not None:
        if style_of is not None or preserve_color:
            raise ValueError("style_weights mixes every style into every frame: it goes with neither style_of nor preserve_color")
        style_weights = np.ascontiguousarray(np.asarray(style_weights, dtype=np.float32))
        if style_weights.shape != (n, len(style_list)):
            raise ValueError(f"style_weights must be [{n}][{len(style_list)}] (one row per frame, one weight per style), got {style_weights.shape}")
    if style_of is None:
        style_of = [0] * n
    if len(style_of) != n:
        raise ValueError("style_of needs one style index per frame")
    dev = engine.device
    on_gpu = dev.type == "cuda"
    gathering = gather and world > 1
    if int(gather_chunks) > 1 and out_hw is None:
        # Pieces are issued inside the frame loop, BEFORE the status word: a rank that fails must still take part in every one of
        # them (with zero-filled blocks), so it has to know what a finished frame looks like without having finished one.  Asking
        # for pieces without out_hw is an error, decided from the arguments alone: the same on every rank and for every world size
        # (round 4 silently ran such a job with one end gather: no overlap and no signal).
        raise ValueError("gather_chunks > 1 needs out_hw (the size of a finished frame): pieces are gathered before the ranks agree")
    transport = sh.device_transport(torch.empty(0, dtype=torch.uint8, device=dev), group) if gathering else None
    if gathering and require_transport and transport != require_transport:
        raise RuntimeError(f"final gather would run over {transport!r}, not {require_transport!r}")

    info = {"rank": rank, "world": world, "shard": (lo, hi), "transport": transport, "gathers": 0}
    t_host0 = time.perf_counter()
    cpu0_thread, cpu0_proc = time.thread_time(), time.process_time()
    abi0 = getattr(engine, "abi_calls", lambda: 0)()
    m0 = _mark(engine)
    copier = HostCopier(dev) if host_out is not None else None
    gathered = _BlockGather(n, rank, world, dst, group, dev, max(1, int(gather_chunks)), out_hw, info, copier, host_out) if gathering else None
    feeder = FrameFeeder(frames, lo, hi, style_of, sub_batch, dev, depth_maps, masks, depth=prefetch,
                         cuts=gathered.cuts() if gathering else (), workers=fetch_workers)
    blocks = []                            # without a gather: the finished sub-batches of this rank that the caller gets
    # At most MAX_QUEUED_BATCHES sub-batches are queued on the device beyond the one that is running: enough that the GPU never
    # waits for the host (a sub-batch is about three megapixels: >= 5 ms of kernels), few enough that this thread sleeps in
    # sleep_wait instead of spinning inside hipLaunchKernel on a full HIP queue.
    queued = []
    err = None
    try:
        switch = _StyleSwitch(engine, style_list, style_cache, preserve_color, mixing=style_weights is not None)
        mix = torch.from_numpy(style_weights).to(dev) if style_weights is not None and hi > lo else None      # the clip's rows, resident for the call
        for batch in feeder:
            if on_gpu and len(queued) >= MAX_QUEUED_BATCHES:
                sleep_wait(queued.pop(0))
            i, j = batch.i, batch.j
            switch.ready(style_of[i])
            u8 = _stylize_batch(engine, batch, alpha, depth_offset, depth_prominence, preserve_color, None if mix is None else mix[i:j])
            feeder.release(batch)
            if on_gpu:
                queued.append(_event(dev))
            if post is not None:
                u8 = post(u8)
            if sink is not None:
                sink(i, j, u8)
            if gathering:
                gathered.add(i, j, u8)
            else:
                if copier is not None:
                    copier.copy(host_out[i:j], u8)
                if gather or sink is None:
                    blocks.append(u8)
    except Exception as e:                 # agreed on below: every rank raises, none is left waiting in the gather
        err = e
    finally:
        feeder.close()
    if err is not None:                    # a failed job: its kernels may still read the feeder's slot buffers - let them finish before
        try:                               # the buffers go back to the allocator on the way out
            engine.synchronize()
        except Exception:
            pass
    info["h2d_bytes"] = feeder.h2d_bytes
    info["fetch_s"] = feeder.fetch_s
    info["feeder"] = {k: (round(v, 4) if isinstance(v, float) else v) for k, v in feeder.stats.items()}
    m1 = _mark(engine)
    info["enqueue_s"] = time.perf_counter() - t_host0      # host WALL time to fetch, upload and launch the whole block (includes
                                                           # time blocked on a full HIP queue or an empty feeder queue)
    # CPU time, which is what eight ranks sharing one host compete for: of the launching thread alone (kernel launches through
    # the C ABI, tensor bookkeeping) and of the whole process (+ feeder, fetch pool, sink writers, the HIP runtime's own threads)
    info["host_cpu_s"] = time.thread_time() - cpu0_thread
    info["process_cpu_s"] = time.process_time() - cpu0_proc
    info["abi_calls"] = getattr(engine, "abi_calls", lambda: 0)() - abi0

    out = m2 = None
    if gathering:
        out = gathered.finish(err)         # the job's status word, then its (last) gather; raises on every rank if one failed
        m2 = _mark(engine)
    elif err is not None:
        raise err
    if on_gpu:                             # sleep until the device has finished this job's work, then the (now immediate) synchronisations
        sleep_wait(_event(dev))
    if copier is not None:
        copier.finish()
        info["d2h_bytes"] = copier.bytes
    engine.synchronize()
    info["compute_s"] = _elapsed(engine, m0, m1)
    info["gather_s"] = _elapsed(engine, m1, m2) if m2 is not None else 0.0
    if not gathering and (gather or sink is None):       # the local block(s) - unless a sink took them
        if len({tuple(u8.shape[1:]) for u8 in blocks}) > 1:
            if gather:
                raise ValueError("stylize_frames_sharded: the gather needs one frame size over the whole job")
            return blocks, info
        out = _cat_blocks(blocks, tuple(out_hw) + (3,) if out_hw is not None else (0, 0, 3), dev)
    return out, info


def video_style_transfer_sharded(engine, frames, styles, *, flows=None, target_resolution=None, blend_alpha=0.7, depth_maps=None,
                                 offset=0.30, prominence=20, alpha=0.5, sub_batch=None, group=None, dst=0, require_transport=None,
                                 gather_chunks=1, preserve_color=False):
    """The video caller (reference video/utils.py:297-369) over a frame list: per-frame AdaIN sharded over the ranks (styles
    switching through the clip as ``style_schedule`` says when several are given; depth-aware when ``depth_maps`` are
    given, which is how the reference runs it: ``use_depth=True``, offset 0.30, prominence 20), ``cv2.resize(...,
    target_resolution, INTER_AREA)`` of every stylised frame on its own rank (:352-353; ``target_resolution`` =
    (width, height)), ONE gather, then on ``dst`` the recurrence ``frame_i = blend(frame_i, warp(result_{i-1}, flow_{i-1}),
    blend_alpha)`` (:355-368) over ``flows`` [n-1,2,H,W] (prev -> current at the target resolution: ``flow.FlowSequence().batch``
    computes the reference's Farneback flows on the device, ``tvl1.TVL1Sequence().batch`` its Dual TV-L1 flows, or the caller brings its own).  Returns ``(frames_u8 on dst | None, info)``."""
    n = len(frames)
    style_list = list(styles) if isinstance(styles, (list, tuple)) else [styles]
    post = out_hw = None
    if target_resolution is not None:
        post = lambda u8: engine.resize_area_u8(u8, target_resolution)
        out_hw = (int(target_resolution[1]), int(target_resolution[0]))
    out, info = stylize_frames_sharded(engine, frames, style_list, style_of=style_schedule(n, len(style_list)), alpha=alpha,
                                       depth_maps=depth_maps, depth_offset=offset, depth_prominence=prominence, post=post,
                                       sub_batch=sub_batch, group=group, dst=dst, require_transport=require_transport,
                                       out_hw=out_hw, gather_chunks=gather_chunks, preserve_color=preserve_color)
    if out is not None and flows is not None and n > 1:
        t0 = time.perf_counter()
        out = engine.temporal_blend(out, flows.to(out.device, torch.float32), blend_alpha)
        engine.synchronize()
        info["temporal_blend_s"] = time.perf_counter() - t0
    return out, info


def precompute_guides_sharded(engine, views, names, output_dir, style, *, masks=None, content_size=512, crop=False, alpha=0.5,
                              depth_maps=None, depth_offset=0.5, depth_prominence=20, save_ext=".jpg", sub_batch=None, group=None,
                              dst=0, write="dst", require_transport=None, writers=4, jpeg_on_device=False, preserve_color=False,
                              jpeg_options=None, png_on_device=False, png_decode_on_device=False):
    """The guide-image precompute of the reference's Style_3DGS/train.py:86-115 over all training views, sharded: every view
    is resized as ``adain_inference(content_size=...)`` resizes it (test.py:190-200), stylised, composited with its mask
    (``gt_image_np > 0``, train.py:97) and saved as ``<output_dir>/<name><save_ext>`` — the reference's naming, so the guide
    loss (train.py:208-221) reads the files back unchanged.  ``write="dst"``: the uint8 views are gathered and rank ``dst``
    writes every file (views must then share one size); ``write="local"``: every rank writes its own block as it is
    finished — nothing is gathered and the views may have any mix of sizes.  The views are decoded / resized on a worker
    thread ahead of the kernels and travel to the device as uint8; the files are encoded and written by ``writers`` threads
    behind them.  ``jpeg_on_device``: .jpg / .jpeg guides are encoded on the device and only the files cross to the host (FileSink;
    the same bytes).  ``jpeg_options`` (``JpegOptions``): quality, subsampling and optimize of .jpg / .jpeg guides, on either route;
    default: Pillow's default save.  ``png_on_device``: .png guides are encoded on the device (FileSink; the same pixels, not Pillow's
    bytes).  ``png_decode_on_device``: 8-bit RGB views given as .png paths are decoded on the device (``rt.png_decode_batch``: the pixels
    PIL decodes) and resized there, a rank's block in batches of the feeder's sub-batch - one call for the views of a batch that share a
    size - on the fetch threads that run ahead of the kernels; grey and RGBA views, and whatever the decoder does not take, keep PIL and
    the host transform.  ``preserve_color``: every view is styled with ``coral(style, view)`` (``stylize_frames_sharded``).  Every rank returns the full {name: Path} map once all files exist (an error on any rank raises on all)."""
    from PIL import Image

    from . import runtime as rt
    from .AdaIN.test import device_transform_u8, test_transform_u8

    if write not in ("dst", "local"):
        raise ValueError("write must be 'dst' or 'local'")
    rank, world = sh.rank_world(group)
    out_dir = Path(output_dir)
    out_dir.mkdir(exist_ok=True, parents=True)
    tf = test_transform_u8(content_size, crop)
    lo, hi = sh.shard_range(len(views), world, rank)
    png_step = max(1, int(sub_batch)) if sub_batch else AUTO_FETCH_SUB_BATCH          # the sub-batch the feeder's fetch window is sized by
    png_lock, png_done, png_frames = threading.Lock(), set(), {}

    def png_view(k):
        """View k, a .png path of this rank's block, decoded and resized on the device - or None: the host opens it (a grey or RGBA file,
        one that png_file.parse refuses or that did not decode cleanly, a transform that is not the device's).  The block's .png paths
        are decoded in batches of the feeder's sub-batch - the RGB files of a batch that share a size in one ``rt.png_decode_batch`` call,
        its record read once - on whichever fetch thread asks first; a frame stays cached until it is consumed."""
        from .AdaIN.test import _device_plan, device_frame_transform_u8

        if not (lo <= k < hi):
            return None
        b = (k - lo) // png_step
        with png_lock:
            if b not in png_done:
                png_done.add(b)
                items = []
                for q in range(lo + b * png_step, min(hi, lo + (b + 1) * png_step)):
                    read = rt.read_input(rt.PNG_INPUT, views[q]) if isinstance(views[q], (str, Path)) and rt.is_png_path(views[q]) else None
                    if read is not None and read[0].c == 3 and _device_plan(read[0].w, read[0].h, content_size, crop) is not None:
                        items.append((q, *read))
                with torch.cuda.device(engine.device):
                    png_frames.update((q, frame) for q, frame, status, _ in rt.settle_decodes(rt.PNG_INPUT, items, engine.device) if status == 0)
            frame = png_frames.pop(k, None)
        if frame is None:
            return None
        with torch.cuda.device(engine.device):
            return device_frame_transform_u8(frame, content_size, crop)[0]

    class _Views:                         # lazy: a rank only opens and resizes the views of its own block
        def __len__(self):
            return len(views)

        def __getitem__(self, k):
            v = views[k]
            if png_decode_on_device and on_gpu and isinstance(v, (str, Path)) and rt.is_png_path(v):
                d = png_view(k)
                if d is not None:
                    return d
            if isinstance(v, (str, Path)):
                v = Image.open(str(v))
            if isinstance(v, (torch.Tensor, np.ndarray)):
                return v
            if on_gpu:                    # RGB: the decoded bytes go up, Resize [+ CenterCrop] run on the device (PIL's bytes exactly)
                d = device_transform_u8(v, content_size, crop, engine.device)
                if d is not None:
                    return d[0]
            return tf(v)

    on_gpu = torch.device(engine.device).type == "cuda"
    names = list(names)
    paths = {nm: out_dir / f"{nm}{save_ext}" for nm in names}
    sink = FileSink(engine.device, workers=writers, jpeg_on_device=jpeg_on_device, jpeg_options=jpeg_options, png_on_device=png_on_device)
    err = None
    info = {}
    try:
        if write == "local":
            _, info = stylize_frames_sharded(engine, _Views(), style, alpha=alpha, depth_maps=depth_maps, depth_offset=depth_offset,
                                             depth_prominence=depth_prominence, masks=masks, sub_batch=sub_batch, group=group, dst=dst,
                                             gather=False, preserve_color=preserve_color, sink=lambda i, j, u8: sink.write(u8, [paths[names[k]] for k in range(i, j)]))
        else:
            u8, info = stylize_frames_sharded(engine, _Views(), style, alpha=alpha, depth_maps=depth_maps, depth_offset=depth_offset,
                                              depth_prominence=depth_prominence, masks=masks, sub_batch=sub_batch, group=group, dst=dst,
                                              gather=True, require_transport=require_transport, preserve_color=preserve_color)
            if rank == dst and len(names):
                step = max(1, sub_batch or auto_sub_batch(*u8.shape[1:3]))
                for a in range(0, len(names), step):
                    sink.write(u8[a:a + step], [paths[nm] for nm in names[a:a + step]])
    except Exception as e:
        err = e
    t0 = time.perf_counter()
    try:
        sink.close()
    except Exception as e:
        err = err or e
    info["write_s"] = time.perf_counter() - t0
    info["d2h_bytes"] = sink.d2h_bytes
    info["sink_wait_s"] = sink.wait_s
    # every file exists when any rank returns - or every rank raises
    all_ok = sh.agree(err is None, group, engine.device)
    if err is not None:
        raise err
    if not all_ok:
        raise RuntimeError("precompute_guides_sharded: another rank failed; the guide set is incomplete")
    return paths, info


# ---------------------------------------------------------------------------------------------------------------------------------
# timed job loop (bench.py --job; driven on CPU by tests/test_distributed_gloo.py)
# ---------------------------------------------------------------------------------------------------------------------------------
def _max_over_ranks(dt, group, device="cuda"):
    """The largest ``dt`` of the ranks: on the host when the group has a CPU backend, else on ``device`` (default: the current one)."""
    if sh.dist_on() and dist.get_world_size(group) > 1:
        t = torch.tensor([dt], dtype=torch.float64)
        if "cpu" not in sh.backend_table(group):
            t = t.to(device)
        dist.all_reduce(t, op=dist.ReduceOp.MAX, group=group)
        dt = float(t.item())
    return dt


def run_timed_jobs(job, steps, warmup, *, barrier, group=None):
    """bench.py's contract around whole jobs: ``warmup`` untimed jobs, ``barrier()``, EXACTLY ``steps`` jobs, ``barrier()``;
    returns (seconds as the MAX over the ranks, the last job's result, per-rank info of the last job).  ``job()`` runs one
    whole sharded job (``stylize_frames_sharded`` ...) and returns ``(result, info)``; ``barrier()`` must leave this rank's
    device idle and every other rank's too."""
    res = info = None
    for _ in range(warmup):
        res, info = job()
    barrier()
    t0 = time.perf_counter()
    for _ in range(steps):
        res, info = job()
    barrier()
    dt = time.perf_counter() - t0
    if isinstance(info, dict):
        info["t0"], info["t1"] = t0, t0 + dt          # host clock at both ends of the timed region (bench.py's telemetry window)
    return _max_over_ranks(dt, group), res, info


# ---------------------------------------------------------------------------------------------------------------------------------
# timed per-step loop (bench.py's default mode with more than one rank; driven on CPU by tests/test_distributed_gloo.py)
# ---------------------------------------------------------------------------------------------------------------------------------
GATHER_MODES = ("end", "overlap")
MAX_END_GATHER_BYTES = 64 << 30        # what rank 0 may be asked to hold for one end-of-region gather


def run_timed_steps(step, steps, warmup, *, barrier, block_shape, device, mode="end", gather=True, group=None, dst=0,
                    mark=None, elapsed=None):
    """bench.py's contract around single steps: (with several ranks: ``barrier()``,) ``warmup`` untimed steps, ``barrier()``, EXACTLY
    ``steps`` steps + the path's one collective, ``barrier()``.  Returns ``(seconds as the MAX over the ranks, gathered frames on dst | None, info)``.

    ``step(out)`` enqueues one pass of the hot path over this rank's ``b`` resident frames and leaves the finished uint8 frames
    in ``out`` [b,H,W,3] (``block_shape`` = (b, H, W, 3)) - or returns another tensor of that shape if it cannot write in place.
    Every step is a job of ``world * b`` frames cut into contiguous per-rank blocks (weak scaling); its frames meet on ``dst``:

    mode "end"      (default) every rank keeps the frames of its ``steps`` steps in HBM ([steps * b, H, W, 3] uint8) and the timed
                    region ENDS with ONE gather of the whole block - the region is one ``steps * world * b``-frame job in frame
                    order, and no transport kernel ever runs beside the compute kernels (which fill every CU and cannot
                    rebalance around a late start: tools/probes/notes/dynamic_tile_scheduling.md).
    mode "overlap"  one asynchronous gather per step, at most two in flight: step k's gather overlaps step k+1's kernels.

    ``gather=False`` (or a single process) runs the steps alone.  ``mark()`` / ``elapsed(a, b)`` are the engine's stream time stamps
    (HIP events); the defaults use the host clock (CPU tests).  ``info`` = {"mode", "gathers", "compute_ms", "gather_ms",
    "gather_bytes"}: compute_ms from the first step to the last kernel of the last step, gather_ms from there to the arrival of
    the last gathered frame on this rank's stream (mode "overlap": the gathers of all but the last two steps lie inside compute_ms)."""
    if mode not in GATHER_MODES:
        raise ValueError(f"gather mode must be one of {GATHER_MODES}, got {mode!r}")
    if steps < 1 or warmup < 0:
        raise ValueError(f"run_timed_steps: steps must be >= 1 and warmup >= 0, got {steps} / {warmup}")
    rank, world = sh.rank_world(group)
    gathering = bool(gather) and sh.dist_on()
    b = int(block_shape[0])
    frame = tuple(int(v) for v in block_shape[1:])
    mark = mark or time.perf_counter
    elapsed = elapsed or (lambda a_, b_: b_ - a_)
    info = {"mode": mode if gathering else None, "gathers": 0, "gather_bytes": 0}
    n_end = steps * b
    if gathering and mode == "end" and n_end * world * int(np.prod(frame)) > MAX_END_GATHER_BYTES:
        raise ValueError(f"--gather end would collect {n_end * world * int(np.prod(frame)) / 2**30:.1f} GiB on rank {dst}: "
                         "use fewer steps or the overlapped gather")
    keep = torch.empty((max(n_end, b),) + frame, dtype=torch.uint8, device=device) if gathering and mode == "end" else None
    # without a kept block a step writes into one of three rotating buffers: at most two gathers are in flight, so the buffer a
    # step overwrites is the one whose gather was waited for (on the stream) a step ago
    scratch = [torch.empty((b,) + frame, dtype=torch.uint8, device=device) for _ in range(3)] if keep is None else None
    pending, got = [], [None]

    def one(k):
        slot = keep[(k % steps) * b:(k % steps + 1) * b] if keep is not None else scratch[k % 3]
        out = step(slot)
        if out is not None and out is not slot:
            if tuple(out.shape) != tuple(slot.shape):
                raise ValueError(f"step returned {tuple(out.shape)}, expected {tuple(slot.shape)}")
            slot.copy_(out)
        if gathering and mode == "overlap":
            info["gathers"] += 1
            info["gather_bytes"] += slot.numel()
            pending.append(sh.gather_frames(slot, world * b, dst=dst, group=group, async_op=True, counts=[b] * world))
            if len(pending) > 2:
                got[0] = pending.pop(0)()

    def finish():
        while pending:
            got[0] = pending.pop(0)()
        if gathering and mode == "end":
            info["gathers"] += 1
            info["gather_bytes"] += n_end * int(np.prod(frame))
            got[0] = sh.gather_frames(keep[:n_end], world * n_end, dst=dst, group=group, counts=[n_end] * world)

    # warm-up, all outside the timing: first - once - the end-of-region collective in the very shape the timed region issues it
    # (communicator set-up, the receive buffer's first allocation), THEN the steps, so that nothing but the barrier lies between
    # the last warm-up step and the first timed one (the chip loses its clock within milliseconds of idling: DESIGN.md section 6)
    if gathering and mode == "end":
        finish()
    if sh.dist_on():
        barrier()                         # the ranks start their warm-up steps together, so none idles long at the barrier behind them
    for k in range(warmup):
        one(k)
    while pending:                        # mode "overlap": the warm-up steps' own gathers
        got[0] = pending.pop(0)()
    got[0] = None
    info["gathers"], info["gather_bytes"] = 0, 0
    barrier()
    t0 = time.perf_counter()
    m0 = mark()
    for k in range(steps):
        one(k)
    m1 = mark()
    finish()
    m2 = mark()
    barrier()
    dt = time.perf_counter() - t0
    info["t0"], info["t1"] = t0, t0 + dt          # host clock (time.perf_counter) at both ends of the timed region
    info["compute_ms"] = elapsed(m0, m1) * 1e3
    info["gather_ms"] = elapsed(m1, m2) * 1e3
    info["local_s"] = dt
    return _max_over_ranks(dt, group, device), got[0], info
