"""Batched AdaIN engine: many frames / views, one style — the shape of the reference's two batch callers
(video/utils.py:327-350 per-frame loop; Style_3DGS/train.py:86-115 per-view loop), which call
``adain_inference`` once per image and re-encode the same style every time.

The engine keeps the packed weights and the style's channel statistics (2 x 512 floats) resident in
HBM and runs encoder -> fused AdaIN/blend -> decoder [-> mask composite] [-> uint8] for a batch of
frames that is already on the GPU.  Sub-batches bound the activation workspace (the full-resolution
activations are 256 B per pixel and frame).  Everything is launched on the current HIP stream.
"""
import torch

from . import runtime as rt


class Style:
    """What a call is styled with: the channel statistics ``mean`` / ``std``, float32 [K,512] on the device (K > 1: the rows that a call's
    ``style_weights`` mix), and ``pixels``: None, or the resized style's pixels (``set_style_image``).  Unpacks as ``mean, std = style``."""
    __slots__ = ("mean", "std", "pixels")

    def __init__(self, mean, std, pixels=None):
        self.mean, self.std, self.pixels = mean, std, pixels

    def __iter__(self):
        return iter((self.mean, self.std))

    k = property(lambda self: self.mean.shape[0])

    @staticmethod
    def check_count(k):
        if not 1 <= k <= rt.MIX_MAX_STYLES:
            raise rt.AdainHipError(f"set_styles: 1 .. {rt.MIX_MAX_STYLES} styles, got {k}")

    @classmethod
    def stack(cls, styles):                # the rows of single-row styles, in order, as one style to mix (no pixels)
        styles = list(styles)
        cls.check_count(len(styles))
        return cls(torch.cat([s.mean for s in styles]).contiguous(), torch.cat([s.std for s in styles]).contiguous())


class AdaINEngine:
    def __init__(self, vgg_state_dict, decoder_state_dict, device=None):
        if not torch.cuda.is_available():
            raise rt.AdainHipError("AdaINEngine needs a GPU (no CPU fallback)")
        self.device = torch.device(device) if device is not None else torch.device("cuda", torch.cuda.current_device())
        self.enc = rt.pack_encoder(vgg_state_dict, self.device)
        self.dec = rt.pack_decoder(decoder_state_dict, self.device)
        self.style = None                 # the ``Style`` that calls are styled with: set_style / set_style_image / set_styles

    def synchronize(self):
        torch.cuda.synchronize(self.device)

    @staticmethod
    def abi_calls():
        """C-ABI compute calls this process has made so far (the job drivers report the difference per job)."""
        return rt.ABI_CALLS[0]

    def mark(self):
        """A time stamp on the current stream (a HIP event); ``elapsed(a, b)`` gives the seconds between two of them once the
        work in between has finished.  The job drivers time their phases with these instead of synchronising per phase."""
        e = torch.cuda.Event(enable_timing=True)
        e.record(torch.cuda.current_stream(self.device))
        return e

    def elapsed(self, a, b):
        b.synchronize()
        return a.elapsed_time(b) * 1e-3

    def style_stats(self):
        return self.style

    def use_style_stats(self, stats):
        """Switches to a ``Style`` obtained earlier from ``style_stats`` or a plain (mean, std) pair (the job drivers keep one per style)."""
        self.style = stats if isinstance(stats, Style) else Style(*stats)
        return self

    def set_style(self, style):
        """style [1,3,hs,ws] (or [1,4,...]: the alpha channel is dropped as in test.py:60-61)."""
        if style.shape[1] == 4:
            style = style[:, :3]
        self.style = Style(*rt.mean_std(rt.encode(style.to(self.device, torch.float32).contiguous(), self.enc), True))
        return self

    def set_styles(self, styles):
        """A list of K style tensors (each as ``set_style`` takes it, sizes may differ) for style interpolation: every style is
        encoded once and the engine holds their statistics as [K,512] rows, mixed per frame by the ``style_weights`` of
        ``stylize`` / ``stylize_depth`` / ``stylize_u8``."""
        styles = list(styles)
        Style.check_count(len(styles))
        self.style = Style.stack([self.set_style(s).style for s in styles])
        return self

    def set_style_image(self, style):
        """``set_style`` that also keeps the (already resized) style's PIXELS on the device, for ``preserve_color=True``: there every
        frame is styled with its own ``coral(style, frame)`` (function.py:26-67), so the pixels are needed, not only the statistics.
        style: float [1,3,hs,ws] (or [1,4,...], alpha dropped) or uint8 [1,hs,ws,3]."""
        style = style.to(self.device)
        style = style.contiguous() if style.dtype == torch.uint8 else style[:, :3].to(torch.float32).contiguous()
        self.style = Style(*rt.mean_std(self._encode(style), True), style)
        return self

    def _call_style(self, content, preserve_color, style_weights):
        """THE place that decides what a call is styled with -> (mean, std, the keywords ``rt.stylize_u8`` takes with them): the engine's
        one style ({}), its K styles mixed by ``style_weights`` (on the device), or - ``preserve_color`` - one recoloured style per frame
        ({"style_n": n}): coral(style, frame_i) for every frame of the sub-batch ``content`` in one call, through the encoder, their channel
        statistics (test.py:201-202 then :77; a frame's row depends on that frame alone).  Every refusal comes before any C-ABI call."""
        style = self.style
        if style is None:
            raise rt.AdainHipError("set_style() first")
        if style_weights is not None:
            if preserve_color:
                raise rt.AdainHipError("preserve_color with style_weights is not supported: it would need coral(style_k, frame) of every "
                                       "style for every frame")
            return style.mean, style.std, {"style_weights": torch.as_tensor(style_weights, dtype=torch.float32).to(self.device).contiguous()}
        if style.k != 1:
            raise rt.AdainHipError(f"the engine holds {style.k} styles (set_styles): pass style_weights to mix them")
        if not preserve_color:
            return style.mean, style.std, {}
        if style.pixels is None:
            raise rt.AdainHipError("preserve_color needs the style's pixels: set_style_image() first")
        recoloured, _record = rt.coral(style.pixels, content)
        return rt.mean_std(rt.encode(recoloured, self.enc), True) + ({"style_n": content.shape[0]},)

    def features(self, images):
        return self._encode(images.to(self.device))

    def _encode(self, content):
        """float NCHW [n,3,h,w] in [0,1], or decoded frames uint8 NHWC [n,h,w,3] (ToTensor then runs inside the first layer's
        kernel: same features bit for bit, a quarter of the bytes)."""
        if content.dtype == torch.uint8:
            return rt.encode_u8(content.contiguous(), self.enc)
        return rt.encode(content.to(torch.float32).contiguous(), self.enc)

    @staticmethod
    def frame_size(content):
        """(h, w) of a content batch in either form (float NCHW / uint8 NHWC)."""
        return tuple(content.shape[1:3]) if content.dtype == torch.uint8 else tuple(content.shape[-2:])

    def stylize(self, content, alpha=0.5, pmap=None, preserve_color=False, style_weights=None):
        """content [n,3,h,w] float (or [n,h,w,3] uint8) on the GPU -> stylised [n,3,8*hc,8*wc].  ``pmap`` [1|n,1,hc,wc] switches
        to the depth-aware blend (test.py:70); otherwise the alpha blend (test.py:80).  ``preserve_color``: every frame is styled
        with ``coral(style, frame)`` (``set_style_image`` first) instead of the style itself.  ``style_weights`` ([K], [n,K],
        [K,hc,wc] or [n,K,hc,wc], used as given): every frame is styled with that mix of the K styles of ``set_styles``
        (style interpolation, ``rt.blend_mix``)."""
        assert 0.0 <= alpha <= 1.0
        if preserve_color:
            content = content.to(self.device) if content.dtype == torch.uint8 else content.to(self.device, torch.float32)
        s_mean, s_std, how = self._call_style(content, preserve_color, style_weights)
        f = self._encode(content)
        c_mean, c_std = rt.mean_std(f, True)
        if "style_weights" in how:
            g = rt.blend_mix(f, True, c_mean, c_std, s_mean, s_std, how["style_weights"], alpha=alpha if pmap is None else None, pmap=pmap)
        elif pmap is not None:
            g = rt.blend_pmap(f, True, c_mean, c_std, s_mean, s_std, pmap)
        else:
            g = rt.blend_alpha(f, True, c_mean, c_std, s_mean, s_std, alpha)
        return rt.decode(g, self.dec)

    def stylize_u8(self, frames_u8, alpha=0.5, depth_maps=None, offset=0.15, prominence=20, masks=None, out=None, preserve_color=False,
                   style_weights=None):
        """A sub-batch of decoded frames uint8 [n,h,w,3] -> finished uint8 frames [n,H,W,3] in ONE call of the C ABI
        (``adain_stylize_u8``): what ``stylize`` / ``stylize_depth`` -> ``composite`` -> ``to_u8`` give, byte for byte, with one
        Python -> C transition per sub-batch instead of eight (the job drivers' launching thread is what eight ranks share).
        ``preserve_color``: coral -> encoder -> statistics of the n recoloured styles first (three more calls), then the same one
        call with one style per frame (``adain_stylize_u8_ex``); a frame's bytes do not depend on the sub-batch it is in.
        ``style_weights``: the mix of ``set_styles``' K styles per frame, as for ``stylize`` (``adain_stylize_u8_mix``, still one call)."""
        assert 0.0 <= alpha <= 1.0 and 0.0 <= offset <= 1.0
        if depth_maps is not None:
            depth_maps = [d.to(self.device, torch.float32) for d in depth_maps]
        if masks is not None:
            masks = masks.to(self.device)
            if masks.dtype not in (torch.uint8, torch.bool, torch.float32):
                masks = masks.float()
        frames_u8 = rt.device_tensor(frames_u8.to(self.device), "frames", torch.uint8)
        s_mean, s_std, how = self._call_style(frames_u8, preserve_color, style_weights)
        return rt.stylize_u8(frames_u8, self.enc, self.dec, s_mean, s_std, alpha, depth_maps, offset, prominence, masks, out, **how)

    def stylize_depth(self, content, depth_maps, offset=0.15, prominence=20, preserve_color=False, style_weights=None):
        """Depth-aware path for a batch: ``depth_maps`` is a list of [h0,w0] GPU tensors, one per frame."""
        assert 0.0 <= offset <= 1.0
        h, w = self.frame_size(content)
        hc, wc = rt.encoded_size(h, w)
        p = torch.cat([rt.strength_map(d, hc, wc, offset, prominence) for d in depth_maps])
        return self.stylize(content, pmap=p, preserve_color=preserve_color, style_weights=style_weights)

    def composite(self, content, stylized, masks):
        """masks [n|1, 1|3, hm, wm] float -> content*(1-m) + resize(stylized)*m (test.py:222-236)."""
        content = content.to(self.device)
        content = rt.u8_to_f32(content.contiguous()) if content.dtype == torch.uint8 else content.to(torch.float32).contiguous()
        size = tuple(content.shape[-2:])
        # F.interpolate to the size a tensor already has is the identity for both modes (nearest: index i -> i; bilinear with
        # align_corners=False: source coordinate i exactly, weight 0 on the neighbour), so equal sizes skip the two resize passes
        # (24 B per pixel each): the usual case - frames whose sides are multiples of 8, masks made from the frame itself
        m = masks.to(self.device, torch.float32).contiguous()
        if tuple(m.shape[-2:]) != size:
            m = rt.resize_nearest(m, size)
        s = stylized if tuple(stylized.shape[-2:]) == size else rt.resize_bilinear(stylized, size)
        return rt.mask_composite(content, s.contiguous(), m)

    def to_u8(self, images, out=None):
        return rt.quantize_u8(images, out)

    def resize_area_u8(self, frames_u8, dsize):
        """cv2.resize(frame, dsize, interpolation=cv2.INTER_AREA) per frame (video/utils.py:352-353); dsize = (width, height)."""
        return rt.resize_area_u8(frames_u8, dsize)

    def resize_pil_u8(self, frames_u8, size, resample=rt.PIL_BILINEAR, crop=None, out=None):
        """``PIL.Image.resize(size, resample)`` per uint8 frame for any of Pillow's six filters, bit for bit (``runtime.resize_pil_u8``:
        tap tables from the host, two passes on the device); size = (width, height)."""
        return rt.resize_pil_u8(frames_u8, size, resample, crop, out)

    def warp_blend_u8(self, cur, prev, flow, alpha=0.7):
        """One step of the video recurrence: blend(cur, warp(prev, flow), alpha) on uint8 HWC frames (video/utils.py:89-105, :223-229)."""
        return rt.warp_blend_u8(cur, prev, flow, alpha)

    def jpeg_encode_u8(self, frames_u8, quality=rt.JPEG_DEFAULT_QUALITY, subsampling=2, optimize=False, progressive=False):
        """The files ``PIL.Image.fromarray(frame).save(f, format="JPEG", quality=quality, subsampling=subsampling, optimize=optimize)``
        writes (with ``progressive``: the same call with ``progressive=True``) for uint8 frames [n,h,w,3|1] on the device, encoded there
        (adain_jpeg_encode_u8 at the defaults, else adain_jpeg_encode_opt_u8 or adain_jpeg_encode_progressive_u8; ``runtime.jpeg_encode_u8``) -> a list of n ``bytes``; only the files cross to the host."""
        return rt.jpeg_files(*rt.jpeg_encode_u8(frames_u8, quality, subsampling, optimize, progressive))

    def png_encode_u8(self, frames_u8, filter=None):
        """Finished uint8 frames [n,h,w,c] (c = 3: RGB, 1: L) on the device -> their PNG files (adain_png_encode_u8; ``runtime.png_encode_u8``:
        files any reader decodes to the frames' pixels, not Pillow's bytes) -> a list of n ``bytes``; only the files cross to the host."""
        return rt.png_files(*rt.png_encode_u8(frames_u8, filter))

    def quantize_palette_u8(self, frames_u8, K=256, per_frame=False, refine=0):
        """Frames uint8 [n,h,w,3] on the device -> (palettes uint8 [P,256,3], used int32 [P]) on the device: at most ``K`` colours chosen
        from the frames themselves, for all of them or ``per_frame``, with ``refine`` rounds of k-means behind the median cut
        (adain_quantize_palette_u8; ``runtime.quantize_palette_u8``)."""
        return rt.quantize_palette_u8(frames_u8, K, per_frame, refine)

    def image_metrics(self, a, b, ssim_map=False):
        """Two clips on the device, uint8 [n,h,w,1|3] or float32 [n,1..4,h,w] -> their per-frame SSIM (window 11), MSE, L1 and PSNR as
        float64 [n] device tensors, with ``ssim_map`` the map as well (adain_image_metrics_u8 / adain_image_metrics_f32;
        ``runtime.image_metrics``)."""
        return rt.image_metrics(a, b, ssim_map)

    def image_metrics_grad(self, a, b, weights, grad_b=False):
        """Two float32 clips [n,1..4,h,w] on the device and ``weights`` float64 [n,3], the upstream gradient of every frame's {ssim,
        mse, l1} -> the float32 gradient by ``a``, with ``grad_b`` (grad_a, grad_b) (adain_image_metrics_grad_f32;
        ``runtime.image_metrics_grad``)."""
        return rt.image_metrics_grad(a, b, weights, grad_b)

    def guide_l1(self, image, guide_u8, resampled=False):
        """A render float32 [n,3,h,w] and its guide views uint8 [n,gh,gw,3] on the device -> train.py's ``l1_loss`` against the guide
        bilinearly resized to the render, per frame as float64 [n], with ``resampled`` the resized guide as well (adain_guide_l1_f32;
        ``runtime.guide_l1``)."""
        return rt.guide_l1(image, guide_u8, resampled)

    def guide_l1_grad(self, image, guide_u8, weights):
        """The same inputs and ``weights`` float64 [n], the upstream gradient of every frame's l1 -> the float32 gradient by the render
        (adain_guide_l1_grad_f32; ``runtime.guide_l1_grad``)."""
        return rt.guide_l1_grad(image, guide_u8, weights)

    def gif_encode_u8(self, index_u8, K, delay_cs):
        """Palette index planes uint8 [n,h,w] on the device, every index below ``K`` -> the frames' GIF records (adain_gif_encode_u8;
        ``runtime.gif_encode_u8``) as (records, lengths) on the device; ``gif_file.assemble`` makes the file of them and only the records
        cross to the host."""
        return rt.gif_encode_u8(index_u8, K, delay_cs)

    def pixelize_u8(self, frames_u8, colors, method="rgb", grayscale=False, brightness=0, contrast=0):
        """Finished uint8 frames [n,h,w,3] (or [h,w,3]) on the device -> the palette page's grey / brightness / contrast / recolouring of
        them (``pixelize.frames_post``: adain_palette_map_u8, or adain_palette_dither_u8 for "floyd-steinberg-diffused" with its error rows in
        the stream's workspace), still on the device - ready for ``png_encode_u8``."""
        from . import pixelize
        return pixelize.frames_post(colors, method, grayscale, brightness, contrast)(rt.device_tensor(frames_u8, "pixelize_u8: frames", torch.uint8))

    def jpeg_decode_u8(self, files, chunk_bits=0, mode=None, report=None, restart=False, progressive=False):
        """The bytes of image files (a list, or one ``bytes``) -> uint8 tensors on the engine's device, the pixels Pillow's ``Image.open``
        gives: baseline JPEG files are decoded on the device (adain_jpeg_decode_restart_u8; with ``restart=True`` those with restart intervals as
        well, with ``progressive=True`` progressive files too: adain_jpeg_decode_progressive_u8), anything else by PIL as before
        (``rt.jpeg_decode_u8``)."""
        return rt.jpeg_decode_u8(files, self.device, chunk_bits, mode, report, restart, progressive)

    def png_decode_u8(self, files, mode=None, report=None):
        """The bytes of PNG files (a list, or one ``bytes``) -> uint8 tensors on the engine's device, the pixels Pillow's ``Image.open``
        gives: 8-bit non-interlaced grey, RGB and RGBA files are decoded on the device (adain_png_decode_u8), anything else by PIL as
        before (``rt.png_decode_u8``)."""
        return rt.png_decode_u8(files, self.device, mode, report)

    def gif_decode_u8(self, data, report=None):
        """The bytes of an animated GIF -> (frames uint8 [n,H,W,3] on the engine's device, ``gif_file.GifInfo``): the frames Pillow's
        ``ImageSequence.Iterator`` + ``convert("RGB")`` gives, decoded and composed on the device (adain_gif_decode_u8), by Pillow
        where the parser or a frame's status says so (``rt.gif_decode_u8``)."""
        return rt.gif_decode_u8(data, self.device, report)

    def jpeg_roundtrip_u8(self, frames_u8, quality=rt.JPEG_DEFAULT_QUALITY):
        """uint8 frames [n,h,w,3|1] on the device -> the frames Pillow decodes from the JPEG files it would save for them at ``quality``
        (what ``video._jpeg_roundtrip`` computes on the host), byte for byte, on the device (adain_jpeg_roundtrip_u8)."""
        return rt.jpeg_roundtrip_u8(frames_u8, quality)

    def colour_transfer_u8(self, fg, bg, out=None):
        """The localized pipeline's foreground colour transfer (localized_style_transfer.py:128-168) on uint8 HWC images -> (adjusted
        foreground, device record); see ``runtime.colour_transfer_u8``."""
        return rt.colour_transfer_u8(fg, bg, out)

    def localized_combine_u8(self, content, stylised, mask, out=None):
        """The localized pipeline's composite with the colour transfer inside (:232-238): content, stylised uint8 [h,w,3], {0,1} background
        mask uint8 [h,w] -> (final uint8 image, device record)."""
        return rt.localized_combine_u8(content, stylised, mask, out)

    def temporal_blend(self, frames_u8, flows, alpha=0.7):
        return temporal_blend(frames_u8, flows, alpha)


def precompute_guides(engine, views, names, output_dir, masks=None, content_size=512, crop=False, alpha=0.5,
                      depth_maps=None, depth_offset=0.5, depth_prominence=20, save_ext=".jpg", sub_batch=8, *, preserve_color=False,
                      jpeg_options=None):
    """Batched counterpart of the guide-image loop of the reference's Style_3DGS/train.py:86-115: every view
    is resized like ``adain_inference(content_size=...)`` does (test.py:190-200), stylised against the engine's
    current style, composited with its mask (``gt_image_np > 0``, train.py:97) and written to
    ``<output_dir>/<name><save_ext>`` — the same file naming, so the guide loss (train.py:208-221) reads it back
    unchanged.  ``views`` are PIL images (or paths); same-sized views are processed ``sub_batch`` at a time.
    ``preserve_color``: every view is styled with ``coral(style, view)`` (``engine.set_style_image`` first).  ``jpeg_options``
    (``runtime.JpegOptions``): how .jpg / .jpeg guides are saved; default: ``AdaIN.test``'s setting.  Returns {name: Path}."""
    from pathlib import Path

    import numpy as np
    from PIL import Image

    from .AdaIN.test import save_image, test_transform

    out_dir = Path(output_dir)
    out_dir.mkdir(exist_ok=True, parents=True)
    tf = test_transform(content_size, crop)
    tensors = []
    for v in views:
        if isinstance(v, (str, Path)):
            v = Image.open(str(v))
        t = tf(v)
        tensors.append(t[:3] if t.shape[0] == 4 else t)
    paths = {}
    i = 0
    while i < len(tensors):
        j = i + 1
        while j < len(tensors) and j - i < sub_batch and tensors[j].shape == tensors[i].shape:
            j += 1
        content = torch.stack(tensors[i:j]).to(engine.device)
        if depth_maps is not None:
            out = engine.stylize_depth(content, [d.to(engine.device, torch.float32) for d in depth_maps[i:j]], depth_offset,
                                       depth_prominence, preserve_color=preserve_color)
        else:
            out = engine.stylize(content, alpha, preserve_color=preserve_color)
        for k in range(i, j):
            img = out[k - i:k - i + 1]
            if masks is not None and masks[k] is not None:
                m = masks[k]
                m = m if isinstance(m, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(m))
                img = engine.composite(content[k - i:k - i + 1], img, m.float().unsqueeze(0))
            p = out_dir / f"{names[k]}{save_ext}"
            save_image(img, str(p), jpeg_options=jpeg_options)
            paths[names[k]] = p
        i = j
    return paths


def pooled_style_embedding(style_f):
    """[1,512,h,w] relu4_1 features -> [1,512] (reference Style_3DGS/train.py:80-84: adaptive_avg_pool2d + view)."""
    return style_f.float().mean(dim=(2, 3)).view(style_f.shape[0], style_f.shape[1])


def temporal_blend(frames_u8, flows, alpha=0.7):
    """Temporal-consistency post-pass of the video caller (reference video/utils.py:352-369): frame 0 is kept,
    frame i becomes blend(frame_i, warp(result_{i-1}, flow_{i-1}), alpha).  ``frames_u8`` [n,h,w,c] uint8 stylised
    frames already at the target resolution, ``flows`` [n-1,2,h,w] float32 (prev -> current, caller-supplied: the
    optical-flow estimator stays outside), both on the GPU.  The recurrence is sequential over frames, so it runs
    on one rank over the gathered frames; each step is one pixel kernel."""
    n = frames_u8.shape[0]
    if flows.shape[0] != max(n - 1, 0):
        raise rt.AdainHipError("temporal_blend: need one flow field per consecutive frame pair")
    out = torch.empty_like(frames_u8)
    if n:
        out[0].copy_(frames_u8[0])
    for i in range(1, n):             # one launch per frame, written straight into the result block (no intermediate, no copy kernel)
        rt.warp_blend_u8(frames_u8[i], out[i - 1], flows[i - 1], alpha, out=out[i])
    return out


class GraphedStylize:
    """The whole ``engine.stylize`` pass (about 30 kernel launches) captured once into a hipGraph and replayed with one
    launch per batch — for the reference's real-world sizes (256 or 512 pixel frames, video/utils.py:264,
    test.py:160) the per-kernel launch overhead of the eager path is a visible share of a 1-2 ms forward.
    Every C-ABI entry point only enqueues work on the given stream and neither allocates nor synchronises, which is
    what makes the capture legal.  The style must be set before capture (its statistics are baked into the graph's
    input buffers by reference, so ``engine.set_style`` followed by a new capture is needed to change it).  The graph
    holds raw addresses of the engine's packed weights and style statistics: the object keeps those tensors alive
    (``_keep``), so a later ``engine.set_style`` cannot hand their memory back to the allocator under a live graph."""

    def __init__(self, engine, n, h, w, alpha=0.5, to_u8=False):
        self.engine = engine
        self._keep = (engine.style, engine.enc, engine.dec)
        self.static_in = torch.zeros((n, 3, h, w), dtype=torch.float32, device=engine.device)
        side = torch.cuda.Stream(engine.device)
        side.wait_stream(torch.cuda.current_stream(engine.device))
        with torch.cuda.stream(side):            # warm-up outside the capture (lazy library state); the activation workspaces are
                                                 # keyed by stream, so the capture below allocates its own from the graph's pool
            for _ in range(2):
                out = engine.stylize(self.static_in, alpha)
                if to_u8:
                    out = engine.to_u8(out)
        torch.cuda.current_stream(engine.device).wait_stream(side)
        torch.cuda.synchronize(engine.device)
        self.graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(self.graph):
            out = engine.stylize(self.static_in, alpha)
            self.static_out = engine.to_u8(out) if to_u8 else out

    def __call__(self, content):
        """content [n,3,h,w] (GPU or pinned host tensor) -> the graph's output buffer (overwritten by the next call)."""
        self.static_in.copy_(content, non_blocking=True)
        self.graph.replay()
        return self.static_out
