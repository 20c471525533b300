"""Video style transfer on the MI355X AdaIN path — the caller of ``adain_inference`` in the reference's video/utils.py
(SURVEY.md 8(f) 3): ``apply_style_transfer_ada`` (:244-295) and ``apply_style_transfer_multi_ada`` (:297-372) with their
parameters, defaults, file naming and per-frame semantics:

    frame -> adain_inference(content_size=256, use_depth=True, depth_offset=offset, depth_prominence=prominence)
          -> cv2.resize(target_resolution, INTER_AREA)
          -> blend(stylized, warp(previous result, flow(previous frame -> frame)), alpha)     (from the second frame on)
          -> <output_dir>/<frame file name>

What runs where: the per-frame AdaIN forwards are independent and go through ``jobs.video_style_transfer_sharded`` (one rank,
or every rank of an initialised ``torch.distributed`` group: contiguous frame blocks, one gather); the INTER_AREA resize, the
flow warp and the blend are GPU pixel kernels; the frame-to-frame recurrence and the file writes run on rank 0.

What stays with the caller, because the reference gets it from libraries this package does not depend on:
  * the proximity maps: ``use_depth=True`` needs the depth provider (``AdaIN.test.set_depth_provider``; the reference pulls
    MiDaS through torch.hub per frame) — or pass ``depth_maps=``;
  * the optical flow: ``set_flow_provider(fn)`` with ``fn(prev_frame_path, frame_path, target_resolution, method) ->
    [2,H,W] float32`` (x then y displacement at the target resolution, what ``estimate_optical_flow`` returns for the two
    resized frames, :75-86, :322-358).  ``set_flow_provider(device_flow_provider)`` plugs in the package's own Farnebäck
    estimator (flow.py, csrc/flow.hip: the reference's ``cv2.calcOpticalFlowFarneback(..., 0.5, 5, 15, 3, 7, 1.5, 0)`` on the
    device); with it installed the rank-0 recurrence expands every frame once (flow.FlowSequence) instead of twice per pair.
    ``set_flow_provider(device_flow_provider_all)`` accepts both of the reference's method names: ``'farneback'`` as above and
    ``'dualtvl1'``, the package's Dual TV-L1 (tvl1.py, csrc/tvl1.hip: ``cv2.optflow.DualTVL1OpticalFlow_create().calc(prev, next,
    None)`` on the device); with it installed and ``'dualtvl1'`` rank 0 computes the clip's n-1 flows before the recurrence
    (tvl1.TVL1Sequence.batch: each frame prepared once, many pairs per launch).  With either installed, a method it does not
    serve is refused before any frame is stylised.
One deliberate difference: the reference writes every stylised frame as a JPEG into a temporary directory and reads it back
(:261-273); here the uint8 frames stay in memory unless ``intermediate_jpeg=True`` re-creates that lossy round trip - through PIL on
the host, or with ``jpeg_on_device=True`` on the GPU, where the whole batch becomes the pixels PIL would decode without a file being
made (csrc/jpeg.hip, adain_jpeg_roundtrip_u8: the same bytes).
"""
import contextlib
import contextvars
import io
import os
from pathlib import Path

import numpy as np
import torch
from PIL import Image

from . import gif_file
from . import jobs
from . import runtime as rt
from .AdaIN import test as adain_test

_flow_provider = None
# The input routes of the clip that is running on THIS thread; the default outside one.  The value is whatever answers
# ``read_rgb(path, device)``: the clip's rt.JpegRoutes - the default, and what a clip without ``png_decode_on_device`` sets, as before
# that switch existed - or, with ``png_decode_on_device``, the clip's whole rt.OutputRoutes, which asks the route that owns the path's
# extension.  Only the public flow providers read it: they are called as fn(prev, cur, resolution, method), also from a caller's
# wrapper, and decode as their clip does.  Everything else is handed the clip's value (the feeder's fetch threads inherit no context).
_routes = contextvars.ContextVar("video_input_routes", default=rt.JpegRoutes())
_IMAGE_EXT = (".jpg", ".jpeg", ".png")


def set_flow_provider(fn):
    """``fn(prev_frame_path, frame_path, target_resolution, method) -> [2,H,W] float32`` (numpy or torch).  None clears it."""
    global _flow_provider
    _flow_provider = fn


def estimate_optical_flow(prev_frame_path, frame_path, target_resolution, method="farneback"):
    if _flow_provider is None:
        raise RuntimeError("no optical-flow provider: call video.set_flow_provider(fn) (the reference uses OpenCV's Farnebäck / "
                           "DualTV-L1 estimators here, which this package does not depend on)")
    f = _flow_provider(prev_frame_path, frame_path, target_resolution, method)
    return torch.as_tensor(np.asarray(f) if not isinstance(f, torch.Tensor) else f, dtype=torch.float32)


@contextlib.contextmanager
def _routes_scope(routes):
    token = _routes.set(routes)
    try:
        yield
    finally:
        _routes.reset(token)


def _decode_gray(path, target_resolution, device, routes):
    """cv2.imread + cv2.resize(target_resolution) + COLOR_RGB2GRAY of the reference (video/utils.py:75-77, :330-332), on the
    device (flow.frames_to_gray).  Decoded with PIL, which does not apply the EXIF orientation cv2.imread applies (unpinned)."""
    from . import flow as fl

    rgb = routes.read_rgb(path, device)          # the same pixels, decoded where they are used
    if rgb is None:
        rgb = torch.from_numpy(np.array(Image.open(path).convert("RGB"))).to(device)
    return fl.frames_to_gray(rgb, target_resolution)


def device_flow_provider(prev_frame_path, frame_path, target_resolution, method="farneback"):
    """A flow provider (``set_flow_provider``) that runs the reference's Farnebäck call on the current GPU: both frames decoded,
    resized and converted as the reference does, then ``cv2.calcOpticalFlowFarneback(prev, cur, None, 0.5, 5, 15, 3, 7, 1.5, 0)``
    (flow.calc_optical_flow_farneback) -> [2,H,W] float32 on the device."""
    from . import flow as fl

    if method != "farneback":
        raise ValueError(f"device_flow_provider: optical-flow method {method!r} is not built in (DualTV-L1 is not; use 'farneback' or "
                         "install a provider of your own)")
    dev = torch.device("cuda", torch.cuda.current_device())
    prev, cur = (_decode_gray(p, target_resolution, dev, _routes.get()) for p in (prev_frame_path, frame_path))
    return fl.calc_optical_flow_farneback(prev, cur, None, 0.5, 5, 15, 3, 7, 1.5, 0).permute(2, 0, 1).contiguous()


def device_flow_provider_all(prev_frame_path, frame_path, target_resolution, method="farneback"):
    """A flow provider (``set_flow_provider``) for both of the reference's methods on the current GPU: ``'farneback'`` is exactly
    ``device_flow_provider``; ``'dualtvl1'`` decodes, resizes and converts both frames the same way and runs
    ``cv2.optflow.DualTVL1OpticalFlow_create().calc(prev, cur, None)`` (tvl1.DualTVL1OpticalFlow_create) -> [2,H,W] float32 on the
    device.  Any other name raises ValueError (the reference would fail with an unbound local there)."""
    if method == "farneback":
        return device_flow_provider(prev_frame_path, frame_path, target_resolution, method)
    if method != "dualtvl1":
        raise ValueError(f"device_flow_provider_all: unknown optical-flow method {method!r} (use 'farneback' or 'dualtvl1')")
    from . import tvl1

    dev = torch.device("cuda", torch.cuda.current_device())
    prev, cur = (_decode_gray(p, target_resolution, dev, _routes.get()) for p in (prev_frame_path, frame_path))
    return tvl1.DualTVL1OpticalFlow_create().calc(prev, cur, None).permute(2, 0, 1).contiguous()


# The package's own providers (by identity: a wrapper of one is an ordinary provider) and the methods each serves.  With one of them
# installed, rank 0 refuses any other method before stylising and runs the served method's sequence path (_flow_source).
_OWN_METHODS = {id(device_flow_provider): ("farneback",), id(device_flow_provider_all): ("farneback", "dualtvl1")}


def _flow_source(content_dir, names, flow_method, size, device, cancel_flag, routes):
    """The recurrence's flows: ``f(i)`` is the [2,H,W] device flow frame i-1 -> frame i, called for i = 1, 2, ... in order.  The
    package's own estimators decode and prepare every frame once, with the same bits as their providers per pair; any other
    provider is called per pair."""
    path = lambda k: os.path.join(content_dir, names[k])
    if flow_method not in _OWN_METHODS.get(id(_flow_provider), ()):
        return lambda i: estimate_optical_flow(path(i - 1), path(i), size, flow_method).to(device)
    gray = lambda k: _decode_gray(path(k), size, device, routes)
    with torch.cuda.device(device):
        if flow_method == "dualtvl1":
            # all n-1 flows before the recurrence, up to max_pairs pairs per call (chunks); None when cancelled
            from . import tvl1

            flows = tvl1.TVL1Sequence().batch([gray(k) for k in range(len(names))], cancel=cancel_flag)
            return lambda i: flows[i - 1]
        # Farneback: one pyramid per frame, streamed (never n-1 flows at once)
        from . import flow as fl

        seq = fl.FlowSequence(0.5, 5, 15, 3, 7, 1.5, 0)
        seq.push(gray(0))

    def push(i):
        with torch.cuda.device(device):
            return seq.push(gray(i))
    return push


def normalize_image(image):
    """uint8 -> float32 in [0,1] before blending (video/utils.py:217-221)."""
    return image.astype(np.float32) / 255.0 if image.dtype == np.uint8 else image


def blend_images(stylized, warped, alpha):
    """The reference's host blend (video/utils.py:223-229), numpy float32: what ``adain_warp_blend_u8`` computes after its warp."""
    blended = alpha * normalize_image(stylized) + (1 - alpha) * normalize_image(warped)
    return np.clip(blended * 255, 0, 255).astype(np.uint8)


def _frame_files(content_dir):
    return sorted(f for f in os.listdir(content_dir) if f.lower().endswith(_IMAGE_EXT))


def _jpeg_roundtrip(u8):
    out = np.empty_like(u8)
    for i, fr in enumerate(u8):
        buf = io.BytesIO()
        Image.fromarray(fr).save(buf, format="JPEG")          # PIL defaults, as torchvision's save_image(".jpg") uses them
        out[i] = np.asarray(Image.open(io.BytesIO(buf.getvalue())).convert("RGB"))
    return out


def _gif_request(path, fps, palette, method):
    """The GIF a clip also writes, settled before anything runs: None without a path."""
    if path is None:
        return None
    palette = gif_file.WEB if palette is None else palette
    gif_file.check_palette(palette)          # refuses a bad palette now
    gif_file.delay_of(fps)
    return {"path": str(path), "fps": fps, "palette": palette, "method": gif_file.default_method(palette) if method is None else method}


def frames_to_gif(image_folder, output_gif, fps=20, palette=gif_file.WEB, method=None, routes=None):
    """The frames of ``image_folder`` (sorted by name, one size) as one animated GIF: the counterpart of the reference's ``frames_to_video``
    (video/utils.py:374-392, cv2's VideoWriter) in the container its results are shown in (Style_3DGS/render.py:29-33).  ``palette``,
    ``method``: ``gif_file.write_gif``'s (``"adaptive"`` / ``"adaptive-local"``: 256 colours chosen from the clip / from every frame; ``gif_file.adaptive``).  With a GPU the frames are read through ``routes`` (an ``rt.OutputRoutes``: decoded on the
    device where it says so, PIL otherwise), recoloured and coded there; without one PIL reads and writes.  Returns ``output_gif``."""
    names = _frame_files(image_folder)
    if not names:
        raise ValueError(f"frames_to_gif: no frames in {image_folder}")
    routes = rt.OutputRoutes() if routes is None else routes
    dev = torch.device("cuda", torch.cuda.current_device()) if torch.cuda.is_available() else None
    frames = []
    for name in names:
        path = os.path.join(image_folder, name)
        rgb = routes.read_rgb(path, dev) if dev is not None else None
        if rgb is None:
            rgb = torch.from_numpy(np.array(Image.open(path).convert("RGB")))
            rgb = rgb.to(dev) if dev is not None else rgb
        if frames and rgb.shape != frames[0].shape:
            raise ValueError(f"frames_to_gif: {name} is {tuple(rgb.shape[:2])}, the first frame {tuple(frames[0].shape[:2])}")
        frames.append(rgb)
    return gif_file.write_gif(torch.stack(frames), output_gif, palette, fps, method)


def _run_clip(content_dir, style_paths, output_dir, flow_method, alpha, target_resolution, cancel_flag, offset, prominence, engine,
              vgg_str, decoder_str, depth_maps, group, preserve_color, crossfade_frames, intermediate_jpeg, outputs, gif=None):
    from . import sharding as sh
    from .engine import AdaINEngine

    os.makedirs(output_dir, exist_ok=True)
    names = _frame_files(content_dir)
    rank, world = sh.rank_world(group)
    dev = engine.device if engine is not None else (torch.device("cuda", torch.cuda.current_device()) if torch.cuda.is_available() else None)
    # Everything that can stop the job is settled BEFORE any rank starts computing, with one status word, so that no rank is
    # ever left waiting in a collective for a peer that has returned or raised: cancellation (the flag is a per-process Event),
    # and the optical-flow provider the rank-0 recurrence will need from the second frame on (one of the package's own: and a
    # method it serves).
    cancelled = cancel_flag is not None and cancel_flag.is_set()
    need_flow = rank == 0 and len(names) > 1 and _flow_provider is None
    own = _OWN_METHODS.get(id(_flow_provider))
    bad_method = rank == 0 and len(names) > 1 and own is not None and flow_method not in own
    go = sh.agree_min(0 if need_flow or bad_method else 1 if cancelled else 2, group, dev)
    if go == 0:
        if need_flow:
            estimate_optical_flow(None, None, None)            # raises the "no optical-flow provider" error
        if bad_method:
            _flow_provider(None, None, None, flow_method)      # raises the provider's own refusal of the method
        raise RuntimeError("video style transfer: rank 0 has no optical-flow provider (video.set_flow_provider) or does not "
                           f"know the method {flow_method!r}")
    if go == 1:                                                # cancelled on some rank: every rank stops, as the reference loop does
        print("Stopping style transfer...")
        return None
    if len(names) == 0:                                        # an empty directory: the reference's loop is a no-op
        return Path(output_dir)
    if engine is None:
        engine = AdaINEngine(torch.load(vgg_str, map_location="cpu"), torch.load(decoder_str, map_location="cpu"))
    tf = adain_test.test_transform_u8(256, False)              # adain_inference(content_size=256) of the reference loop
    on_gpu = torch.device(engine.device).type == "cuda"
    stf = adain_test.test_transform(512, False)                # its default style_size

    class Frames:                                             # lazily: a rank opens only the frames of its own block
        def __len__(self):
            return len(names)

        def __getitem__(self, k):
            if on_gpu and (outputs.jpeg.decode_on_device or outputs.png.decode_on_device):
                # the file's bytes go up and are decoded there: Pillow's pixels (csrc/jpeg_decode.hip, csrc/png_decode.hip)
                with torch.cuda.device(engine.device):
                    rgb = outputs.read_rgb(os.path.join(content_dir, names[k]), engine.device)
                frame = adain_test.device_frame_transform_u8(rgb, 256, False) if rgb is not None else None
                if frame is not None:
                    return frame[0]
            img = Image.open(os.path.join(content_dir, names[k])).convert("RGB")
            if on_gpu:                                        # Resize(256) on the device, PIL's bytes exactly (csrc/resample.hip)
                return adain_test.device_transform_u8(img, 256, False, engine.device)[0]
            return tf(img)

    class Depths:
        def __len__(self):
            return len(names)

        def __getitem__(self, k):
            if depth_maps is not None:
                return torch.as_tensor(depth_maps[k], dtype=torch.float32)
            return torch.as_tensor(adain_test.midas_depth_map_est(Image.open(os.path.join(content_dir, names[k]))), dtype=torch.float32)

    styles = [stf(Image.open(p).convert("RGB")).unsqueeze(0) for p in style_paths]
    # stylise (sharded), resize to the target resolution on the owning rank, gather; the recurrence needs the flows: rank 0 only
    post = None
    if intermediate_jpeg and outputs.jpeg.encode_on_device and on_gpu:
        post = engine.jpeg_roundtrip_u8                        # the same bytes, computed where the batch is (adain_jpeg_roundtrip_u8)
    elif intermediate_jpeg:
        post = lambda u8: torch.from_numpy(_jpeg_roundtrip(u8.cpu().numpy())).to(u8.device)
    if crossfade_frames:        # the styles cross-fade in feature space where the schedule cuts: per-frame weights instead of an index
        which = {"style_weights": jobs.style_crossfade(len(names), len(styles), crossfade_frames)}
    else:
        which = {"style_of": jobs.style_schedule(len(names), len(styles))}
    frames_u8, info = jobs.stylize_frames_sharded(
        engine, Frames(), styles, **which, depth_maps=Depths(), depth_offset=offset,
        depth_prominence=prominence,
        post=(lambda u8: engine.resize_area_u8(post(u8) if post else u8, target_resolution)) if target_resolution is not None else post,
        out_hw=(int(target_resolution[1]), int(target_resolution[0])) if target_resolution is not None else None,
        group=group, preserve_color=preserve_color)
    err = None
    if rank == 0:
        # the frame-to-frame recurrence (video/utils.py:355-368) on the gathered frames; every frame is written by a worker
        # thread behind an asynchronous device -> host copy while the next frame's warp / blend is already running
        sink = jobs.FileSink(engine.device, routes=outputs)
        finals = []
        try:
            n, h, w, _ = frames_u8.shape
            prev = None
            flow_of = _flow_source(content_dir, names, flow_method, (w, h), frames_u8.device, cancel_flag, outputs) if n > 1 else None
            for i, name in enumerate(names):
                if cancel_flag is not None and cancel_flag.is_set():
                    print("Stopping style transfer...")
                    break
                cur = frames_u8[i]
                if prev is not None:
                    cur = engine.warp_blend_u8(cur.contiguous(), prev, flow_of(i), alpha)
                sink.write(cur.unsqueeze(0), [os.path.join(output_dir, name)])
                print(f"Stylized and saved: {os.path.join(output_dir, name)}")
                prev = cur
                if gif is not None:
                    finals.append(cur)
            if finals:                                         # the clip's final frames, still on the device, as one animated GIF
                gif_file.write_gif(torch.stack(finals), gif["path"], gif["palette"], gif["fps"], gif["method"])
        except Exception as e:
            err = e
        try:
            sink.close()
        except Exception as e:
            err = err or e
    ok = sh.agree(err is None, group, engine.device)             # the other ranks leave with rank 0 - or raise with it
    if err is not None:
        raise err
    if not ok:
        raise RuntimeError("video style transfer: the post-pass failed on rank 0")
    return Path(output_dir) if rank == 0 else None


def apply_style_transfer_ada(content_dir, style_image_path, output_dir, flow_method="farneback", alpha=0.7, target_resolution=None,
                             cancel_flag=None, offset=0.30, prominence=20, *, engine=None,
                             vgg_str="Style_3DGS/AdaIN/models/vgg_normalised.pth", decoder_str="Style_3DGS/AdaIN/models/decoder.pth",
                             depth_maps=None, intermediate_jpeg=False, group=None, jpeg_on_device=False, preserve_color=False,
                             jpeg_decode_on_device=False, jpeg_decode_progressive=False, jpeg_options=None, png_on_device=False, png_decode_on_device=False,
                             gif_path=None, gif_fps=20, gif_palette=None, gif_method=None):
    """One style for the whole clip (video/utils.py:244-295); keyword-only extras: a ready ``engine``, checkpoint paths,
    precomputed ``depth_maps``, the reference's lossy intermediate JPEG, a process group, ``preserve_color`` (every frame is styled with
    ``coral(style, frame)``, adain_inference's colour preservation, on the device) and the call's ``rt.JpegRoutes``, field by field:
    ``jpeg_on_device`` (.jpg / .jpeg frames are encoded on the device: the same files, jobs.FileSink; with ``intermediate_jpeg`` and the
    engine on a GPU that round trip runs on the device too, ``AdaINEngine.jpeg_roundtrip_u8``: the same frames), ``jpeg_decode_on_device``
    (baseline .jpg / .jpeg frames are decoded on the device, for the stylisation and for the package's flow providers: the pixels PIL
    decodes; any other file, and the sharded feeder of jobs.py, keep PIL), ``jpeg_decode_progressive`` (with it only: progressive frames
    too), ``jpeg_options`` (``jobs.JpegOptions`` or a (quality, subsampling, optimize) tuple: how the .jpg / .jpeg OUTPUT frames are saved
    on either route, default Pillow's default save; the ``intermediate_jpeg`` round trip stays quality 75 and 4:2:0 whatever they say).
    ``png_on_device`` (default off): .png frames are encoded on the device (the clip's ``rt.OutputRoutes``, jobs.FileSink): files of the
    same pixels, not Pillow's bytes.  ``png_decode_on_device`` (default off): 8-bit non-interlaced grey, RGB and RGBA .png frames are
    decoded on the device (``rt.png_decode_rgb_file``), for the stylisation and for the package's flow providers: the pixels PIL decodes;
    any other .png keeps PIL.
    ``gif_path`` (default None: nothing changes): rank 0 also keeps the clip's final frames on the device and writes them there as one
    animated GIF at the end (``gif_file.write_gif``: ``gif_fps``; ``gif_palette``, ``gif_file.header``'s forms, ``"adaptive"`` / ``"adaptive-local"`` for 256 colours
    chosen from the clip / from every frame, ``gif_file.adaptive(colors, local, refine)``'s strings for another count and rounds of k-means, None for the 6x6x6 cube ``"web"``; ``gif_method``, None for error diffusion onto the cube and the nearest colour onto any other palette)."""
    outputs = rt.OutputRoutes(rt.JpegRoutes(jpeg_on_device, jpeg_decode_on_device, jpeg_decode_progressive, jpeg_options), rt.PngRoute(png_on_device, None, png_decode_on_device))
    with _routes_scope(outputs if outputs.png.decode_on_device else outputs.jpeg):
        return _run_clip(content_dir, [style_image_path], output_dir, flow_method, alpha, target_resolution, cancel_flag, offset, prominence,
                         engine, vgg_str, decoder_str, depth_maps, group, preserve_color, 0, intermediate_jpeg, outputs,
                         _gif_request(gif_path, gif_fps, gif_palette, gif_method))


def apply_style_transfer_multi_ada(content_dir, style_dir, output_dir, flow_method="farneback", alpha=0.7, target_resolution=None,
                                   cancel_flag=None, offset=0.30, prominence=20, *, engine=None,
                                   vgg_str="Style_3DGS/AdaIN/models/vgg_normalised.pth",
                                   decoder_str="Style_3DGS/AdaIN/models/decoder.pth", depth_maps=None, intermediate_jpeg=False,
                                   group=None, jpeg_on_device=False, preserve_color=False, crossfade_frames=0, jpeg_decode_on_device=False,
                                   jpeg_decode_progressive=False, jpeg_options=None, png_on_device=False, png_decode_on_device=False,
                                   gif_path=None, gif_fps=20, gif_palette=None, gif_method=None):
    """The styles of ``style_dir`` (sorted) switch through the clip every ``frames // styles`` frames (video/utils.py:297-372).
    ``preserve_color``: as in ``apply_style_transfer_ada``; each style's pixels stay on the device next to its statistics.
    ``crossfade_frames`` (0, the default: the hard cuts of the reference): the styles cross-fade in feature space over that many
    frames centred on each switch (``jobs.style_crossfade``, style interpolation on the device; at most 16 styles, and not with
    ``preserve_color``).  ``jpeg_on_device``, ``jpeg_decode_on_device``, ``jpeg_decode_progressive``, ``jpeg_options``: the call's
    ``rt.JpegRoutes``, as in ``apply_style_transfer_ada`` (the options: the output files only, never the ``intermediate_jpeg`` round trip);
    ``png_on_device``, ``png_decode_on_device``, ``gif_path``, ``gif_fps``, ``gif_palette``, ``gif_method``: as there."""
    style_images = sorted(os.listdir(style_dir))
    if len(style_images) == 0:
        raise ValueError("No style images found in the style directory.")
    if crossfade_frames and preserve_color:
        raise ValueError("crossfade_frames mixes the styles of a frame; preserve_color is not supported with it")
    outputs = rt.OutputRoutes(rt.JpegRoutes(jpeg_on_device, jpeg_decode_on_device, jpeg_decode_progressive, jpeg_options), rt.PngRoute(png_on_device, None, png_decode_on_device))
    with _routes_scope(outputs if outputs.png.decode_on_device else outputs.jpeg):
        return _run_clip(content_dir, [os.path.join(style_dir, s) for s in style_images], output_dir, flow_method, alpha, target_resolution,
                         cancel_flag, offset, prominence, engine, vgg_str, decoder_str, depth_maps, group, preserve_color, int(crossfade_frames),
                         intermediate_jpeg, outputs, _gif_request(gif_path, gif_fps, gif_palette, gif_method))


def gif_to_frames(gif_path, output_dir, ext=".png", routes=None):
    """The frames of the animated GIF ``gif_path`` as ``frame_0000<ext>``, ... in ``output_dir``: the counterpart of the reference's
    ``video_to_frames`` (video/utils.py:24-42, cv2's VideoCapture) for the one clip container this package reads itself - the directory
    ``apply_style_transfer_ada`` wants.  With a GPU the clip is decoded there (``gif_file.read_gif``) and the files are written through a
    ``jobs.FileSink`` with ``routes`` (an ``rt.OutputRoutes``: ``png_on_device`` / ``jpeg_on_device`` files are encoded on the device);
    without one Pillow reads and writes.  Returns the clip's ``gif_file.GifInfo``."""
    from . import jobs

    os.makedirs(output_dir, exist_ok=True)
    frames, info = gif_file.read_gif(gif_path)
    paths = [os.path.join(str(output_dir), f"frame_{i:04d}{ext}") for i in range(len(frames))]
    if not isinstance(frames, torch.Tensor):
        for frame, path in zip(frames, paths):
            Image.fromarray(frame).save(path)
        return info
    sink = jobs.FileSink(frames.device, routes=rt.OutputRoutes() if routes is None else routes)
    try:
        step = max(1, (32 << 20) // (frames.shape[1] * frames.shape[2] * 3))
        for i in range(0, len(paths), step):
            sink.write(frames[i:i + step], paths[i:i + step])
    finally:
        sink.close()
    return info


def stylize_gif(gif_in, style, gif_out, **keywords):
    """Stylise an animated GIF: its frames are extracted into a temporary directory (``gif_to_frames``), run through
    ``apply_style_transfer_ada`` - ``apply_style_transfer_multi_ada`` when ``style`` is a directory - with ``gif_path=gif_out``, and the
    stylised frames come back as one GIF at the clip's own pace (``gif_fps`` from ``gif_file.clip_fps`` unless one is given).  ``keywords``:
    those of the function that runs, ``output_dir`` too (default: a second temporary directory).  Returns ``gif_out``."""
    import tempfile

    with tempfile.TemporaryDirectory() as work:
        frames_dir, output_dir = os.path.join(work, "frames"), keywords.pop("output_dir", os.path.join(work, "stylised"))
        info = gif_to_frames(gif_in, frames_dir)
        keywords.setdefault("gif_fps", gif_file.clip_fps(info))
        run = apply_style_transfer_multi_ada if os.path.isdir(str(style)) else apply_style_transfer_ada
        run(frames_dir, str(style), output_dir, gif_path=str(gif_out), **keywords)
    return gif_out
