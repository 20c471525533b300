"""AdaIN inference entry points — same names, positional order, defaults and return types as the
reference's Style_3DGS/AdaIN/test.py (file:line cited per function), running on hand-written
gfx950 kernels through the C ABI (include/adain_hip.h).  A GPU is required: there is no CPU path.

Differences that are deliberate and invisible to callers:
  * weights are loaded from disk once per (path, mtime) and packed once, not on every call
    (the reference reloads 94 MB per call, test.py:183-184);
  * the reference's batch callers call ``adain_inference`` once per frame / view with the SAME style (video/utils.py:341-350,
    Style_3DGS/train.py:101) and every call re-encodes it (test.py:63 / :77): here the style's 2 x 512 channel statistics are kept
    per (style file version | style image object, style_size, crop, encoder weights) and a plain RGB content image takes ONE
    C-ABI call (``adain_stylize_u8``); the bytes written are those of the call-by-call path (``set_style_cache(False)`` runs
    that path: tests compare the files);
  * torchvision / cv2 are not needed: ``test_transform`` and ``save_image`` are restated on PIL with
    torchvision 0.13 semantics (environment.yml:20);
  * the MiDaS depth estimator (test.py:84-116) is a pluggable provider (``set_depth_provider``):
    ``torch.hub`` needs the network; a caller-supplied callable or a precomputed depth map
    (``depth_map=`` keyword of ``adain_inference``) replaces it offline.
"""
import threading
import time
import weakref
from collections import OrderedDict
from pathlib import Path
from types import SimpleNamespace

import numpy as np
import torch
from PIL import Image

from .. import runtime as rt
from ..engine import Style
from . import net
from .function import adaptive_instance_normalization, calc_mean_std, coral  # noqa: F401


# ---------------------------------------------------------------------------------------------------------
# test_transform (test.py:16-24): Resize(size) -> [CenterCrop(size)] -> ToTensor, on PIL
# ---------------------------------------------------------------------------------------------------------
def _resize_size(w, h, size):
    # torchvision.transforms.Resize(int): shorter side -> size, longer side -> int(size * long / short)
    short, long_ = (w, h) if w <= h else (h, w)
    if short == size:
        return w, h
    new_short, new_long = size, int(size * long_ / short)
    return (new_short, new_long) if w <= h else (new_long, new_short)


def _center_crop(img, size):
    w, h = img.size
    if w < size or h < size:  # torchvision pads with 0 first
        pad_l, pad_t = max((size - w) // 2, 0), max((size - h) // 2, 0)
        canvas = Image.new(img.mode, (max(w, size), max(h, size)))
        canvas.paste(img, (pad_l, pad_t))
        img = canvas
        w, h = img.size
    top, left = int(round((h - size) / 2.0)), int(round((w - size) / 2.0))
    return img.crop((left, top, left + size, top + size))


def _to_tensor(img):
    # torchvision ToTensor: HWC uint8 -> CHW float32 / 255
    if img.mode in ("I", "I;16", "F"):
        arr = np.array(img, dtype=np.float32)[:, :, None]
        return torch.from_numpy(arr.transpose(2, 0, 1).copy())
    if img.mode == "1":
        img = img.convert("L")
    arr = np.asarray(img, dtype=np.uint8)
    if arr.ndim == 2:
        arr = arr[:, :, None]
    return torch.from_numpy(arr.transpose(2, 0, 1).copy()).float().div(255)


def test_transform(size, crop):
    def transform(img):
        if size != 0:
            img = img.resize(_resize_size(img.size[0], img.size[1], size), Image.BILINEAR)
        if crop:
            img = _center_crop(img, size)
        return _to_tensor(img)

    return transform


test_transform.__test__ = False  # not a pytest test


def test_transform_u8(size, crop):
    """``test_transform`` without its last step: the resized / cropped RGB image as uint8 HWC (numpy).  ToTensor (``/ 255``) then
    runs on the device (``adain_encode_u8`` / ``adain_u8_to_f32``, bit-identical), so a frame crosses PCIe as 3 bytes per pixel.
    Images that are not plain RGB (RGBA, L, ...) come back as the float tensor ``test_transform`` gives."""
    def transform(img):
        if size != 0:
            img = img.resize(_resize_size(img.size[0], img.size[1], size), Image.BILINEAR)
        if crop:
            img = _center_crop(img, size)
        return np.asarray(img, dtype=np.uint8) if img.mode == "RGB" else _to_tensor(img)

    return transform


test_transform_u8.__test__ = False


# ---- test_transform on the device (round 5): the decoded RGB bytes go up as they are, Resize [+ CenterCrop] run as ONE kernel that
# reproduces PIL.Image.resize(BILINEAR) bit for bit (csrc/resample.hip, adain_resize_pil_bilinear_u8), ToTensor happens inside the
# encoder's first layer.  What stays on the host: opening / decoding the file (PIL) and the copy of its pixels into a pinned buffer.
_staging = threading.local()      # per thread (the job feeders fetch frames on a pool): {device index: [pinned uint8 buffer, event after its last upload]}


def _upload_rgb(img, device, mark=None):
    """The pixels of an RGB PIL image as a uint8 [1,h,w,3] device tensor: ``tobytes`` into this thread's pinned staging buffer
    (grown on demand, reused once its previous upload has finished), one asynchronous copy on the current stream."""
    w, h = img.size
    raw = img.tobytes()
    n = len(raw)
    idx = device.index if device.index is not None else torch.cuda.current_device()
    slots = _staging.__dict__.setdefault("slots", {})
    slot = slots.get(idx)
    if slot is None or slot[0].numel() < n:
        slot = slots[idx] = [torch.empty(max(n, 1 << 22), dtype=torch.uint8).pin_memory(), None]
    if slot[1] is not None:
        slot[1].synchronize()
    slot[0].numpy()[:n] = np.frombuffer(raw, dtype=np.uint8)
    with torch.cuda.device(device):
        x = torch.empty((1, h, w, 3), dtype=torch.uint8, device=device)
        if mark is not None:
            mark()                              # (stage timer: the device work of a call starts here)
        x.view(-1).copy_(slot[0][:n], non_blocking=True)
        slot[1] = torch.cuda.Event()
        slot[1].record()
    return x


def _transform_window(w, h, size, crop):
    """((new width, new height), crop window | None) of ``test_transform(size, crop)`` for a w x h image; None when torchvision's
    CenterCrop would have to pad (an image smaller than the crop: the host path handles it)."""
    nw, nh = _resize_size(w, h, size) if size != 0 else (w, h)
    if not crop:
        return (nw, nh), None
    if nw < size or nh < size:
        return None
    return (nw, nh), (int(round((nh - size) / 2.0)), int(round((nw - size) / 2.0)), size, size)


def _device_plan(w, h, size, crop):
    """((new width, new height), crop window | None) when the device runs ``test_transform_u8(size, crop)`` of a w x h RGB image, else None."""
    plan = _transform_window(w, h, size, crop)
    if plan is None:
        return None
    (nw, nh), _ = plan
    if w > 256 * nw or h > 256 * nh:            # beyond the device resize's supported shrink factor: Pillow on the host
        return None
    return plan


def _device_resize(x, w, h, plan):
    """uint8 [1,h,w,3] on the device -> Resize [+ CenterCrop] of ``plan`` there."""
    (nw, nh), win = plan
    if (nw, nh) == (w, h):                      # Image.resize to the size it has is a copy
        if win is None:
            return x
        return x[:, win[0]:win[0] + win[2], win[1]:win[1] + win[3]].contiguous()
    return rt.resize_pil_bilinear_u8(x, (nw, nh), crop=win)


def device_transform_u8(img, size, crop, device, mark=None):
    """``test_transform_u8(size, crop)(img)`` for an RGB PIL image, computed on the device: uint8 [1,h,w,3], byte for byte what PIL's
    resize + crop give (tests/test_gpu_resize_pil.py).  None for anything else (RGBA, L, ...: Pillow resizes those through other
    paths - premultiplied alpha for RGBA -, they keep the host transform)."""
    if getattr(img, "mode", None) != "RGB":
        return None
    plan = _device_plan(img.size[0], img.size[1], size, crop)
    if plan is None:
        return None
    return _device_resize(_upload_rgb(img, device, mark), img.size[0], img.size[1], plan)


def device_frame_transform_u8(rgb, size, crop):
    """``device_transform_u8`` of a frame that is on the device already, uint8 [h,w,3] (a file decoded there): uint8 [1,h',w',3], or
    None when the transform is not the device's."""
    h, w = rgb.shape[:2]
    plan = _device_plan(w, h, size, crop)
    return _device_resize(rgb[None], w, h, plan) if plan is not None else None


def device_decode_transform_u8(path, size, crop, device, mark=None):
    """``device_transform_u8`` of the image file at ``path`` without PIL, when ``_routes`` decode its format on the device
    (``set_device_jpeg_decode``, ``set_device_png_decode``): the file's bytes go up, the frame is decoded there (adain_jpeg_decode_u8,
    adain_png_decode_u8: Pillow's pixels) and resized there.  None when the file is not a three-channel colour file the decoder takes
    (a baseline JPEG, with ``set_device_jpeg_decode(True, progressive=True)`` a progressive one, an RGB PNG: PIL opens grey and RGBA
    files in modes that keep the host transform), or did not decode cleanly, or the transform is not the device's: the caller takes the
    PIL path."""
    fmt, options = _routes.decoder(path) or (None, None)
    read = rt.read_input(fmt, path, **options) if fmt is not None else None
    if read is None or read[0].c != 3:
        return None
    plan = _device_plan(read[0].w, read[0].h, size, crop)          # before anything is uploaded
    if plan is None:
        return None
    if mark is not None:
        with torch.cuda.device(device):
            mark()
    (_, frame, _, _), = rt.settle_decodes(fmt, [(path, *read)], device)
    return _device_resize(frame[None], read[0].w, read[0].h, plan) if frame is not None else None


def save_image(tensor, path, jpeg_options=None):
    """torchvision.utils.save_image for one image (test.py:243-244): x*255 + 0.5, clamp, uint8, PIL save.
    The quantisation runs on the GPU (adain_quantize_u8).  ``jpeg_options`` (``runtime.JpegOptions``): how a .jpg / .jpeg file is
    saved, by PIL or (``set_device_jpeg``) on the device; None: ``set_jpeg_save_options``' value."""
    routes = _routes if jpeg_options is None else _routes.replace(jpeg=_routes.jpeg.replace(options=jpeg_options))
    if tensor.dim() == 3:
        tensor = tensor.unsqueeze(0)
    routes.write(rt.quantize_u8(tensor.float()[:1]), path)


# ---------------------------------------------------------------------------------------------------------
# weights: loaded once per (path, mtime, size)
# ---------------------------------------------------------------------------------------------------------
_loaded = {}


def _device():
    if not torch.cuda.is_available():
        raise rt.AdainHipError("no GPU visible: the AdaIN path runs only on the MI355X HIP kernels (no CPU fallback)")
    return torch.device("cuda", torch.cuda.current_device())


def _param_state(module):
    return tuple((p.data_ptr(), p._version) for p in module.parameters())


def _load_into(module, path, tag):
    """Loads the checkpoint at ``path`` into the module-level singleton unless exactly this file version is what the module
    currently holds: the cache entry also records the parameters' (storage, version) state after the load, so weights written
    into ``net.vgg`` / ``net.decoder`` by anyone else (another ``load_state_dict``, ``.to()``, in-place edits) invalidate it and
    results never depend on call order (the reference reloads on every call, test.py:183-184)."""
    p = Path(path)
    st = p.stat()
    key = (tag, str(p.resolve()), st.st_mtime_ns, st.st_size)
    if _loaded.get(tag) != (key, _param_state(module)):
        module.load_state_dict(torch.load(str(p), map_location="cpu"))
        _loaded[tag] = (key, _param_state(module))


# ---------------------------------------------------------------------------------------------------------
def _ready(module, device):
    """``module.eval().to(device)`` without the walk over ~50 child modules when there is nothing to do (a per-call cost the
    reference's callers pay once per frame)."""
    if module.training:
        module.eval()
    if any(p.device != device for p in module.parameters()):
        module.to(device)
    return module


def _singletons(device, vgg_str=None, decoder_str=None):
    """The module-level encoder / decoder (net.vgg, net.decoder) in eval mode on ``device`` with the checkpoints at the
    given paths loaded (once per file version; the reference re-reads both files on every call, test.py:183-184)."""
    enc, dec = _ready(net.vgg, device), _ready(net.decoder, device)          # move first: .to() replaces the parameter storages
    if vgg_str is not None:
        _load_into(enc, vgg_str, "vgg")
    if decoder_str is not None:
        _load_into(dec, decoder_str, "decoder")
    return enc, dec


def _as_batch(img, size, crop, device, rgb_only=False):
    """PIL image -> [1,C,H,W] float tensor on ``device`` through ``test_transform(size, crop)``."""
    x = test_transform(size, crop)(img).to(device).unsqueeze(0)
    return x[:, :3] if (rgb_only and x.shape[1] == 4) else x


# ---------------------------------------------------------------------------------------------------------
# style cache: what the encoder made of a style image, kept across calls with the same style
# ---------------------------------------------------------------------------------------------------------
_STYLE_CACHE_SIZE = 16
_style_cache = OrderedDict()          # key -> (weakref to the style object | None, value)
_style_cache_lock = threading.Lock()  # the GUI callers run adain_inference on worker threads (one call at a time, but not one thread)
_style_cache_on = True
STYLE_ENCODES = [0]                   # style images encoded by adain_inference / get_style_embeddings so far (tests count it)


_latency_schedule_on = False


def set_latency_schedule(enabled):
    """True: ``adain_inference`` runs its C-ABI calls under ADAIN_SCHEDULE_LATENCY (include/adain_hip.h): the 3x3 layers that one
    small frame leaves under-filled - conv4_1, the decoder's first and fifth layer of a 256-class frame, the reference video loop's
    size (video/utils.py:261-270) - are split along cin.  About 10 % less kernel time for one 256 x 456 frame; the files then differ
    from the batch jobs' (and from the default's) by one LSB in a few bytes per thousand.  Default False: a frame's bytes do not
    depend on how it was batched.  Returns the previous setting."""
    global _latency_schedule_on
    prev, _latency_schedule_on = _latency_schedule_on, bool(enabled)
    return prev


_routes = rt.OutputRoutes()           # who writes (and decodes) the files of ``adain_inference``, the cached per-call path and ``save_image``


def output_routes():
    return _routes


def set_output_routes(routes):
    """All of ``adain_inference``'s file routes at once: a ``runtime.OutputRoutes``, a dict of its keywords, or None for the defaults (PIL
    everywhere, Pillow's default save).  Every setter below changes fields of it.  Returns the previous value."""
    global _routes
    prev, _routes = _routes, rt.OutputRoutes.of(routes)
    return prev


def jpeg_routes():
    return _routes.jpeg


def set_jpeg_routes(routes):
    """The JPEG routes alone: a ``runtime.JpegRoutes``, a dict of its keywords, or None for the defaults.  Returns the previous value."""
    return set_output_routes(_routes.replace(jpeg=routes)).jpeg


def set_device_png(enabled):
    """``adain_inference`` (the cached per-call path and ``save_image``) encodes a ``.png`` output (``save_ext=".png"``) on the device - a
    file of the same pixels, not Pillow's bytes (``runtime.png_encode_u8``) - and brings over the file instead of the raw frame.  An RGBA
    or host frame keeps PIL.  Default False.  Returns the previous setting."""
    return set_output_routes(_routes.replace(png=_routes.png.replace(encode_on_device=enabled))).png.encode_on_device


def set_device_png_decode(enabled):
    """``decode_on_device`` of the .png route: the cached per-call path of ``adain_inference`` decodes a content given as a ``.png`` path on
    the device (the pixels PIL decodes) and resizes it there.  A file the decoder does not take (png_file.parse), a grey or RGBA file, one
    that does not decode cleanly and a PIL image take the PIL path as before.  Default False.  Returns the previous setting."""
    return set_output_routes(_routes.replace(png=_routes.png.replace(decode_on_device=enabled))).png.decode_on_device


def set_device_jpeg(enabled):
    """``encode_on_device``: ``adain_inference`` (the cached per-call path and ``save_image``) encodes a ``.jpg`` / ``.jpeg`` output on the
    device (the bytes PIL writes) and brings over the file instead of the raw frame.  Default False.  Returns the previous setting."""
    return set_jpeg_routes(_routes.jpeg.replace(encode_on_device=enabled)).encode_on_device


def set_jpeg_save_options(quality=rt.JPEG_DEFAULT_QUALITY, subsampling=2, optimize=False, progressive=False):
    """``options``: how ``adain_inference`` saves a ``.jpg`` / ``.jpeg`` output - Pillow's ``quality``, ``subsampling``, ``optimize`` and
    ``progressive`` (``runtime.JpegOptions``, which may be given in place of ``quality``), honoured by PIL and by the device encoder: the same file.
    The defaults are Pillow's default save.  Returns the previous value (a ``JpegOptions``)."""
    new = rt.JpegOptions(quality, subsampling, optimize, progressive) if isinstance(quality, int) else quality
    return set_jpeg_routes(_routes.jpeg.replace(options=new)).options


def set_device_jpeg_decode(enabled, progressive=False):
    """``decode_on_device``: the cached per-call path of ``adain_inference`` decodes a content given as a ``.jpg`` / ``.jpeg`` path on the
    device (the pixels PIL decodes; files with restart intervals too) and resizes it there.  A file the decoder does not take (grey, ...:
    jpeg_file.parse) or that does not decode cleanly, a PIL image and any other extension take the PIL path as before.
    ``decode_progressive`` (with ``enabled`` only): progressive files too.  Default False.  Returns the previous ``enabled``."""
    return set_jpeg_routes(_routes.jpeg.replace(decode_on_device=enabled, decode_progressive=progressive)).decode_on_device


_device_coral_on = False
STYLE_PIXEL_UPLOADS = [0]             # style images whose pixels the device CORAL path brought to the device (tests count it)


def set_device_coral(enabled):
    """True: ``adain_inference(preserve_color=True)`` takes the cached one-call path too: the resized style's PIXELS are kept on the
    device per style (``_style_key``), and every call runs ``coral(style, content)`` there (adain_coral), encodes the recoloured
    style, takes its statistics and styles the frame with them in ``adain_stylize_u8`` - nothing of it on the host.  The file is
    within one LSB of the default's (CORAL in float64 instead of float32).  Default False: CORAL runs on CPU tensors as in the
    reference (test.py:201-202) through the call-by-call path.  Returns the previous setting."""
    global _device_coral_on
    prev, _device_coral_on = _device_coral_on, bool(enabled)
    return prev


def _with_schedule(fn):
    import functools

    @functools.wraps(fn)
    def run(*args, **kwargs):
        if not _latency_schedule_on:
            return fn(*args, **kwargs)
        with rt.schedule(rt.SCHEDULE_LATENCY):
            return fn(*args, **kwargs)

    return run


def set_style_cache(enabled):
    """False: every ``adain_inference`` call re-encodes its style through the call-by-call path, as the reference does
    (test.py:63 / :77); True (default): the style's statistics are kept across calls.  Returns the previous setting."""
    global _style_cache_on
    prev, _style_cache_on = _style_cache_on, bool(enabled)
    return prev


def clear_style_cache():
    with _style_cache_lock:
        _style_cache.clear()


def _pixel_fingerprint(img):
    """A fingerprint of a PIL image's pixels that moves when the image is edited IN PLACE (paste / draw / a GUI reusing one buffer):
    the per-row and per-64-word-column wrap-around sums of ``img.tobytes()`` read as uint64 words - position-sensitive in both
    directions; the cost is the ``tobytes`` copy (about 1 ms for a 933 x 700 image) plus two streaming passes (0.2 ms).  (Pillow's
    zero-copy Arrow export would avoid the copy; it crashed on small images with Pillow 12.2 here, so it is not used.)
    None = cannot fingerprint (the style is then not cached)."""
    try:
        a = np.frombuffer(img.tobytes(), np.uint8)
        n8 = a.size // 8 * 8
        w = a[:n8].view(np.uint64)
        r = w.size // 64
        body = w[: r * 64].reshape(r, 64)
        return hash((body.sum(axis=0).tobytes(), body.sum(axis=1).tobytes(), w[r * 64:].tobytes(), a[n8:].tobytes()))
    except Exception:
        return None


def _style_key(style_img, what, style_size, crop, enc, device):
    """Cache key of a style image: a file by (resolved path, mtime, size) - a rewritten file is another style -, an image object
    by identity (guarded by a weak reference: a dead object's id may be reused) AND a fingerprint of its pixels (an object edited
    in place is another style: the reference re-encodes every call, test.py:63 / :77), plus everything else the result depends on:
    ``style_size``, ``crop``, the device, the launch schedule (statistics computed under ADAIN_SCHEDULE_LATENCY differ in the last
    bits) and the encoder's parameter state (``load_state_dict`` / ``.to()`` / in-place edits all change it).  None = not cacheable."""
    params = (str(device), bool(_latency_schedule_on)) + _param_state(enc)
    if type(style_img) == str or isinstance(style_img, Path):
        try:
            p = Path(style_img).resolve()
            st = p.stat()
        except OSError:
            return None, None
        return (what, "file", str(p), st.st_mtime_ns, st.st_size, int(style_size), bool(crop), params), None
    try:
        ref = weakref.ref(style_img)
    except TypeError:
        return None, None
    fp = _pixel_fingerprint(style_img)
    if fp is None:
        return None, None
    return (what, "object", id(style_img), fp, getattr(style_img, "size", None), getattr(style_img, "mode", None), int(style_size), bool(crop),
            params), ref


def _cached_style(style_img, what, style_size, crop, enc, device, make):
    """``make()`` once per style (see ``_style_key``); an LRU of ``_STYLE_CACHE_SIZE`` entries."""
    key, ref = _style_key(style_img, what, style_size, crop, enc, device) if _style_cache_on else (None, None)
    if key is not None:
        with _style_cache_lock:
            hit = _style_cache.get(key)
            if hit is not None and (hit[0] is None or hit[0]() is style_img):
                _style_cache.move_to_end(key)
                return hit[1]
    value = make()
    if key is not None:
        with _style_cache_lock:
            _style_cache[key] = (ref, value)
            while len(_style_cache) > _STYLE_CACHE_SIZE:
                _style_cache.popitem(last=False)
    return value


def get_style_embeddings(
    style_img,
    vgg_str="Style_3DGS/AdaIN/models/vgg_normalised.pth",
    style_size=512,
    crop=False,
):
    """relu4_1 features of the style image, [1,512,h,w] on the GPU (reference test.py:27-49; an alpha channel of
    the style is dropped, :46-47).  No ``no_grad`` needed: the HIP path builds no autograd graph.  The features of a style image
    object are kept (``set_style_cache``); every call returns its own copy."""
    device = _device()
    enc, _ = _singletons(device, vgg_str=vgg_str)

    def make():
        STYLE_ENCODES[0] += 1
        u8 = device_transform_u8(style_img, style_size, crop, device) if isinstance(enc, net.HipVGG) else None
        if u8 is not None:                       # RGB: resized on the device, ToTensor inside the first layer (bit-identical)
            return rt.encode_u8(u8, enc.packed(device)).permute(0, 3, 1, 2)
        return enc(_as_batch(style_img, style_size, crop, device, rgb_only=True))

    return _cached_style(style_img, "features", style_size, crop, enc, device, make).clone()


def style_transfer(vgg, decoder, content, style, depth_map, alpha=1.0, offset=0.15, prominence=20):
    """Depth-aware transfer (reference test.py:52-71): ``decoder(AdaIN * (1 - P) + content_f * P)`` with the
    strength map P from ``compute_stylization_strength_map``.  ``alpha`` is range-checked and otherwise unused,
    exactly as in the reference; a 4-channel style loses its alpha channel."""
    assert 0.0 <= alpha <= 1.0
    assert 0.0 <= offset <= 1.0
    f_content, f_style = _encode_both(vgg, content, style[:, :3, :, :] if style.shape[1] == 4 else style)
    strength = compute_stylization_strength_map(depth_map, tuple(f_content.shape[2:]), offset, prominence)
    return decoder(_adain_blend(f_content, f_style, pmap=strength))


def style_transfer_simple(vgg, decoder, content, style, alpha=0.5):
    """``decoder(AdaIN * alpha + content_f * (1 - alpha))`` (reference test.py:74-81)."""
    assert 0.0 <= alpha <= 1.0
    content_f, style_f = _encode_both(vgg, content, style)
    return decoder(_adain_blend(content_f, style_f, alpha=alpha))


def style_transfer_interpolated(vgg, decoder, content, styles, alpha=1.0, interpolation_weights=None):
    """Style interpolation, the reference's ``style_transfer(vgg, decoder, content, style, alpha, interpolation_weights)``
    (Style_3DGS/AdaIN/test_video.py:30-45): ``decoder(feat * alpha + content_f * (1 - alpha))`` with ``feat = sum_k w_k *
    AdaIN(content_f, style_f[k])`` accumulated in style order, in one kernel (``rt.blend_mix``).  ``styles``: [K,3,hs,ws], or a list
    of K tensors [3,h,w] / [1,3,h,w] of different sizes (the reference's batch needs one size).  ``interpolation_weights``: K Python
    floats, used as given (the upstream CLI divides them by their sum before it calls; this function, like the reference's, does not)."""
    from .function import _layout, _like

    assert (0.0 <= alpha <= 1.0)
    style_list = list(styles) if isinstance(styles, (list, tuple)) else [styles[i:i + 1] for i in range(styles.shape[0])]
    style_list = [s.unsqueeze(0) if s.dim() == 3 else s for s in style_list]
    if not interpolation_weights or len(interpolation_weights) != len(style_list):
        raise ValueError(f"style_transfer_interpolated: {len(style_list)} styles need as many interpolation_weights, got {interpolation_weights!r}")
    content_f = vgg(content)
    N, C = content_f.size()[:2]
    s_mean, s_std = Style.stack(Style(m.view(1, C), sd.view(1, C)) for m, sd in (calc_mean_std(vgg(s)) for s in style_list))
    c_mean, c_std = calc_mean_std(content_f)
    view, nhwc = _layout(content_f)
    weights = torch.tensor([float(w) for w in interpolation_weights], dtype=torch.float32, device=view.device)
    feat = rt.blend_mix(view, nhwc, c_mean.view(N, C), c_std.view(N, C), s_mean, s_std, weights, alpha=alpha)
    return decoder(_like(feat, nhwc))


def _encode_both(vgg, content, style):
    """``vgg(content), vgg(style)`` (test.py:57,63 / :76-77).  The package's encoder takes both in one pass over its layers
    (``HipVGG.forward_many``: same results bit for bit, one launch per layer); any other module is simply called twice."""
    if isinstance(vgg, net.HipVGG) and content.device == style.device and content.shape[1] == 3 and style.shape[1] == 3:
        return vgg.forward_many(content, style)
    return vgg(content), vgg(style)


def _adain_blend(content_f, style_f, alpha=None, pmap=None):
    """Fused adaptive_instance_normalization + feature blend (one pass over the feature map)."""
    from .function import _layout, _like

    assert (content_f.size()[:2] == style_f.size()[:2])
    N, C = content_f.size()[:2]
    s_mean, s_std = calc_mean_std(style_f)
    c_mean, c_std = calc_mean_std(content_f)
    view, nhwc = _layout(content_f)
    args = (view, nhwc, c_mean.view(N, C), c_std.view(N, C), s_mean.view(N, C), s_std.view(N, C))
    out = rt.blend_pmap(*args, pmap) if pmap is not None else rt.blend_alpha(*args, alpha)
    return _like(out, nhwc)


# ---------------------------------------------------------------------------------------------------------
# depth provider (reference: midas_depth_map_est, test.py:84-116)
# ---------------------------------------------------------------------------------------------------------
_depth_provider = None


def set_depth_provider(fn):
    """``fn(PIL.Image | np.ndarray) -> torch.Tensor [H0,W0]`` (proximity / inverse depth).  None restores the
    default (MiDaS_small through torch.hub, which needs network access)."""
    global _depth_provider
    _depth_provider = fn


def midas_depth_map_est(img):
    if _depth_provider is not None:
        return _depth_provider(img)
    device = _device()
    # default provider, as the reference: MiDaS_small via torch.hub (network); its BGR<->RGB swap
    # (test.py:101-102) is reproduced without cv2 by reversing the channel axis.
    midas = torch.hub.load("intel-isl/MiDaS", "MiDaS_small")
    midas_transforms = torch.hub.load("intel-isl/MiDaS", "transforms")
    midas.to(device)
    midas.eval()
    transform = midas_transforms.small_transform
    if isinstance(img, Image.Image):
        img = np.array(img)
    if img.ndim == 3 and img.shape[-1] == 3:
        img = img[:, :, ::-1].copy()
    input_batch = transform(img).to(device)
    with torch.no_grad():
        prediction = midas(input_batch)
        prediction = torch.nn.functional.interpolate(
            prediction.unsqueeze(1), size=img.shape[:2], mode="bicubic", align_corners=False
        ).squeeze()
    return prediction


def compute_stylization_strength_map(depth_map, encoder_size, offset=0.15, prominence=20):
    """Proximity map -> stylisation strength P [1,1,Hc,Wc] (test.py:119-150), one HIP call chain and no
    host synchronisation (the reference's ``if max_val > min_val`` runs on the device)."""
    Hc, Wc = encoder_size
    if not isinstance(depth_map, torch.Tensor):
        depth_map = torch.as_tensor(np.asarray(depth_map))
    depth_map = depth_map.to(device=_device(), dtype=torch.float32)
    return rt.strength_map(depth_map, int(Hc), int(Wc), offset, prominence)


# ---------------------------------------------------------------------------------------------------------
@_with_schedule
def adain_inference(
    content_img,
    style_img,
    vgg_str="Style_3DGS/AdaIN/models/vgg_normalised.pth",
    decoder_str="Style_3DGS/AdaIN/models/decoder.pth",
    depth_offset=0.5,
    depth_prominence=20,
    content_size=512,
    style_size=512,
    alpha=0.5,
    crop=False,
    save_ext=".jpg",
    output="output",
    file_name="test",
    preserve_color=False,
    content_mask=None,
    use_depth=False,
    depth_map=None,
    style_interpolation_weights=None,
):
    """Stylise one content image with one style image and save it; returns the output ``Path``
    (reference test.py:153-247; same parameters, defaults and return value).  ``depth_map`` (an addition, use it by
    keyword) supplies a precomputed proximity map [H0,W0] for ``use_depth=True`` instead of the depth provider.
    Style interpolation (an addition; test_video.py:30-45): ``style_img`` a list of K style images with
    ``style_interpolation_weights`` a list of K floats, used as given - the content is styled with that mix of the styles."""
    device = _device()
    out_dir = Path(output)
    out_dir.mkdir(exist_ok=True, parents=True)
    enc, dec = _singletons(device, vgg_str, decoder_str)
    target = out_dir / f"{file_name}{save_ext}"
    T = _stage_timer
    call = SimpleNamespace(alpha=alpha, use_depth=use_depth, depth_map=depth_map, depth_offset=depth_offset, depth_prominence=depth_prominence,
                           content_mask=content_mask, target=target)
    if isinstance(style_img, (list, tuple)) or style_interpolation_weights is not None:
        _mix_call(content_img, style_img, style_interpolation_weights, enc, dec, device, content_size, style_size, crop, preserve_color, call)
        print(f"Image saved to {target}")
        return target

    if _style_cache_on and (not preserve_color or _device_coral_on) and isinstance(enc, net.HipVGG) and isinstance(dec, net.HipDecoder):
        # one style, many calls (video/utils.py:341-350, train.py:101): statistics from the cache, the frame in one C-ABI call
        frame, e0 = _content_frame(content_img, content_size, crop, device, call)
        if frame.dtype == torch.uint8 and _mask_fits(content_mask):
            t0 = time.perf_counter()
            if preserve_color:
                stats = _coral_style_stats(style_img, frame, style_size, crop, enc, device)
                T("CORAL + style statistics (device, per call)", t0)
            else:
                stats = _style_stats(style_img, style_size, crop, enc, device, drop_alpha=use_depth)
                T("style statistics (cached after the first call)", t0)
            if stats is not None:
                _one_call(frame, stats, enc, dec, device, call, e0)
                print(f"Image saved to {target}")
                return target
        content = frame[0].cpu().permute(2, 0, 1).float().div(255) if frame.dtype == torch.uint8 else frame      # ToTensor of the resized frame
    else:
        call.pil_content = _open(content_img)
        content = test_transform(content_size, crop)(call.pil_content)
    STYLE_ENCODES[0] += 1
    style = test_transform(style_size, crop)(_open(style_img))
    if preserve_color:                       # CORAL runs on the host tensors, as in the reference (test.py:201-202)
        style = coral(style, content)
    content, style = content.to(device).unsqueeze(0), style.to(device).unsqueeze(0)

    if use_depth:
        proximity = depth_map if depth_map is not None else midas_depth_map_est(call.pil_content)
        result = style_transfer(enc, dec, content, style, proximity, alpha, depth_offset, depth_prominence)
    else:
        result = style_transfer_simple(enc, dec, content, style, alpha)
    if content_mask is not None:
        result = composite_with_mask(content, result, content_mask)
    result = result[:, :3, :, :]             # an RGBA result keeps its colour planes only (test.py:240-241)

    save_image(result, str(target))
    print(f"Image saved to {target}")
    return target


# ---- the one-call form of adain_inference ------------------------------------------------------------------------------------
class _StageTimer:
    """Off by default (one attribute test per stage).  ``bench.py --per-call`` switches it on to see where a call's time goes:
    host stages by the host clock, the kernels by HIP events on the launch stream."""

    def __init__(self):
        self.on, self.host, self.events = False, {}, []

    def __call__(self, stage, t0):
        if self.on:
            self.host[stage] = self.host.get(stage, 0.0) + time.perf_counter() - t0

    def reset(self):
        self.host, self.events = {}, []

    def gpu_ms(self):
        return sum(a.elapsed_time(b) for a, b in self.events)


_stage_timer = _StageTimer()


def _mask_fits(content_mask):
    """The masks the reference's callers pass - [1,H,W] uint8 (localized_style_transfer.py:186), [3,H,W] bool (train.py:97) - and
    their float forms; anything else takes the call-by-call path (and fails there exactly where the reference does)."""
    if content_mask is None:
        return True
    m = content_mask
    if not isinstance(m, (np.ndarray, torch.Tensor)) or m.ndim != 3 or m.shape[0] not in (1, 3):
        return False
    dt = str(m.dtype).replace("torch.", "")
    return dt in ("uint8", "bool", "float32")


def _open(img):
    return Image.open(str(img)) if type(img) == str or isinstance(img, Path) else img


def _content_frame(content_img, content_size, crop, device, call):
    """The content of the one-call path, opened and decoded (``call.pil_content``), after the range asserts of test.py:55-56 / :75 ->
    (``test_transform_u8`` of it: uint8 [1,h,w,3] on the device, or a float tensor if not RGB; the stage timer's event before a device resize)."""
    assert 0.0 <= call.alpha <= 1.0
    if call.use_depth:
        assert 0.0 <= call.depth_offset <= 1.0
    T = _stage_timer
    t0 = time.perf_counter()
    pil_content = call.pil_content = _open(content_img)
    if (type(content_img) == str or isinstance(content_img, Path)) and _routes.decoder(content_img) is not None:
        e0 = torch.cuda.Event(enable_timing=True) if T.on else None
        frame = device_decode_transform_u8(content_img, content_size, crop, device, e0.record if T.on else None)
        if frame is not None:                                        # (pil_content stays lazily opened: decoded only if a depth provider asks)
            T("read + decode + resize content (device)", t0)
            return frame, e0
    pil_content.load()                                               # decode (a lazily opened file) - host work that stays
    T("open + decode content (PIL)", t0)
    t0 = time.perf_counter()
    e0 = torch.cuda.Event(enable_timing=True) if T.on else None
    frame = device_transform_u8(pil_content, content_size, crop, device, e0.record if T.on else None)     # upload + Resize [+ CenterCrop] on the device
    if frame is None:
        frame, e0 = test_transform_u8(content_size, crop)(pil_content), None      # not RGB / padded crop: PIL on the host
        if isinstance(frame, np.ndarray):                                        # (np.asarray of a PIL image is read-only)
            frame = torch.from_numpy(frame if frame.flags.writeable else frame.copy()).unsqueeze(0).to(device)
        T("resize content (PIL, host)", t0)
    else:
        T("upload + resize content (device; enqueue only)", t0)
    return frame, e0


def _style_image(style_img, style_size, crop, device, drop_alpha=False):
    """The transformed style on the device, as the encoder takes it: uint8 [1,h,w,3] for an RGB image (Resize [+ CenterCrop] there),
    else ``test_transform``'s float [1,3,h,w] (``drop_alpha``: without an RGBA image's fourth plane); None for any other channel count."""
    pil_style = _open(style_img)
    u8 = device_transform_u8(pil_style, style_size, crop, device)
    if u8 is not None:
        return u8
    style = test_transform(style_size, crop)(pil_style)
    if style.shape[0] == 4 and drop_alpha:
        style = style[:3]                                                 # test.py:60-61
    return style.unsqueeze(0).to(device).contiguous() if style.shape[0] == 3 else None


def _style_stats(style_img, style_size, crop, enc, device, drop_alpha):
    """The ``Style`` (mean, std each [1,512]) of the style image's relu4_1 features (test.py:63 + function.py:4-12 / :77), computed
    once per style (``_style_key``).  None when the transformed style is not a 3-channel image the encoder can take (4 channels with
    the alpha blend: the reference fails in its first convolution; the call-by-call path reports it)."""
    def make():
        style = _style_image(style_img, style_size, crop, device, drop_alpha)
        if style is None:
            return None
        STYLE_ENCODES[0] += 1
        return Style(*rt.mean_std((rt.encode_u8 if style.dtype == torch.uint8 else rt.encode)(style, enc.packed(device)), True))

    # an RGBA style gives other statistics on the depth path (alpha dropped) than on the alpha path (refused): part of the key
    return _cached_style(style_img, ("stats", bool(drop_alpha)), style_size, crop, enc, device, make)


def _coral_style_stats(style_img, frame, style_size, crop, enc, device):
    """The ``Style`` of ``coral(style, content)``'s relu4_1 features (test.py:201-202, :77) for the resized frame uint8 [1,h,w,3] on
    the device.  The resized style's pixels are kept on the device per style (``_style_key``); CORAL, the encoder and the statistics
    run per call, because the recoloured style depends on the frame.  None when the transformed style is not a 3-channel image (the
    call-by-call path reports it)."""
    def make():
        STYLE_PIXEL_UPLOADS[0] += 1
        return _style_image(style_img, style_size, crop, device)

    pixels = _cached_style(style_img, "pixels", style_size, crop, enc, device, make)
    if pixels is None:
        return None
    STYLE_ENCODES[0] += 1
    recoloured, _record = rt.coral(pixels, frame)
    return Style(*rt.mean_std(rt.encode(recoloured, enc.packed(device)), True))


def _mix_call(content_img, style_imgs, weights, enc, dec, device, content_size, style_size, crop, preserve_color, call):
    """adain_inference with a list of styles: every style's statistics through the style cache, the frame in one C-ABI call
    (``adain_stylize_u8_mix``) with the weights as given."""
    if not isinstance(style_imgs, (list, tuple)) or weights is None or len(weights) != len(style_imgs) or not 1 <= len(style_imgs) <= rt.MIX_MAX_STYLES:
        raise ValueError(f"style interpolation needs a list of 1 .. {rt.MIX_MAX_STYLES} style images and as many style_interpolation_weights")
    if preserve_color:
        raise ValueError("preserve_color with style_interpolation_weights is not supported (it would need coral of every style per frame)")
    if not (isinstance(enc, net.HipVGG) and isinstance(dec, net.HipDecoder)):
        raise rt.AdainHipError("style interpolation runs on the package's encoder and decoder")
    if not _mask_fits(call.content_mask):
        raise ValueError("content_mask must be [1|3,H,W] uint8, bool or float32")
    frame, e0 = _content_frame(content_img, content_size, crop, device, call)
    if frame.dtype != torch.uint8:
        raise ValueError("style interpolation needs an RGB content image")
    stats = [_style_stats(s, style_size, crop, enc, device, drop_alpha=call.use_depth) for s in style_imgs]
    if any(st is None for st in stats):
        raise ValueError("style interpolation needs 3-channel style images")
    w = torch.tensor([float(v) for v in weights], dtype=torch.float32, device=device)
    _one_call(frame, Style.stack(stats), enc, dec, device, call, e0, style_weights=w)


def _one_call(x, style, enc, dec, device, call, e0=None, style_weights=None):
    """A resized RGB frame (uint8 [1,h,w,3] on the device) -> the saved file: ``adain_stylize_u8``, download, PIL save.  ``call``: the
    record of the call's options and its ``pil_content``.  ``e0``: an event recorded before the device-side resize (stage timer)."""
    alpha, use_depth, depth_map, content_mask, target = call.alpha, call.use_depth, call.depth_map, call.content_mask, call.target
    T = _stage_timer
    depth = None
    if use_depth:
        t0 = time.perf_counter()
        proximity = depth_map if depth_map is not None else midas_depth_map_est(call.pil_content)
        if not isinstance(proximity, torch.Tensor):
            proximity = torch.as_tensor(np.asarray(proximity))
        T("depth provider", t0)
    t0 = time.perf_counter()
    if use_depth:
        depth = [proximity.to(device=device, dtype=torch.float32).contiguous()]
    mask = None
    if content_mask is not None:
        m = content_mask if isinstance(content_mask, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(content_mask))
        mask = m.to(device).unsqueeze(0)                                 # test.py:224-226 (the .float() happens in the kernel)
    T("upload (depth map, mask)", t0)
    t0 = time.perf_counter()
    if T.on:
        e1 = torch.cuda.Event(enable_timing=True)
        if e0 is None:
            e0 = torch.cuda.Event(enable_timing=True)
            e0.record()
    u8 = rt.stylize_u8(x, enc.packed(device), dec.packed(device), style.mean, style.std, alpha, depth, call.depth_offset, call.depth_prominence,
                       mask, style_weights=style_weights)
    if T.on:
        e1.record()
        T.events.append((e0, e1))
    stages = iter(("launch (one C-ABI call)", "wait for the kernels + download", "encode + write the file"))

    def mark():
        nonlocal t0
        T(next(stages), t0)
        t0 = time.perf_counter()

    _routes.write(u8, target, mark)


def composite_with_mask(content, output_img, content_mask):
    """The content-mask composite of adain_inference (test.py:222-236): mask -> float -> unsqueeze(0) ->
    nearest resize to the content size; output bilinear-resized to the content size;
    content*(1-m) + output*m."""
    if isinstance(content_mask, torch.Tensor):
        mask_tensor = content_mask.to(device=content.device).float()
    else:
        mask_tensor = torch.from_numpy(np.ascontiguousarray(content_mask)).float().to(content.device)
    mask_tensor = mask_tensor.unsqueeze(0)
    size = tuple(content.shape[-2:])
    # interpolating to the size a tensor already has is the identity in both modes: skipped (see engine.AdaINEngine.composite)
    if tuple(mask_tensor.shape[-2:]) != size:
        mask_tensor = rt.resize_nearest(mask_tensor.contiguous(), size)
    if tuple(output_img.shape[-2:]) != size:
        output_img = rt.resize_bilinear(output_img, size)
    if content.shape[1] != output_img.shape[1]:
        raise ValueError(f"content has {content.shape[1]} channels but the stylised output has {output_img.shape[1]}")
    return rt.mask_composite(content.contiguous(), output_img, mask_tensor)
