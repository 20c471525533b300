"""The modelled project's quality scores with its names and signatures: ``ssim``, ``l1_loss``, ``l2_loss`` (Style_3DGS/utils/loss_utils.py),
``psnr``, ``mse`` (utils/image_utils.py) and the evaluation of Style_3DGS/metrics.py (``evaluate``), so that ``from utils.loss_utils import
ssim`` can be swapped for ``from applied_image_processing_amd.metrics import ssim``.

Where the device scores: float32 GPU tensors [N,C,H,W] (``ssim`` also [C,H,W]) with C in 1..4 that need no gradient, at ``window_size``
11, go through ``runtime.image_metrics`` (adain_image_metrics_f32: one fused pass, float64 sums); ``compare_dirs`` hands it the decoded
uint8 frames (adain_image_metrics_u8).  Everything else - another window size, CPU tensors, other dtypes, tensors that need a gradient
- runs the reference's expressions in torch, with the values they always had.  Without a GPU everything runs in torch on the CPU.

The training loss (Style_3DGS/train.py: ``(1 - lambda_dssim) * l1_loss(image, gt) + lambda_dssim * (1 - ssim(image, gt))``, then
``loss.backward()``) has a device route as well, which is opt-in: after ``set_device_backward(True)`` the same float32 GPU tensors, when
one of them needs a gradient, go through one ``torch.autograd.Function`` whose forward is ``runtime.image_metrics`` and whose backward is
``runtime.image_metrics_grad`` (adain_image_metrics_grad_f32: the SSIM, MSE and L1 gradients in closed form, two kernels).  ``psnr``
chains through its ``mse`` in torch.  ``dssim_loss`` is train.py's expression as one forward and one backward call.  The function is
once differentiable; with the switch off (the default) a tensor that needs a gradient takes the torch route exactly as before.

The second phase of train.py (lines 208-221: ``l1_loss`` of the render against the stylised guide view, read from its file and
``F.interpolate``d to the render's size every iteration) is ``guide_l1_loss`` and ``GuideBank``: the guides stay uint8 on the device at
their own size, and GPU tensors go through one ``torch.autograd.Function`` whose forward is ``runtime.guide_l1`` and whose backward is
``runtime.guide_l1_grad`` (adain_guide_l1_f32 / adain_guide_l1_grad_f32: resample, difference, reduction and gradient fused).  It is a
new function, so it needs no switch.

LPIPS comes by provider only: ``evaluate(paths, lpips_fn=...)`` with a callable (render, gt) -> value on [1,3,H,W] tensors in [0,1].  Its
VGG weights are a network fetch, as those of the other networks are, and are not part of this package.
"""
import json
import os
from math import exp

import numpy as np
import torch
import torch.nn.functional as F

C1, C2 = 0.01 ** 2, 0.03 ** 2


def _device_pair(a, b, dims=(4,)):
    """Do ``a`` and ``b`` take the device call?  float32 GPU tensors of one shape, [N,C,H,W] (or a dimension count in ``dims``), C in 1..4,
    not empty, no gradient wanted."""
    return (isinstance(a, torch.Tensor) and isinstance(b, torch.Tensor) and a.is_cuda and b.is_cuda and a.device == b.device
            and a.dtype == torch.float32 and b.dtype == torch.float32 and a.shape == b.shape and a.dim() in dims and 1 <= a.shape[-3] <= 4
            and a.numel() > 0 and not (torch.is_grad_enabled() and (a.requires_grad or b.requires_grad)))


def _records(a, b):
    from . import runtime as rt

    return rt.image_metrics(a, b)


_device_backward = False


def set_device_backward(enabled):
    """Switches the device route of tensors that need a gradient on or off (off by default); returns the previous value."""
    global _device_backward
    previous, _device_backward = _device_backward, bool(enabled)
    return previous


def device_backward():
    return _device_backward


class _Scores(torch.autograd.Function):
    """(a, b) float32 [N,C,H,W] on the device -> float64 [N,3], every frame's {ssim, mse, l1}; the backward hands the incoming [N,3]
    to ``runtime.image_metrics_grad`` as the frames' weights."""

    @staticmethod
    def forward(ctx, a, b):
        ctx.save_for_backward(a, b)
        return _records(a, b).records[:, :3].contiguous()

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, grad):
        from . import runtime as rt

        a, b = ctx.saved_tensors
        weights = grad.to(torch.float64).contiguous()
        need_a, need_b = ctx.needs_input_grad
        if need_a and need_b:
            return rt.image_metrics_grad(a, b, weights, grad_b=True)
        if need_b:
            return None, rt.image_metrics_grad(b, a, weights)          # grad_b(a, b) is grad_a(b, a), bit for bit
        return rt.image_metrics_grad(a, b, weights), None


def _grad_pair(a, b, dims=(4,)):
    """Do ``a`` and ``b`` take the device call and its backward?  ``_device_pair``'s tensors, one of which needs a gradient, with the
    switch on."""
    return (_device_backward and isinstance(a, torch.Tensor) and isinstance(b, torch.Tensor) and torch.is_grad_enabled() and (a.requires_grad or b.requires_grad)
            and _device_pair(a.detach(), b.detach(), dims))


def _scores(a, b):
    """float64 [N,3] = {ssim, mse, l1} per frame of a ``_grad_pair``, differentiable once."""
    return _Scores.apply(a, b) if a.dim() == 4 else _Scores.apply(a[None], b[None])


def dssim_loss(image, gt, lambda_dssim=0.2):
    """Style_3DGS/train.py's loss, ``(1 - lambda_dssim) * l1_loss(image, gt) + lambda_dssim * (1 - ssim(image, gt))``: on the device route
    one forward and one backward call for both terms; otherwise that expression of this module's ``l1_loss`` and ``ssim``."""
    if _grad_pair(image, gt, dims=(3, 4)):
        s = _scores(image, gt)
        return ((1.0 - lambda_dssim) * s[:, 2].mean() + lambda_dssim * (1.0 - s[:, 0].mean())).to(torch.float32)
    return (1.0 - lambda_dssim) * l1_loss(image, gt) + lambda_dssim * (1.0 - ssim(image, gt))


def l1_loss(network_output, gt):
    if _grad_pair(network_output, gt):
        return _scores(network_output, gt)[:, 2].mean().to(torch.float32)
    if _device_pair(network_output, gt):
        return _records(network_output, gt).l1.mean().to(torch.float32)          # frames of one size: the mean of their means
    return torch.abs((network_output - gt)).mean()


def l2_loss(network_output, gt):
    if _grad_pair(network_output, gt):
        return _scores(network_output, gt)[:, 1].mean().to(torch.float32)
    if _device_pair(network_output, gt):
        return _records(network_output, gt).mse.mean().to(torch.float32)
    return ((network_output - gt) ** 2).mean()


def gaussian(window_size, sigma):
    gauss = torch.tensor([exp(-(x - window_size // 2) ** 2 / float(2 * sigma ** 2)) for x in range(window_size)], dtype=torch.float32)
    return gauss / gauss.sum()


def create_window(window_size, channel):
    g = gaussian(window_size, 1.5).unsqueeze(1)
    return g.mm(g.t()).float().unsqueeze(0).unsqueeze(0).expand(channel, 1, window_size, window_size).contiguous()


def _ssim(img1, img2, window, window_size, channel, size_average=True):
    conv = lambda t: F.conv2d(t, window, padding=window_size // 2, groups=channel)
    mu1, mu2 = conv(img1), conv(img2)
    mu1_sq, mu2_sq, mu1_mu2 = mu1.pow(2), mu2.pow(2), mu1 * mu2
    sigma1_sq, sigma2_sq, sigma12 = conv(img1 * img1) - mu1_sq, conv(img2 * img2) - mu2_sq, conv(img1 * img2) - mu1_mu2
    ssim_map = ((2 * mu1_mu2 + C1) * (2 * sigma12 + C2)) / ((mu1_sq + mu2_sq + C1) * (sigma1_sq + sigma2_sq + C2))
    return ssim_map.mean() if size_average else ssim_map.mean(1).mean(1).mean(1)


def ssim(img1, img2, window_size=11, size_average=True):
    """The reference's ``ssim``: a 0-d tensor, or with ``size_average=False`` one value per image, [N]."""
    if window_size == 11 and _grad_pair(img1, img2, dims=(3, 4) if size_average else (4,)):
        per_frame = _scores(img1, img2)[:, 0]
        return (per_frame.mean() if size_average else per_frame).to(torch.float32)
    if window_size == 11 and _device_pair(img1, img2, dims=(3, 4) if size_average else (4,)):
        per_frame = _records(img1, img2).ssim
        return (per_frame.mean() if size_average else per_frame).to(torch.float32)
    channel = img1.size(-3)
    window = create_window(window_size, channel).to(img1.device).type_as(img1)
    return _ssim(img1, img2, window, window_size, channel, size_average)


def mse(img1, img2):
    if _grad_pair(img1, img2):
        return _scores(img1, img2)[:, 1].to(torch.float32)[:, None]
    if _device_pair(img1, img2):
        return _records(img1, img2).mse.to(torch.float32)[:, None]
    return (((img1 - img2)) ** 2).view(img1.shape[0], -1).mean(1, keepdim=True)


def psnr(img1, img2):
    """The reference's ``psnr``: [N,1]."""
    if _grad_pair(img1, img2):
        return (20 * torch.log10(1.0 / torch.sqrt(_scores(img1, img2)[:, 1]))).to(torch.float32)[:, None]          # autograd chains through mse
    if _device_pair(img1, img2):
        return _records(img1, img2).psnr.to(torch.float32)[:, None]
    return 20 * torch.log10(1.0 / torch.sqrt(mse(img1, img2)))


# --- the guide-view loss of Style_3DGS/train.py:208-221 ---------------------------------------------------------------------------------------
class _GuideL1(torch.autograd.Function):
    """(image float32 [N,3,H,W] or [3,H,W], guide uint8 [N,gh,gw,3] or [gh,gw,3]) on the device -> train.py's ``Ll1``, 0-d float32: the
    mean of the frames' float64 l1 (``runtime.guide_l1``), cast once.  The backward hands the incoming scalar / N to
    ``runtime.guide_l1_grad`` as every frame's weight.  Only ``image`` gets a gradient.  The mean and the cast are inside the function,
    so the graph of a training step holds this one node."""

    @staticmethod
    def forward(ctx, image, guide):
        from . import runtime as rt

        ctx.save_for_backward(image, guide)
        l1 = rt.guide_l1(image, guide).l1
        return (l1[0] if l1.shape[0] == 1 else l1.mean()).to(torch.float32)          # frames of one size: the mean of their means

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, grad):
        from . import runtime as rt

        image, guide = ctx.saved_tensors
        n = image.shape[0] if image.dim() == 4 else 1
        weights = grad.to(torch.float64).reshape(1)
        return rt.guide_l1_grad(image, guide, weights if n == 1 else (weights / n).expand(n).contiguous()), None


def _guide_pair(image, guide):
    """Do ``image`` and ``guide`` take the device call?  A float32 GPU render [3,H,W] or [N,3,H,W] and uint8 guides [gh,gw,3] or [N,gh,gw,3] on
    the same device, one guide per frame, not empty."""
    if not (isinstance(image, torch.Tensor) and isinstance(guide, torch.Tensor) and image.is_cuda and guide.is_cuda and image.device == guide.device
            and image.dtype == torch.float32 and guide.dtype == torch.uint8 and image.dim() in (3, 4) and guide.dim() in (3, 4)
            and image.shape[-3] == 3 and guide.shape[-1] == 3 and image.numel() > 0 and guide.numel() > 0):
        return False
    return (image.shape[0] if image.dim() == 4 else 1) == (guide.shape[0] if guide.dim() == 4 else 1)


def _guide_l1_torch(image, guide):
    """train.py:214-220 after the file is open: ``to_tensor``, ``F.interpolate`` to the render's size, ``l1_loss``."""
    frames = guide if guide.dim() == 4 else guide.unsqueeze(0)
    image_guide_tensor = frames.permute(0, 3, 1, 2).contiguous().to(torch.float32).div(255).to(image.device)          # to_tensor
    image_guide_resized = F.interpolate(image_guide_tensor, size=image.shape[-2:], mode="bilinear", align_corners=False)
    if image.dim() == 3:
        image_guide_resized = image_guide_resized.squeeze(0)
    return torch.abs((image - image_guide_resized)).mean()


def guide_l1_loss(image, guide):
    """Style_3DGS/train.py's ``Ll1`` of its second phase, ``l1_loss(image, F.interpolate(to_tensor(guide)[None], size=image.shape[-2:],
    mode="bilinear", align_corners=False))``, as a 0-d float32 tensor: ``image`` float32 [3,H,W] or [N,3,H,W], ``guide`` the picture as
    uint8 [gh,gw,3] or [N,gh,gw,3] (what ``Image.convert("RGB")`` holds).  On GPU tensors one forward call (``runtime.guide_l1``) and, under
    autograd, one backward call (``runtime.guide_l1_grad``) - no float guide is written; differentiable once, by ``image`` only.  Anything
    else - CPU tensors, another channel count, another dtype - runs the reference's lines in torch."""
    if _guide_pair(image, guide):
        return _GuideL1.apply(image, guide)
    return _guide_l1_torch(image, guide)


class GuideBank:
    """The stylised guide views of a scene by name, uint8 [gh,gw,3] each (sizes may differ), resident on one device: 0.75 MB for a 512 x 512
    view against the 7.7 MB of an 800 x 800 float32 frame.  Without a GPU the tensors are on the CPU and ``loss`` takes the torch route."""

    def __init__(self, frames):
        self._frames = dict(frames)

    @classmethod
    def from_files(cls, paths, device=None, routes=None):
        """``paths``: the {name: path} map ``precompute_guides_sharded`` returns.  Every file is read as train.py reads it back,
        ``Image.open(path).convert("RGB")`` (the pixels after the JPEG) and uploaded once - or decoded on ``device`` where a decode route of
        ``routes`` (an ``OutputRoutes``, or what its ``of`` takes) is switched on and takes the file: the same pixels."""
        device = torch.device(device if device is not None else ("cuda:0" if torch.cuda.is_available() else "cpu"))
        if routes is not None:
            from . import runtime as rt

            routes = rt.OutputRoutes.of(routes)
        return cls((name, _read_rgb(str(path), device, routes).contiguous()) for name, path in paths.items())

    @classmethod
    def from_frames(cls, names, u8):
        """Frames that are already there, one uint8 [gh,gw,3] per name (a tensor [N,gh,gw,3] or a sequence), used as given."""
        names = list(names)
        if len(names) != len(u8):
            raise ValueError(f"GuideBank.from_frames: {len(names)} names for {len(u8)} frames")
        for frame in u8:
            if not (isinstance(frame, torch.Tensor) and frame.dtype == torch.uint8 and frame.dim() == 3):
                raise ValueError("GuideBank.from_frames: every frame must be a uint8 tensor [gh,gw,3]")
        return cls(zip(names, u8))

    def __getitem__(self, name):
        return self._frames[name]

    def __contains__(self, name):
        return name in self._frames

    def __len__(self):
        return len(self._frames)

    def __iter__(self):
        return iter(self._frames)

    @property
    def nbytes(self):
        return sum(f.numel() * f.element_size() for f in self._frames.values())

    def loss(self, image, name):
        """``guide_l1_loss(image, bank[name])``: train.py:208-221 for the view ``name``."""
        return guide_l1_loss(image, self._frames[name])


# --- the evaluation of Style_3DGS/metrics.py -------------------------------------------------------------------------------------------------
def _read_rgb(path, device, routes):
    """The file as uint8 [h,w,3] (alpha dropped) on ``device``: decoded there when a route of ``routes`` is switched on, else by PIL."""
    from PIL import Image

    if device.type == "cuda" and routes is not None:
        frame = routes.read_rgb(path, device)
        if frame is not None:
            return frame
    with Image.open(path) as im:
        return torch.from_numpy(np.asarray(im.convert("RGB")).copy()).to(device)


def compare_dirs(renders_dir, gt_dir, device, routes=None):
    """The files of ``renders_dir`` against the files of the same names in ``gt_dir`` -> {name: {"SSIM": value, "PSNR": value}}, the
    float32 scores Style_3DGS/metrics.py computes per view, as Python floats.  ``routes``: an ``OutputRoutes`` (or what its ``of``
    takes) whose ``decode_on_device`` flags send the files through the device decoders; the pixels are the same either way.  The files of
    one size are scored in one call: on a GPU ``runtime.image_metrics`` on the uint8 frames, without one torch on the CPU."""
    device = torch.device(device)
    if routes is not None:
        from . import runtime as rt

        routes = rt.OutputRoutes.of(routes)
    names = sorted(os.listdir(str(renders_dir)))
    groups = {}
    for name in names:
        render = _read_rgb(os.path.join(str(renders_dir), name), device, routes)
        gt = _read_rgb(os.path.join(str(gt_dir), name), device, routes)
        if render.shape != gt.shape:
            raise ValueError(f"compare_dirs: {name} is {tuple(render.shape[:2])} in {renders_dir} and {tuple(gt.shape[:2])} in {gt_dir}")
        groups.setdefault(tuple(render.shape), []).append((name, render, gt))
    scores = {}
    for members in groups.values():
        a, b = torch.stack([m[1] for m in members]), torch.stack([m[2] for m in members])
        if device.type == "cuda":
            from . import runtime as rt

            got = rt.image_metrics(a, b)
            s, p = got.ssim.to(torch.float32).tolist(), got.psnr.to(torch.float32).tolist()
        else:
            x, y = (t.permute(0, 3, 1, 2).contiguous().to(torch.float32) / 255.0 for t in (a, b))          # to_tensor
            s, p = ssim(x, y, size_average=False).tolist(), psnr(x, y).reshape(-1).tolist()
        for (name, _, _), sv, pv in zip(members, s, p):
            scores[name] = {"SSIM": sv, "PSNR": pv}
    return {name: scores[name] for name in names}


def evaluate(model_paths, lpips_fn=None, device=None, routes=None):
    """Style_3DGS/metrics.py ``evaluate``: for every scene directory and every method under its ``test/`` the ``renders/`` against the
    ``gt/`` -> ``results.json`` ({method: {"SSIM", "PSNR"}}: the means) and ``per_view.json`` ({method: {"SSIM": {name: value}, "PSNR":
    {...}}}) in the scene directory.  "LPIPS" appears in both only with ``lpips_fn``, a callable (render, gt) -> value on [1,3,H,W]
    float32 tensors in [0,1].  Returns {scene: results}.  An unreadable scene raises; the reference prints and goes on."""
    device = torch.device(device if device is not None else ("cuda:0" if torch.cuda.is_available() else "cpu"))
    full = {}
    for scene_dir in model_paths:
        scene_dir = str(scene_dir)
        print("Scene:", scene_dir)
        full[scene_dir], per_view = {}, {}
        test_dir = os.path.join(scene_dir, "test")
        for method in sorted(os.listdir(test_dir)):
            print("Method:", method)
            renders_dir, gt_dir = os.path.join(test_dir, method, "renders"), os.path.join(test_dir, method, "gt")
            scores = compare_dirs(renders_dir, gt_dir, device, routes)
            columns = {"SSIM": [v["SSIM"] for v in scores.values()], "PSNR": [v["PSNR"] for v in scores.values()]}
            if lpips_fn is not None:
                columns["LPIPS"] = []
                for name in scores:
                    render, gt = (_read_rgb(os.path.join(d, name), device, None).permute(2, 0, 1)[None].to(torch.float32) / 255.0 for d in (renders_dir, gt_dir))
                    columns["LPIPS"].append(float(lpips_fn(render, gt)))
            full[scene_dir][method] = {key: torch.tensor(values).mean().item() for key, values in columns.items()}
            per_view[method] = {key: dict(zip(scores, torch.tensor(values).tolist())) for key, values in columns.items()}
            for key, value in full[scene_dir][method].items():
                print("  {:<5}: {:>12.7f}".format(key, value))
            print("")
        with open(os.path.join(scene_dir, "results.json"), "w") as fp:
            json.dump(full[scene_dir], fp, indent=True)
        with open(os.path.join(scene_dir, "per_view.json"), "w") as fp:
            json.dump(per_view, fp, indent=True)
    return full


def main(argv=None):
    import argparse

    ap = argparse.ArgumentParser(prog="python -m applied_image_processing_amd.metrics", description="SSIM and PSNR of every test/<method>/renders against its gt.")
    ap.add_argument("--model_paths", "-m", required=True, nargs="+", type=str, default=[])
    ap.add_argument("--device", default=None, help="default: cuda:0 when there is a GPU, else cpu")
    a = ap.parse_args(argv)
    evaluate(a.model_paths, device=a.device)
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
