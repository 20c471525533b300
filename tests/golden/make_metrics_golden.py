"""Makes the image-metrics fixtures under tests/golden/metrics/: cases.npz and noise.json.

    python tests/golden/make_metrics_golden.py REFERENCE_ROOT

Runs on the CPU.  The modelled project's Style_3DGS/utils/loss_utils.py and utils/image_utils.py are loaded by path, here and nowhere
else; none of their text is copied.

cases.npz: per case of tests/metrics_cases.py (four families x five sizes, two frames each, c = 3; the c = 1 case is channel 0 of it)
  <family>_<h>x<w>_c3_a, _b   the uint8 inputs [2,h,w,3]
  <name>_ssim                 the reference's float32 ssim(size_average=False) on to_tensor's x / 255, [2]
  <name>_psnr                 its float32 psnr, [2]
  <name>_map                  its per-element map, recomputed from its expression with its create_window, float32 [2,c,h,w]
  window                      its gaussian(11, 1.5), float32 [11]
noise.json: the largest distance from the float64 restatement (tests/metrics_ref.py) over these cases of
  R_frame, R_map              the reference's per-image ssim and per-element map
  S_frame, S_map              a float32 emulation of the separable form (a row pass, then a column pass, torch on the CPU)
and the bars the device tests use: bar_frame = 2 max(R_frame, S_frame), bar_map = 2 max(R_map, S_map).
"""
import importlib.util
import json
import os
import sys

import numpy as np
import torch
import torch.nn.functional as F

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))

import metrics_cases as C  # noqa: E402
import metrics_ref as R  # noqa: E402


def load(root, rel, name):
    spec = importlib.util.spec_from_file_location(name, os.path.join(root, rel))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def reference_map(L, x, y):
    """The reference's map from its own window and torch's float32 convolutions."""
    c = x.shape[1]
    win = L.create_window(11, c)
    conv = lambda t: F.conv2d(t, win, padding=5, groups=c)
    mu1, mu2 = conv(x), conv(y)
    s1, s2, s12 = conv(x * x) - mu1.pow(2), conv(y * y) - mu2.pow(2), conv(x * y) - mu1 * mu2
    return ((2 * mu1 * mu2 + 0.01 ** 2) * (2 * s12 + 0.03 ** 2)) / ((mu1.pow(2) + mu2.pow(2) + 0.01 ** 2) * (s1 + s2 + 0.03 ** 2))


def separable_map(x, y):
    """The separable float32 form: 11 taps along the row, then 11 along the column, zero padding."""
    c = x.shape[1]
    g = torch.from_numpy(R.window().copy())
    row, col = g.view(1, 1, 1, 11).expand(c, 1, 1, 11).contiguous(), g.view(1, 1, 11, 1).expand(c, 1, 11, 1).contiguous()
    conv = lambda t: F.conv2d(F.conv2d(t, row, padding=(0, 5), groups=c), col, padding=(5, 0), groups=c)
    mu1, mu2 = conv(x), conv(y)
    s1, s2, s12 = conv(x * x) - mu1 * mu1, conv(y * y) - mu2 * mu2, conv(x * y) - mu1 * mu2
    return ((2 * (mu1 * mu2) + np.float32(R.C1)) * (2 * s12 + np.float32(R.C2))) / ((mu1 * mu1 + mu2 * mu2 + np.float32(R.C1)) * (s1 + s2 + np.float32(R.C2)))


def main(root):
    torch.set_num_threads(1)
    L = load(root, "Style_3DGS/utils/loss_utils.py", "_ref_loss_utils")
    I = load(root, "Style_3DGS/utils/image_utils.py", "_ref_image_utils")
    out = {"window": L.gaussian(11, 1.5).numpy().astype(np.float32)}
    assert out["window"].view(np.uint32).tolist() == list(R.WINDOW_BITS)
    dev = {"R_frame": 0.0, "R_map": 0.0, "S_frame": 0.0, "S_map": 0.0}
    for family in C.FAMILIES:
        for h, w in C.GOLDEN_SIZES:
            a3, b3 = C.pair(family, 2, h, w, 3)
            out[f"{family}_{h}x{w}_c3_a"], out[f"{family}_{h}x{w}_c3_b"] = a3, b3
            for c in (3, 1):
                name = f"{family}_{h}x{w}_c{c}"
                a, b = (a3, b3) if c == 3 else (a3[..., :1], b3[..., :1])
                x, y = torch.from_numpy(C.to_nchw_f32(a)), torch.from_numpy(C.to_nchw_f32(b))
                ssim = L.ssim(x, y, size_average=False).numpy()
                rmap = reference_map(L, x, y).numpy()
                assert np.array_equal(rmap.mean(axis=(1, 2, 3), dtype=np.float32).shape, ssim.shape)
                out[name + "_ssim"], out[name + "_psnr"], out[name + "_map"] = ssim.astype(np.float32), I.psnr(x, y).numpy().reshape(-1).astype(np.float32), rmap
                want = R.metrics_u8(np.ascontiguousarray(a), np.ascontiguousarray(b))
                want_map = want["map"].transpose(0, 3, 1, 2)
                smap = separable_map(x, y).numpy()
                dev["R_frame"] = max(dev["R_frame"], float(np.abs(ssim.astype(np.float64) - want["ssim"]).max()))
                dev["R_map"] = max(dev["R_map"], float(np.abs(rmap.astype(np.float64) - want_map).max()))
                dev["S_frame"] = max(dev["S_frame"], float(np.abs(smap.astype(np.float64).mean(axis=(1, 2, 3)) - want["ssim"]).max()))
                dev["S_map"] = max(dev["S_map"], float(np.abs(smap.astype(np.float64) - want_map).max()))
    os.makedirs(C.GOLDEN, exist_ok=True)
    np.savez_compressed(os.path.join(C.GOLDEN, "cases.npz"), **out)
    dev["bar_frame"], dev["bar_map"] = 2 * max(dev["R_frame"], dev["S_frame"]), 2 * max(dev["R_map"], dev["S_map"])
    dev["torch"] = torch.__version__
    with open(os.path.join(C.GOLDEN, "noise.json"), "w") as f:
        json.dump(dev, f, indent=1, sort_keys=True)
    print(dev)


if __name__ == "__main__":
    main(sys.argv[1])
