"""Makes tests/golden/metrics/grad_noise.json: how far float32 gradients of the SSIM lie from the float64 restatement.

    python tests/golden/make_metrics_grad_golden.py REFERENCE_ROOT

Runs on the CPU.  The modelled project's Style_3DGS/utils/loss_utils.py is loaded by path, here and in make_metrics_golden.py and nowhere
else; none of its text is copied.  The cases are those of tests/golden/metrics/cases.npz (tests/metrics_cases.py: four families x five
sizes, two frames each, c = 3 and c = 1), as float32 NCHW frames scaled as to_tensor does; the gradients are those of every frame's own
ssim by both inputs (the weights {1, 0, 0}).  A frame pair of a case that is equal (a c = 1 case whose difference lies in another channel)
counts with the equal frames.

  R_grad    the reference's float32 ``ssim(size_average=False)`` under torch autograd
  S_grad    a float32 torch emulation of the device's separable two-stage form (tests/metrics_grad_ref.py names the planes): the five
            window statistics by a row pass and a column pass of 11 taps, the derivative planes in the kernel's arrangement, the same
            two passes over them, the combination with the inputs
            both: the largest distance from the float64 restatement over the cases, in units of the frame's largest float64 gradient entry
  bar_grad  2 max(R_grad, S_grad)
  R_equal, S_equal    equal frames (every case's a against itself) have the gradient 0, so the unit above is empty: count max|g| of the
            two float32 forms, count = c h w
  bar_equal 2 max(R_equal, S_equal)
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
import metrics_grad_ref as G  # noqa: E402
import metrics_ref as R  # noqa: E402


def load(root, rel, name):
    spec = importlib.util.spec_from_file_location(name, os.path.join(root, rel))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def reference_grads(L, a, b):
    """The reference's float32 ssim per frame under autograd -> (grad_a, grad_b), numpy float32."""
    x, y = torch.from_numpy(a).requires_grad_(), torch.from_numpy(b).requires_grad_()
    L.ssim(x, y, size_average=False).sum().backward()
    return x.grad.numpy(), y.grad.numpy()


def separable_grads(a, b):
    """The device's form in float32 torch: (grad_a, grad_b) of every frame's own ssim."""
    x, y = torch.from_numpy(a), torch.from_numpy(b)
    c = x.shape[1]
    count = np.float32(1.0 / float(a[0].size))
    g = torch.from_numpy(R.window().copy())
    row, col = g.view(1, 1, 1, 11).expand(c, 1, 1, 11).contiguous(), g.view(1, 1, 11, 1).expand(c, 1, 11, 1).contiguous()
    conv = lambda t: F.conv2d(F.conv2d(t, row, padding=(0, 5), groups=c), col, padding=(5, 0), groups=c)
    c1, c2 = np.float32(R.C1), np.float32(R.C2)
    mu1, mu2 = conv(x), conv(y)
    s1, s2, s12 = conv(x * x) - mu1 * mu1, conv(y * y) - mu2 * mu2, conv(x * y) - mu1 * mu2
    A, B, D, E = 2 * (mu1 * mu2) + c1, 2 * s12 + c2, mu1 * mu1 + mu2 * mu2 + c1, s1 + s2 + c2
    p, q = A / D, B / E
    pq = p * q
    d_mean = lambda mine, other: 2 * ((other * q - mine * pq) / D - (other * p - mine * pq) / E)
    d_e, c12 = conv(-pq / E), conv((2 * p) / E)
    out = []
    for u, v, d_mu in ((x, y, d_mean(mu1, mu2)), (y, x, d_mean(mu2, mu1))):
        out.append((count * ((conv(d_mu) + (2 * u) * d_e) + v * c12)).numpy())
    assert out[0].dtype == np.float32
    return out[0], out[1]


def main(root):
    torch.set_num_threads(1)
    L = load(root, "Style_3DGS/utils/loss_utils.py", "_ref_loss_utils")
    z = C.load_golden()
    dev = {"R_grad": 0.0, "S_grad": 0.0, "R_equal": 0.0, "S_equal": 0.0}
    for name in C.golden_names():
        a8, b8 = C.golden_pair(z, name)
        a, b = C.to_nchw_f32(a8), C.to_nchw_f32(b8)
        n, count = a.shape[0], a[0].size
        want = G.grad(a, b, [[1.0, 0.0, 0.0]] * n)
        differ = [i for i in range(n) if not np.array_equal(a[i], b[i])]          # a c = 1 case can hold a frame pair that is equal
        for key, got in (("R", reference_grads(L, a, b)), ("S", separable_grads(a, b))):
            for i in range(n):
                if i in differ:
                    worst = max(float(G.distance(got[k][i:i + 1], want[k][i:i + 1])[0]) for k in (0, 1))
                    print(name, i, key, worst)
                    dev[key + "_grad"] = max(dev[key + "_grad"], worst)
                else:
                    dev[key + "_equal"] = max(dev[key + "_equal"], float(count * max(np.abs(got[0][i]).max(), np.abs(got[1][i]).max())))
        for key, got in (("R_equal", reference_grads(L, a, a.copy())), ("S_equal", separable_grads(a, a.copy()))):
            dev[key] = max(dev[key], float(count * max(np.abs(got[0]).max(), np.abs(got[1]).max())))
    dev["bar_grad"], dev["bar_equal"] = 2 * max(dev["R_grad"], dev["S_grad"]), 2 * max(dev["R_equal"], dev["S_equal"])
    dev["torch"] = torch.__version__
    with open(os.path.join(C.GOLDEN, "grad_noise.json"), "w") as f:
        json.dump(dev, f, indent=1, sort_keys=True)
    print(dev)


if __name__ == "__main__":
    main(sys.argv[1])
