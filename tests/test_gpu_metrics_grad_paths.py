"""The callers of the device gradient: with ``metrics.set_device_backward(True)`` the package's ``ssim`` / ``l1_loss`` / ``l2_loss`` / ``mse``
/ ``psnr`` on float32 GPU tensors that need a gradient go through ``runtime.image_metrics`` and ``runtime.image_metrics_grad`` (counted by
spies) and give the restatement's gradients; ``dssim_loss`` is train.py's loss in one forward and one backward call; window 7 and
``torch.no_grad()`` are as before; with the switch off nothing reaches the device gradient and the values are torch's."""
import numpy as np
import pytest
import torch

import metrics_grad_cases as K
import metrics_grad_ref as G

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
BARS = K.bars()
SHAPE = (3, 3, 21, 70)
FA, FB = K.edge_pair(SHAPE, seed=8)
N, COUNT = SHAPE[0], FA[0].size
ELEMENT = 4 * 2.0 ** -24


def want(weights):
    return G.grad(FA, FB, np.broadcast_to(np.asarray(weights, dtype=np.float64), (N, 3)))


@pytest.fixture(scope="module")
def M():
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    import applied_image_processing_amd.metrics as M
    import applied_image_processing_amd.runtime as rt

    rt.lib()
    torch.cuda.set_device(0)
    return M


class Spies:
    """Counts the calls of ``rt.image_metrics`` and ``rt.image_metrics_grad`` and remembers whether grad_b was asked for."""

    def __enter__(self):
        import applied_image_processing_amd.runtime as rt

        self.rt, self.real = rt, (rt.image_metrics, rt.image_metrics_grad)
        self.forward, self.backward, self.asked_b = 0, 0, []

        def forward(*a, **k):
            self.forward += 1
            return self.real[0](*a, **k)

        def backward(a, b, weights, grad_b=False):
            self.backward += 1
            self.asked_b.append(bool(grad_b))
            return self.real[1](a, b, weights, grad_b)

        rt.image_metrics, rt.image_metrics_grad = forward, backward
        return self

    def __exit__(self, *exc):
        self.rt.image_metrics, self.rt.image_metrics_grad = self.real


def leaf(v):
    return torch.from_numpy(np.ascontiguousarray(v)).to(DEV).requires_grad_()


def close(got, want64):
    """Within the bar of the restatement, frame by frame."""
    d = G.distance(got.detach().cpu().numpy().reshape(want64.shape), want64)
    print("distance", d.max())
    return bool(np.all(d <= BARS["bar_grad"]))


def test_the_switch_on_sends_gradients_through_the_device(M):
    y = torch.from_numpy(FB).to(DEV)
    previous = M.set_device_backward(True)
    try:
        assert previous is False and M.device_backward() is True
        with Spies() as spy:
            # ssim, the mean over everything: every frame's weight is 1 / N
            x = leaf(FA)
            s = M.ssim(x, y)
            assert s.shape == () and s.dtype == torch.float32 and s.requires_grad
            s.backward()
            assert (spy.forward, spy.backward, spy.asked_b) == (1, 1, [False])
            assert x.grad.dtype == torch.float32 and x.grad.shape == x.shape and close(x.grad, want([1.0 / N, 0, 0])[0])
            # per image, upstream weights of the caller's
            x = leaf(FA)
            up = torch.tensor([1.0, -2.0, 0.5], device=DEV)
            (M.ssim(x, y, size_average=False) * up).sum().backward()
            assert close(x.grad, G.grad(FA, FB, [[1.0, 0, 0], [-2.0, 0, 0], [0.5, 0, 0]])[0])
            # one [C,H,W] image
            x = leaf(FA[1])
            M.ssim(x, y[1]).backward()
            assert x.grad.shape == (3, 21, 70) and close(x.grad[None], G.grad(FA[1:2], FB[1:2], [[1.0, 0, 0]])[0])
            # both inputs need one: a single backward call that asks for grad_b; only the second: the swapped call
            x, y2 = leaf(FA), leaf(FB)
            M.ssim(x, y2).backward()
            assert spy.asked_b[-1] is True and close(x.grad, want([1.0 / N, 0, 0])[0]) and close(y2.grad, want([1.0 / N, 0, 0])[1])
            both = y2.grad.clone()
            y2 = leaf(FB)
            M.ssim(torch.from_numpy(FA).to(DEV), y2).backward()
            assert spy.asked_b[-1] is False and torch.equal(y2.grad, both)
            # a non-contiguous input: the gradient has its shape and the contiguous one's values
            wide = torch.from_numpy(np.ascontiguousarray(FA.transpose(0, 1, 3, 2))).to(DEV).requires_grad_()
            M.ssim(wide.transpose(2, 3), y).backward()
            assert wide.grad.shape == (3, 3, 70, 21) and close(wide.grad.transpose(2, 3), want([1.0 / N, 0, 0])[0])
            # l1_loss, l2_loss and mse: elementwise, the l1 sign exact
            for fn, weights in ((M.l1_loss, [0, 0, 1.0 / N]), (M.l2_loss, [0, 1.0 / N, 0])):
                x = leaf(FA)
                fn(x, y).backward()
                g, w64 = x.grad.cpu().numpy(), want(weights)[0]
                assert np.all(np.abs(g - w64) <= ELEMENT * np.abs(w64)), fn.__name__
                assert fn is not M.l1_loss or np.array_equal(np.sign(g), np.sign(w64))
            x = leaf(FA)
            m = M.mse(x, y)
            assert m.shape == (N, 1) and m.dtype == torch.float32
            m.sum().backward()
            assert np.all(np.abs(x.grad.cpu().numpy() - want([0, 1.0, 0])[0]) <= ELEMENT * np.abs(want([0, 1.0, 0])[0]))
            # psnr chains through mse in torch: d psnr / d mse = -10 / (ln 10 mse) in float64, handed on as mse's weight.  The device's mse is
            # within 8 * 2^-24 of the exact one, relatively (tests/test_gpu_metrics_paths.py), which moves the weight as much; the mse
            # gradient adds its three roundings (ELEMENT); 2 * 2^-24 are left for the float64 operations between them
            x = leaf(FA)
            p = M.psnr(x, y)
            assert p.shape == (N, 1) and p.dtype == torch.float32
            p.sum().backward()
            d = (FA.astype(np.float64) - FB.astype(np.float64))
            mse64 = (d * d).reshape(N, -1).mean(axis=1)
            w64 = want([0, 1.0, 0])[0] * (-10.0 / (np.log(10.0) * mse64))[:, None, None, None]
            assert np.all(np.abs(x.grad.cpu().numpy() - w64) <= (ELEMENT + 10 * 2.0 ** -24) * np.abs(w64))
            calls = (spy.forward, spy.backward)
            # window 7 and no_grad are unchanged: torch for the first, the forward call alone for the second
            x = leaf(FA)
            s7 = M.ssim(x, y, 7)
            g7 = M.gaussian(7, 1.5).unsqueeze(1)
            win = g7.mm(g7.t())[None, None].expand(3, 1, 7, 7).contiguous().to(DEV)
            assert torch.equal(s7, M._ssim(x, y, win, 7, 3, True)) and (spy.forward, spy.backward) == calls
            with torch.no_grad():
                quiet = M.ssim(x, y)
            assert not quiet.requires_grad and (spy.forward, spy.backward) == (calls[0] + 1, calls[1])
            # a second backward through the function is refused, not approximated
            x = leaf(FA)
            (g1,) = torch.autograd.grad(M.ssim(x, y), x, create_graph=True)
            with pytest.raises(RuntimeError):
                g1.sum().backward()
    finally:
        M.set_device_backward(previous)
    assert M.device_backward() is False


def test_dssim_loss_is_one_forward_and_one_backward_call(M):
    y = torch.from_numpy(FB).to(DEV)
    lam = 0.2
    previous = M.set_device_backward(True)
    try:
        with Spies() as spy:
            x = leaf(FA)
            loss = M.dssim_loss(x, y, lam)
            loss.backward()
            assert (spy.forward, spy.backward) == (1, 1) and loss.dtype == torch.float32 and loss.shape == ()
            x2 = leaf(FA)
            composed = (1.0 - lam) * M.l1_loss(x2, y) + lam * (1.0 - M.ssim(x2, y))
            composed.backward()
            assert (spy.forward, spy.backward) == (3, 3)
        assert abs(loss.item() - composed.item()) <= 4 * 2.0 ** -24          # float32 roundings of two ways to one number below 1
        w64 = want([-lam / N, 0, (1.0 - lam) / N])[0]
        assert close(x.grad, w64) and close(x2.grad, w64)
    finally:
        M.set_device_backward(previous)


def test_the_switch_off_keeps_torch(M):
    y = torch.from_numpy(FB).to(DEV)
    assert M.device_backward() is False
    with Spies() as spy:
        x = leaf(FA)
        s = M.ssim(x, y)
        s.backward()
        loss = M.dssim_loss(leaf(FA), y)
        loss.backward()
        assert (spy.forward, spy.backward) == (0, 0)
    win = M.create_window(11, 3).to(DEV)
    x2 = leaf(FA)
    s2 = M._ssim(x2, y, win, 11, 3, True)
    s2.backward()
    assert torch.equal(s, s2) and x.grad is not None and x.grad.shape == x2.grad.shape
    x3 = leaf(FA)
    assert torch.equal(loss, 0.8 * torch.abs(x3 - y).mean() + 0.2 * (1.0 - M._ssim(x3, y, win, 11, 3, True)))
