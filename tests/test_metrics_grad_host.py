"""The gradient of the image metrics without a GPU: the float64 restatement (tests/metrics_grad_ref.py) held to torch's float64 autograd of
``metrics._ssim``, ``l1_loss`` and ``l2_loss``; the recorded float32 noise (tests/golden/metrics/grad_noise.json) and three wrong forms
that its bar must tell apart; the refusals of adain_image_metrics_grad_f32 that need no device, its size query and its declarations; and
the CPU surface of the switch and of ``dssim_loss``."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import metrics_cases as C
import metrics_grad_cases as K
import metrics_grad_ref as G

TILE_EDGE, WEIGHTS, edge_pair = K.TILE_EDGE, K.WEIGHTS, K.edge_pair


def cases():
    out = {f"{family}_{h}x{w}": (family, 2, 3, h, w) for family in C.FAMILIES for h, w in C.GOLDEN_SIZES}
    out.update({"edge_%dx%dx%dx%d" % s: ("edge",) + s for s in TILE_EDGE})
    return out


CASES = cases()


def frames(name):
    family, n, c, h, w = CASES[name]
    if family == "edge":
        return edge_pair((n, c, h, w))
    a, b = C.pair(family, n, h, w, c)
    return C.to_nchw_f32(a), C.to_nchw_f32(b)


def torch_grads(a, b, weights):
    """torch's float64 autograd of sum_i w[i,0] ssim_i + w[i,1] mse_i + w[i,2] l1_i through the package's own torch expressions."""
    import applied_image_processing_amd.metrics as M

    x, y = torch.from_numpy(a).double().requires_grad_(), torch.from_numpy(b).double().requires_grad_()
    wt = torch.tensor(weights, dtype=torch.float64)
    c = x.shape[1]
    window = M.create_window(11, c).double()
    total = (wt[:, 0] * M._ssim(x, y, window, 11, c, False)).sum()
    for i in range(x.shape[0]):
        total = total + wt[i, 1] * M.l2_loss(x[i:i + 1], y[i:i + 1]) + wt[i, 2] * M.l1_loss(x[i:i + 1], y[i:i + 1])
    total.backward()
    return x.grad.numpy(), y.grad.numpy()


@pytest.mark.parametrize("name", list(CASES))
def test_the_restatement_is_torchs_float64_autograd(name):
    a, b = frames(name)
    n = a.shape[0]
    assert all(not np.array_equal(a[i], b[i]) for i in range(n)), "equal frames have no unit to measure in"
    for kind, weights in WEIGHTS.items():
        weights = weights[:n]
        got, want = G.grad(a, b, weights), torch_grads(a, b, weights)
        for which in (0, 1):
            d = G.distance(got[which], want[which])
            print(name, kind, "ab"[which], d.max())
            assert d.max() <= 1e-10, (name, kind, which, d)


@pytest.fixture(scope="module")
def bars():
    return K.bars()


def test_the_fixture_has_its_keys_and_the_bars_are_the_rule(bars):
    assert sorted(bars) == ["R_equal", "R_grad", "S_equal", "S_grad", "bar_equal", "bar_grad", "torch"]
    assert bars["bar_grad"] == 2 * max(bars["R_grad"], bars["S_grad"]) > 0 and bars["bar_equal"] == 2 * max(bars["R_equal"], bars["S_equal"]) > 0
    assert all(bars[k] >= 0 for k in ("R_grad", "S_grad", "R_equal", "S_equal"))


def test_the_bar_tells_three_wrong_forms_apart(bars):
    """Reflect padding, the adjoint window one tap off, and the 2 x conv(d_e11) term left out: on at least one committed case each must
    miss the restatement by ten bars or more, or the bar could not tell that mistake from float32 noise."""
    z = C.load_golden()
    worst = {"reflect": 0.0, "shift": 0.0, "drop": 0.0}
    for name in C.golden_names():
        a8, b8 = C.golden_pair(z, name)
        if a8.shape[1] < 6 or a8.shape[2] < 6:          # numpy's reflect padding of 5 needs 6 samples
            continue
        a, b = C.to_nchw_f32(a8), C.to_nchw_f32(b8)
        differ = [i for i in range(a.shape[0]) if not np.array_equal(a[i], b[i])]
        if not differ:
            continue
        a, b = a[differ], b[differ]
        weights = [[1.0, 0.0, 0.0]] * len(differ)
        want = G.grad(a, b, weights)
        for key, kw in (("reflect", dict(pad="reflect")), ("shift", dict(shift=1)), ("drop", dict(drop_e11=True))):
            got = G.grad(a, b, weights, **kw)
            worst[key] = max(worst[key], max(float(G.distance(got[k], want[k]).max()) for k in (0, 1)))
    print(worst, bars["bar_grad"])
    for key, value in worst.items():
        assert value >= 10 * bars["bar_grad"], (key, value, bars["bar_grad"])


# ---- the built library, without a GPU -----------------------------------------------------------------------------------------------------------
ENTRIES = ("adain_image_metrics_grad_f32_bytes", "adain_image_metrics_grad_f32")


@pytest.fixture(scope="module")
def rt():
    import applied_image_processing_amd.runtime as rt

    rt.lib()
    return rt


def test_the_entries_are_declared_bound_and_exported(rt):
    header = open(os.path.join(os.path.dirname(C.GOLDEN), os.pardir, os.pardir, "include", "adain_hip.h")).read()
    for name in ENTRIES:
        assert re.search(rf"ADAIN_API int {name}\(", header) and name in rt.SIGNATURES and hasattr(rt.lib(), name), name
    assert "#define ADAIN_ABI_VERSION 4" in header and rt.lib().adain_abi_version() == 4
    from applied_image_processing_amd.engine import AdaINEngine

    assert callable(AdaINEngine.image_metrics_grad) and callable(rt.image_metrics_grad) and callable(rt.image_metrics_grad_sizes)


def test_the_size_query_is_the_headers_formula(rt):
    up = lambda v: (v + 255) // 256 * 256
    for n, c, h, w in TILE_EDGE + ((3, 3, 130, 97), (64, 3, 135, 240), (1, 3, 1080, 1920)):
        plane = up(4 * n * c * h * w)
        assert rt.image_metrics_grad_sizes(n, c, h, w) == 3 * plane and rt.image_metrics_grad_sizes(n, c, h, w, grad_b=True) == 5 * plane
    L, b = rt.lib(), ctypes.c_size_t()
    assert L.adain_image_metrics_grad_f32_bytes(1, 4, 8, 8, 0, None) == 0
    for dims, word in (((1, 0, 8, 8), b"c "), ((1, 5, 8, 8), b"c "), ((0, 3, 8, 8), b"n "), ((65536, 3, 8, 8), b"n "), ((1, 3, 0, 8), b"h "), ((1, 3, 8, -1), b"w "),
                       ((1, 4, 32768, 32768), b"2^31")):
        for with_b in (0, 1):
            assert L.adain_image_metrics_grad_f32_bytes(*dims, with_b, ctypes.byref(b)) == -1, dims
            assert b"image_metrics_grad_f32" in L.adain_last_error() and word in L.adain_last_error(), dims


def test_the_refusals_that_need_no_device(rt):
    L = rt.lib()
    buf = ctypes.create_string_buffer(16384)
    p = (ctypes.addressof(buf) + 255) & ~255
    n, c, h, w = 2, 3, 4, 4          # 384 bytes a clip, 48 bytes of weights, planes of 512 bytes
    a, b, wts, ga, gb, ws = p, p + 512, p + 1024, p + 1536, p + 2048, p + 4096
    size3, size5 = rt.image_metrics_grad_sizes(n, c, h, w), rt.image_metrics_grad_sizes(n, c, h, w, grad_b=True)
    assert (size3, size5) == (1536, 2560)

    def call(a=a, b=b, n=n, c=c, h=h, w=w, wts=wts, ga=ga, gb=None, ws=ws, size=size5):
        return L.adain_image_metrics_grad_f32(a, b, n, c, h, w, wts, ga, gb, ws, size, None)

    refusals = [
        (dict(a=None), b"a is a null"), (dict(b=None), b"b is a null"), (dict(wts=None), b"weights is a null"), (dict(ga=None), b"grad_a is a null"),
        (dict(ws=None), b"workspace is a null"), (dict(c=0), b"c outside 1..4"), (dict(c=5), b"c outside 1..4"), (dict(n=0), b"n outside"), (dict(n=65536), b"n outside"),
        (dict(h=0), b"h below 1"), (dict(w=-1), b"w below 1"), (dict(h=32768, w=32768, size=1 << 62), b"2^31 - 1 samples"),
        (dict(size=size3 - 1), b"workspace too small"), (dict(gb=gb, size=size5 - 1), b"workspace too small"),
        (dict(ws=ws + 4), b"workspace must be 8-byte aligned"), (dict(wts=wts + 4), b"weights must be 8-byte aligned"),
        (dict(a=a + 2), b"a must be 4-byte aligned"), (dict(b=b + 1), b"b must be 4-byte aligned"), (dict(ga=ga + 2), b"grad_a must be 4-byte aligned"),
        (dict(gb=gb + 3), b"grad_b must be 4-byte aligned"),
        (dict(ga=a + 380), b"grad_a overlaps a"), (dict(ga=b + 380), b"grad_a overlaps b"), (dict(ga=wts + 44), b"grad_a overlaps weights"),
        (dict(gb=a + 4), b"grad_b overlaps a"), (dict(gb=b + 4), b"grad_b overlaps b"), (dict(gb=wts + 4), b"grad_b overlaps weights"),
        (dict(gb=ga + 380), b"grad_b overlaps grad_a"), (dict(gb=ga), b"grad_b overlaps grad_a"),
        (dict(ws=a + 8), b"workspace overlaps a"), (dict(ws=b + 8), b"workspace overlaps b"), (dict(ws=wts + 40), b"workspace overlaps weights"),
        (dict(ws=ga + 8, size=size3), b"workspace overlaps grad_a"), (dict(gb=gb, ws=gb + 376), b"workspace overlaps grad_b"),
    ]
    for kw, word in refusals:
        assert call(**kw) == -1, (kw, word)
        message = L.adain_last_error()
        assert message.startswith(b"image_metrics_grad_f32: ") and word in message, (kw, message)
    # the same buffer for a and b is no overlap: both are inputs (the call itself needs a device)


# ---- applied_image_processing_amd.metrics on the CPU ------------------------------------------------------------------------------------------
def test_the_switch_returns_the_previous_value_and_the_cpu_route_is_the_composed_expression():
    import applied_image_processing_amd.metrics as M

    assert M.device_backward() is False, "off by default"
    a, b = frames("near_12x33")
    try:
        assert M.set_device_backward(True) is False and M.device_backward() is True
        assert M.set_device_backward(True) is True
        for enabled in (True, False):
            M.set_device_backward(enabled)
            for lam in (0.2, 0.5):
                x, y = torch.from_numpy(a).requires_grad_(), torch.from_numpy(b)
                got = M.dssim_loss(x, y, lam)
                got.backward()
                x2 = torch.from_numpy(a).requires_grad_()
                want = (1.0 - lam) * M.l1_loss(x2, y) + lam * (1.0 - M.ssim(x2, y))
                want.backward()
                assert torch.equal(got, want) and torch.equal(x.grad, x2.grad) and got.dtype == torch.float32
            assert torch.equal(M.dssim_loss(torch.from_numpy(a[0]), torch.from_numpy(b[0])),
                               0.8 * M.l1_loss(torch.from_numpy(a[0]), torch.from_numpy(b[0])) + 0.2 * (1.0 - M.ssim(torch.from_numpy(a[0]), torch.from_numpy(b[0]))))
        assert M.set_device_backward(False) is False
    finally:
        M.set_device_backward(False)
    assert M.device_backward() is False
