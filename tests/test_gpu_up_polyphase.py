"""The decoder's up layers (nearest 2x upsample + ReflectionPad2d(1) + 3x3 conv) as four phase convolutions of the source in Winograd
F(5,2) x F(3,2), 4 x 3 outputs kept per tile (csrc/conv_wino4.hip, W4P; adain_conv3x3_up2x_poly).

CPU: the phase folding and the transforms restated in numpy reproduce the upsample + reflect + conv in float64 (the algebra the pack
and the kernel rest on).  GPU (``-m gpu``): the layer against a float64 torch reference on the decoder's three up shapes, ragged and
tiny maps and batches; a batch is bitwise the frames one by one; the per-layer error stays within 1.3x that of the F(4,3) x F(2,3)
kernel it replaces on the same inputs."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

# transforms of the kernel and its algebra in numpy: tests/conv_exact.py holds the one copy
from conv_exact import A3T, A5T, B2T, B4T, FOLD, G3, G5, polyphase  # noqa: F401


def reference(x, w):
    """x [cin][hs][ws], w [cout][cin][3][3] -> [cout][2 hs][2 ws], float64"""
    up = F.interpolate(torch.from_numpy(x)[None], scale_factor=2, mode="nearest")
    return F.conv2d(F.pad(up, (1, 1, 1, 1), mode="reflect"), torch.from_numpy(w))[0].numpy()


@pytest.mark.parametrize("cin,cout,hs,ws", [(3, 2, 7, 8), (2, 3, 1, 1), (4, 2, 2, 5), (2, 2, 11, 4)])
def test_polyphase_algebra_matches_upsample_reflect_conv(cin, cout, hs, ws):
    rng = np.random.default_rng(cin * 100 + hs * 10 + ws)
    x = rng.standard_normal((cin, hs, ws))
    w = rng.standard_normal((cout, cin, 3, 3))
    ref = reference(x, w)
    got = polyphase(x, w)
    assert np.abs(got - ref).max() <= 1e-11 * np.abs(ref).max()


# ---- GPU -------------------------------------------------------------------------------------------------------------------------------
def _layer(rt, cin, cout, seed):
    g = torch.Generator().manual_seed(seed)
    w = torch.randn(cout, cin, 3, 3, generator=g) * (2.0 / (9 * cin)) ** 0.5
    b = torch.randn(cout, generator=g) * 0.1
    return w, b


def _ref64(x_nhwc, w, b, relu=True):
    x = x_nhwc.double().permute(0, 3, 1, 2).cpu()
    up = F.interpolate(x, scale_factor=2, mode="nearest")
    y = F.conv2d(F.pad(up, (1, 1, 1, 1), mode="reflect"), w.double(), b.double())
    return (y.clamp_min(0) if relu else y).permute(0, 2, 3, 1)


def _rel(a, b):
    a, b = a.detach().cpu().double(), b.detach().cpu().double()
    return float((a - b).norm() / b.norm())


@pytest.fixture(scope="module")
def rt():
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    import applied_image_processing_amd.runtime as rt

    rt.lib()
    return rt


SHAPES = [  # (n, cin, cout, hs, ws): the decoder's three up layers at config-2 sizes, ragged, tiny and batched maps
    (1, 256, 256, 128, 128), (1, 128, 128, 256, 256), (1, 64, 64, 512, 512),
    (1, 64, 64, 37, 53), (1, 128, 64, 1, 1), (1, 64, 32, 2, 9), (1, 16, 32, 21, 25), (3, 64, 64, 45, 31), (2, 256, 256, 16, 24),
]


@pytest.mark.gpu
@pytest.mark.parametrize("n,cin,cout,hs,ws", SHAPES)
def test_up_layer_against_float64(rt, n, cin, cout, hs, ws):
    w, b = _layer(rt, cin, cout, cin + cout + hs)
    x = torch.rand(n, hs, ws, cin, generator=torch.Generator().manual_seed(hs * ws)) * 2
    for relu in (True, False):
        got = rt.conv3x3_up2x_poly(x.cuda(), rt.conv3x3_up2x_poly_pack(w.cuda()), b.cuda(), cout, relu=relu)
        torch.cuda.synchronize()
        ref = _ref64(x, w, b, relu)
        assert got.shape == ref.shape
        assert torch.isfinite(got).all()
        assert _rel(got, ref) < 1e-5, (relu, _rel(got, ref))


@pytest.mark.gpu
def test_batch_is_bitwise_frame_by_frame(rt):
    cin, cout = 128, 128
    w, b = _layer(rt, cin, cout, 7)
    pw, bb = rt.conv3x3_up2x_poly_pack(w.cuda()), b.cuda()
    x = (torch.rand(3, 50, 70, cin, generator=torch.Generator().manual_seed(3)) * 2).cuda()
    whole = rt.conv3x3_up2x_poly(x, pw, bb, cout)
    for i in range(3):
        one = rt.conv3x3_up2x_poly(x[i:i + 1].contiguous(), pw, bb, cout)
        assert torch.equal(one[0], whole[i])


@pytest.mark.gpu
@pytest.mark.parametrize("cin,cout,hs,ws", [(256, 256, 128, 128), (128, 128, 96, 80), (64, 64, 200, 150)])
def test_error_within_the_wino4_kernel_s(rt, cin, cout, hs, ws):
    w, b = _layer(rt, cin, cout, 11)
    x = torch.rand(1, hs, ws, cin, generator=torch.Generator().manual_seed(5)) * 2
    ref = _ref64(x, w, b)
    poly = rt.conv3x3_up2x_poly(x.cuda(), rt.conv3x3_up2x_poly_pack(w.cuda()), b.cuda(), cout)
    old = rt.conv3x3_wino(x.cuda(), rt.conv3x3_wino_pack(w.cuda()), b.cuda(), cout, src_mode=rt.SRC_UP2X)
    torch.cuda.synchronize()
    assert _rel(poly, ref) <= 1.3 * _rel(old, ref), (_rel(poly, ref), _rel(old, ref))


@pytest.mark.gpu
def test_rejects_what_it_cannot_run(rt):
    w, b = _layer(rt, 24, 32, 1)
    with pytest.raises(rt.AdainHipError):
        rt.conv3x3_up2x_poly(torch.zeros(1, 4, 4, 24).cuda(), rt.conv3x3_up2x_poly_pack(w.cuda()), b.cuda(), 32)
