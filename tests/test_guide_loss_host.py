"""The guide-view loss without a GPU: the restatement (tests/guide_loss_ref.py) held to the reference's own four lines in torch on the CPU -
the float64 form to F.interpolate on double input, the float32 gradient to torch's float32 autograd bit for bit; ties; the CPU surface of
``metrics.guide_l1_loss`` and ``GuideBank``; the three entries' declarations and exports; the refusals that need no device."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import guide_loss_cases as K
import guide_loss_ref as R
import pixel_ref as P
from test_pixel_ref_host import BILINEAR_TORCH_ULP

F32, F64 = np.float32, np.float64
T = lambda a: torch.from_numpy(np.array(a))
HOST_SHAPES = K.SHAPES + [K.WORKLOAD]


def reference_lines(image, guide_u8):
    """train.py:214-220 on tensors: to_tensor, F.interpolate to the render's size, l1_loss.  image [n,3,h,w], guide_u8 [n,gh,gw,3]."""
    image_guide_tensor = guide_u8.permute(0, 3, 1, 2).contiguous().to(torch.float32).div(255)
    if image.dtype == torch.float64:
        image_guide_tensor = image_guide_tensor.double()
    image_guide_resized = F.interpolate(image_guide_tensor, size=image.shape[-2:], mode="bilinear", align_corners=False)
    return torch.abs(image - image_guide_resized).mean(), image_guide_resized


@pytest.mark.parametrize("shape", HOST_SHAPES, ids=lambda s: "%dx%dx%d_from_%dx%d" % s)
def test_the_float64_form_is_f_interpolate_on_double_input(shape):
    guide, image = K.guide(shape), K.image_delta(shape)
    n, h, w = shape[:3]
    for i in range(n):          # train.py's loss is per view: one frame at a time
        want_loss, want_g = reference_lines(T(image[i:i + 1]).double(), T(guide[i:i + 1]))
        got_g = R.resampled(guide[i:i + 1], h, w, dtype=F64)
        assert np.abs(got_g - want_g.numpy()).max() <= 1e-12, shape
        assert abs(R.loss64(image[i:i + 1], guide[i:i + 1])[0] - want_loss.item()) <= 1e-12, shape


@pytest.mark.parametrize("shape", HOST_SHAPES, ids=lambda s: "%dx%dx%d_from_%dx%d" % s)
def test_the_float32_gradient_is_torchs_autograd_bit_for_bit(shape):
    """delta >= 2^-10 against torch's recorded distance from the restatement of BILINEAR_TORCH_ULP ulp of a value <= 1: no sample's sign
    can differ between the two."""
    assert K.DELTA_MIN / 2 > 100 * BILINEAR_TORCH_ULP * 2.0 ** -24
    guide, image = K.guide(shape), K.image_delta(shape)
    for i in range(shape[0]):
        x = T(image[i:i + 1].copy()).requires_grad_()
        want_loss, _ = reference_lines(x, T(guide[i:i + 1]))
        want_loss.backward()          # upstream weight 1
        got = R.grad(image[i:i + 1], guide[i:i + 1], [1.0])
        assert np.array_equal(got.view(np.uint32), x.grad.numpy().view(np.uint32)), P.mismatch_message("grad", got, x.grad.numpy())


def test_a_tie_gets_gradient_zero_and_equal_frames_loss_zero():
    image, tie = K.image_ties()
    guide = K.guide(K.SAME_SIZE)
    assert np.array_equal(R.resampled(guide, 3, 5), P.u8_to_f32(guide)), "the same size: g is p exactly"
    got = R.grad(image, guide, [1.0, -0.25])
    assert np.all(got[tie] == 0) and np.all(got[~tie] != 0)
    k0, k1 = F32(1.0 / 45.0), F32(-0.25 / 45.0)
    assert set(np.unique(np.abs(got[0][~tie[0]]))) == {k0} and set(np.unique(np.abs(got[1][~tie[1]]))) == {abs(k1)}
    same = P.u8_to_f32(guide)
    assert np.all(R.loss(same, guide) == 0) and np.all(R.terms(same, guide) == 0) and np.all(R.grad(same, guide, [1.0, 1.0]) == 0)
    # torch agrees: sign(0) = 0 under autograd
    x = T(same[:1].copy()).requires_grad_()
    loss, _ = reference_lines(x, T(guide[:1]))
    loss.backward()
    assert loss.item() == 0 and not x.grad.any()


def test_a_nan_sample_stays_in_its_frame_and_its_slot():
    shape = (2, 17, 65, 11, 23)
    image = K.image_delta(shape).copy()
    image[1, 2, 16, 64] = np.nan
    guide = K.guide(shape)
    loss, grad = R.loss(image, guide), R.grad(image, guide, [1.0, 1.0])
    assert not np.isnan(loss[0]) and np.isnan(loss[1])
    nan = np.isnan(grad)
    assert nan.sum() == 1 and nan[1, 2, 16, 64]
    assert np.all(R.grad(image, guide, [1.0, 0.0])[1] == 0), "a zero weight gives zeros whatever the samples"


# ---- applied_image_processing_amd.metrics on the CPU ------------------------------------------------------------------------------------------
def test_guide_l1_loss_on_cpu_tensors_is_the_reference_expression():
    import applied_image_processing_amd.metrics as M

    for shape in ((1, 5, 7, 2, 3), (2, 17, 65, 11, 23)):
        guide, image = T(K.guide(shape)), K.image_delta(shape)
        x, x2 = T(image.copy()).requires_grad_(), T(image.copy()).requires_grad_()
        got = M.guide_l1_loss(x, guide)
        want, _ = reference_lines(x2, guide)
        got.backward(), want.backward()
        assert got.dim() == 0 and got.dtype == torch.float32 and torch.equal(got, want) and torch.equal(x.grad, x2.grad)
        # one frame without its batch dimension
        one = M.guide_l1_loss(T(image[0]), guide[0])
        assert torch.equal(one, reference_lines(T(image[:1]), guide[:1])[0])
    # another channel count and another dtype take the same lines
    grey = torch.arange(6, dtype=torch.uint8).reshape(2, 3, 1)
    img = torch.rand(1, 4, 5, dtype=torch.float64)
    want = torch.abs(img - F.interpolate(grey.permute(2, 0, 1)[None].float().div(255), size=(4, 5), mode="bilinear", align_corners=False)[0]).mean()
    assert torch.equal(M.guide_l1_loss(img, grey), want)


def test_guide_bank_on_the_cpu(tmp_path):
    from PIL import Image

    import applied_image_processing_amd.metrics as M

    rng = np.random.default_rng(5)
    paths = {}
    for name, (gh, gw) in (("view_a", (32, 48)), ("view_b", (17, 23))):          # guides of different sizes
        smooth = np.clip(np.add.outer(np.linspace(0, 200, gh), np.linspace(0, 55, gw))[:, :, None] + rng.integers(0, 30, (gh, gw, 3)), 0, 255).astype(np.uint8)
        paths[name] = tmp_path / f"{name}.jpg"
        Image.fromarray(smooth).save(paths[name], quality=90)
    bank = M.GuideBank.from_files(paths, "cpu")
    assert len(bank) == 2 and "view_a" in bank and "view_c" not in bank and list(bank) == ["view_a", "view_b"]
    assert bank.nbytes == 32 * 48 * 3 + 17 * 23 * 3
    for name, path in paths.items():
        want = np.asarray(Image.open(path).convert("RGB"))
        assert bank[name].dtype == torch.uint8 and bank[name].device.type == "cpu" and np.array_equal(bank[name].numpy(), want)
    image = torch.rand(3, 40, 56).requires_grad_()
    loss = bank.loss(image, "view_b")
    assert torch.equal(loss, M.guide_l1_loss(image, bank["view_b"])) and torch.equal(loss, reference_lines(image[None], bank["view_b"][None])[0])
    loss.backward()
    assert image.grad is not None and image.grad.abs().max() > 0
    frames = torch.zeros(2, 4, 4, 3, dtype=torch.uint8)
    given = M.GuideBank.from_frames(["a", "b"], frames)
    assert given["b"].data_ptr() == frames[1].data_ptr() and given.nbytes == 96, "used as given"
    with pytest.raises(ValueError):
        M.GuideBank.from_frames(["a"], frames)
    with pytest.raises(KeyError):
        bank.loss(image, "view_c")


# ---- the built library, without a GPU -----------------------------------------------------------------------------------------------------------
ENTRIES = ("adain_guide_l1_f32_bytes", "adain_guide_l1_f32", "adain_guide_l1_grad_f32")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def rt():
    import applied_image_processing_amd.runtime as rt

    rt.lib()
    return rt


def test_the_entries_are_declared_bound_and_exported():
    import applied_image_processing_amd.runtime as rt

    header = open(os.path.join(ROOT, "include", "adain_hip.h")).read()
    for name in ENTRIES:
        assert re.search(rf"ADAIN_API int {name}\(", header), f"{name} is not declared in include/adain_hip.h"
        assert name in rt.SIGNATURES, f"{name} has no ctypes signature in runtime.py"
        assert hasattr(rt.lib(), name), f"{name} is not exported by the built library"
    assert "#define ADAIN_ABI_VERSION 4" in header and rt.lib().adain_abi_version() == 4
    from applied_image_processing_amd.engine import AdaINEngine

    assert callable(AdaINEngine.guide_l1) and callable(AdaINEngine.guide_l1_grad)
    assert callable(rt.guide_l1) and callable(rt.guide_l1_grad) and callable(rt.guide_l1_sizes)


def test_the_size_query_is_the_headers_formula(rt):
    up = lambda v: (v + 255) // 256 * 256
    for n, h, w in [s[:3] for s in K.SHAPES] + [(3, 130, 97), (64, 800, 800), (1, 1080, 1920)]:
        tiles = (h * ((w + 3) // 4) + 255) // 256
        assert rt.guide_l1_sizes(n, h, w) == up(8 * n * tiles), (n, h, w)
    L, b = rt.lib(), ctypes.c_size_t()
    assert L.adain_guide_l1_f32_bytes(1, 8, 8, None) == 0
    for dims, word in (((0, 8, 8), b"n "), ((65536, 8, 8), b"n "), ((1, 0, 8), b"h "), ((1, 8, -1), b"w "), ((1, 32768, 32768), b"2^31")):
        assert L.adain_guide_l1_f32_bytes(*dims, ctypes.byref(b)) == -1, dims
        assert b"guide_l1_f32" in L.adain_last_error() and word in L.adain_last_error(), dims


def test_the_refusals_that_need_no_device(rt):
    L = rt.lib()
    buf = ctypes.create_string_buffer(16384)
    p = (ctypes.addressof(buf) + 255) & ~255
    n, h, w, gh, gw = 2, 4, 4, 3, 5          # 384 bytes of image, 90 of guide, 16 of out and of weights, a workspace of 256
    image, guide, out, res, ws, wts, grad = p, p + 512, p + 1024, p + 1536, p + 2048, p + 2560, p + 3072
    size = rt.guide_l1_sizes(n, h, w)
    assert size == 256

    def forward(image=image, guide=guide, n=n, h=h, w=w, gh=gh, gw=gw, out=out, res=None, ws=ws, size=size):
        return L.adain_guide_l1_f32(image, guide, n, h, w, gh, gw, out, res, ws, size, None)

    def backward(image=image, guide=guide, n=n, h=h, w=w, gh=gh, gw=gw, wts=wts, grad=grad):
        return L.adain_guide_l1_grad_f32(image, guide, n, h, w, gh, gw, wts, grad, None)

    shapes = [(dict(n=0), b"n outside"), (dict(n=65536), b"n outside"), (dict(h=0), b"h below 1"), (dict(w=-1), b"w below 1"), (dict(gh=0), b"gh below 1"),
              (dict(gw=-3), b"gw below 1"), (dict(gh=32768, gw=32768), b"a guide beyond 2^31 - 1 samples")]
    refusals = [(forward, b"guide_l1_f32: ", shapes + [
        (dict(image=None), b"image is a null"), (dict(guide=None), b"guide is a null"), (dict(out=None), b"out is a null"), (dict(ws=None), b"workspace is a null"),
        (dict(h=32768, w=32768, size=1 << 62), b"a frame beyond 2^31 - 1 samples"), (dict(size=size - 1), b"workspace too small"),
        (dict(ws=ws + 4), b"workspace must be 8-byte aligned"), (dict(out=out + 4), b"out must be 8-byte aligned"), (dict(image=image + 2), b"image must be 4-byte aligned"),
        (dict(res=res + 1), b"resampled must be 4-byte aligned"),
        (dict(out=image + 376), b"out overlaps image"), (dict(out=guide + 88), b"out overlaps guide"), (dict(res=image + 380), b"resampled overlaps image"),
        (dict(res=guide + 88), b"resampled overlaps guide"), (dict(res=out - 380), b"resampled overlaps out"), (dict(ws=image + 8), b"workspace overlaps image"),
        (dict(ws=guide + 88), b"workspace overlaps guide"), (dict(ws=out + 8), b"workspace overlaps out"), (dict(res=res, ws=res + 376), b"workspace overlaps resampled")]),
        (backward, b"guide_l1_grad_f32: ", shapes + [
            (dict(image=None), b"image is a null"), (dict(guide=None), b"guide is a null"), (dict(wts=None), b"weights is a null"), (dict(grad=None), b"grad is a null"),
            (dict(h=32768, w=32768), b"a frame beyond 2^31 - 1 samples"), (dict(wts=wts + 4), b"weights must be 8-byte aligned"),
            (dict(image=image + 1), b"image must be 4-byte aligned"), (dict(grad=grad + 2), b"grad must be 4-byte aligned"),
            (dict(grad=image + 380), b"grad overlaps image"), (dict(grad=guide + 88), b"grad overlaps guide"), (dict(grad=wts + 12), b"grad overlaps weights")])]
    for call, prefix, cases in refusals:
        for kw, word in cases:
            assert call(**kw) == -1, (kw, word)
            message = L.adain_last_error()
            assert message.startswith(prefix) and word in message, (kw, message)
