"""adain_guide_l1_f32 and adain_guide_l1_grad_f32 held to tests/guide_loss_ref.py over every shape, byte offset and dispatch path of
tests/guide_loss_cases.py: the resampled guide and the gradient bit for bit, the loss within the derived bound N 2^-52 ref.loss, and a
frame's bits independent of the batch, the stream and what the workspace held."""
import numpy as np
import pytest
import torch

import guide_loss_cases as K
import guide_loss_ref as R
import pixel_ref as P

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
CASES = K.cases()
WEIGHTS = (1.0, -0.25)

# every branch of the two launchers is taken by a case
_TAKEN = {K.select(call, s[2], fo, fo) for s, _go, fo in CASES for call in ("guide_l1", "guide_l1_grad")}
assert _TAKEN == set(K.DISPATCH), sorted(set(K.DISPATCH) - _TAKEN)


@pytest.fixture(scope="module")
def rt():
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    import applied_image_processing_amd.runtime as rt

    rt.lib()
    torch.cuda.set_device(0)
    return rt


def place(host, offset, boundary=16):
    """``host`` (numpy) on the device at ``offset`` bytes behind a ``boundary``-byte boundary -> (pointer, the uint8 view that owns it)."""
    nbytes = host.nbytes
    buf = torch.empty(nbytes + 2 * boundary + offset, dtype=torch.uint8, device=DEV)
    start = (-buf.data_ptr()) % boundary + offset
    view = buf[start:start + nbytes]
    view.copy_(torch.from_numpy(np.array(host, order="C")).view(-1).view(torch.uint8))
    assert (view.data_ptr() - offset) % boundary == 0
    return view.data_ptr(), view


def room(nbytes, offset, boundary=16, fill=0xFF):
    return place(np.full(nbytes, fill, dtype=np.uint8), offset, boundary)


def forward(rt, image, guide, guide_off=0, float_off=0, with_resampled=True, ws_fill=0xFF, stream=None):
    """-> (out float64 [n], resampled float32 of the image's shape or None) as numpy."""
    n, _, h, w = image.shape
    gh, gw = guide.shape[1:3]
    pi, _ki = place(image, float_off)
    pg, _kg = place(guide, guide_off, boundary=4)
    po, out = room(8 * n, 0)
    pr, res = room(image.nbytes, float_off) if with_resampled else (None, None)
    nbytes = rt.guide_l1_sizes(n, h, w)
    pw, _kw = room(nbytes, 0, boundary=256, fill=ws_fill)
    s = stream if stream is not None else torch.cuda.current_stream()
    rc = rt.lib().adain_guide_l1_f32(pi, pg, n, h, w, gh, gw, po, pr, pw, nbytes, s.cuda_stream)
    assert rc == 0, rt.lib().adain_last_error().decode()
    s.synchronize()
    return out.cpu().numpy().view(np.float64).copy(), (res.cpu().numpy().view(np.float32).reshape(image.shape).copy() if with_resampled else None)


def backward(rt, image, guide, weights, guide_off=0, float_off=0, stream=None):
    n, _, h, w = image.shape
    gh, gw = guide.shape[1:3]
    pi, _ki = place(image, float_off)
    pg, _kg = place(guide, guide_off, boundary=4)
    pw, _kw = place(np.asarray(weights, dtype=np.float64), 0)
    pgr, grad = room(image.nbytes, float_off)
    s = stream if stream is not None else torch.cuda.current_stream()
    rc = rt.lib().adain_guide_l1_grad_f32(pi, pg, n, h, w, gh, gw, pw, pgr, s.cuda_stream)
    assert rc == 0, rt.lib().adain_last_error().decode()
    s.synchronize()
    return grad.cpu().numpy().view(np.float32).reshape(image.shape).copy()


def same_bits(got, want):
    return np.array_equal(np.ascontiguousarray(got).view(np.uint8), np.ascontiguousarray(want).view(np.uint8))


@pytest.mark.parametrize("case", CASES, ids=K.case_id)
def test_forward_and_gradient_are_the_restatement(rt, case):
    shape, guide_off, float_off = case
    n, h, w = shape[:3]
    guide, image = K.guide(shape), K.image_delta(shape)
    out, res = forward(rt, image, guide, guide_off, float_off)
    assert same_bits(res, K.g_ref(shape)), P.mismatch_message("resampled", res, K.g_ref(shape))
    # what adain_u8_to_f32 then adain_resize_bilinear write for the same guide
    chained = rt.resize_bilinear(rt.u8_to_f32(torch.from_numpy(np.array(guide)).to(DEV)), (h, w)).cpu().numpy()
    assert same_bits(res, chained), P.mismatch_message("resampled against u8_to_f32 + resize_bilinear", res, chained)
    want = R.loss(image, guide)
    bound = R.loss_bound(image, want)
    print(K.case_id(case), "out", out, "ref", want, "|out - ref|", np.abs(out - want), "bound", bound)
    assert np.all(np.abs(out - want) <= bound)
    bare, _ = forward(rt, image, guide, guide_off, float_off, with_resampled=False)
    assert same_bits(bare, out), "out differs with and without resampled"
    weight_sets = [[wt] * n for wt in WEIGHTS] + ([[0.75, -2.0]] if n == 2 else [])
    for weights in weight_sets:
        got, want_grad = backward(rt, image, guide, weights, guide_off, float_off), R.grad(image, guide, weights)
        assert same_bits(got, want_grad), P.mismatch_message(f"grad at weights {weights}", got, want_grad)


def test_ties_get_zero(rt):
    image, tie = K.image_ties()
    guide = K.guide(K.SAME_SIZE)
    got = backward(rt, image, guide, [1.0, -0.25])
    assert same_bits(got, R.grad(image, guide, [1.0, -0.25])) and np.all(got[tie] == 0) and np.all(got[~tie] != 0)
    same = P.u8_to_f32(guide)
    out, _ = forward(rt, same, guide)
    assert np.all(out == 0) and np.all(backward(rt, same, guide, [1.0, 1.0]) == 0)


@pytest.mark.parametrize("shape", [(2, 17, 65, 11, 23), (2, 33, 128, 20, 50)], ids=["scalar", "vec"])
def test_a_frames_bits_do_not_depend_on_batch_stream_or_workspace(rt, shape):
    guide, image = K.guide(shape), K.image_delta(shape)
    weights = [0.75, -2.0]
    out, _ = forward(rt, image, guide, with_resampled=False)
    grad = backward(rt, image, guide, weights)
    side = torch.cuda.Stream()
    for i in (0, 1):
        alone, _ = forward(rt, image[i:i + 1], guide[i:i + 1], with_resampled=False)
        assert same_bits(alone, out[i:i + 1]), f"frame {i} alone"
        assert same_bits(backward(rt, image[i:i + 1], guide[i:i + 1], weights[i:i + 1]), grad[i:i + 1]), f"frame {i} alone"
    flipped, _ = forward(rt, image[::-1], guide[::-1], with_resampled=False)
    assert same_bits(flipped, out[::-1]) and same_bits(backward(rt, image[::-1], guide[::-1], weights[::-1]), grad[::-1]), "the frames in the other order"
    for fill in (0xA5, 0x00):
        again, _ = forward(rt, image, guide, with_resampled=False, ws_fill=fill)
        assert same_bits(again, out), f"workspace filled with {fill:#x}"
    torch.cuda.synchronize()
    on_side, _ = forward(rt, image, guide, with_resampled=False, stream=side)
    assert same_bits(on_side, out) and same_bits(backward(rt, image, guide, weights, stream=side), grad), "a side stream"


def test_weight_zero_gives_zeros_and_a_nan_stays_in_its_frame_and_slot(rt):
    shape = (2, 17, 65, 11, 23)
    guide, image = K.guide(shape), K.image_delta(shape).copy()
    image[1, 2, 16, 64] = np.nan
    out, _ = forward(rt, image, guide)
    assert not np.isnan(out[0]) and np.isnan(out[1])
    clean, _ = forward(rt, K.image_delta(shape), guide)
    assert same_bits(out[:1], clean[:1]), "frame 0 is untouched by frame 1's NaN"
    grad = backward(rt, image, guide, [1.0, 1.0])
    nan = np.isnan(grad)
    assert nan.sum() == 1 and nan[1, 2, 16, 64] and same_bits(grad, R.grad(image, guide, [1.0, 1.0]))
    zeroed = backward(rt, image, guide, [1.0, 0.0])
    assert same_bits(zeroed, R.grad(image, guide, [1.0, 0.0])) and not zeroed[1].view(np.uint32).any(), "a zero weight gives +0 whatever the samples"
    assert not backward(rt, K.image_delta(shape), guide, [0.0, 0.0]).view(np.uint32).any()


def test_the_wrappers_hand_over_the_same_call(rt):
    shape = (2, 33, 128, 20, 50)
    guide, image = K.guide(shape), K.image_delta(shape)
    out, res = forward(rt, image, guide)
    x, g = torch.from_numpy(np.array(image)).to(DEV), torch.from_numpy(np.array(guide)).to(DEV)
    got = rt.guide_l1(x, g, resampled=True)
    assert same_bits(got.l1.cpu().numpy(), out) and same_bits(got.resampled.cpu().numpy(), res) and rt.guide_l1(x, g).resampled is None
    wts = torch.tensor([0.75, -2.0], dtype=torch.float64, device=DEV)
    assert same_bits(rt.guide_l1_grad(x, g, wts).cpu().numpy(), backward(rt, image, guide, [0.75, -2.0]))
    one = rt.guide_l1(x[0], g[0], resampled=True)
    assert one.l1.shape == (1,) and one.resampled.shape == x[0].shape and same_bits(one.l1.cpu().numpy(), out[:1])
    from applied_image_processing_amd.engine import AdaINEngine

    assert AdaINEngine.guide_l1 is not None
    for bad in (lambda: rt.guide_l1(x.cpu(), g), lambda: rt.guide_l1(x, g[:1]), lambda: rt.guide_l1(x[:, :2], g), lambda: rt.guide_l1_grad(x, g, wts[:1]),
                lambda: rt.guide_l1_grad(x, g, wts.float())):
        with pytest.raises(rt.AdainHipError):
            bad()
