"""Far-batch tests of the image metrics and their gradient (csrc/metrics.hip), the guide-view loss and its gradient (csrc/guide_loss.hip),
CORAL (csrc/coral.hip), the AdaIN statistics and blends (csrc/stats.hip), the layout transposes (csrc/pixel.hip), single 3 x 3 conv layers
(csrc/conv_wino4.hip: adain_conv3x3_wino direct and the polyphase up layer) and the encoder's first layer (csrc/conv_edge.hip through
adain_encode_relu1_1): one call whose buffers pass 2^32 bytes (the case table says which, per call), every frame compared with the result of its
pattern.  tests/far_batch.py states the design and holds the cases.  Run with ``-m gpu``.

The bar is the one the call's own tests use.  Equality: the blends against blend_ref's float32 form, the transposes against numpy,
the mixes against mix_ref's float32 form, the conv layers against conv_exact's and the first layer against edge_exact's float64
convolution of integer operands, the uint8 metrics' mse and l1 against the exact integer ratios.  Where the bar is a tolerance - SSIM and its map (tests/golden/metrics/noise.json), the float metrics' mse / l1 and psnr
(test_gpu_metrics.py), the metrics' gradient (bar_grad of tests/golden/metrics/grad_noise.json, and per element where a row has no ssim
weight, test_gpu_metrics_grad.py), the guide-view loss (N 2^-52 of the exact sum's quotient, test_gpu_guide_loss.py), CORAL's record and
pixels (test_gpu_coral.py), mean and std (1 and 2 float32 ulp, test_gpu_blend_stats.py) - the device's own result on the P frames alone
is held to it, and every frame of the batch must be that result bit for bit.  The resampled guide and the guide loss's gradient are the
restatement's bits (tests/guide_loss_ref.py) on the P frames and in the batch.

Out of scope here as everywhere in the far-batch tests: the keys of far_batch.OUT_OF_SCOPE, each with its reason.

Measured on an MI355X, seconds per test (fill, call and comparison):
image_metrics_u8 0.54, image_metrics_f32 0.08, conv3x3_up2x_poly 0.06, coral/u8 0.05, conv3x3_wino 0.03, coral/f32 0.02, the transposes
0.02 each (4.81 for the one that makes the process's first large allocations), blend_mix/nhwc_maps 1.14, blend_pmap/c1 0.89,
blend_mix/maps 0.04, blend_alpha, blend_pmap and blend_alpha/nhwc 0.02 each, mean_std and mean_std/nhwc 0.01 (0.26 for the first),
image_metrics_grad_f32 0.56, guide_l1_f32 0.04, guide_l1_grad_f32 0.03, encode_relu1_1 0.48."""
import json
import math
import os

import numpy as np
import pytest
import torch

import far_batch as B

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
F32_REL = 8 * 2.0 ** -24          # test_gpu_metrics.py's
PSNR_OF_REL = 10 / math.log(10)
PSNR_ULPS = 8 * 2.0 ** -46


@pytest.fixture(scope="module")
def rt():
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    import applied_image_processing_amd.runtime as rt

    rt.lib()
    torch.cuda.set_device(0)
    return rt


@pytest.fixture(scope="module")
def bars():
    import metrics_cases as C

    with open(os.path.join(C.GOLDEN, "noise.json")) as f:
        return json.load(f)


# ---- metrics ------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("id", ["image_metrics_u8", "image_metrics_f32"])
def test_image_metrics(rt, bars, id):
    case = B.BY_ID[id]
    (a, b), (want, want_map) = case.make()
    u8 = a.dtype == np.uint8
    B.reserve(case, DEV)
    # the P pairs alone, held to the bars of test_gpu_metrics.py
    small = rt.image_metrics(B.upload(a, DEV), B.upload(b, DEV), ssim_map=True)
    torch.cuda.synchronize()
    got, smap = small.records.cpu().numpy(), small.ssim_map.cpu().numpy()
    assert np.abs(got[:, 0] - want[:, 0]).max() <= bars["bar_frame"] and np.abs(smap.astype(np.float64) - want_map).max() <= bars["bar_map"]
    if u8:
        assert got[:, 1].tolist() == want[:, 1].tolist() and got[:, 2].tolist() == want[:, 2].tolist()          # exact
    else:
        assert np.all(np.abs(got[:, 1:3] - want[:, 1:3]) <= F32_REL * want[:, 1:3])
    for g, w in zip(got[:, 3], want[:, 3]):
        assert g == w if math.isinf(w) else abs(g - w) <= (0 if u8 else PSNR_OF_REL * F32_REL) + PSNR_ULPS * 128, (g, w)
    assert B.distinct(got), "two patterns score alike: a frame read from the wrong place could pass"
    # the batch: every record and every map the device's own for the pattern
    dims = a.shape[1:]
    sizes = dict((x[0], x[2]) for x in case.buffers())
    A_, B_ = B.tile(a, case.n, DEV), B.tile(b, case.n, DEV)
    out = B.poisoned((case.n, 4), torch.float64, DEV)
    omap = B.poisoned((case.n,) + dims, torch.float32, DEV)
    ws = B.poisoned((sizes["workspace"],), torch.uint8, DEV)
    try:
        assert sum(t.numel() * t.element_size() for t in (A_, B_, out, omap, ws)) == case.total_bytes()
        rt.call(case.call, torch.device(DEV), A_.data_ptr(), B_.data_ptr(), case.n, *dims, out.data_ptr(), omap.data_ptr(), ws.data_ptr(), ws.numel())
        torch.cuda.synchronize()
        B.assert_frames(id + ": records", out, small.records)
        B.assert_frames(id + ": ssim_map", omap, small.ssim_map)
        B.assert_frames(id + ": a changed", A_, a)
        B.assert_frames(id + ": b changed", B_, b)
    finally:
        del A_, B_, out, omap, ws, small
        rt.free_workspaces()
        B.release()


# ---- the metrics' gradient ----------------------------------------------------------------------------------------------------------------------------
GRAD_ELEMENT = 4 * 2.0 ** -24          # test_gpu_metrics_grad.py's, for a gradient of one term: three roundings and one to spare
# The row without an ssim weight, (x - y) k_mse + sign k_l1 with both weights positive: the difference, the scalar and their product round
# once each, the l1 scalar once, the sum once, and the two terms have the sign of x - y, so nothing cancels: (1 + 2^-24)^4 - 1 < 5 x 2^-24
GRAD_NO_SSIM = 5 * 2.0 ** -24


def test_image_metrics_grad(rt):
    """grad_a of 65535 pairs of three planes under seven kinds of weights (far_batch.GRAD_ROWS), without grad_b (37 GiB, past the cap)."""
    import metrics_grad_cases as K
    import metrics_grad_ref as G

    id = "image_metrics_grad_f32"
    case = B.BY_ID[id]
    (a, b, weights), (want,) = case.make()
    bar = K.bars()["bar_grad"]
    B.reserve(case, DEV)
    # the P pairs alone, held to the bars of test_gpu_metrics_grad.py
    small = rt.image_metrics_grad(B.upload(a, DEV), B.upload(b, DEV), B.upload(weights, DEV))
    torch.cuda.synchronize()
    got = small.cpu().numpy()
    for k, (kind, _row) in enumerate(B.GRAD_ROWS):
        g, w64 = got[k], want[k]
        if kind == "zero":
            assert np.all(g == 0.0), "a frame whose weights are all zero gets zeros"
            continue
        d = float(G.distance(g[None], w64[None])[0])
        print(id, k, kind, "distance", d, "bar", bar)
        assert d <= bar, (k, kind, d)
        if kind in ("mse", "l1", "no_ssim"):          # and the tighter bar of a gradient without the window
            worst = float((np.abs(g - w64) / np.maximum(np.abs(w64), 1e-300)).max())
            print(id, k, kind, "elementwise", worst)
            assert np.all(np.abs(g - w64) <= (GRAD_NO_SSIM if kind == "no_ssim" else GRAD_ELEMENT) * np.abs(w64)), (k, kind, worst)
            assert np.array_equal(np.sign(g), np.sign(w64)), (k, kind, "the sign of x - y is exact")
    assert B.distinct(got), "two patterns have one gradient: a frame read from the wrong place could pass"
    # the batch: every frame's gradient the device's own for the pattern
    dims = a.shape[1:]
    sizes = dict((x[0], x[2]) for x in case.buffers())
    A_, B_, W_ = B.tile(a, case.n, DEV), B.tile(b, case.n, DEV), B.tile(weights, case.n, DEV)
    grad = B.poisoned((case.n,) + dims, torch.float32, DEV)
    ws = B.poisoned((sizes["workspace"],), torch.uint8, DEV)
    try:
        assert sum(t.numel() * t.element_size() for t in (A_, B_, W_, grad, ws)) == case.total_bytes()
        rt.call(case.call, torch.device(DEV), A_.data_ptr(), B_.data_ptr(), case.n, *dims, W_.data_ptr(), grad.data_ptr(), None, ws.data_ptr(), ws.numel())
        torch.cuda.synchronize()
        B.assert_frames(id + ": grad_a", grad, small)
        B.assert_frames(id + ": a changed", A_, a)
        B.assert_frames(id + ": b changed", B_, b)
        B.assert_frames(id + ": the weights changed", W_, weights)
    finally:
        del A_, B_, W_, grad, ws, small
        rt.free_workspaces()
        B.release()


# ---- the guide-view loss ------------------------------------------------------------------------------------------------------------------------------
def test_guide_l1(rt):
    """The vector kernel (w % 4 == 0) with the resampled guide: renders, guides and resampled guides pass 2^32 bytes."""
    import guide_loss_ref as R

    id = "guide_l1_f32"
    case = B.BY_ID[id]
    (image, guide), (want, want_g) = case.make()
    h, w = B.GUIDE_L1_HW
    B.reserve(case, DEV)
    # the P frames alone, by test_gpu_guide_loss.py's rule: the resampled guide bit for bit, the loss within N 2^-52 of the exact sum's
    small = rt.guide_l1(B.upload(image, DEV), B.upload(guide, DEV), resampled=True)
    torch.cuda.synchronize()
    got, got_g = small.l1.cpu().numpy(), small.resampled.cpu().numpy()
    assert np.array_equal(got_g.view(np.uint32), np.ascontiguousarray(want_g).view(np.uint32)), "the resampled guide is the restatement's, bit for bit"
    bound = R.loss_bound(image, want)
    print(id, "out", got, "ref", want, "|out - ref|", np.abs(got - want), "bound", bound)
    assert np.all(np.abs(got - want) <= bound)
    assert B.distinct(got) and B.distinct(got_g), "two patterns score alike: a frame read from the wrong place could pass"
    sizes = dict((x[0], x[2]) for x in case.buffers())
    X, G_ = B.tile(image, case.n, DEV), B.tile(guide, case.n, DEV)
    out = B.poisoned((case.n,), torch.float64, DEV)
    res = B.poisoned((case.n, 3, h, w), torch.float32, DEV)
    ws = B.poisoned((sizes["workspace"],), torch.uint8, DEV)
    try:
        assert sum(t.numel() * t.element_size() for t in (X, G_, out, res, ws)) == case.total_bytes()
        assert X.data_ptr() % 16 == 0 and res.data_ptr() % 16 == 0, "the vector kernel needs 16-byte aligned float buffers"
        rt.call(case.call, torch.device(DEV), X.data_ptr(), G_.data_ptr(), case.n, h, w, B.GUIDE_GH, B.GUIDE_GW, out.data_ptr(), res.data_ptr(), ws.data_ptr(),
                ws.numel())
        torch.cuda.synchronize()
        B.assert_frames(id + ": out", out, small.l1)
        B.assert_frames(id + ": resampled", res, small.resampled)
        B.assert_frames(id + ": the renders changed", X, image)
        B.assert_frames(id + ": the guides changed", G_, guide)
    finally:
        del X, G_, out, res, ws, small
        rt.free_workspaces()
        B.release()


def test_guide_l1_grad(rt):
    """The scalar kernel (w % 4 != 0) under seven weights, one of them zero: renders, guides and gradients pass 2^32 bytes."""
    id = "guide_l1_grad_f32"
    case = B.BY_ID[id]
    (image, guide, weights), (want,) = case.make()
    h, w = B.GUIDE_GRAD_HW
    B.reserve(case, DEV)
    # the P frames alone, by test_gpu_guide_loss.py's rule: the restatement bit for bit
    small = rt.guide_l1_grad(B.upload(image, DEV), B.upload(guide, DEV), B.upload(weights, DEV))
    torch.cuda.synchronize()
    got = small.cpu().numpy()
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), "the gradient is the restatement's, bit for bit"
    zero = B.GUIDE_WEIGHTS.index(0.0)
    assert not got[zero].view(np.uint32).any() and B.distinct(got), "a zero weight gives +0; the other patterns differ"
    B.run_equal(rt, case, DEV, [((3, h, w), torch.float32)],
                lambda X, G_, W_, grad: (X.data_ptr(), G_.data_ptr(), case.n, h, w, B.GUIDE_GH, B.GUIDE_GW, W_.data_ptr(), grad.data_ptr()))
    del small


# ---- CORAL ----------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("id", ["coral/u8", "coral/f32"])
def test_coral(rt, id):
    case = B.BY_ID[id]
    (style, content), (want, wantA, wantb) = case.make()
    u8 = int(style.dtype == np.uint8)
    hs, ws_ = style.shape[1:3] if u8 else style.shape[2:]
    hc, wc = content.shape[1:3] if u8 else content.shape[2:]
    B.reserve(case, DEV)
    # the P pairs alone, held to test_gpu_coral.py's bars: the record under 1e-9 and 16 x 2.7e-15, every pixel within 1 ulp
    small, rec = rt.coral(B.upload(style, DEV), B.upload(content, DEV))
    torch.cuda.synchronize()
    recs, pix = rt.coral_record(rec), small.cpu().numpy()
    for k in range(B.P):
        A, b = wantA[k], wantb[k]
        scale = max(np.abs(A).max(), np.abs(b).max())
        err = max(np.abs(np.array(recs[k]["A"]) - A).max(), np.abs(np.array(recs[k]["b"]) - b).max()) / scale
        assert recs[k]["status"] == 0 and err < 1e-9 and err <= 16 * 2.7e-15, (k, err)
        want32 = want[k].astype(np.float32)
        ulp = np.spacing(np.maximum(np.abs(want32), np.float32(2.0 ** -24 * scale))).astype(np.float64)
        assert (np.abs(pix[k].astype(np.float64) - want32.astype(np.float64)) / ulp).max() <= 1.0, k
    sizes = dict((x[0], x[2]) for x in case.buffers())
    S, C = B.tile(style, case.n, DEV), B.tile(content, case.n, DEV)
    out = B.poisoned((case.n, 3, hs, ws_), torch.float32, DEV)
    ws = B.poisoned((sizes["workspace"],), torch.uint8, DEV)
    try:
        assert sum(t.numel() * t.element_size() for t in (S, C, out, ws)) == case.total_bytes()
        rt.call(case.call, torch.device(DEV), S.data_ptr(), u8, case.n, hs, ws_, C.data_ptr(), u8, case.n, hc, wc, out.data_ptr(), ws.data_ptr(), ws.numel())
        torch.cuda.synchronize()
        B.assert_frames(id + ": out", out, small)
        written = rt.CORAL_RECORD_BYTES - 4          # all of adain_coral_record but its last, reserved int
        B.assert_frames(id + ": records", ws[:case.n * rt.CORAL_RECORD_BYTES].view(case.n, rt.CORAL_RECORD_BYTES)[:, :written], rec[:, :written].contiguous())
        B.assert_frames(id + ": style changed", S, style)
        B.assert_frames(id + ": content changed", C, content)
    finally:
        del S, C, out, ws, small, rec
        rt.free_workspaces()
        B.release()


# ---- statistics and blends --------------------------------------------------------------------------------------------------------------------------------
def test_mean_std(rt):
    case = B.BY_ID["mean_std"]
    (x,), (mean64, std64) = case.make()
    c, hw = B.STATS_C, B.STATS_HW
    B.reserve(case, DEV)
    m, s = rt.mean_std(B.upload(x, DEV), False, 1e-5)
    torch.cuda.synchronize()
    em = np.abs(m.cpu().numpy() - mean64) / np.spacing(np.abs(mean64.astype(np.float32)))
    es = np.abs(s.cpu().numpy() - std64) / np.spacing(std64.astype(np.float32))
    assert float((np.abs(mean64) / std64).max()) <= 1e3 and (em <= 1.0).all() and (es <= 2.0).all(), (em.max(), es.max())
    assert B.distinct(m.cpu().numpy())
    X = B.tile(x, case.n, DEV)
    mean, std = B.poisoned((case.n, c), torch.float32, DEV), B.poisoned((case.n, c), torch.float32, DEV)
    nbytes = rt.lib().adain_mean_std_workspace_bytes(0, case.n, c, hw)
    ws = B.poisoned((max(nbytes, 256),), torch.uint8, DEV)
    try:
        assert X.numel() * 4 + 2 * mean.numel() * 4 == case.total_bytes() and nbytes < (1 << 20)
        rt.call(case.call, torch.device(DEV), X.data_ptr(), 0, case.n, c, hw, 1e-5, mean.data_ptr(), std.data_ptr(), ws.data_ptr(), ws.numel())
        torch.cuda.synchronize()
        B.assert_frames("mean", mean, m)
        B.assert_frames("std", std, s)
        B.assert_frames("mean_std: the features changed", X, x)
    finally:
        del X, mean, std, ws
        rt.free_workspaces()
        B.release()


def test_mean_std_nhwc(rt):
    """The NHWC form: mean_std_nhwc_partial's partial sums in the workspace, then mean_std_finalize."""
    case = B.BY_ID["mean_std/nhwc"]
    (x,), (mean64, std64) = case.make()
    c, hw = B.NHWC_C, B.NHWC_HW
    sizes = dict((b[0], b[2]) for b in case.buffers())
    B.reserve(case, DEV)
    m, s = rt.mean_std(B.upload(x, DEV), True, 1e-5)
    torch.cuda.synchronize()
    em = np.abs(m.cpu().numpy() - mean64) / np.spacing(np.abs(mean64.astype(np.float32)))
    es = np.abs(s.cpu().numpy() - std64) / np.spacing(std64.astype(np.float32))
    assert float((np.abs(mean64) / std64).max()) <= 1e3 and (em <= 1.0).all() and (es <= 2.0).all(), (em.max(), es.max())
    assert B.distinct(m.cpu().numpy())
    X = B.tile(x, case.n, DEV)
    mean, std = B.poisoned((case.n, c), torch.float32, DEV), B.poisoned((case.n, c), torch.float32, DEV)
    ws = B.poisoned((sizes["workspace"],), torch.uint8, DEV)
    try:
        assert sum(t.numel() * t.element_size() for t in (X, mean, std, ws)) == case.total_bytes()
        rt.call(case.call, torch.device(DEV), X.data_ptr(), 1, case.n, c, hw, 1e-5, mean.data_ptr(), std.data_ptr(), ws.data_ptr(), ws.numel())
        torch.cuda.synchronize()
        B.assert_frames("mean", mean, m)
        B.assert_frames("std", std, s)
        B.assert_frames("mean_std/nhwc: the features changed", X, x)
    finally:
        del X, mean, std, ws
        rt.free_workspaces()
        B.release()


@pytest.mark.parametrize("id", ["blend_alpha", "blend_pmap", "blend_pmap/c1", "blend_alpha/nhwc"])
def test_blend(rt, id):
    case = B.BY_ID[id]
    x = case.make()[0][0]
    nhwc = int(id.endswith("nhwc"))
    n, c, hw = case.n, x.shape[3] if nhwc else x.shape[1], x.shape[2] if nhwc else x.shape[3]
    assert (n * c * hw) % 4 == 0 and n * c * hw < 2 ** 31 - 1
    if id.startswith("blend_alpha"):
        args = lambda x, cm, cs, sm, ss, out: (x.data_ptr(), nhwc, n, c, hw, cm.data_ptr(), cs.data_ptr(), sm.data_ptr(), ss.data_ptr(), n, 0.7, float(1 - 0.7), out.data_ptr())
    else:
        args = lambda x, cm, cs, sm, ss, p, out: (x.data_ptr(), nhwc, n, c, hw, cm.data_ptr(), cs.data_ptr(), sm.data_ptr(), ss.data_ptr(), n, p.data_ptr(), n, out.data_ptr())
    B.run_equal(rt, case, DEV, [(x.shape[1:], torch.float32)], args)


@pytest.mark.parametrize("id", ["blend_mix/maps", "blend_mix/nhwc_maps"])
def test_blend_mix(rt, id):
    """MIX_K styles for the whole batch, a weight map per frame and style: weights [n][k][hw] is the blend's one buffer larger than x."""
    case = B.BY_ID[id]
    x = case.make()[0][0]
    nhwc = int(id.endswith("nhwc_maps"))
    n, k, c, hw = case.n, B.MIX_K, x.shape[3] if nhwc else x.shape[1], x.shape[2] if nhwc else x.shape[3]
    assert n * c * hw < 2 ** 31 - 1 and n * k * hw * 4 > B.TWO32
    if nhwc:
        args = lambda x, cm, cs, w, p, sm, ss, out: (x.data_ptr(), 1, n, c, hw, cm.data_ptr(), cs.data_ptr(), sm.data_ptr(), ss.data_ptr(), k, w.data_ptr(), n, hw,
                                                     0.0, 0.0, p.data_ptr(), n, out.data_ptr())
    else:
        args = lambda x, cm, cs, w, sm, ss, out: (x.data_ptr(), 0, n, c, hw, cm.data_ptr(), cs.data_ptr(), sm.data_ptr(), ss.data_ptr(), k, w.data_ptr(), n, hw,
                                                  0.6, float(1 - 0.6), None, 1, out.data_ptr())
    B.run_equal(rt, case, DEV, [(x.shape[1:], torch.float32)], args, shared=2)


# ---- transposes -------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("id", ["nchw_to_nhwc", "nhwc_to_nchw"])
def test_transposes(rt, id):
    case = B.BY_ID[id]
    (x,), (want,) = case.make()
    c, hw = (x.shape[1], x.shape[2]) if id == "nchw_to_nhwc" else (x.shape[2], x.shape[1])
    B.run_equal(rt, case, DEV, [(want.shape[1:], torch.float32)], lambda xd, out: (xd.data_ptr(), out.data_ptr(), case.n, c, hw))


# ---- single conv layers -----------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("id", ["conv3x3_wino", "conv3x3_up2x_poly"])
def test_conv_layer(rt, id):
    case = B.BY_ID[id]
    (x, w, b), (want,) = case.make()
    h, ww, cin = x.shape[1:]
    cout = want.shape[3]
    if id == "conv3x3_wino":
        packed = rt.conv3x3_wino_pack(B.upload(w[0], DEV))
        args = lambda X, _w, bias, out: (X.data_ptr(), out.data_ptr(), packed.data_ptr(), bias.data_ptr(), case.n, h, ww, h, ww, cin, cout, rt.SRC_DIRECT, 1, 0, 5)
    else:
        packed = rt.conv3x3_up2x_poly_pack(B.upload(w[0], DEV))
        args = lambda X, _w, bias, out: (X.data_ptr(), out.data_ptr(), packed.data_ptr(), bias.data_ptr(), case.n, h, ww, cin, cout, 1)
    B.run_equal(rt, case, DEV, [(want.shape[1:], torch.float32)], args, shared=2)


# ---- the encoder's first layer ------------------------------------------------------------------------------------------------------------------------------
def test_first_layer(rt, weights):
    """adain_encode_relu1_1 (conv_first_kernel, float entry) under tests/edge_exact.py's integer weights: 65535 frames of 2 x 2 tiles,
    4.64 GiB of relu1_1, every element the float64 evaluation's as in test_gpu_edge_layers.py."""
    import edge_exact as E

    case = B.BY_ID["encode_relu1_1"]
    packed = rt.pack_encoder(E.first_state_dict(weights[0]), torch.device(DEV))
    B.run_equal(rt, case, DEV, [((B.FIRST_H, B.FIRST_W, 64), torch.float32)],
                lambda X, out: (X.data_ptr(), 0, out.data_ptr(), packed.data_ptr(), case.n, B.FIRST_H, B.FIRST_W))
