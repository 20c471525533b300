"""The callers of the device metrics: applied_image_processing_amd.metrics' ssim / psnr / mse / l1_loss / l2_loss on GPU tensors (the
reference's shapes and dtype, the restatement's values), the torch route of another window size, compare_dirs and evaluate on a directory
of PNG and JPEG pairs with the device decoders on and off, and AdaINEngine.image_metrics."""
import json
import os

import numpy as np
import pytest
import torch
from PIL import Image

import metrics_cases as C
import metrics_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ULP = 2.0 ** -24          # the results are float32: half an ulp of a value below 1 (ssim, mse, l1), and of one below 128 for psnr


@pytest.fixture(scope="module")
def M():
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    import applied_image_processing_amd.metrics as M
    import applied_image_processing_amd.runtime as rt

    rt.lib()
    torch.cuda.set_device(0)
    return M


@pytest.fixture(scope="module")
def bars():
    with open(os.path.join(C.GOLDEN, "noise.json")) as f:
        return json.load(f)


A_U8, B_U8 = C.pair("near", 3, 21, 70, 3, seed=8)
FA, FB = C.to_nchw_f32(A_U8), C.to_nchw_f32(B_U8)
WANT = R.metrics_f32(FA, FB)


def test_the_surface_on_gpu_tensors_is_the_restatement_in_the_references_shapes(M, bars):
    x, y = torch.from_numpy(FA).to(DEV), torch.from_numpy(FB).to(DEV)
    calls = []
    import applied_image_processing_amd.runtime as rt

    real = rt.image_metrics
    try:
        rt.image_metrics = lambda *a, **k: calls.append(1) or real(*a, **k)
        s_all, s_each, s_one = M.ssim(x, y), M.ssim(x, y, size_average=False), M.ssim(x[1], y[1])
        p, m, l1, l2 = M.psnr(x, y), M.mse(x, y), M.l1_loss(x, y), M.l2_loss(x, y)
        assert len(calls) == 7, "a float32 GPU tensor takes the device call"
        s7 = M.ssim(x, y, 7, False)
        grad = M.ssim(x.clone().requires_grad_(), y)
        assert len(calls) == 7, "window 7 and a tensor that wants a gradient take the torch route"
    finally:
        rt.image_metrics = real
    for t, shape in ((s_all, ()), (s_each, (3,)), (s_one, ()), (p, (3, 1)), (m, (3, 1)), (l1, ()), (l2, ()), (s7, (3,))):
        assert t.shape == shape and t.dtype == torch.float32 and t.is_cuda, (t.shape, shape)
    assert grad.requires_grad
    assert np.abs(s_each.cpu().numpy() - WANT["ssim"]).max() <= bars["bar_frame"] + ULP
    assert abs(float(s_all) - WANT["ssim"].mean()) <= bars["bar_frame"] + ULP and abs(float(s_one) - WANT["ssim"][1]) <= bars["bar_frame"] + ULP
    rel = 8 * 2.0 ** -24          # the float-input mse and l1
    assert np.all(np.abs(m.cpu().numpy().reshape(-1) - WANT["mse"]) <= (rel + ULP) * WANT["mse"])
    assert np.abs(p.cpu().numpy().reshape(-1) - WANT["psnr"]).max() <= 10 / np.log(10) * rel + 128 * ULP
    assert abs(float(l1) - WANT["l1"].mean()) <= (rel + ULP) * WANT["l1"].mean() and abs(float(l2) - WANT["mse"].mean()) <= (rel + ULP) * WANT["mse"].mean()
    # window 7: torch's own result on the same tensors
    g = M.gaussian(7, 1.5).unsqueeze(1)
    win = g.mm(g.t())[None, None].expand(3, 1, 7, 7).contiguous().to(DEV)
    assert torch.equal(s7, M._ssim(x, y, win, 7, 3, False))
    # the CPU tensors of the same frames: torch there, the same values to the bar
    assert np.abs(M.ssim(x.cpu(), y.cpu(), size_average=False).numpy() - WANT["ssim"]).max() <= bars["bar_frame"]


def write_pairs(root):
    """renders/ and gt/ under root: three PNG pairs of one size, one PNG pair of another, two JPEG pairs."""
    r, g = os.path.join(root, "renders"), os.path.join(root, "gt")
    os.makedirs(r), os.makedirs(g)
    a, b = C.pair("near", 3, 24, 40, 3, seed=9)
    for i in range(3):
        Image.fromarray(a[i]).save(os.path.join(r, f"v{i}.png")), Image.fromarray(b[i]).save(os.path.join(g, f"v{i}.png"))
    a2, b2 = C.pair("ramp", 1, 17, 33, 3, seed=9)
    Image.fromarray(a2[0]).save(os.path.join(r, "small.png")), Image.fromarray(b2[0]).save(os.path.join(g, "small.png"))
    for i in range(2):
        Image.fromarray(a[i]).save(os.path.join(r, f"j{i}.jpg"), quality=90), Image.fromarray(b[i]).save(os.path.join(g, f"j{i}.jpg"), quality=60)
    return r, g


def test_compare_dirs_scores_the_same_with_the_device_decoders_on_and_off(M, bars, tmp_path):
    import applied_image_processing_amd.runtime as rt

    r, g = write_pairs(str(tmp_path))
    off = M.compare_dirs(r, g, DEV)
    on = M.compare_dirs(r, g, DEV, routes=rt.OutputRoutes(jpeg=dict(decode_on_device=True), png=dict(decode_on_device=True)))
    assert on == off and sorted(off) == ["j0.jpg", "j1.jpg", "small.png", "v0.png", "v1.png", "v2.png"]
    for name, got in off.items():
        a, b = (np.asarray(Image.open(os.path.join(d, name)).convert("RGB"))[None] for d in (r, g))
        want = R.metrics_u8(a, b)
        assert abs(got["SSIM"] - want["ssim"][0]) <= bars["bar_frame"] + ULP and abs(got["PSNR"] - want["psnr"][0]) <= 128 * ULP, name
    # the CPU route of the same directory: torch's float32, within the bar of the same restatement
    cpu = M.compare_dirs(r, g, "cpu")
    assert all(abs(cpu[k]["SSIM"] - off[k]["SSIM"]) <= 2 * bars["bar_frame"] for k in off)


def test_evaluate_on_the_device_writes_the_two_files(M, tmp_path):
    scene = str(tmp_path / "scene")
    os.makedirs(os.path.join(scene, "test"))
    r, g = write_pairs(os.path.join(scene, "test", "ours_1"))
    M.evaluate([scene], device=DEV)
    results, per_view = json.load(open(os.path.join(scene, "results.json"))), json.load(open(os.path.join(scene, "per_view.json")))
    scores = M.compare_dirs(r, g, DEV)
    assert sorted(results["ours_1"]) == ["PSNR", "SSIM"] and per_view["ours_1"]["SSIM"] == {k: v["SSIM"] for k, v in scores.items()}
    assert results["ours_1"]["PSNR"] == torch.tensor([v["PSNR"] for v in scores.values()]).mean().item()


def test_the_engine_forwards(M):
    from applied_image_processing_amd.engine import AdaINEngine
    import applied_image_processing_amd.runtime as rt

    x, y = torch.from_numpy(A_U8).to(DEV), torch.from_numpy(B_U8).to(DEV)
    got, want = AdaINEngine.image_metrics(None, x, y, ssim_map=True), rt.image_metrics(x, y, ssim_map=True)
    assert torch.equal(got.records, want.records) and torch.equal(got.ssim_map, want.ssim_map)
    exact = R.metrics_u8(A_U8, B_U8)
    assert got.mse.cpu().tolist() == exact["mse"].tolist() and got.l1.cpu().tolist() == exact["l1"].tolist()
