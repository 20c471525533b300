"""GPU tests of the localized pipeline's colour transfer on the device (csrc/colour.hip): every case_h case against the REFERENCE's
stored outputs, the device record against the reference's fitted PCAs, empty and one-pixel regions, run-to-run identity, a 1080p
frame against this repository's host path, and the pipeline end to end with the switch on and off.  Run with ``-m gpu``.

The bar throughout is the project's own for this truncating cast (tests/test_oracle_golden.py, case E): no channel off by more than
one level, share of differing channel values below 1e-3."""
import numpy as np
import pytest
import torch

import applied_image_processing_amd.synth as synth
from applied_image_processing_amd import localized as L
from conftest import golden
from golden.make_golden_localized import CASES, case_inputs, regions

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def rt():
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    import applied_image_processing_amd.runtime as rt

    rt.lib()
    return rt


def check_bar(got, want, what):
    assert got.dtype == np.uint8 and got.shape == want.shape, what
    d = np.abs(got.astype(int) - want.astype(int))
    print(f"{what}: max difference {d.max()}, differing channel values {(d > 0).sum()} of {d.size} (share {(d > 0).mean():.2e})")
    assert d.max() <= 1 and (d > 0).mean() < 1e-3, what


@pytest.mark.parametrize("name", list(CASES))
def test_case_h_against_the_reference(rt, name):
    g = golden("case_h.npz")
    content, stylised, m = case_inputs(name)
    fg, bg = regions(name)
    got, rec = L.color_transfer_foreground_device(fg, bg, return_record=True)
    check_bar(got, g[f"{name}/adjusted"], f"{name} adjusted")
    outside = fg.sum(-1) == 0
    assert np.array_equal(got[outside], fg[outside])                         # pixels outside the foreground region: untouched
    # the device record against the reference's fitted PCAs: counts exact, mean_ and components_ (sign included) to case E's bar
    assert rec["status"] == 0 and [rec["fg"]["n"], rec["bg"]["n"]] == [int(v) for v in g[f"{name}/n"]]
    for key, want in (("fg", "f"), ("bg", "b")):
        np.testing.assert_allclose(rec[key]["mean"], g[f"{name}/mean_{want}"], rtol=1e-9, atol=1e-12)
        np.testing.assert_allclose(rec[key]["component"], g[f"{name}/comp_{want}"], rtol=1e-9, atol=1e-12)
    swapped = L.color_transfer_foreground_device(bg, fg)
    check_bar(swapped, g[f"{name}/adjusted_swapped"], f"{name} swapped")
    assert np.array_equal(swapped[bg.sum(-1) == 0], bg[bg.sum(-1) == 0])
    combined = L.combine_localized_device(content, stylised, m)
    check_bar(combined, g[f"{name}/combined"], f"{name} combined")
    assert np.array_equal(combined[m == 1], stylised[m == 1])


def test_types_in_are_types_out(rt, weights):
    content, stylised, m = case_inputs("disc_96x128")
    fg, bg = regions("disc_96x128")
    want = L.color_transfer_foreground_device(fg, bg)
    on_dev = L.color_transfer_foreground_device(torch.from_numpy(fg).cuda(), torch.from_numpy(bg).cuda())
    assert isinstance(on_dev, torch.Tensor) and on_dev.is_cuda and on_dev.dtype == torch.uint8 and np.array_equal(on_dev.cpu().numpy(), want)
    on_cpu = L.color_transfer_foreground_device(torch.from_numpy(fg), torch.from_numpy(bg))
    assert isinstance(on_cpu, torch.Tensor) and not on_cpu.is_cuda and np.array_equal(on_cpu.numpy(), want)
    comb = L.combine_localized_device(torch.from_numpy(content).cuda(), torch.from_numpy(stylised).cuda(), torch.from_numpy(m).cuda())
    assert comb.is_cuda and np.array_equal(comb.cpu().numpy(), L.combine_localized_device(content, stylised, m))
    # a stylised image of another size is nearest-resized to the mask on the host, as in the reference (:223-230)
    small = np.ascontiguousarray(stylised[::2, ::2])
    got = L.combine_localized_device(content, small, m)
    check_bar(got, L.combine_localized(content, small, m), "nearest-resized stylised image")
    # the engine-level entry points and a caller's output buffer
    from applied_image_processing_amd.engine import AdaINEngine

    out = torch.empty(96, 128, 3, dtype=torch.uint8, device="cuda")
    f, b = torch.from_numpy(fg).cuda(), torch.from_numpy(bg).cuda()
    engine = AdaINEngine(*weights, "cuda:0")
    res, record = engine.colour_transfer_u8(f, b, out)
    assert res is out and np.array_equal(out.cpu().numpy(), want) and rt.colour_record(record)["status"] == 0
    comb_dev, _ = engine.localized_combine_u8(torch.from_numpy(content).cuda(), torch.from_numpy(stylised).cuda(), torch.from_numpy(m).cuda())
    assert torch.equal(comb_dev, comb)
    with pytest.raises(rt.AdainHipError, match="distinct"):
        rt.colour_transfer_u8(f, b, out=f)
    with pytest.raises(rt.AdainHipError, match="one size"):
        rt.colour_transfer_u8(f, b[:50].contiguous())


def test_empty_and_single_pixel_regions(rt, capsys):
    fg, bg = regions("disc_96x128")
    z = np.zeros_like(fg)
    capsys.readouterr()
    assert np.array_equal(L.color_transfer_foreground_device(z, bg), z)
    assert capsys.readouterr().out == "Warning: No foreground pixels found.\n"
    assert np.array_equal(L.color_transfer_foreground_device(fg, z), fg)
    assert capsys.readouterr().out == "Warning: No background pixels found for color transfer.\n"
    assert np.array_equal(L.color_transfer_foreground_device(z, z), z)
    assert capsys.readouterr().out == "Warning: No foreground pixels found.\n"
    # a mask that is background everywhere: the composite is the stylised image; foreground everywhere: the content
    content, stylised, m = case_inputs("disc_96x128")
    assert np.array_equal(L.combine_localized_device(content, stylised, np.ones_like(m)), stylised)
    assert np.array_equal(L.combine_localized_device(content, stylised, np.zeros_like(m)), content)
    capsys.readouterr()
    # one pixel: the reference divides by zero; here the status word says so, the output is a copy, the wrapper raises
    one = z.copy()
    one[5, 7] = (10, 200, 30)
    with pytest.raises(ValueError, match="foreground region has one pixel"):
        L.color_transfer_foreground_device(one, bg)
    with pytest.raises(ValueError, match="background region has one pixel"):
        L.color_transfer_foreground_device(fg, one)
    out, record = rt.colour_transfer_u8(torch.from_numpy(one).cuda(), torch.from_numpy(bg).cuda())
    rec = rt.colour_record(record)
    assert rec["status"] == rt.COLOUR_FG_SINGLE and rec["fg"]["n"] == 1 and np.array_equal(out.cpu().numpy(), one)
    assert np.isfinite(rec["fg"]["mean"]).all() and rec["fg"]["component"] == [0.0, 0.0, 0.0]


def test_same_bytes_run_to_run_and_on_a_side_stream(rt):
    content, stylised, m = (torch.from_numpy(a).cuda() for a in case_inputs("disc_250x333"))
    first, rec1 = rt.localized_combine_u8(content, stylised, m)
    second, rec2 = rt.localized_combine_u8(content, stylised, m)
    side = torch.cuda.Stream()
    torch.cuda.synchronize()
    with torch.cuda.stream(side):
        x = torch.randn(1024, 1024, device="cuda")
        for _ in range(4):
            x = x @ x * 1e-3                                                # unrelated work in front of the call
        third, rec3 = rt.localized_combine_u8(content, stylised, m)
    side.synchronize()
    torch.cuda.synchronize()
    assert torch.equal(first, second) and torch.equal(first, third)
    assert torch.equal(rec1, rec2) and torch.equal(rec1, rec3)             # the float64 sums too, bit for bit


def test_1080p_against_the_host_path(rt):
    h, w = 1080, 1920
    rng = np.random.default_rng(5)
    content = np.maximum((synth.image(91, 1, h, w)[0].transpose(1, 2, 0) * np.float32(255)).astype(np.uint8), 1)
    stylised = (synth.image(92, 1, h, w)[0].transpose(1, 2, 0) * np.float32([200, 120, 90]) + np.float32([30, 60, 20])).astype(np.uint8)
    blocks = rng.random((h // 8, w // 8))
    for share in (0.35, 0.7):                                              # random 8 x 8 block masks: foreground larger, then smaller
        m = np.kron((blocks < share).astype(np.uint8), np.ones((8, 8), np.uint8))
        got, rec = L.combine_localized_device(content, stylised, m, return_record=True)
        assert rec["fg"]["n"] == int((m == 0).sum()) and rec["bg"]["n"] == int((m == 1).sum())
        check_bar(got, L.combine_localized(content, stylised, m), f"1080p, background share {share}")
    fg, bg = content * (1 - m)[..., None], stylised * m[..., None]
    check_bar(L.color_transfer_foreground_device(fg, bg), L.color_transfer_foreground(fg, bg), "1080p colour transfer")


def test_pipeline_end_to_end_with_the_switch(rt, weights, tmp_path):
    """run_localized_style_transfer in the shape of test_gpu_jobs.test_localized_pipeline_end_to_end: with colour_on_device the saved
    JPEG decodes to within that test's bar of combine_localized of the re-opened stylised file; with it off the file's bytes are the
    host path's, as before."""
    from PIL import Image

    torch.save(synth.to_torch(synth.vgg_state_dict(0, full=True)), tmp_path / "vgg.pth")
    torch.save(weights[1], tmp_path / "dec.pth")
    u8 = lambda seed, hh, ww: (synth.image(seed, 1, hh, ww)[0].transpose(1, 2, 0) * 255).astype(np.uint8)
    Image.fromarray(u8(430, 64, 96)).save(tmp_path / "c.png")
    Image.fromarray(u8(431, 64, 64)).save(tmp_path / "s.png")
    yy, xx = np.mgrid[:64, :96]
    bgmask = (((yy - 30) ** 2 + (xx - 50) ** 2) > 300).astype(np.uint8)[None]
    kw = dict(file_name="loc", vgg_str=str(tmp_path / "vgg.pth"), decoder_str=str(tmp_path / "dec.pth"), content_size=0, save_ext=".png",
              background_mask=bgmask)
    content = np.asarray(Image.open(tmp_path / "c.png"))
    paths = {}
    for on in (True, False):
        out = tmp_path / ("dev" if on else "host")
        paths[on] = L.run_localized_style_transfer(str(tmp_path / "c.png"), str(tmp_path / "s.png"), output_path=str(out), colour_on_device=on, **kw)
        assert paths[on] == f"{out}/localized_style_transfer_result.jpg"
    sty = np.asarray(Image.open(tmp_path / "dev" / "loc.png"))
    want = L.combine_localized(content, sty, bgmask[0])
    got = np.asarray(Image.open(paths[True]))
    assert got.shape == want.shape and float(np.abs(got.astype(float) - want.astype(float)).mean()) < 8.0
    sty_host = np.asarray(Image.open(tmp_path / "host" / "loc.png"))
    Image.fromarray(L.combine_localized(content, sty_host, bgmask[0])).save(tmp_path / "want.jpg")
    assert open(paths[False], "rb").read() == (tmp_path / "want.jpg").read_bytes()
    # the CLI passes the switch through
    from applied_image_processing_amd import run_semantic_segm as cli

    np.save(tmp_path / "mask.npy", bgmask)
    p = cli.main(["--content", str(tmp_path / "c.png"), "--style", str(tmp_path / "s.png"), "--output", str(tmp_path / "cli"), "--file_name", "loc",
                  "--mask_npy", str(tmp_path / "mask.npy"), "--vgg", str(tmp_path / "vgg.pth"), "--decoder", str(tmp_path / "dec.pth"),
                  "--colour_on_device"])
    q = L.run_localized_style_transfer(str(tmp_path / "c.png"), str(tmp_path / "s.png"), output_path=str(tmp_path / "fn"), colour_on_device=True,
                                       file_name="loc", vgg_str=str(tmp_path / "vgg.pth"), decoder_str=str(tmp_path / "dec.pth"), background_mask=bgmask)
    assert open(p, "rb").read() == open(q, "rb").read()
