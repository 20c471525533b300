"""The callers of the device GIF reader: ``video.gif_to_frames`` writes frame files that decode to the clip, with the PNG route on and
off; ``AdaINEngine.gif_decode_u8``; ``video.stylize_gif`` runs decode -> stylise -> warp / blend -> palette -> encode and its output GIF
reads back with the clip's frame count at the target size.  Run with ``-m gpu``."""
import io

import numpy as np
import pytest
import torch
from PIL import Image

import applied_image_processing_amd.synth as synth
import gif_decode_cases as C
import gif_decode_gpu as G

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SLSO8 = ["#0d2b45", "#203c56", "#544e68", "#8d697a", "#d08159", "#ffaa5e", "#ffd4a3", "#ffecd6"]


@pytest.fixture(scope="module")
def rt():
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    import applied_image_processing_amd.runtime as rt

    rt.lib(), rt.gif_decode_lib()
    torch.cuda.set_device(0)
    return rt


@pytest.fixture(scope="module")
def engine(rt, weights):
    from applied_image_processing_amd.engine import AdaINEngine

    return AdaINEngine(weights[0], weights[1], DEV)


@pytest.mark.parametrize("png_on_device", [False, True])
def test_gif_to_frames_writes_files_that_decode_to_the_clip(rt, tmp_path, monkeypatch, png_on_device):
    from applied_image_processing_amd import video

    name = "pillow_disposal_1"
    path = tmp_path / "clip.gif"
    path.write_bytes(G.data_of(name))
    calls = []
    door = rt.gif_decode_clip
    monkeypatch.setattr(rt, "gif_decode_clip", lambda *a: calls.append(1) or door(*a))
    info = video.gif_to_frames(str(path), str(tmp_path / "frames"), routes=rt.OutputRoutes(png=rt.PngRoute(png_on_device)))
    want = G.expected(name)[1]
    assert calls == [1] and info.durations == [30, 40, 50, 60, 70, 80] and info.loop == 2 and info.size == (50, 40)
    files = sorted(p.name for p in (tmp_path / "frames").iterdir())
    assert files == [f"frame_{i:04d}.png" for i in range(6)]
    got = np.stack([np.asarray(Image.open(tmp_path / "frames" / f).convert("RGB")) for f in files])
    assert np.array_equal(got, want)


def test_the_engine_method(rt, engine):
    report = []
    frames, info = engine.gif_decode_u8(C.CASES["interlaced_later_frame"], report=report)
    assert frames.device == engine.device and report[0]["path"] == "device"
    assert np.array_equal(frames.cpu().numpy(), G.expected("interlaced_later_frame")[1]) and info.size == (7, 9)


def test_stylize_gif_finishes_and_its_output_reads_back(rt, engine, tmp_path):
    from applied_image_processing_amd import gif_file, video
    from applied_image_processing_amd.AdaIN import test as t

    u8 = lambda seed, h, w: (synth.image(seed, 1, h, w)[0].transpose(1, 2, 0) * 255).astype(np.uint8)
    clip = torch.from_numpy(np.stack([u8(800 + i, 32, 32) for i in range(3)])).to(DEV)
    gif_file.write_gif(clip, str(tmp_path / "in.gif"), "web", fps=10)
    Image.fromarray(u8(850, 48, 48)).save(tmp_path / "style.png")
    t.set_depth_provider(lambda img: torch.from_numpy(np.ascontiguousarray(synth.smooth_depth(480, img.size[1], img.size[0]))))
    video.set_flow_provider(video.device_flow_provider)
    try:
        out = video.stylize_gif(str(tmp_path / "in.gif"), str(tmp_path / "style.png"), str(tmp_path / "out.gif"), alpha=0.7, target_resolution=(40, 24), engine=engine,
                                gif_palette=SLSO8, gif_method="kd-tree")
    finally:
        t.set_depth_provider(None)
        video.set_flow_provider(None)
    frames, info = gif_file.read_gif(out, DEV)
    assert tuple(frames.shape) == (3, 24, 40, 3) and info.durations == [100] * 3
    colours = {tuple(c) for c in frames.cpu().numpy().reshape(-1, 3).tolist()}
    assert colours <= {tuple(int(c[i:i + 2], 16) for i in (1, 3, 5)) for c in SLSO8}
