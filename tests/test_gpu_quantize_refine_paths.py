"""The callers of the refined palette: pixelize.extract_palette(..., refine=) on a tensor against its host form, gif_file.write_gif's
":rT" strings (Pillow must decode the file to the pixels the restatement's palette and nearest map give), AdaINEngine.quantize_palette_u8,
and the call with T = 2 captured alone into a hipGraph on one stream - a chain of 3 + 2 T kernels behind a memset, no parallel branch -
and replayed over stale bytes: the direct call's bits."""
import numpy as np
import pytest
import torch
from PIL import Image

import abi_arena as A
import quantize_cases as C
import quantize_ref as Q
import quantize_refine_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
FRAMES = C.gradient(4, 24, 40, 31)
FRAMES.setflags(write=False)


@pytest.fixture(scope="module")
def rt():
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    import applied_image_processing_amd.runtime as rt

    rt.lib()
    torch.cuda.set_device(0)
    return rt


def decoded(path):
    im = Image.open(path)
    out = []
    for i in range(im.n_frames):
        im.seek(i)
        out.append(np.asarray(im.convert("RGB")))
    return np.stack(out)


def test_extract_palette_on_a_tensor_equals_the_host_form(rt):
    from applied_image_processing_amd import pixelize

    x = torch.from_numpy(FRAMES.copy()).to(DEV)
    for K, T in ((3, 1), (64, 4), (256, 8)):
        assert np.array_equal(pixelize.extract_palette(x, K, refine=T), pixelize.extract_palette(FRAMES, K, device="cpu", refine=T))
        for got, want in zip(pixelize.extract_palette(x, K, per_frame=True, refine=T), pixelize.extract_palette(FRAMES, K, per_frame=True, device="cpu", refine=T)):
            assert np.array_equal(got, want)
    pal, used = R.palette(FRAMES[0], 9, 2)
    assert np.array_equal(pixelize.extract_palette(x[0], 9, refine=2), pal[:used])


@pytest.mark.parametrize("source", ["tensor", "array"])
@pytest.mark.parametrize("palette", ["adaptive-local:16:r2", "adaptive:16:r2"])
def test_write_gif_decodes_to_the_restatements_pixels(rt, tmp_path, palette, source):
    from applied_image_processing_amd import gif_file

    local = palette.startswith("adaptive-local")
    frames = torch.from_numpy(FRAMES.copy()).to(DEV) if source == "tensor" else FRAMES.copy()
    path = str(tmp_path / "clip.gif")
    assert gif_file.write_gif(frames, path, palette, fps=10, method=None, sub_batch=3) == path
    pals, used = R.palettes(FRAMES, 16, local, 2)
    tables = [pals[i][:used[i]] for i in range(len(pals))]
    want = np.stack([tables[i if local else 0][Q.nearest(f, tables[i if local else 0])] for i, f in enumerate(FRAMES)])
    assert np.array_equal(decoded(path), want)


def test_engine_method(rt):
    from applied_image_processing_amd.engine import AdaINEngine

    x = torch.from_numpy(FRAMES.copy()).to(DEV)
    pals, used = AdaINEngine.quantize_palette_u8(None, x, 16, True, refine=3)
    want = R.palettes(FRAMES, 16, True, 3)
    assert used.cpu().tolist() == want[1].tolist() and np.array_equal(pals.cpu().numpy(), want[0])
    plain = AdaINEngine.quantize_palette_u8(None, x, 16, True)
    again = rt.quantize_palette_u8(x, 16, True)
    assert torch.equal(plain[0], again[0]) and torch.equal(plain[1], again[1])


@pytest.mark.parametrize("per_frame", [False, True], ids=["global", "per-frame"])
def test_the_call_captured_alone_replays_the_direct_calls_bits(rt, per_frame):
    sets = {"A": C.gradient(3, 37, 53, 41), "B": C.noise(3, 37, 53, 42)}
    n, h, w = 3, 37, 53
    P = n if per_frame else 1
    K, T = 16, 2
    mode = (1 if per_frame else 0) | T << 8
    nbytes = rt.quantize_palette_sizes(n, h, w, per_frame, T)
    specs = [("src", n * h * w * 3, "in", 1), ("palettes", P * 768, "out", 1), ("used", 4 * P, "out", 4), ("workspace", nbytes, "ws", 8)]
    last_error = lambda: rt.lib().adain_last_error().decode()

    def call(arena):
        return rt.lib().adain_quantize_palette_u8(arena.ptr("src"), n, h, w, K, mode, arena.ptr("palettes"), arena.ptr("used"), arena.ptr("workspace"), nbytes, rt._stream())

    setups = {name: (lambda arena, f=frames: arena.put("src", torch.from_numpy(f))) for name, frames in sets.items()}
    eager = A.run_captured(specs, call, DEV, torch.cuda.synchronize, setups, A.hip_graph(last_error), differs=("palettes",), last_error=last_error)
    assert not torch.cuda.is_current_stream_capturing()
    for got, frames in zip(eager, sets.values()):
        pals, used = R.palettes(frames, K, per_frame, T)
        assert got["used"].view(torch.int32).tolist() == used.tolist()
        assert np.array_equal(got["palettes"].cpu().numpy().reshape(-1, 256, 3), pals)
