"""The callers of the device palette chooser: gif_file.write_gif's "adaptive" and "adaptive-local" clips (Pillow must decode each file to
the pixels the restatement's palette and nearest map give), the local colour table's bytes, pixelize.extract_palette on a tensor,
video.frames_to_gif and AdaINEngine.quantize_palette_u8."""
import numpy as np
import pytest
import torch
from PIL import Image

import quantize_cases as C
import quantize_ref as Q

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
FRAMES = C.gradient(5, 24, 40, 31)
FRAMES.setflags(write=False)


@pytest.fixture(scope="module")
def rt():
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    import applied_image_processing_amd.runtime as rt

    rt.lib()
    torch.cuda.set_device(0)
    return rt


@pytest.fixture(scope="module")
def wanted():
    """{(local, colors): (tables, the frames' pixels)} of the restatement, once."""
    out = {}
    for local in (False, True):
        for colors in (256, 6):
            pals, used = Q.palettes(FRAMES, colors, local)
            tables = [pals[i][:used[i]] for i in range(len(pals))]
            out[local, colors] = tables, np.stack([tables[i if local else 0][Q.nearest(f, tables[i if local else 0])] for i, f in enumerate(FRAMES)])
    return out


def decoded(path):
    im = Image.open(path)
    out = []
    for i in range(im.n_frames):
        im.seek(i)
        out.append(np.asarray(im.convert("RGB")))
    return np.stack(out)


@pytest.mark.parametrize("source", ["tensor", "array"])
@pytest.mark.parametrize("colors", [256, 6])
@pytest.mark.parametrize("palette", ["adaptive", "adaptive-local"])
def test_write_gif_decodes_to_the_restatements_pixels(rt, wanted, tmp_path, palette, colors, source):
    from applied_image_processing_amd import gif_file

    frames = torch.from_numpy(FRAMES.copy()).to(DEV) if source == "tensor" else FRAMES.copy()
    path = str(tmp_path / "clip.gif")
    assert gif_file.write_gif(frames, path, gif_file.adaptive(colors, palette == "adaptive-local"), fps=10, method=None, sub_batch=2) == path
    assert np.array_equal(decoded(path), wanted[palette == "adaptive-local", colors][1])


@pytest.mark.parametrize("colors,g", [(256, 8), (6, 3), (2, 1)])
def test_local_tables_flag_and_size_bytes(rt, tmp_path, colors, g):
    """No global table (flags 0x70); every record's descriptor flags 0x80 | (g - 1), then 3 * 2^g table bytes: the frame's palette, zeros."""
    from applied_image_processing_amd import gif_file

    path = str(tmp_path / "clip.gif")
    gif_file.write_gif(torch.from_numpy(FRAMES.copy()).to(DEV), path, gif_file.adaptive(colors, local=True), fps=10)
    data = open(path, "rb").read()
    assert data[:6] == b"GIF89a" and data[10] == 0x70
    at = 13 + 19          # the NETSCAPE2.0 loop extension is 19 bytes
    m = max(2, g)
    for f in FRAMES:
        assert data[at:at + 4] == b"\x21\xf9\x04\x04" and data[at + 8] == 0x2C
        assert data[at + 17] == 0x80 | (g - 1)
        pal, used = Q.palette(f, colors)
        table = data[at + 18:at + 18 + 3 * (1 << g)]
        assert table == pal[:used].tobytes() + bytes(3 * ((1 << g) - used))
        at += 18 + 3 * (1 << g)
        assert data[at] == m
        at += 1
        while data[at]:
            at += 1 + data[at]
        at += 1
    assert data[at:] == b"\x3b"


def test_global_table_is_the_clips_palette(rt, wanted, tmp_path):
    from applied_image_processing_amd import gif_file

    path = str(tmp_path / "clip.gif")
    gif_file.write_gif(torch.from_numpy(FRAMES.copy()).to(DEV), path, "adaptive:6", fps=10)
    data = open(path, "rb").read()
    table = wanted[False, 6][0][0]
    assert data[10] == 0x80 | 0x70 | 2 and data[13:13 + 24] == table.tobytes() + bytes(24 - table.size)
    assert data[13 + 24 + 19 + 17] == 0          # the records keep their descriptor: no local table


def test_extract_palette_on_a_tensor_equals_the_host_form(rt):
    from applied_image_processing_amd import pixelize

    x = torch.from_numpy(FRAMES.copy()).to(DEV)
    for K in (3, 64, 256):
        assert np.array_equal(pixelize.extract_palette(x, K), pixelize.extract_palette(FRAMES, K, device="cpu"))
        for got, want in zip(pixelize.extract_palette(x, K, per_frame=True), pixelize.extract_palette(FRAMES, K, per_frame=True, device="cpu")):
            assert np.array_equal(got, want)
    assert np.array_equal(pixelize.extract_palette(x[0], 9), pixelize.extract_palette(FRAMES[0], 9, device="cpu"))


@pytest.mark.parametrize("palette", ["adaptive", "adaptive-local"])
def test_frames_to_gif_passes_the_strings_through(rt, wanted, tmp_path, palette):
    from applied_image_processing_amd import video

    folder = tmp_path / "frames"
    folder.mkdir()
    for i, f in enumerate(FRAMES):
        Image.fromarray(f).save(folder / f"{i:03d}.png")
    out = video.frames_to_gif(str(folder), str(tmp_path / "clip.gif"), fps=10, palette=palette + ":6")
    assert np.array_equal(decoded(out), wanted[palette == "adaptive-local", 6][1])
    out = video.frames_to_gif(str(folder), str(tmp_path / "full.gif"), fps=10, palette=palette)
    assert np.array_equal(decoded(out), wanted[palette == "adaptive-local", 256][1])
    assert video._gif_request("x.gif", 10, palette, None) == {"path": "x.gif", "fps": 10, "palette": palette, "method": "kd-tree"}
    with pytest.raises(ValueError):
        video._gif_request("x.gif", 10, palette + ":300", None)


def test_engine_method(rt):
    from applied_image_processing_amd.engine import AdaINEngine

    x = torch.from_numpy(FRAMES.copy()).to(DEV)
    pals, used = AdaINEngine.quantize_palette_u8(None, x, 16, True)
    want = Q.palettes(FRAMES, 16, True)
    assert used.cpu().tolist() == want[1].tolist() and np.array_equal(pals.cpu().numpy(), want[0])
