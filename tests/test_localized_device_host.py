"""CPU-only tests of the device colour transfer's host side: the case_h fixtures (the reference's own outputs) against this
repository's host path, the three new C-ABI entry points (declared, bound, exported), and the refusals of the Python wrappers that
must not need a GPU.  The kernels themselves are tested in test_gpu_localized.py."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

from conftest import ROOT, golden

import applied_image_processing_amd.runtime as rt
from applied_image_processing_amd import localized as L
from golden.make_golden_localized import CASES, case_inputs, regions, within_bar

NEW_SYMBOLS = ("adain_colour_transfer_workspace_bytes", "adain_colour_transfer_u8", "adain_localized_combine_u8")


@pytest.mark.parametrize("name", list(CASES))
def test_case_h_host_path_reproduces_the_reference(name):
    """Guards the fixtures and the choice of inputs: the existing host functions stay inside the project's bar for this truncating
    cast (no channel off by more than one level, share of differing channel values below 1e-3) on every case, both ways round and
    through the composite, and the cases hit the branches they were chosen for."""
    g = golden("case_h.npz")
    content, stylised, m = case_inputs(name)
    fg, bg = regions(name)
    nt, ns = (int(v) for v in g[f"{name}/n"])
    assert (nt, ns) == (int((fg.sum(-1) > 0).sum()), int((bg.sum(-1) > 0).sum()))
    assert within_bar(L.color_transfer_foreground(fg, bg), g[f"{name}/adjusted"])
    assert within_bar(L.color_transfer_foreground(bg, fg), g[f"{name}/adjusted_swapped"])
    assert within_bar(L.combine_localized(content, stylised, m), g[f"{name}/combined"])
    if name.startswith("halves"):
        assert nt == ns                                             # the no-resample branch
    elif name.startswith("two_pixels"):
        assert nt == 2 and int(((1 - m).sum())) > 2                # black pixels inside the foreground's area
    else:
        assert nt < ns                                              # swapped: the other resample branch
    if name.startswith("ties"):
        assert len(np.unique(fg[fg.sum(-1) > 0], axis=0)) < nt - 100    # colours repeat


def test_new_entry_points_are_declared_bound_and_exported():
    header = open(os.path.join(ROOT, "include", "adain_hip.h")).read()
    code = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    if not os.path.exists(rt.LIB_PATH):
        import __graft_entry__ as g

        g.build()
    lib = rt.lib()
    for name in NEW_SYMBOLS:
        assert re.search(r"\b%s\s*\(" % name, code), f"{name} is not declared in adain_hip.h"
        assert name in rt.SIGNATURES and hasattr(lib, name)
    assert lib.adain_abi_version() == 4                              # additions only
    # the documented record: two regions of (int64 n, mean[3], component[3], explained_variance) and two 32-bit words
    assert "typedef struct adain_colour_record" in code and rt.COLOUR_RECORD_BYTES == 2 * 64 + 8
    assert lib.adain_colour_transfer_workspace_bytes(0, 5) == 0 and lib.adain_colour_transfer_workspace_bytes(5, -1) == 0
    assert lib.adain_colour_transfer_u8(None, None, None, 4, 4, None, None) == -1 and b"null pointer" in lib.adain_last_error()
    assert lib.adain_localized_combine_u8(None, None, None, None, 4, 4, None, None) == -1


def test_the_kernel_file_carries_the_reference_matrices():
    """csrc/colour.hip holds the four 3 x 3 matrices as literals; they are the ones localized.py computes (numpy.linalg.inv for two)."""
    src = open(os.path.join(ROOT, "applied-image-processing_amd", "csrc", "colour.hip")).read()
    for name in ("RGB_TO_LMS", "LMS_TO_LAB", "LAB_TO_LMS", "LMS_TO_RGB"):
        body = re.search(r"__constant__ double %s\[3\]\[3\] = \{(.*?)\};" % name, src, flags=re.S).group(1)
        vals = np.array([float(v) for v in re.findall(r"-?\d[\d.]*(?:e-?\d+)?", body)]).reshape(3, 3)
        np.testing.assert_allclose(vals, getattr(L, name), rtol=1e-15, atol=1e-30)


def test_wrappers_refuse_bad_inputs_without_a_gpu(capsys):
    img = np.full((6, 8, 3), 9, np.uint8)
    mask = np.zeros((6, 8), np.uint8)
    with pytest.raises(ValueError, match="background_img must be a uint8 \\[6,8,3\\]"):
        L.color_transfer_foreground_device(img, img[:5])
    with pytest.raises(ValueError, match="foreground_img must be a uint8"):
        L.color_transfer_foreground_device(img.astype(np.float32), img)
    with pytest.raises(ValueError, match="foreground_img must be a uint8"):
        L.color_transfer_foreground_device(img[..., 0], img)
    with pytest.raises(ValueError, match="0 and 1"):
        L.combine_localized_device(img, img, mask + 2)
    with pytest.raises(ValueError, match="0 and 1"):
        L.combine_localized_device(img, img, mask.astype(np.float32))
    with pytest.raises(ValueError, match="content_np must be a uint8 \\[6,8,3\\]"):
        L.combine_localized_device(img[:, :7], img, mask)
    with pytest.raises(ValueError, match="stylized_np must be a uint8"):
        L.combine_localized_device(img, torch.zeros(6, 8, 3), mask)
    # the runtime layer takes device buffers only: a CPU tensor is refused, not uploaded
    t = torch.from_numpy(img)
    with pytest.raises(rt.AdainHipError, match="expected a GPU tensor"):
        rt.colour_transfer_u8(t, t)
    with pytest.raises(rt.AdainHipError, match="expected a GPU tensor"):
        rt.localized_combine_u8(t, t, torch.from_numpy(mask))
    if not torch.cuda.is_available():
        with pytest.raises(rt.AdainHipError, match="needs a GPU"):       # no quiet fall-back to the host path
            L.color_transfer_foreground_device(img, img)


def test_default_of_the_pipeline_is_the_host_path():
    import inspect

    p = inspect.signature(L.run_localized_style_transfer).parameters["colour_on_device"]
    assert p.default is False and p.kind is inspect.Parameter.KEYWORD_ONLY
    from applied_image_processing_amd import run_semantic_segm as cli

    assert any(flag == "--colour_on_device" and kw.get("action") == "store_true" for flag, kw in cli._EXTRA_FLAGS)
