"""GPU test of the binding's call path (runtime.call / runtime.scratch): with one device current on the calling thread and every
tensor on ANOTHER, each wrapper makes its size query and its launch with the tensors' device current - the encoder's, the decoder's,
adain_stylize_u8's and the split layer's workspace queries count the current device's compute units (include/adain_hip.h), so a
query made elsewhere sizes the cin-split slabs for the wrong chip and opens a HIP context on a GPU the caller never meant to touch.
A recording stand-in for the loaded library notes the current device of every call; the results are the bytes the same calls give
with the tensors' device made current by the caller.  Needs two GPUs.  Run with ``-m gpu``."""
import fnmatch

import numpy as np
import pytest
import torch

import applied_image_processing_amd.synth as synth

pytestmark = pytest.mark.gpu

# what include/adain_hip.h words as independent of the device: state of the thread, sizes that follow from the shapes alone
DEVICE_FREE = ["adain_abi_version", "adain_last_error", "adain_set_schedule", "adain_get_schedule", "adain_*_packed_floats",
               "adain_encoded_size", "adain_stylize_u8_out_size", "adain_farneback_levels", "adain_farneback_pyramid_bytes",
               "adain_farneback_workspace_bytes", "adain_tvl1_scales", "adain_tvl1_frame_bytes", "adain_tvl1_workspace_bytes"]


class Recorder:
    """Stands in for the loaded CDLL: every function notes (name, current device) and then runs."""

    def __init__(self, lib):
        self.lib, self.calls = lib, []

    def __getattr__(self, name):
        fn = getattr(self.lib, name)

        def recorded(*args):
            self.calls.append((name, torch.cuda.current_device()))
            return fn(*args)

        return recorded


def _u8(seed, *shape):
    n = int(np.prod(shape))
    return torch.from_numpy((synth.image(seed, 1, 1, n, c=1).reshape(shape) * 255).astype(np.uint8))


def _f32(seed, *shape):
    return torch.from_numpy(synth.image(seed, 1, 1, int(np.prod(shape)), c=1).reshape(shape) - 0.5)


def _every_call(rt, fl, weights, dev):
    """Each wrapper once, on tensors of ``dev``: {step: tensor}."""
    vgg_sd, dec_sd = weights
    out = {}
    enc, dec = rt.pack_encoder(vgg_sd, dev), rt.pack_decoder(dec_sd, dev)
    out["pack_encoder"], out["pack_decoder"] = enc, dec
    img = torch.from_numpy(synth.image(1, 2, 16, 24)).to(dev)
    u8 = _u8(2, 2, 16, 24, 3).to(dev)
    feat = out["encode"] = rt.encode(img, enc)
    assert tuple(feat.shape) == (2, 2, 3, 512)
    out["encode_u8"] = rt.encode_u8(u8, enc)
    out["encode_multi0"], out["encode_multi1"] = rt.encode_multi([img[:1], torch.from_numpy(synth.image(3, 1, 24, 16)).to(dev)], enc)
    image = out["decode"] = rt.decode(feat, dec)
    c_mean, c_std = out["mean"], out["std"] = rt.mean_std(feat, True)
    s_mean, s_std = rt.mean_std(out["encode_u8"][:1], True)
    out["blend_alpha"] = rt.blend_alpha(feat, True, c_mean, c_std, s_mean, s_std, 0.7)
    pmap = out["strength_map"] = rt.strength_map(_f32(4, 7, 5).to(dev), 2, 3, 0.15, 20)
    out["blend_pmap"] = rt.blend_pmap(feat, True, c_mean, c_std, s_mean, s_std, pmap)
    mask_u8 = (_u8(5, 1, 1, 16, 24) > 127).to(torch.uint8).to(dev)
    out["stylize_u8"] = rt.stylize_u8(u8, enc, dec, s_mean, s_std)
    out["stylize_u8_mask"] = rt.stylize_u8(u8, enc, dec, s_mean, s_std, mask=mask_u8)
    # cin 128 is the smallest for which an 8 x 8 launch is split (S = 2, at least 64 channels per workgroup): a non-zero slab query
    x, w, b = _f32(6, 1, 8, 8, 128).to(dev), _f32(7, 64, 128, 3, 3).to(dev) * 0.1, _f32(8, 64).to(dev)
    with torch.cuda.device(dev):
        assert rt.conv3x3_wino4_split_bytes(1, 8, 8, 128, 64) > 0
    out["conv3x3_wino4_split"] = rt.conv3x3_wino4_split(x, rt.conv3x3_wino_pack(w), b, 64)
    x, w = _f32(9, 1, 4, 4, 64).to(dev), _f32(10, 64, 64, 3, 3).to(dev) * 0.1
    out["conv3x3_up2x_poly"] = rt.conv3x3_up2x_poly(x, rt.conv3x3_up2x_poly_pack(w), b, 64)
    out["resize_bilinear"], out["resize_nearest"] = rt.resize_bilinear(image, (8, 12)), rt.resize_nearest(image, (8, 12))
    out["mask_composite"] = rt.mask_composite(img, image, mask_u8.float())
    out["quantize_u8"] = rt.quantize_u8(image)
    out["u8_to_f32"] = rt.u8_to_f32(u8)
    out["warp_blend_u8"] = rt.warp_blend_u8(u8[0], u8[1], _f32(11, 2, 16, 24).to(dev) * 4, 0.5)
    out["resize_area_u8"] = rt.resize_area_u8(u8, (12, 8))
    out["resize_pil_bilinear_u8"] = rt.resize_pil_bilinear_u8(u8, (12, 8))
    out["colour_transfer_u8"], out["colour_record"] = rt.colour_transfer_u8(u8[0], u8[1])
    out["localized_combine_u8"], out["combine_record"] = rt.localized_combine_u8(u8[0], u8[1], mask_u8[0, 0])
    files, lengths = rt.jpeg_encode_u8(u8)
    out["jpeg_lengths"] = lengths
    for i, k in enumerate(lengths.cpu().tolist()):           # the rest of a row is not written
        out[f"jpeg_file{i}"] = files[i, :k]
    grays = out["frames_to_gray"] = fl.frames_to_gray(_u8(12, 2, 32, 40, 3).to(dev))
    seq = fl.FlowSequence()
    assert seq.push(grays[0]) is None
    out["farneback"] = seq.push(grays[1])
    tv = fl.DualTVL1OpticalFlow_create(nscales=2, warps=2, outerIterations=2, innerIterations=5)
    out["tvl1"] = tv.calc(grays[0], grays[1], None).contiguous()
    torch.cuda.synchronize(dev)
    return out


def test_every_call_runs_with_the_tensors_device_current(weights, monkeypatch):
    if torch.cuda.device_count() < 2:
        reason = f"needs two GPUs (a tensor on a device that is not the current one), this machine has {torch.cuda.device_count()}"
        print(reason)
        pytest.skip(reason)
    import applied_image_processing_amd.runtime as rt
    from applied_image_processing_amd import flow as fl

    dev = torch.device("cuda", 1)
    before = torch.cuda.current_device()
    torch.cuda.set_device(0)
    try:
        proxy = Recorder(rt.lib())
        monkeypatch.setattr(rt, "_lib", proxy)
        got = _every_call(rt, fl, weights, dev)
        monkeypatch.undo()
        assert torch.cuda.current_device() == 0
        names = {name for name, _ in proxy.calls}
        for needed in ("adain_encode_workspace_bytes", "adain_encode_multi_workspace_bytes", "adain_decode_workspace_bytes",
                       "adain_stylize_u8_workspace_bytes", "adain_conv3x3_wino4_split_workspace_bytes", "adain_jpeg_encode_u8_bytes",
                       "adain_encoder_pack", "adain_farneback_flow", "adain_tvl1_flow"):
            assert needed in names, f"{needed} was not recorded"
        elsewhere = [(name, d) for name, d in proxy.calls if d != 1 and not any(fnmatch.fnmatchcase(name, p) for p in DEVICE_FREE)]
        assert not elsewhere, f"called with another device current than the tensors': {elsewhere}"
        with torch.cuda.device(1):
            want = _every_call(rt, fl, weights, dev)
        assert torch.cuda.current_device() == 0
        assert sorted(got) == sorted(want)
        for step in want:
            assert got[step].device == dev and torch.equal(got[step], want[step]), step
    finally:
        torch.cuda.set_device(before)
