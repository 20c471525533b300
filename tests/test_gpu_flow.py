"""GPU tests of the Farneback optical-flow estimator (csrc/flow.hip, flow.py, video.device_flow_provider) against the NumPy
restatement of OpenCV's rules (tests/farneback_ref.py): the frame preparation bit for bit, every stage and the final flow within
the float32 noise floor of the float64 yardstick, known answers, sequence == pairs, determinism, and the video caller end to end.
Run with ``-m gpu``."""
import os

import numpy as np
import pytest
import torch

import farneback_ref as F

import applied_image_processing_amd.synth as synth
from oracle import adain_oracle as O

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def fl():
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    import applied_image_processing_amd.runtime as rt
    from applied_image_processing_amd import flow

    rt.lib()
    return flow


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _rel(a, b):
    return float(np.linalg.norm(np.asarray(a, np.float64) - b) / np.linalg.norm(b))


@pytest.mark.parametrize("hi,wi,ho,wo", [(100, 150, 37, 61), (20, 30, 45, 70), (72, 128, 36, 64), (41, 53, 41, 53), (256, 256, 256, 256),
                                         (1080, 1920, 256, 455), (33, 17, 20, 40)])
def test_frames_to_gray_bit_exact(fl, hi, wi, ho, wo):
    """Shrink, enlarge, exact 2x (INTER_AREA's 2x2 mean), equal size (a copy), and mixed axes - three frames per launch."""
    rng = np.random.default_rng(hi * 7 + wo)
    rgb = rng.integers(0, 256, (3, hi, wi, 3), dtype=np.uint8)
    got = fl.frames_to_gray(dev(rgb), (wo, ho)).cpu().numpy()
    for i in range(3):
        assert np.array_equal(got[i], F.frame_to_gray(rgb[i], wo, ho)), i
    assert np.array_equal(fl.frames_to_gray(dev(rgb[0]), (wo, ho)).cpu().numpy(), got[0])


@pytest.mark.parametrize("hw", [(256, 256), (331, 255), (1080, 1920)])
def test_pyramid_stages_vs_float64(fl, hw):
    """Level images and polynomial expansions within rel-L2 1e-6 of the float64 restatement (or, where the float32 restatement
    itself is farther, within 2x of its distance)."""
    h, w = hw
    a = F.texture(h, w, seed=5)
    fb = fl.Farneback(h, w)
    got = [(i.cpu().numpy(), r.cpu().numpy()) for i, r in fl.pyramid_views(fb.expand(dev(a)), h, w)]
    want = F.pyramid(a)
    f32 = F.pyramid(a, dtype=np.float32)
    assert len(got) == len(want)
    for k, ((gi, gr), (wi_, wr), (fi, fr)) in enumerate(zip(got, want, f32)):
        assert gi.shape == wi_.shape and gr.shape == wr.shape
        ri, rr = _rel(gi, wi_), _rel(gr, wr)
        assert ri <= max(1e-6, 2 * _rel(fi, wi_)), (k, ri)
        assert rr <= max(1e-6, 2 * _rel(fr, wr)), (k, rr, _rel(fr, wr))


def _epe_stats(f, ref, margin):
    e = F.endpoint_error(f, ref)
    inner = e[margin:-margin, margin:-margin] if margin else e
    return np.array([np.median(e), np.percentile(e, 99), inner.max()])


# measured on an MI355X: (median, p99, interior max) of the endpoint distance from float64 in px, for the device flow and for the
# float32 restatement on the same pair; the test holds the device to <= 2x the float32 restatement's distance on every statistic
# (the device column was measured while flow.hip was built with fused multiply-adds; built without them, as it is now, the device
# follows the float32 restatement operation by operation, see tests/test_gpu_flow_params.py)
MEASURED = {
    (36, 64): ((1.19e-07, 4.75e-07, 3.49e-07), (1.21e-07, 4.20e-07, 3.66e-07)),
    (256, 256): ((3.74e-07, 1.33e-06, 2.22e-06), (3.63e-07, 1.34e-06, 2.34e-06)),
    (331, 255): ((4.18e-07, 1.78e-06, 2.82e-06), (4.21e-07, 1.74e-06, 2.82e-06)),
    (1080, 1920): ((2.07e-06, 8.37e-06, 1.81e-05), (2.07e-06, 8.39e-06, 1.84e-05)),
}


@pytest.mark.parametrize("hw", sorted(MEASURED))
def test_flow_vs_float64_within_the_float32_noise_floor(fl, hw):
    h, w = hw
    a = F.texture(h, w, seed=9)
    b = F.texture(h, w, (1.3, -0.8), seed=9)
    got = fl.calc_optical_flow_farneback(dev(a), dev(b), None, 0.5, 5, 15, 3, 7, 1.5, 0)
    assert got.shape == (h, w, 2) and got.dtype == torch.float32
    got = got.permute(2, 0, 1).cpu().numpy()
    ref = F.farneback(a, b)
    f32 = F.farneback(a, b, dtype=np.float32)
    margin = min(16, h // 4, w // 4)
    dev_s, f32_s = _epe_stats(got, ref, margin), _epe_stats(f32, ref, margin)
    print(f"{hw}: device {dev_s}, float32 restatement {f32_s}")
    assert np.isfinite(got).all()
    assert (dev_s <= 2 * f32_s + 1e-7).all(), (dev_s, f32_s)


def test_identical_frames(fl):
    """Constant frames: exactly zero flow.  Identical textured frames: OpenCV's "else" branch of the matrix update at the last
    row / column leaves a small residual (tests/test_flow_host.py); the device gives the restatement's flow."""
    c = np.full((256, 256), 131, np.uint8)
    assert torch.count_nonzero(fl.calc_optical_flow_farneback(dev(c), dev(c))).item() == 0
    a = F.texture(256, 256, seed=4)
    got = fl.calc_optical_flow_farneback(dev(a), dev(a)).permute(2, 0, 1).cpu().numpy()
    ref = F.farneback(a, a)
    assert F.endpoint_error(got, ref).max() <= 2 * F.endpoint_error(F.farneback(a, a, dtype=np.float32), ref).max() + 1e-6
    assert np.median(F.endpoint_error(got, 0 * ref)) < 1e-4


# the float64 restatement's interior (32 px margin) median / p95 endpoint errors on these translations, measured on the CPU:
# 256^2 (0.6, -0.3): 0.0110 / 0.0345; (3.2, 1.7): 0.0086 / 0.0263; (9.5, -6.0): 0.0206 / 0.0579; 1080p (5.3, -2.7): 0.0128 / 0.0393.
# The bounds are 2x those, rounded up.
TRANSLATIONS = [((256, 256), (0.6, -0.3), 7, 0.022, 0.069), ((256, 256), (3.2, 1.7), 7, 0.018, 0.053),
                ((256, 256), (9.5, -6.0), 7, 0.042, 0.116), ((1080, 1920), (5.3, -2.7), 11, 0.026, 0.079)]


@pytest.mark.parametrize("hw,shift,seed,med_bound,p95_bound", TRANSLATIONS)
def test_known_translation(fl, hw, shift, seed, med_bound, p95_bound):
    h, w = hw
    a = F.texture(h, w, seed=seed)
    b = F.texture(h, w, shift, seed=seed)
    got = fl.calc_optical_flow_farneback(dev(a), dev(b)).permute(2, 0, 1).cpu().numpy()
    e = F.endpoint_error(got, np.array(shift)[:, None, None])[32:-32, 32:-32]
    print(f"{hw} {shift}: median {np.median(e):.4f}, p95 {np.percentile(e, 95):.4f}")
    assert np.median(e) < med_bound and np.percentile(e, 95) < p95_bound, (np.median(e), np.percentile(e, 95))


def test_sequence_equals_pairs_and_is_deterministic(fl):
    frames = [F.texture(180, 320, (0.7 * i, -0.4 * i), seed=2) for i in range(6)]
    grays = [dev(f) for f in frames]
    seq = fl.FlowSequence(0.5, 5, 15, 3, 7, 1.5, 0)
    flows = [f.clone() for f in seq.flows(grays)]
    pairs = [fl.calc_optical_flow_farneback(grays[i], grays[i + 1]).permute(2, 0, 1) for i in range(5)]
    batch = fl.FlowSequence().batch(grays)
    assert len(flows) == 5 and batch.shape == (5, 2, 180, 320)
    for i in range(5):
        assert torch.equal(flows[i], pairs[i]) and torch.equal(batch[i], pairs[i]), i
    again = fl.FlowSequence().batch(grays)
    assert torch.equal(again, batch)


def test_video_caller_with_the_device_provider(fl, weights, tmp_path):
    """apply_style_transfer_multi_ada with video.device_flow_provider (the rank-0 sequence path) writes the same files as with a
    lambda wrapping it (the pair path), and both are within the +-2 LSB rule of O.temporal_blend fed the restatement's flows."""
    from PIL import Image

    import applied_image_processing_amd.jobs as jobs
    from applied_image_processing_amd import video
    from applied_image_processing_amd.AdaIN import test as t
    from applied_image_processing_amd.engine import AdaINEngine

    vgg_sd, dec_sd = weights
    engine = AdaINEngine(vgg_sd, dec_sd, "cuda:0")
    cdir, sdir = tmp_path / "frames", tmp_path / "styles"
    cdir.mkdir(); sdir.mkdir()
    n = 4
    rgb = []
    for i in range(n):
        g = F.texture(72, 128, (1.5 * i, 0.5 * i), seed=21)
        fr = np.stack([g, np.roll(g, 3, axis=1), 255 - g], axis=-1)
        rgb.append(fr)
        Image.fromarray(fr).save(cdir / f"frame_{i:04d}.png")
    for i in range(2):
        Image.fromarray((synth.image(460 + i, 1, 64, 64)[0].transpose(1, 2, 0) * 255).astype(np.uint8)).save(sdir / f"style_{i}.png")
    depth = lambda img: torch.from_numpy(np.ascontiguousarray(synth.smooth_depth(480 + img.size[0] % 7, img.size[1], img.size[0])))
    outs = {}
    t.set_depth_provider(depth)
    try:
        for tag, prov in [("seq", video.device_flow_provider), ("pairs", lambda *a: video.device_flow_provider(*a))]:
            video.set_flow_provider(prov)
            odir = tmp_path / tag
            video.apply_style_transfer_multi_ada(str(cdir), str(sdir), str(odir), alpha=0.7, target_resolution=(64, 36), engine=engine)
            outs[tag] = [np.asarray(Image.open(odir / f"frame_{i:04d}.png")) for i in range(n)]
        video.set_flow_provider(video.device_flow_provider)
        with pytest.raises(ValueError, match="DualTV-L1"):
            video.apply_style_transfer_multi_ada(str(cdir), str(sdir), str(tmp_path / "tv"), flow_method="dualtvl1", alpha=0.7,
                                                 target_resolution=(64, 36), engine=engine)
    finally:
        t.set_depth_provider(None)
        video.set_flow_provider(None)
    for i in range(n):
        assert np.array_equal(outs["seq"][i], outs["pairs"][i]), i
    # oracle chain: stylised + resized frames (oracle), flows from the restatement on the prepared gray frames
    tf, stf = t.test_transform(256, False), t.test_transform(512, False)
    styles = [stf(Image.open(sdir / f"style_{i}.png")).unsqueeze(0) for i in range(2)]
    sched = jobs.style_schedule(n, 2)
    small = []
    for i in range(n):
        c = tf(Image.open(cdir / f"frame_{i:04d}.png")).unsqueeze(0)
        d = depth(Image.open(cdir / f"frame_{i:04d}.png"))
        with torch.no_grad():
            u8 = O.quantize_u8(O.style_transfer(vgg_sd, dec_sd, c, styles[sched[i]], d, 1.0, 0.30, 20))[0].numpy()
        small.append(O.resize_area_u8(u8, (64, 36)))
    grays = [F.frame_to_gray(fr, 64, 36) for fr in rgb]
    flows = np.stack([F.farneback(grays[i], grays[i + 1], dtype=np.float32) for i in range(n - 1)])
    want = O.temporal_blend(np.stack(small), flows, 0.7)
    for i in range(n):
        d = np.abs(outs["seq"][i].astype(int) - want[i].astype(int))
        assert d.max() <= 2 and (d > 0).mean() < 0.02, (i, d.max(), (d > 0).mean())
