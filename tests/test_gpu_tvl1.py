"""GPU tests of the Dual TV-L1 optical-flow estimator (csrc/tvl1.hip, tvl1.py, video.device_flow_provider_all) against the NumPy
restatement of OpenCV's rules (tests/tvl1_ref.py): the prepared frames, every stage through the public parameters, the final flow
within the float32 noise floor of the float64 yardstick, the stop decisions, known answers, batch invariance and determinism, and
the video caller end to end.  Run with ``-m gpu``."""
import numpy as np
import pytest
import torch

import farneback_ref as F
import tvl1_ref as T

import applied_image_processing_amd.synth as synth
from oracle import adain_oracle as O

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def tv():
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    import applied_image_processing_amd.runtime as rt
    from applied_image_processing_amd import tvl1

    rt.lib()
    return tvl1


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _rel(a, b):
    n = np.linalg.norm(b)
    return float(np.linalg.norm(np.asarray(a, np.float64) - b) / (n if n > 0 else 1.0))


def _device_flow(tv, a, b, **params):
    t = tv.TVL1(a.shape[0], a.shape[1], **params)
    it = torch.zeros((1, len(t.scales), t.P.warps), dtype=torch.int32, device="cuda")
    f = t.flows([t.prepare(dev(a))], [t.prepare(dev(b))], iters_out=it)
    return f[0].cpu().numpy(), it[0].cpu().numpy()


@pytest.mark.parametrize("hw", [(36, 64), (256, 256), (255, 331)])
def test_prepared_frames_vs_float64(tv, hw):
    h, w = hw
    a = T.texture(h, w, seed=5)
    t = tv.TVL1(h, w)
    got = [[x.cpu().numpy() for x in s] for s in t.prepared_views(t.prepare(dev(a)))]
    want, f32 = T.prepare(a), T.prepare(a, dtype=np.float32)
    assert len(got) == len(want) == len(t.scales)
    for k, (g, r, f) in enumerate(zip(got, want, f32)):
        for c in range(3):
            assert g[c].shape == r[c].shape
            assert _rel(g[c], r[c]) <= max(1e-6, 2 * _rel(f[c], r[c])), (k, c, _rel(g[c], r[c]), _rel(f[c], r[c]))


STAGES = [dict(nscales=1, warps=1, outerIterations=1, innerIterations=1, medianFiltering=1),    # remap, rho, V, div, U
          dict(nscales=1, warps=1, outerIterations=1, innerIterations=2, medianFiltering=1),    # + the dual update
          dict(nscales=1, warps=1, outerIterations=2, innerIterations=2, medianFiltering=5),    # + the median
          dict(nscales=1, warps=2, outerIterations=1, innerIterations=3, medianFiltering=3),    # + the second remap
          dict(nscales=2, warps=1, outerIterations=1, innerIterations=3, medianFiltering=1)]    # + the upscale


@pytest.mark.parametrize("params", STAGES, ids=lambda p: "-".join(f"{k[0]}{v}" for k, v in p.items()))
def test_stages_vs_restatement(tv, params):
    h, w = 48, 80
    a = T.texture(h, w, seed=11)
    b = T.texture(h, w, (1.2, -0.7), seed=11)
    got, it = _device_flow(tv, a, b, **params)
    ref, rit, _ = T.tvl1(a, b, **params)
    f32, fit, _ = T.tvl1(a, b, dtype=np.float32, **params)
    assert (it == rit).all() and (fit == rit).all(), (it, rit, fit)
    d, d32 = _rel(got, ref), _rel(f32, ref)
    print(f"{params}: device rel-L2 {d:.3e}, float32 restatement {d32:.3e}")
    assert np.isfinite(got).all() and d <= max(2 * d32, 1e-6), (d, d32)


def _epe_stats(f, ref, margin):
    e = T.endpoint_error(f, ref)
    return np.array([np.median(e), np.percentile(e, 99), e[margin:-margin, margin:-margin].max()])


# measured on an MI355X: (median, p99, interior max) of the endpoint distance from float64 in px, for the device flow and for the
# float32 restatement on the same pair (defaults); the test holds the device to <= 2x the float32 restatement's distance
# (seed 9, shift (1.3, -0.8)).  The device's distance equals the float32 restatement's: it follows the same float operations and
# makes the same stop decisions; both are far from float64 where their stop decisions differ from float64's.
MEASURED = {
    (36, 64): ((8.74e-06, 6.70e-04, 6.74e-04), (8.74e-06, 6.70e-04, 6.74e-04)),
    (256, 256): ((7.57e-03, 5.77e-02, 4.86e-02), (7.57e-03, 5.77e-02, 4.86e-02)),
    (255, 331): ((4.94e-03, 2.95e-02, 3.27e-02), (4.94e-03, 2.95e-02, 3.27e-02)),
}


@pytest.mark.parametrize("hw", sorted(MEASURED))
def test_defaults_vs_float64_within_the_float32_noise_floor(tv, hw):
    h, w = hw
    a = T.texture(h, w, seed=9)
    b = T.texture(h, w, (1.3, -0.8), seed=9)
    got = tv.DualTVL1OpticalFlow_create().calc(dev(a), dev(b), None)
    assert got.shape == (h, w, 2) and got.dtype == torch.float32
    got = got.permute(2, 0, 1).cpu().numpy()
    ref, _, _ = T.tvl1(a, b)
    f32, _, _ = T.tvl1(a, b, dtype=np.float32)
    margin = min(8, h // 4, w // 4)
    ds, fs = _epe_stats(got, ref, margin), _epe_stats(f32, ref, margin)
    print(f"{hw}: device {ds}, float32 restatement {fs}")
    assert np.isfinite(got).all()
    assert (ds <= 2 * fs + 1e-6).all(), (ds, fs)


# chosen on the CPU (36 x 64, defaults): every stop decision of the float64 restatement is at least 1e-3 (relative) away from
# scaledEpsilon.  That margin alone does not settle the counts: on about a third of such 36 x 64 fixtures the float32 restatement's
# counts already differ from float64's at the finest scale (the error near the stop is a sum of tiny du^2 whose float rounding
# reaches ~3e-3 relative after hundreds of steps).  The device follows the float32 restatement operation by operation, so its counts
# must equal float32's on every fixture, and float64's on those where float32's do (the last flag, measured on the CPU).
STOP_FIXTURES = [((36, 64), 4, (0.6, -0.3), True), ((36, 64), 5, (1.3, -0.8), True), ((36, 64), 8, (1.3, -0.8), True),
                 ((36, 64), 3, (1.3, -0.8), True), ((36, 64), 2, (0.6, -0.3), False)]


@pytest.mark.parametrize("hw,seed,shift,same_as_f64", STOP_FIXTURES)
def test_stop_decisions_match_the_restatement(tv, hw, seed, shift, same_as_f64):
    h, w = hw
    a, b = T.texture(h, w, seed=seed), T.texture(h, w, shift, seed=seed)
    ref, rit, margins = T.tvl1(a, b)
    _, fit, _ = T.tvl1(a, b, dtype=np.float32)
    assert margins.min() >= 1e-3, margins.min()
    assert (fit == rit).all() == same_as_f64
    _, it = _device_flow(tv, a, b)
    assert (it == fit).all(), (it, fit)
    if same_as_f64:
        assert (it == rit).all(), (it, rit)


def test_known_answers(tv):
    calc = tv.DualTVL1OpticalFlow_create().calc
    a = T.texture(64, 96, seed=4)
    c = np.full((64, 96), 131, np.uint8)
    for f in (a, c):
        assert torch.count_nonzero(calc(dev(f), dev(f))).item() == 0
    shift = (0.6, -0.4)
    b = T.texture(64, 96, shift, seed=4)
    got = calc(dev(a), dev(b)).permute(2, 0, 1).cpu().numpy()
    ref, _, _ = T.tvl1(a, b)
    truth = np.array(shift)[:, None, None]
    e = T.endpoint_error(got, truth)[12:-12, 12:-12]
    er = T.endpoint_error(ref, truth)[12:-12, 12:-12]
    print(f"translation {shift}: device median {np.median(e):.4f}, float64 restatement {np.median(er):.4f}")
    assert np.median(e) <= 2 * np.median(er) + 0.01 and np.median(e) < 0.2


def test_host_or_foreign_buffers_are_refused(tv):
    """out / iters_out / prepared frames that are not device buffers of the frames' device (or not aligned as prepare() aligns
    them) are refused with AdainHipError before anything is launched."""
    import applied_image_processing_amd.runtime as rt

    h, w = 36, 64
    t = tv.TVL1(h, w)
    g = dev(T.texture(h, w, seed=1))
    pa, pb = t.prepare(g), t.prepare(g)
    ns, nw = len(t.scales), t.P.warps
    with pytest.raises(rt.AdainHipError, match="iters_out"):
        t.flows([pa], [pb], iters_out=torch.zeros((1, ns, nw), dtype=torch.int32))
    with pytest.raises(rt.AdainHipError, match="out must"):
        t.flows([pa], [pb], out=torch.empty((1, 2, h, w)))
    with pytest.raises(rt.AdainHipError, match="out must"):
        t.prepare(g, out=torch.empty((1, t.frame_floats)))
    with pytest.raises(rt.AdainHipError, match="prepared frames"):
        t.flows([pa.cpu()], [pb])
    big = torch.empty(t.frame_floats + 64, device="cuda")
    with pytest.raises(rt.AdainHipError, match="prepared frames"):
        t.flows([big[1:]], [pb])
    with pytest.raises(rt.AdainHipError, match="out must"):
        tv.TVL1Sequence().batch([g, g], out=torch.empty((1, 2, h, w)))
    torch.cuda.synchronize()                                     # the device is still fine
    assert torch.count_nonzero(t.flows([pa], [pb])).item() == 0


def test_batch_invariance_and_determinism(tv):
    h, w = 40, 72
    frames = [T.texture(h, w, (0.5 * i, -0.3 * i), seed=30 + i % 3) for i in range(8)]
    t = tv.TVL1(h, w)
    prep = [t.prepare(dev(f)) for f in frames]
    n = 7
    it = torch.zeros((n, len(t.scales), t.P.warps), dtype=torch.int32, device="cuda")
    batch = t.flows(prep[:n], prep[1:n + 1], iters_out=it)
    its = it.cpu().numpy()
    assert len({int(x.sum()) for x in its}) > 1                  # the pairs stop at different points
    for k in (0, n - 1):
        it1 = torch.zeros((1, len(t.scales), t.P.warps), dtype=torch.int32, device="cuda")
        alone = t.flows([prep[k]], [prep[k + 1]], iters_out=it1)
        assert torch.equal(alone[0], batch[k]) and (it1[0].cpu().numpy() == its[k]).all(), k
    # the same pair last in a batch of different pairs
    it2 = torch.zeros((n, len(t.scales), t.P.warps), dtype=torch.int32, device="cuda")
    order = list(range(1, n)) + [0]
    moved = t.flows([prep[j] for j in order], [prep[j + 1] for j in order], iters_out=it2)
    assert torch.equal(moved[n - 1], batch[0]) and (it2[n - 1].cpu().numpy() == its[0]).all()
    again = t.flows(prep[:n], prep[1:n + 1])
    assert torch.equal(again, batch)
    grays = [dev(f) for f in frames]
    seq = tv.TVL1Sequence().batch(grays, max_pairs=3)
    pairs = [tv.DualTVL1OpticalFlow_create().calc(grays[i], grays[i + 1]).permute(2, 0, 1) for i in range(7)]
    assert seq.shape == (7, 2, h, w)
    for i in range(7):
        assert torch.equal(seq[i], pairs[i]) and torch.equal(seq[i], batch[i]), i
    assert torch.equal(tv.TVL1Sequence().batch(grays), seq)


def test_video_caller_with_dualtvl1(tv, weights, tmp_path):
    """apply_style_transfer_multi_ada with video.device_flow_provider_all and flow_method='dualtvl1' writes every frame, within the
    +-2 LSB rule of O.temporal_blend fed the restatement's flows; with 'farneback' its files equal device_flow_provider's."""
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
        for tag, prov, method in [("tv", video.device_flow_provider_all, "dualtvl1"), ("fb_all", video.device_flow_provider_all, "farneback"),
                                  ("fb", video.device_flow_provider, "farneback")]:
            video.set_flow_provider(prov)
            odir = tmp_path / tag
            video.apply_style_transfer_multi_ada(str(cdir), str(sdir), str(odir), flow_method=method, alpha=0.7,
                                                 target_resolution=(64, 36), engine=engine)
            outs[tag] = [np.asarray(Image.open(odir / f"frame_{i:04d}.png")) for i in range(n)]
        with pytest.raises(ValueError, match="unknown optical-flow method"):
            video.set_flow_provider(video.device_flow_provider_all)
            video.apply_style_transfer_multi_ada(str(cdir), str(sdir), str(tmp_path / "x"), flow_method="nope", alpha=0.7,
                                                 target_resolution=(64, 36), engine=engine)
    finally:
        t.set_depth_provider(None)
        video.set_flow_provider(None)
    for i in range(n):
        assert np.array_equal(outs["fb_all"][i], outs["fb"][i]), i
    # the per-pair provider gives the batched path's flow, bit for bit
    tvf = video.device_flow_provider_all(str(cdir / "frame_0000.png"), str(cdir / "frame_0001.png"), (64, 36), "dualtvl1")
    assert tvf.shape == (2, 36, 64)
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
    flows = np.stack([T.tvl1(grays[i], grays[i + 1], dtype=np.float32)[0] for i in range(n - 1)])
    want = O.temporal_blend(np.stack(small), flows, 0.7)
    for i in range(n):
        d = np.abs(outs["tv"][i].astype(int) - want[i].astype(int))
        assert d.max() <= 2 and (d > 0).mean() < 0.02, (i, d.max(), (d > 0).mean())
