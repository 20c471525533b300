"""GPU tests of the Dual TV-L1 estimator (csrc/tvl1.hip, tvl1.py) OFF create()'s defaults and on tiny frames, against the NumPy
restatement (tests/tvl1_ref.py; tests/test_flow_params_host.py checks the restatement itself there).  tests/test_gpu_tvl1.py moves
the loop counts only; here: scaleStep 0.5 (INTER_AREA's 2x shrink of odd sizes) and 1.0 (every scale a copy), tau / lambda / theta /
epsilon off their defaults, no inner steps, no warps, a rule that never stops and one that stops at once, a single scale, and frames
of 3 x 3 and 5 x 4 where every remap window touches the border; batch invariance off the defaults.  The rules are those of
test_stages_vs_restatement and STOP_FIXTURES in tests/test_gpu_tvl1.py, unchanged.  Run with ``-m gpu``."""
import functools

import numpy as np
import pytest
import torch

import tvl1_ref as T

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def tv():
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    import applied_image_processing_amd.runtime as rt
    from applied_image_processing_amd import tvl1

    rt.lib()
    return tvl1


def dev(a):
    return torch.from_numpy(np.array(a)).cuda()


def _rel(a, b):
    n = np.linalg.norm(b)
    return float(np.linalg.norm(np.asarray(a, np.float64) - b) / (n if n > 0 else 1.0))


def _device_flow(tv, a, b, **params):
    t = tv.TVL1(a.shape[0], a.shape[1], **params)
    it = torch.full((1, len(t.scales), t.P.warps), -1, dtype=torch.int32, device="cuda")
    f = t.flows([t.prepare(dev(a))], [t.prepare(dev(b))], iters_out=it)
    return f[0].cpu().numpy(), it[0].cpu().numpy()


TINY = dict(nscales=1, warps=1, outerIterations=1, innerIterations=3, medianFiltering=5)
# id -> (h, w, parameters, seed, shift, the float32 restatement's counts equal float64's (measured on the CPU)).  The pair is
# T.texture(h, w, seed) and its translate by `shift`.  Wherever a count depends on a stop decision the fixture was chosen on the CPU
# (seeds 1.., three shifts) so that every stop decision of the float64 restatement is at least 1e-3 (relative) away from
# scaledEpsilon; the test asserts that condition on the fixture.  It is no tolerance.  The smallest margins, measured on the CPU:
#   39x41-step0.5 1.0e-2, 39x43-step0.5 1.9e-2, 40x72-step1.0 5.7 (no warp stops: 10 steps each), 36x64-tau-lambda-theta 3.9e-3,
#   36x64-eps10 1.0, 16x16 1.4e-2, 17x70 1.5e-2, 3x3 1.5e+2, 5x4 1.6e+2 (no stop within the 3 steps); none where no step runs or epsilon is 0.
CASES = {
    "39x41-step0.5": (39, 41, dict(scaleStep=0.5, nscales=3), 1, (1.3, -0.8), True),
    "39x43-step0.5": (39, 43, dict(scaleStep=0.5, nscales=3), 4, (1.3, -0.8), True),
    "40x72-step1.0": (40, 72, dict(scaleStep=1.0, nscales=2, warps=2, outerIterations=2, innerIterations=5), 1, (0.7, -0.4), True),
    "36x64-tau-lambda-theta": (36, 64, dict(tau=0.1, lambda_=0.05, theta=0.5, medianFiltering=3, epsilon=0.02), 1, (0.6, -0.3), True),
    "36x64-inner0": (36, 64, dict(innerIterations=0, outerIterations=2, warps=1, nscales=1, medianFiltering=5), 1, (0.7, -0.4), True),
    "36x64-warps0": (36, 64, dict(warps=0), 1, (0.7, -0.4), True),
    "36x64-eps0": (36, 64, dict(epsilon=0.0, warps=1, outerIterations=1, innerIterations=4, nscales=2), 1, (0.7, -0.4), True),
    "36x64-eps10": (36, 64, dict(epsilon=10.0), 1, (0.7, -0.4), True),
    "16x16-defaults": (16, 16, dict(), 1, (0.7, -0.4), True),
    "17x70-defaults": (17, 70, dict(), 2, (0.7, -0.4), True),
    "3x3-tiny": (3, 3, TINY, 1, (0.7, -0.4), True),
    "5x4-tiny": (5, 4, TINY, 1, (0.7, -0.4), True),
}

# measured on an MI355X: rel-L2 distance from the float64 restatement's flow of the device flow and of the float32 restatement's
MEASURED = {
    "39x41-step0.5": (5.643e-07, 5.643e-07),
    "39x43-step0.5": (6.821e-07, 6.821e-07),
    "40x72-step1.0": (8.557e-07, 8.557e-07),
    "36x64-tau-lambda-theta": (1.801e-04, 1.801e-04),
    "36x64-inner0": (0.000e+00, 0.000e+00),
    "36x64-warps0": (0.000e+00, 0.000e+00),
    "36x64-eps0": (3.226e-04, 3.226e-04),
    "36x64-eps10": (3.873e-03, 3.873e-03),
    "16x16-defaults": (5.507e-07, 5.507e-07),
    "17x70-defaults": (1.320e-06, 1.320e-06),
    "3x3-tiny": (4.379e-08, 4.379e-08),
    "5x4-tiny": (6.816e-08, 6.816e-08),
}


@functools.lru_cache(maxsize=None)
def _refs(case):
    h, w, params, seed, shift, _ = CASES[case]
    a, b = T.texture(h, w, seed=seed), T.texture(h, w, shift, seed=seed)
    ref, rit, margins = T.tvl1(a, b, **params)
    f32, fit, _ = T.tvl1(a, b, dtype=np.float32, **params)
    for v in (a, b, ref, rit, margins, f32, fit):
        v.setflags(write=False)
    return a, b, ref, rit, margins, f32, fit


@pytest.mark.parametrize("case", list(CASES))
def test_flow_and_counts_off_the_defaults(tv, case):
    h, w, params, _, _, same_as_f64 = CASES[case]
    a, b, ref, rit, margins, f32, fit = _refs(case)
    assert margins.size == 0 or margins.min() >= 1e-3, margins.min()        # a condition on the fixture
    assert bool((fit == rit).all()) == same_as_f64
    got, it = _device_flow(tv, a, b, **params)
    assert it.shape == fit.shape and (it == fit).all(), (it, fit)
    if same_as_f64:
        assert (it == rit).all(), (it, rit)
    d, d32 = _rel(got, ref), _rel(f32, ref)
    print(f"{case}: device rel-L2 {d:.3e}, float32 restatement {d32:.3e}, counts {it.tolist()}")
    assert np.isfinite(got).all() and d <= max(2 * d32, 1e-6), (d, d32)
    # what each case is there for
    if case == "36x64-inner0":
        assert not it.any() and not got.any()                      # medians of a zero flow only
    if case == "36x64-warps0":
        assert it.shape == (4, 0) and not got.any()
    if case == "36x64-eps0":
        assert (it == 4).all()                                     # outer x inner, exactly
    if case == "36x64-eps10":
        assert it.shape == (4, 5) and (it == 1).all()
    if case in ("16x16-defaults", "17x70-defaults", "3x3-tiny", "5x4-tiny"):
        assert it.shape[0] == 1
    if case in ("3x3-tiny", "5x4-tiny"):
        assert (it == 3).all()


@pytest.mark.parametrize("hw", [(39, 41), (39, 43), (37, 39)])
def test_prepared_frames_at_scale_step_one_half(tv, hw):
    """scaleStep 0.5 takes INTER_AREA's 2 x 2 mean whatever the sizes are: 39 rows become 20 and the last holds source row 38 alone,
    43 columns become 22 (a partial last column and a one-pixel corner), 41 become 20 (column 40 is never read), 37 rows become 18."""
    h, w = hw
    p = dict(scaleStep=0.5, nscales=3)
    a = T.texture(h, w, seed=5)
    t = tv.TVL1(h, w, **p)
    got = [[x.cpu().numpy() for x in s] for s in t.prepared_views(t.prepare(dev(a)))]
    want, f32 = T.prepare(a, 3, 0.5), T.prepare(a, 3, 0.5, dtype=np.float32)
    assert len(got) == len(want) == len(t.scales) == 2
    for k, (g, r, f) in enumerate(zip(got, want, f32)):
        for c in range(3):
            assert g[c].shape == r[c].shape
            assert _rel(g[c], r[c]) <= max(1e-6, 2 * _rel(f[c], r[c])), (k, c, _rel(g[c], r[c]), _rel(f[c], r[c]))
    # the partial cells by hand: means of 2, 2 and 1 source pixels (integers: exact in float)
    I0, I1 = got[0][0].astype(np.float64), got[1][0].astype(np.float64)
    if h % 4 == 3:
        assert np.array_equal(I1[-1, :w // 2], 0.5 * (I0[h - 1, 0:w // 2 * 2:2] + I0[h - 1, 1:w // 2 * 2:2]))
    if w % 4 == 3:
        assert np.array_equal(I1[:h // 2, -1], 0.5 * (I0[0:h // 2 * 2:2, w - 1] + I0[1:h // 2 * 2:2, w - 1]))
    if h % 4 == 3 and w % 4 == 3:
        assert I1[-1, -1] == I0[-1, -1]


def test_batch_invariance_off_the_defaults(tv):
    """Five pairs in one call with tau, theta and epsilon off their defaults stop at different steps; a pair alone gives the bits and
    the counts it gives in the batch (test_batch_invariance_and_determinism of tests/test_gpu_tvl1.py runs at the defaults)."""
    h, w = 40, 72
    p = dict(tau=0.15, theta=0.25, epsilon=0.03)
    frames = [T.texture(h, w, (0.5 * i, -0.3 * i), seed=30 + i % 3) for i in range(6)]
    t = tv.TVL1(h, w, **p)
    prep = [t.prepare(dev(f)) for f in frames]
    n = 5
    shape = (len(t.scales), t.P.warps)
    it = torch.full((n,) + shape, -1, dtype=torch.int32, device="cuda")
    batch = t.flows(prep[:n], prep[1:n + 1], iters_out=it)
    its = it.cpu().numpy()
    print("steps per pair:", [int(x.sum()) for x in its])
    assert (its >= 1).all() and len({int(x.sum()) for x in its}) > 1           # the pairs stop at different points
    for k in (0, n - 1):
        it1 = torch.full((1,) + shape, -1, dtype=torch.int32, device="cuda")
        alone = t.flows([prep[k]], [prep[k + 1]], iters_out=it1)
        assert torch.equal(alone[0], batch[k]) and (it1[0].cpu().numpy() == its[k]).all(), k
    assert torch.equal(t.flows(prep[:n], prep[1:n + 1]), batch)
    # the float32 restatement's counts for the first pair: the off-default parameters reach the step kernel
    _, fit, _ = T.tvl1(frames[0], frames[1], dtype=np.float32, **p)
    assert (its[0] == fit).all(), (its[0], fit)
