"""GPU tests of the AdaIN statistics and blend kernels (csrc/stats.hip: ``adain_mean_std``, ``adain_blend_alpha``,
``adain_blend_pmap``) away from the shapes the network produces, against tests/blend_ref.py.  Run with ``-m gpu``.

Blend.  The kernel states "the reference's operation order without FMA contraction" with a correctly rounded divide, and
blend_ref's float32 form is that sequence one rounding at a time, so the bar is equality of every element (``got != want`` nowhere;
never a norm: one wrong element fails).  Equality is the case that holds on the MI355X: no operation rounds differently.  The
inputs make a wrong index visible - statistics distinct per image and channel, strength maps distinct per image, and behind a
single style row a second row that differs from it by 1000, so that a read at ``[c]`` is not the value at ``[0]`` - and they are
kept out of cancellation: the float32 form stays within blend_ref.self_distance_bound of the float64 form on every element.
The NCHW shapes with ``c * hw % 4 != 0`` put a quad of four elements across two images (across four when ``c * hw == 1``).

Statistics.  Both layouts against the two-pass float64 reference, with bounds from the arithmetic.  The kernels accumulate sum and
sum of squares in float64 and take var = (q - s * m) / (hw - 1): one-pass, so its cancellation error is about 2^-53 * (mean / std)^2
relative in the variance.  The inputs keep |mean| / std <= 1e3 (asserted on the reference), which leaves that at 1.1e-10, far
below 2^-24 = 6e-8.  Then: the mean is the float64 mean rounded once - within 1 float32 ulp of it; the std is (float)var, + eps,
sqrtf - three roundings, the first two halved by the square root - within 2 float32 ulp of sqrt(var + eps).  One ulp is
np.spacing of the reference value rounded to float32.  ``eps`` reaches the kernel as a C float, so the reference gets
float(np.float32(1e-5)).  The NHWC sizes walk the launch's decisions: c / 4 thread columns that do or do not divide 256 (idle
threads; 256 rows at c = 4, one row at c = 520 and 1024), hw around the first block boundary rows * 16, a block count between 64
and 256 (the finalize wave strides twice or more) and one past the cap of 256.  Measured on an MI355X: mean at most 0.500 ulp, std at most 1.06 ulp over every case.

Python surface (16 * 2^-24 bound against the oracle in float64, test_python_surface_on_straddling_nchw): with dm <= u |mc|, ds / sc and
dss / ss <= 4 u (2 ulp), u = 2^-24, the error of t = (x - mc) / sc * ss + ms is at most u [(|mc| + 11 |x - mc|) / sc * ss + |ms| + |t|],
which 16 u ((|x| + |mc|) / sc * ss + |ms|) covers."""
import numpy as np
import pytest
import torch

import blend_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
EPS = float(np.float32(1e-5))
F32 = np.float32


@pytest.fixture(scope="module")
def rt():
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    import applied_image_processing_amd.runtime as rt

    rt.lib()
    torch.cuda.set_device(0)
    return rt


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def host(t):
    torch.cuda.synchronize()
    return t.cpu().numpy()


# ---- blend matrix ---------------------------------------------------------------------------------------------------------------------
NCHW_STRADDLING = [(2, 1, 2), (2, 3, 2), (2, 2, 3), (4, 1, 1), (4, 3, 5), (4, 3, 7), (4, 5, 3), (2, 3, 6)]
NCHW_CONTROLS = [(3, 4, 5), (2, 64, 99), (1, 3, 8)]
NCHW_GRID_STRIDE = [(4, 3, 700001)]          # 2100003 quads > 8192 x 256: every thread loops, the plane size is odd
NHWC_SHAPES = [(3, 4, 5), (3, 12, 5), (2, 520, 7), (4, 64, 1)]
SHAPES = [(False,) + s for s in NCHW_STRADDLING + NCHW_CONTROLS + NCHW_GRID_STRIDE] + [(True,) + s for s in NHWC_SHAPES]


def blend_inputs(nhwc, n, c, hw, style_n, pmap_n, seed=0):
    """x O(1); content mean 10 img + 16 ch / max(c, 16) + noise and the style's its negative with other noise, stds in [0.5, 2];
    strength maps 0.05 + 0.2 img + noise (at most 0.85).  The style arrays come with one more row than is handed over: row 0 + 1000."""
    rng = np.random.default_rng([seed, n, c, hw, int(nhwc)])
    x = rng.standard_normal((n, 1, hw, c) if nhwc else (n, c, 1, hw), dtype=F32)
    level = lambda rows: 10.0 * np.arange(rows)[:, None] + 16.0 * np.arange(c)[None, :] / max(c, 16)
    cm = (level(n) + 0.25 * rng.random((n, c))).astype(F32)
    cs = (0.5 + 1.5 * rng.random((n, c))).astype(F32)
    sm = np.concatenate([-(level(style_n) + 0.25 * rng.random((style_n, c))), np.zeros((1, c))]).astype(F32)
    ss = np.concatenate([0.5 + 1.5 * rng.random((style_n, c)), np.zeros((1, c))]).astype(F32)
    sm[style_n], ss[style_n] = sm[0] + 1000, ss[0] + 1000
    p = None
    if pmap_n:
        p = (0.05 + 0.2 * np.arange(pmap_n)[:, None] + 0.2 * rng.random((pmap_n, hw))).astype(F32)
        assert p.max() <= 0.85 + 1e-6
    return x, cm, cs, sm, ss, p


def run_blend(rt, nhwc, x, cm, cs, sm_buf, ss_buf, style_n, alpha=None, p=None):
    """The wrapper call, the style statistics being the first ``style_n`` rows of a longer device array."""
    sm, ss = dev(sm_buf)[:style_n], dev(ss_buf)[:style_n]
    assert sm.shape[0] == style_n
    if p is None:
        return host(rt.blend_alpha(dev(x), nhwc, dev(cm), dev(cs), sm, ss, alpha))
    return host(rt.blend_pmap(dev(x), nhwc, dev(cm), dev(cs), sm, ss, dev(p)))


def assert_equal_elements(what, got, want, nhwc, n, c, hw):
    bad = np.flatnonzero(got.reshape(-1) != want.reshape(-1))
    img, ch, pix = R.indices(n, c, hw, nhwc)
    where = [(int(img[i]), int(ch[i]), int(pix[i])) for i in bad[:8]]
    print(f"{what}: {bad.size} of {got.size} elements differ from the float32 reference" + (f", first (img, ch, pix): {where}" if bad.size else ""))
    assert got.shape == want.shape and got.dtype == want.dtype == F32
    assert bad.size == 0, f"{what}: {bad.size} elements differ, first (img, ch, pix) {where}: got {got.reshape(-1)[bad[:8]]}, want {want.reshape(-1)[bad[:8]]}"


def check_blend(rt, what, nhwc, x, cm, cs, sm, ss, style_n, alpha=None, p=None):
    n, c, hw = R._dims(x, nhwc)
    kw = dict(alpha=alpha) if p is None else dict(pmap=p)
    want = R.blend(x, nhwc, cm, cs, sm[:style_n], ss[:style_n], **kw)
    want64, parts = R.blend(x, nhwc, cm, cs, sm[:style_n], ss[:style_n], dtype=np.float64, parts=True, **kw)
    assert (np.abs(want.astype(np.float64) - want64).reshape(-1) <= R.self_distance_bound(parts)).all(), f"{what}: the inputs cancel"
    got = run_blend(rt, nhwc, x, cm, cs, sm, ss, style_n, alpha=alpha, p=p)
    assert_equal_elements(what, got, want, nhwc, n, c, hw)
    return got


@pytest.mark.parametrize("pmap", ["alpha", "pmap1", "pmapn"])
@pytest.mark.parametrize("style", ["style1", "stylen"])
@pytest.mark.parametrize("nhwc,n,c,hw", SHAPES, ids=[f"{'nhwc' if s[0] else 'nchw'}-{s[1]}x{s[2]}x{s[3]}" for s in SHAPES])
def test_blend_matrix(rt, nhwc, n, c, hw, style, pmap):
    style_n = 1 if style == "style1" else n
    pmap_n = {"alpha": 0, "pmap1": 1, "pmapn": n}[pmap]
    x, cm, cs, sm, ss, p = blend_inputs(nhwc, n, c, hw, style_n, pmap_n)
    what = f"{'NHWC' if nhwc else 'NCHW'} ({n}, {c}, {hw}) style_n {style_n} pmap_n {pmap_n}"
    check_blend(rt, what, nhwc, x, cm, cs, sm, ss, style_n, alpha=0.7 if p is None else None, p=p)


@pytest.mark.parametrize("alpha", [1.0, 0.0])
@pytest.mark.parametrize("nhwc,n,c,hw", [(False, 4, 3, 5), (False, 2, 64, 99), (True, 3, 12, 5)])
def test_alpha_one_and_zero(rt, nhwc, n, c, hw, alpha):
    """alpha = 1 is plain adaptive_instance_normalization (t * 1 + x * 0), alpha = 0 the content (t * 0 + x * 1): both through
    the same float32 sequence, nothing special-cased."""
    x, cm, cs, sm, ss, _ = blend_inputs(nhwc, n, c, hw, 1, 0, seed=1)
    got = check_blend(rt, f"alpha {alpha} ({n}, {c}, {hw})", nhwc, x, cm, cs, sm, ss, 1, alpha=alpha)
    if alpha == 0.0:
        assert np.array_equal(got, x)


# ---- dead and constant channels -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nhwc", [False, True])
@pytest.mark.parametrize("hw", [37, 4096])
def test_dead_and_constant_channels(rt, nhwc, hw):
    """Channel 1 all zeros, channel 2 all 3.0: sum and sum of squares are exact in float64 (3 hw and 9 hw, hw <= 4096), so
    var = 0 and std = sqrtf(0 + eps) exactly; blended with those statistics x - mc = 0 and the channel is ms * w1 + x * w2."""
    n, c = 2, 8
    x, cm, cs, sm, ss, p = blend_inputs(nhwc, n, c, hw, 1, n, seed=2)
    ch_axis = 3 if nhwc else 1
    idx = lambda k: tuple(slice(None) if a != ch_axis else k for a in range(4))
    x[idx(1)], x[idx(2)] = 0.0, 3.0
    mean, std = (host(t) for t in rt.mean_std(dev(x), nhwc, 1e-5))
    flat_std = np.sqrt(F32(0.0) + F32(1e-5), dtype=F32)
    assert std.dtype == F32 and (std[:, 1] == flat_std).all() and (std[:, 2] == flat_std).all()
    assert (mean[:, 1] == 0.0).all() and (mean[:, 2] == 3.0).all()
    for kw in (dict(alpha=0.7), dict(p=p)):
        got = check_blend(rt, f"dead / constant hw {hw} {sorted(kw)}", nhwc, x, mean, std, sm, ss, 1, **kw)
        img, ch, pix = (a.reshape(x.shape) for a in R.indices(n, c, hw, nhwc))
        w2 = p[img, pix] if "p" in kw else np.full(x.shape, F32(1 - 0.7), dtype=F32)
        w1 = F32(1.0) - w2 if "p" in kw else np.full(x.shape, F32(0.7), dtype=F32)
        a, b = sm[0][ch] * w1, x * w2
        want = a + b
        for k in (1, 2):
            assert np.array_equal(got[idx(k)], want[idx(k)]), k


# ---- rejections -------------------------------------------------------------------------------------------------------------------------
FILL = 123.0


def _blend_call(rt, nhwc, n, c, hw, style_n, pmap_n):
    L = rt.lib()
    f = lambda *s: torch.ones(*s, device=DEV)
    x, cm, cs, sm, ss = f(n * c * hw), f(n, c), f(n, c), f(max(style_n, 1), c), f(max(style_n, 1), c)
    out = torch.full((n * c * hw,), FILL, device=DEV)
    keep = (x, cm, cs, sm, ss)
    if pmap_n is None:
        return out, keep, lambda: L.adain_blend_alpha(x.data_ptr(), int(nhwc), n, c, hw, cm.data_ptr(), cs.data_ptr(), sm.data_ptr(), ss.data_ptr(),
                                                      style_n, 0.7, float(1 - 0.7), out.data_ptr(), rt._stream())
    p = f(max(pmap_n, 1), hw)
    return out, keep + (p,), lambda: L.adain_blend_pmap(x.data_ptr(), int(nhwc), n, c, hw, cm.data_ptr(), cs.data_ptr(), sm.data_ptr(), ss.data_ptr(),
                                                        style_n, p.data_ptr(), pmap_n, out.data_ptr(), rt._stream())


@pytest.mark.parametrize("nhwc,n,c,hw,style_n,pmap_n", [
    (False, 1, 3, 5, 1, None),          # NCHW: 15 elements
    (False, 3, 3, 5, 1, 1),             # NCHW: 45 elements
    (True, 2, 6, 4, 1, None),           # NHWC: c = 6 (the element count, 48, is a multiple of 4)
    (True, 4, 2, 2, 4, 4),
    (False, 4, 3, 5, 2, None),          # style batch 2 of 4
    (True, 4, 8, 5, 3, 1),
    (False, 4, 3, 5, 0, None),
    (False, 4, 3, 5, 1, 2),             # pmap batch 2 of 4
    (True, 4, 8, 5, 4, 3),
    (False, 4, 3, 5, 4, 0),
], ids=lambda v: str(v))
def test_blend_rejections_leave_the_output_alone(rt, nhwc, n, c, hw, style_n, pmap_n):
    out, _keep, call = _blend_call(rt, nhwc, n, c, hw, style_n, pmap_n)
    with pytest.raises(rt.AdainHipError):
        rt._check(call(), "adain_blend")
    torch.cuda.synchronize()
    assert (out == FILL).all()


def test_the_accepted_neighbours_of_the_rejections_run(rt):
    """The same calls one step inside the rules return 0 and write the output: the rejections above are the rules', not the harness's."""
    for args in [(False, 4, 3, 5, 1, None), (False, 4, 3, 5, 4, 4), (True, 4, 8, 5, 1, 1), (True, 2, 4, 4, 2, None)]:
        out, _keep, call = _blend_call(rt, *args)
        rt._check(call(), "adain_blend")
        torch.cuda.synchronize()
        assert not (out == FILL).any(), args


def test_mean_std_rejects_1028_channels(rt):
    L = rt.lib()
    n, c, hw = 1, 1028, 3
    x = torch.ones(n * hw * c, device=DEV)
    mean, std = torch.full((n, c), FILL, device=DEV), torch.full((n, c), FILL, device=DEV)
    assert L.adain_mean_std_workspace_bytes(1, n, c, hw) == 0
    nbytes = L.adain_mean_std_workspace_bytes(1, n, 1024, hw)
    ws = torch.full((nbytes,), 0x5A, dtype=torch.uint8, device=DEV)
    with pytest.raises(rt.AdainHipError):
        rt._check(L.adain_mean_std(x.data_ptr(), 1, n, c, hw, 1e-5, mean.data_ptr(), std.data_ptr(), ws.data_ptr(), nbytes, rt._stream()), "adain_mean_std")
    with pytest.raises(rt.AdainHipError):
        rt.mean_std(x.view(n, 1, hw, c), True)
    torch.cuda.synchronize()
    assert (mean == FILL).all() and (std == FILL).all() and (ws == 0x5A).all()
    m, s = rt.mean_std(x.view(n, 1, hw, c)[..., :1024].contiguous(), True)          # 1024 channels are served
    assert (host(m) == 1.0).all() and (host(s) == np.sqrt(F32(1e-5), dtype=F32)).all()


# ---- Python surface ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape,style_shape", [((4, 3, 1, 5), (4, 3, 2, 3)), ((2, 3, 2, 3), (2, 3, 1, 5))])
def test_python_surface_on_straddling_nchw(rt, shape, style_shape):
    """AdaIN.function on NCHW tensors whose planes put quads across images; the style has a row per image, which is where the
    kernel before its fix was right by accident (img * c + c == (img + 1) * c + 0).  Bound: module docstring."""
    from applied_image_processing_amd.AdaIN import function as fn
    from oracle import adain_oracle as O

    rng = np.random.default_rng(7)
    n, c = shape[:2]
    offs = (3.0 * np.arange(n)[:, None] + np.arange(c)[None, :])[:, :, None, None]
    x = (offs + rng.standard_normal(shape)).astype(F32)
    s = (-offs + 2.0 * rng.standard_normal(style_shape)).astype(F32)
    X, S = torch.from_numpy(x), torch.from_numpy(s)
    rcm, rcs = (a.numpy().reshape(n, c) for a in O.calc_mean_std(X.double()))
    rsm, rss = (a.numpy().reshape(n, c) for a in O.calc_mean_std(S.double()))
    assert rcs.min() > 0.1 and rss.min() > 0.1
    for feat, rm, rs in ((X, rcm, rcs), (S, rsm, rss)):
        m, sd = fn.calc_mean_std(feat.to(DEV))
        assert tuple(m.shape) == tuple(sd.shape) == (n, c, 1, 1)
        m, sd = host(m).reshape(n, c), host(sd).reshape(n, c)
        assert (np.abs(m - rm) <= np.spacing(np.abs(rm.astype(F32)))).all()
        assert (np.abs(sd - rs) <= 2 * np.spacing(rs.astype(F32))).all()
    got = host(fn.adaptive_instance_normalization(X.to(DEV), S.to(DEV)))
    want = O.adaptive_instance_normalization(X.double(), S.double()).numpy()
    bound = 16 * 2.0 ** -24 * ((np.abs(x) + np.abs(rcm)[:, :, None, None]) / rcs[:, :, None, None] * rss[:, :, None, None] + np.abs(rsm)[:, :, None, None])
    err = np.abs(got - want)
    print(f"{shape}: largest error / bound {float((err / bound).max()):.3f}")
    assert got.shape == want.shape and (err <= bound).all()
    # and, from the statistics the kernels themselves returned, the float32 sequence exactly
    cm, cs = (host(a).reshape(n, c) for a in fn.calc_mean_std(X.to(DEV)))
    sm, ss = (host(a).reshape(n, c) for a in fn.calc_mean_std(S.to(DEV)))
    assert_equal_elements(f"adaptive_instance_normalization {shape}", got, R.blend(x, False, cm, cs, sm, ss, alpha=1.0), False, n, c, shape[2] * shape[3])


# ---- statistics ---------------------------------------------------------------------------------------------------------------------------
def nhwc_hws(c):
    """hw = 1, 2, 3; around the first block boundary rows * 16; 74 blocks (the finalize wave strides twice); past the cap of 256."""
    g = 256 // (c // 4) * 16
    return [1, 2, 3, g - 1, g, g + 1, 73 * g + 1, 268 * g + 37]


NHWC_STATS = sorted({(c, hw) for c in (4, 12, 36, 64, 520, 1024) for hw in nhwc_hws(c)})
NCHW_STATS = [(c, hw) for c in (1, 3, 5) for hw in (1, 2, 63, 64, 65, 255, 256, 257, 1000)]


def stats_input(nhwc, n, c, hw):
    """x = offset[img, ch] + scale[ch] * (+-1 alternating over the pixels + 0.25 * noise): offsets 5 img + ch % 11 - 3 (distinct per
    image), scales 0.5 .. 2; the alternating term keeps the spread of two and three pixels away from zero."""
    rng = np.random.default_rng([c, hw, int(nhwc)])
    offset = (5.0 * np.arange(n)[:, None] + np.arange(c)[None, :] % 11 - 3.0).astype(F32)
    scale = (0.5 + 0.25 * (np.arange(c) % 7)).astype(F32)
    det = (1.0 - 2.0 * (np.arange(hw) % 2)).astype(F32)
    if nhwc:
        x = rng.standard_normal((n, 1, hw, c), dtype=F32)
        x *= F32(0.25)
        x += det[None, None, :, None]
        x *= scale[None, None, None, :]
        x += offset[:, None, None, :]
    else:
        x = rng.standard_normal((n, c, 1, hw), dtype=F32)
        x *= F32(0.25)
        x += det[None, None, None, :]
        x *= scale[None, :, None, None]
        x += offset[:, :, None, None]
    return x


def check_stats(rt, nhwc, c, hw):
    n = 3
    x = stats_input(nhwc, n, c, hw)
    ref = R.mean_std_f64(x, nhwc, EPS)
    xd = dev(x)
    mean_t, std_t = rt.mean_std(xd, nhwc, 1e-5)
    mean2_t, std2_t = rt.mean_std(xd, nhwc, 1e-5)
    assert torch.equal(mean_t.view(torch.int32), mean2_t.view(torch.int32)) and torch.equal(std_t.view(torch.int32), std2_t.view(torch.int32))
    mean, std = host(mean_t), host(std_t)
    assert mean.shape == std.shape == (n, c) and mean.dtype == std.dtype == F32
    em = np.abs(mean - ref["mean64"]) / np.spacing(np.abs(ref["mean32"]))
    if hw == 1:
        print(f"{'NHWC' if nhwc else 'NCHW'} c {c} hw 1: mean error {float(em.max()):.3f} ulp, std NaN")
        assert np.isnan(std).all() and np.isfinite(mean).all()
        assert np.array_equal(mean, x.reshape(n, c))
        return
    assert float((np.abs(ref["mean64"]) / ref["std64"]).max()) <= 1e3          # the regime the bounds are derived for
    es = np.abs(std - ref["std64"]) / np.spacing(ref["std32"])
    print(f"{'NHWC' if nhwc else 'NCHW'} c {c} hw {hw}: mean error {float(em.max()):.3f} ulp, std error {float(es.max()):.3f} ulp")
    assert (em <= 1.0).all(), f"mean off by {float(em.max())} ulp at {np.unravel_index(em.argmax(), em.shape)}"
    assert (es <= 2.0).all(), f"std off by {float(es.max())} ulp at {np.unravel_index(es.argmax(), es.shape)}"


@pytest.mark.parametrize("c,hw", NHWC_STATS)
def test_mean_std_nhwc(rt, c, hw):
    check_stats(rt, True, c, hw)


@pytest.mark.parametrize("c,hw", NCHW_STATS)
def test_mean_std_nchw(rt, c, hw):
    check_stats(rt, False, c, hw)
