"""Pins tests/blend_ref.py (the yardstick of the statistics and blend kernels) to oracle/adain_oracle.py on the AdaIN arrays of
tests/golden/case_a.npz and case_c.npz.  CPU only.

The float32 form runs the oracle's operations in the oracle's order on the same CPU, one rounding each, so it is held to
``torch.equal`` with the oracle; against the stored ``adain`` array (the reference's own output, made on another machine) it is held
to the tolerance tests/test_oracle_golden.py applies to that array.  ``mean_std_f64`` against ``O.calc_mean_std(x.double())``: both
are float64, torch's variance is a Welford pass and this one two passes, each a few hundred additions at 1.1e-16 relative - 1e-12
relative leaves three orders of room and is six below anything a float32 result can show."""
import numpy as np
import pytest
import torch

import blend_ref as R
from conftest import golden
from oracle import adain_oracle as O
from test_oracle_golden import ATOL, RTOL


def T(a):
    return torch.from_numpy(np.ascontiguousarray(a))


def nhwc(a):
    return np.ascontiguousarray(np.transpose(a, (0, 2, 3, 1)))


def nchw(a):
    return np.transpose(a, (0, 3, 1, 2))


def pmaps(n, h, w, seed):
    rng = np.random.default_rng(seed)
    return (0.85 * rng.random((n, 1, h, w))).astype(np.float32)


def stats(feat):
    m, s = O.calc_mean_std(T(feat))
    n, c = feat.shape[:2]
    return m.numpy().reshape(n, c), s.numpy().reshape(n, c)


def both_layouts(x, *a, **k):
    """The float32 form on NCHW and on NHWC memory: the same values element for element."""
    out = R.blend(x, False, *a, **k)
    assert out.dtype == np.float32 and out.shape == x.shape
    assert np.array_equal(nchw(R.blend(nhwc(x), True, *a, **k)), out)
    return T(out)


def test_case_a_adain_and_blends_equal_the_oracle():
    g = golden("case_a.npz")
    cf, sf = g["content_f"], g["style_f"]
    cm, cs = stats(cf)
    sm, ss = stats(sf)
    with torch.no_grad():
        t = O.adaptive_instance_normalization(T(cf), T(sf))
        assert torch.equal(both_layouts(cf, cm, cs, sm, ss, alpha=1.0), t)                      # t * 1 + x * 0
        np.testing.assert_allclose(R.blend(cf, False, cm, cs, sm, ss, alpha=1.0), g["adain"], rtol=RTOL, atol=ATOL)
        for alpha in (0.5, 0.7, 0.0):
            assert torch.equal(both_layouts(cf, cm, cs, sm, ss, alpha=alpha), t * alpha + T(cf) * (1 - alpha)), alpha      # test.py:80
        p = pmaps(1, *cf.shape[2:], seed=1)
        assert torch.equal(both_layouts(cf, cm, cs, sm, ss, pmap=p), t * (1 - T(p)) + T(cf) * T(p))                     # test.py:70


@pytest.mark.parametrize("style_n", [1, 2])
def test_case_c_batch_of_two(style_n):
    g = golden("case_c.npz")
    cf = g["content_f"]
    n, c, h, w = cf.shape
    assert n == 2
    sm, ss = g["style_mean"].reshape(n, c)[:style_n], g["style_std"].reshape(n, c)[:style_n]
    cm, cs = stats(cf)
    with torch.no_grad():
        # function.py:21-23 on the stored style statistics (the style features themselves are not stored)
        t = (T(cf) - T(cm).view(n, c, 1, 1)) / T(cs).view(n, c, 1, 1) * T(ss).view(style_n, c, 1, 1) + T(sm).view(style_n, c, 1, 1)
        assert torch.equal(both_layouts(cf, cm, cs, sm, ss, alpha=1.0), t)
        assert torch.equal(both_layouts(cf, cm, cs, sm, ss, alpha=0.7), t * 0.7 + T(cf) * (1 - 0.7))
        for pn in (1, 2):
            p = pmaps(pn, h, w, seed=2)
            assert torch.equal(both_layouts(cf, cm, cs, sm, ss, pmap=p), t * (1 - T(p)) + T(cf) * T(p))


def test_float64_form_is_the_same_expression():
    g = golden("case_c.npz")
    cf = g["content_f"]
    n, c = cf.shape[:2]
    cm, cs = stats(cf)
    sm, ss = g["style_mean"].reshape(n, c), g["style_std"].reshape(n, c)
    for kw in (dict(alpha=0.7), dict(pmap=pmaps(2, *cf.shape[2:], seed=3))):
        out64, parts = R.blend(cf, False, cm, cs, sm, ss, dtype=np.float64, parts=True, **kw)
        assert out64.dtype == np.float64
        d = lambda a: T(a).double()
        t = (d(cf) - d(cm).view(n, c, 1, 1)) / d(cs).view(n, c, 1, 1) * d(ss).view(n, c, 1, 1) + d(sm).view(n, c, 1, 1)
        w2 = d(kw["pmap"]) if "pmap" in kw else float(np.float32(1 - 0.7))
        w1 = 1 - d(kw["pmap"]) if "pmap" in kw else float(np.float32(0.7))
        assert torch.equal(T(out64), t * w1 + d(cf) * w2)
        out32 = R.blend(cf, False, cm, cs, sm, ss, **kw)
        assert (np.abs(out32.astype(np.float64) - out64).reshape(-1) <= R.self_distance_bound(parts)).all()


@pytest.mark.parametrize("case,key", [("case_a.npz", "content_f"), ("case_a.npz", "style_f"), ("case_c.npz", "content_f")])
def test_mean_std_f64_agrees_with_the_oracle_in_double(case, key):
    x = golden(case)[key]
    n, c = x.shape[:2]
    rm, rs = O.calc_mean_std(T(x).double())
    for layout, v in ((False, x), (True, nhwc(x))):
        r = R.mean_std_f64(v, layout)
        assert r["mean64"].dtype == r["std64"].dtype == np.float64 and r["mean32"].dtype == r["std32"].dtype == np.float32
        np.testing.assert_allclose(r["mean64"], rm.numpy().reshape(n, c), rtol=1e-12, atol=1e-15)
        np.testing.assert_allclose(r["std64"], rs.numpy().reshape(n, c), rtol=1e-12, atol=0)
        assert np.array_equal(r["mean32"], r["mean64"].astype(np.float32)) and np.array_equal(r["std32"], r["std64"].astype(np.float32))
    if case == "case_a.npz" and key == "content_f":          # the stored float32 statistics of the reference itself
        g = golden(case)
        np.testing.assert_allclose(r["mean32"], g["mean"].reshape(n, c), rtol=RTOL, atol=ATOL)
        np.testing.assert_allclose(r["std32"], g["std"].reshape(n, c), rtol=RTOL, atol=ATOL)


def test_one_pixel_gives_a_nan_std_and_the_pixel_as_mean():
    x = np.arange(24, dtype=np.float32).reshape(2, 3, 1, 4)[:, :, :, :1].copy()
    for layout, v in ((False, x), (True, nhwc(x))):
        r = R.mean_std_f64(v, layout)
        assert np.isnan(r["std64"]).all() and np.isnan(r["std32"]).all()
        assert np.array_equal(r["mean32"], x.reshape(2, 3))
    rm, rs = O.calc_mean_std(T(x).double())
    assert torch.isnan(rs).all()


def test_indices_cover_every_element_once():
    for layout in (False, True):
        n, c, hw = 3, 5, 7
        img, ch, pix = R.indices(n, c, hw, layout)
        a = np.zeros((n, hw, c) if layout else (n, c, hw), dtype=np.int64)
        np.add.at(a, (img, pix, ch) if layout else (img, ch, pix), 1)
        assert (a == 1).all()
        flat = (img * hw + pix) * c + ch if layout else (img * c + ch) * hw + pix
        assert np.array_equal(flat, np.arange(n * c * hw))
