"""Pins tests/conv_exact.py (the yardstick of tests/test_gpu_conv_exact.py) on the CPU: on its integer layers the Winograd algebra of
csrc/conv_wino4.hip restated in numpy with EVERY operation in float32 equals the float64 convolution exactly, for the F(4,3) x F(2,3)
form and for the polyphase F(5,2) x F(3,2) form; every entry of ``CASES`` keeps its partial sums under 2^24 and its measured
output-transform sums under 2^22; and with weights that are not multiples of 48 the same float32 restatement is NOT exact - the
multiple-of-48 rule is what buys exactness, and the comparison can fail."""
import numpy as np
import pytest
import torch

import conv_exact as X


def _ref(x, w, b, up):
    return X.preactivation(x, w, b, up)[0].numpy()


def _restated(fn, x, w, b):
    """The algebra in float32 on image 0 of an NHWC layer, bias added in float32: [cout][H][W]."""
    y = fn(x[0].permute(2, 0, 1).numpy(), w.numpy(), np.float32) + b.numpy()[:, None, None]
    assert y.dtype == np.float32
    return y


FORMS = {"f43": (X.wino_f43, False), "poly": (X.polyphase, True)}
MAPS = [("f43", 7, 9), ("f43", 2, 2), ("poly", 5, 4), ("poly", 1, 1)]          # ragged tiles in both forms, and the smallest maps


@pytest.mark.parametrize("form,hs,ws", MAPS)
@pytest.mark.parametrize("cin,cout,xmax,wmax", [(16, 32, 3, 2), (128, 32, 3, 2), (512, 32, 1, 1)])
def test_float32_algebra_is_exact_on_integer_layers(form, hs, ws, cin, cout, xmax, wmax):
    fn, up = FORMS[form]
    x, w, b = X.int_layer(hs * 100 + ws + cin, cin, cout, 1, hs, ws, xmax, wmax)
    U = X.pack_poly(w.numpy()) if up else X.pack_f43(w.numpy())
    assert np.array_equal(U, np.rint(U)) and np.array_equal(U.astype(np.float32), U), "U is an integer that float32 holds"
    got, want = _restated(fn, x, w, b), _ref(x, w, b, up)
    assert got.shape == want.shape
    assert np.array_equal(got, want), np.argwhere(got != want)[:8]


@pytest.mark.parametrize("form,hs,ws", [m for m in MAPS if m[1] > 2])
def test_weights_off_the_multiples_of_48_are_not_exact(form, hs, ws):
    """Control: plain integers in [-2, 2] as weights.  1/6, 1/12 and 1/24 then leave U off the float32 grid, and the restatement that
    is exact above must differ from the float64 convolution somewhere."""
    fn, up = FORMS[form]
    x, w, b = X.int_layer(7, 64, 32, 1, hs, ws, 3, 2, unit=1)
    assert float(w.abs().max()) == 2 and float((w % 48).abs().max()) > 0
    got, want = _restated(fn, x, w, b), _ref(x, w, b, up)
    assert not np.array_equal(got, want)
    assert np.abs(got - want).max() <= 1e-3 * np.abs(want).max()          # rounding, not another convolution


def test_reference_and_mismatch_report():
    x, w, b = X.int_layer(3, 16, 32, 2, 5, 7, 3, 2)
    pre = X.preactivation(x, w, b, False)
    assert pre.shape == (2, 32, 5, 7) and pre.dtype == torch.float64
    full, pooled = X.finish(pre, True, False), X.finish(pre, True, True)
    assert full.shape == (2, 5, 7, 32) and pooled.shape == (2, 3, 4, 32) and float(full.min()) == 0
    assert torch.equal(pooled[:, 2, 3], full[:, 4, 6])                      # ceil mode: the last window is one pixel
    xu = x.repeat_interleave(2, 1).repeat_interleave(2, 2)                  # nearest 2x upsample, by hand
    assert torch.equal(X.reference(x, w, b, up=True), X.reference(xu, w, b)) and xu.shape == (2, 10, 14, 16)
    other = full.clone()
    other[1, 4, 6, 31] += 1
    other[0, 0, 0, 0] -= 2
    count, first = X.first_mismatches(other, full, k=1)
    assert count == 2 and first == [(0, 0, 0, 0, float(full[0, 0, 0, 0]) - 2, float(full[0, 0, 0, 0]))]
    assert X.first_mismatches(full, full) == (0, [])
    with pytest.raises(AssertionError):
        X.finish(pre + 0.5 ** 30, False, False)                             # not representable in float32: the helper says so


def test_case_table_covers_what_it_is_meant_to():
    ids = [c.id for c in X.CASES]
    assert len(set(ids)) == len(ids)
    one = X.cases("one")
    assert {c.cin for c in one} >= {16, 32, 48, 64, 80, 112, 256, 512} and {c.cout for c in one} >= {32, 96, 160, 512}
    assert {c.n for c in one} == {1, 3}
    for up in (False, True):                 # every stage count meets both geometries, below and above one tile
        for cin in (16, 32, 48, 64, 80, 112):
            assert {X.geometry(c) for c in one if c.cin == cin and c.up == up} == {0, 1}, (up, cin)
    for c in X.CASES:
        assert c.geo is None or X.geometry(c) == c.geo, c.id
        assert c.cin % 16 == 0 and c.cout % 32 == 0
    # the persistent cases are persistent on the 256 compute units of an MI355X, every other launch is a one-tile one
    assert all(X.is_persistent(c, 256) == (c.kind == "persist") for c in X.CASES if c.entry != "poly"), \
        [c.id for c in X.CASES if c.entry != "poly" and X.is_persistent(c, 256) != (c.kind == "persist")]
    assert sorted(X.SPLIT_FACTORS.values()) == [2, 4, 8] and set(X.SPLIT_FACTORS) == {c.id for c in X.cases("split")}


@pytest.mark.parametrize("case", X.CASES, ids=lambda c: c.id)
def test_headroom_of_every_case(case):
    """A condition, not a measurement: (a) every partial sum stays below 2^24, (b) the measured output-transform sums at most 2^22."""
    for form, (a, b) in X.headroom(case).items():
        print(f"{case.id} {form}: cin x max|U| x max|V| = {a:.0f}, measured sum |A||M||A| = {b:.0f}")
        assert a < X.CAP, (form, a)
        assert b <= X.CAP_MEASURED, (form, b)
        assert b > 0
