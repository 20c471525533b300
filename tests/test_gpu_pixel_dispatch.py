"""GPU tests of csrc/pixel.hip on every branch its launchers take, element for element, against tests/pixel_ref.py (pinned on the
host by test_pixel_ref_host.py) and, for the video kernels, against the oracle's bit-for-bit restatements.  Run with ``-m gpu``.

Every ``launch_*`` of pixel.hip picks a kernel from facts the caller does not see: sizes modulo 4 and 8, equal widths, the channel
count, and above all pointer alignment.  pixel_ref.DISPATCH has one row per branch; the case lists below are data, the row each
case takes is computed from the case's own sizes and pointer offsets by pixel_ref.select_*, and the module asserts at import that
every row but pixel_ref.NOT_RUN (resize_area_u8_kernel<0>: more than a million output rows) is taken.

Misaligned inputs are contiguous views into a larger tensor, 4 bytes (float32) or 1 to 3 bytes (uint8) past a 256-byte aligned
address; misaligned outputs go through the wrappers' ``out=`` or, where a wrapper has none, through ``rt.call`` with a raw pointer.
Every output written that way sits between two 256-byte guards filled with 0xA5 that are compared after the call.

Equality is np.array_equal over the whole output (NaN equal to NaN), a failure prints the first mismatching coordinates.  The one
measured bar is the strength map's (device expf, and a mean summed in another order than the host's): per case
pixel_ref.STRENGTH_SELF_ULP, the float32 restatement's own worst distance from the float64 form (17 to 279 float32 ulp of the
result), plus STRENGTH_MARGIN_ULP = 3.  Measured on an MI355X: the device's worst distance per case is the restatement's own to two
decimals (131.58, 16.99, 247.64, 29.76, 74.64, 112.41, 278.75, 107.36, 75.66, 150.41, 30.73, 158.67 ulp: the same element is worst);
0 to 10 % of the elements differ from the float32 restatement, none by more than STRENGTH_EXCESS_ULP = 2.00 ulp further from the
float64 form than the restatement is at the same element (0.00 on the one-row and one-column sources, where every element is
bitwise the restatement's); the margin is 1.5 times that excess, a whole ulp.  The whole file takes under 3 s on an MI355X."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import applied_image_processing_amd.synth as synth
import pixel_ref as R
from oracle import adain_oracle as O

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
F32, F64 = np.float32, np.float64
GUARD = 256
STRENGTH_EXCESS_ULP = 2.0           # measured: the most any element's distance exceeds the float32 restatement's at the same element
STRENGTH_MARGIN_ULP = 3             # 1.5 x 2.0, a whole ulp
TAKEN = set()                       # dispatch rows the case lists below take


def T(a):
    return torch.from_numpy(np.ascontiguousarray(a))


@pytest.fixture(scope="module")
def rt():
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    import applied_image_processing_amd.runtime as rt

    rt.lib()
    torch.cuda.set_device(0)
    return rt


@pytest.fixture(scope="module")
def engine(weights):
    from applied_image_processing_amd.engine import AdaINEngine

    eng = AdaINEngine(weights[0], weights[1], DEV)
    eng.set_style(T(synth.image(4, 1, 96, 128)).cuda())
    return eng


def host(t):
    torch.cuda.synchronize()
    return t.cpu().numpy()


def dev(a, off=0):
    """``a`` on the device as a contiguous tensor whose first byte is ``off`` bytes past a 256-byte aligned address."""
    a = np.ascontiguousarray(a)
    t = T(a.view(np.uint8) if a.dtype == np.bool_ else a)
    item = t.element_size()
    assert off % item == 0
    big = torch.empty(t.numel() + 256 // item, dtype=t.dtype, device=DEV)
    assert big.data_ptr() % 256 == 0
    v = big[off // item: off // item + t.numel()].view(t.shape)
    v.copy_(t)
    assert v.is_contiguous() and v.data_ptr() % 256 == off
    return v.view(torch.bool) if a.dtype == np.bool_ else v


class Guarded:
    """An output of ``shape`` / ``dtype`` that starts ``off`` bytes past a 256-byte aligned address, between two guards of 0xA5."""

    def __init__(self, shape, dtype, off=0):
        self.nbytes = int(np.prod(shape)) * torch.empty((), dtype=dtype).element_size()
        self.buf = torch.full((2 * GUARD + self.nbytes + 16,), 0xA5, dtype=torch.uint8, device=DEV)
        assert self.buf.data_ptr() % 256 == 0
        self.start = GUARD + off
        self.out = self.buf[self.start: self.start + self.nbytes].view(dtype).view(shape)
        assert self.out.data_ptr() % 256 == off and self.out.is_contiguous()

    def ptr(self):
        return self.out.data_ptr()

    def result(self):
        """The output on the host, after the guards have been compared."""
        torch.cuda.synchronize()
        b = self.buf.cpu().numpy()
        assert (b[: self.start] == 0xA5).all() and (b[self.start + self.nbytes:] == 0xA5).all(), "a byte outside the output was written"
        return self.out.cpu().numpy()


def same(what, got, want):
    got, want = R._np(got), R._np(want)
    assert got.shape == want.shape and got.dtype == want.dtype, (what, got.shape, want.shape, got.dtype, want.dtype)
    assert np.array_equal(got, want, equal_nan=got.dtype.kind == "f"), R.mismatch_message(what, got, want)


# ---- resize ---------------------------------------------------------------------------------------------------------------------------------
# (planes, hi, wi, ho, wo, in_off, out_off)
RESIZE_GRID = [(p, 4, 100, ho, wo, 0, 0) for wo in (1, 3, 4, 5, 255, 256, 257, 260) for ho in (1, 3, 4, 5) for p in (1, 3)]
RESIZE_THIN = [(3, 1, 100, 5, 260, 0, 0), (3, 1, 100, 1, 37, 0, 0), (3, 70, 1, 5, 4, 0, 0), (3, 70, 1, 130, 1, 0, 0), (1, 1, 1, 3, 8, 0, 0),
               (3, 9, 40, 4, 64, 0, 0), (3, 9, 40, 20, 24, 0, 0), (3, 4, 100, 3, 256, 4, 0), (3, 4, 100, 3, 256, 0, 4), (3, 4, 100, 3, 256, 4, 4)]
SAMEW_SHAPES = [(3, hi, w, ho, w) for w in (4, 256, 260) for hi, ho in ((5, 5), (5, 9), (9, 4))]
SAMEW_ODD = [(3, 5, 257, 5, 257, 0, 0), (3, 5, 257, 9, 257, 0, 0), (1, 9, 3, 4, 3, 0, 0)]
RESIZE_CASES = RESIZE_GRID + RESIZE_THIN + SAMEW_ODD + [s + (i, o) for s in SAMEW_SHAPES for i, o in ((0, 0), (4, 0), (0, 4))]
NONFINITE = [(0, 0), (4, 0)]          # (in_off, out_off) of the Inf / NaN plane: the same-width form and the generic one
for _c in RESIZE_CASES:
    TAKEN |= {R.select_resize_bilinear(_c[2], _c[4], _c[5], _c[6]), R.select_resize_nearest(_c[2], _c[4], _c[5], _c[6])}
assert {R.select_resize_bilinear(12, 12, i, o) for i, o in NONFINITE} == {"resize_bilinear/samew", "resize_bilinear/samew_in_off"}


def run_resize(rt, name, x, ho, wo, in_off, out_off):
    n, c, hi, wi = x.shape
    g = Guarded((n, c, ho, wo), torch.float32, out_off)
    xd = dev(x, in_off)
    rt.call(name, xd.device, xd.data_ptr(), g.ptr(), n * c, hi, wi, ho, wo)
    return g.result()


@pytest.mark.parametrize("group", ["grid", "thin", "samew_odd"])
def test_resize_equals_the_restatement(rt, group):
    for planes, hi, wi, ho, wo, i, o in {"grid": RESIZE_GRID, "thin": RESIZE_THIN, "samew_odd": SAMEW_ODD}[group]:
        x = synth.uniform_sym(100 + hi + wi, (1, planes, hi, wi), 2.0)
        what = f"{planes} x {hi} x {wi} -> {ho} x {wo}, in +{i}, out +{o}"
        same("bilinear " + what, run_resize(rt, "adain_resize_bilinear", x, ho, wo, i, o), R.resize_bilinear(x, ho, wo))
        near = run_resize(rt, "adain_resize_nearest", x, ho, wo, i, o)
        same("nearest " + what, near, R.resize_nearest(x, ho, wo))
        same("nearest vs torch " + what, near, F.interpolate(T(x), size=(ho, wo), mode="nearest").numpy())


@pytest.mark.parametrize("planes,hi,wi,ho,wo", SAMEW_SHAPES)
def test_same_width_forms_give_one_answer(rt, planes, hi, wi, ho, wo):
    """wi == wo, wo % 4 == 0: the same-width kernel (aligned), the generic vector form (input 4 bytes off) and the scalar stores
    (output 4 bytes off) are bitwise one output, the restatement's; through the wrapper too."""
    x = synth.uniform_sym(200 + hi + wi, (1, planes, hi, wi), 2.0)
    for name, ref in (("adain_resize_bilinear", R.resize_bilinear(x, ho, wo)), ("adain_resize_nearest", R.resize_nearest(x, ho, wo))):
        for i, o in ((0, 0), (4, 0), (0, 4)):
            same(f"{name} {hi} x {wi} -> {ho} x {wo}, in +{i}, out +{o}", run_resize(rt, name, x, ho, wo, i, o), ref)
    same("wrapper", host(rt.resize_bilinear(dev(x), (ho, wo))), R.resize_bilinear(x, ho, wo))
    if hi == ho:
        same("identity", run_resize(rt, "adain_resize_bilinear", x, ho, wo, 0, 0), x)


@pytest.mark.parametrize("hi,ho", [(6, 6), (6, 11), (7, 3)])
def test_non_finite_neighbours_propagate_as_in_the_restatement(rt, hi, ho):
    """+Inf in column 4 and NaN in column 9 of one plane: the zero-weight right-hand taps give NaN in columns 3 and 8 (0 * Inf, 0 * NaN),
    in the same-width kernel (column 4 is the extra element of the quad 0..3) as in the generic form."""
    x = synth.uniform_sym(300 + hi, (1, 2, hi, 12), 2.0)
    x[0, 0, :, 4], x[0, 0, :, 9] = np.inf, np.nan
    want = R.resize_bilinear(x, ho, 12)
    assert np.isnan(want[0, 0][:, [3, 8, 9]]).all() and np.isfinite(want[0, 1]).all()
    for i, o in NONFINITE:
        same(f"Inf / NaN plane {hi} -> {ho}, in +{i}", run_resize(rt, "adain_resize_bilinear", x, ho, 12, i, o), want)


# ---- mask composite ---------------------------------------------------------------------------------------------------------------------------
COMPOSITE_HW = [1, 3, 1023, 1024, 1025, 1028]
COMPOSITE_OFFS = [(0, 0, 0, 0), (4, 0, 0, 0), (0, 4, 0, 0), (0, 0, 4, 0), (0, 0, 0, 4)]          # content, stylised, mask, out
TAKEN |= {R.select_mask_composite(hw, offs) for hw in COMPOSITE_HW for offs in COMPOSITE_OFFS}


@pytest.mark.parametrize("hw", COMPOSITE_HW)
def test_mask_composite_equals_the_restatement(rt, hw):
    n = 3
    for c in (1, 3, 4):
        a, b = synth.image(400 + c, n, 1, hw, c=c), synth.uniform_sym(410 + c, (n, c, 1, hw), 1.0)
        for mc in sorted({1, c}):
            for mn in (1, n):
                m = synth.image(420 + mc + 10 * mn, mn, 1, hw, c=mc)          # fractional: another image's or channel's row cannot agree
                want = R.mask_composite(a, b, m)
                for offs in COMPOSITE_OFFS:
                    g = Guarded(a.shape, torch.float32, offs[3])
                    ad, bd, md = dev(a, offs[0]), dev(b, offs[1]), dev(m, offs[2])
                    rt.call("adain_mask_composite", ad.device, ad.data_ptr(), bd.data_ptr(), md.data_ptr(), mc, mn, g.ptr(), n, c, hw)
                    same(f"mask_composite hw {hw} c {c} mask_c {mc} mask_n {mn} offsets {offs}", g.result(), want)
                same("wrapper", host(rt.mask_composite(dev(a), dev(b), dev(m))), want)


# ---- quantiser and ToTensor -----------------------------------------------------------------------------------------------------------------------
QUANT_HW = [1, 4, 1020, 1024, 1028, 1029]
QUANT_OFFS = [(0, 0), (4, 0), (0, 1), (0, 2), (0, 3), (4, 1)]          # (float pointer, byte pointer)
TAKEN |= {R.select_quantize_u8(c, hw, f, b) for c in (1, 3, 4) for hw in QUANT_HW for f, b in QUANT_OFFS}
TAKEN |= {R.select_u8_to_f32(c, hw, b, f) for c in (1, 3, 4) for hw in QUANT_HW for f, b in QUANT_OFFS}


@pytest.mark.parametrize("hw", QUANT_HW)
def test_quantize_u8_equals_the_restatement_and_the_oracle(rt, hw):
    values = R.quantiser_edge_values()
    for c in (1, 3, 4):
        x = R.fill(values, (2, c, 1, hw), seed=c + hw)
        want = R.quantize_u8(x)
        assert torch.equal(T(want), O.quantize_u8(T(x)))
        for f_off, b_off in QUANT_OFFS:
            g = Guarded(want.shape, torch.uint8, b_off)
            assert rt.quantize_u8(dev(x, f_off), out=g.out) is g.out
            same(f"quantize_u8 c {c} hw {hw}, in +{f_off}, out +{b_off}", g.result(), want)
        same("no out", host(rt.quantize_u8(dev(x))), want)


@pytest.mark.parametrize("hw", QUANT_HW)
def test_u8_to_f32_equals_the_restatement(rt, hw):
    for c in (1, 3, 4):
        u = R.fill(np.arange(256, dtype=np.uint8), (2, 1, hw, c), seed=c)
        if hw >= 1020:
            assert all(set(u[i, ..., ch].reshape(-1).tolist()) == set(range(256)) for i in range(2) for ch in range(c))
        want = R.u8_to_f32(u)
        for f_off, b_off in QUANT_OFFS:
            g = Guarded(want.shape, torch.float32, f_off)
            ud = dev(u, b_off)
            rt.call("adain_u8_to_f32", ud.device, ud.data_ptr(), g.ptr(), 2, c, 1, hw)
            same(f"u8_to_f32 c {c} hw {hw}, in +{b_off}, out +{f_off}", g.result(), want)
        same("wrapper", host(rt.u8_to_f32(dev(u))), want)


# ---- the tails of adain_stylize_u8 ------------------------------------------------------------------------------------------------------------
TAIL_H, TAIL_W, TAIL_N = 64, 104, 2
TAIL_OFFS = [(0, 0), (1, 0), (0, 1), (1, 1)]          # (frames, out)
TAIL_MASK_SIZES = [(64, 104), (32, 52), (25, 35)]
TAKEN |= {R.select_stylize_tail(TAIL_H, TAIL_W, None, 0, 0, o) for o in (0, 1)}
TAKEN |= {R.select_stylize_tail(TAIL_H, TAIL_W, ms, f, a, b) for ms in TAIL_MASK_SIZES for f in (0, 1) for a, b in TAIL_OFFS}


@pytest.fixture(scope="module")
def tail(engine):
    """The frames, and the float image the decoder gives for them (engine.stylize): computed once, read only."""
    frames = np.stack([(synth.image(740 + i, 1, TAIL_H, TAIL_W)[0].transpose(1, 2, 0) * 255).astype(np.uint8) for i in range(TAIL_N)])
    sty = host(engine.stylize(dev(frames), 0.5))
    assert sty.shape == (TAIL_N, 3, TAIL_H, TAIL_W)
    return frames, sty


def test_unaligned_output_without_a_mask(engine, tail):
    frames, _sty = tail
    aligned = host(engine.stylize_u8(dev(frames), alpha=0.5))
    assert aligned.shape == (TAIL_N, TAIL_H, TAIL_W, 3)
    for f_off, o_off in ((0, 1), (1, 1), (1, 0), (0, 2)):
        g = Guarded(aligned.shape, torch.uint8, o_off)
        assert engine.stylize_u8(dev(frames, f_off), alpha=0.5, out=g.out) is g.out
        same(f"no mask, frames +{f_off}, out +{o_off}", g.result(), aligned)


@pytest.mark.parametrize("kind", ["u8", "bool", "f32"])
@pytest.mark.parametrize("mh,mw", TAIL_MASK_SIZES)
def test_fused_tails_equal_the_five_pass_restatement(engine, tail, mh, mw, kind):
    frames, sty = tail
    for mc in (1, 3):
        for mn in (1, TAIL_N):
            m = synth.image(760 + mc + 10 * mn + mh, mn, mh, mw, c=mc)
            m = {"u8": (m > 0.5).astype(np.uint8), "bool": m > 0.5, "f32": m}[kind]
            want = R.composite_quantize_u8(frames, sty, m, None if (mh, mw) == (TAIL_H, TAIL_W) else (mh, mw))
            changed = float((want != frames).mean())
            assert 0.2 < changed < 1.0          # the mask takes from both images
            for f_off, o_off in TAIL_OFFS:
                g = Guarded(want.shape, torch.uint8, o_off)
                engine.stylize_u8(dev(frames, f_off), alpha=0.5, masks=dev(m), out=g.out)
                same(f"mask {kind} [{mn}, {mc}, {mh}, {mw}], frames +{f_off}, out +{o_off}", g.result(), want)


# ---- strength map ---------------------------------------------------------------------------------------------------------------------------
TAKEN |= {R.select_strength_map(c[3], c[4]) for c in R.STRENGTH_CASES}


@pytest.mark.parametrize("case", R.STRENGTH_CASES, ids=[c[0] for c in R.STRENGTH_CASES])
def test_strength_map_within_the_measured_bar(rt, case):
    name, h0, w0, hc, wc, off, prom, kind = case
    d = R.strength_input(name, h0, w0, kind)
    got = host(rt.strength_map(dev(d), hc, wc, off, prom))
    assert got.shape == (1, 1, hc, wc) and got.dtype == F32
    got = got.reshape(hc, wc)
    want64, parts = R.strength_map(d, hc, wc, off, prom, dtype=F64, parts=True)
    if parts["constant"]:
        assert not got.any(), f"{name}: a constant map must give exact zeros"
        return
    dist = R.ulp_distance(got, want64)
    ref32 = R.strength_map(d, hc, wc, off, prom)
    excess = float((dist - R.ulp_distance(ref32, want64)).max())          # element by element: what expf and the cast mean add
    print(f"strength {name}: device {float(dist.max()):.2f} ulp from the float64 form, restatement {R.STRENGTH_SELF_ULP[name]}, "
          f"largest excess of an element {excess:.2f} ulp; {float((got != ref32).mean()):.4f} of the elements differ from the float32 restatement")
    bar = R.STRENGTH_SELF_ULP[name] + STRENGTH_MARGIN_ULP
    assert (dist <= bar).all(), f"{name}: {float(dist.max()):.2f} ulp at {np.unravel_index(dist.argmax(), dist.shape)}, bar {bar}"
    if name in R.CAP_CLEAR_CASES:
        cap32 = F32(1) - F32(off)
        want_set = parts["sg"] >= parts["cap"]
        assert want_set.any() and not want_set.all()
        same(f"{name}: the elements at the cap", got == cap32, want_set)
        assert (got <= cap32).all()


# ---- warp + blend ---------------------------------------------------------------------------------------------------------------------------
WARP_OFFS = [(0, 0, 0, 0), (4, 0, 0, 0), (0, 1, 0, 0), (0, 0, 1, 0), (0, 0, 0, 1)]          # flow, cur, prev, out
for _h, _w in R.WARP_FRAMES:
    TAKEN |= {R.select_warp_blend_u8(_h, _w, c) for c in (1, 3, 4)}
    if _h * _w % 4 == 0:
        TAKEN |= {R.select_warp_blend_u8(_h, _w, 3, f, c, o) for f, c, _p, o in WARP_OFFS}
assert R.select_warp_blend_u8(16, 64, 3) == R.select_warp_blend_u8(2, 6, 3) == "warp_blend_u8/rgb4" and R.select_warp_blend_u8(15, 67, 3) == "warp_blend_u8/scalar"


def run_warp(rt, cur, prev, flow, alpha, offs=(0, 0, 0, 0)):
    g = Guarded(cur.shape, torch.uint8, offs[3])
    assert rt.warp_blend_u8(dev(cur, offs[1]), dev(prev, offs[2]), dev(flow, offs[0]), alpha, out=g.out) is g.out
    return g.result()


@pytest.mark.parametrize("h,w", R.WARP_FRAMES)
def test_warp_blend_equals_the_oracle_on_every_flow(rt, h, w):
    rng = np.random.default_rng([7, h, w])
    flows = R.warp_flows(h, w)
    for c in (1, 3, 4):
        cur, prev = (rng.integers(0, 256, (h, w, c), dtype=np.uint8) for _ in range(2))
        for name, flow in flows.items():
            want = O.warp_blend_u8(cur, prev, flow, 0.7)
            same(f"warp_blend {h} x {w} x {c} flow {name}", run_warp(rt, cur, prev, flow, 0.7), want)
            if c == 3 and h * w % 4 == 0:
                for offs in WARP_OFFS[1:]:          # flow, cur and out off: the scalar kernel; prev off: still the vector kernel
                    same(f"warp_blend {h} x {w} flow {name} offsets {offs}", run_warp(rt, cur, prev, flow, 0.7, offs), want)


# ---- area resize ------------------------------------------------------------------------------------------------------------------------------
AREA_OFF_CASES = {"taps4_64x16": [(1, 0), (0, 1)], "taps4_65x17": [(1, 0)], "rgbw_tail": [(1, 0), (2, 0)], "2x2_w8": [(1, 0), (0, 1), (1, 1)],
                  "2x2_w8_wide": [(0, 1)]}          # (in, out) byte offsets
for _name, _hi, _wi, _c, _ho, _wo in R.AREA_CASES:
    TAKEN |= {R.select_resize_area_u8(_hi, _wi, _c, _ho, _wo, i, o) for i, o in [(0, 0)] + AREA_OFF_CASES.get(_name, [])}


@pytest.mark.parametrize("case", R.AREA_CASES, ids=[c[0] for c in R.AREA_CASES])
def test_resize_area_equals_the_oracle(rt, case):
    name, hi, wi, c, ho, wo = case
    n = 2
    frames = np.random.default_rng([11, hi, wi, c]).integers(0, 256, (n, hi, wi, c), dtype=np.uint8)
    want = np.stack([O.resize_area_u8(f, (wo, ho)).reshape(ho, wo, c) for f in frames])
    same(f"resize_area {name} wrapper", host(rt.resize_area_u8(dev(frames), (wo, ho))), want)
    for i, o in [(0, 0)] + AREA_OFF_CASES.get(name, []):
        g = Guarded(want.shape, torch.uint8, o)
        fd = dev(frames, i)
        rt.call("adain_resize_area_u8", fd.device, fd.data_ptr(), g.ptr(), n, hi, wi, c, ho, wo)
        same(f"resize_area {name}, in +{i}, out +{o}", g.result(), want)


# ---- transposes ---------------------------------------------------------------------------------------------------------------------------------
TAKEN |= {"transpose/nhwc_to_nchw", "transpose/nchw_to_nhwc"}


def test_transposes_equal_numpy(rt):
    sizes = (1, 31, 32, 33, 65)
    for c in sizes:
        for hw in sizes:
            x = synth.uniform_sym(900 + c + 100 * hw, (2, c, 1, hw), 1.0)
            same(f"nchw_to_nhwc c {c} hw {hw}", host(rt.nchw_to_nhwc(dev(x))), np.ascontiguousarray(np.transpose(x, (0, 2, 3, 1))))
            y = synth.uniform_sym(901 + c + 100 * hw, (2, 1, hw, c), 1.0)
            same(f"nhwc_to_nchw c {c} hw {hw}", host(rt.nhwc_to_nchw(dev(y))), np.ascontiguousarray(np.transpose(y, (0, 3, 1, 2))))


# ---- every row of the table has a case --------------------------------------------------------------------------------------------------------
assert TAKEN <= set(R.DISPATCH), sorted(TAKEN - set(R.DISPATCH))
assert set(R.DISPATCH) - TAKEN == R.NOT_RUN, f"dispatch rows without a case: {sorted(set(R.DISPATCH) - TAKEN - R.NOT_RUN)}"


def test_every_dispatch_row_but_the_named_exception_has_a_case():
    assert set(R.DISPATCH) - TAKEN == R.NOT_RUN == {"resize_area_u8/untabled"}
