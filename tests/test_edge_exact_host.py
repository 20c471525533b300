"""Pins tests/edge_exact.py (the yardsticks of tests/test_gpu_edge_layers.py) on the CPU.  First layer: every case keeps the kernel's
partial sums and the fold's own under 2^24, and a float32 numpy restatement of the fold and the K = 28 product equals the float64
reference of the unfolded sequence exactly.  Last layer: a float32 convolution of an input with the device's statistics stays inside
the gamma_577 bound at every element.  Both: each single fault of ``FAULTS`` applied to the reference breaks the assertion the GPU
test makes - equality for the first layer, the bound at one element or more for the last - so the GPU tests can fail.  And the
restated workspace plan of ``adain_decode`` matches ``arch.decoder_plan()``."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import edge_exact as E
from applied_image_processing_amd import arch

CUS = 256                                                     # an MI355X; the GPU test builds its walks for the device it runs on
FIRST = E.FIRST_CASES + [E.walk_case(CUS, "border"), E.walk_case(CUS, "mixed")]
FAULTS_FIRST = ["tap_shift", "clamp_row", "clamp_col", "seam", "quad_swap", "colour_swap", "no_bias", "conv0_T"]
FAULTS_LAST = ["tap_shift", "clamp_row", "clamp_col", "seam", "quad_swap", "colour_swap", "no_bias"]


# ---- first layer ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", FIRST, ids=lambda c: c.id)
def test_first_layer_headroom_and_float32_restatement(case):
    x = E.first_image(case)
    assert x.shape == (case.n, 3, case.H, case.W) and torch.equal(x, x.round())
    for i in range(case.n):                                   # distinct values per pixel and per plane
        assert x[i].unique().numel() == x[i].numel()
    a, b = E.first_headroom(x)
    print(f"{case.id}: 27 max|x| max|W'| + max|b'| = {a:.0f}, the fold's largest sum = {b:.0f}")
    assert a < E.CAP and b < E.CAP
    k = min(case.n, 2)                                        # (the walks: two frames stand for the batch here)
    want = E.to_float32_exact(E.first_reference(x[:k]))
    for i in range(k):
        got = E.first_restated32(x[i].numpy())
        assert np.array_equal(got, want[i].numpy()), np.argwhere(got != want[i].numpy())[:8]


def test_first_layer_weights_are_what_the_cases_need():
    w0, b0, w1, b1 = E.first_weights()
    assert not torch.equal(w0, w0.t()) and float((w0 - torch.diag(torch.diag(w0))).abs().max()) > 0          # not symmetric, not diagonal
    for t in (w0, b0, w1, b1):
        assert torch.equal(t, t.round())
    wf, bf = E.fold(w0, b0, w1, b1)
    assert float(wf[E.CH_ZERO].abs().max()) == 0 and float(bf[E.CH_ZERO]) == 0
    assert float(bf[E.CH_NEG]) < 0 and float(bf[E.CH_POS]) > 0 and float(wf[E.CH_NEG].abs().max()) == 0
    assert float(bf[E.CH_ZERO_FOLD]) == 0 and float(wf[E.CH_ZERO_FOLD].abs().max()) > 0 and float(b1[E.CH_ZERO_FOLD]) != 0
    # the fold is the unfolded sequence: same float64 answer on a seeded image
    case = next(c for c in E.FIRST_CASES if (c.H, c.W) == (9, 33) and c.kind == "map")
    x = E.first_image(case)
    ref, _mag = E.first_bounded_reference(x)
    assert torch.equal(ref, E.first_reference(x))
    # pre-activations of every sign, exact zeros included, and channels that are not constant
    pre = E.conv_ref(F.conv2d(x.double(), w0.reshape(3, 3, 1, 1), b0), w1, b1)
    assert float(pre[:, E.CH_ZERO].abs().max()) == 0 and float(pre[:, E.CH_NEG].max()) < 0 and float(pre[:, E.CH_POS].min()) > 0
    rest = pre[:, 4:]
    assert int((rest < 0).sum()) > rest.numel() // 4 and int((rest > 0).sum()) > rest.numel() // 4


def test_first_layer_cases_cover_the_tile_classes():
    maps = [c for c in E.FIRST_CASES if c.kind == "map"]
    assert {(c.H, c.W) for c in maps} >= {(2, 2), (2, 40), (40, 2), (25, 97)}
    for W in E.WIDTHS:                                        # every width class meets a full and a partial last tile row
        hs = {c.H for c in maps if c.W == W}
        assert any(h % E.FIRST_TH == 0 for h in hs) and any(h % E.FIRST_TH for h in hs), W
    kinds = [k for (_y, _x, k) in E.first_tiles(25, 97)]
    assert len(kinds) == 16 and sum(kinds) == 4              # interior tiles beside border tiles
    assert sorted(c.n for c in E.FIRST_CASES if c.kind == "batch") == [2, 3]
    # all 256 byte values in each plane of at least one case
    full = [c for c in E.FIRST_CASES if all(E.first_image_u8(c)[0, :, :, p].unique().numel() == 256 for p in range(3))]
    assert full and {(c.H, c.W) for c in full} >= {(25, 97), (16, 32)}
    assert len({c.id for c in FIRST}) == len(FIRST)


@pytest.mark.parametrize("which", ["border", "mixed"])
def test_walks_are_persistent_launches(which):
    for cus in (256, 304, 64, 120):
        c = E.walk_case(cus, which)
        ntiles, grid = E.first_grid(c.n, c.H, c.W, cus)
        per = len(E.first_tiles(c.H, c.W))
        assert grid == 3 * cus and ntiles > 3 * grid and ntiles > 9 * cus and ntiles % grid != 0 and grid % per != 0, (cus, c.id)
        assert ntiles < 4 * grid                              # some workgroups walk 3 tiles and others 4
        assert c.n * c.H * c.W * 64 * 4 < (110 << 20) * max(1, cus // 256), (cus, c.id)
        interior = any(k for (_y, _x, k) in E.first_tiles(c.H, c.W))
        assert interior == (which == "mixed")


@pytest.mark.parametrize("fault", FAULTS_FIRST)
def test_each_fault_breaks_first_layer_equality(fault):
    """The GPU assertion is ``torch.equal`` against ``first_reference``: a kernel with this one fault would give the faulted
    reference's answer, which must differ on every case the fault can occur in."""
    ran = 0
    for case in E.FIRST_CASES:
        if fault == "seam" and case.W <= E.SEAM:
            continue
        x = E.first_image(case)
        good, bad = E.first_reference(x), E.first_reference(x, fault=fault)
        assert not torch.equal(good, bad), case.id
        ran += 1
    assert ran >= 20


@pytest.mark.parametrize("fault", FAULTS_FIRST)
def test_each_fault_leaves_the_uint8_bound(fault):
    """The uint8 entry is held to gamma_28 (sum |x| |W'| + |b'|); the unfaulted float32 restatement stays inside it and every fault
    leaves it."""
    case = next(c for c in E.FIRST_CASES if (c.H, c.W) == (17, 65) and c.kind == "map")
    x = E.u8_as_float_nchw(E.first_image_u8(case))
    ref, mag = E.first_bounded_reference(x)
    got = torch.from_numpy(E.first_restated32(x[0].numpy()))[None]
    assert E.worst_excess(got, ref, E.GAMMA_FIRST * mag)[0] == 0
    bad = E.first_reference(x, fault=fault)
    assert E.worst_excess(bad, ref, E.GAMMA_FIRST * mag)[0] > 0


# ---- last layer -------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def last_input(weights):
    """The last layer's input for a 3 x 5 feature map (24 x 40 pixels: a partial last tile row and column, a seam at column 32),
    from the float64 decoder on the CPU: the statistics the device meets."""
    x = E.decoder_head(weights[1], E.last_feature(1, 3, 5)).float().double()          # float32 values, as on the device
    assert x.shape == (1, 24, 40, 64) and E.is_activation(x)
    return x


@pytest.mark.parametrize("which", ["dense", "tap0", "tap5"])
def test_float32_last_layer_is_inside_the_bound(last_input, which):
    w, b = E.last_weights(which)
    ref, mag = E.last_reference(last_input, which)
    x32 = last_input.float().permute(0, 3, 1, 2)
    got = F.conv2d(F.pad(x32, (1, 1, 1, 1), mode="reflect"), w.float(), b.float())
    assert got.dtype == torch.float32
    count, first = E.worst_excess(got, ref, E.GAMMA_LAST * mag)
    assert count == 0, first
    assert float((got.double() - ref).abs().max()) > 0       # float32 does round here: the bound is not vacuous


@pytest.mark.parametrize("which", ["dense", "tap0", "tap4", "tap8"])
@pytest.mark.parametrize("fault", FAULTS_LAST)
def test_each_fault_leaves_the_last_layer_bound(last_input, which, fault):
    ref, mag = E.last_reference(last_input, which)
    bad, _ = E.last_reference(last_input, which, fault=fault)
    count, _first = E.worst_excess(bad, ref, E.GAMMA_LAST * mag)
    if which != "dense" and fault in ("clamp_row", "clamp_col", "seam") and fault not in _reached(which):
        assert count == 0                                     # this tap never reads the faulted position: the dense set is what catches it
    else:
        assert count > 0, (which, fault)


def _reached(which):
    """The geometric faults a one-tap set can see: a tap in the last window row / column reads the pad behind the last row /
    column; a tap in the first window column reads column 31 for output column 32."""
    t = int(which[3:])
    out = set()
    if t // 3 == 2:
        out.add("clamp_row")
    if t % 3 == 2:
        out.add("clamp_col")
    if t % 3 == 0:
        out.add("seam")
    return out


def test_last_layer_weight_sets():
    w, b = E.last_weights("dense")
    assert w.unique().numel() == 1728 and float(w.abs().min()) >= 1 and float(b.abs().min()) > 0
    for t in range(9):
        wt, _ = E.last_weights(f"tap{t}")
        nz = torch.nonzero(wt.abs().sum((0, 1)))
        assert nz.tolist() == [[t // 3, t % 3]]
        assert bool((torch.sign(wt[:, :, t // 3, t % 3]) == E.TAP_SIGN[t]).all()) and wt[:, :, t // 3, t % 3].abs().unique().numel() == 192
    s = torch.tensor(E.TAP_SIGN).view(3, 3)
    assert not any(torch.equal(s, m) for m in (s.flip(0), s.flip(1), s.t(), s.flip(0).flip(1)))
    assert [E.last_grid(*c) for c in E.LAST_SHAPES] == [(1, False), (1, False), (4, False), (9, False), (16, True), (12, False)]


@pytest.mark.parametrize("n,hc,wc", E.LAST_SHAPES)
def test_decoder_plan_restatement(n, hc, wc):
    plan = arch.decoder_plan()
    assert len(plan) == 9 and (plan[-1]["cin"], plan[-1]["cout"], plan[-1]["relu"]) == (64, 3, False)
    a, b, layers = E.decoder_buffers(n, hc, wc)
    assert [buf for (buf, *_rest) in layers] == [0, 1, 0, 1, 0, 1, 0, 1]
    assert layers[7] == (1, n, 8 * hc, 8 * wc, 64, 64)       # the last layer's input: buffer B, the image's size, 64 channels
    # every layer's size, walked through the plan's own entries
    h, w = hc, wc
    for (buf, ln, lh, lw, cin, cout), L in zip(layers, plan):
        if L["src"] == "up":
            h, w = 2 * h, 2 * w
        assert (ln, lh, lw, cin, cout) == (n, h, w, L["cin"], L["cout"])
    # the maxima in closed form: A holds 256 ch at 2x (1024 floats per feature position), B 64 ch at 8x (4096)
    assert a == -(-1024 * n * hc * wc // 64) * 64 and b == -(-4096 * n * hc * wc // 64) * 64
    assert arch.conv_flops_decoder(hc, wc) * n == sum(2 * ln * lh * lw * cin * cout * 9 for (_b, ln, lh, lw, cin, cout) in layers) \
        + 2 * n * 64 * hc * wc * 64 * 3 * 9
    assert E.decoder_workspace_floats(n, hc, wc, lambda *dims: 0) == a + b
    assert E.decoder_workspace_floats(n, hc, wc, lambda *dims: 4 * 65) == a + b + 128
