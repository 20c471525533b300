"""GPU tests that hold the two kernels of csrc/conv_edge.hip to per-element answers, through the entry points the product uses.

First layer (``conv_first_kernel<U8>`` through ``rt.encode_relu1_1``): integer weights and integer-valued images, on which the fold
and the K = 28 fp32 MFMA chain are exact (tests/edge_exact.py; tests/test_edge_exact_host.py checks the head-room of every case), so
the float entry is ``torch.equal`` to a float64 evaluation of the unfolded conv0 -> pad -> conv1_1 -> ReLU - at maps from 2 x 2 over
every width and height class of the 8 x 32 tile to maps with interior tiles, in batches, and in persistent launches where a workgroup
walks 3 or 4 tiles of different images through its two halo slots.  The uint8 entry is bitwise the float entry on v / 255 and within
gamma_28 (sum |x| |W'| + |b'|) of float64.  No output element may be -0.0.

Last layer (``conv_last_kernel<false>`` through ``adain_decode``): its weights are the test's integers, its input is read back from
the workspace the test owns (pre-filled with NaN), and every output element is within gamma_577 (sum |x| |w| + |bias|) of
bias + sum x w in float64 - the bound of ANY summation order, derived in tests/edge_exact.py, with no number taken from a kernel.

A wrong column at a tile seam, a clamp for a reflection, swapped channels or planes, a stale halo slot, a dropped bias: each is a
failure at coordinates the message names (tests/test_edge_exact_host.py shows that each of them fails these assertions).
Run with ``-m gpu``."""
import pytest
import torch

import edge_exact as E

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
NEG_ZERO = -2 ** 31                 # the bit pattern of -0.0 as int32


@pytest.fixture(scope="module")
def rt():
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    import applied_image_processing_amd.runtime as rt

    rt.lib()
    torch.cuda.set_device(0)
    return rt


@pytest.fixture(scope="module")
def cus():
    return torch.cuda.get_device_properties(0).multi_processor_count


@pytest.fixture(scope="module")
def enc(rt, weights):
    return rt.pack_encoder(E.first_state_dict(weights[0]), torch.device(DEV))


@pytest.fixture(scope="module")
def dec(rt, weights):
    packed = {}

    def get(which):
        if which not in packed:
            packed[which] = rt.pack_decoder(E.last_state_dict(weights[1], which), torch.device(DEV))
        return packed[which]
    return get


# ---- first layer ------------------------------------------------------------------------------------------------------------------------
def _no_negative_zero(what, got):
    """The integer-max ReLU gives +0 for negative and zero pre-activations."""
    bad = torch.nonzero(got.view(torch.int32) == NEG_ZERO)
    assert bad.shape[0] == 0, f"{what}: {bad.shape[0]} elements are -0.0; first (n, y, x, c): {bad[:8].tolist()}"


def _float_entry(rt, enc, case, x):
    got = rt.encode_relu1_1(x.cuda(), enc)
    torch.cuda.synchronize()
    want = E.to_float32_exact(E.first_reference(x))
    got = got.cpu()
    assert got.shape == want.shape == (case.n, case.H, case.W, 64)
    assert torch.equal(got, want), E.mismatch_message(f"{case.id} float entry", got, want)
    _no_negative_zero(f"{case.id} float entry", got)
    return got


def _u8_entry(rt, enc, case, u8):
    xf = E.u8_as_float_nchw(u8)
    got = rt.encode_relu1_1(u8.cuda(), enc)
    same = rt.encode_relu1_1(xf.cuda(), enc)
    torch.cuda.synchronize()
    got, same = got.cpu(), same.cpu()
    assert torch.equal(got, same), E.mismatch_message(f"{case.id} uint8 entry against the float entry on v / 255", got, same)
    ref, mag = E.first_bounded_reference(xf)
    count, first = E.worst_excess(got, ref, E.GAMMA_FIRST * mag)
    print(f"{case.id} uint8 entry: worst |got - float64| / (sum |x| |W'| + |b'|) = {float(((got.double() - ref).abs() / mag.clamp_min(1e-300)).max()):.3e}"
          f", gamma_28 = {E.GAMMA_FIRST:.3e}")
    assert count == 0, E.bound_message(f"{case.id} uint8 entry", got, ref, E.GAMMA_FIRST * mag, "n, y, x, c")
    _no_negative_zero(f"{case.id} uint8 entry", got)
    return got


def _frames_one_by_one(rt, enc, case, image, whole):
    for i in range(case.n):
        one = rt.encode_relu1_1(image[i:i + 1].contiguous().cuda(), enc)
        torch.cuda.synchronize()
        assert torch.equal(one.cpu()[0], whole[i]), E.mismatch_message(f"{case.id} frame {i} alone against the batch", one.cpu(), whole[i:i + 1])


@pytest.mark.parametrize("case", E.FIRST_CASES, ids=lambda c: c.id)
def test_first_layer_float_entry_is_exact(rt, enc, case):
    x = E.first_image(case)
    got = _float_entry(rt, enc, case, x)
    if case.kind == "batch":
        _frames_one_by_one(rt, enc, case, x, got)


@pytest.mark.parametrize("case", E.FIRST_CASES, ids=lambda c: c.id)
def test_first_layer_uint8_entry_is_the_float_entry_and_within_gamma_28(rt, enc, case):
    u8 = E.first_image_u8(case)
    got = _u8_entry(rt, enc, case, u8)
    if case.kind == "batch":
        _frames_one_by_one(rt, enc, case, u8, got)


@pytest.mark.parametrize("which", ["border", "mixed"])
def test_first_layer_persistent_walk(rt, enc, cus, which):
    """More than three tiles per workgroup and no multiple of the grid: some workgroups walk 3 tiles and others 4, through both halo
    slots, over tiles at different positions of different images ("mixed": interior and reflected tiles in one walk)."""
    case = E.walk_case(cus, which)
    ntiles, grid = E.first_grid(case.n, case.H, case.W, cus)
    per = len(E.first_tiles(case.H, case.W))
    assert grid == 3 * cus and ntiles > 3 * grid and ntiles % grid != 0 and grid % per != 0, (case.id, ntiles, grid)
    assert any(k for (_y, _x, k) in E.first_tiles(case.H, case.W)) == (which == "mixed")
    _float_entry(rt, enc, case, E.first_image(case))
    _u8_entry(rt, enc, case, E.first_image_u8(case))


# ---- last layer -------------------------------------------------------------------------------------------------------------------------
def _decode_in_owned_workspace(rt, feat, packed):
    """``adain_decode`` through ``rt.lib()`` with a NaN-filled workspace of exactly the documented size: (image NCHW, the last layer's
    input NHWC as the eighth generic layer left it in buffer B)."""
    n, hc, wc, _ = feat.shape
    L = rt.lib()
    nbytes = L.adain_decode_workspace_bytes(n, hc, wc)
    a, b, layers = E.decoder_buffers(n, hc, wc)
    assert 4 * E.decoder_workspace_floats(n, hc, wc, rt.conv3x3_wino4_split_bytes) == nbytes, "the decoder's workspace plan changed: edge_exact.decoder_buffers must follow it"
    buf, ln, H, W, _cin, cout = layers[7]
    assert (buf, ln, H, W, cout) == (1, n, 8 * hc, 8 * wc, 64)
    ws = torch.full((nbytes // 4,), float("nan"), dtype=torch.float32, device=feat.device)
    img = torch.full((n, 3, H, W), float("nan"), dtype=torch.float32, device=feat.device)
    rc = L.adain_decode(feat.data_ptr(), img.data_ptr(), packed.data_ptr(), ws.data_ptr(), nbytes, n, hc, wc, None, rt._stream())
    assert rc == 0, f"rc {rc}: {L.adain_last_error().decode()}"
    torch.cuda.synchronize()
    x = ws[a:a + n * H * W * 64].view(n, H, W, 64).cpu()
    return img.cpu(), x


def _last_layer(rt, dec, which, n, hc, wc):
    feat = E.last_feature(n, hc, wc).cuda()
    img, x = _decode_in_owned_workspace(rt, feat, dec(which))
    what = f"last layer, {which} weights, {n} x {hc} x {wc}"
    assert E.is_activation(x), f"{what}: the tensor read back from buffer B is not the last layer's input"
    ref, mag = E.last_reference(x, which)
    rel = float(((img.double() - ref).abs() / mag).max())
    print(f"{what}: worst |got - float64| / (sum |x| |w| + |bias|) = {rel:.3e}, gamma_577 = {E.GAMMA_LAST:.3e}")
    assert E.worst_excess(img, ref, E.GAMMA_LAST * mag)[0] == 0, E.bound_message(what, img, ref, E.GAMMA_LAST * mag, "n, plane, y, x")
    return feat, img


@pytest.mark.parametrize("n,hc,wc", E.LAST_SHAPES)
def test_last_layer_dense_weights_within_gamma_577(rt, dec, n, hc, wc):
    """One tile at half its width, one whole tile, partial last tile rows and columns, a grid of 16 (a multiple of 8: the tile list is
    remapped over the XCDs) and one of 12 (not remapped); batches against their frames decoded one by one."""
    if (n, hc, wc) == (2, 8, 8):
        assert E.last_grid(n, hc, wc) == (16, True)
    if (n, hc, wc) == (3, 3, 5):
        assert E.last_grid(n, hc, wc) == (12, False)
    feat, img = _last_layer(rt, dec, "dense", n, hc, wc)
    whole = rt.decode(feat, dec("dense"))
    torch.cuda.synchronize()
    assert torch.equal(whole.cpu(), img), "the call in the owned workspace and the runtime wrapper disagree"
    for i in range(n if n > 1 else 0):
        one = rt.decode(feat[i:i + 1].contiguous(), dec("dense"))
        torch.cuda.synchronize()
        got, want = one.cpu().permute(0, 2, 3, 1), img[i:i + 1].permute(0, 2, 3, 1)
        assert torch.equal(got, want), E.mismatch_message(f"frame {i} decoded alone against the batch", got, want)


@pytest.mark.parametrize("tap", range(9))
def test_last_layer_single_taps_within_gamma_577(rt, dec, tap):
    """One non-zero tap at a time, each with its own sign and magnitudes: a shifted or mirrored tap or a swapped output plane cannot
    cancel against another tap.  24 x 40 pixels: partial last tile row and column, a seam at column 32."""
    _last_layer(rt, dec, f"tap{tap}", 1, 3, 5)
