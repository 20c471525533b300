"""Data, references and yardsticks for the two edge layers of the networks (csrc/conv_edge.hip): the first encoder layer
(``conv_first_kernel``: conv0 folded into conv1_1, 3 -> 64, reached through ``adain_encode_relu1_1``) and the last decoder layer
(``conv_last_kernel``: 64 -> 3, reached through ``adain_decode`` at the sizes 8 hc x 8 wc the product runs it at).

First layer - exact integers.  conv0 and conv1_1 are small integers, so ``pack_conv_first_kernel``'s fp32 fold W' = sum w1 w0,
b' = b1 + sum w1 b0 is exact; the images are integer-valued, so every product and partial sum of the kernel's K = 28 fp32 MFMA chain
(27 taps and the bias row against a constant 1) is an integer, and below 2^24 exact in any order.  The float entry must then be
``torch.equal`` to a float64 evaluation of the UNFOLDED sequence conv0 1x1 -> ReflectionPad2d(1) -> conv1_1 -> ReLU.  The uint8 entry
sees v / 255, which is no integer: it is held bitwise to the float entry and, against float64, to the a-priori bound of a 28-term
fp32 sum in any order, gamma_28 (sum |x| |W'| + |b'|).

Last layer - a derived bound.  Its input is whatever the eight generic layers in front of it produced; the test reads that tensor
back from the caller-owned workspace (``decoder_buffers`` restates where the plan puts it) and holds every output element to
bias + sum x w in float64 within gamma_577 (sum |x| |w| + |bias|): 576 products and the bias, in any summation order.

``gamma(n) = n u / (1 - n u)`` with u = 2^-24 (Higham, Accuracy and Stability of Numerical Algorithms, lemma 3.1 and section 3.1): n
roundings, each of relative size at most u, compound to at most gamma(n); a sum of n terms whose products were rounded once takes at
most n roundings per term in any order.  No figure in this file was read off a kernel.

``conv_ref`` takes a single FAULT (a shifted tap, a clamp for a reflection, a seam column from the neighbouring pixel, ...):
tests/test_edge_exact_host.py shows on this module's own data that each of them breaks the assertion the GPU tests make."""
from collections import namedtuple

import numpy as np
import torch
import torch.nn.functional as F

from applied_image_processing_amd import arch
from conv_exact import first_mismatches, mismatch_message  # noqa: F401  (the failure messages of the equality tests)

CAP = float(2 ** 24)                # integers below it are exact in fp32
U = 2.0 ** -24                      # unit roundoff of fp32, round to nearest


def gamma(n):
    return n * U / (1 - n * U)


GAMMA_FIRST = gamma(28)             # 27 taps + the bias row: one rounding per product, at most 27 per sum
GAMMA_LAST = gamma(577)             # 576 products + the bias


# ---- one reference for both layers, with single faults ---------------------------------------------------------------------------------
SEAM = 32                           # both kernels' tiles are 32 columns wide: column 32 is the first of the second tile column


def _pad_index(n, clamp_last):
    """Source index of the n + 2 positions of ReflectionPad2d(1); ``clamp_last``: the position past the end repeats the last one."""
    return [1] + list(range(n)) + [n - 1 if clamp_last else n - 2]


def conv_ref(x, w, b, fault=None):
    """ReflectionPad2d(1) + Conv2d in float64: x NCHW, w OIHW, b [O] -> NCHW.  ``fault`` (None: the layer as it is):
    "tap_shift" every tap moved one column, "clamp_row" / "clamp_col" a clamp in place of the reflection behind the last row /
    column, "seam" output column 32 computed with input column 31 taken from its neighbour 32 (a stale or shifted halo column at a
    tile seam; needs W >= 33), "no_bias"."""
    x, w, b = x.double(), w.double(), b.double()
    if fault == "tap_shift":
        w = torch.roll(w, 1, 3)
    if fault == "no_bias":
        b = torch.zeros_like(b)
    H, W = x.shape[2:]
    rows, cols = _pad_index(H, fault == "clamp_row"), _pad_index(W, fault == "clamp_col")
    out = F.conv2d(x[:, :, rows][:, :, :, cols], w, b)
    if fault == "seam":
        assert W > SEAM, "the seam fault needs two tile columns"
        xs = x.clone()
        xs[:, :, :, SEAM - 1] = x[:, :, :, SEAM]
        out[:, :, :, SEAM] = F.conv2d(xs[:, :, rows][:, :, :, cols], w, b)[:, :, :, SEAM]
    return out


def to_float32_exact(y):
    """A float64 tensor of integers as float32; the cast is exact and asserted to be."""
    out = y.float()
    assert torch.equal(out.double(), y), "the float64 reference does not fit float32: not an integer case"
    return out


def worst_excess(got, ref, bound, k=4):
    """(number of elements with |got - ref| > bound, the first k of them as (index..., got, ref, bound))."""
    got, ref, bound = got.detach().cpu().double(), ref.detach().cpu().double(), bound.detach().cpu().double()
    assert got.shape == ref.shape == bound.shape, (tuple(got.shape), tuple(ref.shape), tuple(bound.shape))
    bad = torch.nonzero(~((got - ref).abs() <= bound))               # (a NaN is an excess)
    return int(bad.shape[0]), [(*(int(i) for i in idx), float(got[tuple(idx)]), float(ref[tuple(idx)]), float(bound[tuple(idx)])) for idx in bad[:k]]


def bound_message(what, got, ref, bound, layout):
    count, first = worst_excess(got, ref, bound)
    return f"{what}: {count} of {ref.numel()} elements outside the bound; first ({layout}, got, float64, bound): {first}"


# ---- first layer: weights ------------------------------------------------------------------------------------------------------------
# conv0 [c'][c]: neither diagonal nor symmetric, so a transposed fold or a swapped colour shows
W0 = torch.tensor([[2, -1, 3], [1, 4, -2], [-3, 1, 2]], dtype=torch.float64)
B0 = torch.tensor([1, -2, 3], dtype=torch.float64)
# channels with a constant pre-activation: exactly zero, negative, positive; ZERO_FOLD has weights but a folded bias b' of exactly 0
CH_ZERO, CH_NEG, CH_POS, CH_ZERO_FOLD = 0, 1, 2, 3
QUAD_SWAP = (5, 6)                  # the two channels of quad 1 the "quad_swap" fault exchanges


def first_weights():
    """(w0 [3][3], b0 [3], w1 [64][3][3][3], b1 [64]) in float64: seeded integers, |w1| <= 3, |b1| <= 50."""
    g = torch.Generator().manual_seed(7)
    w1 = torch.randint(-3, 4, (64, 3, 3, 3), generator=g).double()
    b1 = torch.randint(-50, 51, (64,), generator=g).double()
    for ch, bias in ((CH_ZERO, 0.0), (CH_NEG, -5.0), (CH_POS, 7.0)):
        w1[ch] = 0
        b1[ch] = bias
    b1[CH_ZERO_FOLD] = -(w1[CH_ZERO_FOLD].sum((1, 2)) * B0).sum()
    return W0.clone(), B0.clone(), w1, b1


def first_state_dict(base):
    """The encoder's state dict ``base`` with conv0 and conv1_1 replaced by ``first_weights``."""
    w0, b0, w1, b1 = first_weights()
    sd = dict(base)
    sd["0.weight"], sd["0.bias"] = w0.float().view(3, 3, 1, 1).contiguous(), b0.float()
    sd["2.weight"], sd["2.bias"] = w1.float(), b1.float()
    return sd


def fold(w0, b0, w1, b1):
    """(W' [64][3][3][3], b' [64]) in float64: W'[o][c][t] = sum_c' w1[o][c'][t] w0[c'][c], b'[o] = b1[o] + sum_{c',t} w1[o][c'][t] b0[c']
    (a pointwise conv commutes with the reflection pad)."""
    return torch.einsum("opyx,pc->ocyx", w1, w0), b1 + torch.einsum("opyx,p->o", w1, b0)


# ---- first layer: references ------------------------------------------------------------------------------------------------------------
def first_reference(x, weights=None, fault=None):
    """The UNFOLDED layer in float64 on NCHW ``x``: conv0 1x1, ReflectionPad2d(1), conv1_1, ReLU, as NHWC float64.  Faults: those of
    ``conv_ref`` (applied to conv1_1; "no_bias" drops the folded bias, b0's share included), "quad_swap" (two output channels of a
    quad), "colour_swap" (input planes 0 and 2), "conv0_T" (conv0 transposed)."""
    w0, b0, w1, b1 = weights or first_weights()
    x = x.double()
    if fault == "colour_swap":
        x = x[:, [2, 1, 0]]
    if fault == "conv0_T":
        w0 = w0.t()
    if fault == "no_bias":
        b0 = torch.zeros_like(b0)
    y = F.conv2d(x, w0.reshape(3, 3, 1, 1), b0)
    pre = conv_ref(y, w1, b1, fault if fault in ("tap_shift", "clamp_row", "clamp_col", "seam", "no_bias") else None)
    if fault == "quad_swap":
        order = list(range(64))
        order[QUAD_SWAP[0]], order[QUAD_SWAP[1]] = QUAD_SWAP[1], QUAD_SWAP[0]
        pre = pre[:, order]
    return pre.clamp_min(0).permute(0, 2, 3, 1).contiguous()


def first_bounded_reference(x, weights=None):
    """The FOLDED layer in float64 on NCHW ``x`` (the float32 values the kernel multiplies, exact in float64), with the magnitude the
    gamma_28 bound scales: (ReLU output NHWC, sum |x| |W'| + |b'| NHWC).  ReLU moves two numbers no further apart than they were."""
    wf, bf = fold(*(weights or first_weights()))
    x = x.double()
    rows, cols = _pad_index(x.shape[2], False), _pad_index(x.shape[3], False)
    xp = x[:, :, rows][:, :, :, cols]
    ref = F.conv2d(xp, wf, bf).clamp_min(0)
    mag = F.conv2d(xp.abs(), wf.abs(), bf.abs())
    return ref.permute(0, 2, 3, 1).contiguous(), mag.permute(0, 2, 3, 1).contiguous()


def first_restated32(x, weights=None):
    """The kernel's arithmetic in float32 numpy on ONE image x [3][H][W]: the pack kernel's fold in its order, then K = 28 - row
    e = 3 tap + colour of the weight matrix for e < 27, the folded bias against a constant 1 at e = 27 - and ReLU: [H][W][64]."""
    w0, b0, w1, b1 = (np.asarray(v, np.float32) for v in (weights or first_weights()))
    w1 = w1.reshape(64, 3, 9)
    wf = np.zeros((64, 3, 9), np.float32)
    bf = b1.copy()
    for cp in range(3):
        wf += w1[:, cp, None, :] * w0[cp][None, :, None]
        for t in range(9):
            bf += w1[:, cp, t] * b0[cp]
    A = np.concatenate([wf.transpose(2, 1, 0).reshape(27, 64), bf[None]], 0)                    # [e][o]
    x = np.asarray(x, np.float32)
    _, H, W = x.shape
    xp = np.pad(x, ((0, 0), (1, 1), (1, 1)), mode="reflect")
    P = np.ones((H * W, 28), np.float32)
    for tap in range(9):
        for c in range(3):
            P[:, 3 * tap + c] = xp[c, tap // 3:tap // 3 + H, tap % 3:tap % 3 + W].ravel()
    out = np.maximum(P @ A, np.float32(0))
    assert out.dtype == np.float32
    return out.reshape(H, W, 64)


def first_headroom(x, weights=None):
    """(27 max|x| max|W'| + max|b'|, the largest partial sum of the fold itself): both must stay below 2^24."""
    w0, b0, w1, b1 = weights or first_weights()
    wf, bf = fold(w0, b0, w1, b1)
    a = 27 * float(x.abs().max()) * float(wf.abs().max()) + float(bf.abs().max())
    b = max(3 * float(w1.abs().max()) * float(w0.abs().max()), float(b1.abs().max()) + 27 * float(w1.abs().max()) * float(b0.abs().max()))
    return a, b


# ---- first layer: images and cases ------------------------------------------------------------------------------------------------------
# kind: "map" one image, "batch" held against its frames one by one too, "walk" a persistent launch (built for the device's compute
# units by ``walk_case``)
FirstCase = namedtuple("FirstCase", "id kind n H W seed")
FIRST_TH, FIRST_TW = 8, 32
WIDTHS, HEIGHTS = (31, 32, 33, 63, 64, 65, 97), (7, 8, 9, 15, 16, 17, 25)


def _first_cases():
    t = []

    def add(kind, n, H, W):
        t.append(FirstCase(f"{kind}-n{n}-{H}x{W}", kind, n, H, W, 2000 + len(t)))

    for H, W in ((2, 2), (2, 40), (40, 2)):                  # reflect on both sides within one halo
        add("map", 1, H, W)
    for H in HEIGHTS:                                        # every width class meets full (8, 16) and partial last tile rows
        for W in WIDTHS:
            add("map", 1, H, W)
    add("batch", 2, 17, 65)
    add("batch", 3, 9, 33)
    return t


FIRST_CASES = _first_cases()


def first_tiles(H, W):
    """(ty0, tx0, interior) of a frame's tiles in list order; ``interior``: the halo lies inside the image, the kernel takes its
    constant-offset loads (mirrors conv_first_kernel)."""
    return [(ty0, tx0, ty0 >= 1 and ty0 + 9 <= H and tx0 >= 1 and tx0 + 33 <= W)
            for ty0 in range(0, H, FIRST_TH) for tx0 in range(0, W, FIRST_TW)]


def first_grid(n, H, W, cus):
    """(tiles of the launch, workgroups) - mirrors launch_conv_first: 3 workgroups per compute unit walk the tile list."""
    ntiles = n * len(first_tiles(H, W))
    return ntiles, min(ntiles, 3 * cus)


WALK_FRAMES = {"border": [(17, 34), (33, 34), (49, 20)], "mixed": [(25, 97), (33, 65), (17, 65), (49, 65)]}         # 6, 10, 7 and 16, 15, 9, 21 tiles


def walk_case(cus, which):
    """A batch of small frames that is a persistent launch on ``cus`` compute units: more than 3 tiles per workgroup and a tile
    count that is no multiple of the grid (a quarter of the workgroups walk 4 tiles, the rest 3: both LDS parities are used and the
    walk ends on either), of the first candidate frame whose tile count does not divide the grid - so a workgroup's consecutive
    tiles sit at different positions of different images.  "mixed": frames with interior tiles beside border tiles."""
    grid = 3 * cus
    for H, W in WALK_FRAMES[which]:
        per = len(first_tiles(H, W))
        if grid % per:
            n = -(-(3 * grid + grid // 4) // per)
            if (n * per) % grid == 0:
                n += 1
            return FirstCase(f"walk-{which}-n{n}-{H}x{W}", "walk", n, H, W, 3000 + len(which))
    raise AssertionError(f"no walk frame for {cus} compute units")


def first_image(case):
    """Integer-valued float NCHW [n][3][H][W]: per frame a seeded permutation of 3 H W consecutive integers centred on 0 - every pixel
    of every plane has its own value."""
    g = torch.Generator().manual_seed(case.seed)
    k = 3 * case.H * case.W
    perm = torch.rand(case.n, k, generator=g).argsort(1)
    return (perm - k // 2).float().view(case.n, 3, case.H, case.W).contiguous()


def first_image_u8(case):
    """Decoded frames uint8 [n][H][W][3]: per plane a seeded permutation of 0 .. H W - 1 modulo 256 - from 256 pixels on every byte
    value occurs in every plane."""
    g = torch.Generator().manual_seed(case.seed + 500)
    perm = torch.rand(case.n, 3, case.H * case.W, generator=g).argsort(2)
    return (perm % 256).to(torch.uint8).view(case.n, 3, case.H, case.W).permute(0, 2, 3, 1).contiguous()


def u8_as_float_nchw(u8):
    """torchvision's ToTensor: float32(v) / 255, NCHW."""
    return u8.permute(0, 3, 1, 2).float().div(255).contiguous()


# ---- last layer: weights, input, reference ----------------------------------------------------------------------------------------------
LAST_KEY = arch.conv_indices(arch.DECODER_MODULES)[-1]
LAST_TH, LAST_TW = 16, 32
LAST_SHAPES = [(1, 2, 2), (1, 2, 4), (1, 3, 5), (1, 5, 9), (2, 8, 8), (3, 3, 5)]          # (n, hc, wc): the image is 8 hc x 8 wc
LAST_BIAS = torch.tensor([300, -500, 700], dtype=torch.float64)
TAP_SIGN = (1, -1, -1, 1, -1, 1, 1, 1, -1)                                                # no mirror or transposition of the taps keeps it
LAST_SETS = ["dense"] + [f"tap{t}" for t in range(9)]


def last_weights(which):
    """(w [3][64][3][3], b [3]) in float64.  "dense": the 1728 integers -864 .. 864 without 0, shuffled - different for every
    (cout, cin, tap).  "tap<t>": tap t alone, TAP_SIGN[t] x a shuffle of 1 .. 192 of its own."""
    w = torch.zeros(3, 64, 3, 3, dtype=torch.float64)
    if which == "dense":
        g = torch.Generator().manual_seed(11)
        vals = torch.cat([torch.arange(-864, 0), torch.arange(1, 865)])
        w = vals[torch.randperm(1728, generator=g)].double().view(3, 64, 3, 3)
    else:
        t = int(which[3:])
        g = torch.Generator().manual_seed(100 + t)
        w[:, :, t // 3, t % 3] = TAP_SIGN[t] * (torch.randperm(192, generator=g) + 1).double().view(3, 64)
    return w, LAST_BIAS.clone()


def last_state_dict(base, which):
    """The decoder's state dict ``base`` with only the last layer replaced: the eight layers in front keep their weights, so the
    last layer's input is a post-ReLU map that varies per pixel."""
    w, b = last_weights(which)
    sd = dict(base)
    sd[f"{LAST_KEY}.weight"], sd[f"{LAST_KEY}.bias"] = w.float(), b.float()
    return sd


def last_feature(n, hc, wc):
    """A non-negative relu4_1-like feature map NHWC [n][hc][wc][512], seeded by its shape."""
    g = torch.Generator().manual_seed(10000 * n + 100 * hc + wc)
    return (torch.rand(n, hc, wc, 512, generator=g) * 2).contiguous()


def last_reference(x_nhwc, which, fault=None):
    """(bias + sum x w, sum |x| |w| + |bias|) in float64 over the reflect-padded 3 x 3 x 64 window, both NCHW [n][3][H][W].  Faults:
    those of ``conv_ref``, "quad_swap" (two input channels of a quad), "colour_swap" (output planes 0 and 2)."""
    w, b = last_weights(which)
    x = x_nhwc.detach().cpu().double().permute(0, 3, 1, 2)
    mag = conv_ref(x.abs(), w.abs(), b.abs())
    if fault == "quad_swap":
        order = list(range(64))
        order[QUAD_SWAP[0]], order[QUAD_SWAP[1]] = QUAD_SWAP[1], QUAD_SWAP[0]
        x = x[:, order]
    ref = conv_ref(x, w, b, fault if fault in ("tap_shift", "clamp_row", "clamp_col", "seam", "no_bias") else None)
    if fault == "colour_swap":
        ref = ref[:, [2, 1, 0]]
    return ref, mag


def is_activation(x_nhwc):
    """What the last layer's input must look like wherever it comes from: no NaN, non-negative, a non-zero channel at every pixel
    and more than a quarter of all elements non-zero (a ReLU behind zero-mean weights passes somewhat under half)."""
    x = x_nhwc.detach().cpu()
    return (not bool(torch.isnan(x).any()) and float(x.min()) >= 0 and bool((x > 0).any(-1).all())
            and int((x > 0).sum()) > x.numel() // 4)


def last_grid(n, hc, wc):
    """Workgroups of the last layer's launch (one per 16 x 32 tile) and whether its tile list is remapped over the XCDs."""
    grid = n * -(-8 * hc // LAST_TH) * -(-8 * wc // LAST_TW)
    return grid, grid % 8 == 0


def decoder_head(sd, feat_nhwc):
    """The eight generic decoder layers in float64 torch on the CPU: NHWC [n][hc][wc][512] -> NHWC [n][8 hc][8 wc][64] (what the last
    layer reads; the host tests use it as an input of the statistics the device tests meet)."""
    x = feat_nhwc.double().permute(0, 3, 1, 2)
    for L in arch.decoder_plan()[:-1]:
        if L["src"] == "up":
            x = F.interpolate(x, scale_factor=2, mode="nearest")
        x = F.relu(conv_ref(x, sd[f"{L['idx']}.weight"], sd[f"{L['idx']}.bias"]))
    return x.permute(0, 2, 3, 1).contiguous()


# ---- the decoder's workspace, restated ---------------------------------------------------------------------------------------------------
def _align64(v):
    return (v + 63) // 64 * 64


def decoder_buffers(n, hc, wc):
    """Where ``adain_decode`` keeps its generic layers' outputs, restated from ``arch.decoder_plan()``: the layers write the ping-pong
    buffers A, B, A, ... (the input is the caller's tensor), a buffer is the 64-float aligned maximum over the layers that write it,
    and B follows A in the workspace.  Returns (floats of A, floats of B, [(buffer 0 | 1, n, H, W, cin, cout) per layer])."""
    h, w, mx, layers = hc, wc, [0, 0], []
    for l, L in enumerate(arch.decoder_plan()[:-1]):
        if L["src"] == "up":
            h, w = 2 * h, 2 * w
        mx[l % 2] = max(mx[l % 2], n * h * w * L["cout"])
        layers.append((l % 2, n, h, w, L["cin"], L["cout"]))
    return _align64(mx[0]), _align64(mx[1]), layers


def decoder_workspace_floats(n, hc, wc, split_bytes):
    """A + B + slabs in floats; ``split_bytes(n, h, w, cin, cout)``: the library's own answer for the cin split's partial-sum slabs
    of one layer (``runtime.conv3x3_wino4_split_bytes``)."""
    a, b, layers = decoder_buffers(n, hc, wc)
    slab = max(split_bytes(ln, h, w, cin, cout) // 4 for (_buf, ln, h, w, cin, cout) in layers)
    return a + b + _align64(slab)
