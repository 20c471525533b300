"""Integer data on which the 3x3 Winograd kernels (csrc/conv_wino4.hip) must be EXACT, and the yardstick they are held to.

The kernels' arithmetic is fp32 (v_mfma_f32_32x32x2_f32) with dyadic input and output transforms; the only non-dyadic constants
(1/6, 1/12, 1/24) sit in the pack kernels, which evaluate U = G g G^T in double and round once.  With an integer input, an integer bias
and weights that are integer multiples of 48 (1/24 x 1/2, the smallest entries of G4 / G5 times that of G2 / G3), U is an integer, and
so is every transformed input, product, partial sum and output-transform intermediate.  While all of them stay below 2^24 every fp32
operation is exact: the result does not depend on accumulation order, tile geometry, stage count, persistent hand-over, cin split or
phase folding, and must be ``torch.equal`` to a float64 convolution.

This module holds the transform matrices (one copy for every test file), the seeded integer layers, the float64 reference, the
algebra restated in numpy at a chosen precision, the head-room of a case against 2^24, and ``CASES`` - the one table of shapes that
tests/test_conv_exact_host.py checks for head-room on the CPU and tests/test_gpu_conv_exact.py runs on the device."""
from collections import namedtuple

import numpy as np
import torch
import torch.nn.functional as F

from applied_image_processing_amd import arch

# ---- transforms ------------------------------------------------------------------------------------------------------------------------
# F(4,3) down the rows (points 0, +-1, +-2, inf), F(2,3) along the columns; the polyphase up layers use F(5,2) / F(3,2) on the same
# points, so the input transform B4^T d B2 is shared.  B2T's last row is (0, 1, 0, -1): G2's last row is then (0, 0, -1) and A2T's last
# entry +1, as G3's last row is (0, -1) and A3T's last entry +1.
B4T = np.array([[4, 0, -5, 0, 1, 0], [0, -4, -4, 1, 1, 0], [0, 4, -4, -1, 1, 0], [0, -2, -1, 2, 1, 0], [0, 2, -1, -2, 1, 0], [0, 4, 0, -5, 0, 1]], float)
B2T = np.array([[1, 0, -1, 0], [0, 1, 1, 0], [0, -1, 1, 0], [0, 1, 0, -1]], float)
G4 = np.array([[1 / 4, 0, 0], [-1 / 6, -1 / 6, -1 / 6], [-1 / 6, 1 / 6, -1 / 6], [1 / 24, 1 / 12, 1 / 6], [1 / 24, -1 / 12, 1 / 6], [0, 0, 1]])
G2 = np.array([[1, 0, 0], [1 / 2, 1 / 2, 1 / 2], [1 / 2, -1 / 2, 1 / 2], [0, 0, -1]])
A4T = np.array([[1, 1, 1, 1, 1, 0], [0, 1, -1, 2, -2, 0], [0, 1, 1, 4, 4, 0], [0, 1, -1, 8, -8, 1]], float)
A2T = np.array([[1, 1, 1, 0], [0, 1, -1, 1]], float)
A5T = np.array([[1, 1, 1, 1, 1, 0], [0, 1, -1, 2, -2, 0], [0, 1, 1, 4, 4, 0], [0, 1, -1, 8, -8, 0], [0, 1, 1, 16, 16, 1]], float)
A3T = np.array([[1, 1, 1, 0], [0, 1, -1, 0], [0, 1, 1, 1]], float)
G5 = np.array([[1 / 4, 0], [-1 / 6, -1 / 6], [-1 / 6, 1 / 6], [1 / 24, 1 / 12], [1 / 24, -1 / 12], [0, 1]])
G3 = np.array([[1, 0], [1 / 2, 1 / 2], [1 / 2, -1 / 2], [0, -1]])
FOLD = [np.array([[1, 0, 0], [0, 1, 1]], float), np.array([[1, 1, 0], [0, 0, 1]], float)]      # even / odd phase

WEIGHT_UNIT = 48                    # weights are integer multiples of it: 1 / (1/24 x 1/2)
CAP = float(2 ** 24)                # integers below it are exact in fp32
CAP_MEASURED = float(2 ** 22)       # the measured output-transform sums stay 4x under the cap
V_GAIN = float(np.abs(B4T).sum(1).max() * np.abs(B2T).sum(1).max())      # max |B4^T d B2| over |d| <= 1: 10 x 2


# ---- data and reference ----------------------------------------------------------------------------------------------------------------
def int_layer(seed, cin, cout, n, hs, ws, xmax, wmax, unit=WEIGHT_UNIT):
    """x [n][hs][ws][cin] with integers in [-xmax, xmax], w [cout][cin][3][3] with ``unit`` x integers in [-wmax, wmax], b [cout] with
    integers in [-100, 100]; float32, seeded."""
    g = torch.Generator().manual_seed(seed)
    x = torch.randint(-xmax, xmax + 1, (n, hs, ws, cin), generator=g).float()
    w = (unit * torch.randint(-wmax, wmax + 1, (cout, cin, 3, 3), generator=g)).float()
    b = torch.randint(-100, 101, (cout,), generator=g).float()
    return x, w, b


def preactivation(x, w, b, up):
    """[nearest 2x upsample +] ReflectionPad2d(1) + Conv2d of NHWC ``x`` in float64 on the CPU: NCHW float64."""
    v = x.detach().cpu().double().permute(0, 3, 1, 2)
    if up:
        v = F.interpolate(v, scale_factor=2, mode="nearest")
    return F.conv2d(F.pad(v, (1, 1, 1, 1), mode="reflect"), w.detach().cpu().double(), b.detach().cpu().double())


def finish(pre, relu, pool):
    """[ReLU] [+ MaxPool2d(2, 2, ceil_mode=True)] of a ``preactivation``, as NHWC float32; the cast is exact and asserted to be."""
    y = pre.clamp_min(0) if relu else pre
    if pool:
        y = F.max_pool2d(y, 2, 2, 0, ceil_mode=True)
    y = y.permute(0, 2, 3, 1).contiguous()
    out = y.float()
    assert torch.equal(out.double(), y), "the float64 reference does not fit float32: not an integer case"
    return out


def reference(x, w, b, up=False, relu=False, pool=False):
    """The layer in float64 torch on the CPU, NHWC float32 (x NHWC, w OIHW)."""
    return finish(preactivation(x, w, b, up), relu, pool)


def first_mismatches(got, want, k=8):
    """(number of unequal elements, the first k of them as (n, y, x, c, got, want)) of two NHWC tensors."""
    got, want = got.detach().cpu(), want.detach().cpu()
    assert got.shape == want.shape, (tuple(got.shape), tuple(want.shape))
    bad = torch.nonzero(got != want)
    return int(bad.shape[0]), [(*(int(i) for i in idx), float(got[tuple(idx)]), float(want[tuple(idx)])) for idx in bad[:k]]


def mismatch_message(what, got, want):
    count, first = first_mismatches(got, want)
    return f"{what}: {count} of {want.numel()} elements differ; first (n, y, x, c, got, want): {first}"


# ---- the algebra, restated ---------------------------------------------------------------------------------------------------------------
def pack_f43(w):
    """U = G4 g G2^T [cout][cin][6][4] in float64 (the pack kernel's precision; the caller rounds once)."""
    return np.einsum("ra,oiab,jb->oirj", G4, np.asarray(w, np.float64), G2)


def pack_poly(w):
    """Per phase 2 py + px the folded 2 x 2 filter in F(5,2) x F(3,2): [4][cout][cin][6][4] in float64."""
    w = np.asarray(w, np.float64)
    return np.stack([np.einsum("ra,oiab,jb->oirj", G5, np.einsum("at,oits,bs->oiab", FOLD[py], w, FOLD[px]), G3)
                     for py in range(2) for px in range(2)])


def _f43_index(H, W):
    """Source rows [tiles_y][6] and columns [tiles_x][4] of the 4 x 2 output tiles of an H x W map under ReflectionPad2d(1); positions
    past the pad (ragged tiles: they feed no kept output) are clamped."""
    def axis(n, step, taps):
        v = np.clip(np.arange(0, n, step)[:, None] + np.arange(-1, taps - 1)[None, :], -1, n)
        v = np.abs(v)
        return np.where(v >= n, 2 * n - 2 - v, v)

    return axis(H, 4, 6), axis(W, 2, 4)


def _poly_index(hs, ws, py, px):
    """Source rows [tiles_y][6] and columns [tiles_x][4] of phase (py, px)'s 4 x 3 output tiles: a clamp pad."""
    rows = np.clip(np.arange(0, hs, 4)[:, None] + np.arange(-1 + py, 5 + py)[None, :], 0, hs - 1)
    cols = np.clip(np.arange(0, ws, 3)[:, None] + np.arange(-1 + px, 3 + px)[None, :], 0, ws - 1)
    return rows, cols


def _products(x, U, rows, cols, iy, ix, dtype):
    """M [tile][cout][6][4] = sum_cin U .* (B4^T d B2) for the tiles (iy[k], ix[k]) of one image x [cin][H][W]; every operation in
    ``dtype`` (U is rounded to it once)."""
    d = np.asarray(x, dtype)[:, rows[iy][:, :, None], cols[ix][:, None, :]]                    # [cin][tile][6][4]
    V = np.einsum("ra,itac,jc->rjti", B4T.astype(dtype), d, B2T.astype(dtype))
    Ur = np.ascontiguousarray(np.asarray(U).astype(dtype).transpose(2, 3, 1, 0))             # [6][4][cin][cout]
    M = np.matmul(V, Ur)                                                                        # [6][4][tile][cout]
    assert M.dtype == dtype
    return M.transpose(2, 3, 0, 1)


def wino_f43(x, w, dtype=np.float64):
    """x [cin][H][W], w [cout][cin][3][3] -> ReflectionPad2d(1) + conv [cout][H][W] as the kernel's F(4,3) x F(2,3) algebra."""
    _, H, W = x.shape
    rows, cols = _f43_index(H, W)
    iy, ix = (v.ravel() for v in np.meshgrid(np.arange(len(rows)), np.arange(len(cols)), indexing="ij"))
    M = _products(x, pack_f43(w), rows, cols, iy, ix, dtype)
    Y = np.einsum("ar,torj,bj->toab", A4T.astype(dtype), M, A2T.astype(dtype))
    assert Y.dtype == dtype
    out = np.zeros((w.shape[0], H, W), dtype)
    for k, (ty, tx) in enumerate(zip(4 * iy, 2 * ix)):
        ny, nx = min(4, H - ty), min(2, W - tx)
        out[:, ty:ty + ny, tx:tx + nx] = Y[k, :, :ny, :nx]
    return out


def polyphase(x, w, dtype=np.float64):
    """x [cin][hs][ws], w [cout][cin][3][3] -> nearest 2x upsample + ReflectionPad2d(1) + conv [cout][2 hs][2 ws] as the kernel's
    algebra: per phase, tiles of 4 x 3 outputs (rows 0-3 of F(5,2)) of the clamp-padded source, 6 x 4 patches."""
    _, hs, ws = x.shape
    U = pack_poly(w)
    out = np.zeros((w.shape[0], 2 * hs, 2 * ws), dtype)
    for py in range(2):
        for px in range(2):
            rows, cols = _poly_index(hs, ws, py, px)
            iy, ix = (v.ravel() for v in np.meshgrid(np.arange(len(rows)), np.arange(len(cols)), indexing="ij"))
            M = _products(x, U[2 * py + px], rows, cols, iy, ix, dtype)
            Y = np.einsum("ar,torj,bj->toab", A5T[:4].astype(dtype), M, A3T.astype(dtype))
            assert Y.dtype == dtype
            for k, (ty, tx) in enumerate(zip(4 * iy, 3 * ix)):
                ny, nx = min(4, hs - ty), min(3, ws - tx)
                out[:, 2 * ty + py:2 * (ty + ny):2, 2 * tx + px:2 * (tx + nx):2] = Y[k, :, :ny, :nx]
    return out


# ---- the cases ---------------------------------------------------------------------------------------------------------------------------
# entry: the runtime call ("wino": conv3x3_wino, "split": conv3x3_wino4_split, "poly": conv3x3_up2x_poly, which is also run in the
# gathered form conv3x3_wino(SRC_UP2X)); up: hs x ws is the SOURCE, the conv runs on 2 hs x 2 ws; geo: the tile geometry the case is
# meant to reach (None: either); kind: the group of tests that runs it.
Case = namedtuple("Case", "id kind entry up n cin cout hs ws xmax wmax seed geo")


def conv_size(c):
    return (2 * c.hs, 2 * c.ws) if (c.up or c.entry == "poly") else (c.hs, c.ws)


def _case(table, kind, entry, up, n, cin, cout, hs, ws, geo=None):
    # the value ranges that keep cin x max|U| x max|V| under 2^24 (test_conv_exact_host checks every entry)
    xmax, wmax = (3, 2) if cin <= 128 else (1, 1)
    cid = f"{kind}-{entry}{'-up' if up else ''}-n{n}-c{cin}x{cout}-{hs}x{ws}"
    table.append(Case(cid, kind, entry, up, n, cin, cout, hs, ws, xmax, wmax, 1000 + len(table), geo))


def _build_cases():
    t = []
    cins = (16, 32, 48, 64, 80, 112)

    def channels(i, j):             # a Latin square over the maps: every cin meets every row and column class
        return cins[(i + j) % 6], (32, 96)[(i + j // 2) % 2], (3 if (6 * i + j) % 4 == 1 else 1)

    # one-tile launches around the 8 x 32 tile: direct maps, and sources whose doubled size sits below, on and above it
    for i, h in enumerate((2, 3, 7, 8, 9, 17)):
        for j, w in enumerate((2, 3, 31, 32, 33, 65)):
            cin, cout, n = channels(i, j)
            _case(t, "one", "wino", False, n, cin, cout, h, w)
    for i, h in enumerate((1, 2, 4, 5, 8, 9)):
        for j, w in enumerate((1, 2, 15, 16, 17, 33)):
            cin, cout, n = channels(j, i)
            _case(t, "one", "wino", True, n, cin, cout, h, w)
    # ... and around the 16 x 16 tile, on maps the launcher gives geometry 1.  It never does for H in {15, 16, 17} at W = 17 or 49 nor
    # for H = 17 at W = 48 (the 8 x 32 tiles cover those with as few tiles); their neighbours with a ragged second tile row or a
    # ragged last tile column that do get it: H = 25 and W = 33, 47.
    geo1 = [(15, 15), (15, 16), (15, 33), (15, 47), (15, 48), (16, 15), (16, 16), (16, 33), (16, 47), (16, 48), (17, 15), (17, 16),
            (25, 33), (25, 47), (25, 48)]
    for k, (h, w) in enumerate(geo1):
        cin, cout, n = channels(k % 6, k // 6 + 1)
        _case(t, "one", "wino", False, n, cin, cout, h, w, geo=1)
    for k, (h, w) in enumerate([(7, 8), (8, 8), (9, 8), (8, 17), (8, 24)]):
        cin, cout, n = channels(k, 2)
        _case(t, "one", "wino", True, n, cin, cout, h, w, geo=1)
    _case(t, "one", "wino", False, 1, 256, 160, 9, 33)
    _case(t, "one", "wino", False, 1, 512, 512, 10, 35)

    # persistent launches (on 256 compute units: at least 1024 items; the GPU test asserts it for the device it runs on)
    _case(t, "persist", "wino", False, 1, 32, 128, 125, 509, geo=0)          # ragged, two stages
    _case(t, "persist", "wino", False, 1, 48, 128, 125, 509, geo=0)          # three stages
    _case(t, "persist", "wino", False, 1, 80, 128, 125, 509, geo=0)          # five stages
    _case(t, "persist", "wino", False, 4, 32, 64, 150, 200, geo=1)           # batch
    _case(t, "persist", "wino", False, 1, 256, 160, 9, 3281, geo=0)          # walk group 1 of 5 channel tiles: 2 x 103 ragged tiles
    _case(t, "persist", "wino", True, 1, 64, 64, 125, 255, geo=0)            # gathered 2x upsample of a ragged source

    # cin split: the smallest of test_gpu_split.SPLIT_SHAPES for S = 2, 4, 8
    _case(t, "split", "split", False, 1, 128, 128, 37, 50)
    _case(t, "split", "split", True, 1, 256, 256, 16, 29)
    _case(t, "split", "split", False, 1, 512, 32, 9, 11)

    # polyphase up layers around the 16 x 24 phase-grid tile and its 4-row, 3-column Winograd tiles
    phs, pws = (1, 2, 3, 4, 5, 15, 16, 17, 33), (1, 2, 3, 23, 24, 25, 49)
    for h in phs:
        for w in pws:
            _case(t, "poly", "poly", True, 1, 16, 32, h, w)
    for cin, cout in ((48, 96), (80, 32)):
        for h in phs:
            for w in pws:
                if h in (phs[0], phs[-1]) or w in (pws[0], pws[-1]):
                    _case(t, "poly", "poly", True, 1, cin, cout, h, w)
    _case(t, "poly", "poly", True, 1, 256, 256, 5, 25)
    _case(t, "poly", "poly", True, 3, 48, 96, 17, 25)

    # a ragged three-image batch through each entry point, against its frames one by one
    _case(t, "batch", "wino", False, 3, 48, 96, 19, 37)
    _case(t, "batch", "split", False, 3, 128, 64, 13, 21)
    _case(t, "batch", "poly", True, 3, 32, 64, 9, 26)
    assert len({c.id for c in t}) == len(t)
    return t


CASES = _build_cases()
SPLIT_FACTORS = {"split-split-n1-c128x128-37x50": 2, "split-split-up-n1-c256x256-16x29": 4, "split-split-n1-c512x32-9x11": 8}


def cases(kind):
    return [c for c in CASES if c.kind == kind]


def case_layer(c):
    return int_layer(c.seed, c.cin, c.cout, c.n, c.hs, c.ws, c.xmax, c.wmax)


def forms(c):
    """The transform sets a case runs through: the polyphase entry is also compared with the gathered F(4,3) x F(2,3) form."""
    return ("poly", "f43") if c.entry == "poly" else ("f43",)


# ---- head-room -----------------------------------------------------------------------------------------------------------------------------
def _tile_list(n, ny, nx, whole, seed):
    """(image, tile row, tile column) of every tile (``whole``) or of a seeded sample of 256 plus the four corner tiles of image 0."""
    if whole:
        return [v.ravel() for v in np.meshgrid(np.arange(n), np.arange(ny), np.arange(nx), indexing="ij")]
    rng = np.random.default_rng(seed)
    im, iy, ix = rng.integers(0, n, 256), rng.integers(0, ny, 256), rng.integers(0, nx, 256)
    return (np.concatenate([im, [0, 0, 0, 0]]), np.concatenate([iy, [0, 0, ny - 1, ny - 1]]), np.concatenate([ix, [0, nx - 1, 0, nx - 1]]))


def _measured(x, U, rows, cols, AT, AcT, whole, seed):
    """max over the tiles of sum |A^T| |M| |A| in float64 (x [n][cin][H][W])."""
    im, iy, ix = _tile_list(x.shape[0], len(rows), len(cols), whole, seed)
    worst = 0.0
    for i in np.unique(im):
        k = im == i
        M = _products(x[i], U, rows, cols, iy[k], ix[k], np.float64)
        worst = max(worst, float(np.einsum("ar,torj,bj->toab", np.abs(AT), np.abs(M), np.abs(AcT)).max()))
    return worst


def headroom(c):
    """{form: (a, b)} in float64 for the transform sets the case runs through ("f43": F(4,3) x F(2,3), "poly": the polyphase form).
    (a) cin x max|U| x max|V| with U from the case's own weights and V from its value range: bounds every partial sum of the products,
    in any order and under any split.  (b) the measured sum |A^T| |M| |A| of the output transform over the case's own tiles: all of
    them on maps up to 64 x 64, a seeded sample of 256 plus the four corners beyond."""
    x, w, _ = case_layer(c)
    x = x.double().permute(0, 3, 1, 2).numpy()
    w = w.double().numpy()
    out = {}
    for form in forms(c):
        if form == "f43":
            src = x.repeat(2, axis=2).repeat(2, axis=3) if (c.up or c.entry == "poly") else x
            H, W = src.shape[2:]
            U = pack_f43(w)
            rows, cols = _f43_index(H, W)
            b = _measured(src, U, rows, cols, A4T, A2T, H <= 64 and W <= 64, c.seed)
        else:
            U = pack_poly(w)
            b = 0.0
            for ph in range(4):
                rows, cols = _poly_index(c.hs, c.ws, ph >> 1, ph & 1)
                b = max(b, _measured(x, U[ph], rows, cols, A5T[:4], A3T, c.hs <= 64 and c.ws <= 64, c.seed + ph))
        assert np.array_equal(U, np.rint(U)), "weights that are multiples of 48 pack to integers"
        out[form] = (float(c.cin * np.abs(U).max() * V_GAIN * c.xmax), b)
    return out


# ---- launch arithmetic of the device side (mirrors launch_conv3x3_wino4) -------------------------------------------------------------------
def geometry(c):
    H, W = conv_size(c)
    return arch.wino4_geometry([(c.n, H, W)])


def launch_items(c):
    H, W = conv_size(c)
    th, tw = (16, 16) if geometry(c) else (8, 32)
    return c.n * (-(-H // th)) * (-(-W // tw)) * (c.cout // 32)


def is_persistent(c, cus):
    pgrid = 2 * cus - (2 * cus) % 8
    return launch_items(c) >= 2 * pgrid and c.cin >= 32
