"""Every C-ABI call that launches a kernel, called through ``rt.lib()`` with raw pointers into a guard-band arena (tests/abi_arena.py):
outputs and workspaces of exactly their documented size, regions at the alignment include/adain_hip.h states and no better, two
fills (0xFF bytes; a non-zero position-dependent pattern) of everything that is not an input.  Asserted, all bitwise: no byte outside
the declared outputs and workspaces changes; the outputs do not depend on the fill; they are the bytes the runtime.py wrapper returns
(which the parity tests hold to the references); and the same call after a call of another shape has used the workspace gives them
a third time.  No value tolerance anywhere in this file.

Calls for which the header states no alignment get 256-byte aligned regions (what torch hands out): everything except the TV-L1 frames
and flows (16 B, stated) and the colour workspace (8 B, stated); the Farneback pyramid is taken at the 256 B of its blocks.

Entry point -> cases (every export of the library that launches a kernel; the host-only calls and the size queries are the rest):
  adain_conv3x3_wino                     test_conv3x3_wino: both tile geometries, one-tile and persistent, direct / up / pooled, H or W = 2,
                                         W = 1 and 31 mod 32, H = 1 and 7 mod 8, batch 3, cout 32 and 96; direct, up and pooled at 2 GiB
  adain_conv3x3_wino4_split              test_conv3x3_wino4_split: three split launches, workspace = the slab bytes
  adain_conv3x3_up2x_poly                test_conv3x3_up2x_poly: 1 x 1, 2 x 9, 37 x 53, batch 3, the 2 GiB output
  adain_conv3x3_wino4_pack, _up2x_poly_pack   test_single_layer_packs
  adain_encoder_pack, adain_decoder_pack      test_network_packs_write_every_float_of_the_query
  adain_encode, adain_encode_u8          test_encode, test_encode_u8: 9 x 9, 37 x 99 batch 2, 1080p, two single frames under the latency
                                         schedule; 4096 x 2208 once (uint8)
  adain_encode_relu1_1                   test_encode_relu1_1: 2 x 2, ragged batch 2 (float, uint8), 1080p
  adain_encode_multi                     test_encode_multi: 1, 2 and 4 segments of different sizes
  adain_decode                           test_decode: 2 x 2, 5 x 13 batch 2, 1080p, two latency-schedule frames, 276 x 512
  adain_stylize_u8                       test_stylize_u8: no mask (2 sizes), the two fused tails, the general composite, depth maps, mask_n 1 / n,
                                         byte and float masks
  adain_mean_std                         test_mean_std;  adain_strength_map: test_strength_map
  adain_blend_alpha, adain_blend_pmap    test_blend: NHWC c = 512 and 12, NCHW 64 x 9 x 11 and 32 x 1 x 1; NCHW planes of 15 and 6 floats (a quad
                                         of four elements lies across two images) with one style row, whose neighbours are the changing fill
  adain_resize_bilinear, _nearest        test_resize;  adain_mask_composite: test_mask_composite
  adain_quantize_u8, adain_u8_to_f32     test_quantize_u8_and_u8_to_f32: c = 1, 3, 4 x widths 1, 3, 5, 67
  adain_nhwc_to_nchw, adain_nchw_to_nhwc test_layout_changes
  adain_warp_blend_u8                    test_warp_blend_u8;  adain_resize_area_u8: test_resize_area_u8
  adain_resize_pil_bilinear_u8           test_resize_pil_bilinear_u8: 3 and 4 bytes per pixel, crop or not, shrink and enlarge
  adain_flow_gray_u8                     test_flow_gray_u8: copy, exact 2x, general, enlarged
  adain_farneback_expand, _flow          test_farneback: 37 x 61 and 1080p
  adain_tvl1_prepare, adain_tvl1_flow    test_tvl1: two pairs sharing a frame, iters_out present and NULL
  adain_colour_transfer_u8, adain_localized_combine_u8   test_colour_calls: a case_h case, an empty region, the 1080p block mask,
                                         1 x 7 with three pixels a region (every array of the workspace far below one 256-byte block)"""
import ctypes

import pytest
import torch

import abi_arena as A

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
D, U = 0, 1          # ADAIN_SRC_DIRECT, ADAIN_SRC_UP2X


@pytest.fixture(scope="module")
def rt():
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    import applied_image_processing_amd.runtime as rt

    rt.lib()
    torch.cuda.set_device(0)
    return rt


@pytest.fixture(scope="module")
def packed(rt, weights):
    return rt.pack_encoder(weights[0], torch.device(DEV)), rt.pack_decoder(weights[1], torch.device(DEV))


class Case:
    """The regions of one call, in memory order: inp (a tensor, or f(arena) -> tensor for tables of arena pointers), out, ws."""

    def __init__(self, rt):
        self.rt, self.specs, self.inputs = rt, [], {}

    def inp(self, name, t, align=256, nbytes=None, holes=()):
        self.specs.append((name, t.numel() * t.element_size() if nbytes is None else nbytes, "in", align, holes))
        self.inputs[name] = t
        return self

    def out(self, name, nbytes, align=256, holes=()):
        self.specs.append((name, nbytes, "out", align, holes))
        return self

    def ws(self, name, nbytes, align=256):
        self.specs.append((name, nbytes, "ws", align))
        return self

    def _setup(self, arena):
        for name, t in self.inputs.items():
            arena.put(name, t(arena) if callable(t) else t)

    def run(self, call, history=None, extra=None):
        def checked(fn):
            def go(arena):
                rc = fn(arena)
                assert rc == 0, f"rc {rc}: {self.rt.lib().adain_last_error().decode()}"
            return go
        return A.run_case(self.specs, checked(call), DEV, torch.cuda.synchronize, None if history is None else checked(history),
                          setup=self._setup, extra=extra)


def same(outs, holes=(), **wrapper):
    """The arena call's outputs are the bytes the runtime.py wrapper returned (``holes``: the declared padding of all of them)."""
    torch.cuda.synchronize()
    want = {k: A.as_bytes(v).clone() for k, v in wrapper.items()}
    for v in want.values():
        for a, b in holes:
            v[a:b] = 0
    A.compare_outputs({k: outs[k] for k in wrapper}, want, "the call in the arena", "the runtime wrapper")


def block_holes(blocks, base=0):
    """Byte ranges of the padding behind blocks of ``blocks`` floats, each block starting at a multiple of 64 floats from ``base``."""
    holes, off = [], base
    for floats in blocks:
        end = off + (floats + 63) // 64 * 64
        holes.append((4 * (off + floats), 4 * end))
        off = end
    return [hb for hb in holes if hb[1] > hb[0]], off


def S(rt):
    return rt._stream()


def randn(*shape, seed=0, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(*shape, generator=g) * scale).to(DEV)


def randu8(*shape, seed=0):
    g = torch.Generator().manual_seed(seed)
    return torch.randint(0, 256, shape, generator=g, dtype=torch.uint8).to(DEV)


def ints(*v):
    return (ctypes.c_int * len(v))(*v)


def host_ptrs(*p):
    arr = (ctypes.c_void_p * len(p))(*p)
    return ctypes.cast(arr, ctypes.POINTER(ctypes.c_void_p)), arr


def layer(cin, cout, seed):
    g = torch.Generator().manual_seed(seed)
    w = torch.randn(cout, cin, 3, 3, generator=g) * (2.0 / (9 * cin)) ** 0.5
    return w.to(DEV), (torch.randn(cout, generator=g) * 0.1).to(DEV)


# ---- the harness sees a change on the device ---------------------------------------------------------------------------------------------
def test_a_torch_write_into_a_guard_is_seen(rt):
    specs = [("x", 1024, "in", 256), ("out", 4096, "out", 256)]
    for fill in A.FILLS:
        arena = A.Arena(specs, fill, DEV)
        arena.put("x", randu8(1024))
        arena.bytes("out").zero_()
        arena.check()
        arena.buf[arena.region("out").offset + 4096 + 3] ^= 0x40          # an indexing write by torch, never a kernel
        torch.cuda.synchronize()
        with pytest.raises(A.ArenaViolation) as e:
            arena.check()
        assert e.value.region == "guard after out" and e.value.first == e.value.last == 3 and e.value.count == 1


# ---- adain_conv3x3_wino (form 5), adain_conv3x3_wino4_split, adain_conv3x3_up2x_poly ----------------------------------------------------
WINO = [  # n, h, w (conv size), cin, cout, src_mode, pool_out, geometry, persistent
    (1, 8, 33, 16, 32, D, 0, 0, False),        # W = 1 mod 32
    (1, 2, 63, 16, 32, D, 0, 0, False),        # H = 2, W = 31 mod 32
    (1, 9, 2, 16, 32, D, 1, 1, False),         # W = 2, pooled odd H
    (1, 9, 63, 16, 32, D, 1, 0, False),        # H = 1 mod 8, pooled odd H and W
    (3, 7, 31, 32, 96, D, 1, 0, False),        # batch 3, cout 96, H = 7 mod 8, pooled odd H and W
    (1, 16, 16, 16, 32, U, 0, 1, False),       # 16 x 16 tiles, source upsampled
    (3, 15, 33, 32, 32, D, 1, 1, False),       # 16 x 16 tiles, pooled odd H and W
    (3, 153, 191, 32, 96, D, 0, 0, True),      # persistent, H = 1 mod 8, W = 31 mod 32
    (3, 153, 191, 32, 96, D, 1, 0, True),
    (3, 200, 200, 32, 96, U, 0, 1, True),      # persistent, 16 x 16 tiles, ragged in both
    (3, 201, 201, 32, 96, D, 1, 1, True),
    (1, 2200, 4096, 32, 64, D, 0, 0, True),    # 2 GiB and more: the per-tile descriptors, nothing clamps a store
    (1, 2200, 4096, 16, 64, U, 0, 0, False),   # (16 input channels: the one-tile form of it)
    (1, 2201, 4096, 32, 64, D, 1, 0, True),
]


@pytest.mark.parametrize("n,h,w,cin,cout,mode,pool,geo,persist", WINO)
def test_conv3x3_wino(rt, n, h, w, cin, cout, mode, pool, geo, persist):
    import applied_image_processing_amd.arch as arch

    big = h * w * cout * 4 >= 0x7ffffff0
    th, tw = (16, 16) if geo else (8, 32)
    items = n * -(-h // th) * -(-w // tw) * (cout // 32)
    pgrid = 2 * torch.cuda.get_device_properties(0).multi_processor_count // 8 * 8
    assert (0 if big else arch.wino4_geometry([(n, h, w)])) == geo and (items >= 2 * pgrid and cin >= 32) == persist      # the case is what it says
    hs, ws = (h // 2, w // 2) if mode == U else (h, w)
    oh, ow = ((h + 1) // 2, (w + 1) // 2) if pool else (h, w)
    wt, b = layer(cin, cout, 1)
    x, pk = randn(n, hs, ws, cin, seed=2), rt.conv3x3_wino_pack(wt)
    c = Case(rt).inp("x", x).inp("packed", pk).inp("bias", b).out("out", n * oh * ow * cout * 4)
    outs = c.run(lambda a: rt.lib().adain_conv3x3_wino(a.ptr("x"), a.ptr("out"), a.ptr("packed"), a.ptr("bias"), n, h, w, hs, ws, cin, cout,
                                                       mode, 1, pool, 5, S(rt)))
    same(outs, out=rt.conv3x3_wino(x, pk, b, cout, src_mode=mode, relu=True, pool_out=bool(pool)))


@pytest.mark.parametrize("n,h,w,cin,cout,mode,pool", [(1, 16, 16, 512, 256, D, 0), (1, 9, 31, 256, 64, D, 1), (1, 16, 32, 256, 128, U, 0)])
def test_conv3x3_wino4_split(rt, n, h, w, cin, cout, mode, pool):
    L = rt.lib()
    q = L.adain_conv3x3_wino4_split_workspace_bytes(n, h, w, cin, cout)
    assert q > 0, "the case must be one the latency schedule splits"
    hs, ws = (h // 2, w // 2) if mode == U else (h, w)
    oh, ow = ((h + 1) // 2, (w + 1) // 2) if pool else (h, w)
    wt, b = layer(cin, cout, 3)
    x, pk = randn(n, hs, ws, cin, seed=4), rt.conv3x3_wino_pack(wt)
    c = Case(rt).inp("x", x).inp("packed", pk).inp("bias", b).ws("ws", q).out("out", n * oh * ow * cout * 4)
    h2, hs2 = (h - 4, hs - 2) if mode == U else (h - 3, hs - 3)          # another shape through the same slabs
    q2 = L.adain_conv3x3_wino4_split_workspace_bytes(n, h2, w, cin, cout)
    assert 0 < q2 <= q

    def call(a):
        return L.adain_conv3x3_wino4_split(a.ptr("x"), a.ptr("out"), a.ptr("packed"), a.ptr("bias"), n, h, w, hs, ws, cin, cout, mode, 1, pool,
                                           a.ptr("ws"), q, S(rt))

    def other(a):
        return L.adain_conv3x3_wino4_split(a.ptr("x"), a.ptr("out"), a.ptr("packed"), a.ptr("bias"), n, h2, w, hs2, ws, cin, cout, mode, 1, pool,
                                           a.ptr("ws"), q2, S(rt))
    outs = c.run(call, history=other)
    same(outs, out=rt.conv3x3_wino4_split(x, pk, b, cout, src_mode=mode, relu=True, pool_out=bool(pool)))


@pytest.mark.parametrize("n,hs,ws,cin,cout", [(1, 1, 1, 16, 32), (1, 2, 9, 16, 32), (1, 37, 53, 32, 64), (3, 5, 7, 16, 96), (1, 1100, 2048, 16, 64)])
def test_conv3x3_up2x_poly(rt, n, hs, ws, cin, cout):
    wt, b = layer(cin, cout, 5)
    x, pk = randn(n, hs, ws, cin, seed=6), rt.conv3x3_up2x_poly_pack(wt)
    c = Case(rt).inp("x", x).inp("packed", pk).inp("bias", b).out("out", n * 4 * hs * ws * cout * 4)
    outs = c.run(lambda a: rt.lib().adain_conv3x3_up2x_poly(a.ptr("x"), a.ptr("out"), a.ptr("packed"), a.ptr("bias"), n, hs, ws, cin, cout, 1, S(rt)))
    same(outs, out=rt.conv3x3_up2x_poly(x, pk, b, cout))


# ---- the packs: every float the *_floats query counts is written ---------------------------------------------------------------------
@pytest.mark.parametrize("which", ["wino4", "up2x_poly"])
def test_single_layer_packs(rt, which):
    L = rt.lib()
    cin, cout = 48, 96
    wt, b = layer(cin, cout, 7)
    floats = getattr(L, f"adain_conv3x3_{which}_packed_floats")(cin, cout)
    pack = getattr(L, f"adain_conv3x3_{which}_pack")
    outs = Case(rt).inp("w", wt).out("packed", floats * 4).run(lambda a: pack(a.ptr("w"), a.ptr("packed"), cin, cout, S(rt)))
    same(outs, packed=rt.conv3x3_wino_pack(wt) if which == "wino4" else rt.conv3x3_up2x_poly_pack(wt))
    # a layer run from the arena's pack is the layer run from the wrapper's
    pk = outs["packed"].view(torch.float32)
    x = randn(2, 6, 10, cin, seed=8)
    run = (lambda p: rt.conv3x3_wino(x, p, b, cout)) if which == "wino4" else (lambda p: rt.conv3x3_up2x_poly(x, p, b, cout))
    assert torch.equal(run(pk), run(rt.conv3x3_wino_pack(wt) if which == "wino4" else rt.conv3x3_up2x_poly_pack(wt)))


@pytest.mark.parametrize("net", ["encoder", "decoder"])
def test_network_packs_write_every_float_of_the_query(rt, weights, net):
    L = rt.lib()
    sd, keys = (weights[0], rt.ENC_KEYS) if net == "encoder" else (weights[1], rt.DEC_KEYS)
    wsrc = [sd[f"{k}.weight"].float().to(DEV) for k in keys]
    bsrc = [sd[f"{k}.bias"].float().to(DEV) for k in keys]
    floats = getattr(L, f"adain_{net}_packed_floats")()
    c = Case(rt)
    for i, (w, b) in enumerate(zip(wsrc, bsrc)):
        c.inp(f"w{i}", w).inp(f"b{i}", b)
    c.out("packed", floats * 4)

    def call(a):
        wp, _k1 = host_ptrs(*[a.ptr(f"w{i}") for i in range(len(keys))])
        bp, _k2 = host_ptrs(*[a.ptr(f"b{i}") for i in range(len(keys))])
        return getattr(L, f"adain_{net}_pack")(wp, bp, a.ptr("packed"), S(rt))
    outs = c.run(call)            # equal between the fills: no float of the buffer is left as the caller handed it over
    ref = (rt.pack_encoder if net == "encoder" else rt.pack_decoder)(sd, torch.device(DEV))
    same(outs, packed=ref)
    pk = outs["packed"].view(torch.float32)
    if net == "encoder":
        img = randn(1, 3, 40, 56, seed=9).abs().clamp(0, 1)
        assert torch.equal(rt.encode(img, pk), rt.encode(img, ref))
    else:
        feat = randn(1, 5, 7, 512, seed=9).abs()
        assert torch.equal(rt.decode(feat, pk), rt.decode(feat, ref))


# ---- encoder / decoder ---------------------------------------------------------------------------------------------------------------
ENC_SHAPES = [(1, 9, 9, 0), (2, 37, 99, 0), (1, 1080, 1920, 0), (1, 64, 64, 1), (1, 256, 456, 1)]      # n, h, w, latency schedule


def _encode_case(rt, packed, n, h, w, latency, u8):
    L = rt.lib()
    hc, wc = rt.encoded_size(h, w)
    img = randu8(n, h, w, 3, seed=h) if u8 else randn(n, 3, h, w, seed=h).abs().clamp(0, 1)
    q = L.adain_encode_workspace_bytes(n, h, w)
    fn = L.adain_encode_u8 if u8 else L.adain_encode
    h2, w2 = max(9, h - 5), max(9, w - 3)
    q2 = L.adain_encode_workspace_bytes(n, h2, w2)
    assert 0 < q2 <= q
    c = Case(rt).inp("image", img).inp("packed", packed[0]).ws("ws", q).out("feat", n * hc * wc * 512 * 4)
    with rt.schedule(rt.SCHEDULE_LATENCY if latency else rt.SCHEDULE_BATCH):
        if latency:
            assert L.adain_conv3x3_wino4_split_workspace_bytes(n, (h + 7) // 8, (w + 7) // 8, 256, 512) > 0      # the slab term is live
        outs = c.run(lambda a: fn(a.ptr("image"), a.ptr("feat"), a.ptr("packed"), a.ptr("ws"), q, n, h, w, None, S(rt)),
                     history=lambda a: fn(a.ptr("image"), a.ptr("feat"), a.ptr("packed"), a.ptr("ws"), q2, n, h2, w2, None, S(rt)))
        same(outs, feat=(rt.encode_u8 if u8 else rt.encode)(img, packed[0]))


@pytest.mark.parametrize("n,h,w,latency", ENC_SHAPES)
def test_encode(rt, packed, n, h, w, latency):
    _encode_case(rt, packed, n, h, w, latency, u8=False)


@pytest.mark.parametrize("n,h,w,latency", ENC_SHAPES + [(1, 2208, 4096, 0)])
def test_encode_u8(rt, packed, n, h, w, latency):
    _encode_case(rt, packed, n, h, w, latency, u8=True)


@pytest.mark.parametrize("n,h,w,u8", [(1, 2, 2, 0), (2, 37, 99, 0), (2, 37, 99, 1), (1, 1080, 1920, 1)])
def test_encode_relu1_1(rt, packed, n, h, w, u8):
    img = randu8(n, h, w, 3, seed=h) if u8 else randn(n, 3, h, w, seed=h).abs().clamp(0, 1)
    c = Case(rt).inp("image", img).inp("packed", packed[0]).out("relu1_1", n * h * w * 64 * 4)
    outs = c.run(lambda a: rt.lib().adain_encode_relu1_1(a.ptr("image"), u8, a.ptr("relu1_1"), a.ptr("packed"), n, h, w, S(rt)))
    same(outs, relu1_1=rt.encode_relu1_1(img, packed[0]))


@pytest.mark.parametrize("sizes", [[(1, 37, 99)], [(2, 256, 320), (1, 9, 9)], [(1, 512, 640), (1, 9, 9), (2, 37, 99), (1, 128, 72)]])
def test_encode_multi(rt, packed, sizes):
    L = rt.lib()
    k = len(sizes)
    imgs = [randn(n, 3, h, w, seed=i).abs().clamp(0, 1) for i, (n, h, w) in enumerate(sizes)]
    N, H, W = ints(*[s[0] for s in sizes]), ints(*[s[1] for s in sizes]), ints(*[s[2] for s in sizes])
    q = L.adain_encode_multi_workspace_bytes(k, N, H, W)
    c = Case(rt)
    for i, im in enumerate(imgs):
        c.inp(f"image{i}", im)
    c.inp("packed", packed[0]).ws("ws", q)
    for i, (n, h, w) in enumerate(sizes):
        hc, wc = rt.encoded_size(h, w)
        c.out(f"feat{i}", n * hc * wc * 512 * 4)

    def call(a):
        ip, _k1 = host_ptrs(*[a.ptr(f"image{i}") for i in range(k)])
        fp, _k2 = host_ptrs(*[a.ptr(f"feat{i}") for i in range(k)])
        return L.adain_encode_multi(k, ip, fp, N, H, W, a.ptr("packed"), a.ptr("ws"), q, None, S(rt))

    def other(a):          # the first batch alone, through adain_encode, in the same workspace
        n, h, w = sizes[0]
        return L.adain_encode(a.ptr("image0"), a.ptr("feat0"), a.ptr("packed"), a.ptr("ws"), L.adain_encode_workspace_bytes(n, h, w), n, h, w,
                              None, S(rt))
    outs = c.run(call, history=other)
    same(outs, **{f"feat{i}": f for i, f in enumerate(rt.encode_multi(imgs, packed[0]))})


@pytest.mark.parametrize("n,hc,wc,latency", [(1, 2, 2, 0), (2, 5, 13, 0), (1, 135, 240, 0), (1, 8, 8, 1), (1, 32, 57, 1), (1, 276, 512, 0)])
def test_decode(rt, packed, n, hc, wc, latency):
    L = rt.lib()
    feat = randn(n, hc, wc, 512, seed=hc).abs()
    q = L.adain_decode_workspace_bytes(n, hc, wc)
    hc2 = max(2, hc - 1)
    q2 = L.adain_decode_workspace_bytes(n, hc2, wc)
    assert 0 < q2 <= q
    c = Case(rt).inp("feat", feat).inp("packed", packed[1]).ws("ws", q).out("image", n * 3 * 64 * hc * wc * 4)
    with rt.schedule(rt.SCHEDULE_LATENCY if latency else rt.SCHEDULE_BATCH):
        if latency:
            assert L.adain_conv3x3_wino4_split_workspace_bytes(n, hc, wc, 512, 256) > 0
        outs = c.run(lambda a: L.adain_decode(a.ptr("feat"), a.ptr("image"), a.ptr("packed"), a.ptr("ws"), q, n, hc, wc, None, S(rt)),
                     history=lambda a: L.adain_decode(a.ptr("feat"), a.ptr("image"), a.ptr("packed"), a.ptr("ws"), q2, n, hc2, wc, None, S(rt)))
        same(outs, image=rt.decode(feat, packed[1]))


# ---- adain_stylize_u8 ----------------------------------------------------------------------------------------------------------------
STYLIZE = [  # n, h, w, mask (None | (mask_n, mask_c, mh, mw, is_float)), depth
    (2, 64, 72, None, False),                         # the decoder's last layer quantises
    (2, 37, 99, None, False),                         # output 40 x 104
    (2, 64, 72, (1, 1, 64, 72, 0), False),            # mask at the frame's size, sides multiples of 8: the fused tail
    (2, 64, 72, (2, 3, 31, 45, 1), False),            # mask at another size: the fused tail samples it
    (2, 37, 99, (2, 1, 37, 99, 0), False),            # sides not multiples of 8: bilinear + composite path
    (2, 37, 99, (1, 3, 20, 50, 1), True),             # the same with a resized float mask and depth maps
    (1, 64, 72, None, True),
]


@pytest.mark.parametrize("n,h,w,mask,depth", STYLIZE)
def test_stylize_u8(rt, packed, n, h, w, mask, depth):
    L = rt.lib()
    frames = randu8(n, h, w, 3, seed=11)
    s_mean, s_std = randn(1, 512, seed=12), randn(1, 512, seed=13).abs() + 0.1
    c = Case(rt).inp("frames", frames).inp("enc", packed[0]).inp("dec", packed[1]).inp("s_mean", s_mean).inp("s_std", s_std)
    mn = mc = mh = mw = mf = 0
    m = None
    if mask is not None:
        mn, mc, mh, mw, mf = mask
        m = (randn(mn, mc, mh, mw, seed=14) > 0)
        m = m.float() if mf else m.to(torch.uint8)
        c.inp("mask", m)
    dmaps = [randn(23 + i, 31, seed=15 + i).abs() for i in range(n)] if depth else None
    for i, d in enumerate(dmaps or []):
        c.inp(f"depth{i}", d)
    oh, ow = ctypes.c_int(), ctypes.c_int()
    L.adain_stylize_u8_out_size(h, w, int(mask is not None), ctypes.byref(oh), ctypes.byref(ow))
    q = L.adain_stylize_u8_workspace_bytes(n, h, w, int(depth), mn, mc, mh, mw, mf)
    q2 = L.adain_stylize_u8_workspace_bytes(n, h - 8, w, 0, 0, 0, 0, 0, 0)
    assert 0 < q2 <= q
    c.ws("ws", q).out("out", n * oh.value * ow.value * 3)

    def call(a):
        dp, _k = host_ptrs(*[a.ptr(f"depth{i}") for i in range(n)]) if depth else (None, None)
        dh, dw = (ints(*[d.shape[0] for d in dmaps]), ints(*[d.shape[1] for d in dmaps])) if depth else (None, None)
        return L.adain_stylize_u8(a.ptr("frames"), n, h, w, a.ptr("enc"), a.ptr("dec"), a.ptr("s_mean"), a.ptr("s_std"), 0.5, 0.5, dp, dh, dw,
                                  0.15, 20.0, a.ptr("mask") if m is not None else None, mf, mn, mc, mh, mw, a.ptr("out"), a.ptr("ws"), q, S(rt))

    def other(a):          # shorter frames, no mask, no depth: every block of the carve lands elsewhere
        return L.adain_stylize_u8(a.ptr("frames"), n, h - 8, w, a.ptr("enc"), a.ptr("dec"), a.ptr("s_mean"), a.ptr("s_std"), 0.5, 0.5, None, None,
                                  None, 0.15, 20.0, None, 0, 0, 0, 0, 0, a.ptr("out"), a.ptr("ws"), q2, S(rt))
    outs = c.run(call, history=other)
    same(outs, out=rt.stylize_u8(frames, packed[0], packed[1], s_mean, s_std, alpha=0.5, depth_maps=dmaps, mask=m))


# ---- statistics, blend, strength map ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nhwc,n,c,h,w", [(1, 2, 512, 1, 1), (0, 2, 64, 1, 1), (1, 2, 512, 64, 80), (0, 3, 64, 128, 130), (1, 1, 32, 3, 5)])
def test_mean_std(rt, nhwc, n, c, h, w):
    L = rt.lib()
    x = randn(n, h, w, c, seed=20) if nhwc else randn(n, c, h, w, seed=20)
    q = L.adain_mean_std_workspace_bytes(nhwc, n, c, h * w)
    q2 = L.adain_mean_std_workspace_bytes(nhwc, 1, c, h * w)
    assert q2 <= q
    cs = Case(rt).inp("x", x).ws("ws", q).out("mean", n * c * 4).out("std", n * c * 4)
    outs = cs.run(lambda a: L.adain_mean_std(a.ptr("x"), nhwc, n, c, h * w, 1e-5, a.ptr("mean"), a.ptr("std"), a.ptr("ws"), q, S(rt)),
                  history=lambda a: L.adain_mean_std(a.ptr("x"), nhwc, 1, c, h * w, 1e-5, a.ptr("mean"), a.ptr("std"), a.ptr("ws"), q2, S(rt)))
    mean, std = rt.mean_std(x, bool(nhwc))
    same(outs, mean=mean, std=std)


@pytest.mark.parametrize("nhwc,n,c,h,w,style_n,pmap_n", [(1, 3, 512, 5, 7, 1, 0), (1, 3, 512, 5, 7, 3, 1), (0, 2, 64, 9, 11, 2, 2), (0, 2, 32, 1, 1, 1, 0),
                                                          (0, 4, 3, 1, 5, 1, 4), (0, 2, 3, 1, 2, 1, 0), (1, 3, 12, 1, 5, 1, 3)])
def test_blend(rt, nhwc, n, c, h, w, style_n, pmap_n):
    L = rt.lib()
    x = randn(n, h, w, c, seed=21) if nhwc else randn(n, c, h, w, seed=21)
    cm, cstd = randn(n, c, seed=22), randn(n, c, seed=23).abs() + 0.1
    sm, sstd = randn(style_n, c, seed=24), randn(style_n, c, seed=25).abs() + 0.1
    cs = Case(rt).inp("x", x).inp("c_mean", cm).inp("c_std", cstd).inp("s_mean", sm).inp("s_std", sstd)
    if pmap_n:
        p = randn(pmap_n, h, w, seed=26).sigmoid()
        cs.inp("pmap", p).out("out", x.numel() * 4)
        outs = cs.run(lambda a: L.adain_blend_pmap(a.ptr("x"), nhwc, n, c, h * w, a.ptr("c_mean"), a.ptr("c_std"), a.ptr("s_mean"), a.ptr("s_std"),
                                                   style_n, a.ptr("pmap"), pmap_n, a.ptr("out"), S(rt)))
        same(outs, out=rt.blend_pmap(x, bool(nhwc), cm, cstd, sm, sstd, p))
    else:
        cs.out("out", x.numel() * 4)
        outs = cs.run(lambda a: L.adain_blend_alpha(a.ptr("x"), nhwc, n, c, h * w, a.ptr("c_mean"), a.ptr("c_std"), a.ptr("s_mean"), a.ptr("s_std"),
                                                    style_n, 0.7, float(1 - 0.7), a.ptr("out"), S(rt)))
        same(outs, out=rt.blend_alpha(x, bool(nhwc), cm, cstd, sm, sstd, 0.7))


@pytest.mark.parametrize("h0,w0,hc,wc", [(23, 31, 5, 13), (480, 640, 64, 80), (7, 5, 1, 1)])
def test_strength_map(rt, h0, w0, hc, wc):
    L = rt.lib()
    depth = randn(h0, w0, seed=27).abs()
    q = L.adain_strength_map_workspace_bytes(hc, wc)
    cs = Case(rt).inp("depth", depth).ws("ws", q).out("pmap", hc * wc * 4)
    outs = cs.run(lambda a: L.adain_strength_map(a.ptr("depth"), h0, w0, hc, wc, 0.15, 20.0, a.ptr("pmap"), a.ptr("ws"), q, S(rt)),
                  history=lambda a: L.adain_strength_map(a.ptr("depth"), h0, w0, 1, 1, 0.15, 20.0, a.ptr("pmap"), a.ptr("ws"),
                                                         L.adain_strength_map_workspace_bytes(1, 1), S(rt)))
    same(outs, pmap=rt.strength_map(depth, hc, wc, 0.15, 20.0))


# ---- pixel kernels -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["bilinear", "nearest"])
@pytest.mark.parametrize("planes,hi,wi,ho,wo", [(6, 40, 104, 37, 99), (3, 5, 7, 13, 1), (1, 1, 1, 3, 5), (2, 67, 3, 5, 67)])
def test_resize(rt, kind, planes, hi, wi, ho, wo):
    x = randn(1, planes, hi, wi, seed=30)
    fn = getattr(rt.lib(), f"adain_resize_{kind}")
    outs = Case(rt).inp("x", x).out("out", planes * ho * wo * 4).run(lambda a: fn(a.ptr("x"), a.ptr("out"), planes, hi, wi, ho, wo, S(rt)))
    same(outs, out=getattr(rt, f"resize_{kind}")(x, (ho, wo)))


@pytest.mark.parametrize("n,c,h,w,mn,mc", [(2, 3, 37, 99, 1, 1), (2, 3, 37, 99, 2, 3), (1, 3, 1, 5, 1, 3), (3, 3, 8, 67, 3, 1)])
def test_mask_composite(rt, n, c, h, w, mn, mc):
    content, sty, m = randn(n, c, h, w, seed=31), randn(n, c, h, w, seed=32), (randn(mn, mc, h, w, seed=33) > 0).float()
    cs = Case(rt).inp("content", content).inp("stylized", sty).inp("mask", m).out("out", n * c * h * w * 4)
    outs = cs.run(lambda a: rt.lib().adain_mask_composite(a.ptr("content"), a.ptr("stylized"), a.ptr("mask"), mc, mn, a.ptr("out"), n, c, h * w, S(rt)))
    same(outs, out=rt.mask_composite(content, sty, m))


@pytest.mark.parametrize("c", [1, 3, 4])
@pytest.mark.parametrize("w", [1, 3, 5, 67])
def test_quantize_u8_and_u8_to_f32(rt, c, w):
    n, h = 2, 3
    img = randn(n, c, h, w, seed=34) * 0.5 + 0.5
    outs = Case(rt).inp("image", img).out("out", n * h * w * c).run(
        lambda a: rt.lib().adain_quantize_u8(a.ptr("image"), a.ptr("out"), n, c, h, w, S(rt)))
    same(outs, out=rt.quantize_u8(img))
    u8 = randu8(n, h, w, c, seed=35)
    outs = Case(rt).inp("frames", u8).out("out", n * c * h * w * 4).run(
        lambda a: rt.lib().adain_u8_to_f32(a.ptr("frames"), a.ptr("out"), n, c, h, w, S(rt)))
    same(outs, out=rt.u8_to_f32(u8))


@pytest.mark.parametrize("n,c,h,w", [(2, 512, 5, 13), (1, 3, 37, 99), (3, 64, 1, 1), (1, 1, 1, 67)])
def test_layout_changes(rt, n, c, h, w):
    x = randn(n, h, w, c, seed=36)
    outs = Case(rt).inp("x", x).out("out", x.numel() * 4).run(lambda a: rt.lib().adain_nhwc_to_nchw(a.ptr("x"), a.ptr("out"), n, c, h * w, S(rt)))
    same(outs, out=rt.nhwc_to_nchw(x))
    y = randn(n, c, h, w, seed=37)
    outs = Case(rt).inp("x", y).out("out", y.numel() * 4).run(lambda a: rt.lib().adain_nchw_to_nhwc(a.ptr("x"), a.ptr("out"), n, c, h * w, S(rt)))
    same(outs, out=rt.nchw_to_nhwc(y))


# ---- video post-pass and resizes on uint8 --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("h,w,c", [(36, 64, 3), (37, 61, 3), (5, 7, 1)])
def test_warp_blend_u8(rt, h, w, c):
    cur, prev = randu8(h, w, c, seed=40), randu8(h, w, c, seed=41)
    flow = randn(2, h, w, seed=42, scale=0.6 * max(h, w))          # many vectors leave the frame
    cs = Case(rt).inp("cur", cur).inp("prev", prev).inp("flow", flow).out("out", h * w * c)
    outs = cs.run(lambda a: rt.lib().adain_warp_blend_u8(a.ptr("cur"), a.ptr("prev"), a.ptr("flow"), a.ptr("out"), h, w, c, 0.6, float(1 - 0.6), S(rt)))
    same(outs, out=rt.warp_blend_u8(cur, prev, flow, 0.6))


@pytest.mark.parametrize("n,hi,wi,c,ho,wo", [(2, 37, 61, 3, 37, 61), (2, 74, 122, 3, 37, 61), (1, 111, 244, 3, 37, 61), (2, 100, 99, 3, 37, 61),
                                             (1, 100, 30, 3, 37, 61), (1, 9, 9, 1, 3, 4)])
def test_resize_area_u8(rt, n, hi, wi, c, ho, wo):
    x = randu8(n, hi, wi, c, seed=43)
    outs = Case(rt).inp("in", x).out("out", n * ho * wo * c).run(
        lambda a: rt.lib().adain_resize_area_u8(a.ptr("in"), a.ptr("out"), n, hi, wi, c, ho, wo, S(rt)))
    same(outs, out=rt.resize_area_u8(x, (wo, ho)))


@pytest.mark.parametrize("pix,n,hi,wi,ho,wo,crop", [(3, 2, 100, 133, 37, 61, None), (4, 2, 100, 133, 37, 61, (3, 5, 30, 51)), (3, 1, 20, 31, 64, 99, None),
                                                    (4, 1, 20, 31, 64, 99, (0, 19, 64, 64)), (3, 1, 1080, 1920, 256, 455, (0, 99, 256, 256))])
def test_resize_pil_bilinear_u8(rt, pix, n, hi, wi, ho, wo, crop):
    L = rt.lib()
    x = randu8(n, hi, wi, pix, seed=44)
    y0, x0, ch, cw = crop or (0, 0, ho, wo)
    q = L.adain_resize_pil_bilinear_u8_workspace_bytes(hi, wi, ho, wo)
    q2 = L.adain_resize_pil_bilinear_u8_workspace_bytes(hi - 1, wi - 1, ho, wo)
    assert 0 < q2 <= q
    cs = Case(rt).inp("in", x).ws("ws", q).out("out", n * ch * cw * 3)
    outs = cs.run(lambda a: L.adain_resize_pil_bilinear_u8(a.ptr("in"), pix, n, hi, wi, a.ptr("out"), ho, wo, y0, x0, ch, cw, a.ptr("ws"), q, S(rt)),
                  history=lambda a: L.adain_resize_pil_bilinear_u8(a.ptr("in"), pix, 1, hi - 1, wi - 1, a.ptr("out"), ho, wo, y0, x0, ch, cw,
                                                                   a.ptr("ws"), q2, S(rt)))
    same(outs, out=rt.resize_pil_bilinear_u8(x, (wo, ho), crop=crop))


# ---- optical flow ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,hi,wi,ho,wo", [(2, 37, 61, 37, 61), (2, 74, 122, 37, 61), (1, 100, 133, 37, 61), (1, 20, 31, 37, 61)])
def test_flow_gray_u8(rt, n, hi, wi, ho, wo):
    import applied_image_processing_amd.flow as flow

    x = randu8(n, hi, wi, 3, seed=50)
    outs = Case(rt).inp("rgb", x).out("gray", n * ho * wo).run(
        lambda a: rt.lib().adain_flow_gray_u8(a.ptr("rgb"), n, hi, wi, a.ptr("gray"), ho, wo, S(rt)))
    same(outs, gray=flow.frames_to_gray(x, (wo, ho)))


def _smooth_u8(h, w, seed):
    y, x = torch.meshgrid(torch.arange(h, dtype=torch.float32), torch.arange(w, dtype=torch.float32), indexing="ij")
    v = 128 + 60 * torch.sin(x / 7 + seed) * torch.cos(y / 5 - seed) + 40 * torch.sin((x + 2 * y) / 11 + 2 * seed)
    return v.clamp(0, 255).to(torch.uint8).to(DEV)


@pytest.mark.parametrize("h,w", [(37, 61), (1080, 1920)])
def test_farneback(rt, h, w):
    import applied_image_processing_amd.flow as flow

    L = rt.lib()
    fb = flow.Farneback(h, w)
    g0, g1 = _smooth_u8(h, w, 0.0), _smooth_u8(h, w, 0.3)
    pb, q = L.adain_farneback_pyramid_bytes(h, w, 0.5, 5), L.adain_farneback_workspace_bytes(h, w)
    assert pb == fb.pyr_bytes and q == fb.ws_bytes
    h2, w2 = h - 5, w - 3
    q2 = L.adain_farneback_workspace_bytes(h2, w2)
    pb2 = L.adain_farneback_pyramid_bytes(h2, w2, 0.5, 5)
    assert 0 < q2 <= q and 0 < pb2 <= pb
    # the padding behind the pyramid's 256-byte aligned blocks is not part of the result: never written, never read
    pyr_holes = lambda hh, ww: block_holes([f for (wl, hl, _k, _s) in flow.level_schedule(hh, ww, 0.5, 5) for f in (wl * hl, 5 * wl * hl)])
    holes, floats = pyr_holes(h, w)
    assert 4 * floats == pb
    # (the other shape's pyramid has its blocks elsewhere: it goes to a region of its own, which no assertion reads)
    cs = Case(rt).inp("gray", g0).ws("ws", q).out("pyramid", pb, holes=holes).ws("other pyramid", pb2)
    outs = cs.run(lambda a: L.adain_farneback_expand(a.ptr("gray"), h, w, 0.5, 5, 7, 1.5, a.ptr("pyramid"), a.ptr("ws"), q, S(rt)),
                  history=lambda a: L.adain_farneback_expand(a.ptr("gray"), h2, w2, 0.5, 5, 7, 1.5, a.ptr("other pyramid"), a.ptr("ws"), q2, S(rt)))
    p0, p1 = fb.expand(g0), fb.expand(g1)
    same(outs, holes=holes, pyramid=p0)
    fb2 = flow.Farneback(h2, w2)
    s0, s1 = fb2.expand(g0[:h2, :w2].contiguous()), fb2.expand(g1[:h2, :w2].contiguous())      # a smaller pair through the same workspace
    holes2 = pyr_holes(h2, w2)[0]
    cs = (Case(rt).inp("prev", p0, holes=holes).inp("next", p1, holes=holes).inp("prev2", s0, holes=holes2).inp("next2", s1, holes=holes2)
          .ws("ws", q).out("flow", 2 * h * w * 4))
    outs = cs.run(lambda a: L.adain_farneback_flow(a.ptr("prev"), a.ptr("next"), h, w, 0.5, 5, 15, 3, 0, a.ptr("flow"), a.ptr("ws"), q, S(rt)),
                  history=lambda a: L.adain_farneback_flow(a.ptr("prev2"), a.ptr("next2"), h2, w2, 0.5, 5, 15, 3, 0, a.ptr("flow"), a.ptr("ws"), q2, S(rt)))
    same(outs, flow=fb.flow(p0, p1))


@pytest.mark.parametrize("h,w,with_iters", [(37, 61, True), (37, 61, False), (120, 160, True)])
def test_tvl1(rt, h, w, with_iters):
    import applied_image_processing_amd.tvl1 as tvl1

    L = rt.lib()
    tv = tvl1.TVL1(h, w, nscales=3, warps=2, outerIterations=3, innerIterations=10)
    P = ctypes.addressof(tv.P)
    grays = torch.stack([_smooth_u8(h, w, 0.2 * i) for i in range(3)])
    fbytes = L.adain_tvl1_frame_bytes(h, w, P)
    assert fbytes == tv.frame_bytes
    # the frames exactly frame_bytes apart, at the 16 bytes the header asks of them
    # the padding behind a frame's 256-byte aligned scale blocks is not part of the result: never written, never read
    holes, floats = [], 0
    for _frame in range(3):
        hb, floats = block_holes([4 * ws_ * hs_ for (ws_, hs_) in tv.scales], floats)
        holes += hb
    assert 4 * floats == 3 * fbytes
    outs = Case(rt).inp("gray", grays).out("prepared", 3 * fbytes, align=16, holes=holes).run(
        lambda a: L.adain_tvl1_prepare(a.ptr("gray"), 3, h, w, P, a.ptr("prepared"), S(rt)))
    prep = tv.prepare(grays)
    same(outs, holes=holes, prepared=prep)
    npairs = 2                                                               # (0 -> 1), (1 -> 2): frame 1 is in both
    q, q1 = L.adain_tvl1_workspace_bytes(h, w, npairs, P), L.adain_tvl1_workspace_bytes(h, w, 1, P)
    assert 0 < q1 <= q
    nit = npairs * len(tv.scales) * tv.P.warps

    def table(a):
        base = a.ptr("frames")
        return torch.tensor([base, base + fbytes, base + fbytes, base + 2 * fbytes], dtype=torch.int64)
    cs = Case(rt).inp("frames", prep, align=16, holes=holes).inp("table", table, nbytes=32).ws("ws", q).out("flows", npairs * 2 * h * w * 4, align=16)
    if with_iters:
        cs.out("iters", nit * 4)
    outs = cs.run(lambda a: L.adain_tvl1_flow(a.ptr("table"), a.ptr("table") + 16, npairs, h, w, P, a.ptr("flows"),
                                              a.ptr("iters") if with_iters else None, a.ptr("ws"), q, S(rt)),
                  history=lambda a: L.adain_tvl1_flow(a.ptr("table") + 8, a.ptr("table") + 24, 1, h, w, P, a.ptr("flows"), None, a.ptr("ws"), q1, S(rt)))
    iters = torch.empty((npairs, len(tv.scales), tv.P.warps), dtype=torch.int32, device=DEV)
    flows = tv.flows([prep[0], prep[1]], [prep[1], prep[2]], iters_out=iters)
    same(outs, flows=flows, **({"iters": iters} if with_iters else {}))


# ---- the localized pipeline's colour calls: the record at the start of the workspace is an output, the rest scratch ---------------------
def _colour_cases():
    import numpy as np
    from golden.make_golden_localized import case_inputs

    content, stylised, m = case_inputs("disc_96x128")
    yield "case_h", content, stylised, m
    yield "empty", content, stylised, np.ones_like(m)                         # background everywhere: the foreground region is empty
    rng = np.random.default_rng(5)
    h, w = 1080, 1920
    blocks = (rng.random((h // 8, w // 8)) < 0.4).astype(np.uint8)
    yield "1080p", rng.integers(1, 256, (h, w, 3), dtype=np.uint8), rng.integers(1, 256, (h, w, 3), dtype=np.uint8), np.kron(blocks, np.ones((8, 8), np.uint8))
    import colour_fixtures

    yield ("n3_n3",) + colour_fixtures.combine_fixture("n3_n3")              # hw = 7: key and sort arrays of 56 bytes


@pytest.mark.parametrize("which", ["case_h", "empty", "1080p", "n3_n3"])
def test_colour_calls(rt, which):
    L = rt.lib()
    name, content, stylised, m = next(c for c in _colour_cases() if c[0] == which)
    content, stylised, m = (torch.from_numpy(v.copy()).to(DEV) for v in (content, stylised, m))
    h, w = m.shape
    q = L.adain_colour_transfer_workspace_bytes(h, w)
    assert q >= rt.COLOUR_RECORD_BYTES
    h2, w2 = (h - 8, w) if h > 8 else (h, w - 3)                              # the other shape that used the workspace before
    record = lambda a: {"record": a.bytes("ws")[:rt.COLOUR_RECORD_BYTES].clone()}
    cs = Case(rt).inp("content", content).inp("stylised", stylised).inp("mask", m).ws("ws", q, align=8).out("out", h * w * 3)
    outs = cs.run(lambda a: L.adain_localized_combine_u8(a.ptr("content"), a.ptr("stylised"), a.ptr("mask"), a.ptr("out"), h, w, a.ptr("ws"), S(rt)),
                  history=lambda a: L.adain_colour_transfer_u8(a.ptr("content"), a.ptr("stylised"), a.ptr("out"), h2, w2, a.ptr("ws"), S(rt)),
                  extra=record)
    out, rec = rt.localized_combine_u8(content, stylised, m)
    same(outs, out=out, record=rec)
    fg, bg = content * (1 - m)[..., None], stylised * m[..., None]
    cs = Case(rt).inp("fg", fg).inp("bg", bg).ws("ws", q, align=8).out("out", h * w * 3)
    outs = cs.run(lambda a: L.adain_colour_transfer_u8(a.ptr("fg"), a.ptr("bg"), a.ptr("out"), h, w, a.ptr("ws"), S(rt)),
                  history=lambda a: L.adain_colour_transfer_u8(a.ptr("bg"), a.ptr("fg"), a.ptr("out"), h2, w2, a.ptr("ws"), S(rt)), extra=record)
    out, rec = rt.colour_transfer_u8(fg, bg)
    same(outs, out=out, record=rec)
