"""The style-interpolation entries of the C ABI under the guard-band arena of tests/abi_arena.py (see tests/test_gpu_abi_memory.py), in
the manner of tests/test_gpu_coral_arena.py: ``adain_blend_mix`` writes ``out`` and nothing else - with the statistics, the weights
and the strength map at 4-byte alignment where the kernel reads them as scalars, 16 where it reads quads - and ``adain_stylize_u8_mix``
writes ``out`` and its workspace and nothing else; stale bytes (the 0xFF fill, the pattern fill, another shape's intermediates) do not
change a byte of either result.  Run with ``-m gpu``."""
import ctypes

import pytest
import torch

from test_gpu_abi_memory import Case, S, host_ptrs, ints, packed, randn, randu8, rt, same  # noqa: F401  (rt, packed: fixtures)

pytestmark = pytest.mark.gpu

# nhwc, n, c, hw, k, weights_n, maps, pmap_n (0: alpha form)
BLEND_MIX = [
    (True, 2, 512, 35, 2, 2, False, 0),          # the product branch, a row per frame
    (True, 2, 512, 35, 16, 1, True, 2),          # sixteen styles, weight maps, strength maps
    (True, 3, 12, 5, 3, 3, True, 1),             # the flat NHWC kernel
    (False, 4, 3, 5, 5, 1, False, 4),            # NCHW, quads across images
    (False, 2, 64, 99, 2, 2, True, 0),
]


@pytest.mark.parametrize("nhwc,n,c,hw,k,wn,maps,pn", BLEND_MIX)
def test_blend_mix(rt, nhwc, n, c, hw, k, wn, maps, pn):
    L = rt.lib()
    x = randn(n, 1, hw, c, seed=1) if nhwc else randn(n, c, 1, hw, seed=1)
    cm, cs = randn(n, c, seed=2), randn(n, c, seed=3).abs() + 0.5
    sm, ss = randn(k, c, seed=4), randn(k, c, seed=5).abs() + 0.5
    whw = hw if maps else 1
    w = torch.rand(wn, k, whw, generator=torch.Generator().manual_seed(6)).to(x.device) * 0.85 + 0.05
    p = (torch.rand(max(pn, 1), hw, generator=torch.Generator().manual_seed(7)) * 0.85).to(x.device)
    quad = 16 if nhwc else 4                      # NHWC reads the statistics as quads of channels
    case = (Case(rt).inp("x", x, align=16).inp("cm", cm, align=quad).inp("cs", cs, align=quad).inp("sm", sm, align=quad).inp("ss", ss, align=quad)
            .inp("w", w, align=4).inp("p", p, align=4).out("out", x.numel() * 4, align=16))

    def call(a):
        return L.adain_blend_mix(a.ptr("x"), int(nhwc), n, c, hw, a.ptr("cm"), a.ptr("cs"), a.ptr("sm"), a.ptr("ss"), k, a.ptr("w"), wn, whw, 0.6,
                                 float(1 - 0.6), a.ptr("p") if pn else None, pn or 1, a.ptr("out"), S(rt))

    outs = case.run(call)
    wt = w.view((wn, k, 1, hw) if maps else (wn, k))
    if wn == 1 and n > 1:
        wt = wt[0]
    want = rt.blend_mix(x, nhwc, cm, cs, sm, ss, wt.contiguous(), alpha=None if pn else 0.6, pmap=p if pn else None)
    same(outs, out=want)


@pytest.mark.parametrize("depth,mask,k,wn,maps", [(False, None, 2, 3, False), (True, (3, 1, 64, 80, 0), 3, 1, True), (False, (1, 3, 31, 45, 1), 16, 3, True)])
def test_stylize_u8_mix(rt, packed, depth, mask, k, wn, maps):
    L = rt.lib()
    n, h, w = 3, 64, 80
    hc, wc = rt.encoded_size(h, w)
    frames = randu8(n, h, w, 3, seed=31)
    s_mean, s_std = randn(k, 512, seed=32), randn(k, 512, seed=33).abs() + 0.1
    whw = hc * wc if maps else 1
    wts = torch.rand(wn, k, whw, generator=torch.Generator().manual_seed(36)).to(frames.device) * 0.85 / k + 0.05 / k
    c = Case(rt).inp("frames", frames).inp("enc", packed[0]).inp("dec", packed[1]).inp("s_mean", s_mean).inp("s_std", s_std).inp("wts", wts, align=4)
    mn = mc = mh = mw = mf = 0
    m = None
    if mask is not None:
        mn, mc, mh, mw, mf = mask
        m = (randn(mn, mc, mh, mw, seed=34) > 0)
        m = m.float() if mf else m.to(torch.uint8)
        c.inp("mask", m)
    dmaps = [randn(23 + i, 31, seed=35 + i).abs() for i in range(n)] if depth else None
    for i, d in enumerate(dmaps or []):
        c.inp(f"depth{i}", d)
    oh, ow = ctypes.c_int(), ctypes.c_int()
    L.adain_stylize_u8_out_size(h, w, int(mask is not None), ctypes.byref(oh), ctypes.byref(ow))
    q = L.adain_stylize_u8_mix_workspace_bytes(n, h, w, int(depth), mn, mc, mh, mw, mf)
    assert q == L.adain_stylize_u8_workspace_bytes(n, h, w, int(depth), mn, mc, mh, mw, mf) > 0
    q2 = L.adain_stylize_u8_mix_workspace_bytes(n, h - 8, w, 0, 0, 0, 0, 0, 0)
    c.ws("ws", q).out("out", n * oh.value * ow.value * 3)

    def call(a):
        dp, _k = host_ptrs(*[a.ptr(f"depth{i}") for i in range(n)]) if depth else (None, None)
        dh, dw = (ints(*[d.shape[0] for d in dmaps]), ints(*[d.shape[1] for d in dmaps])) if depth else (None, None)
        return L.adain_stylize_u8_mix(a.ptr("frames"), n, h, w, a.ptr("enc"), a.ptr("dec"), a.ptr("s_mean"), a.ptr("s_std"), k, a.ptr("wts"), wn, whw,
                                      0.5, 0.5, dp, dh, dw, 0.15, 20.0, a.ptr("mask") if m is not None else None, mf, mn, mc, mh, mw, a.ptr("out"),
                                      a.ptr("ws"), q, S(rt))

    def other(a):          # shorter frames, one style through the single-style entry, no mask, no depth: every block of the carve lands elsewhere
        return L.adain_stylize_u8_ex(a.ptr("frames"), n, h - 8, w, a.ptr("enc"), a.ptr("dec"), a.ptr("s_mean"), a.ptr("s_std"), 1, 0.5, 0.5, None,
                                     None, None, 0.15, 20.0, None, 0, 0, 0, 0, 0, a.ptr("out"), a.ptr("ws"), q2, S(rt))
    outs = c.run(call, history=other)
    wt = wts.view((wn, k, hc, wc) if maps else (wn, k))
    if wn == 1:
        wt = wt[0]
    same(outs, out=rt.stylize_u8(frames, packed[0], packed[1], s_mean, s_std, alpha=0.5, depth_maps=dmaps, mask=m, style_weights=wt.contiguous()))
