"""The colour-preserving path's C-ABI entries under the guard-band arena of tests/abi_arena.py (see tests/test_gpu_abi_memory.py):
``adain_coral`` writes ``out``, the records at the head of its workspace and the rest of the workspace, nothing else, with each
region at the alignment the header states for it and no better (uint8 images at odd addresses, float images and ``out`` at 4 bytes,
the workspace at 8), and stale workspace bytes - the 0xFF fill, the pattern fill, another shape's partial sums - do not change a byte
of the result; ``adain_stylize_u8_ex`` the same with one style per frame.  Run with ``-m gpu``."""
import ctypes

import pytest
import torch

from test_gpu_abi_memory import Case, S, host_ptrs, ints, packed, randn, randu8, rt, same  # noqa: F401  (rt, packed: fixtures)

pytestmark = pytest.mark.gpu

# style n, h, w, form; content n, h, w, form
CORAL = [
    (1, 1, 2, "u8", 1, 3, 5, "u8"),
    (3, 33, 67, "u8", 3, 7, 9, "f32"),
    (1, 67, 129, "f32", 3, 33, 67, "u8"),
    (3, 200, 333, "f32", 3, 67, 129, "f32"),
    (2, 200, 332, "u8", 2, 200, 333, "u8"),
]


def _image(k, h, w, form, seed):
    u8 = randu8(k, h, w, 3, seed=seed)
    return u8 if form == "u8" else u8.permute(0, 3, 1, 2).float().div(255).contiguous()


@pytest.mark.parametrize("sn,hs,ws,sf,n,hc,wc,cf", CORAL)
def test_coral(rt, sn, hs, ws, sf, n, hc, wc, cf):
    L = rt.lib()
    style, content = _image(sn, hs, ws, sf, 21), _image(n, hc, wc, cf, 22)
    q = L.adain_coral_workspace_bytes(n, sn, hs, ws, hc, wc)
    assert q >= n * rt.CORAL_RECORD_BYTES
    # the call that used the workspace before: the two sides swapped where the counts allow it, another size otherwise
    swap = sn == n
    q2 = L.adain_coral_workspace_bytes(n, sn, hc, wc, hs, ws) if swap else L.adain_coral_workspace_bytes(n, sn, hs, ws, hc, max(1, wc - 1))
    nrec = n * rt.CORAL_RECORD_BYTES
    hw_out = max(hs * ws, hc * wc if swap else 0)
    c = (Case(rt).inp("style", style, align=1 if sf == "u8" else 4).inp("content", content, align=1 if cf == "u8" else 4)
         .ws("ws", max(q, q2), align=8).out("out", n * 3 * hs * ws * 4, align=4).ws("out2", n * 3 * hw_out * 4, align=4))

    def call(a):
        return L.adain_coral(a.ptr("style"), int(sf == "u8"), sn, hs, ws, a.ptr("content"), int(cf == "u8"), n, hc, wc, a.ptr("out"), a.ptr("ws"), q, S(rt))

    def other(a):
        if swap:
            return L.adain_coral(a.ptr("content"), int(cf == "u8"), n, hc, wc, a.ptr("style"), int(sf == "u8"), n, hs, ws, a.ptr("out2"), a.ptr("ws"), q2, S(rt))
        return L.adain_coral(a.ptr("style"), int(sf == "u8"), sn, hs, ws, a.ptr("content"), int(cf == "u8"), n, hc, max(1, wc - 1), a.ptr("out2"),
                             a.ptr("ws"), q2, S(rt))

    outs = c.run(call, history=other, extra=lambda a: {"record": a.bytes("ws")[:nrec].clone()})
    out, rec = rt.coral(style, content)
    same(outs, out=out, record=rec)


def test_coral_refuses_before_it_launches(rt):
    L = rt.lib()
    x = randu8(2, 5, 5, 3, seed=1)
    out = torch.empty(2 * 3 * 25, dtype=torch.float32, device=x.device)
    ws = torch.empty(4096, dtype=torch.uint8, device=x.device)
    assert L.adain_coral_workspace_bytes(3, 2, 5, 5, 5, 5) == 0 and L.adain_coral_workspace_bytes(0, 1, 5, 5, 5, 5) == 0
    assert L.adain_coral_workspace_bytes(1, 1, 5, 0, 5, 5) == 0 and L.adain_coral_workspace_bytes(1, 1, 40000, 40000, 5, 5) == 0
    q = L.adain_coral_workspace_bytes(2, 2, 5, 5, 5, 5)
    args = lambda **kw: [kw.get("style", x.data_ptr()), 1, kw.get("sn", 2), 5, 5, x.data_ptr(), 1, 2, 5, 5, kw.get("out", out.data_ptr()),
                         kw.get("ws", ws.data_ptr()), kw.get("q", q), S(rt)]
    assert L.adain_coral(*args()) == 0
    for bad in (dict(style=None), dict(sn=3), dict(q=q - 1), dict(ws=ws.data_ptr() + 4), dict(out=out.data_ptr() + 2)):
        assert L.adain_coral(*args(**bad)) == -1, bad
    torch.cuda.synchronize()


@pytest.mark.parametrize("depth,mask", [(False, None), (True, (3, 1, 64, 80, 0)), (False, (1, 3, 31, 45, 1))])
def test_stylize_u8_ex(rt, packed, depth, mask):
    L = rt.lib()
    n, h, w = 3, 64, 80
    frames = randu8(n, h, w, 3, seed=31)
    s_mean, s_std = randn(n, 512, seed=32), randn(n, 512, seed=33).abs() + 0.1
    c = Case(rt).inp("frames", frames).inp("enc", packed[0]).inp("dec", packed[1]).inp("s_mean", s_mean).inp("s_std", s_std)
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
    q = L.adain_stylize_u8_ex_workspace_bytes(n, h, w, int(depth), mn, mc, mh, mw, mf)
    assert q == L.adain_stylize_u8_workspace_bytes(n, h, w, int(depth), mn, mc, mh, mw, mf) > 0
    q2 = L.adain_stylize_u8_ex_workspace_bytes(n, h - 8, w, 0, 0, 0, 0, 0, 0)
    c.ws("ws", q).out("out", n * oh.value * ow.value * 3)

    def call(a):
        dp, _k = host_ptrs(*[a.ptr(f"depth{i}") for i in range(n)]) if depth else (None, None)
        dh, dw = (ints(*[d.shape[0] for d in dmaps]), ints(*[d.shape[1] for d in dmaps])) if depth else (None, None)
        return L.adain_stylize_u8_ex(a.ptr("frames"), n, h, w, a.ptr("enc"), a.ptr("dec"), a.ptr("s_mean"), a.ptr("s_std"), n, 0.5, 0.5, dp, dh, dw,
                                     0.15, 20.0, a.ptr("mask") if m is not None else None, mf, mn, mc, mh, mw, a.ptr("out"), a.ptr("ws"), q, S(rt))

    def other(a):          # shorter frames, one style, no mask, no depth: every block of the carve lands elsewhere
        return L.adain_stylize_u8_ex(a.ptr("frames"), n, h - 8, w, a.ptr("enc"), a.ptr("dec"), a.ptr("s_mean"), a.ptr("s_std"), 1, 0.5, 0.5, None,
                                     None, None, 0.15, 20.0, None, 0, 0, 0, 0, 0, a.ptr("out"), a.ptr("ws"), q2, S(rt))
    outs = c.run(call, history=other)
    same(outs, out=rt.stylize_u8(frames, packed[0], packed[1], s_mean, s_std, alpha=0.5, depth_maps=dmaps, mask=m, style_n=n))
