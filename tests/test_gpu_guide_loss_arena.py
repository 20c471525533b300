"""The memory contract of adain_guide_l1_f32 and adain_guide_l1_grad_f32 through the guard-band arena (tests/abi_arena.py): a workspace of
exactly the query's size, no byte outside out, resampled, grad and the workspace changes, the inputs stay as they were, two fills and a
previous call of another shape give the same bits (nothing is read from the workspace that the call did not write), and every refusal -
misaligned and overlapping buffers among them - is ADAIN_EINVAL with nothing written."""
import numpy as np
import pytest
import torch

import abi_arena as A
import guide_loss_cases as K
import guide_loss_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
EINVAL = -1
SHAPE = (2, 17, 65, 11, 23)          # two frames, w % 4 != 0, two workgroups a frame
N, H, W, GH, GW = SHAPE
GUIDE, IMAGE = K.guide(SHAPE), K.image_delta(SHAPE)
WEIGHTS = np.array([0.75, -2.0])
OTHER = (1, 40, 9, 5, 7)             # the call of another shape in the workspace's history


@pytest.fixture(scope="module")
def rt():
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    import applied_image_processing_amd.runtime as rt

    rt.lib()
    torch.cuda.set_device(0)
    assert rt.lib().adain_guide_l1_f32(None, None, 1, 1, 1, 1, 1, None, None, None, 0, None) == EINVAL          # ADAIN_EINVAL is what a null gets
    return rt


def put_inputs(arena):
    arena.put("image", torch.from_numpy(np.array(IMAGE))), arena.put("guide", torch.from_numpy(np.array(GUIDE)))


@pytest.mark.parametrize("with_resampled", [False, True], ids=["out", "out_and_resampled"])
def test_the_forward_call_stays_in_its_buffers_and_reads_nothing_stale(rt, with_resampled):
    nbytes = rt.guide_l1_sizes(N, H, W)
    specs = [("image", IMAGE.nbytes, "in", 4), ("guide", GUIDE.nbytes, "in", 1), ("out", 8 * N, "out", 8),
             ("resampled", IMAGE.nbytes, "out" if with_resampled else "in", 4), ("workspace", nbytes, "ws", 8)]
    stream = torch.cuda.current_stream().cuda_stream

    def call(arena, shape=SHAPE):
        n, h, w, gh, gw = shape
        rc = rt.lib().adain_guide_l1_f32(arena.ptr("image"), arena.ptr("guide"), n, h, w, gh, gw, arena.ptr("out"), arena.ptr("resampled") if with_resampled else None,
                                         arena.ptr("workspace"), nbytes, stream)
        assert rc == 0, rt.lib().adain_last_error().decode()

    def history(arena):          # a call of another shape leaves its partials elsewhere, then the workspace is poisoned
        assert rt.guide_l1_sizes(*OTHER[:3]) <= nbytes
        call(arena, OTHER)
        arena.bytes("workspace").fill_(0xA5)

    outs = A.run_case(specs, call, DEV, torch.cuda.synchronize, history=history, setup=put_inputs)
    got, want = outs["out"].cpu().numpy().view(np.float64), R.loss(IMAGE, GUIDE)
    assert np.all(np.abs(got - want) <= R.loss_bound(IMAGE, want))
    if with_resampled:
        assert np.array_equal(outs["resampled"].cpu().numpy().view(np.float32).reshape(IMAGE.shape).view(np.uint32), K.g_ref(SHAPE).view(np.uint32))
    # the wrapper hands the same call its own buffers: the same bits
    wrapped = rt.guide_l1(torch.from_numpy(np.array(IMAGE)).to(DEV), torch.from_numpy(np.array(GUIDE)).to(DEV), resampled=with_resampled)
    assert torch.equal(A.as_bytes(wrapped.l1), outs["out"].to(DEV))
    if with_resampled:
        assert torch.equal(A.as_bytes(wrapped.resampled), outs["resampled"].to(DEV))


def test_the_gradient_call_stays_in_its_buffer(rt):
    specs = [("image", IMAGE.nbytes, "in", 4), ("guide", GUIDE.nbytes, "in", 1), ("weights", WEIGHTS.nbytes, "in", 8), ("grad", IMAGE.nbytes, "out", 4)]
    stream = torch.cuda.current_stream().cuda_stream

    def call(arena):
        rc = rt.lib().adain_guide_l1_grad_f32(arena.ptr("image"), arena.ptr("guide"), N, H, W, GH, GW, arena.ptr("weights"), arena.ptr("grad"), stream)
        assert rc == 0, rt.lib().adain_last_error().decode()

    def setup(arena):
        put_inputs(arena), arena.put("weights", torch.from_numpy(WEIGHTS))

    outs = A.run_case(specs, call, DEV, torch.cuda.synchronize, setup=setup)
    got = outs["grad"].cpu().numpy().view(np.float32).reshape(IMAGE.shape)
    assert np.array_equal(got.view(np.uint32), R.grad(IMAGE, GUIDE, WEIGHTS).view(np.uint32))
    x, g, w = (torch.from_numpy(np.array(v)).to(DEV) for v in (IMAGE, GUIDE, WEIGHTS))
    assert torch.equal(A.as_bytes(rt.guide_l1_grad(x, g, w)), outs["grad"].to(DEV))


def test_every_refusal_is_einval_and_writes_nothing(rt):
    nbytes = rt.guide_l1_sizes(N, H, W)
    specs = [("image", IMAGE.nbytes, "in", 4), ("guide", GUIDE.nbytes, "in", 1), ("weights", WEIGHTS.nbytes, "in", 8), ("out", 8 * N, "out", 8),
             ("resampled", IMAGE.nbytes, "out", 4), ("grad", IMAGE.nbytes, "out", 4), ("workspace", nbytes, "ws", 8)]
    arena = A.Arena(specs, "B", DEV)
    put_inputs(arena), arena.put("weights", torch.from_numpy(WEIGHTS))
    pi, pg, pw, po, pr, pgr, ws = (arena.ptr(k) for k in ("image", "guide", "weights", "out", "resampled", "grad", "workspace"))
    stream = torch.cuda.current_stream().cuda_stream
    good = dict(image=pi, guide=pg, n=N, h=H, w=W, gh=GH, gw=GW, out=po, resampled=pr, workspace=ws, workspace_bytes=nbytes, weights=pw, grad=pgr)
    last = IMAGE.nbytes - 4          # the offset of a clip's last float
    down8 = lambda p: p - p % 8

    def forward(v):
        return rt.lib().adain_guide_l1_f32(v["image"], v["guide"], v["n"], v["h"], v["w"], v["gh"], v["gw"], v["out"], v["resampled"], v["workspace"], v["workspace_bytes"], stream)

    def backward(v):
        return rt.lib().adain_guide_l1_grad_f32(v["image"], v["guide"], v["n"], v["h"], v["w"], v["gh"], v["gw"], v["weights"], v["grad"], stream)

    shapes = [("n outside", dict(n=0)), ("n outside", dict(n=65536)), ("h below 1", dict(h=0)), ("w below 1", dict(w=-2)), ("gh below 1", dict(gh=0)), ("gw below 1", dict(gw=-1)),
              ("a frame beyond 2^31 - 1 samples", dict(h=32768, w=32768, workspace_bytes=1 << 62)), ("a guide beyond 2^31 - 1 samples", dict(gh=32768, gw=32768))]
    refusals = [(forward, "guide_l1_f32: ", shapes + [          # (what adain_last_error names, the argument that is wrong)
        ("image is a null", dict(image=None)), ("guide is a null", dict(guide=None)), ("out is a null", dict(out=None)), ("workspace is a null", dict(workspace=None)),
        ("workspace too small", dict(workspace_bytes=nbytes - 1)), ("workspace must be 8-byte aligned", dict(workspace=ws + 4)), ("out must be 8-byte aligned", dict(out=po + 4)),
        ("image must be 4-byte aligned", dict(image=pi + 2)), ("resampled must be 4-byte aligned", dict(resampled=pr + 1)),
        ("out overlaps image", dict(out=down8(pi + last))), ("out overlaps guide", dict(out=down8(pg + GUIDE.nbytes - 1))),
        ("resampled overlaps image", dict(resampled=pi + last)), ("resampled overlaps guide", dict(resampled=pg - pg % 4)), ("resampled overlaps out", dict(resampled=po + 12)),
        ("workspace overlaps image", dict(workspace=down8(pi))), ("workspace overlaps guide", dict(workspace=down8(pg))), ("workspace overlaps out", dict(workspace=po + 8)),
        ("workspace overlaps resampled", dict(workspace=down8(pr + last)))]),
        (backward, "guide_l1_grad_f32: ", shapes[:6] + [
            ("a frame beyond 2^31 - 1 samples", dict(h=32768, w=32768)), ("a guide beyond 2^31 - 1 samples", dict(gh=32768, gw=32768)),
            ("image is a null", dict(image=None)), ("guide is a null", dict(guide=None)), ("weights is a null", dict(weights=None)), ("grad is a null", dict(grad=None)),
            ("weights must be 8-byte aligned", dict(weights=pw + 4)), ("image must be 4-byte aligned", dict(image=pi + 1)), ("grad must be 4-byte aligned", dict(grad=pgr + 2)),
            ("grad overlaps image", dict(grad=pi - last)), ("grad overlaps guide", dict(grad=pg - pg % 4)), ("grad overlaps weights", dict(grad=pw + 12))])]
    for call, prefix, cases in refusals:
        for text, change in cases:
            rc = call(dict(good, **change))
            message = rt.lib().adain_last_error().decode()
            assert rc == EINVAL, (text, rc)
            assert message.startswith(prefix) and text in message, (text, message)
    for query in ((0, 4, 4), (1, 0, 4), (1, 4, 0), (1, 32768, 32768)):
        assert rt.lib().adain_guide_l1_f32_bytes(*query, None) == EINVAL
    torch.cuda.synchronize()
    arena.check()
    for name in ("out", "resampled", "grad", "workspace"):
        r = arena.region(name)
        assert bool((arena.bytes(name) == arena._expected(r.offset, r.offset + r.nbytes)).all()), f"a refused call wrote into {name}"
