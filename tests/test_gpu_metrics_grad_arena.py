"""The memory contract of adain_image_metrics_grad_f32 through the guard-band arena (tests/abi_arena.py): a workspace of exactly the
query's size, no byte outside grad_a, grad_b and the workspace changes, the inputs and the weights stay as they were, two fills and a
previous call of another shape give the same bits (nothing is read from the workspace that the call did not write), and every refusal -
misaligned and overlapping buffers among them - is ADAIN_EINVAL with nothing written."""
import numpy as np
import pytest
import torch

import abi_arena as A
import metrics_grad_cases as K
import metrics_grad_ref as G

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
EINVAL = -1
BARS = K.bars()
SHAPE = (2, 3, 19, 67)          # n, c, h, w: two tiles down, two across
FA, FB = K.edge_pair(SHAPE, seed=6)
WEIGHTS = np.array([[-0.2, 0.7, 0.8], [1.0, 0.0, -0.5]])
WANT = G.grad(FA, FB, WEIGHTS)


@pytest.fixture(scope="module")
def rt():
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    import applied_image_processing_amd.runtime as rt

    rt.lib()
    torch.cuda.set_device(0)
    assert rt.lib().adain_image_metrics_grad_f32(None, None, 1, 1, 1, 1, None, None, None, None, 0, None) == EINVAL          # ADAIN_EINVAL is what a null gets
    return rt


@pytest.mark.parametrize("with_b", [False, True], ids=["grad_a", "grad_a_and_b"])
def test_the_call_stays_in_its_buffers_and_reads_nothing_stale(rt, with_b):
    nbytes = rt.image_metrics_grad_sizes(*SHAPE, grad_b=with_b)
    specs = [("a", FA.nbytes, "in", 4), ("b", FB.nbytes, "in", 4), ("weights", WEIGHTS.nbytes, "in", 8), ("grad_a", FA.nbytes, "out", 4),
             ("grad_b", FA.nbytes, "out" if with_b else "in", 4), ("workspace", nbytes, "ws", 8)]
    stream = torch.cuda.current_stream().cuda_stream

    def call(arena, shape=SHAPE):
        rc = rt.lib().adain_image_metrics_grad_f32(arena.ptr("a"), arena.ptr("b"), *shape, arena.ptr("weights"), arena.ptr("grad_a"),
                                                   arena.ptr("grad_b") if with_b else None, arena.ptr("workspace"), nbytes, stream)
        assert rc == 0, rt.lib().adain_last_error().decode()

    def history(arena):          # a call of another shape leaves its planes elsewhere, then the workspace is poisoned
        call(arena, (1, 2, 40, 9))
        arena.bytes("workspace").fill_(0xA5)

    def setup(arena):
        arena.put("a", torch.from_numpy(FA)), arena.put("b", torch.from_numpy(FB)), arena.put("weights", torch.from_numpy(WEIGHTS))

    outs = A.run_case(specs, call, DEV, torch.cuda.synchronize, history=history, setup=setup)
    for which, name in enumerate(("grad_a", "grad_b")[:2 if with_b else 1]):
        got = outs[name].cpu().numpy().view(np.float32).reshape(FA.shape)
        assert np.all(G.distance(got, WANT[which]) <= BARS["bar_grad"]), name
    # the wrapper hands the same call its own buffers: the same bits
    x, y, w = (torch.from_numpy(v).to(DEV) for v in (FA, FB, WEIGHTS))
    wrapped = rt.image_metrics_grad(x, y, w, grad_b=with_b)
    wrapped = wrapped if with_b else (wrapped,)
    for name, t in zip(("grad_a", "grad_b"), wrapped):
        assert torch.equal(A.as_bytes(t), outs[name].to(DEV)), name


def test_every_refusal_is_einval_and_writes_nothing(rt):
    n, c, h, w = SHAPE
    nbytes = rt.image_metrics_grad_sizes(*SHAPE, grad_b=True)
    specs = [("a", FA.nbytes, "in", 4), ("b", FB.nbytes, "in", 4), ("weights", WEIGHTS.nbytes, "in", 8), ("grad_a", FA.nbytes, "out", 4), ("grad_b", FA.nbytes, "out", 4),
             ("workspace", nbytes, "ws", 8)]
    arena = A.Arena(specs, "B", DEV)
    arena.put("a", torch.from_numpy(FA)), arena.put("b", torch.from_numpy(FB)), arena.put("weights", torch.from_numpy(WEIGHTS))
    pa, pb, pw, ga, gb, ws = (arena.ptr(k) for k in ("a", "b", "weights", "grad_a", "grad_b", "workspace"))
    stream = torch.cuda.current_stream().cuda_stream
    good = dict(a=pa, b=pb, n=n, c=c, h=h, w=w, weights=pw, grad_a=ga, grad_b=gb, workspace=ws, workspace_bytes=nbytes)
    last = FA.nbytes - 4          # the offset of a clip's last float
    refusals = [          # (what adain_last_error names, the argument that is wrong)
        ("a is a null", dict(a=None)), ("b is a null", dict(b=None)), ("weights is a null", dict(weights=None)), ("grad_a is a null", dict(grad_a=None)),
        ("workspace is a null", dict(workspace=None)), ("c outside 1..4", dict(c=0)), ("c outside 1..4", dict(c=5)), ("n outside", dict(n=0)), ("n outside", dict(n=65536)),
        ("h below 1", dict(h=0)), ("w below 1", dict(w=-2)), ("2^31 - 1 samples", dict(h=32768, w=32768, workspace_bytes=1 << 62)),
        ("workspace too small", dict(workspace_bytes=nbytes - 1)), ("workspace must be 8-byte aligned", dict(workspace=ws + 4)),
        ("weights must be 8-byte aligned", dict(weights=pw + 4)), ("a must be 4-byte aligned", dict(a=pa + 2)), ("b must be 4-byte aligned", dict(b=pb + 1)),
        ("grad_a must be 4-byte aligned", dict(grad_a=ga + 2)), ("grad_b must be 4-byte aligned", dict(grad_b=gb + 3)),
        ("grad_a overlaps a", dict(grad_a=pa + last)), ("grad_a overlaps b", dict(grad_a=pb - last)), ("grad_a overlaps weights", dict(grad_a=pw + 44)),
        ("grad_b overlaps a", dict(grad_b=pa - last)), ("grad_b overlaps b", dict(grad_b=pb + 4)), ("grad_b overlaps weights", dict(grad_b=pw - last)),
        ("grad_b overlaps grad_a", dict(grad_b=ga)), ("grad_b overlaps grad_a", dict(grad_b=ga + last)),
        ("workspace overlaps a", dict(workspace=pa - pa % 8)), ("workspace overlaps b", dict(workspace=pb + 8 - pb % 8)), ("workspace overlaps weights", dict(workspace=pw + 40)),
        ("workspace overlaps grad_a", dict(workspace=ga + 8 - ga % 8)), ("workspace overlaps grad_b", dict(workspace=gb - gb % 8)),
    ]
    for text, change in refusals:
        v = dict(good, **change)
        rc = rt.lib().adain_image_metrics_grad_f32(v["a"], v["b"], v["n"], v["c"], v["h"], v["w"], v["weights"], v["grad_a"], v["grad_b"], v["workspace"],
                                                   v["workspace_bytes"], stream)
        message = rt.lib().adain_last_error().decode()
        assert rc == EINVAL, (text, rc)
        assert message.startswith("image_metrics_grad_f32: ") and text in message, (text, message)
    for query in ((0, 3, 4, 4, 0), (1, 0, 4, 4, 1), (1, 3, 0, 4, 0), (1, 4, 32768, 32768, 1)):
        assert rt.lib().adain_image_metrics_grad_f32_bytes(*query, None) == EINVAL
    torch.cuda.synchronize()
    arena.check()
    for name in ("grad_a", "grad_b", "workspace"):
        r = arena.region(name)
        assert bool((arena.bytes(name) == arena._expected(r.offset, r.offset + r.nbytes)).all()), f"a refused call wrote into {name}"
