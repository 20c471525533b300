"""The guard-band harness (tests/abi_arena.py) must be able to fail: on a host-memory arena, with a plain Python stand-in for a call of
the C ABI, each kind of fault it exists to find is reported with the right region and offset, and a well-behaved stand-in passes."""
import pytest
import torch

import abi_arena as A

N = 1000          # floats of the stand-in's input and output
WS = 4096         # bytes of its workspace


def _specs():
    return [("x", 4 * N, "in", 256), ("bias", 4 * 3, "in", 256), ("ws", WS, "ws", 8), ("out", 4 * N, "out", 16)]


def _setup(arena):
    arena.put("x", torch.arange(N, dtype=torch.float32))
    arena.put("bias", torch.tensor([1.0, 2.0, 3.0]))


def _good(arena):
    """out = 2 x + bias[0], through the workspace - which it writes before it reads, as a call must."""
    x = arena.bytes("x").view(torch.float32)
    ws = arena.bytes("ws").view(torch.float32)
    ws[:] = 0
    ws[:N] = 2 * x
    arena.bytes("out").view(torch.float32).copy_(ws[:N] + arena.bytes("bias").view(torch.float32)[0])


def _run(call, **kw):
    return A.run_case(_specs(), call, "cpu", lambda: None, setup=_setup, **kw)


def test_regions_have_their_size_alignment_and_guards():
    for fill in A.FILLS:
        arena = A.Arena(_specs(), fill, "cpu")
        prev_end = 0
        for r in arena.regions:
            p = arena.ptr(r.name)
            assert p % r.align == 0 and p % (2 * r.align) == r.align          # that alignment and no better
            assert arena.bytes(r.name).numel() == r.nbytes
            assert r.offset - prev_end >= (A.EDGE if prev_end == 0 else A.GUARD)
            prev_end = r.offset + r.nbytes
        assert arena.size - prev_end >= A.EDGE
        arena.check()                                                          # untouched: passes
    b = A.Arena(_specs(), "B", "cpu").buf
    assert int((b == 0).sum()) == 0 and b[:4096].unique().numel() > 200        # no zero byte, position-dependent
    assert int((A.Arena(_specs(), "A", "cpu").buf != 0xFF).sum()) == 0


def test_a_well_behaved_call_passes_and_returns_its_outputs():
    outs = _run(_good, history=lambda arena: arena.bytes("ws").fill_(7))
    assert torch.equal(outs["out"].view(torch.float32), 2 * torch.arange(N, dtype=torch.float32) + 1)


def test_a_write_one_byte_before_an_output_is_reported():
    def call(arena):
        _good(arena)
        arena.buf[arena.region("out").offset - 1] = 0
    with pytest.raises(A.ArenaViolation) as e:
        _run(call)
    gap = A.Arena(_specs(), "A", "cpu")
    width = gap.region("out").offset - (gap.region("ws").offset + WS)
    assert e.value.region == "guard between ws and out" and e.value.first == e.value.last == width - 1 and e.value.count == 1


def test_a_write_one_byte_after_an_output_is_reported():
    def call(arena):
        _good(arena)
        arena.buf[arena.region("out").offset + 4 * N] = 0
    with pytest.raises(A.ArenaViolation) as e:
        _run(call)
    assert e.value.region == "guard after out" and e.value.first == e.value.last == 0 and e.value.count == 1


def test_a_write_into_an_input_is_reported():
    def call(arena):
        _good(arena)
        arena.bytes("x")[40:44] += 1          # the call "normalises its input in place"
    with pytest.raises(A.ArenaViolation) as e:
        _run(call)
    assert e.value.region == "x" and (e.value.first, e.value.last, e.value.count) == (40, 43, 4)


def test_a_write_into_an_input_nobody_put_is_reported():
    def call(arena):
        arena.bytes("bias")[5] = 0
    with pytest.raises(A.ArenaViolation) as e:
        A.run_case(_specs(), call, "cpu", lambda: None)
    assert e.value.region == "bias" and e.value.first == e.value.last == 5


def test_a_read_of_a_stale_workspace_byte_that_reaches_the_output_is_reported():
    def call(arena):
        """Forgets to clear float 10 of the workspace before accumulating into it."""
        x = arena.bytes("x").view(torch.float32)
        ws = arena.bytes("ws").view(torch.int32)
        stale = ws[10].clone()
        ws[:] = 0
        ws[10] = stale
        ws[:N] += (2 * x).to(torch.int32)
        arena.bytes("out").view(torch.int32).copy_(ws[:N])
    with pytest.raises(A.ArenaViolation) as e:
        _run(call)
    assert e.value.region == "out" and 40 <= e.value.first <= e.value.last <= 43 and "fill A and fill B" in str(e.value)


def test_a_result_that_depends_on_the_previous_call_is_reported_by_the_history_rerun():
    def call(arena):
        """Leans on a flag in the workspace that only its own earlier run leaves there."""
        ws = arena.bytes("ws")
        first = bool(ws[0] != 0x5A)
        _good(arena)
        arena.bytes("out").view(torch.float32)[3] += 0.0 if first else 1.0
        ws[0] = 0x5A
    _run(call)                                # fills A and B agree: both are first runs
    with pytest.raises(A.ArenaViolation) as e:
        _run(call, history=lambda arena: None)
    assert e.value.region == "out" and 12 <= e.value.first <= 15 and "rerun" in str(e.value)


def test_outputs_of_different_sizes_are_reported():
    with pytest.raises(A.ArenaViolation):
        A.compare_outputs({"o": torch.zeros(4, dtype=torch.uint8)}, {"o": torch.zeros(5, dtype=torch.uint8)}, "a", "b")


def test_declared_padding_of_an_output_is_guarded_and_of_an_input_is_poisoned():
    specs = [("x", 64, "in", 256, [(40, 64)]), ("out", 128, "out", 256, [(100, 128)])]

    def call(arena, spill=0, peek=False):
        x = arena.bytes("x")
        arena.bytes("out")[:100 + spill] = 1 + (int(x[50]) // 2 if peek else 0)

    setup = lambda arena: arena.put("x", torch.zeros(64, dtype=torch.uint8))
    outs = A.run_case(specs, call, "cpu", lambda: None, setup=setup)
    assert int(outs["out"][:100].sum()) == 100 and int(outs["out"][100:].sum()) == 0
    with pytest.raises(A.ArenaViolation) as e:          # a write into the output's padding
        A.run_case(specs, lambda a: call(a, spill=2), "cpu", lambda: None, setup=setup)
    assert e.value.region == "padding of out at its offset 100" and (e.value.first, e.value.last, e.value.count) == (0, 1, 2)
    with pytest.raises(A.ArenaViolation) as e:          # a read of the input's padding that reaches the output
        A.run_case(specs, lambda a: call(a, peek=True), "cpu", lambda: None, setup=setup)
    assert e.value.region == "out" and "fill A and fill B" in str(e.value)


# ---- run_captured: the same harness around a call that is recorded once and replayed ---------------------------------------------------
class Recorder:
    """The stand-in for a graph capture: while ``capture`` runs, a stand-in call appends what it would enqueue to ``ops`` and runs
    nothing; ``replay`` runs the recorded ops."""

    def __init__(self):
        self.ops, self.replays = None, 0

    def enqueue(self, op):
        if self.ops is None:
            op()
        else:
            self.ops.append(op)

    def capture(self, do):
        self.ops = ops = []
        try:
            rc = do()
        finally:
            self.ops = None
        if rc not in (None, 0):
            raise A.CaptureFailed(f"rc {rc}")

        def replay():
            self.replays += 1
            for op in ops:
                op()
        return replay


def _sets():
    def put(scale):
        def setup(arena):
            arena.put("x", scale * torch.arange(N, dtype=torch.float32))
            arena.put("bias", torch.tensor([1.0, 2.0, 3.0]))
        return setup
    return {"A": put(1.0), "B": put(3.0)}


def _captured(call, rec, **kw):
    return A.run_captured(_specs(), call, "cpu", lambda: None, _sets(), rec.capture, differs=("out",), **kw)


def test_a_well_behaved_call_is_captured_and_replayed_three_times():
    rec = Recorder()
    ea, eb = _captured(lambda arena: rec.enqueue(lambda: _good(arena)), rec)
    assert rec.replays == 3
    assert torch.equal(ea["out"].view(torch.float32), 2 * torch.arange(N, dtype=torch.float32) + 1)
    assert torch.equal(eb["out"].view(torch.float32), 6 * torch.arange(N, dtype=torch.float32) + 1)


def test_a_host_side_copy_of_the_input_taken_at_capture_is_caught_by_the_second_replay():
    rec = Recorder()

    def call(arena):
        """Stages its input through host memory when it is called: the graph replays the copy, not the input."""
        staged = arena.bytes("x").view(torch.float32).clone()

        def op():
            arena.bytes("ws").zero_()
            arena.bytes("out").view(torch.float32).copy_(2 * staged + arena.bytes("bias").view(torch.float32)[0])
        rec.enqueue(op)
    with pytest.raises(A.ArenaViolation) as e:
        _captured(call, rec)
    assert e.value.region == "out" and "second replay" in str(e.value) and rec.replays == 2


def test_work_done_at_capture_time_instead_of_enqueued_is_caught_before_any_replay():
    rec = Recorder()

    def call(arena):
        arena.bytes("ws")[:16] = 0          # "clears a counter" right away, outside the stream
        rec.enqueue(lambda: _good(arena))
    with pytest.raises(A.ArenaViolation) as e:
        _captured(call, rec)
    assert e.value.region == "ws" and "captured" in str(e.value) and rec.replays == 0


def test_a_result_that_depends_on_what_the_previous_replay_left_is_caught_by_the_third_replay():
    rec = Recorder()

    def op(arena):
        ws = arena.bytes("ws")
        again = bool(ws[0] == 0x5A) and bool(ws[1] == 0x5A)          # only its own earlier run leaves both
        _good(arena)
        arena.bytes("out").view(torch.float32)[3] += 1.0 if again else 0.0
        ws[:2] = 0x5A
    with pytest.raises(A.ArenaViolation) as e:
        _captured(lambda arena: rec.enqueue(lambda: op(arena)), rec)
    assert e.value.region == "out" and "third replay" in str(e.value) and rec.replays == 3


def test_a_call_that_fails_while_it_is_captured_is_never_replayed():
    rec = Recorder()

    def call(arena):
        if rec.ops is not None:
            return -2
        rec.enqueue(lambda: _good(arena))
    with pytest.raises(A.CaptureFailed):
        _captured(call, rec, last_error=lambda: "refused")
    assert rec.replays == 0


def test_data_sets_whose_outputs_do_not_differ_are_refused():
    rec = Recorder()

    def call(arena):          # ignores x: both sets give the same output
        rec.enqueue(lambda: (arena.bytes("ws").zero_(), arena.bytes("out").zero_()))
    with pytest.raises(AssertionError, match="could show nothing"):
        _captured(call, rec)
    assert rec.replays == 0
