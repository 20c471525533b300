"""Guard-band arenas for calls of the C ABI (include/adain_hip.h): where a call writes, and what it reads that it never wrote.

One ``torch.uint8`` allocation per call under test, carved into named regions - each input, each output, the packed weights, the
workspace.  Outputs and workspaces have exactly their documented size, every region starts at the alignment the header states for it
and no better (a multiple of ``align`` that is not a multiple of ``2 * align``), neighbours are at least ``GUARD`` bytes apart and
``EDGE`` bytes lie before the first and after the last.  The whole arena starts from one of two fills - ``A``: every byte 0xFF (NaN
as float, -1 as int), ``B``: a position-dependent pattern of non-zero bytes - the inputs are then put in place, and after the call
every byte that is not a declared output or workspace is compared with what was put there, on the arena's own device.

``run_case`` drives one case: fresh arenas with fills A and B, outputs bitwise equal between them, and (``history``) the same call
again in arena B after another call has used the same workspace.  Works on a host arena with a Python stand-in for the call
(tests/test_abi_arena_host.py) exactly as on the GPU (tests/test_gpu_abi_memory.py).

``run_captured`` drives one row of tests/capture_cases.py: the call captured alone into a graph (``hip_graph``; a Python recorder on a
host arena) and replayed on the captured data, on a second data set put into the same regions, and on the workspace that replay left,
each time to the eager call's outputs bit for bit (tests/test_gpu_graph_capture.py).
"""
import torch

GUARD = 64 << 10          # between neighbouring regions, at least
EDGE = 4 << 20            # before the first and after the last region, at least (a row of 4096 x 64 floats is 1 MiB)
FILLS = ("A", "B")
_CHUNK = 32 << 20         # bytes compared / generated at a time


class ArenaViolation(AssertionError):
    """A byte outside the declared outputs and workspaces changed, or outputs differ where they must be bitwise equal."""

    def __init__(self, message, region=None, first=None, last=None, count=None):
        super().__init__(message)
        self.region, self.first, self.last, self.count = region, first, last, count


def pattern(start, stop, device):
    """Fill B for arena offsets [start, stop): a byte in 1..251 that depends on the offset (never zero, period 251 x 2^16 and more)."""
    i = torch.arange(start, stop, dtype=torch.int64, device=device)
    return ((i * 167 + (i >> 8) * 13 + (i >> 16) * 7) % 251 + 1).to(torch.uint8)


class Region:
    def __init__(self, name, nbytes, role, align, holes=()):
        assert role in ("in", "out", "ws") and nbytes >= 0 and align >= 1 and align & (align - 1) == 0
        self.name, self.nbytes, self.role, self.align = name, int(nbytes), role, int(align)
        # byte ranges [a, b) of the region that the header declares padding: an output's are not written (they are checked like a
        # guard and left out of the compared outputs), an input's are left as the fill (nothing may read them)
        self.holes = sorted((int(a), int(b)) for a, b in holes if b > a)
        assert all(0 <= a < b <= self.nbytes for a, b in self.holes)
        self.offset = None
        self.data = None          # role "in": the bytes put there (uint8 tensor on the arena's device)


class Arena:
    """``specs``: [(name, nbytes, role, align[, holes])] in memory order; role "in" (inputs, packed weights, bias, pointer tables: must not
    change), "out" or "ws" (the call may write them; nothing else)."""

    def __init__(self, specs, fill, device):
        assert fill in FILLS
        self.fill, self.device = fill, torch.device(device)
        self.regions = [Region(*s) for s in specs]
        assert len({r.name for r in self.regions}) == len(self.regions), "region names must be unique"
        # the allocation is placed first, then the regions by its real address: an alignment is a property of the pointer handed over
        worst = EDGE + sum(r.nbytes + GUARD + 2 * r.align for r in self.regions) + EDGE
        self.buf = torch.empty(worst, dtype=torch.uint8, device=self.device)
        base = self.buf.data_ptr()
        off = EDGE
        for r in self.regions:
            a = r.align
            p = (base + off + a - 1) // a * a
            if p % (2 * a) == 0:                         # a multiple of a, not of 2a
                p += a
            r.offset = off = p - base
            off += r.nbytes + GUARD
        self.size = off - GUARD + EDGE
        assert self.size <= worst
        self.buf = self.buf[:self.size]
        self._by_name = {r.name: r for r in self.regions}
        for a in range(0, self.size, _CHUNK):
            b = min(self.size, a + _CHUNK)
            if fill == "A":
                self.buf[a:b] = 0xFF
            else:
                self.buf[a:b] = pattern(a, b, self.device)

    # ---- access --------------------------------------------------------------------------------------------------------------------
    def region(self, name):
        return self._by_name[name]

    def ptr(self, name):
        r = self._by_name[name]
        p = self.buf.data_ptr() + r.offset
        assert p % r.align == 0 and p % (2 * r.align) != 0
        return p

    def nbytes(self, name):
        return self._by_name[name].nbytes

    def bytes(self, name):
        r = self._by_name[name]
        return self.buf[r.offset:r.offset + r.nbytes]

    def put(self, name, tensor):
        """Places an input (any dtype, contiguous; exactly the region's size) and remembers it as what must still be there afterwards."""
        r = self._by_name[name]
        assert r.role == "in", f"{name}: only inputs are put"
        src = tensor.contiguous().view(-1).view(torch.uint8).to(self.device)
        assert src.numel() == r.nbytes, f"{name}: {src.numel()} bytes for a region of {r.nbytes}"
        if r.holes:
            src = src.clone()
            for a, b in r.holes:
                src[a:b] = self._expected(r.offset + a, r.offset + b)
        self.bytes(name).copy_(src)
        r.data = src

    def outputs(self):
        """{name: a copy of the region's bytes} of every declared output, its padding zeroed."""
        outs = {}
        for r in self.regions:
            if r.role == "out":
                outs[r.name] = self.bytes(r.name).clone()
                for a, b in r.holes:
                    outs[r.name][a:b] = 0
        return outs

    # ---- the check -----------------------------------------------------------------------------------------------------------------
    def _expected(self, a, b):
        if self.fill == "A":
            return torch.full((b - a,), 0xFF, dtype=torch.uint8, device=self.device)
        return pattern(a, b, self.device)

    def _diff(self, a, b, expected_of):
        """(first, last, count) of changed bytes in arena offsets [a, b), offsets relative to a; None when unchanged."""
        first = last = None
        count = 0
        for c in range(a, b, _CHUNK):
            d = min(b, c + _CHUNK)
            ne = self.buf[c:d] != expected_of(c, d)
            k = int(ne.sum())
            if k:
                idx = ne.nonzero()
                if first is None:
                    first = c - a + int(idx[0])
                last = c - a + int(idx[-1])
                count += k
        return None if first is None else (first, last, count)

    def check(self):
        """Every byte outside the declared outputs and workspaces still holds what was put there; raises ArenaViolation naming the
        region, the first and last changed offset (from the region's start) and the count.  The caller has synchronised the stream."""
        spans = []                # (label, start, stop, expected_of)
        at = 0
        for i, r in enumerate(self.regions):
            before = "guard before " + r.name if i == 0 else f"guard between {self.regions[i - 1].name} and {r.name}"
            spans.append((before, at, r.offset, self._expected))
            if r.role == "in":
                if r.data is None:
                    spans.append((r.name, r.offset, r.offset + r.nbytes, self._expected))
                else:
                    spans.append((r.name, r.offset, r.offset + r.nbytes, lambda a, b, r=r: r.data[a - r.offset:b - r.offset]))
            elif r.role == "out":
                spans += [(f"padding of {r.name} at its offset {a}", r.offset + a, r.offset + b, self._expected) for a, b in r.holes]
            at = r.offset + r.nbytes
        spans.append(("guard after " + self.regions[-1].name, at, self.size, self._expected))
        for label, a, b, expected_of in spans:
            if b <= a:
                continue
            d = self._diff(a, b, expected_of)
            if d is not None:
                first, last, count = d
                raise ArenaViolation(f"fill {self.fill}: {label} ({b - a} bytes at arena offset {a}) changed: {count} byte(s), first at "
                                     f"offset {first}, last at offset {last} of it", label, first, last, count)


def compare_outputs(got, want, what_got, what_want):
    """Bitwise equality of two {name: uint8 tensor} output sets; raises ArenaViolation naming the output, first and last offset, count."""
    assert got.keys() == want.keys()
    for name in got:
        g, w = got[name], want[name].to(got[name].device)
        if g.numel() != w.numel():
            raise ArenaViolation(f"output {name}: {g.numel()} bytes from {what_got}, {w.numel()} from {what_want}", name)
        ne = g != w
        k = int(ne.sum())
        if k:
            idx = ne.nonzero()
            first, last = int(idx[0]), int(idx[-1])
            raise ArenaViolation(f"output {name} differs between {what_got} and {what_want}: {k} of {g.numel()} byte(s), first at offset "
                                 f"{first}, last at offset {last}", name, first, last, k)


def as_bytes(t):
    return t.contiguous().view(-1).view(torch.uint8)


def run_case(specs, call, device, sync, history=None, setup=None, extra=None):
    """One case on fresh arenas with fills A and B.  ``specs``: the regions; ``setup(arena)`` puts the inputs; ``call(arena)`` makes the
    call under test with pointers into the arena; ``sync()`` waits for its stream.  After each call the arena is checked.  The outputs
    must be bitwise equal between the fills.  ``history(arena)``: another call (another shape) that uses the same workspace region of
    arena B; after it the call under test runs there again and must give the same bits a third time.  ``extra(arena)``: further
    outputs as {name: uint8 tensor} (the part of a workspace that the header declares a result).  Returns fill A's outputs."""
    def outputs(arena):
        return dict(arena.outputs(), **(extra(arena) if extra is not None else {}))

    outs = {}
    arena_b = None
    for fill in FILLS:
        arena = Arena(specs, fill, device)
        if setup is not None:
            setup(arena)
        call(arena)
        sync()
        arena.check()
        outs[fill] = outputs(arena)
        arena_b = arena
    compare_outputs(outs["A"], outs["B"], "fill A", "fill B")
    if history is not None:
        history(arena_b)
        sync()
        arena_b.check()
        call(arena_b)
        sync()
        arena_b.check()
        compare_outputs(outputs(arena_b), outs["B"], "the rerun after a call of another shape", "fill B")
    return outs["A"]


# ---- the same call captured into a graph and replayed ----------------------------------------------------------------------------------
class CaptureFailed(AssertionError):
    """The call returned an error while it was being captured, or the capture did not end clean.  Nothing was replayed."""


def hip_graph(last_error=lambda: ""):
    """``capture`` of ``run_captured`` on the GPU: ``capture(do)`` opens a side stream, captures the single call ``do()`` (which returns
    the call's return value) into a ``torch.cuda.graph`` on that one stream - no second stream, no fork, no event: the graph is a chain
    - and returns ``replay()``.  A non-zero return value or a capture that ends in an error raises CaptureFailed with
    ``last_error()``, after making sure that no stream is left capturing; a graph whose capture did not end clean is never replayed."""
    def capture(do):
        torch.cuda.synchronize()
        before = torch.cuda.current_stream()
        side = torch.cuda.Stream()
        graph = torch.cuda.CUDAGraph()
        rc, err = None, None
        try:
            with torch.cuda.graph(graph, stream=side):
                rc = do()                      # (no raise inside: the capture is ended first, whatever the call answered)
        except Exception as e:                 # the runtime refused the capture: an error code, read below
            err = e
        text = last_error()
        with torch.cuda.stream(side):
            still = torch.cuda.is_current_stream_capturing()
        still = still or torch.cuda.is_current_stream_capturing()
        if still:                              # end it, so that the next test starts from a stream that is not capturing
            try:
                graph.capture_end()
            except Exception:
                pass
            with torch.cuda.stream(side):
                assert not torch.cuda.is_current_stream_capturing(), "the capture could not be ended"
        # where the capture's end raised, torch did not leave its stream context: the side stream must not stay the current one
        torch.cuda.set_stream(before)
        if err is not None or still or (rc is not None and rc != 0):
            del graph
            raise CaptureFailed(f"the call could not be captured: rc {rc}, {text!r}" + (f", capture error: {err}" if err is not None else "")
                                + (", the stream was still capturing" if still else ""))
        torch.cuda.synchronize()

        def replay():
            graph.replay()
        return replay
    return capture


def _overwrite(arena, how):
    """Every byte of every output and workspace that the call may write (an output's declared padding stays, it is guarded) gets 0xFF
    (``how`` "ff") or the arena's position-dependent pattern (``how`` "pattern")."""
    for r in arena.regions:
        if r.role == "in":
            continue
        at = 0
        for a, b in list(r.holes) + [(r.nbytes, r.nbytes)]:
            for c in range(at, a, _CHUNK):
                d = min(a, c + _CHUNK)
                arena.buf[r.offset + c:r.offset + d] = 0xFF if how == "ff" else pattern(r.offset + c, r.offset + d, arena.device)
            at = b


def _still_ff(arena):
    """The name of the first output or workspace with a byte that is no longer the 0xFF of ``_overwrite``; None when all are."""
    for r in arena.regions:
        if r.role == "in":
            continue
        at = 0
        for a, b in list(r.holes) + [(r.nbytes, r.nbytes)]:
            if a > at and bool((arena.buf[r.offset + at:r.offset + a] != 0xFF).any()):
                return r.name
            at = b
    return None


def run_captured(specs, call, device, sync, sets, capture, differs=(), extra=None, last_error=lambda: ""):
    """One call held to the promise that it may be captured into a graph.  ``sets``: {"A": setup_a, "B": setup_b}, each ``setup(arena)``
    puts one data set of the same shapes; ``call(arena)`` makes the call with pointers into the arena and returns its return value (None
    counts as 0); ``capture(do)`` records the single call ``do()`` without running it and returns ``replay()`` (``hip_graph`` on the GPU,
    a Python stand-in on a host arena).  ``differs``: the outputs (names of ``arena.outputs()`` and of ``extra``) that must differ
    between the eager results of the two sets, so that the replay on set B has something to show.  The steps:

    1. eager: set A in a fresh arena (fill B), the call, ``arena.check()`` -> E_A; set B in another -> E_B (these are the warm-up too);
    2. a fresh arena with set A, every output and workspace overwritten with 0xFF, the capture of the single call; afterwards they
       still hold 0xFF and the arena checks: capturing wrote nothing.  A call or a capture that fails raises CaptureFailed, no replay;
    3. first replay: the outputs are E_A bit for bit;
    4. set B put into the same input regions, outputs and workspaces overwritten with the position-dependent pattern, second replay:
       the outputs are E_B bit for bit;
    5. third replay with nothing refilled - the workspace holds what the second left: E_B again.

    Every comparison is an equality.  Returns (E_A, E_B)."""
    def outputs(arena):
        return dict(arena.outputs(), **(extra(arena) if extra is not None else {}))

    def checked(arena, what):
        rc = call(arena)
        assert rc is None or rc == 0, f"{what}: rc {rc}: {last_error()}"

    eager = {}
    for name in ("A", "B"):
        arena = Arena(specs, "B", device)
        sets[name](arena)
        checked(arena, f"the eager call on set {name}")
        sync()
        arena.check()
        eager[name] = outputs(arena)
    assert differs, "a row names what differs between its data sets"
    for name in differs:
        a, b = eager["A"][name], eager["B"][name]
        assert a.numel() != b.numel() or not torch.equal(a, b), f"output {name} is the same for both data sets: the replay on set B could show nothing"
    arena = Arena(specs, "B", device)
    sets["A"](arena)
    _overwrite(arena, "ff")
    sync()
    replay = capture(lambda: call(arena))
    sync()
    touched = _still_ff(arena)
    if touched is not None:
        raise ArenaViolation(f"{touched} was written while the call was captured, before any replay", touched)
    arena.check()
    replay()
    sync()
    arena.check()
    compare_outputs(outputs(arena), eager["A"], "the first replay", "the eager call on set A")
    sets["B"](arena)                                   # in place: the graph holds the addresses
    _overwrite(arena, "pattern")
    sync()
    replay()
    sync()
    arena.check()
    compare_outputs(outputs(arena), eager["B"], "the second replay (set B in place)", "the eager call on set B")
    replay()
    sync()
    arena.check()
    compare_outputs(outputs(arena), eager["B"], "the third replay (the workspace as the second left it)", "the eager call on set B")
    return eager["A"], eager["B"]
