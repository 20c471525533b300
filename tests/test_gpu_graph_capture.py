"""include/adain_hip.h: "No call allocates, frees or synchronises, so every call may be captured into a hipGraph."  Every launch of the
header but the stated exception (tests/capture_cases.py holds the table and the exception, test_capture_cases_host.py holds both to the
header) is captured alone into a graph on one side stream and replayed three times by tests/abi_arena.run_captured: on the data it was
captured with, on a second data set of the same shapes and host arguments put into the same buffers, and once more on the workspace the
second replay left.  Each replay gives the eager call's outputs bit for bit - lengths, records and statuses included - and changes no
byte outside the declared outputs and workspaces; capturing itself writes nothing.  Where a row's data come with a restatement's
results, the eager results the replays were held to are held to those as well, under the bar of the call's own test: equality for
most, the own bars of the metrics, their gradient, the guide loss, CORAL, the statistics, the strength map and the TV-L1 preparation
(capture_cases' ``held``) for those.  Between a replay and the eager call there is no tolerance anywhere.  The rows on seeded noise -
the network calls, the packs, the split layer, the Farneback pyramids - have no restatement in their own arena tests and none here.
One more test captures the video path's chain of four calls into one graph.  Run with ``-m gpu``.

A capture that the runtime refuses is a failure to read (abi_arena.CaptureFailed carries adain_last_error()); nothing is replayed after
it."""
import ctypes

import numpy as np
import pytest
import torch

import abi_arena as A
import capture_cases as K

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


@pytest.fixture(scope="module")
def rt():
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    import applied_image_processing_amd.runtime as rt

    rt.lib()
    torch.cuda.set_device(0)
    return rt


class Env:
    def __init__(self, rt, weights):
        self.device, self.weights = torch.device(DEV), weights
        self.packed = rt.pack_encoder(weights[0], self.device), rt.pack_decoder(weights[1], self.device)


@pytest.fixture(scope="module")
def env(rt, weights):
    return Env(rt, weights)


def last_error(rt):
    return lambda: rt.lib().adain_last_error().decode()


def held_by_equality(name, got, want):
    """``got``: an output's bytes (uint8 tensor); ``want``: the restatement's value, in the output's number format."""
    got = got.cpu().numpy()
    want = np.ascontiguousarray(np.stack(want) if isinstance(want, (list, tuple)) else want)
    if want.dtype.kind in "iu" and want.size and got.size // want.size != want.dtype.itemsize:          # an integer result in a wider host type
        assert int(want.min()) >= 0 and got.size % want.size == 0
        want = want.astype({1: np.uint8, 4: np.int32}[got.size // want.size])
    want = want.view(np.uint8).reshape(-1)
    assert got.size == want.size, (name, got.size, want.size)
    bad = np.flatnonzero(got != want)
    assert bad.size == 0, f"{name}: {bad.size} of {got.size} bytes differ from the restatement's, first at {int(bad[0])}"


@pytest.mark.parametrize("row", K.ROWS, ids=lambda r: r.id)
def test_the_call_captured_alone_replays_the_eager_results(rt, env, row):
    a, b = row.data()
    with rt.schedule(rt.SCHEDULE_LATENCY if row.latency else rt.SCHEDULE_BATCH):
        plan = row.plan(rt, env, a, b)
        torch.cuda.synchronize()
        ea, eb = A.run_captured(plan.specs, plan.call, DEV, torch.cuda.synchronize, {"A": plan.setup("A"), "B": plan.setup("B")},
                                A.hip_graph(last_error(rt)), differs=tuple(row.differs), extra=plan.extra, last_error=last_error(rt))
    assert not torch.cuda.is_current_stream_capturing()
    for which, e in ((a, ea), (b, eb)):
        for name, want in which.get("_expected", {}).items():
            held_by_equality(f"{row.id}: {name}", e[name], want)
        if row.held is not None:          # a restatement whose bar in the call's own test is not equality: that bar
            row.held(which, e)
        if "_status" in which:          # the PNG decoder: the restatement's statuses, and its pixels where a file is sound
            n = len(which["_status"])
            assert e["record"].cpu().view(torch.int32).reshape(n, 2)[:, 0].tolist() == which["_status"]
            px = e["out"].cpu().numpy().reshape(n, -1)
            for i, status in enumerate(which["_status"]):
                assert status != 0 or np.array_equal(px[i], which["_pixels"][i].reshape(-1)), f"file {i}"


# ---- the video path: decode -> resize -> stylize -> encode, one graph, one stream ---------------------------------------------------------
CHAIN_GEOMETRY = (40, 64, 3, 2)          # the content frames' files: 40 x 64, 4:2:0
CHAIN_SIZE = (32, 48)                    # what the frames are resized to before they are stylised


class Chain:
    """The four calls' static buffers, each call with a workspace of its own, and ``enqueue()`` - the four calls on the current stream."""

    def __init__(self, rt, env, host):
        offsets, lengths, (h, w, c, sampling) = host
        self.rt, self.n, n = rt, 2, 2
        L = self.L = rt.lib()
        ho, wo = CHAIN_SIZE
        code = rt.pil_filter("BICUBIC")
        oh, ow = ctypes.c_int(), ctypes.c_int()
        L.adain_stylize_u8_out_size(ho, wo, 0, ctypes.byref(oh), ctypes.byref(ow))
        oh, ow = oh.value, ow.value
        with torch.cuda.device(env.device):
            q_sty = L.adain_stylize_u8_workspace_bytes(n, ho, wo, 0, 0, 0, 0, 0, 0)
        q_dec = rt.jpeg_decode_sizes(n, h, w, c, sampling, max(lengths))
        q_res = rt._size_query("adain_resize_pil_u8_bytes", n, h, w, ho, wo, 3, code, 0, 0, ho, wo)[0]
        self.stride, q_enc = rt._size_query("adain_jpeg_encode_u8_bytes", n, oh, ow, 3, results=2)
        u8 = lambda *shape: torch.full(shape, 0xA5, dtype=torch.uint8, device=DEV)
        self.files, self.blobs = u8(len(K.LEAD) + sum(lengths)), None
        self.decoded, self.record, self.resized, self.stylised = u8(n, h, w, 3), u8(n, 8), u8(n, ho, wo, 3), u8(n, oh, ow, 3)
        self.rows, self.lengths = u8(n, self.stride), u8(n, 4)
        self.ws = [u8(max(q, 256)) for q in (q_dec, q_res, q_sty, q_enc)]
        taps = []
        for a_, b_ in ((w, wo), (h, ho)):
            k, bounds, t = rt.pil_resize_taps(code, a_, b_)
            taps.append((k, torch.from_numpy(bounds.copy()).to(DEV), torch.from_numpy(t.copy()).to(DEV)))
        (kx, bx, tx), (ky, by, ty) = self.taps = taps
        g = torch.Generator().manual_seed(5)
        self.s_mean, self.s_std = torch.randn(1, 512, generator=g).to(DEV), (torch.randn(1, 512, generator=g).abs() + 0.1).to(DEV)
        off, ln = (ctypes.c_uint64 * n)(*offsets), (ctypes.c_uint32 * n)(*lengths)
        S = rt._stream
        P = lambda t: t.data_ptr()
        self.calls = [
            lambda: L.adain_jpeg_decode_u8(P(self.files), self.files.numel(), P(self.blobs), n, h, w, c, sampling, off, ln, P(self.decoded), P(self.record),
                                           P(self.ws[0]), q_dec, 0, S()),
            lambda: L.adain_resize_pil_u8(P(self.decoded), 3, n, h, w, P(self.resized), ho, wo, code, P(bx), P(tx), kx, P(by), P(ty), ky, 0, 0, ho, wo,
                                          P(self.ws[1]), q_res, S()),
            lambda: L.adain_stylize_u8(P(self.resized), n, ho, wo, P(env.packed[0]), P(env.packed[1]), P(self.s_mean), P(self.s_std), 0.5, 0.5, None, None, None,
                                       0.15, 20.0, None, 0, 0, 0, 0, 0, P(self.stylised), P(self.ws[2]), q_sty, S()),
            lambda: L.adain_jpeg_encode_u8(P(self.stylised), n, oh, ow, 3, 75, P(self.rows), self.stride, P(self.lengths), P(self.ws[3]), q_enc, S()),
        ]

    def load(self, data):
        """Set ``data`` into the static input buffers, in place."""
        files, blobs = torch.from_numpy(data["files"].copy()).to(DEV), torch.from_numpy(data["blobs"].copy()).to(DEV)
        assert files.numel() == self.files.numel()
        self.files.copy_(files)
        if self.blobs is None:
            self.blobs = blobs.clone()
        else:
            self.blobs.copy_(blobs)

    def poison(self, value):
        for t in [self.decoded, self.record, self.resized, self.stylised, self.rows, self.lengths] + self.ws:
            t.fill_(value)

    def enqueue(self):
        for call in self.calls:
            rc = call()
            if rc != 0:
                return rc
        return 0

    def results(self):
        torch.cuda.synchronize()
        ln = self.lengths.view(torch.int32).view(-1).tolist()
        assert all(0 < k <= self.stride for k in ln), ln
        return {"decoded": self.decoded.clone(), "record": self.record.clone(), "resized": self.resized.clone(), "stylised": self.stylised.clone(),
                "lengths": self.lengths.clone(), "files": torch.cat([self.rows[i, :k].clone() for i, k in enumerate(ln)])}


def chain_data():
    twins = K.designed_twins("jpeg", CHAIN_GEOMETRY)
    sets = {}
    for which in ("A", "B"):
        parts = [K._segments("jpeg", d) for d in twins[which]]
        segs = [s for _p, ss, _b in parts for s in ss]
        lengths = [len(s) for s in segs]
        offsets = [len(K.LEAD) + sum(lengths[:i]) for i in range(len(segs))]
        sets[which] = {"files": np.frombuffer(K.LEAD + b"".join(segs), np.uint8), "blobs": np.frombuffer(b"".join(b for _p, _s, b in parts), np.uint8),
                       "host": (tuple(offsets), tuple(lengths), tuple(parts[0][0].geometry))}
    assert sets["A"]["host"] == sets["B"]["host"], "the graph bakes the offsets and lengths in"
    return sets


def test_the_video_chain_in_one_graph_replays_the_eager_chain(rt, env):
    """adain_jpeg_decode_u8 -> adain_resize_pil_u8 -> adain_stylize_u8 -> adain_jpeg_encode_u8 on one stream in one graph, replayed on
    two files of set A, then on their twins of equal length (set B) put in place: every stage's bytes, the files and ``lengths`` are
    the eager chain's."""
    sets = chain_data()
    eager = {}
    for which in ("A", "B"):          # the eager chains are the warm-up too
        c = Chain(rt, env, sets[which]["host"])
        c.load(sets[which])
        assert c.enqueue() == 0, last_error(rt)()
        eager[which] = c.results()
        assert not eager[which]["record"].view(torch.int32)[:, 0].any(), "the files decode"
    for name in ("decoded", "stylised", "files"):
        assert not torch.equal(eager["A"][name], eager["B"][name]), f"{name} is the same for both sets: the second replay could show nothing"
    c = Chain(rt, env, sets["A"]["host"])
    c.load(sets["A"])
    c.poison(0xFF)
    replay = A.hip_graph(last_error(rt))(c.enqueue)
    torch.cuda.synchronize()
    assert all(bool((t == 0xFF).all()) for t in [c.decoded, c.record, c.resized, c.stylised, c.rows, c.lengths] + c.ws), "capturing the chain wrote something"
    for which, fill in (("A", 0xFF), ("B", 0x5B), ("B", None)):
        c.load(sets[which])
        if fill is not None:
            c.poison(fill)
        replay()
        A.compare_outputs(c.results(), eager[which], f"the replayed chain on set {which}", "the eager chain")
