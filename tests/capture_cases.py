"""The graph-capture table (tests/test_capture_cases_host.py, tests/test_gpu_graph_capture.py).  Not a test module.

include/adain_hip.h promises of the whole library that "no call allocates, frees or synchronises, so every call may be captured into a
hipGraph", and states one exception, adain_tvl1_flow.  ``ROWS`` holds one row per launch of the header (``abi_launches.launches()``),
``EXEMPT`` the launches without a row, each with its reason; test_capture_cases_host.py holds the two to the header, so that an entry
point added later fails until it has a row or a reason.

A row is a small case of its call, laid out as the arena tests lay theirs out (tests/abi_arena.py: inputs, outputs and workspaces of
exactly their documented size, at the alignment the call's own arena test hands them and no better), with TWO data sets of the same
shapes and the same host arguments:

* ``data()`` -> (A, B): {input name: array}; the key ``_host`` holds the host arguments that come from the data (a decoder's offsets,
  lengths and parsed tables), which a graph bakes in and which must therefore be equal in both sets; ``_expected`` holds, where the
  data come from a table with a restatement's results, {output name: the restatement's value} held by equality;
* ``differs``: {output name: what differs there between the eager results of A and B} - the test asserts that they do differ;
* ``plan(rt, env, A, B)`` -> a ``Plan``: the regions, the two set-ups and ``call(arena)``, which makes the C call on ``rt._stream()``
  with pointers into the arena and returns its return value.

The data come from the generators and restatements the calls' own tests use: far_batch.py's ``make()`` patterns (patterns 0..2 are set
A, 3..5 set B, a value shared by a batch is pattern 0's in both), png_decode_cases, jpeg_designed, colour_fixtures, and for the calls
whose arena tests run on seeded noise (the network, the packs, the flow pyramids) seeded noise of two seeds.  ``N`` = 3 frames wherever
a call takes n, so that the frame index is live.  tests/abi_arena.run_captured drives a row."""
import ctypes
import functools
import json
import math
import os

import numpy as np

import far_batch as B

N = 3
D, U = 0, 1          # ADAIN_SRC_DIRECT, ADAIN_SRC_UP2X

EXEMPT = {
    "adain_tvl1_flow": "include/adain_hip.h: the one call that synchronises - it waits on the stream between outer passes to read the stopping test's "
                       "residual, so it must not be captured into a hipGraph",
}


# ---- a row and its plan -------------------------------------------------------------------------------------------------------------------
class Row:
    """``id``: the call's name, with a suffix where a call has a second row; ``latency``: run under ADAIN_SCHEDULE_LATENCY;
    ``host_equal``: the sentence that says why the host arguments of A and B are equal."""

    def __init__(self, call, differs, data, plan, id=None, latency=False, host_equal="the host arguments are the shapes alone: one tuple for both sets",
                 held=None, same=None):
        self.call, self.id, self.differs, self._data, self.plan, self.latency, self.host_equal = call, id or call, dict(differs), data, plan, latency, host_equal
        self.same = dict(same or {})          # {name of an expected value: why ``differs`` does not list it}
        self.held = held          # held(set, outputs): the outputs against the set's ``_ref`` values, under the bar of the call's own test

    @functools.lru_cache(maxsize=None)
    def data(self):
        return self._data()

    def __repr__(self):
        return f"Row({self.id})"


def tensor(a):
    import torch

    if isinstance(a, torch.Tensor):
        return a
    a = np.ascontiguousarray(a)
    if not a.flags.writeable:          # a view of bytes, a broadcast row
        a = a.copy()
    return torch.from_numpy(a.view(np.uint8) if a.dtype == np.bool_ else a)


def nbytes_of(a):
    t = tensor(a)
    return t.numel() * t.element_size()


class Plan:
    """The regions of one call in memory order and the two set-ups.  ``inp(name, a, b)``: an input with set A's and set B's value
    (``b`` None: one value for both - packed weights, tables; a callable is ``f(arena) -> tensor``, for tables of arena pointers)."""

    def __init__(self):
        self.specs, self.sets, self.call, self.extra, self.keep = [], {"A": {}, "B": {}}, None, None, []

    def inp(self, name, a, b=None, align=256, holes=(), nbytes=None):
        b = a if b is None else b
        if nbytes is None:
            nbytes = nbytes_of(a)
            assert nbytes_of(b) == nbytes, f"{name}: the two sets differ in size"
        self.specs.append((name, nbytes, "in", align, holes))
        self.sets["A"][name], self.sets["B"][name] = a, b
        return self

    def out(self, name, nbytes, align=256, holes=()):
        self.specs.append((name, nbytes, "out", align, holes))
        return self

    def ws(self, name, nbytes, align=256):
        self.specs.append((name, nbytes, "ws", align))
        return self

    def setup(self, which):
        def put(arena):
            for name, t in self.sets[which].items():
                arena.put(name, tensor(t(arena) if callable(t) else t))
        return put


def S(rt):
    return rt._stream()


def ints(*v):
    return (ctypes.c_int * len(v))(*v)


def host_ptrs(*p):
    arr = (ctypes.c_void_p * len(p))(*p)
    return ctypes.cast(arr, ctypes.POINTER(ctypes.c_void_p)), arr


def noise_f32(seed, *shape, scale=1.0):
    return (np.random.default_rng([77, seed]).standard_normal(shape) * scale).astype(np.float32)


def noise_u8(seed, *shape):
    return np.random.default_rng([78, seed]).integers(0, 256, shape, dtype=np.uint8)


def split(make, names, outs=(), shared=(), refs=()):
    """Sets A and B from a far_batch ``make()``: per-frame inputs ``names`` (in make's order) are patterns 0..N-1 and N..2N-1, the ones
    in ``shared`` pattern 0 in both; ``outs``: a name per expected value held by equality, None for one that is not; ``refs``: a name
    per expected value that the row's ``held`` holds under the bar of the call's own test (key ``_ref``)."""
    def data():
        inputs, expected = make()
        assert len(inputs) == len(names) and 2 * N <= B.P
        sets = []
        for lo in (0, N):
            d = {nm: (np.ascontiguousarray(x[0]) if nm in shared else np.ascontiguousarray(x[lo:lo + N])) for nm, x in zip(names, inputs)}
            d["_expected"] = {nm: e[lo:lo + N] for nm, e in zip(outs, expected) if nm is not None}
            d["_ref"] = {nm: np.asarray(e[lo:lo + N]) for nm, e in zip(refs, expected) if nm is not None}
            sets.append(d)
        return tuple(sets)
    return data


def block_holes(blocks, base=0):
    """Byte ranges of the padding behind blocks of ``blocks`` floats, each block starting at a multiple of 64 floats from ``base``."""
    holes, off = [], base
    for floats in blocks:
        end = off + (floats + 63) // 64 * 64
        holes.append((4 * (off + floats), 4 * end))
        off = end
    return [hb for hb in holes if hb[1] > hb[0]], off


def file_records(n, stride):
    """``extra`` of an encoder: the first lengths[i] bytes of every row of ``out`` as one output (behind them a row is not written)."""
    def extra(arena):
        import torch

        ln = arena.bytes("lengths").view(torch.int32).tolist()
        assert all(0 < k <= stride for k in ln), ln
        return {"files": torch.cat([arena.bytes("out")[i * stride:i * stride + k].clone() for i, k in enumerate(ln)])}
    return extra


ROWS = []


def add(*a, **kw):
    ROWS.append(Row(*a, **kw))


# ---- pixel kernels ------------------------------------------------------------------------------------------------------------------------
def _simple(call, names, out_bytes, args, aligns=None, ws=None):
    """plan of a call whose regions are its inputs, one output ``out`` and at most one workspace: ``args(ptr, A) -> the C arguments``
    (``ptr(name)``: the region's address); ``out_bytes(A)``; ``ws(rt, A) -> bytes``."""
    def plan(rt, env, A, Bset):
        p = Plan()
        for nm in names:
            p.inp(nm, A[nm], Bset[nm], align=(aligns or {}).get(nm, 1 if A[nm].dtype == np.uint8 else A[nm].dtype.itemsize))
        q = ws(rt, A) if ws is not None else 0
        if ws is not None:
            p.ws("workspace", q, 8)
        p.out("out", out_bytes(A), (aligns or {}).get("out", 4))
        fn = getattr(rt.lib(), call)
        p.call = lambda a: fn(*args(a.ptr, A), *((a.ptr("workspace"), q) if ws is not None else ()), S(rt))
        return p
    return plan


_PIX = {"out": "the pixels: other frames"}
add("adain_quantize_u8", _PIX, split(B._quantize(3, 4, 67), ["x"], ["out"]),
    _simple("adain_quantize_u8", ["x"], lambda A: N * 4 * 67 * 3, lambda ptr, A: (ptr("x"), ptr("out"), N, 3, 4, 67), {"out": 1}))
add("adain_u8_to_f32", _PIX, split(B._to_f32(3, 4, 67), ["x"], ["out"]),
    _simple("adain_u8_to_f32", ["x"], lambda A: N * 3 * 4 * 67 * 4, lambda ptr, A: (ptr("x"), ptr("out"), N, 3, 4, 67)))
add("adain_resize_bilinear", _PIX, split(B._resize("bilinear", 5, 7, 13, 9), ["x"], ["out"]),
    _simple("adain_resize_bilinear", ["x"], lambda A: N * 13 * 9 * 4, lambda ptr, A: (ptr("x"), ptr("out"), N, 5, 7, 13, 9)))
add("adain_resize_nearest", _PIX, split(B._resize("nearest", 5, 7, 13, 12), ["x"], ["out"]),
    _simple("adain_resize_nearest", ["x"], lambda A: N * 13 * 12 * 4, lambda ptr, A: (ptr("x"), ptr("out"), N, 5, 7, 13, 12)))
add("adain_mask_composite", _PIX, split(B._composite(67), ["content", "stylized", "mask"], ["out"]),          # N images of one channel, a mask per image
    _simple("adain_mask_composite", ["content", "stylized", "mask"], lambda A: N * 67 * 4,
            lambda ptr, A: (ptr("content"), ptr("stylized"), ptr("mask"), 1, N, ptr("out"), N, 1, 67)))
add("adain_resize_area_u8", _PIX, split(B._area(100, 99, 3, 37, 61), ["x"], ["out"]),
    _simple("adain_resize_area_u8", ["x"], lambda A: N * 37 * 61 * 3, lambda ptr, A: (ptr("x"), ptr("out"), N, 100, 99, 3, 37, 61), {"out": 1}))
add("adain_flow_gray_u8", _PIX, split(B._gray(20, 31, 37, 61), ["rgb"], ["out"]),
    _simple("adain_flow_gray_u8", ["rgb"], lambda A: N * 37 * 61, lambda ptr, A: (ptr("rgb"), N, 20, 31, ptr("out"), 37, 61), {"out": 1}))
add("adain_nchw_to_nhwc", _PIX, split(B._transpose(True, 3, 67), ["x"], ["out"]),
    _simple("adain_nchw_to_nhwc", ["x"], lambda A: N * 3 * 67 * 4, lambda ptr, A: (ptr("x"), ptr("out"), N, 3, 67)))
add("adain_nhwc_to_nchw", _PIX, split(B._transpose(False, 3, 67), ["x"], ["out"]),
    _simple("adain_nhwc_to_nchw", ["x"], lambda A: N * 3 * 67 * 4, lambda ptr, A: (ptr("x"), ptr("out"), N, 3, 67)))


def _tvl1_plan(rt, env, A, Bset):
    import applied_image_processing_amd.tvl1 as tvl1

    h, w = A["gray"].shape[1:]
    tv = tvl1.TVL1(h, w)
    fbytes = rt.lib().adain_tvl1_frame_bytes(h, w, ctypes.addressof(tv.P))
    holes, floats = [], 0
    for _frame in range(N):
        hb, floats = block_holes([4 * ws_ * hs_ for (ws_, hs_) in tv.scales], floats)
        holes += hb
    assert 4 * floats == N * fbytes
    p = Plan().inp("gray", A["gray"], Bset["gray"], 1).out("prepared", N * fbytes, 16, holes)
    p.keep.append(tv)
    p.call = lambda a: rt.lib().adain_tvl1_prepare(a.ptr("gray"), N, h, w, ctypes.addressof(tv.P), a.ptr("prepared"), S(rt))
    return p


def _tvl1_held(d, e):
    """test_gpu_tvl1.py's bar as test_gpu_far_batch_pixel.py restates it: per scale and component, rel L2 from the float64 restatement
    within max(1e-6, twice the float32 restatement's own)."""
    import applied_image_processing_amd.tvl1 as tvl1
    import tvl1_ref as TV

    gray = d["gray"]
    tv = tvl1.TVL1(*gray.shape[1:])
    got = e["prepared"].cpu().numpy().view(np.float32).reshape(N, -1)
    rel = lambda a, b: float(np.linalg.norm(a.astype(np.float64) - b) / max(np.linalg.norm(b), 1e-30))
    for k in range(N):
        r64, r32 = TV.prepare(gray[k]), TV.prepare(gray[k], dtype=np.float32)
        assert np.array_equal(np.concatenate([c.ravel() for s in r64 for c in s]), d["_ref"]["prepared"][k]), "the table's expected is this restatement"
        off = 0
        for (ws_, hs_), r, f in zip(tv.scales, r64, r32):
            v = got[k, off:off + 4 * ws_ * hs_].reshape(hs_, ws_, 4)
            for c in range(3):
                assert rel(v[..., c], r[c]) <= max(1e-6, 2 * rel(f[c], r[c])), (k, (ws_, hs_), c)
            off += (4 * ws_ * hs_ + 63) // 64 * 64
        assert off == got.shape[1]


add("adain_tvl1_prepare", {"prepared": "the (I, I_x, I_y) blocks of every scale: other textures"}, split(B._tvl1(37, 61), ["gray"], refs=["prepared"]), _tvl1_plan,
    held=_tvl1_held)


WARP_H, WARP_W = 16, 64          # pixel_ref.WARP_FRAMES' frame of the vector kernel


def _warp_data():
    """test_gpu_pixel_dispatch.py's recipe: seeded frames under pixel_ref.warp_flows - A the random flow, B the flow whose every map
    value lands half-way between two 1/32 steps; expected: the oracle's bit-for-bit restatement."""
    import pixel_ref as R
    from oracle import adain_oracle as O

    assert (WARP_H, WARP_W) in R.WARP_FRAMES
    rng = np.random.default_rng([7, WARP_H, WARP_W])
    flows = R.warp_flows(WARP_H, WARP_W)
    sets = []
    for name in ("random", "ties_pos"):
        cur, prev = (rng.integers(0, 256, (WARP_H, WARP_W, 3), dtype=np.uint8) for _ in range(2))
        sets.append(dict(cur=cur, prev=prev, flow=flows[name], _expected={"out": O.warp_blend_u8(cur, prev, flows[name], 0.7)}))
    return tuple(sets)


add("adain_warp_blend_u8", _PIX, _warp_data,
    _simple("adain_warp_blend_u8", ["cur", "prev", "flow"], lambda A: WARP_H * WARP_W * 3,
            lambda ptr, A: (ptr("cur"), ptr("prev"), ptr("flow"), ptr("out"), WARP_H, WARP_W, 3, 0.7, float(1 - 0.7)), {"out": 1}))

STRENGTH = ("total256", 40, 50, 16, 16, 0.3, 12.0, "smooth")          # a row of pixel_ref.STRENGTH_CASES
STRENGTH_MARGIN_ULP = 3          # test_gpu_pixel_dispatch.py's


def _strength_data():
    """Set A: the case's own depth map (pixel_ref.strength_input); set B: synth.smooth_depth of another seed at the same size."""
    import applied_image_processing_amd.synth as synth
    import pixel_ref as R

    assert STRENGTH in R.STRENGTH_CASES
    name, h0, w0, hc, wc, off, prom, kind = STRENGTH
    sets = []
    for depth in (R.strength_input(name, h0, w0, kind), np.ascontiguousarray(synth.smooth_depth(4242, h0, w0).astype(np.float32))):
        want64, parts = R.strength_map(depth, hc, wc, off, prom, dtype=np.float64, parts=True)
        assert not parts["constant"]
        sets.append(dict(depth=depth, _ref={"out": want64}))
    return tuple(sets)


def _strength_held(d, e):
    """test_gpu_pixel_dispatch.py's bar: within the float32 restatement's own distance from the float64 form, rounded up to a whole
    ulp (pixel_ref.STRENGTH_SELF_ULP is that figure for set A's map), plus its margin of 3 ulp."""
    import pixel_ref as R

    name, _h0, _w0, hc, wc, off, prom, _kind = STRENGTH
    want64 = d["_ref"]["out"]
    own = math.ceil(float(R.ulp_distance(R.strength_map(d["depth"], hc, wc, off, prom), want64).max()))
    if np.array_equal(d["depth"], R.strength_input(*STRENGTH[:3], STRENGTH[7])):
        assert own == R.STRENGTH_SELF_ULP[name]
    got = e["out"].cpu().numpy().view(np.float32).reshape(hc, wc)
    dist = R.ulp_distance(got, want64)
    assert (dist <= own + STRENGTH_MARGIN_ULP).all(), (float(dist.max()), own)


add("adain_strength_map", {"out": "the strength map: another depth map"}, _strength_data,
    _simple("adain_strength_map", ["depth"], lambda A: STRENGTH[3] * STRENGTH[4] * 4, lambda ptr, A: (ptr("depth"), *STRENGTH[1:7], ptr("out")),
            ws=lambda rt, A: rt.lib().adain_strength_map_workspace_bytes(STRENGTH[3], STRENGTH[4])), held=_strength_held)


# ---- Pillow's resizes ---------------------------------------------------------------------------------------------------------------------
PIL_IN, PIL_OUT = (20, 31), (37, 29)


def _pil_plan(rt, env, A, Bset):
    (hi, wi), (ho, wo) = PIL_IN, PIL_OUT
    code = rt.pil_filter("BICUBIC")
    q = rt._size_query("adain_resize_pil_u8_bytes", N, hi, wi, ho, wo, 3, code, 0, 0, ho, wo)[0]
    p = Plan().inp("src", A["src"], Bset["src"], 1)
    ks = []
    for axis, (a, b) in zip("xy", ((wi, wo), (hi, ho))):
        k, bounds, taps = rt.pil_resize_taps(code, a, b)
        assert k > 0
        ks.append(k)
        p.inp("bounds_" + axis, bounds.copy(), align=4).inp("taps_" + axis, taps.copy(), align=4)
    p.ws("workspace", q, 1).out("out", N * ho * wo * 3, 1)
    p.call = lambda a: rt.lib().adain_resize_pil_u8(a.ptr("src"), 3, N, hi, wi, a.ptr("out"), ho, wo, code, a.ptr("bounds_x"), a.ptr("taps_x"), ks[0],
                                                   a.ptr("bounds_y"), a.ptr("taps_y"), ks[1], 0, 0, ho, wo, a.ptr("workspace"), q, S(rt))
    return p


add("adain_resize_pil_u8", _PIX, split(B._pil(*PIL_IN, *PIL_OUT, 3, "BICUBIC"), ["src"], ["out"]), _pil_plan,
    host_equal="the tap tables depend on the sizes and the filter alone: both sets read the same device tables")
add("adain_resize_pil_bilinear_u8", _PIX, split(B._pil(*PIL_IN, *PIL_OUT, 3, "BILINEAR"), ["src"], ["out"]),
    _simple("adain_resize_pil_bilinear_u8", ["src"], lambda A: N * PIL_OUT[0] * PIL_OUT[1] * 3,
            lambda ptr, A: (ptr("src"), 3, N, *PIL_IN, ptr("out"), *PIL_OUT, 0, 0, *PIL_OUT), {"out": 1},
            ws=lambda rt, A: rt.lib().adain_resize_pil_bilinear_u8_workspace_bytes(*PIL_IN, *PIL_OUT)))


# ---- the file encoders --------------------------------------------------------------------------------------------------------------------
FILE_H, FILE_W = 40, 33
_FILES = {"lengths": "the files' lengths", "files": "the files' bytes"}


def _encoder(call, query, qdims, head, src="src"):
    """plan of an encoder: ``head(ptr) -> the arguments before (out, stride, lengths, workspace, bytes)``."""
    def plan(rt, env, A, Bset):
        stride, q = B._sizes(query, N, *qdims)
        p = Plan().inp(src, A[src], Bset[src], 1).ws("out", N * stride, 1).out("lengths", 4 * N, 4).ws("workspace", q, 8)
        p.extra = file_records(N, stride)
        fn = getattr(rt.lib(), call)
        p.call = lambda a: fn(*head(a.ptr), a.ptr("out"), stride, a.ptr("lengths"), a.ptr("workspace"), q, S(rt))
        return p
    return plan


def _file_data(make):
    """far_batch's encoder patterns -> the sets, the expected files as (lengths, files)."""
    def data():
        (frames,), (files,) = make()
        sets = []
        for lo in (0, N):
            mine = files[lo:lo + N]
            sets.append({"src": np.ascontiguousarray(frames[lo:lo + N]),
                         "_expected": {"lengths": np.array([len(f) for f in mine], dtype=np.int32), "files": np.frombuffer(b"".join(mine), np.uint8)}})
        return tuple(sets)
    return data


add("adain_jpeg_encode_u8", _FILES, _file_data(B._jpeg(FILE_H, FILE_W, 3)),
    _encoder("adain_jpeg_encode_u8", "adain_jpeg_encode_u8_bytes", (FILE_H, FILE_W, 3), lambda ptr: (ptr("src"), N, FILE_H, FILE_W, 3, 75)))
add("adain_jpeg_encode_opt_u8", _FILES, _file_data(B._jpeg(FILE_H, FILE_W, 3, subsampling=0, optimize=True)),
    _encoder("adain_jpeg_encode_opt_u8", "adain_jpeg_encode_opt_u8_bytes", (FILE_H, FILE_W, 3, 0, 1), lambda ptr: (ptr("src"), N, FILE_H, FILE_W, 3, 75, 0, 1)))
add("adain_jpeg_encode_progressive_u8", _FILES, _file_data(B._jpeg(FILE_H, FILE_W, 3, progressive=True)),
    _encoder("adain_jpeg_encode_progressive_u8", "adain_jpeg_encode_progressive_u8_bytes", (FILE_H, FILE_W, 3, 2),
             lambda ptr: (ptr("src"), N, FILE_H, FILE_W, 3, 75, 2)))
add("adain_png_encode_u8", _FILES, _file_data(B._png(FILE_H, FILE_W, 3)),
    _encoder("adain_png_encode_u8", "adain_png_encode_u8_bytes", (FILE_H, FILE_W, 3), lambda ptr: (ptr("src"), N, FILE_H, FILE_W, 3, -1)))
GIF_H, GIF_W, GIF_K = 3, 683, 16          # 2049 pixels a frame: two segments run
add("adain_gif_encode_u8", _FILES, _file_data(B._gif(GIF_K, GIF_H, GIF_W)),
    _encoder("adain_gif_encode_u8", "adain_gif_encode_u8_bytes", (GIF_H, GIF_W, GIF_K), lambda ptr: (ptr("src"), N, GIF_H, GIF_W, GIF_K, 5)))
add("adain_jpeg_roundtrip_u8", _PIX, split(B._roundtrip(FILE_H, FILE_W, 3), ["src"], ["out"]),
    _simple("adain_jpeg_roundtrip_u8", ["src"], lambda A: N * FILE_H * FILE_W * 3, lambda ptr, A: (ptr("src"), N, FILE_H, FILE_W, 3, 75, ptr("out")), {"out": 1},
            ws=lambda rt, A: B._query("adain_jpeg_roundtrip_u8_bytes", N, FILE_H, FILE_W, 3)))


# ---- the file decoders: offsets, lengths and parsed tables are host arguments, equal in both sets ---------------------------------------
DESIGNED_GEOMETRY = (33, 17, 3, 2)
LEAD = b"\xa5\xa5\xa5"          # in front of the first segment, as in the decoders' arena tests: odd offsets


def _designed_build(kind, coef, geometry):
    import jpeg_designed as JD
    import jpeg_options_ref as O

    if kind == "progressive":
        return JD.progressive(coef, geometry, JD.scripts(3)["spectral selection"])
    return JD.baseline(coef, geometry, O.STANDARD, ri=1 if kind == "restart" else 0)


def _parse(kind, data):
    import applied_image_processing_amd.jpeg_file as F

    p = F.parse(data, **B.DECODERS[kind][2])
    return p, (p.scans if kind == "progressive" else [p])


def _segments(kind, data):
    p, scans = _parse(kind, data)
    return p, [data[s.seg_offset:s.seg_offset + s.seg_length] for s in scans], b"".join(s.blob for s in scans)


@functools.lru_cache(maxsize=None)
def designed_twins(kind, geometry=DESIGNED_GEOMETRY):
    """Two jpeg_designed files of one geometry (set A) and their twins (set B): the same coefficients but for ONE AC value per file,
    which becomes the other value of its size and sign (2 <-> 3, -5 <-> -4, ...).  Symbols, code lengths and tables are the same, so
    every segment keeps its length as long as the change moves no stuffed 0xFF byte: the first such value whose file keeps every
    segment length is taken."""
    import jpeg_designed as JD

    real = JD.real_blocks(geometry)
    out = {"A": [], "B": []}
    for seed in (3, 4):
        coef = JD.designed_coefficients(geometry, seed, (1, 2, 2), progressive=kind == "progressive")
        a = _designed_build(kind, coef, geometry)
        want = [len(s) for s in _segments(kind, a)[1]]
        twin = None
        for blk, k in zip(*np.nonzero(np.abs(coef[:, 1:58]) >= 2)):
            if not real[blk]:
                continue
            v = int(coef[blk, k + 1])
            t = coef.copy()
            t[blk, k + 1] = (abs(v) ^ 1) * (1 if v > 0 else -1)
            b = _designed_build(kind, t, geometry)
            if len(b) == len(a) and [len(s) for s in _segments(kind, b)[1]] == want:
                twin = b
                break
        assert twin is not None and twin != a, "no twin of equal segment lengths"
        out["A"].append(a)
        out["B"].append(twin)
    return out


def _jpeg_decode_data(kind):
    def data():
        ref = __import__({"jpeg": "jpeg_file_ref", "restart": "jpeg_restart_ref", "progressive": "jpeg_progressive_ref"}[kind])
        sets = []
        for which in ("A", "B"):
            files = designed_twins(kind)[which]
            parts = [_segments(kind, d) for d in files]
            segs = [s for _p, ss, _b in parts for s in ss]
            lengths = [len(s) for s in segs]
            offsets = [len(LEAD) + sum(lengths[:i]) for i in range(len(segs))]
            p0 = parts[0][0]
            res = [ref.decode(d) for d in files]
            assert all(r[1] == 0 for r in res) and all(p.geometry == DESIGNED_GEOMETRY for p, _s, _b in parts)
            host = (tuple(offsets), tuple(lengths), tuple(p0.geometry), p0.restart_interval if kind == "restart" else 0,
                    tuple(map(tuple, p0.script)) if kind == "progressive" else ())
            sets.append({"files": np.frombuffer(LEAD + b"".join(segs), np.uint8), "blobs": np.frombuffer(b"".join(b for _p, _s, b in parts), np.uint8),
                         "_host": host, "_expected": {"dst": np.stack([r[0] for r in res])}})
        return tuple(sets)
    return data


def _jpeg_decode_plan(kind):
    def plan(rt, env, A, Bset):
        offsets, lengths, (h, w, c, sampling), ri, script = A["_host"]
        n = 2
        off, ln = (ctypes.c_uint64 * len(offsets))(*offsets), (ctypes.c_uint32 * len(lengths))(*lengths)
        L = rt.lib()
        if kind == "progressive":
            desc = []
            for comps, ss, se, ah, al in script:
                desc += [len(comps)] + list(comps) + [0] * (3 - len(comps)) + [ss, se, ah, al]
            scans = (ctypes.c_int32 * len(desc))(*desc)
            q = rt.jpeg_decode_progressive_sizes(n, h, w, c, sampling, len(script), max(lengths))
            head = lambda a: (L.adain_jpeg_decode_progressive_u8, (n, h, w, c, sampling, len(script), scans, off, ln))
        elif kind == "restart":
            q = rt.jpeg_decode_sizes(n, h, w, c, sampling, max(lengths), 0, ri)
            head = lambda a: (L.adain_jpeg_decode_restart_u8, (n, h, w, c, sampling, ri, off, ln))
        else:
            q = rt.jpeg_decode_sizes(n, h, w, c, sampling, max(lengths))
            head = lambda a: (L.adain_jpeg_decode_u8, (n, h, w, c, sampling, off, ln))
        p = (Plan().inp("files", A["files"], Bset["files"], 1).inp("blobs", A["blobs"], Bset["blobs"], 1).out("dst", n * h * w * c, 1).out("record", 8 * n, 4)
             .ws("workspace", q, 8))

        def call(a):
            fn, mid = head(a)
            return fn(a.ptr("files"), a.nbytes("files"), a.ptr("blobs"), *mid, a.ptr("dst"), a.ptr("record"), a.ptr("workspace"), q, 0, S(rt))
        p.call = call
        return p
    return plan


_TWINS = ("two jpeg_designed files and their twins of equal segment lengths (one AC value per file becomes the other value of its size): "
          "offsets, lengths, geometry, restart interval and scan script are equal")
for _kind, _call in (("jpeg", "adain_jpeg_decode_u8"), ("restart", "adain_jpeg_decode_restart_u8"), ("progressive", "adain_jpeg_decode_progressive_u8")):
    add(_call, {"dst": "the pixels of the 8 x 8 blocks (16 x 16 under 4:2:0 chroma) whose coefficient changed; the statuses are 0 in both sets"},
        _jpeg_decode_data(_kind), _jpeg_decode_plan(_kind), host_equal=_TWINS)


def _png_decode_data():
    """Stored-block streams (zlib level 0): the stream's length depends on the sizes alone.  A: two sound files; B: another picture
    in slot 0 and, in slot 1, A's stream with one bit of its Adler-32 flipped - other pixels AND another status."""
    import png_decode_cases as C
    import png_decode_ref

    import applied_image_processing_amd.png_file as png_file

    h, w = FILE_H, FILE_W
    stream = lambda px: png_file.parse(C.file_of(px, C.mixed_filters(h), level=0)).stream
    a0, a1, b0 = stream(C.noise(h, w, 3, 1)), stream(C.gradient(h, w, 3, 2)), stream(C.noise(h, w, 3, 3))
    b1 = a1[:-1] + bytes([a1[-1] ^ 1])
    sets = []
    for streams in ([a0, a1], [b0, b1]):
        offsets = [0]
        for s in streams:
            offsets.append(offsets[-1] + len(s))
        res = [png_decode_ref.decode(s, h, w, 3) for s in streams]
        sets.append({"streams": np.frombuffer(b"".join(streams), np.uint8), "_host": (tuple(offsets), h, w, 3),
                     "_status": [int(r[1]) for r in res], "_pixels": [r[0] for r in res], "_expected": {}})
    return tuple(sets)


def _png_decode_plan(rt, env, A, Bset):
    offsets, h, w, c = A["_host"]
    n = len(offsets) - 1
    q = rt.png_decode_sizes(n, h, w, c, max(b - a for a, b in zip(offsets, offsets[1:])))
    off = (ctypes.c_uint64 * (n + 1))(*offsets)
    p = Plan().inp("streams", A["streams"], Bset["streams"], 1).out("out", n * h * w * 3, 1).out("record", 8 * n, 4).ws("workspace", q, 8)
    p.call = lambda a: rt.lib().adain_png_decode_u8(a.ptr("streams"), a.nbytes("streams"), off, n, h, w, c, 3, a.ptr("out"), a.ptr("record"), a.ptr("workspace"),
                                                    q, S(rt))
    return p


add("adain_png_decode_u8", {"out": "the pixels: another picture in slot 0", "record": "the status of slot 1: its Adler-32 is wrong in set B"},
    _png_decode_data, _png_decode_plan, host_equal="stored-block streams of one size: the offsets are equal whatever the pixels")


# ---- palette control and the palette chooser ----------------------------------------------------------------------------------------------
PAL_H, PAL_W, PAL_K = 32, 44, B.PALETTE_K
_PAL_OUT = {"out": "the recoloured pixels", "index": "the index planes"}


def _palette_plan(call, second, args, ws=None, index=True):
    def plan(rt, env, A, Bset):
        q = ws(rt) if ws else 0
        p = Plan().inp("src", A["src"], Bset["src"], 1).inp(second, A[second], Bset[second], 1).out("out", N * PAL_H * PAL_W * 3, 1)
        if index:
            p.out("index", N * PAL_H * PAL_W, 1)
        if ws:
            p.ws("workspace", q, 8)
        fn = getattr(rt.lib(), call)
        p.call = lambda a: fn(*args(a.ptr), *((a.ptr("workspace"), q) if ws else ()), S(rt))
        return p
    return plan


add("adain_palette_map_u8", _PAL_OUT, split(B._map(PAL_H, PAL_W, "nearest"), ["src", "palette"], ["out", "index"], shared=("palette",)),
    _palette_plan("adain_palette_map_u8", "palette", lambda ptr: (ptr("src"), N, PAL_H, PAL_W, ptr("palette"), PAL_K, 1, None, 0, ptr("out"), ptr("index"))),
    host_equal="one palette (pattern 0's) for both sets; the host arguments are the shapes, K and the metric")
add("adain_tone_u8", {"out": "the toned pixels"}, split(B._tone(PAL_H, PAL_W), ["src", "lut"], ["out"], shared=("lut",)),
    _palette_plan("adain_tone_u8", "lut", lambda ptr: (ptr("src"), N, PAL_H, PAL_W, ptr("lut"), 1, ptr("out")), index=False))
add("adain_palette_dither_u8", _PAL_OUT, split(B._dither(PAL_H, PAL_W), ["src", "palette"], ["out", "index"], shared=("palette",)),
    _palette_plan("adain_palette_dither_u8", "palette", lambda ptr: (ptr("src"), N, PAL_H, PAL_W, ptr("palette"), PAL_K, None, 0, ptr("out"), ptr("index")),
                  ws=lambda rt: B._query("adain_palette_dither_u8_bytes", N, PAL_H, PAL_W)),
    host_equal="one palette (pattern 0's) for both sets; the host arguments are the shapes and K")


def _chooser_plan(rt, env, A, Bset):
    q = B._query("adain_quantize_palette_u8_bytes", N, PAL_H, PAL_W, 1)
    p = Plan().inp("src", A["src"], Bset["src"], 1).out("palettes", N * 768, 1).out("used", 4 * N, 4).ws("workspace", q, 8)
    p.call = lambda a: rt.lib().adain_quantize_palette_u8(a.ptr("src"), N, PAL_H, PAL_W, PAL_K, 1, a.ptr("palettes"), a.ptr("used"), a.ptr("workspace"), q, S(rt))
    return p


add("adain_quantize_palette_u8", {"palettes": "the palettes' entries"}, split(B._quantize_per_frame(PAL_H, PAL_W), ["src"], ["palettes", "used"]), _chooser_plan,
    same={"used": B._USED[1]})


# ---- metrics, their gradients, the guide loss ---------------------------------------------------------------------------------------------
MET_H, MET_W, MET_C = 17, 65, 3
_MET = {"out": "the records (ssim, mse, l1, psnr)", "map": "the SSIM maps"}


def _metrics_plan(u8):
    def plan(rt, env, A, Bset):
        dims = (MET_H, MET_W, MET_C) if u8 else (MET_C, MET_H, MET_W)
        name = "adain_image_metrics_u8" if u8 else "adain_image_metrics_f32"
        q = B._query(name + "_bytes", N, *dims)
        al = 1 if u8 else 4
        p = (Plan().inp("a", A["a"], Bset["a"], al).inp("b", A["b"], Bset["b"], al).out("out", N * 32, 8).out("map", N * MET_H * MET_W * MET_C * 4, 4)
             .ws("workspace", q, 8))
        p.call = lambda a: getattr(rt.lib(), name)(a.ptr("a"), a.ptr("b"), N, *dims, a.ptr("out"), a.ptr("map"), a.ptr("workspace"), q, S(rt))
        return p
    return plan


F32_REL = 8 * 2.0 ** -24          # test_gpu_metrics.py's bars, as test_gpu_far_batch_metrics.py restates them
PSNR_OF_REL = 10 / math.log(10)
PSNR_ULPS = 8 * 2.0 ** -46


def _metrics_held(u8):
    def held(d, e):
        import metrics_cases as C

        with open(os.path.join(C.GOLDEN, "noise.json")) as f:
            bars = json.load(f)
        want, want_map = d["_ref"]["out"], d["_ref"]["map"]
        got = e["out"].cpu().numpy().view(np.float64).reshape(N, 4)
        smap = e["map"].cpu().numpy().view(np.float32).reshape(want_map.shape)
        assert np.abs(got[:, 0] - want[:, 0]).max() <= bars["bar_frame"] and np.abs(smap.astype(np.float64) - want_map).max() <= bars["bar_map"]
        if u8:
            assert got[:, 1].tolist() == want[:, 1].tolist() and got[:, 2].tolist() == want[:, 2].tolist()          # exact
        else:
            assert np.all(np.abs(got[:, 1:3] - want[:, 1:3]) <= F32_REL * want[:, 1:3])
        for g, w in zip(got[:, 3], want[:, 3]):
            assert g == w if math.isinf(w) else abs(g - w) <= (0 if u8 else PSNR_OF_REL * F32_REL) + PSNR_ULPS * 128, (g, w)
    return held


add("adain_image_metrics_u8", _MET, split(B._metrics_u8(MET_H, MET_W, MET_C), ["a", "b"], refs=["out", "map"]), _metrics_plan(True), held=_metrics_held(True))
add("adain_image_metrics_f32", _MET, split(B._metrics_f32(MET_H, MET_W, MET_C), ["a", "b"], refs=["out", "map"]), _metrics_plan(False), held=_metrics_held(False))


def _metrics_grad_plan(rt, env, A, Bset):
    q = B._query("adain_image_metrics_grad_f32_bytes", N, MET_C, MET_H, MET_W, 1)
    fb = nbytes_of(A["a"])
    p = (Plan().inp("a", A["a"], Bset["a"], 4).inp("b", A["b"], Bset["b"], 4).inp("weights", A["weights"], Bset["weights"], 8).out("grad_a", fb, 4)
         .out("grad_b", fb, 4).ws("workspace", q, 8))
    p.call = lambda a: rt.lib().adain_image_metrics_grad_f32(a.ptr("a"), a.ptr("b"), N, MET_C, MET_H, MET_W, a.ptr("weights"), a.ptr("grad_a"), a.ptr("grad_b"),
                                                             a.ptr("workspace"), q, S(rt))
    return p


GRAD_ELEMENT, GRAD_NO_SSIM = 4 * 2.0 ** -24, 5 * 2.0 ** -24          # test_gpu_metrics_grad.py's and test_gpu_far_batch_metrics.py's


def _metrics_grad_held(d, e):
    """grad_a under test_gpu_far_batch_metrics.py's bars: the distance under bar_grad; per element, and the sign exactly, for the
    rows without an ssim weight; zeros under zero weights."""
    import metrics_grad_cases as GC
    import metrics_grad_ref as G

    bar = GC.bars()["bar_grad"]
    want = d["_ref"]["grad_a"]
    got = e["grad_a"].cpu().numpy().view(np.float32).reshape(want.shape)
    kinds = {row: kind for kind, row in B.GRAD_ROWS}
    for k in range(N):
        kind, g, w64 = kinds[tuple(float(v) for v in d["weights"][k])], got[k], want[k]
        if kind == "zero":
            assert np.all(g == 0.0), "a frame whose weights are all zero gets zeros"
            continue
        dist = float(G.distance(g[None], w64[None])[0])
        assert dist <= bar, (k, kind, dist)
        if kind in ("mse", "l1", "no_ssim"):
            assert np.all(np.abs(g - w64) <= (GRAD_NO_SSIM if kind == "no_ssim" else GRAD_ELEMENT) * np.abs(w64)), (k, kind)
            assert np.array_equal(np.sign(g), np.sign(w64)), (k, kind, "the sign of x - y is exact")


add("adain_image_metrics_grad_f32", {"grad_a": "the gradients: other pairs under other weights (A: ssim, mse, l1 alone; B: mixed, zero, no ssim)",
                                     "grad_b": "likewise"},
    split(B._metrics_grad(MET_H, MET_W, MET_C), ["a", "b", "weights"], refs=["grad_a"]), _metrics_grad_plan, held=_metrics_grad_held)


def _guide_l1_plan(rt, env, A, Bset):
    h, w = B.GUIDE_L1_HW
    q = B._query("adain_guide_l1_f32_bytes", N, h, w)
    p = (Plan().inp("image", A["image"], Bset["image"], 4).inp("guide", A["guide"], Bset["guide"], 1).out("out", 8 * N, 8)
         .out("resampled", nbytes_of(A["image"]), 4).ws("workspace", q, 8))
    p.call = lambda a: rt.lib().adain_guide_l1_f32(a.ptr("image"), a.ptr("guide"), N, h, w, B.GUIDE_GH, B.GUIDE_GW, a.ptr("out"), a.ptr("resampled"),
                                                   a.ptr("workspace"), q, S(rt))
    return p


def _guide_grad_plan(rt, env, A, Bset):
    h, w = B.GUIDE_GRAD_HW
    p = (Plan().inp("image", A["image"], Bset["image"], 4).inp("guide", A["guide"], Bset["guide"], 1).inp("weights", A["weights"], Bset["weights"], 8)
         .out("grad", nbytes_of(A["image"]), 4))
    p.call = lambda a: rt.lib().adain_guide_l1_grad_f32(a.ptr("image"), a.ptr("guide"), N, h, w, B.GUIDE_GH, B.GUIDE_GW, a.ptr("weights"), a.ptr("grad"), S(rt))
    return p


def _guide_l1_held(d, e):
    """test_gpu_guide_loss.py's rule: the loss within guide_loss_ref.loss_bound of the exact sum's (the resampled guide: bit for bit)."""
    import guide_loss_ref as R

    want = d["_ref"]["out"]
    got = e["out"].cpu().numpy().view(np.float64)
    assert np.all(np.abs(got - want) <= R.loss_bound(d["image"], want)), (got, want)


add("adain_guide_l1_f32", {"out": "the losses", "resampled": "the resampled guides"},
    split(B._guide_l1(B.GUIDE_L1_HW), ["image", "guide"], [None, "resampled"], refs=["out", None]), _guide_l1_plan, held=_guide_l1_held)
add("adain_guide_l1_grad_f32", {"grad": "the gradients: other renders under other weights, one of set B's is 0"},
    split(B._guide_l1_grad(B.GUIDE_GRAD_HW), ["image", "guide", "weights"], ["grad"]), _guide_grad_plan)


# ---- CORAL, statistics, blends ------------------------------------------------------------------------------------------------------------
CORAL_S, CORAL_C = (37, 23), (23, 37)


def _coral_plan(rt, env, A, Bset):
    (hs, ws_), (hc, wc) = CORAL_S, CORAL_C
    q = rt.lib().adain_coral_workspace_bytes(N, N, hs, ws_, hc, wc)
    rec = rt.CORAL_RECORD_BYTES
    p = Plan().inp("style", A["style"], Bset["style"], 1).inp("content", A["content"], Bset["content"], 1).ws("workspace", q, 8).out("out", N * 3 * hs * ws_ * 4, 4)
    # the records at the start of the workspace are a result: all of adain_coral_record but its last, reserved int
    p.extra = lambda a: {"records": a.bytes("workspace")[:N * rec].view(N, rec)[:, :rec - 4].contiguous().view(-1).clone()}
    p.call = lambda a: rt.lib().adain_coral(a.ptr("style"), 1, N, hs, ws_, a.ptr("content"), 1, N, hc, wc, a.ptr("out"), a.ptr("workspace"), q, S(rt))
    return p


def _coral_held(d, e):
    """test_gpu_coral.py's bars as test_gpu_far_batch_metrics.py restates them: the record under 1e-9 and 16 x 2.7e-15, every pixel
    within 1 ulp."""
    import applied_image_processing_amd.runtime as rt

    want, wantA, wantb = d["_ref"]["out"], d["_ref"]["A"], d["_ref"]["b"]
    rec = rt.CORAL_RECORD_BYTES
    full = np.zeros((N, rec), np.uint8)
    full[:, :rec - 4] = e["records"].cpu().numpy().reshape(N, rec - 4)          # the last, reserved int is not a result
    recs = rt.coral_record(tensor(full))
    pix = e["out"].cpu().numpy().view(np.float32).reshape(want.shape)
    for k in range(N):
        A_, b_ = wantA[k], wantb[k]
        scale = max(np.abs(A_).max(), np.abs(b_).max())
        err = max(np.abs(np.array(recs[k]["A"]) - A_).max(), np.abs(np.array(recs[k]["b"]) - b_).max()) / scale
        assert recs[k]["status"] == 0 and err < 1e-9 and err <= 16 * 2.7e-15, (k, err)
        want32 = want[k].astype(np.float32)
        ulp = np.spacing(np.maximum(np.abs(want32), np.float32(2.0 ** -24 * scale))).astype(np.float64)
        assert (np.abs(pix[k].astype(np.float64) - want32.astype(np.float64)) / ulp).max() <= 1.0, k


add("adain_coral", {"out": "the recoloured styles", "records": "the records' matrices and offsets"},
    split(B._coral(*CORAL_S, *CORAL_C, "u8"), ["style", "content"], refs=["out", "A", "b"]), _coral_plan, held=_coral_held,
    same={"A": "a reference value for ``records``, not an output", "b": "likewise"})


def _mean_std_plan(rt, env, A, Bset):
    c, hw = B.NHWC_C, B.NHWC_HW
    q = rt.lib().adain_mean_std_workspace_bytes(1, N, c, hw)
    p = Plan().inp("x", A["x"], Bset["x"], 4).ws("workspace", q, 8).out("mean", N * c * 4, 4).out("std", N * c * 4, 4)
    p.call = lambda a: rt.lib().adain_mean_std(a.ptr("x"), 1, N, c, hw, 1e-5, a.ptr("mean"), a.ptr("std"), a.ptr("workspace"), q, S(rt))
    return p


def _mean_std_held(d, e):
    """test_gpu_far_batch_metrics.py's bar: the mean within 1 ulp, the deviation within 2 ulp of the float64 restatement's."""
    mean64, std64 = d["_ref"]["mean"], d["_ref"]["std"]
    m, s = (e[k].cpu().numpy().view(np.float32).reshape(mean64.shape) for k in ("mean", "std"))
    em = np.abs(m - mean64) / np.spacing(np.abs(mean64.astype(np.float32)))
    es = np.abs(s - std64) / np.spacing(std64.astype(np.float32))
    assert float((np.abs(mean64) / std64).max()) <= 1e3 and (em <= 1.0).all() and (es <= 2.0).all(), (em.max(), es.max())


add("adain_mean_std", {"mean": "the means: a level per pattern", "std": "the deviations"}, split(B._mean_std_nhwc(), ["x"], refs=["mean", "std"]), _mean_std_plan,
    held=_mean_std_held)

_BLEND_IN = ["x", "c_mean", "c_std", "s_mean", "s_std"]


def _blend_plan(kind):
    def plan(rt, env, A, Bset):
        nhwc = int(kind != "pmap")
        x = A["x"]
        c, hw = (x.shape[3], x.shape[2]) if nhwc else (x.shape[1], x.shape[3])
        assert (N * c * hw) % 4 == 0
        p = Plan()
        for nm in A:
            if not nm.startswith("_"):
                p.inp(nm, A[nm], Bset[nm], 4)
        p.out("out", nbytes_of(x), 4)
        L, stats = rt.lib(), lambda a: (a.ptr("c_mean"), a.ptr("c_std"), a.ptr("s_mean"), a.ptr("s_std"))
        if kind == "alpha":
            p.call = lambda a: L.adain_blend_alpha(a.ptr("x"), nhwc, N, c, hw, *stats(a), N, 0.7, float(1 - 0.7), a.ptr("out"), S(rt))
        elif kind == "pmap":
            p.call = lambda a: L.adain_blend_pmap(a.ptr("x"), nhwc, N, c, hw, *stats(a), N, a.ptr("pmap"), N, a.ptr("out"), S(rt))
        else:
            p.call = lambda a: L.adain_blend_mix(a.ptr("x"), nhwc, N, c, hw, *stats(a), B.MIX_K, a.ptr("weights"), N, hw, 0.0, 0.0, a.ptr("pmap"), N, a.ptr("out"),
                                                 S(rt))
        return p
    return plan


_BLEND = {"out": "the blended features"}
add("adain_blend_alpha", _BLEND, split(B._blend_at("alpha", True, B.NHWC_C, B.NHWC_HW), _BLEND_IN, ["out"]), _blend_plan("alpha"))
add("adain_blend_pmap", _BLEND, split(B._blend_at("pmap", False, 4, 67), _BLEND_IN + ["pmap"], ["out"]), _blend_plan("pmap"))
add("adain_blend_mix", _BLEND, split(B._blend_at("mix_pmap", True, B.NHWC_C, B.NHWC_HW), ["x", "c_mean", "c_std", "weights", "pmap", "s_mean", "s_std"], ["out"],
                                     shared=("s_mean", "s_std")), _blend_plan("mix"),
    host_equal="the four styles are the batch's, one value for both sets; the host arguments are the shapes and k")


# ---- single conv layers, the packs, the encoder's first layer -------------------------------------------------------------------------
def _conv_plan(entry):
    def plan(rt, env, A, Bset):
        import torch

        x = A["x"]
        _n, h, w, cin = x.shape
        cout = A["w"].shape[0]
        wt = tensor(A["w"]).to(env.device)
        up = entry == "poly"
        packed = (rt.conv3x3_up2x_poly_pack if up else rt.conv3x3_wino_pack)(wt)
        p = Plan().inp("x", x, Bset["x"], 256).inp("packed", packed).inp("bias", A["b"], align=256).out("out", N * (4 if up else 1) * h * w * cout * 4, 256)
        L = rt.lib()
        if up:
            p.call = lambda a: L.adain_conv3x3_up2x_poly(a.ptr("x"), a.ptr("out"), a.ptr("packed"), a.ptr("bias"), N, h, w, cin, cout, 1, S(rt))
        else:
            p.call = lambda a: L.adain_conv3x3_wino(a.ptr("x"), a.ptr("out"), a.ptr("packed"), a.ptr("bias"), N, h, w, h, w, cin, cout, D, 1, 0, 5, S(rt))
        return p
    return plan


_CONV = {"out": "the layer's output: other integer-valued images"}
_SAME_WEIGHTS = "one layer (weights, bias) for both sets; the host arguments are the shapes"
add("adain_conv3x3_wino", _CONV, split(B._conv("wino"), ["x", "w", "b"], ["out"], shared=("w", "b")), _conv_plan("wino"), host_equal=_SAME_WEIGHTS)
add("adain_conv3x3_up2x_poly", _CONV, split(B._conv("poly"), ["x", "w", "b"], ["out"], shared=("w", "b")), _conv_plan("poly"), host_equal=_SAME_WEIGHTS)


def _layer(seed, cin, cout):
    rng = np.random.default_rng([79, seed])
    return (rng.standard_normal((cout, cin, 3, 3)) * (2.0 / (9 * cin)) ** 0.5).astype(np.float32), (rng.standard_normal(cout) * 0.1).astype(np.float32)


SPLIT = (1, 16, 16, 512, 256)          # n, h, w, cin, cout: a case the latency schedule splits (test_gpu_abi_memory.py)


def _split_data():
    n, h, w, cin, cout = SPLIT
    wt, b = _layer(3, cin, cout)
    return tuple(dict(x=noise_f32(4 + s, n, h, w, cin), w=wt, b=b) for s in (0, 1))


def _split_plan(rt, env, A, Bset):
    import torch

    n, h, w, cin, cout = SPLIT
    L = rt.lib()
    with torch.cuda.device(env.device):
        q = L.adain_conv3x3_wino4_split_workspace_bytes(n, h, w, cin, cout)
    assert q > 0, "the case must be one the latency schedule splits"
    packed = rt.conv3x3_wino_pack(tensor(A["w"]).to(env.device))
    p = Plan().inp("x", A["x"], Bset["x"], 256).inp("packed", packed).inp("bias", A["b"], align=256).ws("workspace", q, 256).out("out", n * h * w * cout * 4, 256)
    p.call = lambda a: L.adain_conv3x3_wino4_split(a.ptr("x"), a.ptr("out"), a.ptr("packed"), a.ptr("bias"), n, h, w, h, w, cin, cout, D, 1, 0, a.ptr("workspace"), q,
                                                   S(rt))
    return p


add("adain_conv3x3_wino4_split", {"out": "the layer's output: another input"}, _split_data, _split_plan, host_equal=_SAME_WEIGHTS)


def _pack_plan(which):
    def plan(rt, env, A, Bset):
        cout, cin = A["w"].shape[:2]
        floats = getattr(rt.lib(), f"adain_conv3x3_{which}_packed_floats")(cin, cout)
        p = Plan().inp("w", A["w"], Bset["w"], 256).out("packed", floats * 4, 256)
        p.call = lambda a: getattr(rt.lib(), f"adain_conv3x3_{which}_pack")(a.ptr("w"), a.ptr("packed"), cin, cout, S(rt))
        return p
    return plan


_PACKED = {"packed": "the packed weights: another layer"}
add("adain_conv3x3_wino4_pack", _PACKED, lambda: tuple(dict(w=_layer(7 + s, 48, 96)[0]) for s in (0, 1)), _pack_plan("wino4"))
add("adain_conv3x3_up2x_poly_pack", _PACKED, lambda: tuple(dict(w=_layer(9 + s, 48, 96)[0]) for s in (0, 1)), _pack_plan("up2x_poly"))


def _net_pack_data(net):
    def data():
        import applied_image_processing_amd.runtime as rt
        import applied_image_processing_amd.synth as synth

        sets = []
        for seed in (0, 1):
            sd = synth.vgg_state_dict(seed, full=False) if net == "encoder" else synth.decoder_state_dict(seed)
            keys = rt.ENC_KEYS if net == "encoder" else rt.DEC_KEYS
            d = {}
            for i, k in enumerate(keys):
                d[f"w{i}"], d[f"b{i}"] = np.asarray(sd[f"{k}.weight"], dtype=np.float32), np.asarray(sd[f"{k}.bias"], dtype=np.float32)
            sets.append(d)
        return tuple(sets)
    return data


def _net_pack_plan(net):
    def plan(rt, env, A, Bset):
        k = len(A) // 2
        floats = getattr(rt.lib(), f"adain_{net}_packed_floats")()
        p = Plan()
        for i in range(k):
            p.inp(f"w{i}", A[f"w{i}"], Bset[f"w{i}"], 256).inp(f"b{i}", A[f"b{i}"], Bset[f"b{i}"], 256)
        p.out("packed", floats * 4, 256)

        def call(a):
            wp, _k1 = host_ptrs(*[a.ptr(f"w{i}") for i in range(k)])
            bp, _k2 = host_ptrs(*[a.ptr(f"b{i}") for i in range(k)])
            return getattr(rt.lib(), f"adain_{net}_pack")(wp, bp, a.ptr("packed"), S(rt))
        p.call = call
        return p
    return plan


_PTRS = "the host arrays hold the layers' device pointers, which are the arena's regions in both sets"
add("adain_encoder_pack", {"packed": "the packed network: the weights of another seed"}, _net_pack_data("encoder"), _net_pack_plan("encoder"), host_equal=_PTRS)
add("adain_decoder_pack", {"packed": "the packed network: the weights of another seed"}, _net_pack_data("decoder"), _net_pack_plan("decoder"), host_equal=_PTRS)


def _first_plan(rt, env, A, Bset):
    import edge_exact as E

    packed = rt.pack_encoder(E.first_state_dict(env.weights[0]), env.device)
    p = Plan().inp("image", A["image"], Bset["image"], 256).inp("packed", packed).out("relu1_1", N * B.FIRST_H * B.FIRST_W * 64 * 4, 256)
    p.call = lambda a: rt.lib().adain_encode_relu1_1(a.ptr("image"), 0, a.ptr("relu1_1"), a.ptr("packed"), N, B.FIRST_H, B.FIRST_W, S(rt))
    return p


add("adain_encode_relu1_1", {"relu1_1": "the first layer's output: other integer-valued images"}, split(B._first_layer(), ["image"], ["relu1_1"]), _first_plan,
    host_equal="one packed encoder for both sets; the host arguments are the shapes")


# ---- the network calls: seeded noise, as in their arena tests ---------------------------------------------------------------------------
NET_N, NET_H, NET_W = 2, 37, 99
_NET = "one packed network for both sets; the host arguments are the shapes"


def _encode_plan(u8):
    def plan(rt, env, A, Bset):
        import torch

        L = rt.lib()
        n, h, w = NET_N, NET_H, NET_W
        hc, wc = rt.encoded_size(h, w)
        with torch.cuda.device(env.device):
            q = L.adain_encode_workspace_bytes(n, h, w)
        fn = L.adain_encode_u8 if u8 else L.adain_encode
        p = Plan().inp("image", A["image"], Bset["image"], 256).inp("packed", env.packed[0]).ws("workspace", q, 256).out("feat", n * hc * wc * 512 * 4, 256)
        p.call = lambda a: fn(a.ptr("image"), a.ptr("feat"), a.ptr("packed"), a.ptr("workspace"), q, n, h, w, None, S(rt))
        return p
    return plan


_FEAT = {"feat": "relu4_1 of other images"}
add("adain_encode", _FEAT, lambda: tuple(dict(image=np.clip(np.abs(noise_f32(100 + s, NET_N, 3, NET_H, NET_W)), 0, 1)) for s in (0, 1)), _encode_plan(False),
    host_equal=_NET)
add("adain_encode_u8", _FEAT, lambda: tuple(dict(image=noise_u8(102 + s, NET_N, NET_H, NET_W, 3)) for s in (0, 1)), _encode_plan(True), host_equal=_NET)

MULTI = [(2, 37, 99), (1, 9, 9)]


def _multi_plan(rt, env, A, Bset):
    import torch

    L, k = rt.lib(), len(MULTI)
    Ns, Hs, Ws = ints(*[s[0] for s in MULTI]), ints(*[s[1] for s in MULTI]), ints(*[s[2] for s in MULTI])
    with torch.cuda.device(env.device):
        q = L.adain_encode_multi_workspace_bytes(k, Ns, Hs, Ws)
    p = Plan()
    for i in range(k):
        p.inp(f"image{i}", A[f"image{i}"], Bset[f"image{i}"], 256)
    p.inp("packed", env.packed[0]).ws("workspace", q, 256)
    for i, (n, h, w) in enumerate(MULTI):
        hc, wc = rt.encoded_size(h, w)
        p.out(f"feat{i}", n * hc * wc * 512 * 4, 256)

    def call(a):
        ip, _k1 = host_ptrs(*[a.ptr(f"image{i}") for i in range(k)])
        fp, _k2 = host_ptrs(*[a.ptr(f"feat{i}") for i in range(k)])
        return L.adain_encode_multi(k, ip, fp, Ns, Hs, Ws, a.ptr("packed"), a.ptr("workspace"), q, None, S(rt))
    p.call = call
    return p


add("adain_encode_multi", {"feat0": "relu4_1 of other images", "feat1": "likewise"},
    lambda: tuple({f"image{i}": np.clip(np.abs(noise_f32(110 + 10 * s + i, n, 3, h, w)), 0, 1) for i, (n, h, w) in enumerate(MULTI)} for s in (0, 1)), _multi_plan,
    host_equal="the host arrays hold the sizes and the segments' device pointers, the arena's regions in both sets")


def _decode_plan(n, hc, wc):
    def plan(rt, env, A, Bset):
        import torch

        L = rt.lib()
        with torch.cuda.device(env.device):
            q = L.adain_decode_workspace_bytes(n, hc, wc)
            if n == 1:
                assert L.adain_conv3x3_wino4_split_workspace_bytes(n, hc, wc, 512, 256) > 0, "the latency row must split a layer"
        p = Plan().inp("feat", A["feat"], Bset["feat"], 256).inp("packed", env.packed[1]).ws("workspace", q, 256).out("image", n * 3 * 64 * hc * wc * 4, 256)
        p.call = lambda a: L.adain_decode(a.ptr("feat"), a.ptr("image"), a.ptr("packed"), a.ptr("workspace"), q, n, hc, wc, None, S(rt))
        return p
    return plan


_IMG = {"image": "the decoded images: other features"}
add("adain_decode", _IMG, lambda: tuple(dict(feat=np.abs(noise_f32(120 + s, 2, 5, 13, 512))) for s in (0, 1)), _decode_plan(2, 5, 13), host_equal=_NET)
# the schedule is enqueue-time state of the calling thread: what was enqueued under LATENCY at capture is what every replay runs
add("adain_decode", _IMG, lambda: tuple(dict(feat=np.abs(noise_f32(122 + s, 1, 8, 8, 512))) for s in (0, 1)), _decode_plan(1, 8, 8), id="adain_decode/latency",
    latency=True, host_equal=_NET)

STY_MASK = (1, 3, 20, 50)          # mask_n, mask_c, mh, mw; float: the bilinear + composite path, with depth maps
STY_DEPTH = [(23, 31), (24, 31)]
STY_K = 2


def _stylize_data(kind):
    def data():
        sets = []
        for s in (0, 1):
            rows = {"one": 1, "ex": NET_N, "mix": STY_K}[kind]
            d = dict(frames=noise_u8(130 + s, NET_N, NET_H, NET_W, 3), s_mean=noise_f32(132 + s, rows, 512), s_std=np.abs(noise_f32(134 + s, rows, 512)) + 0.1,
                     mask=(noise_f32(136 + s, *STY_MASK) > 0).astype(np.float32))
            for i, (dh, dw) in enumerate(STY_DEPTH):
                d[f"depth{i}"] = np.abs(noise_f32(138 + 10 * s + i, dh, dw))
            if kind == "mix":
                d["weights"] = (0.05 + 0.85 * np.random.default_rng([80, s]).random((NET_N, STY_K, 1))).astype(np.float32)
            d["_host"] = (tuple(STY_DEPTH),)
            sets.append(d)
        return tuple(sets)
    return data


def _stylize_plan(kind):
    def plan(rt, env, A, Bset):
        import torch

        L = rt.lib()
        n, h, w = NET_N, NET_H, NET_W
        mn, mc, mh, mw = STY_MASK
        oh, ow = ctypes.c_int(), ctypes.c_int()
        L.adain_stylize_u8_out_size(h, w, 1, ctypes.byref(oh), ctypes.byref(ow))
        query = {"one": "adain_stylize_u8_workspace_bytes", "ex": "adain_stylize_u8_ex_workspace_bytes", "mix": "adain_stylize_u8_mix_workspace_bytes"}[kind]
        with torch.cuda.device(env.device):
            q = getattr(L, query)(n, h, w, 1, mn, mc, mh, mw, 1)
        p = Plan().inp("frames", A["frames"], Bset["frames"], 256).inp("enc", env.packed[0]).inp("dec", env.packed[1])
        for nm in ("s_mean", "s_std", "mask") + tuple(f"depth{i}" for i in range(n)) + (("weights",) if kind == "mix" else ()):
            p.inp(nm, A[nm], Bset[nm], 256)
        p.ws("workspace", q, 256).out("out", n * oh.value * ow.value * 3, 256)
        dh, dw = ints(*[s[0] for s in STY_DEPTH]), ints(*[s[1] for s in STY_DEPTH])

        def call(a):
            dp, _k = host_ptrs(*[a.ptr(f"depth{i}") for i in range(n)])
            head = (a.ptr("frames"), n, h, w, a.ptr("enc"), a.ptr("dec"), a.ptr("s_mean"), a.ptr("s_std"))
            tail = (0.5, 0.5, dp, dh, dw, 0.15, 20.0, a.ptr("mask"), 1, mn, mc, mh, mw, a.ptr("out"), a.ptr("workspace"), q, S(rt))
            if kind == "one":
                return L.adain_stylize_u8(*head, *tail)
            if kind == "ex":
                return L.adain_stylize_u8_ex(*head, n, *tail)
            return L.adain_stylize_u8_mix(*head, STY_K, a.ptr("weights"), n, 1, *tail)
        p.call = call
        return p
    return plan


_STY = {"out": "the stylised frames: other frames, styles, masks and depth maps"}
_STY_HOST = "depth_h_host / depth_w_host are the depth maps' shapes, equal in both sets; the pointer array holds the arena's regions"
add("adain_stylize_u8", _STY, _stylize_data("one"), _stylize_plan("one"), host_equal=_STY_HOST)
add("adain_stylize_u8_ex", _STY, _stylize_data("ex"), _stylize_plan("ex"), host_equal=_STY_HOST)
add("adain_stylize_u8_mix", _STY, _stylize_data("mix"), _stylize_plan("mix"), host_equal=_STY_HOST)


# ---- Farneback ----------------------------------------------------------------------------------------------------------------------------
FB_H, FB_W = 37, 61


def smooth_u8(h, w, seed):
    y, x = np.meshgrid(np.arange(h, dtype=np.float32), np.arange(w, dtype=np.float32), indexing="ij")
    v = 128 + 60 * np.sin(x / 7 + seed) * np.cos(y / 5 - seed) + 40 * np.sin((x + 2 * y) / 11 + 2 * seed)
    return np.clip(v, 0, 255).astype(np.uint8)


def _pyramid_holes(rt, h, w):
    import applied_image_processing_amd.flow as flow

    return block_holes([f for (wl, hl, _k, _s) in flow.level_schedule(h, w, 0.5, 5) for f in (wl * hl, 5 * wl * hl)])


def _expand_plan(rt, env, A, Bset):
    L, (h, w) = rt.lib(), (FB_H, FB_W)
    pb, q = L.adain_farneback_pyramid_bytes(h, w, 0.5, 5), L.adain_farneback_workspace_bytes(h, w)
    holes, floats = _pyramid_holes(rt, h, w)
    assert 4 * floats == pb
    p = Plan().inp("gray", A["gray"], Bset["gray"], 256).ws("workspace", q, 256).out("pyramid", pb, 256, holes)
    p.call = lambda a: L.adain_farneback_expand(a.ptr("gray"), h, w, 0.5, 5, 7, 1.5, a.ptr("pyramid"), a.ptr("workspace"), q, S(rt))
    return p


def _fb_flow_plan(rt, env, A, Bset):
    import torch

    import applied_image_processing_amd.flow as flow

    L, (h, w) = rt.lib(), (FB_H, FB_W)
    fb = flow.Farneback(h, w)
    q = L.adain_farneback_workspace_bytes(h, w)
    holes, _floats = _pyramid_holes(rt, h, w)
    pyr = {k: [fb.expand(torch.from_numpy(d[g]).to(env.device)) for g in ("prev", "next")] for k, d in (("A", A), ("B", Bset))}
    torch.cuda.synchronize()
    p = (Plan().inp("prev", pyr["A"][0], pyr["B"][0], 256, holes).inp("next", pyr["A"][1], pyr["B"][1], 256, holes).ws("workspace", q, 256)
         .out("flow", 2 * h * w * 4, 256))
    p.call = lambda a: L.adain_farneback_flow(a.ptr("prev"), a.ptr("next"), h, w, 0.5, 5, 15, 3, 0, a.ptr("flow"), a.ptr("workspace"), q, S(rt))
    return p


add("adain_farneback_expand", {"pyramid": "the polynomial pyramid of another frame"}, lambda: (dict(gray=smooth_u8(FB_H, FB_W, 0.0)), dict(gray=smooth_u8(FB_H, FB_W, 0.3))),
    _expand_plan)
add("adain_farneback_flow", {"flow": "the flow of another pair of frames"},
    lambda: (dict(prev=smooth_u8(FB_H, FB_W, 0.0), next=smooth_u8(FB_H, FB_W, 0.3)), dict(prev=smooth_u8(FB_H, FB_W, 0.5), next=smooth_u8(FB_H, FB_W, 0.9))),
    _fb_flow_plan, host_equal="the pyramids of both sets are expanded on the device from the rows' frames; the host arguments are the shapes and parameters")


# ---- the localized pipeline's colour calls ----------------------------------------------------------------------------------------------
def _colour_data(combine):
    def data():
        import colour_fixtures as F

        names = ("content", "stylised", "mask") if combine else ("fg", "bg")
        return tuple(dict(zip(names, (np.ascontiguousarray(v) for v in (F.combine_fixture if combine else F.fixture)(which)))) for which in ("equal_n", "fg_plus1"))
    return data


def _colour_plan(combine):
    def plan(rt, env, A, Bset):
        L = rt.lib()
        names = [k for k in A if not k.startswith("_")]
        h, w = A[names[0]].shape[:2]
        q = L.adain_colour_transfer_workspace_bytes(h, w)
        p = Plan()
        for nm in names:
            p.inp(nm, A[nm], Bset[nm], 1)
        p.ws("workspace", q, 8).out("out", h * w * 3, 1)
        p.extra = lambda a: {"record": a.bytes("workspace")[:rt.COLOUR_RECORD_BYTES].clone()}          # the record at its start is a result
        if combine:
            p.call = lambda a: L.adain_localized_combine_u8(a.ptr("content"), a.ptr("stylised"), a.ptr("mask"), a.ptr("out"), h, w, a.ptr("workspace"), S(rt))
        else:
            p.call = lambda a: L.adain_colour_transfer_u8(a.ptr("fg"), a.ptr("bg"), a.ptr("out"), h, w, a.ptr("workspace"), S(rt))
        return p
    return plan


_COLOUR = {"out": "the pixels", "record": "the record: another relation of the regions' sizes (equal_n / fg_plus1)"}
add("adain_colour_transfer_u8", _COLOUR, _colour_data(False), _colour_plan(False))
add("adain_localized_combine_u8", _COLOUR, _colour_data(True), _colour_plan(True))

BY_ID = {r.id: r for r in ROWS}
assert len(BY_ID) == len(ROWS)


def inputs_of(d):
    return {k: v for k, v in d.items() if not k.startswith("_")}
