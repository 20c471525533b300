"""The case table and the helpers of the far-batch tests (test_far_batch_host.py, test_gpu_far_batch_*.py).  Not a test module.

Every entry point that takes ``n`` frames forms ``frame index * frame bytes`` in its kernels.  The rest of the suite runs each kernel
at the smallest shapes that reach its branches, so an offset formed in 32 bits would go unnoticed: it does not fault, frame 63 550
of a batch of 67 584-byte frames reads and writes inside frame 0.  The cases here hand each call one batch whose buffers pass 2^32
bytes, made of many small frames so that the host references stay cheap:

* a batch holds ``n <= 65535`` frames of ``F`` bytes in each buffer the case aims at, ``n F > 2^32``; by default n = 65535 frames of
  128 x 176 x 3 bytes (F = 67 584, 4.12 GiB: frames 31 776 .. straddle 2^31, frames 63 550 .. 65 534 lie past 2^32);
* ``F`` does not divide 2^32 (a wrapped offset lands inside a frame, 2^32 mod 67 584 = 4096);
* frame ``i`` is pattern ``i mod P`` of P = 7 distinct small frames from the call's own case generators, and P is coprime to
  floor(2^32 / F), so the frame a wrapped offset lands in holds another pattern (63 550 mod 7 = 4);
* the batch is tiled on the device from the P uploaded patterns (``tile``); the expected values are the P results of the restatement
  the call's own tests use, held to the bar those tests use; every result buffer is filled with 0xA5 before the call (``poisoned``)
  and every frame of it is compared with ``expected[i mod P]`` on the device (``bad_frames``), in pieces of at most 1 GiB;
* a test holds at most 32 GiB of device memory: ``reserve`` asserts that from the case's buffer sizes (the library's own size
  queries where a buffer is a workspace or a block of file rows) and from ``torch.cuda.mem_get_info()`` before anything is
  allocated, and fails - it does not skip - when the memory is short.

``CASES`` states per case which of the call's buffers that scale with ``n`` pass 2^32 (``past``) and which do not, with the reason
(``below``).  test_far_batch_host.py checks the arithmetic of every row without a device.

The file decoders (adain_png_decode_u8, adain_jpeg_decode_u8, _restart_u8, _progressive_u8) take their segments by ``uint64`` offsets
into one buffer of streams, from host tables.  Their rows put the P files' segments, tiled on the device group by group, behind a
``LEAD`` of more than 2^32 bytes, so that every offset lies past 2^32, and decode n = 65535 files, so that ``dst`` passes 2^32 in the
same call; the offsets and lengths are computed arithmetically (``decode_tables``), no file is parsed more than once.

The gradient of the metrics (adain_image_metrics_grad_f32) runs without ``grad_b``: that form needs nine buffers of more than 2^32
bytes each (a, b, two gradients, five derivative planes), 37 GiB at the smallest legal frame, which no case under the cap can hold.
Its two extra planes lie 3 and 4 pitches behind the first and are reached by the ``size_t`` product ``j * dplane_pitch`` that plane 2
uses, which the case here already puts past 8 GiB.

Out of scope: the launches of include/adain_hip.h that are no ``call`` of a row are the keys of ``OUT_OF_SCOPE``, each with its
reason; test_far_batch_host.py holds the two to the header, so that a new entry point has a row or a reason."""
import functools
import math

import numpy as np

P = 7                      # distinct patterns; frame i holds pattern i % P
N = 65535                  # the largest batch every call takes
H, W = 128, 176            # the default frame: 128 x 176 x 3 bytes
TWO32 = 1 << 32
CAP = 32 << 30             # device memory one test may hold
PIECE = 1 << 30            # largest temporary of a comparison
F32 = np.float32


class Case:
    """One row of the table.  ``buffers(n)``: [(name, role, bytes)] of every buffer of the call that scales with ``n`` (role: source,
    result, workspace, rows, streams), sized by the library's queries where the library sizes them; ``past``: the names that pass 2^32 in this
    case; ``below``: {name: why it stays below 2^32 here}; ``make()``: (inputs, expected) - tuples of arrays whose first axis is the P
    patterns; ``same``: {index into expected: why that value does not differ from pattern to pattern} - every other expected value
    differs pairwise."""

    def __init__(self, id, family, call, n, frames, buffers, past, make, below=None, same=None):
        self.id, self.family, self.call, self.n, self.frames = id, family, call, n, frames
        self._buffers, self.past, self.below, self._make, self.same = buffers, tuple(past), dict(below or {}), make, dict(same or {})

    def buffers(self):
        return self._buffers(self.n)

    def frame_bytes(self, name):
        """Bytes per frame of buffer ``name`` (the floor, for a workspace whose blocks are rounded to 256 bytes)."""
        return dict((b[0], b[2]) for b in self.buffers())[name] // self.n

    def total_bytes(self):
        return sum(b[2] for b in self.buffers())

    @functools.lru_cache(maxsize=None)
    def make(self):
        inputs, expected = self._make()
        assert all(len(a) == P for a in inputs) and all(len(e) == P for e in expected), self.id
        return inputs, expected

    def __repr__(self):
        return f"Case({self.id})"


def check_arithmetic(case):
    """The rules of the module docstring for one row; AssertionError names the row and the rule."""
    assert 1 <= case.n <= N, (case.id, "n")
    names = [b[0] for b in case.buffers()]
    assert set(case.past) | set(case.below) == set(names) and not set(case.past) & set(case.below), (case.id, "every buffer is past or below", names)
    for name, role, nbytes in case.buffers():
        if name in case.past:
            F = case.frame_bytes(name)
            assert nbytes > TWO32 and case.n * F > TWO32, (case.id, name, "n F > 2^32", nbytes)
            if role in ("workspace", "streams"):          # several blocks, each with a per-frame stride of the library's choosing; segments of
                continue                                  # their files' lengths behind a lead: only the size is the case's
            assert TWO32 % F != 0, (case.id, name, "F divides 2^32", F)
            assert math.gcd(P, TWO32 // F) == 1, (case.id, name, "P is not coprime to floor(2^32 / F)", F, TWO32 // F)
        else:
            assert nbytes <= TWO32, (case.id, name, "listed as below 2^32 but passes it", nbytes)
    assert case.total_bytes() + 2 * PIECE <= CAP, (case.id, "memory cap", case.total_bytes())


def distinct(arrays):
    """The P rows of an expected value differ pairwise."""
    rows = [a if isinstance(a, bytes) else np.ascontiguousarray(a).tobytes() for a in arrays]
    return len(set(rows)) == len(rows) == P


# ---- device helpers (torch is imported where they run) ----------------------------------------------------------------------------------------
def reserve(case, dev):
    """Before anything is allocated: the case fits the 32 GiB cap and the device has that much free.  Fails, does not skip."""
    import torch

    need = case.total_bytes() + 2 * PIECE
    assert need <= CAP, f"{case.id}: {need} bytes are more than a test may hold"
    torch.cuda.empty_cache()
    free, _total = torch.cuda.mem_get_info(dev)
    assert free >= need, f"{case.id}: needs {need >> 20} MiB of device memory, {free >> 20} MiB are free"


def release():
    import torch

    torch.cuda.synchronize()
    torch.cuda.empty_cache()


def upload(patterns, dev):
    import torch

    a = np.array(patterns, order="C", copy=True)          # a few small frames: a writable copy (a broadcast view is read-only)
    return torch.from_numpy(a.view(np.uint8) if a.dtype == np.bool_ else a).to(dev)


def tile(patterns, n, dev):
    """[n, ...] on the device with frame i = patterns[i % P]; nothing of the batch's size exists on the host."""
    import torch

    p = patterns if isinstance(patterns, torch.Tensor) else upload(patterns, dev)
    assert p.shape[0] == P
    out = torch.empty((n,) + tuple(p.shape[1:]), dtype=p.dtype, device=dev)
    for k in range(P):
        out[k::P] = p[k]
    return out


def poisoned(shape, dtype, dev):
    """A result buffer of ``shape`` whose every byte is 0xA5."""
    import torch

    t = torch.empty(shape, dtype=dtype, device=dev)
    t.view(-1).view(torch.uint8).fill_(0xA5)
    return t


_BITS = {1: "uint8", 2: "int16", 4: "int32", 8: "int64"}


def _bits(t):
    import torch

    return t if t.dtype in (torch.uint8, torch.int16, torch.int32, torch.int64) else t.view(getattr(torch, _BITS[t.element_size()]))


def bad_frames(got, expected, limit=8, lengths=None):
    """The first ``limit`` indices i with got[i] != expected[i % P], bit for bit, compared on the device residue by residue in pieces
    of at most 1 GiB.  ``lengths`` (ints, one per pattern): only the first lengths[k] elements of a row of pattern k count."""
    import torch

    n = got.shape[0]
    expected = expected if isinstance(expected, torch.Tensor) else upload(expected, got.device)
    if got.dim() == 1:
        got, expected = got[:, None], expected[:, None]
    g, e = _bits(got).flatten(1), _bits(expected).flatten(1)
    assert e.shape[0] == P and (lengths is not None or e.shape[1] == g.shape[1]), (g.shape, e.shape)
    bad = []
    for k in range(P):
        rows = g[k::P]
        width = g.shape[1] if lengths is None else int(lengths[k])
        if width == 0:
            continue
        step = max(1, PIECE // width)
        for r0 in range(0, rows.shape[0], step):
            ne = (rows[r0:r0 + step, :width] != e[k, :width]).any(dim=1)
            bad += [k + P * (r0 + int(j)) for j in torch.nonzero(ne).flatten()[:limit].tolist()]
    bad.sort()
    assert all(0 <= i < n for i in bad)
    return bad[:limit]


def assert_frames(what, got, expected, lengths=None):
    bad = bad_frames(got, expected, lengths=lengths)
    assert not bad, f"{what}: frames {bad} (first of those that differ) do not hold the result of their pattern; 2^32 / F = {TWO32 / max(1, got[0].numel() * got.element_size()):.1f}"


def device_of(dev):
    import torch

    return torch.device(dev)


def run_equal(rt, case, dev, outs, args, workspace=0, shared=0):
    """The common shape of a far-batch test whose bar is equality: tile the case's inputs, poison the results ``outs`` = [(shape per
    frame, dtype)] (and a workspace of ``workspace`` bytes), make the one call ``args(*inputs, *outs[, ws]) -> the C arguments``, compare
    every frame of result j with ``expected[j]`` and every input with its pattern, free everything.  The last ``shared`` inputs are one
    value for the whole batch (a palette, a filter): row 0 is uploaded as it is.  The bytes held are asserted to be the case's
    ``buffers()``."""
    import torch

    reserve(case, dev)
    inputs, expected = case.make()
    per_frame = inputs[:len(inputs) - shared]
    tiled = [tile(x, case.n, dev) for x in per_frame]
    once = [upload(x[0], dev) for x in inputs[len(per_frame):]]
    results = [poisoned((case.n,) + tuple(shape), dtype, dev) for shape, dtype in outs]
    ws = [poisoned((workspace,), torch.uint8, dev)] if workspace else []
    held = sum(t.numel() * t.element_size() for t in tiled + results + ws)
    try:
        assert held == case.total_bytes(), (case.id, held, case.total_bytes())
        rt.call(case.call, device_of(dev), *args(*tiled, *once, *results, *ws))
        torch.cuda.synchronize()
        for j, r in enumerate(results):
            assert_frames(f"{case.id}: result {j}", r, expected[j])
        for t, x in zip(tiled, per_frame):
            assert_frames(case.id + ": an input changed", t, x)
    finally:
        del tiled, results, ws, once
        release()


# ---- the cases ------------------------------------------------------------------------------------------------------------------------------------
def _fixed(*buffers):
    """buffers(n) of a call whose buffers are n frames of a fixed size each: (name, role, bytes per frame)."""
    return lambda n: [(name, role, n * per) for name, role, per in buffers]


def _quantize(c, h, w):
    def make():
        import pixel_ref as R

        x = R.fill(R.quantiser_edge_values(), (P, c, h, w), seed=c + h)
        return (x,), (R.quantize_u8(x),)
    return make


def _to_f32(c, h, w):
    def make():
        import pixel_ref as R

        u = R.fill(np.arange(256, dtype=np.uint8), (P, h, w, c), seed=c + h)
        return (u,), (R.u8_to_f32(u),)
    return make


def _resize(which, hi, wi, ho, wo):
    def make():
        import applied_image_processing_amd.synth as synth
        import pixel_ref as R

        x = synth.uniform_sym(100 + hi + wi, (P, 1, hi, wi), 2.0)
        return (x,), ((R.resize_bilinear if which == "bilinear" else R.resize_nearest)(x, ho, wo),)
    return make


def _composite(hw):
    def make():
        """P planes; the call sees them as n images of 3 channels, pattern = plane % P."""
        import applied_image_processing_amd.synth as synth
        import pixel_ref as R

        a, b = synth.image(400, P, 1, hw, c=1), synth.uniform_sym(410, (P, 1, 1, hw), 1.0)
        m = synth.image(420, P, 1, hw, c=1)
        return (a, b, m), (R.mask_composite(a, b, m),)
    return make


def _area(hi, wi, c, ho, wo):
    def make():
        from oracle import adain_oracle as O

        frames = np.random.default_rng([11, hi, wi, c]).integers(0, 256, (P, hi, wi, c), dtype=np.uint8)
        return (frames,), (np.stack([O.resize_area_u8(f, (wo, ho)).reshape(ho, wo, c) for f in frames]),)
    return make


def _transpose(to_nhwc, c, hw):
    def make():
        import applied_image_processing_amd.synth as synth

        x = synth.uniform_sym(900 + c + hw, (P, c, hw) if to_nhwc else (P, hw, c), 1.0)
        return (x,), (np.ascontiguousarray(np.transpose(x, (0, 2, 1))),)
    return make


PIXEL = [
    Case("quantize_u8/rgb4", "pixel", "adain_quantize_u8", N, "float32 [n,3,128,176] -> uint8 [n,128,176,3]",
         _fixed(("src", "source", 3 * H * W * 4), ("out", "result", 3 * H * W)), ("src", "out"), _quantize(3, H, W)),
    Case("quantize_u8/generic", "pixel", "adain_quantize_u8", N, "float32 [n,1,257,257] -> uint8 [n,257,257,1] (hw % 4 != 0, c = 1: the one-pixel kernel)",
         _fixed(("src", "source", 257 * 257 * 4), ("out", "result", 257 * 257)), ("src", "out"), _quantize(1, 257, 257)),
    Case("u8_to_f32/rgb4", "pixel", "adain_u8_to_f32", N, "uint8 [n,128,176,3] -> float32 [n,3,128,176]",
         _fixed(("src", "source", 3 * H * W), ("out", "result", 3 * H * W * 4)), ("src", "out"), _to_f32(3, H, W)),
    Case("u8_to_f32/generic", "pixel", "adain_u8_to_f32", N, "uint8 [n,257,257,1] -> float32 [n,1,257,257]",
         _fixed(("src", "source", 257 * 257), ("out", "result", 257 * 257 * 4)), ("src", "out"), _to_f32(1, 257, 257)),
    Case("resize_bilinear", "pixel", "adain_resize_bilinear", N, "65535 float32 planes 129 x 131 -> 131 x 127 (scalar stores)",
         _fixed(("src", "source", 129 * 131 * 4), ("out", "result", 131 * 127 * 4)), ("src", "out"), _resize("bilinear", 129, 131, 131, 127)),
    Case("resize_nearest", "pixel", "adain_resize_nearest", N, "65535 float32 planes 129 x 131 -> 127 x 136 (b128 stores)",
         _fixed(("src", "source", 129 * 131 * 4), ("out", "result", 127 * 136 * 4)), ("src", "out"), _resize("nearest", 129, 131, 127, 136)),
    Case("mask_composite", "pixel", "adain_mask_composite", N, "21845 images x 3 channels = 65535 float32 planes of 16899, a mask per image and channel",
         _fixed(("content", "source", 16899 * 4), ("stylized", "source", 16899 * 4), ("mask", "source", 16899 * 4), ("out", "result", 16899 * 4)),
         ("content", "stylized", "mask", "out"), _composite(16899)),
    Case("resize_area_u8/linear", "pixel", "adain_resize_area_u8", N, "uint8 [n,128,176,3] -> [n,130,177,3] (an enlarged axis)",
         _fixed(("src", "source", 3 * H * W), ("out", "result", 130 * 177 * 3)), ("src", "out"), _area(H, W, 3, 130, 177)),
    Case("resize_area_u8/2x2_rgb4", "pixel", "adain_resize_area_u8", N, "uint8 [n,256,352,3] -> [n,128,176,3] (16.5 GiB of frames)",
         _fixed(("src", "source", 12 * H * W), ("out", "result", 3 * H * W)), ("src", "out"), _area(2 * H, 2 * W, 3, H, W)),
    Case("resize_area_u8/tab_rgbw", "pixel", "adain_resize_area_u8", N, "uint8 [n,139,191,3] -> [n,128,176,3] (fractional scale, four taps)",
         _fixed(("src", "source", 139 * 191 * 3), ("out", "result", 3 * H * W)), ("src", "out"), _area(139, 191, 3, H, W)),
    Case("nchw_to_nhwc", "metrics", "adain_nchw_to_nhwc", N, "float32 [n,3,5633] -> [n,5633,3]",
         _fixed(("src", "source", 3 * 5633 * 4), ("out", "result", 3 * 5633 * 4)), ("src", "out"), _transpose(True, 3, 5633)),
    Case("nhwc_to_nchw", "metrics", "adain_nhwc_to_nchw", N, "float32 [n,5633,3] -> [n,3,5633]",
         _fixed(("src", "source", 3 * 5633 * 4), ("out", "result", 3 * 5633 * 4)), ("src", "out"), _transpose(False, 3, 5633)),
]



def _gray(hi, wi, ho, wo):
    def make():
        import farneback_ref as FB

        rgb = np.random.default_rng([17, hi, wi]).integers(0, 256, (P, hi, wi, 3), dtype=np.uint8)
        return (rgb,), (np.stack([FB.frame_to_gray(f, wo, ho) for f in rgb]),)
    return make


def _tvl1_frame_bytes(h, w):
    import applied_image_processing_amd.tvl1 as tvl1

    return tvl1.TVL1(h, w).frame_bytes


def _tvl1(h, w):
    def make():
        """Expected: the float64 restatement's (I, I_x, I_y) per scale; the device test holds the P frames alone to the bar of
        test_gpu_tvl1.py and the batch to those P device results, bit for bit."""
        import tvl1_ref as TV

        gray = np.stack([TV.texture(h, w, seed=5 + k) for k in range(P)])
        return (gray,), ([np.concatenate([c.ravel() for s in TV.prepare(g) for c in s]) for g in gray],)
    return make


PIXEL += [
    Case("flow_gray_u8", "pixel", "adain_flow_gray_u8", N, "uint8 [n,128,176,3] -> gray [n,257,259] (cv2's fixed-point linear resize)",
         _fixed(("rgb", "source", 3 * H * W), ("gray", "result", 257 * 259)), ("rgb", "gray"), _gray(H, W, 257, 259)),
    Case("tvl1_prepare", "pixel", "adain_tvl1_prepare", 5000, "gray uint8 [n,128,176] -> prepared float32 frames of 895 488 bytes",
         lambda n: [("gray", "source", n * H * W), ("prepared", "result", n * _tvl1_frame_bytes(H, W))], ("prepared",), _tvl1(H, W),
         below={"gray": "a prepared frame is 39.75 x its gray frame: a source past 2^32 bytes needs 171 GiB of prepared frames"}),
]


# ---- PIL resizes ------------------------------------------------------------------------------------------------------------------------------------
def _pil_ws(n, hi, wi, ho, wo, pix, code):
    import applied_image_processing_amd.runtime as rt

    return rt._size_query("adain_resize_pil_u8_bytes", n, hi, wi, ho, wo, pix, code, 0, 0, ho, wo)[0]


def _pil(hi, wi, ho, wo, pix, name):
    def make():
        from PIL import Image

        import pil_resize_ref as R

        rgb = np.stack([R.picture(300 + k, hi, wi) for k in range(P)])
        src = np.ascontiguousarray(rgb[..., 1:2]) if pix == 1 else rgb
        want = np.stack([np.asarray(Image.fromarray(f[..., 0] if pix == 1 else f).resize((wo, ho), R.FILTERS[name])) for f in src])
        if pix == 4:          # Pillow's own 4-byte storage of the same pictures
            src = np.stack([np.frombuffer(Image.fromarray(f).tobytes("raw", "RGBX"), np.uint8).reshape(hi, wi, 4) for f in rgb])
        return (src,), (want.reshape(P, ho, wo, -1),)
    return make


def _pil_case(id, call, hi, wi, ho, wo, pix, name, code, below=None):
    c = 1 if pix == 1 else 3
    bufs = lambda n: [("src", "source", n * hi * wi * pix), ("out", "result", n * ho * wo * c)] + (
        [("workspace", "workspace", _pil_ws(n, hi, wi, ho, wo, pix, code))] if call == "adain_resize_pil_u8" else [])
    past = ("src", "out") + (("workspace",) if call == "adain_resize_pil_u8" and not below else ())
    return Case(id, "resize", call, N, f"uint8 [n,{hi},{wi},{pix}] -> [n,{ho},{wo},{c}], {name}", bufs, past, _pil(hi, wi, ho, wo, pix, name), below=below)


RESIZE = [
    _pil_case("resize_pil_u8/bicubic_rgb", "adain_resize_pil_u8", H, W, 125, 181, 3, "BICUBIC", 3),
    _pil_case("resize_pil_u8/nearest_rgb", "adain_resize_pil_u8", H, W, 125, 181, 3, "NEAREST", 0,
              below={"workspace": "NEAREST runs no pass that needs the intermediate: the query answers 0 bytes"}),
    _pil_case("resize_pil_u8/lanczos_l", "adain_resize_pil_u8", 257, 259, 263, 261, 1, "LANCZOS", 1),
    _pil_case("resize_pil_u8/hamming_rgbx", "adain_resize_pil_u8", H, W, 125, 181, 4, "HAMMING", 5),
    _pil_case("resize_pil_bilinear_u8", "adain_resize_pil_bilinear_u8", H, W, 125, 181, 3, "BILINEAR", 2),
]


# ---- file encoders -----------------------------------------------------------------------------------------------------------------------------------
def _sizes(query, *dims):
    """(out_stride, workspace_bytes) of an encoder's host-only size query."""
    import applied_image_processing_amd.runtime as rt

    return rt._size_query(query, *dims, results=2)


def _query(query, *dims):
    """workspace_bytes of a host-only size query with one result."""
    import applied_image_processing_amd.runtime as rt

    return rt._size_query(query, *dims)[0]


def _jpeg_frames(h, w, c):
    import jpeg_ref as J

    kinds = ["noise", "smooth", "binary", "smooth", "noise", "binary", "smooth"]
    return [J.content(kind, h, w, c, seed=k) for k, kind in enumerate(kinds)]


def _jpeg(h, w, c, **save):
    def make():
        import io

        from PIL import Image

        frames = _jpeg_frames(h, w, c)
        files = []
        for a in frames:
            f = io.BytesIO()
            Image.fromarray(a).save(f, format="JPEG", quality=75, **save)
            files.append(f.getvalue())
        return (np.stack(frames).reshape(P, h, w, c),), (files,)
    return make


def _files_case(id, call, query, qdims, n, frames, src_bytes, make, below=None, past=("src", "rows", "workspace")):
    def bufs(n):
        stride, ws = _sizes(query, n, *qdims)
        return [("src", "source", n * src_bytes), ("rows", "rows", n * stride), ("workspace", "workspace", ws)]
    return Case(id, "encode", call, n, frames, bufs, past, make, below=below)


def _png(h, w, c):
    def make():
        import png_cases
        import png_ref

        frames = [png_cases.noisy_gradient(h, w, seed=1 + k) for k in range(P)]
        frames = [f if c == 3 else np.ascontiguousarray(f[..., :1]) for f in frames]
        return (np.stack(frames),), ([png_ref.encode(f if c == 3 else f[..., 0]) for f in frames],)
    return make


def _gif(K, h, w):
    def make():
        import gif_cases
        import gif_ref

        kinds = ["noise", "run", "noise", "flat", "noise", "run", "noise"]
        idx = np.stack([(gif_cases.indices(kind, K, h, w, seed=k).astype(np.int64) + (k if kind != "noise" else 0)) % K for k, kind in enumerate(kinds)]).astype(np.uint8)
        return (idx,), ([gif_ref.record(i, K, 5) for i in idx],)
    return make


def _roundtrip(h, w, c):
    def make():
        import io

        from PIL import Image

        frames = _jpeg_frames(h, w, c)
        out = []
        for a in frames:
            f = io.BytesIO()
            Image.fromarray(a).save(f, format="JPEG", quality=75)
            out.append(np.asarray(Image.open(io.BytesIO(f.getvalue()))).reshape(h, w, c))
        return (np.stack(frames).reshape(P, h, w, c),), (np.stack(out),)
    return make


_SMALL_SRC = "rows and workspace are 12 x the frames for this call: frames past 2^32 bytes need more than 50 GiB; adain_jpeg_encode_u8 takes its source past 2^32"
ENCODE = [
    _files_case("jpeg_encode_u8", "adain_jpeg_encode_u8", "adain_jpeg_encode_u8_bytes", (H, W, 3), N, "uint8 [n,128,176,3], quality 75, 4:2:0",
                3 * H * W, _jpeg(H, W, 3)),
    _files_case("jpeg_encode_opt_u8", "adain_jpeg_encode_opt_u8", "adain_jpeg_encode_opt_u8_bytes", (H, W, 3, 0, 1), 20000,
                "uint8 [20000,128,176,3], quality 75, 4:4:4, optimize", 3 * H * W, _jpeg(H, W, 3, subsampling=0, optimize=True),
                below={"src": _SMALL_SRC}, past=("rows", "workspace")),
    _files_case("jpeg_encode_progressive_u8", "adain_jpeg_encode_progressive_u8", "adain_jpeg_encode_progressive_u8_bytes", (H, W, 3, 2), 20000,
                "uint8 [20000,128,176,3], quality 75, 4:2:0, progressive", 3 * H * W, _jpeg(H, W, 3, progressive=True),
                below={"src": _SMALL_SRC}, past=("rows", "workspace")),
    _files_case("png_encode_u8", "adain_png_encode_u8", "adain_png_encode_u8_bytes", (H, W, 3), N, "uint8 [n,128,176,3], adaptive filters",
                3 * H * W, _png(H, W, 3)),
    _files_case("gif_encode_u8", "adain_gif_encode_u8", "adain_gif_encode_u8_bytes", (257, 257, 16), N, "index planes uint8 [n,257,257], K = 16",
                257 * 257, _gif(16, 257, 257)),
    Case("jpeg_roundtrip_u8", "encode", "adain_jpeg_roundtrip_u8", N, "uint8 [n,128,176,3] -> the pixels Pillow decodes from its own quality 75 file",
         lambda n: [("src", "source", n * 3 * H * W), ("dst", "result", n * 3 * H * W),
                    ("workspace", "workspace", _query("adain_jpeg_roundtrip_u8_bytes", n, H, W, 3))],
         ("src", "dst", "workspace"), _roundtrip(H, W, 3)),
]


# ---- file decoders -----------------------------------------------------------------------------------------------------------------------------------
LEAD = TWO32 + 12345          # spare bytes in front of the first segment: every offset is past 2^32 (and odd ones occur)
DECODERS = {"jpeg": ("adain_jpeg_decode_u8", {}, {}), "restart": ("adain_jpeg_decode_restart_u8", {"restart_marker_rows": 1}, {"restart": True}),
            "progressive": ("adain_jpeg_decode_progressive_u8", {"progressive": True}, {"progressive": True}), "png": ("adain_png_decode_u8", None, None)}


@functools.lru_cache(maxsize=None)
def decode_files(kind):
    """The P files of a decoder's row, parsed once: dict(parsed, datas, segments = per file the bytes of its entropy-coded segments
    (its scans, of a progressive file; its zlib stream, of a PNG) back to back, lengths = per file the length of each, blobs uint8
    [P, scans * BLOB_BYTES] (JPEG), expected = the restatement's pixels)."""
    import io

    from PIL import Image

    if kind == "png":
        import png_cases
        import png_decode_ref
        import png_ref

        import applied_image_processing_amd.png_file as png_file

        datas = [png_ref.encode(png_cases.noisy_gradient(H, W, seed=1 + k)) for k in range(P)]
        parsed = [png_file.parse(d) for d in datas]
        res = [png_decode_ref.decode(p.stream, H, W, 3) for p in parsed]
        assert all(r[1] == 0 for r in res)
        return dict(parsed=parsed, datas=datas, segments=[p.stream for p in parsed], lengths=[[len(p.stream)] for p in parsed], blobs=None,
                    expected=np.stack([r[0] for r in res]))
    import applied_image_processing_amd.jpeg_file as jpeg_file

    _call, save, parse = DECODERS[kind]
    ref = __import__({"jpeg": "jpeg_file_ref", "restart": "jpeg_restart_ref", "progressive": "jpeg_progressive_ref"}[kind])
    datas = []
    for a in _jpeg_frames(H, W, 3):
        f = io.BytesIO()
        Image.fromarray(a).save(f, format="JPEG", quality=75, **save)
        datas.append(f.getvalue())
    parsed = [jpeg_file.parse(d, **parse) for d in datas]
    streams = [p.scans if kind == "progressive" else [p] for p in parsed]
    res = [ref.decode(d) for d in datas]
    assert all(r[1] == 0 for r in res) and all(p.geometry == (H, W, 3, 2) for p in parsed)
    return dict(parsed=parsed, datas=datas, segments=[b"".join(d[s.seg_offset:s.seg_offset + s.seg_length] for s in ss) for ss, d in zip(streams, datas)],
                lengths=[[s.seg_length for s in ss] for ss in streams],
                blobs=np.stack([np.frombuffer(b"".join(s.blob for s in ss), np.uint8) for ss in streams]), expected=np.stack([r[0] for r in res]))


def decode_tables(kind, n, lead=LEAD):
    """(offsets uint64, lengths uint32, bytes of one group of P files, groups) of the batch's segments: file i is pattern i % P and
    lies in group i // P; a group is the P files' segments back to back, the groups follow one another behind ``lead`` bytes.  The
    JPEG tables hold a row per file and scan; the PNG table n + 1 offsets (stream i runs from offsets[i] to offsets[i + 1])."""
    lengths = np.array(decode_files(kind)["lengths"], dtype=np.uint64)          # [P, scans]
    per_file = lengths.sum(axis=1)
    group = int(per_file.sum())
    file_at = np.concatenate([[0], np.cumsum(per_file)[:-1]]).astype(np.uint64)
    scan_at = np.concatenate([np.zeros((P, 1), np.uint64), np.cumsum(lengths, axis=1)[:, :-1]], axis=1)
    i = np.arange(n, dtype=np.uint64)
    k = (i % P).astype(np.int64)
    off = (np.uint64(lead) + (i // np.uint64(P)) * np.uint64(group) + file_at[k])[:, None] + scan_at[k]
    ln = lengths[k]
    if kind == "png":
        off = np.concatenate([off[:, 0], off[-1:, 0] + ln[-1:, 0]])
    return np.ascontiguousarray(off.reshape(-1)), np.ascontiguousarray(ln.reshape(-1).astype(np.uint32)), group, (n + P - 1) // P


def _decode_ws(kind, n):
    import applied_image_processing_amd.runtime as rt

    d = decode_files(kind)
    longest = max(max(row) for row in d["lengths"])
    if kind == "png":
        return rt.png_decode_sizes(n, H, W, 3, longest)
    if kind == "progressive":
        return rt.jpeg_decode_progressive_sizes(n, H, W, 3, 2, len(d["parsed"][0].script), longest)
    return rt.jpeg_decode_sizes(n, H, W, 3, 2, longest, 0, d["parsed"][0].restart_interval)


def _decode_case(kind, frames):
    def bufs(n):
        d = decode_files(kind)
        _off, _ln, group, groups = decode_tables(kind, n)
        blobs = [] if kind == "png" else [("blobs", "source", n * d["blobs"].shape[1])]
        return [("files", "streams", LEAD + groups * group + 1)] + blobs + [("dst", "result", n * 3 * H * W), ("record", "result", n * 8),
                                                                             ("workspace", "workspace", _decode_ws(kind, n))]

    def make():
        d = decode_files(kind)
        return (d["segments"],) + (() if kind == "png" else (d["blobs"],)), (d["expected"],)
    below = {"record": "8 bytes per file"}
    if kind != "png":
        below["blobs"] = "the tables of a file: 3848 bytes a scan, 2.4 GiB at ten scans; read through one pointer and a 64-bit stride as the files are"
    return Case(f"{kind}_decode" if kind == "png" else f"jpeg_decode/{kind}", "decode", DECODERS[kind][0], N, frames, bufs, ("files", "dst", "workspace"), make,
                below=below)


DECODE = [
    _decode_case("jpeg", "65535 baseline files of 128 x 176 x 3, 4:2:0, behind a lead of 2^32 + 12345 bytes -> uint8 [n,128,176,3]"),
    _decode_case("restart", "the same with a restart interval of one MCU row (11 MCUs)"),
    _decode_case("progressive", "the same as progressive files of ten scans: 655 350 segments"),
    _decode_case("png", "65535 PNG files of 128 x 176 x 3, adaptive filters, behind the same lead"),
]


# ---- palette control and the palette chooser ---------------------------------------------------------------------------------------------------------
PALETTE_K = 16


def _palette_frames(h, w):
    import quantize_cases as C

    return C.gradient(P, h, w, seed=31)


def _palette_of(frames):
    import quantize_ref as Q

    pal, used = Q.palette(frames[0], PALETTE_K)
    assert used == PALETTE_K
    return np.ascontiguousarray(pal[:PALETTE_K])


def _map(h, w, metric):
    def make():
        import palette_ref as R

        frames = _palette_frames(h, w)
        pal = _palette_of(frames)
        idx = R.map_index(frames, pal, metric).astype(np.uint8)
        return (frames, np.broadcast_to(pal, (P,) + pal.shape)), (pal[idx], idx)
    return make


def _tone(h, w):
    def make():
        import palette_ref as R

        frames = _palette_frames(h, w)
        lut = R.tone_lut(0.1, 0.2)
        return (frames, np.broadcast_to(lut, (P, 3, 256))), (R.tone(frames, lut, grey_first=True),)
    return make


def _dither(h, w):
    def make():
        import palette_ref as R

        frames = _palette_frames(h, w)
        pal = _palette_of(frames)
        out, idx = R.dither(frames, pal)
        return (frames, np.broadcast_to(pal, (P,) + pal.shape)), (out, idx)
    return make


def _quantize_per_frame(h, w, repeat=1):
    def make():
        """``repeat``: the device frame is the pattern ``repeat`` times one below the other - the palette of the pattern counted
        ``repeat`` times, which is the pattern's own (every moment is multiplied by the same whole number... but the rounding of an
        entry is not: the weighted restatement is asked)."""
        import quantize_ref as Q

        frames = _palette_frames(h, w)
        res = [Q.palette_weighted([f], [repeat], PALETTE_K) for f in frames]
        return (frames,), (np.stack([p for p, _ in res]), np.asarray([u for _, u in res], dtype=np.int32))
    return make


def _quantize_global(h, w, n):
    def make():
        """One palette over n frames, frame i = pattern i % P: the patterns with their multiplicities."""
        import quantize_ref as Q

        frames = _palette_frames(h, w)
        weights = [n // P + (1 if k < n % P else 0) for k in range(P)]
        pal, used = Q.palette_weighted(frames, weights, 256)
        plain, _ = Q.palette(frames, 256)
        assert not np.array_equal(pal, plain) or n % P == 0, "the multiplicities are meant to matter"
        assert distinct(frames)          # the palette is one value, not P: what differs from pattern to pattern is its input
        return (frames,), (np.broadcast_to(pal, (P, 256, 3)), np.full((P, 1), used, dtype=np.int32))
    return make


_USED = {1: "the count of entries used: all 16 for every pattern; the palettes (expected 0) tell the patterns apart"}
TALL = 977          # pattern repeats per frame of quantize_palette_u8/per_frame_source: 977 x 128 rows of 176 pixels, 66.0 MB
PALETTE = [
    Case("palette_map_u8", "palette", "adain_palette_map_u8", N, "uint8 [n,128,176,3], K = 16, metric nearest, with the index plane",
         _fixed(("src", "source", 3 * H * W), ("out", "result", 3 * H * W), ("index", "result", H * W)), ("src", "out"), _map(H, W, "nearest"),
         below={"index": "a third of the frames; past 2^32 in palette_map_u8/index"}),
    Case("palette_map_u8/index", "palette", "adain_palette_map_u8", N, "uint8 [n,257,259,3], K = 16, metric rgb: the index plane alone is 4.06 GiB",
         _fixed(("src", "source", 3 * 257 * 259), ("out", "result", 3 * 257 * 259), ("index", "result", 257 * 259)), ("src", "out", "index"),
         _map(257, 259, "rgb")),
    Case("tone_u8", "palette", "adain_tone_u8", N, "uint8 [n,128,176,3], grey then a lut",
         _fixed(("src", "source", 3 * H * W), ("out", "result", 3 * H * W)), ("src", "out"), _tone(H, W)),
    Case("palette_dither_u8", "palette", "adain_palette_dither_u8", N, "uint8 [n,128,176,3], K = 16, with the index plane",
         lambda n: [("src", "source", n * 3 * H * W), ("out", "result", n * 3 * H * W), ("index", "result", n * H * W),
                    ("workspace", "workspace", _query("adain_palette_dither_u8_bytes", n, H, W))], ("src", "out"), _dither(H, W),
         below={"index": "a third of the frames: past 2^32 in palette_dither_u8/index",
                "workspace": "one error row of 12 w bytes per frame: past 2^32 in palette_dither_u8/wide"}),
    Case("palette_dither_u8/index", "palette", "adain_palette_dither_u8", N, "uint8 [n,257,259,3], K = 16: the index plane alone is 4.06 GiB (28.7 GiB in all)",
         lambda n: [("src", "source", n * 3 * 257 * 259), ("out", "result", n * 3 * 257 * 259), ("index", "result", n * 257 * 259),
                    ("workspace", "workspace", _query("adain_palette_dither_u8_bytes", n, 257, 259))], ("src", "out", "index"), _dither(257, 259),
         below={"workspace": "one error row of 12 w bytes per frame: past 2^32 in palette_dither_u8/wide"}),
    Case("palette_dither_u8/wide", "palette", "adain_palette_dither_u8", N, "uint8 [n,4,5463,3]: the workspace's error rows, 12 x 5463 bytes a frame, pass 2^32",
         lambda n: [("src", "source", n * 12 * 5463), ("out", "result", n * 12 * 5463), ("index", "result", n * 4 * 5463),
                    ("workspace", "workspace", _query("adain_palette_dither_u8_bytes", n, 4, 5463))], ("src", "out", "workspace"), _dither(4, 5463),
         below={"index": "a third of the frames: past 2^32 in palette_dither_u8/index"}),
    Case("quantize_palette_u8/per_frame", "palette", "adain_quantize_palette_u8", 4096, "uint8 [4096,128,176,3], a palette per frame: 1.1 MB of cells per frame",
         lambda n: [("src", "source", n * 3 * H * W), ("palettes", "result", n * 768), ("used", "result", n * 4),
                    ("workspace", "workspace", _query("adain_quantize_palette_u8_bytes", n, H, W, 1))], ("workspace",), _quantize_per_frame(H, W),
         below={"src": "past 2^32 in quantize_palette_u8/per_frame_source", "palettes": "768 bytes per frame: 48 MiB at n = 65535",
                "used": "4 bytes per frame"}, same=_USED),
    Case("quantize_palette_u8/per_frame_source", "palette", "adain_quantize_palette_u8", 70,
         "uint8 [70,125056,176,3]: 66 MB frames, each its pattern 977 times one below the other",
         lambda n: [("src", "source", n * TALL * 3 * H * W), ("palettes", "result", n * 768), ("used", "result", n * 4),
                    ("workspace", "workspace", _query("adain_quantize_palette_u8_bytes", n, TALL * H, W, 1))], ("src",),
         _quantize_per_frame(H, W, TALL),
         below={"workspace": "past 2^32 in quantize_palette_u8/per_frame", "palettes": "768 bytes per frame", "used": "4 bytes per frame"}, same=_USED),
    Case("quantize_palette_u8/global", "palette", "adain_quantize_palette_u8", N, "uint8 [n,128,176,3], one palette over 1.48 G pixels: 4.12 GiB inside one palette",
         lambda n: [("src", "source", n * 3 * H * W), ("workspace", "workspace", _query("adain_quantize_palette_u8_bytes", n, H, W, 0))], ("src",),
         _quantize_global(H, W, N), below={"workspace": "one palette's cells, whatever n"},
         same={0: "one palette for the whole clip, the same row P times", 1: "its count of entries, likewise"}),
]


# ---- metrics, CORAL, statistics, blends, transposes, single conv layers --------------------------------------------------------------------------------
def _metrics_u8(h, w, c):
    def make():
        import metrics_cases as C
        import metrics_ref as R

        a, b = C.pair("near", P, h, w, c, seed=6)
        want = R.metrics_u8(a, b)
        return (a, b), (np.stack([want[k] for k in ("ssim", "mse", "l1", "psnr")], axis=1), want["map"])
    return make


def _metrics_f32(h, w, c):
    def make():
        import metrics_cases as C
        import metrics_ref as R

        a, b = (C.to_nchw_f32(x) for x in C.pair("near", P, h, w, c, seed=7))
        want = R.metrics_f32(a, b)
        return (a, b), (np.stack([want[k] for k in ("ssim", "mse", "l1", "psnr")], axis=1), want["map"])
    return make


def _coral(hs, ws, hc, wc, form):
    def make():
        import coral_ref as R

        style = np.stack([R.u8_image(1000 + k, hs, ws) for k in range(P)])
        content = np.stack([R.u8_image(2000 + k, hc, wc) for k in range(P)])
        if form == "f32":
            style, content = np.stack([R.chw(x) for x in style]), np.stack([R.chw(x) for x in content])
        res = [R.coral(s, c) for s, c in zip(style, content)]
        assert all(r[3] == 0 for r in res)
        return (style, content), (np.stack([r[0] for r in res]), np.stack([r[1] for r in res]), np.stack([r[2] for r in res]))
    return make


def _coral_ws(n, hs, ws, hc, wc):
    import applied_image_processing_amd.runtime as rt

    return rt.lib().adain_coral_workspace_bytes(n, n, hs, ws, hc, wc)


STATS_C, STATS_HW = 3, 5633


def _stats_input():
    """float32 [P,3,1,5633] NCHW, test_gpu_blend_stats.stats_input's recipe with a level per pattern."""
    rng = np.random.default_rng([STATS_C, STATS_HW, 0])
    offset = (5.0 * np.arange(P)[:, None] + np.arange(STATS_C)[None, :] % 11 - 3.0).astype(F32)
    scale = (0.5 + 0.25 * (np.arange(STATS_C) % 7)).astype(F32)
    det = (1.0 - 2.0 * (np.arange(STATS_HW) % 2)).astype(F32)
    x = rng.standard_normal((P, STATS_C, 1, STATS_HW), dtype=F32)
    x *= F32(0.25)
    x += det[None, None, None, :]
    x *= scale[None, :, None, None]
    x += offset[:, :, None, None]
    return x


def _mean_std():
    def make():
        import blend_ref as R

        x = _stats_input()
        ref = R.mean_std_f64(x, False, float(F32(1e-5)))
        return (x,), (ref["mean64"], ref["std64"])
    return make


def _blend(kind):
    def make():
        """test_gpu_blend_stats.blend_inputs' recipe: statistics per image and channel, a strength map per image."""
        import blend_ref as R

        rng = np.random.default_rng([5, P, STATS_C, STATS_HW])
        x = rng.standard_normal((P, STATS_C, 1, STATS_HW), dtype=F32)
        level = 10.0 * np.arange(P)[:, None] + 16.0 * np.arange(STATS_C)[None, :] / 16
        cm, cs = (level + 0.25 * rng.random((P, STATS_C))).astype(F32), (0.5 + 1.5 * rng.random((P, STATS_C))).astype(F32)
        sm, ss = (-(level + 0.25 * rng.random((P, STATS_C)))).astype(F32), (0.5 + 1.5 * rng.random((P, STATS_C))).astype(F32)
        p = (0.05 + 0.1 * np.arange(P)[:, None] + 0.2 * rng.random((P, STATS_HW))).astype(F32)
        kw = dict(alpha=0.7) if kind == "alpha" else dict(pmap=p)
        want = R.blend(x, False, cm, cs, sm, ss, **kw)
        want64, parts = R.blend(x, False, cm, cs, sm, ss, dtype=np.float64, parts=True, **kw)
        assert (np.abs(want.astype(np.float64) - want64).reshape(-1) <= R.self_distance_bound(parts)).all(), "the inputs cancel"
        return (x, cm, cs, sm, ss) + ((p,) if kind == "pmap" else ()), (want,)
    return make


NHWC_C, NHWC_HW = 4, 4225          # the NHWC rows: 4 channels (one quad per pixel), frames of 67 600 bytes
C1_HW = 3 * STATS_HW               # blend_pmap/c1: one channel, so that the strength map is as large as the features
MIX_K = 4


def _shaped(a, nhwc):
    """[P,c,hw] -> the call's layout, NHWC [P,1,hw,c] or NCHW [P,c,1,hw]."""
    return np.ascontiguousarray(a.transpose(0, 2, 1)[:, None]) if nhwc else np.ascontiguousarray(a[:, :, None, :])


def _mean_std_nhwc():
    def make():
        """_stats_input's recipe at [P,4,4225], handed over as NHWC."""
        import blend_ref as R

        c, hw = NHWC_C, NHWC_HW
        rng = np.random.default_rng([c, hw, 1])
        offset = (5.0 * np.arange(P)[:, None] + np.arange(c)[None, :] - 3.0).astype(F32)
        scale = (0.5 + 0.25 * np.arange(c)).astype(F32)
        det = (1.0 - 2.0 * (np.arange(hw) % 2)).astype(F32)
        x = (rng.standard_normal((P, c, hw), dtype=F32) * F32(0.25) + det[None, None, :]) * scale[None, :, None] + offset[:, :, None]
        x = _shaped(x.astype(F32), True)
        ref = R.mean_std_f64(x, True, float(F32(1e-5)))
        return (x,), (ref["mean64"], ref["std64"])
    return make


def _blend_at(kind, nhwc, c, hw):
    def make():
        """_blend's recipe at any layout; kind "mix": MIX_K styles for the whole batch, a weight map per frame and style
        (test_gpu_blend_mix.mix_inputs' ranges), held to tests/mix_ref.py as test_gpu_blend_mix.py holds the call."""
        import blend_ref as R
        import mix_ref as M

        rng = np.random.default_rng([6, P, c, hw, int(nhwc)])
        x = _shaped(rng.standard_normal((P, c, hw), dtype=F32), nhwc)
        level = 10.0 * np.arange(P)[:, None] + 16.0 * np.arange(c)[None, :] / 16
        cm, cs = (level + 0.25 * rng.random((P, c))).astype(F32), (0.5 + 1.5 * rng.random((P, c))).astype(F32)
        p = (0.05 + 0.1 * np.arange(P)[:, None] + 0.2 * rng.random((P, hw))).astype(F32)
        if kind.startswith("mix"):
            chan = 16.0 * np.arange(c)[None, :] / 16
            sm = (-(7.0 * np.arange(MIX_K)[:, None] + chan + 0.25 * rng.random((MIX_K, c)))).astype(F32)
            ss = (0.5 + 1.5 * rng.random((MIX_K, c))).astype(F32)
            w = (0.05 + 0.85 * rng.random((P, MIX_K, hw))).astype(F32)
            kw = dict(pmap=p) if kind == "mix_pmap" else dict(alpha=0.6)
            want = M.mix(x, nhwc, cm, cs, sm, ss, w, **kw)
            want64, parts = M.mix(x, nhwc, cm, cs, sm, ss, w, dtype=np.float64, parts=True, **kw)
            assert (np.abs(want.astype(np.float64) - want64).reshape(-1) <= M.self_distance_bound(parts)).all(), "the inputs cancel"
            rows = lambda t: np.broadcast_to(t, (P,) + t.shape)
            return (x, cm, cs, w) + ((p,) if kind == "mix_pmap" else ()) + (rows(sm), rows(ss)), (want,)
        sm, ss = (-(level + 0.25 * rng.random((P, c)))).astype(F32), (0.5 + 1.5 * rng.random((P, c))).astype(F32)
        kw = dict(alpha=0.7) if kind == "alpha" else dict(pmap=p)
        want = R.blend(x, nhwc, cm, cs, sm, ss, **kw)
        want64, parts = R.blend(x, nhwc, cm, cs, sm, ss, dtype=np.float64, parts=True, **kw)
        assert (np.abs(want.astype(np.float64) - want64).reshape(-1) <= R.self_distance_bound(parts)).all(), "the inputs cancel"
        return (x, cm, cs, sm, ss) + ((p,) if kind == "pmap" else ()), (want,)
    return make


def _mean_std_ws(n, c, hw):
    import applied_image_processing_amd.runtime as rt

    return rt.lib().adain_mean_std_workspace_bytes(1, n, c, hw)


CONV_N, CONV_H, CONV_W, CONV_C = 27000, 29, 45, 32


def conv_exact_case(entry):
    """The far-batch layer as a tests/conv_exact.py Case of the P patterns (its head-room is checked on the host)."""
    import conv_exact as X

    return X.Case(f"far-{entry}", "far", entry, entry == "poly", P, CONV_C, CONV_C, CONV_H, CONV_W, 3, 2, 4242, None)


def _conv(entry):
    def make():
        import conv_exact as X

        x, w, b = X.case_layer(conv_exact_case(entry))
        want = X.reference(x, w, b, up=entry == "poly", relu=True)
        rows = lambda t: np.broadcast_to(t.numpy(), (P,) + tuple(t.shape))
        return (x.numpy(), rows(w), rows(b)), (want.numpy(),)
    return make


_CONV_F = CONV_H * CONV_W * CONV_C * 4
_RECORDS = "32 bytes per frame: 2 MiB at n = 65535"
_METRICS_WS = "a few partial records per tile, 2.5 % of a frame: past 2^32 only with 160 GiB of frames"
METRICS = [
    Case("image_metrics_u8", "metrics", "adain_image_metrics_u8", N, "uint8 [n,128,176,3] pairs, with the SSIM map (16.5 GiB)",
         lambda n: [("a", "source", n * 3 * H * W), ("b", "source", n * 3 * H * W), ("out", "result", n * 32), ("ssim_map", "result", n * 12 * H * W),
                    ("workspace", "workspace", _query("adain_image_metrics_u8_bytes", n, H, W, 3))], ("a", "b", "ssim_map"), _metrics_u8(H, W, 3),
         below={"out": _RECORDS, "workspace": _METRICS_WS}),
    Case("image_metrics_f32", "metrics", "adain_image_metrics_f32", N, "float32 [n,1,129,131] pairs, with the SSIM map",
         lambda n: [("a", "source", n * 4 * 129 * 131), ("b", "source", n * 4 * 129 * 131), ("out", "result", n * 32), ("ssim_map", "result", n * 4 * 129 * 131),
                    ("workspace", "workspace", _query("adain_image_metrics_f32_bytes", n, 1, 129, 131))], ("a", "b", "ssim_map"), _metrics_f32(129, 131, 1),
         below={"out": _RECORDS, "workspace": _METRICS_WS}),
    Case("coral/u8", "metrics", "adain_coral", N, "uint8 styles and contents [n,128,176,3], a style per content -> float32 [n,3,128,176]",
         lambda n: [("style", "source", n * 3 * H * W), ("content", "source", n * 3 * H * W), ("out", "result", n * 12 * H * W),
                    ("workspace", "workspace", _coral_ws(n, H, W, H, W))],
         ("style", "content", "out"), _coral(H, W, H, W, "u8"), below={"workspace": "a record and a few partial sums per pair: 75 MiB at n = 65535"}),
    Case("coral/f32", "metrics", "adain_coral", N, "float32 styles [n,3,75,73] and contents [n,3,73,75]",
         lambda n: [("style", "source", n * 12 * 75 * 73), ("content", "source", n * 12 * 75 * 73), ("out", "result", n * 12 * 75 * 73),
                    ("workspace", "workspace", _coral_ws(n, 75, 73, 73, 75))],
         ("style", "content", "out"), _coral(75, 73, 73, 75, "f32"), below={"workspace": "a record and a few partial sums per pair"}),
    Case("mean_std", "metrics", "adain_mean_std", 65532, "float32 NCHW [65532,3,1,5633] -> mean, std [n,3]",
         lambda n: [("feat", "source", n * 12 * STATS_HW), ("mean", "result", n * 12), ("std", "result", n * 12)], ("feat",), _mean_std(),
         below={"mean": "12 bytes per image; the call takes fewer than 2^31 elements", "std": "12 bytes per image"}),
    Case("blend_alpha", "metrics", "adain_blend_alpha", 65532, "float32 NCHW [65532,3,1,5633], statistics and style per image (1.1 G elements: the call's limit is 2^31 - 1)",
         lambda n: [("x", "source", n * 12 * STATS_HW), ("out", "result", n * 12 * STATS_HW), ("stats", "source", n * 48)], ("x", "out"), _blend("alpha"),
         below={"stats": "four rows of 12 bytes per image"}),
    Case("blend_pmap", "metrics", "adain_blend_pmap", 65532, "float32 NCHW [65532,3,1,5633], a strength map per image",
         lambda n: [("x", "source", n * 12 * STATS_HW), ("out", "result", n * 12 * STATS_HW), ("stats", "source", n * 48), ("pmap", "source", n * 4 * STATS_HW)],
         ("x", "out"), _blend("pmap"),
         below={"stats": "four rows of 12 bytes per image", "pmap": "a third of the features at c = 3: past 2^32 in blend_pmap/c1"}),
    Case("blend_pmap/c1", "metrics", "adain_blend_pmap", 65532, "float32 NCHW [65532,1,1,16899]: one channel, the strength maps are as large as the features",
         lambda n: [("x", "source", n * 4 * C1_HW), ("out", "result", n * 4 * C1_HW), ("stats", "source", n * 16), ("pmap", "source", n * 4 * C1_HW)],
         ("x", "out", "pmap"), _blend_at("pmap", False, 1, C1_HW), below={"stats": "four rows of 4 bytes per image"}),
    Case("blend_alpha/nhwc", "metrics", "adain_blend_alpha", N, "float32 NHWC [n,1,4225,4], statistics and style per image (adain_blend_kernel<NHWC>)",
         lambda n: [("x", "source", n * 16 * NHWC_HW), ("out", "result", n * 16 * NHWC_HW), ("stats", "source", n * 64)], ("x", "out"),
         _blend_at("alpha", True, NHWC_C, NHWC_HW), below={"stats": "four rows of 16 bytes per image"}),
    Case("blend_mix/maps", "metrics", "adain_blend_mix", 65532, "float32 NCHW [65532,3,1,5633], 4 styles, a weight map per image and style: 5.5 GiB of weights",
         lambda n: [("x", "source", n * 12 * STATS_HW), ("out", "result", n * 12 * STATS_HW), ("stats", "source", n * 24),
                    ("weights", "source", n * MIX_K * 4 * STATS_HW)],
         ("x", "out", "weights"), _blend_at("mix", False, STATS_C, STATS_HW), below={"stats": "two rows of 12 bytes per image (the styles are the batch's)"}),
    Case("blend_mix/nhwc_maps", "metrics", "adain_blend_mix", N, "float32 NHWC [n,1,4225,4], 4 styles, weight maps and a strength map per image (adain_mix_walk_kernel)",
         lambda n: [("x", "source", n * 16 * NHWC_HW), ("out", "result", n * 16 * NHWC_HW), ("stats", "source", n * 32),
                    ("weights", "source", n * MIX_K * 4 * NHWC_HW), ("pmap", "source", n * 4 * NHWC_HW)],
         ("x", "out", "weights"), _blend_at("mix_pmap", True, NHWC_C, NHWC_HW),
         below={"stats": "two rows of 16 bytes per image", "pmap": "a quarter of the features at c = 4: past 2^32 in blend_pmap/c1"}),
    Case("mean_std/nhwc", "metrics", "adain_mean_std", N, "float32 NHWC [n,1,4225,4] -> mean, std [n,4] (the partial sums and their finalize)",
         lambda n: [("feat", "source", n * 16 * NHWC_HW), ("mean", "result", n * 16), ("std", "result", n * 16),
                    ("workspace", "workspace", _mean_std_ws(n, NHWC_C, NHWC_HW))], ("feat",), _mean_std_nhwc(),
         below={"mean": "16 bytes per image", "std": "16 bytes per image",
                "workspace": "at most 256 partial sums of 16 c bytes per image, as many as 16 c pixel rows: past 2^32 only with features past 2^32 elements"}),
    Case("conv3x3_wino", "metrics", "adain_conv3x3_wino", CONV_N, "float32 NHWC [27000,29,45,32] -> 32 channels, direct, ReLU, integer-exact operands",
         _fixed(("x", "source", _CONV_F), ("out", "result", _CONV_F)), ("x", "out"), _conv("wino")),
    Case("conv3x3_up2x_poly", "metrics", "adain_conv3x3_up2x_poly", CONV_N, "float32 NHWC [27000,29,45,32] -> [27000,58,90,32], the polyphase up layer",
         _fixed(("x", "source", _CONV_F), ("out", "result", 4 * _CONV_F)), ("x", "out"), _conv("poly")),
]

# ---- the 3DGS training loss: the metrics' gradient and the guide-view loss ----------------------------------------------------------------------------
GRAD_C, GRAD_H, GRAD_W = 3, 43, 131          # three planes (the plane term of plane_at is live), 3 x 3 tiles, one-sample slivers each way
# (how the pattern's gradient is held to the restatement, its upstream {ssim, mse, l1}): the first row of each of
# metrics_grad_cases.WEIGHTS; a row of zeros, whose frames receive zeros though nothing of them is read; a zero ssim weight beside mse
# and l1 weights of one sign (the planes pass returns early, the combine pass skips its staging); one more mixed row
GRAD_ROWS = (("ssim", (1.0, 0.0, 0.0)), ("mse", (0.0, 1.0, 0.0)), ("l1", (0.0, 0.0, 1.0)), ("mixed", (-0.2, 0.7, 0.8)), ("zero", (0.0, 0.0, 0.0)),
             ("no_ssim", (0.0, 0.7, 0.8)), ("mixed", (-1.5, -0.3, 0.4)))
GUIDE_GH, GUIDE_GW = H, W                    # the guides are the table's default frame
GUIDE_L1_HW = (73, 104)                      # w % 4 == 0: guide_l1_tile_kernel<true>
GUIDE_GRAD_HW = (75, 101)                    # w % 4 != 0: guide_l1_grad_kernel<false>
GUIDE_WEIGHTS = (1.0, -0.25, 0.75, 0.0, -2.0, 0.5, 3.0)          # pattern 3: +0 everywhere, neither its image nor its guide is read
assert len(GRAD_ROWS) == P and len(GUIDE_WEIGHTS) == P


def _metrics_grad(h, w, c):
    def make():
        """Expected: the float64 restatement's grad_a; the device test holds the P frames alone to it (bar_grad, or per element for
        the rows without an ssim weight) and the batch to those P device results, bit for bit."""
        import metrics_cases as C
        import metrics_grad_ref as G

        a, b = (C.to_nchw_f32(x) for x in C.pair("near", P, h, w, c, seed=8))
        weights = np.array([row for _kind, row in GRAD_ROWS], dtype=np.float64)
        return (a, b, weights), (G.grad(a, b, weights)[0],)
    return make


def guide_shape(hw):
    """The guide_loss_cases shape of the P patterns of a guide case."""
    return (P,) + tuple(hw) + (GUIDE_GH, GUIDE_GW)


def _guide_l1(hw):
    def make():
        """guide_loss_cases' own guides and renders (g +- delta, no sample near a tie) -> the restatement's loss and resampled guide."""
        import guide_loss_cases as K
        import guide_loss_ref as R

        shape = guide_shape(hw)
        image, guide = K.image_delta(shape), K.guide(shape)
        return (image, guide), (R.loss(image, guide), K.g_ref(shape))
    return make


def _guide_l1_grad(hw):
    def make():
        import guide_loss_cases as K
        import guide_loss_ref as R

        shape = guide_shape(hw)
        image, guide, weights = K.image_delta(shape), K.guide(shape), np.array(GUIDE_WEIGHTS, dtype=np.float64)
        return (image, guide, weights), (R.grad(image, guide, weights),)
    return make


_GRAD_F = GRAD_C * GRAD_H * GRAD_W * 4
_GUIDE_F = 3 * GUIDE_GH * GUIDE_GW
METRICS += [
    Case("image_metrics_grad_f32", "metrics", "adain_image_metrics_grad_f32", N,
         "float32 [n,3,43,131] pairs, weights float64 [n,3] of seven kinds, grad_a only (24.8 GiB; with grad_b: 37 GiB, past the cap)",
         lambda n: [("a", "source", n * _GRAD_F), ("b", "source", n * _GRAD_F), ("weights", "source", n * 24), ("grad_a", "result", n * _GRAD_F),
                    ("workspace", "workspace", _query("adain_image_metrics_grad_f32_bytes", n, GRAD_C, GRAD_H, GRAD_W, 0))],
         ("a", "b", "grad_a", "workspace"), _metrics_grad(GRAD_H, GRAD_W, GRAD_C), below={"weights": "24 bytes per frame: 1.5 MB at n = 65535"}),
    Case("guide_l1_f32", "metrics", "adain_guide_l1_f32", N, "float32 renders [n,3,73,104] (w % 4 == 0) against uint8 guides [n,128,176,3], with the resampled guide",
         lambda n: [("image", "source", n * 12 * 73 * 104), ("guide", "source", n * _GUIDE_F), ("out", "result", n * 8), ("resampled", "result", n * 12 * 73 * 104),
                    ("workspace", "workspace", _query("adain_guide_l1_f32_bytes", n, *GUIDE_L1_HW))],
         ("image", "guide", "resampled"), _guide_l1(GUIDE_L1_HW),
         below={"out": "8 bytes per frame", "workspace": "a float64 per 1024 pixels of a render, about 1/1500 of it: past 2^32 only with 6 TiB of renders"}),
    Case("guide_l1_grad_f32", "metrics", "adain_guide_l1_grad_f32", N,
         "float32 renders [n,3,75,101] (w % 4 != 0) against uint8 guides [n,128,176,3], weights float64 [n] of seven values, one of them 0",
         lambda n: [("image", "source", n * 12 * 75 * 101), ("guide", "source", n * _GUIDE_F), ("weights", "source", n * 8), ("grad", "result", n * 12 * 75 * 101)],
         ("image", "guide", "grad"), _guide_l1_grad(GUIDE_GRAD_HW), below={"weights": "8 bytes per frame"}),
]

# ---- the encoder's first layer alone ---------------------------------------------------------------------------------------------------------------------
FIRST_H, FIRST_W = 9, 33          # tests/edge_exact.py's batch frame: 2 x 2 tiles of 8 x 32 with a seam, a partial row and a one-pixel column


def first_layer_case():
    """The far-batch first layer as a tests/edge_exact.py FirstCase of the P patterns (its head-room is checked on the host)."""
    import edge_exact as E

    return E.FirstCase("far-first", "batch", P, FIRST_H, FIRST_W, 4100)


def _first_layer():
    def make():
        """Integer-valued images under edge_exact's integer weights: the float64 evaluation of the unfolded layer is what the kernel
        gives, element for element."""
        import edge_exact as E

        x = E.first_image(first_layer_case())
        return (x.numpy(),), (E.to_float32_exact(E.first_reference(x)).numpy(),)
    return make


METRICS += [
    Case("encode_relu1_1", "metrics", "adain_encode_relu1_1", N, "float32 images [n,3,9,33] -> relu1_1 NHWC [n,9,33,64] (4.64 GiB), integer-exact operands",
         _fixed(("image", "source", 12 * FIRST_H * FIRST_W), ("relu1_1", "result", 256 * FIRST_H * FIRST_W)), ("relu1_1",), _first_layer(),
         below={"image": "12 bytes a pixel for 256 of relu1_1: images past 2^32 bytes need 91 GiB of output"}),
]
METRICS += [c for c in PIXEL if c.family == "metrics"]
PIXEL = [c for c in PIXEL if c.family == "pixel"]

CASES = PIXEL + RESIZE + ENCODE + DECODE + PALETTE + METRICS
BY_ID = {c.id: c for c in CASES}
assert len(BY_ID) == len(CASES)


# ---- the launches without a row, and why ---------------------------------------------------------------------------------------------------------------
_NETWORK = "a whole network per call: its ping-pong workspace is 28 x the float frames (335 MB per 1024 x 1024 image), more than 100 GiB before the frames pass 2^32"
_NO_N = "one frame per call: no n, so no frame index"
_PACK = "packs one set of weights: no n, no frame index"
OUT_OF_SCOPE = {
    "adain_encoder_pack": _PACK, "adain_decoder_pack": _PACK, "adain_conv3x3_wino4_pack": _PACK, "adain_conv3x3_up2x_poly_pack": _PACK,
    "adain_encode": _NETWORK, "adain_encode_u8": _NETWORK, "adain_encode_multi": _NETWORK, "adain_decode": _NETWORK,
    "adain_stylize_u8": _NETWORK, "adain_stylize_u8_ex": _NETWORK, "adain_stylize_u8_mix": _NETWORK,
    "adain_tvl1_flow": "takes its frames by pointer, one pair at a time: no frame index into a caller's batch (its per-pair workspace slots are not "
                       "taken past 2^32 here)",
    "adain_farneback_expand": "one frame's pyramid per call: no n, so no frame index",
    "adain_farneback_flow": "one pair of pyramids per call: no n, so no frame index",
    "adain_colour_transfer_u8": _NO_N, "adain_strength_map": _NO_N, "adain_localized_combine_u8": _NO_N, "adain_warp_blend_u8": _NO_N,
    "adain_conv3x3_wino4_split": "splits along cin only while tiles x channel tiles x 2 <= the device's compute units (wino4_ksplit): at most 128 tiles of "
                                 "256 pixels on 256 units, an output of 4 MiB, and a source past 2^32 bytes only from 32768 input channels on; a larger "
                                 "launch leaves no unit idle, is not split and is adain_conv3x3_wino's launch, which has a row",
}


def cases_of(family):
    return [c for c in CASES if c.family == family]
