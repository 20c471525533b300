"""NumPy restatement of the reference's per-channel statistics and AdaIN feature blend (Style_3DGS/AdaIN/function.py:4-23,
test.py:69-70 and :79-80): the yardstick of csrc/stats.hip (``adain_mean_std``, ``adain_blend_alpha``, ``adain_blend_pmap``).
Imported by tests only.

* ``mean_std_f64``: two-pass mean and unbiased variance in float64, std = sqrt(var + eps) in float64.  One pixel gives 0 / 0 = NaN
  as torch.var does.  Returned with the float64 values rounded once to float32: what an implementation that loses nothing gives.
* ``blend``: out = t * w1 + x * w2 with t = (x - mc) / sc * ss + ms, one array operation per operation of the reference, in its
  order.  ``dtype=np.float32`` rounds after every operation, as the reference's torch float32 ops do (no fused multiply-add: numpy
  runs each operation as a loop of its own); ``dtype=np.float64`` is the same expression on the same float32 inputs in double.
  alpha form: w1 = alpha, w2 = float(1 - alpha) computed in double on the host (runtime.blend_alpha; the reference's Python
  scalars reach torch the same way), both rounded to float32 as the C ABI takes them.  pmap form: w1 = 1 - P in ``dtype``, w2 = P.

Every element looks its own image, channel and pixel up from its flat index alone: nothing is grouped, so the yardstick cannot share
an indexing mistake with a kernel that handles several elements at once.

Layouts: ``nhwc`` true = [n][pixels...][c], false = [n][c][pixels...]; the pixel axes may be one (hw) or two (h, w).  Statistics are
[n][c] (style statistics [1][c] or [n][c]); the strength map is [1 or n][pixels...]."""
import numpy as np


def _np(a):
    return a.detach().cpu().numpy() if hasattr(a, "detach") else np.asarray(a)


def _dims(x, nhwc):
    n = x.shape[0]
    c = x.shape[-1] if nhwc else x.shape[1]
    return n, c, x.size // (n * c)


def mean_std_f64(x, nhwc, eps=1e-5):
    """-> dict(mean64, var64, std64 [n][c] float64; mean32, std32: those rounded to float32).  ``eps`` is used as the double it is:
    a caller comparing with a C ABI that takes a float passes float(np.float32(eps))."""
    x = _np(x)
    n, c, hw = _dims(x, nhwc)
    v = x.reshape(n, hw, c).transpose(0, 2, 1) if nhwc else x.reshape(n, c, hw)
    v = v.astype(np.float64)
    mean = v.sum(axis=2) / hw
    with np.errstate(invalid="ignore", divide="ignore"):
        var = ((v - mean[:, :, None]) ** 2).sum(axis=2) / np.float64(hw - 1)
        std = np.sqrt(var + np.float64(eps))
    return dict(mean64=mean, var64=var, std64=std, mean32=mean.astype(np.float32), std32=std.astype(np.float32))


def indices(n, c, hw, nhwc):
    """(image, channel, pixel) of every flat element index, each from the index alone."""
    e = np.arange(n * c * hw, dtype=np.int64)
    img = e // (c * hw)
    if nhwc:
        return img, e % c, (e // c) % hw
    return img, (e // hw) % c, e % hw


def blend(x, nhwc, c_mean, c_std, s_mean, s_std, alpha=None, pmap=None, dtype=np.float32, parts=False):
    """-> out, shaped like ``x``, in ``dtype``; with ``parts`` also a dict of the flat intermediates x, nrm_ss (= (x - mc) / sc * ss),
    t, w1, w2.  Exactly one of ``alpha`` (a Python float) and ``pmap`` is given."""
    assert (alpha is None) != (pmap is None)
    x = _np(x)
    assert x.dtype == np.float32
    n, c, hw = _dims(x, nhwc)
    c_mean, c_std, s_mean, s_std = (_np(a).astype(np.float32).reshape(-1, c) for a in (c_mean, c_std, s_mean, s_std))
    assert c_mean.shape == c_std.shape == (n, c) and s_mean.shape == s_std.shape and s_mean.shape[0] in (1, n)
    img, ch, pix = indices(n, c, hw, nhwc)
    simg = img if s_mean.shape[0] == n else np.zeros_like(img)
    v = x.reshape(-1).astype(dtype)
    mc, sc = c_mean[img, ch].astype(dtype), c_std[img, ch].astype(dtype)
    ms, ss = s_mean[simg, ch].astype(dtype), s_std[simg, ch].astype(dtype)
    if pmap is not None:
        p = _np(pmap).astype(np.float32)
        p = p.reshape(p.shape[0], -1)
        assert p.shape[0] in (1, n) and p.shape[1] == hw
        w2 = p[img if p.shape[0] == n else np.zeros_like(img), pix].astype(dtype)
        w1 = dtype(1.0) - w2
    else:
        w1 = np.full(v.shape, np.float32(alpha), dtype=np.float32).astype(dtype)
        w2 = np.full(v.shape, np.float32(1.0 - float(alpha)), dtype=np.float32).astype(dtype)
    nrm = (v - mc) / sc
    nrm_ss = nrm * ss
    t = nrm_ss + ms
    a = t * w1
    b = v * w2
    out = a + b
    assert out.dtype == dtype
    out = out.reshape(x.shape)
    if parts:
        return out, dict(x=v, nrm_ss=nrm_ss, t=t, w1=w1, w2=w2)
    return out


def self_distance_bound(parts):
    """Per element: what the float32 form may differ from the float64 form by when nothing cancels, 8 * 2^-24 * (|t| |w1| +
    |x| |w2| + |nrm * ss|) on the float64 form's intermediates.  Counting half-ulp roundings: x - mc, the divide and the product by ss
    put 3 on |nrm * ss|; the sum with ms 1 on |t|; 1 - P, t * w1 and the last sum at most 3 on |t| |w1| (|out| <= |t| |w1| +
    |x| |w2|); x * w2 and the last sum 2 on |x| |w2|.  8 covers every count with room for the second-order terms."""
    return 8 * 2.0 ** -24 * (np.abs(parts["t"]) * np.abs(parts["w1"]) + np.abs(parts["x"]) * np.abs(parts["w2"]) + np.abs(parts["nrm_ss"]))
