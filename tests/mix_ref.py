"""NumPy restatement of the reference's style interpolation (Style_3DGS/AdaIN/test_video.py:36-44 over function.py:21-23): the
yardstick of ``adain_blend_mix`` (csrc/stats.hip), in the manner of tests/blend_ref.py.  Imported by tests only.

``mix``: one array operation per operation of the reference, in its order -

    nrm  = (x - mc) / sc                       function.py:21-22, the same for every style
    b_k  = nrm * ss[k] + ms[k]                 function.py:23
    feat = 0 ; feat = feat + w_k * b_k         test_video.py:37-40, k = 0 .. K-1 in this order
    out  = feat * w1 + x * w2                  test_video.py:44 (alpha form); w1 = 1 - P, w2 = P for the depth-aware form (test.py:70)

``dtype=np.float32`` rounds after every operation (numpy runs each as a loop of its own: no fused multiply-add), ``dtype=np.float64``
is the same expression on the same float32 inputs in double.  The leading ``0 + w_0 * b_0`` is kept as the reference writes it; it
is exact (a kernel that starts from ``w_0 * b_0`` gives the same values; only the sign of a zero could differ, which ``!=`` does
not see).  alpha form: w1 = alpha, w2 = float(1 - alpha) computed in double on the host, both rounded to float32 as the C ABI takes
them.  Weights: [1 or n][K] scalars or [1 or n][K][pixels...] maps (the leading axis is always there); W[k][pixel] stands where
w_k stood.  They are used as given (nothing is normalised).

Every element looks its own image, channel and pixel up from its flat index alone (``blend_ref.indices``)."""
import numpy as np

from blend_ref import _dims, _np, indices


def mix(x, nhwc, c_mean, c_std, s_mean, s_std, weights, alpha=None, pmap=None, dtype=np.float32, parts=False):
    """-> out, shaped like ``x``, in ``dtype``; with ``parts`` also a dict of flat intermediates for ``self_distance_bound``: x, w1,
    w2, k, ``wb`` = sum_k |w_k| |b_k| and ``wns`` = sum_k |w_k| |nrm * ss[k]|.  s_mean / s_std are [K][c]: one set of styles for the
    batch; ``weights`` [1|n][K] or [1|n][K][pixels...].  Exactly one of ``alpha`` (a Python float) and ``pmap`` is given."""
    assert (alpha is None) != (pmap is None)
    x = _np(x)
    assert x.dtype == np.float32
    n, c, hw = _dims(x, nhwc)
    c_mean, c_std, s_mean, s_std = (_np(a).astype(np.float32).reshape(-1, c) for a in (c_mean, c_std, s_mean, s_std))
    k = s_mean.shape[0]
    assert c_mean.shape == c_std.shape == (n, c) and s_std.shape == (k, c) and k >= 1
    w = _np(weights).astype(np.float32)
    assert w.ndim >= 2 and w.shape[0] in (1, n) and w.shape[1] == k, w.shape
    w = w.reshape(w.shape[0], k, -1)
    assert w.shape[2] in (1, hw), w.shape
    img, ch, pix = indices(n, c, hw, nhwc)
    wimg = img if w.shape[0] == n else np.zeros_like(img)
    wpix = pix if w.shape[2] == hw else np.zeros_like(pix)
    v = x.reshape(-1).astype(dtype)
    mc, sc = c_mean[img, ch].astype(dtype), c_std[img, ch].astype(dtype)
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
    feat = np.zeros(v.shape, dtype=dtype)
    wb = np.zeros(v.shape, dtype=np.float64)
    wns = np.zeros(v.shape, dtype=np.float64)
    for j in range(k):
        ms, ss = s_mean[j, ch].astype(dtype), s_std[j, ch].astype(dtype)
        wj = w[wimg, j, wpix].astype(dtype)
        ns = nrm * ss
        b = ns + ms
        t = wj * b
        feat = feat + t
        wb += np.abs(wj).astype(np.float64) * np.abs(b)
        wns += np.abs(wj).astype(np.float64) * np.abs(ns)
    left = feat * w1
    right = v * w2
    out = left + right
    assert out.dtype == dtype
    out = out.reshape(x.shape)
    if parts:
        return out, dict(x=v, w1=w1, w2=w2, k=k, wb=wb, wns=wns)
    return out


def self_distance_bound(parts):
    """Per element: what the float32 form may differ from the float64 form by when nothing cancels, on the float64 form's
    intermediates: 2^-24 * (8 * (wb |w1| + |x| |w2| + wns) + 2 K wb), wb = sum_k |w_k| |b_k| (which bounds |feat| and every partial
    sum of it), wns = sum_k |w_k| |nrm * ss[k]|.  The first term is blend_ref.self_distance_bound's count with the weighted sums
    standing where |t| and |nrm * ss| stood: per style x - mc, the divide and the product by ss[k] put 3 half-ulp roundings on
    |nrm * ss[k]| and the sum with ms[k] 1 on |b_k|, both carried into feat scaled by |w_k|; 1 - P, feat * w1 and the last sum at
    most 3 on |feat| |w1|; x * w2 and the last sum 2 on |x| |w2|; 8 covers every count with room for the second-order terms.  The
    second term is what a mix adds: two roundings per style, w_k * b_k (on |w_k| |b_k|) and the running sum (on a partial sum),
    each at most 2^-24 wb."""
    return 2.0 ** -24 * (8 * (parts["wb"] * np.abs(parts["w1"]) + np.abs(parts["x"]) * np.abs(parts["w2"]) + parts["wns"])
                         + 2 * parts["k"] * parts["wb"])
