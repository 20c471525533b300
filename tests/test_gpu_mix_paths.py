"""GPU tests of the layers above ``adain_blend_mix``: ``adain_stylize_u8_mix`` through ``rt.stylize_u8(style_weights=...)``, the
engine's ``set_styles`` / ``style_weights``, the job driver's ``style_weights`` rows, ``style_transfer_interpolated`` against the
oracle's composition of the reference's function, and ``adain_inference`` with a list of styles.  16 x 24 and 40 x 56 uint8 frames,
the seeded weight sets.  Run with ``-m gpu``."""
import numpy as np
import pytest
import torch

import applied_image_processing_amd.synth as synth
from oracle import adain_oracle as O

pytestmark = pytest.mark.gpu

SIZES = [(16, 24), (40, 56)]


def T(a):
    return torch.from_numpy(np.ascontiguousarray(a))


def u8frames(seed, n, h, w):
    return T(np.stack([(synth.image(seed + i, 1, h, w)[0].transpose(1, 2, 0) * 255).astype(np.uint8) for i in range(n)]))


@pytest.fixture(scope="module")
def rt():
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    import applied_image_processing_amd.runtime as rt

    rt.lib()
    return rt


@pytest.fixture(scope="module")
def engine(weights):
    from applied_image_processing_amd.engine import AdaINEngine

    return AdaINEngine(weights[0], weights[1], "cuda:0")


@pytest.fixture(scope="module")
def styles():
    """Three style images of different sizes, float [1,3,h,w]."""
    return [T(synth.image(4100 + i, 1, h, w)) for i, (h, w) in enumerate([(40, 56), (48, 40), (33, 47)])]


def rows(n, k, seed, hw=None):
    """Synthetic per-frame weights in [0.05, 0.9] / k: [n,k], or maps [n,k,hc,wc] with ``hw`` = (hc, wc)."""
    g = torch.Generator().manual_seed(seed)
    shape = (n, k) if hw is None else (n, k) + tuple(hw)
    return ((0.05 + 0.85 * torch.rand(shape, generator=g)) / k * 2).cuda()


# ---- rt.stylize_u8(style_weights=...) = the step-by-step calls ------------------------------------------------------------------------
@pytest.mark.parametrize("h,w", SIZES)
@pytest.mark.parametrize("path", ["alpha", "mask_resized", "depth"])
@pytest.mark.parametrize("maps", [False, True])
def test_one_call_equals_the_steps(rt, engine, styles, h, w, path, maps):
    n, k = 3, 3
    frames = u8frames(4200, n, h, w).cuda()
    engine.set_styles(styles)
    s_mean, s_std = engine.style_stats()
    assert tuple(s_mean.shape) == tuple(s_std.shape) == (k, 512)
    hc, wc = rt.encoded_size(h, w)
    wts = rows(n, k, 1, (hc, wc) if maps else None)
    f = rt.encode_u8(frames, engine.enc)
    c_mean, c_std = rt.mean_std(f, True)
    kw = {}
    if path == "depth":
        depth = [T(synth.smooth_depth(50 + i, 30 + i, 41)).cuda() for i in range(n)]
        kw = dict(depth_maps=depth, depth_offset=0.3, depth_prominence=15)
        p = torch.cat([rt.strength_map(d, hc, wc, 0.3, 15) for d in depth])
        g = rt.blend_mix(f, True, c_mean, c_std, s_mean, s_std, wts, pmap=p)
    else:
        g = rt.blend_mix(f, True, c_mean, c_std, s_mean, s_std, wts, alpha=0.6)
    img = rt.decode(g, engine.dec)
    if path == "mask_resized":
        m = (T(synth.image(60, n, 11, 13)) > 0.4).cuda()
        kw = dict(mask=m)
        img = engine.composite(frames, img, m.float())
    want = rt.quantize_u8(img)
    got = rt.stylize_u8(frames, engine.enc, engine.dec, s_mean, s_std, alpha=0.6, style_weights=wts, **kw)
    assert torch.equal(got, want)


def test_engine_frame_bytes_do_not_depend_on_the_sub_batch(rt, engine, styles):
    engine.set_styles(styles)
    for h, w in SIZES:
        frames = u8frames(4300, 3, h, w).cuda()
        wts = rows(3, 3, 2)
        got = engine.stylize_u8(frames, alpha=0.5, style_weights=wts)
        for i in range(3):
            assert torch.equal(engine.stylize_u8(frames[i:i + 1].contiguous(), alpha=0.5, style_weights=wts[i:i + 1].contiguous()), got[i:i + 1]), (h, w, i)
            assert torch.equal(engine.stylize_u8(frames[i:i + 1].contiguous(), alpha=0.5, style_weights=wts[i]), got[i:i + 1]), (h, w, i)
        assert torch.equal(engine.to_u8(engine.stylize(frames, 0.5, style_weights=wts)), got)
        assert not torch.equal(got[0], got[1])


def test_one_hot_rows_are_the_single_style_bytes(rt, engine, styles):
    frames = u8frames(4400, 3, 40, 56).cuda()
    one_hot = torch.eye(3, device="cuda")
    engine.set_styles(styles)
    mixed = engine.stylize_u8(frames, alpha=0.5, style_weights=one_hot)
    state = engine.style_stats()
    for i in range(3):
        engine.set_style(styles[i].cuda())
        assert torch.equal(engine.stylize_u8(frames[i:i + 1].contiguous(), alpha=0.5), mixed[i:i + 1]), i
    engine.use_style_stats(state)
    assert torch.equal(engine.stylize_u8(frames, alpha=0.5, style_weights=one_hot), mixed)


def test_engine_refusals(rt, engine, styles):
    frames = u8frames(4500, 2, 16, 24).cuda()
    engine.set_styles(styles)
    with pytest.raises(rt.AdainHipError, match="preserve_color"):
        engine.stylize_u8(frames, style_weights=rows(2, 3, 3), preserve_color=True)
    with pytest.raises(rt.AdainHipError, match="preserve_color"):
        engine.stylize(frames, style_weights=rows(2, 3, 3), preserve_color=True)
    with pytest.raises(rt.AdainHipError, match="style_weights"):
        engine.stylize_u8(frames)                                   # three styles and no weights
    with pytest.raises(rt.AdainHipError):
        engine.stylize_u8(frames, style_weights=rows(2, 2, 3))      # two weights for three styles
    with pytest.raises(rt.AdainHipError):
        engine.set_styles([styles[0]] * 17)


# ---- style_transfer_interpolated against the oracle's composition of the reference ------------------------------------------------
@pytest.mark.parametrize("which", ["kaiming", "trained_like"])
def test_style_transfer_interpolated_against_the_oracle(which, weights, weights_tl):
    """The reference's style_transfer(..., interpolation_weights) (test_video.py:30-45) composed from the oracle on the CPU: content
    64 x 64, styles 48 x 56 and 64 x 48 (one AdaIN per style: the reference's batch needs one size).  The project's bar: relative
    L2 <= 1e-4."""
    from applied_image_processing_amd.AdaIN import net, test as t

    vgg_sd, dec_sd = (weights if which == "kaiming" else weights_tl)
    full = synth.to_torch(synth.vgg_state_dict(0, full=True)) if which == "kaiming" else vgg_sd
    net.vgg.load_state_dict(full)
    net.decoder.load_state_dict(dec_sd)
    net.vgg.to("cuda").eval()
    net.decoder.to("cuda").eval()
    try:
        c = T(synth.image(4600, 1, 64, 64))
        ss = [T(synth.image(4601, 1, 48, 56)), T(synth.image(4602, 1, 64, 48))]
        ws = [0.3, 0.7]
        for alpha in (1.0, 0.6):
            out = t.style_transfer_interpolated(net.vgg, net.decoder, c.cuda(), [s.cuda() for s in ss], alpha, ws)
            torch.cuda.synchronize()
            with torch.no_grad():
                content_f = O.encode(vgg_sd, c)
                feat = torch.zeros_like(content_f)
                for w_, s in zip(ws, ss):
                    feat = feat + w_ * O.adaptive_instance_normalization(content_f, O.encode(vgg_sd, s))
                ref = O.decode(dec_sd, feat * alpha + content_f * (1 - alpha))
            rel = float((out.cpu() - ref).norm() / ref.norm())
            print(f"{which} alpha {alpha}: relative L2 {rel:.3e}")
            assert out.shape == ref.shape and rel <= 1e-4
        stacked = torch.cat([T(synth.image(4603 + i, 1, 40, 56)) for i in range(2)]).cuda()          # [K,3,hs,ws], the reference's own form
        a = t.style_transfer_interpolated(net.vgg, net.decoder, c.cuda(), stacked, 0.6, ws)
        b = t.style_transfer_interpolated(net.vgg, net.decoder, c.cuda(), [stacked[0], stacked[1:2]], 0.6, ws)
        assert torch.equal(a, b)
        with pytest.raises(ValueError):
            t.style_transfer_interpolated(net.vgg, net.decoder, c.cuda(), stacked, 0.6, None)
    finally:
        net.vgg.load_state_dict(synth.to_torch(synth.vgg_state_dict(0, full=True)))
        net.decoder.load_state_dict(synth.to_torch(synth.decoder_state_dict(0)))


# ---- the job driver ---------------------------------------------------------------------------------------------------------------
def test_job_driver_slices_the_rows(rt, engine, styles):
    import applied_image_processing_amd.jobs as jobs

    two = styles[:2]
    clip = [f.numpy() for f in u8frames(4700, 6, 16, 24)]
    w = jobs.style_crossfade(6, 2, 2)
    cache = {}
    out, info = jobs.stylize_frames_sharded(engine, clip, two, alpha=0.5, sub_batch=4, style_weights=w, style_cache=cache)
    assert "mix" in cache and tuple(cache["mix"].mean.shape) == (2, 512)
    engine.set_styles(two)
    for k in range(6):
        assert torch.equal(out[k:k + 1], engine.stylize_u8(T(clip[k])[None].cuda(), alpha=0.5, style_weights=T(w[k]))), k
    cut, _ = jobs.stylize_frames_sharded(engine, clip, two, style_of=jobs.style_schedule(6, 2), alpha=0.5, sub_batch=4)
    hot, _ = jobs.stylize_frames_sharded(engine, clip, two, alpha=0.5, sub_batch=5, style_weights=jobs.style_crossfade(6, 2, 0))
    assert torch.equal(cut, hot) and not torch.equal(cut, out)
    with pytest.raises(ValueError):
        jobs.stylize_frames_sharded(engine, clip, two, style_weights=w, preserve_color=True)
    with pytest.raises(ValueError):
        jobs.stylize_frames_sharded(engine, clip, two, style_weights=w[:5])


# ---- adain_inference ------------------------------------------------------------------------------------------------------------
def test_adain_inference_with_two_style_files(rt, weights, tmp_path):
    import io

    from PIL import Image

    from applied_image_processing_amd.AdaIN import test as t
    from applied_image_processing_amd.engine import AdaINEngine

    def img(seed, h, w):
        return Image.fromarray((synth.image(seed, 1, h, w)[0].transpose(1, 2, 0) * 255).astype(np.uint8))

    torch.save(synth.to_torch(synth.vgg_state_dict(0, full=True)), tmp_path / "vgg.pth")
    torch.save(synth.to_torch(synth.decoder_state_dict(0)), tmp_path / "dec.pth")
    content = img(4800, 40, 56)
    paths = []
    for i, (h, w) in enumerate([(48, 56), (64, 48)]):
        paths.append(str(tmp_path / f"style{i}.png"))
        img(4801 + i, h, w).save(paths[-1])
    ws = [0.25, 0.75]
    kw = dict(vgg_str=str(tmp_path / "vgg.pth"), decoder_str=str(tmp_path / "dec.pth"), content_size=0, style_size=0, alpha=0.6, output=str(tmp_path / "o"))
    t.clear_style_cache()
    e0 = t.STYLE_ENCODES[0]
    target = t.adain_inference(content, paths, file_name="a", style_interpolation_weights=ws, **kw)
    t.adain_inference(content, paths, file_name="b", style_interpolation_weights=ws, **kw)
    assert t.STYLE_ENCODES[0] - e0 == 2                                       # each style through the style cache, once
    eng = AdaINEngine(synth.to_torch(synth.vgg_state_dict(0, full=True)), weights[1], "cuda:0")
    eng.set_styles([T(np.asarray(Image.open(p)).transpose(2, 0, 1)[None]).float().div(255) for p in paths])
    frame = eng.stylize_u8(T(np.asarray(content))[None].cuda(), alpha=0.6, style_weights=ws)[0].cpu().numpy()
    buf = io.BytesIO()
    Image.fromarray(frame).save(buf, format="JPEG")
    want = np.asarray(Image.open(io.BytesIO(buf.getvalue())))
    assert target.suffix == ".jpg" and np.array_equal(np.asarray(Image.open(target)), want)
    assert (tmp_path / "o" / "b.jpg").read_bytes() == target.read_bytes()
    with pytest.raises(ValueError):
        t.adain_inference(content, paths, file_name="c", **kw)                 # a list of styles without weights
    with pytest.raises(ValueError):
        t.adain_inference(content, paths, file_name="c", style_interpolation_weights=ws, preserve_color=True, **kw)
    t.clear_style_cache()
