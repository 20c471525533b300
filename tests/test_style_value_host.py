"""Host tests of the style plumbing: the ``Style`` value of ``engine.py`` on CPU tensors, and the job driver's style helper
(``jobs._StyleSwitch``) run by the real ``stylize_frames_sharded`` against a counting stand-in for the engine."""
import pytest
import torch

import applied_image_processing_amd.jobs as jobs
import applied_image_processing_amd.runtime as rt
from applied_image_processing_amd.engine import Style


def one(v):
    return Style(torch.full((1, 512), float(v)), torch.full((1, 512), float(v) + 0.5))


def test_style_unpacks_as_mean_and_std():
    s = Style(torch.zeros(1, 512), torch.ones(1, 512), pixels=torch.zeros(1, 4, 4, 3, dtype=torch.uint8))
    mean, std = s
    assert mean is s.mean and std is s.std and s.k == 1 and s.pixels is not None
    assert Style(mean, std).pixels is None


@pytest.mark.parametrize("k", [1, 3, 16])
def test_stack_keeps_the_rows_in_order_and_drops_the_pixels(k):
    styles = [one(i) for i in range(k)]
    styles[0].pixels = torch.zeros(1, 4, 4, 3, dtype=torch.uint8)
    s = Style.stack(styles)
    assert s.k == k and tuple(s.mean.shape) == tuple(s.std.shape) == (k, 512) and s.pixels is None
    assert s.mean.is_contiguous() and s.std.is_contiguous()
    assert torch.equal(s.mean[:, 0], torch.arange(k, dtype=torch.float32)) and torch.equal(s.std, s.mean + 0.5)


@pytest.mark.parametrize("k", [0, 17])
def test_stack_refuses_no_styles_and_too_many(k):
    with pytest.raises(rt.AdainHipError, match=rf"set_styles: 1 \.\. 16 styles, got {k}"):
        Style.stack([one(0)] * k)


class CountingEngine:
    """AdaINEngine's style surface on the CPU: a style is the mean of its image, ``made`` lists every style that was made."""
    device = torch.device("cpu")

    def __init__(self):
        self.made, self.cur = [], None

    def synchronize(self):
        pass

    def set_style(self, style):
        self.made.append(("style", float(style.mean())))
        self.cur = ("style", float(style.mean()))
        return self

    def set_style_image(self, style):
        self.made.append(("image", float(style.mean())))
        self.cur = ("image", float(style.mean()))
        return self

    def set_styles(self, styles):
        self.made.append(("mix", len(styles)))
        self.cur = ("mix", torch.tensor([float(s.mean()) for s in styles]))
        return self

    def style_stats(self):
        return self.cur

    def use_style_stats(self, stats):
        self.cur = stats
        return self

    def stylize(self, content, alpha=0.5, preserve_color=False, style_weights=None):
        kind, value = self.cur
        assert kind == ("mix" if style_weights is not None else "image" if preserve_color else "style")
        level = (style_weights @ value).view(-1, 1, 1, 1) if style_weights is not None else value
        return content * 0 + level

    def to_u8(self, images):
        return (images * 255 + 0.5).clamp(0, 255).to(torch.uint8).permute(0, 2, 3, 1).contiguous()


STYLE_OF = [0, 0, 1, 1, 0]
LEVELS = [0.2, 0.6]


def run(engine, cache, **mode):
    frames = [torch.rand(3, 12, 20, generator=torch.Generator().manual_seed(i)) for i in range(5)]
    styles = [torch.full((1, 3, 4, 4), v) for v in LEVELS]
    if "style_weights" not in mode:
        mode["style_of"] = STYLE_OF
    out, _ = jobs.stylize_frames_sharded(engine, frames, styles, sub_batch=2, style_cache=cache, **mode)
    return out[:, 0, 0, 0].tolist()


def test_plain_styles_are_made_once_each():
    eng, cache = CountingEngine(), {}
    got = run(eng, cache)
    assert sorted(eng.made) == [("style", pytest.approx(v)) for v in LEVELS] and set(cache) == {0, 1}
    assert got == [int(LEVELS[s] * 255 + 0.5) for s in STYLE_OF]
    assert run(eng, cache) == got and len(eng.made) == 2              # the second job finds both in the cache


def test_preserve_color_keeps_pixel_entries():
    eng, cache = CountingEngine(), {}
    run(eng, cache, preserve_color=True)
    assert sorted(eng.made) == [("image", pytest.approx(v)) for v in LEVELS] and set(cache) == {("pixels", 0), ("pixels", 1)}


def test_style_weights_keep_one_mix_entry():
    eng, cache = CountingEngine(), {}
    got = run(eng, cache, style_weights=jobs.style_crossfade(5, 2, 0))
    assert eng.made == [("mix", 2)] and set(cache) == {"mix"}
    assert got == [int(LEVELS[s] * 255 + 0.5) for s in jobs.style_schedule(5, 2)]


def test_a_cache_filled_by_the_caller_makes_nothing():
    eng = CountingEngine()
    cache = {0: ("style", 0.25)}                                     # one style for the whole job, as the benchmark hands it in
    frames = [torch.zeros(3, 12, 20) for _ in range(5)]
    out, _ = jobs.stylize_frames_sharded(eng, frames, torch.full((1, 3, 4, 4), 0.9), sub_batch=2, style_cache=cache)
    assert eng.made == [] and set(cache) == {0} and out[:, 0, 0, 0].tolist() == [64] * 5
