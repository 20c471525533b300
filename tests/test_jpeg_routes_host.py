"""``runtime.JpegRoutes``, the one value that carries a call's JPEG routes, and its callers' host side: the value itself, ``AdaIN.test``'s
setters on top of it, the encode-or-save decision, ``run_depth.main`` restoring what it set, and the video path's call-scoped state across
threads.  No GPU."""
import threading

import pytest

import applied_image_processing_amd.runtime as rt
from applied_image_processing_amd import video
from applied_image_processing_amd.AdaIN import run_depth
from applied_image_processing_amd.AdaIN import test as t

FIELDS = ("encode_on_device", "decode_on_device", "decode_progressive", "options")


@pytest.fixture
def routes_restored():
    before = t.jpeg_routes()
    yield
    t.set_jpeg_routes(before)


# ---- the value ---------------------------------------------------------------------------------------------------------------------
def test_defaults_are_everything_off_and_pillows_default_save():
    r = rt.JpegRoutes()
    assert (r.encode_on_device, r.decode_on_device, r.decode_progressive) == (False, False, False)
    assert r.options == rt.JpegOptions() and r.options.is_default
    assert repr(r) == ("JpegRoutes(encode_on_device=False, decode_on_device=False, decode_progressive=False, "
                       "options=JpegOptions(quality=75, subsampling=2, optimize=False))")


def test_progressive_is_off_without_decode_on_device():
    assert rt.JpegRoutes(decode_progressive=True).decode_progressive is False
    assert rt.JpegRoutes(decode_on_device=True, decode_progressive=True).decode_progressive is True
    assert rt.JpegRoutes(decode_on_device=True).decode_progressive is False
    both = rt.JpegRoutes(decode_on_device=True, decode_progressive=True)
    assert both.replace(decode_on_device=False).decode_progressive is False
    assert rt.JpegRoutes().replace(decode_progressive=True).decode_progressive is False
    assert rt.JpegRoutes().replace(decode_on_device=True, decode_progressive=True) == both
    assert both.replace(encode_on_device=True).decode_progressive is True          # another field's change leaves it


def test_fields_are_bools_and_a_jpeg_options():
    r = rt.JpegRoutes(1, "yes", 1, (90, "4:4:4", True))
    assert (r.encode_on_device, r.decode_on_device, r.decode_progressive) == (True, True, True)
    assert r.options == rt.JpegOptions(90, 0, True)
    assert rt.JpegRoutes(options={"quality": 50}).options == rt.JpegOptions(50)


def test_of_takes_none_an_instance_and_a_dict():
    r = rt.JpegRoutes(True, True, False, rt.JpegOptions(90, 1, False))
    assert rt.JpegRoutes.of(None) == rt.JpegRoutes()
    assert rt.JpegRoutes.of(r) is r
    assert rt.JpegRoutes.of({"encode_on_device": True, "decode_on_device": True, "options": (90, "4:2:2", False)}) == r
    assert rt.JpegRoutes.of({"decode_progressive": True}) == rt.JpegRoutes()
    for bad in (True, (True, False), "on"):
        with pytest.raises(rt.AdainHipError, match="JpegRoutes"):
            rt.JpegRoutes.of(bad)


def test_equality_and_hash_are_the_values():
    a, b = rt.JpegRoutes(True, options=(90, 0, True)), rt.JpegRoutes(1, options=rt.JpegOptions(90, "4:4:4", 1))
    assert a == b and hash(a) == hash(b) and a is not b
    others = [a.replace(encode_on_device=False), a.replace(decode_on_device=True), a.replace(decode_on_device=True, decode_progressive=True),
              a.replace(options=None)]
    assert len({a, b, *others}) == 5
    assert all(a != o for o in others) and a != (True, False, False, rt.JpegOptions(90, 0, True)) and a != rt.JpegOptions(90, 0, True)


def test_the_value_is_immutable():
    r = rt.JpegRoutes()
    for name in FIELDS + ("anything",):
        with pytest.raises(AttributeError):
            setattr(r, name, True)
    assert r.replace(encode_on_device=True) is not r and r == rt.JpegRoutes()
    with pytest.raises(TypeError):
        r.replace(quality=90)


@pytest.mark.parametrize("bad,match", [((0, 2, False), "quality"), ((75, 3, False), "subsampling"), ((75, 2, 2), "optimize"), ("q90", "jpeg_options")])
def test_refused_options_raise_as_jpeg_options_does(bad, match):
    with pytest.raises(rt.AdainHipError, match=match) as want:
        rt.JpegOptions.of(bad)
    for make in (lambda: rt.JpegRoutes(options=bad), lambda: rt.JpegRoutes().replace(options=bad), lambda: rt.JpegRoutes.of({"options": bad})):
        with pytest.raises(rt.AdainHipError, match=match) as got:
            make()
        assert str(got.value) == str(want.value)


# ---- the setters of AdaIN.test -----------------------------------------------------------------------------------------------------
def test_each_setter_returns_its_previous_field_and_changes_only_its_own(routes_restored):
    start = rt.JpegRoutes(False, True, True, (60, 1, True))
    t.set_jpeg_routes(start)

    assert t.set_device_jpeg(True) is False
    assert t.jpeg_routes() == start.replace(encode_on_device=True)
    assert t.set_device_jpeg(False) is True and t.jpeg_routes() == start

    assert t.set_jpeg_save_options(90, "4:4:4") == rt.JpegOptions(60, 1, True)
    assert t.jpeg_routes() == start.replace(options=(90, 0, False))
    assert t.set_jpeg_save_options(rt.JpegOptions(60, 1, True)) == rt.JpegOptions(90, 0, False) and t.jpeg_routes() == start
    assert t.set_jpeg_save_options() == rt.JpegOptions(60, 1, True) and t.jpeg_routes() == start.replace(options=None)
    t.set_jpeg_save_options(60, 1, True)

    assert t.set_device_jpeg_decode(False) is True
    assert t.jpeg_routes() == start.replace(decode_on_device=False) and t.jpeg_routes().decode_progressive is False
    assert t.set_device_jpeg_decode(True) is False
    assert t.jpeg_routes() == start.replace(decode_progressive=False)          # ``progressive`` defaults to off with every call
    assert t.set_device_jpeg_decode(True, progressive=True) is True and t.jpeg_routes() == start


def test_progressive_stays_off_when_decode_is_switched_off(routes_restored):
    t.set_jpeg_routes(None)
    assert t.set_device_jpeg_decode(False, progressive=True) is False
    assert t.jpeg_routes() == rt.JpegRoutes()


def test_set_jpeg_routes_returns_the_previous_value_and_a_round_trip_restores_it(routes_restored):
    a, b = rt.JpegRoutes(True, True, True, (90, 0, True)), rt.JpegRoutes(decode_on_device=True)
    t.set_jpeg_routes(a)
    assert t.set_jpeg_routes(b) == a and t.jpeg_routes() == b
    assert t.set_jpeg_routes({"encode_on_device": True}) == b and t.jpeg_routes() == rt.JpegRoutes(True)
    assert t.set_jpeg_routes(None) == rt.JpegRoutes(True) and t.jpeg_routes() == rt.JpegRoutes()
    prev = t.set_jpeg_routes(a)
    t.set_device_jpeg(False), t.set_jpeg_save_options(50), t.set_device_jpeg_decode(False)
    t.set_jpeg_routes(prev)
    assert t.jpeg_routes() == rt.JpegRoutes()
    with pytest.raises(rt.AdainHipError, match="quality"):
        t.set_jpeg_save_options(0)
    assert t.jpeg_routes() == rt.JpegRoutes()          # a refused value changes nothing


# ---- the decision ------------------------------------------------------------------------------------------------------------------
def test_the_device_encodes_jpeg_paths_only_and_only_when_switched_on(tmp_path):
    on, off = rt.JpegRoutes(encode_on_device=True), rt.JpegRoutes(decode_on_device=True)
    for path in ("a.jpg", "A.JPEG", "dir.png/b.Jpg", tmp_path / "c.jpeg"):
        assert on.encodes(path) is True and on.encodes([path]) is True and off.encodes(path) is False and rt.is_jpeg_path(path)
    for path in ("a.png", "a.jpg.png", "jpg", tmp_path / "c.bmp"):
        assert on.encodes(path) is False and off.encodes(path) is False and not rt.is_jpeg_path(path)
    assert on.encodes(["a.jpg", "b.JPEG", tmp_path / "c.jpeg"]) is True
    assert on.encodes(["a.jpg", "b.png", "c.jpeg"]) is False          # one file of a block that PIL must save: PIL saves the block
    assert on.encodes([]) is False and on.encodes(()) is False
    assert off.encodes(["a.jpg", "b.JPEG"]) is False and off.encodes([]) is False


def test_the_host_route_of_the_writer_is_options_save(tmp_path):
    """A frame on the host, the switch off or a .png path: the file ``JpegOptions.save`` writes, and the three steps are marked."""
    import numpy as np
    import torch
    from PIL import Image

    frame = (np.arange(16 * 24 * 3) % 251).astype(np.uint8).reshape(16, 24, 3)
    options = rt.JpegOptions(90, "4:4:4", True)
    for name, routes in (("a.jpg", rt.JpegRoutes(options=options)), ("b.png", rt.JpegRoutes(True, options=options))):
        options.save(Image.fromarray(frame), tmp_path / ("want_" + name))
        for form in (frame, torch.from_numpy(frame)[None], torch.from_numpy(frame)):
            marks = []
            routes.write(form, tmp_path / name, lambda: marks.append(1))
            assert (tmp_path / name).read_bytes() == (tmp_path / ("want_" + name)).read_bytes() and len(marks) == 3
    rt.JpegRoutes().write(frame[:, :, :1], tmp_path / "grey.jpg")
    assert Image.open(tmp_path / "grey.jpg").mode == "L"


# ---- run_depth.main ----------------------------------------------------------------------------------------------------------------
def test_run_depth_restores_the_routes_and_the_coral_switch_when_the_call_raises(routes_restored, monkeypatch):
    before = rt.JpegRoutes(False, True, False, (60, 1, True))
    t.set_jpeg_routes(before)
    coral_before = t.set_device_coral(False)
    seen = []

    def failing(*args, **kwargs):
        seen.append((t.jpeg_routes(), t._device_coral_on))
        raise RuntimeError("no device here")

    monkeypatch.setattr(run_depth, "adain_inference", failing)
    try:
        with pytest.raises(RuntimeError, match="no device here"):
            run_depth.main(["--content", "c.jpg", "--style", "s.jpg", "--jpeg_on_device", "--jpeg_quality", "90", "--jpeg_subsampling", "4:4:4",
                            "--jpeg_decode_progressive", "--coral_on_device"])
        assert seen == [(rt.JpegRoutes(True, True, True, (90, 0, False)), True)]          # what the flags say, during the call
        assert t.jpeg_routes() == before and t._device_coral_on is False
        with pytest.raises(RuntimeError, match="no device here"):
            run_depth.main(["--content", "c.jpg", "--style", "s.jpg"])
        assert seen[1] == (rt.JpegRoutes(), False) and t.jpeg_routes() == before and t._device_coral_on is False
    finally:
        t.set_device_coral(coral_before)


# ---- the video path's call-scoped routes -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("raises", [False, True])
def test_a_clips_routes_are_invisible_to_other_threads_and_gone_afterwards(raises):
    """Thread A is inside a clip's scope with decode_on_device=True and waits; thread B reads the default meanwhile; after A has left -
    normally or with an exception - both read the default."""
    clip = rt.JpegRoutes(decode_on_device=True, decode_progressive=True)
    inside, b_done = threading.Event(), threading.Event()
    seen = {}

    def a():
        try:
            with video._routes_scope(clip):
                seen["a inside"] = video._routes.get()
                inside.set()
                assert b_done.wait(30)
                if raises:
                    raise KeyError("the clip failed")
        except KeyError:
            seen["a raised"] = True
        seen["a after"] = video._routes.get()

    def b():
        assert inside.wait(30)
        seen["b meanwhile"] = video._routes.get()
        b_done.set()
        ta.join(30)
        seen["b after"] = video._routes.get()

    ta, tb = threading.Thread(target=a), threading.Thread(target=b)
    ta.start(), tb.start()
    tb.join(60)
    assert not ta.is_alive() and not tb.is_alive()
    assert seen["a inside"] == clip and seen.get("a raised", False) is raises
    assert seen["b meanwhile"] == seen["a after"] == seen["b after"] == video._routes.get() == rt.JpegRoutes()
