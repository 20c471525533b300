"""The GIF reader on the host: gif_file.parse over every designed file of tests/gif_decode_cases.py and every refused kind; the
restatement tests/gif_decode_ref.py pinned to Pillow, array-equal, on every designed file, and to Pillow's exceptions on the damaged ones;
read_gif without a GPU, clip_fps, the command line, the second library's exports and its size query.  No GPU."""
import io
import os
import re
import subprocess

import numpy as np
import pytest
from PIL import Image, ImageSequence

import gif_decode_cases as C
import gif_decode_ref as R
from applied_image_processing_amd import gif_file
from applied_image_processing_amd import runtime as rt

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def pillow(data):
    return np.stack([np.asarray(f.convert("RGB")) for f in ImageSequence.Iterator(Image.open(io.BytesIO(data)))])


def all_sound():
    clips = dict(C.CASES)
    clips.update(C.pillow_clips())
    return clips


def test_the_designed_files_cover_what_they_are_named_for():
    assert len(C.CASES) > 560 and sorted(C.pillow_clips()) == [f"pillow_disposal_{d}" for d in range(4)]
    full = gif_file.parse(C.CASES["table_full_deferred"]).frames[0]
    assert R.unlzw(full.data, 8, 96 * 80)[2] > 4096 + 2                     # more codes than the table has entries
    one = C.greedy(np.full((3, 64), 1), 2).codes[2:-2]                      # behind CLEAR and the root; in front of the remainder and the end code
    assert len(one) > 15 and [c for c, _ in one] == list(range(6, 6 + len(one)))          # every code is the entry just made
    width_steps()
    for d in range(4):
        frames = gif_file.parse(C.pillow_clips()[f"pillow_disposal_{d}"]).frames
        assert len(frames) == 6 and {f.disposal for f in frames} == {d}
        assert d == 2 or any((f.w, f.h) != (50, 40) for f in frames)          # sub-rectangles (for disposal 2 Pillow writes whole frames)


def width_steps():
    co = C.Coder(2).emit(4)
    for i in range(4500):
        co.emit(i % 3)
    assert {w for _, w in co.codes} == set(range(3, 13))                     # a width step at each power of two
    return co.codes


@pytest.mark.parametrize("group", range(8))
def test_restatement_equals_pillow_on_every_designed_file(group):
    names = sorted(all_sound())[group::8]
    for name in names:
        data = all_sound()[name]
        statuses, got = R.decode(data)
        want = pillow(data)
        assert not any(statuses) and got.shape == want.shape and np.array_equal(got, want), name


def test_parser_accepts_every_designed_file_and_its_fields():
    for name, data in all_sound().items():
        clip = gif_file.parse(data)
        ref = R.walk(data)
        im = Image.open(io.BytesIO(data))
        assert (clip.w, clip.h) == im.size == (ref["w"], ref["h"]) and clip.loop == im.info.get("loop") == ref["loop"], name
        assert len(clip.frames) == im.n_frames == len(ref["frames"]) and clip.background == ref["background"], name
        for f, g in zip(clip.frames, ref["frames"]):
            assert (f.left, f.top, f.w, f.h) == g["rect"] and (f.interlace, f.code_size, f.disposal, f.transparent, f.delay_cs) == (
                g["interlace"], g["code_size"], g["disposal"], g["transparent"], g["delay"]) and f.table == g["table"] and f.data == g["data"], name
        assert clip.durations == [f.info.get("duration", 0) for f in ImageSequence.Iterator(im)], name
    clip = gif_file.parse(C.CASES["local_tables"])
    assert [f.local for f in clip.frames] == [True, True, False] and [len(f.table) for f in clip.frames] == [6, 768, 12]
    assert gif_file.parse(C.CASES["no_global_table"]).background == 0 and gif_file.parse(C.CASES["loop_3"]).loop == 3
    assert gif_file.parse(C.CASES["sub_blocks_of_1"]).frames[0].data == gif_file.parse(C.CASES["sub_blocks_of_7"]).frames[0].data


@pytest.mark.parametrize("name", sorted(C.REFUSED))
def test_parser_refuses_with_the_reason(name):
    data, word = C.REFUSED[name]
    with pytest.raises(gif_file.UnsupportedGif, match=re.escape(word)):
        gif_file.parse(data)


def test_parser_refuses_more_than_65535_frames():
    one = C.frame([[1]], 2)
    assert len(gif_file.parse(C.gif((1, 1), C.table_of(C._colours(4)), [one] * 65535)).frames) == 65535
    with pytest.raises(gif_file.UnsupportedGif, match="more than 65535 frames"):
        gif_file.parse(C.gif((1, 1), C.table_of(C._colours(4)), [one] * 65536))


def test_parser_raises_nothing_else_on_truncations_and_byte_flips():
    rng = np.random.default_rng(0)
    names = sorted(C.CASES)
    taken = 0
    for i in range(200):
        data = bytearray(C.CASES[names[int(rng.integers(len(names)))]])
        if i % 2:
            data = data[:int(rng.integers(len(data)))]
        else:
            for _ in range(int(rng.integers(1, 4))):
                data[int(rng.integers(len(data)))] = int(rng.integers(256))
        try:
            clip = gif_file.parse(bytes(data))
        except gif_file.UnsupportedGif as e:
            assert str(e)
            continue
        taken += 1
        rows, blob = rt.gif_decode_table(clip)                    # what is taken is inside the blob
        assert all(r[0] + r[1] <= len(blob) and r[4] + 3 * r[5] <= len(blob) for r in rows)
    assert 0 < taken < 200


@pytest.mark.parametrize("name", sorted(C.DAMAGED))
def test_damaged_files_pillow_raises_and_the_restatement_reports_the_status(name):
    data, status = C.DAMAGED[name]
    with pytest.raises(OSError, match="truncated" if status in (R.TRUNCATED, R.EOI) else "broken data stream"):
        pillow(data)
    assert R.decode(data)[0] == [status]
    assert len(gif_file.parse(data).frames) == 1                  # the parser takes it: the damage is the device's to find


def test_read_gif_without_a_gpu_equals_pillow(tmp_path):
    data = C.pillow_clips()["pillow_disposal_2"]
    path = tmp_path / "clip.gif"
    path.write_bytes(data)
    for source in (data, str(path), path):
        frames, info = gif_file.read_gif(source, device="cpu")
        assert isinstance(frames, np.ndarray) and np.array_equal(frames, pillow(data))
        assert info == gif_file.GifInfo([30, 40, 50, 60, 70, 80], 2, (50, 40))
    with pytest.raises(OSError):
        gif_file.read_gif(C.DAMAGED["cut_at_1000_bytes"][0], device="cpu")


def test_clip_fps():
    info = lambda d: gif_file.GifInfo(d, 0, (1, 1))
    assert gif_file.clip_fps(info([40, 40, 40])) == 25 and gif_file.clip_fps(info([100])) == 10 and gif_file.clip_fps(info([30, 40, 50, 60, 70, 80])) == 100 / 6
    assert gif_file.clip_fps(info([0, 0])) == 20 == gif_file.DEFAULT_FPS and gif_file.clip_fps(info([])) == 20 and gif_file.clip_fps(info([4])) == 20
    assert gif_file.delay_of(gif_file.clip_fps(info([70, 70]))) == 7


def test_the_command_line_extracts_and_parses_as_before(tmp_path, monkeypatch, capsys):
    from applied_image_processing_amd import video

    seen = []
    monkeypatch.setattr(video, "gif_to_frames", lambda *a, **k: seen.append(("extract", a, k)) or gif_file.GifInfo([50, 50], 0, (6, 5)))
    monkeypatch.setattr(video, "frames_to_gif", lambda *a, **k: seen.append(("write", a, k)))
    assert gif_file.main(["--extract", "in.gif", "out_dir"]) == 0 and seen[-1] == ("extract", ("in.gif", "out_dir"), {})
    assert "2 frames of 6 x 5, 20 fps" in capsys.readouterr().out
    assert gif_file.main(["frames", "out.gif", "--palette", "web", "--fps", "12"]) == 0
    assert seen[-1][0] == "write" and seen[-1][1] == ("frames", "out.gif") and seen[-1][2]["palette"] == "web" and seen[-1][2]["fps"] == 12
    with pytest.raises(SystemExit):
        gif_file.main(["frames", "out.gif"])                      # --palette is still required without --extract
    assert "--palette" in capsys.readouterr().err


def test_the_second_library_exports_the_header_and_runtime_launches_through_the_call_path():
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "adain_gif_decode.h")).read(), flags=re.S)
    declared = sorted(set(re.findall(r"ADAIN_API\s+[a-z_ ]+?\*?\s*(adain_[a-z0-9_]+)\s*\(", header)))
    assert declared == sorted(rt.GIF_DECODE_SIGNATURES) == ["adain_gif_decode_last_error", "adain_gif_decode_u8", "adain_gif_decode_u8_bytes"]
    lib = rt.gif_decode_lib()
    nm = subprocess.run(["nm", "-D", "--defined-only", rt.GIF_DECODE_LIB_PATH], capture_output=True, text=True, check=True).stdout
    assert sorted(ln.split()[2] for ln in nm.splitlines() if len(ln.split()) == 3 and ln.split()[1] == "T") == declared
    assert all(hasattr(lib, name) for name in declared) and not set(declared) & set(rt.SIGNATURES)
    assert rt._entry("adain_gif_decode_u8") is not None and rt._entry("adain_png_decode_u8") is not None
    launches = re.findall(r"\b(adain_[a-z0-9_]+)\s*\([^;{}]*\badain_stream_t\b[^;{}]*\)\s*;", header)
    assert launches == ["adain_gif_decode_u8"]
    pkg = os.path.join(ROOT, "applied-image-processing_amd")
    for name in sorted(os.listdir(pkg)):
        if name.endswith(".py"):
            text = open(os.path.join(pkg, name)).read()
            assert not re.search(r"lib\(\)\s*\.\s*adain_gif_decode_u8\s*\(", text), f"{name} calls the launch on the library itself"
            if name != "runtime.py":
                assert "adain_gif_decode_u8\"" not in text, f"{name} launches outside runtime.py"
    text = open(os.path.join(pkg, "runtime.py")).read()
    assert text.count('_launch("adain_gif_decode_u8"') == 1 and "def _launch(name, *args):" in text and "_entry(name)(*args, _stream())" in text
    build = open(os.path.join(pkg, "build.py")).read()
    assert "adain_gif_decode.h" in build and "gif_unlzw.h" in build and "gif_decode.hip" in build


def test_the_header_is_plain_c_and_cxx(tmp_path):
    import shutil

    if shutil.which("gcc") is None or shutil.which("g++") is None:
        pytest.skip("no gcc / g++ here")
    src = tmp_path / "use.c"
    src.write_text('#include "adain_gif_decode.h"\nint main(void) { return adain_gif_decode_last_error() == 0 || ADAIN_GIFD_ROW_FLAGS(2, 1, 3, -1) == 0; }\n')
    inc = os.path.join(ROOT, "include")
    for cmd in (["gcc", "-std=c99", "-pedantic-errors", "-Wall", "-Werror", "-fsyntax-only"], ["g++", "-std=c++17", "-Wall", "-Werror", "-fsyntax-only", "-x", "c++"]):
        r = subprocess.run(cmd + ["-I", inc, str(src)], capture_output=True, text=True)
        assert r.returncode == 0, r.stderr


def test_the_size_query_and_its_refused_edges():
    assert rt.gif_decode_sizes(1, 1, 1, 1) == 1 and rt.gif_decode_sizes(6, 40, 50, 2000) == 12000 and rt.gif_decode_sizes(3, 7, 9, 20) == 60
    assert rt.gif_decode_sizes(65535, 65535, 65535, (1 << 31) - 1) == 65535 * ((1 << 31) - 1)
    assert rt.gif_decode_sizes(65535, 128, 176, 128 * 176) == 65535 * 128 * 176 < 1 << 32
    for dims, word in (((0, 4, 4, 16), "n outside"), ((65536, 4, 4, 16), "n outside"), ((1, 0, 4, 1), "side outside"), ((1, 4, 0, 1), "side outside"),
                       ((1, 65536, 4, 16), "side outside"), ((1, 4, 65536, 16), "side outside"), ((1, 4, 4, 0), "max_frame_pixels"), ((1, 4, 4, 17), "max_frame_pixels"),
                       ((1, 65535, 65535, 1 << 31), "2^31")):
        with pytest.raises(rt.AdainHipError, match=re.escape(word)):
            rt.gif_decode_sizes(*dims)
    assert "gif_decode_u8" in rt.gif_decode_lib().adain_gif_decode_last_error().decode()


def test_the_frame_table_is_the_headers_layout():
    clip = gif_file.parse(C.CASES["local_tables"])
    rows, blob = rt.gif_decode_table(clip)
    assert len(rows) == 3 and all(len(r) == rt.GIFD_ROW_WORDS for r in rows)
    for r, f in zip(rows, clip.frames):
        assert blob[r[0]:r[0] + r[1]] == f.data and blob[r[4]:r[4] + 3 * r[5]] == f.table
        assert r[2] == f.left | f.top << 16 | f.w << 32 | f.h << 48 and r[6] == clip.background == 3 and r[7] == 0
        assert r[3] == f.code_size | int(f.interlace) << 8 | f.disposal << 16 | (0 if f.transparent is None else f.transparent + 1) << 32
    assert rows[1][3] >> 32 == 201 and rows[0][4] != rows[1][4] and len(blob) == 6 + 768 + 12 + sum(len(f.data) for f in clip.frames)
    lead_rows, lead_blob = rt.gif_decode_table(clip, lead=1000)
    assert lead_blob[1000:] == blob and [r[0] - 1000 for r in lead_rows] == [r[0] for r in rows]
