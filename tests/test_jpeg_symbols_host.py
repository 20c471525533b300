"""Conditions on the designed JPEG frames (tests/jpeg_symbols.py), settled on the host from the restatement alone (tests/jpeg_ref.py:
scan_blocks, entropy_bits): which DC categories, run/size symbols, ZRL chains, pattern lengths, bit offsets and chunk-boundary 0xFF
bytes the frames make the entropy coder emit.  They are conditions, not tolerances: they keep tests/test_gpu_jpeg_symbols.py from passing
on a fixture that quietly shrank.  Then the Pillow anchor: on every designed frame the restatements write Pillow's file and decode
Pillow's pixels.  Run with -s for the coverage tables."""
import io

import numpy as np
import pytest
from PIL import Image

import jpeg_decode_ref as D
import jpeg_ref as J
import jpeg_symbols as S

TABLES = ("luma", "chroma")


def test_the_mosaics_reach_what_the_entropy_coder_can_emit():
    cov = S.designed_coverage()
    print("\n" + S.report(cov, "designed mosaics, L and RGB, each at its quality"))
    print(f"  listed as not reached: {S.UNREACHED}")
    for name in TABLES:
        c = cov[name]
        assert c["dc"] == set(range(12)), name
        reached = c["ac"] & S.ALL_AC
        assert c["ac"] <= S.ALL_AC, f"{name}: a symbol outside the tables: {sorted(c['ac'] - S.ALL_AC)}"
        assert len(reached) >= S.AC_FLOOR[name] and S.AC_FLOOR[name] >= {"luma": 158, "chroma": 146}[name], name
        assert all(isinstance(why, str) and why for why in S.UNREACHED[name].values())
        assert reached == S.ALL_AC - set(S.UNREACHED[name]), f"{name}: {sorted(S.ALL_AC - reached)} not reached, {sorted(S.UNREACHED[name])} listed"
        assert {1, 2, 3} <= set(c["chains"]), name
        assert c["ends_at_63"], name
    assert set(range(1, 9)) <= cov["luma"]["chains"][3]
    assert S.LONGEST_PATTERN >= 60 and cov["longest"] == S.LONGEST_PATTERN
    assert cov["offsets"] == set(range(32))
    assert cov["ff_last"] and cov["ff_first"]


def test_the_old_fixtures_reach_less():
    """The numbers that made these frames necessary, recomputed: the content of tests/test_gpu_jpeg.py's byte tests codes 108 luma and 68
    chroma AC symbols, no chroma DC category 11 and patterns of 50 bits at most; the mosaics' coverage is a strict superset."""
    old, new = S.old_fixture_coverage(), S.designed_coverage()
    print("\n" + S.report(old, "the fixtures of tests/test_gpu_jpeg.py"))
    assert len(old["luma"]["ac"]) == 108 and len(old["chroma"]["ac"]) == 68 and old["longest"] == 50
    assert 11 in old["luma"]["dc"] and 11 not in old["chroma"]["dc"]
    for name in TABLES:
        a, b = old[name], new[name]
        assert a["dc"] <= b["dc"] and a["ac"] < b["ac"], name
        assert all(sizes <= b["chains"][k] for k, sizes in a["chains"].items()), name
        assert any(sizes < b["chains"][k] for k, sizes in a["chains"].items()), name
        assert b["ends_at_63"] or not a["ends_at_63"]
    assert old["longest"] < new["longest"] and old["offsets"] <= new["offsets"]


def test_what_the_frames_contain():
    for mode, table, shape in (("L", S.LUMA, (S.SIDE, S.SIDE)), ("RGB", S.CHROMA, (S.SIDE, S.SIDE, 3))):
        blocks = S.designed_blocks(table)
        kinds = {b[1] for b in blocks}
        assert kinds == {"one", "two1", "two3"}
        for kind in kinds:                                                   # every run behind the DC and behind another coefficient
            runs = {b[2] for b in blocks if b[1] == kind}
            assert runs == set(range(63 - {"one": 0, "two1": 1, "two3": 3}[kind])), (mode, kind)
        assert any(b[1] == "one" and b[2] == 62 for b in blocks)              # position 63 alone
        assert {b[4] for b in blocks} == {1, -1}
        fr = S.frames(mode)
        assert len({f[0] for f in fr}) == len(fr)
        assert all(f[2].shape == shape and f[2].dtype == np.uint8 and not f[2].flags.writeable and max(f[2].shape) <= 320 for f in fr)
        by_quality = {}
        for name, quality, img in fr:
            by_quality.setdefault(quality, []).append(len(J.encode(img, quality)))
        assert set(by_quality) == set(S.QUALITIES)
        # uneven batches: no two files of a batch have one length, and beside the dense frame the others are a tenth and less
        assert all(len(v) >= 2 and len(set(v)) == len(v) for v in by_quality.values()), by_quality
        assert max(by_quality[100]) > 10 * min(by_quality[100]) and max(by_quality[75]) > 2 * min(by_quality[75]), by_quality
        ladder = S.dc_ladder(mode)
        if mode == "L":
            assert {0, 255} == set(ladder[-2:].reshape(-1).tolist())
        else:
            assert [tuple(p[0, 0]) for p in ladder[-2:]] == [(255, 255, 0), (0, 0, 255)]
        assert np.array_equal(S._mosaic(ladder, S.SIDE // ladder.shape[1])[:ladder.shape[1], :ladder.shape[1]], fr[-2][2][:ladder.shape[1], :ladder.shape[1]])
        cov100 = S.coverage([f[2] for f in fr if f[1] == 100], 100)
        assert 11 in cov100["luma"]["dc"] and (mode == "L" or 11 in cov100["chroma"]["dc"])


def test_a_block_is_kept_on_its_scan_not_on_its_target():
    """A size-10 value of 640 at position 12 clips: the target says (11, 10), scan_blocks says otherwise, and the block is not kept."""
    px = S.grey_block([(12, 640)], 100)
    nz, run, size, _ = S._coded(px[None], S.LUMA, 100)
    assert not (run[0, 12] == 11 and size[0, 12] == 10)
    assert not any(b[1] == "one" and b[2] == 11 and b[3] == 10 and np.array_equal(b[5], px) for b in S.designed_blocks(S.LUMA))
    assert any(b[2] == 11 and b[3] == 10 for b in S.designed_blocks(S.LUMA))          # the sweep's value is kept instead


def test_the_dense_frame_is_denser_than_the_old_arena_content():
    for mode, c in (("L", 1), ("RGB", 3)):
        name, quality, img = S.densest(mode)
        assert name.endswith("dense")
        new, old = S.bits_per_block(img, quality), S.bits_per_block(J.content("binary", S.SIDE, S.SIDE, c), 75)
        print(f"\n{name}: {new:.1f} bits per block, 0/255 noise at quality 75: {old:.1f}, the bound: {J.max_block_bits()}")
        assert old < new <= J.max_block_bits()


def pillow_bytes(a, quality):
    f = io.BytesIO()
    Image.fromarray(a).save(f, format="JPEG", quality=quality)
    return f.getvalue()


@pytest.mark.parametrize("mode", ["L", "RGB"])
def test_the_restatements_equal_pillow_on_every_designed_frame(mode):
    for name, quality, img in S.frames(mode):
        want = pillow_bytes(img, quality)
        assert J.encode(img, quality) == want, name
        decoded = np.asarray(Image.open(io.BytesIO(want)).convert(mode))
        assert np.array_equal(D.roundtrip(img, quality), decoded), name
