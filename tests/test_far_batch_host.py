"""The arithmetic of every row of tests/far_batch.py, without a device: the buffers a row names pass 2^32 bytes (sized by the
library's host-only ``*_bytes`` queries where the library sizes them), the frame size does not divide 2^32, P is coprime to
floor(2^32 / F), the row fits the memory cap, and its P expected values exist and differ pairwise."""
import math

import numpy as np
import pytest

import far_batch as B


def test_the_default_frame_is_the_one_the_table_describes():
    F = B.H * B.W * 3
    assert F == 67584 and B.N * F > B.TWO32 and B.N * F == 4429117440
    assert B.TWO32 % F == 4096 and B.TWO32 // F == 63550 and 63550 % B.P == 4 and math.gcd(B.P, 63550) == 1
    assert (1 << 31) // F == 31775          # frame 31775 straddles 2^31, frames 63550 .. 65534 lie past 2^32
    assert B.P == 7 and B.N == 65535 and B.CAP == 32 << 30 and B.PIECE == 1 << 30


@pytest.mark.parametrize("case", B.CASES, ids=[c.id for c in B.CASES])
def test_the_row_passes_2_32_where_it_says(case):
    B.check_arithmetic(case)
    assert case.past, "a row aims at one buffer at least"
    roles = {b[1] for b in case.buffers()}
    assert roles <= {"source", "result", "workspace", "rows", "streams"}


@pytest.mark.parametrize("case", B.CASES, ids=[c.id for c in B.CASES])
def test_the_expected_values_exist_and_differ(case):
    inputs, expected = case.make()
    assert inputs and expected
    assert set(case.same) < set(range(len(expected))) or case.id == "quantize_palette_u8/global", "one expected value at least tells the patterns apart"
    for j, e in enumerate(expected):
        assert isinstance(e, np.ndarray) or all(isinstance(x, (bytes, np.ndarray)) for x in e)
        if j in case.same:
            assert case.same[j] and not B.distinct(e)
        else:
            assert B.distinct(e), f"expected value {j}: two patterns have one result, a frame read from the wrong place could pass"


def test_every_buffer_of_every_call_passes_2_32_in_some_case():
    """Per call the union of the buffers its rows name; a buffer no row takes past 2^32 must be named in ``below`` by every row of the call."""
    calls = {}
    for c in B.CASES:
        entry = calls.setdefault(c.call, {"past": set(), "all": set(), "below": {}})
        entry["past"] |= set(c.past)
        entry["all"] |= {b[0] for b in c.buffers()}
        entry["below"].update(c.below)
    for call, e in calls.items():
        for name in e["all"] - e["past"]:
            assert e["below"].get(name), f"{call}: no case takes {name} past 2^32 and none says why"


def test_ids_are_unique_and_families_known():
    assert len({c.id for c in B.CASES}) == len(B.CASES)
    assert {c.family for c in B.CASES} <= {"pixel", "resize", "encode", "decode", "palette", "metrics"}


@pytest.mark.parametrize("entry", ["wino", "poly"])
def test_the_conv_layers_operands_are_integer_exact(entry):
    """The far-batch conv layers are tests/conv_exact.py layers: every partial sum and every output-transform sum below 2^24."""
    import conv_exact as X

    c = B.conv_exact_case(entry)
    assert (c.cin, c.cout, c.hs, c.ws) == (B.CONV_C, B.CONV_C, B.CONV_H, B.CONV_W) and c.n == B.P
    for form, (a, b) in X.headroom(c).items():
        assert a < X.CAP and b < X.CAP, (entry, form, a, b)


@pytest.mark.parametrize("kind", sorted(B.DECODERS))
def test_the_decoders_tables_put_every_segment_past_2_32(kind):
    """The offsets computed arithmetically are the ones a walk over the files gives: behind the lead, back to back, pattern i % P."""
    d = B.decode_files(kind)
    n = 3 * B.P + 2
    off, ln, group, groups = B.decode_tables(kind, n, lead=5)
    at, want_off, want_ln = 5, [], []
    for i in range(n):
        for length in d["lengths"][i % B.P]:
            want_off.append(at)
            want_ln.append(length)
            at += length
    assert off.tolist() == want_off + ([at] if kind == "png" else []) and ln.tolist() == want_ln
    assert group == sum(map(len, d["segments"])) and groups == 4 and 5 + groups * group >= at
    off, ln, group, groups = B.decode_tables(kind, B.N)
    assert off.dtype == np.uint64 and ln.dtype == np.uint32 and int(off.min()) > B.TWO32 and int(off[-1]) + int(ln[-1]) <= B.LEAD + groups * group
    assert B.distinct(d["segments"]) and (d["blobs"] is None or len(d["blobs"]) == B.P)
