"""The arithmetic of every row of tests/far_batch.py, without a device: the buffers a row names pass 2^32 bytes (sized by the
library's host-only ``*_bytes`` queries where the library sizes them), the frame size does not divide 2^32, P is coprime to
floor(2^32 / F), the row fits the memory cap, and its P expected values exist and differ pairwise.  And the table's completeness: every
launch of include/adain_hip.h (tests/abi_launches.py) is the call of a row or a key of far_batch.OUT_OF_SCOPE."""
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


def test_every_launch_of_the_header_has_a_row_or_a_reason():
    """The table cannot fall behind the header: a declaration of include/adain_hip.h that ends in ``adain_stream_t stream`` is the
    ``call`` of a row or a key of OUT_OF_SCOPE, never both, and OUT_OF_SCOPE names nothing the header does not declare."""
    import abi_launches

    assert len(abi_launches.launches()) >= 58
    abi_launches.audit({c.call for c in B.CASES}, B.OUT_OF_SCOPE, "tests/far_batch.py")


def test_the_header_parse_sees_a_new_launch_and_nothing_else():
    """What the check above rests on: a launch added to the header's text is found, whatever its line breaks and comments; a host-only
    query and a declaration that only mentions a stream in a comment are not."""
    import abi_launches

    with open(abi_launches.HEADER) as f:
        text = f.read()
    more = text + ("\nADAIN_API int adain_new_thing_u8(const uint8_t* src, int n, /* frames */ int h,\n        int w,   // width\n"
                   "        adain_stream_t\n        stream);\n"
                   "ADAIN_API int adain_new_thing_u8_bytes(int n, int h, int w, size_t* workspace_bytes);   /* adain_stream_t stream */\n")
    assert abi_launches.launches(more) == abi_launches.launches(text) + ["adain_new_thing_u8"]
    assert "adain_image_metrics_grad_f32" in abi_launches.launches() and "adain_image_metrics_grad_f32_bytes" not in abi_launches.launches()


def test_the_gradient_rows_are_the_ones_the_gradients_own_tests_use():
    import metrics_grad_cases as K

    rows = [list(row) for _kind, row in B.GRAD_ROWS]
    assert rows[:4] == [K.WEIGHTS[k][0] for k in ("ssim", "mse", "l1", "mixed")] and rows[6] == K.WEIGHTS["mixed"][1]
    assert len({tuple(r) for r in rows}) == B.P and rows[4] == [0.0, 0.0, 0.0]
    kind, (ssim, mse, l1) = B.GRAD_ROWS[5]
    assert kind == "no_ssim" and ssim == 0.0 and mse > 0.0 and l1 > 0.0, "one sign: the two terms of a sample cannot cancel"
    assert len(set(B.GUIDE_WEIGHTS)) == B.P and B.GUIDE_WEIGHTS.count(0.0) == 1
    assert B.GUIDE_L1_HW[1] % 4 == 0 and B.GUIDE_GRAD_HW[1] % 4 != 0, "one case per kernel form"


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


def test_the_first_layers_operands_are_integer_exact():
    """The far-batch first layer is a tests/edge_exact.py case: the fold's and the layer's partial sums stay below 2^24."""
    import edge_exact as E

    c = B.first_layer_case()
    assert (c.n, c.H, c.W) == (B.P, B.FIRST_H, B.FIRST_W) and len(E.first_tiles(c.H, c.W)) == 4
    a, b = E.first_headroom(E.first_image(c))
    assert a < E.CAP and b < E.CAP, (a, b)


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
