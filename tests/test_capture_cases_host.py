"""The graph-capture table (tests/capture_cases.py) without a device: it covers the header, every row's two data sets have equal shapes
and equal host arguments, every row names what differs between them, and where the row carries a restatement's results those differ."""
import numpy as np
import pytest

import abi_launches
import capture_cases as K


def test_every_launch_of_the_header_has_a_row_or_a_reason():
    abi_launches.audit([r.call for r in K.ROWS], K.EXEMPT, "graph capture")
    assert list(K.EXEMPT) == ["adain_tvl1_flow"], "the header states one exception"


def test_the_audit_fails_and_names_a_launch_whose_row_is_missing():
    with pytest.raises(AssertionError, match="adain_gif_encode_u8"):
        abi_launches.audit([r.call for r in K.ROWS if r.call != "adain_gif_encode_u8"], K.EXEMPT, "graph capture")


def test_a_schedule_row_runs_a_network_call_under_the_latency_schedule():
    assert [r.id for r in K.ROWS if r.latency] == ["adain_decode/latency"]


@pytest.mark.parametrize("row", K.ROWS, ids=lambda r: r.id)
def test_the_two_data_sets_have_equal_shapes_and_host_arguments_and_differ(row):
    A, B = row.data()
    a, b = K.inputs_of(A), K.inputs_of(B)
    assert a and list(a) == list(b)
    for name in a:
        x, y = np.asarray(a[name]), np.asarray(b[name])
        assert x.shape == y.shape and x.dtype == y.dtype, (name, x.shape, y.shape, x.dtype, y.dtype)
    assert any(not np.array_equal(a[name], b[name]) for name in a), "set B is set A"
    assert A.get("_host", ()) == B.get("_host", ()), "the host arguments, which a graph bakes in, differ between the sets"
    assert row.host_equal.strip()
    assert row.differs and all(isinstance(v, str) and v.strip() for v in row.differs.values()), "a row names what differs between its sets"
    # the restatement's results for A and B differ where the row says the outputs do
    ea, eb = A.get("_expected", {}), B.get("_expected", {})
    assert list(ea) == list(eb)
    for name in ea:
        assert (name in row.differs) != (name in row.same), f"{name}: an expected value of an output the row says nothing about"
        if name in row.differs:
            x, y = np.asarray(ea[name]), np.asarray(eb[name])
            assert x.shape != y.shape or not np.array_equal(x, y), f"{name}: the restatement gives the same for both sets"
    ra, rb = A.get("_ref", {}), B.get("_ref", {})
    assert list(ra) == list(rb) and (not ra or row.held is not None), "reference values that nothing holds the outputs to"
    for name in ra:
        assert (name in row.differs or name in row.same) and not np.array_equal(ra[name], rb[name]), f"{name}: the restatement gives the same for both sets"
    if "_status" in A:          # the PNG decoder: pixels of slot 0, status of slot 1
        assert A["_status"] == [0, 0] and B["_status"][0] == 0 and B["_status"][1] != 0
        assert not np.array_equal(A["_pixels"][0], B["_pixels"][0])


def test_the_decoders_twins_keep_every_segment_length():
    for kind in ("jpeg", "restart", "progressive"):
        t = K.designed_twins(kind)
        for a, b in zip(t["A"], t["B"]):
            assert a != b and len(a) == len(b)
            assert [len(s) for s in K._segments(kind, a)[1]] == [len(s) for s in K._segments(kind, b)[1]]
            assert K._segments(kind, a)[2] == K._segments(kind, b)[2], "the parsed tables are the same"
