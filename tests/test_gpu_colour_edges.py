"""GPU tests of the device colour transfer (csrc/colour.hip) where its branches depend on the data: the fixtures of
tests/colour_fixtures.py (equal and neighbouring region sizes, regions of two and three pixels, exact ties in a handful of pixels,
rank-1 and zero covariances, saturation at the cast, a near-cancelling principal axis, a frame one block longer than the pixel grid)
through ``rt.colour_transfer_u8`` and, where the regions do not overlap, ``rt.localized_combine_u8``, each both ways round; and the
two calls captured into one hipGraph.  Run with ``-m gpu``.

The bar is equality: every foreground byte is floor(p), p the host path's float64 level before its truncating cast
(colour_fixtures.host_stages), except at the values colour_fixtures.excluded marks - within 1e-9 of an integer level, or of a pixel
whose key is within 1e-12 of another colour's - where the project's bar for this cast applies (at most one level).
tests/test_colour_host.py counts those on the host alone: none on any fixture.  Why 1e-9 is wide enough: the chain from uint8 to p
is about 40 float64 operations at 2.2e-16 relative on values of at most 255; ln 10 times the log-domain magnitude amplifies by at
most ~10 and the row sums of |LMS_TO_RGB| by at most 8.2, which stays below 1e-12 of a level."""
import numpy as np
import pytest
import torch

import colour_fixtures as F
from applied_image_processing_amd import localized as L

pytestmark = pytest.mark.gpu
FILL = 0xA5
BOTH_WAYS = [(name, swapped) for name in F.SMALL + ("stride",) for swapped in (False, True)]


@pytest.fixture(scope="module")
def rt():
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    import applied_image_processing_amd.runtime as rt

    rt.lib()
    return rt


def dev(a):
    return torch.from_numpy(np.array(a)).cuda()


def run(rt, fn, *images, fill=FILL):
    """One call into an output pre-filled with ``fill`` -> (output on the host, record as a dict, record bytes on the device)."""
    images = [dev(a) for a in images]
    out = torch.full(tuple(images[0].shape), fill, dtype=torch.uint8, device="cuda")
    res, record = fn(*images, out=out)
    assert res is out
    return out.cpu().numpy(), rt.colour_record(record), record


def check_levels(what, got_fg, stages, fg):
    """Item 1: equality with floor(p) outside the excluded set, the one-level bar inside it."""
    want = np.floor(stages["levels"]).astype(np.uint8)
    mask, near_int, near_tie = F.excluded(stages, fg)
    d = np.abs(got_fg.astype(int) - want.astype(int))
    print(f"{what}: {d.size} foreground values, excluded {int(mask.sum())} (near an integer {near_int}, near-tied pixels {near_tie}), "
          f"differing {int((d > 0).sum())}, largest difference {int(d.max())}")
    assert got_fg.shape == want.shape
    assert not d[~mask].any(), f"{what}: {(d[~mask] > 0).sum()} values outside the excluded set differ, by up to {d[~mask].max()} levels"
    assert not mask.any() or d[mask].max() <= 1, what


def check_record(rec, stages):
    """Item 3: counts exact, mean, component (sign included) and explained variance against the host's PCA1, status 0."""
    assert rec["status"] == 0 and (rec["fg"]["n"], rec["bg"]["n"]) == (stages["nt"], stages["ns"])
    for key in ("fg", "bg"):
        pca = stages[f"{key}_pca"]
        np.testing.assert_allclose(rec[key]["mean"], pca.mean_, rtol=1e-9, atol=1e-12)
        np.testing.assert_allclose(rec[key]["component"], pca.components_[0], rtol=1e-9, atol=1e-12)
        ev, want = rec[key]["explained_variance"], float(pca.explained_variance_[0])
        if want < 1e-20:
            assert np.isfinite(ev) and ev >= 0
        else:
            np.testing.assert_allclose(ev, want, rtol=1e-9, atol=0)


@pytest.mark.parametrize("name,swapped", BOTH_WAYS)
def test_fixture_against_the_host_levels(rt, name, swapped):
    fg, bg = F.pair(name, swapped)
    s = F.host_stages(name, swapped)
    in_fg = s["in_fg"]
    what = f"{name}{' swapped' if swapped else ''}"
    got, rec, raw = run(rt, rt.colour_transfer_u8, fg, bg)
    check_levels(f"{what} colour_transfer_u8", got[in_fg], s, fg)
    assert np.array_equal(got[~in_fg], fg[~in_fg])                           # item 2: outside the region the input's bytes (never the fill)
    check_record(rec, s)
    combined = None
    if F.combine_fixture(name) is not None:
        content, stylised, m = F.swapped_combine_fixture(name) if swapped else F.combine_fixture(name)
        combined, crec, craw = run(rt, rt.localized_combine_u8, content, stylised, m)
        check_levels(f"{what} localized_combine_u8", combined[in_fg], s, fg)
        assert np.array_equal(combined[m == 1], stylised[m == 1])            # background pixels are the stylised image's
        assert np.array_equal(combined[(m == 0) & ~in_fg], content[(m == 0) & ~in_fg])
        check_record(crec, s)
        assert np.array_equal(combined[in_fg], got[in_fg]) and torch.equal(craw, raw)      # one transfer behind both entry points
    if name == "stride":                                                     # item 4: the pixels past the grid's first pass
        tail = in_fg.ravel()[-256:]
        for image in (got, combined):
            flat = image.reshape(-1, 3)
            assert (flat[-256:][tail] != fg.reshape(-1, 3)[-256:][tail]).any(1).all()          # transferred, not copied
            want = fg.reshape(-1, 3).copy() if image is got else np.where((m == 1).reshape(-1, 1), stylised.reshape(-1, 3), fg.reshape(-1, 3))
            want[in_fg.ravel()] = np.floor(s["levels"]).astype(np.uint8)
            filled = (flat == FILL).all(1)
            assert not (filled & ~(want == FILL).all(1)).any()               # no pixel of the 0xA5 pre-fill survives, over the whole buffer
            if not F.excluded(s, fg)[0].any():
                assert np.array_equal(flat, want)


@pytest.mark.parametrize("name", F.FLAT)
def test_flat_region(rt, name):
    """A region of one colour has zero covariance: the reference's axis is rounding noise, so nothing is compared with it.  What must
    hold: the call succeeds, the record is sane, every output byte is written, nothing outside the region moves, equal inputs give
    equal outputs."""
    fg, bg = F.fixture(name)
    in_fg, in_bg = fg.sum(-1) > 0, bg.sum(-1) > 0
    flat_key, flat_img, flat_in = ("fg", fg, in_fg) if name == "flat_fg" else ("bg", bg, in_bg)
    lab = L.rgb_to_lab_pixels(flat_img[flat_in][:1])[0]
    content, stylised, m = F.combine_fixture(name)
    for fn, images in ((rt.colour_transfer_u8, (fg, bg)), (rt.localized_combine_u8, (content, stylised, m))):
        got, rec, raw = run(rt, fn, *images)                                 # a refused call raises in the wrapper: returning is rc == 0
        again, _, raw2 = run(rt, fn, *images, fill=0x5A)
        assert np.array_equal(got, again) and torch.equal(raw, raw2)         # every byte written (two fills), the same bytes twice
        assert rec["status"] == 0 and (rec["fg"]["n"], rec["bg"]["n"]) == (int(in_fg.sum()), int(in_bg.sum()))
        region = rec[flat_key]
        np.testing.assert_allclose(region["mean"], lab, rtol=0, atol=1e-12)
        for key in ("fg", "bg"):
            c, ev = np.array(rec[key]["component"]), rec[key]["explained_variance"]
            assert np.isfinite(c).all() and abs(float(np.sqrt((c * c).sum())) - 1.0) <= 1e-12
            assert np.isfinite(ev) and ev >= 0
        print(f"{name} {fn.__name__}: flat region's component {region['component']}, explained variance {region['explained_variance']:.3e}")
        if fn is rt.colour_transfer_u8:
            assert np.array_equal(got[~in_fg], fg[~in_fg])
        else:
            assert np.array_equal(got[m == 1], stylised[m == 1]) and np.array_equal(got[(m == 0) & ~in_fg], content[(m == 0) & ~in_fg])
        assert len(np.unique(got[in_fg], axis=0)) == 1                       # one key in (flat_fg) or one value out (flat_bg): one colour


def test_both_calls_in_one_hipgraph(rt):
    """include/adain_hip.h promises that every call may be captured.  The two colour calls, rocprim's sort inside, captured into one
    graph over static buffers (the workspace comes from the graph's pool, as in engine.GraphedStylize), replayed, replayed again on
    other data of another region-size relation: the eager results byte for byte, records included."""
    eager = {}
    for name in ("equal_n", "fg_plus1"):
        fg, bg = F.fixture(name)
        content, stylised, m = F.combine_fixture(name)
        t, _, trec = run(rt, rt.colour_transfer_u8, fg, bg)
        c, _, crec = run(rt, rt.localized_combine_u8, content, stylised, m)
        eager[name] = (t, trec.cpu(), c, crec.cpu())
    assert not torch.equal(eager["equal_n"][1], eager["fg_plus1"][1])        # the second replay has something to show
    static = [dev(a) for a in F.fixture("equal_n") + F.combine_fixture("equal_n")]
    out_t, out_c = (torch.full((9, 11, 3), FILL, dtype=torch.uint8, device="cuda") for _ in range(2))
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):                                            # warm-up outside the capture
        rt.colour_transfer_u8(static[0], static[1], out=out_t)
        rt.localized_combine_u8(static[2], static[3], static[4], out=out_c)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        _, rec_t = rt.colour_transfer_u8(static[0], static[1], out=out_t)
        _, rec_c = rt.localized_combine_u8(static[2], static[3], static[4], out=out_c)
    for name in ("equal_n", "fg_plus1"):
        for buf, a in zip(static, F.fixture(name) + F.combine_fixture(name)):
            buf.copy_(dev(a))                                                # in place: the graph holds the addresses
        for buf in (out_t, out_c, rec_t, rec_c):
            buf.fill_(FILL)
        graph.replay()
        torch.cuda.synchronize()
        t, trec, c, crec = eager[name]
        assert np.array_equal(out_t.cpu().numpy(), t) and np.array_equal(out_c.cpu().numpy(), c), name
        assert torch.equal(rec_t.cpu(), trec) and torch.equal(rec_c.cpu(), crec), name
