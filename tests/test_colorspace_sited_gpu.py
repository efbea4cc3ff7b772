"""GPU: the colorspace HIP drop-in and C ABI with the chroma where the stream sites it.  Bit-exact to the sited checker
(tools/colorspace_sited_check.c: the oracle's conversion under the sited up- and down-sampling) where the oracle covers
the conversion, and within colour_model.judge of the sited float64 model (tests/colour_model_sited.py) everywhere - the
constant-luminance case has the model only.  tests/test_colorspace_sited_cpu.py shows that the frames tell the sitings
apart (the left-sited picture fails judge on them) and that the two yardsticks agree."""
import numpy as np
import pytest

from handbrake_amd import hbrt, hip
import chroma_siting_model as csm
import colour_model as cm
import colour_model_sited as cms
import oracle_lib as ol
import sited_lib as sl

pytestmark = pytest.mark.gpu


def _params(cid):
    case = cms.CONVERSIONS[cid][0]
    return ol.colorspace_params(case[1], case[3], **case[4])


def held(got, cid, depth, layout, loc, name):
    """bit-exact to the sited checker (where the oracle covers the conversion), and within the sited model's tolerances"""
    what = f"{cid} {depth} bits {layout} location {loc} {name}"
    fr = cms.frame(name, depth, layout)
    if cms.has_oracle(cid):
        want = sl.colorspace_frame_at(fr, _params(cid), loc, depth, *cms.LAYOUTS[layout][1])
        for c in range(3):
            np.testing.assert_array_equal(np.asarray(got[c]), want[c], err_msg=f"{what}: plane {c} vs the sited checker")
    st, fails = cm.judge(cms.result(cid, depth, layout, loc, name), got, hdr_source=cms.hdr_source(cid))
    assert not fails, f"{what}: " + "; ".join(fails) + f" {st}"


@pytest.mark.parametrize("name", cms.FRAMES)
@pytest.mark.parametrize("cid,depth,layout,loc", cms.CASES, ids=lambda v: str(v))
def test_drop_in_follows_the_location(built, cid, depth, layout, loc, name):
    case = cms.CONVERSIONS[cid][0]
    fr = cms.frame(name, depth, layout)
    hbrt.set_source_color(*case[1])
    hbrt.set_source_chroma_location(loc)
    try:
        out = hbrt.run_stream(hip.filters(), [("hb_filter_colorspace_hip", case[2])], [fr],
                              pix_fmt=hbrt.PIX_FMT[(cms.LAYOUTS[layout][0], depth)])
    finally:
        hbrt.set_source_color()
        hbrt.set_source_chroma_location()
    assert len(out) == 1
    held(out[0].planes, cid, depth, layout, loc, name)


@pytest.fixture(scope="module")
def ctx():
    c = hip.Ctx(0)
    yield c
    c.close()


def _abi(ctx, cid, depth, frames, loc, lw=1, lh=1):
    case = cms.CONVERSIONS[cid][0]
    h, w = frames[0][0].shape
    flt = hip.colorspace_device_filter(ctx, w, h, case[1], case[3], depth=depth, log2_cw=lw, log2_ch=lh,
                                       chroma_location=loc, **case[4])
    try:
        return sl.process_dev(flt, ctx, frames, [p.shape for p in frames[0]], depth)
    finally:
        flt.close()


@pytest.mark.parametrize("cid,depth", [("pq_709_hable", 10), ("601_709", 8)])
def test_batch_of_three_at_topleft(built, ctx, cid, depth):
    """three frames of distinct content through one hbhip_filter_process_dev at location 3"""
    rng = np.random.default_rng(5)
    base = cms.frame("random", depth, "420")
    frames = [base, tuple(np.roll(p, 3, axis=1) for p in base), tuple(p ^ rng.integers(0, 4, p.shape).astype(p.dtype) for p in base)]
    got = _abi(ctx, cid, depth, frames, 3)
    for t, fr in enumerate(frames):
        want = sl.colorspace_frame_at(fr, _params(cid), 3, depth, 1, 1)
        for c in range(3):
            np.testing.assert_array_equal(got[t][c], want[c], err_msg=f"frame {t} plane {c}")
    held(got[0], cid, depth, "420", 3, "random")


@pytest.mark.parametrize("loc", range(7))
def test_every_location_selects_its_form(built, ctx, loc):
    """all seven locations on the random frame, 4:2:0 at 8 bits: 0, 1 and 5 are the call without a location (and the
    oracle itself), 6 is 2 (vertical bottom stays centred), and the four forms differ from each other"""
    fr = cms.frame("random", 8, "420")
    got = _abi(ctx, "601_709", 8, [fr], loc)[0]
    want = sl.colorspace_frame_at(fr, _params("601_709"), loc, 8, 1, 1)
    for c in range(3):
        np.testing.assert_array_equal(got[c], want[c], err_msg=f"location {loc} plane {c}")
    if csm.colour_forms(loc) == (False, False):
        plain = _abi(ctx, "601_709", 8, [fr], None)[0]
        unsited = ol.orc_colorspace_frame(fr, _params("601_709"), depth=8)
        for c in range(3):
            np.testing.assert_array_equal(got[c], plain[c])
            np.testing.assert_array_equal(got[c], unsited[c])
    else:
        unsited = ol.orc_colorspace_frame(fr, _params("601_709"), depth=8)
        assert any(not np.array_equal(got[c], unsited[c]) for c in range(3))


@pytest.mark.parametrize("depth", [8, 10])
def test_440_takes_the_vertical_siting(built, ctx, depth):
    """chroma subsampled vertically only (the C ABI admits it): the rows co-sited at location 3, no columns to site"""
    rng = np.random.default_rng(depth)
    dt, s = (np.uint8 if depth == 8 else np.uint16), depth - 8
    w, h = 70, 66
    fr = ((rng.integers(48, 191, (h, w)) << s).astype(dt), (rng.integers(104, 153, (h // 2, w)) << s).astype(dt),
          (rng.integers(104, 153, (h // 2, w)) << s).astype(dt))
    for loc, vc in ((3, True), (2, False)):
        got = _abi(ctx, "601_709", depth, [fr], loc, lw=0, lh=1)[0]
        want = sl.colorspace_frame_sited(fr, _params("601_709"), depth, 0, 1, False, vc)
        for c in range(3):
            np.testing.assert_array_equal(got[c], want[c], err_msg=f"location {loc} plane {c}")
