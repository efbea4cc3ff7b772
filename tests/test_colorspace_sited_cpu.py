"""CPU: the sited colour-conversion checker (tools/colorspace_sited_check.c) and the sited float64 model
(tests/colour_model_sited.py), the two yardsticks tests/test_colorspace_sited_gpu.py holds the kernel to.
  - with both siting axes off the checker is oracle/colorspace_oracle.c's orc_colorspace_frame, bit for bit;
  - on every (conversion, depth, layout, location, frame) the GPU test runs, the checker passes colour_model.judge
    against the sited model, under judge's own tolerances and caps;
  - the frames can tell the sitings apart: the left-sited / vertically centred oracle FAILS judge against the centre
    and the top-left model on them."""
import numpy as np
import pytest

import chroma_siting_model as csm
import colour_model as cm
import colour_model_sited as cms
import oracle_lib as ol
import sited_lib as sl


def _params(cid):
    case = cms.CONVERSIONS[cid][0]
    return ol.colorspace_params(case[1], case[3], **case[4])


@pytest.mark.parametrize("name", ["columns", "random"])
@pytest.mark.parametrize("layout", list(cms.LAYOUTS))
@pytest.mark.parametrize("cid,depth", [("601_709", 8), ("601_709", 10), ("pq_709_hable", 10), ("709_full", 8)])
def test_checker_without_siting_is_the_oracle(built, cid, depth, layout, name):
    fr = cms.frame(name, depth, layout)
    subw, subh = cms.LAYOUTS[layout][1]
    want = ol.orc_colorspace_frame(fr, _params(cid), depth=depth, subw=subw, subh=subh)
    for loc in (0, 1, 5):                                # the locations that select this form
        got = sl.colorspace_frame_at(fr, _params(cid), loc, depth, subw, subh)
        for c in range(3):
            np.testing.assert_array_equal(got[c], want[c], err_msg=f"location {loc} plane {c}")


ORACLE_CASES = [c for c in cms.CASES if cms.has_oracle(c[0])]


@pytest.mark.parametrize("name", cms.FRAMES)
@pytest.mark.parametrize("cid,depth,layout,loc", ORACLE_CASES, ids=lambda v: str(v))
def test_checker_is_within_the_sited_model(built, cid, depth, layout, loc, name):
    """the yardsticks agree with each other before the kernel meets either: judge's tolerances and caps as they are"""
    fr = cms.frame(name, depth, layout)
    got = sl.colorspace_frame_at(fr, _params(cid), loc, depth, *cms.LAYOUTS[layout][1])
    st, fails = cm.judge(cms.result(cid, depth, layout, loc, name), got, hdr_source=cms.hdr_source(cid))
    assert not fails, f"{cid} {depth} bits {layout} location {loc} {name}: " + "; ".join(fails) + f" {st}"


def test_sited_model_without_siting_is_the_model():
    fr = cms.frame("random", 8, "420")
    conv = cms.conversion("601_709", 8)
    a, b = conv.convert(fr, 1, 1), cms.convert(conv, fr, 1, 1)
    for c in range(3):
        np.testing.assert_allclose(b.value[c], a.value[c], rtol=0, atol=1e-9)
        np.testing.assert_array_equal(b.planes[c], a.planes[c])


# location 2 (centre) differs from the oracle's siting in the columns, location 3 (top-left) in the rows
TELLING = [("columns", 2), ("rows", 3), ("random", 2), ("random", 3), ("tiny", 2), ("tiny", 3)]


@pytest.mark.parametrize("name,loc", TELLING)
@pytest.mark.parametrize("cid,depth", [("601_709", 8), ("pq_709_hable", 10), ("709_full", 8)])
def test_frames_tell_the_sitings_apart(built, cid, depth, name, loc):
    """what the filter did for every location before - the oracle's left-sited, vertically centred picture - is NOT
    within the model of location 2 or 3 on these frames: a test on them fails without the sited forms"""
    fr = cms.frame(name, depth, "420")
    unsited = ol.orc_colorspace_frame(fr, _params(cid), depth=depth, subw=1, subh=1)
    _, fails = cm.judge(cms.result(cid, depth, "420", loc, name), unsited, hdr_source=cms.hdr_source(cid))
    assert fails, f"{name} cannot tell location {loc} from location 1 ({cid}, {depth} bits)"
    assert csm.colour_forms(loc) != csm.colour_forms(1)
