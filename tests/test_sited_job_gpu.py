"""GPU: init->chroma_location reaches both zscale drop-ins behind the adapters.  One device-resident job on yuv420p10le,
HDR10, built the way do_job() builds it (hbh_job_open: by id, so crop/scale 256 x 128 -> 128 x 64 runs before the
PQ -> BT.709 hable colour conversion), with the source's chroma top-left (location 3): the pictures equal the sited
checker on the crop/scale oracle under the model's shifts.  The same job at location 1 is what it was before."""
import numpy as np
import pytest

from handbrake_amd import hbrt, hip
import colour_model_sited as cms
import oracle_lib as ol
import sited_lib as sl

pytestmark = pytest.mark.gpu
F = hbrt.FILTER_ID
W, H, OW, OH, DEPTH = 256, 128, 128, 64, 10
CASE = cms.CONVERSIONS["pq_709_hable"][0]
UP, DOWN = "HIP upload adapter", "HIP download adapter"


@pytest.fixture()
def job_filters(built):
    # both filters are settings holders for an avfilter graph in the reference: their ids resolve to the drop-ins
    ids = {F["crop_scale"]: "hb_filter_crop_scale_hip", F["colorspace"]: "hb_filter_colorspace_hip"}
    hbrt.register_filters(hip.filters(), ids)
    hbrt.set_source_color(*CASE[1])
    yield [(F["colorspace"], CASE[2]), (F["crop_scale"], f"width={OW}:height={OH}")]
    hbrt.set_source_color()
    hbrt.set_source_chroma_location()
    hbrt.register_filters(hip.filters(), {k: None for k in ids})


def frames():
    rng = np.random.default_rng(3)
    s = DEPTH - 8
    return [((rng.integers(48, 191, (H, W)) << s).astype(np.uint16), (rng.integers(104, 153, (H // 2, W // 2)) << s).astype(np.uint16),
             (rng.integers(104, 153, (H // 2, W // 2)) << s).astype(np.uint16)) for _ in range(3)]


def run(filters, loc):
    hbrt.set_source_chroma_location(loc)
    names, out = hbrt.run_job(filters, frames(), pix_fmt=hbrt.PIX_FMT[("2x2", DEPTH)], use_hip=True)
    assert names[0] == UP and names[-1] == DOWN and len(names) == 4, names
    assert "scale" in names[1].lower() and "colorspace" in names[2].lower(), names      # by id: 22 before 32
    assert len(out) == 3
    return out


def test_topleft_source_reaches_both_drop_ins(job_filters):
    params = ol.colorspace_params(CASE[1], CASE[3], **CASE[4])
    out = run(job_filters, 3)
    left = []
    for o, fr in zip(out, frames()):
        scaled = sl.cropscale_frame_at(fr, OW, OH, 3, DEPTH, "2x2")
        want = sl.colorspace_frame_at(scaled, params, 3, DEPTH, 1, 1)
        left.append(ol.orc_colorspace_frame(ol.orc_cropscale_frame(fr, OW, OH, depth=DEPTH), params, depth=DEPTH))
        for c in range(3):
            np.testing.assert_array_equal(o.planes[c], want[c], err_msg=f"plane {c}")
        # each drop-in alone on the other's left-sited picture is something else again
        half = sl.colorspace_frame_at(ol.orc_cropscale_frame(fr, OW, OH, depth=DEPTH), params, 3, DEPTH, 1, 1)
        assert not np.array_equal(o.planes[1], half[1]) and not np.array_equal(o.planes[1], left[-1][1])


def test_left_sited_source_is_as_before(job_filters):
    params = ol.colorspace_params(CASE[1], CASE[3], **CASE[4])
    for o, fr in zip(run(job_filters, 1), frames()):
        want = ol.orc_colorspace_frame(ol.orc_cropscale_frame(fr, OW, OH, depth=DEPTH), params, depth=DEPTH)
        for c in range(3):
            np.testing.assert_array_equal(o.planes[c], want[c], err_msg=f"plane {c}")
