"""CPU: the extended colour model (tests/colour_model_wide.py) against published numbers and against itself, and the
caps of every case tests/test_colorspace_wide_gpu.py runs - the in-gamut, ill-conditioned and excluded fractions
depend on the input and the model alone, so they are asserted here, without a GPU."""
import numpy as np
import pytest

import colour_model as cm
import colour_model_wide as cw


def flat(depth, y, cb, cr):
    dt = np.uint8 if depth == 8 else np.uint16
    return tuple(np.full((2, 2), c, dt) for c in (y, cb, cr))


def px(res):
    return tuple(int(p[0, 0]) for p in res.planes)


def test_cl_constants_are_table_4():
    """BT.2020 table 4: Pb, Nb, Pr, Nr to four decimals, from the OETF with the exact alpha and beta"""
    assert abs(cw.BT2020_ALPHA - 1.09929682680944) < 1e-12 and abs(cw.BT2020_BETA - 0.018053968510807) < 1e-13
    for got, want in ((cw.CL_PB, 0.7910), (cw.CL_NB, 0.9702), (cw.CL_PR, 0.4969), (cw.CL_NR, 0.8591)):
        assert round(got, 4) == want
    # the seven-digit values the filter's host code states, to a unit of their last digit (2e-3 of a 12-bit code)
    for got, want in ((cw.CL_PB, 0.7909854), (cw.CL_NB, 0.9701716), (cw.CL_PR, 0.4969147), (cw.CL_NR, 0.8591209)):
        assert abs(got - want) < 1e-7


def test_ictcp_matrices_keep_grey():
    np.testing.assert_allclose(cw.M_LMS.sum(axis=1), 1.0, atol=1e-15)
    for m in cw.M_ICTCP.values():
        assert m[0].sum() == 1.0
        np.testing.assert_allclose(m[1:].sum(axis=1), 0.0, atol=1e-15)


@pytest.mark.parametrize("src,dst", [(cw.NC, cw.CLSDR), (cw.PQ_NC, cw.PQ_ICTCP)], ids=["nc_cl", "pqnc_ictcp"])
def test_grey_ramp_stays_grey(src, dst):
    """a grey ramp keeps Cb = Cr = the mid code and its Y (I) within a code"""
    ys = np.arange(64, 941, 4, dtype=np.uint16)[None, :].repeat(2, axis=0)
    mid = np.full_like(ys, 512)
    res = cw.Conversion(src, dst, 10, peak=100.0).convert((ys, mid, mid))
    assert np.array_equal(res.planes[1], mid) and np.array_equal(res.planes[2], mid)
    assert np.abs(res.planes[0].astype(int) - ys).max() <= 1


def test_pq_white_is_the_top_of_i():
    """100 % PQ white (10000 cd/m2, every component 1.0): I = the top luma code"""
    res = cw.Conversion(cw.PQ_NC, cw.PQ_ICTCP, 10, peak=100.0).convert(flat(10, 940, 512, 512))
    assert px(res) == (940, 512, 512)


@pytest.mark.parametrize("via", [cw.CLSDR, cw.PQ_CL, cw.PQ_ICTCP, cw.HLG_ICTCP, (9, 14, 12, 1), (12, 13, 12, 1)],
                         ids=["cl", "pq_cl", "pq_ictcp", "hlg_ictcp", "cdnc_2020", "cdnc_p3"])
def test_round_trips_in_the_model(via):
    """X -> new matrix -> X at 10 bits within the 2 / 3 / 3 codes, and on the five colours, of
    test_colorspace_cpu.py::test_round_trips_through_the_new_outputs"""
    start = (via[0], via[1], 9 if via[0] == 9 else 1, 1)
    for code, cb, cr in [(64, 512, 512), (300, 512, 512), (502, 400, 600), (940, 512, 512), (700, 620, 380)]:
        there = cw.Conversion(start, via, 10, tonemap="none").convert(flat(10, code, cb, cr))
        back = cw.Conversion(via, start, 10, tonemap="none").convert(there.planes)
        y, u, v = px(back)
        assert abs(y - code) <= 2 and abs(u - cb) <= 3 and abs(v - cr) <= 3, (via, code, px(there), (y, u, v))


def test_chroma_derived_nc_is_the_named_matrix_where_one_exists():
    assert cw.kr_kb(12, 1) == cm.KR_KB[1] and cw.kr_kb(12, 9) == cm.KR_KB[9]
    kr, kb = cw.kr_kb(12, 12)                                 # Display P3 (SMPTE EG 432-1): Y = 0.2290 R + 0.6917 G + 0.0793 B
    assert abs(kr - 0.2290) < 5e-5 and abs(kb - 0.0793) < 5e-5


def test_what_is_not_covered_is_refused():
    for src, dst in [(cm.BT709, (1, 1, 10, 1)), (cm.BT709, (1, 1, 13, 1)), (cm.BT709, (1, 1, 14, 1)),
                     (cw.PQ_NC, (9, 14, 14, 1)), ((9, 1, 14, 1), cw.NC), (cm.BT709, (10, 1, 12, 1))]:
        with pytest.raises(ValueError):
            cw.Conversion(src, dst, 10)


@pytest.mark.parametrize("case,depth,layout", cw.LATTICE, ids=[f"{c[0]}-{d}-{lay}" for c, d, lay in cw.LATTICE])
def test_caps_of_the_gpu_cases(case, depth, layout):
    """what colour_model.judge caps, from the model alone (its own planes judged): ill-conditioned <= 10 % of in-gamut
    and excluded <= 20 % for CL / ICtCp / PQ / HLG sources, 0.1 % and 5 % otherwise; at least 10 % in gamut; nothing
    ill-conditioned or excluded where only the destination is new"""
    _, src, _, dst, _, _ = case
    res = cw.result(case, depth, layout)
    st, fails = cm.judge(res, res.planes, hdr_source=cw.hdr_source(src))
    print(case[0], depth, layout, {k: st[k] for k in ("samples", "in_gamut", "ill", "excluded")})
    assert not fails, fails
    assert st["in_gamut"] >= 0.10 * st["samples"]
    if cw.matrix_form(src[2]) is None and src[1] not in (16, 18) and cw.matrix_form(dst[2]) is not None:
        assert st["ill"] == 0 and st["excluded"] == 0


def caps(res, src):
    st, fails = cm.judge(res, res.planes, hdr_source=cw.hdr_source(src))
    print({k: st[k] for k in ("samples", "in_gamut", "ill", "excluded")})
    assert not fails, fails
    assert st["in_gamut"] >= 0.10 * st["samples"]


@pytest.mark.parametrize("cid,depth,w,h", cw.EDGES, ids=[f"{c}-{d}-{w}x{h}" for c, d, w, h in cw.EDGES])
def test_caps_of_the_edge_frames(cid, depth, w, h):
    _, src, _, dst, kw, _ = cw.BY_ID[cid]
    caps(cw.Conversion(src, dst, depth, **kw).convert(cw.edge_frame(depth, w, h), 1, 1), src)


def test_caps_of_the_batched_frame_the_model_judges():
    cid, t = cw.BATCHED_JUDGED
    _, src, _, dst, kw, _ = cw.BY_ID[cid]
    caps(cw.Conversion(src, dst, 10, **kw).convert(cw.batched_stream()[t], 1, 1), src)
