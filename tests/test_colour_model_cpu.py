"""The colorspace oracle (oracle/colorspace_oracle.c) against the independent float64 model (tests/colour_model.py),
and the model against published numbers, so that the oracle and the model cannot share a mistake unnoticed."""

import numpy as np
import pytest

import colour_model as cm
import oracle_lib as ol


# ---- anchors of the model ----------------------------------------------------------------------------------------
def test_bt2087_709_to_2020_matrix():
    want = [[0.6274, 0.3293, 0.0433], [0.0691, 0.9195, 0.0114], [0.0164, 0.0880, 0.8956]]      # BT.2087-0 (4)
    np.testing.assert_allclose(cm.gamut_matrix(1, 9), want, atol=0.5e-4)


@pytest.mark.parametrize("matrix,prim,tol", [(1, 1, 1e-4), (9, 9, 1e-4), (7, 7, 0.5e-3), (4, 4, 0.5e-2)],
                         ids=["bt709", "bt2020", "smpte240m", "fcc"])
def test_kr_kb_from_primaries(matrix, prim, tol):
    """the luma weights the standards state, within their rounding, from the primaries and white"""
    kr, kb = cm.kr_kb_from_primaries(prim)
    assert abs(kr - cm.KR_KB[matrix][0]) <= tol and abs(kb - cm.KR_KB[matrix][1]) <= tol, (kr, kb)


def test_bradford_adapts_white_to_white():
    for p_in, p_out in ((4, 1), (11, 9), (1, 8)):
        np.testing.assert_allclose(cm.gamut_matrix(p_in, p_out).sum(axis=1), 1.0, atol=1e-12)


@pytest.mark.parametrize("nits,code", [(100, 0.5081), (203, 0.5807), (1000, 0.7518), (10000, 1.0)])
def test_pq_codes(nits, code):
    assert abs(cm.pq_inverse_eotf(np.float64(nits / 10000)) - code) <= 5e-4
    assert abs(cm.pq_eotf(np.float64(cm.pq_inverse_eotf(np.float64(nits / 10000)))) * 10000 - nits) <= 1e-6 * nits


def test_hlg_anchors():
    assert abs(cm.hlg_inverse_oetf(np.float64(0.5)) - 1 / 12) < 1e-12
    assert abs(cm.hlg_oetf(np.float64(1 / 12)) - 0.5) < 1e-12
    assert abs(cm.hlg_oetf(np.float64(1.0)) - 1.0) < 1e-6                       # full scale at E = 1
    # BT.2408: 75 % HLG is 203 cd/m2 on a 1000 cd/m2 display (grey: per-component OOTF = the luminance one)
    assert abs(cm.to_linear(18, np.float64(0.75)) * 1000 - 203) <= 1
    assert abs(cm.HLG_B - 0.28466892) < 1e-8 and abs(cm.HLG_C - 0.55991073) < 1e-8


@pytest.mark.parametrize("tc,knee", [(13, cm.SRGB_BETA * 12.92), (7, 4 * cm.SMPTE240_BETA), (18, 0.5)],
                         ids=["srgb", "240m", "hlg"])
def test_piecewise_curves_are_continuous(tc, knee):
    """the two pieces meet at the knee to the rounding of the standard's constants (240M: 4 digits, a 2e-5 step)"""
    below, above = cm.to_linear(tc, np.float64(knee) - 1e-12), cm.to_linear(tc, np.float64(knee) + 1e-12)
    assert abs(below - above) <= 1e-3 * abs(above), (below, above)
    lin = cm.to_linear(tc, np.float64(knee))
    back = cm.to_gamma(tc, np.float64(lin))
    assert abs(back - knee) <= 1e-4


@pytest.mark.parametrize("tc", cm.TRANSFERS)
def test_transfer_pairs_invert(tc):
    v = np.linspace(0.0, 1.0, 401)
    if tc in (9, 10):
        v = v[v > 0.05]                  # the log curves are flat at their floor
    np.testing.assert_allclose(cm.to_gamma(tc, cm.to_linear(tc, v)), v, atol=1e-9)


def test_tone_curves_end_at_peak():
    """every operator but none / linear / clip brings the signal peak to 1 (vf_tonemap's normalisation)"""
    for op in ("hable", "reinhard", "mobius", "gamma"):
        for peak in (10.0, 100.0):
            assert abs(cm.tonemap_curve(op, np.float64(peak), float("nan"), peak) - 1.0) < 1e-6, (op, peak)
    # mobius is the identity up to j, continuous there
    assert cm.tonemap_curve("mobius", np.float64(0.3), float("nan"), 10.0) == 0.3
    assert abs(cm.tonemap_curve("mobius", np.float64(0.3 + 1e-9), float("nan"), 10.0) - 0.3) < 1e-8


# ---- the oracle against the model on lattice frames --------------------------------------------------------------
LATTICE = [(c, d) for c in cm.CASES for d in c[5]]


def check(case, depth, frame, sub=(0, 0)):
    cid, src, _, dst, kw, _ = case
    want = ol.orc_colorspace_frame(frame, ol.colorspace_params(src, dst, **kw), depth=depth, subw=sub[0], subh=sub[1])
    res = cm.Conversion(src, dst, depth, **kw).convert(frame, *sub)
    st, fails = cm.judge(res, want, hdr_source=src[1] in (16, 18))
    assert not fails, f"{cid} at {depth} bits: " + "; ".join(fails)
    return st


@pytest.mark.parametrize("case,depth", LATTICE, ids=[f"{c[0]}-{d}" for c, d in LATTICE])
def test_oracle_against_model_on_the_lattice(built, case, depth):
    """every Y code x a 33 x 33 (Cb, Cr) lattice in 4:4:4: in gamut within 1 code, ill-conditioned samples within
    1 + their spread and under 0.1 %, out of gamut within cm.TOL_OUT_OF_GAMUT wherever the model is finite and
    well-conditioned; the rest (out of gamut) is counted and bounded"""
    st = check(case, depth, cm.lattice_frame(depth))
    assert st["in_gamut"] > 0.1 * st["samples"]
    print(f"{case[0]} {depth}: {st}")


def test_the_pq_pole_saturates_under_hable(built):
    """beyond the PQ pole the linear light is ~1e35; Hable's curve must saturate there, not overflow to NaN"""
    frame = tuple(np.full((2, 2), v, np.uint16) for v in (868, 1023, 0))
    got = ol.orc_colorspace_frame(frame, ol.colorspace_params(cm.HDR10, cm.BT709, peak=100.0), depth=10, subw=0, subh=0)
    assert [int(p[0, 0]) for p in got] == [131, 988, 468]


# ---- chroma resampling -------------------------------------------------------------------------------------------
def resampling_frame(w, h, sub, hard, rng):
    subw, subh = sub
    cw, ch = (w + 1) >> 1 if subw else w, (h + 1) >> 1 if subh else h
    luma = rng.integers(90, 170, (h, w))
    if hard:
        cb = np.where(rng.random((ch, cw)) < 0.5, 112, 144)
        cr = np.where((np.arange(cw)[None, :] // 3 + np.arange(ch)[:, None] // 2) % 2, 114, 142)
    else:
        yy, xx = np.mgrid[0:ch, 0:cw]
        cb = np.round(128 + 14 * np.sin(xx / 3.1 + yy / 5.3))
        cr = np.round(128 + 13 * np.cos(xx / 4.7 - yy / 2.9))
    return luma.astype(np.uint8), cb.astype(np.uint8), cr.astype(np.uint8)


@pytest.mark.parametrize("sub", [(1, 1), (1, 0), (0, 1)], ids=["420", "422", "440"])
@pytest.mark.parametrize("w,h", [(67, 35), (64, 36), (5, 3)])
@pytest.mark.parametrize("hard", [False, True], ids=["smooth", "edges"])
@pytest.mark.parametrize("case", [cm.CASES[0], cm.CASES[1]], ids=["601_709", "709_170m"])
def test_chroma_resampling_against_model(built, sub, w, h, hard, case):
    """up- and down-sampling as the oracle header states it, odd sizes and frame edges included: within 1 code"""
    rng = np.random.default_rng(w * 7 + h + 100 * hard + 10 * sub[0] + sub[1])
    frame = resampling_frame(w, h, sub, hard, rng)
    want = ol.orc_colorspace_frame(frame, ol.colorspace_params(case[1], case[3]), subw=sub[0], subh=sub[1])
    res = cm.Conversion(case[1], case[3], 8).convert(frame, *sub)
    assert all(ig.all() for ig in res.in_gamut)
    for c in range(3):
        assert want[c].shape == res.planes[c].shape
        d = np.abs(want[c].astype(int) - res.planes[c].astype(int))
        assert d.max() <= 1, (c, np.argwhere(d > 1)[:4])


@pytest.mark.parametrize("sub", [(1, 1), (1, 0), (0, 1)], ids=["420", "422", "440"])
def test_lattice_in_subsampled_layouts(built, sub):
    """the 10-bit lattice laid out for 4:2:0 / 4:2:2 / 4:4:0: hard chroma edges between every lattice point"""
    check(cm.CASES[0], 10, cm.lattice_frame(10, ystep=4, sub=sub), sub)
    check(cm.CASES[-4], 10, cm.lattice_frame(10, ystep=4, sub=sub), sub)
