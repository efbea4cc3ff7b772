"""CPU: the two models of the format filter's chroma down-sampling (tests/format_resample_model.py) against the definition
- coefficient sums, flat planes, siting by position - and against each other."""
import numpy as np
import pytest

import format_resample_model as m

DEPTHS = (8, 10, 12)
SIZES = (11, 12, 19, 33, 34, 37, 38, 66, 67, 70, 130, 540, 541, 1080)


def _dt(depth):
    return np.uint8 if depth == 8 else np.uint16


@pytest.mark.parametrize("one,dst_pos", [(1 << 14, 64), (1 << 12, 128)])
def test_every_coefficient_row_sums_to_one(one, dst_pos):
    """14-bit horizontal (left-sited: target position 64) and 12-bit vertical (centred: 128) tables, even and odd source
    sizes from the smallest the filter takes: every row sums to exactly `one`, and no row is longer than nine taps"""
    for src in SIZES:
        pos, coef, taps = m.sws_bicubic_table(src, -(-src // 2), one, 128, dst_pos)
        assert 7 <= taps <= 9
        assert len(coef) == -(-src // 2)
        for i, row in enumerate(coef):
            assert sum(row) == one, f"src {src} row {i}: {row}"
            assert 0 <= pos[i] and pos[i] + taps <= src


def test_identity_dimension_is_one_tap():
    pos, coef, taps = m.sws_bicubic_table(33, 33, 1 << 14, 64, 64)
    assert taps == 1 and pos == list(range(33)) and coef[0] == [1 << 14]


@pytest.mark.parametrize("depth", DEPTHS)
@pytest.mark.parametrize("src,dst", m.PAIRS)
def test_flat_plane_stays_flat(depth, src, dst):
    full = (1 << depth) - 1
    for value in (0, 1, full // 2, full - 1, full):
        for shape in ((38, 66), (37, 67)):
            p = np.full(shape, value, _dt(depth))
            out = m.resample_frame((p, p, p), depth, src, dst)
            for c in range(3):
                assert out[c].min() == value and out[c].max() == value, f"{value} plane {c}"
            f64 = m.resample_frame_f64((p, p, p), depth, src, dst)
            assert f64[1].min() == value and f64[1].max() == value


@pytest.mark.parametrize("depth", DEPTHS)
def test_siting_by_position(depth):
    """a ramp is reproduced by any interpolating filter at the position it samples: the horizontal one comes out as
    a + b * 2i (co-sited with source column 2i), the vertical one as a + b * (2j + 0.5) (midway between rows 2j, 2j + 1)"""
    a, b = 3 << (depth - 8), 3 << (depth - 8)
    h, w = 40, 64
    x = np.arange(w)[None, :].repeat(h, axis=0)
    y = np.arange(h)[:, None].repeat(w, axis=1)
    for model in (m.resample_plane, m.resample_plane_f64):
        hr = model((a + b * x).astype(_dt(depth)), depth, True, False).astype(np.float64)
        want = a + b * 2.0 * np.arange(w // 2)
        assert np.abs(hr[:, 4:-4] - want[None, 4:-4]).max() <= 1
        vr = model((a + b * y).astype(_dt(depth)), depth, False, True).astype(np.float64)
        want = a + b * (2.0 * np.arange(h // 2) + 0.5)
        assert np.abs(vr[4:-4] - want[4:-4, None]).max() <= 1
        both = model((a + b * x).astype(_dt(depth)), depth, True, True).astype(np.float64)
        assert both.shape == (h // 2, w // 2)
        assert np.abs(both[:, 4:-4] - (a + b * 2.0 * np.arange(w // 2))[None, 4:-4]).max() <= 1


def _measure(kinds, pairs, sizes=((66, 38), (67, 37)), saturate=False):
    worst = {d: 0 for d in DEPTHS}
    share = 0.0
    for kind in kinds:
        for depth in DEPTHS:
            for src, dst in pairs:
                for w, h in sizes:
                    fr = m.frame(kind, w, h, 0, depth, src)
                    gi = m.resample_frame(fr, depth, src, dst)
                    (sw, sh), (tw, th) = m.SUB[src], m.SUB[dst]
                    gf = [m.resample_plane_f64(p, depth, tw > sw, th > sh, saturate=saturate) for p in fr[1:]]
                    assert np.array_equal(gi[0], fr[0])
                    for c in (1, 2):
                        d = np.abs(gi[c].astype(np.int64) - gf[c - 1].astype(np.int64))
                        worst[depth] = max(worst[depth], int(d.max()))
                        share = max(share, float((d > 0).mean()))
    return worst, share


def test_integer_model_against_float64(capsys):
    """the measurement behind ALLOW_MAX_ABS / ALLOW_SHARE: random, banded and progressive content, the three pairs, three
    depths, an even and an odd size.  `random` through BOTH passes is measured by the next test."""
    worst, share = _measure(("banded", "progressive"), m.PAIRS)
    w2, s2 = _measure(("random",), (("422", "420"), ("444", "422")))
    worst = {d: max(worst[d], w2[d]) for d in DEPTHS}
    share = max(share, s2)
    with capsys.disabled():
        print(f"\nformat resample, integer vs float64: max |diff| by depth {worst}, largest share of differing samples {share:.4f}")
    for d in DEPTHS:
        assert worst[d] <= m.ALLOW_MAX_ABS[d]
    assert share <= m.ALLOW_SHARE


def test_intermediate_saturation_is_the_only_larger_difference(capsys):
    """full-scale noise through both passes: swscale's 15-bit intermediate clips a horizontal overshoot above full scale
    BEFORE the vertical pass, a single-rounding float model clips once at the end - several code values apart.  Give
    the float model the same clip between its passes and the difference is the ordinary one again."""
    plain, _ = _measure(("random",), (("444", "420"),))
    same, share = _measure(("random",), (("444", "420"),), saturate=True)
    with capsys.disabled():
        print(f"\nformat resample, 4:4:4 -> 4:2:0 on noise: max |diff| {plain} without, {same} with the intermediate clip "
              f"in the float model (share {share:.4f})")
    assert max(plain.values()) > max(m.ALLOW_MAX_ABS.values())          # (the effect is there: the test means something)
    for d in DEPTHS:
        assert plain[d] <= m.ALLOW_MAX_ABS_UNSATURATED[d]
        assert same[d] <= m.ALLOW_MAX_ABS[d]
    assert share <= m.ALLOW_SHARE


@pytest.mark.parametrize("depth", DEPTHS)
def test_clamp(depth):
    """rows alternating 0 and full scale (the issue's case) and bars of four (where every positive tap sits on one level and
    the negative lobes on the other, 1.11 x full scale before the clip): the output stays inside the range, reaches both
    ends of it on the bars, and equals the float model's clipped result (clipped between the passes as well, as the
    15-bit intermediate is)"""
    full = (1 << depth) - 1
    for kind in ("rows", "bars"):
        for src, dst in m.PAIRS:
            fr = m.frame(kind, 66, 38, 0, depth, src)
            gi = m.resample_frame(fr, depth, src, dst)
            (sw, sh), (tw, th) = m.SUB[src], m.SUB[dst]
            for c in (1, 2):
                # (the float model with swscale's clip between the passes: the bars overshoot horizontally too)
                gf = m.resample_plane_f64(fr[c], depth, tw > sw, th > sh, saturate=True)
                assert gi[c].min() >= 0 and gi[c].max() <= full
                assert np.abs(gi[c].astype(np.int64) - gf.astype(np.int64)).max() <= m.ALLOW_MAX_ABS[depth]
            if kind == "bars":
                assert gi[1].min() == 0 and gi[1].max() == full
    # the unclipped value does leave the range: the 12-bit vertical row at phase 1/2
    pos, coef, taps = m.sws_bicubic_table(38, 19, 1 << 12, 128, 128)
    row = coef[9]
    assert sum(q for q in row if q > 0) > (1 << 12) and sum(q for q in row if q < 0) < 0


def test_small_planes_are_where_the_filter_is_cut_short():
    """initFilter clamps the tap count to src - 2: from 11 source samples on the nine taps are all there (what the
    drop-in's init() requires of every resampled chroma dimension)"""
    for src in range(11, 40):
        for one, dp in ((1 << 14, 64), (1 << 12, 128)):
            assert 1 + (4 * src + -(-src // 2) - 1) // -(-src // 2) <= src - 2
    assert 1 + (4 * 10 + 5 - 1) // 5 > 10 - 2
