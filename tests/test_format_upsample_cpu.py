"""CPU: the two models of the format filter's chroma up-sampling (tests/format_upsample_model.py) against the definition
- coefficient sums, flat planes, siting by position, luma's plain shift - and against each other; the ABI symbol."""
import os
import re

import numpy as np
import pytest

import format_upsample_model as m

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIZES = (7, 8, 9, 10, 17, 19, 33, 34, 37, 38, 66, 67, 70, 130, 540, 541, 960, 961, 1080)
SHAPES = ((66, 38), (67, 37))


def _dt(depth):
    return np.uint8 if depth == 8 else np.uint16


@pytest.mark.parametrize("one,src_pos", [(1 << 14, 64), (1 << 12, 128)])
def test_every_coefficient_row_sums_to_one(one, src_pos):
    """14-bit horizontal (left-sited: source position 64) and 12-bit vertical (centred: 128) tables, targets of 2 s and
    2 s - 1 samples from the smallest plane the filter takes: every row sums to exactly `one`, has four taps, and lies
    inside the window the kernel's nominal frame gives it - six samples from 2 * (i >> 2) - 2 on, the non-zero taps in
    (i >> 1) - 1 .. (i >> 1) + 2 horizontally and (i >> 1) - 2 .. (i >> 1) + 2 vertically"""
    lo = -1 if src_pos == 64 else -2
    for src in SIZES:
        for dst in (2 * src, 2 * src - 1):
            pos, coef, taps = m.sws_bicubic_table(src, dst, one, src_pos, 128)
            assert taps == 4 and len(coef) == dst
            for i, row in enumerate(coef):
                assert sum(row) == one, f"src {src} dst {dst} row {i}: {row}"
                assert 0 <= pos[i] and pos[i] + taps <= src
                used = [pos[i] + t for t in range(taps) if row[t]]
                assert (i >> 1) + lo <= min(used) and max(used) <= (i >> 1) + 2, f"src {src} dst {dst} row {i}"
                assert 2 * (i >> 2) - 2 <= min(used) and max(used) <= 2 * (i >> 2) + 3


def test_interior_rows_are_what_the_definition_gives():
    """even columns are copies, odd columns the half-sample row; rows alternate the quarter-sample row and its mirror;
    the largest absolute row sums (what the 15-bit intermediate and the clips have to hold)"""
    pos, coef, _ = m.sws_bicubic_table(960, 1920, 1 << 14, 64, 128)
    assert coef[100] == [0, 16384, 0, 0] and coef[101] == [-1229, 9421, 9421, -1229]
    assert pos[100] + 1 == 50 and pos[101] + 1 == 50
    assert max(sum(abs(q) for q in row) for row in coef) == 21300
    pos, coef, _ = m.sws_bicubic_table(540, 1080, 1 << 12, 128, 128)
    assert coef[101] == [-346, 3572, 985, -115] and coef[100] == [-115, 985, 3572, -346]
    assert pos[101] + 1 == 50 and pos[100] + 2 == 50
    assert max(sum(abs(q) for q in row) for row in coef) == 5018
    # an odd target walks through every phase: the largest sum of all sizes, 1.3 x
    coef = m.sws_bicubic_table(541, 1081, 1 << 12, 128, 128)[1]
    assert max(sum(abs(q) for q in row) for row in coef) == 5326
    for src in SIZES:
        for dst in (2 * src, 2 * src - 1):
            assert max(sum(abs(q) for q in row) for row in m.sws_bicubic_table(src, dst, 1 << 14, 64, 128)[1]) <= 21300
            assert max(sum(abs(q) for q in row) for row in m.sws_bicubic_table(src, dst, 1 << 12, 128, 128)[1]) <= 5326


@pytest.mark.parametrize("sd,dd", m.STEPS)
@pytest.mark.parametrize("src,dst", m.PAIRS)
def test_flat_plane_stays_flat(sd, dd, src, dst):
    full = (1 << sd) - 1
    for value in (0, 1, full // 2, full - 1, full):
        for w, h in SHAPES:
            cw, ch = m.chroma_size(w, h, src)
            fr = (np.full((h, w), value, _dt(sd)), np.full((ch, cw), value, _dt(sd)), np.full((ch, cw), value, _dt(sd)))
            out = m.upsample_frame(fr, sd, dd, src, dst)
            f64 = m.upsample_frame_f64(fr, sd, dd, src, dst)
            dcw, dch = m.chroma_size(w, h, dst)
            assert out[0].shape == (h, w) and out[1].shape == out[2].shape == (dch, dcw)
            for c in range(3):
                assert out[c].dtype == _dt(dd)
                assert out[c].min() == out[c].max() == value << (dd - sd), f"{value} plane {c}"
                assert f64[c].min() == f64[c].max() == value << (dd - sd)


@pytest.mark.parametrize("sd,dd", m.STEPS)
def test_siting_on_ramps(sd, dd):
    """an even interior target column IS its source column (the one tap of 1 << 14); a ramp down the rows comes out a
    quarter above source row j at target row 2j and a quarter below it at 2j + 1"""
    a, b = 3 << (sd - 8), 4 << (sd - 8)
    h, w = 20, 32
    x = np.arange(w)[None, :].repeat(h, axis=0)
    y = np.arange(h)[:, None].repeat(w, axis=1)
    k = 1 << (dd - sd)
    for model in (m.scale_plane, m.scale_plane_f64):
        ramp = (a + b * x).astype(_dt(sd))
        hr = model(ramp, sd, dd, 2 * w, h).astype(np.int64)
        assert np.array_equal(hr[:, 4:-4:2], ramp.astype(np.int64)[:, 2:-2] * k)
        assert np.abs(hr[:, 5:-4:2] - (a + b * (np.arange(2, w - 2) + 0.5))[None, :] * k).max() <= 1
        vr = model((a + b * y).astype(_dt(sd)), sd, dd, w, 2 * h).astype(np.float64)
        rows = np.arange(2, h - 2)
        assert np.abs(vr[4:-4:2] - ((a + b * (rows - 0.25)) * k)[:, None]).max() <= 1
        assert np.abs(vr[5:-4:2] - ((a + b * (rows + 0.25)) * k)[:, None]).max() <= 1
        both = model(ramp, sd, dd, 2 * w, 2 * h).astype(np.int64)
        assert both.shape == (2 * h, 2 * w)
        assert np.abs(both[4:-4, 4:-4:2] - ramp.astype(np.int64)[:1, 2:-2] * k).max() <= 1


@pytest.mark.parametrize("sd,dd", m.STEPS)
def test_luma_is_a_plain_shift(sd, dd):
    """the identity filters and the output stage: v << (dd - sd) for every v, whatever the range"""
    v = np.arange(1 << sd, dtype=_dt(sd)).reshape(-1, 64)
    for src, dst in m.PAIRS:
        cw, ch = m.chroma_size(v.shape[1], v.shape[0], src)
        fr = (v, np.zeros((ch, cw), _dt(sd)), np.zeros((ch, cw), _dt(sd)))
        out = m.upsample_frame(fr, sd, dd, src, dst)
        assert out[0].dtype == _dt(dd)
        assert np.array_equal(out[0].astype(np.int64), v.astype(np.int64) << (dd - sd))


def test_luma_8_to_10_is_not_the_unscaled_full_range_copy():
    """format_kernel's full-range luma replicates the top bits, (v << 2) | (v >> 6): 255 -> 1023.  The scaler does not:
    255 -> 1020, in both ranges."""
    v = np.arange(256, dtype=np.uint8).reshape(4, 64)
    fr = (v, np.zeros((2, 32), np.uint8), np.zeros((2, 32), np.uint8))
    got = m.upsample_frame(fr, 8, 10, "420", "422")[0].astype(np.int64)
    replicated = (v.astype(np.int64) << 2) | (v.astype(np.int64) >> 6)
    assert int(got.max()) == 1020 and int(replicated.max()) == 1023
    assert int((got != replicated).sum()) == 256 - 64                          # v >> 6 is 0 for the first 64 values only


def _measure(kinds, pairs, saturate, edge=m.EDGE):
    """edge: the target samples left out along each border of a plane in a direction that is up-sampled (0: none)"""
    worst = {step: 0 for step in m.STEPS}
    share = 0.0
    for kind in kinds:
        for sd, dd in m.STEPS:
            for src, dst in pairs:
                for w, h in SHAPES:
                    fr = m.frame(kind, w, h, 0, sd, src)
                    gi = m.upsample_frame(fr, sd, dd, src, dst)
                    gf = m.upsample_frame_f64(fr, sd, dd, src, dst, saturate=saturate)
                    assert np.array_equal(gi[0], gf[0])
                    for c in (1, 2):
                        d = np.abs(gi[c].astype(np.int64) - gf[c].astype(np.int64))
                        if edge and m.SUB[dst][0] < m.SUB[src][0]:
                            d = d[:, edge:-edge]
                        if edge and m.SUB[dst][1] < m.SUB[src][1]:
                            d = d[edge:-edge]
                        worst[(sd, dd)] = max(worst[(sd, dd)], int(d.max()))
                        share = max(share, float((d > 0).mean()))
    return worst, share


def test_integer_model_against_float64(capsys):
    """the measurement behind ALLOW_MAX_ABS / ALLOW_SHARE: random, progressive and bars, the three pairs, the six depth
    pairs, an even and an odd size.  The float model clips its intermediate where the 15-bit one saturates; that changes
    nothing for a single pass or on `progressive` (32767 / 128 is above every 8-bit value, the output clip does the
    same), only for full-scale content through BOTH passes, which the next test takes apart.  The recorded figures are
    the measured ones: equalities, not bounds."""
    kinds = ("random", "progressive", "bars")
    worst, share = _measure(kinds, m.PAIRS, True)
    whole, whole_share = _measure(kinds, m.PAIRS, True, edge=0)
    with capsys.disabled():
        print(f"\nformat upsample, integer vs float64: max |diff| by step {worst}, largest share of differing samples {share:.4f}"
              f"; with the {m.EDGE} border samples {whole}, share {whole_share:.4f}")
    assert worst == m.ALLOW_MAX_ABS
    assert round(share, 4) == m.ALLOW_SHARE
    assert whole == m.ALLOW_MAX_ABS_EDGE


def test_the_border_is_initfilters_truncated_division():
    """what ALLOW_MAX_ABS_EDGE is made of: target row 2 of a 19 -> 38 table lies at source row 0.75 and the cubic's four
    taps there are rows -1 .. 2, the first folded onto row 0.  initFilter's first tap is (x - 3 * 65536) / 131072 in C's
    division, which truncates TOWARDS ZERO: for the negative numerators of the first rows that is one row further down
    than the floor, the tap at distance 1.75 is never computed, and the three that are left are normalised to 4096"""
    pos, coef, taps = m.sws_bicubic_table(19, 38, 1 << 12, 128, 128)
    k = m.keys_cubic(np.array([1.75, 0.75, 0.25, 1.25]))
    folded = np.array([k[0] + k[1], k[2], k[3]])
    assert pos[2] == 0 and coef[2][3] == 0
    assert np.abs(np.array(coef[2][:3]) / 4096 - folded).max() > 0.02         # not the cubic with its edge replicated ...
    three = np.array([k[1], k[2], k[3]]) / (k[1] + k[2] + k[3])
    assert np.abs(np.array(coef[2][:3]) / 4096 - three).max() < 1e-3           # ... but three of its taps, normalised
    assert pos[6] == 1 and np.abs(np.array(coef[6]) / 4096 - m.keys_cubic(np.array([1.75, 0.75, 0.25, 1.25]))).max() < 1e-3


def test_intermediate_saturation_is_the_only_larger_difference(capsys):
    """full-scale noise and bars through both passes: the half-sample column (-1229 9421 9421 -1229) / 16384 overshoots
    full scale by up to 15 %, swscale's 15-bit intermediate clips that BEFORE the vertical pass, a single-rounding float
    model clips once at the end.  Give the float model the same clip between its passes and the difference is the
    ordinary one again."""
    plain, _ = _measure(("random", "bars"), (("420", "444"),), False)
    same, share = _measure(("random", "bars"), (("420", "444"),), True)
    with capsys.disabled():
        print(f"\nformat upsample, 4:2:0 -> 4:4:4 on noise and bars: max |diff| {plain} without, {same} with the intermediate "
              f"clip in the float model (share {share:.4f})")
    assert plain == m.ALLOW_MAX_ABS_UNSATURATED
    for step in m.STEPS:
        assert plain[step] > m.ALLOW_MAX_ABS[step]                             # (the effect is there: the test means something)
        assert same[step] <= m.ALLOW_MAX_ABS[step]
    assert round(share, 4) <= m.ALLOW_SHARE
    # and a single pass does not show it: the saturated intermediate is above full scale, the output clip takes both there
    one_pass, _ = _measure(("random", "bars"), (("422", "444"), ("420", "422")), False)
    for step in m.STEPS:
        assert one_pass[step] <= m.ALLOW_MAX_ABS[step]


@pytest.mark.parametrize("sd,dd", m.STEPS)
def test_clips(sd, dd):
    """rows alternating 0 and full scale and bars of four: the output stays inside the target's range and reaches both
    ends of it; full-scale flat chroma stays full scale (<< only: full << (dd - sd), not the target's full scale)"""
    full = (1 << dd) - 1
    for kind in ("rows", "bars", "flat"):
        for src, dst in m.PAIRS:
            fr = m.frame(kind, 66, 38, 0, sd, src)
            gi = m.upsample_frame(fr, sd, dd, src, dst)
            for c in (1, 2):
                assert gi[c].min() >= 0 and gi[c].max() <= full
            if kind == "bars":
                assert gi[1].min() == 0 and gi[1].max() == full               # (the overshoot reaches the TARGET's top)
            if kind == "flat":
                assert gi[1].min() == gi[1].max() == ((1 << sd) - 1) << (dd - sd)


def test_small_planes_are_where_the_filter_is_cut_short():
    """initFilter clamps the tap count to src - 2: from 7 source samples on the 1 + 4 taps are all there (what the create
    function requires of every up-sampled chroma dimension).  What the model's table is at 6 is not looked at."""
    assert m.MIN_SAMPLES == 7
    for src in range(m.MIN_SAMPLES, 40):
        assert min(1 + 4, src - 2) == 5
    assert min(1 + 4, (m.MIN_SAMPLES - 1) - 2) < 5


def test_abi_symbol_is_declared_and_exported():
    from handbrake_amd import hip
    text = open(os.path.join(ROOT, "include", "hbhip.h")).read()
    proto = re.search(r"int\s+hbhip_format_upsample_create\s*\(([^;]*)\)\s*;", text)
    assert proto, "hbhip_format_upsample_create is not declared in include/hbhip.h"
    args = [a.strip() for a in proto.group(1).split(",")]
    assert len(args) == 11 and "src_depth" in args[3] and "dst_depth" in args[4] and "chroma_location" in args[9]
    assert "hbhip_format_upsample_create" in hip.ABI_SYMBOLS
    assert hasattr(hip, "format_upsample_device_filter")
    lib = os.path.join(ROOT, "handbrake_amd", "libhbhip.so")
    if not os.path.exists(lib):
        pytest.fail("handbrake_amd/libhbhip.so is not built")
    import ctypes
    assert hasattr(ctypes.CDLL(lib), "hbhip_format_upsample_create")
    host = open(os.path.join(ROOT, "handbrake_amd", "libhb", "hbhip_host.h")).read()
    assert re.search(r'#define\s+HBHIP_FORMAT_UP_STEP\s+"hip-up-step"', host)
