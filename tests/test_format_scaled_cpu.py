"""CPU: the two models of the format filter's scaler path at a lower depth (tests/format_scaled_model.py) against the
definition - the dither table, flat planes, Cr's offset - against each other, and against format_resample_model where
the depth stays; and the C ABI's entry point for it."""
import os
import re

import numpy as np
import pytest

import format_resample_model as rm
import format_scaled_model as m

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KINDS = ("progressive", "banded", "random", "flat", "rows", "bars")
SIZES = ((66, 38), (67, 37), (130, 70))


def test_dither_table_is_a_permutation_of_the_even_numbers():
    t = m.DITHER_8X8_128
    assert t.shape == (8, 8)
    assert sorted(t.ravel().tolist()) == list(range(0, 128, 2))
    for r in range(4):
        assert not np.array_equal(t[r], t[r + 4]), f"rows {r} and {r + 4}"
    assert int(t.sum()) == 64 * 63                 # mean 63 / 128: what keeps a flat plane's mean (next test)


@pytest.mark.parametrize("sd,dd", m.STEPS)
@pytest.mark.parametrize("src,dst", m.PAIRS)
def test_flat_plane_keeps_its_mean_and_its_ends(sd, dd, src, dst):
    """a flat plane: every aligned 8 x 8 cell of every output plane has the exact mean to within 1 / 128 code value (to 8
    bits: the dither's 64 thresholds; to 10 bits: the flat half, 12 -> 10 only rounds), full scale maps to full scale and
    0 to 0 in every sample"""
    full_s, full_d = (1 << sd) - 1, (1 << dd) - 1
    h, w = 64, 96                                    # 4:2:0 planes of 32 x 48: whole cells, edge cells included
    for value in (0, 1, 514 << (sd - 10), full_s // 3, full_s - 1, full_s):
        lcw, lch = m.SUB[src]
        fr = (np.full((h, w), value, np.uint16),) + (np.full((h >> lch, w >> lcw), value, np.uint16),) * 2
        out = m.scaled_frame(fr, sd, dd, src, dst)
        exact = min(value / (1 << (sd - dd)), full_d)
        for c, p in enumerate(out):
            assert p.dtype == (np.uint8 if dd == 8 else np.uint16)
            if value in (0, full_s):
                assert p.min() == p.max() == (0 if value == 0 else full_d), f"{value} plane {c}"
                continue
            cells = p.reshape(p.shape[0] // 8, 8, p.shape[1] // 8, 8).astype(np.float64).mean(axis=(1, 3))
            if dd == 8:
                assert np.abs(cells - exact).max() <= 1 / 128 + 1e-9, f"{value} plane {c}: {cells.min()} .. {cells.max()}"
            else:
                assert p.min() == p.max() == int(np.floor(exact + 0.5)), f"{value} plane {c}"


def test_flat_514_becomes_128_and_129():
    fr = (np.full((38, 66), 514, np.uint16), np.full((38, 33), 514, np.uint16), np.full((38, 33), 514, np.uint16))
    for p in m.scaled_frame(fr, 10, 8, "422", "420"):
        assert sorted(np.unique(p).tolist()) == [128, 129]
        assert p[:16, :16].mean() == 128.5


@pytest.mark.parametrize("sd", (10, 12))
@pytest.mark.parametrize("src,dst", m.PAIRS)
def test_cr_pattern_is_cbs_moved_three_columns(sd, src, dst):
    """identical Cb and Cr planes: Cr reads the dither table three columns on, so Cr's output at column x is Cb's at
    x + 3 wherever the content under both is the same - a flat plane, and columns of a picture that varies by row only"""
    h, w = 70, 130
    lcw, lch = m.SUB[src]
    ch, cw = -(-h >> lch), -(-w >> lcw)
    ramp = ((np.arange(ch) * 37 + 11) % (1 << sd)).astype(np.uint16)[:, None].repeat(cw, axis=1)
    for chroma in (np.full((ch, cw), (1 << sd) // 3, np.uint16), ramp):
        y, cb, cr = m.scaled_frame((np.zeros((h, w), np.uint16), chroma, chroma), sd, 8, src, dst)
        np.testing.assert_array_equal(cr[:, :-3], cb[:, 3:])
        assert not np.array_equal(cr, cb)
    # and on any content Cr equals Cb computed with the offset: nothing else tells the planes apart
    fr = m.frame("random", w, h, 0, sd, src)
    (sw, sh), (tw, th) = m.SUB[src], m.SUB[dst]
    np.testing.assert_array_equal(m.scaled_frame((fr[0], fr[1], fr[1]), sd, 8, src, dst)[2],
                                  m.scaled_plane(fr[1], sd, 8, tw > sw, th > sh, m.CR_OFFSET))


def test_depth_only_differs_from_the_unscaled_copy_in_cr():
    """libswscale's dither matrices nest: ff_dither_8x8_128 >> 5 is the unscaled copy's 2 x 2 matrix {1, 2; 3, 0}, so at
    10 -> 8 with the subsampling unchanged Y and Cb come out as format_kernel's DITHER_COPY gives them - and Cr, read
    three columns on, does not.  That plane is what tells `yuv420p10le -> nv12` from 10 -> 8 followed by an interleave."""
    assert np.array_equal(m.DITHER_8X8_128[:2, :2] >> 5, [[1, 2], [3, 0]])
    assert np.array_equal(m.DITHER_8X8_128 >> 5, np.tile([[1, 2], [3, 0]], (4, 4)))
    fr = m.frame("random", 66, 38, 0, 10, "420")     # (the synthetic pictures are 8-bit ones shifted up: nothing to dither)
    got = m.scaled_frame(fr, 10, 8, "420", "420")

    def unscaled(p):
        d2 = np.array([[1, 2], [3, 0]])[(np.arange(p.shape[0]) & 1)[:, None], (np.arange(p.shape[1]) & 1)[None, :]]
        t = (p.astype(np.int64) + d2) >> 2
        return t - (t >> 8)
    assert np.array_equal(got[0], unscaled(fr[0])) and np.array_equal(got[1], unscaled(fr[1]))
    assert not np.array_equal(got[2], unscaled(fr[2]))
    assert np.abs(got[2].astype(np.int64) - unscaled(fr[2])).max() == 1


def test_integer_model_against_float64(capsys):
    """the measurement behind ALLOW_LUMA / ALLOW_CHROMA / ALLOW_SHARE: the six kinds, the four pairs, the three steps,
    three sizes, against the unrounded float64 form"""
    for sd, dd in m.STEPS:
        worst = [0.0, 0.0]
        share = [0.0, 0.0]
        for src, dst in m.PAIRS:
            for kind in KINDS:
                for w, h in SIZES:
                    fr = m.frame(kind, w, h, 0, sd, src)
                    gi = m.scaled_frame(fr, sd, dd, src, dst)
                    gf = m.scaled_frame_f64(fr, sd, dd, src, dst)
                    for c in range(3):
                        assert gi[c].shape == gf[c].shape
                        d = np.abs(gi[c].astype(np.float64) - gf[c])
                        worst[c > 0] = max(worst[c > 0], float(d.max()))
                        share[c > 0] = max(share[c > 0], float((d > 0.5).mean()))
        with capsys.disabled():
            print(f"\nformat scaled {sd} -> {dd}, integer vs float64: luma max {worst[0]:.4f} share {share[0]:.4f}, "
                  f"chroma max {worst[1]:.4f} share {share[1]:.4f}")
        assert worst[0] <= m.ALLOW_LUMA[sd, dd]
        assert worst[1] <= m.ALLOW_CHROMA[sd, dd] < m.CEILING[sd, dd]
        assert max(share) <= m.ALLOW_SHARE
        if dd == 10:
            assert share[0] == 0.0                      # luma 12 -> 10 is a plain rounding


@pytest.mark.parametrize("depth", (8, 10, 12))
@pytest.mark.parametrize("src,dst", rm.PAIRS)
def test_equal_depth_is_the_resample_model(depth, src, dst):
    """sd == dd: the two definitions are one"""
    for kind in ("random", "bars"):
        fr = rm.frame(kind, 67, 37, 1, depth, src)
        got, want = m.scaled_frame(fr, depth, depth, src, dst), rm.resample_frame(fr, depth, src, dst)
        for c in range(3):
            np.testing.assert_array_equal(got[c], want[c])


@pytest.mark.parametrize("sd,dd", m.STEPS)
def test_chroma_passes_are_the_resample_models_up_to_the_output_stage(sd, dd):
    """with a zero dither / the flat half the scaled chroma is the equal-depth model's accumulator shifted further: the
    tables, the siting and the 15-bit intermediate are shared, only the output stage is new"""
    fr = rm.frame("random", 67, 37, 0, sd, "444")
    want = rm.resample_frame(fr, sd, "444", "420")[1].astype(np.int64)
    got = m.scaled_plane(fr[1], sd, dd, True, True, 0).astype(np.int64)
    assert np.abs(got - want / (1 << (sd - dd))).max() <= 1.0 + 1e-9


def test_abi_symbol_is_declared_and_exported():
    from handbrake_amd import hip
    text = open(os.path.join(ROOT, "include", "hbhip.h")).read()
    proto = re.search(r"int\s+hbhip_format_scaled_create\s*\(([^;]*)\)\s*;", text)
    assert proto, "hbhip_format_scaled_create is not declared in include/hbhip.h"
    args = [a.strip() for a in proto.group(1).split(",")]
    assert len(args) == 11 and "src_depth" in args[3] and "dst_depth" in args[4]
    assert "hbhip_format_scaled_create" in hip.ABI_SYMBOLS
    assert hasattr(hip, "format_scaled_device_filter")
    lib = os.path.join(ROOT, "handbrake_amd", "libhbhip.so")
    if not os.path.exists(lib):
        pytest.fail("handbrake_amd/libhbhip.so is not built")
    import ctypes
    assert hasattr(ctypes.CDLL(lib), "hbhip_format_scaled_create")
