"""CPU: the two models of the format filter's scaler path to fewer chroma samples at a HIGHER depth
(tests/format_deepen_model.py) against the definition - luma, flat planes, the tables' sums - and against each other; the
C ABI's entry point and the settings key for it; and what hb_hip_setup_hw_filters / hb_hip_filter_init_failed
(libhb/hip_common.c) make of a job's list that ends in such a `format=` entry, without a device."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from handbrake_amd import hbrt, hip
import format_deepen_model as m

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KINDS = ("progressive", "banded", "random", "flat", "rows", "bars")
SIZES = ((66, 38), (67, 37), (130, 70))
KEY = "hip-deepen-step"
SYM = "hbhip_format_deepen_create"
YUV422P, YUV444P = hbrt.PIX_FMT[("2x1", 8)], hbrt.PIX_FMT[("1x1", 8)]


# ---- the model ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sd,dd", m.STEPS)
def test_luma_is_a_shift_and_nothing_else(sd, dd):
    """every value of the source depth: v << (dd - sd), no top-bit replication - full scale stays short of full scale"""
    full = (1 << sd) - 1
    ramp = np.arange(1 << sd, dtype=np.uint8 if sd == 8 else np.uint16).reshape(-1, 64)
    fr = (ramp, np.zeros((ramp.shape[0], 32), ramp.dtype), np.zeros((ramp.shape[0], 32), ramp.dtype))
    y = m.deepen_frame(fr, sd, dd, "422", "420")[0]
    assert y.dtype == np.uint16
    np.testing.assert_array_equal(y, ramp.astype(np.uint16) << (dd - sd))
    assert int(y.max()) == full << (dd - sd) < (1 << dd) - 1
    if (sd, dd) == (8, 10):
        assert int(y.max()) == 1020
    for src, dst in m.PAIRS:
        for kind in ("random", "bars"):
            f = m.frame(kind, 67, 37, 0, sd, src)
            np.testing.assert_array_equal(m.deepen_frame(f, sd, dd, src, dst)[0], f[0].astype(np.uint16) << (dd - sd))


@pytest.mark.parametrize("sd,dd", m.STEPS)
@pytest.mark.parametrize("src,dst", m.PAIRS)
def test_flat_chroma_is_shifted_like_luma(sd, dd, src, dst):
    """a flat chroma plane of value v comes out as v << (dd - sd) in every sample, edge rows and columns included: the
    tables sum to one"""
    full = (1 << sd) - 1
    dt = np.uint8 if sd == 8 else np.uint16
    lcw, lch = m.SUB[src]
    for w, h in ((66, 38), (67, 37)):
        cw, ch = -((-w) >> lcw), -((-h) >> lch)
        for value in (0, 1, full // 3, full - 1, full):
            fr = (np.zeros((h, w), dt), np.full((ch, cw), value, dt), np.full((ch, cw), full - value, dt))
            out = m.deepen_frame(fr, sd, dd, src, dst)
            assert int(out[1].min()) == int(out[1].max()) == value << (dd - sd), f"{value} {w}x{h}"
            assert int(out[2].min()) == int(out[2].max()) == (full - value) << (dd - sd), f"{full - value} {w}x{h}"


@pytest.mark.parametrize("one,src_pos,dst_pos", [(1 << 14, 128, 64), (1 << 12, 128, 128)])
def test_tables_sum_to_one(one, src_pos, dst_pos):
    for n in (11, 19, 33, 37, 65, 70):
        _, rows, _ = m.sws_bicubic_table(n, -(-n // 2), one, src_pos, dst_pos)
        assert all(sum(r) == one for r in rows), n


def test_integer_model_against_float64(capsys):
    """the measurement behind ALLOW_CHROMA: the six kinds, the three pairs, the three steps, three sizes, against the
    unrounded float64 form.  Luma is exact."""
    for sd, dd in m.STEPS:
        worst = 0.0
        for src, dst in m.PAIRS:
            for kind in KINDS:
                for w, h in SIZES:
                    fr = m.frame(kind, w, h, 0, sd, src)
                    gi = m.deepen_frame(fr, sd, dd, src, dst)
                    gf = m.deepen_frame_f64(fr, sd, dd, src, dst)
                    for c in range(3):
                        assert gi[c].shape == gf[c].shape and gi[c].dtype == np.uint16
                    assert float(np.abs(gi[0].astype(np.float64) - gf[0]).max()) == 0.0
                    for c in (1, 2):
                        worst = max(worst, float(np.abs(gi[c].astype(np.float64) - gf[c]).max()))
        with capsys.disabled():
            print(f"\nformat deepen {sd} -> {dd}, integer vs float64: luma max 0, chroma max {worst:.4f} "
                  f"(allowed {m.ALLOW_CHROMA[sd, dd]}, ceiling {m.CEILING[sd, dd]:.4f})")
        assert worst <= m.ALLOW_CHROMA[sd, dd] < m.CEILING[sd, dd]
        assert m.CEILING[sd, dd] == 0.5 + (1.25 * 4.8 / 4096 + 1.0 / 32768) * (1 << dd)


# ---- the ABI ------------------------------------------------------------------------------------------------------------
def test_abi_symbol_is_declared_listed_and_exported():
    text = open(os.path.join(ROOT, "include", "hbhip.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    proto = re.search(r"\bint\s+%s\s*\(([^;]*)\)\s*;" % SYM, text)
    assert proto, f"{SYM} is not declared in include/hbhip.h"
    args = [a.strip() for a in proto.group(1).split(",")]
    assert len(args) == 11 and "src_depth" in args[3] and "dst_depth" in args[4] and "chroma_location" in args[9]
    assert SYM in hip.ABI_SYMBOLS
    assert hasattr(hip, "format_deepen_device_filter")
    lib = os.path.join(ROOT, "handbrake_amd", "libhbhip.so")
    if not os.path.exists(lib):
        pytest.fail("handbrake_amd/libhbhip.so is not built")
    assert hasattr(hip.lib(), SYM), f"{SYM} is not exported by libhbhip.so"
    host = open(os.path.join(ROOT, "handbrake_amd", "libhb", "hbhip_host.h")).read()
    assert re.search(r'#define\s+HBHIP_FORMAT_DEEPEN_STEP\s+"%s"' % KEY, host)


# ---- the list -----------------------------------------------------------------------------------------------------------
LAP = "y-strength=0.2:y-kernel=isolap"
VFR = "mode=0:rate=30000/1001"
MARKS = ("hip-planar-step", "hip-up-step", "hip-widen-step", KEY)


@pytest.fixture()
def stubs(built, monkeypatch):
    """CPU `decomb`, `lapsharp`, `vfr` and `format` objects that do nothing (no frame is pushed), registered as their ids' filters"""
    monkeypatch.setenv("HBHIP_FORCE_SWAP", "1")
    hip.filters()
    F = hbrt.FILTER_ID
    keep = {}
    rt = hbrt.runtime()
    for name, shown in (("decomb", "Decomb"), ("lapsharp", "Sharpen (lapsharp)"), ("vfr", "Framerate Shaper"), ("format", "Format")):
        addr, keep[name] = hbrt.filter_stub(F[name], shown)
        rt.hbhip_rt_register_filter(F[name], addr)
    yield F
    for name in keep:
        rt.hbhip_rt_register_filter(F[name], None)


@pytest.mark.parametrize("pix_fmt,target", [(YUV422P, "yuv420p10le"), (YUV444P, "yuv420p10le"), (YUV444P, "yuv422p10le"),
                                            (YUV422P, "yuv420p12le"), (hbrt.PIX_FMT[("1x1", 10)], "yuv422p12le")])
def test_list_is_marked_and_bracketed_before_any_init(stubs, pix_fmt, target):
    jl = hbrt.JobList([(stubs["lapsharp"], LAP), (stubs["format"], f"format={target}")], 66, 38, pix_fmt)
    try:
        assert [n for n, _ in jl.entries()] == ["Sharpen (lapsharp)", "Format"]
        got = jl.setup()
        assert len(got) == 4 and "HIP" in got[1][0] and "harp" in got[1][0]
        assert [got[0][0], got[2][0], got[3][0]] == ["HIP upload adapter", "Format (HIP)", "HIP download adapter"]
        assert got[0][1] == {}
        assert got[2][1] == {"format": target, KEY: "1"}               # the entry keeps its own setting beside the mark
        assert got[3][1] == {}                                         # a planar target: nothing for the adapter to repack
    finally:
        jl.close()


def test_marked_behind_a_transparent_filter(stubs):
    """the list is kept in the order of the ids: decomb (6), the frame-rate shaper (11), format (33)"""
    jl = hbrt.JobList([(stubs["decomb"], "mode=7"), (stubs["vfr"], VFR), (stubs["format"], "format=yuv420p10le")], 66, 38, YUV422P)
    try:
        got = jl.setup()
        assert len(got) == 5 and "HIP" in got[1][0]
        assert [n for n, _ in got][0::2] == ["HIP upload adapter", "Framerate Shaper", "HIP download adapter"]
        assert got[3] == ("Format (HIP)", {"format": "yuv420p10le", KEY: "1"})
    finally:
        jl.close()


def test_what_is_not_marked(stubs):
    """a lone entry (only a transparent filter in front), an equal or lower depth, more chroma samples in a dimension, a
    9-bit target, a semi-planar one"""
    lap = (stubs["lapsharp"], LAP)
    for pix_fmt, filters in ((YUV422P, [(stubs["vfr"], VFR), (stubs["format"], "format=yuv420p10le")]),
                             (YUV422P, [(stubs["format"], "format=yuv420p10le")]),
                             (YUV422P, [lap, (stubs["format"], "format=yuv420p")]),
                             (hbrt.PIX_FMT[("2x1", 10)], [lap, (stubs["format"], "format=yuv420p10le")]),
                             (hbrt.PIX_FMT[("2x1", 12)], [lap, (stubs["format"], "format=yuv420p10le")]),
                             (YUV422P, [lap, (stubs["format"], "format=yuv422p10le")]),
                             (YUV422P, [lap, (stubs["format"], "format=yuv420p9le")]),
                             (YUV422P, [lap, (stubs["format"], "format=p010le")])):
        jl = hbrt.JobList(filters, 66, 38, pix_fmt)
        try:
            for name, settings in jl.setup():
                assert KEY not in settings, (pix_fmt, name, settings)
        finally:
            jl.close()
    # 4:2:2 -> 4:4:4 at a higher depth is the UP step's, 4:4:0-like mixes (one dimension gains) are nobody's
    jl = hbrt.JobList([lap, (stubs["format"], "format=yuv444p10le")], 66, 38, YUV422P)
    try:
        assert jl.setup()[2][1] == {"format": "yuv444p10le", "hip-up-step": "1"}
    finally:
        jl.close()


def test_a_failed_init_in_front_takes_the_mark_away(stubs):
    """hb_hip_filter_init_failed on the drop-in the entry stood behind: the CPU filter comes back, what follows is marked
    afresh - and a `format` entry with no drop-in in front of it is not"""
    jl = hbrt.JobList([(stubs["lapsharp"], LAP), (stubs["format"], "format=yuv420p10le")], 66, 38, YUV422P)
    try:
        got = jl.setup()
        assert got[2][1] == {"format": "yuv420p10le", KEY: "1"}
        assert hip.filters().hb_hip_filter_init_failed(C.byref(jl.job), 1, C.byref(jl.init)) > 0
        got = jl.entries()
        assert [n for n, _ in got][-2:] == ["Sharpen (lapsharp)", "Format (HIP)"], got
        assert "HIP download adapter" not in [n for n, _ in got]
        assert got[-1][1] == {"format": "yuv420p10le"}
    finally:
        jl.close()


@pytest.mark.skipif(__import__("torch").cuda.is_available(), reason="needs a box WITHOUT a GPU: every drop-in init must fail")
@pytest.mark.parametrize("with_vfr", [False, True])
def test_after_the_fallbacks_the_cpu_filters_hold_their_own_settings(stubs, with_vfr):
    mid = [(stubs["vfr"], VFR)] if with_vfr else []
    jl = hbrt.JobList([(stubs["lapsharp"], LAP)] + mid + [(stubs["format"], "format=yuv420p10le")], 66, 38, YUV422P)
    try:
        jl.setup()
        got = jl.init_all()
        assert [n for n, _ in got] == ["Framerate Shaper"] * with_vfr + ["Sharpen (lapsharp)", "Format"]   # no adapter left
        assert got[-2][1] == dict(kv.split("=") for kv in LAP.split(":"))
        assert got[-1][1] == {"format": "yuv420p10le"}                 # exactly that: no internal key
        for _, settings in got:
            assert not any(k in settings for k in MARKS)
    finally:
        jl.close()
