"""CPU: `format=p010le` behind an 8-bit 4:2:0 run without a device - the numpy definition (tests/p010_widen_model.py), the
new entry points of include/hbhip.h, and what hb_hip_setup_hw_filters / hb_hip_filter_init_failed (libhb/hip_common.c) make
of a job's list: the mark and the bracket before any init(), and the CPU filters with their own settings after every
drop-in has declined (HBHIP_FORCE_SWAP=1: no device, every init() fails)."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from handbrake_amd import hbrt, hip
import p010_widen_model as pw

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ERR_ARG = -3
NV12, YUV422P = hbrt.AV_PIX_FMT_NV12, hbrt.PIX_FMT[("2x1", 8)]
KEY = "hip-widen-step"
NEW = ["hbhip_frame_download_widen", "hbhip_frame_download_widen_async",
       "hbhip_frame_export_surface_widen", "hbhip_frame_export_surface_widen_async"]


# ---- the model ----------------------------------------------------------------------------------------------------------
def test_every_word_is_the_byte_twice():
    t = np.arange(256, dtype=np.uint8).reshape(16, 16)
    w = pw.widen(t)
    assert w.dtype == np.uint16
    np.testing.assert_array_equal(w >> 8, t)                         # the high byte is the sample ...
    np.testing.assert_array_equal(w & 0xFF, t)                       # ... and so is the low one: not t << 8
    assert w[0, 0] == 0 and w[15, 15] == 65535
    assert (w & 0x3F).any()                                          # P010's six spare bits are not zero
    np.testing.assert_array_equal(w, t.astype(np.uint32) * 257)


@pytest.mark.parametrize("w,h", [(2, 2), (3, 3), (18, 2), (33, 7), (66, 38)])
def test_chroma_geometry_rounds_up(w, h):
    rng = np.random.default_rng(w * 100 + h)
    ch, cw = pw.chroma_shape(w, h)
    assert (ch, cw) == (-(-h // 2), -(-w // 2))
    x = (rng.integers(0, 256, (h, w), dtype=np.uint8), rng.integers(0, 256, (ch, cw), dtype=np.uint8),
         rng.integers(0, 256, (ch, cw), dtype=np.uint8))
    y, c = pw.merge(x)
    assert y.shape == (h, w) and c.shape == (ch, 2 * cw)
    np.testing.assert_array_equal(c[:, 0::2] >> 8, x[1])             # Cb first, the last pair of an odd width included
    np.testing.assert_array_equal(c[:, 1::2] >> 8, x[2])
    np.testing.assert_array_equal(c[:, -2:], np.stack([pw.widen(x[1][:, -1]), pw.widen(x[2][:, -1])], axis=1))
    # placed into a block of bytes: little endian, the samples' bytes only
    pitch, offset = (2 * w + 10, 4 * cw + 6), (5, 5 + (2 * w + 10) * h + 3)
    buf = np.full(offset[1] + pitch[1] * ch + 7, 0xA5, dtype=np.uint8)
    pw.place(buf, offset, pitch, x)
    assert buf[offset[0]] == buf[offset[0] + 1] == x[0][0, 0]
    assert buf[offset[1] + 2] == buf[offset[1] + 3] == x[2][0, 0]
    assert int((buf != 0xA5).sum()) <= 2 * w * h + 4 * cw * ch
    assert (buf[:offset[0]] == 0xA5).all() and (buf[offset[0] + 2 * w:offset[0] + pitch[0]] == 0xA5).all()


# ---- the ABI ------------------------------------------------------------------------------------------------------------
def test_new_symbols_are_declared_exported_and_bound():
    text = open(os.path.join(ROOT, "include", "hbhip.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    for sym in NEW:
        assert re.search(r"\bint\s+%s\s*\(" % sym, text), f"{sym} is not declared in include/hbhip.h"
        assert sym in hip.ABI_SYMBOLS
    path = os.path.join(ROOT, "handbrake_amd", "libhbhip.so")
    if not os.path.exists(path):
        pytest.fail("handbrake_amd/libhbhip.so is not built")
    L = hip.lib()
    for sym in NEW:
        assert hasattr(L, sym), f"{sym} is not exported by libhbhip.so"
    tok = C.c_void_p()
    assert L.hbhip_frame_download_widen(None, None) == ERR_ARG
    assert L.hbhip_frame_export_surface_widen(None, None) == ERR_ARG
    assert L.hbhip_frame_download_widen_async(None, None, C.byref(tok)) == ERR_ARG and not tok.value
    assert L.hbhip_frame_export_surface_widen_async(None, None, C.byref(tok)) == ERR_ARG and not tok.value
    host = open(os.path.join(ROOT, "handbrake_amd", "libhb", "hbhip_host.h")).read()
    assert re.search(r'#define\s+HBHIP_FORMAT_WIDEN_STEP\s+"%s"' % KEY, host)


# ---- the list -----------------------------------------------------------------------------------------------------------
LAP = "y-strength=0.2:y-kernel=isolap"


@pytest.fixture()
def stubs(built, monkeypatch):
    """CPU `lapsharp` and `format` objects that do nothing (no frame is pushed), registered as their ids' filters"""
    monkeypatch.setenv("HBHIP_FORCE_SWAP", "1")
    hip.filters()
    F = hbrt.FILTER_ID
    keep = {}
    rt = hbrt.runtime()
    for name, shown in (("lapsharp", "Sharpen (lapsharp)"), ("format", "Format")):
        addr, keep[name] = hbrt.filter_stub(F[name], shown)
        rt.hbhip_rt_register_filter(F[name], addr)
    yield F
    for name in keep:
        rt.hbhip_rt_register_filter(F[name], None)


def _names(entries):
    return [n for n, _ in entries]


@pytest.mark.parametrize("pix_fmt", [hbrt.AV_PIX_FMT_YUV420P, NV12])
def test_list_is_marked_and_bracketed_before_any_init(stubs, pix_fmt):
    jl = hbrt.JobList([(stubs["lapsharp"], LAP), (stubs["format"], "format=p010le")], 66, 38, pix_fmt)
    try:
        assert _names(jl.entries()) == ["Sharpen (lapsharp)", "Format"]
        got = jl.setup()
        assert len(got) == 4 and "HIP" in got[1][0] and "harp" in got[1][0]
        assert [got[0][0], got[2][0], got[3][0]] == ["HIP upload adapter", "Format (HIP)", "HIP download adapter"]
        assert got[0][1] == {}
        assert got[2][1] == {"format": "p010le", KEY: "1"}           # the entry keeps its own setting beside the mark
        assert got[3][1] == {"format": "p010le", KEY: "1"}
    finally:
        jl.close()


@pytest.mark.skipif(__import__("torch").cuda.is_available(), reason="needs a box WITHOUT a GPU: every drop-in init must fail")
@pytest.mark.parametrize("pix_fmt", [hbrt.AV_PIX_FMT_YUV420P, NV12])
def test_after_the_fallbacks_the_cpu_filters_hold_their_own_settings(stubs, pix_fmt):
    jl = hbrt.JobList([(stubs["lapsharp"], LAP), (stubs["format"], "format=p010le")], 66, 38, pix_fmt)
    try:
        jl.setup()
        got = jl.init_all()
        assert _names(got) == ["Sharpen (lapsharp)", "Format"]       # no adapter left, nothing dropped
        assert got[0][1] == dict(kv.split("=") for kv in LAP.split(":"))
        assert got[1][1] == {"format": "p010le"}                     # exactly that: no internal key
    finally:
        jl.close()


def test_a_dropped_entry_takes_format_and_key_off_its_adapter(stubs):
    """the drop-in registered as its own id's filter (nothing to fall back to): when the marked entry is dropped the
    download adapter behind it loses `format` and the key together"""
    rt = hbrt.runtime()
    rt.hbhip_rt_register_filter(stubs["format"], C.addressof(C.c_char.in_dll(hip.filters(), "hb_filter_format_hip")))
    jl = hbrt.JobList([(stubs["lapsharp"], LAP), (stubs["format"], "format=p010le")], 66, 38)
    try:
        got = jl.setup()
        assert got[2][1] == {"format": "p010le", KEY: "1"} and got[3][1] == {"format": "p010le", KEY: "1"}
        flt = hip.filters()
        assert flt.hb_hip_filter_init_failed(C.byref(jl.job), 2, C.byref(jl.init)) == 0      # work.c drops the entry
        assert jl.entries()[3] == ("HIP download adapter", {})
    finally:
        jl.close()


def test_422_and_lone_entries_are_not_marked(stubs):
    for pix_fmt, filters in ((YUV422P, [(stubs["lapsharp"], LAP), (stubs["format"], "format=p010le")]),
                             (hbrt.AV_PIX_FMT_YUV420P, [(stubs["format"], "format=p010le")]),
                             (NV12, [(stubs["format"], "format=p010le")])):
        jl = hbrt.JobList(filters, 66, 38, pix_fmt)
        try:
            for name, settings in jl.setup():
                assert KEY not in settings and "hip-planar-step" not in settings, (pix_fmt, name, settings)
                if name == "HIP download adapter":
                    assert "format" not in settings
        finally:
            jl.close()


def test_download_template_is_unchanged_and_has_no_widen_key(built):
    off = dict(ln.split() for ln in open(os.path.join(ROOT, "tests", "golden", "filter_object_layout.txt")))["settings_template"]
    addr = C.addressof(C.c_char.in_dll(hip.filters(), "hb_filter_hip_download")) + int(off)
    assert C.cast(addr, C.POINTER(C.c_char_p))[0].decode() == "format=^(nv12|p010le)$:surface=^([01])$"
