"""CPU: hb_get_preview's list - the job's picture filters, a display rescale, `format=bgra` - through
hb_hip_setup_hw_filters / hb_hip_filter_init_failed (libhb/hip_common.c) without a device: the mark and the bracket before
any init(), and the list as hb_get_preview built it after every drop-in has declined (HBHIP_FORCE_SWAP=1: no device,
every init() fails).  Plus the new entry points of include/hbhip.h and the stand-in's four packed pixel formats."""
import ctypes as C
import os
import re

import pytest

from handbrake_amd import hbrt, hip

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ERR_ARG = -3
KEY = "hip-rgb-step"
MARKS = ("hip-planar-step", "hip-up-step", "hip-widen-step", "hip-deepen-step", KEY)
SCALE = "width=64:height=36:crop-top=0:crop-bottom=0:crop-left=0:crop-right=0"
NEW = ["hbhip_frame_download_rgb32", "hbhip_frame_download_rgb32_async"]
RGB32 = {"argb": 25, "rgba": 26, "abgr": 27, "bgra": 28}          # FFmpeg's numbers


@pytest.fixture()
def stubs(built, monkeypatch):
    """CPU `crop_scale` and `format` objects that do nothing (no frame is pushed), registered as their ids' filters"""
    monkeypatch.setenv("HBHIP_FORCE_SWAP", "1")
    hip.filters()
    F = hbrt.FILTER_ID
    keep = {}
    rt = hbrt.runtime()
    for name, shown in (("crop_scale", "Crop and Scale"), ("format", "Format")):
        addr, keep[name] = hbrt.filter_stub(F[name], shown)
        rt.hbhip_rt_register_filter(F[name], addr)
    yield F
    for name in keep:
        rt.hbhip_rt_register_filter(F[name], None)


@pytest.mark.parametrize("order", ["bgra", "rgba", "argb", "abgr"])
def test_the_format_entry_is_marked_and_the_adapter_told(stubs, order):
    jl = hbrt.JobList([(stubs["crop_scale"], SCALE), (stubs["format"], "format=" + order)], 96, 54)
    try:
        assert [n for n, _ in jl.entries()] == ["Crop and Scale", "Format"]
        got = jl.setup()
        assert len(got) == 4 and "HIP" in got[1][0] and "cale" in got[1][0], got
        assert [got[0][0], got[2][0], got[3][0]] == ["HIP upload adapter", "Format (HIP)", "HIP download adapter"]
        assert got[0][1] == {}
        assert got[2][1] == {"format": order, KEY: "1"}              # the entry keeps its own setting beside the mark
        assert got[3][1] == {"format": order, KEY: "1"}
    finally:
        jl.close()


@pytest.mark.skipif(__import__("torch").cuda.is_available(), reason="needs a box WITHOUT a GPU: every drop-in init must fail")
def test_after_the_fallbacks_the_list_is_hb_get_previews(stubs):
    jl = hbrt.JobList([(stubs["crop_scale"], SCALE), (stubs["format"], "format=bgra")], 96, 54)
    try:
        jl.setup()
        got = jl.init_all()
        assert [n for n, _ in got] == ["Crop and Scale", "Format"]      # CPU objects, no adapter left, nothing dropped
        assert got[0][1] == dict(kv.split("=") for kv in SCALE.split(":"))
        assert got[1][1] == {"format": "bgra"}                           # exactly that: no internal key
        assert not any(k in s for _, s in got for k in MARKS)
    finally:
        jl.close()


def test_a_dropped_entry_takes_format_and_key_off_its_adapter(stubs):
    """the drop-in registered as its own id's filter (nothing to fall back to): when the marked entry is dropped the download
    adapter behind it loses `format` and the key together"""
    rt = hbrt.runtime()
    rt.hbhip_rt_register_filter(stubs["format"], C.addressof(C.c_char.in_dll(hip.filters(), "hb_filter_format_hip")))
    jl = hbrt.JobList([(stubs["crop_scale"], SCALE), (stubs["format"], "format=bgra")], 96, 54)
    try:
        got = jl.setup()
        assert got[2][1] == {"format": "bgra", KEY: "1"} and got[3][1] == {"format": "bgra", KEY: "1"}
        assert hip.filters().hb_hip_filter_init_failed(C.byref(jl.job), 2, C.byref(jl.init)) == 0      # work.c drops the entry
        assert jl.entries()[3] == ("HIP download adapter", {})
    finally:
        jl.close()


def test_lone_422_and_10bit_entries_are_not_marked(stubs):
    both = [(stubs["crop_scale"], SCALE), (stubs["format"], "format=bgra")]
    for pix_fmt, filters in ((hbrt.AV_PIX_FMT_YUV420P, [(stubs["format"], "format=bgra")]),
                             (hbrt.PIX_FMT[("2x1", 8)], both), (hbrt.PIX_FMT[("1x1", 8)], both),
                             (hbrt.AV_PIX_FMT_YUV420P10, both), (hbrt.AV_PIX_FMT_NV12, both)):
        jl = hbrt.JobList(filters, 96, 54, pix_fmt)
        try:
            for name, settings in jl.setup():
                assert not any(k in settings for k in MARKS), (pix_fmt, name, settings)
                if name == "HIP download adapter":
                    assert settings.get("format") in (None, "nv12"), (pix_fmt, settings)      # (an nv12 job's own format)
        finally:
            jl.close()


def test_other_rgb_targets_are_not_marked(stubs):
    """rgb24 / bgr24, the 0-alpha orders, gbrp: names the stand-in does not even know, and no mark"""
    for target in ("rgb24", "bgr24", "bgr0", "rgb0", "gbrp"):
        jl = hbrt.JobList([(stubs["crop_scale"], SCALE), (stubs["format"], "format=" + target)], 96, 54)
        try:
            got = jl.setup()
            assert not any(k in s for _, s in got for k in MARKS), (target, got)
            assert "format" not in got[-1][1] or got[-1][0] != "HIP download adapter", (target, got)
        finally:
            jl.close()


# ---- the ABI and the stand-in's formats -------------------------------------------------------------------------------------
def test_new_symbols_are_declared_exported_and_bound(built):
    text = open(os.path.join(ROOT, "include", "hbhip.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    for sym in NEW:
        assert re.search(r"\bint\s+%s\s*\(" % sym, text), f"{sym} is not declared in include/hbhip.h"
        assert sym in hip.ABI_SYMBOLS
    assert re.search(r"enum\s*\{\s*HBHIP_RGB32_BGRA\s*,\s*HBHIP_RGB32_RGBA\s*,\s*HBHIP_RGB32_ARGB\s*,\s*HBHIP_RGB32_ABGR\s*\}", text)
    L = hip.lib()
    for sym in NEW:
        assert hasattr(L, sym), f"{sym} is not exported by libhbhip.so"
    tok = C.c_void_p(1)
    assert L.hbhip_frame_download_rgb32(None, None, 0, 0, 1, 0) == ERR_ARG
    assert L.hbhip_frame_download_rgb32_async(None, None, 0, 0, 1, 0, C.byref(tok)) == ERR_ARG
    host = open(os.path.join(ROOT, "handbrake_amd", "libhb", "hbhip_host.h")).read()
    assert re.search(r'#define\s+HBHIP_FORMAT_RGB_STEP\s+"%s"' % KEY, host)
    assert hip.RGB32_ORDERS == ("bgra", "rgba", "argb", "abgr")


@pytest.mark.parametrize("name", sorted(RGB32))
def test_the_stand_in_lays_a_packed_picture_out(built, name):
    rt = hbrt.runtime()
    rt.av_get_pix_fmt.argtypes, rt.av_get_pix_fmt.restype = [C.c_char_p], C.c_int
    fmt = rt.av_get_pix_fmt(name.encode())
    assert fmt == RGB32[name]
    for w, h in ((2, 2), (66, 34), (1920, 1080)):
        info = hbrt.frame_layout(fmt, w, h)
        assert info.nplanes == 1
        assert info.plane_width[0] == w and info.plane_height[0] == h
        assert info.plane_stride[0] >= 4 * w and info.plane_stride[0] % 64 == 0 and info.plane_stride[0] < 4 * w + 64
