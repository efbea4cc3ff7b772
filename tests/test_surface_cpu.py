"""CPU: device surfaces without a device - the numpy model of the repack (tests/surface_model.py), what the new entry points
of include/hbhip.h answer to missing arguments, and the adapters' surface setting at the plugin boundary."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from handbrake_amd import hbrt, hip
import surface_model as sm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ERR_NODEVICE, ERR_ARG = -1, -3
SIZES = [(2, 2), (18, 10), (33, 7), (66, 38), (130, 6)]
LAYOUTS = [(16, 1), (256, 16), (64, 2)]


def planar(rng, w, h, depth):
    dt = np.uint8 if depth == 8 else np.uint16
    ch, cw = (h + 1) // 2, (w + 1) // 2
    return tuple(rng.integers(0, 1 << depth, s).astype(dt) for s in ((h, w), (ch, cw), (ch, cw)))


@pytest.mark.parametrize("depth", [8, 10])
@pytest.mark.parametrize("pitch_align,rows_align", LAYOUTS)
@pytest.mark.parametrize("w,h", SIZES)
def test_merge_then_split_is_the_identity_and_touches_nothing_else(w, h, depth, pitch_align, rows_align):
    rng = np.random.default_rng(w * 100 + h + depth)
    lay = sm.pooled(w, h, depth, pitch_align, rows_align, lead=48, tail=80)
    x = planar(rng, w, h, depth)
    buf = np.full(lay.size, 0xA5, dtype=np.uint8)
    sm.merge(buf, lay, x)
    for got, want in zip(sm.split(buf, lay), x):
        np.testing.assert_array_equal(got, want)
    assert (buf[~lay.written()] == 0xA5).all()
    if depth == 10:
        for p in range(2):
            assert (sm.plane_rows(buf, lay, p) & 63 == 0).all()           # merge leaves no stale bits in the low end


@pytest.mark.parametrize("depth", [8, 10])
@pytest.mark.parametrize("w,h", SIZES)
def test_split_then_merge_restores_the_samples(w, h, depth):
    rng = np.random.default_rng(7 * w + h)
    lay = sm.pooled(w, h, depth, 256, 16)
    buf = rng.integers(0, 256, lay.size, dtype=np.uint8)
    back = sm.merge(np.zeros_like(buf), lay, sm.split(buf, lay))
    keep = 0xFFC0 if depth == 10 else 0xFF                                # P010LE: the low six bits are not samples
    for p in range(2):
        np.testing.assert_array_equal(sm.plane_rows(back, lay, p), sm.plane_rows(buf, lay, p) & keep)


def test_chroma_is_even_cb_odd_cr():
    lay = sm.pooled(6, 4, 8, 16, 1)
    buf = np.zeros(lay.size, dtype=np.uint8)
    buf[lay.offset[1]:lay.offset[1] + 6] = [10, 20, 11, 21, 12, 22]
    _, cb, cr = sm.split(buf, lay)
    assert list(cb[0]) == [10, 11, 12] and list(cr[0]) == [20, 21, 22]
    lay10 = sm.pooled(2, 2, 10, 16, 1)
    buf10 = np.zeros(lay10.size, dtype=np.uint8)
    buf10[0:2] = [0xFF, 0xFF]                                             # 0xffff >> 6 = 1023; the low bits vanish
    assert sm.split(buf10, lay10)[0][0, 0] == 1023


def test_new_entry_points_refuse_null_arguments(built):
    L = hip.lib()
    out = C.c_void_p()
    mem = hip.DevSurface()
    assert L.hbhip_surface_alloc(None, 66, 38, 8, 256, 16, C.byref(out)) == ERR_ARG
    assert L.hbhip_surface_alloc(None, 66, 38, 8, 256, 16, None) == ERR_ARG
    assert L.hbhip_surface_wrap(None, C.byref(mem), 66, 38, 8, None, None, C.byref(out)) == ERR_ARG
    assert L.hbhip_surface_describe(None, C.byref(mem), None, None, None) == ERR_ARG
    assert L.hbhip_surface_set_ready_event(None, None) == ERR_ARG
    L.hbhip_surface_retain(None)
    L.hbhip_surface_release(None)
    tok = C.c_void_p()
    for fn in (L.hbhip_frame_import_surface, L.hbhip_frame_export_surface):
        assert fn(None, None) == ERR_ARG
    for fn in (L.hbhip_frame_import_surface_async, L.hbhip_frame_export_surface_async):
        assert fn(None, None, C.byref(tok)) == ERR_ARG and not tok.value
    assert L.hbhip_ctx_bus_bytes(None, None, None) == ERR_ARG
    if L.hbhip_device_count() == 0:
        ctx = C.c_void_p()
        assert L.hbhip_ctx_create(0, C.byref(ctx)) == ERR_NODEVICE and not ctx.value     # no context, so no surface either


def template_of(symbol):
    off = dict(ln.split() for ln in open(os.path.join(ROOT, "tests", "golden", "filter_object_layout.txt")))["settings_template"]
    addr = C.addressof(C.c_char.in_dll(hip.filters(), symbol)) + int(off)
    return C.cast(addr, C.POINTER(C.c_char_p))[0].decode()


def template_accepts(template, settings):
    """hb_validate_filter_string's rule (param.c): every key is one of the template's and its value matches the key's regex"""
    rules = dict(kv.split("=", 1) for kv in template.split(":"))
    for kv in settings.split(":"):
        key, _, value = kv.partition("=")
        if key not in rules or re.search(rules[key], value) is None:
            return False
    return True


def test_download_template_takes_the_surface_setting(built):
    t = template_of("hb_filter_hip_download")
    assert t == "format=^(nv12|p010le)$:surface=^([01])$"
    assert template_accepts(t, "format=nv12:surface=1")
    assert template_accepts(t, "format=p010le:surface=0")
    assert template_accepts(t, "format=nv12")
    assert not template_accepts(t, "format=nv12:surface=2")
    assert not template_accepts(t, "format=nv16:surface=1")


def test_adapters_fail_init_cleanly_without_a_device(built):
    if hip.lib().hbhip_device_count() > 0:
        return  # running on a GPU box: nothing to assert here
    F = hip.filters()
    for pix_fmt in (hbrt.AV_PIX_FMT_NV12, hbrt.AV_PIX_FMT_P010LE):
        for stage in (("hb_filter_hip_upload", ""), ("hb_filter_hip_download", "format=nv12:surface=1"),
                      ("hb_filter_hip_download", "surface=1")):
            with pytest.raises(RuntimeError):
                hbrt.Chain(F, [stage], 66, 38, pix_fmt=pix_fmt)
