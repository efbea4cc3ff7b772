"""CPU: the deband drop-in's host side - its offset table is FFmpeg's, element for element (hbhip_deband_offsets against
the libm-through-ctypes model of tests/deband_model.py), the settings resolve to the thresholds FFmpeg would derive, the
drop-in declines what would not build a graph, it is registered under the reference's id, and the model's two forms
agree."""
import ctypes as C

import numpy as np
import pytest

import deband_model as dm
from handbrake_amd import hbrt, hip, synth


def _c_offsets(w, h, rng, direction=dm.DIRECTION):
    L = hip.lib()
    L.hbhip_deband_offsets.restype = C.c_int
    L.hbhip_deband_offsets.argtypes = [C.c_int, C.c_int, C.c_int, C.c_float, C.POINTER(C.c_int), C.POINTER(C.c_int)]
    xp = np.zeros(w * h, dtype=np.int32)
    yp = np.zeros(w * h, dtype=np.int32)
    rc = L.hbhip_deband_offsets(w, h, rng, float(direction), xp.ctypes.data_as(C.POINTER(C.c_int)),
                                yp.ctypes.data_as(C.POINTER(C.c_int)))
    return rc, xp.reshape(h, w), yp.reshape(h, w)


RANGES = [16, 0, 1, -1, -16, 127, 128, 200, 5000, 1 << 30]


@pytest.mark.parametrize("rng", RANGES)
def test_offset_table_is_the_models(built, rng):
    rc, xp, yp = _c_offsets(64, 48, rng)
    assert rc == 0
    want_x, want_y = dm.offsets(64, 48, rng)
    np.testing.assert_array_equal(xp, want_x)
    np.testing.assert_array_equal(yp, want_y)
    if rng > 1:
        assert len(np.unique(xp)) > 3 and len(np.unique(yp)) > 3      # the table really varies
    if rng < 0:
        assert np.all(np.hypot(xp, yp) <= -rng + 1)


def test_offset_table_1080p(built):
    rc, xp, yp = _c_offsets(1920, 1080, 16)
    assert rc == 0
    want_x, want_y = dm.offsets(1920, 1080, 16)
    np.testing.assert_array_equal(xp, want_x)
    np.testing.assert_array_equal(yp, want_y)
    assert 10 < max(np.abs(xp).max(), np.abs(yp).max()) <= 15


def test_offset_table_declines(built):
    assert _c_offsets(8, 8, (1 << 30) + 1)[0] != 0
    assert _c_offsets(8, 8, -(1 << 30) - 1)[0] != 0
    assert _c_offsets(0, 8, 16)[0] != 0


def test_numpy_sin_is_not_libm():
    """why the model calls libm: numpy's float32 sin differs from it often enough to move offsets"""
    x = np.arange(256, dtype=np.float32)[None, :]
    y = np.arange(256, dtype=np.float32)[:, None]
    arg = (x * dm.HASH_X + y * dm.HASH_Y).astype(np.float32)
    r = (np.sin(arg) * dm.HASH_SCALE).astype(np.float32)
    r = r - np.floor(r)
    xp, _ = dm.offsets(256, 256, 16)
    d = np.trunc((r * np.float32(16)).astype(np.float32))
    mine = np.trunc((np.cos((r * dm.DIRECTION).astype(np.float32)) * d).astype(np.float32)).astype(np.int64)
    assert (mine != xp).mean() > 0.001


# ---- thresholds ------------------------------------------------------------------------------------------------------
PINNED = {8: {0.02: 5, 0.5: 127, 0.00003: 0}, 10: {0.02: 20, 0.5: 511, 0.00003: 0}, 12: {0.02: 81, 0.5: 2047, 0.00003: 0}}


def _c_params(settings, depth):
    F = hip.filters()
    F.hbhip_deband_params_from_settings.restype = C.c_int
    F.hbhip_deband_params_from_settings.argtypes = [C.c_char_p, C.c_int, C.POINTER(hip.DebandParams)]
    p = hip.DebandParams()
    rc = F.hbhip_deband_params_from_settings(settings.encode(), depth, C.byref(p))
    return rc, p


@pytest.mark.parametrize("depth", [8, 10, 12])
def test_pinned_thresholds(built, depth):
    for t, want in PINNED[depth].items():
        assert dm.threshold(t, depth) == want, (depth, t)
        rc, p = _c_params(f"1thr={t}:2thr={t}:3thr={t}", depth)
        assert rc == 0 and list(p.thr) == [want] * 3, (depth, t)


SWEEP = [0.00003, 0.0001, 0.001, 0.003, 0.005, 0.01, 0.015, 0.02, 0.025, 0.03, 0.04, 0.05, 0.0625, 0.07, 0.1, 0.125,
         0.15, 0.2, 0.25, 0.3, 0.33, 0.4, 0.45, 0.49, 0.5, 1 / 3, 0.123456789]


@pytest.mark.parametrize("depth", [8, 10, 12])
def test_c_resolution_matches_the_model(built, depth):
    for i, t in enumerate(SWEEP):
        t2, t3 = SWEEP[(i + 5) % len(SWEEP)], SWEEP[(i + 11) % len(SWEEP)]
        st = f"1thr={t!r}:2thr={t2!r}:3thr={t3!r}:range={i - 7}:blur={i % 2}"
        rc, p = _c_params(st, depth)
        want = dm.resolve(st, depth)
        assert rc == 0, st
        assert tuple(p.thr) == want["thr"], st
        assert (p.range, p.blur) == (want["range"], want["blur"]) == (i - 7, i % 2)
        assert np.float32(p.direction) == dm.DIRECTION


def test_defaults_are_deband_cs(built):
    rc, p = _c_params("", 8)
    assert rc == 0 and list(p.thr) == [5, 5, 5] and (p.range, p.blur) == (16, 1)
    assert dm.resolve("", 8) == dict(thr=(5, 5, 5), range=16, blur=1)


DECLINED = ["1thr=0.6", "2thr=0.51", "3thr=0.00002", "4thr=0.7", "1thr=0", "blur=2", "blur=-1",
            f"range={(1 << 30) + 1}", f"range={-(1 << 30) - 1}", "range=-2147483648"]
ACCEPTED = ["1thr=0.00003", "4thr=0.5", "1thr=0.5:2thr=0.5:3thr=0.5", "blur=0", "blur=1",
            f"range={1 << 30}", f"range={-(1 << 30)}", "range=0"]


@pytest.mark.parametrize("st", DECLINED)
def test_declined_settings(built, st):
    assert _c_params(st, 8)[0] != 0
    with pytest.raises(dm.Declined):
        dm.resolve(st, 8)


@pytest.mark.parametrize("st", ACCEPTED)
def test_accepted_settings(built, st):
    assert _c_params(st, 8)[0] == 0
    dm.resolve(st, 8)


def test_declined_init_fails_before_the_device(built, monkeypatch):
    """init() refuses declined settings before it looks for a device, so the refusal does not depend on one"""
    monkeypatch.setenv("HBHIP_FORCE_SWAP", "1")
    for st in ("1thr=0.6", "blur=2", "range=-2147483648"):
        with pytest.raises(RuntimeError):
            hbrt.Chain(hip.filters(), [("hb_filter_deband_hip", st)], 64, 48)


def test_init_fails_without_a_device(built):
    """no device: init() fails with the default settings too, so libhb keeps its CPU filter (work.c's fallback)"""
    if hip.lib().hbhip_device_count() > 0:
        pytest.skip("a GPU is present")
    with pytest.raises(RuntimeError):
        hbrt.Chain(hip.filters(), [("hb_filter_deband_hip", "")], 64, 48)


def test_drop_in_registered_under_the_deband_id(built):
    F = hip.filters()
    F.hbhip_filter_get.restype = C.c_void_p
    F.hbhip_filter_get.argtypes = [C.c_int]
    addr = C.addressof(C.c_char.in_dll(F, "hb_filter_deband_hip"))
    assert C.c_int.in_dll(F, "hb_filter_deband_hip").value == 13 == hbrt.FILTER_ID["deband"]
    assert F.hbhip_filter_get(13) == addr
    assert "hbhip_deband_offsets" in hip.ABI_SYMBOLS and hasattr(hip.lib(), "hbhip_deband_create")


# ---- the model's two forms -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rng", [16, -5, 0, 40, 200])
@pytest.mark.parametrize("blur", [0, 1])
def test_model_forms_agree(rng, blur):
    W, H = 37, 23
    xp, yp = dm.offsets(W, H, rng)
    planes = [synth.picture("banded", W, H, 0, cfg=3 + rng % 7)[0],
              synth.picture("banded", W, H, 1, cfg=5, depth=10)[0]]
    changed = 0
    for k, pl in enumerate(planes):
        for (h, w) in [(H, W), ((H + 1) // 2, (W + 1) // 2)]:
            sub = np.ascontiguousarray(pl[:h, :w])
            thr = 6 if k == 0 else 24
            want = dm.deband_plane_loop(sub, xp, yp, thr, blur)
            got = dm.deband_plane(sub, xp, yp, thr, blur)
            np.testing.assert_array_equal(got, want, err_msg=f"{w}x{h} range {rng} blur {blur}")
            changed += int((got != sub).sum())
    if rng != 0:
        assert changed > 0


@pytest.mark.parametrize("depth", [8, 10])
def test_banded_content_takes_both_branches(depth):
    """at the default settings the banded model has samples that are replaced and samples that are kept, with either
    blur, in every plane"""
    fr = synth.stream("banded", 320, 180, 1, depth=depth)[0]
    for blur in (1, 0):
        out = dm.deband_frame(fr, f"blur={blur}", depth)
        for c in range(3):
            diff = out[c] != fr[c]
            assert 0.05 < diff.mean() < 0.95, (blur, c, diff.mean())
