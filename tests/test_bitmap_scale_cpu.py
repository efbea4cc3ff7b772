"""CPU: tests/bitmap_scale_model.py - what the GPU tests hold hbhip_blend_set_bitmaps to - against cases worked out by hand
from scale_subtitle (rendersub.c:242-377), and the new entry points' argument checks, which need no device."""
import ctypes as C

import numpy as np
import pytest

from handbrake_amd import hbrt, hip, synth
import bitmap_scale_model as bm

FW, FH = 192, 108
CROP = (8, 12, 16, 4)                  # top, bottom, left, right


def test_size_and_position_by_hand():
    # 192 / 128 = 108 / 72 = 1.5: (int)(37 * 1.5) = 55, (int)(11 * 1.5) = 16, (int)(5 * 1.5) = 7, (int)(3 * 1.5) = 4
    assert bm.factor(FW, FH, (128, 72)) == 1.5
    assert bm.geometry(FW, FH, 5, 3, 37, 11, (128, 72)) == (7, 4, 55, 16)
    # 192 / 191 = 1.0052..., 108 / 108 = 1: the larger is within 1 % of 1 - the bitmap is used as it is
    f = bm.factor(FW, FH, (191, 108))
    assert 1.0052 < f < 1.0053 and not bm.is_scaled(f)
    assert bm.geometry(FW, FH, 5, 3, 37, 11, (191, 108)) == (5, 3, 37, 11)
    # the larger factor wins (the cropped-video case): 192 / 72 = 2.667 against 108 / 54 = 2
    assert bm.factor(FW, FH, (72, 54)) == FW / 72
    assert bm.geometry(FW, FH, 3, 3, 30, 12, (72, 54)) == (8, 8, 80, 32)
    # no canvas: no scaling
    assert bm.factor(FW, FH, (0, 0)) == 1.0 and bm.geometry(FW, FH, 5, 3, 37, 11, (0, 72)) == (5, 3, 37, 11)
    # just past the threshold either way
    assert bm.is_scaled(bm.factor(FW, FH, (190, 108))) is True              # 1.0105
    assert bm.is_scaled(bm.factor(200, 100, (202, 101))) is False           # 0.990099: |f - 1| = 0.0099


# visible height 108 - 8 - 12 = 88, margin 88 * 2 / 100 = 1; visible width 192 - 16 - 4 = 172
@pytest.mark.parametrize("what,xywh,want", [
    ("top margin", (50, 2, 40, 10), (50, 8 + 1)),
    ("bottom margin", (50, 100, 40, 10), (50, 108 - 12 - 1 - 10)),
    ("too wide", (10, 40, 150, 10), (16 + (172 - 150) // 2, 40)),
    ("fits", (60, 40, 40, 10), (60, 40)),
    ("left margin", (20, 40, 40, 10), (16 + 20, 40)),
    ("right margin", (140, 40, 40, 10), (192 - 4 - 20 - 40, 40)),
    ("too high", (60, 0, 40, 91), (60, 8 - 1)),                             # (88 - 91) / 2 in C: -1, towards 0
])
def test_placement_by_hand(what, xywh, want):
    assert bm.place(FW, FH, *xywh, CROP) == want, what


def test_margin_is_capped_at_20_rows():
    # 2160 rows: 2 % is 43, the margin 20
    assert bm.place(3840, 2160, 100, 5, 400, 100) == (100, 20)
    assert bm.place(3840, 2160, 100, 2100, 400, 100) == (100, 2160 - 20 - 100)


def test_factor_1_keeps_the_bitmap_and_places_it_as_rendersub_does():
    """the rule tests/test_rendersub_cpu.py holds the reference's own rendersub.c to, on the bitmaps that test burns in"""
    for ov in synth.overlays(FW, FH, 4, seed=5, inside=True):
        x, y, planes = ov
        bh, bw = planes[0].shape
        for crop in ((0, 0, 0, 0), CROP):
            margin = min((FH - crop[0] - crop[1]) * 2 // 100, 20)
            if bh > FH - crop[0] - crop[1] - 2 * margin:
                top = crop[0] + (FH - crop[0] - crop[1] - bh) // 2
            elif y < crop[0] + margin:
                top = crop[0] + margin
            elif y > FH - crop[1] - margin - bh:
                top = FH - crop[1] - margin - bh
            else:
                top = y
            if bw > FW - crop[2] - crop[3] - 40:
                left = crop[2] + (FW - crop[2] - crop[3] - bw) // 2
            elif x < crop[2] + 20:
                left = crop[2] + 20
            elif x > FW - crop[3] - 20 - bw:
                left = FW - crop[3] - 20 - bw
            else:
                left = x
            for window in ((0, 0), (FW, FH), (191, 108)):
                gx, gy, gp = bm.render(FW, FH, (x, y, planes, window), crop)
                assert (gx, gy) == (left, top)
                for a, b in zip(gp, planes):
                    np.testing.assert_array_equal(a, b)


def test_scaled_planes_are_the_oracles():
    """every plane, alpha included, through orc_cropscale_plane_sws as a luma plane; a flat plane stays flat"""
    sub = bm.random_sub(37, 11, 5, 3, (128, 72))
    x, y, planes = bm.render(FW, FH, sub)
    assert (x, y) == bm.place(FW, FH, 7, 4, 55, 16) and all(p.shape == (16, 55) for p in planes)
    flat = tuple(np.full((11, 37), v, np.uint8) for v in (16, 128, 240, 255))
    for p, v in zip(bm.render(FW, FH, (5, 3, flat, (128, 72)))[2], (16, 128, 240, 255)):
        assert (p == v).all()


def test_entry_points_check_their_arguments(built):
    L = hip.lib()
    L.hbhip_blend_set_bitmaps.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p]
    L.hbhip_blend_debug_bitmap_stats.argtypes = [C.c_void_p] * 4
    assert L.hbhip_blend_set_bitmaps(None, None, 0, None) == -3
    assert L.hbhip_blend_debug_bitmap_stats(None, None, None, None) == -3
    assert C.sizeof(hip.BitmapSub) == 80
    F = hip.filters()
    F.hb_blend_hip_set_bitmaps.argtypes = [C.c_void_p] * 3 + [C.c_int, C.c_void_p]
    assert F.hb_blend_hip_set_bitmaps(None, None, None, 0, None) == -3
    if L.hbhip_device_count() > 0:
        return
    sub = bm.random_sub(37, 11, 5, 3, (128, 72))
    with pytest.raises(RuntimeError):                                       # no device: an error, not a CPU path
        hbrt.blend_run_bitmaps(F, "hb_blend_hip", bm.frame(FW, FH), [sub + (0,)], [[0]])
