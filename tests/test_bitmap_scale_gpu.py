"""GPU: bitmap subtitles scaled and placed on the device (hbhip_blend_set_bitmaps, csrc/bitmap_scale.hip) against
tests/bitmap_scale_model.py - scale_subtitle's arithmetic (rendersub.c:242-377) with the planes through the oracle's
restatement of libswscale (orc_cropscale_plane_sws).  Integer arithmetic: tolerance 0.

(1) the overlay in the object's device store - position, size, all four planes - equals the model's, over the factors the
    reference meets and at the kernel's tile seams;
(2) the placement rule on the device;
(3) a frame composited after set_bitmaps equals, over the whole frame, the frame composited by set_overlays from the model's
    scaled and placed bitmap - planar frames at two subsamplings and depths, a device-resident frame and an NV12 host frame
    through hb_blend_hip + hb_blend_hip_set_bitmaps;
(4) the cache: a subtitle is uploaded and scaled once, a hit costs nothing;
(5) what is refused, and that a refusal leaves the list empty.
"""
import functools

import numpy as np
import pytest

from handbrake_amd import hbrt, hip
import bitmap_scale_model as bm

pytestmark = pytest.mark.gpu
FW, FH = 192, 108
CROP = (8, 12, 16, 4)                                  # top, bottom, left, right
TILE_W, TILE_H = 64, 16                                # BMS_TILE_W / BMS_TILE_H of csrc/bitmap_scale.h
UNSUPPORTED, ARG = -5, -3
LAYOUT = {"420": (1, 1), "444": (0, 0)}
PIX_FMT = {("420", 8): 0, ("444", 8): 5, ("420", 10): 62, ("444", 10): 68}
NV12 = 23

# canvas -> the bitmap on it (width, height, x, y): inside the frame once scaled
CANVASES = {
    (96, 54): (40, 10, 24, 27),                        # factor 2
    (128, 72): (53, 14, 32, 36),                       # 1.5
    (288, 162): (90, 30, 72, 81),                      # 0.667
    (72, 54): (30, 10, 18, 27),                        # x 2.667 against y 2: the larger wins
    (192, 81): (80, 16, 48, 40),                       # 1.333: the cropped-video case
    (768, 432): (320, 86, 192, 216),                   # 0.25, the lower bound: 22 to 24 taps
    (191, 108): (80, 21, 48, 54),                      # 1.005: not scaled
}


@functools.lru_cache(maxsize=None)
def case(w, h, x, y, window, seed=1, crop=(0, 0, 0, 0), fw=FW, fh=FH):
    """(subtitle, the model's overlay for it): computed once, shared, never written to"""
    sub = bm.random_sub(w, h, x, y, window, seed)
    want = bm.render(fw, fh, sub, crop)
    for p in sub[2] + want[2]:
        p.setflags(write=False)
    return sub, want


@pytest.fixture(scope="module")
def ctx(built):
    c = hip.Ctx(0)
    yield c
    c.close()


def device(ctx, fmt="420", depth=8, fw=FW, fh=FH, **kw):
    lcw, lch = LAYOUT[fmt]
    return hip.BlendDevice(ctx, fw, fh, depth=depth, log2_cw=lcw, log2_ch=lch, **kw)


def composite(ctx, b, frame):
    """the object's current list on a copy of `frame`, in HBM"""
    import torch
    planes = [torch.from_numpy(np.ascontiguousarray(p).view(np.int16 if p.dtype == np.uint16 else np.uint8)).to("cuda:0")
              for p in frame]
    torch.cuda.synchronize()
    b.apply_dev(hip.dev_frame(planes))
    ctx.sync()
    return [p.cpu().numpy().view(f.dtype) for p, f in zip(planes, frame)]


def same_overlay(got, want, what):
    (gx, gy, gp), (wx, wy, wp) = got, want
    assert (gx, gy) + gp[0].shape == (wx, wy) + wp[0].shape, what
    for c, (g, w) in enumerate(zip(gp, wp)):
        np.testing.assert_array_equal(g, w, err_msg=f"{what} plane {c}")


def same_frame(got, want, what):
    for c, (g, w) in enumerate(zip(got, want)):
        np.testing.assert_array_equal(g, w, err_msg=f"{what} plane {c}")


def stored(ctx, subs, crop=(0, 0, 0, 0)):
    b = device(ctx)
    try:
        b.set_bitmaps([s + (k,) for k, s in enumerate(subs)], crop)
        return b.overlays(0, 0)
    finally:
        b.close()


@pytest.mark.parametrize("canvas", list(CANVASES))
def test_store_equals_the_model(ctx, canvas):
    sub, want = case(*CANVASES[canvas], canvas)
    scaled = bm.is_scaled(bm.factor(FW, FH, canvas))
    assert scaled == (canvas != (191, 108)) and (want[2][0].shape != sub[2][0].shape) == scaled
    assert 0 <= want[0] and want[0] + want[2][0].shape[1] <= FW and 0 <= want[1] and want[1] + want[2][0].shape[0] <= FH
    got = stored(ctx, [sub])
    assert len(got) == 1
    same_overlay(got[0], want, f"canvas {canvas}")


def test_odd_size_and_position(ctx):
    sub, want = case(37, 11, 5, 3, (128, 72))
    assert want[2][0].shape == (16, 55)
    same_overlay(stored(ctx, [sub])[0], want, "37 x 11 at (5, 3), factor 1.5")


@pytest.mark.parametrize("w,h,canvas,off", [(49, 13, (144, 81), 1), (42, 10, (128, 72), -1)])
def test_tile_seams(ctx, w, h, canvas, off):
    """a scaled bitmap one sample larger / smaller than the kernel's tile in each direction"""
    sub, want = case(w, h, 30, 20, canvas, seed=7)
    assert want[2][0].shape == (TILE_H + off, TILE_W + off)
    same_overlay(stored(ctx, [sub])[0], want, f"tile {off:+d}")


# at factor 1.5 with CROP: margin 1 row; a 40 x 10 bitmap becomes 60 x 15, a 100 x 10 one 150 x 15 (wider than 172 - 40)
@pytest.mark.parametrize("what,xywh,moved", [("top margin", (40, 2, 40, 10), True), ("bottom margin", (40, 60, 40, 10), True),
                                              ("too wide", (10, 30, 100, 10), True), ("fits", (40, 30, 40, 10), False)])
def test_placement_on_the_device(ctx, what, xywh, moved):
    x, y, w, h = xywh
    sub, want = case(w, h, x, y, (128, 72), seed=3, crop=CROP)
    assert ((want[0], want[1]) != (int(x * 1.5), int(y * 1.5))) == moved, what
    b = device(ctx)
    try:
        b.set_bitmaps([sub + (9,)], CROP)
        (gx, gy, gp), = b.overlays(0, 0)
    finally:
        b.close()
    assert (gx, gy, gp[0].shape[1], gp[0].shape[0]) == (want[0], want[1], want[2][0].shape[1], want[2][0].shape[0]), what


@pytest.mark.parametrize("fmt,depth", [("420", 8), ("444", 8), ("420", 10), ("444", 10)])
def test_composited_frame(ctx, fmt, depth):
    subs, wants = zip(*[case(*CANVASES[c], c) for c in ((128, 72), (191, 108))])
    frame = bm.frame(FW, FH, fmt, depth)
    for sub, want in zip(subs, wants):
        b = device(ctx, fmt, depth)
        try:
            b.set_bitmaps([sub + (1,)])
            got = composite(ctx, b, frame)
            b.set_overlays([want])
            ref = composite(ctx, b, frame)
        finally:
            b.close()
        assert any((r != f).any() for r, f in zip(ref, frame))
        same_frame(got, ref, f"{fmt} {depth}")


@pytest.mark.parametrize("kind", ["host", "device", "device444", "nv12"])
def test_through_the_drop_in(ctx, kind):
    """hb_blend_hip_set_bitmaps for two frames in a row, then work() with an empty list, equals work() with the model's overlay"""
    F = hip.filters()
    fmt = "444" if kind == "device444" else "420"
    sub, want = case(*CANVASES[(96, 54)], (96, 54), crop=CROP)
    frame = bm.frame(FW, FH, fmt)
    pix_fmt = PIX_FMT[(fmt, 8)]
    if kind == "nv12":
        frame = (frame[0], np.ascontiguousarray(np.stack(frame[1:], axis=2).reshape(FH // 2, FW)))
        pix_fmt = NV12
    got = hbrt.blend_run_bitmaps(F, "hb_blend_hip", frame, [sub + (3003,)], [[0], [0]], crop=CROP, pix_fmt=pix_fmt,
                                 dev_ctx=ctx if kind.startswith("device") else None)
    ref = hbrt.blend_run(F, "hb_blend_hip", frame, [want], pix_fmt=pix_fmt)
    assert any((r != f).any() for r, f in zip(ref, frame)), kind
    same_frame(got, ref, kind)


def test_two_overlapping_bitmaps_in_one_list(ctx):
    """VOBSUBs may overlap in time: the store keeps the list's order and the second lands on the first"""
    a, wa = case(40, 12, 24, 27, (96, 54), seed=11)
    c, wc = case(53, 14, 50, 40, (128, 72), seed=12)       # a list may mix canvases
    assert wa[0] < wc[0] < wa[0] + wa[2][0].shape[1] and wa[1] < wc[1] + wc[2][0].shape[0] and wc[1] < wa[1] + wa[2][0].shape[0]
    frame = bm.frame(FW, FH)
    for subs, wants in (((a, c), (wa, wc)), ((c, a), (wc, wa))):
        b = device(ctx)
        try:
            b.set_bitmaps([s + (k + 1,) for k, s in enumerate(subs)])
            got = b.overlays(0, 0)
            assert len(got) == 2
            for g, w in zip(got, wants):
                same_overlay(g, w, "overlapping")
            out = composite(ctx, b, frame)
            b.set_overlays(list(wants))
            same_frame(out, composite(ctx, b, frame), "overlapping")
        finally:
            b.close()


def test_cache(ctx):
    a, wa = case(*CANVASES[(96, 54)], (96, 54))
    c, wc = case(*CANVASES[(191, 108)], (191, 108), seed=2)
    d, wd = case(37, 11, 5, 3, (128, 72))
    frame = bm.frame(FW, FH)
    b = device(ctx)
    try:
        assert b.bitmap_stats() == (0, 0, 0)
        for k in range(3):                                                  # one scaled, one as it is: n = 2
            b.set_bitmaps([a + (1,), c + (2,)])
            assert b.bitmap_stats() == (1, 2, 2 * k)
        for g, w in zip(b.overlays(0, 0), (wa, wc)):
            same_overlay(g, w, "after three calls")
        b.set_bitmaps([a + (1,), d + (3,)])                                 # one key replaced: exactly one more scale
        assert b.bitmap_stats() == (2, 3, 5)
        for g, w in zip(b.overlays(0, 0), (wa, wd)):
            same_overlay(g, w, "one key replaced")
        b.set_bitmaps([a + (1,), c + (2,)])                                 # the dropped key is new again
        assert b.bitmap_stats() == (2, 4, 6)
        a2 = a[:3] + ((128, 72),)                                           # the same key on another canvas: rescaled
        b.set_bitmaps([a2 + (1,)])
        assert b.bitmap_stats() == (3, 5, 6)
        same_overlay(b.overlays(0, 0)[0], bm.render(FW, FH, a2), "same key, another geometry")
        moved = (a2[0] + 4, a2[1] + 2) + a2[2:]                             # ... at another place: the same pixels, placed anew
        b.set_bitmaps([moved + (1,)])
        assert b.bitmap_stats() == (3, 5, 7)
        same_overlay(b.overlays(0, 0)[0], bm.render(FW, FH, moved), "same key, another position")
        empty = (0, 0, tuple(np.zeros((0, 0), np.uint8) for _ in range(4)), (96, 54))
        b.set_bitmaps([empty + (4,)])                                       # a PGS "clear" packet
        assert b.overlays(0, 0) == [] and b.bitmap_stats() == (3, 5, 7)
        b.set_bitmaps([a + (1,)])
        b.set_bitmaps([])
        assert b.overlays(0, 0) == []
        same_frame(composite(ctx, b, frame), frame, "n == 0")
    finally:
        b.close()
    # the drop-in: work() after an empty list returns the frame as it came
    F = hip.filters()
    same_frame(hbrt.blend_run_bitmaps(F, "hb_blend_hip", frame, [a + (0,)], [[0], []]), frame, "drop-in, n == 0")


def test_refusals_leave_the_list_empty(ctx):
    ok, _ = case(*CANVASES[(96, 54)], (96, 54))
    small = bm.random_sub(6, 6, 10, 10, (96, 54))
    b = device(ctx)
    try:
        for what, sub, rc in (("factor 5", ok[:3] + ((38, 21),), UNSUPPORTED), ("factor 0.2", ok[:3] + ((960, 540),), UNSUPPORTED),
                              ("6 x 6 at factor 2", small, UNSUPPORTED)):
            b.set_bitmaps([ok + (1,)])
            assert len(b.overlays(0, 0)) == 1
            assert b.set_bitmaps([ok + (1,), sub + (2,)], raise_on_error=False) == rc, what
            assert b.overlays(0, 0) == [], what
        b.set_bitmaps([small[:3] + ((192, 108),) + (2,)])                   # as it is, 6 x 6 is fine
        assert len(b.overlays(0, 0)) == 1
        short = [[p.strides[0] for p in ok[2]]]
        short[0][3] -= 1
        assert b.set_bitmaps([ok + (1,)], strides=short, raise_on_error=False) == ARG
        assert b.overlays(0, 0) == []
        with pytest.raises(hip.HipError):
            b.set_bitmaps([ok[:3] + ((38, 21),) + (1,)])
    finally:
        b.close()
    b = device(ctx, overlay_log2_cw=1, overlay_log2_ch=1)                   # 4:2:0 overlays: not a bitmap subtitle's format
    try:
        assert b.set_bitmaps([ok + (1,)], raise_on_error=False) == UNSUPPORTED
        assert b.overlays(1, 1) == []
    finally:
        b.close()
