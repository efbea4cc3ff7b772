"""GPU: text subtitles composed on the device (hbhip_blend_set_ass_images, csrc/ass_compose.hip) against
tests/ass_compose_model.py, which tests/test_ass_compose_cpu.py pins to the reference's own compose_subsample_ass.
Integer arithmetic: tolerance 0.

(a) the overlays in the object's device store equal the model's - luma and alpha everywhere, chroma on the model's mask of
    defined samples.  They are read back through the debug getter hbhip_blend_debug_get_overlay (hip.BlendDevice.overlays).
(b) a frame composited after set_ass_images equals, over the whole frame, the frame composited by the set_overlays path
    from the model's overlays with undefined chroma 0: what the mask leaves out cannot change a frame.
(c) the same through hb_blend_hip + hb_blend_hip_set_ass_images on a host frame, a device-resident frame and an NV12 frame.
(d) a second list replaces the first, an empty one clears it.
"""
import functools

import numpy as np
import pytest

from handbrake_amd import hbrt, hip
import ass_compose_model as am

pytestmark = pytest.mark.gpu
NAMES = list(am.CASES)
LOC_CROP = [(loc, crop) for loc in (1, 2, 3) for crop in ((0, 0), (1, 1))]        # crop = (left, top)


@functools.lru_cache(maxsize=None)
def model(name, fmt, loc, crop):
    """(frame width, frame height, images, overlays, masks) of a case: computed once, shared, never written to"""
    fw, fh, images = am.build(name, fmt)
    overlays, masks = am.render(images, *am.SHIFTS[fmt], loc, *crop)
    for _, _, planes in overlays:
        for p in planes:
            p.setflags(write=False)
    return fw, fh, images, overlays, masks


@pytest.fixture(scope="module")
def ctx(built):
    c = hip.Ctx(0)
    yield c
    c.close()


def device(ctx, fw, fh, fmt, loc, depth=8):
    ws, hs = am.SHIFTS[fmt]
    return hip.BlendDevice(ctx, fw, fh, depth=depth, log2_cw=ws, log2_ch=hs, chroma_location=loc, overlay_log2_cw=ws,
                           overlay_log2_ch=hs)


def composite(ctx, b, frame):
    """the object's current list on a copy of `frame`, in HBM"""
    import torch
    planes = [torch.from_numpy(np.ascontiguousarray(p).view(np.int16 if p.dtype == np.uint16 else np.uint8)).to("cuda:0")
              for p in frame]
    torch.cuda.synchronize()
    b.apply_dev(hip.dev_frame(planes))
    ctx.sync()
    return [p.cpu().numpy().view(f.dtype) for p, f in zip(planes, frame)]


def same_overlays(got, want, masks, what):
    assert len(got) == len(want), what
    for (gx, gy, gp), (wx, wy, wp), mask in zip(got, want, masks):
        assert (gx, gy) == (wx, wy), what
        assert [p.shape for p in gp] == [p.shape for p in wp], what
        np.testing.assert_array_equal(gp[0], wp[0], err_msg=what + " Y")
        np.testing.assert_array_equal(gp[3], wp[3], err_msg=what + " A")
        for c in (1, 2):
            np.testing.assert_array_equal(gp[c][mask], wp[c][mask], err_msg=what + f" plane {c}")


def same_frame(got, want, what):
    for c, (g, w) in enumerate(zip(got, want)):
        np.testing.assert_array_equal(g, w, err_msg=what + f" plane {c}")


# every case on 4:2:0 / 4:2:2 / 4:4:4 frames at 8 bits, `pair` at 10 bits too
@pytest.mark.parametrize("name,fmt,depth", [(n, f, 8) for n in NAMES for f in ("420", "422", "444")] + [("pair", "420", 10)])
def test_overlays_and_frames_equal_the_model(ctx, name, fmt, depth):
    """(a) and (b), at both crops and the three chroma sitings"""
    ws, hs = am.SHIFTS[fmt]
    for loc, crop in LOC_CROP:
        fw, fh, images, want, masks = model(name, fmt, loc, crop)
        what = f"{name} {fmt} loc {loc} crop {crop}"
        assert am.defined_share(masks) >= 0.7, what    # of the MODEL's mask: (a) compares something
        frame = am.frame(fw, fh, fmt, depth)
        b = device(ctx, fw, fh, fmt, loc, depth)
        try:
            b.set_ass_images(images, *crop)
            same_overlays(b.overlays(ws, hs), want, masks, what)
            got = composite(ctx, b, frame)
            b.set_overlays(want)
            ref = composite(ctx, b, frame)
        finally:
            b.close()
        assert any((r != f).any() for r, f in zip(ref, frame)), what
        same_frame(got, ref, what)


@pytest.mark.parametrize("name,kind", [(n, k) for n in NAMES for k in ("host", "device", "nv12")] + [("pair", "host10")])
def test_through_the_drop_in(ctx, name, kind):
    """(c): hb_blend_hip_set_ass_images, then work() with an empty list, equals work() with the model's overlays"""
    F = hip.filters()
    fmts = {"host": ("420", "422", "444"), "host10": ("420",), "device": ("420", "444"), "nv12": ("420",)}[kind]
    depth = 10 if kind == "host10" else 8
    for fmt, (loc, crop) in zip(fmts, ((1, (1, 1)), (2, (0, 0)), (3, (1, 1)))):
        fw, fh, images, want, _ = model(name, fmt, loc, crop)
        what = f"{name} {kind} {fmt} loc {loc} crop {crop}"
        frame = am.frame(fw, fh, fmt, depth)
        pix_fmt = am.FRAME_FMT[(fmt, depth)]
        if kind == "nv12":
            frame = (frame[0], np.ascontiguousarray(np.stack(frame[1:], axis=2).reshape(fh // 2, fw)))
            pix_fmt = am.NV12
        kw = dict(pix_fmt=pix_fmt, overlay_fmt=am.OVERLAY_FMT[fmt], chroma_location=loc)
        got = hbrt.blend_run_ass(F, "hb_blend_hip", frame, [images], crop=(crop[1], 0, crop[0], 0), depth=depth,
                                 dev_ctx=ctx if kind == "device" else None, **kw)
        ref = hbrt.blend_run(F, "hb_blend_hip", frame, list(want), **kw)
        assert any((r != f).any() for r, f in zip(ref, frame)), what
        same_frame(got, ref, what)


def test_a_second_list_replaces_the_first_and_none_clears(ctx):
    """(d), on the object and through the drop-in"""
    fw, fh, first, _, _ = model("pair", "420", 1, (1, 1))
    _, _, second, want, masks = model("stack", "420", 1, (1, 1))
    frame = am.frame(fw, fh)
    b = device(ctx, fw, fh, "420", 1)
    try:
        b.set_ass_images(first, 1, 1)
        b.set_ass_images(second, 1, 1)
        same_overlays(b.overlays(), want, masks, "second list")
        got = composite(ctx, b, frame)
        b.set_overlays(want)
        same_frame(got, composite(ctx, b, frame), "second list")
        b.set_ass_images(first, 1, 1)
        b.set_ass_images([], 1, 1)
        assert b.overlays() == []
        same_frame(composite(ctx, b, frame), frame, "cleared")
        empty = [(np.zeros((5, 0), np.uint8), 0, 30, 30, (1, 2, 3, 0))]         # images without an area only: no box
        b.set_ass_images(first, 1, 1)
        b.set_ass_images(empty, 1, 1)
        assert b.overlays() == []
    finally:
        b.close()
    F = hip.filters()
    kw = dict(pix_fmt=am.FRAME_FMT[("420", 8)], overlay_fmt=am.OVERLAY_FMT["420"])
    got = hbrt.blend_run_ass(F, "hb_blend_hip", frame, [first, second], crop=(1, 0, 1, 0), **kw)
    same_frame(got, hbrt.blend_run(F, "hb_blend_hip", frame, list(want), **kw), "drop-in, second list")
    same_frame(hbrt.blend_run_ass(F, "hb_blend_hip", frame, [first, []], crop=(1, 0, 1, 0), **kw), frame, "drop-in, cleared")


def test_overlay_subsampling_other_than_the_frames_is_refused(ctx):
    """compose_subsample_ass makes overlays in the frame's subsampling (ssa_post_init, rendersub.c:679-712)"""
    b = hip.BlendDevice(ctx, 96, 64)                   # 4:4:4 overlays on a 4:2:0 frame
    try:
        with pytest.raises(hip.HipError):
            b.set_ass_images(am.build("pair")[2])
    finally:
        b.close()
