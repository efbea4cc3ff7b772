"""GPU: the ordering rule of device-resident frames (hbhip_core.hip, "How frames are ordered") through the C ABI:
a copy into a frame of another context of the GPU, and the one locked step in which hbhip_filter_push_frame decides
to adopt a frame."""
import numpy as np
import pytest

from handbrake_amd import hip, synth

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("w,h,depth", [(1920, 1080, 8), (322, 186, 10)])
def test_copy_into_a_frame_of_a_second_context(built, w, h, depth):
    """hbhip_frame_copy with dst on another context of the same device: the copy runs on dst's stream behind the
    source's upload, still in flight on the source context's upload stream; dst downloads as the source"""
    a, b = hip.Ctx(0), hip.Ctx(0)
    try:
        planes = [np.ascontiguousarray(p) for p in synth.stream("interlaced", w, h, 1, depth=depth)[0]]
        src, dst = hip.Frame(a, w, h, depth), hip.Frame(b, w, h, depth)
        token = src.upload_async(planes)
        dst.copy_from(src)
        got = dst.download()
        src.upload_done(token)
        for p in range(3):
            np.testing.assert_array_equal(got[p], planes[p], err_msg=f"plane {p}")
        src.close()
        dst.close()
    finally:
        b.close()
        a.close()


def test_push_frame_adopts_only_a_frame_with_one_holder(built):
    """decomb in frames mode takes a frame whose caller is its only holder as its input picture (a reference of its
    own: 2); a frame that somebody else holds too, or a push into a filter that does not work on frames, is copied"""
    w, h = 320, 180
    ctx = hip.Ctx(0)
    frames_mode, plain = hip.DecombDevice(ctx, w, h, mode=7), hip.DecombDevice(ctx, w, h, mode=7)
    try:
        frames_mode.use_frames()
        planes = [np.ascontiguousarray(p) for p in synth.stream("interlaced", w, h, 1)[0]]
        sole, shared, copied = (hip.Frame(ctx, w, h) for _ in range(3))
        for f in (sole, shared, copied):
            f.upload(planes)
        shared.retain()
        frames_mode.push_frame(sole)
        frames_mode.push_frame(shared)
        plain.push_frame(copied)
        assert (sole.refs(), shared.refs(), copied.refs()) == (2, 2, 1)
        ctx.sync()
        shared.release()
        for f in (sole, shared, copied):
            f.close()
    finally:
        frames_mode.close()
        plain.close()
        ctx.close()
