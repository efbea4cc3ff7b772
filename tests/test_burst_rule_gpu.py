"""GPU: the one burst rule of the one-in / one-out filters (csrc/hbhip_internal.h: hbhip_for_each_burst) where no other
test pins it - pad, format and colorspace.  A launch takes up to 16 consecutive frames whose six pitches agree: 20 frames
in one process_dev call give the bytes of 20 calls of one frame each (the path the oracle tests hold), and the context's
profile shows the cut: 16 + 4 with one pitch, 9 + 11 with a pitch change at frame 9, 20 launches with alternating pitches.

160 x 96 4:2:0 with row paddings of 0 / 16 / 64 samples: every plane address and pitch stays a multiple of 16 bytes, so
the frames take SimpleFilter's direct path and the mixed pitches really reach process_many (with odd paddings they would
go through the filter's own pictures instead)."""
import ctypes as C
import functools

import numpy as np
import pytest

from burst_util import bursts
from handbrake_amd import hip, synth

pytestmark = pytest.mark.gpu
W, H, N = 160, 96, 20
BT601, BT709 = (6, 6, 6, 1), (1, 1, 1, 1)


class PadParams(C.Structure):
    _fields_ = [("width", C.c_int), ("height", C.c_int), ("x", C.c_int), ("y", C.c_int), ("fill", C.c_int * 3)]


def _pad(depth):
    pp = PadParams(192, 128, 16, 16, (C.c_int * 3)(16 << (depth - 8), 128 << (depth - 8), 128 << (depth - 8)))
    make = lambda ctx: hip._create("hbhip_pad_create", ctx, [C.c_void_p, C.POINTER(PadParams)] + [C.c_int] * 5 + [C.POINTER(C.c_void_p)],
                                   ctx.h, C.byref(pp), W, H, depth, 1, 1)
    return make, dict(depth=depth, out_shape=(128, 192))


def _format(depth, out_depth):
    make = lambda ctx: hip._create("hbhip_format_create", ctx, [C.c_void_p] + [C.c_int] * 7 + [C.POINTER(C.c_void_p)],
                                   ctx.h, W, H, depth, out_depth, 1, 1, 0)
    return make, dict(depth=depth, out_depth=out_depth)


def _colorspace(depth):
    return (lambda ctx: hip.colorspace_device_filter(ctx, W, H, BT601, BT709, depth=depth)), dict(depth=depth)


FILTERS = {
    "pad-8": ("pad", lambda: _pad(8)), "pad-10": ("pad", lambda: _pad(10)),
    "format-8to10": ("format", lambda: _format(8, 10)), "format-10to8": ("format", lambda: _format(10, 8)),
    "colorspace-8": ("colorspace", lambda: _colorspace(8)), "colorspace-10": ("colorspace", lambda: _colorspace(10)),
}
# paddings per frame, launches expected
CASES = {"one-pitch": ((0,), 2), "change-at-9": ((0,) * 9 + (64,) * 11, 2), "alternating": ((0, 16), 20)}


@functools.lru_cache(maxsize=None)
def _frame_by_frame(which):
    """(the input frames, what the filter makes of them one process_dev call per frame), computed once; leave them unchanged"""
    make, kw = FILTERS[which][1]()
    frames = synth.stream("random", W, H, N, depth=kw["depth"])
    return frames, bursts(make, frames, [1] * N, **kw)


@pytest.mark.parametrize("case", sorted(CASES))
@pytest.mark.parametrize("which", sorted(FILTERS))
def test_twenty_frames_are_cut_by_the_shared_rule(built, which, case):
    name, (make, kw) = FILTERS[which][0], FILTERS[which][1]()
    pads, launches = CASES[case]
    frames, want = _frame_by_frame(which)
    ctx = hip.Ctx(0)
    try:
        ctx.profile(True)
        got = bursts(make, frames, [N], pads=pads, ctx=ctx, **kw)
        stats = ctx.profile_stats()
    finally:
        ctx.close()
    assert len(got) == len(want) == N
    for t in range(N):
        for c in range(3):
            assert got[t][c].shape == want[t][c].shape
            np.testing.assert_array_equal(got[t][c], want[t][c], err_msg=f"{which} {case} frame {t} plane {c}")
    assert stats[name][0] == launches, stats
