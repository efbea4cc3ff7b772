"""GPU: the one burst rule of the one-in / one-out filters (csrc/hbhip_internal.h: hbhip_for_each_run, and
hbhip_for_each_burst on top of it) for the filters where no other test pins it: pad, format and colorspace, which take
the filling form, and rotate, grayscale, lapsharp, unsharp / chroma smooth, crop/scale and hqdn3d, which take the cut
alone and fill argument structs of their own.  A launch takes up to maxf consecutive frames whose six pitches agree (16,
the two-pass scaler 8): 20 frames in one process_dev call give the bytes of 20 calls of one frame each (the path the
oracle tests hold), and the context's profile shows the cut - 16 + 4 with one pitch, 9 + 11 with a pitch change at frame
9, 20 runs with alternating pitches.  A run that the filter's batched kernel cannot take (10-bit rotate, grayscale and
unsharp, a 5 x 5 lapsharp kernel) goes frame by frame through the generic kernels: the launches are counted per frame then.

160 x 96 4:2:0 with row paddings of 0 / 16 / 64 samples: every plane address and pitch stays a multiple of 16 bytes, so
the frames take SimpleFilter's direct path and the mixed pitches really reach process_many (with odd paddings they would
go through the filter's own pictures instead).  The one output whose rows are no such multiple - the 40-byte chroma rows
of the 8-bit 80 x 48 picture - gets a 16-byte pitch (out_row_bytes)."""
import ctypes as C
import functools

import numpy as np
import pytest

import oracle_lib as ol
from burst_util import bursts
from handbrake_amd import hip, synth

pytestmark = pytest.mark.gpu
W, H, N = 160, 96, 20
BT601, BT709 = (6, 6, 6, 1), (1, 1, 1, 1)
CASES = {"one-pitch": (0,), "change-at-9": (0,) * 9 + (64,) * 11, "alternating": (0, 16)}      # paddings per frame


# ---- launches expected under a profile name, from the paddings of the N frames ----
def _runs(pads, maxf):
    """the lengths of the maximal runs of at most maxf consecutive frames with one pitch"""
    seq = [pads[i % len(pads)] for i in range(N)]
    out = []
    for i, p in enumerate(seq):
        if i and p == seq[i - 1] and out[-1] < maxf:
            out[-1] += 1
        else:
            out.append(1)
    assert sum(out) == N
    return out


def per_run(k=1, maxf=16):
    return lambda pads: k * len(_runs(pads, maxf))


def per_frame(k=1):
    return lambda pads: k * N


assert [len(_runs(p, 16)) for p in CASES.values()] == [2, 2, 20] and [len(_runs(p, 8)) for p in CASES.values()] == [3, 4, 20]


# ---- the filters: (make(ctx), bursts' keywords, {profile name: launches(pads)}) ----
class PadParams(C.Structure):
    _fields_ = [("width", C.c_int), ("height", C.c_int), ("x", C.c_int), ("y", C.c_int), ("fill", C.c_int * 3)]


class BlurParams(C.Structure):
    _fields_ = [("amount", C.c_int * 3), ("size", C.c_int * 3)]


class Hqdn3dParams(C.Structure):
    _fields_ = [("coef", (C.c_int16 * 8192) * 6)]


def _pad(depth):
    pp = PadParams(192, 128, 16, 16, (C.c_int * 3)(16 << (depth - 8), 128 << (depth - 8), 128 << (depth - 8)))
    make = lambda ctx: hip._create("hbhip_pad_create", ctx, [C.c_void_p, C.POINTER(PadParams)] + [C.c_int] * 5 + [C.POINTER(C.c_void_p)],
                                   ctx.h, C.byref(pp), W, H, depth, 1, 1)
    return make, dict(depth=depth, out_shape=(128, 192)), {"pad": per_run()}


def _format(depth, out_depth):
    make = lambda ctx: hip._create("hbhip_format_create", ctx, [C.c_void_p] + [C.c_int] * 7 + [C.POINTER(C.c_void_p)],
                                   ctx.h, W, H, depth, out_depth, 1, 1, 0)
    return make, dict(depth=depth, out_depth=out_depth), {"format": per_run()}


def _colorspace(depth):
    return (lambda ctx: hip.colorspace_device_filter(ctx, W, H, BT601, BT709, depth=depth)), dict(depth=depth), {"colorspace": per_run()}


def _rotate(angle, flip, depth):
    make = lambda ctx: hip._create("hbhip_rotate_create", ctx, [C.c_void_p] + [C.c_int] * 7 + [C.POINTER(C.c_void_p)],
                                   ctx.h, angle, flip, W, H, depth, 1, 1)
    kw = dict(depth=depth, out_shape=(W, H)) if angle in (90, 270) else dict(depth=depth)
    return make, kw, {"rotate": per_run() if depth == 8 else per_frame(3)}          # the generic kernel: a plane per launch


def _grayscale(depth):
    make = lambda ctx: hip._create("hbhip_grayscale_create", ctx, [C.c_void_p] + [C.c_double] * 4 + [C.c_int] * 5 + [C.POINTER(C.c_void_p)],
                                   ctx.h, 0.1, -0.2, 0.8, 0.3, W, H, depth, 1, 1)
    return make, dict(depth=depth), ({"monochrome": per_run()} if depth == 8 else
                                     {"monochrome": per_frame(), "monochrome_fill": per_frame(2)})


def _lapsharp(kernel, depth):
    """kernel 1: isolap (3 x 3, the rows kernels); 2: log (5 x 5, the generic kernels) - on every plane"""
    make = lambda ctx: hip.lapsharp_device_filter(ctx, W, H, strength=0.2, kernel=kernel, depth=depth)
    return make, dict(depth=depth), ({"lapsharp_3x3": per_run()} if kernel == 1 else {"lapsharp_5x5": per_frame()})


def _blur(fn, name, amounts, sizes, depth):
    p = BlurParams((C.c_int * 3)(*amounts), (C.c_int * 3)(*sizes))
    make = lambda ctx: hip._create(fn, ctx, [C.c_void_p, C.POINTER(BlurParams)] + [C.c_int] * 5 + [C.POINTER(C.c_void_p)],
                                   ctx.h, C.byref(p), W, H, depth, 1, 1)
    # the rows kernel (8 bits): one launch per distinct step value among the filtered planes, copies ride on the first;
    # the generic kernel (10 bits, every plane filtered here): the planes of a frame in one launch
    steps = {s // 2 for a, s in zip(amounts, sizes) if a}
    return make, dict(depth=depth), {name: per_run(len(steps)) if depth == 8 else per_frame()}


def _unsharp(ysz, csz, depth):
    return _blur("hbhip_unsharp_create", "unsharp_blur_mix", (16384, 98304, 98304), (ysz, csz, csz), depth)


def _chroma_smooth():
    return _blur("hbhip_chroma_smooth_create", "chroma_smooth_blur_mix", (0, 163840, 19660), (7, 7, 7), 8)       # luma copied


def _cropscale(out_w, out_h, crop, depth, counts):
    make = lambda ctx: hip.cropscale_device_filter(ctx, W, H, out_w, out_h, crop=crop, depth=depth)
    return make, dict(depth=depth, out_shape=(out_h, out_w), out_row_bytes=16), counts


def _scale_up(depth):
    return _cropscale(2 * W, 2 * H, (0, 0, 0, 0), depth, {"cropscale_lanczos_fused": per_run()})


def _scale_down(depth):
    return _cropscale(W // 2, H // 2, (0, 0, 0, 0), depth, {"cropscale_lanczos_h": per_run(maxf=8), "cropscale_lanczos_v": per_run(maxf=8)})


def _crop_only(depth):
    """(top, bottom, left, right) = (2, 2, 16, 16): no scale, the three planes are identity copies of the window, a launch
    each; 128 x 92, so that the output rows stay multiples of 16 bytes"""
    return _cropscale(W - 32, H - 4, (2, 2, 16, 16), depth, {"crop_copy": per_frame(3)})


def _hqdn3d(depth):
    orc = ol.OrcHqdn3d(W, H, depth=depth, y_spatial=2, cb_spatial=1.5, cr_spatial=1.5, y_temporal=3, cb_temporal=2.25, cr_temporal=2.25)
    hq = Hqdn3dParams()
    for k in range(6):
        C.memmove(hq.coef[k], orc.coef[k], 8192 * 2)
    make = lambda ctx: hip._create("hbhip_hqdn3d_create", ctx, [C.c_void_p, C.POINTER(Hqdn3dParams)] + [C.c_int] * 5 + [C.POINTER(C.c_void_p)],
                                   ctx.h, C.byref(hq), W, H, depth, 1, 1)
    return make, dict(depth=depth), {"hqdn3d_h": per_run()}


FILTERS = {
    "pad-8": lambda: _pad(8), "pad-10": lambda: _pad(10),
    "format-8to10": lambda: _format(8, 10), "format-10to8": lambda: _format(10, 8),
    "colorspace-8": lambda: _colorspace(8), "colorspace-10": lambda: _colorspace(10),
    "rotate90-8": lambda: _rotate(90, 0, 8), "rotate90-10": lambda: _rotate(90, 0, 10),
    "rotate180hflip-8": lambda: _rotate(180, 1, 8), "rotate180hflip-10": lambda: _rotate(180, 1, 10),
    "grayscale-8": lambda: _grayscale(8), "grayscale-10": lambda: _grayscale(10),
    "lapsharp-isolap-8": lambda: _lapsharp(1, 8), "lapsharp-isolap-10": lambda: _lapsharp(1, 10),
    "lapsharp-log-8": lambda: _lapsharp(2, 8), "lapsharp-log-10": lambda: _lapsharp(2, 10),
    "unsharp-7x7-8": lambda: _unsharp(7, 7, 8), "unsharp-3x9-8": lambda: _unsharp(3, 9, 8), "unsharp-7x7-10": lambda: _unsharp(7, 7, 10),
    "chromasmooth-7-8": _chroma_smooth,
    "scaleup-8": lambda: _scale_up(8), "scaleup-10": lambda: _scale_up(10),
    "scaledown-8": lambda: _scale_down(8), "scaledown-10": lambda: _scale_down(10),
    "croponly-8": lambda: _crop_only(8), "croponly-10": lambda: _crop_only(10),
    "hqdn3d-8": lambda: _hqdn3d(8), "hqdn3d-10": lambda: _hqdn3d(10),
}
# hqdn3d with alternating pitches: every run is one frame and takes the frame-at-a-time kernels; the bytes are held there
NO_COUNT = {("hqdn3d-8", "alternating"), ("hqdn3d-10", "alternating")}


@functools.lru_cache(maxsize=None)
def _frame_by_frame(which):
    """(the input frames, what the filter makes of them one process_dev call per frame), computed once; leave them unchanged"""
    make, kw, _ = FILTERS[which]()
    frames = synth.stream("random", W, H, N, depth=kw["depth"])
    return frames, bursts(make, frames, [1] * N, **kw)


@pytest.mark.parametrize("case", sorted(CASES))
@pytest.mark.parametrize("which", sorted(FILTERS))
def test_twenty_frames_are_cut_by_the_shared_rule(built, which, case):
    make, kw, counts = FILTERS[which]()
    pads = CASES[case]
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
    launches = {name: stats.get(name, (0, 0.0))[0] for name in counts}
    print(f"{which} {case}: launches {launches}, runs of 16 {_runs(pads, 16)}, of 8 {_runs(pads, 8)}")
    if (which, case) not in NO_COUNT:
        assert launches == {name: rule(pads) for name, rule in counts.items()}, stats
