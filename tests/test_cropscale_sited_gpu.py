"""GPU: crop/scale with the chroma where the stream sites it (AVCHROMA_LOC_* 2, 3, 4, 6), through the drop-in
(init->chroma_location) and through the C ABI (hbhip_cropscale_create_sited), bit for bit against the committed
restatement of zimg's fixed point (oracle/alias_oracle.c: orc_cropscale_plane_fx / _fx16) called with the shifts of
tests/chroma_siting_model.py per plane.  Luma never moves.  The sizes reach the fused up-scaler (whose window checks now
run on vertically shifted tables too), the two-pass kernels with a ratio of its own per axis, a plane whose width is kept
(no horizontal shift, a vertical one), and a frame so small that every tap is reflected."""
import math

import numpy as np
import pytest

from handbrake_amd import hbrt, hip
import chroma_siting_model as csm
import oracle_lib as ol
import sited_lib as sl

pytestmark = pytest.mark.gpu

FORMATS = [("2x2", 8), ("2x2", 10), ("2x1", 10)]
LOCATIONS = [2, 3, 4, 6]
SIZES = [(128, 96, 256, 192), (256, 192, 128, 96), (192, 128, 128, 96), (64, 48, 64, 96), (16, 8, 32, 16)]
TW, TH, MAXR, SRC_DW8, SRC_DW16 = 256, 16, 24, 68, 138      # alias.hip: SU_TW, SU_TH, SU_MAXR, SU_SRC_DW, SW_SRC_DW


def source(w, h, sub, depth, seed=0):
    lw, lh = ol.SUBSAMPLING[sub]
    rng = np.random.default_rng(1000 * seed + w + h + depth)
    dt = np.uint8 if depth == 8 else np.uint16
    return tuple(rng.integers(0, 1 << depth, s).astype(dt) for s in ((h, w), (h >> lh, w >> lw), (h >> lh, w >> lw)))


def planes_of(w, h, ow, oh, sub, loc):
    """(src_w, src_h, dst_w, dst_h, shift_x, shift_y) of the three planes"""
    lw, lh = ol.SUBSAMPLING[sub]
    sx, sy = csm.shifts(loc, lw, lh, w, ow, h, oh)
    return [(w, h, ow, oh, 0.0, 0.0)] + [(w >> lw, h >> lh, ow >> lw, oh >> lh, sx, sy)] * 2


def fused_expected(w, h, ow, oh, sub, depth, loc):
    """CropScaleFilter::setup's decision, restated: six taps either way (no direction shrinks) and the source window of
    every 256 x 16 tile inside the fused kernel's LDS frame, on the first-tap tables shifted as the location asks"""
    for sw, sh, dw, dh, sx, sy in planes_of(w, h, ow, oh, sub, loc):
        if (sw, sh, sx, sy) == (dw, dh, 0.0, 0.0):
            continue                                             # copied
        if dw < sw or dh < sh:
            return False
        bx = [math.floor((i + 0.5) * sw / dw + sx - 2.5) for i in range(dw)]
        by = [math.floor((i + 0.5) * sh / dh + sy - 2.5) for i in range(dh)]
        for x0 in range(0, dw, TW):
            last = bx[min(x0 + TW, dw) - 1] + 5
            if depth == 8 and (last - (bx[x0] & ~3)) // 4 + 1 > SRC_DW8 - 2:
                return False
            if depth > 8 and (last - (bx[x0] & ~1)) // 2 + 2 > SRC_DW16:
                return False
        if any(by[min(y0 + TH, dh) - 1] + 5 - by[y0] + 1 > MAXR for y0 in range(0, dh, TH)):
            return False
    return True


def compare(got, want, what):
    for c in range(3):
        np.testing.assert_array_equal(np.asarray(got[c]), want[c], err_msg=f"{what}: plane {c}")


_left = {}


def drop_in(fr, ow, oh, sub, depth, loc):
    hbrt.set_source_chroma_location(loc)
    try:
        out = hbrt.run_stream(hip.filters(), [("hb_filter_crop_scale_hip", f"width={ow}:height={oh}")], [fr],
                              pix_fmt=hbrt.PIX_FMT[(sub, depth)])
    finally:
        hbrt.set_source_chroma_location()
    assert len(out) == 1
    return [np.asarray(p) for p in out[0].planes]


@pytest.mark.parametrize("loc", LOCATIONS)
@pytest.mark.parametrize("sub,depth", FORMATS, ids=[f"{s}-{d}" for s, d in FORMATS])
@pytest.mark.parametrize("w,h,ow,oh", SIZES, ids=[f"{a}x{b}to{c}x{d}" for a, b, c, d in SIZES])
def test_drop_in_follows_the_location(built, w, h, ow, oh, sub, depth, loc):
    fr = source(w, h, sub, depth)
    got = drop_in(fr, ow, oh, sub, depth, loc)
    compare(got, sl.cropscale_frame_at(fr, ow, oh, loc, depth, sub), f"location {loc}")
    key = (w, h, ow, oh, sub, depth)
    if key not in _left:
        _left[key] = drop_in(fr, ow, oh, sub, depth, 1)
        compare(_left[key], ol.orc_cropscale_frame(fr, ow, oh, depth=depth, sub=sub), "location 1")
    np.testing.assert_array_equal(got[0], _left[key][0], err_msg="luma moved with the chroma location")
    lw, lh = ol.SUBSAMPLING[sub]
    if csm.shifts(loc, lw, lh, w, ow, h, oh) != csm.shifts(1, lw, lh, w, ow, h, oh):
        assert not np.array_equal(got[1], _left[key][1]), "chroma is where location 1 puts it"


@pytest.fixture(scope="module")
def ctx():
    c = hip.Ctx(0)
    c.profile(True)
    yield c
    c.profile(False)
    c.close()


@pytest.mark.parametrize("loc", LOCATIONS)
@pytest.mark.parametrize("sub,depth", FORMATS, ids=[f"{s}-{d}" for s, d in FORMATS])
@pytest.mark.parametrize("w,h,ow,oh", SIZES, ids=[f"{a}x{b}to{c}x{d}" for a, b, c, d in SIZES])
def test_c_abi_follows_the_location_on_the_kernels_setup_chose(built, ctx, w, h, ow, oh, sub, depth, loc):
    lw, lh = ol.SUBSAMPLING[sub]
    fr = source(w, h, sub, depth, seed=1)
    flt = hip.cropscale_device_filter(ctx, w, h, ow, oh, depth=depth, log2_cw=lw, log2_ch=lh, chroma_location=loc)
    try:
        ctx.profile_reset()
        shapes = [(oh, ow), (oh >> lh, ow >> lw), (oh >> lh, ow >> lw)]
        got = sl.process_dev(flt, ctx, [fr], shapes, depth)[0]
        names = {k for k, v in ctx.profile_stats().items() if v[0] > 0 and k.startswith("cropscale")}
    finally:
        flt.close()
    compare(got, sl.cropscale_frame_at(fr, ow, oh, loc, depth, sub), f"location {loc}")
    if fused_expected(w, h, ow, oh, sub, depth, loc):
        assert names == {"cropscale_lanczos_fused"}, names
    else:
        assert names == {"cropscale_lanczos_h", "cropscale_lanczos_v"}, names
    if (w, h, ow, oh) == (128, 96, 256, 192):
        assert "cropscale_lanczos_fused" in names                # the 2 x up-scale is the fused kernel's at every location


@pytest.mark.parametrize("sub,depth", [("2x2", 8), ("2x2", 10)])
def test_burst_of_three_frames(built, ctx, sub, depth):
    """three frames of distinct content through one hbhip_filter_process_dev, 2 x up (fused) and 2 -> 1 (two passes)"""
    lw, lh = ol.SUBSAMPLING[sub]
    for w, h, ow, oh in ((128, 96, 256, 192), (256, 192, 128, 96)):
        frames = [source(w, h, sub, depth, seed=s) for s in (2, 3, 4)]
        flt = hip.cropscale_device_filter(ctx, w, h, ow, oh, depth=depth, log2_cw=lw, log2_ch=lh, chroma_location=3)
        try:
            got = sl.process_dev(flt, ctx, frames, [(oh, ow), (oh >> lh, ow >> lw), (oh >> lh, ow >> lw)], depth)
        finally:
            flt.close()
        for t, fr in enumerate(frames):
            compare(got[t], sl.cropscale_frame_at(fr, ow, oh, 3, depth, sub), f"frame {t} of {w}x{h}")


def test_locations_0_and_1_are_the_call_without_one(built, ctx):
    w, h, ow, oh = 128, 96, 256, 192
    fr = source(w, h, "2x2", 8, seed=5)
    shapes = [(oh, ow), (oh // 2, ow // 2), (oh // 2, ow // 2)]
    outs = []
    for loc in (None, 0, 1):
        flt = hip.cropscale_device_filter(ctx, w, h, ow, oh, chroma_location=loc)
        try:
            outs.append(sl.process_dev(flt, ctx, [fr], shapes, 8)[0])
        finally:
            flt.close()
    for o in outs[1:]:
        compare(o, outs[0], "location 0 / 1 against hbhip_cropscale_create")
    compare(outs[0], ol.orc_cropscale_frame(fr, ow, oh), "hbhip_cropscale_create")


@pytest.mark.parametrize("loc", [-1, 7])
def test_a_location_outside_the_enum_is_an_argument_error(built, ctx, loc):
    with pytest.raises(hip.HipError):
        hip.cropscale_device_filter(ctx, 128, 96, 256, 192, chroma_location=loc)
    with pytest.raises(hip.HipError):
        hip.colorspace_device_filter(ctx, 128, 96, (6, 6, 6, 1), (1, 1, 1, 1), chroma_location=loc)
