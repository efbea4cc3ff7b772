"""The `format` filter's scaler path at a LOWER target depth (10 -> 8, 12 -> 8, 12 -> 10 bits), with or without fewer
chroma samples, twice:

* scaled_frame(): the INTEGER model - libswscale's general scaler where libavfilter's auto-inserted `scale` takes it
  instead of the unscaled planar copy: whenever the subsampling changes, and whenever the target is semi-planar (the
  planar frame in front of the NV12 / P010LE repack).  EVERY plane runs through it, luma included: the horizontal pass
  or its identity (hScale16To15), then the output stage at the target depth - to 8 bits with the 8 x 8 ordered dither
  ff_dither_8x8_128 (yuv2plane1_8 / yuv2planeX_8; Cr reads the table three columns on), to 10 bits with a flat half
  (yuv2plane1_10 / yuv2planeX_10).  Recalled from libswscale's C paths, PARITY UNPINNED: libswscale is not in the
  reference tree, this file is the definition the GPU tests hold the kernel to (tolerance 0).  The tables, the siting
  and the nominal frame are format_resample_model's; no code is shared with handbrake_amd/csrc.
* scaled_frame_f64(): the float64 model - format_resample_model's Keys cubic with the 15-bit saturation between the
  passes, divided by 2 ** (sd - dd), NOT rounded.  What the integer model is held to (test_format_scaled_cpu.py).

No range conversion on this path: the source and the target range are the same, and both take the same arithmetic."""
import numpy as np

from format_resample_model import SUB, _apply, _resample_axis_f64, frame, resample_frame, sws_bicubic_table  # noqa: F401

# libswscale's ff_dither_8x8_128 (rows 0 .. 7): a permutation of the even numbers 0 .. 126
DITHER_8X8_128 = np.array([
    [36, 68, 60, 92, 34, 66, 58, 90],
    [100, 4, 124, 28, 98, 2, 122, 26],
    [52, 84, 44, 76, 50, 82, 42, 74],
    [116, 20, 108, 12, 114, 18, 106, 10],
    [32, 64, 56, 88, 38, 70, 62, 94],
    [96, 0, 120, 24, 102, 6, 126, 30],
    [48, 80, 40, 72, 54, 86, 46, 78],
    [112, 16, 104, 8, 118, 22, 110, 14],
], np.int64)
CR_OFFSET = 3                                 # the C path's constant: Y and Cb read column x, Cr column x + 3

STEPS = ((10, 8), (12, 8), (12, 10))          # source depth, target depth
# every pair of layouts the scaled form takes: the three of format_resample_model and the depth-only one
PAIRS = (("422", "420"), ("444", "422"), ("444", "420"), ("420", "420"))

# Measured by tests/test_format_scaled_cpu.py::test_integer_model_against_float64 (and asserted there): the largest
# |integer - unrounded float64| by step over format_resample_model.frame's six kinds, the four pairs, at 66 x 38, 67 x 37
# and 130 x 70, luma and chroma apart, in code values of the target.
# Luma is the identity and its figure is exact: floor(x + d / 128) with d in 0 .. 126 is at most max(f, 1 - f) off for a
# fractional part f, and x has 2 (10 -> 8) or 4 (12 -> 8) fractional bits: 3/4 and 15/16; the flat half of 12 -> 10: 1/2.
# Chroma adds the truncated 15-bit intermediate and the rounded coefficients (format_resample_model: the 12-bit vertical
# row at phase 1/2 is off the cubic by 4.8 / 4096 in absolute sum, the 14-bit horizontal ones by a quarter of that); the
# largest of all is 4:2:2 -> 4:2:0 on full-scale noise at 130 x 70.  CEILING is what those terms add up to at worst
# (output stage + 1.25 * 4.8 / 4096 of full scale + one 15-bit step): no measurement may come near it.
ALLOW_LUMA = {(10, 8): 0.75, (12, 8): 0.9375, (12, 10): 0.5}
ALLOW_CHROMA = {(10, 8): 1.01, (12, 8): 1.04, (12, 10): 0.91}
CEILING = {(sd, dd): ALLOW_LUMA[sd, dd] + (1.25 * 4.8 / 4096 + 1.0 / 32768) * (1 << dd) for sd, dd in ALLOW_LUMA}
# the largest share of one plane's samples further than 1/2 from the exact value (what a single rounding would never be).
# A sample with fractional part f is rounded up in about f of the dither's 64 cells, and is then further than 1/2 when
# f < 1/2 (else when rounded down): min(f, 1 - f) <= 1/2 of the cells.  12 -> 10 has no dither: only the tables' error.
ALLOW_SHARE = 0.5


def _dtype(depth: int):
    return np.uint8 if depth == 8 else np.uint16


def dither_plane(h: int, w: int, off: int):
    """the round term of every sample of an h x w OUTPUT plane"""
    return DITHER_8X8_128[(np.arange(h) & 7)[:, None], ((np.arange(w) + off) & 7)[None, :]]


def scaled_plane(plane, sd: int, dd: int, down_w: bool, down_h: bool, off: int):
    """one plane through swscale's two passes at source depth sd (10 / 12), out at dd < sd; a pass that does not
    resample is the identity filter (one tap)"""
    assert sd in (10, 12) and dd in (8, 10) and dd < sd
    h, w = plane.shape
    dw, dh = (-(-w // 2) if down_w else w), (-(-h // 2) if down_h else h)
    if down_w:
        px, qx, tx = sws_bicubic_table(w, dw, 1 << 14, 128, 64)
        hbuf = np.minimum(_apply(plane, px, qx, tx, 1) >> (sd - 1), (1 << 15) - 1)       # hScale16To15
    else:
        hbuf = plane.astype(np.int64) << (15 - sd)
    if down_h:
        py, qy, ty = sws_bicubic_table(h, dh, 1 << 12, 128, 128)
        acc = _apply(hbuf, py, qy, ty, 0)
        if dd == 8:
            out = ((dither_plane(dh, dw, off) << 12) + acc) >> 19                          # yuv2planeX_8
        else:
            out = (acc + (1 << 16)) >> 17                                                   # yuv2planeX_10
    elif dd == 8:
        out = (hbuf + dither_plane(dh, dw, off)) >> 7                                       # yuv2plane1_8
    else:
        out = (hbuf + 16) >> 5                                                              # yuv2plane1_10
    return np.clip(out, 0, (1 << dd) - 1).astype(_dtype(dd))


def scaled_frame(frame, sd: int, dd: int, src: str, dst: str):
    """(Y, Cb, Cr) of depth sd in layout `src` -> depth dd in layout `dst` ("444" / "422" / "420")"""
    if sd == dd:
        return resample_frame(frame, sd, src, dst)
    (sw, sh), (tw, th) = SUB[src], SUB[dst]
    assert tw >= sw and th >= sh
    return (scaled_plane(frame[0], sd, dd, False, False, 0),
            scaled_plane(frame[1], sd, dd, tw > sw, th > sh, 0),
            scaled_plane(frame[2], sd, dd, tw > sw, th > sh, CR_OFFSET))


# ---- float64 ------------------------------------------------------------------------------------------------------------
def scaled_plane_f64(plane, sd: int, dd: int, down_w: bool, down_h: bool):
    """float64 code values of depth dd, not rounded; clipped to the target's range, and between the passes where the
    15-bit intermediate saturates"""
    p = plane.astype(np.float64)
    if down_w:
        p = _resample_axis_f64(p, -(-plane.shape[1] // 2), 0.25, 1)
    p = np.minimum(p, 32767.0 / (1 << (15 - sd)))
    if down_h:
        p = _resample_axis_f64(p, -(-plane.shape[0] // 2), 0.5, 0)
    return np.clip(p / (1 << (sd - dd)), 0.0, float((1 << dd) - 1))


def scaled_frame_f64(frame, sd: int, dd: int, src: str, dst: str):
    (sw, sh), (tw, th) = SUB[src], SUB[dst]
    return (scaled_plane_f64(frame[0], sd, dd, False, False),) + \
        tuple(scaled_plane_f64(p, sd, dd, tw > sw, th > sh) for p in frame[1:])
