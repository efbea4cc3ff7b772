"""The `format` filter's scaler path to FEWER chroma samples at a HIGHER depth (8 -> 10, 8 -> 12, 10 -> 12 bits; 4:2:2 ->
4:2:0, 4:4:4 -> 4:2:2, 4:4:4 -> 4:2:0), twice:

* deepen_frame(): the INTEGER model - libswscale's general scaler, which libavfilter's auto-inserted `scale` takes for
  every plane as soon as the subsampling changes.  The horizontal pass or its identity by the SOURCE depth (hScale8To15:
  sum >> 7, the identity v << 7; hScale16To15: sum >> (sd - 1), the identity v << (15 - sd); saturated at 32767, a negative
  intermediate is kept), then the output stage by the TARGET depth, which has more than 8 bits: no dither and no offset
  for Cr, the flat half of the shift - one tap (yuv2plane1_10 / _12): (t + (1 << (14 - dd))) >> (15 - dd); several
  (yuv2planeX_10 / _12): (sum + (1 << (26 - dd))) >> (27 - dd) - clipped to [0, 2 ** dd - 1].  Luma takes the identity and
  the one-tap stage: v << (dd - sd), no top-bit replication, so full scale does not map to full scale (255 -> 1020).
  Recalled from libswscale's C paths, PARITY UNPINNED: libswscale is not in the reference tree, this file is the
  definition the GPU tests hold the kernel to (tolerance 0).  The tables, the siting and the nominal frame are
  format_resample_model's; no code is shared with handbrake_amd/csrc.
* deepen_frame_f64(): the float64 model - format_resample_model's Keys cubic with the 15-bit saturation between the
  passes, multiplied by 2 ** (dd - sd), NOT rounded.  What the integer model is held to (test_format_deepen_cpu.py).

No range conversion on this path: the source and the target range are the same, and both take the same arithmetic."""
import numpy as np

from format_resample_model import PAIRS, SUB, _apply, _resample_axis_f64, frame, sws_bicubic_table  # noqa: F401

STEPS = ((8, 10), (8, 12), (10, 12))          # source depth, target depth

# Measured by tests/test_format_deepen_cpu.py::test_integer_model_against_float64 (and asserted there): the largest
# |integer - unrounded float64| in chroma by step over format_resample_model.frame's six kinds, the three pairs, at
# 66 x 38, 67 x 37 and 130 x 70, in code values of the target.  (Luma differs by 0: v << (dd - sd) is exact.)
# What adds up: the output stage's rounding (half a target step), the rounded coefficients (format_resample_model: the
# 12-bit vertical row at phase 1/2 is off the cubic by 4.8 / 4096 in absolute sum, the 14-bit horizontal ones by a quarter
# of that) on samples of at most the SOURCE's full scale - (2 ** sd - 1) * 2 ** (dd - sd) target values, just under
# 2 ** dd - and the truncated 15-bit intermediate, one step of 2 ** dd / 32768.  CEILING is those terms at their worst,
# the form of format_scaled_model.CEILING with a half for its output stage; no measurement may come near it.  The largest
# are 4:4:4 -> 4:2:0 on `rows` at 67 x 37 (8 -> 10) and full-scale noise through 4:2:2 -> 4:2:0's vertical pass (to 12 bits).
ALLOW_CHROMA = {(8, 10): 0.89, (8, 12): 2.03, (10, 12): 2.07}
CEILING = {(sd, dd): 0.5 + (1.25 * 4.8 / 4096 + 1.0 / 32768) * (1 << dd) for sd, dd in STEPS}


def deepen_plane(plane, sd: int, dd: int, down_w: bool, down_h: bool):
    """one plane through swscale's two passes at source depth sd, out at dd > sd (uint16); a pass that does not resample
    is the identity filter (one tap)"""
    assert (sd, dd) in STEPS
    h, w = plane.shape
    dw, dh = (-(-w // 2) if down_w else w), (-(-h // 2) if down_h else h)
    if down_w:
        px, qx, tx = sws_bicubic_table(w, dw, 1 << 14, 128, 64)
        hbuf = np.minimum(_apply(plane, px, qx, tx, 1) >> (7 if sd == 8 else sd - 1), (1 << 15) - 1)   # hScale8To15 / 16To15
    else:
        hbuf = plane.astype(np.int64) << (7 if sd == 8 else 15 - sd)
    if down_h:
        py, qy, ty = sws_bicubic_table(h, dh, 1 << 12, 128, 128)
        out = (_apply(hbuf, py, qy, ty, 0) + (1 << (26 - dd))) >> (27 - dd)                             # yuv2planeX_10 / _12
    else:
        out = (hbuf + (1 << (14 - dd))) >> (15 - dd)                                                    # yuv2plane1_10 / _12
    return np.clip(out, 0, (1 << dd) - 1).astype(np.uint16)


def deepen_frame(frame, sd: int, dd: int, src: str, dst: str):
    """(Y, Cb, Cr) of depth sd in layout `src` -> depth dd > sd in layout `dst` ("444" / "422" / "420"), fewer chroma
    samples in one direction at least"""
    (sw, sh), (tw, th) = SUB[src], SUB[dst]
    assert tw >= sw and th >= sh and (tw, th) != (sw, sh)
    return (deepen_plane(frame[0], sd, dd, False, False),) + \
        tuple(deepen_plane(p, sd, dd, tw > sw, th > sh) for p in frame[1:])


# ---- float64 ------------------------------------------------------------------------------------------------------------
def deepen_plane_f64(plane, sd: int, dd: int, down_w: bool, down_h: bool):
    """float64 code values of depth dd, not rounded; clipped to the target's range, and between the passes where the
    15-bit intermediate saturates"""
    p = plane.astype(np.float64)
    if down_w:
        p = _resample_axis_f64(p, -(-plane.shape[1] // 2), 0.25, 1)
    p = np.minimum(p, 32767.0 / (1 << (15 - sd)))
    if down_h:
        p = _resample_axis_f64(p, -(-plane.shape[0] // 2), 0.5, 0)
    return np.clip(p * (1 << (dd - sd)), 0.0, float((1 << dd) - 1))


def deepen_frame_f64(frame, sd: int, dd: int, src: str, dst: str):
    (sw, sh), (tw, th) = SUB[src], SUB[dst]
    return (deepen_plane_f64(frame[0], sd, dd, False, False),) + \
        tuple(deepen_plane_f64(p, sd, dd, tw > sw, th > sh) for p in frame[1:])
