"""The `format` filter's chroma UP-sampling (4:2:0 -> 4:2:2, 4:2:2 -> 4:4:4, 4:2:0 -> 4:4:4) at equal or higher depth
(8 -> 8, 10 -> 10, 12 -> 12, 8 -> 10, 8 -> 12, 10 -> 12 bits), twice:

* upsample_frame(): the INTEGER model - what libavfilter's auto-inserted `scale` computes when the target has more chroma
  samples than the stream: libswscale's general scaler at its default flags (bicubic, B = 0, C = 0.6).  The tables are
  initFilter's (sws_bicubic_table of format_resample_model.py, its x_inc <= 1 << 16 arm: 1 + 4 taps before the trimming),
  the passes hScale8To15 / hScale16To15 and the output stage of the TARGET's depth, yuv2planeX_8 with its flat round term
  (the depth does not fall, so nothing is dithered) or yuv2planeX_10 / _12.  EVERY plane goes through the scaler, luma
  through its identity filters: a copy at equal depth and v << (ddepth - sdepth) above it, in BOTH ranges - the scaler
  replicates no top bits, which is NOT what the unscaled planar copy (format_kernel, oracle/alias_oracle.c:
  orc_format_plane) gives full-range luma at 8 -> 10 bits, (v << 2) | (v >> 6).  PARITY UNPINNED: libswscale is not in
  the reference tree, this file is the definition the GPU tests hold the kernel to (tolerance 0).  It shares no code
  with handbrake_amd/csrc.
* upsample_frame_f64(): the float64 model - a Keys cubic (a = -0.6) at its own width (the ratio is below 1: nothing is
  stretched), weights normalised, edges replicated, one rounding at the end, after the scale by 2 ** (ddepth - sdepth).
  What the integer model is held to (test_format_upsample_cpu.py).

Siting (both models; s source and d target samples of a direction, r = s / d, 1/2 except for an odd target size):
target row j lies at source row (j + 1/2) * r - 1/2, a quarter above source row j / 2 for an even j and a quarter below
it for an odd one (srcPos = dstPos = 128); target column i lies at source column (i + 1/2) * r - 1/4, ON source column
i / 2 for an even i (left-sited chroma whatever chroma_location says: the down-sampling's srcPos 128 / dstPos 64 with
source and target swapped).  The target's chroma planes are -((-luma) >> log2) samples, 2 s or 2 s - 1."""
import numpy as np

from format_resample_model import SUB, frame, keys_cubic, sws_bicubic_table  # noqa: F401  (frame: the tests' inputs)

# Measured by tests/test_format_upsample_cpu.py::test_integer_model_against_float64 (and asserted there, as equalities):
# the largest |integer - float64| by (source depth, target depth) over its inputs - `random`, `progressive`, `bars`, the
# three pairs, 66 x 38 and 67 x 37 - and the largest share of samples of one plane that differ at all, both over the
# INTERIOR of a plane: without the EDGE target samples along each border of a direction that is up-sampled.  1 code value
# is the two roundings; a 12-bit target gets 2 because the vertical coefficients have 12 bits as well, (-346 3572 985
# -115) / 4096 for the cubic's (-0.0844 0.8719 0.2406 -0.0281) * 4096 = (-345.6 3571.2 985.6 -115.2).  The float model
# clips its intermediate here (saturate=True); see ALLOW_MAX_ABS_UNSATURATED for what that hides.
EDGE = 4
ALLOW_MAX_ABS = {(8, 8): 1, (10, 10): 1, (12, 12): 2, (8, 10): 1, (8, 12): 2, (10, 12): 2}
ALLOW_SHARE = 0.2848
# The same over whole planes.  The border is not the cubic with its edge replicated: initFilter's first tap is a division
# in C, which truncates towards zero, so the first rows / columns (negative numerators) start one sample late, lose
# their outermost tap and are normalised without it - target row 2 is (959 3473 -336) / 4096 where the replicated edge
# gives (870 3571 -346).  On full-scale noise that is 3.5 % of full scale
# (test_the_border_is_initfilters_truncated_division).  It is libswscale's arithmetic, and the kernel's.
ALLOW_MAX_ABS_EDGE = {(8, 8): 9, (10, 10): 35, (12, 12): 153, (8, 10): 36, (8, 12): 140, (10, 12): 139}
# `random` and `bars` through BOTH passes (interior) against the float model without its intermediate clip: the 15-bit
# intermediate saturates (the half-sample column (-1229 9421 9421 -1229) / 16384 overshoots full scale by up to 15 %, which
# is clipped at 32767 BEFORE the vertical pass; the float model then clips once at the end).  With the same clip between
# the float model's passes the figures of ALLOW_MAX_ABS hold: test_intermediate_saturation_is_the_only_larger_difference
# measures both.
ALLOW_MAX_ABS_UNSATURATED = {(8, 8): 19, (10, 10): 85, (12, 12): 327, (8, 10): 78, (8, 12): 312, (10, 12): 339}

PAIRS = (("420", "422"), ("422", "444"), ("420", "444"))
STEPS = ((8, 8), (10, 10), (12, 12), (8, 10), (8, 12), (10, 12))
MIN_SAMPLES = 7                                # of a chroma plane in a direction that is up-sampled: initFilter's src - 2 >= 5


def chroma_size(w: int, h: int, layout: str):
    lcw, lch = SUB[layout]
    return -((-w) >> lcw), -((-h) >> lch)


def _dtype(depth: int):
    return np.uint8 if depth == 8 else np.uint16


def _apply(plane, pos, coef, taps, axis):
    """sum over the taps along `axis`, int64"""
    p = plane.astype(np.int64)
    if axis == 0:
        p = p.T
    idx = np.asarray(pos)[:, None] + np.arange(taps)[None, :]
    acc = (p[:, idx] * np.asarray(coef, np.int64)[None, :, :]).sum(axis=2)
    return acc.T if axis == 0 else acc


def scale_plane(plane, sdepth: int, ddepth: int, dw: int, dh: int):
    """one plane of h x w samples through swscale's two passes to dh x dw; a direction whose size stays takes the identity"""
    h, w = plane.shape
    assert dw >= w and dh >= h and ddepth >= sdepth
    if dw != w:
        px, qx, tx = sws_bicubic_table(w, dw, 1 << 14, 64, 128)
        hbuf = np.minimum(_apply(plane, px, qx, tx, 1) >> (7 if sdepth == 8 else sdepth - 1), (1 << 15) - 1)
    else:
        hbuf = plane.astype(np.int64) << (15 - sdepth)
    if dh != h:
        py, qy, ty = sws_bicubic_table(h, dh, 1 << 12, 128, 128)
        acc = _apply(hbuf, py, qy, ty, 0)
    else:
        acc = hbuf << 12
    if ddepth == 8:
        out = (acc + (64 << 12)) >> 19
    else:
        out = (acc + (1 << (26 - ddepth))) >> (27 - ddepth)
    return np.clip(out, 0, (1 << ddepth) - 1).astype(_dtype(ddepth))


def upsample_frame(fr, sdepth: int, ddepth: int, src: str, dst: str):
    """(Y, Cb, Cr) in layout `src` at sdepth bits -> layout `dst` ("420" / "422" / "444") at ddepth bits"""
    (sw, sh), (tw, th) = SUB[src], SUB[dst]
    assert tw <= sw and th <= sh and (tw, th) != (sw, sh)
    h, w = fr[0].shape
    dcw, dch = chroma_size(w, h, dst)
    return (scale_plane(fr[0], sdepth, ddepth, w, h),) + tuple(scale_plane(p, sdepth, ddepth, dcw, dch) for p in fr[1:])


# ---- float64 ------------------------------------------------------------------------------------------------------------
def _upsample_axis_f64(p, dst: int, offset: float, axis: int):
    src = p.shape[axis]
    centre = (np.arange(dst) + 0.5) * (src / dst) - offset
    k = np.floor(centre)[:, None] + np.arange(-1, 3)[None, :]              # the cubic's support of 2 either side
    wgt = keys_cubic(k - centre[:, None])
    wgt /= wgt.sum(axis=1, keepdims=True)
    idx = np.clip(k, 0, src - 1).astype(np.int64)                           # edges replicated
    if axis == 1:
        return (p[:, idx] * wgt[None, :, :]).sum(axis=2)
    return (p.T[:, idx] * wgt[None, :, :]).sum(axis=2).T


def scale_plane_f64(plane, sdepth: int, ddepth: int, dw: int, dh: int, saturate: bool = False):
    """saturate: clip the horizontal result where swscale's 15-bit intermediate does (32767 / 2 ** (15 - sdepth))"""
    h, w = plane.shape
    p = plane.astype(np.float64)
    if dw != w:
        p = _upsample_axis_f64(p, dw, 0.25, 1)
        if saturate:
            p = np.minimum(p, 32767.0 / (1 << (15 - sdepth)))
    if dh != h:
        p = _upsample_axis_f64(p, dh, 0.5, 0)
    p = p * (1 << (ddepth - sdepth))
    return np.clip(np.floor(p + 0.5), 0, (1 << ddepth) - 1).astype(_dtype(ddepth))


def upsample_frame_f64(fr, sdepth: int, ddepth: int, src: str, dst: str, saturate: bool = False):
    h, w = fr[0].shape
    dcw, dch = chroma_size(w, h, dst)
    return (scale_plane_f64(fr[0], sdepth, ddepth, w, h),) + \
        tuple(scale_plane_f64(p, sdepth, ddepth, dcw, dch, saturate) for p in fr[1:])
