"""Planar 8-bit 4:2:0 to a packed 32-bit RGB picture: the definition of handbrake_amd/csrc/rgb_pack.hip, in integers.

PARITY UNPINNED, like the other alias-family models: this restates libswscale's unscaled yuv420p -> bgra / rgba / argb /
abgr path in its C form (yuv2rgb.c: ff_yuv2rgb_c_init_tables + yuv2rgb_c_32) from recollection; FFmpeg is not available to
this tree, so nothing here has been run against it.  The kernel equals THIS file bit for bit (tests/test_format_rgb_gpu.py)
and this file is held to an independent float64 form within 2 codes (tests/test_rgb32_model_cpu.py).

The structure:
  * chroma is taken nearest - one Cb / Cr pair serves its 2 x 2 luma block, chroma_location is not looked at;
  * the coefficients are the 16.16 row {crv, cbu, cgu, cgv} of the frame's matrix; in limited range luma is scaled by
    cy = 65536 * 255 / 219, in full range the chroma coefficients by 224 / 255;
  * each chroma coefficient is divided by cy, so that a chroma term is a WHOLE number of luma steps:
    off(c, inc) = (c * inc >> 16) - (inc >> 9) (the second term is the 128 of the chroma zero), what swscale keeps as
    pointers (table_rV, table_bU) and an integer offset (table_gU + table_gV) into a clipped luma ramp;
  * the ramp: entry k is clip8((cy * (k - luma zero) + 0x8000) >> 16), the luma zero 16 in limited range and 0 in full;
  * alpha is 255.

ONE DEPARTURE from the recollection, forced by the float64 check.  As recalled, swscale places the ramp's limited-range
zero by subtracting 16 OUTPUT codes from a ramp read 326 entries in - the ramp entry of luma code Y is
clip8((cy * (326 + Y) - (400 << 16) + 0x8000) >> 16), whose zero lies at Y = 17.53 and not at 16: 1.78 codes too dark over
the whole ramp (white, Y = 235, as 253).  With that constant the model misses the float64 form by 3 codes in every
channel, a third to a half of all samples by 2 (RAMP_AS_RECALLED below keeps it measurable), so it cannot stand; the ramp here has its zero at 16 exactly.  Full range
is not touched by this (cy = 65536, the two forms are the same ramp).
"""
import numpy as np

ORDERS = ("bgra", "rgba", "argb", "abgr")
# ff_yuv2rgb_coeffs rows {crv, cbu, cgu, cgv} by HB_COLR_MAT_* / H.273 number; 2 (unspecified) is BT.601, as in swscale
_ROW_709, _ROW_601, _ROW_FCC, _ROW_240M, _ROW_2020 = ((117489, 138438, 13975, 34925), (104597, 132201, 25675, 53279),
                                                      (104448, 132798, 24759, 53109), (117579, 136230, 16907, 35559),
                                                      (110013, 140363, 12277, 42626))
COEFFS = {1: _ROW_709, 2: _ROW_601, 4: _ROW_FCC, 5: _ROW_601, 6: _ROW_601, 7: _ROW_240M, 9: _ROW_2020, 10: _ROW_2020}
RAMP_AS_RECALLED = False       # True: the limited-range ramp with swscale's constants as recalled (see above); measurements only


def _cdiv(a, b):
    """C's integer division: towards zero"""
    return abs(a) // b * (1 if a >= 0 else -1)


def constants(matrix, full_range):
    """(cy, yb, crv, cbu, cgu, cgv): the ramp entry k is clip8((yb + k * cy) >> 16), the chroma increments in luma steps"""
    crv, cbu, cgu, cgv = COEFFS[matrix]
    cgu, cgv = -cgu, -cgv
    cy = 1 << 16
    if not full_range:
        cy = (cy * 255) // 219
        yb = -16 * cy
        if RAMP_AS_RECALLED:
            yb = 326 * cy - (384 << 16) - (16 << 16)
    else:
        crv, cbu, cgu, cgv = (_cdiv(c * 224, 255) for c in (crv, cbu, cgu, cgv))
        yb = 0
    crv, cbu, cgu, cgv = (_cdiv(c * (1 << 16) + 0x8000, cy) for c in (crv, cbu, cgu, cgv))
    return cy, yb + 0x8000, crv, cbu, cgu, cgv


def _off(c, inc):
    return ((c * inc) >> 16) - (inc >> 9)


def rgb_planes(y, cb, cr, matrix=1, full_range=False):
    """(R, G, B) uint8 planes of y's size; y is (h, w) with h, w even, cb / cr (h / 2, w / 2)"""
    h, w = y.shape
    assert h % 2 == 0 and w % 2 == 0 and cb.shape == cr.shape == (h // 2, w // 2)
    cy, yb, crv, cbu, cgu, cgv = constants(matrix, full_range)
    u = np.repeat(np.repeat(cb.astype(np.int64), 2, axis=0), 2, axis=1)
    v = np.repeat(np.repeat(cr.astype(np.int64), 2, axis=0), 2, axis=1)
    yy = y.astype(np.int64)

    def ramp(k):
        return np.clip((yb + k * cy) >> 16, 0, 255).astype(np.uint8)
    return ramp(yy + _off(v, crv)), ramp(yy + _off(u, cgu) + _off(v, cgv)), ramp(yy + _off(u, cbu))


def pack(planes, matrix=1, full_range=False, order="bgra"):
    """the packed picture, (h, w, 4) uint8 in memory order, of the three planes of a yuv420p frame"""
    r, g, b = rgb_planes(planes[0], planes[1], planes[2], matrix, full_range)
    a = np.full_like(r, 255)
    return np.stack([{"r": r, "g": g, "b": b, "a": a}[ch] for ch in order], axis=-1)


def all_triples():
    """the 4096 x 4096 4:2:0 picture that holds every (Y, Cb, Cr) once: chroma pair (Cb, Cr) = (i & 255, i >> 8) for chroma
    sample i = row * 2048 + column takes 2^16 pairs x 64 blocks; block number i >> 16 holds the luma codes 4 * (i >> 16) ..
    + 3 in its four places"""
    i = np.arange(2048 * 2048, dtype=np.int64).reshape(2048, 2048)
    cb, cr = (i & 255).astype(np.uint8), ((i >> 8) & 255).astype(np.uint8)
    y = np.empty((4096, 4096), np.uint8)
    base = (4 * (i >> 16)).astype(np.uint8)
    for dy in range(2):
        for dx in range(2):
            y[dy::2, dx::2] = base + (2 * dy + dx)
    return y, cb, cr
