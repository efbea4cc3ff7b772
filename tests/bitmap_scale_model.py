"""What scale_subtitle (rendersub.c:242-377) makes of a decoded bitmap subtitle, for tests/test_bitmap_scale_cpu.py and
tests/test_bitmap_scale_gpu.py: the size and position arithmetic in Python floats (the reference's doubles), the placement
rule, and the four planes through the oracle's restatement of libswscale's lanczos + accurate_rnd
(oracle/alias_oracle.c:orc_cropscale_plane_sws, chroma_h = 0: on a 4:4:4 picture every plane takes the luma filter).

A subtitle here is (x, y, (Y, Cb, Cr, A), (window_width, window_height)): the bitmap, its place on its canvas, the canvas.
"""
import ctypes as C

import numpy as np

from handbrake_amd import synth
import oracle_lib as ol


def factor(fw, fh, window):
    """the one factor both axes take (:249-266): the larger of the two, 1 without a canvas"""
    ww, wh = window
    if ww <= 0 or wh <= 0:
        return 1.0
    return max(fw / ww, fh / wh)


def is_scaled(f):
    return abs(f - 1) > 0.01                                               # :267


def geometry(fw, fh, x, y, w, h, window):
    """(x, y, width, height) of the bitmap at the frame's scale (:273-283), before placement"""
    f = factor(fw, fh, window)
    if not is_scaled(f):
        return x, y, w, h
    return int(x * f), int(y * f), int(w * f), int(h * f)


def place(fw, fh, x, y, w, h, crop=(0, 0, 0, 0)):
    """:311-375: out of the cropped zones (crop = top, bottom, left, right), 2 % of the height (at most 20 rows) clear of the
    top and bottom and 20 columns of the sides, centred where it does not fit.  C's `/` truncates: int(a / b)."""
    margin = min(int((fh - crop[0] - crop[1]) * 2 / 100), 20)
    if h > fh - crop[0] - crop[1] - 2 * margin:
        top = crop[0] + int((fh - crop[0] - crop[1] - h) / 2)
    elif y < crop[0] + margin:
        top = crop[0] + margin
    elif y > fh - crop[1] - margin - h:
        top = fh - crop[1] - margin - h
    else:
        top = y
    if w > fw - crop[2] - crop[3] - 40:
        left = crop[2] + int((fw - crop[2] - crop[3] - w) / 2)
    elif x < crop[2] + 20:
        left = crop[2] + 20
    elif x > fw - crop[3] - 20 - w:
        left = fw - crop[3] - 20 - w
    else:
        left = x
    return left, top


def scale_planes(planes, dw, dh):
    fn = ol.oracle().orc_cropscale_plane_sws
    fn.restype = None
    fn.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int]
    out = []
    for p in planes:
        p = np.ascontiguousarray(p, dtype=np.uint8)
        h, w = p.shape
        dst = np.zeros((dh, dw), np.uint8)
        fn(p.ctypes.data, p.strides[0], 0, 0, w, h, dst.ctypes.data, dst.strides[0], dw, dh, 0)
        out.append(dst)
    return tuple(out)


def render(fw, fh, sub, crop=(0, 0, 0, 0)):
    """the overlay the compositor gets for `sub` on a fw x fh frame: (x, y, (Y, Cb, Cr, A))"""
    x, y, planes, window = sub
    h, w = planes[0].shape
    sx, sy, sw, sh = geometry(fw, fh, x, y, w, h, window)
    if (sw, sh) != (w, h):
        planes = scale_planes(planes, sw, sh)
    else:
        planes = tuple(np.ascontiguousarray(p).copy() for p in planes)
    left, top = place(fw, fh, sx, sy, sw, sh, crop)
    return left, top, planes


def random_sub(w, h, x, y, window, seed=1):
    """a w x h bitmap of LCG noise with a ragged alpha: transparent, opaque and soft areas, edges that are not straight"""
    v = (synth.lcg_stream(synth.frame_seed(0x5b, seed), 4 * w * h) >> np.uint32(24)).astype(np.uint8)
    yy, cb, cr, a = (v[k * w * h:(k + 1) * w * h].reshape(h, w).copy() for k in range(4))
    gx, gy = np.arange(w)[None, :], np.arange(h)[:, None]
    a[(gx // 5 + gy // 3) % 4 == 0] = 0
    a[(gx // 7 + gy // 4) % 5 == 1] = 255
    a[(gx + 2 * gy) % 11 == 0] = 0
    return x, y, (yy, cb, cr, a), window


def frame(fw, fh, fmt="420", depth=8, seed=3):
    """a progressive synthetic frame in planar 4:2:0 / 4:4:4 at 8 or 10 bits"""
    return synth.picture("progressive", fw, fh, seed, depth=depth, chroma={"420": "2x2", "444": "1x1"}[fmt])
