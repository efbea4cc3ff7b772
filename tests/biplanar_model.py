"""NV12 / P010LE in numpy: the repack to and from planar 4:2:0 and the reference's four biplanar compositor functions
(libhb/blend.c), restated with line citations - the oracle of the HIP kernels in csrc/biplanar.hip.  Pinned to the
reference's own hb_blend by tests/test_biplanar_cpu.py.

A biplanar frame is (Y, CbCr): CbCr has ceil(h / 2) rows of interleaved Cb Cr samples.  NV12 is uint8; P010LE is uint16
with its 10 bits in the high end.  The repack has no arithmetic to argue about: NV12 <-> yuv420p is a permutation of
bytes, P010LE <-> yuv420p10le a shift by six (the definition of the format).

blend_bi encodes the two departures the planar kernels have (csrc/blend.hip:16-19): no stray chroma write in front of the
row / plane when a same-subsampling overlay hangs over the left / top edge by an odd amount, and writes stop at the
frame edge."""
import numpy as np


class Declined(Exception):
    """what the HIP drop-in declines (hbhip_blend_create_biplanar: HBHIP_ERR_UNSUPPORTED)"""


def _check(depth, w, h):
    if depth not in (8, 10) or w < 2 or h < 2:
        raise Declined(f"depth {depth}, {w}x{h}")


def split(frame2, depth):
    y, c = frame2
    _check(depth, y.shape[1], y.shape[0])
    sh = 6 if depth == 10 else 0
    return (y >> sh, np.ascontiguousarray(c[:, 0::2]) >> sh, np.ascontiguousarray(c[:, 1::2]) >> sh)


def merge(frame3, depth):
    y, cb, cr = frame3
    _check(depth, y.shape[1], y.shape[0])
    sh = 6 if depth == 10 else 0
    c = np.empty((cb.shape[0], 2 * cb.shape[1]), dtype=y.dtype)
    c[:, 0::2] = cb << sh
    c[:, 1::2] = cr << sh
    return (y << sh, c)


def chroma_coeffs(chroma_location):
    """hb_compute_chroma_smoothing_coefficient, common.c:7054-7091, for 4:2:0: a window into 1 3 9 27 9 3 1"""
    base = [1, 3, 9, 27, 9, 3, 1]
    wx = wy = 4 - 2
    if chroma_location in (1, 3, 5):
        wx += 1
    if 3 <= chroma_location <= 6:              # the switch falls through top / bottom alike
        wy += 1
    return ([(base[i + wx] + base[i + wx + (not wx & 1)]) >> 1 for i in range(2)],
            [(base[i + wy] + base[i + wy + (not wy & 1)]) >> 1 for i in range(2)])


def _same(Y, C, ov, shift, ss):
    """blend8onbi8 :606-691 (shift = ss = 0) / blend8onbi1x :693-786 (alpha << 2, max 1023, samples av_bswap16 = << 8)"""
    left, top, (oy_, ou, ov_, oa) = ov
    H, W = Y.shape
    sh, sw = oy_.shape
    mx = (256 << shift) - 1                                                   # :733
    x0, y0 = max(-left, 0), max(-top, 0)                                      # :618-626 / :712-720
    ww = sw if sw - x0 <= W - left else W - left + x0                         # :628-637 / :722-731
    hh = sh if sh - y0 <= H - top else H - top + y0
    if ww > x0 and hh > y0:                                                   # luma, :640-653 / :736-749
        a = oa[y0:hh, x0:ww].astype(np.uint32) << shift
        s = oy_[y0:hh, x0:ww].astype(np.uint32) << ss
        d = Y[top + y0:top + hh, left + x0:left + ww]
        d[...] = ((d.astype(np.uint32) * (mx - a) + s * a) // mx).astype(Y.dtype)
    # chroma, :668-690 / :763-785 (wshift = hshift = 1: plane 1 is smaller than plane 0 both ways)
    ch, cw = C.shape[0], C.shape[1] // 2
    for yy in range(y0 >> 1, hh >> 1):
        dy = yy + (top >> 1)
        if dy < 0 or dy >= ch:                 # the departures: nothing in front of the plane, nothing past its end
            continue
        for xx in range(x0 >> 1, ww >> 1):
            dx = (left >> 1) + xx
            if dx < 0 or dx >= cw:
                continue
            a = int(oa[yy << 1, xx << 1]) << shift
            for k, src in ((0, ou), (1, ov_)):
                C[dy, 2 * dx + k] = (int(C[dy, 2 * dx + k]) * (mx - a) + (int(src[yy, xx]) << ss) * a) // mx


def _subsample(Y, C, ov, shift, ss, coeffs, bounded):
    """blend_subsample_8onbi8 :330-423 (bounded = False: its inner loops run the whole chroma block, :388-390) /
    blend_subsample_8onbi1x :142-234 (bounded by the overlay's edge, :200-202)"""
    x0, y0, (oy_, ou, ov_, oa) = ov
    H, W = Y.shape
    sh, sw = oy_.shape
    mx = (256 << shift) - 1                                                   # :149
    half = mx >> 1
    x0c, y0c = max(x0 & ~1, 0), max(y0 & ~1, 0)                               # :155-165 / :344-354
    width = sw if sw - x0 <= W - x0 else W                                    # :167-168 / :356-357 (left == x0)
    height = sh if sh - y0 <= H - y0 else H
    ch, cw = C.shape[0], C.shape[1] // 2
    yy = y0c
    while yy - y0 < height and yy >> 1 < ch:                                  # chroma lines, :175-187 / :364-376
        xx = x0c
        while xx - x0 < width and xx >> 1 < cw:
            ox, oy = xx - x0, yy - y0
            acc = [0, 0]
            total = 0
            cur = [int(C[yy >> 1, (xx >> 1) * 2]), int(C[yy >> 1, (xx >> 1) * 2 + 1])]      # :206-207 / :394-395
            for yz in range(2):
                if bounded and oy + yz >= height:
                    break
                for xz in range(2):
                    if bounded and ox + xz >= width:
                        break
                    coeff = coeffs[0][xz] * coeffs[1][yz]                     # :205 / :393
                    res = list(cur)
                    if ox + xz >= 0 and oy + yz >= 0 and ox + xz < width and oy + yz < height:      # :210 / :398
                        a = int(oa[oy + yz, ox + xz]) << shift
                        for k, src in ((0, ou), (1, ov_)):
                            res[k] = (res[k] * (mx - a) + (int(src[oy + yz, ox + xz]) << ss) * a + half) // mx
                        # the luma sample at the same place, :190-194 / :379-382; writes stop at the frame edge
                        if xx + xz < W and yy + yz < H:
                            Y[yy + yz, xx + xz] = (int(Y[yy + yz, xx + xz]) * (mx - a) +
                                                   (int(oy_[oy + yz, ox + xz]) << ss) * a + half) // mx
                    acc[0] += coeff * res[0]
                    acc[1] += coeff * res[1]
                    total += coeff
            if total:                                                          # :226-230 / :414-418
                C[yy >> 1, (xx >> 1) * 2] = ((acc[0] + (total >> 1)) // total) & 0xffff
                C[yy >> 1, (xx >> 1) * 2 + 1] = ((acc[1] + (total >> 1)) // total) & 0xffff
            xx += 2
        yy += 2


def blend_bi(frame2, overlays, depth, chroma_location=1, overlay_shifts=(0, 0)):
    """hb_blend_work :848-873 on an NV12 / P010LE frame: the overlays (x, y, (Y, Cb, Cr, A) uint8) in list order, by the
    function hb_blend_init :815-842 picks for two planes.  overlay_shifts: the overlay's log2 chroma subsampling."""
    Y, C = (np.array(p, copy=True) for p in frame2)
    _check(depth, Y.shape[1], Y.shape[0])
    shift = depth - 8
    ss = 8 if depth == 10 else 0                   # av_bswap16 of an 8-bit value (:193, :747)
    same = tuple(overlay_shifts) == (1, 1)
    if not same and tuple(overlay_shifts) != (0, 0):
        raise Declined("the subsample functions index the overlay's chroma at full resolution (:212-217)")
    coeffs = chroma_coeffs(chroma_location)
    for ov in overlays:
        if same:
            _same(Y, C, ov, shift, ss)
        else:
            _subsample(Y, C, ov, shift, ss, coeffs, bounded=depth != 8)
    return Y, C
