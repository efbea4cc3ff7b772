"""Where a stream's chroma samples sit, and what a resize has to do about it - the test side's own statement, written
from the geometry and not from handbrake_amd/csrc/chroma_siting.h.

Coordinates: a luma sample i of a direction covers [i, i + 1) and sits at i + 0.5.  A chroma sample j of a direction
subsampled by two covers [2j, 2j + 2); centred it sits at 2j + 1, co-sited with the first luma sample (left / top) at
2j + 0.5, with the second (bottom) at 2j + 1.5: `offset` below, in luma samples from the centre, is 0, -0.5, +0.5.

A resize of that direction by dst / src (luma sizes) keeps the picture's edges where they are, so a destination chroma
sample at luma coordinate X_d = 2 j_d + 1 + offset shows the source picture at X_s = X_d * src / dst, which is source
chroma index (X_s - 1 - offset) / 2 - in the resampler's own convention, where index j has its centre at j + 0.5,
the position (X_s - offset) / 2.  Without siting the resampler reads at (j_d + 0.5) * src / dst = (X_d - offset) / 2 *
src / dst.  The difference is the shift:  offset / 2 * (src / dst - 1)  =  -offset * 0.5 * (1 - src / dst).
AVCHROMA_LOC_* numbers: 0 unspecified (taken as left), 1 left, 2 center, 3 topleft, 4 top, 5 bottomleft, 6 bottom."""
from fractions import Fraction

LOCATIONS = range(7)
#          location: (horizontal offset, vertical offset) in luma samples from the centre of the chroma sample's cell
OFFSETS = {0: (-0.5, 0.0), 1: (-0.5, 0.0), 2: (0.0, 0.0), 3: (-0.5, -0.5), 4: (0.0, -0.5), 5: (-0.5, 0.5), 6: (0.0, 0.5)}


def offsets(loc, log2_cw=1, log2_ch=1):
    """(horizontal, vertical) offset; a direction that is not subsampled has none"""
    ox, oy = OFFSETS[loc]
    return (ox if log2_cw else 0.0, oy if log2_ch else 0.0)


def shift(offset, src, dst):
    """the resampler's shift, in source chroma samples, of one direction (exact in Fractions, then one rounding)"""
    return float(Fraction(offset) / 2 * (Fraction(src, dst) - 1))


def shifts(loc, log2_cw, log2_ch, src_w, dst_w, src_h, dst_h):
    ox, oy = offsets(loc, log2_cw, log2_ch)
    return shift(ox, src_w, dst_w), shift(oy, src_h, dst_h)


def luma_position(j, offset):
    """luma coordinate of chroma sample j of a direction subsampled by two"""
    return 2 * j + 1 + offset


def colour_forms(loc):
    """(columns centred, rows co-sited) of the colour conversion's up- and down-sampling; vertical bottom stays centred"""
    ox, oy = OFFSETS[loc]
    return ox == 0.0, oy < 0
