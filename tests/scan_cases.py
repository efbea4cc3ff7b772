"""Pictures for the title-scan tests (tests/test_scan_cpu.py, tests/test_scan_gpu.py): the contents the border walk and
hb_detect_comb can go wrong on, for any even size >= 8 x 8.  Everything is generated from fixed seeds.

SHAPES: 64 x 48 (border = 0, h4 = 12), 100 x 240 (border = 2, w4 = 25, a width that is no multiple of 8),
322 x 200 (chroma 161 x 100: an odd chroma width, border = 2); 1920 x 1080 once, for the launch shape of a real preview."""
import numpy as np

from handbrake_amd import synth
import scan_model as sm

SHAPES = [(64, 48), (100, 240), (322, 200)]
BIG = (1920, 1080)


def _bright(w, h, seed=7):
    """a busy picture nobody takes for a border: luma 60 .. 219, chroma around 128"""
    r = np.random.default_rng(seed)
    y = r.integers(60, 220, (h, w), dtype=np.uint8)
    c = [r.integers(118, 139, (h // 2, w // 2), dtype=np.uint8) for _ in range(2)]
    return [y, c[0], c[1]]


def _dark_noise(shape, seed):
    """what a matte looks like: 16 .. 22"""
    return np.random.default_rng(seed).integers(16, 23, shape, dtype=np.uint8)


def no_border(w, h):
    return _bright(w, h)


def all_black(w, h):
    p = _bright(w, h)
    p[0][:] = 16
    return p


def letterbox(w, h, line21=True, seed=11):
    """matte of h / 8 rows at the top and h / 6 at the bottom; line21: a bright row 0 and a bright last row inside the
    `border` region (for border = 0 there is no such region: the picture then has no matte as far as the walk can tell)"""
    p = _bright(w, h)
    t, b = h // 8, h // 6
    p[0][:t] = _dark_noise((t, w), seed)
    p[0][h - b:] = _dark_noise((b, w), seed + 1)
    if line21:
        p[0][0, ::2] = 235
        p[0][h - 1, 1::3] = 200
    return p


def border_rows(w, h, top_bright=None, bottom_bright=None):
    """the `top <= border` branch: row `border` is picture, rows [0, border) are dark but for the one named (None: all dark
    -> 0; k: -> k).  Same at the bottom, counted from the last row."""
    p = _bright(w, h)
    border = h // 100
    if border:
        p[0][:border] = _dark_noise((border, w), 21)
        p[0][h - border:] = _dark_noise((border, w), 22)
    if top_bright is not None and 0 <= top_bright < border:
        p[0][top_bright, w // 3] = 180
    if bottom_bright is not None and 0 <= bottom_bright < border:
        p[0][h - 1 - bottom_bright, w // 2] = 90
    return p


def pillarbox(w, h, matte=False):
    """dark columns: w / 10 on the left, w / 7 on the right.  A bright row 0 crosses them: with a matte on top the column
    range starts below it and the pillars count; without one row 0 is part of every column and none is dark."""
    p = letterbox(w, h, line21=False) if matte else _bright(w, h)
    l, r = max(w // 10, 1), max(w // 7, 2)
    t = h // 8 if matte else 0
    b = h // 6 if matte else 0
    p[0][t:h - b, :l] = _dark_noise((h - b - t, l), 31)
    p[0][t:h - b, w - r:] = _dark_noise((h - b - t, r), 32)
    if h // 100:                                          # (border = 0: row 0 is the walk's first row, leave it)
        p[0][0, :] = 235
    return p


def average_31_32(w, h):
    """rows [0, h / 8) sum to 32 w - 1 (average 31: dark), row h / 8 to 32 w (average 32: not); the bottom rows are all 31"""
    p = _bright(w, h)
    t = h // 8
    p[0][:t + 1] = 32
    p[0][:t, w // 2] = 31
    p[0][h - h // 5:] = 31
    return p


def below_16(w, h):
    """a matte of 0 / 33 samples: clamped they are 16 / 33, average 24, every one within 16; unclamped the 33s would be 17
    off an average of 16.  The pillars the same."""
    p = _bright(w, h)
    t = h // 8
    p[0][:t, 0::2] = 0
    p[0][:t, 1::2] = 33
    p[0][h - t:, :] = 5
    p[0][t:h - t, :max(w // 9, 1)] = np.array([0, 33], np.uint8)[(np.arange(h - 2 * t) & 1)][:, None]
    return p


def sixteen_seventeen(w, h):
    """dark rows of 16s with one sample exactly 16 off the average (32: still dark) down to row h / 8, which has one 17 off
    (33: not dark); the bottom the same with the last h / 7 rows; one such column pair on the left"""
    p = _bright(w, h)
    t, b = h // 8, h // 7
    p[0][:t + 1] = 16
    p[0][:t, 5] = 32
    p[0][t, 5] = 33
    p[0][h - b - 1:] = 16
    p[0][h - b:, w - 3] = 32
    p[0][h - b - 1, w - 3] = 33
    p[0][t + 1:h - b - 1, :3] = 16
    p[0][(t + h - b) // 2, 0:2] = 32
    p[0][(t + h - b) // 2, 2] = 33
    return p


def interlaced(w, h):
    return [np.ascontiguousarray(a) for a in synth.interlaced_frame(w, h, 1)]


def progressive(w, h):
    return [np.ascontiguousarray(a) for a in synth.progressive_frame(w, h, 1)]


def chroma_only_combed(w, h, params=sm.DEFAULT_PARAMS):
    """flat luma and Cr, Cb combed in its first m columns - m the smallest for which the picture counts as combed only
    because Cb's counts are still in the counters when Cr's score is taken (hb.c never resets cc_1 / cc_2)"""
    p = [np.full((h, w), 100, np.uint8), np.full((h // 2, w // 2), 128, np.uint8), np.full((h // 2, w // 2), 128, np.uint8)]
    for m in range(1, w // 2 + 1):
        p[1][0::2, m - 1] = 90
        p[1][1::2, m - 1] = 170
        carried = sm.reduced_detect_comb(p, 0, params, carry=True)
        alone = sm.reduced_detect_comb(p, 0, params, carry=False)
        if carried[2] and not alone[2]:
            return p
        if alone[2]:
            break
    raise AssertionError(f"no chroma-only case at {w}x{h}")


CROP_CASES = {
    "no_border": no_border,
    "all_black": all_black,
    "letterbox_line21": letterbox,
    "letterbox_plain": lambda w, h: letterbox(w, h, line21=False),
    "border_rows_dark": border_rows,
    "border_row_bright": lambda w, h: border_rows(w, h, top_bright=h // 100 - 1, bottom_bright=h // 100 - 1),
    "pillarbox": pillarbox,
    "pillarbox_matte": lambda w, h: pillarbox(w, h, matte=True),
    "average_31_32": average_31_32,
    "below_16": below_16,
    "sixteen_seventeen": sixteen_seventeen,
}
COMB_CASES = {
    "interlaced": interlaced,
    "progressive": progressive,
    "chroma_only_combed": chroma_only_combed,
}
CASES = dict(CROP_CASES, **COMB_CASES)

# pic_flags with and without bit 16 under two pairs of sensitivity triples: scan.c's, and one whose prog_* triple is blind
FLAG_PARAMS = [(0, sm.DEFAULT_PARAMS), (16, sm.DEFAULT_PARAMS), (0, (12, 20, 3, 2, 120, 900)), (16 | 2, (12, 20, 3, 2, 120, 900))]
