"""Comb detect, mask by mask: the content, sizes and configurations shared by tests/test_comb_masks_cpu.py (which keeps
this list from going vacuous, with the oracle alone) and tests/test_comb_masks_gpu.py (which holds the kernels of
csrc/comb_detect.hip to the oracle's masks cell by cell).  numpy only.

Every content function is a deterministic function of its arguments and returns n luma planes (uint8, or uint16 for
depth > 8) with amplitudes scaled by << (depth - 8)."""
import numpy as np


# ---------------------------------------------------------------------------------------------------------- content
def _dtype(depth):
    return np.uint8 if depth == 8 else np.uint16


def _parity(w, h, t):
    """+1 / -1 by row parity, flipping every frame (so that both motion tests of the detector pass)"""
    return np.where((np.arange(h)[:, None] + t) % 2 == 0, 1, -1) * np.ones((1, w), np.int64)


def comb_field(w, h, n, seed, depth=8):
    """128 +- 50 by row parity (flipping per frame), uniform noise -3 .. 3 on every pixel, then 10 % of the pixels of
    each frame, chosen at random, set to 128: every neighbour count of the erode / dilate passes occurs."""
    rs = np.random.RandomState(seed)
    up = depth - 8
    out = []
    for t in range(n):
        v = 128 + 50 * _parity(w, h, t) + rs.randint(-3, 4, size=(h, w))
        v[rs.random_sample((h, w)) < 0.10] = 128
        out.append((v << up).astype(_dtype(depth)))
    return out


def comb_threshold(w, h, n, seed, depth=8, spatial_thresh=3):
    """A horizontal ramp from 0 to the maximum value, displaced by +-a by row parity (flipping per frame) with a drawn
    per pixel from 0 .. 2 * spatial_thresh + 2 (in 8-bit steps, scaled with the depth), clipped: the spatial and motion
    differences fall on both sides of every threshold, for the gamma metric at every slope of the table and at its two
    clipped ends.  (Spatial metric 0 wants |v - d1| > 15 and finds next to nothing here: comb_field is its content.)"""
    rs = np.random.RandomState(seed)
    up = depth - 8
    maxv = (1 << depth) - 1
    ramp = np.rint(np.arange(w) * (maxv / max(w - 1, 1))).astype(np.int64)[None, :]
    out = []
    for t in range(n):
        a = rs.randint(0, ((2 * spatial_thresh + 2) << up) + 1, size=(h, w))
        out.append(np.clip(ramp + _parity(w, h, t) * a, 0, maxv).astype(_dtype(depth)))
    return out


def comb_patch(w, h, n, seed, depth=8, rect=(0, 0, 0, 0)):
    """Flat 128 with comb_field's pattern inside rect = (x0, y0, x1, y1), x1 / y1 exclusive."""
    x0, y0, x1, y1 = rect
    out = []
    for f in comb_field(w, h, n, seed, depth):
        v = np.full((h, w), 128 << (depth - 8), _dtype(depth))
        v[y0:y1, x0:x1] = f[y0:y1, x0:x1]
        out.append(v)
    return out


# ------------------------------------------------------------------------------------------------------------ sizes
# Around the smallest supported frame (4 x 5), the partial dword of the four-pixels-a-lane detector, the 64-cell mask
# tiles and their 4-cell apron, widths whose mask stride equals the width (64, 128, 192, 320: column `width` is the next
# row's column 0), the 256-pixel detector workgroup (258), and the 4-row and 16-row tiles.  Nothing larger is needed.
WIDTHS = [4, 5, 6, 7, 8, 17, 62, 63, 64, 65, 66, 67, 68, 126, 128, 130, 192, 258, 320]
HEIGHTS = [5, 6, 7, 8, 16, 17, 18, 19, 20, 21, 32, 33, 35]


def sizes():
    """(w, h): every width at heights 21 and 35, every height at widths 64 and 67"""
    s = [(w, h) for w in WIDTHS for h in (21, 35)]
    s += [(w, h) for w in (64, 67) for h in HEIGHTS if (w, h) not in s]
    return s


def heights_of(w):
    return [h for ww, h in sizes() if ww == w]


DEEP_WIDTHS, DEEP_HEIGHTS = [5, 63, 64, 67, 130], [7, 21]          # depths 10 and 12


def mask_stride(w):
    return (w + 63) // 64 * 64


# --------------------------------------------------------------------------------------------------- configurations
def _cfg(name, first, deep=False, **par):
    return dict(name=name, first=first, deep=deep, par=par)


# `par` are the keyword arguments of both oracle_lib.OrcComb and hip.CombDetectDevice.  `first` names the content of the
# first classifications a case makes (the last is always comb_field, see case_lumas); `deep` marks what also runs at
# depths 10 and 12.  Filter mode 0 is the reference's quirk: its only pass writes the intermediate mask and the score
# reads a filtered mask that nothing wrote.
CONFIGS = [
    _cfg("gamma_f2_16x16", "threshold", True, mode=3, motion_thresh=1, spatial_thresh=3, filter_mode=2, block_thresh=40),
    _cfg("gamma_f1_8x8", "threshold", True, mode=3, motion_thresh=1, spatial_thresh=3, filter_mode=1, block_thresh=20,
         block_width=8, block_height=8),
    _cfg("gamma_f0_4x4", "threshold", False, mode=3, motion_thresh=2, spatial_thresh=1, filter_mode=0, block_thresh=6,
         block_width=4, block_height=4),
    _cfg("gamma_plain_32x8", "threshold", True, mode=1, motion_thresh=1, spatial_thresh=1, block_thresh=60,
         block_width=32, block_height=8),
    _cfg("gamma_f2_mt0_32x8", "threshold", False, mode=3, motion_thresh=0, spatial_thresh=3, filter_mode=2, block_thresh=60,
         block_width=32, block_height=8),
]
_BLOCKS = [(16, 16, 40), (8, 8, 20), (4, 4, 6), (32, 8, 60)]
for _m in (0, 1, 2):
    for _mt in (0, 2):
        for _filt in (True, False):
            _bw, _bh, _bt = _BLOCKS[len(CONFIGS) % 4]
            CONFIGS.append(_cfg(f"m{_m}_mt{_mt}_{'f2' if _filt else 'plain'}_{_bw}x{_bh}", "field" if _m == 0 else "threshold",
                                (_m, _mt, _filt) in ((2, 2, True), (1, 2, False), (0, 0, True)),
                                mode=2 if _filt else 0, spatial_metric=_m, motion_thresh=_mt, spatial_thresh=3, filter_mode=2,
                                block_thresh=_bt, block_width=_bw, block_height=_bh))
DEEP_CONFIGS = [c for c in CONFIGS if c["deep"]]


def filtered(cfg):
    return bool(cfg["par"]["mode"] & 2)


# At the smallest frames an edge is a handful of cells (one cell, for a column of a frame five rows high), which a
# draw's 10 % of flat pixels can leave without an expected one.  The sizes below (at width 4, where the passes can set
# one column: the size / configuration pairs) take a later draw, the first one at which every configuration's expected
# masks reach every edge (tests/test_comb_masks_cpu.py asserts that they do).
SEED_BUMP = {(5, 21): 143, (5, 35): 108, (6, 21): 5, (6, 35): 75, (7, 21): 11, (7, 35): 10, (8, 21): 18, (8, 35): 2,
             (66, 21): 1, (67, 21): 1, (128, 21): 1, (130, 35): 1, (192, 21): 1, (64, 5): 40, (64, 6): 1, (64, 8): 24,
             (64, 16): 2, (64, 18): 1, (67, 5): 6, (67, 8): 8, (67, 16): 1, (67, 17): 2, (67, 18): 1, (67, 19): 1,
             (4, 21, "gamma_f2_16x16"): 4, (4, 21, "gamma_f1_8x8"): 1, (4, 21, "m0_mt0_f2_8x8"): 49,
             (4, 21, "m0_mt2_f2_32x8"): 128, (4, 21, "m1_mt2_f2_32x8"): 2, (4, 35, "gamma_f2_16x16"): 1,
             (4, 35, "m0_mt0_f2_8x8"): 237, (4, 35, "m0_mt2_f2_32x8"): 25}


def seed_of(w, h, cfg):
    return 1000 * w + 10 * h + CONFIGS.index(cfg) + 1000000 * SEED_BUMP.get((w, h, cfg["name"]), SEED_BUMP.get((w, h), 0))


def case_lumas(w, h, cfg, depth=8):
    """The classifications a case makes on one instance, one after the other: [((prev, cur, next), force)].  The first
    repeats its first frame, as the first frame of a stream does, so no pixel passes a motion test and (with a motion
    threshold) only force_exhaustive fills the mask; comb_threshold then comes once more with motion and without force
    (the motion differences at the thresholds); the last is comb_field with motion in every pixel, without force - the
    one whose expected masks the CPU test holds to the edges."""
    s = seed_of(w, h, cfg)
    b = comb_field(w, h, 3, s + 5, depth)
    if cfg["first"] == "threshold":
        a = comb_threshold(w, h, 3, s, depth, cfg["par"]["spatial_thresh"])
        return [((a[0], a[0], a[1]), True), ((a[0], a[1], a[2]), False), ((b[0], b[1], b[2]), False)]
    a = comb_field(w, h, 2, s, depth)
    return [((a[0], a[0], a[1]), True), ((b[0], b[1], b[2]), False)]


# ----------------------------------------------------------------------------------------- knife-edge block scores
def knife_cases():
    """(w, h, par, rect, expected verdicts): comb_patch rectangles covering exactly one block.  With S that block's
    score, block thresholds S - 1, S and 2 * S + 2 give HEAVY, LIGHT, NONE - except for the block in the column that
    `x < width - block_width` leaves unscored when the width is a multiple of the block width: NONE whatever the
    threshold.  16 x 16 blocks on a filtered mask (the score kernel's dword path), 8 x 8 on the detector's mask (its
    r[-1] & r[0] & r[1] path)."""
    out = []
    h = 35
    for bw, bh, par in [(16, 16, dict(mode=3, motion_thresh=1, spatial_thresh=3, filter_mode=2)),
                        (8, 8, dict(mode=0, spatial_metric=2, motion_thresh=2, spatial_thresh=3))]:
        par = dict(par, block_width=bw, block_height=bh)
        for w in (64, 67, 130):
            last_x = (-(-(w - bw) // bw) - 1) * bw                   # the last x of `for x = 0; x < w - bw; x += bw`
            last_y = (h // bh - 1) * bh
            blocks = [("first", 0, 0), ("last_col", last_x, 0), ("last_row", bw, last_y)]
            if w % bw == 0:
                blocks.append(("unscored", w - bw, bh if last_y >= bh else 0))
            for name, x, y in blocks:
                out.append(dict(name=f"{bw}x{bh}_w{w}_{name}", w=w, h=h, par=par, rect=(x, y, x + bw, y + bh),
                                want=(0, 0, 0) if name == "unscored" else (2, 1, 0)))
    return out


def block_score(mask, rect, width, filt):
    """One block's score from a mask (height x stride), as check_filtered_combing_mask / check_combing_mask sum it
    (comb_detect.c:221-276, 384-454)"""
    x0, y0, x1, y1 = rect
    m = mask.astype(np.int64)
    if filt:
        return int(m[y0:y1, x0:x1].sum())
    s = 0
    for x in range(x0, x1):
        c = m[y0:y1, x]
        if x == 0:
            s += int((c & m[y0:y1, 1]).sum())
        elif x == width - 1:
            s += int((m[y0:y1, x - 1] & c).sum())
        else:
            s += int((m[y0:y1, x - 1] & c & m[y0:y1, x + 1]).sum())
    return s
