"""Full-range content and the shapes for the deinterlacers of csrc/decomb.hip (decomb's yadif / blend / cubic, FFmpeg-style
yadif and bwdif), shared by tests/test_deint_fullrange_cpu.py and tests/test_deint_fullrange_gpu.py.  No GPU code here.

The `interlaced` model every other deinterlacer test runs on keeps luma within 57 .. 173 of 255: no clamp binds, the
diagonal search meets two bar levels, bwdif's operands stay small.  The three contents here use the whole range of the
depth, 0 .. (1 << depth) - 1 and never more - above that the reference's crop table is overrun and nothing is defined:

  random  uniform samples (synth's model, at the depth)
  cells   cells of 5 columns x 1 row, each 0 or max: five is coprime to the four samples a thread owns, so cell edges fall
          at every phase of a thread's dword, and rows are independent, so every pattern of five vertically adjacent rows
          over {0, max} occurs - blend, cubic and bwdif's intra filter overshoot both ways
  steps   areas of 0 and max separated by edges of slope +-1 and +-2 that move three samples a field (top field first, as
          synth.interlaced_frame), +-2 noise clipped to the range so that scores are not all ties: what the +-1 / +-2
          cascade of the diagonal search is for

reach() counts how often a stream gets to each of the things the contents are there for; REACH_FLOOR is what every count
has to come to, over the three contents of one shape and depth taken together."""
import numpy as np

from handbrake_amd import synth

CONTENTS = ("random", "cells", "steps")
DEPTHS = (8, 10, 12)
N_FRAMES = 5

# luma sizes: the smallest that still reach each edge of the kernels' geometry
SHAPES = [
    (32, 32),       # HandBrake's minimum; chroma 16 x 16
    (35, 33),       # luma width = 3 mod 4; chroma 18 x 17: width = 2 mod 4 and an odd height - both ragged store() tails
    (37, 22),       # luma width = 1 mod 4; chroma 19 (= 3 mod 4) x 11
    (70, 10),       # chroma 35 x 5: almost every row a vertical_edge row of decomb and an edge row of bwdif
    (322, 182),     # several workgroups; chroma 161 (= 1 mod 4)
]

# the modes test_oracle_vs_ref.py::test_decomb_matches_reference pins on the interlaced model
DECOMB_MODES = (1, 2, 4, 5, 7, 3, 23, 21, 39, 55)
COMBED = [2, 1, 0, 2, 1]                 # HB_COMB_*: the selective modes take their blend branch and their copy branch

REACH_FLOOR = 32
REACH_KEYS = ("blend<0", "blend>max", "cubic<0", "cubic>max", "intra<0", "intra>max", "j=-2", "j=-1", "j=0", "j=+1", "j=+2")
# (shape, depth) -> keys that cannot come to REACH_FLOOR there, with the reason.  Empty: every shape has a luma plane of
# ten rows or more, which is enough for all of them (the five-row chroma planes of (70, 10) have no row with rows y +- 3
# inside the plane, so they add nothing to the cubic and intra counts; its luma plane does).
REACH_EXCEPTIONS = {}


def _plane_dims(w, h):
    cw, ch = (w + 1) // 2, (h + 1) // 2
    return [(h, w), (ch, cw), (ch, cw)]


def _dtype(depth):
    return np.uint8 if depth == 8 else np.uint16


def _cells_frame(w, h, t, depth):
    maxv = (1 << depth) - 1
    planes = []
    for c, (ph, pw) in enumerate(_plane_dims(w, h)):
        nx = (pw + 4) // 5
        bits = synth.lcg_stream(synth.frame_seed(0x21 + c, t), ph * nx) >> np.uint32(31)       # the LCG's best bit
        cells = bits.reshape(ph, nx).astype(_dtype(depth)) * _dtype(depth)(maxv)
        planes.append(np.ascontiguousarray(np.repeat(cells, 5, axis=1)[:, :pw]))
    return tuple(planes)


def _steps_frame(w, h, t, depth):
    maxv = (1 << depth) - 1
    slopes = np.array([1, -1, 2, -2], dtype=np.int64)
    planes = []
    for c, (ph, pw) in enumerate(_plane_dims(w, h)):
        x = np.arange(pw, dtype=np.int64)[None, :]
        y = np.arange(ph, dtype=np.int64)[:, None]
        ft = 2 * t + (y & 1)                                         # even rows at field time 2 t, odd rows at 2 t + 1
        s = slopes[(x // 12 + y // 6 + t + c) % 4]                   # areas of 12 x 6 samples, each with one slope
        level = np.where(((x + s * y + 3 * ft + 7000) // 7) & 1, maxv, 0)
        r = synth.lcg_stream(synth.frame_seed(0x31 + c, t), ph * pw) >> np.uint32(16)
        noise = (r.astype(np.int64) % 5 - 2).reshape(ph, pw)
        planes.append(np.clip(level + noise, 0, maxv).astype(_dtype(depth)))
    return tuple(planes)


def stretch(frames, sub, w, h):
    """4:2:0 frames with the chroma planes stretched to 4:2:2 ("2x1") or 4:4:4 ("1x1") by sample repetition, as
    test_formats_gpu.frames_for does."""
    if sub == "2x2":
        return frames
    out = []
    for y, u, v in frames:
        if sub == "2x1":
            u, v = np.repeat(u, 2, axis=0)[:h], np.repeat(v, 2, axis=0)[:h]
        else:
            u, v = (np.repeat(np.repeat(p, 2, axis=0), 2, axis=1)[:h, :w] for p in (u, v))
        out.append((y, np.ascontiguousarray(u), np.ascontiguousarray(v)))
    return out


def random(w, h, n, depth, sub="2x2"):
    return stretch(synth.stream("random", w, h, n, depth=depth), sub, w, h)


def cells(w, h, n, depth, sub="2x2"):
    return stretch([_cells_frame(w, h, t, depth) for t in range(n)], sub, w, h)


def steps(w, h, n, depth, sub="2x2"):
    return stretch([_steps_frame(w, h, t, depth) for t in range(n)], sub, w, h)


_GEN = {"random": random, "cells": cells, "steps": steps}
_CACHE = {}


def content(name, w, h, depth, n=N_FRAMES, sub="2x2"):
    """The stream, made once per process and shared (read only) by every test that asks for it."""
    key = (name, w, h, depth, n, sub)
    if key not in _CACHE:
        frames = _GEN[name](w, h, n, depth, sub)
        for fr in frames:
            for p in fr:
                p.setflags(write=False)
        _CACHE[key] = frames
    return _CACHE[key]


def reach(frames, depth):
    """A census of what the stream gets the line filters to, over every plane of every frame and every row that a field
    of either parity rebuilds, wherever the rows (and columns) the expression reads lie inside the plane:
      blend   (-a + 2 b + 6 c + 2 d - e) >> 3 over rows y - 2 .. y + 2, unclipped: how often < 0 and > max
      cubic   (-3 a + 23 b + 23 c - 3 d) / 40 over rows y - 3, y - 1, y + 1, y + 3 (C division): the same
      intra   bwdif's (5077 (c1 + e1) - 981 (c3 + e3)) >> 13 over the same rows: the same
      j       which slope wins the score cascade of the diagonal search between rows y - 1 and y + 1 at 3 <= x <= w - 4:
              best = slope(0) - 1, then j = -1 and (only behind it) -2, then +1 and (only behind it) +2, each taken when
              strictly lower than the best so far.
    Returns {key: count} over REACH_KEYS."""
    maxv = (1 << depth) - 1
    out = dict.fromkeys(REACH_KEYS, 0)

    def both(name, v):
        out[name + "<0"] += int((v < 0).sum())
        out[name + ">max"] += int((v > maxv).sum())

    for fr in frames:
        for plane in fr:
            p = plane.astype(np.int64)
            h, w = p.shape
            assert p.min() >= 0 and p.max() <= maxv, "a sample outside the depth: the reference is undefined there"
            if h >= 5:
                both("blend", (-p[:-4] + 2 * p[1:-3] + 6 * p[2:-2] + 2 * p[3:-1] - p[4:]) >> 3)
            if h >= 7:
                a, b, c, d = p[:-6], p[2:-4], p[4:-2], p[6:]
                cub = -3 * a + 23 * b + 23 * c - 3 * d
                both("cubic", np.sign(cub) * (np.abs(cub) // 40))                     # C division truncates
                both("intra", (5077 * (b + c) - 981 * (a + d)) >> 13)
            if h >= 3 and w >= 7:
                up, dn = p[:-2], p[2:]

                def slope(j):
                    return sum(np.abs(up[:, 3 + i + j: w - 3 + i + j] - dn[:, 3 + i - j: w - 3 + i - j]) for i in (-1, 0, 1))

                best = slope(0) - 1
                win = np.zeros(best.shape, dtype=np.int64)
                for side in (-1, 1):
                    s1 = slope(side)
                    t1 = s1 < best
                    best = np.where(t1, s1, best)
                    win = np.where(t1, side, win)
                    s2 = slope(2 * side)
                    t2 = t1 & (s2 < best)
                    best = np.where(t2, s2, best)
                    win = np.where(t2, 2 * side, win)
                for j in (-2, -1, 0, 1, 2):
                    out["j=%+d" % j if j else "j=0"] += int((win == j).sum())
    return out


def blend_extremes(frames):
    """(lowest, highest) unclipped blend value of the stream.  On `cells` they are (-2 max) >> 3 and (10 max) >> 3: at 12
    bits -1024 and 5118, the first and the last entry of the reference's crop table that a blend can index."""
    lo, hi = 0, 0
    for fr in frames:
        for plane in fr:
            p = plane.astype(np.int64)
            if p.shape[0] >= 5:
                v = (-p[:-4] + 2 * p[1:-3] + 6 * p[2:-2] + 2 * p[3:-1] - p[4:]) >> 3
                lo, hi = min(lo, int(v.min())), max(hi, int(v.max()))
    return lo, hi


def reach_of_shape(w, h, depth):
    """(total, per content) reach counts of the three contents at one shape and depth."""
    per = {name: reach(content(name, w, h, depth), depth) for name in CONTENTS}
    total = {k: sum(per[name][k] for name in CONTENTS) for k in REACH_KEYS}
    return total, per
