"""FFmpeg's `bm3d` as libhb's bm3d.c configures it (sigma only, every other option at its default, so group size 1), written
from the definition of DESIGN.md §4.18 in numpy - independent of handbrake_amd/csrc/bm3d.hip.

Per plane: a 16 x 16 block at every origin 0, 4, 8, ... of each axis, the last origin clamped to size - 16; an unnormalised
separable DCT-II of the raw samples; a hard threshold; the matching DCT-III; each sample accumulates num += w * estimate and
den += w with w = 1 / retained; out = clip(rint(num / den)).

bm3d_plane() is the reference: float64 throughout.  bm3d_plane_f32() does the same in float32, block after block in raster
order - the "reference arithmetic" the allowance of a float32 implementation is measured with (ALLOW_* below)."""
import numpy as np

# ---- what is recalled of FFmpeg's vf_bm3d, in one place (handbrake_amd/csrc/bm3d.hip: BM_*) ---------------------------------
RECALLED = dict(block=16, bstep=4, group=1, range=9, mstep=1, thmse=0.0, hdthr=2.7, estim=0, planes=7)   # estim 0 = basic
SIGMA_MAX = 99999.9                 # sigma: a float option, 0 .. 99999.9
B, STEP = RECALLED["block"], RECALLED["bstep"]

# ---- the allowance of a float32 implementation against bm3d_plane() --------------------------------------------------------
# Measured by tests/test_bm3d_cpu.py::test_float32_allowance: bm3d_plane_f32 against bm3d_plane on every shape, depth and
# content of bm3d_cases.py at sigma 1, 3 and 6 (135 frames, 405 planes).  43 planes differed at all, none at 8 bits beyond
# one sample; the largest |difference| was 1 code value and the largest share of differing samples in one plane 26 / 1440
# (the 36 x 40 Cb plane of 72 x 40 4:2:2, 10 bits, random, sigma 6: one coefficient of one block falls on the other side of
# its threshold in float32, which shifts that block's estimate by a fraction of a code value and so moves the samples of
# the block whose quotient num / den lay next to a half; the other planes differ in one to five samples of that kind).
ALLOW_MAX_ABS = 1
ALLOW_SHARE = 26 / 1440
GPU_SHARE_FACTOR = 2                # the kernel sums in another order than the raster model; both are float32


class Declined(Exception):
    pass


def resolve(settings, depth):
    """settings -> sigma as FFmpeg holds it (bm3d.c: a double, default 1, handed on as "%g" text; FFmpeg: a float option)
    and the three thresholds; Declined where FFmpeg's graph would fail"""
    if depth not in (8, 10, 12):
        raise Declined(f"depth {depth}")
    sigma = 1.0
    for tok in (settings or "").split(":"):
        if tok.startswith("sigma=") and len(tok) > 6:
            try:
                sigma = float(tok[6:])
            except ValueError:
                pass
    d = float("%g" % sigma)
    if not (0.0 <= d <= SIGMA_MAX):
        raise Declined(f"sigma {d}")
    s = np.float32(d)
    return dict(sigma=s, thr=thresholds(s, depth))


def thresholds(sigma, depth):
    """thr[z] for a coefficient with z of its two frequencies zero: t0 * sqrt2^(1 + z), the 1 for the group index 0"""
    r2 = float(np.sqrt(np.float64(2.0)))
    t0 = float(np.float32(RECALLED["hdthr"])) * float(np.float32(sigma)) * r2 * B * B * float(1 << (depth - 8)) / 255.0
    return np.array([t0 * r2, t0 * 2.0, t0 * (2.0 * r2)]).astype(np.float32)


def dct_table():
    """C[k][n] = cos(pi (2n + 1) k / 32) in double, rounded once to float"""
    k = np.arange(B, dtype=np.float64)[:, None]
    n = np.arange(B, dtype=np.float64)[None, :]
    return np.cos(np.pi * ((2 * n + 1) * k) / 32.0).astype(np.float32)


def origins(size):
    if size < B:
        raise Declined(f"a plane of {size} samples holds no block")
    out = list(range(0, size - B + 1, STEP))
    if out[-1] != size - B:
        out.append(size - B)
    return out


def _matrices(dtype):
    c = dct_table().astype(dtype)                                    # forward: Y = C X C^T
    scale = np.full(B, 2.0 / B, dtype=dtype)
    scale[0] = 1.0 / B
    d = (c * scale[:, None]).T.copy()                                # inverse: X = D Y D^T, D[n][k] = C[k][n] * (k ? 2 : 1) / 16
    zeros = (np.arange(B)[:, None] == 0).astype(int) + (np.arange(B)[None, :] == 0).astype(int)
    return c, d, zeros


def bm3d_plane(plane, thr, depth, want_den=False):
    """float64, all blocks at once"""
    h, w = plane.shape
    c, d, zeros = _matrices(np.float64)
    t = thr.astype(np.float64)[zeros]
    ys, xs = origins(h), origins(w)
    src = plane.astype(np.float64)
    win = np.lib.stride_tricks.sliding_window_view(src, (B, B))[np.ix_(ys, xs)]          # [by][bx][r][c]
    coef = np.matmul(np.matmul(c, win), c.T)
    keep = np.abs(coef) > t
    coef = np.where(keep, coef, 0.0)
    retained = keep.sum(axis=(2, 3))
    wgt = np.where(retained > 0, 1.0 / np.maximum(retained, 1), 1.0)
    est = np.matmul(np.matmul(d, coef), d.T)
    num = np.zeros((h, w))
    den = np.zeros((h, w))
    for i, y0 in enumerate(ys):
        for j, x0 in enumerate(xs):
            num[y0:y0 + B, x0:x0 + B] += wgt[i, j] * est[i, j]
            den[y0:y0 + B, x0:x0 + B] += wgt[i, j]
    if want_den:
        return den
    out = np.clip(np.rint(num / den), 0, (1 << depth) - 1)
    return out.astype(plane.dtype)


def bm3d_plane_f32(plane, thr, depth):
    """float32 throughout; the blocks add to num / den one after the other in raster order"""
    h, w = plane.shape
    c, d, zeros = _matrices(np.float32)
    t = thr.astype(np.float32)[zeros]
    ys, xs = origins(h), origins(w)
    win = np.lib.stride_tricks.sliding_window_view(plane.astype(np.float32), (B, B))[np.ix_(ys, xs)]
    coef = np.matmul(np.matmul(c, win), c.T)
    keep = np.abs(coef) > t
    coef = np.where(keep, coef, np.float32(0.0))
    retained = keep.sum(axis=(2, 3))
    wgt = np.where(retained > 0, np.float32(1.0) / np.maximum(retained, 1).astype(np.float32), np.float32(1.0))
    est = np.matmul(np.matmul(d, coef), d.T)
    num = np.zeros((h, w), dtype=np.float32)
    den = np.zeros((h, w), dtype=np.float32)
    for i, y0 in enumerate(ys):
        for j, x0 in enumerate(xs):
            num[y0:y0 + B, x0:x0 + B] += wgt[i, j] * est[i, j]
            den[y0:y0 + B, x0:x0 + B] += wgt[i, j]
    assert coef.dtype == est.dtype == wgt.dtype == num.dtype == den.dtype == np.float32
    out = np.clip(np.rint(num / den), 0, (1 << depth) - 1)
    return out.astype(plane.dtype)


def bm3d_frame(planes, settings, depth=8, f32=False):
    thr = resolve(settings, depth)["thr"]
    fn = bm3d_plane_f32 if f32 else bm3d_plane
    return tuple(fn(np.ascontiguousarray(p), thr, depth) for p in planes)              # planes = 7: all three
