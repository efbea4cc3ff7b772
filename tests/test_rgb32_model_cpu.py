"""tests/rgb32_model.py - the integer definition of the packed-RGB download (csrc/rgb_pack.hip) - held to an independent
float64 form built from colour_model's matrices: exact Kr / Kb, limited or full range in, full range out, nearest chroma,
round half up, clip.

The cap is 2 codes a channel, and it follows from the model's structure, not from what it measures: each chroma term is
rounded to a whole luma step, at most 255 / 219 / 2 = 0.58 of a code in limited range (green has two such terms), and the
final rounding adds 0.5.  The measured maxima and the shares of samples at 1 and at 2 are in DESIGN.md 4.6.11."""
import numpy as np
import pytest

import colour_model as cm
import rgb32_model as rm

CAP = 2


def float_form(y, cb, cr, matrix, full_range):
    """(R, G, B) uint8 planes"""
    m = cm.ycbcr_to_rgb(matrix)
    u = np.repeat(np.repeat(cb, 2, axis=0), 2, axis=1).astype(np.float64) - 128.0
    v = np.repeat(np.repeat(cr, 2, axis=0), 2, axis=1).astype(np.float64) - 128.0
    if full_range:
        yy, u, v = y.astype(np.float64) / 255.0, u / 255.0, v / 255.0
    else:
        yy, u, v = (y.astype(np.float64) - 16.0) / 219.0, u / 224.0, v / 224.0
    return tuple(np.clip(np.floor(255.0 * (m[c, 0] * yy + m[c, 1] * u + m[c, 2] * v) + 0.5), 0, 255).astype(np.uint8)
                 for c in range(3))


def differences(y, cb, cr, matrix, full_range):
    """per channel: (maximum, share of samples at 1, share at 2) of |model - float form|"""
    got = rm.rgb_planes(y, cb, cr, matrix, full_range)
    want = float_form(y, cb, cr, matrix, full_range)
    out = []
    for g, w in zip(got, want):
        d = np.abs(g.astype(np.int16) - w.astype(np.int16))
        out.append((int(d.max()), float(np.mean(d == 1)), float(np.mean(d == 2))))
    return out


def random_with_corners(seed):
    """512 x 512 of seeded random triples, the eight corners of the code cube in its first blocks"""
    rng = np.random.default_rng(seed)
    y = rng.integers(0, 256, (512, 512), dtype=np.uint8)
    cb = rng.integers(0, 256, (256, 256), dtype=np.uint8)
    cr = rng.integers(0, 256, (256, 256), dtype=np.uint8)
    for k in range(8):
        y[0:2, 2 * k:2 * k + 2] = 255 * (k & 1)
        cb[0, k] = 255 * (k >> 1 & 1)
        cr[0, k] = 255 * (k >> 2 & 1)
    return y, cb, cr


def test_every_triple_bt709_limited():
    y, cb, cr = rm.all_triples()
    # every (Y, Cb, Cr) is there exactly once
    code = (y.astype(np.uint32) << 16) | (np.repeat(np.repeat(cb, 2, 0), 2, 1).astype(np.uint32) << 8) | np.repeat(np.repeat(cr, 2, 0), 2, 1)
    assert np.array_equal(np.sort(code, axis=None), np.arange(1 << 24, dtype=np.uint32))
    res = differences(y, cb, cr, 1, False)
    print("BT.709 limited, every triple: (max, share at 1, share at 2) for R, G, B:", res)
    assert all(r[0] <= CAP for r in res), res


@pytest.mark.parametrize("matrix,full_range", [(1, True), (6, False), (6, True), (9, False), (9, True), (4, False), (7, True)])
def test_random_triples_and_corners(matrix, full_range):
    res = differences(*random_with_corners(1000 + matrix), matrix, full_range)
    print("matrix %d %s: (max, share at 1, share at 2) for R, G, B:" % (matrix, "full" if full_range else "limited"), res)
    assert all(r[0] <= CAP for r in res), res


def test_unspecified_is_bt601_and_the_orders_permute():
    y, cb, cr = random_with_corners(7)
    assert all(np.array_equal(a, b) for a, b in zip(rm.rgb_planes(y, cb, cr, 2, False), rm.rgb_planes(y, cb, cr, 6, False)))
    r, g, b = rm.rgb_planes(y, cb, cr, 1, False)
    for order in rm.ORDERS:
        p = rm.pack((y, cb, cr), 1, False, order)
        assert p.shape == (512, 512, 4) and p.dtype == np.uint8
        for k, ch in enumerate(order):
            assert np.array_equal(p[..., k], {"r": r, "g": g, "b": b}.get(ch, np.full_like(r, 255)))
