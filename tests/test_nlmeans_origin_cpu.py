"""The NLMeans origin term in single precision (nlmeans.hip, ORG1): the reference adds origin_tune to the weight sum and
origin_tune * pixel to the pixel sum in double and rounds to float (nlmeans_template.c:644-655).  With origin_tune == 1
the kernel adds in float.  The two are the same number: checked here over every float32 exponent from 2^-40 to 2^11,
for the addend 1 and for every pixel 0..255 - all-zero, all-one and single-low-bit mantissas, a seeded random sample of
each exponent, and the values one float ulp either side of every half-integer tie of the result."""
import numpy as np

EXPONENTS = range(-40, 12)
PIX = np.arange(256, dtype=np.float64)


def mantissa_cases(rng):
    """23-bit mantissa fields: all zero, all one, each single bit, and 64 random ones"""
    m = [0, (1 << 23) - 1] + [1 << b for b in range(23)] + [((1 << 23) - 1) ^ (1 << b) for b in range(23)]
    m += [int(x) for x in rng.integers(0, 1 << 23, 64)]
    return np.array(m, dtype=np.uint32)


def floats_of_exponent(e, mant):
    bits = (np.uint32(e + 127) << np.uint32(23)) | mant
    return bits.view(np.float32)


def near_ties():
    """float32 values one ulp either side of (and on) every point where a + t, t an integer in 0..255, lies half way
    between two floats of the result's binade - and the same around the points a quarter of the way, which a double
    rounding would have to cross first"""
    out = []
    for j in range(0, 9):                                   # result in [2^j, 2^(j+1)): float ulp 2^(j-23)
        half = np.float64(2.0) ** (j - 24)
        for k in (1, 2, 3, 5, 7, 255, 256, 257, (1 << 20) + 1, (1 << 23) - 1, (1 << 23) + 1):
            for frac in (1.0, 0.5, 1.5):
                a = np.float32(k * half * frac)
                if not np.isfinite(a) or a <= 0:
                    continue
                out += [np.nextafter(a, np.float32(0)), a, np.nextafter(a, np.float32(np.inf))]
    # the fractional parts k + 1/2 ulp directly: a = n + (2k + 1) * 2^(j-24) for integers n around the binade's ends
    for j in range(0, 12):
        for n in (0, 1, 2 ** j - 1, 2 ** j, 2 ** (j + 1) - 256, 2 ** (j + 1) - 1):
            if n < 0:
                continue
            for odd in (1, 3, 2 ** 10 + 1):
                a = np.float32(np.float64(n) + odd * np.float64(2.0) ** (j - 24))
                out += [np.nextafter(a, np.float32(0)), a, np.nextafter(a, np.float32(np.inf))]
    return np.array(out, dtype=np.float32)


def check(a):
    a = np.asarray(a, dtype=np.float32)
    one = (a.astype(np.float64) + 1.0).astype(np.float32)
    assert np.array_equal(one, a + np.float32(1)), "a + 1"
    wide = (a.astype(np.float64)[:, None] + PIX[None, :]).astype(np.float32)
    narrow = a[:, None] + PIX.astype(np.float32)[None, :]
    assert narrow.dtype == np.float32
    bad = np.argwhere(wide != narrow)
    assert bad.size == 0, f"a = {a[bad[0][0]]!r}, pix = {bad[0][1]}"


def test_every_exponent_every_pixel():
    rng = np.random.default_rng(20240607)
    for e in EXPONENTS:
        check(floats_of_exponent(e, mantissa_cases(rng)))


def test_zero_and_the_ties_of_the_result():
    check(np.array([0.0], dtype=np.float32))
    check(near_ties())
