"""The arithmetic of lapsharp3_wide_kernel (handbrake_amd/csrc/lapsharp_rowdot.h) on the host.  The header's own text is
what runs: tools/lapsharp_rowdot_check compiles it for the host and writes its results; every expectation here is the plain
form of lapsharp.c:148-175 in numpy."""
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "tools", "lapsharp_rowdot_check")
# (corner, edge, centre, coef) of the two 3 x 3 tables, lapsharp.c:37-52
TABLES = {"lap": (0, -1, 5, 1.0), "isolap": (-1, -4, 25, 1.0 / 5)}


@pytest.fixture(scope="module")
def exe():
    if not os.path.exists(EXE):                        # built by `make product` (__graft_entry__.build())
        subprocess.run(["make", "-C", ROOT, "tools/lapsharp_rowdot_check"], capture_output=True, timeout=600)
    assert os.path.exists(EXE), "tools/lapsharp_rowdot_check is not built (make product)"
    return EXE


def _run(exe, *args):
    r = subprocess.run([exe, *[str(a) for a in args]], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    return r.stdout


@pytest.mark.parametrize("table", sorted(TABLES))
def test_row_sums_every_window(exe, tmp_path, table):
    """every (l, m, r) of 8-bit samples, whatever the window's fourth byte: U = -(a (l + r) + b m), H = -b (l + r)"""
    a, b, c, _ = TABLES[table]
    out = tmp_path / "rows.bin"
    _run(exe, "rows", a, b, c, out)
    got = np.fromfile(out, dtype="<u4")
    assert got.size == 1 << 24
    w = np.arange(1 << 24, dtype=np.int64)
    left, mid, right = w & 255, (w >> 8) & 255, (w >> 16) & 255
    assert np.array_equal(got & 0xFFFF, -(a * (left + right) + b * mid))
    assert np.array_equal(got >> 16, -b * (left + right))


def _float_mix_constant(a, b, c, coef, strength):
    """lap_float_mix's search (sharpen.hip; tests/test_eedi2_identities_cpu.py runs it too): the float beside coef * strength
    whose one multiply gives the double form's truncation for every (sum, centre)"""
    ki = round(1 / coef)
    acc = np.arange(255 * (4 * a + 4 * b), 255 * c + 1, dtype=np.int64)[:, None]
    cen = np.arange(256, dtype=np.int64)[None, :]
    ref = np.trunc(((acc.astype(np.float64) * coef) - cen.astype(np.float64)) * strength).astype(np.int64)
    q = (acc - ki * cen).astype(np.float32)
    s = np.float32(coef * strength)
    for f in (s, np.nextafter(s, np.float32(np.inf)), np.nextafter(s, np.float32(-np.inf))):
        if np.array_equal(np.trunc(q * f).astype(np.int64), ref):
            return ki, f
    raise AssertionError("no float form")


def _windows():
    """3 rows x 12 bytes (columns x - 4 .. x + 7): every 0 / 255 assignment of the 3 x 6 samples the four pixels see (the
    largest and smallest sums of every sign pattern), all 0, all 255, flat greys, and random bytes"""
    rng = np.random.default_rng(1148)
    n = 1 << 18
    bits = (np.arange(n, dtype=np.int64)[:, None] >> np.arange(18)[None, :]) & 1
    corners = np.zeros((n, 3, 12), np.uint8)
    corners[:, :, 3:9] = (bits * 255).astype(np.uint8).reshape(n, 3, 6)
    flat = np.stack([np.full((3, 12), v, np.uint8) for v in (0, 1, 127, 128, 254, 255)])
    rand = rng.integers(0, 256, size=(200000, 3, 12)).astype(np.uint8)
    near = np.clip(rng.integers(0, 256, size=(50000, 1, 1)) + rng.integers(-3, 4, size=(50000, 3, 12)), 0, 255).astype(np.uint8)
    return np.concatenate([corners, flat, rand, near])


@pytest.mark.parametrize("table", sorted(TABLES))
def test_nine_taps_and_float_mix(exe, tmp_path, table):
    """the four pixels of a dword through the header (windows, row sums, their combination, the float mix) against the
    plain 9-tap sum and the reference's double mix, truncated through int16 and clamped"""
    a, b, c, coef = TABLES[table]
    strength = 0.2
    ki, mixf = _float_mix_constant(a, b, c, coef, strength)
    wins = _windows()
    src, out = tmp_path / "windows.bin", tmp_path / "quad.bin"
    np.ascontiguousarray(wins).view("<u4").tofile(src)
    _run(exe, "quad", a, b, c, ki, int(np.float32(mixf).view(np.uint32)), src, out)
    got = np.fromfile(out, dtype="<i4").reshape(len(wins), 4, 2)
    taps = np.array([[a, b, a], [b, c, b], [a, b, a]], dtype=np.int64)
    w = wins.astype(np.int64)
    for p in range(4):
        acc = sum(taps[r, k] * w[:, r, 3 + p + k] for r in range(3) for k in range(3))
        assert np.array_equal(got[:, p, 0], acc), (table, p)
        centre = w[:, 1, 4 + p]
        mixed = ((acc.astype(np.float64) * coef) - centre.astype(np.float64)) * strength
        want = np.clip(np.trunc(mixed).astype(np.int64).astype(np.int16).astype(np.int64) + centre, 0, 255)
        assert np.array_equal(got[:, p, 1], want), (table, p)
    assert got[:, :, 0].min() == 255 * (4 * a + 4 * b) and got[:, :, 0].max() == 255 * c
    assert got[:, :, 1].min() == 0 and got[:, :, 1].max() == 255


def test_window_of_a_wide_lane(exe):
    """lrd_window for a lane of four dwords: pixel p sees bytes 3 + p .. 6 + p of (left, own x 4, right)"""
    got = [int(v) for v in _run(exe, "window").split()]
    assert got == [sum((3 + p + k) << (8 * k) for k in range(4)) for p in range(16)]
