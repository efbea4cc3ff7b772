"""The identities the four-pixel dir-map vote (handbrake_amd/csrc/eedi2_dirmap_vote.h) rests on, exhaustively on the host.
The header's own text is what runs: tools/dirmap_vote_check compiles it for the host and prints its results, and every
expectation here is written out independently in Python (eedi2_filter_dir_map, eedi2_template.c:649-707, pixel by pixel)."""
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "tools", "dirmap_vote_check")
ABSENT = 0x7FFF
LIMLUT = [6, 6, 7, 7, 8, 8, 9, 9, 9, 10, 10, 11, 11] + [12] * 18 + [255, 255]


@pytest.fixture(scope="module")
def exe():
    if not os.path.exists(EXE):                        # built by `make product` (__graft_entry__.build())
        subprocess.run(["make", "-C", ROOT, "tools/dirmap_vote_check"], capture_output=True, timeout=600)
    assert os.path.exists(EXE), "tools/dirmap_vote_check is not built (make product)"
    return EXE


def _lines(exe, *args):
    r = subprocess.run([exe, *args], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    return [tuple(int(t) for t in ln.split()) for ln in r.stdout.splitlines()]


def test_rank_selection_against_sort(exe):
    """0-1 principle with a third level for the slots without a value: every assignment of {0, 1, absent} to the nine
    slots - which holds every absent count 0 .. 9 in every arrangement - gives ranks 1 .. 4 of sorted()."""
    got = _lines(exe, "ranks")
    assert len(got) == 3 ** 9
    val = (0, 1, ABSENT)
    counts = set()
    for c, g in enumerate(got):
        v, t = [], c
        for _ in range(9):
            v.append(val[t % 3])
            t //= 3
        counts.add(v.count(ABSENT))
        assert g == tuple(sorted(v)[1:5]), (v, g)
    assert counts == set(range(10))


def test_vote_avg_quotient(exe):
    """(int)((float)a / (float)b + 0.5f) for every a <= 2559, 1 <= b <= 10 from one truncated product."""
    got = np.array(_lines(exe, "avg"), dtype=np.int64).reshape(2560, 10)
    a = np.arange(2560, dtype=np.float32)[:, None]
    b = np.arange(1, 11, dtype=np.float32)[None, :]
    want = ((a / b).astype(np.float32) + np.float32(0.5)).astype(np.float32).astype(np.int64)
    assert np.array_equal(got, want)
    assert np.array_equal(want, (2 * a.astype(np.int64) + b.astype(np.int64)) // (2 * b.astype(np.int64)))
    # the device's reciprocal is not the host's: the truncation must hold for any reciprocal within 4 ulp of 1 / 4b
    num = (4 * a.astype(np.int64) + 2 * b.astype(np.int64) + 1).astype(np.float32)
    r = (np.float32(1) / (4 * b)).astype(np.float32)
    for ulps in (-4, -1, 1, 4):
        rr = (r.view(np.int32) + np.int32(ulps)).view(np.float32)
        assert np.array_equal((num * rr).astype(np.float32).astype(np.int64), want), ulps


def _ref_pixel(n9):
    """eedi2_filter_dir_map for one pixel on the mask: n9 = its 3 x 3 neighbourhood, row by row (255 = no direction)."""
    present = sorted(v for v in n9 if v != 255)
    n = len(present)
    if n < 4:
        return 255
    mid = present[n // 2] if n & 1 else (present[n // 2 - 1] + present[n // 2] + 1) >> 1
    lim = LIMLUT[abs(mid - 128) >> 2]
    votes = [v for v in present if abs(v - mid) <= lim]
    if len(votes) < 4 or (len(votes) < 5 and n9[4] == 255):
        return 255
    return int(np.float32(np.float32(sum(votes) + mid) / np.float32(len(votes) + 1)) + np.float32(0.5))


def _windows():
    """Windows of 3 rows x 12 bytes (columns x - 4 .. x + 7): random ones at every density of peaks, all-peak, no-peak,
    values next to the peak (254) and at both ends of limlut, and near-flat ones where nearly every value votes."""
    rng = np.random.default_rng(20260)
    out = [np.full((3, 12), 255, np.uint8), np.full((3, 12), 254, np.uint8), np.zeros((3, 12), np.uint8),
           np.full((3, 12), 128, np.uint8)]
    for p in (0.0, 0.1, 0.3, 0.5, 0.7, 0.9, 1.0):
        for spread in (256, 24, 6):
            for _ in range(160):
                base = int(rng.integers(0, 256 - spread + 1)) if spread < 256 else 0
                w = rng.integers(base, min(base + spread, 255), size=(3, 12)).astype(np.uint8)
                w[rng.random((3, 12)) < p] = 255
                out.append(w)
    for _ in range(200):                                       # whole rows that do not count (first / last rows of the _2x forms)
        w = rng.integers(100, 140, size=(3, 12)).astype(np.uint8)
        w[rng.random((3, 12)) < 0.2] = 255
        w[int(rng.integers(0, 2)) * 2] = 255
        out.append(w)
    return np.stack(out)


def test_quad_against_per_pixel_vote(exe, tmp_path):
    wins = _windows()
    path = tmp_path / "windows.bin"
    np.ascontiguousarray(wins).view("<u4").tofile(path)
    got = _lines(exe, "quad", str(path))
    assert len(got) == len(wins)
    seen = set()
    for w, (q3, q1, q2, ab01, ab23) in zip(wins, got):
        want, absent = [], []
        for k in range(4):
            n9 = [int(w[r][4 + k + dc]) for r in range(3) for dc in (-1, 0, 1)]
            want.append(_ref_pixel(n9))
            absent.append(n9.count(255))
        seen.update(absent)
        # the byte-level peak counts of the two pixel pairs (units of 0x0100 per half) against a per-pixel count
        assert ab01 == (absent[0] << 8) | (absent[1] << 24), (w, ab01, absent)
        assert ab23 == (absent[2] << 8) | (absent[3] << 24), (w, ab23, absent)
        assert [(q3 >> (8 * k)) & 255 for k in range(4)] == want, (w, hex(q3), want)
        # the ring's half votes: the pair next to the tile only
        assert [(q1 >> (8 * k)) & 255 for k in range(2)] == want[:2], (w, hex(q1), want)
        assert [(q2 >> (8 * k)) & 255 for k in range(2, 4)] == want[2:], (w, hex(q2), want)
    assert seen == set(range(10)), "the windows must hold every absent count 0 .. 9"
