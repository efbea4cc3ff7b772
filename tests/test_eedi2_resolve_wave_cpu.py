"""k_lattice_resolve with one wave per row (eedi2.hip): the composition it performs, against the serial walk.

Nothing here runs a kernel.  The kernel resolves a row in passes of 256 pixels, four per lane: a lane composes the
2-state maps of its four pixels, the lanes' maps are scanned inside the wave on DPP moves, and the state entering the
next pass is the last lane's map applied to the state that entered this one.  Restated in numpy, that must give the
outcomes the pixel-by-pixel walk gives, for widths that are and are not multiples of a pass.
"""
import numpy as np


def _compose(later, earlier):
    """lr_compose (eedi2.hip): the 2-state map that applies `earlier` first; bit s = outcome for incoming state s."""
    return ((later >> (earlier & 1)) & 1) | (((later >> ((earlier >> 1) & 1)) & 1) << 1)


def _dpp_scan(maps):
    """The kernel's inclusive scan: row_shr 1 / 2 / 4 / 8 inside rows of 16 lanes, then row_bcast:15 into rows 1 and 3
    and row_bcast:31 into rows 2 and 3.  A lane without a source keeps the identity map 2."""
    tm = [int(m) for m in maps]
    for n in (1, 2, 4, 8):
        src = [tm[lane - n] if lane % 16 >= n else 2 for lane in range(64)]
        tm = [_compose(tm[lane], src[lane]) for lane in range(64)]
    src = [tm[16 * (lane // 16) - 1] if lane // 16 in (1, 3) else 2 for lane in range(64)]
    tm = [_compose(tm[lane], src[lane]) for lane in range(64)]
    src = [tm[31] if lane // 16 in (2, 3) else 2 for lane in range(64)]
    tm = [_compose(tm[lane], src[lane]) for lane in range(64)]
    return tm


def _wave_resolve(maps, width, lanes=64, px=4):
    assert lanes == 64
    out, carry = [], 0
    for x0 in range(0, width, lanes * px):
        pm = np.zeros((lanes, px), dtype=np.int64)
        for lane in range(lanes):
            for k in range(px):
                x = x0 + px * lane + k
                m = int(maps[x]) if x < width else 0
                pm[lane, k] = m if k == 0 else _compose(m, int(pm[lane, k - 1]))
        tm = _dpp_scan(pm[:, px - 1])
        for lane in range(lanes):
            before = 2 if lane == 0 else int(tm[lane - 1])
            sin = (before >> carry) & 1
            for k in range(px):
                if x0 + px * lane + k < width:
                    out.append((int(pm[lane, k]) >> sin) & 1)
        carry = (int(tm[lanes - 1]) >> carry) & 1               # readlane 63: the pass's map applied to its entry state
    return out


def test_lattice_resolve_wave_per_row_equals_the_serial_walk():
    rng = np.random.default_rng(23)
    for width in (1, 3, 4, 5, 63, 64, 255, 256, 257, 511, 960, 1000, 1024, 1918, 1920, 4096):
        for _ in range(3):
            maps = rng.integers(0, 4, width)
            maps[0] = 3 * int(rng.integers(0, 2))                # pixel 0's incoming state is irrelevant (both bits equal)
            state, serial = 0, []
            for m in maps:
                state = (int(m) >> state) & 1
                serial.append(state)
            assert _wave_resolve(maps, width) == serial, width


def test_dpp_scan_is_the_inclusive_prefix_composition():
    rng = np.random.default_rng(5)
    for _ in range(200):
        maps = rng.integers(0, 4, 64)
        want, acc = [], 2
        for m in maps:
            acc = _compose(int(m), acc)
            want.append(acc)
        assert _dpp_scan(maps) == want
