"""GPU parity of EEDI2 behind the queued form of k_filter_map (eedi2.hip): the threads of a 256 x 8 tile list their
candidate pixels by walk length (one step / more) from the two ends of one array, a lane then walks one listed pixel.
Every scratch frame of DecombDevice(mode=24) against the oracle after each pushed frame, all three planes, both field
parities.

Before a case compares anything it computes from the oracle's planes in front of the pass (`npasses=8`: the mask and the
map filter_map reads) what the pass meets, and asserts what the case is there for: which walk lengths occur, that the two
length classes meet in one tile, that walks are clipped at the row ends, that a tile's pixels are all listed."""
import functools

import numpy as np
import pytest

from handbrake_amd import hip, synth
import oracle_lib as ol

pytestmark = pytest.mark.gpu

# the kernel's tile (eedi2.hip: FM_W, FM_ROWS)
TILE_W, TILE_ROWS = 256, 8


def stripes(w, h, n):
    """diagonal stripes 24 pixels wide, 6 columns a row, 3 columns a frame; flat chroma (no edge: maskless planes)"""
    cw, ch = (w + 1) // 2, (h + 1) // 2
    x, y = np.arange(w, dtype=np.int64)[None, :], np.arange(h, dtype=np.int64)[:, None]
    return [((40 + 180 * (((x + 6 * y + 3 * t) // 24) % 2)).astype(np.uint8),
             np.full((ch, cw), 128, np.uint8), np.full((ch, cw), 128, np.uint8)) for t in range(n)]


@functools.lru_cache(maxsize=None)
def frames_of(model, w, h, n):
    return stripes(w, h, n) if model == "stripes" else synth.stream(model, w, h, n)


def plane_width(w, c):
    return w if c == 0 else (w + 1) // 2


@functools.lru_cache(maxsize=None)
def pass_input(model, w, h, n):
    """What filter_map meets on the fields the case processes (frames 0 .. n - 2, both parities, three planes)."""
    frames = frames_of(model, w, h, n)
    fields = [(t, tff) for t in range(n - 1) for tff in (1, 0)]
    st = {"lengths": set(), "clipped": 0, "mixed_tile": False, "full_tile": False, "cand": [0, 0, 0], "mask": [0, 0, 0],
          "luma_px": 0}
    for i in range(len(fields)):
        oe = ol.OrcEedi2(w, h)
        try:
            for t, tff in fields[:i]:
                oe.run(frames[t], tff)
            oe.run(frames[fields[i][0]], fields[i][1], npasses=8)
            planes = [(oe.plane(1, c)[:, :plane_width(w, c)], oe.plane(2, c)[:, :plane_width(w, c)]) for c in range(3)]
        finally:
            oe.close()
        for c, (msk, dmap) in enumerate(planes):
            ph, pw = msk.shape
            cand = (msk == 255) & (dmap != 255)
            cand[0, :] = cand[-1, :] = False
            cand[:, 0] = cand[:, -1] = False
            length = np.abs(((dmap.astype(np.int32) - 128) >> 2) >> 2)
            st["cand"][c] += int(cand.sum())
            st["mask"][c] += int((msk == 255).sum())
            if c == 0:
                st["luma_px"] += ph * pw
            st["lengths"] |= set(int(v) for v in np.unique(length[cand]))
            xs = np.arange(pw)[None, :]
            st["clipped"] += int((cand & (length > 0) & ((xs < 8) | (xs >= pw - 8))).sum())
            for y0 in range(0, ph, TILE_ROWS):
                for x0 in range(0, pw, TILE_W):
                    tc, tl = cand[y0:y0 + TILE_ROWS, x0:x0 + TILE_W], length[y0:y0 + TILE_ROWS, x0:x0 + TILE_W]
                    got = tl[tc]
                    if (got == 0).any() and (got >= 1).any():
                        st["mixed_tile"] = True
                    # every pixel of the tile that can be a candidate is one: a list as long as it gets
                    y1, x1 = min(y0 + TILE_ROWS, ph - 1), min(x0 + TILE_W, pw - 1)
                    if got.size == (y1 - max(y0, 1)) * (x1 - max(x0, 1)) > 0:
                        st["full_tile"] = True
    return st


def compare(model, w, h, n):
    frames = frames_of(model, w, h, n)
    ctx = hip.Ctx(0)
    dev = hip.DecombDevice(ctx, w, h, mode=24)
    oe = ol.OrcEedi2(w, h)
    try:
        dev.push(frames[0])                      # first frame only primes the ring
        for t in range(1, n):
            dev.push(frames[t])                  # processes frame t-1: fields tff=1 then tff=0
            for tff in (1, 0):
                oe.run(frames[t - 1], tff)
            while dev.pull() is not None:
                pass
            for b in range(9):
                for c in range(3):
                    np.testing.assert_array_equal(dev.eedi_plane(b, c), oe.plane(b, c),
                                                  err_msg=f"{ol.EEDI2_BUFFERS[b]} plane {c} after frame {t - 1}")
    finally:
        oe.close()
        dev.close()
        ctx.close()


def test_corners_every_length_class_and_clipped_walks(built):
    """260 x 24: a pixel-dword past a 256-wide tile, 12 field rows (a tile and a half)."""
    st = pass_input("corners", 260, 24, 3)
    print("corners 260x24:", st)
    assert {0, 1, 3, 4, 5} <= st["lengths"]
    assert st["clipped"] > 0, "no candidate with a direction within 8 pixels of a row end"
    assert st["mixed_tile"], "no tile holds both length classes"
    compare("corners", 260, 24, 3)


@pytest.mark.parametrize("w,h", [(260, 24), (516, 40)])
def test_stripes_two_step_walks_and_maskless_chroma(built, w, h):
    st = pass_input("stripes", w, h, 3)
    print(f"stripes {w}x{h}:", st)
    assert {0, 1, 2, 3} <= st["lengths"]
    assert st["mixed_tile"], "no tile holds both length classes"
    assert st["mask"][1] == 0 and st["mask"][2] == 0, "chroma planes are not maskless"
    compare("stripes", w, h, 3)


def test_lengths_up_to_five_are_covered():
    got = set()
    for case in (("corners", 260, 24, 3), ("stripes", 260, 24, 3), ("stripes", 516, 40, 3)):
        got |= pass_input(*case)["lengths"]
    assert set(range(6)) <= got


@pytest.mark.parametrize("w,h", [(260, 24), (64, 16)])
def test_random_nearly_every_pixel_listed(built, w, h):
    """Noise: every pixel off the border a one-step candidate - list 0 as long as a tile can make it."""
    st = pass_input("random", w, h, 3)
    print(f"random {w}x{h}:", st)
    assert st["cand"][0] >= 0.7 * st["luma_px"]
    assert st["lengths"] == {0}
    assert st["full_tile"]
    compare("random", w, h, 3)


def test_interlaced_partial_last_tile(built):
    """1918 x 120: the row length is no multiple of 4, the last tile is partial, 60 field rows are no multiple of 8."""
    st = pass_input("interlaced", 1918, 120, 3)
    print("interlaced 1918x120:", st)
    assert st["cand"][0] > 0 and {0, 1} <= st["lengths"]
    compare("interlaced", 1918, 120, 3)
