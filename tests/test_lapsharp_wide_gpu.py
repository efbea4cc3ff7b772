"""GPU parity, tolerance 0: the 8-bit 3 x 3 lapsharp kernels on device-resident frames against the oracle -
lapsharp3_wide_kernel (csrc/sharpen.hip: one load per lane and row, neighbours by DPP, byte dot products) where every plane
and pitch is 8-byte aligned and luma is at least a wave's span wide, lapsharp3_rows_kernel everywhere else.  The sizes
sit on the edges of a lane (8 columns), of a wave (512) and of a workgroup (1024 columns; 8 rows a thread, 16 a workgroup) and
on either side of the width below which the narrower kernel runs; rows beyond a plane's width hold junk, which the
kernels must read as the zero padding the reference sees."""
import numpy as np
import pytest

import oracle_lib as ol
import sharpen_dev as sd

pytestmark = pytest.mark.gpu

LANE, WAVE_SPAN, WG_SPAN, ROWS, WG_ROWS = 8, 512, 1024, 8, 16     # sharpen.hip: LW_PX, LW_WAVE_SPAN, LW_SPAN, LW_ROWS, LW_BY * LW_ROWS
KERNELS = ("lap", "isolap")
STRENGTHS = (0.2, 0.35)                                               # the one-float-multiply mix, the double mix


def _planes(rng, w, h, lcw, lch, content):
    shapes = [(h, w)] + [(-(-h >> lch), -(-w >> lcw))] * 2
    if content == "random":
        return [rng.integers(0, 256, size=s).astype(np.uint8) for s in shapes]
    if content == "checker":
        return [(((np.add.outer(np.arange(s[0]), np.arange(s[1]))) & 1) * 255).astype(np.uint8) for s in shapes]
    return [np.full(s, {"zeros": 0, "ones": 255}[content], np.uint8) for s in shapes]


def _run(w, h, frames, kern, strength, lcw=1, lch=1, pad=0, offset=0):
    """frames (lists of three planes) through one process_dev call; rows are padded to 64 samples + pad and filled with
    junk beyond the width; offset moves every input plane's first byte"""
    return sd.run_dev("lapsharp", sd.lapsharp_params([kern] * 3, [strength] * 3), w, h, 8, frames, lcw, lch, pad, offset)


def _check(w, h, frames, kern, strength, **kw):
    got = _run(w, h, frames, kern, strength, **kw)
    for t, f in enumerate(frames):
        for c in range(3):
            want = ol.orc_lapsharp_plane(f[c], strength, kern)
            np.testing.assert_array_equal(got[t][c], want, err_msg=f"{w}x{h} {kern} {strength} {kw} frame {t} plane {c}")


WIDTHS = (list(range(1, 10)) + [63, 64, 65, 255, 256, 257]                      # the narrower kernel's lanes and waves
          + [WAVE_SPAN - 1, WAVE_SPAN, WAVE_SPAN + 1, WG_SPAN + 1]                # either side of the switch; one past a wave / a workgroup
          + [WG_SPAN + d for d in range(2, 10)]                                   # a last lane with 2 .. 9 columns
          + [WG_SPAN + 63, WG_SPAN + 64, WG_SPAN + 65, WG_SPAN + 255, WG_SPAN + 256, WG_SPAN + 257]
          + [2 * WG_SPAN - 1, 2 * WG_SPAN, 2 * WG_SPAN + 1])                      # chroma on the switch (4:2:0), two workgroups and one column


@pytest.mark.parametrize("lc", [(1, 1), (0, 0)], ids=["420", "444"])
@pytest.mark.parametrize("w", sorted(set(WIDTHS)))
def test_widths(built, w, lc):
    rng = np.random.default_rng(w)
    h = ROWS + 3
    frames = [_planes(rng, w, h, *lc, "random") for _ in range(2)]
    for i, (kern, strength) in enumerate((k, s) for k in KERNELS for s in STRENGTHS):
        _check(w, h, frames, kern, strength, lcw=lc[0], lch=lc[1])


HEIGHTS = [1, 2, 3, 4, 5, ROWS - 1, ROWS, ROWS + 1, WG_ROWS - 1, WG_ROWS, WG_ROWS + 1, 2 * WG_ROWS + ROWS + 1]


@pytest.mark.parametrize("w", [72, WG_SPAN + 40], ids=["narrow", "wide"])
@pytest.mark.parametrize("h", HEIGHTS)
def test_heights(built, w, h):
    rng = np.random.default_rng(1000 * h + w)
    for lc in ((1, 1), (0, 0)):
        frames = [_planes(rng, w, h, *lc, "random")]
        for kern, strength in zip(KERNELS, STRENGTHS):
            _check(w, h, frames, kern, strength, lcw=lc[0], lch=lc[1])


@pytest.mark.parametrize("content", ["random", "zeros", "ones", "checker"])
@pytest.mark.parametrize("strength", STRENGTHS)
@pytest.mark.parametrize("kern", KERNELS)
def test_content(built, kern, strength, content):
    """all 0, all 255 and the 0 / 255 checkerboard hold the largest and smallest sums of both tables and both clamps"""
    rng = np.random.default_rng(7)
    for w, h in ((200, 21), (WG_SPAN + 72, 37)):
        for lc in ((1, 1), (0, 0)):
            _check(w, h, [_planes(rng, w, h, *lc, content)], kern, strength, lcw=lc[0], lch=lc[1])


@pytest.mark.parametrize("w", [136, WG_SPAN + 24], ids=["narrow", "wide"])
@pytest.mark.parametrize("n", [1, 16, 17])
def test_frames_per_call(built, n, w):
    """a launch takes up to 16 frames: 17 are a launch of 16 and one of 1"""
    rng = np.random.default_rng(n)
    h = 19
    frames = [_planes(rng, w, h, 1, 1, "random") for _ in range(n)]
    _check(w, h, frames, "isolap", 0.2)
    _check(w, h, frames, "lap", 0.35)


@pytest.mark.parametrize("w", [136, WG_SPAN + 24, 2 * WG_SPAN + 200], ids=["narrow", "wide", "wider"])
@pytest.mark.parametrize("how", [dict(pad=16), dict(pad=64), dict(pad=4), dict(offset=4), dict(pad=16, offset=4)],
                         ids=["pitch+16", "pitch+64", "pitch+4", "base+4", "pitch+16-base+4"])
def test_pitch_and_base(built, w, how):
    """pitches padded by a multiple of 16 bytes stay on the wide kernel; a pitch padded by 4 or a plane that starts 4 bytes
    off does not allow its vector loads (the filter then works on aligned copies or the narrower kernel): the same result"""
    rng = np.random.default_rng(w)
    h = 2 * ROWS + 3
    frames = [_planes(rng, w, h, 1, 1, "random") for _ in range(2)]
    for kern, strength in zip(KERNELS, STRENGTHS):
        _check(w, h, frames, kern, strength, **how)
