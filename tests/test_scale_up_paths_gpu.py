"""GPU: every path of the fused 8-bit Lanczos upscaler (csrc/alias.hip: scale8_up_kernel), bit for bit against the
committed restatement of zimg's 16-bit fixed point (oracle/alias_oracle.c: orc_cropscale_plane_fx through
oracle_stream.cropscale_stream).  Small planes that still reach: both tile heights, more than one tile each way with
ragged last tiles, the tile seam, the reflected borders, even and odd first rows, an odd number of staged rows (the
horizontal pass works on row pairs), crop origins off a dword, and several frames in one launch.  Two contents: seeded
random bytes, and saturated runs (blocks of 0 and 255) whose overshoot drives both clamps and, through them, the pack
of four bytes into a dword - compared byte lane by byte lane."""
import math

import numpy as np
import pytest

from handbrake_amd import hbrt, hip, synth
import oracle_stream as os_

pytestmark = pytest.mark.gpu

TW, TH, MAXR = 256, 16, 24          # the kernel's tile width, short tile height, and staged rows (alias.hip: SU_*)


def saturated_frame(w, h, seed):
    """Blocks of 0 and 255, one to seven samples wide and high: every Lanczos lobe overshoots somewhere."""
    rng = np.random.default_rng(seed)

    def plane(pw, ph):
        out = np.zeros((ph, pw), np.uint8)
        y = 0
        while y < ph:
            bh = int(rng.integers(1, 8))
            x = 0
            while x < pw:
                bw = int(rng.integers(1, 8))
                out[y:y + bh, x:x + bw] = 255 * int(rng.integers(0, 2))
                x += bw
            y += bh
        return out
    return plane(w, h), plane((w + 1) // 2, (h + 1) // 2), plane((w + 1) // 2, (h + 1) // 2)


def contents(w, h, n=1):
    return {"random": [synth.random_frame(w, h, t) for t in range(n)],
            "saturated": [saturated_frame(w, h, 100 + t) for t in range(n)]}


def first_rows(src, dst):
    """First tapped source row of every output row before reflection (alias.hip: lanczos_table, six taps)."""
    return [math.floor((i + 0.5) * src / dst - 2.5) for i in range(dst)]


def tile_height(src_h, dst_h):
    """32 where the source rows 32 output rows tap fit the staged rows in every plane, else 16 (alias.hip: setup)."""
    for s, d in ((src_h, dst_h), ((src_h + 1) // 2, (dst_h + 1) // 2)):
        by = first_rows(s, d)
        if any(by[min(y0 + 2 * TH, d) - 1] + 5 - by[y0] + 1 > MAXR for y0 in range(0, d, 2 * TH)):
            return TH
    return 2 * TH


def staged_rows(src_h, dst_h, th):
    by = first_rows(src_h, dst_h)
    return [by[min(y0 + th, dst_h) - 1] + 5 - by[y0] + 1 for y0 in range(0, dst_h, th)]


def byte_lanes(got, want, what):
    """Equal, and if not: which byte lane of the output dwords differs first (two bytes packed over stale upper halves
    was a compiler fault this kernel's pack once met)."""
    assert got.shape == want.shape, f"{what}: shape {got.shape} against {want.shape}"
    if np.array_equal(got, want):
        return
    w4 = got.shape[1] & ~3
    for lane in range(4):
        bad = np.argwhere(got[:, lane:w4:4] != want[:, lane:w4:4])
        if len(bad):
            y, q = bad[0]
            x = 4 * q + lane
            raise AssertionError(f"{what}: byte lane {lane} differs first at row {y} column {x}: "
                                 f"{got[y, x]} against {want[y, x]} ({len(bad)} in this lane)")
    np.testing.assert_array_equal(got, want, err_msg=what)


def through(frames, w, h, ow, oh, crop=(0, 0, 0, 0)):
    t, b, l, r = crop
    st = f"width={ow}:height={oh}:crop-top={t}:crop-bottom={b}:crop-left={l}:crop-right={r}"
    got = hbrt.run_stream(hip.filters(), [("hb_filter_crop_scale_hip", st)], frames)
    want = os_.cropscale_stream(frames, dict(width=ow, height=oh, top=t, bottom=b, left=l, right=r))
    assert len(got) == len(want)
    return [g.planes for g in got], want


def compare(got, want, name):
    for t in range(len(want)):
        for c in range(3):
            byte_lanes(np.asarray(got[t][c]), want[t][c], f"{name} frame {t} plane {c}")


@pytest.mark.parametrize("content", ["random", "saturated"])
def test_2x_two_tiles_each_way_ragged(built, content):
    """264 x 72 -> 528 x 144: luma three tiles wide (256, 256, 16 columns) and five high at 32 rows (the last has 16),
    chroma 264 x 72 with a ragged second column tile: the seam, the reflected borders on all four sides, even and odd
    first rows."""
    w, h, ow, oh = 264, 72, 528, 144
    assert tile_height(h, oh) == 2 * TH
    parity = {b & 1 for b in (v - first_rows(h, oh)[0] for v in first_rows(h, oh)[:32])}
    assert parity == {0, 1}
    got, want = through(contents(w, h)[content], w, h, ow, oh)
    compare(got, want, f"2x {content}")


@pytest.mark.parametrize("content", ["random", "saturated"])
@pytest.mark.parametrize("w,h,ow,oh", [(130, 70, 260, 140), (132, 36, 264, 70)])
def test_2x_odd_number_of_staged_rows(built, content, w, h, ow, oh):
    """A last tile that taps an odd number of source rows: the horizontal pass makes row pairs, the last pair's upper
    half comes from a row nothing staged, and no output row may see it.  130 x 70 -> 260 x 140: the chroma planes
    (65 x 35 -> 130 x 70); 132 x 36 -> 264 x 70 (35/18 x): luma."""
    th = tile_height(h, oh)
    assert th == 2 * TH
    last = [staged_rows(h, oh, th)[-1], staged_rows((h + 1) // 2, (oh + 1) // 2, th)[-1]]
    assert any(n & 1 for n in last), last
    got, want = through(contents(w, h)[content], w, h, ow, oh)
    compare(got, want, f"odd rows {content}")


@pytest.mark.parametrize("content", ["random", "saturated"])
@pytest.mark.parametrize("left", [1, 2, 3])
def test_crop_origin_off_a_dword(built, content, left):
    """A left crop of 1, 2, 3 samples (chroma: 0, 1, 1): staged rows that do not start on a dword are gathered bytewise;
    522 output columns end the luma rows off a dword as well, and 261 chroma columns leave a one-byte last quad.  (The
    crop is the same on both sides: an odd cropped width would leave zimg's branch.)"""
    w, h = 268, 40
    ow, oh = 522, 76
    got, want = through(contents(w, h)[content], w, h, ow, oh, crop=(0, 2, left, left))
    compare(got, want, f"left crop {left} {content}")


@pytest.mark.parametrize("content", ["random", "saturated"])
@pytest.mark.parametrize("w,h,ow,oh,th", [(96, 54, 128, 72, 16), (100, 60, 120, 72, 16), (90, 60, 168, 112, 32)])
def test_ratios_with_no_fixed_row_parity(built, content, w, h, ow, oh, th):
    """4/3 x and 1.2 x (16-row tiles: 32 output rows would tap 30 and 33 source rows, the frame holds 24) and 28/15 x
    (32-row tiles of 23 and 19 staged rows, odd ones not only last): the first rows' parity follows no fixed pattern."""
    assert tile_height(h, oh) == th
    got, want = through(contents(w, h)[content], w, h, ow, oh)
    compare(got, want, f"{ow}/{w} {content}")


@pytest.mark.parametrize("content", ["random", "saturated"])
def test_1x_rows_under_a_crop(built, content):
    """Sides cropped, height kept: the vertical pass resamples at 1 x - the taps of every row are the filter's centre row
    (0, 0, 1, 0, 0, 0 in 14 bits), so an output row is a staged row or nothing - while the columns stretch 96/80."""
    w, h = 96, 40
    assert tile_height(h, h) == TH
    got, want = through(contents(w, h)[content], w, h, w, h, crop=(0, 0, 8, 8))
    compare(got, want, f"1x rows {content}")


def test_three_frames_in_one_launch(built):
    """process_many: three device frames of distinct content through one launch (grid.z = 3 * frame + plane)."""
    import torch
    w, h, ow, oh = 264, 40, 528, 80
    frames = [synth.random_frame(w, h, 0), saturated_frame(w, h, 7), synth.random_frame(w, h, 2)]
    assert not np.array_equal(frames[0][0], frames[2][0])
    want = os_.cropscale_stream(frames, dict(width=ow, height=oh))
    ctx = hip.Ctx(0)
    flt = hip.cropscale_device_filter(ctx, w, h, ow, oh)
    try:
        dev_in = [[torch.from_numpy(np.ascontiguousarray(p)).cuda() for p in f] for f in frames]
        outs = [[torch.zeros((oh, ow), dtype=torch.uint8, device="cuda"),
                 torch.zeros((oh // 2, ow // 2), dtype=torch.uint8, device="cuda"),
                 torch.zeros((oh // 2, ow // 2), dtype=torch.uint8, device="cuda")] for _ in frames]
        torch.cuda.synchronize()
        n = len(frames)
        arr_in = (hip.DevFrame * n)(*[hip.dev_frame(f) for f in dev_in])
        arr_out = (hip.DevFrame * n)(*[hip.dev_frame(o) for o in outs])
        assert flt.process_dev(arr_in, 0, arr_out) == n
        ctx.sync()
        got = [[p.cpu().numpy() for p in o] for o in outs]
    finally:
        flt.close()
        ctx.close()
    compare(got, want, "batch of 3")
