"""GPU: the Format drop-in's chroma down-sampling to a HIGHER depth (4:2:2 -> 4:2:0, 4:4:4 -> 4:2:2, 4:4:4 -> 4:2:0 at
8 -> 10, 8 -> 12, 10 -> 12 bits) against the integer model tests/format_deepen_model.py, tolerance 0 (parity unpinned:
libswscale is outside the reference tree); and the jobs that end in `format=yuv420p10le | yuv422p10le` behind an 8-bit
4:2:2 / 4:4:4 pipeline."""
import functools

import numpy as np
import pytest

from handbrake_amd import hbrt, hip
import format_deepen_model as m

pytestmark = pytest.mark.gpu
LAYOUT = {"444": "1x1", "422": "2x1", "420": "2x2"}
LAP = "y-strength=0.2:y-kernel=isolap"
MARKER = 7


def _fmt(layout, depth):
    return hbrt.PIX_FMT[(LAYOUT[layout], depth)]


def _dt(depth):
    return np.uint8 if depth == 8 else np.uint16


@functools.lru_cache(maxsize=None)
def _case(kind, w, h, n, sd, dd, src, dst):
    """(inputs, expected): computed once, shared, only read"""
    frames = tuple(m.frame(kind, w, h, t, sd, src) for t in range(n))
    return frames, tuple(m.deepen_frame(fr, sd, dd, src, dst) for fr in frames)


def _padded(p):
    """a device copy of a plane with rows 64 samples apart at least (the library's own layout: dword / qword moves)"""
    import torch
    a = np.ascontiguousarray(p)
    t = torch.zeros((a.shape[0], (a.shape[1] + 63) // 64 * 64), dtype=torch.uint8 if a.dtype == np.uint8 else torch.int16,
                    device="cuda")
    v = t[:, :a.shape[1]]
    v.copy_(torch.from_numpy(a if a.dtype == np.uint8 else a.view(np.int16)))
    return v


def _host(t, dtype):
    a = t.cpu().numpy()
    return a if dtype == np.uint8 else a.view(np.uint16)


def _resident(frames, wants, sd, dd, src, dst, n=None, what=""):
    """`n` device-resident frames (the inputs shared round-robin) through one process_dev call; the output pictures are
    prefilled with a marker value; the inputs are unchanged afterwards.  Returns the outputs as host planes."""
    import torch
    n = n or len(frames)
    h, w = frames[0][0].shape
    ctx = hip.Ctx(0)
    flt = hip.format_deepen_device_filter(ctx, w, h, m.SUB[src], m.SUB[dst], sd, dd)
    try:
        k = len(frames)
        dev_in = [[_padded(p) for p in fr] for fr in frames]
        outs = [[_padded(np.full_like(p, MARKER)) for p in wants[0]] for _ in range(n)]
        torch.cuda.synchronize()
        arr_in = (hip.DevFrame * n)(*[hip.dev_frame(dev_in[i % k]) for i in range(n)])
        arr_out = (hip.DevFrame * n)(*[hip.dev_frame(o) for o in outs])
        assert flt.process_dev(arr_in, 0, arr_out) == n
        ctx.sync()
        got = [[_host(outs[i][c], _dt(dd)) for c in range(3)] for i in range(n)]
        for i in range(n):
            for c in range(3):
                assert got[i][c].dtype == wants[i % k][c].dtype and got[i][c].shape == wants[i % k][c].shape
                np.testing.assert_array_equal(got[i][c], wants[i % k][c],
                                              err_msg=f"{what} {src}->{dst} {sd}->{dd} bits frame {i} plane {c}")
        for j in range(k):
            for c in range(3):
                np.testing.assert_array_equal(_host(dev_in[j][c], _dt(sd)), frames[j][c], err_msg=f"input {j} plane {c} was written")
        return got
    finally:
        flt.close()
        ctx.close()


@pytest.mark.parametrize("sd,dd", m.STEPS)
@pytest.mark.parametrize("src,dst", m.PAIRS)
def test_pairs_steps_odd_planes(built, src, dst, sd, dd):
    """67 x 37: odd planes, ragged dword and qword tails, an odd source size (the filter's step is then not 2)"""
    frames, wants = _case("random", 67, 37, 2, sd, dd, src, dst)
    _resident(frames, wants, sd, dd, src, dst)


@pytest.mark.parametrize("src,dst", m.PAIRS)
def test_more_than_one_workgroup_each_way(built, src, dst):
    """530 x 134: luma wider than a workgroup's 256 columns and taller than its 16 rows; a 4:2:2 target's chroma wider
    too, and every target's chroma taller than the rows of a workgroup"""
    frames, wants = _case("random", 530, 134, 1, 8, 10, src, dst)
    _resident(frames, wants, 8, 10, src, dst)


@pytest.mark.parametrize("kind", ["rows", "bars", "flat"])
@pytest.mark.parametrize("sd,dd", [(8, 10), (10, 12)])
def test_both_clips_and_the_saturated_intermediate(built, kind, sd, dd):
    """full-scale bars overshoot the bicubic: the top clip, the bottom clip (the negative lobes: a negative intermediate
    is kept) and the 15-bit saturation between the passes are all reached"""
    for src, dst in m.PAIRS:
        frames, wants = _case(kind, 66, 38, 2, sd, dd, src, dst)
        got = _resident(frames, wants, sd, dd, src, dst, what=kind)
        full, top = (1 << dd) - 1, ((1 << sd) - 1) << (dd - sd)
        if kind == "flat":
            assert int(got[0][1].min()) == int(got[0][1].max()) == top         # full-scale flat chroma is shifted, like luma
        if kind in ("rows", "bars"):
            assert int(got[0][0].min()) == 0 and int(got[0][0].max()) == top
        if kind == "bars":
            assert int(got[0][1].min()) == 0 and int(got[0][1].max()) == full   # (the overshoot reaches the clip)


@pytest.mark.parametrize("src,dst,w,h", [("422", "420", 24, 11), ("444", "422", 11, 6), ("444", "420", 11, 11)])
def test_smallest_planes_taken(built, src, dst, w, h):
    """eleven chroma samples in every resampled direction: every row and column is an edge one"""
    frames, wants = _case("random", w, h, 1, 8, 10, src, dst)
    _resident(frames, wants, 8, 10, src, dst)


@pytest.mark.parametrize("src,dst", m.PAIRS)
def test_seventeen_frames_one_full_burst_plus_one(built, src, dst):
    """130 x 70 at 8 -> 10, 17 device-resident frames in one call: a launch of 16 and a launch of one.  The 17 inputs are
    four frames shared between the entries; they are only read."""
    frames = tuple(m.frame("random" if t & 1 else "progressive", 130, 70, t, 8, src) for t in range(4))
    wants = tuple(m.deepen_frame(fr, 8, 10, src, dst) for fr in frames)
    _resident(frames, wants, 8, 10, src, dst, n=17)


def test_create_declines(built):
    """an equal or lower depth, equal subsampling, more chroma samples in any direction, a depth outside 8 / 10 / 12, a
    resampled chroma direction under 11 samples"""
    ctx = hip.Ctx(0)
    try:
        for src, dst, sd, dd, w, h in [
                ((1, 0), (1, 1), 8, 8, 128, 72), ((0, 0), (1, 1), 10, 10, 128, 72), ((0, 0), (1, 0), 12, 12, 128, 72),
                ((1, 0), (1, 1), 10, 8, 128, 72), ((0, 0), (1, 0), 12, 10, 128, 72), ((0, 0), (1, 1), 12, 8, 128, 72),
                ((1, 1), (1, 1), 8, 10, 128, 72), ((1, 0), (1, 0), 8, 12, 128, 72), ((0, 0), (0, 0), 10, 12, 128, 72),
                ((1, 1), (1, 0), 8, 10, 128, 72), ((1, 0), (0, 0), 8, 10, 128, 72), ((1, 1), (0, 0), 10, 12, 128, 72),
                ((1, 1), (0, 1), 8, 10, 128, 72), ((0, 1), (1, 0), 8, 10, 128, 72),
                ((1, 0), (1, 1), 9, 10, 128, 72), ((1, 0), (1, 1), 8, 16, 128, 72), ((1, 0), (1, 1), 6, 8, 128, 72),
                ((1, 0), (1, 1), 10, 14, 128, 72), ((1, 0), (1, 1), 8, 9, 128, 72),
                ((1, 0), (1, 1), 8, 10, 128, 10), ((0, 0), (1, 0), 8, 10, 10, 72), ((0, 0), (1, 1), 10, 12, 128, 10),
                ((0, 0), (1, 1), 8, 12, 10, 72)]:
            with pytest.raises(hip.HipError, match="(?i)unsupported|not supported"):
                hip.format_deepen_device_filter(ctx, w, h, src, dst, sd, dd)
        for src, dst in m.PAIRS:
            for sd, dd in m.STEPS:
                hip.format_deepen_device_filter(ctx, 128, 72, m.SUB[src], m.SUB[dst], sd, dd).close()
        # a direction that keeps its size may be as small as it likes
        hip.format_deepen_device_filter(ctx, 128, 11, (1, 0), (1, 1), 8, 10).close()
        hip.format_deepen_device_filter(ctx, 11, 2, (0, 0), (1, 0), 8, 10).close()
    finally:
        ctx.close()


# ---- jobs ---------------------------------------------------------------------------------------------------------------
def _job(entries, target, src, depth, kind="random", w=66, h=38, n=3):
    """`entries` ("lapsharp", "vfr", "format") on a yuv<src>p<depth> job with the HIP objects registered (the drop-in
    object stands in for the list entry libhb's own `format` would be: the swap leaves an object that already is the
    drop-in alone).  Returns (stage names, OutFrames, the input frames)."""
    F = hbrt.FILTER_ID
    flt = hip.filters()
    # With the drop-in registered as its own id's filter, a library without this entry point must fail here, before a job is
    # opened, not inside one.
    assert hasattr(hip.lib(), "hbhip_format_deepen_create"), "libhbhip.so has no hbhip_format_deepen_create"
    frames = [m.frame(kind, w, h, t, depth, src) for t in range(n)]
    settings = {"lapsharp": LAP, "vfr": "mode=0:rate=30000/1001", "format": f"format={target}"}
    hbrt.register_filters(flt, {F["lapsharp"]: "hb_filter_lapsharp_hip", F["vfr"]: "hb_filter_vfr_standin",
                                F["format"]: "hb_filter_format_hip"})
    try:
        names, got = hbrt.run_job([(F[e], settings[e]) for e in entries], frames, pix_fmt=_fmt(src, depth))
    finally:
        hbrt.register_filters(flt, {F["lapsharp"]: None, F["vfr"]: None, F["format"]: None})
    return names, got, frames


def _sharp(frames, depth):
    import oracle_stream as os_
    import golden_cases as gc
    return os_.lapsharp_stream(frames, [gc.lap(depth=depth)] * len(frames))


def _check_job(names, got, sharp, sd, dd, src, dst, stages=4):
    assert len(names) == stages, names
    assert names[-4] == "HIP upload adapter" and names[-2] == "Format (HIP)" and names[-1] == "HIP download adapter"
    assert "HIP" in names[-3] and "harp" in names[-3]
    assert not any("HIP" in n for n in names[:-4])
    assert len(got) == len(sharp)
    for t, fr in enumerate(sharp):
        want = m.deepen_frame(fr, sd, dd, src, dst)
        assert len(got[t].planes) == 3
        for c in range(3):
            assert got[t].planes[c].dtype == np.uint16 and got[t].planes[c].shape == want[c].shape
            np.testing.assert_array_equal(got[t].planes[c], want[c], err_msg=f"job {src}->{dst} {sd}->{dd} frame {t} plane {c}")


def test_job_422_8_bit_to_yuv420p10le(built):
    """the ordinary job: an 8-bit 4:2:2 title in front of SVT-AV1 or VP9 at 10 bits"""
    names, got, frames = _job(["lapsharp", "format"], "yuv420p10le", "422", 8)
    _check_job(names, got, _sharp(frames, 8), 8, 10, "422", "420")


def test_job_444_8_bit_to_yuv420p10le(built):
    names, got, frames = _job(["lapsharp", "format"], "yuv420p10le", "444", 8)
    _check_job(names, got, _sharp(frames, 8), 8, 10, "444", "420")


def test_job_444_8_bit_to_yuv422p10le(built):
    """an 8-bit 4:4:4 title in front of ProRes 422 or DNxHR at 10 bits"""
    names, got, frames = _job(["lapsharp", "format"], "yuv422p10le", "444", 8)
    _check_job(names, got, _sharp(frames, 8), 8, 10, "444", "422")


def test_job_with_vfr_between(built):
    """the frame-rate shaper every preset-built job has: by its id it stands in front of lapsharp, outside the run, and
    moves no sample - five stages, the entry still behind a drop-in"""
    names, got, frames = _job(["lapsharp", "vfr", "format"], "yuv420p10le", "422", 8)
    _check_job(names, got, _sharp(frames, 8), 8, 10, "422", "420", stages=5)


def test_lone_drop_in_still_declines(built):
    """the mark outside of a device-resident run changes nothing: a lone `format` on host frames keeps its CPU filter"""
    for target in ("yuv420p10le", "yuv420p10le:hip-deepen-step=1"):
        with pytest.raises(RuntimeError):
            hbrt.Chain(hip.filters(), [("hb_filter_format_hip", f"format={target}")], 128, 72, _fmt("422", 8))


def test_job_whose_deepen_step_declines_ends_planar(built):
    """[lapsharp, format=yuv420p10le] on a 128 x 10 yuv422p job: the entry is marked, its init() declines (ten chroma rows:
    libswscale cuts its filter short under 11), and the run in front of it ends planar in the stream's own format and
    samples through a plain download adapter.  (Dropped instead of replaced: the drop-in is registered as its own id's
    filter.)"""
    names, got, frames = _job(["lapsharp", "format"], "yuv420p10le", "422", 8, w=128, h=10)
    sharp = _sharp(frames, 8)
    assert len(names) == 3 and names[0] == "HIP upload adapter" and names[2] == "HIP download adapter", names
    assert "HIP" in names[1] and "harp" in names[1]
    assert len(got) == len(sharp)
    for t, fr in enumerate(sharp):
        assert len(got[t].planes) == 3
        for c in range(3):
            assert got[t].planes[c].dtype == np.uint8
            np.testing.assert_array_equal(got[t].planes[c], fr[c], err_msg=f"frame {t} plane {c}")
