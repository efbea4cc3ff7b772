"""GPU: the Format drop-in's scaler path at a lower depth (10 -> 8, 12 -> 8, 12 -> 10 bits; with 4:2:2 -> 4:2:0,
4:4:4 -> 4:2:2, 4:4:4 -> 4:2:0, or - for NV12 / P010LE targets - the subsampling unchanged) against the integer model
tests/format_scaled_model.py, tolerance 0 (parity unpinned: libswscale is outside the reference tree); and the jobs that end
in `format=yuv420p | nv12 | p010le` behind a deeper or denser pipeline."""
import numpy as np
import pytest

from handbrake_amd import hbrt, hip
import biplanar_model as bm
import format_scaled_model as m

pytestmark = pytest.mark.gpu
LAYOUT = {"444": "1x1", "422": "2x1", "420": "2x2"}
RESAMPLED = m.PAIRS[:3]                        # the pairs the drop-in takes on its own; 4:2:0 -> 4:2:0 needs the registry's mark
LAP = "y-strength=0.2:y-kernel=isolap"


def _fmt(layout, depth):
    return hbrt.PIX_FMT[(LAYOUT[layout], depth)]


def _name(layout, depth):
    return f"yuv{layout}p" + {8: "", 10: "10le", 12: "12le"}[depth]


def _through_drop_in(frames, sd, dd, src, dst):
    return hbrt.run_stream(hip.filters(), [("hb_filter_format_hip", f"format={_name(dst, dd)}")], frames,
                           pix_fmt=_fmt(src, sd))


def _check(got, frames, sd, dd, src, dst, what=""):
    assert len(got) == len(frames)
    for t, fr in enumerate(frames):
        want = m.scaled_frame(fr, sd, dd, src, dst)
        assert len(got[t].planes) == 3
        for c in range(3):
            assert got[t].planes[c].dtype == want[c].dtype and got[t].planes[c].shape == want[c].shape
            np.testing.assert_array_equal(got[t].planes[c], want[c],
                                          err_msg=f"{what} {src}->{dst} {sd}->{dd} bits frame {t} plane {c}")


def test_format_yuv420p_on_a_yuv422p10le_stream(built):
    """the ordinary job: 10-bit 4:2:2 camera footage in front of an 8-bit 4:2:0 encoder"""
    frames = [m.frame("progressive", 66, 38, t, 10, "422") for t in range(2)]
    _check(_through_drop_in(frames, 10, 8, "422", "420"), frames, 10, 8, "422", "420")


@pytest.mark.parametrize("w,h", [(66, 38), (67, 37)])
@pytest.mark.parametrize("sd,dd", m.STEPS)
@pytest.mark.parametrize("src,dst", RESAMPLED)
def test_pairs_steps_odd_planes(built, src, dst, sd, dd, w, h):
    """odd planes, ragged dword tails, an odd source size (the filter's step is then not 2), and for 8-bit targets a tail
    that ends inside a dither dword"""
    frames = [m.frame("random", w, h, t, sd, src) for t in range(2)]
    _check(_through_drop_in(frames, sd, dd, src, dst), frames, sd, dd, src, dst)


@pytest.mark.parametrize("src,dst", RESAMPLED)
def test_more_than_one_workgroup_each_way(built, src, dst):
    """530 x 134 at 10 -> 8: planes wider than a workgroup's 256 columns and taller than its rows; rows past 8, so the
    dither's row wraps"""
    frames = [m.frame("random", 530, 134, 0, 10, src)]
    _check(_through_drop_in(frames, 10, 8, src, dst), frames, 10, 8, src, dst)


@pytest.mark.parametrize("kind", ["rows", "bars", "flat"])
@pytest.mark.parametrize("sd,dd", m.STEPS)
def test_clip_after_the_dither_at_both_ends(built, kind, sd, dd):
    for src, dst in RESAMPLED:
        frames = [m.frame(kind, 66, 38, t, sd, src) for t in range(2)]
        got = _through_drop_in(frames, sd, dd, src, dst)
        _check(got, frames, sd, dd, src, dst, kind)
        full = (1 << dd) - 1
        if kind == "flat":
            assert int(got[0].planes[1].min()) == int(got[0].planes[1].max()) == full
        if kind in ("rows", "bars"):
            assert int(got[0].planes[0].min()) == 0 and int(got[0].planes[0].max()) == full
        if kind == "bars":
            assert int(got[0].planes[1].min()) == 0 and int(got[0].planes[1].max()) == full


@pytest.mark.parametrize("src,dst,w,h", [("422", "420", 24, 11), ("444", "422", 11, 6), ("444", "420", 11, 11)])
def test_smallest_planes_taken(built, src, dst, w, h):
    """eleven chroma samples in a resampled direction, 12 -> 8: every row is an edge row"""
    frames = [m.frame("random", w, h, 0, 12, src)]
    _check(_through_drop_in(frames, 12, 8, src, dst), frames, 12, 8, src, dst)


# ---- the C ABI ----------------------------------------------------------------------------------------------------------
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


@pytest.mark.parametrize("src,dst", m.PAIRS)
def test_seventeen_frames_one_full_burst_plus_one(built, src, dst):
    """130 x 70 at 10 -> 8, 17 device-resident frames in one call: a launch of 16 and a launch of one; the three pairs
    and the depth-only form.  The 17 inputs are four frames shared between the entries; they are only read."""
    import torch
    w, h, n = 130, 70, 17
    frames = [m.frame("random" if t & 1 else "progressive", w, h, t, 10, src) for t in range(4)]
    wants = [m.scaled_frame(fr, 10, 8, src, dst) for fr in frames]
    ctx = hip.Ctx(0)
    flt = hip.format_scaled_device_filter(ctx, w, h, m.SUB[src], m.SUB[dst], 10, 8)
    try:
        dev_in = [[_padded(p) for p in fr] for fr in frames]
        outs = [[_padded(np.full_like(p, 7)) for p in wants[0]] for _ in range(n)]
        torch.cuda.synchronize()
        arr_in = (hip.DevFrame * n)(*[hip.dev_frame(dev_in[i % 4]) for i in range(n)])
        arr_out = (hip.DevFrame * n)(*[hip.dev_frame(o) for o in outs])
        assert flt.process_dev(arr_in, 0, arr_out) == n
        ctx.sync()
        for i in range(n):
            for c in range(3):
                np.testing.assert_array_equal(_host(outs[i][c], np.uint8), wants[i % 4][c], err_msg=f"frame {i} plane {c}")
        for k in range(4):
            for c in range(3):
                np.testing.assert_array_equal(_host(dev_in[k][c], np.uint16), frames[k][c], err_msg=f"input {k} plane {c} was written")
    finally:
        flt.close()
        ctx.close()


@pytest.mark.parametrize("layout", ["422", "444"])
@pytest.mark.parametrize("sd,dd", [(12, 8), (12, 10)])
def test_depth_alone_at_the_other_layouts(built, layout, sd, dd):
    """the form with neither pass is not bound to 4:2:0: 67 x 37, two resident frames"""
    import torch
    w, h = 67, 37
    frames = [m.frame("random", w, h, t, sd, layout) for t in range(2)]
    wants = [m.scaled_frame(fr, sd, dd, layout, layout) for fr in frames]
    dt = np.uint8 if dd == 8 else np.uint16
    ctx = hip.Ctx(0)
    flt = hip.format_scaled_device_filter(ctx, w, h, m.SUB[layout], m.SUB[layout], sd, dd)
    try:
        dev_in = [[_padded(p) for p in fr] for fr in frames]
        outs = [[_padded(np.full_like(p, 7)) for p in wants[0]] for _ in range(2)]
        torch.cuda.synchronize()
        arr_in = (hip.DevFrame * 2)(*[hip.dev_frame(f) for f in dev_in])
        arr_out = (hip.DevFrame * 2)(*[hip.dev_frame(o) for o in outs])
        assert flt.process_dev(arr_in, 0, arr_out) == 2
        ctx.sync()
        for i in range(2):
            for c in range(3):
                np.testing.assert_array_equal(_host(outs[i][c], dt), wants[i][c], err_msg=f"frame {i} plane {c}")
    finally:
        flt.close()
        ctx.close()


def test_create_declines(built):
    """a higher target depth, depths outside 8 / 10 / 12, more chroma samples, nothing to do, a resampled chroma direction
    under 11 samples"""
    ctx = hip.Ctx(0)
    try:
        for src, dst, sd, dd, w, h in [
                ((1, 0), (1, 1), 8, 10, 128, 72), ((0, 0), (1, 0), 10, 12, 128, 72), ((1, 1), (1, 1), 8, 10, 128, 72),
                ((1, 0), (1, 1), 9, 8, 128, 72), ((1, 0), (1, 1), 16, 8, 128, 72), ((1, 0), (1, 1), 10, 6, 128, 72),
                ((1, 1), (1, 0), 10, 8, 128, 72), ((1, 0), (0, 0), 12, 8, 128, 72), ((0, 0), (0, 1), 10, 8, 128, 72),
                ((1, 1), (1, 1), 10, 10, 128, 72),
                ((1, 0), (1, 1), 10, 8, 128, 10), ((0, 0), (1, 0), 12, 10, 10, 72), ((0, 0), (1, 1), 12, 8, 128, 10)]:
            with pytest.raises(hip.HipError, match="(?i)unsupported|not supported"):
                hip.format_scaled_device_filter(ctx, w, h, src, dst, sd, dd)
        # at equal depth it is the chroma down-sampling, and without a pass it takes any plane size
        hip.format_scaled_device_filter(ctx, 128, 72, (1, 0), (1, 1), 10, 10).close()
        hip.format_scaled_device_filter(ctx, 8, 4, (1, 1), (1, 1), 10, 8).close()
    finally:
        ctx.close()


def test_drop_in_still_declines_what_nothing_asks_for(built):
    """without the registry's mark the depth-only step stays format_kernel's and a biplanar target is declined; a higher
    depth with fewer chroma samples is declined as before"""
    for stream, sd, target in [("422", 10, "nv12"), ("420", 10, "nv12"), ("420", 12, "p010le"), ("422", 8, "yuv420p10le"),
                               ("444", 10, "yuv422p12le")]:
        with pytest.raises(RuntimeError):
            hbrt.Chain(hip.filters(), [("hb_filter_format_hip", f"format={target}")], 128, 72, _fmt(stream, sd))
    # the mark outside of a device-resident run changes nothing: there is no adapter to repack
    with pytest.raises(RuntimeError):
        hbrt.Chain(hip.filters(), [("hb_filter_format_hip", "format=nv12:hip-planar-step=1")], 128, 72, _fmt("422", 10))


# ---- jobs ---------------------------------------------------------------------------------------------------------------
def _job(target, src, depth, kind="random", w=66, h=38, n=3):
    """[lapsharp, format=<target>] on a yuv<src>p<depth> job with the HIP objects registered (the drop-in object stands in
    for the list entry libhb's own `format` would be: the swap leaves an object that already is the drop-in alone).
    Returns (stage names, OutFrames, the lapsharp oracle's frames)."""
    import oracle_stream as os_
    import golden_cases as gc
    F = hbrt.FILTER_ID
    flt = hip.filters()
    # With the drop-in registered as its own id's filter, a library from before the scaled form hands a declining init()
    # itself as its fallback, over and over: fail here, before a job is opened, rather than spin inside one.  (The guard
    # against that loop came into hb_hip_filter_init_failed together with this entry point.)
    assert hasattr(hip.lib(), "hbhip_format_scaled_create"), "libhbhip.so has no hbhip_format_scaled_create"
    frames = [m.frame(kind, w, h, t, depth, src) for t in range(n)]
    hbrt.register_filters(flt, {F["lapsharp"]: "hb_filter_lapsharp_hip", F["format"]: "hb_filter_format_hip"})
    try:
        names, got = hbrt.run_job([(F["lapsharp"], LAP), (F["format"], f"format={target}")], frames, pix_fmt=_fmt(src, depth))
    finally:
        hbrt.register_filters(flt, {F["lapsharp"]: None, F["format"]: None})
    return names, got, os_.lapsharp_stream(frames, [gc.lap(depth=depth)] * n)


def _four_stages(names):
    assert len(names) == 4, names
    assert names[0] == "HIP upload adapter" and names[2] == "Format (HIP)" and names[3] == "HIP download adapter"
    assert "HIP" in names[1] and "harp" in names[1]


def _check_biplanar(got, want3, depth):
    assert len(got) == len(want3)
    for t, fr in enumerate(want3):
        want = bm.merge(fr, depth)
        assert len(got[t].planes) == 2
        for p in range(2):
            assert got[t].planes[p].dtype == want[p].dtype and got[t].planes[p].shape == want[p].shape
            np.testing.assert_array_equal(got[t].planes[p], want[p], err_msg=f"frame {t} plane {p}")


def test_job_422_10_bit_to_yuv420p(built):
    names, got, sharp = _job("yuv420p", "422", 10)
    _four_stages(names)
    _check(got, sharp, 10, 8, "422", "420", "job")


def test_job_422_10_bit_to_nv12(built):
    names, got, sharp = _job("nv12", "422", 10)
    _four_stages(names)
    _check_biplanar(got, [m.scaled_frame(fr, 10, 8, "422", "420") for fr in sharp], 8)


def test_job_420_10_bit_to_nv12_is_the_scaler_not_the_unscaled_copy(built):
    """the depth-only scaled form.  format_kernel's 10 -> 8 on the same frames, interleaved, is NOT the result: Cr is
    dithered three columns on."""
    names, got, sharp = _job("nv12", "420", 10)
    _four_stages(names)
    _check_biplanar(got, [m.scaled_frame(fr, 10, 8, "420", "420") for fr in sharp], 8)
    plain = hbrt.run_stream(hip.filters(), [("hb_filter_format_hip", "format=yuv420p")], sharp, pix_fmt=_fmt("420", 10))
    differ = 0
    for t in range(len(sharp)):
        unscaled = bm.merge(tuple(plain[t].planes), 8)
        np.testing.assert_array_equal(got[t].planes[0], unscaled[0])          # (luma and Cb: the dither matrices nest)
        differ += int((got[t].planes[1] != unscaled[1]).sum())
    assert differ > 0


def test_job_420_10_bit_to_p010le_is_an_exact_repack(built):
    """the identity step: the entry passes the frames through and the download adapter repacks them"""
    names, got, sharp = _job("p010le", "420", 10)
    _four_stages(names)
    _check_biplanar(got, sharp, 10)


def test_job_444_10_bit_to_p010le_and_420_12_bit_to_p010le(built):
    """the equal-depth resample and the depth-only 12 -> 10 behind a biplanar target"""
    names, got, sharp = _job("p010le", "444", 10)
    _four_stages(names)
    _check_biplanar(got, [m.scaled_frame(fr, 10, 10, "444", "420") for fr in sharp], 10)
    names, got, sharp = _job("p010le", "420", 12)
    _four_stages(names)
    _check_biplanar(got, [m.scaled_frame(fr, 12, 10, "420", "420") for fr in sharp], 10)


def test_job_8_bit_422_under_p010le_is_not_rewritten(built):
    """8 bits under a 10-bit target: the entry is not marked, init() fails as before, and the download adapter is told
    nothing: the run ends planar.  (The drop-in is registered as its own id's filter here, so nothing is left to fall
    back to and the entry is dropped: the run's adapters stay around the lapsharp and deliver the stream's own format.)"""
    names, got, sharp = _job("p010le", "422", 8)
    assert len(names) == 3 and names[0] == "HIP upload adapter" and names[2] == "HIP download adapter", names
    assert "HIP" in names[1] and "harp" in names[1]
    assert len(got) == len(sharp)
    for t, fr in enumerate(sharp):
        assert len(got[t].planes) == 3
        for c in range(3):
            np.testing.assert_array_equal(got[t].planes[c], fr[c], err_msg=f"frame {t} plane {c}")


def test_job_whose_planar_step_declines_ends_planar(built):
    """[lapsharp, format=nv12] on yuv422p10le with ten chroma rows: the entry is marked, its init() declines (libswscale
    cuts its filter short under 11 samples), and the run in front of it ends planar through a plain download adapter.
    (Dropped instead of replaced, as in the test above: the drop-in is registered as its own id's filter.)"""
    names, got, sharp = _job("nv12", "422", 10, w=128, h=10)
    assert len(names) == 3 and names[0] == "HIP upload adapter" and names[2] == "HIP download adapter", names
    assert len(got) == len(sharp)
    for t, fr in enumerate(sharp):
        assert len(got[t].planes) == 3
        for c in range(3):
            np.testing.assert_array_equal(got[t].planes[c], fr[c], err_msg=f"frame {t} plane {c}")
