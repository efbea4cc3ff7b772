"""GPU: the Format drop-in's chroma down-sampling (4:2:2 -> 4:2:0, 4:4:4 -> 4:2:2, 4:4:4 -> 4:2:0 at equal depth) against
the integer model tests/format_resample_model.py, tolerance 0 (parity unpinned: libswscale is outside the reference tree)."""
import ctypes as C

import numpy as np
import pytest

from handbrake_amd import hbrt, hip
import format_resample_model as m

pytestmark = pytest.mark.gpu
LAYOUT = {"444": "1x1", "422": "2x1", "420": "2x2"}
DEPTHS = (8, 10, 12)


def _fmt(layout, depth):
    return hbrt.PIX_FMT[(LAYOUT[layout], depth)]


def _name(layout, depth):
    return f"yuv{layout}p" + {8: "", 10: "10le", 12: "12le"}[depth]


def _through_drop_in(frames, depth, src, dst):
    return hbrt.run_stream(hip.filters(), [("hb_filter_format_hip", f"format={_name(dst, depth)}")], frames,
                           pix_fmt=_fmt(src, depth))


def _check(got, frames, depth, src, dst, what=""):
    assert len(got) == len(frames)
    for t, fr in enumerate(frames):
        want = m.resample_frame(fr, depth, src, dst)
        assert len(got[t].planes) == 3
        for c in range(3):
            assert got[t].planes[c].dtype == want[c].dtype and got[t].planes[c].shape == want[c].shape
            np.testing.assert_array_equal(got[t].planes[c], want[c], err_msg=f"{what} {src}->{dst} {depth} bits frame {t} plane {c}")


def test_format_yuv420p_on_a_yuv422p_stream(built):
    """the ordinary job: a 4:2:2 source in front of a 4:2:0-only encoder (init() declined this before the feature)"""
    frames = [m.frame("progressive", 66, 38, t, 8, "422") for t in range(2)]
    _check(_through_drop_in(frames, 8, "422", "420"), frames, 8, "422", "420")


@pytest.mark.parametrize("w,h", [(66, 38), (67, 37)])
@pytest.mark.parametrize("depth", DEPTHS)
@pytest.mark.parametrize("src,dst", m.PAIRS)
def test_pairs_depths_odd_planes(built, src, dst, depth, w, h):
    """odd planes, ragged dword tails, an odd source size (the filter's step is then not 2)"""
    frames = [m.frame("random", w, h, t, depth, src) for t in range(2)]
    _check(_through_drop_in(frames, depth, src, dst), frames, depth, src, dst)


@pytest.mark.parametrize("depth", [8, 10])
@pytest.mark.parametrize("src,dst", m.PAIRS)
def test_more_than_one_workgroup_each_way(built, src, dst, depth):
    """530 x 134: the target's chroma planes are wider than a workgroup's 256 columns and taller than its 32 / 64 rows"""
    frames = [m.frame("random", 530, 134, 0, depth, src)]
    _check(_through_drop_in(frames, depth, src, dst), frames, depth, src, dst)


@pytest.mark.parametrize("kind", ["rows", "bars", "flat"])
@pytest.mark.parametrize("src,dst", m.PAIRS)
def test_clamp_and_flat_content(built, src, dst, kind):
    for depth in DEPTHS:
        frames = [m.frame(kind, 66, 38, t, depth, src) for t in range(2)]
        got = _through_drop_in(frames, depth, src, dst)
        _check(got, frames, depth, src, dst, kind)
        if kind == "flat":
            assert int(got[0].planes[1].min()) == int(got[0].planes[1].max()) == (1 << depth) - 1
        if kind == "bars":
            assert int(got[0].planes[1].min()) == 0 and int(got[0].planes[1].max()) == (1 << depth) - 1


@pytest.mark.parametrize("src,dst,w,h", [("422", "420", 24, 11), ("444", "422", 11, 6), ("444", "420", 11, 11)])
def test_smallest_planes_taken(built, src, dst, w, h):
    """eleven chroma samples in a resampled direction: libswscale's nine taps are all there, and every row is an edge row"""
    frames = [m.frame("random", w, h, 0, 10, src)]
    _check(_through_drop_in(frames, 10, src, dst), frames, 10, src, dst)


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


@pytest.mark.parametrize("depth", [8, 10])
@pytest.mark.parametrize("src,dst", m.PAIRS)
def test_seventeen_frames_one_full_burst_plus_one(built, src, dst, depth):
    """130 x 70, 17 device-resident frames in one call: a launch of 16 and a launch of one.  The 17 inputs are four
    frames shared between the entries; they are only read."""
    import torch
    w, h, n = 130, 70, 17
    frames = [m.frame("random" if t & 1 else "progressive", w, h, t, depth, src) for t in range(4)]
    wants = [m.resample_frame(fr, depth, src, dst) for fr in frames]
    dt = np.uint8 if depth == 8 else np.uint16
    ctx = hip.Ctx(0)
    flt = hip.format_resample_device_filter(ctx, w, h, m.SUB[src], m.SUB[dst], depth)
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
                np.testing.assert_array_equal(_host(outs[i][c], dt), wants[i % 4][c], err_msg=f"frame {i} plane {c}")
        for k in range(4):
            for c in range(3):
                np.testing.assert_array_equal(_host(dev_in[k][c], dt), frames[k][c], err_msg=f"input {k} plane {c} was written")
    finally:
        flt.close()
        ctx.close()


def test_device_resident_job_422_10_bit_to_420(built):
    """[lapsharp, format=yuv420p10le] on a yuv422p10le job with the HIP objects registered: one device-resident run, the
    frames leave it as yuv420p10le and equal the model applied to the lapsharp oracle's output"""
    import oracle_stream as os_
    import golden_cases as gc
    F = hbrt.FILTER_ID
    flt = hip.filters()
    w, h, n = 66, 38, 3
    frames = [m.frame("progressive", w, h, t, 10, "422") for t in range(n)]
    # The drop-in has to take these settings before it may stand in for the job's own `format` entry: with the same object
    # registered as the CPU filter of its id, a declining init() would be handed itself as its fallback, over and over.
    hbrt.Chain(flt, [("hb_filter_format_hip", "format=yuv420p10le")], w, h, _fmt("422", 10)).close()
    hbrt.register_filters(flt, {F["lapsharp"]: "hb_filter_lapsharp_hip", F["format"]: "hb_filter_format_hip"})
    try:
        names, got = hbrt.run_job([(F["lapsharp"], "y-strength=0.2:y-kernel=isolap"), (F["format"], "format=yuv420p10le")],
                                  frames, pix_fmt=_fmt("422", 10))
    finally:
        hbrt.register_filters(flt, {F["lapsharp"]: None, F["format"]: None})
    assert names[0] == "HIP upload adapter" and names[2] == "Format (HIP)" and names[3] == "HIP download adapter"
    assert len(names) == 4 and "HIP" in names[1] and "harp" in names[1]
    sharp = os_.lapsharp_stream(frames, [gc.lap(depth=10)] * 3)
    _check(got, sharp, 10, "422", "420", "job")


@pytest.mark.parametrize("stream,target,w,h", [
    ("420", "yuv422p", 128, 72),              # upsampling: taken only as a marked step behind another drop-in
    ("420", "yuv444p", 128, 72),
    ("422", "yuv444p", 128, 72),
    ("422", "yuv420p10le", 128, 72),          # fewer chroma samples AND another depth: one swscale pass with its own dither
    ("444", "yuv422p12le", 128, 72),
    ("422", "nv12", 128, 72),                 # biplanar and RGB targets
    ("444", "gbrp", 128, 72),
    ("422", "yuv420p", 128, 10),              # ten chroma rows: libswscale cuts its filter short
    ("444", "yuv422p", 10, 72),
    ("444", "yuv420p", 128, 10),
])
def test_declined_targets_keep_the_cpu_filter(built, stream, target, w, h):
    with pytest.raises(RuntimeError):
        hbrt.Chain(hip.filters(), [("hb_filter_format_hip", f"format={target}")], w, h, _fmt(stream, 8))


def test_create_declines_what_is_not_down_sampling(built):
    ctx = hip.Ctx(0)
    try:
        for src, dst, depth in [((1, 1), (1, 0), 8), ((1, 0), (0, 0), 8), ((1, 1), (1, 1), 8), ((0, 0), (0, 0), 10),
                                ((1, 0), (1, 1), 9), ((0, 0), (1, 1), 16), ((0, 0), (0, 1), 8)]:
            with pytest.raises(hip.HipError, match="(?i)unsupported|not supported"):
                hip.format_resample_device_filter(ctx, 128, 72, src, dst, depth)
    finally:
        ctx.close()
