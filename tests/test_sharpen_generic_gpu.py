"""GPU parity, tolerance 0: the sharpen kernels that tests/test_lapsharp_wide_gpu.py and test_unsharp_strips_and_edges do
not reach, on device-resident frames against the oracle (csrc/sharpen.hip; the oracle itself is held to the reference at
these shapes by tests/test_sharpen16_oracle_cpu.py):

  lapsharp3_rows16_kernel      depth 10 / 12, every plane a 3 x 3 table           test_lap3_*
  lapsharp16_kernel<5>, <3>    depth 10 / 12, some plane log / isolog             test_lap5_*[10|12]
  lapsharp_kernel<5>, <3>      depth 8, some plane log / isolog                   test_lap5_*[8]
  blur_mix_kernel<uint16_t>    unsharp / chroma smooth at depth 10 / 12           test_blur_*
  blur_mix_kernel<uint8_t>     unsharp / chroma smooth at depth 8, a size of 11 - 15

The shapes sit where these kernels can go wrong: planes narrower than a thread's columns and than the mirrored stride
padding the 16-bit lapsharp kernels rebuild, every stride_border of a 64-byte row, a few rows, one off a thread, a
workgroup or a tile, more frames than a launch takes, pitches and bases off the alignment the direct path wants; the
contents hold both clamp ends and take the binomial sums through their 2^32 wrap (all max from size 13 at 10 / 12 bits, at
size 15 at 8 bits).  Rows carry junk behind the width, which no kernel may read into a filtered sample or write over.
The cases and their guards against a vacuous pass are tests/sharpen_cases.py's."""
import numpy as np
import pytest

from handbrake_amd import hbrt, hip
import oracle_lib as ol
import sharpen_cases as sc
import sharpen_dev as sd

pytestmark = pytest.mark.gpu


def _cases(name):
    args = sc.GPU_CASES[name][0]
    return pytest.mark.parametrize("args", args, ids=[sc.case_id(a) for a in args])


def _check(name, args):
    sd.check_jobs(sc.GPU_CASES[name][1](*args), exempt=sc.case_id(args) in sc.CLAMP_EXEMPT.get(name, ()))


# ---------------------------------------------------------------- lapsharp3_rows16_kernel
@_cases("lap3_widths")
def test_lap3_widths(built, args):
    _check("lap3_widths", args)


@_cases("lap3_heights")
def test_lap3_heights(built, args):
    _check("lap3_heights", args)


@_cases("lap3_content")
def test_lap3_content(built, args):
    _check("lap3_content", args)


@_cases("lap3_frames")
def test_lap3_frames_per_call(built, args):
    """a launch takes up to 16 frames: 17 are a launch of 16 and one of 1"""
    for job in sc.GPU_CASES["lap3_frames"][1](*args):
        launches = {}
        sd.check_job(job, launches=launches)
        assert launches == {"lapsharp_3x3": -(-args[0] // 16)}, sc.describe(job)


@_cases("lap3_layouts")
def test_lap3_pitch_and_base(built, args):
    """a pitch or a base off 16 bytes takes the frames through aligned copies (SimpleFilter::process_dev_batch): the same
    result"""
    _check("lap3_layouts", args)


# ---------------------------------------------------------------- lapsharp_kernel<S>, lapsharp16_kernel<S>
@_cases("lap5_widths")
def test_lap5_widths(built, args):
    _check("lap5_widths", args)


@_cases("lap5_heights")
def test_lap5_heights(built, args):
    _check("lap5_heights", args)


@_cases("lap5_content")
def test_lap5_content(built, args):
    _check("lap5_content", args)


@_cases("lap5_frames")
def test_lap5_frames_per_call(built, args):
    """this path goes frame by frame, a launch per kernel size present: every frame must still arrive"""
    for job in sc.GPU_CASES["lap5_frames"][1](*args):
        launches = {}
        sd.check_job(job, launches=launches)
        sizes = {"lapsharp_3x3" if k in ("lap", "isolap") else "lapsharp_5x5" for k in job.par[0]}
        assert launches == {name: len(job.frames) for name in sizes}, sc.describe(job)


# ---------------------------------------------------------------- blur_mix_kernel
@_cases("blur_widths")
def test_blur_widths(built, args):
    _check("blur_widths", args)


@_cases("blur_heights")
def test_blur_heights(built, args):
    _check("blur_heights", args)


@_cases("blur_content")
def test_blur_content(built, args):
    """ones and extremes at sizes 13 and 15 (size 15 at 8 bits) take the uint32 sums through their wrap"""
    _check("blur_content", args)


@_cases("blur_frames")
def test_blur_frames_per_call(built, args):
    for job in sc.GPU_CASES["blur_frames"][1](*args):
        launches = {}
        sd.check_job(job, launches=launches)
        name = job.filter + "_blur_mix"
        assert launches.pop(name) == len(job.frames), sc.describe(job)             # blur_mix_kernel, a launch per frame
        assert launches == ({"plane_copy": len(job.frames)} if job.filter == "chroma_smooth" else {}), sc.describe(job)


@_cases("blur_layouts")
def test_blur_pitch_and_base(built, args):
    _check("blur_layouts", args)


# ---------------------------------------------------------------- through the plugins, host frames
@pytest.mark.parametrize("content", ["random", "extremes"])
@pytest.mark.parametrize("w,h", [(58, 10), (62, 10), (66, 12)])
def test_plugins_depth10(built, w, h, content):
    """hb_filter_lapsharp_hip / hb_filter_unsharp_hip on 4:2:0 10-bit host frames: stride_border comes from the buffer's own
    stride here (3, 1 and 15 for luma, 1, 0 and 15 for chroma)"""
    depth = 10
    frames = [tuple(fr) for fr in sc.frames(2, w, h, (1, 1), depth, content)]
    fmt = hbrt.PIX_FMT[("2x2", depth)]

    def eq(got, want, what):
        assert len(got) == len(want), what
        for t in range(len(want)):
            for c in range(3):
                np.testing.assert_array_equal(got[t].planes[c], want[t][c], err_msg=f"{what} {w}x{h} {content} frame {t} plane {c}")
    for (ky, sy), (kc, sc_) in ((("isolap", 0.35), ("isolap", 0.35)), (("isolog", 1.1), ("lap", 0.4))):
        got = hbrt.run_stream(hip.filters(), [("hb_filter_lapsharp_hip", f"y-strength={sy}:y-kernel={ky}:cb-strength={sc_}:cb-kernel={kc}")],
                              frames, pix_fmt=fmt)
        want = [[ol.orc_lapsharp_plane(fr[c], s, k, depth) for c, (k, s) in enumerate(((ky, sy), (kc, sc_), (kc, sc_)))] for fr in frames]
        eq(got, want, f"lapsharp {ky} / {kc}")
        if content == "random":
            assert not np.array_equal(want[0][0], frames[0][0]) and not np.array_equal(want[0][1], frames[0][1])
    got = hbrt.run_stream(hip.filters(), [("hb_filter_unsharp_hip", "y-strength=1.5:y-size=13:cb-strength=0.25:cb-size=5")], frames, pix_fmt=fmt)
    want = [[ol.orc_unsharp_plane(fr[c], s, z, depth) for c, (s, z) in enumerate(((1.5, 13), (0.25, 5), (0.25, 5)))] for fr in frames]
    eq(got, want, "unsharp 13 / 5")
