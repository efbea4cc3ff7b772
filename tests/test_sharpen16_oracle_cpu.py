"""CPU, tolerance 0: the sharpen-family oracle (orc_lapsharp_plane16, orc_unsharp_plane16, orc_chroma_smooth_plane16 and
their 8-bit forms) against the reference's own filters at the shapes and contents tests/test_sharpen_generic_gpu.py holds
the HIP kernels to - planes narrower than the mirrored stride padding, a few rows high, either side of a 64-byte row, all
0, all max and 0 / max content -, so that a difference found on the GPU is the kernel's.  The last test walks the GPU
file's jobs with the oracle alone: its guards against a vacuous pass must hold before anything goes to a GPU."""
import numpy as np
import pytest

from handbrake_amd import hbrt
import oracle_lib as ol
import sharpen_cases as sc

needs_ref = pytest.mark.skipif(ol.ref() is None, reason="oracle/_ref/libhbref.so not built")

WIDTHS = list(range(1, 12)) + list(range(29, 35)) + [61, 63, 64, 65, 66] + list(range(127, 131))    # at height 9
HEIGHTS = [1, 2, 3, 4, 5, 6, 7, 9, 15, 16, 17, 33]                                                    # at width 66
SHAPES = [(w, 9) for w in WIDTHS] + [(66, h) for h in HEIGHTS if h != 9] + [(1, 1), (2, 2), (5, 5)]
LAP = (("lap", 1.5), ("isolap", 0.35), ("isolog", 1.1), ("log", 0.2))
SIZES = (3, 5, 7, 9, 11, 13, 15)
STRENGTHS = (1.5, 0.25)
# per depth: the lapsharp settings and blur sizes.  Depth 8 adds what tests/test_oracle_vs_ref.py has on progressive and
# random content only: the 5 x 5 tables and the sizes past blur_rows8_kernel.
PLAN = {8: (LAP[2:], SIZES[4:]), 10: (LAP, SIZES), 12: (LAP, SIZES)}


def _content_frames(w, h, depth, sub="1x1"):
    """one frame of each content, seeded from the shape"""
    lc = ol.SUBSAMPLING[sub]
    rng = np.random.default_rng([w, h, depth])
    return [tuple(sc.frame(rng, w, h, lc[0], lc[1], depth, content)) for content in sc.CONTENTS]


def _eq(got, want, what):
    assert len(got) == len(want), what
    for t in range(len(want)):
        for c in range(3):
            np.testing.assert_array_equal(got[t].planes[c], want[t][c], err_msg=f"{what} {sc.CONTENTS[t]} plane {c}")


def _ref(stage, settings, frames, sub, depth):
    return hbrt.run_stream(ol.ref(), [(stage, settings)], frames, pix_fmt=hbrt.PIX_FMT[(sub, depth)])


def _lapsharp(frames, sub, depth, ky, sy, kc, sc_):
    got = _ref("hb_filter_lapsharp", f"y-strength={sy}:y-kernel={ky}:cb-strength={sc_}:cb-kernel={kc}", frames, sub, depth)
    want = [[ol.orc_lapsharp_plane(fr[c], s, k, depth) for c, (k, s) in enumerate(((ky, sy), (kc, sc_), (kc, sc_)))] for fr in frames]
    _eq(got, want, f"lapsharp {ky} {sy} / {kc} {sc_} depth {depth} {sub} {frames[0][0].shape}")


def _unsharp(frames, sub, depth, sy, zy, sc_, zc):
    got = _ref("hb_filter_unsharp", f"y-strength={sy}:y-size={zy}:cb-strength={sc_}:cb-size={zc}", frames, sub, depth)
    want = [[ol.orc_unsharp_plane(fr[c], s, z, depth) for c, (s, z) in enumerate(((sy, zy), (sc_, zc), (sc_, zc)))] for fr in frames]
    _eq(got, want, f"unsharp {sy} {zy} / {sc_} {zc} depth {depth} {sub} {frames[0][0].shape}")


def _chroma_smooth(frames, sub, depth, strength, size):
    got = _ref("hb_filter_chroma_smooth", f"cb-strength={strength}:cb-size={size}", frames, sub, depth)
    want = [[fr[0]] + [ol.orc_chroma_smooth_plane(fr[c], strength, size, depth) for c in (1, 2)] for fr in frames]
    _eq(got, want, f"chroma smooth {strength} {size} depth {depth} {sub} {frames[0][0].shape}")


@needs_ref
@pytest.mark.parametrize("w,h", SHAPES, ids=[f"{w}x{h}" for w, h in SHAPES])
def test_oracle_matches_reference_444(built, w, h):
    for depth, (lap, sizes) in PLAN.items():
        frames = _content_frames(w, h, depth)
        for kern, strength in lap:
            _lapsharp(frames, "1x1", depth, kern, strength, kern, strength)
        for size in sizes:
            for strength in STRENGTHS:
                _unsharp(frames, "1x1", depth, strength, size, strength, size)
                _chroma_smooth(frames, "1x1", depth, strength, size)


@needs_ref
@pytest.mark.parametrize("depth", [8, 10, 12])
def test_oracle_matches_reference_420_odd(built, depth):
    """4:2:0 with an odd luma size: chroma planes of 34 x 10 beside luma of 67 x 19, kernels and sizes that differ by plane"""
    frames = _content_frames(67, 19, depth, "2x2")
    _lapsharp(frames, "2x2", depth, "isolog", 1.1, "lap", 0.4)
    _lapsharp(frames, "2x2", depth, "isolap", 0.35, "log", 0.6)
    _unsharp(frames, "2x2", depth, 1.5, 13, 0.25, 5)
    _unsharp(frames, "2x2", depth, 0.25, 3, 1.5, 15)
    _chroma_smooth(frames, "2x2", depth, 1.5, 15)
    _chroma_smooth(frames, "2x2", depth, 0.25, 7)


def test_case_builders():
    for depth in (8, 10, 12):
        top = sc.vmax(depth)
        rng = np.random.default_rng(depth)
        for content in sc.CONTENTS:
            p = sc.plane(rng, (33, 65), depth, content)
            assert p.dtype == sc.dtype(depth) and p.shape == (33, 65) and int(p.max()) <= top, content
        assert set(np.unique(sc.plane(rng, (33, 65), depth, "extremes"))) == {0, top}
        chk = sc.plane(rng, (4, 5), depth, "checker")
        assert chk[0, 0] == 0 and chk[0, 1] == top and chk[1, 0] == top and chk[1, 1] == 0
        assert not sc.plane(rng, (4, 5), depth, "zeros").any() and (sc.plane(rng, (4, 5), depth, "ones") == top).all()
    fr = sc.frames(2, 67, 19, (1, 1), 10)
    assert [p.shape for p in fr[0]] == [(19, 67), (10, 34), (10, 34)] and not np.array_equal(fr[0][0], fr[1][0])
    np.testing.assert_array_equal(fr[1][2], sc.frames(2, 67, 19, (1, 1), 10)[1][2])                 # seeded from the shape
    # stride_border by width: 64-byte rows of 16-bit samples (lapsharp.c:137-145)
    assert [sc.stride_border(w, 10) for w in (1, 27, 28, 31, 32, 33, 35, 64, 65)] == [15, 2, 2, 0, 0, 15, 14, 0, 15]
    assert [sc.stride_border(w, 8) for w in (1, 61, 64, 65)] == [31, 1, 0, 31]
    assert not sc.lap_filtered(9, 7, 10, "lap") and sc.lap_filtered(27, 7, 10, "lap") and not sc.lap_filtered(27, 3, 10, "lap")
    assert not sc.lap_filtered(66, 5, 10, "log") and sc.lap_filtered(66, 6, 10, "log") and not sc.lap_filtered(11, 9, 12, "isolog")


@pytest.mark.parametrize("name", sorted(sc.GPU_CASES))
def test_gpu_case_guards(built, name):
    """every job of tests/test_sharpen_generic_gpu.py through the oracle alone: copy-only planes come back as they went in,
    filtered random planes do not, and an item's random planes reach both clamp ends unless the item is listed in
    CLAMP_EXEMPT - a list that says what the oracle says and stays below one item in ten of a parametrization"""
    args, jobs = sc.GPU_CASES[name]
    missing = set()
    for a in args:
        guard = sc.Guard()
        for job in jobs(*a):
            guard.note(job, sc.expected(job))
        if guard.missing():
            missing.add(sc.case_id(a))
    assert missing == set(sc.CLAMP_EXEMPT.get(name, ())), name
    assert 10 * len(missing) <= len(args), name
