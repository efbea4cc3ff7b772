"""What the sharpen-family edge tests share (tests/test_sharpen16_oracle_cpu.py, tests/test_sharpen_generic_gpu.py): plane
builders by depth, the shape lists, the jobs of every GPU parametrization, what the oracle expects of a job and the
guards against a vacuous pass.  Nothing here needs a GPU: the CPU file walks the very jobs the GPU file runs.

A job is one filter call: its frames (lists of three planes), settings and the layout of the device planes.  `par` is
(kernels, strengths) per plane for lapsharp and (strengths, sizes) per plane for unsharp / chroma smooth (chroma smooth:
luma strength 0, the plane is copied)."""
import collections

import numpy as np

import oracle_lib as ol

CONTENTS = ("random", "extremes", "checker", "zeros", "ones")
SUBSAMPLINGS = {"420": (1, 1), "444": (0, 0)}
DEPTHS16 = (10, 12)

Job = collections.namedtuple("Job", "filter w h depth lcw lch frames par content how")


def dtype(depth):
    return np.uint8 if depth == 8 else np.uint16


def vmax(depth):
    return (1 << depth) - 1


def plane(rng, shape, depth, content):
    """random: the full range 0 .. max; extremes: random 0 / max; checker: 0 / max by (x + y) & 1; zeros; ones: all max"""
    top, dt = vmax(depth), dtype(depth)
    if content == "random":
        return rng.integers(0, top + 1, size=shape).astype(dt)
    if content == "extremes":
        return (rng.integers(0, 2, size=shape) * top).astype(dt)
    if content == "checker":
        return ((np.add.outer(np.arange(shape[0]), np.arange(shape[1])) & 1) * top).astype(dt)
    return np.full(shape, {"zeros": 0, "ones": top}[content], dt)


def frame(rng, w, h, lcw, lch, depth, content):
    return [plane(rng, s, depth, content) for s in [(h, w)] + [(-(-h >> lch), -(-w >> lcw))] * 2]


def frames(n, w, h, lc, depth, content="random"):
    """n frames, seeded from the shape"""
    rng = np.random.default_rng([w, h, depth, lc[0], lc[1]])
    return [frame(rng, w, h, lc[0], lc[1], depth, content) for _ in range(n)]


# ---------------------------------------------------------------- what the reference filters of a plane
def stride_border(w, depth):
    """lapsharp.c:145 with hb_image_stride's rows (a multiple of 64 bytes), in samples"""
    bps = 1 if depth == 8 else 2
    return ((w * bps + 63) // 64 * 64 // bps - w) // 2


def lap_filtered(w, h, depth, kernel):
    """whether lapsharp filters any sample of a w x h plane: rows HI .. h - HI, columns stride_border + HI ..
    min(w - 1, w + stride_border - HI) (lapsharp.c:167-171), HI = 2 for the 3 x 3 tables and 3 for the 5 x 5 ones"""
    hi = 2 if kernel in ("lap", "isolap") else 3
    sb = stride_border(w, depth)
    return h - hi >= hi and min(w - 1, w + sb - hi) >= sb + hi


def clamp_ends(flt, depth):
    """the two values a result is clamped to (chroma_smooth.c:233-235: max / 16 .. max - max / 16 of max = 1 << depth)"""
    if flt == "chroma_smooth":
        return (1 << depth) // 16, (1 << depth) - (1 << depth) // 16
    return 0, vmax(depth)


def expected(job):
    """the oracle's frames for a job"""
    a, b = job.par
    out = []
    for fr in job.frames:
        if job.filter == "lapsharp":
            out.append([ol.orc_lapsharp_plane(fr[c], b[c], a[c], job.depth) for c in range(3)])
        elif job.filter == "unsharp":
            out.append([ol.orc_unsharp_plane(fr[c], a[c], b[c], job.depth) for c in range(3)])
        else:
            out.append([fr[0].copy()] + [ol.orc_chroma_smooth_plane(fr[c], a[c], b[c], job.depth) for c in (1, 2)])
    return out


def describe(job):
    return f"{job.filter} {job.w}x{job.h} depth {job.depth} chroma >> {job.lcw},{job.lch} {job.content} {job.par} {job.how}"


class Guard:
    """The guards of one test item, fed with every job of the item and what the oracle expects of it.  A plane that is
    copy-only by construction must come out as it went in; a filtered plane of random content must not, and over the
    item's jobs both clamp ends must be reached, per filter and depth, by samples that did not start there."""

    def __init__(self):
        self.ends = {}

    def note(self, job, want):
        lo, hi = clamp_ends(job.filter, job.depth)
        for t, (fr, wf) in enumerate(zip(job.frames, want)):
            for c in range(3):
                what = f"{describe(job)} frame {t} plane {c}"
                ph, pw = fr[c].shape
                if job.filter == "lapsharp":
                    filtered = lap_filtered(pw, ph, job.depth, job.par[0][c])
                else:
                    filtered = job.par[0][c] != 0                      # a blur reaches every sample of a plane
                if not filtered:
                    np.testing.assert_array_equal(wf[c], fr[c], err_msg="copy-only by construction: " + what)
                elif job.content == "random":
                    assert not np.array_equal(wf[c], fr[c]), "the oracle left a filtered plane as it was: " + what
                    seen = self.ends.setdefault((job.filter, job.depth), set())
                    if ((wf[c] == lo) & (fr[c] != lo)).any():
                        seen.add(lo)
                    if ((wf[c] == hi) & (fr[c] != hi)).any():
                        seen.add(hi)

    def missing(self):
        """(filter, depth) of the item whose random planes were filtered without reaching both clamp ends"""
        return sorted(k for k, seen in self.ends.items() if len(seen) < 2)

    def finish(self, exempt=False):
        if not exempt:
            assert not self.missing(), f"no sample reaches both clamp ends: {self.missing()}"


# ---------------------------------------------------------------- lapsharp, every plane a 3 x 3 kernel, depth 10 / 12
# (LapsharpFilter::process_many with rows3: lapsharp3_rows16_kernel, four columns x four rows a thread, 256 x 16 a workgroup)
LAP3_SETTINGS = (("lap", 1.5), ("isolap", 0.35))
LAP3_WIDTHS = (list(range(1, 10))            # inside one thread's four columns; stride_border + 2 > w: all copied
               + list(range(27, 36))         # every stride_border from 2 down to 0 and up to 15: both sides of a 64-byte row
               + list(range(61, 68)) + list(range(253, 260))         # ... of 128 bytes; one workgroup's 256 columns
               + list(range(509, 516)) + [1027])
LAP3_WIDTHS_H = 7
LAP3_HEIGHTS = [1, 2, 3, 4, 5, 7, 8, 9, 15, 16, 17, 37]
LAP3_HEIGHTS_W = (72, 300)
LAP3_CONTENT_SHAPES = ((200, 21), (300, 37))
LAP3_FRAMES = (1, 16, 17)                    # a launch takes up to 16 frames (LS_FRAMES)
LAP3_FRAMES_SHAPE = (136, 19)
LAP3_LAYOUTS = {"pitch+4": dict(pad=4), "pitch+16": dict(pad=16), "pitch+64": dict(pad=64), "base+2": dict(offset=2),
                "base+4": dict(offset=4), "base+16": dict(offset=16), "pitch+16-base+4": dict(pad=16, offset=4)}
LAP3_LAYOUT_WIDTHS = (136, 300)
LAP3_LAYOUT_H = 11


def _lap(w, h, depth, lc, frs, kernels, strengths, content="random", how=None):
    return Job("lapsharp", w, h, depth, lc[0], lc[1], frs, (tuple(kernels), tuple(strengths)), content, how or {})


def _lap3(w, h, lcs, n=2, content="random", how=None):
    for lc in lcs:
        for depth in DEPTHS16:
            frs = frames(n, w, h, lc, depth, content)
            for kern, strength in LAP3_SETTINGS:
                yield _lap(w, h, depth, lc, frs, [kern] * 3, [strength] * 3, content, how)


def lap3_width_jobs(w, lc):
    return _lap3(w, LAP3_WIDTHS_H, [lc])


def lap3_height_jobs(w, h):
    return _lap3(w, h, SUBSAMPLINGS.values(), n=1)


def lap3_content_jobs(content):
    for w, h in LAP3_CONTENT_SHAPES:
        yield from _lap3(w, h, SUBSAMPLINGS.values(), n=1, content=content)


def lap3_frames_jobs(n):
    return _lap3(*LAP3_FRAMES_SHAPE, [(1, 1)], n=n)


def lap3_layout_jobs(w, how):
    return _lap3(w, LAP3_LAYOUT_H, [(1, 1)], how=how)


# ---------------------------------------------------------------- lapsharp with a 5 x 5 plane, depth 8, 10 and 12
# (LapsharpFilter::one_frame, a launch per kernel size present: lapsharp_kernel<5|3> at depth 8, four columns a thread and
# 1024 a workgroup; lapsharp16_kernel<5|3> at depth 10 / 12, two columns a thread and 512 a workgroup)
LAP5_SETTINGS = ((("isolog", 1.1), ("isolog", 1.1)), (("log", 0.2), ("log", 0.2)),
                 (("isolog", 1.1), ("lap", 0.4)),                      # the 3 x 3 instantiation beside the 5 x 5 one
                 (("lap", 1.5), ("log", 0.6)))
LAP5_WIDTHS = {8: list(range(1, 12)) + list(range(61, 68)) + list(range(1021, 1028))}
LAP5_WIDTHS[10] = LAP5_WIDTHS[12] = list(range(1, 12)) + list(range(27, 36)) + list(range(61, 68)) + list(range(509, 516))
LAP5_WIDTHS_H = 9
LAP5_HEIGHTS = [1, 2, 3, 4, 5, 6, 7, 9]
LAP5_HEIGHTS_W = (66, 300)
LAP5_CONTENT_SHAPES = ((70, 50), (300, 21))
LAP5_FRAMES_SHAPE = (136, 19)


def _lap5(w, h, depth, lcs, n=1, content="random"):
    for lc in lcs:
        frs = frames(n, w, h, lc, depth, content)
        for (ky, sy), (kc, sc) in LAP5_SETTINGS:
            yield _lap(w, h, depth, lc, frs, (ky, kc, kc), (sy, sc, sc), content)


def lap5_width_jobs(depth, w):
    return _lap5(w, LAP5_WIDTHS_H, depth, SUBSAMPLINGS.values())


def lap5_height_jobs(depth, w, h):
    return _lap5(w, h, depth, SUBSAMPLINGS.values())


def lap5_content_jobs(depth, content):
    for w, h in LAP5_CONTENT_SHAPES:
        yield from _lap5(w, h, depth, SUBSAMPLINGS.values(), content=content)


def lap5_frames_jobs(depth):
    return _lap5(*LAP5_FRAMES_SHAPE, depth, [(1, 1)], n=3)


# ---------------------------------------------------------------- unsharp / chroma smooth through blur_mix_kernel
# (BlurMixFilter::one_frame: every size at depth 10 / 12, sizes 11 - 15 at depth 8; tiles of 64 x 16 with an apron of
# size / 2 samples)
BLUR_SIZES = {8: (11, 13, 15), 10: (3, 5, 7, 9, 11, 13, 15), 12: (3, 5, 7, 9, 11, 13, 15)}
UNSHARP_STRENGTHS = (1.5, 0.25)
UNSHARP_MIXED_SIZES = ((3, 15), (13, 5))     # luma / chroma; at depth 8 a size above 9 takes the whole frame to this kernel
SMOOTH_STRENGTHS = (2.5, 0.3)                # cb / cr
BLUR_WIDTHS = [1, 2, 3, 7, 8, 9, 15, 16, 63, 64, 65, 127, 128, 129, 200]
BLUR_WIDTHS_H = 18
BLUR_HEIGHTS = [1, 2, 3, 7, 8, 15, 16, 17, 31, 32, 33]
BLUR_HEIGHTS_W = 70
BLUR_CONTENT_SHAPE = (96, 40)
BLUR_FRAMES_SHAPE = (129, 33)
BLUR_LAYOUTS = {"pitch+4": dict(pad=4), "base+2": dict(offset=2)}
BLUR_LAYOUT_SHAPE = (70, 18)


def blur_jobs(w, h, lc, depth, n=1, content="random", how=None):
    frs = frames(n, w, h, lc, depth, content)
    a, b = UNSHARP_STRENGTHS

    def job(flt, strengths, sizes):
        return Job(flt, w, h, depth, lc[0], lc[1], frs, (tuple(strengths), tuple(sizes)), content, how or {})
    for size in BLUR_SIZES[depth]:
        yield job("unsharp", (a, b, b), [size] * 3)                 # either strength on the luma and on the chroma shape
        yield job("unsharp", (b, a, a), [size] * 3)
        yield job("chroma_smooth", (0.0,) + SMOOTH_STRENGTHS, [size] * 3)
    for ysz, csz in UNSHARP_MIXED_SIZES:
        yield job("unsharp", (a, b, b), (ysz, csz, csz))


def blur_shape_jobs(w, h, lc):
    for depth in (8, 10, 12):
        yield from blur_jobs(w, h, lc, depth)


def blur_content_jobs(depth, content, lc):
    return blur_jobs(*BLUR_CONTENT_SHAPE, lc, depth, content=content)


def blur_frames_jobs(depth):
    return blur_jobs(*BLUR_FRAMES_SHAPE, (1, 1), depth, n=3)


def blur_layout_jobs(depth, how):
    return blur_jobs(*BLUR_LAYOUT_SHAPE, (1, 1), depth, how=how)


# ---------------------------------------------------------------- every GPU parametrization, for both files
# name -> (argument tuples of the parametrization, jobs of one of them)
GPU_CASES = {
    "lap3_widths": ([(w, lc) for w in LAP3_WIDTHS for lc in SUBSAMPLINGS.values()], lap3_width_jobs),
    "lap3_heights": ([(w, h) for w in LAP3_HEIGHTS_W for h in LAP3_HEIGHTS], lap3_height_jobs),
    "lap3_content": ([(c,) for c in CONTENTS], lap3_content_jobs),
    "lap3_frames": ([(n,) for n in LAP3_FRAMES], lap3_frames_jobs),
    "lap3_layouts": ([(w, k) for w in LAP3_LAYOUT_WIDTHS for k in LAP3_LAYOUTS],
                     lambda w, k: lap3_layout_jobs(w, LAP3_LAYOUTS[k])),
    "lap5_widths": ([(d, w) for d in (8, 10, 12) for w in LAP5_WIDTHS[d]], lap5_width_jobs),
    "lap5_heights": ([(d, w, h) for d in (8, 10, 12) for w in LAP5_HEIGHTS_W for h in LAP5_HEIGHTS], lap5_height_jobs),
    "lap5_content": ([(d, c) for d in (8, 10, 12) for c in CONTENTS], lap5_content_jobs),
    "lap5_frames": ([(d,) for d in (8, 10, 12)], lap5_frames_jobs),
    "blur_widths": ([(w, lc) for w in BLUR_WIDTHS for lc in SUBSAMPLINGS.values()],
                    lambda w, lc: blur_shape_jobs(w, BLUR_WIDTHS_H, lc)),
    "blur_heights": ([(h, lc) for h in BLUR_HEIGHTS for lc in SUBSAMPLINGS.values()],
                     lambda h, lc: blur_shape_jobs(BLUR_HEIGHTS_W, h, lc)),
    "blur_content": ([(d, c, lc) for d in (8, 10, 12) for c in CONTENTS for lc in SUBSAMPLINGS.values()], blur_content_jobs),
    "blur_frames": ([(d,) for d in (8, 10, 12)], blur_frames_jobs),
    "blur_layouts": ([(d, k) for d in DEPTHS16 for k in BLUR_LAYOUTS], lambda d, k: blur_layout_jobs(d, BLUR_LAYOUTS[k])),
}

# Items whose random planes are filtered but too small to reach both clamp ends (found with the oracle alone,
# tests/test_sharpen16_oracle_cpu.py::test_gpu_case_guards holds the list to what the oracle says and to one item in ten
# of a parametrization).  They are left out of the clamp assertion only: every comparison runs.
CLAMP_EXEMPT = {"blur_widths": ("1-420",)}            # luma of 1 x 18, chroma of 1 x 9


def case_id(args):
    def one(a):
        if isinstance(a, tuple):
            return {v: k for k, v in SUBSAMPLINGS.items()}.get(a, "x".join(map(str, a)))
        return str(a)
    return "-".join(one(a) for a in args)
