"""GPU parity: hqdn3d HIP drop-in vs the oracle (bit-exact, stateful over frames)."""
import functools

import numpy as np
import pytest

from handbrake_amd import hbrt, hip, synth
import oracle_stream as os_
import hqdn3d_dev as hd
from hqdn3d_dev import STRONG, flat_noisy as _flat_noisy

pytestmark = pytest.mark.gpu

CASES = [
    ("", {}),
    ("y-spatial=2:cb-spatial=1.5:cr-spatial=1.5:y-temporal=3:cb-temporal=2.25:cr-temporal=2.25",
     dict(y_spatial=2, cb_spatial=1.5, cr_spatial=1.5, y_temporal=3, cb_temporal=2.25, cr_temporal=2.25)),
    ("y-spatial=0:y-temporal=6:cb-spatial=0:cb-temporal=4", dict(y_spatial=0, y_temporal=6, cb_spatial=0, cb_temporal=4)),
    ("y-spatial=8:cb-spatial=6:y-temporal=0", dict(y_spatial=8, cb_spatial=6, y_temporal=0)),
]


@pytest.mark.parametrize("model", ["progressive", "random"])
@pytest.mark.parametrize("w,h", [(64, 48), (638, 362), (1920, 1080)])
def test_hqdn3d(built, model, w, h):
    frames = synth.stream(model, w, h, 3 if w > 1000 else 5)
    for st, par in CASES:
        got = hbrt.run_stream(hip.filters(), [("hb_filter_denoise_hip", st)], frames)
        want = os_.hqdn3d_stream(frames, par)
        assert len(got) == len(want)
        for t in range(len(want)):
            for c in range(3):
                np.testing.assert_array_equal(got[t].planes[c], want[t][c], err_msg=f"{st} frame {t} plane {c}")


@pytest.mark.parametrize("warmup", [None, "0", "3", "1000"])
@pytest.mark.parametrize("w,h", [(638, 362), (1920, 1080), (2050, 1102)])
def test_speculative_segments_are_exact(built, monkeypatch, warmup, w, h):
    """The segmented recurrences must equal the serial ones whatever the warm-up: 0 / 3 make nearly
    every segment start from a wrong state (all repaired), 1000 makes every warm-up start at the
    chain's first sample, None is the shipped setting."""
    if warmup is None:
        monkeypatch.delenv("HBHIP_HQDN3D_WARMUP", raising=False)
    else:
        monkeypatch.setenv("HBHIP_HQDN3D_WARMUP", warmup)
    frames = _flat_noisy(w, h, 2) + synth.stream("progressive", w, h, 1) + _flat_noisy(w, h, 1, amp=3, seed=8)
    for st, par in (CASES[0], STRONG):
        got = hbrt.run_stream(hip.filters(), [("hb_filter_denoise_hip", st)], frames)
        want = os_.hqdn3d_stream(frames, par)
        for t in range(len(want)):
            for c in range(3):
                np.testing.assert_array_equal(got[t].planes[c], want[t][c], err_msg=f"{st} frame {t} plane {c}")


@pytest.mark.parametrize("depth", [8, 10])
@pytest.mark.parametrize("w,h", [(66, 50), (638, 362), (1920, 1080)])
@pytest.mark.parametrize("case", [0, 1, 2, 3])
def test_hqdn3d_batched_equals_frame_by_frame(built, case, w, h, depth):
    """Several frames per call (hbhip_filter_process_dev -> Hqdn3dFilter::process_many): the spatial passes of the
    whole batch in one launch each, the temporal step frame after frame per sample.  Nine frames as calls of 5, 1
    and 3: the first batch seeds the temporal state from its own first frame, the single frame in between goes
    through the frame-at-a-time kernels on the state the batch left, the last batch continues from there - all
    against the oracle's frame-by-frame stream.  Case 2 has no spatial filter on any plane.
    The planes are contiguous, so only 1920 x 1080 (pitches that are multiples of 16 bytes) is handed to process_many as a
    whole; at the two smaller sizes process_dev pushes frame by frame (see hqdn3d_dev.run_dev) - the tests below pad."""
    if depth > 8 and (w, h) == (1920, 1080) and case != 1:
        pytest.skip("one 10-bit 1080p case is enough")
    n = 9
    frames = synth.stream("progressive", w, h, n, depth=depth)
    st, par = CASES[case]
    want = os_.hqdn3d_stream(frames, dict(par, depth=depth)) if depth > 8 else os_.hqdn3d_stream(frames, par)
    got = hd.run_dev(frames, par, depth, (5, 1, 3))
    for i in range(n):
        for c in range(3):
            np.testing.assert_array_equal(got[i][c], want[i][c], err_msg=f"{st} frame {i} plane {c}")


# ---- the verify / repair walks of every kernel form ------------------------------------------------------------------
# hq_h_rows and hq_v_cols each exist frame-at-a-time and batched, for bytes and for 16-bit containers.  A repair walk
# runs only where a segment guessed its start state wrong: forced with HBHIP_HQDN3D_WARMUP = 0 / 3 on nearly flat
# pictures (tests/test_hqdn3d_segments_cpu.py counts, on these very frames, how many guesses are wrong and how the
# repairs end), and met unforced at 10 / 12 bits, where flat content does not forget within the shipped warm-up.
# Tolerance 0 against the serial oracle everywhere.
HOOKS = [None, "0", "3", "1000"]
# `temporal` is case 2 of CASES: with y-spatial = 0 and cb-spatial = 0 the defaulting (cr-spatial = cb-spatial) leaves NO plane
# with a spatial filter; `mixed` is the case that does mix: only Cb has one
SETTINGS = {"default": CASES[0], "strong": STRONG, "temporal": CASES[2],
            "mixed": ("y-spatial=0:y-temporal=6:cb-spatial=3:cb-temporal=4:cr-spatial=0:cr-temporal=4",
                      dict(y_spatial=0, y_temporal=6, cb_spatial=3, cb_temporal=4, cr_spatial=0, cr_temporal=4))}


def _batched(frames, name, depth, calls, lcw=1, lch=1):
    """run_dev on rows padded to 16 bytes - contiguous rows of these widths would be pushed frame by frame and never
    reach the batched kernels - and the proof that they ran: the launches the context's profile counted"""
    launches = {}
    got = hd.run_dev(frames, SETTINGS[name][1], depth, calls, lcw, lch, pitch_align=16, launches=launches)
    assert {k: v for k, v in launches.items() if k.startswith("hqdn3d")} == hd.expected_launches(calls, SETTINGS[name][1]), name
    return got


def _hook(monkeypatch, warmup):
    if warmup is None:
        monkeypatch.delenv("HBHIP_HQDN3D_WARMUP", raising=False)
    else:
        monkeypatch.setenv("HBHIP_HQDN3D_WARMUP", warmup)


@functools.lru_cache(maxsize=None)
def _segment_case(w, h, depth, n, setting, sub="2x2"):
    """(frames, the oracle's frame-by-frame stream on them): computed once, shared by every hook value, left unchanged"""
    lcw, lch = {"2x2": (1, 1), "2x1": (1, 0), "1x1": (0, 0)}[sub]
    frames = hd.stretch_chroma(hd.segment_frames(w, h, depth, n), lcw, lch)
    return frames, os_.hqdn3d_stream(frames, dict(SETTINGS[setting][1], depth=depth))


@functools.lru_cache(maxsize=None)
def _rails_case(w, h, depth, setting):
    frames = hd.rails(w, h, depth)
    return frames, os_.hqdn3d_stream(frames, dict(SETTINGS[setting][1], depth=depth))


def _same(got, want, what):
    assert len(got) == len(want)
    for t in range(len(want)):
        for c in range(3):
            assert got[t][c].dtype == want[t][c].dtype
            np.testing.assert_array_equal(got[t][c], want[t][c], err_msg=f"{what} frame {t} plane {c}")


def _drop_in(frames, st, depth):
    got = hbrt.run_stream(hip.filters(), [("hb_filter_denoise_hip", st)], frames, pix_fmt=hbrt.PIX_FMT_FOR_DEPTH[depth])
    return [g.planes for g in got]


@pytest.mark.parametrize("warmup", HOOKS)
@pytest.mark.parametrize("w,h", [(200, 150), (202, 150)])
@pytest.mark.parametrize("depth", [8, 10, 12])
def test_segments_drop_in_path(built, monkeypatch, depth, w, h, warmup):
    """hq_h_rows / hq_v_cols<TEMPORAL = true> frame-at-a-time (host buffers take one_frame()), above all for 16-bit
    containers: NS = 8 samples per load, and at 202 x 150 chroma rows of 101 samples, which are no multiple of 16
    bytes, so the head, block and tail loops of hq_h_rows all run.  2 flat-noisy amp 1, 1 progressive, 1 flat-noisy
    amp 3, 1 rails frame; default and strong settings.  8 bits: the same frames at 200 x 150, so that every form x
    depth runs the content the CPU test counts the repairs of."""
    if depth == 8 and ((w, h) != (200, 150) or warmup == "1000"):
        pytest.skip("8-bit frame-at-a-time repairs: test_speculative_segments_are_exact; here hooks None / 0 / 3 at 200 x 150 only")
    if depth == 12 and (w, h) != (200, 150) and warmup in ("3", "1000"):
        pytest.skip("depth 12 runs the kernels of depth 10 with another shift: hooks None / 0 at the second shape")
    _hook(monkeypatch, warmup)
    for name in ("default", "strong"):
        frames, want = _segment_case(w, h, depth, 5, name)
        _same(_drop_in(frames, SETTINGS[name][0], depth), want, f"{name} warm-up {warmup}")


@pytest.mark.parametrize("warmup", HOOKS)
@pytest.mark.parametrize("w,h", [(200, 150), (202, 50), (18, 10)])
@pytest.mark.parametrize("depth", [8, 10, 12])
def test_segments_batched_path(built, monkeypatch, depth, w, h, warmup):
    """hq_h_rows with HB_SEG = 8 and hq_v_cols<TEMPORAL = false> with VB_SEG = 4 segments, then hqdn3d_tn_kernel: what a
    device-resident run uses.  Seven frames as calls of 3, 1, 2 and 1 on one filter: a batch, a single frame (the
    frame-at-a-time kernels), the smallest batch and a single frame, all on one temporal state.  202 x 50: every
    column segment's warm-up reaches row 0, chroma 101 x 25; 18 x 10: fewer live segments than lanes, chroma 9 x 5.
    `temporal` (case 2 of CASES) has no spatial filter, `mixed` has one on Cb only: the temporal state must survive
    both across calls.  Rows are padded to 16 bytes and the launches counted (_batched): contiguous rows of these
    widths never reach the batched kernels."""
    if depth == 12 and (w, h) != (200, 150) and warmup in ("3", "1000"):
        pytest.skip("depth 12 runs the kernels of depth 10 with another shift: hooks None / 0 at the small shapes")
    _hook(monkeypatch, warmup)
    for name in ("default", "strong", "temporal", "mixed"):
        frames, want = _segment_case(w, h, depth, 7, name)
        _same(_batched(frames, name, depth, hd.CALLS), want, f"{name} warm-up {warmup}")


def test_segments_batch_cut(built, monkeypatch):
    """17 frames in one call: a run of HQ_BATCH = 16 and the frame-at-a-time kernels behind it, every guess wrong"""
    _hook(monkeypatch, "0")
    frames, want = _segment_case(200, 150, 10, 17, "default")
    _same(_batched(frames, "default", 10, (17,)), want, "17 frames")


@pytest.mark.parametrize("sub", ["1x1", "2x1"])
def test_segments_batched_other_subsamplings(built, monkeypatch, sub):
    """4:4:4 and 4:2:2 through process_dev (tests/test_formats_gpu.py reaches them through host buffers only): the cut is
    taken from the luma plane and used on chroma planes of the full width / the full size"""
    _hook(monkeypatch, "0")
    lcw, lch = {"2x1": (1, 0), "1x1": (0, 0)}[sub]
    frames, want = _segment_case(200, 150, 10, 7, "strong", sub)
    assert frames[0][1].shape == (150 >> lch, 200 >> lcw)
    _same(_batched(frames, "strong", 10, hd.CALLS, lcw, lch), want, sub)


@pytest.mark.parametrize("path", ["drop-in", "batched"])
@pytest.mark.parametrize("depth", [8, 10, 12])
def test_rails_under_the_shipped_warmup(built, monkeypatch, depth, path):
    """all 0, all max, one-sample stripes 0 / max, top half 0 and bottom half max: jumps past the LUT's support and the
    states next to both ends of the 16-bit range, as shipped; top half max and bottom half 0 for the state that wraps
    at 12 bits; random samples within 8 codes of either end; the CLIMB frame, whose columns carry the vertical result
    past 65535 at 10 bits too (hqdn3d_dev.rails; tests/test_hqdn3d_segments_cpu.py counts the samples that get there).
    Batched: calls of 1 and 8 - every frame that wraps in the batch."""
    _hook(monkeypatch, None)
    for name in ("default", "strong"):
        frames, want = _rails_case(200, 150, depth, name)
        got = _drop_in(frames, SETTINGS[name][0], depth) if path == "drop-in" else _batched(frames, name, depth, (1, 8))
        _same(got, want, f"rails {name}")
