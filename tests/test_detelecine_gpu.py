"""GPU: the HIP detelecine drop-in (hb_filter_detelecine_hip over csrc/detelecine.hip) against the reference's own
recorded output (tests/golden/detelecine_*.npz) and against the independent model (tests/pullup_model.py)."""
import ctypes as C

import numpy as np
import pytest

import detelecine_cases as dc
import oracle_lib as ol
import pullup_model as pm
from handbrake_amd import hbrt, hip

pytestmark = pytest.mark.gpu
F = hbrt.FILTER_ID
NLM = hip.NLMEANS_MEDIUM + ":threads=2"
LAP = "y-strength=0.2:y-kernel=isolap:cb-strength=0.2:cb-kernel=isolap"
COMB = ("mode=3:spatial-metric=2:motion-thresh=1:spatial-thresh=1:filter-mode=2:"
        "block-thresh=40:block-width=16:block-height=16")
UP, DOWN, NAME = "HIP upload adapter", "HIP download adapter", "Detelecine (pullup) (HIP)"
REF = {F["comb_detect"]: "hb_filter_comb_detect", F["decomb"]: "hb_filter_decomb", F["nlmeans"]: "hb_filter_nlmeans",
       F["lapsharp"]: "hb_filter_lapsharp"}
LCW = {"2x2": (1, 1), "2x1": (1, 0), "1x1": (0, 0)}


class Params(C.Structure):
    _fields_ = [("skip_left", C.c_int), ("skip_right", C.c_int), ("skip_top", C.c_int), ("skip_bottom", C.c_int),
                ("strict_breaks", C.c_int), ("plane", C.c_int), ("parity", C.c_int)]


def params(settings=""):
    s = pm.parse_settings(settings)
    return Params(s.get("skip-left", 1), s.get("skip-right", 1), s.get("skip-top", 4), s.get("skip-bottom", 4),
                  s.get("strict-breaks", -1), s.get("plane", 0), s.get("parity", -1))


def create(ctx, w, h, depth=8, chroma="2x2", settings=""):
    L = hip.lib()
    L.hbhip_detelecine_create.argtypes = [C.c_void_p, C.POINTER(Params)] + [C.c_int] * 5 + [C.POINTER(C.c_void_p)]
    h_ = C.c_void_p()
    rc = L.hbhip_detelecine_create(ctx.h, C.byref(params(settings)), w, h, depth, *LCW[chroma], C.byref(h_))
    return rc, h_


def same_frames(got, want, what):
    assert len(got) == len(want), f"{what}: {len(got)} frames, want {len(want)}"
    for t, (g, (wp, wm)) in enumerate(zip(got, want)):
        assert (g.start, g.stop) == tuple(wm[:2]), f"{what} frame {t}: times {(g.start, g.stop)} != {wm[:2]}"
        for c in range(3):
            assert np.array_equal(g.planes[c], wp[c]), f"{what} frame {t} plane {c} differs"


@pytest.fixture()
def registered(built):
    if ol.ref() is None:
        pytest.skip("oracle/_ref not built (no /root/reference)")
    hbrt.register_filters(hip.filters(), {F["detelecine"]: "hb_filter_detelecine_hip"})
    hbrt.register_filters(ol.ref(), REF)
    yield
    hbrt.register_filters(ol.ref(), {k: None for k in REF})
    hbrt.register_filters(hip.filters(), {F["detelecine"]: None})


@pytest.mark.parametrize("name", sorted(dc.CASES))
def test_fixture_through_the_drop_in_host_buffers(built, name):
    frames, flags, depth, chroma, settings = dc.build(name)
    got = dc.run_chain(hip.filters(), "hb_filter_detelecine_hip", settings, frames, flags, depth, chroma)
    want = dc.load_golden(name)
    same_frames(got, want, name)
    for t, (g, (_, wm)) in enumerate(zip(got, want)):
        assert g.flags == wm[2], f"{name} frame {t}: flags {g.flags} != {wm[2]}"


def reference_after(outputs, stages, depth, chroma):
    """the model's detelecine outputs, with their props, through a reference chain"""
    h, w = outputs[0][0][0].shape
    out = []
    with hbrt.Chain(ol.ref(), stages, w, h, dc.pix_fmt(depth, chroma)) as ch:
        for planes, (start, stop, flags) in outputs:
            ch.push(planes, start=start, stop=stop, flags=flags)
            out += ch.drain()
        ch.push_eof()
        out += ch.drain()
    return [(o.planes, (o.start, o.stop, o.flags)) for o in out]


def run_job(filters, frames, flags, depth, chroma):
    h, w = frames[0][0].shape
    out = []
    with hbrt.Job(filters, w, h, dc.pix_fmt(depth, chroma), use_hip=True) as job:
        names = job.stages()
        for i, (fr, fl) in enumerate(zip(frames, flags)):
            job.push(fr, start=i * dc.DURATION, stop=(i + 1) * dc.DURATION, flags=fl)
            out += job.drain()
        job.push_eof()
        out += job.drain()
    return names, out


@pytest.mark.parametrize("name", ["hard_tff", "soft_rff", "broken_cadence", "hard_10bit", "parity1"])
def test_device_resident_run_with_decomb_and_nlmeans(registered, name):
    frames, flags, depth, chroma, settings = dc.build(name)
    names, got = run_job([(F["detelecine"], settings), (F["decomb"], "mode=7"), (F["nlmeans"], NLM)],
                         frames, flags, depth, chroma)
    assert names[0] == UP and names[1] == NAME and names[-1] == DOWN, names
    want = reference_after(dc.expected(name), [("hb_filter_decomb", "mode=7"), ("hb_filter_nlmeans", NLM)], depth, chroma)
    same_frames(got, want, name)


@pytest.mark.parametrize("threaded", [False, True])
def test_job_detelecine_comb_detect_decomb_nlmeans_lapsharp(registered, threaded):
    name = "broken_cadence"
    frames, flags, depth, chroma, settings = dc.build(name)
    hbrt.set_threaded(threaded)
    try:
        names, got = run_job([(F["detelecine"], settings), (F["comb_detect"], COMB), (F["decomb"], "mode=7"),
                              (F["nlmeans"], NLM), (F["lapsharp"], LAP)], frames, flags, depth, chroma)
    finally:
        hbrt.set_threaded(False)
    assert names[0] == UP and names[1] == NAME and names[-1] == DOWN and len(names) == 7, names
    assert all("HIP" in n for n in names), names
    want = reference_after(dc.expected(name), [("hb_filter_comb_detect", COMB), ("hb_filter_decomb", "mode=7"),
                                               ("hb_filter_nlmeans", NLM), ("hb_filter_lapsharp", LAP)], depth, chroma)
    same_frames(got, want, f"{name} threaded={threaded}")


def run_frames(frames, flags, depth, chroma, settings=""):
    """Through the C ABI with device frames (hbhip_filter_use_frames): every output frame is held, not read, until
    the stream has ended - a later write into a frame already handed on would show in the comparison."""
    L = hip.lib()
    L.hbhip_detelecine_push_frame.argtypes = [C.c_void_p, C.c_void_p, C.c_int64, C.c_int]
    L.hbhip_filter_pull_frame.argtypes = [C.c_void_p, C.POINTER(C.c_void_p), C.POINTER(C.c_int64)]
    ctx = hip.Ctx()
    h, w = frames[0][0].shape
    rc, flt = create(ctx, w, h, depth, chroma, settings)
    hip.check(rc, ctx.h, "detelecine_create")
    held = []
    try:
        hip.check(L.hbhip_filter_use_frames(flt), ctx.h, "use_frames")
        for i, (planes, fl) in enumerate(zip(frames, flags)):
            fr = hip.Frame(ctx, w, h, depth, *LCW[chroma])
            fr.upload([np.ascontiguousarray(p) for p in planes])
            hip.check(L.hbhip_detelecine_push_frame(flt, fr.h, i, fl), ctx.h, "push_frame")
            fr.close()                                   # the filter's reference is the only one now
            while L.hbhip_filter_pending(flt) > 0:
                o, tag = C.c_void_p(), C.c_int64()
                hip.check(L.hbhip_filter_pull_frame(flt, C.byref(o), C.byref(tag)), ctx.h, "pull_frame")
                out = hip.Frame.__new__(hip.Frame)
                out.ctx, out.h, out.shape = ctx, o, (w, h, depth, *LCW[chroma])
                held.append((tag.value, out))
        hip.check(L.hbhip_filter_flush(flt), ctx.h, "flush")
        ctx.sync()
        return [(tag, fr.download()) for tag, fr in held]
    finally:
        for _, fr in held:
            fr.close()
        L.hbhip_filter_destroy(flt)
        ctx.close()


def compare_model(frames, flags, depth, chroma, settings, what):
    got = run_frames(frames, flags, depth, chroma, settings)
    want = pm.run(frames, flags, depth, settings)
    assert len(got) == len(want), f"{what}: {len(got)} frames, the model makes {len(want)}"
    for t, ((gt, gp), (wt, wp)) in enumerate(zip(got, want)):
        assert gt == wt, f"{what} frame {t}: made at input {gt}, the model at {wt}"
        for c in range(3):
            assert np.array_equal(gp[c], wp[c]), f"{what} frame {t} plane {c} differs"
    return len(got)


@pytest.mark.parametrize("seed,depth,chroma,w,h,settings", [
    (0, 8, "2x2", 128, 64, ""),
    (1, 10, "2x1", 136, 72, "strict-breaks=1"),
    (2, 12, "1x1", 96, 48, "plane=1"),
    (3, 8, "2x2", 200, 96, "strict-breaks=0"),
    (4, 10, "2x2", 160, 80, "skip-left=2:skip-top=5"),
    (5, 8, "1x1", 120, 64, "parity=0"),
])
def test_seeded_long_streams_against_the_model(built, seed, depth, chroma, w, h, settings):
    frames, flags = dc.seeded_stream(seed, 230, w, h, depth, chroma)
    assert len(frames) >= 190 and sum(1 for f in flags if f & dc.PIC_FLAG_REPEAT_FIRST_FIELD) > 10
    n = compare_model(frames, flags, depth, chroma, settings, f"seed {seed}")
    assert n > len(frames) * 2 // 3


def test_1080p_stream_against_the_model(built):
    """31 654 metric blocks a field: the reductions span many workgroups"""
    frames, flags = dc.seeded_stream(7, 48, 1920, 1080)
    compare_model(frames, flags, 8, "2x2", "", "1080p")


@pytest.mark.parametrize("w,h,chroma", [(128, 65, "2x2"), (128, 66, "2x2"), (128, 65, "1x1")])
def test_odd_plane_height_is_declined(built, w, h, chroma):
    ctx = hip.Ctx()
    try:
        rc, flt = create(ctx, w, h, 8, chroma)
        assert rc == -5 and not flt.value                      # HBHIP_ERR_UNSUPPORTED
    finally:
        ctx.close()
    with pytest.raises(RuntimeError):
        hbrt.Chain(hip.filters(), [("hb_filter_detelecine_hip", "")], w, h, dc.pix_fmt(8, chroma))


def test_margins_wider_than_the_plane_are_declined(built):
    with pytest.raises(RuntimeError):
        hbrt.Chain(hip.filters(), [("hb_filter_detelecine_hip", "skip-left=10:skip-right=7")], 128, 64)
