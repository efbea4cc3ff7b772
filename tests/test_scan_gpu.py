"""GPU: the title scan on device pictures (handbrake_amd/csrc/scan.hip through hbhip_scan_* and libhb/scan_hip.c), exact
against the model of tests/scan_model.py - whose reduced form tests/test_scan_cpu.py holds to the reference's loops as
written - on the contents of tests/scan_cases.py.  All arithmetic is integer: no tolerance anywhere."""
import ctypes as C
import functools

import numpy as np
import pytest

from handbrake_amd import hbrt, hip
import scan_cases as sc
import scan_model as sm

pytestmark = pytest.mark.gpu

ERR_ARG, ERR_UNSUPPORTED = -3, -5
shapes = pytest.mark.parametrize("shape", sc.SHAPES, ids=lambda s: "%dx%d" % s)


@pytest.fixture(scope="module")
def ctx(built):
    c = hip.Ctx(0)
    yield c
    c.close()


@functools.lru_cache(maxsize=None)
def picture(case, shape):
    return tuple(sc.CASES[case](*shape))


@functools.lru_cache(maxsize=None)
def want(case, shape, flags=0, params=sm.DEFAULT_PARAMS):
    """computed once per case and shared"""
    return sm.reduced_scan(picture(case, shape), flags, params)


def uploaded(ctx, planes):
    h, w = planes[0].shape
    fr = hip.Frame(ctx, w, h)
    fr.upload([np.ascontiguousarray(p) for p in planes])
    return fr


def helper_view(result):
    """a model tuple as hb_hip_scan_picture reports it: (combed, top, bottom, left, right, recorded)"""
    return (result[7],) + tuple(result[0:5])


@shapes
def test_device_frames_equal_the_model_on_every_content(ctx, shape):
    """every content of scan_cases at this size, all in flight at once, pulled in push order"""
    scan = hip.ScanDevice(ctx, *shape)
    frames = []
    try:
        names = sorted(sc.CASES)
        for name in names:
            frames.append(uploaded(ctx, picture(name, shape)))
            scan.push(frames[-1])
        assert scan.inflight() == len(names)
        for name in names:
            assert scan.pull().as_tuple() == want(name, shape), name
        assert scan.pull() is None and scan.inflight() == 0
    finally:
        scan.close()
        for fr in frames:
            fr.close()


@shapes
def test_flags_and_sensitivities(ctx, shape):
    """pic_flags with and without bit 16 under two pairs of triples, on the three combing contents"""
    scan = hip.ScanDevice(ctx, *shape)
    frames = {name: uploaded(ctx, picture(name, shape)) for name in sc.COMB_CASES}
    try:
        for name, fr in frames.items():
            for flags, params in sc.FLAG_PARAMS:
                scan.push(fr, flags, params)
                assert scan.pull().as_tuple() == want(name, shape, flags, params), (name, flags, params)
        # no parameters: scan.c's six numbers
        scan.push(frames["interlaced"], 0, None)
        assert scan.pull().as_tuple() == want("interlaced", shape)
    finally:
        scan.close()
        for fr in frames.values():
            fr.close()


def preview_1080p():
    """a combed 1080p picture behind a matte with line-21 rows and unequal pillars"""
    w, h = sc.BIG
    p = list(sc.interlaced(w, h))
    matte = sc.pillarbox(w, h, matte=True)[0]
    inside = np.zeros((h, w), bool)
    inside[h // 8:h - h // 6, w // 10:w - w // 7] = True
    p[0] = np.where(inside, p[0], matte)
    p[0][3, ::2] = 235                                               # inside the border region (border = 10)
    return p


def test_a_1080p_preview_and_what_it_sends_over_the_bus(ctx):
    w, h = sc.BIG
    planes = preview_1080p()
    expect = sm.reduced_scan(planes)
    assert expect[:5] == (h // 8, h // 6, w // 10, w // 7, 1) and expect[7] == 1
    scan = hip.ScanDevice(ctx, w, h)
    fr = uploaded(ctx, planes)
    try:
        before = ctx.bus_bytes()
        scan.push(fr)
        got = scan.pull().as_tuple()
        after = ctx.bus_bytes()
        assert got == expect
        assert after[0] == before[0] and after[1] - before[1] == hip.SCAN_RECORD_BYTES   # the record and nothing else
        assert fr.refs() == 1                                         # the object's reference went with the pull
    finally:
        scan.close()
        fr.close()


def test_eight_pictures_in_flight_come_back_in_order(ctx):
    shape = (100, 240)
    names = ["all_black", "pillarbox_matte", "interlaced", "no_border", "below_16", "progressive", "letterbox_line21",
             "chroma_only_combed"]
    scan = hip.ScanDevice(ctx, *shape)
    frames = [uploaded(ctx, picture(n, shape)) for n in names]
    try:
        for round_ in range(2):                                      # the second round reuses the first one's slots
            for i, fr in enumerate(frames):
                scan.push(fr, flags=16 if i & 1 else 0)
                assert scan.inflight() == i + 1 and fr.refs() == 2
            for i, n in enumerate(names):
                assert scan.pull().as_tuple() == want(n, shape, 16 if i & 1 else 0), (round_, n)
                assert scan.inflight() == len(names) - 1 - i
        assert scan.pull() is None
    finally:
        scan.close()
        for fr in frames:
            fr.close()


@shapes
def test_an_nv12_surface_imported_first(ctx, shape):
    name = "pillarbox_matte"
    src = uploaded(ctx, picture(name, shape))
    surface = hip.Surface(ctx, *shape)
    fr = hip.Frame(ctx, *shape)
    scan = hip.ScanDevice(ctx, *shape)
    try:
        src.export_surface(surface)
        fr.import_surface(surface)
        scan.push(fr)
        assert scan.pull().as_tuple() == want(name, shape)
    finally:
        scan.close()
        for o in (fr, surface, src):
            o.close()


# ---------------------------------------------------------------- the libhb side
@shapes
def test_host_buffers_through_the_libhb_helper(built, shape):
    F = hip.filters()
    for name in ("letterbox_line21", "border_row_bright", "sixteen_seventeen", "interlaced", "chroma_only_combed"):
        rc, got = hbrt.scan_run(F, picture(name, shape))
        assert rc == 0 and got == helper_view(want(name, shape)), name
    rc, got = hbrt.scan_run(F, picture("interlaced", shape), flags=16)
    assert rc == 0 and got == helper_view(want("interlaced", shape, 16))


def test_device_buffers_through_the_libhb_helper(ctx):
    """a buffer whose picture is a device frame, and one whose picture is a decoder's NV12 surface"""
    F = hip.filters()
    shape, name = (322, 200), "pillarbox_matte"
    rc, got = hbrt.scan_run(F, picture(name, shape), frame=uploaded(ctx, picture(name, shape)))
    assert rc == 0 and got == helper_view(want(name, shape))
    src, surface = uploaded(ctx, picture(name, shape)), hip.Surface(ctx, *shape)
    try:
        src.export_surface(surface)
    finally:
        src.close()
    rc, got = hbrt.scan_run(F, picture(name, shape), surface=surface)
    assert rc == 0 and got == helper_view(want(name, shape))


def test_the_libhb_helper_declines_what_the_abi_refuses(ctx):
    F = hip.filters()
    planes = picture("no_border", (64, 48))
    assert hbrt.scan_run(F, planes, open_size=(6, 48))[0] == 1                       # open: below 8
    assert hbrt.scan_run(F, planes, open_size=(65, 48))[0] == 1                      # open: odd
    assert hbrt.scan_run(F, planes, open_size=(100, 240))[0] == 2                    # picture: another size
    assert hbrt.scan_run(F, planes, pix_fmt=hbrt.AV_PIX_FMT_YUV420P10)[0] == 2       # picture: not 8-bit
    deep = hip.Frame(ctx, 64, 48, 10)
    assert hbrt.scan_run(F, planes, frame=deep, pix_fmt=hbrt.AV_PIX_FMT_YUV420P10)[0] == 2


# ---------------------------------------------------------------- refusals
def test_every_refusal_queues_nothing(ctx):
    L = hip.lib()
    h = C.c_void_p()
    for w, hh in ((6, 48), (64, 6), (65, 48), (64, 47)):
        assert L.hbhip_scan_create(ctx.h, w, hh, C.byref(h)) == ERR_UNSUPPORTED and not h.value
    scan = hip.ScanDevice(ctx, 64, 48)
    bad = {"10 bit": hip.Frame(ctx, 64, 48, 10), "4:2:2": hip.Frame(ctx, 64, 48, 8, 1, 0), "4:4:4": hip.Frame(ctx, 64, 48, 8, 0, 0),
           "odd width": hip.Frame(ctx, 65, 48), "odd height": hip.Frame(ctx, 64, 47), "another size": hip.Frame(ctx, 100, 240),
           "below 8": hip.Frame(ctx, 6, 48)}
    good = uploaded(ctx, picture("no_border", (64, 48)))
    try:
        ctx.sync()
        before = ctx.bus_bytes()
        for what, fr in bad.items():
            assert scan.push_rc(fr) == ERR_UNSUPPORTED, what
            assert fr.refs() == 1, what
        assert L.hbhip_scan_push(scan.h, None, 0, None) == ERR_ARG
        if L.hbhip_device_count() > 1:                               # a frame of another GPU
            other = hip.Ctx(1)
            far = hip.Frame(other, 64, 48)
            try:
                assert scan.push_rc(far) == ERR_ARG
            finally:
                far.close()
                other.close()
        assert scan.inflight() == 0 and scan.pull() is None
        assert ctx.bus_bytes() == before                             # no traffic for a refused call
        scan.push(good)                                              # and the object takes the next picture as ever
        assert scan.pull().as_tuple() == want("no_border", (64, 48))
        # more in flight than the object holds
        for _ in range(hip.SCAN_INFLIGHT_MAX):
            scan.push(good)
        assert scan.push_rc(good) == -6                              # HBHIP_ERR_STATE
        for _ in range(hip.SCAN_INFLIGHT_MAX):
            assert scan.pull().as_tuple() == want("no_border", (64, 48))
        assert good.refs() == 1
    finally:
        scan.close()
        good.close()
        for fr in bad.values():
            fr.close()
