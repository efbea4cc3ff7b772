"""What a filter took, it gave back: every hipMalloc / hipHostMalloc of the library is held by one of the two owner types of
csrc/hbhip_internal.h, which keep two process-wide byte counts (hbhip_mem_live: device, pinned).  The counts are read around
every factory handbrake_amd/hip.py has - three rounds of create, use, destroy on one context - around the blend object's
growing stores, and around the creates the "declines" tests of the other files show to be refused.

Frames are 128 x 96, 4:2:0: who owns a buffer does not depend on its size.  Their content is zeros for the same reason.
torch's own allocations are not the library's and are not counted."""
import ctypes as C

import numpy as np
import pytest

from handbrake_amd import hip

pytestmark = pytest.mark.gpu

W, H = 128, 96
UNSUPPORTED = -5


def planes(w=W, h=H, depth=8, lcw=1, lch=1):
    """three zeroed device planes, rows 256 bytes apart or a multiple (what the zero-copy paths want)"""
    import torch
    dt, es = (torch.uint8, 1) if depth == 8 else (torch.int16, 2)

    def plane(pw, ph):
        return torch.zeros((ph, -(-pw * es // 256) * 256 // es), dtype=dt, device="cuda")[:, :pw]
    cw, ch = -(-w >> lcw), -(-h >> lch)
    return [plane(w, h), plane(cw, ch), plane(cw, ch)]


def through(flt, n, gin=(), gout=None):
    """n frames of geometry gin = (w, h, depth, lcw, lch) through a DeviceFilter in one process_dev call, then its flush"""
    ins = [planes(*gin) for _ in range(n)]
    outs = [planes(*(gin if gout is None else gout)) for _ in range(n)]
    arr_in = (hip.DevFrame * n)(*[hip.dev_frame(p) for p in ins])
    arr_out = (hip.DevFrame * n)(*[hip.dev_frame(p) for p in outs])
    flt.process_dev(arr_in, 0, arr_out)
    flt.flush()
    flt.ctx.sync()


def simple(make, n=2, gin=(), gout=None):
    def use(ctx):
        flt = make(ctx)
        try:
            through(flt, n, gin, gout)
        finally:
            flt.close()
    return use


def hqdn3d(depth):
    class HQ(C.Structure):
        _fields_ = [("coef", (C.c_int16 * 8192) * 6)]

    def make(ctx):
        hq = HQ()
        for k in range(6):
            hq.coef[k][0] = 1 if k % 2 == 0 else 0                  # spatial strength != 0: the planes take the spatial kernels
        return hip._create("hbhip_hqdn3d_create", ctx, [C.c_void_p, C.POINTER(HQ)] + [C.c_int] * 5 + [C.POINTER(C.c_void_p)],
                           ctx.h, C.byref(hq), W, H, depth, 1, 1)
    # one frame: the frame-at-a-time arrays; then two in one call: the batched kernels' arrays, made at the first such call
    def use(ctx):
        flt = make(ctx)
        try:
            through(flt, 1, (W, H, depth))
            through(flt, 2, (W, H, depth))
        finally:
            flt.close()
    return use


def nlmeans(ctx):
    # batches of four frames: the job tables are made, and grown, by the first launches
    flt = hip.nlmeans_device_filter(ctx, hip.NLMEANS_MEDIUM, W, H, batch=4)
    try:
        through(flt, 6, (W, H, 8))
    finally:
        flt.close()


def comb_detect(mode=3, filter_mode=2):
    def use(ctx):
        dev = hip.CombDetectDevice(ctx, W, H, mode=mode, filter_mode=filter_mode)
        try:
            lumas = [planes()[0] for _ in range(5)]
            for luma in lumas[:3]:
                dev.store_dev(luma.data_ptr(), luma.stride(0))
            dev.classify()
            if mode == 3 and filter_mode == 2:
                dev.classify_many([l.data_ptr() for l in lumas], lumas[0].stride(0))
        finally:
            dev.close()
    return use


def comb_detect_10bit(ctx):
    """the (1 << depth)-entry gamma table and the 16-bit ring: the generic kernel's path"""
    L = hip.lib()
    hip.CombDetectDevice(ctx, W, H).close()                           # (declares the entry points' arguments)
    L.hbhip_comb_detect_set_gamma_lut.argtypes = [C.c_void_p, C.POINTER(C.c_float), C.c_int]
    par = hip.CombDetectParams(3, 2, 1, 1, 2, 40, 16, 16)
    h = C.c_void_p()
    hip.check(L.hbhip_comb_detect_create(ctx.h, C.byref(par), W, H, 10, C.byref(h)), ctx.h, "comb_detect_create")
    try:
        lut = (C.c_float * 1024)(*[(i / 1023.0) ** 2.2 for i in range(1024)])
        hip.check(L.hbhip_comb_detect_set_gamma_lut(h, lut, 1024), ctx.h, "set_gamma_lut")
        for _ in range(3):
            luma = planes(depth=10)[0]
            hip.check(L.hbhip_comb_detect_store_dev(h, C.c_void_p(luma.data_ptr()), luma.stride(0) * 2), ctx.h, "store_dev")
        out = C.c_int()
        hip.check(L.hbhip_comb_detect_classify(h, 0, C.byref(out)), ctx.h, "classify")
    finally:
        L.hbhip_filter_destroy(h)


def decomb(depth, search, postproc=3):
    def use(ctx):
        dev = hip.DecombDevice(ctx, W, H, mode=24, search=search, postproc=postproc, depth=depth)
        try:
            dt = np.uint8 if depth == 8 else np.uint16
            frame = [np.zeros((H, W), dt), np.zeros((H // 2, W // 2), dt), np.zeros((H // 2, W // 2), dt)]
            for _ in range(3):
                dev.push(frame)
                while dev.pull() is not None:
                    pass
            dev.flush()
            while dev.pull() is not None:
                pass
        finally:
            dev.close()
    return use


def small_set():
    ov = tuple(np.full((8, 16), 128, np.uint8) for _ in range(4))
    return [(8, 8, ov)]


def large_set():
    ov = tuple(np.full((40, 96), 128, np.uint8) for _ in range(4))
    return [(8, 8, ov), (16, 48, ov)]


def ass_set(n, w, h):
    return [(np.full((h, w), 200, np.uint8), w, 8 + 4 * i, 8 + 20 * i, (180, 128, 128, 0)) for i in range(n)]


def bitmap_set(n):
    sub = tuple(np.full((16, 32), 128, np.uint8) for _ in range(4))
    # one at the frame's own size, the others from a window twice as large: those are scaled on the device
    return [(4, 4 + 20 * i, sub, (W, H) if i == 0 else (2 * W, 2 * H), 100 + i) for i in range(n)]


def blend(ctx):
    frame = hip.dev_frame(planes())
    b444 = hip.BlendDevice(ctx, W, H)                                   # YUVA444P overlays: plain lists and bitmap subtitles
    b420 = hip.BlendDevice(ctx, W, H, overlay_log2_cw=1, overlay_log2_ch=1)   # the frame's subsampling: text subtitles
    try:
        b444.set_overlays(large_set())
        b444.apply_dev(frame)
        b444.set_bitmaps(bitmap_set(3))
        b444.apply_dev(frame)
        b444.set_bitmaps(bitmap_set(1))                                 # two keys go
        b444.apply_dev(frame)
        b420.set_ass_images(ass_set(3, 24, 12))
        b420.apply_dev(frame)
        ctx.sync()
    finally:
        b444.close()
        b420.close()


def scan(ctx):
    dev = hip.ScanDevice(ctx, W, H)
    frames = [hip.Frame(ctx, W, H) for _ in range(2)]
    try:
        for fr in frames:
            fr.upload(fr.planes())
            dev.push(fr)
        while dev.pull() is not None:
            pass
    finally:
        dev.close()
        for fr in frames:
            fr.close()


def frames_and_surfaces(ctx):
    fr, s8, s10 = hip.Frame(ctx, W, H), hip.Surface(ctx, W, H), hip.Surface(ctx, W, H, 10)
    try:
        fr.upload(fr.planes())
        fr.export_surface(s8)
        fr.export_surface_widen(s10)
        fr.import_surface(s8)
        fr.download()
        ctx.sync()
    finally:
        for x in (fr, s8, s10):
            x.close()


def chain(own_contexts):
    """hip.Chain over crop/scale and lapsharp: stages on the chain's context, or each on a context of its own"""
    def use(ctx):
        ctxs = [hip.Ctx(0), hip.Ctx(0)] if own_contexts else [ctx, ctx]
        ch = hip.Chain(ctx, [hip.cropscale_device_filter(ctxs[0], W, H, 64, 48), hip.lapsharp_device_filter(ctxs[1], 64, 48)])
        try:
            n = 3
            ins, outs = [planes() for _ in range(n)], [planes(64, 48) for _ in range(n)]
            arr_in = (hip.DevFrame * n)(*[hip.dev_frame(p) for p in ins])
            arr_out = (hip.DevFrame * n)(*[hip.dev_frame(p) for p in outs])
            ch.process_dev(arr_in, arr_out)
            ch.flush_dev(arr_out)
            ch.sync()
        finally:
            ch.close()                                                   # (closes its stages)
            if own_contexts:
                for c in ctxs:
                    c.close()
    return use


BT709, BT601 = (1, 1, 1, 1), (6, 6, 6, 1)
FACTORIES = {
    "chain": chain(False),
    "chain, a context a stage": chain(True),
    "frame, surface": frames_and_surfaces,
    "scan": scan,
    "nlmeans": nlmeans,
    "hqdn3d 8": hqdn3d(8),
    "hqdn3d 10": hqdn3d(10),
    "comb detect": comb_detect(),
    "comb detect, mask mode": comb_detect(mode=7),
    "comb detect, filter mode 0": comb_detect(filter_mode=0),
    "comb detect, filter mode 1": comb_detect(filter_mode=1),
    "comb detect 10": comb_detect_10bit,
    "decomb eedi2 8": decomb(8, 24),
    "decomb eedi2 8, search 32": decomb(8, 32),
    "decomb eedi2 10": decomb(10, 24),
    "lapsharp": simple(lambda ctx: hip.lapsharp_device_filter(ctx, W, H), gin=(W, H, 8)),
    "cropscale": simple(lambda ctx: hip.cropscale_device_filter(ctx, W, H, 192, 144), gin=(W, H, 8), gout=(192, 144, 8)),
    "cropscale down": simple(lambda ctx: hip.cropscale_device_filter(ctx, W, H, 64, 48), 3, gin=(W, H, 8), gout=(64, 48, 8)),
    "cropscale sws": simple(lambda ctx: hip.cropscale_device_filter(ctx, W, H, 65, 49, sws=True), gin=(W, H, 8), gout=(65, 49, 8)),
    "cropscale sited": simple(lambda ctx: hip.cropscale_device_filter(ctx, W, H, 64, 48, chroma_location=2),
                              gin=(W, H, 8), gout=(64, 48, 8)),
    "colorspace": simple(lambda ctx: hip.colorspace_device_filter(ctx, W, H, BT709, BT601, tonemap="none"), gin=(W, H, 8)),
    "format resample": simple(lambda ctx: hip.format_resample_device_filter(ctx, W, H), gin=(W, H, 8, 1, 0), gout=(W, H, 8, 1, 1)),
    "format scaled": simple(lambda ctx: hip.format_scaled_device_filter(ctx, W, H), gin=(W, H, 10, 1, 0), gout=(W, H, 8, 1, 1)),
    "format deepen": simple(lambda ctx: hip.format_deepen_device_filter(ctx, W, H), gin=(W, H, 8, 1, 0), gout=(W, H, 10, 1, 1)),
    "format upsample": simple(lambda ctx: hip.format_upsample_device_filter(ctx, W, H), gin=(W, H, 8, 1, 1), gout=(W, H, 8, 1, 0)),
    "blend": blend,
}


@pytest.mark.parametrize("name", sorted(FACTORIES))
def test_three_rounds_take_what_the_first_took_and_the_context_gives_it_all_back(built, name):
    use = FACTORIES[name]
    before = hip.mem_live()
    ctx = hip.Ctx(0)
    try:
        after = []
        for _ in range(3):
            use(ctx)
            ctx.sync()
            after.append(hip.mem_live())
    finally:
        ctx.close()
    print(name, "before", before, "rounds", after, "closed", hip.mem_live())
    assert after[1] == after[0] and after[2] == after[0], f"{name}: a round left memory behind: {after}"
    assert hip.mem_live() == before, f"{name}: the closed context still holds memory"


def test_blend_stores_grow_once(built):
    """small, large, small: the device count rises at the large set and the small one behind it takes nothing and frees
    nothing, for plain overlay lists and for text subtitles"""
    ctx = hip.Ctx(0)
    b444 = hip.BlendDevice(ctx, W, H)
    b420 = hip.BlendDevice(ctx, W, H, overlay_log2_cw=1, overlay_log2_ch=1)
    try:
        for what, put, small, large in (("set_overlays", b444.set_overlays, small_set(), large_set()),
                                        ("set_ass_images", b420.set_ass_images, ass_set(1, 8, 8), ass_set(4, 64, 24))):
            counts = []
            for s in (small, large, small):
                put(s)
                ctx.sync()
                counts.append(hip.mem_live()[0])
            print(what, counts)
            assert counts[1] > counts[0], f"{what}: the large set fitted the small set's store: {counts}"
            assert counts[2] == counts[1], f"{what}: the small set behind the large one changed the store: {counts}"
    finally:
        b444.close()
        b420.close()
        ctx.close()


def test_a_wrapped_surface_is_the_callers(built):
    """hip.Surface.wrap: memory of the caller's.  The library neither counts it nor frees it - the counts do not move when
    it is wrapped, used or released, and the memory is still the caller's to read afterwards"""
    import torch
    ctx = hip.Ctx(0)
    fr = hip.Frame(ctx, W, H)
    try:
        ctx.sync()
        before = hip.mem_live()
        mem = torch.full((H + H // 2, 256), 77, dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()
        s = hip.Surface.wrap(ctx, (mem.data_ptr(), mem.data_ptr() + H * 256), (256, 256), W, H)
        assert hip.mem_live() == before
        fr.import_surface(s)
        ctx.sync()
        s.close()
        assert hip.mem_live() == before
        assert int(mem[H + H // 2 - 1, 255]) == 77 and int(mem[0, 0]) == 77
        assert all(int(p.min()) == 77 == int(p.max()) for p in fr.download()[:1])
    finally:
        fr.close()
        ctx.close()


def _raw(fn, argtypes, *args):
    """the code of a create through the raw ABI, and whether it left a handle"""
    f = getattr(hip.lib(), fn)
    f.argtypes = argtypes
    h = C.c_void_p()
    return f(*args, C.byref(h)), h.value


def _params(fn):
    """the argument tuples of a test's (single) parametrize mark"""
    (mark,) = [m for m in fn.pytestmark if m.name == "parametrize"]
    values = [getattr(v, "values", v) for v in mark.args[1]]
    return [tuple(v) if isinstance(v, (tuple, list)) else (v,) for v in values]


# The case lists of the create-declines tests that keep theirs inside the test function, as they stand there:
# (src, dst, source depth, target depth, w, h)
DEEPEN_DECLINED = [                                                          # test_format_deepen_gpu.test_create_declines
    ((1, 0), (1, 1), 8, 8, 128, 72), ((0, 0), (1, 1), 10, 10, 128, 72), ((0, 0), (1, 0), 12, 12, 128, 72),
    ((1, 0), (1, 1), 10, 8, 128, 72), ((0, 0), (1, 0), 12, 10, 128, 72), ((0, 0), (1, 1), 12, 8, 128, 72),
    ((1, 1), (1, 1), 8, 10, 128, 72), ((1, 0), (1, 0), 8, 12, 128, 72), ((0, 0), (0, 0), 10, 12, 128, 72),
    ((1, 1), (1, 0), 8, 10, 128, 72), ((1, 0), (0, 0), 8, 10, 128, 72), ((1, 1), (0, 0), 10, 12, 128, 72),
    ((1, 1), (0, 1), 8, 10, 128, 72), ((0, 1), (1, 0), 8, 10, 128, 72),
    ((1, 0), (1, 1), 9, 10, 128, 72), ((1, 0), (1, 1), 8, 16, 128, 72), ((1, 0), (1, 1), 6, 8, 128, 72),
    ((1, 0), (1, 1), 10, 14, 128, 72), ((1, 0), (1, 1), 8, 9, 128, 72),
    ((1, 0), (1, 1), 8, 10, 128, 10), ((0, 0), (1, 0), 8, 10, 10, 72), ((0, 0), (1, 1), 10, 12, 128, 10),
    ((0, 0), (1, 1), 8, 12, 10, 72)]
SCALED_DECLINED = [                                                          # test_format_scaled_gpu.test_create_declines
    ((1, 0), (1, 1), 8, 10, 128, 72), ((0, 0), (1, 0), 10, 12, 128, 72), ((1, 1), (1, 1), 8, 10, 128, 72),
    ((1, 0), (1, 1), 9, 8, 128, 72), ((1, 0), (1, 1), 16, 8, 128, 72), ((1, 0), (1, 1), 10, 6, 128, 72),
    ((1, 1), (1, 0), 10, 8, 128, 72), ((1, 0), (0, 0), 12, 8, 128, 72), ((0, 0), (0, 1), 10, 8, 128, 72),
    ((1, 1), (1, 1), 10, 10, 128, 72),
    ((1, 0), (1, 1), 10, 8, 128, 10), ((0, 0), (1, 0), 12, 10, 10, 72), ((0, 0), (1, 1), 12, 8, 128, 10)]
UPSAMPLE_DECLINED = [                                                        # test_format_upsample_gpu.test_create_declines
    ((1, 1), (1, 0), 9, 10, 128, 72), ((1, 1), (1, 0), 8, 16, 128, 72), ((1, 1), (1, 0), 6, 8, 128, 72),
    ((1, 1), (1, 0), 10, 8, 128, 72), ((1, 0), (0, 0), 12, 10, 128, 72), ((1, 1), (0, 0), 12, 8, 128, 72),
    ((1, 0), (1, 1), 8, 8, 128, 72), ((0, 0), (1, 0), 8, 10, 128, 72), ((0, 0), (1, 1), 10, 10, 128, 72),
    ((1, 1), (0, 1), 8, 8, 128, 72),
    ((1, 1), (1, 1), 8, 8, 128, 72), ((1, 0), (1, 0), 8, 10, 128, 72), ((0, 0), (0, 0), 10, 12, 128, 72),
    ((1, 1), (0, 0), 8, 8, 12, 12), ((1, 1), (1, 0), 8, 8, 128, 12), ((1, 0), (0, 0), 10, 10, 12, 72),
    ((1, 1), (0, 0), 8, 10, 128, 11), ((1, 1), (0, 0), 8, 10, 11, 72)]
RESAMPLE_DECLINED = [((1, 1), (1, 0), 8), ((1, 0), (0, 0), 8), ((1, 1), (1, 1), 8), ((0, 0), (0, 0), 10),   # test_format_resample_gpu
                     ((1, 0), (1, 1), 9), ((0, 0), (1, 1), 16), ((0, 0), (0, 1), 8)]   # .test_create_declines_what_is_not_down_sampling
SCAN_DECLINED = ((6, 48), (64, 6), (65, 48), (64, 47))                       # test_scan_gpu.test_every_refusal_queues_nothing
BIPLANAR_BLEND_DECLINED = ((66, 38, 12), (1, 38, 8))                         # test_biplanar_gpu.test_what_the_abi_declines
# the drop-ins: (entries, w, h, pixel format as (layout, depth) of the test's own _fmt, or None)
BM3D_DECLINED = [("sigma=3", 24, 18), ("sigma=-1", 64, 48), ("sigma=100000", 64, 48)]   # test_bm3d_gpu.test_declined_keep_the_cpu_filter
SCALED_DROPIN_DECLINED = [("422", 10, "nv12"), ("420", 10, "nv12"), ("420", 12, "p010le"), ("422", 8, "yuv420p10le"),
                          ("444", 10, "yuv422p12le"), ("422", 10, "nv12:hip-planar-step=1")]   # test_format_scaled_gpu.test_drop_in_still_declines_...


def test_declined_creates_hold_nothing(built, monkeypatch):
    """Every create the "declines" tests of the GPU suite show to be refused - through the ABI and through the drop-ins'
    init() - with both counts read before and after it: a refused create holds nothing.  The case lists are the other
    tests' own: taken from their parametrize marks, or repeated above where a test keeps its list inside its body."""
    import test_alias_gpu  # noqa: F401  (the modules whose cases these are: a renamed test fails here, not silently)
    import test_biplanar_gpu as tb
    import test_colorspace_gpu as tc
    import test_colorspace_wide_gpu as tcw
    import test_deblock_gpu as tdb
    import test_bm3d_gpu as tbm
    import test_detelecine_gpu as dt
    import test_format_resample_gpu as tfr
    import test_nlmeans_gpu as tn
    from handbrake_amd import hbrt
    F = hip.filters()
    monkeypatch.delenv("HBHIP_SWSCALE", raising=False)
    ctx = hip.Ctx(0)
    try:
        # what is made once and kept first: this context's frame pool, and the drop-ins' own context
        hip.Frame(ctx, W, H).close()
        hbrt.Chain(F, [("hb_filter_hip_upload", ""), ("hb_filter_lapsharp_hip", tb.LAP), ("hb_filter_hip_download", "")], 66, 38).close()
        ctx.sync()
        held = []

        def declined(what, call, raises=None):
            before = hip.mem_live()
            if raises:
                with pytest.raises(raises):
                    call()
            else:
                rc, handle = call()
                assert rc < 0 and not handle, f"{what}: {rc}"
            held.append((what, before, hip.mem_live()))

        def chain(what, entries, w, h, fmt=None):
            declined(what, lambda: hbrt.Chain(F, entries, w, h, *([] if fmt is None else [fmt])), RuntimeError)

        # ---- through the ABI
        for make, cases in ((hip.format_deepen_device_filter, DEEPEN_DECLINED), (hip.format_scaled_device_filter, SCALED_DECLINED),
                            (hip.format_upsample_device_filter, UPSAMPLE_DECLINED)):
            for src, dst, sd, dd, w, h in cases:
                declined(f"{make.__name__} {src} {dst} {sd} {dd} {w}x{h}", lambda: make(ctx, w, h, src, dst, sd, dd), hip.HipError)
        for src, dst, depth in RESAMPLE_DECLINED:
            declined(f"format resample {src} {dst} {depth}", lambda: hip.format_resample_device_filter(ctx, 128, 72, src, dst, depth),
                     hip.HipError)
        declined("decomb eedi2, odd chroma height", lambda: hip.DecombDevice(ctx, 638, 362, mode=24), hip.HipError)
        declined("blend 4:2:0 on 4:4:4", lambda: _raw("hbhip_blend_create", [C.c_void_p] + [C.c_int] * 8 + [C.POINTER(C.c_void_p)],
                                                      ctx.h, 64, 48, 8, 0, 0, 1, 1, 1))
        for w, h, depth in BIPLANAR_BLEND_DECLINED:
            declined(f"blend biplanar {w}x{h} {depth}", lambda: _raw("hbhip_blend_create_biplanar", [C.c_void_p] + [C.c_int] * 6 +
                                                                     [C.POINTER(C.c_void_p)], ctx.h, w, h, depth, 1, 0, 0))
        for w, h in SCAN_DECLINED:
            declined(f"scan {w}x{h}", lambda: _raw("hbhip_scan_create", [C.c_void_p, C.c_int, C.c_int, C.POINTER(C.c_void_p)], ctx.h, w, h))
        par = hip.NLMeansParams()
        F.hbhip_nlmeans_params_from_settings(hip.NLMEANS_MEDIUM.encode(), 8, C.byref(par))
        declined("nlmeans 16x16", lambda: _raw("hbhip_nlmeans_create", [C.c_void_p, C.POINTER(hip.NLMeansParams)] + [C.c_int] * 5 +
                                               [C.POINTER(C.c_void_p)], ctx.h, C.byref(par), 16, 16, 8, 1, 1))
        for w, h, chroma in _params(dt.test_odd_plane_height_is_declined):
            declined(f"detelecine {w}x{h} {chroma}", lambda: (lambda rc, handle: (rc, handle.value))(*dt.create(ctx, w, h, 8, chroma)))
            chain(f"detelecine drop-in {w}x{h} {chroma}", [("hb_filter_detelecine_hip", "")], w, h, dt.dc.pix_fmt(8, chroma))

        # ---- through the drop-ins
        chain("detelecine margins", [("hb_filter_detelecine_hip", "skip-left=10:skip-right=7")], 128, 64)
        chain("decomb eedi2 drop-in", [("hb_filter_decomb_hip", "mode=31")], 638, 362)
        chain("nlmeans patch 33", [("hb_filter_nlmeans_hip", tn.MEDIUM.replace("y-patch-size=7", "y-patch-size=33"))], 320, 180)
        for st, w, h in BM3D_DECLINED:
            chain(f"bm3d {st} {w}x{h}", [(tbm.DROPIN, st)], w, h)
        chain("deblock 640x362", [(tdb.DROPIN, "strength=strong")], 640, 362)
        chain("crop/scale to odd", [("hb_filter_crop_scale_hip", "width=641:height=361")], 321, 181)
        chain("crop/scale from odd", [("hb_filter_crop_scale_hip", "width=640:height=360")], 641, 360)
        try:
            hbrt.set_source_color(*tc.BT709)
            chain("colorspace bt2020c", [("hb_filter_colorspace_hip", "matrix=bt2020c")], 320, 180)
            for src, settings in _params(tcw.test_still_declined):
                hbrt.set_source_color(*src)
                chain(f"colorspace {src} {settings}", [("hb_filter_colorspace_hip", settings)], 320, 180, hbrt.PIX_FMT[("2x2", 10)])
        finally:
            hbrt.set_source_color()
        for stream, target, w, h in _params(tfr.test_declined_targets_keep_the_cpu_filter):
            chain(f"format {stream} -> {target} {w}x{h}", [("hb_filter_format_hip", f"format={target}")], w, h, tfr._fmt(stream, 8))
        for target in ("yuv420p10le", "yuv420p10le:hip-deepen-step=1"):                 # test_format_deepen_gpu.test_lone_drop_in_still_declines
            chain(f"format 422 -> {target}", [("hb_filter_format_hip", f"format={target}")], 128, 72, tfr._fmt("422", 8))
        for stream, sd, target in SCALED_DROPIN_DECLINED:
            chain(f"format {stream} {sd} -> {target}", [("hb_filter_format_hip", f"format={target}")], 128, 72, tfr._fmt(stream, sd))
        chain("format nv12", [("hb_filter_format_hip", "format=nv12")], 128, 72)      # test_biplanar_gpu.test_format_drop_in_still_declines_nv12
        for (fmt,) in _params(tb.test_adapters_refuse_other_two_plane_formats):
            chain(f"adapters, pixel format {fmt}", [("hb_filter_hip_upload", ""), ("hb_filter_hip_download", "")], 66, 38, fmt)
            # test_biplanar_gpu.test_compositor_refuses_other_two_plane_formats: the compositor's init(), frames of the format's own shape
            assert fmt in (tb.NV16, tb.P012LE)
            frame = (np.zeros((38, 66), np.uint8),) * 2 if fmt == tb.NV16 else (np.zeros((38, 66), np.uint16), np.zeros((19, 66), np.uint16))
            for overlay_fmt in (tb.bc.YUVA420P, tb.bc.YUVA444P):
                declined(f"compositor, pixel format {fmt}, overlays {overlay_fmt}",
                         lambda: hbrt.blend_run(F, "hb_blend_hip", frame, tb.bc.overlays(66, 38, overlay_fmt), pix_fmt=fmt,
                                                overlay_fmt=overlay_fmt), RuntimeError)
        chain("download p010le of 8 bits", [("hb_filter_hip_upload", ""), ("hb_filter_hip_download", "format=p010le")], 66, 38)
        chain("download nv12 of 4:2:2", [("hb_filter_hip_upload", ""), ("hb_filter_hip_download", "format=nv12")], 66, 38, 4)

        print(len(held), "declined creates;", "counts before the first", held[0][1])
        for what, before, after in held:
            assert after == before, f"{what}: a declined create kept memory: {after} against {before}"
    finally:
        ctx.close()
