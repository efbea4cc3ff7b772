"""GPU: P010LE from 8-bit 4:2:0 frames - the widening merge (bi_widen_merge_kernel, csrc/biplanar.hip) through the C ABI
(hbhip_frame_download_widen*, hbhip_frame_export_surface_widen*), through the adapters and through jobs that end in
`format=p010le`, against tests/p010_widen_model.py.  Tolerance 0 throughout."""
import ctypes as C

import numpy as np
import pytest

from handbrake_amd import hbrt, hip
import biplanar_cases as bc
import biplanar_model as bm
import p010_widen_model as pw
import surface_model as sm
from test_surface_gpu import Mem, Rows, fill, plugin_ctx, read

pytestmark = pytest.mark.gpu
ERR_ARG, ERR_UNSUPPORTED = -3, -5
SENTINEL = 0xA5
# 2x2 the smallest legal; 3x3 odd both ways (chroma 2x2 from a 3-wide frame); 18x2 and 34x6 rows that end inside a 16-byte
# output unit (36 and 68 bytes of luma); 66x38 the frame's 128-byte luma pitch against the staging buffer's 192; 130x70 more
# than one workgroup (a 260-byte luma row is 17 units, 105 rows on the grid's y)
SIZES = [(2, 2), (3, 3), (18, 2), (34, 6), (66, 38), (130, 70)]
# (16, 1) wrapped inside one larger allocation / hbhip_surface_alloc's (16, 1) and (256, 16) / two allocations
KINDS = ["tight", "pool16", "hw", "two"]
LAP = "y-strength=0.2:y-kernel=isolap"
WIDEN = "format=p010le:hip-widen-step=1"


@pytest.fixture(scope="module")
def ctx():
    c = hip.Ctx(0)
    yield c
    c.close()


class Pool16(Mem):
    """hbhip_surface_alloc with (pitch_align, rows_align) = (16, 1): both planes in one allocation of the library's, end to end"""

    def __init__(self, ctx, w, h, depth):
        self.ctx, self.kind, self.allocs = ctx, "pool16", []
        self.surface = hip.Surface(ctx, w, h, depth, 16, 1)
        self.lay = sm.pooled(w, h, depth, 16, 1)
        planes, pitches, *_ = self.surface.describe()
        assert pitches == self.lay.pitch and planes[1] - planes[0] == self.lay.offset[1]
        self.parts = [(planes[0], self.lay.size)]


def surface_mem(ctx, kind, w, h):
    return Pool16(ctx, w, h, 10) if kind == "pool16" else Mem(ctx, kind, w, h, 10)


def planar8(rng, w, h):
    ch, cw = pw.chroma_shape(w, h)
    return tuple(rng.integers(0, 256, s, dtype=np.uint8) for s in ((h, w), (ch, cw), (ch, cw)))


def put(fr, x):
    """the samples into the frame, its row padding all ones (a recycled frame's stale bytes: the merge reads them)"""
    rows = Rows(fr)
    rows.buf[:] = 0xFF
    for c in range(3):
        rows.plane(c)[:, :x[c].shape[1]] = x[c]
    rows.upload(fr)


class Host:
    """A P010LE host picture inside one sentinel-filled block.  extra == 0: hb_frame_buffer_init's layout (64-byte rows,
    plane 1 right behind plane 0), which the download fills in one copy, whole rows; else `extra` bytes a row more and a
    gap between the planes, and only the samples' bytes of each row may change."""

    def __init__(self, w, h, extra):
        ch, cw = pw.chroma_shape(w, h)
        self.row_bytes, self.rows = [2 * w, 4 * cw], [h, ch]
        self.pitch = [sm.align(r, 64) for r in self.row_bytes]
        self.stride = [p + extra for p in self.pitch]
        self.may = self.pitch if extra == 0 else self.row_bytes
        gap = 0 if extra == 0 else 192
        self.off = [256, 256 + self.stride[0] * h + gap]
        self.buf = np.full(self.off[1] + self.stride[1] * ch + 256, SENTINEL, dtype=np.uint8)

    def struct(self):
        return hip.HostBiplanar((C.c_void_p * 2)(*[self.buf.ctypes.data + o for o in self.off]), (C.c_int * 2)(*self.stride))

    def _idx(self, p, n):
        return self.off[p] + np.arange(self.rows[p])[:, None] * self.stride[p] + np.arange(n)[None, :]

    def read(self):
        return tuple(np.ascontiguousarray(self.buf[self._idx(p, self.row_bytes[p])]).view("<u2") for p in range(2))

    def untouched(self):
        mask = np.ones(self.buf.size, dtype=bool)
        for p in range(2):
            mask[self._idx(p, self.may[p]).ravel()] = False
        return bool((self.buf[mask] == SENTINEL).all())


def same(got, want, what=""):
    assert len(got) == len(want) == 2
    for p in range(2):
        assert got[p].dtype == np.uint16 and got[p].shape == want[p].shape, (what, p, got[p].shape, want[p].shape)
        np.testing.assert_array_equal(got[p], want[p], err_msg=f"{what} plane {p}")


# ---- the two download forms ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("form", ["sync", "async"])
@pytest.mark.parametrize("extra", [0, 64])
@pytest.mark.parametrize("w,h", SIZES)
def test_download_widen_is_the_model_and_writes_nothing_else(built, ctx, w, h, extra, form):
    L = hip.lib()
    x = planar8(np.random.default_rng(100 * w + h + extra), w, h)
    fr = hip.Frame(ctx, w, h, 8)
    try:
        put(fr, x)
        dst = Host(w, h, extra)
        hb = dst.struct()
        if form == "sync":
            hip.check(L.hbhip_frame_download_widen(fr.h, C.byref(hb)), ctx.h, "download_widen")
        else:
            tok = C.c_void_p()
            hip.check(L.hbhip_frame_download_widen_async(fr.h, C.byref(hb), C.byref(tok)), ctx.h, "download_widen_async")
            assert tok.value
            hip.check(L.hbhip_frame_download_wait(fr.h, tok), ctx.h, "download_wait")
        same(dst.read(), pw.merge(x))
        assert dst.untouched()
        for got, was in zip(fr.download(), x):                          # the frame is only read
            np.testing.assert_array_equal(got, was)
    finally:
        fr.close()


def test_the_result_is_not_the_shifted_form(built, ctx):
    """t | t << 8, not t << 8 (and not the 10-bit merges' << 6): the low byte of every word is the sample again"""
    w, h = 66, 38
    x = planar8(np.random.default_rng(9), w, h)
    fr = hip.Frame(ctx, w, h, 8)
    s = Mem(ctx, "hw", w, h, 10)
    try:
        put(fr, x)
        dst = Host(w, h, 0)
        hb = dst.struct()
        hip.check(hip.lib().hbhip_frame_download_widen(fr.h, C.byref(hb)), ctx.h, "download_widen")
        fr.export_surface_widen(s.surface)
        buf = s.download()
        for got in (dst.read(), tuple(sm.plane_rows(buf, s.lay, p) for p in range(2))):
            assert (got[0] & 0xFF).any() and (got[1] & 0xFF).any()
            assert any((got[p] != (got[p] & 0xFF00)).any() for p in range(2))            # t << 8 would fail here
            np.testing.assert_array_equal(got[0] & 0xFF, x[0])
            np.testing.assert_array_equal(got[0] >> 8, x[0])
            np.testing.assert_array_equal(got[1][:, 0::2] & 0xFF, x[1])
            np.testing.assert_array_equal(got[1][:, 1::2] & 0xFF, x[2])
    finally:
        s.close()
        fr.close()


# ---- the two export forms -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("form", ["sync", "async"])
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("w,h", SIZES)
def test_export_widen_is_the_model_and_writes_nothing_else(built, ctx, w, h, kind, form):
    """guard bands, row padding, padded rows and the gap between the planes hold 0xA5 before and after: only
    [0, align16(row bytes)) of the sample rows may change, and the samples there are the model's"""
    L = hip.lib()
    x = planar8(np.random.default_rng(200 * w + h), w, h)
    mem = surface_mem(ctx, kind, w, h)
    fr = hip.Frame(ctx, w, h, 8)
    try:
        lay = mem.lay
        mem.upload(np.full(lay.size, SENTINEL, dtype=np.uint8))
        put(fr, x)
        if form == "sync":
            fr.export_surface_widen(mem.surface)
        else:
            tok = C.c_void_p()
            hip.check(L.hbhip_frame_export_surface_widen_async(fr.h, mem.surface.h, C.byref(tok)), ctx.h, "export_widen_async")
            assert tok.value
            hip.check(L.hbhip_frame_download_wait(fr.h, tok), ctx.h, "download_wait")
        got = mem.download()
        want = pw.place(np.full(lay.size, SENTINEL, dtype=np.uint8), lay.offset, lay.pitch, x)
        same(tuple(sm.plane_rows(got, lay, p) for p in range(2)), tuple(sm.plane_rows(want, lay, p) for p in range(2)))
        same(tuple(sm.plane_rows(got, lay, p) for p in range(2)), pw.merge(x))
        assert (got[~lay.written()] == SENTINEL).all(), "bytes outside [0, align16(row bytes)) of the sample rows were written"
        for g, was in zip(fr.download(), x):
            np.testing.assert_array_equal(g, was)
    finally:
        fr.close()
        mem.close()


# ---- order --------------------------------------------------------------------------------------------------------------
def test_seventeen_in_flight_exports_and_downloads_share_their_inputs(built, ctx):
    """four resident frames, seventeen exports and seventeen downloads of them queued without a wait: one staging buffer and
    one stream carry the downloads, each pair in order; the shared inputs are only read"""
    L = hip.lib()
    w, h, n = 66, 38, 17
    rng = np.random.default_rng(17)
    xs = [planar8(rng, w, h) for _ in range(4)]
    frames = [hip.Frame(ctx, w, h, 8) for _ in range(4)]
    mems = [Mem(ctx, "hw" if i & 1 else "tight", w, h, 10) for i in range(n)]
    hosts = [Host(w, h, 0 if i & 1 else 64) for i in range(n)]
    structs = [hst.struct() for hst in hosts]
    try:
        for fr, x in zip(frames, xs):
            put(fr, x)
        for m in mems:
            m.upload(np.full(m.lay.size, SENTINEL, dtype=np.uint8))
        tokens = []
        for i in range(n):
            fr = frames[i % 4]
            for call, arg in ((L.hbhip_frame_export_surface_widen_async, mems[i].surface.h),
                              (L.hbhip_frame_download_widen_async, C.byref(structs[i]))):
                t = C.c_void_p()
                hip.check(call(fr.h, arg, C.byref(t)), ctx.h, "queue")
                tokens.append((fr, t))
        for fr, t in tokens:
            hip.check(L.hbhip_frame_download_wait(fr.h, t), ctx.h, "download_wait")
        for i in range(n):
            want = pw.merge(xs[i % 4])
            same(hosts[i].read(), want, f"download {i}")
            assert hosts[i].untouched()
            buf = mems[i].download()
            same(tuple(sm.plane_rows(buf, mems[i].lay, p) for p in range(2)), want, f"export {i}")
            assert (buf[~mems[i].lay.written()] == SENTINEL).all()
        for fr, x in zip(frames, xs):
            for got, was in zip(fr.download(), x):
                np.testing.assert_array_equal(got, was, err_msg="an input was written")
    finally:
        ctx.sync()
        for fr in frames:
            fr.close()
        for m in mems:
            m.close()


def test_export_waits_for_an_earlier_import_of_the_surface(built, ctx):
    """picture A in the surface; an import of it and, with no wait between, an export of picture B into it: the import
    delivers A (as ten-bit samples: the words >> 6), the surface ends as B"""
    L = hip.lib()
    w, h = 1922, 1082
    rng = np.random.default_rng(5)
    a, b = planar8(rng, w, h), planar8(rng, w, h)
    fa, fb, back = hip.Frame(ctx, w, h, 8), hip.Frame(ctx, w, h, 8), hip.Frame(ctx, w, h, 10)
    mem = Mem(ctx, "hw", w, h, 10)
    try:
        fa.upload(a)
        fb.upload(b)
        fa.export_surface_widen(mem.surface)
        ti, te = C.c_void_p(), C.c_void_p()
        hip.check(L.hbhip_frame_import_surface_async(back.h, mem.surface.h, C.byref(ti)), ctx.h, "import async")
        hip.check(L.hbhip_frame_export_surface_widen_async(fb.h, mem.surface.h, C.byref(te)), ctx.h, "export_widen_async")
        hip.check(L.hbhip_ctx_upload_done(ctx.h, ti, 1), ctx.h, "upload_done")
        hip.check(L.hbhip_frame_download_wait(fb.h, te), ctx.h, "download_wait")
        for got, was in zip(back.download(), a):
            np.testing.assert_array_equal(got, pw.widen(was) >> 6, err_msg="the import saw the later export")
        buf = mem.download()
        same(tuple(sm.plane_rows(buf, mem.lay, p) for p in range(2)), pw.merge(b))
    finally:
        ctx.sync()
        for f in (fa, fb, back):
            f.close()
        mem.close()


# ---- refusals -----------------------------------------------------------------------------------------------------------
def test_what_is_refused_before_anything_is_queued(built, ctx):
    L = hip.lib()
    w, h = 18, 10
    s10, s8, wider = hip.Surface(ctx, w, h, 10, 16, 1), hip.Surface(ctx, w, h, 8, 16, 1), hip.Surface(ctx, w + 2, h, 10, 16, 1)
    host = Host(w, h, 64)
    hb = host.struct()
    tok = C.c_void_p()
    block = C.c_void_p()
    hip.check(L.hbhip_dev_alloc(ctx.h, 1 << 16, C.byref(block)), ctx.h, "dev_alloc")
    try:
        before = ctx.bus_bytes()
        for fw, fh, depth, lcw, lch, s in ((w, h, 8, 1, 0, s10),          # a 4:2:2 frame
                                           (w, h, 8, 0, 0, s10),          # 4:4:4
                                           (w, h, 10, 1, 1, s10),         # a frame that has ten bits already: the plain export's
                                           (w, h, 12, 1, 1, s10),
                                           (w, h, 8, 1, 1, s8),           # a surface that is not depth 10
                                           (w, h, 8, 1, 1, wider),        # of another size
                                           (1, h, 8, 1, 1, s10),          # a width below 2
                                           (w, 1, 8, 1, 1, s10)):         # a height below 2
            fr = hip.Frame(ctx, fw, fh, depth, lcw, lch)
            assert L.hbhip_frame_export_surface_widen(fr.h, s.h) == ERR_UNSUPPORTED
            assert L.hbhip_frame_export_surface_widen_async(fr.h, s.h, C.byref(tok)) == ERR_UNSUPPORTED and not tok.value
            if s is s10:                                                   # (the download looks at the frame alone)
                assert L.hbhip_frame_download_widen(fr.h, C.byref(hb)) == ERR_UNSUPPORTED
                assert L.hbhip_frame_download_widen_async(fr.h, C.byref(hb), C.byref(tok)) == ERR_UNSUPPORTED and not tok.value
            fr.close()
        fr = hip.Frame(ctx, w, h, 8)
        short = hip.HostBiplanar((C.c_void_p * 2)(*hb.plane), (C.c_int * 2)(2 * w - 2, hb.stride[1]))     # under P010's 36 bytes
        narrow = hip.HostBiplanar((C.c_void_p * 2)(*hb.plane), (C.c_int * 2)(hb.stride[0], 4 * 9 - 2))
        missing = hip.HostBiplanar((C.c_void_p * 2)(hb.plane[0], None), (C.c_int * 2)(*hb.stride))
        for bad in (short, narrow, missing):
            assert L.hbhip_frame_download_widen(fr.h, C.byref(bad)) == ERR_ARG
            assert L.hbhip_frame_download_widen_async(fr.h, C.byref(bad), C.byref(tok)) == ERR_ARG and not tok.value
        assert L.hbhip_frame_download_widen_async(fr.h, C.byref(hb), None) == ERR_ARG
        assert L.hbhip_frame_export_surface_widen_async(fr.h, s10.h, None) == ERR_ARG
        assert L.hbhip_frame_export_surface_widen(fr.h, None) == ERR_ARG
        # the plain entry points still refuse the depth mismatch this pair exists for
        assert L.hbhip_frame_export_surface(fr.h, s10.h) == ERR_UNSUPPORTED
        fr.close()
        # a depth-10 surface's pitch, address and overlap conditions (hbhip_surface_wrap's): the row is 36 bytes of luma here
        out, b = C.c_void_p(), block.value

        def wrap(planes, pitches):
            mem = hip.DevSurface((C.c_void_p * 2)(*planes), (C.c_int * 2)(*pitches))
            rc = L.hbhip_surface_wrap(ctx.h, C.byref(mem), w, h, 10, None, None, C.byref(out))
            assert (rc == 0) == bool(out.value)
            return rc

        assert wrap([b, b + 4096], [32, 48]) == ERR_ARG                    # a pitch below the row bytes
        assert wrap([b, b + 4096], [48, 32]) == ERR_ARG
        assert wrap([b, b + 4096], [40, 48]) == ERR_UNSUPPORTED            # no multiple of 16
        assert wrap([b + 8, b + 4096], [48, 48]) == ERR_UNSUPPORTED        # a base that is no multiple of 16
        assert wrap([b, b + 48 * 9], [48, 48]) == ERR_ARG                  # plane 1 starts inside plane 0's last row
        assert ctx.bus_bytes() == before
        assert (host.buf == SENTINEL).all()
    finally:
        L.hbhip_dev_free(ctx.h, block)
        for s in (s10, s8, wider):
            s.close()


# ---- jobs ---------------------------------------------------------------------------------------------------------------
W, H, N = 66, 38, 3


@pytest.fixture(scope="module")
def pictures():
    """three 8-bit 4:2:0 frames and what the lapsharp oracle makes of them, widened: computed once, only read"""
    import oracle_stream as os_
    import golden_cases as gc
    rng = np.random.default_rng(66)
    frames = [planar8(rng, W, H) for _ in range(N)]
    sharp = os_.lapsharp_stream(frames, [gc.lap(depth=8)] * 3)
    assert any((sharp[0][0] != frames[0][0]).ravel())                       # the filter did something
    want = [pw.merge(fr) for fr in sharp]
    for p in want[0]:
        p.flags.writeable = False
    return frames, want


def _registered():
    F = hbrt.FILTER_ID
    # (guard as in tests/test_format_scaled_gpu.py: a library from before the fallback's own guard would spin in the job)
    assert hasattr(hip.lib(), "hbhip_format_scaled_create") and hasattr(hip.lib(), "hbhip_frame_download_widen")
    return hbrt.register_filters(hip.filters(), {F["lapsharp"]: "hb_filter_lapsharp_hip", F["format"]: "hb_filter_format_hip"})


def _unregister():
    F = hbrt.FILTER_ID
    hbrt.register_filters(hip.filters(), {F["lapsharp"]: None, F["format"]: None})


def _four_stages(names):
    assert len(names) == 4, names
    assert names[0] == "HIP upload adapter" and names[2] == "Format (HIP)" and names[3] == "HIP download adapter", names
    assert "HIP" in names[1] and "harp" in names[1]


def _job_filters():
    F = hbrt.FILTER_ID
    return [(F["lapsharp"], LAP), (F["format"], "format=p010le")]


def test_job_lapsharp_format_p010le_on_yuv420p(built, pictures):
    frames, want = pictures
    _registered()
    try:
        names, got = hbrt.run_job(_job_filters(), frames)
    finally:
        _unregister()
    _four_stages(names)
    assert len(got) == N
    for t in range(N):
        same(got[t].planes, want[t], f"frame {t}")
    assert (got[0].planes[0] & 0xFF).any()                                  # not << 8


def test_run_with_surface_1_ends_in_depth_10_surfaces(built, pictures):
    """the same list with surface=1 on its download adapter: P010LE surface buffers of the pool, nothing of them over the bus"""
    frames, want = pictures
    pctx = plugin_ctx()
    stages = [("hb_filter_hip_upload", ""), ("hb_filter_lapsharp_hip", LAP), ("hb_filter_format_hip", WIDEN),
              ("hb_filter_hip_download", WIDEN + ":surface=1")]
    got = []
    try:
        with hbrt.Chain(hip.filters(), stages, W, H) as ch:
            d2h = pctx.bus_bytes()[1]
            for t, fr in enumerate(frames):
                ch.push(fr, start=t * 3003, stop=(t + 1) * 3003)
            ch.push_eof()
            while ch.pending():
                o = ch.pop_surface()
                assert o is not None or ch.eof
                if o is not None:
                    got.append(o)
            assert ch.eof
        assert pctx.bus_bytes()[1] == d2h
        assert len(got) == N
        for t, (s, info) in enumerate(got):
            assert (info.start, info.fmt, info.width, info.height, info.nplanes) == (t * 3003, bc.P010LE, W, H, 0)
            assert s.describe()[2:] == (W, H, 10)
            same(read(pctx, s), want[t], f"frame {t}")
    finally:
        for s, _ in got:
            s.close()


def test_the_widen_key_is_internal_and_bound_to_its_case(built):
    """without the key the adapter and the drop-in decline as before; with it, only format=p010le on 8-bit 4:2:0 frames
    inside a run is taken"""
    F = hip.filters()
    up = ("hb_filter_hip_upload", "")
    for stages, pix_fmt in (([up, ("hb_filter_hip_download", "format=p010le")], 0),
                            ([up, ("hb_filter_hip_download", "format=nv12:hip-widen-step=1")], hbrt.PIX_FMT[("2x2", 10)]),
                            ([up, ("hb_filter_hip_download", WIDEN)], hbrt.PIX_FMT[("2x1", 8)]),
                            ([up, ("hb_filter_hip_download", WIDEN)], hbrt.PIX_FMT[("2x2", 12)]),
                            ([("hb_filter_format_hip", WIDEN)], 0),                           # a lone drop-in: no run, no adapter
                            ([up, ("hb_filter_format_hip", WIDEN), ("hb_filter_hip_download", "")], hbrt.PIX_FMT[("2x1", 8)]),
                            ([up, ("hb_filter_format_hip", "format=p010le"), ("hb_filter_hip_download", "")], 0)):
        with pytest.raises(RuntimeError):
            hbrt.Chain(F, stages, W, H, pix_fmt)
    hbrt.Chain(F, [up, ("hb_filter_hip_download", WIDEN)], W, H).close()
    hbrt.Chain(F, [up, ("hb_filter_hip_download", WIDEN)], W, H, hbrt.PIX_FMT[("2x2", 10)]).close()      # ten bits: the plain repack


def _nv12(frames):
    return [bm.merge(fr, 8) for fr in frames]


def test_job_on_an_nv12_job_with_host_pictures_in(built, pictures):
    frames, want = pictures
    _registered()
    try:
        names, got = hbrt.run_job(_job_filters(), _nv12(frames), pix_fmt=bc.NV12)
    finally:
        _unregister()
    _four_stages(names)
    assert len(got) == N
    for t in range(N):
        same(got[t].planes, want[t], f"frame {t}")


def test_job_on_an_nv12_job_with_surfaces_in(built, pictures):
    frames, want = pictures
    pctx = plugin_ctx()
    hip.filters()
    _registered()
    srcs, got = [], []
    try:
        with hbrt.Job(_job_filters(), W, H, bc.NV12) as job:                 # (opened first: the context exists from here on)
            names = job.stages()
            srcs = [hip.Surface(pctx, W, H, 8) for _ in range(N)]
            for s, pic in zip(srcs, _nv12(frames)):
                fill(pctx, s, pic)
            h2d = pctx.bus_bytes()[0]
            for t, s in enumerate(srcs):
                job.push_surface(s, pts=t * 3003)
                got += job.drain()
            job.push_eof()
            got += job.drain()
            assert pctx.bus_bytes()[0] == h2d                               # nothing went up over the bus
    finally:
        _unregister()
        for s in srcs:
            s.close()
    _four_stages(names)
    assert len(got) == N
    for t in range(N):
        same(got[t].planes, want[t], f"frame {t}")
