"""GPU: NV12 / P010LE through the C ABI (repack kernels, csrc/biplanar.hip), the compositor drop-in, the upload / download
adapters and a job - against tests/biplanar_model.py, which tests/test_biplanar_cpu.py pins to the reference."""
import ctypes as C

import numpy as np
import pytest

from handbrake_amd import hbrt, hip
import biplanar_model as bm
import biplanar_cases as bc

pytestmark = pytest.mark.gpu
SIZES = [(2, 2), (66, 38), (258, 130)]       # narrower than one vector access / rows of an odd count of dwords / > one workgroup
SENTINEL = 0xA5


def align64(n):
    return -(-n // 64) * 64


class HostPlanes:
    """Host planes inside one sentinel-filled block: `extra` bytes of stride beyond the 64-byte pitch, a guard in front of,
    between and behind the planes.  untouched(): every byte outside the planes' rows-and-padding still is the sentinel."""

    def __init__(self, row_bytes, rows, extra):
        self.row_bytes, self.rows = row_bytes, rows
        self.pitch = [align64(r) for r in row_bytes]
        self.stride = [p + extra for p in self.pitch]
        guard = 0 if extra == 0 else 192                                  # extra == 0: the planes back to back (the 1-D copy)
        self.off, at = [], 256
        for s, n in zip(self.stride, rows):
            self.off.append(at)
            at += s * n + guard
        self.buf = np.full(at + 256, SENTINEL, dtype=np.uint8)

    def plane(self, p):
        return self.buf[self.off[p]:self.off[p] + self.stride[p] * self.rows[p]].reshape(self.rows[p], self.stride[p])

    def fill(self, arrays):
        for p, a in enumerate(arrays):
            self.plane(p)[:, :self.row_bytes[p]] = np.ascontiguousarray(a).view(np.uint8).reshape(self.rows[p], -1)

    def read(self, dtype):
        return tuple(np.ascontiguousarray(self.plane(p)[:, :self.row_bytes[p]]).view(dtype) for p in range(len(self.rows)))

    def struct(self, cls):
        s = cls()
        for p in range(len(self.rows)):
            s.plane[p] = self.buf.ctypes.data + self.off[p]
            s.stride[p] = self.stride[p]
        return s

    def untouched(self):
        mask = np.ones(self.buf.size, dtype=bool)
        for p in range(len(self.rows)):
            rows = np.arange(self.rows[p])[:, None] * self.stride[p] + self.off[p]
            mask[(rows + np.arange(self.pitch[p])[None, :]).ravel()] = False
        return bool((self.buf[mask] == SENTINEL).all())


def planar_host(w, h, bps, extra=0):
    ch, cw = (h + 1) // 2, (w + 1) // 2
    return HostPlanes([w * bps, cw * bps, cw * bps], [h, ch, ch], extra)


def biplanar_host(w, h, bps, extra=0):
    ch, cw = (h + 1) // 2, (w + 1) // 2
    return HostPlanes([w * bps, 2 * cw * bps], [h, ch], extra)


@pytest.fixture(scope="module")
def ctx():
    c = hip.Ctx(0)
    yield c
    c.close()


def new_frame(ctx, w, h, depth):
    fr = C.c_void_p()
    hip.check(hip.lib().hbhip_frame_alloc(ctx.h, w, h, depth, 1, 1, C.byref(fr)), ctx.h, "frame_alloc")
    return fr


@pytest.mark.parametrize("extra", [0, 64])
@pytest.mark.parametrize("pix_fmt", [bc.NV12, bc.P010LE])
@pytest.mark.parametrize("w,h", SIZES)
def test_upload_biplanar_is_split_and_download_biplanar_is_merge(built, ctx, w, h, pix_fmt, extra):
    L = hip.lib()
    depth, bps, dt = (8, 1, np.uint8) if pix_fmt == bc.NV12 else (10, 2, np.uint16)
    y = bc.frame(pix_fmt, w, h, seed=extra)
    fr = new_frame(ctx, w, h, depth)
    try:
        src = biplanar_host(w, h, bps, extra)
        src.fill(y)
        hb = src.struct(hip.HostBiplanar)
        hip.check(L.hbhip_frame_upload_biplanar(fr, C.byref(hb)), ctx.h, "upload_biplanar")
        dst = planar_host(w, h, bps, extra)
        hf = dst.struct(hip.HostFrame)
        hip.check(L.hbhip_frame_download(fr, C.byref(hf)), ctx.h, "download")
        for got, want in zip(dst.read(dt), bm.split(y, depth)):
            np.testing.assert_array_equal(got, want)
        assert dst.untouched()
        # and back: the planar frame as it is in HBM now, merged
        back = biplanar_host(w, h, bps, extra)
        hb2 = back.struct(hip.HostBiplanar)
        hip.check(L.hbhip_frame_download_biplanar(fr, C.byref(hb2)), ctx.h, "download_biplanar")
        for got, want in zip(back.read(dt), y):
            np.testing.assert_array_equal(got, want)
        assert back.untouched()
    finally:
        L.hbhip_frame_release(fr)


@pytest.mark.parametrize("pix_fmt", [bc.NV12, bc.P010LE])
@pytest.mark.parametrize("w,h", SIZES)
def test_planar_upload_then_download_biplanar_is_merge(built, ctx, w, h, pix_fmt):
    """arbitrary planar content, a frame whose row padding came from a planar host upload: the merge is << 6 with the low
    six bits zero"""
    L = hip.lib()
    depth, bps, dt = (8, 1, np.uint8) if pix_fmt == bc.NV12 else (10, 2, np.uint16)
    rng = np.random.default_rng(depth + w)
    ch, cw = (h + 1) // 2, (w + 1) // 2
    x = tuple(rng.integers(0, 1 << depth, s).astype(dt) for s in ((h, w), (ch, cw), (ch, cw)))
    fr = new_frame(ctx, w, h, depth)
    try:
        src = planar_host(w, h, bps)
        src.fill(x)
        hf = src.struct(hip.HostFrame)
        hip.check(L.hbhip_frame_upload(fr, C.byref(hf)), ctx.h, "upload")
        dst = biplanar_host(w, h, bps)
        hb = dst.struct(hip.HostBiplanar)
        hip.check(L.hbhip_frame_download_biplanar(fr, C.byref(hb)), ctx.h, "download_biplanar")
        for got, want in zip(dst.read(dt), bm.merge(x, depth)):
            np.testing.assert_array_equal(got, want)
        assert dst.untouched()
    finally:
        L.hbhip_frame_release(fr)


@pytest.mark.parametrize("pix_fmt", [bc.NV12, bc.P010LE])
def test_host_row_padding_travels_on_the_strided_upload(built, ctx, pix_fmt):
    """A host picture with strides of its own takes the 2-D copy: its row padding (up to the 64-byte pitch) comes along and
    the split hands it on, as the planar upload does - the filters behind read it (lapsharp.c:145-157).  Seen through a
    planar download in the frame's own layout, which moves whole rows."""
    L = hip.lib()
    w, h = 66, 38
    depth, bps, dt = (8, 1, np.uint8) if pix_fmt == bc.NV12 else (10, 2, np.uint16)
    rng = np.random.default_rng(7)
    fr = new_frame(ctx, w, h, depth)
    try:
        src = biplanar_host(w, h, bps, extra=64)
        for p in range(2):
            src.plane(p)[:, :src.pitch[p]] = rng.integers(0, 256, (src.rows[p], src.pitch[p]), dtype=np.uint8)
        hb = src.struct(hip.HostBiplanar)
        hip.check(L.hbhip_frame_upload_biplanar(fr, C.byref(hb)), ctx.h, "upload_biplanar")
        dst = planar_host(w, h, bps)
        hf = dst.struct(hip.HostFrame)
        hip.check(L.hbhip_frame_download(fr, C.byref(hf)), ctx.h, "download")
        whole = tuple(np.ascontiguousarray(src.plane(p)[:, :src.pitch[p]]).view(dt) for p in range(2))
        want = bm.split(whole, depth)                        # the rows as wide as their pitch
        got = [np.ascontiguousarray(dst.plane(p)).view(dt) for p in range(3)]
        np.testing.assert_array_equal(got[0], want[0])
        half = want[1].shape[1]                              # half the interleaved pitch <= the planar pitch
        for p in (1, 2):
            np.testing.assert_array_equal(got[p][:, :half], want[p], err_msg=f"plane {p}")
            assert (got[p][:, half:] == 0).all()             # where the planar row is the longer one the split clears it
    finally:
        L.hbhip_frame_release(fr)


@pytest.mark.parametrize("pix_fmt", [bc.NV12, bc.P010LE])
def test_eight_in_flight_keep_their_order(built, ctx, pix_fmt):
    L = hip.lib()
    w, h, n = 258, 130, 8
    depth, bps, dt = (8, 1, np.uint8) if pix_fmt == bc.NV12 else (10, 2, np.uint16)
    pics = [bc.frame(pix_fmt, w, h, seed=k) for k in range(n)]
    frames = [new_frame(ctx, w, h, depth) for _ in range(n)]
    try:
        srcs, tokens = [], []
        for k in range(n):
            s = biplanar_host(w, h, bps)
            s.fill(pics[k])
            srcs.append((s, s.struct(hip.HostBiplanar)))
            t = C.c_void_p()
            hip.check(L.hbhip_frame_upload_biplanar_async(frames[k], C.byref(srcs[k][1]), C.byref(t)), ctx.h, "upload async")
            tokens.append(t)
        for t in tokens:
            assert L.hbhip_ctx_upload_done(ctx.h, t, 1) == 0
        dsts, tokens = [], []
        for k in range(n):
            d = biplanar_host(w, h, bps)
            dsts.append((d, d.struct(hip.HostBiplanar)))
            t = C.c_void_p()
            hip.check(L.hbhip_frame_download_biplanar_async(frames[k], C.byref(dsts[k][1]), C.byref(t)), ctx.h, "download async")
            tokens.append(t)
        for k in range(n):
            assert L.hbhip_frame_download_wait(frames[k], tokens[k]) == 0
        for k in range(n):
            for got, want in zip(dsts[k][0].read(dt), pics[k]):
                np.testing.assert_array_equal(got, want, err_msg=f"picture {k}")
            assert dsts[k][0].untouched()
        # the planar pictures in between are the split ones
        chk = planar_host(w, h, bps)
        hf = chk.struct(hip.HostFrame)
        hip.check(L.hbhip_frame_download(frames[n - 1], C.byref(hf)), ctx.h, "download")
        for got, want in zip(chk.read(dt), bm.split(pics[n - 1], depth)):
            np.testing.assert_array_equal(got, want)
    finally:
        for fr in frames:
            L.hbhip_frame_release(fr)


def test_what_the_abi_declines(built, ctx):
    L = hip.lib()
    host = biplanar_host(66, 38, 2)
    hb = host.struct(hip.HostBiplanar)
    for w, h, depth, lcw, lch in ((66, 38, 12, 1, 1), (66, 38, 8, 1, 0), (1, 38, 8, 1, 1), (66, 1, 8, 1, 1)):
        fr = C.c_void_p()
        hip.check(L.hbhip_frame_alloc(ctx.h, w, h, depth, lcw, lch, C.byref(fr)), ctx.h, "frame_alloc")
        assert L.hbhip_frame_upload_biplanar(fr, C.byref(hb)) == -5          # HBHIP_ERR_UNSUPPORTED
        assert L.hbhip_frame_download_biplanar(fr, C.byref(hb)) == -5
        L.hbhip_frame_release(fr)
    L.hbhip_blend_create_biplanar.argtypes = [C.c_void_p] + [C.c_int] * 6 + [C.POINTER(C.c_void_p)]
    L.hbhip_blend_create.argtypes = [C.c_void_p] + [C.c_int] * 8 + [C.POINTER(C.c_void_p)]
    L.hbhip_blend_destroy.argtypes = [C.c_void_p]
    L.hbhip_blend_destroy.restype = None
    for fn in ("hbhip_blend_apply", "hbhip_blend_apply_dev", "hbhip_blend_apply_biplanar"):
        getattr(L, fn).argtypes = [C.c_void_p, C.c_void_p]
    b = C.c_void_p()
    assert L.hbhip_blend_create_biplanar(ctx.h, 66, 38, 12, 1, 0, 0, C.byref(b)) == -5
    assert L.hbhip_blend_create_biplanar(ctx.h, 1, 38, 8, 1, 0, 0, C.byref(b)) == -5
    assert L.hbhip_blend_create_biplanar(ctx.h, 66, 38, 8, 1, 0, 0, C.byref(b)) == 0
    hf, df = hip.HostFrame(), hip.DevFrame()
    assert L.hbhip_blend_apply(b, C.byref(hf)) == -3                          # HBHIP_ERR_ARG
    assert L.hbhip_blend_apply_dev(b, C.byref(df)) == -3
    L.hbhip_blend_destroy(b)
    assert L.hbhip_blend_create(ctx.h, 66, 38, 8, 1, 1, 1, 0, 0, C.byref(b)) == 0
    assert L.hbhip_blend_apply_biplanar(b, C.byref(hb)) == -3
    L.hbhip_blend_destroy(b)


# ---- compositor -----------------------------------------------------------------------------------------------------
def check_blend(pix_fmt, overlay_fmt, loc, w, h, ovs, passes=1):
    frame = bc.frame(pix_fmt, w, h)
    got = hbrt.blend_run(hip.filters(), "hb_blend_hip", frame, ovs, pix_fmt=pix_fmt, overlay_fmt=overlay_fmt,
                         chroma_location=loc, passes=passes)
    want = bm.blend_bi(frame, ovs, bc.DEPTH[pix_fmt], loc, bc.SHIFTS[overlay_fmt])
    assert any((a != b).any() for a, b in zip(want, frame))
    for p in range(2):
        np.testing.assert_array_equal(got[p], want[p], err_msg=f"plane {p}")
    return got


@pytest.mark.parametrize("w,h", [(66, 38), (258, 130)])
@pytest.mark.parametrize("pix_fmt,overlay_fmt,loc", bc.CASES)
def test_compositor_is_the_model(built, pix_fmt, overlay_fmt, loc, w, h):
    got = check_blend(pix_fmt, overlay_fmt, loc, w, h, bc.overlays(w, h, overlay_fmt))
    if pix_fmt == bc.P010LE:
        assert any((p & 63 != 0).any() for p in got)          # composited MSB-aligned, not as planar 10-bit


@pytest.mark.parametrize("pix_fmt", [bc.NV12, bc.P010LE])
@pytest.mark.parametrize("overlay_fmt", [bc.YUVA420P, bc.YUVA444P])
def test_nine_disjoint_overlays_take_two_launches(built, pix_fmt, overlay_fmt):
    check_blend(pix_fmt, overlay_fmt, 1, 258, 130, bc.nine_disjoint(258, 130, overlay_fmt))


@pytest.mark.parametrize("pix_fmt", [bc.NV12, bc.P010LE])
def test_unchanged_overlays_are_reused(built, pix_fmt):
    check_blend(pix_fmt, bc.YUVA444P, 1, 66, 38, bc.overlays(66, 38, bc.YUVA444P), passes=2)


NV16, P012LE = 101, 207          # the stand-in runtime's numbers for two more of the family (libhb/hb_runtime.c)


@pytest.mark.parametrize("pix_fmt", [NV16, P012LE])
def test_compositor_refuses_other_two_plane_formats(built, pix_fmt):
    """with a device present init() gets as far as the two-plane rule: NV16 (4:2:2) and P012LE (12 bits, shift 4) have no
    kernels.  The frames have the formats' own shapes, so that an init() that took them would not read past them."""
    w, h = 66, 38
    assert hbrt.runtime().av_pix_fmt_count_planes(pix_fmt) == 2
    rng = np.random.default_rng(pix_fmt)
    if pix_fmt == NV16:
        frame = (rng.integers(0, 256, (h, w), dtype=np.uint8), rng.integers(0, 256, (h, w), dtype=np.uint8))
    else:
        frame = tuple((rng.integers(0, 4096, s) << 4).astype(np.uint16) for s in ((h, w), (h // 2, w)))
    for overlay_fmt in (bc.YUVA420P, bc.YUVA444P):
        with pytest.raises(RuntimeError):
            hbrt.blend_run(hip.filters(), "hb_blend_hip", frame, bc.overlays(w, h, overlay_fmt), pix_fmt=pix_fmt,
                           overlay_fmt=overlay_fmt)
    # the drop-in itself works here: the same call on NV12 goes through
    hbrt.blend_run(hip.filters(), "hb_blend_hip", bc.frame(bc.NV12, w, h), bc.overlays(w, h, bc.YUVA444P), pix_fmt=bc.NV12)


@pytest.mark.parametrize("pix_fmt", [NV16, P012LE])
def test_adapters_refuse_other_two_plane_formats(built, pix_fmt):
    with pytest.raises(RuntimeError):
        hbrt.Chain(hip.filters(), [("hb_filter_hip_upload", ""), ("hb_filter_hip_download", "")], 66, 38, pix_fmt=pix_fmt)


# ---- adapters ---------------------------------------------------------------------------------------------------------
LAP = "y-strength=0.2:y-kernel=isolap"


@pytest.mark.parametrize("pix_fmt,name", [(bc.NV12, "nv12"), (bc.P010LE, "p010le")])
def test_stream_enters_and_leaves_biplanar(built, pix_fmt, name):
    import oracle_stream as os_
    import golden_cases as gc
    depth = bc.DEPTH[pix_fmt]
    frames = [bc.frame(pix_fmt, 66, 38, seed=t) for t in range(3)]
    chain = [("hb_filter_hip_upload", ""), ("hb_filter_lapsharp_hip", LAP), ("hb_filter_hip_download", f"format={name}")]
    got = hbrt.run_stream(hip.filters(), chain, frames, pix_fmt=pix_fmt)
    want = [bm.merge(f, depth) for f in os_.lapsharp_stream([bm.split(f, depth) for f in frames], [gc.lap(depth=depth)] * 3)]
    assert len(got) == 3
    for t in range(3):
        assert len(got[t].planes) == 2
        for p in range(2):
            np.testing.assert_array_equal(got[t].planes[p], want[t][p], err_msg=f"frame {t} plane {p}")


def test_download_format_must_fit_the_run(built):
    with pytest.raises(RuntimeError):
        hbrt.Chain(hip.filters(), [("hb_filter_hip_upload", ""), ("hb_filter_hip_download", "format=p010le")], 66, 38)
    with pytest.raises(RuntimeError):
        hbrt.Chain(hip.filters(), [("hb_filter_hip_upload", ""), ("hb_filter_hip_download", "format=nv12")], 66, 38, pix_fmt=4)


def test_format_drop_in_still_declines_nv12(built):
    """the old contract (tests/test_format_gpu.py::test_unsupported_targets_keep_the_cpu_filter): the repack lives in the
    adapters, hb_filter_format_hip has no biplanar target"""
    with pytest.raises(RuntimeError):
        hbrt.Chain(hip.filters(), [("hb_filter_format_hip", "format=nv12")], 128, 72)


# ---- a job ------------------------------------------------------------------------------------------------------------
def test_nv12_job_keeps_its_format(built):
    """pix_fmt NV12: [render_sub, lapsharp] - the lone drop-in gets its adapters (it cannot move NV12 frames itself), the
    download adapter format=nv12, and the job delivers NV12 buffers equal to the all-reference job on the split frames,
    merged.  The bitmap is of the frame's size: no chroma block lies half under it, where blend_subsample_8onbi8 and
    _8on8 differ (blend.c:388-390 / :294-296)."""
    import oracle_lib as ol
    F = hbrt.FILTER_ID
    regs = {F["render_sub"]: "hb_filter_render_sub", F["lapsharp"]: "hb_filter_lapsharp"}
    w, h, n = 66, 38, 3
    frames = [bc.frame(bc.NV12, w, h, seed=t) for t in range(n)]
    sub = bc.overlay(0, 0, w, h, False, 77)
    filters = [(F["render_sub"], ""), (F["lapsharp"], LAP + ":cb-strength=0.2:cb-kernel=isolap")]

    def run(frs, pix_fmt, use_hip):
        out = []
        with hbrt.Job(filters, w, h, pix_fmt, use_hip=use_hip) as job:
            names = job.stages()
            job.push_subtitle(sub, 0, -1)
            for i, fr in enumerate(frs):
                job.push(fr, start=i * 3003, stop=(i + 1) * 3003)
                out += job.drain()
            job.push_eof()
            out += job.drain()
        return names, out

    hbrt.register_filters(ol.ref(), regs)
    hbrt.set_job_subtitle("pgs")
    try:
        names, got = run(frames, bc.NV12, True)
        _, want = run([bm.split(f, 8) for f in frames], 0, False)
    finally:
        hbrt.set_job_subtitle(None)
        hbrt.register_filters(ol.ref(), {k: None for k in regs})
    assert names[0] == "Subtitle renderer" and names[1] == "HIP upload adapter" and names[3] == "HIP download adapter"
    assert len(names) == 4 and "HIP" in names[2]
    assert len(got) == len(want) == n
    for t in range(n):
        merged = bm.merge(want[t].planes, 8)
        assert len(got[t].planes) == 2
        for p in range(2):
            np.testing.assert_array_equal(got[t].planes[p], merged[p], err_msg=f"frame {t} plane {p}")


def test_nv12_job_with_a_format_filter_ends_planar(built):
    """hip_common.c:job_host_fmt - a `format` filter in the list says itself what the frames are to become, so the run is
    uploaded as NV12 and leaves planar, as runs always did: [lapsharp, format=yuv420p] on an NV12 job delivers yuv420p
    frames equal to the lapsharp oracle on the split frames.  (The drop-in object stands in for the list entry libhb's
    own `format` would be: the swap leaves an object that already is the drop-in alone.)"""
    import oracle_stream as os_
    import golden_cases as gc
    F = hbrt.FILTER_ID
    flt = hip.filters()
    w, h, n = 66, 38, 3
    frames = [bc.frame(bc.NV12, w, h, seed=t) for t in range(n)]
    hbrt.register_filters(flt, {F["lapsharp"]: "hb_filter_lapsharp_hip", F["format"]: "hb_filter_format_hip"})
    try:
        names, got = hbrt.run_job([(F["lapsharp"], LAP), (F["format"], "format=yuv420p")], frames, pix_fmt=bc.NV12)
    finally:
        hbrt.register_filters(flt, {F["lapsharp"]: None, F["format"]: None})
    assert names[0] == "HIP upload adapter" and names[2] == "Format (HIP)" and names[3] == "HIP download adapter"
    assert len(names) == 4 and "HIP" in names[1]
    want = os_.lapsharp_stream([bm.split(f, 8) for f in frames], [gc.lap(depth=8)] * n)
    assert len(got) == n
    for t in range(n):
        assert len(got[t].planes) == 3
        for p in range(3):
            np.testing.assert_array_equal(got[t].planes[p], want[t][p], err_msg=f"frame {t} plane {p}")
