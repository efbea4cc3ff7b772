"""GPU: the planar ends of a device-resident run, and what the six asynchronous entry points share (hbhip_core.hip:
hbhip_frame_upload_async / _upload_biplanar_async / _import_surface_async, hbhip_frame_download_async /
_download_biplanar_async / _export_surface_async) - which form of copy a host layout gets, what it leaves alone, what the
bus counter says, what a refused call leaves behind - and the hbhip_filter_submit_async pipe against push / pull.
Tolerance 0 throughout."""
import ctypes as C

import numpy as np
import pytest

from handbrake_amd import hip

pytestmark = pytest.mark.gpu
ERR_ARG = -3
SENTINEL, SLACK = 0xA5, 96
# the sizes of test_surface_gpu.py that matter here: the minimum; pitches wider than rows; odd both ways (odd chroma)
SIZES = [(2, 2), (66, 38), (67, 39)]


@pytest.fixture(scope="module")
def ctx():
    c = hip.Ctx(0)
    L = hip.lib()
    L.hbhip_frame_download_async.argtypes = [C.c_void_p, C.POINTER(hip.HostFrame), C.POINTER(C.c_void_p)]
    L.hbhip_filter_submit_async.argtypes = [C.c_void_p, C.POINTER(hip.HostFrame), C.POINTER(hip.HostFrame), C.c_int64]
    L.hbhip_filter_wait.argtypes = [C.c_void_p, C.POINTER(C.c_int64)]
    yield c
    c.close()


def align64(n):
    return -(-n // 64) * 64


class Host:
    """Three host planes in one byte array filled with `fill`.
      own    the frame's layout: strides = the rows rounded up to 64 bytes, the planes back to back, nothing around them
      tight  strides = the rows, SLACK bytes in front of, between and behind the planes"""

    def __init__(self, w, h, depth, layout, fill=0):
        self.bps, self.dtype = (1, np.uint8) if depth == 8 else (2, np.uint16)
        cw, ch = (w + 1) // 2, (h + 1) // 2
        self.dims = [(h, w), (ch, cw), (ch, cw)]
        own = layout == "own"
        self.stride = [align64(pw * self.bps) if own else pw * self.bps for _, pw in self.dims]
        self.offset, at = [], 0
        for (ph, _), s in zip(self.dims, self.stride):
            at += 0 if own else SLACK
            self.offset.append(at)
            at += s * ph
        self.buf = np.full(at + (0 if own else SLACK), fill, dtype=np.uint8)
        self.samples = sum(ph * pw * self.bps for ph, pw in self.dims)

    def rows(self, c):
        """plane c, whole rows, as bytes"""
        ph, s = self.dims[c][0], self.stride[c]
        return self.buf[self.offset[c]:self.offset[c] + s * ph].reshape(ph, s)

    def plane(self, c):
        """the samples of plane c"""
        return self.rows(c)[:, :self.dims[c][1] * self.bps].view(self.dtype)

    def put(self, planes):
        for c in range(3):
            self.plane(c)[:] = planes[c]
        return self

    def outside(self):
        """every byte that is no sample"""
        mask = np.ones(self.buf.size, dtype=bool)
        for c, (ph, pw) in enumerate(self.dims):
            idx = self.offset[c] + np.arange(ph)[:, None] * self.stride[c] + np.arange(pw * self.bps)[None, :]
            mask[idx] = False
        return self.buf[mask]

    def struct(self, null_plane=None, short_stride=None):
        f = hip.HostFrame()
        for c in range(3):
            f.plane[c] = None if c == null_plane else self.rows(c).ctypes.data
            f.stride[c] = self.dims[c][1] * self.bps - 1 if c == short_stride else self.stride[c]
        return f


def picture(w, h, depth, seed):
    rng = np.random.default_rng(seed)
    dt = np.uint8 if depth == 8 else np.uint16
    ch, cw = (h + 1) // 2, (w + 1) // 2
    return [rng.integers(0, 1 << depth, s).astype(dt) for s in ((h, w), (ch, cw), (ch, cw))]


def upload(ctx, fr, host, blocking):
    L, f = hip.lib(), host.struct()
    if blocking:
        hip.check(L.hbhip_frame_upload(fr.h, C.byref(f)), ctx.h, "upload")
        return
    t = C.c_void_p()
    hip.check(L.hbhip_frame_upload_async(fr.h, C.byref(f), C.byref(t)), ctx.h, "upload async")
    assert t.value
    assert L.hbhip_ctx_upload_done(ctx.h, t, 1) == 0


def download(ctx, fr, host, blocking):
    L, f = hip.lib(), host.struct()
    if blocking:
        hip.check(L.hbhip_frame_download(fr.h, C.byref(f)), ctx.h, "download")
        return
    t = C.c_void_p()
    hip.check(L.hbhip_frame_download_async(fr.h, C.byref(f), C.byref(t)), ctx.h, "download async")
    assert t.value
    assert L.hbhip_frame_download_wait(fr.h, t) == 0


# ---- which copy a host layout gets ------------------------------------------------------------------------------------
@pytest.mark.parametrize("blocking", [False, True], ids=["async", "blocking"])
@pytest.mark.parametrize("depth", [8, 10])
@pytest.mark.parametrize("w,h", SIZES)
def test_the_frames_own_layout_moves_as_one_block(built, ctx, w, h, depth, blocking):
    """both ways: the counter grows by the block, and the row padding travels - up into the frame, down into a zeroed
    buffer of the same layout"""
    x = picture(w, h, depth, seed=100 * w + depth)
    src = Host(w, h, depth, "own")
    src.buf[:] = np.random.default_rng(7).integers(1, 256, src.buf.size, dtype=np.uint8)      # a pattern in the padding
    src.put(x)
    fr = hip.Frame(ctx, w, h, depth)
    try:
        b0 = ctx.bus_bytes()
        upload(ctx, fr, src, blocking)
        b1 = ctx.bus_bytes()
        assert (b1[0] - b0[0], b1[1] - b0[1]) == (src.buf.size, 0)
        dst = Host(w, h, depth, "own")
        download(ctx, fr, dst, blocking)
        b2 = ctx.bus_bytes()
        assert (b2[0] - b1[0], b2[1] - b1[1]) == (0, dst.buf.size)
        np.testing.assert_array_equal(dst.buf, src.buf)
    finally:
        fr.close()


@pytest.mark.parametrize("blocking", [False, True], ids=["async", "blocking"])
@pytest.mark.parametrize("depth", [8, 10])
@pytest.mark.parametrize("w,h", SIZES)
def test_tight_planes_move_plane_by_plane(built, ctx, w, h, depth, blocking):
    """the counter grows by the samples; up, the frame's row padding stays what it was; down, the host's bytes beyond the
    samples do"""
    x = picture(w, h, depth, seed=200 * w + depth)
    fr = hip.Frame(ctx, w, h, depth)
    try:
        stale = Host(w, h, depth, "own", fill=0xFF)
        upload(ctx, fr, stale, True)
        src = Host(w, h, depth, "tight", fill=SENTINEL).put(x)
        b0 = ctx.bus_bytes()
        upload(ctx, fr, src, blocking)
        b1 = ctx.bus_bytes()
        assert (b1[0] - b0[0], b1[1] - b0[1]) == (src.samples, 0)
        dst = Host(w, h, depth, "tight", fill=SENTINEL)
        download(ctx, fr, dst, blocking)
        b2 = ctx.bus_bytes()
        assert (b2[0] - b1[0], b2[1] - b1[1]) == (0, dst.samples)
        for c in range(3):
            np.testing.assert_array_equal(dst.plane(c), x[c], err_msg=f"plane {c}")
        assert (dst.outside() == SENTINEL).all(), "a download into tight planes wrote beyond the samples"
        whole = Host(w, h, depth, "own")
        download(ctx, fr, whole, True)
        for c in range(3):
            np.testing.assert_array_equal(whole.plane(c), x[c], err_msg=f"plane {c}, whole rows")
        assert (whole.outside() == 0xFF).all(), "an upload from tight planes wrote the frame's row padding"
    finally:
        fr.close()


# ---- order --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("layout", ["own", "tight"])
@pytest.mark.parametrize("depth", [8, 10])
def test_eight_planar_in_flight_keep_their_order(built, ctx, depth, layout):
    """the planar twin of test_biplanar_gpu.py::test_eight_in_flight_keep_their_order"""
    L = hip.lib()
    w, h, n = 67, 39, 8
    pics = [picture(w, h, depth, seed=k) for k in range(n)]
    frames = [hip.Frame(ctx, w, h, depth) for _ in range(n)]
    try:
        srcs, tokens = [], []
        for k in range(n):
            s = Host(w, h, depth, layout).put(pics[k])
            srcs.append((s, s.struct()))
            t = C.c_void_p()
            hip.check(L.hbhip_frame_upload_async(frames[k].h, C.byref(srcs[k][1]), C.byref(t)), ctx.h, "upload async")
            tokens.append(t)
        for t in tokens:
            assert L.hbhip_ctx_upload_done(ctx.h, t, 1) == 0
        dsts, tokens = [], []
        for k in range(n):
            d = Host(w, h, depth, layout, fill=SENTINEL)
            dsts.append((d, d.struct()))
            t = C.c_void_p()
            hip.check(L.hbhip_frame_download_async(frames[k].h, C.byref(dsts[k][1]), C.byref(t)), ctx.h, "download async")
            tokens.append(t)
        for k in range(n):
            assert L.hbhip_frame_download_wait(frames[k].h, tokens[k]) == 0
        for k in range(n):
            for c in range(3):
                np.testing.assert_array_equal(dsts[k][0].plane(c), pics[k][c], err_msg=f"picture {k} plane {c}")
    finally:
        for fr in frames:
            fr.close()


# ---- refusals ---------------------------------------------------------------------------------------------------------
def biplanar_of(x, depth):
    """the NV12 / P010LE host picture of planar `x`: (arrays, hbhip_host_biplanar)"""
    sh = 6 if depth == 10 else 0
    uv = np.empty((x[1].shape[0], 2 * x[1].shape[1]), dtype=x[1].dtype)
    uv[:, 0::2], uv[:, 1::2] = x[1] << sh, x[2] << sh
    return [np.ascontiguousarray(x[0] << sh), uv]


def bi_struct(arrays, null_plane=None, short_stride=None):
    hb = hip.HostBiplanar()
    for p, a in enumerate(arrays):
        hb.plane[p] = None if p == null_plane else a.ctypes.data
        hb.stride[p] = a.strides[0] - 1 if p == short_stride else a.strides[0]
    return hb


@pytest.mark.parametrize("depth", [8, 10])
def test_a_refused_call_leaves_nothing_behind(built, ctx, depth):
    """every asynchronous end with a null plane and with a stride below the row (the surface ends: with no surface - a
    surface's planes and pitches are refused when it is wrapped, test_surface_gpu.py): HBHIP_ERR_ARG, no token, nothing
    counted, and the same frame takes the correct call straight afterwards"""
    L = hip.lib()
    w, h = 66, 38
    x, y = picture(w, h, depth, seed=31), picture(w, h, depth, seed=32)
    fr, other = hip.Frame(ctx, w, h, depth), hip.Frame(ctx, w, h, depth)
    surface = hip.Surface(ctx, w, h, depth)
    tok = C.c_void_p()

    def refused(call, structs):
        before = ctx.bus_bytes()
        for s in structs:
            none = C.c_void_p()
            assert call(fr.h, C.byref(s) if s is not None else None, C.byref(none)) == ERR_ARG
            assert not none.value
        assert ctx.bus_bytes() == before

    def same(got, want, what):
        for c in range(3):
            np.testing.assert_array_equal(got[c], want[c], err_msg=f"{what}, plane {c}")

    try:
        host = Host(w, h, depth, "tight").put(x)
        bad = [host.struct(null_plane=c) for c in range(3)] + [host.struct(short_stride=c) for c in range(3)]
        # planar upload
        refused(L.hbhip_frame_upload_async, bad)
        hip.check(L.hbhip_frame_upload_async(fr.h, C.byref(host.struct()), C.byref(tok)), ctx.h, "upload async")
        assert L.hbhip_ctx_upload_done(ctx.h, tok, 1) == 0
        same(fr.download(), x, "upload")
        # planar download
        out = Host(w, h, depth, "tight", fill=SENTINEL)
        refused(L.hbhip_frame_download_async, [out.struct(null_plane=c) for c in range(3)] +
                [out.struct(short_stride=c) for c in range(3)])
        assert (out.buf == SENTINEL).all()
        hip.check(L.hbhip_frame_download_async(fr.h, C.byref(out.struct()), C.byref(tok)), ctx.h, "download async")
        assert L.hbhip_frame_download_wait(fr.h, tok) == 0
        same([out.plane(c) for c in range(3)], x, "download")
        # NV12 / P010LE upload
        bi = biplanar_of(y, depth)
        refused(L.hbhip_frame_upload_biplanar_async, [bi_struct(bi, null_plane=p) for p in range(2)] +
                [bi_struct(bi, short_stride=p) for p in range(2)])
        hip.check(L.hbhip_frame_upload_biplanar_async(fr.h, C.byref(bi_struct(bi)), C.byref(tok)), ctx.h, "upload biplanar async")
        assert L.hbhip_ctx_upload_done(ctx.h, tok, 1) == 0
        same(fr.download(), y, "upload biplanar")
        # NV12 / P010LE download
        back = [np.full_like(a, SENTINEL) for a in bi]
        refused(L.hbhip_frame_download_biplanar_async, [bi_struct(back, null_plane=p) for p in range(2)] +
                [bi_struct(back, short_stride=p) for p in range(2)])
        hip.check(L.hbhip_frame_download_biplanar_async(fr.h, C.byref(bi_struct(back)), C.byref(tok)), ctx.h, "download biplanar async")
        assert L.hbhip_frame_download_wait(fr.h, tok) == 0
        for p in range(2):
            np.testing.assert_array_equal(back[p], bi[p], err_msg=f"download biplanar, plane {p}")
        # export: fr holds y; what the surface then holds comes back through an import into another frame
        refused(L.hbhip_frame_export_surface_async, [None])
        hip.check(L.hbhip_frame_export_surface_async(fr.h, surface.h, C.byref(tok)), ctx.h, "export async")
        assert L.hbhip_frame_download_wait(fr.h, tok) == 0
        other.import_surface(surface)
        same(other.download(), y, "export")
        # import: the surface takes x from the other frame, fr takes it from the surface
        other.upload(x)
        other.export_surface(surface)
        refused(L.hbhip_frame_import_surface_async, [None])
        hip.check(L.hbhip_frame_import_surface_async(fr.h, surface.h, C.byref(tok)), ctx.h, "import async")
        assert L.hbhip_ctx_upload_done(ctx.h, tok, 1) == 0
        same(fr.download(), x, "import")
    finally:
        surface.close()
        other.close()
        fr.close()


# ---- the pipelined host path --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("depth", [8, 10])
def test_submit_and_wait_with_two_in_flight_is_push_and_pull(built, ctx, depth):
    L = hip.lib()
    w, h, n = 66, 38, 5
    pics = [picture(w, h, depth, seed=40 + k) for k in range(n)]
    ref = hip.lapsharp_device_filter(ctx, w, h, 0.2, 1, depth)
    flt = hip.lapsharp_device_filter(ctx, w, h, 0.2, 1, depth)
    fr = hip.Frame(ctx, w, h, depth)
    try:
        want = []
        for k in range(n):
            out, tag = fr.planes(), C.c_int64()
            hip.check(L.hbhip_filter_push(ref.h, C.byref(hip.host_frame(pics[k])), k), ctx.h, "push")
            hip.check(L.hbhip_filter_pull(ref.h, C.byref(hip.host_frame(out)), C.byref(tag)), ctx.h, "pull")
            assert tag.value == k
            want.append(out)
        assert any((want[0][0] != pics[0][0]).ravel())                   # the filter did something
        got = [fr.planes() for _ in range(n)]
        structs = [(hip.host_frame(pics[k]), hip.host_frame(got[k])) for k in range(n)]
        waited = []

        def wait():
            tag = C.c_int64()
            hip.check(L.hbhip_filter_wait(flt.h, C.byref(tag)), ctx.h, "wait")
            waited.append(tag.value)

        for k in range(n):
            if L.hbhip_filter_inflight(flt.h) == 2:
                wait()
            hip.check(L.hbhip_filter_submit_async(flt.h, C.byref(structs[k][0]), C.byref(structs[k][1]), k), ctx.h, "submit")
        assert L.hbhip_filter_inflight(flt.h) == 2
        wait()
        wait()
        assert waited == list(range(n)) and L.hbhip_filter_wait(flt.h, None) == 1      # HBHIP_AGAIN: none in flight
        for k in range(n):
            for c in range(3):
                np.testing.assert_array_equal(got[k][c], want[k][c], err_msg=f"picture {k} plane {c}")
    finally:
        fr.close()
        flt.close()
        ref.close()
