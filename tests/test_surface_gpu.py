"""GPU: device surfaces - NV12 / P010LE pictures in HBM imported into and exported from planar frames without a host copy
(bi_surface_split_kernel / bi_surface_merge_kernel, csrc/biplanar.hip), through the C ABI and through the adapters, against
tests/surface_model.py.  Tolerance 0 throughout."""
import ctypes as C

import numpy as np
import pytest

from handbrake_amd import hbrt, hip
import biplanar_cases as bc
import surface_model as sm

pytestmark = pytest.mark.gpu
ERR_ARG, ERR_UNSUPPORTED = -3, -5
SENTINEL, GUARD = 0xA5, 4096
# 2x2 the minimum; 18x10 rows that are no multiple of 16 bytes; 33x7 odd both ways (a 34-byte interleaved row, 4 chroma rows);
# 66x38 the frame's 128-byte pitch against a tight 80-byte surface pitch and against 256; 130x6; 1922x1082 more than one
# workgroup a row, a multi-row grid
SIZES = [(2, 2), (18, 10), (33, 7), (66, 38), (130, 6), (1922, 1082)]
KINDS = ["tight", "hw", "two"]
LAP = "y-strength=0.2:y-kernel=isolap"


@pytest.fixture(scope="module")
def ctx():
    c = hip.Ctx(0)
    yield c
    c.close()


class Mem:
    """A surface and the device memory under it, mirrored on the host as ONE byte array (two allocations: end to end).
      tight  pitch = align16(row bytes), UV right behind luma, inside a larger allocation: 4 KiB in front and behind
      hw     256-byte pitch, 16 padded rows, from hbhip_surface_alloc (the memory is the library's: no bands around it)
      two    two hbhip_dev_alloc allocations, a different pitch each, 4 KiB in front of and behind either plane"""

    def __init__(self, ctx, kind, w, h, depth, release=None):
        L = hip.lib()
        self.ctx, self.kind, self.allocs = ctx, kind, []
        bps = 2 if depth > 8 else 1
        cw, ch = (w + 1) // 2, (h + 1) // 2
        if kind == "hw":
            self.surface = hip.Surface(ctx, w, h, depth, 256, 16)
            self.lay = sm.pooled(w, h, depth, 256, 16)
            planes, pitches, *_ = self.surface.describe()
            assert pitches == self.lay.pitch and planes[1] - planes[0] == self.lay.offset[1] and planes[0] % 256 == 0
            self.parts = [(planes[0], self.lay.size)]
            return
        if kind == "tight":
            self.lay = sm.pooled(w, h, depth, 16, 1, lead=GUARD, tail=GUARD)
            sizes = [self.lay.size]
        else:
            pitch = (sm.align(w * bps, 64) + 64, sm.align(2 * cw * bps, 16) + 16)
            size0 = GUARD + pitch[0] * h + GUARD
            self.lay = sm.Layout(w, h, depth, pitch, (GUARD, size0 + GUARD), (h, ch), size0 + GUARD + pitch[1] * ch + GUARD)
            sizes = [size0, self.lay.size - size0]
        self.parts = []
        for n in sizes:
            p = C.c_void_p()
            hip.check(L.hbhip_dev_alloc(ctx.h, n, C.byref(p)), ctx.h, "dev_alloc")
            self.allocs.append(p)
            self.parts.append((p.value, n))
        base = [self.parts[0][0], self.parts[-1][0] - (self.lay.size - self.parts[-1][1])]     # of the array's byte 0, per plane
        self.surface = hip.Surface.wrap(ctx, [base[p] + self.lay.offset[p] for p in range(2)], self.lay.pitch, w, h, depth,
                                        release=release)

    def upload(self, buf):
        at = 0
        for ptr, n in self.parts:
            part = np.ascontiguousarray(buf[at:at + n])
            hip.check(hip.lib().hbhip_dev_upload(self.ctx.h, ptr, part.ctypes.data, n), self.ctx.h, "dev_upload")
            at += n

    def download(self):
        buf = np.empty(self.lay.size, dtype=np.uint8)
        at = 0
        for ptr, n in self.parts:
            hip.check(hip.lib().hbhip_dev_download(self.ctx.h, buf[at:at + n].ctypes.data, ptr, n), self.ctx.h, "dev_download")
            at += n
        return buf

    def close(self):
        self.surface.close()
        for p in self.allocs:
            hip.lib().hbhip_dev_free(self.ctx.h, p)
        self.allocs = []


class Rows:
    """Host planes in the frame's own layout (its pitches, the planes back to back): uploads and downloads then move whole
    rows in one copy, so the frame's row padding can be set and seen."""

    def __init__(self, fr):
        d = hip.DevFrame()
        hip.check(hip.lib().hbhip_frame_describe(fr.h, C.byref(d), None, None), what="frame_describe")
        w, h, depth, lcw, lch = fr.shape
        self.dtype = np.uint8 if depth == 8 else np.uint16
        self.pitch = list(d.stride)
        self.rows = [h, -(-h >> lch), -(-h >> lch)]
        self.buf = np.zeros(sum(p * r for p, r in zip(self.pitch, self.rows)), dtype=np.uint8)

    def plane(self, c):
        at = sum(p * r for p, r in zip(self.pitch[:c], self.rows[:c]))
        return self.buf[at:at + self.pitch[c] * self.rows[c]].reshape(self.rows[c], self.pitch[c]).view(self.dtype)

    def struct(self):
        f = hip.HostFrame()
        for c in range(3):
            f.plane[c] = self.plane(c).ctypes.data
            f.stride[c] = self.pitch[c]
        return f

    def upload(self, fr):
        hip.check(hip.lib().hbhip_frame_upload(fr.h, C.byref(self.struct())), fr.ctx.h, "frame_upload")

    def download(self, fr):
        hip.check(hip.lib().hbhip_frame_download(fr.h, C.byref(self.struct())), fr.ctx.h, "frame_download")
        return self


def planar(rng, w, h, depth):
    dt = np.uint8 if depth == 8 else np.uint16
    ch, cw = (h + 1) // 2, (w + 1) // 2
    return tuple(rng.integers(0, 1 << depth, s).astype(dt) for s in ((h, w), (ch, cw), (ch, cw)))


def pad_to(a, n):
    """the first n columns of `a`, zeros where it has fewer"""
    out = np.zeros((a.shape[0], n), dtype=a.dtype)
    k = min(n, a.shape[1])
    out[:, :k] = a[:, :k]
    return out


# ---- import -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("depth", [8, 10])
@pytest.mark.parametrize("w,h", SIZES)
def test_import_is_the_split_and_fills_every_row_of_the_frame(built, ctx, w, h, depth, kind):
    """random bytes everywhere - padding, padded rows, guard bands, P010 low bits: the samples are the model's, and every
    frame row is written up to the frame's pitch, from the surface's row as far as ITS pitch reaches and zero beyond"""
    rng = np.random.default_rng(1000 * w + 10 * h + depth)
    mem = Mem(ctx, kind, w, h, depth)
    fr = hip.Frame(ctx, w, h, depth)
    try:
        buf = rng.integers(0, 256, mem.lay.size, dtype=np.uint8)
        mem.upload(buf)
        stale = Rows(fr)
        stale.buf[:] = 0xFF                                             # a recycled frame: stale bytes in samples and padding
        stale.upload(fr)
        fr.import_surface(mem.surface)
        for got, want in zip(fr.download(), sm.split(buf, mem.lay)):
            np.testing.assert_array_equal(got, want)
        rows = Rows(fr).download(fr)
        whole = sm.split(buf, mem.lay, whole_pitch=True)                # the surface's rows as wide as their pitch
        for c in range(3):
            got = rows.plane(c)
            np.testing.assert_array_equal(got, pad_to(whole[c], got.shape[1]), err_msg=f"plane {c}, whole rows")
    finally:
        fr.close()
        mem.close()


def pull_host(flt, fr, tag=0):
    L = hip.lib()
    L.hbhip_filter_push_frame.argtypes = [C.c_void_p, C.c_void_p, C.c_int64]
    hip.check(L.hbhip_filter_push_frame(flt.h, fr.h, tag), flt.ctx.h, "push_frame")
    out = fr.planes()
    hip.check(L.hbhip_filter_pull(flt.h, C.byref(hip.host_frame(out)), None), flt.ctx.h, "pull")
    return out


@pytest.mark.parametrize("pix_fmt", [bc.NV12, bc.P010LE])
def test_imported_row_padding_is_what_the_staging_split_hands_on(built, ctx, pix_fmt):
    """lapsharp reads row padding: the same picture through hbhip_frame_upload_biplanar (zeroed host padding) and through a
    surface with zeroed padding gives the same output"""
    w, h, depth = 66, 38, bc.DEPTH[pix_fmt]
    pic = bc.frame(pix_fmt, w, h, seed=3)
    L = hip.lib()
    flt = hip.lapsharp_device_filter(ctx, w, h, 0.2, 1, depth)
    outs = []
    try:
        for kind in ("host", "tight", "hw"):
            fr = hip.Frame(ctx, w, h, depth)
            stale = Rows(fr)
            stale.buf[:] = 0xFF
            stale.upload(fr)
            if kind == "host":
                stride = [sm.align(a.shape[1] * a.itemsize, 64) for a in pic]
                host = [np.zeros((a.shape[0], s), dtype=np.uint8) for a, s in zip(pic, stride)]
                for a, hp in zip(pic, host):
                    hp[:, :a.shape[1] * a.itemsize] = a.view(np.uint8)
                hb = hip.HostBiplanar((C.c_void_p * 2)(*[hp.ctypes.data for hp in host]), (C.c_int * 2)(*stride))
                hip.check(L.hbhip_frame_upload_biplanar(fr.h, C.byref(hb)), ctx.h, "upload_biplanar")
            else:
                mem = Mem(ctx, kind, w, h, depth)
                buf = np.zeros(mem.lay.size, dtype=np.uint8)
                for p in range(2):
                    raw = pic[p].view(np.uint8)
                    idx = mem.lay.offset[p] + np.arange(raw.shape[0])[:, None] * mem.lay.pitch[p] + np.arange(raw.shape[1])[None, :]
                    buf[idx] = raw
                mem.upload(buf)
                fr.import_surface(mem.surface)
                mem.close()
            outs.append(pull_host(flt, fr))
            fr.close()
    finally:
        flt.close()
    assert any((outs[0][0] != (pic[0] >> (6 if depth == 10 else 0))).ravel())        # the filter did something
    for other in outs[1:]:
        for c in range(3):
            np.testing.assert_array_equal(other[c], outs[0][c], err_msg=f"plane {c}")


# ---- export -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("depth", [8, 10])
@pytest.mark.parametrize("w,h", SIZES)
def test_export_is_the_merge_and_writes_nothing_else(built, ctx, w, h, depth, kind):
    """guard bands, row padding, padded rows and the gap between the planes hold 0xA5 before and after; the samples are the
    model's; the frame's row padding is all ones, and still no low bit of a P010 sample written is set"""
    rng = np.random.default_rng(2000 * w + 10 * h + depth)
    mem = Mem(ctx, kind, w, h, depth)
    fr = hip.Frame(ctx, w, h, depth)
    try:
        lay = mem.lay
        mem.upload(np.full(lay.size, SENTINEL, dtype=np.uint8))
        x = planar(rng, w, h, depth)
        rows = Rows(fr)
        rows.buf[:] = 0xFF
        for c in range(3):
            rows.plane(c)[:, :x[c].shape[1]] = x[c]
        rows.upload(fr)
        fr.export_surface(mem.surface)
        got = mem.download()
        want = sm.merge(np.full(lay.size, SENTINEL, dtype=np.uint8), lay, x)
        for p in range(2):
            np.testing.assert_array_equal(sm.plane_rows(got, lay, p), sm.plane_rows(want, lay, p), err_msg=f"plane {p}")
        written = lay.written()
        assert (got[~written] == SENTINEL).all(), "bytes outside [0, align16(row bytes)) of the sample rows were written"
        if depth == 10:
            assert (got[written].view(np.uint16) & 63 == 0).all()
    finally:
        fr.close()
        mem.close()


# ---- order --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("pix_fmt", [bc.NV12, bc.P010LE])
def test_eight_in_flight_keep_their_order_and_their_surfaces(built, ctx, pix_fmt):
    L = hip.lib()
    L.hbhip_filter_push_frame.argtypes = [C.c_void_p, C.c_void_p, C.c_int64]
    L.hbhip_filter_pull_frame.argtypes = [C.c_void_p, C.POINTER(C.c_void_p), C.POINTER(C.c_int64)]
    w, h, n, depth = 66, 38, 8, bc.DEPTH[pix_fmt]
    pics = [bc.frame(pix_fmt, w, h, seed=k) for k in range(n)]
    flt = hip.lapsharp_device_filter(ctx, w, h, 0.2, 1, depth)
    hip.check(L.hbhip_filter_use_frames(flt.h), ctx.h, "use_frames")           # frames in, frames out, nothing copied
    ref = hip.lapsharp_device_filter(ctx, w, h, 0.2, 1, depth)
    # the host path's result for picture k: upload_biplanar, lapsharp, download
    want = []
    for k in range(n):
        fr = hip.Frame(ctx, w, h, depth)
        stride = [sm.align(a.shape[1] * a.itemsize, 64) for a in pics[k]]
        host = [np.zeros((a.shape[0], s), dtype=np.uint8) for a, s in zip(pics[k], stride)]
        for a, hp in zip(pics[k], host):
            hp[:, :a.shape[1] * a.itemsize] = a.view(np.uint8)
        hb = hip.HostBiplanar((C.c_void_p * 2)(*[hp.ctypes.data for hp in host]), (C.c_int * 2)(*stride))
        hip.check(L.hbhip_frame_upload_biplanar(fr.h, C.byref(hb)), ctx.h, "upload_biplanar")
        want.append(pull_host(ref, fr))
        fr.close()
    ref.close()
    assert any((want[0][0] != (pics[0][0] >> (6 if depth == 10 else 0))).ravel())

    called = [0] * n
    callbacks = [hip.SURFACE_RELEASE(lambda _, k=k: called.__setitem__(k, called[k] + 1)) for k in range(n)]
    ins = [Mem(ctx, "tight", w, h, depth, release=callbacks[k]) for k in range(n)]
    outs = [Mem(ctx, "hw", w, h, depth) for _ in range(n)]
    frames = [hip.Frame(ctx, w, h, depth) for _ in range(n)]
    again = [hip.Frame(ctx, w, h, depth) for _ in range(n)]
    made = []
    try:
        for k in range(n):
            buf = np.zeros(ins[k].lay.size, dtype=np.uint8)
            for p in range(2):
                raw = pics[k][p].view(np.uint8)
                lay = ins[k].lay
                buf[lay.offset[p] + np.arange(raw.shape[0])[:, None] * lay.pitch[p] + np.arange(raw.shape[1])[None, :]] = raw
            ins[k].upload(buf)
        tokens = []
        for k in range(n):                                              # eight imports, nothing waited for
            t = C.c_void_p()
            hip.check(L.hbhip_frame_import_surface_async(frames[k].h, ins[k].surface.h, C.byref(t)), ctx.h, "import async")
            tokens.append(t)
        for k in range(n):
            ins[k].surface.close()                                      # the last reference of the caller's: the library still holds its own
        for k in range(n):                                              # each through lapsharp, each exported, each imported again
            hip.check(L.hbhip_filter_push_frame(flt.h, frames[k].h, k), ctx.h, "push_frame")
            o, tag = C.c_void_p(), C.c_int64()
            assert L.hbhip_filter_pull_frame(flt.h, C.byref(o), C.byref(tag)) == 0 and tag.value == k
            made.append(o)
            t = C.c_void_p()
            hip.check(L.hbhip_frame_export_surface_async(o, outs[k].surface.h, C.byref(t)), ctx.h, "export async")
            tokens.append(t)
        for k in range(n):                                              # no host wait between the export and this import
            t = C.c_void_p()
            hip.check(L.hbhip_frame_import_surface_async(again[k].h, outs[k].surface.h, C.byref(t)), ctx.h, "import again")
            tokens.append(t)
        for k in range(n):
            # release(opaque) only once the split has read the memory: a callback that has run means a token that is done
            if called[k]:
                assert L.hbhip_ctx_upload_done(ctx.h, tokens[k], 0) == 0
            else:
                assert L.hbhip_ctx_upload_done(ctx.h, tokens[k], 1) == 0
        for k in range(n):
            assert L.hbhip_frame_download_wait(made[k], tokens[n + k]) == 0
        for k in range(n):
            assert L.hbhip_ctx_upload_done(ctx.h, tokens[2 * n + k], 1) == 0
        ctx.sync()
        assert called == [1] * n
        for k in range(n):
            got = sm.split(outs[k].download(), outs[k].lay)
            back = again[k].download()
            for c in range(3):
                np.testing.assert_array_equal(got[c], want[k][c], err_msg=f"picture {k} plane {c}")
                np.testing.assert_array_equal(back[c], want[k][c], err_msg=f"picture {k} plane {c}, imported again")
    finally:
        ctx.sync()                                                      # (a failure above: nothing queued may outlive the memory)
        for o in made:
            L.hbhip_frame_release(o)
        for f in frames + again:
            f.close()
        flt.close()
        for m in ins + outs:
            m.close()
    ctx.sync()
    assert called == [1] * n


# ---- refusals ---------------------------------------------------------------------------------------------------------
def test_what_is_refused_before_anything_is_queued(built, ctx):
    L = hip.lib()
    w, h = 18, 10
    block = C.c_void_p()
    hip.check(L.hbhip_dev_alloc(ctx.h, 1 << 16, C.byref(block)), ctx.h, "dev_alloc")
    out = C.c_void_p()

    def wrap(planes, pitches, w=w, h=h, depth=8):
        mem = hip.DevSurface((C.c_void_p * 2)(*planes), (C.c_int * 2)(*pitches))
        rc = L.hbhip_surface_wrap(ctx.h, C.byref(mem), w, h, depth, None, None, C.byref(out))
        assert (rc == 0) == bool(out.value)
        return rc

    b = block.value
    try:
        assert wrap([b, b + 4096], [24, 32]) == ERR_UNSUPPORTED             # a pitch that is no multiple of 16 (it holds the 18-byte row)
        assert wrap([b, b + 4096], [32, 40]) == ERR_UNSUPPORTED
        assert wrap([b + 8, b + 4096], [32, 32]) == ERR_UNSUPPORTED         # a base that is no multiple of 16
        assert wrap([b, b + 4096 + 8], [32, 32]) == ERR_UNSUPPORTED
        assert wrap([b, b + 4096], [16, 32]) == ERR_ARG                     # a pitch below the row bytes
        assert wrap([b, b + 4096], [32, 16]) == ERR_ARG
        assert wrap([b, b + 32 * 9], [32, 32]) == ERR_ARG                   # plane 1 starts inside plane 0's last row
        assert wrap([b, b + 4096], [32, 32], w=1) == ERR_UNSUPPORTED        # width 1
        assert wrap([b, b + 4096], [32, 32], h=1) == ERR_UNSUPPORTED
        assert wrap([b, b + 4096], [64, 64], depth=12) == ERR_UNSUPPORTED
        assert L.hbhip_surface_alloc(ctx.h, 1, h, 8, 256, 16, C.byref(out)) == ERR_UNSUPPORTED
        assert L.hbhip_surface_alloc(ctx.h, w, h, 12, 256, 16, C.byref(out)) == ERR_UNSUPPORTED
        assert L.hbhip_surface_alloc(ctx.h, w, h, 8, 24, 16, C.byref(out)) == ERR_ARG
        assert wrap([b, b + 4096], [32, 32]) == 0
        s8 = hip.Surface.adopt(C.c_void_p(out.value))
        assert wrap([b + 8192, b + 12288], [64, 64], depth=10) == 0
        s10 = hip.Surface.adopt(C.c_void_p(out.value))
        tok = C.c_void_p()
        before = ctx.bus_bytes()
        for fw, fh, depth, lcw, lch, s, want in ((w, h, 8, 1, 0, s8, ERR_UNSUPPORTED),       # a 4:2:2 frame
                                                 (w, h, 12, 1, 1, s10, ERR_UNSUPPORTED),     # a depth-12 frame
                                                 (w, h, 10, 1, 1, s8, ERR_UNSUPPORTED),      # depth of the frame against the surface's
                                                 (w, h, 8, 1, 1, s10, ERR_UNSUPPORTED),
                                                 (w + 2, h, 8, 1, 1, s8, ERR_UNSUPPORTED),   # another size
                                                 (1, h, 8, 1, 1, s8, ERR_UNSUPPORTED)):      # width 1
            fr = hip.Frame(ctx, fw, fh, depth, lcw, lch)
            assert L.hbhip_frame_import_surface(fr.h, s.h) == want
            assert L.hbhip_frame_export_surface(fr.h, s.h) == want
            assert L.hbhip_frame_import_surface_async(fr.h, s.h, C.byref(tok)) == want and not tok.value
            assert L.hbhip_frame_export_surface_async(fr.h, s.h, C.byref(tok)) == want and not tok.value
            fr.close()
        assert ctx.bus_bytes() == before
        s8.close()
        s10.close()
    finally:
        L.hbhip_dev_free(ctx.h, block)


def test_pooled_surfaces_are_recycled_and_laid_out_as_asked(built, ctx):
    a = hip.Surface(ctx, 66, 38, 10, 16, 1)
    planes, pitches, w, h, depth = a.describe()
    lay = sm.pooled(66, 38, 10, 16, 1)
    assert (pitches, planes[1] - planes[0], w, h, depth) == (lay.pitch, lay.offset[1], 66, 38, 10)
    a.close()
    b = hip.Surface(ctx, 66, 38, 10, 16, 1)
    assert b.describe()[0] == planes                                    # the same memory again
    c = hip.Surface(ctx, 66, 38, 10, 256, 16)
    assert c.describe()[1] == (256, 256) and c.describe()[0][1] - c.describe()[0][0] == 256 * 48
    b.close()
    c.close()


def test_bus_bytes_count_the_host_copies_only(built, ctx):
    w, h = 66, 38
    fr = hip.Frame(ctx, w, h, 8)
    s = hip.Surface(ctx, w, h, 8)
    try:
        x = planar(np.random.default_rng(5), w, h, 8)
        b0 = ctx.bus_bytes()
        fr.upload(x)
        b1 = ctx.bus_bytes()
        assert b1[0] - b0[0] == sum(a.size for a in x) and b1[1] == b0[1]       # tight host planes: the samples
        fr.export_surface(s)
        fr.import_surface(s)
        assert ctx.bus_bytes() == b1
        got = fr.download()
        b2 = ctx.bus_bytes()
        assert b2[1] - b1[1] == sum(a.size for a in x) and b2[0] == b1[0]
        for c in range(3):
            np.testing.assert_array_equal(got[c], x[c])
    finally:
        s.close()
        fr.close()


# ---- plugin surface -----------------------------------------------------------------------------------------------------
def plugin_ctx():
    c = hip.Ctx.__new__(hip.Ctx)                # the adapters' context (hbhip_registry.c): lives as long as the process
    c.h = C.c_void_p(hip.filters().hbhip_host_ctx_ptr())
    return c


def fill(pctx, surface, pic):
    planes, pitches, w, h, depth = surface.describe()
    lay = sm.pooled(w, h, depth, 256, 16)
    assert pitches == lay.pitch and planes[1] - planes[0] == lay.offset[1]
    buf = np.zeros(lay.size, dtype=np.uint8)
    for p in range(2):
        raw = pic[p].view(np.uint8)
        buf[lay.offset[p] + np.arange(raw.shape[0])[:, None] * lay.pitch[p] + np.arange(raw.shape[1])[None, :]] = raw
    hip.check(hip.lib().hbhip_dev_upload(pctx.h, planes[0], buf.ctypes.data, buf.size), pctx.h, "dev_upload")


def read(pctx, surface):
    planes, pitches, w, h, depth = surface.describe()
    lay = sm.pooled(w, h, depth, 256, 16)
    assert pitches == lay.pitch and planes[1] - planes[0] == lay.offset[1]
    buf = np.empty(lay.size, dtype=np.uint8)
    hip.check(hip.lib().hbhip_dev_download(pctx.h, buf.ctypes.data, planes[0], buf.size), pctx.h, "dev_download")
    return tuple(sm.plane_rows(buf, lay, p) for p in range(2))


def surface_list(name):
    return [("hb_filter_hip_upload", ""), ("hb_filter_lapsharp_hip", LAP), ("hb_filter_vfr_standin", "mode=0:rate=30000/1001"),
            ("hb_filter_hip_download", f"format={name}:surface=1")]


@pytest.mark.parametrize("pix_fmt,name", [(bc.NV12, "nv12"), (bc.P010LE, "p010le")])
def test_a_run_starts_and_ends_on_surfaces(built, pix_fmt, name):
    w, h, n, depth = 66, 38, 9, bc.DEPTH[pix_fmt]
    pctx = plugin_ctx()
    frames = [bc.frame(pix_fmt, w, h, seed=t) for t in range(n)]
    host_list = surface_list(name)[:3] + [("hb_filter_hip_download", f"format={name}")]
    hip.filters()
    b0 = None
    with hbrt.Chain(hip.filters(), host_list, w, h, pix_fmt) as ch:       # (opened first: the context exists from here on)
        b0 = pctx.bus_bytes()
        want = []
        for t, fr in enumerate(frames):
            ch.push(fr, start=t * 3003, stop=(t + 1) * 3003)
            want += ch.drain()
        ch.push_eof()
        want += ch.drain()
    b1 = pctx.bus_bytes()
    assert b1[0] > b0[0] and b1[1] > b0[1]                                # the host run moved its frames over the bus
    srcs = [hip.Surface(pctx, w, h, depth) for _ in range(n)]
    got = []
    try:
        for s, fr in zip(srcs, frames):
            fill(pctx, s, fr)
        b1 = pctx.bus_bytes()
        with hbrt.Chain(hip.filters(), surface_list(name), w, h, pix_fmt) as ch:
            for t, s in enumerate(srcs):
                ch.push_surface(s, pts=t * 3003)
            ch.push_eof()
            while ch.pending():
                o = ch.pop_surface()
                assert o is not None or ch.eof                            # surface buffers, then the end of the stream
                if o is not None:
                    got.append(o)
            assert ch.eof
        assert pctx.bus_bytes() == b1                                     # nothing of the surface run went over the bus
        assert len(got) == len(want) == n
        for t in range(n):
            s, info = got[t]
            assert (info.start, info.fmt, info.width, info.height, info.nplanes) == (want[t].start, pix_fmt, w, h, 0)
            for p, a in enumerate(read(pctx, s)):
                np.testing.assert_array_equal(a, want[t].planes[p], err_msg=f"frame {t} plane {p}")
    finally:
        for s, _ in got:
            s.close()
        for s in srcs:
            s.close()


def test_surface_setting_needs_a_format_and_a_biplanar_adapter(built):
    F = hip.filters()
    with pytest.raises(RuntimeError):
        hbrt.Chain(F, [("hb_filter_hip_upload", ""), ("hb_filter_hip_download", "surface=1")], 66, 38)
    with pytest.raises(RuntimeError):
        hbrt.Chain(F, [("hb_filter_hip_upload", ""), ("hb_filter_hip_download", "surface=1")], 66, 38, pix_fmt=bc.NV12)
    with pytest.raises(RuntimeError):
        hbrt.Chain(F, [("hb_filter_hip_upload", ""), ("hb_filter_hip_download", "format=p010le:surface=1")], 66, 38, pix_fmt=bc.NV12)
    hbrt.Chain(F, [("hb_filter_hip_upload", ""), ("hb_filter_hip_download", "format=nv12:surface=0")], 66, 38, pix_fmt=bc.NV12).close()
    # a surface buffer on an adapter initialised for yuv420p: work() fails, nothing reaches the device
    pctx = plugin_ctx()
    s = hip.Surface(pctx, 66, 38, 8)
    try:
        before = pctx.bus_bytes()
        with hbrt.Chain(F, [("hb_filter_hip_upload", ""), ("hb_filter_hip_download", "")], 66, 38) as ch:
            with pytest.raises(RuntimeError):
                ch.push_surface(s)
        assert pctx.bus_bytes() == before
    finally:
        s.close()


def test_surfaces_outlive_the_chain_that_made_them(built):
    """popped surfaces held across the chain's close, released afterwards: they go back to the pool, and a second chain runs
    on surfaces of the pool again - no two of them, and none of the inputs, the same memory"""
    w, h, n = 66, 38, 8
    pctx = plugin_ctx()
    frames = [bc.frame(bc.NV12, w, h, seed=t) for t in range(n)]
    srcs = [hip.Surface(pctx, w, h, 8) for _ in range(n)]
    for s, fr in zip(srcs, frames):
        fill(pctx, s, fr)

    def run():
        got = []
        with hbrt.Chain(hip.filters(), surface_list("nv12"), w, h, bc.NV12) as ch:
            for t, s in enumerate(srcs):
                ch.push_surface(s, pts=t * 3003)
            ch.push_eof()
            while ch.pending():
                o = ch.pop_surface()
                assert o is not None or ch.eof
                if o is not None:
                    got.append(o[0])
        return got                                                        # the chain is closed, the surfaces are ours

    try:
        first = run()
        assert len(first) == n
        pics = [read(pctx, s) for s in first]
        assert len({s.describe()[0] for s in first + srcs}) == 2 * n
        for s in first:
            s.close()
        second = run()
        assert len(second) == n
        assert len({s.describe()[0] for s in second + srcs}) == 2 * n
        for a, s in zip(pics, second):
            for p, b in enumerate(read(pctx, s)):
                np.testing.assert_array_equal(b, a[p])
        for s in second:
            s.close()
    finally:
        for s in srcs:
            s.close()
