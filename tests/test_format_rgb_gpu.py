"""GPU: packed 32-bit RGB pictures from 8-bit 4:2:0 frames - rgb32_pack_kernel (csrc/rgb_pack.hip) through the C ABI
(hbhip_frame_download_rgb32, hbhip_frame_download_rgb32_async) against tests/rgb32_model.py, byte for byte."""
import ctypes as C

import numpy as np
import pytest

from handbrake_amd import hip
import rgb32_model as rm

pytestmark = pytest.mark.gpu
ERR_ARG, ERR_UNSUPPORTED = -3, -5
SENTINEL = 0xA5
# 2x2 the smallest legal; 16x16 whole lanes; 18x16 and 66x34 a row that ends in a lane with two live pixels (66x34: 17
# lanes, an odd count of row pairs against the block's four); 258x18 more than one wave and more than one block a row pair
SIZES = [(2, 2), (16, 16), (18, 16), (66, 34), (258, 18)]


@pytest.fixture(scope="module")
def ctx():
    c = hip.Ctx(0)
    yield c
    c.close()


def planar8(rng, w, h):
    return tuple(rng.integers(0, 256, s, dtype=np.uint8) for s in ((h, w), (h // 2, w // 2), (h // 2, w // 2)))


def saturated(w, h):
    """Y, Cb, Cr in {0, 255}, in blocks: every corner of the code cube"""
    cy, cx = np.mgrid[0:h // 2, 0:w // 2]
    y = np.where((np.mgrid[0:h, 0:w][1] // 2 + np.mgrid[0:h, 0:w][0] // 6) % 2, 255, 0).astype(np.uint8)
    cb = np.where((cx // 2) % 2, 255, 0).astype(np.uint8)
    cr = np.where((cx // 4 + cy // 5) % 2, 255, 0).astype(np.uint8)
    return y, cb, cr


class Host:
    """a packed picture inside one sentinel-filled block: `extra` bytes a row beyond 4 * width, rows in front and behind"""

    def __init__(self, w, h, extra=0):
        self.w, self.h, self.stride = w, h, 4 * w + extra
        self.off = 4 * self.stride
        self.buf = np.full(self.off + self.stride * (h + 4), SENTINEL, dtype=np.uint8)

    @property
    def ptr(self):
        return self.buf.ctypes.data + self.off

    def _rows(self):
        return self.buf[self.off:self.off + self.stride * self.h].reshape(self.h, self.stride)

    def read(self):
        return np.ascontiguousarray(self._rows()[:, :4 * self.w]).reshape(self.h, self.w, 4)

    def untouched(self):
        """the rows in front of and behind the picture, and every row's bytes beyond 4 * width"""
        around = (self.buf[:self.off] == SENTINEL).all() and (self.buf[self.off + self.stride * self.h:] == SENTINEL).all()
        return bool(around and (self._rows()[:, 4 * self.w:] == SENTINEL).all())


def download(ctx, fr, dst, order, matrix, full, form="sync"):
    L = hip.lib()
    o = hip.RGB32_ORDERS.index(order)
    if form == "sync":
        hip.check(L.hbhip_frame_download_rgb32(fr.h, dst.ptr, dst.stride, o, matrix, int(full)), ctx.h, "download_rgb32")
        return
    tok = C.c_void_p()
    hip.check(L.hbhip_frame_download_rgb32_async(fr.h, dst.ptr, dst.stride, o, matrix, int(full), C.byref(tok)), ctx.h, "download_rgb32_async")
    assert tok.value
    hip.check(L.hbhip_frame_download_wait(fr.h, tok), ctx.h, "download_wait")


def run(ctx, x, order="bgra", matrix=1, full=False, extra=0, form="sync"):
    h, w = x[0].shape
    fr = hip.Frame(ctx, w, h, 8)
    try:
        fr.upload(x)
        dst = Host(w, h, extra)
        download(ctx, fr, dst, order, matrix, full, form)
        assert dst.untouched()
        for got, was in zip(fr.download(), x):                          # the frame is only read
            np.testing.assert_array_equal(got, was)
        return dst.read()
    finally:
        fr.close()


@pytest.mark.parametrize("form", ["sync", "async"])
@pytest.mark.parametrize("w,h", SIZES)
def test_sizes_equal_the_model(built, ctx, w, h, form):
    x = planar8(np.random.default_rng(100 * w + h), w, h)
    np.testing.assert_array_equal(run(ctx, x, form=form), rm.pack(x, 1, False, "bgra"))


def test_every_triple_equals_the_model(built, ctx):
    """4096 x 4096: every (Y, Cb, Cr) once, BT.709 limited, bgra"""
    x = rm.all_triples()
    got = run(ctx, x)
    want = rm.pack(x, 1, False, "bgra")
    assert np.array_equal(got, want), "first difference at %s" % (np.argwhere(got != want)[:1],)


@pytest.mark.parametrize("full", [False, True])
@pytest.mark.parametrize("matrix", [1, 6, 9])
@pytest.mark.parametrize("order", rm.ORDERS)
def test_orders_matrices_ranges(built, ctx, order, matrix, full):
    w, h = 66, 34
    for what, x in (("random", planar8(np.random.default_rng(7 * matrix + full), w, h)), ("saturated", saturated(w, h))):
        np.testing.assert_array_equal(run(ctx, x, order, matrix, full), rm.pack(x, matrix, full, order), err_msg=what)


def test_unspecified_matrix_is_bt601(built, ctx):
    x = planar8(np.random.default_rng(3), 18, 16)
    np.testing.assert_array_equal(run(ctx, x, matrix=2), rm.pack(x, 6, False, "bgra"))


@pytest.mark.parametrize("form", ["sync", "async"])
@pytest.mark.parametrize("w,h", [(66, 34), (16, 16)])
def test_a_wider_destination_keeps_its_padding(built, ctx, w, h, form):
    """stride 4 * width + 48 over a sentinel: the 48 bytes of every row and the rows around the picture stay (run() checks)"""
    x = planar8(np.random.default_rng(11), w, h)
    np.testing.assert_array_equal(run(ctx, x, "rgba", 6, True, extra=48, form=form), rm.pack(x, 6, True, "rgba"))


def test_six_downloads_in_flight(built, ctx):
    """six different frames, every download queued before the first wait: each arrives as its own picture"""
    L = hip.lib()
    w, h = 66, 34
    rng = np.random.default_rng(21)
    xs = [planar8(rng, w, h) for _ in range(6)]
    frames, hosts, toks = [], [], []
    try:
        for x in xs:
            fr = hip.Frame(ctx, w, h, 8)
            frames.append(fr)
            fr.upload(x)
        for k, fr in enumerate(frames):
            dst, tok = Host(w, h, 16 * (k % 2)), C.c_void_p()
            hip.check(L.hbhip_frame_download_rgb32_async(fr.h, dst.ptr, dst.stride, k % 4, 1, 0, C.byref(tok)), ctx.h, "download_rgb32_async")
            hosts.append(dst)
            toks.append(tok)
        for fr, tok in zip(frames, toks):
            hip.check(L.hbhip_frame_download_wait(fr.h, tok), ctx.h, "download_wait")
        for k, (x, dst) in enumerate(zip(xs, hosts)):
            np.testing.assert_array_equal(dst.read(), rm.pack(x, 1, False, rm.ORDERS[k % 4]), err_msg=f"frame {k}")
            assert dst.untouched()
    finally:
        for fr in frames:
            fr.close()


# (frame geometry: w, h, depth, lcw, lch), stride - 4 w, order, matrix -> the error code
REFUSALS = [
    ((16, 16, 10, 1, 1), 0, 0, 1, ERR_UNSUPPORTED),         # not depth 8
    ((16, 16, 8, 1, 0), 0, 0, 1, ERR_UNSUPPORTED),          # 4:2:2
    ((16, 16, 8, 0, 0), 0, 0, 1, ERR_UNSUPPORTED),          # 4:4:4
    ((17, 16, 8, 1, 1), 0, 0, 1, ERR_UNSUPPORTED),          # odd width
    ((16, 15, 8, 1, 1), 0, 0, 1, ERR_UNSUPPORTED),          # odd height
    ((1, 2, 8, 1, 1), 0, 0, 1, ERR_UNSUPPORTED),            # under 2 x 2
    ((2, 1, 8, 1, 1), 0, 0, 1, ERR_UNSUPPORTED),
    ((16, 16, 8, 1, 1), 0, 0, 0, ERR_UNSUPPORTED),          # RGB
    ((16, 16, 8, 1, 1), 0, 0, 8, ERR_UNSUPPORTED),          # YCgCo
    ((16, 16, 8, 1, 1), 0, 0, 12, ERR_UNSUPPORTED),         # chroma-derived
    ((16, 16, 8, 1, 1), 0, 0, 13, ERR_UNSUPPORTED),
    ((16, 16, 8, 1, 1), 0, 0, 14, ERR_UNSUPPORTED),         # ICtCp
    ((16, 16, 8, 1, 1), -4, 0, 1, ERR_ARG),                 # a stride below 4 * width
    ((16, 16, 8, 1, 1), 0, 4, 1, ERR_ARG),                  # an order outside the enum
    ((16, 16, 8, 1, 1), 0, -1, 1, ERR_ARG),
]


@pytest.mark.parametrize("geometry,dstride,order,matrix,code", REFUSALS)
def test_refusals_answer_their_code_and_write_nothing(built, ctx, geometry, dstride, order, matrix, code):
    L = hip.lib()
    w, h = geometry[:2]
    fr = hip.Frame(ctx, *geometry)
    try:
        dst = Host(w, h)
        before = dst.buf.copy()
        assert L.hbhip_frame_download_rgb32(fr.h, dst.ptr, dst.stride + dstride, order, matrix, 0) == code
        tok = C.c_void_p(1)
        assert L.hbhip_frame_download_rgb32_async(fr.h, dst.ptr, dst.stride + dstride, order, matrix, 0, C.byref(tok)) == code
        assert not tok.value
        ctx.sync()
        assert np.array_equal(dst.buf, before)
    finally:
        fr.close()
