"""NLMeans around its displacement walks: the tile staging (every load of a thread in flight; the interior and the
reflected path; the next frame's tile fetched under frame 0's light walks), the job of a tile by arithmetic, and both
forms of the origin term - bit-exact against the CPU oracle (oracle_lib.orc_nlmeans_plane, through
oracle_stream.nlmeans_stream) on the smallest frames that reach each path."""
import ctypes as C
import functools

import numpy as np
import pytest

from handbrake_amd import hbrt, hip, synth
import oracle_stream as ostream

pytestmark = pytest.mark.gpu

MEDIUM = hip.NLMEANS_MEDIUM


def par(strength=6, origin_tune=1.0, patch=7, rng=3, nframes=2, prefilter=0):
    return dict(strength=strength, origin_tune=origin_tune, patch=patch, range=rng, nframes=nframes, prefilter=prefilter)


def settings_of(y, cb):
    def one(name, p):
        return (f"{name}-strength={p['strength']}:{name}-origin-tune={p['origin_tune']}:{name}-patch-size={p['patch']}:"
                f"{name}-range={p['range']}:{name}-frame-count={p['nframes']}:{name}-prefilter={p['prefilter']}")
    return one("y", y) + ":" + one("cb", cb)


def check_stream(frames, settings, pp, pix_fmt=hbrt.AV_PIX_FMT_YUV420P):
    got = hbrt.run_stream(hip.filters(), [("hb_filter_nlmeans_hip", settings)], frames, pix_fmt=pix_fmt)
    want = ostream.nlmeans_stream(frames, pp)
    assert len(got) == len(frames)
    for t in range(len(frames)):
        for c in range(3):
            np.testing.assert_array_equal(got[t].planes[c], want[t][c], err_msg=f"frame {t} plane {c}")


# 122 x 66: a second tile column 2 pixels wide and a second tile row 2 rows high; chroma 61 x 33, rows that are not whole
# dwords.  242 x 130: three tiles each way.  260 x 136: the smallest frame with a tile whose halo lies wholly inside the
# plane (tile column 1 needs 112 + 144 <= w, tile row 1 needs 60 + 72 <= h), so the only one here that takes the
# interior path - next to eight tiles that take the reflected one.  32 x 32: chroma 16 x 16, the smallest plane the
# filter takes - every read of its halo reflected, the far ones clamped.
@pytest.mark.parametrize("w,h", [(32, 32), (122, 66), (242, 130), (260, 136)])
def test_medium_at_the_sizes_where_the_staging_paths_change(built, w, h):
    frames = synth.stream("random", w, h, 3)
    check_stream(frames, MEDIUM, [par(), par(), par()])


def test_16x16_every_plane(built):
    """A 16 x 16 frame whose chroma is 16 x 16 too (4:4:4): the smallest frame the filter takes.  (With 4:2:0 its chroma
    would be 8 x 8, narrower than the reference's 16-pixel mirrored border, which the reference fills from bytes it has
    not written yet: the filter declines such planes - see the test below.)"""
    base = synth.stream("random", 32, 32, 3)
    frames = [tuple(np.ascontiguousarray(p[:16, :16]) for p in (y, y[16:, 16:], y[:16, 16:])) for y, _, _ in base]
    check_stream(frames, MEDIUM, [par(), par(), par()], pix_fmt=SUBSAMPLING["444"][0])


def test_16x16_with_8x8_chroma_is_declined(built):
    p = hip.NLMeansParams()
    hip.filters().hbhip_nlmeans_params_from_settings(MEDIUM.encode(), 8, C.byref(p))
    ctx = hip.Ctx(0)
    handle = C.c_void_p()
    assert hip.lib().hbhip_nlmeans_create(ctx.h, C.byref(p), 16, 16, 8, 1, 1, C.byref(handle)) == -5    # HBHIP_ERR_UNSUPPORTED
    ctx.close()


CASES = {
    # a third tile, staged with nothing fetched ahead
    "frame-count-3": (par(nframes=3), par(nframes=3)),
    # range 5: no shared pairs
    "range-5": (par(rng=5), par(rng=5)),
    # a prefilter: four tiles (the prefiltered and the raw twin of both frames)
    "prefilter": (par(prefilter=1), par(prefilter=2)),
    # the origin term in double
    "origin-tune-0.5": (par(origin_tune=0.5), par(origin_tune=0.5)),
    "origin-tune-0.8": (par(origin_tune=0.8), par(origin_tune=0.8)),
    # one plane at 1, one not: the launch takes the double form for both
    "origin-tune-mixed": (par(origin_tune=1.0), par(origin_tune=0.8)),
    "patch-3": (par(patch=3), par(patch=3)),
    "patch-9": (par(patch=9), par(patch=9)),
}


@pytest.mark.parametrize("case", sorted(CASES))
def test_settings_at_122x66(built, case):
    y, cb = CASES[case]
    frames = synth.stream("random", 122, 66, 4)
    check_stream(frames, settings_of(y, cb), [y, cb, cb])


@pytest.mark.parametrize("w,h", [(122, 66), (260, 136)])
def test_10bit(built, w, h):
    frames = synth.stream("random", w, h, 3, depth=10)
    pp = [dict(par(), depth=10) for _ in range(3)]
    check_stream(frames, MEDIUM, pp, pix_fmt=hbrt.PIX_FMT_FOR_DEPTH[10])


# ---- the job of a tile by arithmetic: launches of 1, 2 and 5 frames -------------------------------------------------
SUBSAMPLING = {"420": (0, 1, 1), "422": (4, 1, 0), "444": (5, 0, 0)}        # AVPixelFormat, log2 chroma w, log2 chroma h
BW, BH, BN = 122, 66, 7


@functools.lru_cache(maxsize=None)
def batch_stream(fmt):
    """frames of the subsampling and what the filter makes of them streamed one by one (computed once per format)"""
    pix_fmt, lcw, lch = SUBSAMPLING[fmt]
    base = synth.stream("random", 2 * BW, 2 * BH, BN)
    frames = [(np.ascontiguousarray(y[:BH, :BW]), np.ascontiguousarray(cb[:-(-BH >> lch), :-(-BW >> lcw)]),
               np.ascontiguousarray(cr[:-(-BH >> lch), :-(-BW >> lcw)])) for y, cb, cr in base]
    want = hbrt.run_stream(hip.filters(), [("hb_filter_nlmeans_hip", MEDIUM)], frames, pix_fmt=pix_fmt)
    return frames, [[p.copy() for p in o.planes] for o in want]


def device_filter(ctx, settings, w, h, batch, lcw, lch):
    p = hip.NLMeansParams()
    hip.filters().hbhip_nlmeans_params_from_settings(settings.encode(), 8, C.byref(p))
    handle = C.c_void_p()
    hip.check(hip.lib().hbhip_nlmeans_create(ctx.h, C.byref(p), w, h, 8, lcw, lch, C.byref(handle)), ctx.h, "hbhip_nlmeans_create")
    hip.check(hip.lib().hbhip_nlmeans_set_batch(handle, batch), ctx.h, "set_batch")
    return hip.DeviceFilter(ctx, handle)


def run_batched(flt, ctx, dev_in, dev_out):
    got = 0
    for t in range(len(dev_in)):
        flt.push_dev(hip.dev_frame(dev_in[t]), t)
        while flt.pending():
            assert flt.pull_dev(hip.dev_frame(dev_out[got])) == got
            got += 1
    flt.flush()
    while flt.pending():
        assert flt.pull_dev(hip.dev_frame(dev_out[got])) == got
        got += 1
    ctx.sync()
    return got


@pytest.mark.parametrize("batch", [1, 2, 5])
@pytest.mark.parametrize("fmt", sorted(SUBSAMPLING))
def test_batched_launches_equal_streamed(built, fmt, batch):
    """The device-resident batched entry (one launch for `batch` frames: batch x 3 jobs, found by arithmetic) gives the
    bytes of the same frames streamed one by one - for the per-plane tile counts of 4:2:0 (4, 1, 1), 4:2:2 (4, 2, 2) and
    4:4:4 (4, 4, 4)."""
    import torch
    _, lcw, lch = SUBSAMPLING[fmt]
    frames, want = batch_stream(fmt)
    ctx = hip.Ctx(0)
    flt = device_filter(ctx, MEDIUM, BW, BH, batch, lcw, lch)
    dev_in = [[torch.from_numpy(p.copy()).cuda() for p in fr] for fr in frames]
    dev_out = [[torch.zeros_like(p) for p in fr] for fr in dev_in]
    torch.cuda.synchronize()
    assert run_batched(flt, ctx, dev_in, dev_out) == BN
    for t in range(BN):
        for c in range(3):
            np.testing.assert_array_equal(dev_out[t][c].cpu().numpy(), want[t][c], err_msg=f"frame {t} plane {c}")
    flt.close()
    ctx.close()


def test_planes_one_byte_off_a_dword(built):
    """Planes whose rows start 1 byte past a dword boundary (and whose pitch is odd), in and out, through the device-frame
    entry."""
    import torch
    frames, want = batch_stream("420")

    def off_by_one(shape):
        h, w = shape
        pitch = w + 3 + (w & 1)                                         # odd
        buf = torch.zeros(h * pitch + 8, dtype=torch.uint8, device="cuda")
        start = 1 + (-buf.data_ptr()) % 4                               # address = 1 (mod 4)
        view = buf[start:start + h * pitch].view(h, pitch)[:, :w]
        assert view.data_ptr() % 4 == 1 and view.stride(0) % 2 == 1
        return view

    ctx = hip.Ctx(0)
    flt = device_filter(ctx, MEDIUM, BW, BH, 2, 1, 1)
    dev_in, dev_out = [], []
    for fr in frames:
        planes = [off_by_one(p.shape) for p in fr]
        for d, p in zip(planes, fr):
            d.copy_(torch.from_numpy(p.copy()))
        dev_in.append(planes)
        dev_out.append([off_by_one(p.shape) for p in fr])
    torch.cuda.synchronize()
    assert run_batched(flt, ctx, dev_in, dev_out) == BN
    for t in range(BN):
        for c in range(3):
            np.testing.assert_array_equal(dev_out[t][c].cpu().numpy(), want[t][c], err_msg=f"frame {t} plane {c}")
    flt.close()
    ctx.close()
