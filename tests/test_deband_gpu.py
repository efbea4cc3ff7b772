"""GPU: the deband drop-in (csrc/deband.hip, libhb/deband_hip.c) is bit-exact with the numpy model
(tests/deband_model.py) - the defaults at 1080p, blur on and off, the thresholds' range, per-plane thresholds, 8/10/12
bits on 4:2:0/4:2:2/4:4:4 with odd and tiny sizes, every range of the table test on both kernels, the tile kernel at
its largest halo and the cut-over past it, bursts with mixed pitches - and inside a device-resident job between VFR and NLMeans."""
import ctypes as C

import numpy as np
import pytest

import deband_model as dm
from burst_util import bursts
from handbrake_amd import hbrt, hip, synth

pytestmark = pytest.mark.gpu
DROPIN = "hb_filter_deband_hip"
LCW = {"2x2": (1, 1), "2x1": (1, 0), "1x1": (0, 0)}


def model(frames, settings, depth=8):
    return [dm.deband_frame(fr, settings, depth) for fr in frames]


def check(got, want, what=""):
    assert len(got) == len(want) > 0
    for t in range(len(want)):
        for c in range(3):
            g = got[t].planes[c] if hasattr(got[t], "planes") else got[t][c]
            assert g.shape == want[t][c].shape, f"{what} frame {t} plane {c} shape"
            np.testing.assert_array_equal(g, want[t][c], err_msg=f"{what} frame {t} plane {c}")


def test_defaults_1080p(built):
    frames = synth.stream("banded", 1920, 1080, 2)
    got = hbrt.run_stream(hip.filters(), [(DROPIN, "")], frames)
    check(got, model(frames, ""), "defaults")
    for c in range(3):
        diff = got[0].planes[c] != frames[0][c]
        assert diff.any() and not diff.all(), c


@pytest.mark.parametrize("thr", [0.00003, 0.02, 0.1, 0.5])
@pytest.mark.parametrize("blur", [0, 1])
def test_thresholds_and_blur(built, thr, blur):
    frames = synth.stream("banded", 352, 200, 3, cfg=5)
    st = f"1thr={thr}:2thr={thr}:3thr={thr}:blur={blur}"
    check(hbrt.run_stream(hip.filters(), [(DROPIN, st)], frames), model(frames, st), st)


@pytest.mark.parametrize("blur", [0, 1])
def test_per_plane_thresholds(built, blur):
    """three different thresholds in one run: a plane mix-up changes the picture"""
    frames = synth.stream("banded", 320, 184, 2, cfg=7)
    st = f"1thr=0.005:2thr=0.04:3thr=0.2:range=12:blur={blur}"
    want = model(frames, st)
    check(hbrt.run_stream(hip.filters(), [(DROPIN, st)], frames), want, st)
    for perm in ("1thr=0.04:2thr=0.2:3thr=0.005", "1thr=0.2:2thr=0.005:3thr=0.04"):
        other = model(frames, f"{perm}:range=12:blur={blur}")
        assert any(not np.array_equal(other[0][c], want[0][c]) for c in range(3))


def _format_cases():
    out = []
    for w, h in [(637, 359), (640, 360), (24, 18)]:
        for sub in ("2x2", "2x1", "1x1"):
            for depth in (8, 10, 12):
                out.append((w, h, sub, depth))
    return out


@pytest.mark.parametrize("w,h,sub,depth", _format_cases())
def test_depths_and_layouts(built, w, h, sub, depth):
    frames = [synth.picture("banded", w, h, t, cfg=21, depth=depth, chroma=sub) for t in range(2)]
    for st in ("", "blur=0:range=7"):
        got = hbrt.run_stream(hip.filters(), [(DROPIN, st)], frames, pix_fmt=hbrt.PIX_FMT[(sub, depth)])
        check(got, model(frames, st, depth), f"{w}x{h} {sub} {depth} {st!r}")


# ---- the C ABI directly: both kernels, bursts ------------------------------------------------------------------------
def _make(ctx, settings, w, h, depth=8):
    p = hip.DebandParams()
    F = hip.filters()
    F.hbhip_deband_params_from_settings.argtypes = [C.c_char_p, C.c_int, C.POINTER(hip.DebandParams)]
    assert F.hbhip_deband_params_from_settings(settings.encode(), depth, C.byref(p)) == 0
    return hip._create("hbhip_deband_create", ctx, [C.c_void_p, C.POINTER(hip.DebandParams)] + [C.c_int] * 5 + [C.POINTER(C.c_void_p)],
                       ctx.h, C.byref(p), w, h, depth, 1, 1)


def _bursts(settings, frames, sizes, kernel=0, pads=(0,), depth=8):
    """burst_util.bursts through the deband filter with hbhip_deband_set_kernel(kernel).  None: the filter refuses `kernel`"""
    h, w = frames[0][0].shape
    hip.lib().hbhip_deband_set_kernel.argtypes = [C.c_void_p, C.c_int]
    return bursts(lambda ctx: _make(ctx, settings, w, h, depth), frames, sizes, pads=pads, depth=depth,
                  setup=lambda flt: hip.lib().hbhip_deband_set_kernel(flt.h, kernel))


@pytest.mark.parametrize("rng", [16, 0, 1, -1, -16, 127, 128, 200, 5000, 1 << 30])
def test_ranges_on_both_kernels(built, rng):
    """every range of the CPU table test: int8 and int16 tables, the clamp, the LDS tile where its halo fits and the
    global gather everywhere"""
    frames = synth.stream("banded", 256, 144, 3, cfg=9)
    st = f"range={rng}:1thr=0.05:2thr=0.05:3thr=0.05"
    want = model(frames, st)
    gather = _bursts(st, frames, [3], kernel=2, pads=(0, 3))
    check(gather, want, f"gather range {rng}")
    tile = _bursts(st, frames, [3], kernel=1, pads=(0, 3))
    if abs(rng) <= 16:
        assert tile is not None                                          # the default range's halo fits the tile
    if tile is not None:
        check(tile, want, f"tile range {rng}")
    auto = _bursts(st, frames, [3], kernel=0)
    check(auto, want, f"auto range {rng}")


@pytest.mark.parametrize("st", ["", "blur=0:range=24", "range=-9:blur=1"])
@pytest.mark.parametrize("depth", [8, 10])
def test_bursts_equal_frame_by_frame(built, st, depth):
    frames = synth.stream("banded", 320, 200, 20, depth=depth)
    want = model(frames, st, depth)
    for kernel in (0, 2):
        check(_bursts(st, frames, [1, 3, 16], kernel=kernel, pads=(0, 0, 64, 5), depth=depth), want, f"bursts 1/3/16 kernel {kernel}")
    check(_bursts(st, frames, [1] * 20, depth=depth), want, "frame by frame")


# ---- the tile kernel's capacity -------------------------------------------------------------------------------------------
# The tile kernel holds (32 + 2R) rows of (128 + 2RP) / 4 four-sample groups, RP = R rounded up to 4, and a thread fetches
# at most 16 of them: (32 + 2R) * (128 + 2RP) / 4 <= 16 * 256 holds up to R = 28 (4 048 groups; R = 29: 4 320).
# `range` settings whose 256 x 144 table has a largest |offset| R of 27, 28 and 29: a negative range is a constant
# distance, a positive one a spread of distances and directions.
TILE_W, TILE_H = 256, 144
RANGES_FOR_R = {27: (-27, 29), 28: (-28, 30), 29: (-29, 31)}
THR = "1thr=0.05:2thr=0.05:3thr=0.05"


def _table_R(w, h, rng):
    """the largest |offset| of the model's table as the drop-in keeps it: clamped to +-max(w, h)"""
    lim = max(w, h)
    return max(int(np.abs(np.clip(t, -lim, lim)).max()) for t in dm.offsets(w, h, rng))


def _tile_groups(R):
    return (32 + 2 * R) * ((128 + 2 * ((R + 3) & ~3)) // 4)


@pytest.mark.parametrize("blur", [0, 1])
@pytest.mark.parametrize("depth", [8, 10, 12])
@pytest.mark.parametrize("R,rng", [(R, rng) for R in (27, 28) for rng in RANGES_FOR_R[R]])
def test_tile_kernel_at_its_largest_halo(built, R, rng, depth, blur):
    """R = 27 and R = 28, the last halo that fits (all 16 fetch slots of a thread live, 32 KB of LDS at 10 / 12 bits):
    the tile kernel, the gather and the automatic choice equal the model, on aligned and on sample stores"""
    assert _table_R(TILE_W, TILE_H, rng) == R and _tile_groups(R) <= 16 * 256
    assert _tile_groups(28) > 15 * 256 and _tile_groups(29) > 16 * 256
    frames = synth.stream("banded", TILE_W, TILE_H, 2, cfg=9, depth=depth)
    st = f"range={rng}:{THR}:blur={blur}"
    want = model(frames, st, depth)
    assert any(not np.array_equal(want[0][c], frames[0][c]) for c in range(3))
    for kernel in (1, 2, 0):
        got = _bursts(st, frames, [2], kernel=kernel, pads=(0, 3), depth=depth)
        assert got is not None, f"kernel {kernel} refused at R = {R}"
        check(got, want, f"kernel {kernel} R {R} depth {depth} blur {blur}")


@pytest.mark.parametrize("depth", [8, 10, 12])
@pytest.mark.parametrize("rng", RANGES_FOR_R[29])
def test_past_the_tile_kernels_capacity(built, rng, depth):
    """R = 29: the tile kernel is refused, the automatic choice falls to the gather"""
    assert _table_R(TILE_W, TILE_H, rng) == 29 and _tile_groups(29) > 16 * 256
    frames = synth.stream("banded", TILE_W, TILE_H, 2, cfg=9, depth=depth)
    st = f"range={rng}:{THR}"
    want = model(frames, st, depth)
    assert _bursts(st, frames, [2], kernel=1, depth=depth) is None
    for kernel in (0, 2):
        check(_bursts(st, frames, [2], kernel=kernel, pads=(0, 3), depth=depth), want, f"kernel {kernel} R 29 depth {depth}")


@pytest.mark.parametrize("depth", [8, 10, 12])
@pytest.mark.parametrize("rng", RANGES_FOR_R[28])
def test_tile_kernel_on_a_frame_inside_its_halo(built, rng, depth):
    """24 x 18 on 4:2:0 with R = 28's ranges: the table is clamped to +-24, at least the size of every plane both ways, so
    the tile kernel's halo fetches are all clamped ones"""
    w, h = 24, 18
    R = _table_R(w, h, rng)
    assert R >= h and (R + 3) & ~3 >= w and _tile_groups(R) <= 16 * 256
    frames = [synth.picture("banded", w, h, t, cfg=21, depth=depth, chroma="2x2") for t in range(2)]
    for blur in (0, 1):
        st = f"range={rng}:{THR}:blur={blur}"
        got = _bursts(st, frames, [2], kernel=1, pads=(0, 3), depth=depth)
        assert got is not None
        check(got, model(frames, st, depth), f"tile kernel, {w}x{h}, depth {depth}, blur {blur}")


# ---- inside device-resident runs --------------------------------------------------------------------------------------
def test_device_run_between_decomb_and_nlmeans(built):
    """[upload, decomb, deband, nlmeans, download] equals decomb and nlmeans on host frames with the model between"""
    TFF = 0x0008
    frames = synth.stream("interlaced", 320, 184, 6)
    st = ""
    UP, DOWN = ("hb_filter_hip_upload", ""), ("hb_filter_hip_download", "")
    dev = hbrt.run_stream(hip.filters(), [UP, ("hb_filter_decomb_hip", "mode=31"), (DROPIN, st),
                                          ("hb_filter_nlmeans_hip", hip.NLMEANS_MEDIUM), DOWN], frames, flags=TFF)
    mid = hbrt.run_stream(hip.filters(), [("hb_filter_decomb_hip", "mode=31")], frames, flags=TFF)
    deb = [dm.deband_frame(m.planes, st, 8) for m in mid]
    assert any(not np.array_equal(d[0], m.planes[0]) for d, m in zip(deb, mid))
    want = hbrt.run_stream(hip.filters(), [("hb_filter_nlmeans_hip", hip.NLMEANS_MEDIUM)], deb, flags=TFF)
    check(dev, [w.planes for w in want], "device run")


VFR = 11
UPN, DOWNN = "HIP upload adapter", "HIP download adapter"


@pytest.fixture()
def job_filters(built):
    import oracle_lib as ol
    if ol.ref() is None:
        pytest.skip("oracle/_ref not built (no /root/reference)")
    from test_job_swap_cpu import REF
    hip.filters()
    hbrt.register_filters(ol.ref(), REF)
    hbrt.register_filters(ol.ref(), {VFR: "hb_filter_vfr"})
    # crop/scale and deband are alias filters in the reference (settings for the combined avfilter graph; FFmpeg is
    # not in the image): the ids resolve to the drop-ins themselves, which the swap then leaves in place
    hbrt.register_filters(hip.filters(), {hbrt.FILTER_ID["crop_scale"]: "hb_filter_crop_scale_hip", 13: DROPIN})
    yield ol
    hbrt.register_filters(ol.ref(), {VFR: None})
    hbrt.register_filters(ol.ref(), {k: None for k in REF})
    hbrt.register_filters(hip.filters(), {hbrt.FILTER_ID["crop_scale"]: None, 13: None})


@pytest.mark.parametrize("vfr", ["mode=0:rate=30000/1001", "mode=1:rate=90000/1001"], ids=["same_as_source", "constant_dup"])
def test_job_with_deband_stays_one_device_run(job_filters, vfr):
    """[decomb 31, vfr, deband, nlmeans, crop_scale, lapsharp] through the plugin surface: one upload / download pair
    around all six, and the pictures of the CPU job before deband, the model, and the CPU job after it.  With vfr
    duplicating frames (one shared device picture) no picture is debanded twice."""
    ol = job_filters
    F = hbrt.FILTER_ID
    TFF = 0x0008
    NLM = hip.NLMEANS_MEDIUM + ":threads=2"
    LAP = "y-strength=0.2:y-kernel=isolap:cb-strength=0.2:cb-kernel=isolap"
    st = "1thr=0.02:2thr=0.02:3thr=0.02:4thr=0.02:range=16:blur=1"
    frames = synth.stream("interlaced", 320, 184, 9, cfg=3)
    filters = [(F["decomb"], "mode=31"), (VFR, vfr), (F["deband"], st), (F["nlmeans"], NLM),
               (F["crop_scale"], "width=640:height=368"), (F["lapsharp"], LAP)]
    with hbrt.Job(filters, 320, 184, use_hip=True) as job:
        names = job.stages()
    assert names.count(UPN) == 1 and names.count(DOWNN) == 1 and names[0] == UPN and names[-1] == DOWNN
    assert "Deband (HIP)" in names and len(names) == 8
    _, out = hbrt.run_job(filters, frames, flags=TFF, use_hip=True)
    _, mid = hbrt.run_job([(F["decomb"], "mode=31"), (VFR, vfr)], frames, flags=TFF, use_hip=False)
    deb = [dm.deband_frame(m.planes, st, 8) for m in mid]
    den = hbrt.run_stream(ol.ref(), [("hb_filter_nlmeans", NLM)], deb, flags=TFF)
    scaled = [ol.orc_cropscale_frame(d.planes, width=640, height=368) for d in den]
    want = hbrt.run_stream(ol.ref(), [("hb_filter_lapsharp", LAP)], scaled)
    assert len(out) == len(want) == len(mid) > 0
    if vfr.startswith("mode=1"):
        assert len(mid) > len(frames)                                    # vfr did duplicate
    for o, wt, m in zip(out, want, mid):
        assert (o.start, o.stop) == (m.start, m.stop)
        for c in range(3):
            np.testing.assert_array_equal(o.planes[c], wt.planes[c])
