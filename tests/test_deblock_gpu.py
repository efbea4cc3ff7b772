"""GPU: the deblock drop-in (csrc/deblock.hip, libhb/deblock_hip.c) is bit-exact with the numpy model
(tests/deblock_model.py) - every preset and tune, 8/10/12 bits, 4:2:0/4:2:2/4:4:4, the threshold boundaries, block sizes
that put edges everywhere in the local kernel's tile and halo, the web kernel's chunked block row, edge counts and forced
repair path, bursts with mixed pitches and past 16 frames, the clip - and inside a device-resident job between VFR and
NLMeans.  The case lists are tests/deblock_cases.py."""
import ctypes as C
import functools

import numpy as np
import pytest

import deblock_cases as dc
import deblock_model as dm
from burst_util import bursts
from handbrake_amd import hbrt, hip, synth

pytestmark = pytest.mark.gpu
DROPIN = "hb_filter_deblock_hip"
LCW = dc.LCW


def model(frames, settings, depth=8):
    return [dm.deblock_frame(fr, settings, depth) for fr in frames]


def check(got, want, what=""):
    assert len(got) == len(want) > 0
    for t in range(len(want)):
        for c in range(3):
            g = got[t].planes[c] if hasattr(got[t], "planes") else got[t][c]
            assert g.shape == want[t][c].shape, f"{what} frame {t} plane {c} shape"
            np.testing.assert_array_equal(g, want[t][c], err_msg=f"{what} frame {t} plane {c}")


@pytest.mark.parametrize("tune", sorted(dm.TUNES))
@pytest.mark.parametrize("preset", sorted(dm.PRESETS))
def test_presets_and_tunes_1080p(built, preset, tune):
    frames = synth.stream("blocky", 1920, 1080, 1)
    st = dm.settings_for(preset, tune)
    got = hbrt.run_stream(hip.filters(), [(DROPIN, st)], frames)
    check(got, model(frames, st), st)
    assert not np.array_equal(got[0].planes[0], frames[0][0])


@pytest.mark.parametrize("w,h,sub,depth,st", dc.FORMAT_CASES)
def test_depths_and_layouts(built, w, h, sub, depth, st):
    frames = [synth.picture("blocky", w, h, t, cfg=21, depth=depth, chroma=sub) for t in range(1 if w > 1000 else 2)]
    got = hbrt.run_stream(hip.filters(), [(DROPIN, st)], frames, pix_fmt=hbrt.PIX_FMT[(sub, depth)])
    check(got, model(frames, st, depth), st)


def test_declined_sizes_fail_init(built):
    with pytest.raises(RuntimeError):
        hbrt.Chain(hip.filters(), [(DROPIN, "strength=strong")], 640, 362)      # 362 % 8 == 2
    hbrt.Chain(hip.filters(), [(DROPIN, "strength=weak")], 640, 362).close()


def _edge_picture(w, h, delta, inner, depth, b=8):
    """flat b x b blocks whose steps across every edge are `delta` (alternating up / down) with an in-block ramp of
    `inner` next to the edge: the skip tests sit exactly at (or one below) a threshold"""
    maxv = (1 << depth) - 1
    x = np.arange(w)[None, :]
    y = np.arange(h)[:, None]
    lvl = maxv // 2 + delta * (((x // b) + (y // b)) % 2)
    ramp = np.where((x % b) == b - 1, inner, 0) + np.where((y % b) == b - 1, inner, 0)
    return np.clip(lvl + ramp, 0, maxv).astype(np.uint8 if depth == 8 else np.uint16)


@pytest.mark.parametrize("depth", [8, 10])
@pytest.mark.parametrize("strong", [True, False])
def test_threshold_boundaries(built, depth, strong):
    st = ("strength=strong" if strong else "strength=weak") + ":thresh=20"
    ath, bth, _, _ = dm.thresholds(20, depth)
    w, h = 128, 64
    frames = []
    for delta in (ath, ath - 1):
        for inner in (bth, bth - 1, 0):
            y = _edge_picture(w, h, delta, inner, depth)
            c = _edge_picture(w // 2, h // 2, delta, inner, depth)
            frames.append((y, c, c.copy()))
    got = hbrt.run_stream(hip.filters(), [(DROPIN, st)], frames, pix_fmt=hbrt.PIX_FMT_FOR_DEPTH[depth])
    want = model(frames, st, depth)
    check(got, want, st)
    changed = [not np.array_equal(wt[0], fr[0]) for wt, fr in zip(want, frames)]
    assert any(changed) and not all(changed)


# ---- the C ABI directly: block sizes, the web kernel's shapes, bursts, the clip ----------------------------------------------
def _make(ctx, settings, w, h, depth=8, sub="2x2"):
    p = hip.DeblockParams()
    F = hip.filters()
    lcw, lch = LCW[sub]
    F.hbhip_deblock_params_from_settings.argtypes = [C.c_char_p] + [C.c_int] * 5 + [C.POINTER(hip.DeblockParams)]
    assert F.hbhip_deblock_params_from_settings(settings.encode(), depth, w, h, lcw, lch, C.byref(p)) == 0
    return hip._create("hbhip_deblock_create", ctx, [C.c_void_p, C.POINTER(hip.DeblockParams)] + [C.c_int] * 5 + [C.POINTER(C.c_void_p)],
                       ctx.h, C.byref(p), w, h, depth, lcw, lch)


def _set_warmup(flt, warmup):
    hip.lib().hbhip_deblock_set_warmup.argtypes = [C.c_void_p, C.c_int]
    assert hip.lib().hbhip_deblock_set_warmup(flt.h, warmup) == 0
    return 0


def _bursts(settings, frames, sizes, warmup=None, pads=(0,), depth=8, sub="2x2"):
    """burst_util.bursts through the deblock filter, with hbhip_deblock_set_warmup(warmup) where one is given"""
    h, w = frames[0][0].shape
    return bursts(lambda ctx: _make(ctx, settings, w, h, depth, sub), frames, sizes, pads=pads, depth=depth,
                  setup=None if warmup is None else (lambda flt: _set_warmup(flt, warmup)))


@functools.lru_cache(maxsize=None)
def _case(kind, w, h, sub, depth, st, n=2):
    """(frames, the model's frames, the model's edge statistics) of a case, computed once; leave them unchanged"""
    if kind == "blocky+flat":          # blocky content skips edges, the near-flat frame fires nearly all of them
        frames = [synth.picture("blocky", w, h, 0, cfg=21, depth=depth, chroma=sub), dc.near_flat(w, h, sub, depth, w + h)]
    elif kind == "flat":
        frames = [dc.near_flat(w, h, sub, depth, w + h)]
    elif kind == "stream":
        frames = synth.stream("blocky", w, h, n, depth=depth)
    elif kind == "white+black":
        frames = [dc.near_white(w, h, sub, depth, depth), dc.near_white(w, h, sub, depth, depth + 1, mirror=True)]
    stats = {}
    want = [dm.deblock_frame(fr, st, depth, stats) for fr in frames]
    for fr in list(frames) + want:
        for p in fr:
            p.setflags(write=False)
    return frames, want, stats


@pytest.mark.parametrize("w,h,sub,depth,st", dc.LOCAL_CASES)
def test_block_sizes_on_the_local_kernel(built, w, h, sub, depth, st):
    """block sizes that do not divide the 128 x 32 tile (edges at every position of tile and halo), the tightest
    non-overlapping windows (strong b = 6 / 7), b past the tile's height and width (tiles without an edge), b past the
    plane (a copy), last windows that end on the plane's last sample - at every depth and layout, through the C ABI"""
    frames, want, stats = _case("blocky+flat", w, h, sub, depth, st)
    check(_bursts(st, list(frames), [2], depth=depth, sub=sub), want, f"{w}x{h} {sub} {depth} {st}")
    if dc.has_edge(w, h, sub, st):
        assert 0 < stats["fired"] < stats["edges"], stats
        assert any(not np.array_equal(wt[0], fr[0]) for wt, fr in zip(want, frames))
    else:
        assert stats["edges"] == 0
        check(want, frames, "no edge: the model's output is its input")


@pytest.mark.parametrize("st", ["strength=strong:thresh=20", "strength=weak:thresh=20",
                                "strength=strong:thresh=50:blocksize=4", "strength=strong:thresh=20:blocksize=5"])
def test_bursts_equal_frame_by_frame(built, st):
    frames = synth.stream("blocky", 320, 200, 20)
    want = model(frames, st)
    check(_bursts(st, frames, [1, 3, 16]), want, "bursts 1/3/16")
    check(_bursts(st, frames, [1] * 20), want, "frame by frame")


@pytest.mark.parametrize("w,h,sub,depth,st", dc.PITCH_CASES)
def test_mixed_pitches_in_a_burst(built, w, h, sub, depth, st):
    """process_many groups the frames of a burst by equal pitches: bursts whose input pitches differ (and the uint16
    kernels through the C ABI) equal the model and the frame-by-frame result"""
    frames, want, _ = _case("stream", w, h, sub, depth, st, 5)
    single = _bursts(st, list(frames), [1] * 5, depth=depth)
    check(single, want, "frame by frame")
    for pads in ((0, 0, 64, 5, 0), (0, 16)):
        got = _bursts(st, list(frames), [5], pads=pads, depth=depth)
        check(got, want, f"pads {pads}")
        check(got, single, f"pads {pads} against frame by frame")


@pytest.mark.parametrize("w,h,sub,depth,st", dc.CUT_CASES)
def test_bursts_past_16_frames(built, w, h, sub, depth, st):
    """a launch takes 16 frames: a burst of 20 at one pitch is cut at 16, one whose pitch changes at frame 9 at 9"""
    frames, want, _ = _case("stream", w, h, sub, depth, st, 20)
    single = _bursts(st, list(frames), [1] * 20)
    check(single, want, "frame by frame")
    for pads in ((0,), (0,) * 9 + (64,) * 11):
        got = _bursts(st, list(frames), [20], pads=pads)
        check(got, want, f"burst of 20, pads {set(pads)}")
        check(got, single, "against frame by frame")


def _repair_frames(w, h, sub, depth, seed):
    frames = [dc.near_flat(w, h, sub, depth, seed + t, t) for t in range(3)]
    return frames + [synth.picture("blocky", w, h, t, cfg=13, depth=depth, chroma=sub) for t in range(2)]


@pytest.mark.parametrize("b", [4, 5])
def test_repair_path_forced(built, b):
    """warm-up 0 and near-flat content (every edge fires, the chains never forget): every segment's guessed entry is
    wrong and the repair walk makes the whole row - still exact"""
    w, h = 640, 360
    rng = np.random.default_rng(b)
    frames = []
    for t in range(3):
        y = (120 + rng.integers(-2, 3, size=(h, w)) + (np.arange(w)[None, :] // 7 + t) % 5).astype(np.uint8)
        cb = (128 + rng.integers(-2, 3, size=(h // 2, w // 2))).astype(np.uint8)
        frames.append((y, cb, cb.copy()))
    frames += synth.stream("blocky", w, h, 2)
    st = f"strength=strong:thresh=50:blocksize={b}"
    want = model(frames, st)
    for warmup in (0, 1, 64):
        check(_bursts(st, frames, [len(frames)], warmup=warmup), want, f"warmup {warmup}")


@pytest.mark.parametrize("depth,sub", [(10, "2x2"), (8, "1x1")])
@pytest.mark.parametrize("b", [4, 5])
def test_repair_path_forced_deep_and_444(built, b, depth, sub):
    """the same through the uint16 kernel, and with chroma planes as wide as luma"""
    w, h = 160, 80
    frames = _repair_frames(w, h, sub, depth, b)
    st = dc.settings(True, b, 50)
    want = model(frames, st, depth)
    for warmup in (0, 1, 64):
        check(_bursts(st, frames, [len(frames)], warmup=warmup, depth=depth, sub=sub), want, f"warmup {warmup}")


@pytest.mark.parametrize("depth", dc.WEB_DEPTHS)
@pytest.mark.parametrize("w,h,sub,b", dc.WEB_WIDE)
def test_web_block_row_in_chunks(built, w, h, sub, b, depth):
    """a luma row so wide that LDS holds fewer rows than a block row has: the walk of a block row takes several chunks"""
    # DeblockFilter::web_rows: 48 KiB / (2 w + 8 ceil(floor((w - 1) / b) / 8)) rows of the luma width fit, at most b
    nseg = -(-((w - 1) // b) // 8)
    rows_lds = min(b, 48 * 1024 // (2 * w + 8 * nseg))
    assert 1 <= rows_lds < b and rows_lds == dc.web_rows(w, b)
    st = dc.settings(True, b, dc.WEB_THRESH)
    frames, want, stats = _case("flat", w, h, sub, depth, st)
    assert stats["fired"] > 0.9 * stats["edges"], stats                  # the chains do not forget
    for warmup in (0, None):
        check(_bursts(st, list(frames), [1], warmup=warmup, depth=depth, sub=sub), want, f"{w}x{h} warmup {warmup}")


def _web_shape(w, h, sub, b):
    st = dc.settings(True, b, dc.WEB_THRESH)
    for depth in dc.WEB_DEPTHS:
        frames, want, stats = _case("blocky+flat", w, h, sub, depth, st)
        if dc.has_edge(w, h, sub, st):
            assert stats["fired"] > 0, stats
        for warmup in (0, None):
            check(_bursts(st, list(frames), [2], warmup=warmup, depth=depth, sub=sub), want, f"{w}x{h} {sub} {depth} warmup {warmup}")


@pytest.mark.parametrize("tall", [False, True], ids=["h<=b", "h=b+3"])
@pytest.mark.parametrize("ne", [0, 1, 7, 8, 9, 16])
@pytest.mark.parametrize("b", [4, 5])
def test_web_edge_counts(built, b, ne, tall):
    """rows of no edge (only horizontal edges exist), one, fewer than one 8-edge segment, exactly one, one more, exactly
    two; planes of one block row (only vertical edges exist) and of two - on all three planes (4:4:4)"""
    w, h = dc.WEB_WIDTHS[b][ne], dc.web_heights(b)[tall]
    assert (w - 1) // b == ne and (h > b) == tall
    _web_shape(w, h, "1x1", b)


@pytest.mark.parametrize("w,h,b", sorted(dc.WEB_SPLIT))
def test_web_luma_and_chroma_differ_in_segments(built, w, h, b):
    """4:2:0: one launch whose luma rows have more segments than its chroma rows (the LDS layout is per plane)"""
    ny, nc = (w - 1) // b, (-(-w // 2) - 1) // b
    assert -(-ny // 8) > -(-nc // 8) >= 1
    _web_shape(w, h, "2x2", b)


def _unclipped_first_block_row(plane, b, strong, thr):
    """the taps, before the clip, of every fired vertical edge of block row 0 - from the input and the model's arithmetic
    (block row 0 has no horizontal edge before it and at b = 8 no two windows overlap, so its edges see the input)"""
    L = 3 if strong else 2
    cols = np.arange(b, plane.shape[1], b)[:, None] + np.arange(-L, L)[None, :]
    win = plane.astype(np.int64)[:b][:, cols]
    _, fire = dm.edge(win, strong, thr, 1 << 20)
    d = win[..., L] - win[..., L - 1]
    div = dm.STRONG_DIV if strong else dm.WEAK_DIV
    taps = np.stack([win[..., k] + (1 if k < L else -1) * dm._div(d, div[k]) for k in range(2 * L)], axis=-1)
    return taps[fire]


@pytest.mark.parametrize("w,h,sub,depth,st", dc.CLIP_CASES)
def test_clip_at_both_ends(built, w, h, sub, depth, st):
    """thresh=100 on content next to the top of the range and on its mirror next to 0: fired edges push taps past
    both ends, and the clipped result is the model's"""
    frames, want, _ = _case("white+black", w, h, sub, depth, st)
    p = dm.resolve(st, depth)
    maxv = (1 << depth) - 1
    white = _unclipped_first_block_row(frames[0][0], p["block"], p["strong"], p["thr"])
    black = _unclipped_first_block_row(frames[1][0], p["block"], p["strong"], p["thr"])
    assert white.size and (white > maxv).any() and black.size and (black < 0).any()
    check(_bursts(st, list(frames), [2], depth=depth, sub=sub), want, st)


# ---- inside device-resident runs --------------------------------------------------------------------------------------
def test_device_run_between_decomb_and_nlmeans(built):
    """[upload, decomb, deblock, nlmeans, download] equals decomb and nlmeans on host frames with the model between"""
    TFF = 0x0008
    frames = synth.stream("interlaced", 320, 184, 6)
    st = dm.settings_for("medium")
    UP, DOWN = ("hb_filter_hip_upload", ""), ("hb_filter_hip_download", "")
    dev = hbrt.run_stream(hip.filters(), [UP, ("hb_filter_decomb_hip", "mode=31"), (DROPIN, st),
                                          ("hb_filter_nlmeans_hip", hip.NLMEANS_MEDIUM), DOWN], frames, flags=TFF)
    mid = hbrt.run_stream(hip.filters(), [("hb_filter_decomb_hip", "mode=31")], frames, flags=TFF)
    deb = [dm.deblock_frame(m.planes, st, 8) for m in mid]
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
    # crop/scale and deblock are alias filters in the reference (settings for the combined avfilter graph; FFmpeg is
    # not in the image): the ids resolve to the drop-ins themselves, which the swap then leaves in place
    hbrt.register_filters(hip.filters(), {hbrt.FILTER_ID["crop_scale"]: "hb_filter_crop_scale_hip", 12: DROPIN})
    yield ol
    hbrt.register_filters(ol.ref(), {VFR: None})
    hbrt.register_filters(ol.ref(), {k: None for k in REF})
    hbrt.register_filters(hip.filters(), {hbrt.FILTER_ID["crop_scale"]: None, 12: None})


@pytest.mark.parametrize("vfr", ["mode=0:rate=30000/1001", "mode=1:rate=90000/1001"], ids=["same_as_source", "constant_dup"])
def test_job_with_deblock_stays_one_device_run(job_filters, vfr):
    """[decomb 31, vfr, deblock medium, nlmeans, crop_scale, lapsharp] through the plugin surface: one upload / download
    pair around all six, and the pictures of the CPU job before deblock, the model, and the CPU job after it.  With vfr
    duplicating frames (one shared device picture) no picture is deblocked twice."""
    ol = job_filters
    F = hbrt.FILTER_ID
    TFF = 0x0008
    NLM = hip.NLMEANS_MEDIUM + ":threads=2"
    LAP = "y-strength=0.2:y-kernel=isolap:cb-strength=0.2:cb-kernel=isolap"
    st = dm.settings_for("medium")
    frames = synth.stream("interlaced", 320, 184, 9, cfg=3)
    filters = [(F["decomb"], "mode=31"), (VFR, vfr), (F["deblock"], st), (F["nlmeans"], NLM),
               (F["crop_scale"], "width=640:height=368"), (F["lapsharp"], LAP)]
    with hbrt.Job(filters, 320, 184, use_hip=True) as job:
        names = job.stages()
    assert names.count(UPN) == 1 and names.count(DOWNN) == 1 and names[0] == UPN and names[-1] == DOWNN
    assert "Deblock (HIP)" in names and len(names) == 8
    _, out = hbrt.run_job(filters, frames, flags=TFF, use_hip=True)
    _, mid = hbrt.run_job([(F["decomb"], "mode=31"), (VFR, vfr)], frames, flags=TFF, use_hip=False)
    deb = [dm.deblock_frame(m.planes, st, 8) for m in mid]
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
