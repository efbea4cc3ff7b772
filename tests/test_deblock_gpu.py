"""GPU: the deblock drop-in (csrc/deblock.hip, libhb/deblock_hip.c) is bit-exact with the numpy model
(tests/deblock_model.py) - every preset and tune, 8/10/12 bits, 4:2:0/4:2:2/4:4:4, the threshold boundaries, the forced
repair path of the strong b = 4 / 5 kernel, bursts - and inside a device-resident job between VFR and NLMeans."""
import ctypes as C

import numpy as np
import pytest

import deblock_model as dm
from handbrake_amd import hbrt, hip, synth

pytestmark = pytest.mark.gpu
DROPIN = "hb_filter_deblock_hip"
LCW = {"2x2": (1, 1), "2x1": (1, 0), "1x1": (0, 0)}


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


def _format_cases():
    out = []
    for w, h in [(638, 362), (1918, 1078), (64, 48)]:
        for sub in ("2x2", "2x1", "1x1"):
            for depth in (10, 12) if sub == "2x2" else (8, 10, 12):
                lcw, lch = LCW[sub]
                sizes = [(w, h), (-((-w) >> lcw), -((-h) >> lch))]
                for st in ("strength=weak:thresh=50", "strength=strong:thresh=20", "strength=strong:thresh=50:blocksize=16",
                           "strength=strong:thresh=75:blocksize=4", "strength=strong:thresh=20:blocksize=5"):
                    if w > 1000 and "blocksize=16" not in st:
                        continue                  # (the large size: one case per layout keeps the numpy model's time down)
                    try:
                        dm.resolve(st, depth, sizes)
                    except dm.Declined:
                        continue
                    out.append((w, h, sub, depth, st))
    return out


@pytest.mark.parametrize("w,h,sub,depth,st", _format_cases())
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


# ---- the C ABI directly: bursts and the repair path ------------------------------------------------------------------
def _make(ctx, settings, w, h):
    p = hip.DeblockParams()
    F = hip.filters()
    F.hbhip_deblock_params_from_settings.argtypes = [C.c_char_p] + [C.c_int] * 5 + [C.POINTER(hip.DeblockParams)]
    assert F.hbhip_deblock_params_from_settings(settings.encode(), 8, w, h, 1, 1, C.byref(p)) == 0
    return hip._create("hbhip_deblock_create", ctx, [C.c_void_p, C.POINTER(hip.DeblockParams)] + [C.c_int] * 5 + [C.POINTER(C.c_void_p)],
                       ctx.h, C.byref(p), w, h, 8, 1, 1)


def _bursts(settings, frames, sizes, warmup=None):
    """frames through one filter in device-resident bursts of the given sizes (one process_dev call each)"""
    import torch
    h, w = frames[0][0].shape
    ctx = hip.Ctx(0)
    flt = _make(ctx, settings, w, h)
    out = []
    try:
        if warmup is not None:
            hip.lib().hbhip_deblock_set_warmup.argtypes = [C.c_void_p, C.c_int]
            assert hip.lib().hbhip_deblock_set_warmup(flt.h, warmup) == 0
        at = 0
        for n in sizes:
            part = frames[at:at + n]
            at += n
            dev_in = [[torch.from_numpy(np.ascontiguousarray(p)).cuda() for p in f] for f in part]
            outs = [[torch.full(p.shape, 7, dtype=torch.uint8, device="cuda") for p in f] for f in part]
            torch.cuda.synchronize()
            arr_in = (hip.DevFrame * n)(*[hip.dev_frame(f) for f in dev_in])
            arr_out = (hip.DevFrame * n)(*[hip.dev_frame(o) for o in outs])
            assert flt.process_dev(arr_in, 0, arr_out) == n
            ctx.sync()
            out += [[p.cpu().numpy() for p in o] for o in outs]
            for f, d in zip(part, dev_in):                               # out of place: the inputs are untouched
                for c in range(3):
                    np.testing.assert_array_equal(d[c].cpu().numpy(), f[c])
        return out
    finally:
        flt.close()
        ctx.close()


@pytest.mark.parametrize("st", ["strength=strong:thresh=20", "strength=weak:thresh=20",
                                "strength=strong:thresh=50:blocksize=4", "strength=strong:thresh=20:blocksize=5"])
def test_bursts_equal_frame_by_frame(built, st):
    frames = synth.stream("blocky", 320, 200, 20)
    want = model(frames, st)
    check(_bursts(st, frames, [1, 3, 16]), want, "bursts 1/3/16")
    check(_bursts(st, frames, [1] * 20), want, "frame by frame")


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
