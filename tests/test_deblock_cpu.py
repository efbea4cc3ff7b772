"""CPU: the deblock model's two forms agree (tests/deblock_model.py), the settings resolve to the thresholds FFmpeg would
derive - in the model and in the drop-in's own C (hbhip_deblock_params_from_settings) - the drop-in declines what has no
defined result, and it is registered under the reference's id."""
import ctypes as C

import numpy as np
import pytest

import deblock_cases as dc
import deblock_model as dm
from handbrake_amd import hbrt, hip, synth


def _planes(kind, w, h, depth, seed):
    if kind == "blocky":
        return [synth.stream("blocky", w, h, 1, cfg=seed + k, depth=depth)[0][0] for k in range(2)]
    rng = np.random.default_rng(seed)
    maxv = (1 << depth) - 1
    # random but smooth enough that edges fire: a random walk of small steps around mid-grey
    base = rng.integers(-3, 4, size=(h, w)).cumsum(axis=1) // 4 + rng.integers(-2, 3, size=(h, 1))
    return [np.clip((maxv + 1) // 2 + base * (1 << (depth - 8)), 0, maxv).astype(np.uint8 if depth == 8 else np.uint16)]


@pytest.mark.parametrize("b", [4, 5, 6, 8, 16, 13])
@pytest.mark.parametrize("strong", [True, False])
@pytest.mark.parametrize("depth", [8, 10, 12])
def test_model_forms_agree(b, strong, depth):
    """the raster transcription and the block-row form give the same planes, on sizes that are and are not multiples
    of b (only sizes with a defined result: see plane_ok), and the edges fire often enough for that to mean something"""
    sizes = [(4 * b, 3 * b), (4 * b + 3, 3 * b + 4)]
    if not strong:
        sizes.append((5 * b + 2, 2 * b + 2))
    thr = dm.thresholds(20, depth)
    stats = {}
    for w, h in sizes:
        assert dm.plane_ok(w, b, strong) and dm.plane_ok(h, b, strong)
        for kind, seed in [("blocky", 13 + b), ("random", b * 7 + depth)]:
            for pl in _planes(kind, w, h, depth, seed):
                want = dm.deblock_plane_raster(pl, b, strong, thr, depth)
                got = dm.deblock_plane(pl, b, strong, thr, depth, stats)
                np.testing.assert_array_equal(got, want, err_msg=f"{kind} {w}x{h} b={b} strong={strong}")
    assert stats["fired"] > 0.15 * stats["edges"], stats


def _gpu_groups():
    groups = {}
    for b, strong, depth, thresh, w, h in dc.model_cases():
        groups.setdefault((b, strong, depth, thresh), []).append((w, h))
    return sorted(groups.items())


@pytest.mark.parametrize("key,sizes", _gpu_groups(), ids=lambda v: "-".join(map(str, v)) if isinstance(v[0], int) else f"{len(v)}sizes")
def test_model_forms_agree_on_the_gpu_cases(key, sizes):
    """the GPU tests compare against the block-row form, which rests on the same dependency argument as the kernels; this
    holds it to the literal raster transcription at every (b, strength, depth, thresh) they run, on their own plane sizes
    (tests/deblock_cases.py: large planes cut to three edges with the same remainder) - on blocky content, on near-flat
    content where nearly every edge fires, and at thresh=100 on near-white and near-black content where taps clip"""
    b, strong, depth, thresh = key
    thr = dm.thresholds(thresh, depth)
    stats = {}
    for w, h in sizes:
        planes = [synth.picture("blocky", w, h, 0, cfg=13 + b, depth=depth, chroma="1x1")[0], dc.near_flat(w, h, "1x1", depth, b)[0]]
        if thresh == 100:
            planes += [dc.near_white(w, h, "1x1", depth, b)[0], dc.near_white(w, h, "1x1", depth, b, mirror=True)[0]]
        for k, pl in enumerate(planes):
            want = dm.deblock_plane_raster(pl, b, strong, thr, depth)
            got = dm.deblock_plane(pl, b, strong, thr, depth, stats)
            np.testing.assert_array_equal(got, want, err_msg=f"content {k} {w}x{h} b={b} strong={strong} depth={depth}")
    if any(dc.edges(w, b) + dc.edges(h, b) for w, h in sizes):
        assert stats["fired"] > 0.15 * stats["edges"], stats


@pytest.mark.parametrize("preset", sorted(dm.PRESETS))
@pytest.mark.parametrize("b", [4, 8, 16])
def test_blocky_content_fires_and_skips(preset, b):
    """the blocky model makes every preset fire on many edges, and those up to `strong` skip many others (past
    thresh=50 nearly every step of 8-bit content is under the thresholds: that is what those presets are for)"""
    st = dm.resolve(dm.PRESETS[preset] + f":blocksize={b}", 8)
    stats = {}
    dm.deblock_plane(synth.stream("blocky", 192, 96, 1)[0][0], b, st["strong"], st["thr"], 8, stats)
    assert stats["fired"] > 0.2 * stats["edges"], stats
    if preset in ("ultralight", "light", "medium", "strong"):
        assert stats["fired"] < 0.97 * stats["edges"], stats


def test_overlapping_windows_chain():
    """strong b = 4: a vertical edge reads what the one before it wrote - filtering every edge from the unfiltered
    plane instead (what an elementwise kernel would do) gives a different picture, so the chain is real"""
    pl = synth.stream("blocky", 64, 48, 1, cfg=5)[0][0]
    thr = dm.thresholds(100, 8)
    want = dm.deblock_plane_raster(pl, 4, True, thr, 8)
    out = pl.astype(np.int64).copy()
    for x in range(4, 64, 4):
        out[0:4, x - 3:x + 3] = dm.edge(pl.astype(np.int64)[0:4, x - 3:x + 3], True, thr, 255)[0]
    assert not np.array_equal(out[0:4], want[0:4].astype(np.int64))


# ---- thresholds ------------------------------------------------------------------------------------------------------
# (ath, bth) per depth for the presets' thresholds and for `thresh` absent (FFmpeg's defaults); gth = dth = bth
PINNED = {8: {None: (24, 12), 20: (51, 25), 50: (127, 63), 75: (191, 95), 100: (255, 127)},
          10: {None: (100, 51), 20: (204, 102), 50: (511, 255), 75: (767, 383), 100: (1023, 511)},
          12: {None: (401, 204), 20: (819, 409), 50: (2047, 1023), 75: (3071, 1535), 100: (4095, 2047)}}


def _c_params(settings, depth, w=64, h=48, lcw=1, lch=1):
    F = hip.filters()
    F.hbhip_deblock_params_from_settings.restype = C.c_int
    F.hbhip_deblock_params_from_settings.argtypes = [C.c_char_p] + [C.c_int] * 5 + [C.POINTER(hip.DeblockParams)]
    p = hip.DeblockParams()
    rc = F.hbhip_deblock_params_from_settings(settings.encode(), depth, w, h, lcw, lch, C.byref(p))
    return rc, p


@pytest.mark.parametrize("depth", [8, 10, 12])
def test_preset_thresholds_are_pinned(depth):
    for t, (a, b) in PINNED[depth].items():
        assert dm.thresholds(t, depth) == (a, b, b, b), (depth, t)
    assert dm.thresholds(0, depth) == dm.thresholds(-1, depth) == dm.thresholds(None, depth)


@pytest.mark.parametrize("depth", [8, 10, 12])
def test_c_resolution_matches_the_model_for_every_thresh(built, depth):
    for t in [None] + list(range(1, 101)):
        st = "strength=weak" + ("" if t is None else f":thresh={t}")
        rc, p = _c_params(st, depth)
        assert rc == 0, st
        assert (p.ath, p.bth, p.gth, p.dth) == dm.thresholds(t, depth), (depth, t)
        assert (p.strong, p.block) == (0, 8)


@pytest.mark.parametrize("preset", sorted(dm.PRESETS))
@pytest.mark.parametrize("tune", sorted(dm.TUNES))
def test_presets_and_tunes_resolve(built, preset, tune):
    st = dm.settings_for(preset, tune)
    rc, p = _c_params(st, 8, 1920, 1080)
    want = dm.resolve(st, 8)
    assert rc == 0
    assert (bool(p.strong), p.block, (p.ath, p.bth, p.gth, p.dth)) == (want["strong"], want["block"], want["thr"])
    assert p.block == {"small": 4, "medium": 8, "large": 16}[tune]
    assert p.strong == (preset not in ("ultralight", "light"))


def test_defaults_are_ffmpegs(built):
    rc, p = _c_params("", 8)
    assert rc == 0 and (p.strong, p.block, p.ath, p.bth) == (1, 8, 24, 12)


DECLINED = [("strength=medium", 64, 48, 1, 1), ("blocksize=3", 64, 48, 1, 1), ("blocksize=513", 1024, 1024, 1, 1),
            ("thresh=101", 64, 48, 1, 1),
            ("strength=strong", 65, 48, 1, 1),       # luma width % 8 == 1
            ("strength=strong", 66, 48, 1, 1),       # luma % 8 == 2
            ("strength=strong", 68, 48, 1, 1),       # chroma width 34: % 8 == 2
            ("strength=weak", 64, 50, 0, 1)]         # chroma height 25: % 8 == 1
ACCEPTED = [("strength=weak", 70, 48, 1, 1), ("strength=weak", 66, 48, 0, 1), ("strength=strong", 64, 48, 1, 1), ("strength=strong", 70, 48, 1, 1),
            ("strength=strong:blocksize=16", 64, 36, 0, 0), ("strength=strong", 6, 6, 1, 1), ("thresh=100", 64, 48, 1, 1)]


@pytest.mark.parametrize("st,w,h,lcw,lch", DECLINED)
def test_declined_settings(built, st, w, h, lcw, lch):
    rc, _ = _c_params(st, 8, w, h, lcw, lch)
    assert rc != 0
    with pytest.raises(dm.Declined):
        cw, ch = -((-w) >> lcw), -((-h) >> lch)
        dm.resolve(st, 8, [(w, h), (cw, ch)])


@pytest.mark.parametrize("st,w,h,lcw,lch", ACCEPTED)
def test_accepted_settings(built, st, w, h, lcw, lch):
    rc, _ = _c_params(st, 8, w, h, lcw, lch)
    assert rc == 0
    dm.resolve(st, 8, [(w, h), (-((-w) >> lcw), -((-h) >> lch))])


def test_declined_init_fails_without_a_device(built, monkeypatch):
    """init() refuses declined settings before it looks for a device, so the refusal does not depend on one"""
    monkeypatch.setenv("HBHIP_FORCE_SWAP", "1")
    for st in ("strength=medium", "thresh=101", "blocksize=600"):
        with pytest.raises(RuntimeError):
            hbrt.Chain(hip.filters(), [("hb_filter_deblock_hip", st)], 64, 48)


def test_drop_in_registered_under_the_deblock_id(built):
    F = hip.filters()
    F.hbhip_filter_get.restype = C.c_void_p
    F.hbhip_filter_get.argtypes = [C.c_int]
    addr = C.addressof(C.c_char.in_dll(F, "hb_filter_deblock_hip"))
    assert C.c_int.in_dll(F, "hb_filter_deblock_hip").value == 12 == hbrt.FILTER_ID["deblock"]
    assert F.hbhip_filter_get(12) == addr
    assert hasattr(hip.lib(), "hbhip_deblock_create") and "hbhip_deblock_create" in hip.ABI_SYMBOLS
