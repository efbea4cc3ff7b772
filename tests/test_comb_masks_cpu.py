"""CPU: the comb-detect case list of tests/comb_cases.py cannot go vacuous.  With the oracle alone (ol.OrcComb and
orc_comb_mask): every size / configuration pair puts expected ones on the cells where the kernels of
csrc/comb_detect.hip have their edges - detector columns 0 and w - 1 (the last partial dword), rows 2 and h - 3, the
first column and the first and last rows the mask passes can set, column w - 1 where the mask stride equals the width -
and every knife-edge block score yields the verdicts it is meant to.  Where oracle/_ref is present, three sizes of the
same content also go through the reference itself (one segment thread, mask-only overlay): the oracle's masks on this
content are the reference's."""
import numpy as np
import pytest

from handbrake_amd import hbrt
import comb_cases as cc
import oracle_lib as ol
import oracle_stream as os_

TFF = 0x0008


def oracle_masks(oc, h):
    """the oracle's three masks (0 detector, 1 filtered, 2 intermediate), each the whole height x stride buffer"""
    lib = ol.oracle()
    lib.orc_comb_mask.restype = ol.C.POINTER(ol.C.c_uint8)
    lib.orc_comb_mask.argtypes = [ol.C.c_void_p, ol.C.c_int, ol.C.POINTER(ol.C.c_int)]
    st = ol.C.c_int()
    return [np.ctypeslib.as_array(lib.orc_comb_mask(oc.h, which, ol.C.byref(st)), shape=(h, st.value)).copy()
            for which in range(3)]


def oracle_case(w, h, cfg, depth=8):
    """[(verdict, masks)] of the classifications of a case, on one oracle instance"""
    oc = ol.OrcComb(w, h, depth=depth, **cfg["par"])
    try:
        out = []
        for (p, c, n), force in cc.case_lumas(w, h, cfg, depth):
            v = oc.classify(p, c, n, force)
            out.append((v, oracle_masks(oc, h)))
        return out
    finally:
        oc.close()


def settable_cells(w, h, cfg, depth=8):
    """The cells of the filtered mask the pass order can set, from the oracle's own passes: those it sets when the
    detector's mask is full (rows 2 .. h - 3, every column).  The passes are monotone - a triple AND, an erosion, a
    dilation - so no other detector mask sets a cell that this one leaves empty."""
    par = dict(cfg["par"], mode=cfg["par"]["mode"] & 2, spatial_metric=2, motion_thresh=0, spatial_thresh=3)
    v = (128 + 50 * cc._parity(w, h, 0)) << (depth - 8)
    v = v.astype(np.uint8 if depth == 8 else np.uint16)
    oc = ol.OrcComb(w, h, depth=depth, **par)
    try:
        oc.classify(v, v, v, True)
        m = oracle_masks(oc, h)
    finally:
        oc.close()
    assert m[0][2:h - 2, :w].all() and not m[0][:2].any() and not m[0][h - 2:].any()
    return m[1]


def settable_rows(w, h, cfg):
    return [y for y in range(h) if settable_cells(w, h, cfg)[y].any()]


def coverage_gaps(w, h, cfg):
    """what a size / configuration pair's expected masks (of its last classification) fail to reach: [] when nothing"""
    steps = oracle_case(w, h, cfg)
    m2 = steps[-1][1]
    det, gaps = m2[0], []
    if not det[:, 0].any(): gaps.append("detector column 0")
    if not det[:, w - 1].any(): gaps.append("detector column w - 1")
    if w % 4 and not det[:, w // 4 * 4:w].any(): gaps.append("the last partial dword")
    if not det[2, :w].any(): gaps.append("detector row 2")
    if not det[h - 3, :w].any(): gaps.append("detector row h - 3")
    if det[:, w:].any() or det[:2].any() or det[h - 2:].any(): gaps.append("ones outside the detector's rows and columns")
    if not any((a[1][0] > b[1][0]).any() for a, b in zip(steps, steps[1:])): gaps.append("no classification has a cell to clear")
    if cc.filtered(cfg) and cfg["par"]["filter_mode"] in (1, 2):
        can, f = settable_cells(w, h, cfg), m2[1]
        if (f > can).any(): gaps.append("a cell the full mask does not set")
        rows = [y for y in range(h) if can[y].any()]
        if rows and not (f[rows[0]].any() and f[rows[-1]].any()): gaps.append(f"filtered rows {rows[0]}, {rows[-1]}")
        if can[:, 2].any() and not f[:, 2].any(): gaps.append("filtered column 2")
        if can[:, :2].any() or can[0].any() or can[h - 1].any() or can[:, w:].any(): gaps.append("a cell no pass writes")
    return gaps


@pytest.mark.parametrize("w", cc.WIDTHS)
def test_every_pair_reaches_the_edges(built, w):
    for h in cc.heights_of(w):
        for cfg in cc.CONFIGS:
            assert coverage_gaps(w, h, cfg) == [], (w, h, cfg["name"])


def test_settable_rows_are_not_the_rows_a_pass_walks(built):
    """rows 0 and 1 of the detector's mask are zero, so the passes (which walk rows 1 .. h - 2) cannot set them all"""
    f2 = next(c for c in cc.CONFIGS if c["name"] == "gamma_f2_16x16")
    f1 = next(c for c in cc.CONFIGS if c["name"] == "gamma_f1_8x8")
    rows2, rows1 = settable_rows(67, 21, f2), settable_rows(67, 21, f1)
    assert rows1 == list(range(2, 19))
    assert rows2 and rows2[0] > 1 and rows2[-1] < 19 and rows2 == list(range(rows2[0], rows2[-1] + 1))
    assert settable_rows(64, 5, f2) == []
    assert not settable_cells(64, 7, f2)[:, 2].any() and settable_cells(64, 8, f2)[:, 2].any()


def test_column_w_minus_1_where_the_stride_is_the_width(built):
    """the passes read column `width` for it: the next row's column 0 when the rows are packed"""
    for w in (64, 128, 192, 320):
        assert cc.mask_stride(w) == w
        hit = 0
        for h in cc.heights_of(w):
            for cfg in cc.CONFIGS:
                if cc.filtered(cfg) and cfg["par"]["filter_mode"] in (1, 2):
                    hit += int(oracle_case(w, h, cfg)[-1][1][1][:, w - 1].any())
        assert hit, w
    for w in (63, 67, 130):                                  # ... and the zero padding otherwise: nothing can set it
        for cfg in cc.CONFIGS:
            if cc.filtered(cfg):
                assert not oracle_case(w, 21, cfg)[-1][1][1][:, w - 1].any()


def test_threshold_content_straddles_the_thresholds(built):
    """comb_threshold's detector density lies between 0.2 and 0.9 for every metric it is used with (and the first
    classification of such a case, which has no motion, is filled by force_exhaustive alone)"""
    seen = set()
    for cfg in cc.CONFIGS:
        if cfg["first"] != "threshold":
            continue
        seen.add((cfg["par"]["mode"] & 1, cfg["par"].get("spatial_metric", 2)))
        for depth in (8, 10, 12) if cfg["deep"] else (8,):
            for w, h in [(67, 21), (130, 21), (320, 35)] if depth == 8 else [(67, 21), (130, 21)]:
                oc = ol.OrcComb(w, h, depth=depth, **cfg["par"])
                a = cc.comb_threshold(w, h, 3, cc.seed_of(w, h, cfg), depth, cfg["par"]["spatial_thresh"])
                oc.classify(a[0], a[1], a[2], False)
                d = oracle_masks(oc, h)[0][2:h - 2, :w].mean()
                oc.classify(a[0], a[0], a[1], True)
                forced = oracle_masks(oc, h)[0][2:h - 2, :w].mean()
                oc.classify(a[0], a[0], a[1], False)
                unforced = oracle_masks(oc, h)[0][2:h - 2, :w].mean()
                oc.close()
                assert 0.2 < d < 0.9, (cfg["name"], depth, w, h, d)
                assert 0.2 < forced < 0.9, (cfg["name"], depth, w, h, forced)
                if cfg["par"]["motion_thresh"] > 0:
                    assert unforced == 0, (cfg["name"], depth, w, h)
    assert seen == {(1, 2), (0, 1), (0, 2)}


def knife_scores(k):
    """(S, the three block thresholds) of a knife-edge case, S from the oracle's mask in numpy"""
    lumas = cc.comb_patch(k["w"], k["h"], 3, 77, 8, k["rect"])
    filt = bool(k["par"]["mode"] & 2)
    oc = ol.OrcComb(k["w"], k["h"], block_thresh=1 << 20, **k["par"])
    assert oc.classify(lumas[0], lumas[1], lumas[2], False) == 0
    m = oracle_masks(oc, k["h"])
    oc.close()
    s = cc.block_score(m[1 if filt else 0], k["rect"], k["w"], filt)
    return lumas, s, (s - 1, s, 2 * s + 2)


def test_knife_edge_scores(built):
    cases = cc.knife_cases()
    assert {k["want"] for k in cases} == {(2, 1, 0), (0, 0, 0)}
    for k in cases:
        lumas, s, thr = knife_scores(k)
        assert s >= 8, (k["name"], s)
        got = []
        for t in thr:
            oc = ol.OrcComb(k["w"], k["h"], block_thresh=t, **k["par"])
            got.append(oc.classify(lumas[0], lumas[1], lumas[2], False))
            oc.close()
        assert tuple(got) == k["want"], (k["name"], s, got)


@pytest.fixture()
def one_thread():
    rt = hbrt.runtime()
    rt.hbhip_set_cpu_count(1)
    yield
    rt.hbhip_set_cpu_count(0)


def _settings(par):
    names = dict(mode="mode", spatial_metric="spatial-metric", motion_thresh="motion-thresh", spatial_thresh="spatial-thresh",
                 filter_mode="filter-mode", block_thresh="block-thresh", block_width="block-width", block_height="block-height")
    return ":".join(f"{names[k]}={v}" for k, v in par.items())


@pytest.mark.parametrize("w,h", [(67, 21), (64, 35), (130, 21)])
@pytest.mark.parametrize("depth", [8, 10])
def test_masks_on_this_content_are_the_reference_s(built, one_thread, w, h, depth):
    """The reference draws what its mask holds with mode 4 (mask only) added: luma = the mask the score read, plus the
    box.  Through test_comb_overlay_cpu.py's comparison, on comb_field and comb_threshold streams."""
    if ol.ref() is None:
        pytest.skip("oracle/_ref not built")
    half = 1 << (depth - 1)
    cw, ch = (w + 1) // 2, (h + 1) // 2
    dt = np.uint8 if depth == 8 else np.uint16
    for cfg in cc.CONFIGS if depth == 8 else cc.DEEP_CONFIGS:
        par = dict(cfg["par"], mode=cfg["par"]["mode"] | 4, block_thresh=2)
        s = cc.seed_of(w, h, cfg)
        lumas = cc.comb_field(w, h, 3, s, depth) + cc.comb_threshold(w, h, 3, s, depth, par["spatial_thresh"])
        frames = [(y, np.full((ch, cw), half, dt), np.full((ch, cw), half, dt)) for y in lumas]
        got = hbrt.run_stream(ol.ref(), [("hb_filter_comb_detect", _settings(par))], frames, flags=TFF,
                              pix_fmt=hbrt.PIX_FMT_FOR_DEPTH[depth])
        want = os_.comb_detect_overlay_stream(frames, dict(par, depth=depth))
        assert [g.combed for g in got] == [c for c, _ in want], cfg["name"]
        if par.get("filter_mode", 2) != 0 or not par["mode"] & 2:          # (filter mode 0: the score reads an empty mask)
            assert any(c for c, _ in want), cfg["name"]
        for t, (c, planes) in enumerate(want):
            for p in range(3):
                np.testing.assert_array_equal(got[t].planes[p], planes[p], err_msg=f"{cfg['name']} frame {t} plane {p}")
