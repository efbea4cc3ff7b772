"""tests/colour_model.py's float64 colour conversion with the chroma where the stream sites it: the up- and down-sampling
of a subsampled direction co-sited or centred (the forms of include/hbhip.h: hbhip_colorspace_create_sited), around
colour_model.Conversion's (or colour_model_wide.Conversion's) own convert_444.  Plain float64 sums; nothing here follows
the order of operations of the checker or of the kernel.  Also the frames and the cases the sited tests share."""
import numpy as np

import chroma_siting_model as csm
import colour_model as cm
import colour_model_wide as cmw


def _taps_up(n_out, n_in, cosited):
    """(near index, far index, far weight) of every output position of one direction"""
    i = np.arange(n_out)
    k = i >> 1
    if cosited:
        return k, cm._rep(n_in, k + 1), np.where(i & 1, 0.5, 0.0)
    return k, np.where(i & 1, cm._rep(n_in, k + 1), cm._rep(n_in, k - 1)), np.full(n_out, 0.25)


def upsample(c, w, h, subw, subh, h_centred=False, v_cosited=False):
    """chroma plane -> luma grid.  co-sited: 2k: c[k], 2k + 1: (c[k] + c[k+1]) / 2; centred: 2k: c[k-1] / 4 + 3 c[k] / 4,
    2k + 1: 3 c[k] / 4 + c[k+1] / 4; edges repeat"""
    c = np.asarray(c, np.float64)
    if subh:
        near, far, wf = _taps_up(h, c.shape[0], v_cosited)
        c = (1 - wf)[:, None] * c[near] + wf[:, None] * c[far]
    if subw:
        near, far, wf = _taps_up(w, c.shape[1], not h_centred)
        c = (1 - wf)[None, :] * c[:, near] + wf[None, :] * c[:, far]
    return c


def _taps_down(cosited):
    return ((0.25, -1), (0.5, 0), (0.25, 1)) if cosited else ((0.125, -1), (0.375, 0), (0.375, 1), (0.125, 2))


def downsample(o, subw, subh, h_centred=False, v_cosited=False, combine=None):
    """luma grid -> chroma plane.  co-sited: 2k - 1 .. 2k + 1 with 1/4 1/2 1/4; centred: 2k - 1 .. 2k + 2 with 1/8 3/8 3/8
    1/8; edges repeat.  combine as colour_model.downsample's"""
    combine = combine or (lambda terms: sum(wt * a for wt, a in terms))
    h, w = o.shape
    if subh:
        r = 2 * np.arange((h + 1) >> 1)
        o = combine([(wt, o[cm._rep(h, r + d)]) for wt, d in _taps_down(v_cosited)])
    if subw:
        c = 2 * np.arange((w + 1) >> 1)
        o = combine([(wt, o[:, cm._rep(w, c + d)]) for wt, d in _taps_down(not h_centred)])
    return o


def convert(conv, frame, subw, subh, h_centred=False, v_cosited=False):
    """colour_model.Conversion.convert with the sited resamplers -> colour_model.Result"""
    hc, vc = bool(h_centred and subw), bool(v_cosited and subh)
    y = np.asarray(frame[0], np.float64)
    h, w = y.shape
    u, v = (upsample(p, w, h, subw, subh, hc, vc) for p in frame[1:])
    out, in_gamut, finite, spread = conv.convert_444_rows(y, u, v, not (subw or subh))
    every = lambda t: np.logical_and.reduce([a for _, a in t])
    value, ig, fin, spr = [out[0]], [in_gamut], [finite[0]], [spread[0]]
    for k in (1, 2):
        value.append(downsample(out[k], subw, subh, hc, vc))
        ig.append(downsample(in_gamut, subw, subh, hc, vc, every))
        fin.append(downsample(finite[k], subw, subh, hc, vc, every))
        spr.append(downsample(spread[k], subw, subh, hc, vc))
    planes = []
    for val, f in zip(value, fin):
        q = np.clip(np.rint(np.where(f, val, 0.0)), 0, conv.vmax)
        planes.append(q.astype(np.uint8 if conv.depth == 8 else np.uint16))
    return cm.Result(tuple(planes), tuple(value), tuple(ig), tuple(fin), tuple(spr))


# ---- what the sited tests run ----------------------------------------------------------------------------------------
_CM = {c[0]: c for c in cm.CASES}
# (case, model class, depths): no linearisation; a primaries change; the HDR10 -> BT.709 tone mapping; constant luminance
CONVERSIONS = {"709_full": (_CM["709_full"], cm.Conversion, (8, 10)),
               "601_709": (_CM["601_709"], cm.Conversion, (8,)),
               "pq_709_hable": (_CM["pq_709_hable"], cm.Conversion, (10,)),
               "cl_nc": (cmw.BY_ID["cl_nc"], cmw.Conversion, (8, 10))}
LAYOUTS = {"420": ("2x2", (1, 1)), "422": ("2x1", (1, 0))}
SITINGS = {"709_full": (("420", 2), ("420", 3)), "cl_nc": (("420", 2), ("420", 3)),
           "601_709": (("420", 2), ("420", 3), ("420", 4), ("422", 2)),
           "pq_709_hable": (("420", 2), ("420", 3), ("420", 4), ("422", 2))}
FRAMES = ("columns", "rows", "random", "tiny")
CASES = [(cid, depth, lay, loc) for cid in CONVERSIONS for depth in CONVERSIONS[cid][2] for lay, loc in SITINGS[cid]]
YSTEP = {8: 4, 10: 16}


def has_oracle(cid):
    return CONVERSIONS[cid][1] is cm.Conversion          # the constant-luminance matrices have the model only


def hdr_source(cid):
    return cmw.hdr_source(CONVERSIONS[cid][0][1])


def conversion(cid, depth):
    case, cls, _ = CONVERSIONS[cid]
    return cls(case[1], case[3], depth, **case[4])


def _moderate(depth, luma, cb, cr):
    dt, s = (np.uint8 if depth == 8 else np.uint16), depth - 8
    return (luma << s).astype(dt), (cb << s).astype(dt), (cr << s).astype(dt)


def frame(name, depth, layout):
    """columns: colour_model.lattice_frame - chroma changes along the rows' direction only, which shows the horizontal
    siting and is blind to the vertical one.  rows: the same laid down the rows (transposed), for the vertical siting.
    random: 130 x 70, a tile and a remainder in both directions, both sides' edges; moderately saturated noise around
    the grey axis (the model's caps need a frame mostly in gamut), every chroma sample unlike its neighbours.
    tiny: 6 x 4, every tap of every sample clamped at an edge."""
    subw, subh = LAYOUTS[layout][1]
    if name == "columns":
        return cm.lattice_frame(depth, ystep=YSTEP[depth], sub=(subw, subh))
    if name == "rows":
        return tuple(np.ascontiguousarray(p.T) for p in cm.lattice_frame(depth, ystep=YSTEP[depth], sub=(subh, subw)))
    w, h = (130, 70) if name == "random" else (6, 4)
    rng = np.random.default_rng(20 + depth + 7 * (name == "tiny") + subh)
    cw, ch = (w + subw) >> subw, (h + subh) >> subh
    return _moderate(depth, rng.integers(48, 191, (h, w)), rng.integers(104, 153, (ch, cw)), rng.integers(104, 153, (ch, cw)))


_results = {}


def result(cid, depth, layout, loc, name):
    """the sited model's Result of a case on a frame, computed once and shared (never written to)"""
    key = (cid, depth, layout, loc, name)
    if key not in _results:
        hc, vc = csm.colour_forms(loc)
        _results[key] = convert(conversion(cid, depth), frame(name, depth, layout), *LAYOUTS[layout][1], hc, vc)
    return _results[key]
