"""The `format` filter's chroma down-sampling (4:2:2 -> 4:2:0, 4:4:4 -> 4:2:2, 4:4:4 -> 4:2:0 at equal depth), twice:

* resample_frame(): the INTEGER model - what libavfilter's auto-inserted `scale` computes for such a pair, libswscale's
  general scaler at its default flags (bicubic, B = 0, C = 0.6), restated here from the definition: initFilter's integer
  cubic, its trimming / edge folding / normalisation to 14-bit (horizontal) and 12-bit (vertical) coefficients, then
  hScale8To15 / hScale16To15 and yuv2planeX_8 / _10 / _12.  Luma runs through identity filters and is a copy.  PARITY
  UNPINNED: libswscale is not in the reference tree, this file is the definition the GPU tests hold the kernel to
  (tolerance 0).  It shares no code with handbrake_amd/csrc.
* resample_frame_f64(): the float64 model - a Keys cubic (a = -0.6) stretched by the size ratio, weights normalised,
  edges replicated, one rounding at the end.  What the integer model is held to (test_format_resample_cpu.py).

Siting (both models): target row j lies at source row (j + 1/2) * r - 1/2, midway between rows 2j and 2j + 1 at r = 2;
target column i lies at source column (i + 1/4) * r - 1/2, ON source column 2i at r = 2 (left-sited chroma, whatever
chroma_location says: the crop/scale drop-in's rule).  r = source size / target size is 2 except for an odd source size
(then 2 - 1 / target size)."""
import numpy as np

# Measured by tests/test_format_resample_cpu.py::test_integer_model_against_float64 (and asserted there): the largest
# |integer - float64| by depth over its inputs, and the largest share of samples of one plane that differ at all.
# 1 code value is the two roundings; 12 bits get 2 because the vertical coefficients have 12 bits as well: the row at phase
# 1/2, (-58 -172 492 1786 1786 492 -172 -58) / 4096, is off the cubic by 0.4 + 0.8 + 0.8 + 0.4 twice = 4.8 / 4096 in
# absolute sum, up to 4.8 code values of a 12-bit sample on content that lines up with the signs (1.2 at 10 bits, 0.3 at
# 8); full-scale noise reaches 2 and differs by 1 in 38 % of the samples.
ALLOW_MAX_ABS = {8: 1, 10: 1, 12: 2}
ALLOW_SHARE = 0.39
# Full-scale noise through BOTH passes, against the float model as it stands: the 15-bit intermediate saturates
# (min(val >> sh, 32767): a horizontal overshoot above full scale is clipped BEFORE the vertical pass, where the float
# model clips once at the end).  With the same clip between the float model's passes the figures above hold again:
# test_intermediate_saturation_is_the_only_larger_difference measures both.
ALLOW_MAX_ABS_UNSATURATED = {8: 1, 10: 17, 12: 1}

SUB = {"420": (1, 1), "422": (1, 0), "444": (0, 0)}
PAIRS = (("422", "420"), ("444", "422"), ("444", "420"))


def _tdiv(a: int, b: int) -> int:
    """C's integer division (towards zero)"""
    q = abs(a) // abs(b)
    return q if (a < 0) == (b < 0) else -q


def _rounded_div(a: int, b: int) -> int:
    return _tdiv(a + (b >> 1), b) if a >= 0 else _tdiv(a - (b >> 1), b)


def sws_bicubic_table(src: int, dst: int, one: int, src_pos: int, dst_pos: int):
    """(positions, coefficient rows, taps) of one dimension: libswscale utils.c:initFilter for SWS_BICUBIC at the
    default parameters.  Row i taps source samples pos[i] .. pos[i] + taps - 1."""
    ratio_log2 = max(src // dst, 1).bit_length() - 1
    fone = 1 << (54 - min(ratio_log2, 8))
    x_inc = ((src << 16) + (dst >> 1)) // dst
    if abs(x_inc - 0x10000) < 10 and src_pos == dst_pos:
        return list(range(dst)), [[one]] * dst, 1
    size = 1 + 4 if x_inc <= (1 << 16) else 1 + (4 * src + dst - 1) // dst
    size = max(min(size, src - 2), 1)
    B, C = 0, int(0.6 * (1 << 24))
    rows, pos = [], []
    x_dst_in_src = ((dst_pos * x_inc) >> 7) - ((src_pos * 0x10000) >> 7)
    for i in range(dst):
        xx = _tdiv(x_dst_in_src - (size - 2) * (1 << 16), 1 << 17)
        pos.append(xx)
        row = []
        for j in range(size):
            d = abs(xx * (1 << 17) - x_dst_in_src) << 13
            if x_inc > (1 << 16):
                d = d * dst // src
            if d >= (1 << 31):
                c = 0
            else:
                dd = (d * d) >> 30
                ddd = (dd * d) >> 30
                if d < (1 << 30):
                    c = (12 * (1 << 24) - 9 * B - 6 * C) * ddd + (-18 * (1 << 24) + 12 * B + 6 * C) * dd + \
                        (6 * (1 << 24) - 2 * B) * (1 << 30)
                else:
                    c = (-B - 6 * C) * ddd + (6 * B + 30 * C) * dd + (-12 * B - 48 * C) * d + (8 * B + 24 * C) * (1 << 30)
            row.append(_tdiv(c, (1 << 54) // fone))
            xx += 1
        rows.append(row)
        x_dst_in_src += 2 * x_inc
    # trim what is near zero: at the front by moving the row, at the back by shortening every row to the longest need
    cut = 0.002 * fone
    min_size = 0
    for i in range(dst - 1, -1, -1):
        row = rows[i]
        cut_off = 0
        for _ in range(size):
            cut_off += abs(row[0])
            if cut_off > cut:
                break
            if i < dst - 1 and pos[i] >= pos[i + 1]:
                break
            row[:] = row[1:] + [0]
            pos[i] += 1
        cut_off, mn = 0, size
        for j in range(size - 1, 0, -1):
            cut_off += abs(row[j])
            if cut_off > cut:
                break
            mn -= 1
        min_size = max(min_size, mn)
    taps = min_size
    rows = [r[:taps] for r in rows]
    # taps outside the plane fold onto the edge sample
    for i in range(dst):
        row = rows[i]
        if pos[i] < 0:
            for j in range(1, taps):
                left = max(j + pos[i], 0)
                row[left] += row[j]
                row[j] = 0
            pos[i] = 0
        if pos[i] + taps > src:
            shift = pos[i] + min(taps - src, 0)
            acc = 0
            for j in range(taps - 1, -1, -1):
                if pos[i] + j >= src:
                    acc += row[j]
                    row[j] = 0
            for j in range(taps - 1, -1, -1):
                row[j] = 0 if j < shift else row[j - shift]
            pos[i] -= shift
            row[src - 1 - pos[i]] += acc
    # normalise to `one`, the rounding error carried along the row
    out = []
    for row in rows:
        total = _tdiv(sum(row) + one // 2, one) or 1
        error, q = 0, []
        for v in row:
            v += error
            iv = _rounded_div(v, total)
            q.append(iv)
            error = v - iv * total
        out.append(q)
    return pos, out, taps


def _apply(plane, pos, coef, taps, axis):
    """sum over the taps along `axis`, int64"""
    p = plane.astype(np.int64)
    if axis == 0:
        p = p.T
    idx = np.asarray(pos)[:, None] + np.arange(taps)[None, :]              # (dst, taps)
    acc = (p[:, idx] * np.asarray(coef, np.int64)[None, :, :]).sum(axis=2)
    return acc.T if axis == 0 else acc


def resample_plane(plane, depth: int, down_w: bool, down_h: bool):
    """one chroma plane through swscale's two passes; a pass that does not resample is the identity filter"""
    h, w = plane.shape
    dw, dh = (-(-w // 2) if down_w else w), (-(-h // 2) if down_h else h)
    # left-sited chroma: source position 128 (full resolution), target position 128 >> 1; vertically centred, 128 both
    px, qx, tx = sws_bicubic_table(w, dw, 1 << 14, 128, 64 if down_w else 128)
    py, qy, ty = sws_bicubic_table(h, dh, 1 << 12, 128, 128)
    hbuf = np.minimum(_apply(plane, px, qx, tx, 1) >> (7 if depth == 8 else depth - 1), (1 << 15) - 1)
    shift = 19 if depth == 8 else 27 - depth
    rnd = 64 << 12 if depth == 8 else 1 << (shift - 1)
    out = (_apply(hbuf, py, qy, ty, 0) + rnd) >> shift
    return np.clip(out, 0, (1 << depth) - 1).astype(plane.dtype)


def resample_frame(frame, depth: int, src: str, dst: str):
    """(Y, Cb, Cr) in layout `src` -> layout `dst` ("444" / "422" / "420")"""
    (sw, sh), (tw, th) = SUB[src], SUB[dst]
    assert tw >= sw and th >= sh and (tw, th) != (sw, sh)
    return (frame[0].copy(),) + tuple(resample_plane(p, depth, tw > sw, th > sh) for p in frame[1:])


# ---- float64 ------------------------------------------------------------------------------------------------------------
def keys_cubic(x, a=-0.6):
    x = np.abs(x)
    return np.where(x <= 1, (a + 2) * x ** 3 - (a + 3) * x ** 2 + 1,
                    np.where(x < 2, a * x ** 3 - 5 * a * x ** 2 + 8 * a * x - 4 * a, 0.0))


def _resample_axis_f64(p, dst: int, offset: float, axis: int):
    src = p.shape[axis]
    r = src / dst
    centre = (np.arange(dst) + offset) * r - 0.5
    k = np.floor(centre)[:, None] + np.arange(-5, 7)[None, :]              # wider than the support of 2 r <= 4
    wgt = keys_cubic((k - centre[:, None]) / r)
    wgt /= wgt.sum(axis=1, keepdims=True)
    idx = np.clip(k, 0, src - 1).astype(np.int64)                           # edges replicated
    if axis == 1:
        return (p[:, idx] * wgt[None, :, :]).sum(axis=2)
    return (p.T[:, idx] * wgt[None, :, :]).sum(axis=2).T


def resample_plane_f64(plane, depth: int, down_w: bool, down_h: bool, saturate: bool = False):
    """saturate: clip the horizontal result where swscale's 15-bit intermediate does (32767 / 2 ** (15 - depth))"""
    p = plane.astype(np.float64)
    if down_w:
        p = _resample_axis_f64(p, -(-plane.shape[1] // 2), 0.25, 1)
        if saturate:
            p = np.minimum(p, 32767.0 / (1 << (15 - depth)))
    if down_h:
        p = _resample_axis_f64(p, -(-plane.shape[0] // 2), 0.5, 0)
    return np.clip(np.floor(p + 0.5), 0, (1 << depth) - 1).astype(plane.dtype)


def resample_frame_f64(frame, depth: int, src: str, dst: str):
    (sw, sh), (tw, th) = SUB[src], SUB[dst]
    return (frame[0].copy(),) + tuple(resample_plane_f64(p, depth, tw > sw, th > sh) for p in frame[1:])


# ---- inputs -----------------------------------------------------------------------------------------------------------------
def frame(kind: str, w: int, h: int, t: int, depth: int, layout: str):
    """a (Y, Cb, Cr) frame in layout "444" / "422" / "420": synth's `progressive` / `banded` pictures, `random` (every
    sample drawn from the LCG over the whole range), `flat`, `rows` (rows alternating 0 and full scale) and `bars` (four
    rows / columns of 0, four of full scale: every positive tap on one level, the negative lobes on the other)"""
    from handbrake_amd import synth
    lcw, lch = SUB[layout]
    cw, ch = -((-w) >> lcw), -((-h) >> lch)
    full = (1 << depth) - 1
    dt = np.uint8 if depth == 8 else np.uint16
    if kind in ("progressive", "banded"):
        chroma = {"444": "1x1", "422": "2x1", "420": "2x2"}[layout]
        return synth.picture(kind, w, h, t, cfg=2 if kind == "progressive" else 17, depth=depth, chroma=chroma)
    if kind == "random":
        v = synth.lcg_stream(synth.frame_seed(0x3d, t + 16 * depth), w * h + 2 * cw * ch)
        v = ((v >> np.uint32(32 - depth)) & np.uint32(full)).astype(dt)
        return (v[:w * h].reshape(h, w).copy(), v[w * h:w * h + cw * ch].reshape(ch, cw).copy(),
                v[w * h + cw * ch:].reshape(ch, cw).copy())
    if kind == "flat":
        return tuple(np.full(s, val, dt) for s, val in (((h, w), full // 3), ((ch, cw), full), ((ch, cw), 1 + t)))
    if kind == "rows":
        def rows(n, m, first):
            return np.repeat((((np.arange(n) + first) & 1) * full).astype(dt)[:, None], m, axis=1)
        return (rows(h, w, 0), rows(ch, cw, t & 1), rows(ch, cw, 1 - (t & 1)))
    if kind == "bars":
        def bars(n, m, first):
            gy, gx = np.arange(n)[:, None] + 4 * first, np.arange(m)[None, :]
            return ((((gy >> 2) ^ (gx >> 2)) & 1) * full).astype(dt)
        return (bars(h, w, 0), bars(ch, cw, t & 1), bars(ch, cw, 1 - (t & 1)))
    raise ValueError(kind)
