"""The float64 colour model (tests/colour_model.py) extended to the matrices that are no plain Kr / Kb matrix:
bt2020c (10) and chroma-derived-c (13), constant luminance; chroma-derived-nc (12), Kr / Kb from the primaries; ictcp
(14), BT.2100's ICtCp in its PQ and its HLG form.  numpy only, float64 throughout, every constant derived below from
BT.2020, BT.2100 or H.273, nothing read from the kernel (handbrake_amd/csrc/colorspace.hip).  oracle/ refuses these
ids, so this model is all the new paths are held to (tests/test_colorspace_wide_gpu.py), besides the bit-for-bit
agreement of the filter's own two entry points.

The reference hands these ids to zscale (libhb/colorspace.c:108-112, 180-182); zimg is not in the reference tree, so
what it does is stated FROM MEMORY and parity stays unpinned.  The choices, which the kernel follows too:

  choice                                  | model                                   | reason
  ----------------------------------------+-----------------------------------------+---------------------------------
  where CL and ICtCp meet other matrices  | in linear light only: CL(T) <-> linear  | zimg's graph has no edge between
                                          | RGB, ICtCp(T) <-> L'M'S'(T) <-> LMS <-> | CL / ICtCp and a gamma-domain
                                          | RGB; linear light forced for 10, 13, 14 | node (from memory)
  CL chroma scales Pb Nb Pr Nr            | 1 - OETF(Kb), OETF(1 - Kb), 1 -         | BT.2020 table 4 (0.7910, 0.9702,
                                          | OETF(Kr), OETF(1 - Kr), BT.2020's OETF  | 0.4969, 0.8591); fixed whatever
                                          | with the exact alpha and beta           | transfer the stream signals
  CL transfer functions                   | the side's own, display referred as     | zimg's set, as for every other
                                          | every other path (cm.to_linear / gamma) | path (from memory)
  CL and chroma-derived-c primaries       | BT.2020 only; otherwise not covered     | zimg has no path (from memory)
  chroma-derived-nc Kr, Kb                | the standard's rounded pair on BT.709 / | H.273: derived from the primaries;
                                          | BT.2020 primaries, else the Y row of    | for 709 / 2020 the named matrix
                                          | RGB -> XYZ                              | is that derivation, rounded
  ICtCp                                   | BT.2020 primaries and PQ or HLG only;   | BT.2100 tables 7 and 8
                                          | I Ct Cp in the Y Cb Cr slots and code   |
                                          | ranges                                  |
  HLG OOTF on ICtCp                       | 1.2 power on each of L, M, S            | the filter's HLG pair is per
                                          |                                         | component (zimg's arib_b67)
  npl scale, tone mapping, gamut matrix   | on linear RGB, as in colour_model.py    | unchanged stages
  CL chroma on the way out                | division by 2 Pb / 2 Nb ...; the kernel | a multiplication by the host's
                                          | multiplies by the rounded reciprocal    | float reciprocal: 1 ulp apart
  in gamut                                | the source's linear RGB inside [0, 1]   | R'G'B' does not exist on a CL or
                                          |                                         | an ICtCp source

The conditioning box of colour_model.Conversion.convert_444 is extended to the new intermediates: the three values
that enter the transfer functions ((R', Y', B') or L'M'S') move by +-PERTURBATION_SOURCE relative, the three that leave
them ((R, Yl, B) or LMS) by +-PERTURBATION relative, and the output of each new 3 x 3 (to linear RGB on the way in, to
(R, Yl, B) / LMS on the way out) by +-PERTURBATION of sum_j |m_ij| |c_j|: the bound of a single-precision dot
product's error, which cancellation (G = (Yl - Kr R - Kb B) / Kg) leaves large against the result.
"""
import numpy as np

import colour_model as cm

CL, ICTCP = "cl", "ictcp"
KR2020, KB2020 = cm.KR_KB[9]


def matrix_form(m):
    return CL if m in (10, 13) else ICTCP if m == 14 else None


# ---- BT.2020 table 4: the OETF with the exact alpha, beta (the curve and its slope continuous at beta) -----------
def _bt2020_alpha_beta():
    # 4.5 b = a b^0.45 - (a - 1) and 4.5 = 0.45 a b^-0.55  =>  a = 10 b^0.55,  5.5 b - 10 b^0.55 + 1 = 0
    lo, hi = 0.01, 0.03
    for _ in range(200):
        mid = 0.5 * (lo + hi)
        if 5.5 * mid - 10 * mid ** 0.55 + 1 > 0:
            lo = mid
        else:
            hi = mid
    b = 0.5 * (lo + hi)
    return 10 * b ** 0.55, b


BT2020_ALPHA, BT2020_BETA = _bt2020_alpha_beta()


def bt2020_oetf(x):
    return 4.5 * x if x < BT2020_BETA else BT2020_ALPHA * x ** 0.45 - (BT2020_ALPHA - 1)


CL_PB, CL_NB = 1 - bt2020_oetf(KB2020), bt2020_oetf(1 - KB2020)
CL_PR, CL_NR = 1 - bt2020_oetf(KR2020), bt2020_oetf(1 - KR2020)

# ---- BT.2100 tables 7 and 8 --------------------------------------------------------------------------------------
M_LMS = np.array([[1688, 2146, 262], [683, 2951, 462], [99, 309, 3688]]) / 4096
M_ICTCP = {16: np.array([[2048, 2048, 0], [6610, -13613, 7003], [17933, -17390, -543]]) / 4096,
           18: np.array([[2048, 2048, 0], [3625, -7465, 3840], [9500, -9212, -288]]) / 4096}


def kr_kb(matrix, prim):
    """(Kr, Kb) of a matrix id beside a primaries id; chroma-derived-nc takes them from the primaries"""
    if matrix != 12:
        return cm.KR_KB[matrix]
    if prim in (1, 9):
        return cm.KR_KB[prim]
    return cm.kr_kb_from_primaries(cm.primaries_class(prim))


def rgb_to_ycbcr(kr, kb):
    luma = np.array([kr, 1 - kr - kb, kb])
    return np.stack([luma, (np.array([0.0, 0.0, 1.0]) - luma) / (2 * (1 - kb)),
                     (np.array([1.0, 0.0, 0.0]) - luma) / (2 * (1 - kr))])


def _dot(m, c, s=None):
    """rows of m on the triple c; s: move each by its sign times the dot product's error bound"""
    out = [m[i, 0] * c[0] + m[i, 1] * c[1] + m[i, 2] * c[2] for i in range(3)]
    if s is not None:
        with np.errstate(invalid="ignore", over="ignore"):
            out = [o + si * cm.PERTURBATION * (abs(m[i, 0]) * np.abs(c[0]) + abs(m[i, 1]) * np.abs(c[1]) + abs(m[i, 2]) * np.abs(c[2]))
                   for i, (o, si) in enumerate(zip(out, s))]
    return out


class Conversion(cm.Conversion):
    """colour_model.Conversion with matrix ids 10, 12, 13 and 14 on either side"""

    def __init__(self, src, dst, depth, **kw):
        (pi, ti, mi, ri), (po, to, mo, ro) = src, dst
        self.form_in, self.form_out = matrix_form(mi), matrix_form(mo)
        for form, p, t, m in ((self.form_in, pi, ti, mi), (self.form_out, po, to, mo)):
            if form is not None and p != 9:
                raise ValueError("constant luminance and ICtCp are covered on BT.2020 primaries only")
            if form == ICTCP and t not in (16, 18):
                raise ValueError("ICtCp is covered with PQ and HLG only")
            if m == 12 and cm.primaries_class(p) not in cm.PRIMARIES:
                raise ValueError("primaries not covered")
        plain = lambda m: 9 if m in (10, 12, 13, 14) else m                      # stands in while the base class sets up
        super().__init__((pi, ti, plain(mi), ri), (po, to, plain(mo), ro), depth, **kw)
        if mi == 12:
            self.m_in = np.linalg.inv(rgb_to_ycbcr(*kr_kb(mi, pi)))
        if mo == 12:
            self.m_out = rgb_to_ycbcr(*kr_kb(mo, po))
        if self.form_in == ICTCP:
            self.m_in = np.linalg.inv(M_ICTCP[ti])
        if self.form_out == ICTCP:
            self.m_out = M_ICTCP[to]
        self.wide = self.form_in is not None or self.form_out is not None
        if self.wide:
            self.linear = True
            if self.tc_in not in cm.TRANSFERS or self.tc_out not in cm.TRANSFERS:
                raise ValueError("transfer not covered")
        yl = np.array([[1.0, 0.0, 0.0], [KR2020, 1 - KR2020 - KB2020, KB2020], [0.0, 0.0, 1.0]])   # (R, G, B) -> (R, Yl, B)
        self.post = {CL: yl, ICTCP: M_LMS, None: None}[self.form_out]
        self.pre = {CL: np.linalg.inv(yl), ICTCP: np.linalg.inv(M_LMS), None: None}[self.form_in]

    # ---- source codes -> linear RGB (after the npl scale) ------------------------------------------------------------
    def source_linear(self, y, u, v, s=None):
        """(linear RGB, in-gamut mask); s: signs of the moves of the intermediates (see the docstring)"""
        yf = (y - self.yoff_in) / self.ydiv_in
        uf, vf = (u - self.coff) / self.cdiv_in, (v - self.coff) / self.cdiv_in
        if self.form_in == CL:
            e = [yf + vf * 2 * np.where(vf < 0, CL_NR, CL_PR), yf, yf + uf * 2 * np.where(uf < 0, CL_NB, CL_PB)]
        else:
            e = [self.m_in[i, 0] * yf + self.m_in[i, 1] * uf + self.m_in[i, 2] * vf for i in range(3)]
        if s is not None:
            e = [ei * (1 + si * cm.PERTURBATION_SOURCE) for ei, si in zip(e, s)]
        with np.errstate(over="ignore", invalid="ignore"):
            t = [cm.to_linear(self.tc_in, ei) for ei in e]
            if self.pre is None:
                rgb = t
            else:
                if s is not None:
                    t = [ti * (1 + si * cm.PERTURBATION) for ti, si in zip(t, s)]
                rgb = _dot(self.pre, t, s)
            in_gamut = np.logical_and.reduce([(c >= 0) & (c <= 1) for c in (e if self.pre is None else rgb)])
            return [c * self.lin_scale for c in rgb], in_gamut

    # ---- linear RGB -> output codes -----------------------------------------------------------------------------------
    def back(self, c, s=None):
        if self.form_out is None:
            return super().back(c, s)
        if s is not None:
            c = [ci * (1 + si * cm.PERTURBATION) for ci, si in zip(c, s)]
        if self.tonemap is not None:
            sig = np.maximum(np.maximum(np.maximum(c[0], c[1]), c[2]), 1e-6)
            with np.errstate(invalid="ignore", over="ignore"):
                k = cm.tonemap_curve(self.tonemap, sig, self.param, self.peak) / sig
            c = [ci * k for ci in c]
        with np.errstate(invalid="ignore", over="ignore"):
            if self.gamut is not None:
                c = _dot(self.gamut, c, s)
            c = _dot(self.post, c, s)
            g = [cm.to_gamma(self.tc_out, ci * self.gam_scale) for ci in c]
            if self.form_out == CL:
                db, dr = g[2] - g[1], g[0] - g[1]
                out = [g[1], db / (2 * np.where(db < 0, CL_NB, CL_PB)), dr / (2 * np.where(dr < 0, CL_NR, CL_PR))]
            else:
                out = [self.m_out[i, 0] * g[0] + self.m_out[i, 1] * g[1] + self.m_out[i, 2] * g[2] for i in range(3)]
        return [out[0] * self.ymul_out + self.yoff_out, out[1] * self.cmul_out + self.coff,
                out[2] * self.cmul_out + self.coff]

    def convert_444(self, y, u, v, clip_chroma=True):
        """colour_model.Conversion.convert_444 with the box of moves extended as the docstring says"""
        if not self.wide:
            return super().convert_444(y, u, v, clip_chroma)
        y, u, v = (np.asarray(a, np.float64) for a in (y, u, v))
        c, in_gamut = self.source_linear(y, u, v)
        single = np.logical_and.reduce([np.abs(ci) < np.finfo(np.float32).max for ci in c])
        out = self.back(c)
        clip = lambda planes: [np.clip(o, -1, self.vmax + 1) if i == 0 or clip_chroma else o for i, o in enumerate(planes)]
        with np.errstate(invalid="ignore"):
            lo = hi = clip(out)
        for s in np.ndindex(2, 2, 2):
            s = [2 * si - 1 for si in s]
            moved = self.back(self.source_linear(y, u, v, s)[0], s)
            with np.errstate(invalid="ignore"):
                moved = clip(moved)
                lo = [np.fmin(a, m) for a, m in zip(lo, moved)]
                hi = [np.fmax(a, m) for a, m in zip(hi, moved)]
        with np.errstate(invalid="ignore"):
            spread = [b - a for a, b in zip(lo, hi)]
        finite = [np.isfinite(o) & single & np.isfinite(sp) for o, sp in zip(out, spread)]
        return out, in_gamut, finite, spread


def hdr_source(src):
    """the looser pair of caps of colour_model.judge: PQ / HLG sources, and the CL / ICtCp decodes, which cancel"""
    return matrix_form(src[2]) is not None or src[1] in (16, 18)


# ---- the conversions the GPU tests run: (id, source, settings of the drop-in, destination, model keywords, depths) ----
BT709 = cm.BT709
NC, CLSDR, CLFULL, CDC = (9, 14, 9, 1), (9, 14, 10, 1), (9, 14, 10, 2), (9, 14, 13, 1)
PQ_NC, PQ_CL, PQ_ICTCP = (9, 16, 9, 1), (9, 16, 10, 1), (9, 16, 14, 1)
HLG_NC, HLG_ICTCP = (9, 18, 9, 1), (9, 18, 14, 1)
TO709 = "primaries=bt709:transfer=bt709:matrix=bt709"
PQ_KW, HLG_KW = dict(peak=100.0), dict(peak=10.0)                              # determine_signal_peak without metadata
CASES = [
    ("cl_nc", CLSDR, "matrix=bt2020nc", NC, {}, (8, 10, 12)),
    ("nc_cl", NC, "matrix=bt2020c", CLSDR, {}, (10,)),
    ("cl_709", CLSDR, TO709, BT709, {}, (10,)),
    ("709_cl", BT709, "primaries=bt2020:transfer=bt2020-10:matrix=bt2020c", CLSDR, {}, (8,)),
    ("clfull_nc", CLFULL, "matrix=bt2020nc:range=tv", NC, {}, (10,)),
    ("pqcl_709_hable", PQ_CL, TO709 + ":tonemap=hable", BT709, dict(tonemap="hable", **PQ_KW), (10, 12)),
    ("pqcl_709_mobius", PQ_CL, TO709 + ":tonemap=mobius", BT709, dict(tonemap="mobius", **PQ_KW), (10, 12)),
    ("pqictcp_nc", PQ_ICTCP, "matrix=bt2020nc", PQ_NC, PQ_KW, (10, 12)),
    ("pqnc_ictcp", PQ_NC, "matrix=ictcp", PQ_ICTCP, PQ_KW, (10,)),
    ("hlgictcp_nc", HLG_ICTCP, "matrix=bt2020nc", HLG_NC, HLG_KW, (10,)),
    ("hlgnc_ictcp", HLG_NC, "matrix=ictcp", HLG_ICTCP, HLG_KW, (10,)),
    ("pqictcp_709_hable", PQ_ICTCP, TO709 + ":tonemap=hable", BT709, dict(tonemap="hable", **PQ_KW), (10,)),
    ("pqictcp_709_reinhard0.7", PQ_ICTCP, TO709 + ":tonemap=reinhard:param=0.7", BT709,
     dict(tonemap="reinhard", param=0.7, **PQ_KW), (10,)),
    ("hlgictcp_709_mobius", HLG_ICTCP, TO709 + ":tonemap=mobius", BT709, dict(tonemap="mobius", **HLG_KW), (10,)),
    ("pqcl_ictcp", PQ_CL, "matrix=ictcp", PQ_ICTCP, PQ_KW, (10,)),
    ("709_pqictcp", BT709, "primaries=bt2020:transfer=smpte2084:matrix=ictcp", PQ_ICTCP, {}, (10,)),
    ("cdnc2020_170m", (9, 14, 12, 1), "matrix=smpte170m", (9, 14, 6, 1), {}, (10,)),
    ("601_cdnc709", (1, 1, 6, 1), "matrix=chroma-derived-nc", (1, 1, 12, 1), {}, (8,)),
    ("709_p3cdnc", BT709, "primaries=smpte432:transfer=iec61966-2-1:matrix=chroma-derived-nc", (12, 13, 12, 1), {}, (10,)),
    ("p3cdnc_709", (12, 13, 12, 1), "matrix=bt709", (12, 13, 1, 1), {}, (10,)),
    ("cdc_nc", CDC, "matrix=bt2020nc", NC, {}, (10,)),
]
BY_ID = {c[0]: c for c in CASES}
YSTEP = {8: 4, 10: 16, 12: 64}           # 65 / 66 rows against the 33 x 33 chroma lattice
LAYOUTS = {"444": ("1x1", (0, 0)), "420": ("2x2", (1, 1)), "422": ("2x1", (1, 0))}
# every (case, depth) in 4:4:4 and 4:2:0; 4:2:2 for one CL and one ICtCp conversion
LATTICE = [(c, d, lay) for c in CASES for d in c[5] for lay in ("444", "420")]
LATTICE += [(BY_ID["cl_nc"], 10, "422"), (BY_ID["pqictcp_nc"], 10, "422")]


def frame(depth, layout):
    return cm.lattice_frame(depth, ystep=YSTEP[depth], sub=LAYOUTS[layout][1])


# frames at the kernel's edges, 4:2:0: one full 60 x 30 tile with a one-column and a one-row remainder, and the smallest
# frame the filter admits; (case id, depth, width, height)
EDGES = [(cid, depth, w, h) for w, h in ((62, 34), (2, 2))
         for cid, depth in (("cl_nc", 8), ("cl_nc", 10), ("pqictcp_nc", 8), ("pqictcp_nc", 10))]


def edge_frame(depth, w, h):
    """moderately saturated content around the grey axis (the caps need a frame mostly in gamut, and a 2 x 2 frame has
    six samples in all): luma codes 48 .. 190 and chroma within 12 of the mid code, both at 8 bits' scale"""
    dt, s = (np.uint8 if depth == 8 else np.uint16), depth - 8
    x, y = np.arange(w)[None, :], np.arange(h)[:, None]
    cx, cy = np.arange(w // 2)[None, :], np.arange(h // 2)[:, None]
    luma = (48 + 2 * ((3 * x + 5 * y) % 72)) << s
    cb = (128 + (7 * cx + 3 * cy) % 25 - 12) << s
    cr = (128 + (5 * cx + 11 * cy) % 25 - 12) << s
    return luma.astype(dt), cb.astype(dt), cr.astype(dt)


BATCHED = (644, 364, 19)                  # width, height, frames: one launch of 16 and a rest
BATCHED_JUDGED = ("pqictcp_709_hable", 0)  # the case and the frame of its stream that the model judges too


def batched_stream():
    """the 10-bit 4:2:0 stream of the batched-path test: moving natural-like content, then one frame of noise"""
    from handbrake_amd import synth
    w, h, n = BATCHED
    return synth.stream("progressive", w, h, n - 1, depth=10) + synth.stream("random", w, h, 1, depth=10)


_results = {}


def result(case, depth, layout):
    """the model's Result of a lattice case, computed once and shared (never written to)"""
    key = (case[0], depth, layout)
    if key not in _results:
        _, src, _, dst, kw, _ = case
        _results[key] = Conversion(src, dst, depth, **kw).convert(frame(depth, layout), *LAYOUTS[layout][1])
    return _results[key]
