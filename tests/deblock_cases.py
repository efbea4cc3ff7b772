"""The cases the deblock GPU tests run (tests/test_deblock_gpu.py), as explicit lists, and what tests/test_deblock_cpu.py
derives from them: the (b, strength, depth, plane size) at which the model's raster transcription and its block-row form
are held equal.  Every list is checked when it is built - a case the model declines, or a list that lost one of the
geometries it is there for, is an error at collection, never a shorter list."""
import numpy as np

import deblock_model as dm

LCW = {"2x2": (1, 1), "2x1": (1, 0), "1x1": (0, 0)}
TW, TH, HX, HY = 128, 32, 8, 5            # deblock_local_kernel's tile and halo (csrc/deblock.hip: DB_TW, DB_TH, DB_HX, DB_HY)
WEB_SEG, WEB_LDS = 8, 48 * 1024           # deblock_web_kernel's edges per segment and LDS budget (DB_WEB_SEG, DB_WEB_LDS)


def plane_sizes(w, h, sub):
    """[(w, h)] of the three planes"""
    lcw, lch = LCW[sub]
    c = (-((-w) >> lcw), -((-h) >> lch))
    return [(w, h), c, c]


def accepted(cases):
    """the list itself; dm.Declined (at collection) if the model declines any plane of any case"""
    for w, h, sub, depth, st in cases:
        dm.resolve(st, depth, plane_sizes(w, h, sub))
    assert len(set(cases)) == len(cases)
    return cases


def settings(strong, b, thresh):
    return f"strength={'strong' if strong else 'weak'}:thresh={thresh}:blocksize={b}"


def tile_edges(size, b, L, tile, halo):
    """per tile along one axis: the edges whose window the local kernel finds wholly loaded (its xa / xz / nx, ya / yz / ny)"""
    out = []
    for t0 in range(0, size, tile):
        s, e = max(t0 - halo, 0), min(t0 + tile + halo, size)
        a, z = max(b, (s + L + b - 1) // b * b), min(e - L, size - 1)
        out.append((z - a) // b + 1 if z >= a else 0)
    return out


def edges(size, b):
    return (size - 1) // b if size > b else 0


# ---- content -----------------------------------------------------------------------------------------------------------
def _dtype(depth):
    return np.uint8 if depth == 8 else np.uint16


def near_flat(w, h, sub, depth, seed, t=0):
    """+-2 codes of noise on a slow staircase: nearly every edge fires, so the chains of the web kernel never forget"""
    rng = np.random.default_rng(seed)
    sh = depth - 8
    out = []
    for c, (pw, ph) in enumerate(plane_sizes(w, h, sub)):
        base = 120 + (np.arange(pw)[None, :] // 7 + t) % 5 if c == 0 else 128
        p = ((base + rng.integers(-2, 3, size=(ph, pw))) << sh) + rng.integers(0, 1 << sh, size=(ph, pw), endpoint=False)
        out.append(p.astype(_dtype(depth)))
    return tuple(out)


def near_white(w, h, sub, depth, seed, mirror=False):
    """max - uniform[0, 60) * 2^(depth - 8) (mirror: the same distance from 0): fired edges push taps past the range"""
    rng = np.random.default_rng(seed)
    maxv = (1 << depth) - 1
    out = []
    for pw, ph in plane_sizes(w, h, sub):
        d = rng.integers(0, 60, size=(ph, pw)) << (depth - 8)
        out.append((d if mirror else maxv - d).astype(_dtype(depth)))
    return tuple(out)


# ---- depths and layouts: what test_depths_and_layouts ran before the lists were explicit, and the sizes added since --------
W50, S20 = "strength=weak:thresh=50", "strength=strong:thresh=20"
S50_16, S75_4, S20_5 = "strength=strong:thresh=50:blocksize=16", "strength=strong:thresh=75:blocksize=4", "strength=strong:thresh=20:blocksize=5"
_LAYOUTS = [("2x2", 10), ("2x2", 12), ("2x1", 8), ("2x1", 10), ("2x1", 12), ("1x1", 8), ("1x1", 10), ("1x1", 12)]
FORMAT_CASES = accepted(
    # 638 x 362: 362 % 4 = 362 % 5 = 362 % 8 = 2, so of the strong settings only b = 16 has a defined result
    [(638, 362, sub, depth, st) for sub, depth in _LAYOUTS for st in (W50, S50_16)] +
    # the large size: one case per layout keeps the numpy model's time down
    [(1918, 1078, sub, depth, S50_16) for sub, depth in _LAYOUTS] +
    # 64 x 48: strong b = 5 on 4:4:4 only (chroma width 32 % 5 = 2)
    [(64, 48, sub, depth, st) for sub, depth in _LAYOUTS
     for st in (W50, S20, S50_16, S75_4) + ((S20_5,) if sub == "1x1" else ())] +
    # 640 x 360 (chroma 320 x 180 / 320 x 360): strong b = 8 (180 % 8 = 4) and b = 5 (every remainder 0) on the
    # subsampled layouts at 10 and 12 bits, which no size above lets through
    [(640, 360, sub, depth, st) for sub in ("2x2", "2x1") for depth in (10, 12) for st in (S20, S20_5)])
assert len(FORMAT_CASES) == 59 + 8

# ---- block sizes on the local kernel ---------------------------------------------------------------------------------------
# (w, h, layout, depth, strong, b, thresh).  "end": w % b = h % b = L, the last edge's window ends on the plane's last
# sample; "mult": w % b = h % b = 0.  Luma is a little over one tile each way unless said otherwise.
_LOCAL = [
    (129, 33, "1x1", 8, True, 6, 20),       # end on every plane; the tightest non-overlapping windows
    (132, 36, "2x2", 10, True, 6, 50),      # mult; chroma 66 x 18
    (129, 38, "1x1", 10, True, 7, 50),      # end
    (133, 42, "2x1", 12, True, 7, 20),      # mult; chroma 67 x 42 (67 % 7 = 4)
    (129, 39, "1x1", 12, True, 9, 20),      # end
    (135, 36, "2x2", 8, True, 9, 50),       # mult; chroma 68 x 18 (68 % 9 = 5)
    (138, 48, "2x2", 12, True, 9, 50),      # end in luma; chroma 69 x 24 (remainder 6)
    (135, 39, "2x1", 8, True, 12, 20),      # end in luma; chroma 68 x 39 (68 % 12 = 8)
    (132, 36, "1x1", 10, True, 12, 50),     # mult
    (133, 42, "1x1", 8, True, 13, 50),      # end
    (130, 39, "2x1", 10, True, 13, 20),     # mult; chroma 65 x 39
    (135, 69, "1x1", 12, True, 33, 20),     # end; three tile rows
    (132, 66, "2x2", 8, True, 33, 50),      # mult; chroma 66 x 33: two tile rows and no horizontal edge
    (163, 83, "1x1", 10, True, 40, 50),     # end; luma's first tile row holds no horizontal edge
    (160, 80, "2x2", 12, True, 40, 20),     # mult; chroma 80 x 40: two tile rows and no horizontal edge
    (263, 133, "1x1", 8, True, 130, 50),    # end; three tile columns
    (260, 260, "2x2", 10, True, 130, 20),   # mult; chroma 130 x 130: two tile columns and no edge at all
    (515, 515, "2x2", 8, True, 512, 50),    # end; luma has one edge each way, chroma (258 x 258) none
    (1024, 36, "1x1", 10, True, 512, 20),   # mult; the vertical edge at 512 only, tile columns 0 - 2 and 5 - 7 without one
    (512, 300, "2x1", 12, True, 512, 50),   # b >= every plane: the output is the input
    (130, 34, "1x1", 12, False, 4, 20),     # weak: end
    (132, 40, "2x1", 8, False, 4, 50),      # mult; chroma 66 x 40 (66 % 4 = 2: end)
    (132, 37, "1x1", 8, False, 5, 50),      # end
    (130, 40, "2x2", 12, False, 5, 20),     # mult; chroma 65 x 20
    (135, 37, "2x2", 10, False, 7, 20),     # end in luma; chroma 68 x 19 (remainder 5)
    (133, 35, "1x1", 12, False, 7, 50),     # mult
    (134, 68, "1x1", 8, False, 33, 20),     # end
    (132, 66, "2x1", 12, False, 33, 50),    # mult; chroma 66 x 66
]
LOCAL_CASES = accepted([(w, h, sub, depth, settings(strong, b, th)) for w, h, sub, depth, strong, b, th in _LOCAL])


def _check_local():
    assert {(d, s) for _, _, s, d, *_ in _LOCAL} == {(d, s) for d in (8, 10, 12) for s in LCW}
    by = {}
    for w, h, sub, depth, strong, b, _ in _LOCAL:
        assert not (strong and b < 6), "the web kernel's block sizes belong to WEB_CASES"
        by.setdefault((strong, b), []).append((w, h, sub))
    assert set(by) == {(True, b) for b in (6, 7, 9, 12, 13, 33, 40, 130, 512)} | {(False, b) for b in (4, 5, 7, 33)}
    for (strong, b), cs in by.items():
        L = 3 if strong else 2
        assert any(w > b and w % b == L for w, h, _ in cs), (b, "no case ends on the last sample")
        assert any(w > b and w % b == 0 for w, h, _ in cs), (b, "no multiple of b")
        if b <= 40:
            assert any(h > b and h % b == L for w, h, _ in cs) and any(h > b and h % b == 0 for w, h, _ in cs), b
        if strong and b <= 13:                    # 2 x 2 luma tiles, the last a few samples wide and a few rows high
            assert all(0 < w - TW <= 16 and 0 < h - TH <= 16 for w, h, _ in cs), b
        per_plane = [[(tile_edges(pw, b, L, TW, HX), tile_edges(ph, b, L, TH, HY)) for pw, ph in plane_sizes(w, h, sub)[:2]]
                     for w, h, sub in cs]
        if strong and b in (33, 40):              # two tile rows of some case without a horizontal edge
            assert any(sum(ny.count(0) for _, ny in planes) >= 2 for planes in per_plane), b
        if strong and b == 130:                   # two tile columns without a vertical edge
            assert any(sum(nx.count(0) for nx, _ in planes) >= 2 for planes in per_plane), b
    has = lambda w, h, sub, b: [edges(pw, b) + edges(ph, b) > 0 for pw, ph in plane_sizes(w, h, sub)[:2]]
    big = [has(w, h, sub, 512) for w, h, sub in by[(True, 512)]]
    assert [True, False] in big and [False, False] in big


_check_local()


def has_edge(w, h, sub, st):
    b = dm.resolve(st, 8)["block"]
    return any(edges(pw, b) + edges(ph, b) > 0 for pw, ph in plane_sizes(w, h, sub))


# ---- the web kernel (strong, b = 4 / 5) --------------------------------------------------------------------------------------
def web_rows(w, b):
    """rows of a block row the web kernel holds in LDS at once (DeblockFilter::web_rows for luma width w): 48 KiB over a
    row's bytes - 2 per sample plus 8 per segment of 8 edges, of (w - 1) / b edges"""
    nseg = ((w - 1) // b + WEB_SEG - 1) // WEB_SEG
    return min(b, WEB_LDS // (2 * w + 8 * nseg))


# the chunked block row: (w, h, layout, b), luma wide enough that rows_lds < b; four block rows high
WEB_WIDE = [(4800, 20, "2x2", 5), (7680, 16, "2x2", 4)]
# edge counts of a row: b -> {edges: width}, widths with a defined result (w % b not 1 or 2, or w <= b)
WEB_WIDTHS = {4: {0: 4, 1: 7, 7: 32, 8: 35, 9: 40, 16: 68}, 5: {0: 5, 1: 8, 7: 38, 8: 44, 9: 50, 16: 85}}
# 4:2:0 with luma and chroma on different sides of a segment boundary: (w, h, b) -> luma edges, chroma edges
WEB_SPLIT = {(85, 18, 5): (16, 8), (72, 16, 4): (17, 8), (50, 18, 5): (9, 4)}
WEB_DEPTHS = (8, 10)
WEB_THRESH = 50


def web_heights(b):
    return (b, b + 3)                     # no horizontal edge; one, whose band ends on the last row


def web_shapes():
    """every (w, h, layout, b) the web-kernel shape tests run"""
    out = list(WEB_WIDE)
    out += [(w, h, "1x1", b) for b, ws in WEB_WIDTHS.items() for w in ws.values() for h in web_heights(b)]
    out += [(w, h, "2x2", b) for w, h, b in WEB_SPLIT]
    return out


def _check_web():
    for b, ws in WEB_WIDTHS.items():
        assert sorted(ws) == [0, 1, 7, 8, 9, 16]
        for ne, w in ws.items():
            assert (w - 1) // b == ne and (ne > 0 or w <= b), (b, ne, w)
        assert [edges(h, b) for h in web_heights(b)] == [0, 1]
    for (w, h, b), (ny, nc) in WEB_SPLIT.items():
        assert ((w - 1) // b, (-(-w // 2) - 1) // b) == (ny, nc)
        assert -(-ny // WEB_SEG) != -(-nc // WEB_SEG)                      # another number of segments
    for w, h, sub, b in WEB_WIDE:
        assert web_rows(w, b) < b and 3 <= h // b <= 4
    accepted([(w, h, sub, d, settings(True, b, WEB_THRESH)) for w, h, sub, b in web_shapes() for d in WEB_DEPTHS])


_check_web()

# ---- launch side and clipping: (w, h, layout, depth, settings) ---------------------------------------------------------------
# (small frames of two luma tile columns and several tile rows: the numpy model of the web case is what takes the time)
PITCH_SETTINGS = [(160, 96, settings(True, 8, 20)), (160, 100, settings(False, 5, 20)), (160, 96, settings(True, 4, 50))]
PITCH_CASES = accepted([(w, h, "2x2", d, st) for w, h, st in PITCH_SETTINGS for d in (8, 10)])
CUT_CASES = accepted([(96, 64, "2x2", 8, st) for st in (settings(True, 8, 20), settings(True, 4, 50))])
CLIP_CASES = accepted([(128, 64, "2x2", d, settings(strong, 8, 100)) for d in (8, 12) for strong in (True, False)])


# ---- what the CPU test holds the two forms of the model equal on ---------------------------------------------------------
def _small(size, b):
    """a plane size the raster form can afford with the same geometry: sizes of up to three edges as they are, larger
    ones cut to three edges with the same remainder (the position of the last window against the plane's end)"""
    return size if size <= 3 * b + b - 1 else 3 * b + size % b


def model_cases():
    """sorted (b, strong, depth, thresh, w, h): every plane of every case above, cut by _small, and per (b, strong,
    depth) with b <= 130 the sizes 3b x (2b + 3), b x 2b, 2b x b, (b - 1) x (b - 1) and about 131 x 37 where they have a
    defined result"""
    out = set()
    lists = FORMAT_CASES[-8:] + LOCAL_CASES + PITCH_CASES + CUT_CASES + CLIP_CASES + \
        [(w, h, sub, d, settings(True, b, WEB_THRESH)) for w, h, sub, b in web_shapes() for d in WEB_DEPTHS]
    for w, h, sub, depth, st in lists:
        p = dm.resolve(st, depth)
        b, strong = p["block"], p["strong"]
        thresh = int(dict(kv.split("=") for kv in st.split(":"))["thresh"])
        for pw, ph in plane_sizes(w, h, sub):
            out.add((b, strong, depth, thresh, _small(pw, b), _small(ph, b)))
        near = lambda s: next(v for v in range(s, s + b) if dm.plane_ok(v, b, strong))
        if b > 130:                       # (b = 512: its own planes only - megapixel planes are the raster form's limit)
            continue
        for sw, sh in [(3 * b, 2 * b + 3), (b, 2 * b), (2 * b, b), (b - 1, b - 1), (near(131), near(37))]:
            if dm.plane_ok(sw, b, strong) and dm.plane_ok(sh, b, strong):
                out.add((b, strong, depth, thresh, sw, sh))
    for b, strong, depth, thresh, w, h in out:
        assert dm.plane_ok(w, b, strong) and dm.plane_ok(h, b, strong)
    return sorted(out)
