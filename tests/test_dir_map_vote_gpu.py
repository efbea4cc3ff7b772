"""GPU parity of EEDI2's dir-map passes (k_dir_map_fe<1, false>, <2, false>, <2, true>, k_dir_map4: the four-pixel vote of
eedi2_dirmap_vote.h) where their tiles are cut - 14 rows x 256 columns with a one-pixel ring - and on neighbourhoods with
every number of missing directions; and of the half-height pair as two launches (k_dir_map4 / k_dir_map_c, q_dir_map4 /
q_dir_map) where their blocks are cut and on planes without a mask sample: every scratch plane of a field against the
oracle, tolerance 0."""
import numpy as np
import pytest

from handbrake_amd import hbrt, hip, synth
import oracle_lib as ol

pytestmark = pytest.mark.gpu


def crafted_frames(w, h, n, chroma_edges=True, depth=8):
    """Flat pictures with a few isolated edges: short slanted bars, a wedge and a lone dot per 64 x 32 cell, moving a pixel
    per frame.  Away from them nothing has a direction (neighbourhoods with 0 - 3 values: the result is a peak or
    unchanged), along and around them the direction map thins out through every count of missing neighbours.
    chroma_edges=False leaves the chroma planes constant (128 and 120); depth > 8: the same pictures, uint16, scaled up."""
    out = []
    for t in range(n):
        planes = []
        for c, (pw, ph, flat) in enumerate(((w, h, 60), ((w + 1) // 2, (h + 1) // 2, 128), ((w + 1) // 2, (h + 1) // 2, 120))):
            if c and not chroma_edges:
                planes.append(np.full((ph, pw), flat, np.uint8))
                continue
            y, x = np.mgrid[0:ph, 0:pw]
            xx, yy = (x + t) % 64, y % 32
            p = np.full((ph, pw), flat, np.int32)
            p[np.abs((xx - 8) - 2 * (yy - 4)) <= 2] += 90                       # a steep bar
            p[(np.abs((xx - 30) * 2 + (yy - 16) * 3) <= 3) & (yy > 6) & (yy < 26)] += 70   # a shallow one
            p[(xx > 44) & (xx < 60) & (yy > 8) & (yy - 8 < (xx - 44))] -= 50    # a wedge
            p[(xx == 40) & (yy == 28)] += 100                                   # a dot
            planes.append(np.clip(p, 0, 255).astype(np.uint8))
        if depth > 8:
            planes = [q.astype(np.uint16) << (depth - 8) for q in planes]
        out.append(tuple(planes))
    return out


def absent_counts(dmap, mask, tff):
    """How many of the 9 slots of eedi2_filter_dir_map_2x hold no value, for every pixel the pass works on, from the
    oracle's own planes (dmap = the pass's input, mask = msk2p): the set of counts that occur."""
    h, w = dmap.shape
    seen = set()
    d = dmap.astype(np.int32)
    for y in range(2 - tff, h - 1, 2):
        work = (mask[y - 1, 1:w - 1] == 255) | (mask[y + 1, 1:w - 1] == 255)
        miss = np.zeros(w - 2, np.int32)
        for yy, ok in ((y - 2, y > 1), (y, True), (y + 2, y < h - 2)):
            for dx in (0, 1, 2):
                miss += (d[yy, dx:w - 2 + dx] == 255) if ok else 1
        seen.update(int(v) for v in np.unique(miss[work]))
    return seen


def _parity(frames, w, h, postproc=1, search=None, sub=None, need_counts=False, depth=8, empty_chroma_masks=False):
    kw = {} if search is None else {"search": search}
    n = len(frames)
    ctx = hip.Ctx(0)
    if sub is None:
        dev = hip.DecombDevice(ctx, w, h, mode=24, postproc=postproc, depth=depth, **kw)
        oe = ol.OrcEedi2(w, h, postproc=postproc, **kw) if depth == 8 else ol.OrcEedi2_16(w, h, depth, postproc=postproc, **kw)
        lcw = 1
    else:
        lcw, lch = ol.SUBSAMPLING[sub]
        dev = hip.DecombDevice(ctx, w, h, mode=24, postproc=postproc, lcw=lcw, lch=lch)
        oe = ol.RefEedi2Fmt(w, h, hbrt.PIX_FMT[(sub, 8)], 8, f"mode=8:postproc={postproc}")
    seen = set()
    try:
        dev.push(frames[0])
        for t in range(1, n):
            dev.push(frames[t])
            for tff in (1, 0):
                oe.run(frames[t - 1], tff)
                if empty_chroma_masks:                # the case is about planes without a mask sample, under a luma with some
                    mskp = ol.EEDI2_BUFFERS.index("mskp")
                    assert oe.plane(mskp, 0)[:, :w].any(), "the luma mask must hold edges"
                    for c in (1, 2):
                        assert not oe.plane(mskp, c)[:, :-(-w >> lcw)].any(), f"the mask of plane {c} must be empty"
                if need_counts:                       # tmp2p2 = the map in front of the last filter_dir_map_2x, msk2p its mask
                    seen |= absent_counts(oe.plane(5, 0)[:, :w], oe.plane(6, 0)[:, :w], tff)
            while dev.pull() is not None:
                pass
            for b in range(9):
                for c in range(3):
                    pw = w if c == 0 else -(-w >> lcw)
                    np.testing.assert_array_equal(dev.eedi_plane(b, c)[:, :pw], oe.plane(b, c)[:, :pw],
                                                  err_msg=f"{ol.EEDI2_BUFFERS[b]} plane {c} after frame {t - 1}")
    finally:
        oe.close()
        dev.close()
        ctx.close()
    if need_counts:
        assert seen == set(range(10)), f"the input must hold every count of missing neighbours 0 .. 9, has {sorted(seen)}"


# 328 x 80: luma fields of 40 rows x 328 columns - two tile columns, the second partial, both ring columns in use, a partial
# last tile row (FE_R = 14) at half height and a different one at full height; chroma 164 wide, one partial tile.
# 200 x 144: narrower than a tile, fields of 72 rows.  330 x 80: neither plane's width a multiple of 4 (330, 165).
@pytest.mark.parametrize("postproc", [0, 1])
@pytest.mark.parametrize("model,w,h", [("random", 328, 80), ("corners", 328, 80), ("random", 200, 144), ("corners", 330, 80)])
def test_tiles_and_rings(built, model, w, h, postproc):
    _parity(synth.stream(model, w, h, 3), w, h, postproc=postproc)


@pytest.mark.parametrize("w,h", [(328, 80), (200, 144)])
def test_every_absent_count(built, w, h):
    _parity(crafted_frames(w, h, 3), w, h, postproc=1, need_counts=True)


def test_444(built):
    from test_formats_gpu import frames_for
    _parity(frames_for("1x1", 8, 328, 80, 3, "interlaced"), 328, 80, postproc=1, sub="1x1")


# A search distance past the tiled calc_directions' halo (30) takes the half-height dir-map pair as two launches: k_dir_map4 /
# k_dir_map_c, q_dir_map4 / q_dir_map at 10 bits.  328 x 80: more than one 256-column block, the second partial.  330 x 80:
# neither plane's width a multiple of 4 (the partial last dword column and its store).  200 x 144: narrower than a block;
# fields of 72 rows, no multiple of k_dir_map_c's 16 rows per block (of 4, though: no partial block row in the 4-row kernels).
# "flat_chroma": the chroma planes constant under a luma with edges - their masks stay empty (asserted from the oracle's
# own mask planes) and every kernel of the pair takes its shortest way, the stores of a partial last column included.
# The distance is 32, the last one the reference defines: its table of limits has 33 entries and calc_directions looks it up
# by the length of the direction it found (eedi2_template.c:500), so where a longer one wins the reference reads behind its
# table - "corners" at 40 does, and neither the oracle nor any build of the kernels has a defined answer there.  The random
# stream at 40 is the case this test has always had; no direction wins on random bytes.
UNFUSED = [(8, 40, "random", 328, 80)] + [(depth, 32, model, w, h) for depth in (8, 10) for model, w, h in
                                          (("random", 328, 80), ("corners", 330, 80), ("random", 200, 144), ("flat_chroma", 330, 80))]


@pytest.mark.parametrize("depth,search,model,w,h", UNFUSED)
def test_unfused_filter(built, depth, search, model, w, h):
    flat = model == "flat_chroma"
    frames = crafted_frames(w, h, 3, chroma_edges=False, depth=depth) if flat else synth.stream(model, w, h, 3, depth=depth)
    _parity(frames, w, h, postproc=1, search=search, depth=depth, empty_chroma_masks=flat)
