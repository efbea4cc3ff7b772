"""Text subtitles: an independent numpy restatement of what the reference's rendersub.c does with libass's glyph images
(render_ssa_subs :623-665) - the boxes of hb_box_vec_append / _merge / _compact (:144-226), their alignment to the chroma
plane of the cropped picture (:648-653) and compose_subsample_ass (:474-612) - and the cases the tests and the recorder
(tests/golden/make_ass_compose_golden.py) share.

An image is (bitmap, w, dst_x, dst_y, (y, cb, cr, a)): `bitmap` a 2-D uint8 array whose row pitch is the stride and whose
first `w` columns are the image, the colour as rgb2yuv_fn(color >> 8) gives it, a = color & 0xff (0 = opaque) - what
hbrt.ass_image_array takes.
"""
import numpy as np

SHIFTS = {"420": (1, 1), "422": (1, 0), "444": (0, 0)}
OVERLAY_FMT = {"420": 33, "422": 78, "444": 79}                    # AV_PIX_FMT_YUVA420P / 422P / 444P
FRAME_FMT = {("420", 8): 0, ("422", 8): 4, ("444", 8): 5, ("420", 10): 62}   # AV_PIX_FMT_YUV420P / 422P / 444P / 420P10LE
NV12 = 23


def chroma_coeffs(chroma_location, wshift, hshift):
    """hb_compute_chroma_smoothing_coefficient, common.c:7054-7091: a window into 1 3 9 27 9 3 1"""
    base = [1, 3, 9, 27, 9, 3, 1]
    wx, wy = 4 - (1 << wshift), 4 - (1 << hshift)
    if chroma_location in (1, 3, 5):
        wx += (1 << wshift) - 1
    if 3 <= chroma_location <= 6:              # the switch falls through top / bottom alike
        wy += (1 << hshift) - 1
    return ([(base[i + wx] + base[i + wx + (not wx & 1)]) >> 1 for i in range(1 << wshift)],
            [(base[i + wy] + base[i + wy + (not wy & 1)]) >> 1 for i in range(1 << hshift)])


# ---- hb_box_vec_* (:144-226) ----
def _intersect(a, b, offset):
    return min(a[2], b[2]) + offset - max(a[0], b[0]) >= 0 and min(a[3], b[3]) + offset - max(a[1], b[1]) >= 0


def boxes_of(images):
    """[x1, y1, x2, y2] of render_ssa_subs' boxes: appended image by image, merged and compacted after every append.  A box
    the merge has cleared stays in the vector as [0, 0, 0, 0] for the rest of the pass, as in the reference."""
    vec = []
    for bitmap, w, x, y, _ in images:
        h = bitmap.shape[0]
        if w == 0 or h == 0:                                                   # x1 == x2 || y1 == y2: an empty box
            continue
        vec.append([x, y, x + w, y + h])
        for i in range(len(vec) - 1):
            for j in range(i + 1, len(vec)):
                a, b = vec[i], vec[j]
                if _intersect(a, b, 8):
                    vec[i] = [min(a[0], b[0]), min(a[1], b[1]), max(a[2], b[2]), max(a[3], b[3])]
                    vec[j] = [0, 0, 0, 0]
        vec = [b for b in vec if b[2] != 0 or b[3] != 0]
    return vec


def _div255(x):
    return ((x + ((x + 128) >> 8)) + 128) >> 8


def compose(images, x, y, width, height, wshift, hshift, coeffs):
    """compose_subsample_ass for the box (x, y, width, height): (Y, Cb, Cr, A) and the mask of the chroma samples the
    reference defines (accu_c > 0, :593); the others are 0 here."""
    compo = np.zeros((4, height, width), np.int64)                             # Y, Cb, Cr, A
    for bitmap, w, dx, dy, (fy, fu, fv, fa) in images:
        h = bitmap.shape[0]
        # :503-505.  x and y are unsigned there: a box pulled back past the origin (x1 = 0 under an odd crop) has x = -1 =
        # UINT_MAX, which no dst_x reaches - its overlay stays empty
        if not (w and h and 0 <= x <= dx and x + width >= dx + w and 0 <= y <= dy and y + height >= dy + h):
            continue
        g = bitmap[:, :w].astype(np.int64)
        a = _div255((255 - fa) * g)                                            # ssa_alpha :478-486
        reg = compo[:, dy - y:dy - y + h, dx - x:dx - x + w]
        old_a = reg[3].copy()
        first, later = (a > 0) & (old_a == 0), (a > 0) & (old_a > 0)
        ain, acomp = a * 255, old_a * (255 - a)
        res = np.where(later, ain + acomp, 1)
        for c, f in enumerate((fy, fu, fv)):
            blended = (ain * f + reg[c] * acomp + (res >> 1)) // res           # ALPHA_BLEND :474-475
            reg[c] = np.where(first, f, np.where(later, blended, reg[c]))
        reg[3] = np.where(first, a, np.where(later, _div255(res), old_a))
    # :568-608.  The inner loops run over the block's (1 << wshift) x (1 << hshift) positions, clipped at the right and
    # bottom edge (:580-582), but every position of a row reads that row's FIRST pixel (the index has no xz term,
    # :585-590): a chroma sample is made of the left column of its block, each row weighted by the sum of the horizontal
    # weights that passed the clip.
    bw, bh = 1 << wshift, 1 << hshift
    cw, ch = -(-width >> wshift), -(-height >> hshift)
    accu = np.zeros((3, ch, cw), np.int64)                                     # accu_a, accu_b, accu_c
    xx = np.arange(cw) << wshift
    for yz in range(bh):
        left = compo[:, yz::bh, ::bw]                                          # the rows with yz + yy < height
        rows = left.shape[1]
        for xz in range(bw):
            coeff = coeffs[0][xz] * coeffs[1][yz] * left[3] * (xz + xx < width)
            accu[0, :rows] += coeff * left[1]
            accu[1, :rows] += coeff * left[2]
            accu[2, :rows] += coeff
    defined = accu[2] > 0
    den = np.where(defined, accu[2], 1)
    cb = np.where(defined, (accu[0] + (den >> 1)) // den, 0)
    cr = np.where(defined, (accu[1] + (den >> 1)) // den, 0)
    assert compo.max() <= 255 and cb.max(initial=0) <= 255 and cr.max(initial=0) <= 255
    u8 = lambda p: np.ascontiguousarray(p, dtype=np.uint8)
    return (u8(compo[0]), u8(cb), u8(cr), u8(compo[3])), defined


def render(images, wshift, hshift, chroma_location, crop_left=0, crop_top=0):
    """render_ssa_subs with `changed` set: ([(x, y, (Y, Cb, Cr, A))] as the compositor takes them, [defined-chroma mask])"""
    coeffs = chroma_coeffs(chroma_location, wshift, hshift)
    overlays, masks = [], []
    for x1, y1, x2, y2 in boxes_of(images):
        x = x1 - ((x1 + crop_left) & ((1 << wshift) - 1))                      # :650-653
        y = y1 - ((y1 + crop_top) & ((1 << hshift) - 1))
        planes, defined = compose(images, x, y, x2 - x, y2 - y, wshift, hshift, coeffs)
        overlays.append((x + crop_left, y + crop_top, planes))                 # :658-659
        masks.append(defined)
    return overlays, masks


def defined_share(masks):
    return sum(int(m.sum()) for m in masks) / max(sum(m.size for m in masks), 1)


# ---- the cases ----
# name -> (frame width, frame height, [(w, h, x, y, a)], extra bytes of bitmap stride)
CASES = {
    # overlap blend; odd origin (the box is padded left and up by one); odd width and height (clipped last chroma column and row)
    "pair": (96, 64, [(37, 15, 11, 7, 0), (31, 11, 13, 9, 64)], 0),
    # a = 255 contributes nothing; order dependence; repeated ALPHA_BLEND
    "stack": (96, 64, [(40, 20, 20, 16, 0), (36, 16, 22, 18, 128), (40, 20, 20, 16, 255), (30, 18, 27, 17, 200), (38, 14, 21, 20, 16)], 0),
    # an 8-pixel gap merges, a 9-pixel gap does not: two boxes
    "gap": (96, 64, [(20, 10, 4, 4, 0), (20, 10, 32, 4, 32), (20, 10, 61, 4, 0)], 0),
    # a box wider than one 256-column tile of the kernel, images straddling the tile edge
    "wide": (320, 32, [(150, 9, 3, 3, 0), (151, 9, 140, 5, 96), (90, 13, 100, 1, 0)], 0),
    # an empty image is skipped; a 1 x 1 box
    "tiny": (96, 64, [(1, 1, 9, 9, 0), (0, 5, 30, 30, 0), (12, 8, 50, 50, 0)], 0),
    # stride != w
    "stride": (96, 64, [(37, 15, 11, 7, 0), (31, 11, 13, 9, 64)], 5),
    # hb_box_vec_merge as it is: the third image joins the first and leaves a cleared box behind, (0, 0, 0, 0), which the
    # second - within 8 pixels of the origin - then "intersects": its box grows to the origin.  Under an odd crop that box is
    # pulled back to x = y = -1, where the reference's unsigned compare lets no image in: an empty overlay
    "origin": (96, 64, [(40, 16, 30, 30, 0), (9, 9, 1, 1, 0), (40, 16, 32, 32, 48)], 0),
}
# The tests ask that the model define 70 % of a case's chroma samples at least.  A sample is defined where the LEFT column of
# its block holds a covered pixel (see compose), and a quarter of a bitmap's pixels is zero: a singly covered column is
# defined in 15 of 16 blocks at 4:2:0 but in 3 of 4 at 4:2:2 and 4:4:4, which `gap` and `wide`, their boxes a fifth empty,
# cannot afford; a box padded left by one loses its first chroma column, which the small boxes of `tiny` and `origin`
# cannot.  Where named here a case carries every image twice - the second a "shadow" of the same size and place with
# another colour and transparency, which leaves the boxes as they are and a pixel uncovered only where both bitmaps are
# zero.  (`tiny` has a 12 x 8 image where a 2 x 2 one would do for the boxes, for the same reason.)
DOUBLED = {"gap": ("422", "444"), "wide": ("422", "444"), "tiny": ("420", "422", "444"), "origin": ("420", "422", "444")}


def build(name, fmt="420"):
    """(frame width, frame height, images) of a case; bitmaps random in 1..255 with a quarter of the pixels zeroed"""
    fw, fh, rects, extra = CASES[name]
    rng = np.random.default_rng(20260 + list(CASES).index(name.replace("stride", "pair")))          # `stride` has the pixels of `pair`
    images = []
    for layer in range(2 if fmt in DOUBLED.get(name, ()) else 1):
        for w, h, x, y, a in rects:
            bitmap = np.full((h, w + extra), 255, np.uint8)                    # what lies between the rows is not the image's
            bitmap[:, :w] = rng.integers(1, 256, (h, w), dtype=np.uint8)
            bitmap[:, :w][rng.random((h, w)) < 0.25] = 0
            colour = tuple(int(v) for v in rng.integers(16, 240, 3))
            images.append((bitmap, w, x, y, colour + ((a + 40 * layer) & 255,)))
    return fw, fh, images


def frame(fw, fh, fmt="420", depth=8, seed=7):
    """a random planar frame"""
    rng = np.random.default_rng(seed)
    ws, hs = SHIFTS[fmt]
    dt = np.uint8 if depth == 8 else np.uint16
    return tuple(rng.integers(0, 1 << depth, s, dtype=dt) for s in ((fh, fw), (fh >> hs, fw >> ws), (fh >> hs, fw >> ws)))
