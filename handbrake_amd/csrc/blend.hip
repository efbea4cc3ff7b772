// blend.hip — the reference's subtitle compositor (libhb/blend.c) for planar frames on gfx950.
//
//   blend_same_kernel        blend8on8 :425-509 / blend8on1x :511-604   (overlay in the frame's subsampling)
//   blend_subsample_kernel   blend_subsample_8on8 :236-328 / blend_subsample_8on1x :48-140
//                            (4:4:4 overlay on a chroma-subsampled frame, chroma-location aware)
//
// The 8-bit functions are the 16-bit ones with shift 0, so each kernel is one template over the
// sample type.  Integer arithmetic throughout: bit-exact with the reference.  A thread owns one
// chroma sample of the frame and the (1 << wshift) x (1 << hshift) luma samples that go with it, so a
// frame sample is read and written by exactly one thread; overlays are composited in list order
// (they may overlap, hb_blend_work :866-869): consecutive overlays that touch disjoint parts of the frame - the
// usual case, a few lines of text - go into one launch (grid.z = overlay; the groups are found when the list is
// set), one that overlaps an earlier one of its group starts the next launch.  Overlay bitmaps are uploaded once per
// change (rendersub's `changed`), not per frame.
//
// Not reproduced: the reference's stray chroma writes one sample before the row when a
// same-subsampling overlay hangs over the left / top edge by an odd amount (:485-505), and its
// running past the row / plane when an overlay sticks out to the right / bottom (:74-75): writes stop
// at the frame edge.  The kernel bodies are in blend_body.h, shared with the biplanar (NV12 / P010LE) forms of biplanar.hip;
// an object made by hbhip_blend_create_biplanar composites those on a staging buffer in the host picture's own layout.
#include "hbhip_internal.h"

#include <algorithm>
#include <cmath>
#include <vector>

#include "blend_body.h"
#include "ass_compose.h"
#include "bitmap_scale.h"
#include "sws_filter.h"

namespace {

// grid: overlay chroma samples (xx, yy) in the overlay's own coordinates
template <typename PIX>
__global__ __launch_bounds__(256) void blend_same_kernel(BlendArgs a, OverlayGroup G)
{
    blend_same_body<PIX, false>(a, G);
}

// grid: frame chroma samples starting at (bx0, by0) = the first one the overlay touches
template <typename PIX>
__global__ __launch_bounds__(256) void blend_subsample_kernel(BlendArgs a, OverlayGroup G)
{
    blend_subsample_body<PIX, false>(a, G);
}

} // namespace

struct hbhip_blend
{
    hbhip_ctx *ctx = nullptr;
    PicGeometry geo;
    int chroma_location = 1, ov_wshift = 0, ov_hshift = 0;
    bool subsample = false;
    unsigned coeff[2][2] = {{1, 1}, {1, 1}};
    DevBuf<uint8_t> d_store;             // the uploaded overlay bitmaps, back to back
    std::vector<OverlayDev> overlays;
    struct Launch { OverlayGroup g; int n; dim3 grid; };
    std::vector<Launch> launches;        // the overlays in list order, grouped (build_launches)
    hbhip_frame *staging = nullptr;      // device frame of the host-frame entry point
    bool biplanar = false;               // made by hbhip_blend_create_biplanar
    DevBuf<uint8_t> bi_stage;            // its staging buffer: the host picture as it is (BiLayout)
    // hbhip_blend_set_ass_images: box table, image table and glyph bitmaps, packed in pinned memory and uploaded in one copy
    PinnedBuf<uint8_t> h_ass;
    DevBuf<uint8_t> d_ass;
    hipEvent_t ass_uploaded = nullptr;   // behind the last copy out of h_ass: the next call packs into it after this
    // hbhip_blend_set_bitmaps: the bitmap subtitles the object holds, scaled, each in an allocation of its own (they come
    // and go one by one); it packs its tables and source planes into h_ass / d_ass as well
    struct Bitmap { uint64_t key; int sw, sh, dw, dh; DevBuf<uint8_t> d; };   // d: Y, Cb, Cr, A back to back, stride align16(dw)
    std::vector<Bitmap> bitmaps;
    int64_t bmp_scaled = 0, bmp_uploaded = 0, bmp_hits = 0;

    ~hbhip_blend()                       // (the buffers go with their members, behind this)
    {
        if (ass_uploaded) (void)hipEventDestroy(ass_uploaded);
        if (staging) hbhip_frame_release(staging);
    }
};

// The launches of an overlay list: what a launch of one overlay used to cover (its grid and, for the subsampling
// kernel, its origin), and consecutive overlays joined while the frame rectangles they touch - luma, widened to whole
// chroma samples and by one more sample for the odd-origin cases - stay disjoint.
static void build_launches(hbhip_blend *b)
{
    b->launches.clear();
    const int ws = b->geo.log2_cw, hs = b->geo.log2_ch, W = b->geo.width, H = b->geo.height;
    struct Rect { int x0, y0, x1, y1; };
    std::vector<Rect> rects;                                    // of the overlays in the group being filled
    hbhip_blend::Launch cur;
    cur.n = 0;
    cur.grid = dim3(0, 0, 0);
    auto flush = [&]() {
        if (cur.n) { cur.grid.z = cur.n; b->launches.push_back(cur); }
        cur.n = 0; cur.grid = dim3(0, 0, 0); rects.clear();
    };
    for (const OverlayDev &o : b->overlays)
    {
        int bx0 = 0, by0 = 0, nx, ny;
        if (b->subsample)
        {
            int x0c = o.x & ~((1 << ws) - 1), y0c = o.y & ~((1 << hs) - 1);
            if (x0c < 0) x0c = 0;
            if (y0c < 0) y0c = 0;
            const int ow = o.width <= W ? o.width : W, oh = o.height <= H ? o.height : H;
            int x1 = o.x + ow, y1 = o.y + oh;                     // one past the last frame sample touched
            if (x1 > W) x1 = W;
            if (y1 > H) y1 = H;
            if (x1 <= x0c || y1 <= y0c) continue;
            bx0 = x0c >> ws; by0 = y0c >> hs;
            nx = ((x1 - 1) >> ws) - bx0 + 1; ny = ((y1 - 1) >> hs) - by0 + 1;
        }
        else
        {
            nx = -((-o.width) >> ws); ny = -((-o.height) >> hs);
        }
        const int m = 2 << (ws > hs ? ws : hs);
        const Rect r = { o.x - m, o.y - m, o.x + o.width + m, o.y + o.height + m };
        bool clash = cur.n == BL_GROUP;
        for (const Rect &q : rects) clash = clash || (r.x0 < q.x1 && q.x0 < r.x1 && r.y0 < q.y1 && q.y0 < r.y1);
        if (clash) flush();
        cur.g.o[cur.n] = o; cur.g.bx0[cur.n] = bx0; cur.g.by0[cur.n] = by0;
        cur.grid.x = std::max<unsigned>(cur.grid.x, (nx + 63) / 64);
        cur.grid.y = std::max<unsigned>(cur.grid.y, (ny + 3) / 4);
        cur.n++;
        rects.push_back(r);
    }
    flush();
}

extern "C" int hbhip_blend_create(hbhip_ctx *ctx, int width, int height, int depth, int log2_chroma_w, int log2_chroma_h,
                                  int chroma_location, int overlay_log2_chroma_w, int overlay_log2_chroma_h,
                                  hbhip_blend **out)
{
    if (!ctx || !out) return HBHIP_ERR_ARG;
    *out = nullptr;
    if (depth != 8 && depth != 10 && depth != 12) return HBHIP_ERR_UNSUPPORTED;
    if (log2_chroma_w < 0 || log2_chroma_w > 1 || log2_chroma_h < 0 || log2_chroma_h > 1 || width < 1 || height < 1)
        return HBHIP_ERR_ARG;
    const bool subsample = log2_chroma_w != overlay_log2_chroma_w || log2_chroma_h != overlay_log2_chroma_h;
    // the reference's subsampling functions index the overlay's chroma at full resolution (blend.c:117-122)
    if (subsample && (overlay_log2_chroma_w || overlay_log2_chroma_h)) return HBHIP_ERR_UNSUPPORTED;
    hbhip_blend *b = new (std::nothrow) hbhip_blend;
    if (!b) return HBHIP_ERR_NOMEM;
    b->ctx = ctx;
    b->geo.set(width, height, depth, log2_chroma_w, log2_chroma_h);
    b->chroma_location = chroma_location;
    b->ov_wshift = overlay_log2_chroma_w;
    b->ov_hshift = overlay_log2_chroma_h;
    b->subsample = subsample;
    // hb_compute_chroma_smoothing_coefficient (common.c:7054-7091): window into 1 3 9 27 9 3 1
    static const unsigned base[] = { 1, 3, 9, 27, 9, 3, 1 };
    int wx = 4 - (1 << log2_chroma_w), wy = 4 - (1 << log2_chroma_h);
    const bool left = chroma_location == 1 || chroma_location == 3 || chroma_location == 5;
    const bool vert = chroma_location >= 3 && chroma_location <= 6;       // the switch falls through top / bottom alike
    if (left) wx += (1 << log2_chroma_w) - 1;
    if (vert) wy += (1 << log2_chroma_h) - 1;
    for (int i = 0; i < 2; i++)
    {
        b->coeff[0][i] = (base[i + wx] + base[i + wx + !(wx & 1)]) >> 1;
        b->coeff[1][i] = (base[i + wy] + base[i + wy + !(wy & 1)]) >> 1;
    }
    *out = b;
    return HBHIP_OK;
}

extern "C" void hbhip_blend_destroy(hbhip_blend *b)
{
    if (!b) return;
    (void)hipSetDevice(b->ctx->device);
    (void)hipStreamSynchronize(b->ctx->stream);
    delete b;
}

extern "C" int hbhip_blend_set_overlays(hbhip_blend *b, const hbhip_overlay *ov, int n)
{
    if (!b || n < 0 || (n > 0 && !ov)) return HBHIP_ERR_ARG;
    hbhip_ctx *ctx = b->ctx;
    (void)hipSetDevice(ctx->device);
    // launches of the previous set may still be reading the store
    HBHIP_CHECK(ctx, hipStreamSynchronize(ctx->stream));
    b->overlays.clear();
    b->launches.clear();
    size_t total = 0;
    for (int i = 0; i < n; i++)
    {
        if (ov[i].width < 1 || ov[i].height < 1) return HBHIP_ERR_ARG;
        const int cw = -((-ov[i].width) >> b->ov_wshift), ch = -((-ov[i].height) >> b->ov_hshift);
        total += 2 * (size_t)hbhip_align_up(ov[i].width, 16) * ov[i].height + 2 * (size_t)hbhip_align_up(cw, 16) * ch;
    }
    if (const int rc = b->d_store.reserve(ctx, total)) return rc;
    uint8_t *at = b->d_store.get();
    for (int i = 0; i < n; i++)
    {
        OverlayDev d;
        d.x = ov[i].x; d.y = ov[i].y; d.width = ov[i].width; d.height = ov[i].height;
        const int cw = -((-ov[i].width) >> b->ov_wshift), ch = -((-ov[i].height) >> b->ov_hshift);
        for (int p = 0; p < 4; p++)
        {
            const bool chroma = p == 1 || p == 2;
            const int w = chroma ? cw : ov[i].width, h = chroma ? ch : ov[i].height;
            d.stride[p] = hbhip_align_up(w, 16);
            d.plane[p] = at;
            HBHIP_CHECK(ctx, hipMemcpy2DAsync(at, d.stride[p], ov[i].plane[p], ov[i].stride[p], w, h,
                                              hipMemcpyHostToDevice, ctx->stream));
            at += (size_t)d.stride[p] * h;
        }
        b->overlays.push_back(d);
    }
    build_launches(b);
    // the caller may free its bitmaps as soon as this returns
    HBHIP_CHECK(ctx, hipStreamSynchronize(ctx->stream));
    return HBHIP_OK;
}

// The pinned staging buffer h_ass and its device twin d_ass, both at least `bytes`.  On return the previous call's copy has
// left the staging buffer; a twin that has to grow waits for the kernels that may still be reading the old one.
static int reserve_upload(hbhip_blend *b, size_t bytes)
{
    hbhip_ctx *ctx = b->ctx;
    if (bytes > b->d_ass.count())
    {
        HBHIP_CHECK(ctx, hipStreamSynchronize(ctx->stream));
        if (const int rc = b->d_ass.alloc(ctx, bytes)) return rc;
    }
    if (!b->ass_uploaded) HBHIP_CHECK(ctx, hipEventCreateWithFlags(&b->ass_uploaded, hipEventDisableTiming));
    else HBHIP_CHECK(ctx, hipEventSynchronize(b->ass_uploaded));
    return b->h_ass.reserve(ctx, bytes);
}

// ---- text subtitles: libass's glyph images composed on the device (ass_compose.hip) ----
namespace {
struct AssBox { int x1, y1, x2, y2; };

// hb_box_intersect / hb_box_vec_merge / _compact (rendersub.c:144-199) as they are: a box cleared by the merge stays in the
// vector until the compaction and takes part in the rest of the pass as (0, 0, 0, 0)
bool ass_box_intersect(const AssBox &a, const AssBox &b, int offset)
{
    return std::min(a.x2, b.x2) + offset - std::max(a.x1, b.x1) >= 0 && std::min(a.y2, b.y2) + offset - std::max(a.y1, b.y1) >= 0;
}

void ass_box_append(std::vector<AssBox> &v, int x1, int y1, int x2, int y2)          // hb_box_vec_append :201-226
{
    if (x1 == x2 || y1 == y2) return;
    v.push_back({ x1, y1, x2, y2 });
    for (size_t i = 0; i + 1 < v.size(); i++)
        for (size_t j = i + 1; j < v.size(); j++)
            if (ass_box_intersect(v[i], v[j], 8))
            {
                v[i].x1 = std::min(v[i].x1, v[j].x1); v[i].y1 = std::min(v[i].y1, v[j].y1);
                v[i].x2 = std::max(v[i].x2, v[j].x2); v[i].y2 = std::max(v[i].y2, v[j].y2);
                v[j] = { 0, 0, 0, 0 };
            }
    size_t k = 0;
    for (size_t i = 0; i < v.size(); i++)
        if (v[i].x2 != 0 || v[i].y2 != 0) v[k++] = v[i];
    v.resize(k);
}
} // namespace

// render_ssa_subs (rendersub.c:623-665) behind ass_render_frame: boxes on the host, compose_subsample_ass on the device
extern "C" int hbhip_blend_set_ass_images(hbhip_blend *b, const hbhip_ass_image *img, int n, int crop_left, int crop_top)
{
    if (!b || n < 0 || (n > 0 && !img)) return HBHIP_ERR_ARG;
    if (b->subsample) return HBHIP_ERR_UNSUPPORTED;          // compose_subsample_ass makes overlays in the frame's subsampling
    const int ws = b->ov_wshift, hs = b->ov_hshift;
    std::vector<AssBox> boxes;
    size_t bits = 0;
    for (int i = 0; i < n; i++)
    {
        const hbhip_ass_image &m = img[i];
        if (m.w < 0 || m.h < 0 || m.dst_x < 0 || m.dst_y < 0 || m.dst_x > (1 << 20) || m.dst_y > (1 << 20) ||
            m.w > (1 << 20) || m.h > (1 << 20))
            return HBHIP_ERR_ARG;
        if (m.w && m.h && (!m.bitmap || m.stride < m.w)) return HBHIP_ERR_ARG;
        if (m.w && m.h) bits += (size_t)m.w * m.h;
        ass_box_append(boxes, m.dst_x, m.dst_y, m.dst_x + m.w, m.dst_y + m.h);
    }
    hbhip_ctx *ctx = b->ctx;
    (void)hipSetDevice(ctx->device);
    b->overlays.clear();
    b->launches.clear();
    if (boxes.empty()) return HBHIP_OK;                      // clear_ssa_rendered_sub_cache :614-621

    const size_t box_bytes = boxes.size() * sizeof(AssBoxDev), img_bytes = (size_t)n * sizeof(AssImageDev);
    const size_t bits_at = (box_bytes + img_bytes + 15) & ~(size_t)15;
    const size_t up_bytes = bits_at + ASS_BITS_PAD + ((bits + 15) & ~(size_t)15) + ASS_BITS_PAD;
    if (up_bytes > 0x7fffffff) return HBHIP_ERR_UNSUPPORTED;
    size_t total = 0;
    std::vector<OverlayDev> ovs(boxes.size());
    for (size_t k = 0; k < boxes.size(); k++)
    {
        // the overlay is aligned to the chroma plane of the cropped picture, padded left and up as needed (:648-653)
        OverlayDev &d = ovs[k];
        d.x = boxes[k].x1 - ((boxes[k].x1 + crop_left) & ((1 << ws) - 1));
        d.y = boxes[k].y1 - ((boxes[k].y1 + crop_top) & ((1 << hs) - 1));
        d.width = boxes[k].x2 - d.x; d.height = boxes[k].y2 - d.y;
        if (d.width < 1 || d.height < 1) return HBHIP_ERR_ARG;
        const int cw = -((-d.width) >> ws), ch = -((-d.height) >> hs);
        d.stride[0] = d.stride[3] = hbhip_align_up(d.width, 16);
        d.stride[1] = d.stride[2] = hbhip_align_up(cw, 16);
        total += 2 * (size_t)d.stride[0] * d.height + 2 * (size_t)d.stride[1] * ch;
    }
    if (total > b->d_store.count() || up_bytes > b->d_ass.count())
        HBHIP_CHECK(ctx, hipStreamSynchronize(ctx->stream));                  // launches of the previous set may still be reading them
    if (const int rc = b->d_store.reserve(ctx, total)) return rc;
    const int rs = reserve_upload(b, up_bytes);
    if (rs != HBHIP_OK) return rs;

    uint8_t *const h_ass = b->h_ass.get(), *const d_ass = b->d_ass.get();
    AssBoxDev *hb = reinterpret_cast<AssBoxDev *>(h_ass);
    AssImageDev *hi = reinterpret_cast<AssImageDev *>(h_ass + box_bytes);
    uint8_t *at = b->d_store.get();
    dim3 grid(1, 1, (unsigned)boxes.size());
    for (size_t k = 0; k < boxes.size(); k++)
    {
        OverlayDev &d = ovs[k];
        const int ch = -((-d.height) >> hs);
        for (int p = 0; p < 4; p++)
        {
            d.plane[p] = at;
            hb[k].plane[p] = at;
            hb[k].stride[p] = d.stride[p];
            at += (size_t)d.stride[p] * (p == 1 || p == 2 ? ch : d.height);
        }
        hb[k].x = d.x; hb[k].y = d.y; hb[k].w = d.width; hb[k].h = d.height;
        grid.x = std::max<unsigned>(grid.x, (d.width + ASS_TILE_W - 1) / ASS_TILE_W);
        grid.y = std::max<unsigned>(grid.y, (ch + ASS_TILE_WAVES - 1) / ASS_TILE_WAVES);
        d.x += crop_left; d.y += crop_top;                                  // :658-659
    }
    memset(h_ass + box_bytes + img_bytes, 0, bits_at + ASS_BITS_PAD - (box_bytes + img_bytes));
    size_t off = ASS_BITS_PAD;
    for (int i = 0; i < n; i++)
    {
        const hbhip_ass_image &m = img[i];
        const bool empty = !m.w || !m.h;
        hi[i].off = (int)off; hi[i].w = empty ? 0 : m.w; hi[i].h = empty ? 0 : m.h; hi[i].x = m.dst_x; hi[i].y = m.dst_y;
        hi[i].yuva = (unsigned)m.y | (unsigned)m.cb << 8 | (unsigned)m.cr << 16 | (unsigned)m.a << 24;
        hi[i].pad[0] = hi[i].pad[1] = 0;
        if (empty) continue;
        for (int r = 0; r < m.h; r++) memcpy(h_ass + bits_at + off + (size_t)r * m.w, m.bitmap + (size_t)r * m.stride, m.w);
        off += (size_t)m.w * m.h;
    }
    memset(h_ass + bits_at + off, 0, up_bytes - bits_at - off);
    // the caller may free its bitmaps from here on: they are in the staging buffer
    HBHIP_CHECK(ctx, hipMemcpyAsync(d_ass, h_ass, up_bytes, hipMemcpyHostToDevice, ctx->stream));
    HBHIP_CHECK(ctx, hipEventRecord(b->ass_uploaded, ctx->stream));

    AssArgs a;
    a.box = reinterpret_cast<const AssBoxDev *>(d_ass);
    a.img = reinterpret_cast<const AssImageDev *>(d_ass + box_bytes);
    a.bits = d_ass + bits_at;
    a.n_img = n;
    for (int i = 0; i < 2; i++) { a.cx[i] = b->coeff[0][i]; a.cy[i] = b->coeff[1][i]; }
    const int rc = hbhip_ass_compose_launch(ctx, ws, hs, grid, a);
    if (rc != HBHIP_OK) return rc;
    b->overlays = std::move(ovs);
    build_launches(b);
    return HBHIP_OK;
}

// ---- bitmap subtitles: scale_subtitle (rendersub.c:242-377) with the scaling on the device (bitmap_scale.hip) ----
namespace {
struct BitmapPlan
{
    const hbhip_bitmap_sub *sub;
    int dw, dh, x, y;                    // scaled size, placed position
    bool scale, fresh;                   // fresh: this call made the entry and fills it
    size_t entry;                        // in hbhip_blend::bitmaps
    size_t at, planes_at;                // a fresh one's bytes in the staging buffer: tables (scaled ones), packed source planes
    std::vector<int> px, py;
    std::vector<short> qx, qy;
    int tx, ty, rows;
};

// everything the object holds goes, once what may still be reading it has run
void drop_bitmaps(hbhip_blend *b)
{
    if (b->bitmaps.empty()) return;
    (void)hipSetDevice(b->ctx->device);
    (void)hipStreamSynchronize(b->ctx->stream);
    b->bitmaps.clear();
}

// :311-375: out of the cropped zones, 2 % of the height (20 rows at most) clear of top and bottom and 20 columns of the
// sides, centred where it does not fit.  crop = top, bottom, left, right.
void place_bitmap(int W, int H, const int crop[4], int w, int h, int &x, int &y)
{
    int margin_top = ((H - crop[0] - crop[1]) * 2) / 100;
    if (margin_top > 20) margin_top = 20;
    if (h > H - crop[0] - crop[1] - margin_top * 2) y = crop[0] + (H - crop[0] - crop[1] - h) / 2;
    else if (y < crop[0] + margin_top)              y = crop[0] + margin_top;
    else if (y > H - crop[1] - margin_top - h)      y = H - crop[1] - margin_top - h;
    if (w > W - crop[2] - crop[3] - 40)             x = crop[2] + (W - crop[2] - crop[3] - w) / 2;
    else if (x < crop[2] + 20)                      x = crop[2] + 20;
    else if (x > W - crop[3] - 20 - w)              x = W - crop[3] - 20 - w;
}

// the tables of a bitmap that has to be scaled, and the most source rows a tile of bitmap_scale_kernel taps (its own walk)
int plan_tables(BitmapPlan &pl)
{
    const int sw = pl.sub->width, sh = pl.sub->height;
    pl.tx = sws_filter(sw, pl.dw, 1 << 14, 128, 128, pl.px, pl.qx);
    pl.ty = sws_filter(sh, pl.dh, 1 << 12, 128, 128, pl.py, pl.qy);
    for (int v : pl.px) if (v < 0 || v + pl.tx > sw) return HBHIP_ERR_UNSUPPORTED;
    for (int v : pl.py) if (v < 0 || v + pl.ty > sh) return HBHIP_ERR_UNSUPPORTED;
    pl.rows = 0;
    for (int y0 = 0; y0 < pl.dh; y0 += BMS_TILE_H)
    {
        int r0 = pl.py[y0], r1 = r0 + pl.ty;
        for (int y = y0 + 1; y < std::min(y0 + BMS_TILE_H, pl.dh); y++)
        {
            r0 = std::min(r0, pl.py[y]);
            r1 = std::max(r1, pl.py[y] + pl.ty);
        }
        pl.rows = std::max(pl.rows, r1 - r0);
    }
    return pl.rows <= BMS_MAX_ROWS ? HBHIP_OK : HBHIP_ERR_UNSUPPORTED;
}

int set_bitmaps(hbhip_blend *b, const hbhip_bitmap_sub *sub, int n, const int crop[4])
{
    if (n < 0 || (n > 0 && !sub) || !crop) return HBHIP_ERR_ARG;
    if (b->ov_wshift || b->ov_hshift) return HBHIP_ERR_UNSUPPORTED;       // bitmap subtitles are YUVA444P (:418, :1073)
    hbhip_ctx *ctx = b->ctx;
    (void)hipSetDevice(ctx->device);
    const int W = b->geo.width, H = b->geo.height;

    // sizes and positions, in the reference's double arithmetic (:246-283)
    std::vector<BitmapPlan> plans;
    for (int i = 0; i < n; i++)
    {
        const hbhip_bitmap_sub &s = sub[i];
        if (s.width < 0 || s.height < 0) return HBHIP_ERR_ARG;
        if (!s.width || !s.height) continue;                                // a PGS "clear" packet (:1043-1055)
        for (int p = 0; p < 4; p++)
            if (!s.plane[p] || s.stride[p] < s.width) return HBHIP_ERR_ARG;
        double factor = 1.;
        if (s.window_width > 0 && s.window_height > 0)
        {
            const double xfactor = (double)W / s.window_width, yfactor = (double)H / s.window_height;
            factor = xfactor > yfactor ? xfactor : yfactor;
        }
        BitmapPlan pl;
        pl.sub = &s;
        pl.scale = std::fabs(factor - 1) > 0.01;
        pl.fresh = false;
        pl.dw = s.width; pl.dh = s.height; pl.x = s.x; pl.y = s.y;
        if (pl.scale)
        {
            // below 8 samples libswscale clamps its tap count to the plane (initFilter: size <= src - 2)
            if (factor < 0.25 || factor > 4. || s.width < 8 || s.height < 8) return HBHIP_ERR_UNSUPPORTED;
            pl.dw = (int)(s.width * factor); pl.dh = (int)(s.height * factor);
            pl.x = (int)(s.x * factor); pl.y = (int)(s.y * factor);
            if (pl.dw < 1 || pl.dh < 1) return HBHIP_ERR_UNSUPPORTED;
        }
        place_bitmap(W, H, crop, pl.dw, pl.dh, pl.x, pl.y);
        pl.entry = pl.at = pl.planes_at = 0;
        pl.tx = pl.ty = pl.rows = 0;
        plans.push_back(std::move(pl));
    }

    // A key the object holds at this geometry is a hit.  Any other gets an entry, once every hit is known: in the allocation
    // of an entry this call does not name where one is large enough - whoever still reads that is queued on the stream ahead
    // of what fills it again, so a subtitle that replaces another waits for nothing and allocates nothing - or a new one.
    std::vector<signed char> used(b->bitmaps.size(), 0);
    auto find = [&](const BitmapPlan &pl) {
        const hbhip_bitmap_sub &s = *pl.sub;
        size_t e = 0;
        while (e < b->bitmaps.size() && !(used[e] >= 0 && b->bitmaps[e].key == s.key && b->bitmaps[e].sw == s.width &&
                                          b->bitmaps[e].sh == s.height && b->bitmaps[e].dw == pl.dw && b->bitmaps[e].dh == pl.dh))
            e++;
        return e;
    };
    const size_t held = b->bitmaps.size();
    for (BitmapPlan &pl : plans)
        if ((pl.entry = find(pl)) < held) used[pl.entry] = 1;
    for (size_t e = 0; e < held; e++)
        if (!used[e]) used[e] = -1;                                         // not named: its key means nothing from here on
    for (BitmapPlan &pl : plans)
    {
        if (pl.entry == held) pl.entry = find(pl);                          // (a key named twice in a list: made once)
        if (pl.entry < b->bitmaps.size())
        {
            b->bmp_hits++;
            continue;
        }
        const hbhip_bitmap_sub &s = *pl.sub;
        if (pl.scale)
        {
            const int rt = plan_tables(pl);
            if (rt != HBHIP_OK) return rt;
        }
        const size_t need = 4 * (size_t)hbhip_align_up(pl.dw, 16) * pl.dh;
        size_t e = b->bitmaps.size();
        for (size_t k = 0; k < held; k++)
            if (used[k] < 0 && b->bitmaps[k].d.count() >= need && (e == b->bitmaps.size() || b->bitmaps[k].d.count() < b->bitmaps[e].d.count())) e = k;
        if (e == b->bitmaps.size())
        {
            hbhip_blend::Bitmap m = {};
            if (const int rc = m.d.alloc(ctx, need)) return rc;
            b->bitmaps.push_back(std::move(m));
            used.push_back(1);
        }
        hbhip_blend::Bitmap &m = b->bitmaps[e];
        m.key = s.key; m.sw = s.width; m.sh = s.height; m.dw = pl.dw; m.dh = pl.dh;
        used[e] = 1;
        pl.entry = e;
        pl.fresh = true;
    }

    // the fresh ones through the staging buffer: [tables][source planes] of every one to scale, in one copy to its twin,
    // then the planes of the others, each copied to where it stays
    std::vector<BitmapPlan *> fresh;
    for (int scale = 1; scale >= 0; scale--)
        for (BitmapPlan &pl : plans)
            if (pl.fresh && pl.scale == (scale != 0)) fresh.push_back(&pl);
    size_t up_bytes = 0, scaled_bytes = 0;
    for (BitmapPlan *pl : fresh)
    {
        pl->at = up_bytes;
        if (pl->scale)
            up_bytes += ((pl->px.size() + pl->py.size()) * sizeof(int) + (pl->qx.size() + pl->qy.size()) * sizeof(short) + 15) & ~(size_t)15;
        pl->planes_at = up_bytes;
        up_bytes += 4 * (size_t)hbhip_align_up(pl->sub->width, 16) * pl->sub->height;
        if (pl->scale) scaled_bytes = up_bytes;
    }
    if (up_bytes > 0x7fffffff) return HBHIP_ERR_UNSUPPORTED;
    if (!fresh.empty())
    {
        const int rs = reserve_upload(b, up_bytes);
        if (rs != HBHIP_OK) return rs;
        uint8_t *const h_ass = b->h_ass.get(), *const d_ass = b->d_ass.get();
        for (BitmapPlan *pl : fresh)
        {
            const hbhip_bitmap_sub &s = *pl->sub;
            uint8_t *at = h_ass + pl->at;
            if (pl->scale)
            {
                memset(h_ass + pl->planes_at - 16, 0, 16);                   // (the tables end inside these)
                memcpy(at, pl->px.data(), pl->px.size() * sizeof(int));   at += pl->px.size() * sizeof(int);
                memcpy(at, pl->py.data(), pl->py.size() * sizeof(int));   at += pl->py.size() * sizeof(int);
                memcpy(at, pl->qx.data(), pl->qx.size() * sizeof(short)); at += pl->qx.size() * sizeof(short);
                memcpy(at, pl->qy.data(), pl->qy.size() * sizeof(short));
            }
            const int sp = hbhip_align_up(s.width, 16);
            at = h_ass + pl->planes_at;
            for (int p = 0; p < 4; p++)
                for (int r = 0; r < s.height; r++, at += sp)
                {
                    memcpy(at, s.plane[p] + (size_t)r * s.stride[p], s.width);
                    memset(at + s.width, 0, sp - s.width);
                }
        }
        // the caller may free its bitmaps from here on: they are in the staging buffer
        if (scaled_bytes) HBHIP_CHECK(ctx, hipMemcpyAsync(d_ass, h_ass, scaled_bytes, hipMemcpyHostToDevice, ctx->stream));
        for (BitmapPlan *pl : fresh)
        {
            const hbhip_bitmap_sub &s = *pl->sub;
            const size_t src_plane = (size_t)hbhip_align_up(s.width, 16) * s.height;
            uint8_t *dst = b->bitmaps[pl->entry].d.get();
            b->bmp_uploaded++;
            if (!pl->scale)
            {
                HBHIP_CHECK(ctx, hipMemcpyAsync(dst, h_ass + pl->planes_at, 4 * src_plane, hipMemcpyHostToDevice, ctx->stream));
                continue;
            }
            BitmapScaleArgs a;
            a.spitch = hbhip_align_up(s.width, 16); a.dpitch = hbhip_align_up(pl->dw, 16);
            a.dw = pl->dw; a.dh = pl->dh; a.tx = pl->tx; a.ty = pl->ty;
            for (int p = 0; p < 4; p++)
            {
                a.src[p] = d_ass + pl->planes_at + p * src_plane;
                a.dst[p] = dst + p * (size_t)a.dpitch * pl->dh;
            }
            a.px = reinterpret_cast<const int *>(d_ass + pl->at);
            a.py = a.px + pl->px.size();
            a.qx = reinterpret_cast<const short *>(a.py + pl->py.size());
            a.qy = a.qx + pl->qx.size();
            const int rl = hbhip_bitmap_scale_launch(ctx, a, pl->rows);
            if (rl != HBHIP_OK) return rl;
            b->bmp_scaled++;
        }
        HBHIP_CHECK(ctx, hipEventRecord(b->ass_uploaded, ctx->stream));
    }

    // the list, in list order; then the keys this call did not name go
    for (const BitmapPlan &pl : plans)
    {
        const hbhip_blend::Bitmap &m = b->bitmaps[pl.entry];
        OverlayDev d;
        d.x = pl.x; d.y = pl.y; d.width = m.dw; d.height = m.dh;
        for (int p = 0; p < 4; p++)
        {
            d.stride[p] = hbhip_align_up(m.dw, 16);
            d.plane[p] = m.d.get() + p * (size_t)d.stride[p] * m.dh;
        }
        b->overlays.push_back(d);
    }
    if (std::find(used.begin(), used.end(), -1) != used.end())
    {
        HBHIP_CHECK(ctx, hipStreamSynchronize(ctx->stream));                // launches of the previous list may still be reading them
        size_t keep = 0;
        for (size_t e = 0; e < b->bitmaps.size(); e++)
            if (used[e] > 0) b->bitmaps[keep++] = std::move(b->bitmaps[e]);
        b->bitmaps.erase(b->bitmaps.begin() + (ptrdiff_t)keep, b->bitmaps.end());
    }
    build_launches(b);
    return HBHIP_OK;
}
} // namespace

extern "C" int hbhip_blend_set_bitmaps(hbhip_blend *b, const hbhip_bitmap_sub *sub, int n, const int crop[4])
{
    if (!b) return HBHIP_ERR_ARG;
    b->overlays.clear();
    b->launches.clear();
    const int rc = set_bitmaps(b, sub, n, crop);
    if (rc != HBHIP_OK)
    {
        // an empty list, and nothing half-made behind it: the caller takes this frame's subtitles down its other path
        b->overlays.clear();
        b->launches.clear();
        drop_bitmaps(b);
    }
    return rc;
}

extern "C" int hbhip_blend_debug_bitmap_stats(hbhip_blend *b, int64_t *scaled, int64_t *uploaded, int64_t *hits)
{
    if (!b) return HBHIP_ERR_ARG;
    if (scaled) *scaled = b->bmp_scaled;
    if (uploaded) *uploaded = b->bmp_uploaded;
    if (hits) *hits = b->bmp_hits;
    return HBHIP_OK;
}

extern "C" int hbhip_blend_debug_overlay_count(hbhip_blend *b) { return b ? (int)b->overlays.size() : HBHIP_ERR_ARG; }

extern "C" int hbhip_blend_debug_get_overlay(hbhip_blend *b, int index, uint8_t *const plane[4], const int stride[4], int xywh[4])
{
    if (!b || !xywh || index < 0 || index >= (int)b->overlays.size()) return HBHIP_ERR_ARG;
    hbhip_ctx *ctx = b->ctx;
    (void)hipSetDevice(ctx->device);
    const OverlayDev &d = b->overlays[index];
    xywh[0] = d.x; xywh[1] = d.y; xywh[2] = d.width; xywh[3] = d.height;
    if (!plane) return HBHIP_OK;
    if (!stride) return HBHIP_ERR_ARG;
    const int cw = -((-d.width) >> b->ov_wshift), ch = -((-d.height) >> b->ov_hshift);
    for (int p = 0; p < 4; p++)
    {
        const bool chroma = p == 1 || p == 2;
        const int w = chroma ? cw : d.width, h = chroma ? ch : d.height;
        if (!plane[p] || stride[p] < w) return HBHIP_ERR_ARG;
        HBHIP_CHECK(ctx, hipMemcpy2DAsync(plane[p], stride[p], d.plane[p], d.stride[p], w, h, hipMemcpyDeviceToHost, ctx->stream));
    }
    HBHIP_CHECK(ctx, hipStreamSynchronize(ctx->stream));
    return HBHIP_OK;
}

extern "C" int hbhip_blend_apply_dev(hbhip_blend *b, const hbhip_dev_frame *frame)
{
    if (!b || !frame || b->biplanar) return HBHIP_ERR_ARG;
    hbhip_ctx *ctx = b->ctx;
    (void)hipSetDevice(ctx->device);
    BlendArgs a;
    for (int c = 0; c < 3; c++) { a.dst[c] = (uint8_t *)frame->plane[c]; a.pitch[c] = frame->stride[c]; }
    a.width = b->geo.width; a.height = b->geo.height; a.cw = b->geo.pw[1]; a.ch = b->geo.ph[1];
    a.wshift = b->geo.log2_cw; a.hshift = b->geo.log2_ch; a.shift = b->geo.depth - 8;
    for (int i = 0; i < 2; i++) { a.coeff[0][i] = b->coeff[0][i]; a.coeff[1][i] = b->coeff[1][i]; }
    const dim3 blk(64, 4);
    for (const hbhip_blend::Launch &l : b->launches)
    {
        if (b->subsample)
        {
            if (b->geo.bps == 1) HBHIP_LAUNCH(ctx, "blend_subsample", blend_subsample_kernel<uint8_t>, l.grid, blk, 0, a, l.g);
            else                 HBHIP_LAUNCH(ctx, "blend_subsample", blend_subsample_kernel<uint16_t>, l.grid, blk, 0, a, l.g);
        }
        else
        {
            if (b->geo.bps == 1) HBHIP_LAUNCH(ctx, "blend", blend_same_kernel<uint8_t>, l.grid, blk, 0, a, l.g);
            else                 HBHIP_LAUNCH(ctx, "blend", blend_same_kernel<uint16_t>, l.grid, blk, 0, a, l.g);
        }
    }
    HBHIP_CHECK(ctx, hipGetLastError());
    return HBHIP_OK;
}

extern "C" int hbhip_blend_apply(hbhip_blend *b, const hbhip_host_frame *frame)
{
    if (!b || !frame || b->biplanar) return HBHIP_ERR_ARG;
    if (b->overlays.empty()) return HBHIP_OK;
    if (!b->staging)
    {
        int rc = hbhip_frame_alloc(b->ctx, b->geo.width, b->geo.height, b->geo.depth, b->geo.log2_cw, b->geo.log2_ch, &b->staging);
        if (rc != HBHIP_OK) return rc;
    }
    int rc = hbhip_frame_upload(b->staging, frame);
    if (rc != HBHIP_OK) return rc;
    hbhip_dev_frame d;
    rc = hbhip_frame_describe(b->staging, &d, nullptr, nullptr);
    if (rc != HBHIP_OK) return rc;
    rc = hbhip_blend_apply_dev(b, &d);
    if (rc == HBHIP_OK) rc = hbhip_frame_mark_ready(b->staging);        // the download waits for the compositor
    if (rc != HBHIP_OK) return rc;
    return hbhip_frame_download(b->staging, frame);
}

extern "C" int hbhip_blend_create_biplanar(hbhip_ctx *ctx, int width, int height, int depth, int chroma_location,
                                           int overlay_log2_chroma_w, int overlay_log2_chroma_h, hbhip_blend **out)
{
    if (!ctx || !out) return HBHIP_ERR_ARG;
    *out = nullptr;
    if ((depth != 8 && depth != 10) || width < 2 || height < 2) return HBHIP_ERR_UNSUPPORTED;
    const int rc = hbhip_blend_create(ctx, width, height, depth, 1, 1, chroma_location, overlay_log2_chroma_w,
                                      overlay_log2_chroma_h, out);
    if (rc == HBHIP_OK) (*out)->biplanar = true;
    return rc;
}

// H2D into the staging buffer, the overlays in list order on it in place (hb_blend_work :866-869), D2H
extern "C" int hbhip_blend_apply_biplanar(hbhip_blend *b, const hbhip_host_biplanar *frame)
{
    if (!b || !frame || !b->biplanar) return HBHIP_ERR_ARG;
    BiLayout l;
    hbhip_bi_layout(b->geo.width, b->geo.height, b->geo.depth, &l);
    for (int p = 0; p < 2; p++)
        if (frame->plane[p] == nullptr || frame->stride[p] < l.row_bytes[p]) return HBHIP_ERR_ARG;
    if (b->overlays.empty()) return HBHIP_OK;
    hbhip_ctx *ctx = b->ctx;
    (void)hipSetDevice(ctx->device);
    if (const int rc = b->bi_stage.reserve(ctx, l.bytes)) return rc;
    uint8_t *plane[2] = { b->bi_stage.get(), b->bi_stage.get() + (size_t)l.pitch[0] * l.rows[0] };
    for (int p = 0; p < 2; p++)
        HBHIP_CHECK(ctx, hipMemcpy2DAsync(plane[p], l.pitch[p], frame->plane[p], frame->stride[p], l.row_bytes[p], l.rows[p],
                                          hipMemcpyHostToDevice, ctx->stream));
    BlendArgs a;
    a.dst[0] = plane[0]; a.dst[1] = plane[1]; a.dst[2] = plane[1] + b->geo.bps;      // Cb Cr Cb Cr ...
    a.pitch[0] = l.pitch[0]; a.pitch[1] = a.pitch[2] = l.pitch[1];
    a.width = b->geo.width; a.height = b->geo.height; a.cw = b->geo.pw[1]; a.ch = b->geo.ph[1];
    a.wshift = a.hshift = 1; a.shift = b->geo.depth - 8;
    for (int i = 0; i < 2; i++) { a.coeff[0][i] = b->coeff[0][i]; a.coeff[1][i] = b->coeff[1][i]; }
    for (const hbhip_blend::Launch &ln : b->launches)
    {
        const int rc = hbhip_bi_blend_launch(ctx, b->subsample, b->geo.bps, ln.grid, a, ln.g);
        if (rc != HBHIP_OK) return rc;
    }
    HBHIP_CHECK(ctx, hipGetLastError());
    for (int p = 0; p < 2; p++)
        HBHIP_CHECK(ctx, hipMemcpy2DAsync(frame->plane[p], frame->stride[p], plane[p], l.pitch[p], l.row_bytes[p], l.rows[p],
                                          hipMemcpyDeviceToHost, ctx->stream));
    HBHIP_CHECK(ctx, hipStreamSynchronize(ctx->stream));
    return HBHIP_OK;
}
