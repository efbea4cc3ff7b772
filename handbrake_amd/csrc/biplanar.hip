// biplanar.hip — NV12 / P010LE on gfx950: the repack between a biplanar staging buffer and a planar 4:2:0 frame, and
// the reference's biplanar compositor forms applied to the staging buffer in place.
//
//   bi_split_kernel           staging -> the three planes of a planar frame (NV12: luma copied, chroma de-interleaved;
//                             P010LE: every sample >> 6 into a 10-bit planar frame)
//   bi_merge_kernel           the inverse (P010LE: every sample << 6, low six bits zero)
//   blend_bi_same_kernel      blend8onbi8 :606-691 / blend8onbi1x :693-786
//   blend_bi_subsample_kernel blend_subsample_8onbi8 :330-423 / blend_subsample_8onbi1x :142-234   (blend_body.h)
//
// The staging buffer is laid out the way hb_frame_buffer_init lays a biplanar 4:2:0 hb_buffer_t out (fifo.c:820-881):
// plane 0 is h rows, plane 1 ceil(h / 2) rows of interleaved Cb Cr, every row rounded up to 64 bytes, the planes back to
// back.  The frame's rows are rounded up to 64 bytes too (hbhip_frame_alloc), so that
//   * the luma plane has the same pitch on both sides and is one contiguous run of 16-byte units,
//   * a 16-byte unit of an interleaved chroma row is 8 bytes of the Cb row and 8 of the Cr row, and half the interleaved
//     pitch, align32(cw * bps), never exceeds the planar pitch, align64(cw * bps): a unit stays inside its rows on both
//     sides for every width.  Row padding is read on the source side and written on the destination side; nothing else.
//     Where the planar pitch is the larger one the split clears the rest of the row: the filters behind it read row
//     padding (lapsharp.c:145-157), a planar upload brings the host's along, and a recycled frame has stale bytes there.
// Pure bandwidth: a lane moves one unit with one 16-byte access on the interleaved side and one 16-byte (luma) or two
// 8-byte (chroma) accesses on the planar side; v_perm_b32 does the (de-)interleave, two lanes of 16 bits shift at once.
#include "blend_body.h"

namespace {

struct BiRepack
{
    uint8_t *stage;                  // plane 0, plane 1 behind it
    uint8_t *plane[3];               // the planar frame
    int cpitch;                      // of its chroma planes
    int spitch1;                     // of the staging buffer's plane 1
    unsigned luma_units;             // 16-byte units of the luma plane (pitch * rows / 16)
    unsigned stage_units_row;        // spitch1 / 16
    unsigned chroma_units_row;       // merge: stage_units_row; split: cpitch / 8, the whole planar row (see bi_split_kernel)
    unsigned chroma_units;           // chroma_units_row * chroma rows
};

// selectors of v_perm_b32(hi, lo): byte k of the result is byte sel[k] of {hi:lo}
template <typename PIX> struct Sel;
template <> struct Sel<uint8_t>
{
    static constexpr unsigned even = 0x06040200u, odd = 0x07050301u;         // de-interleave
    static constexpr unsigned zip_lo = 0x05010400u, zip_hi = 0x07030602u;    // interleave
};
template <> struct Sel<uint16_t>
{
    static constexpr unsigned even = 0x05040100u, odd = 0x07060302u;
    static constexpr unsigned zip_lo = 0x05040100u, zip_hi = 0x07060302u;
};

// P010LE <-> 10-bit samples, two to a dword; NV12: nothing
template <typename PIX> __device__ __forceinline__ unsigned to_planar(unsigned v)
{
    return sizeof(PIX) == 2 ? (v >> 6) & 0x03ff03ffu : v;
}
template <typename PIX> __device__ __forceinline__ unsigned to_biplanar(unsigned v)
{
    return sizeof(PIX) == 2 ? (v << 6) & 0xffc0ffc0u : v;
}

template <typename PIX>
__global__ __launch_bounds__(256) void bi_split_kernel(BiRepack a)
{
    const unsigned u = blockIdx.x * 256u + threadIdx.x;
    if (u < a.luma_units)
    {
        uint4 v = *reinterpret_cast<const uint4 *>(a.stage + (size_t)u * 16);
        v.x = to_planar<PIX>(v.x); v.y = to_planar<PIX>(v.y); v.z = to_planar<PIX>(v.z); v.w = to_planar<PIX>(v.w);
        *reinterpret_cast<uint4 *>(a.plane[0] + (size_t)u * 16) = v;
        return;
    }
    const unsigned c = u - a.luma_units;
    if (c >= a.chroma_units) return;
    const unsigned row = c / a.chroma_units_row, col = c - row * a.chroma_units_row;
    uint4 v = make_uint4(0, 0, 0, 0);
    if (col < a.stage_units_row)
        v = *reinterpret_cast<const uint4 *>(a.stage + (size_t)a.luma_units * 16 + (size_t)row * a.spitch1 + (size_t)col * 16);
    uint2 cb, cr;
    cb.x = to_planar<PIX>(__builtin_amdgcn_perm(v.y, v.x, Sel<PIX>::even));
    cb.y = to_planar<PIX>(__builtin_amdgcn_perm(v.w, v.z, Sel<PIX>::even));
    cr.x = to_planar<PIX>(__builtin_amdgcn_perm(v.y, v.x, Sel<PIX>::odd));
    cr.y = to_planar<PIX>(__builtin_amdgcn_perm(v.w, v.z, Sel<PIX>::odd));
    const size_t at = (size_t)row * a.cpitch + (size_t)col * 8;
    *reinterpret_cast<uint2 *>(a.plane[1] + at) = cb;
    *reinterpret_cast<uint2 *>(a.plane[2] + at) = cr;
}

template <typename PIX>
__global__ __launch_bounds__(256) void bi_merge_kernel(BiRepack a)
{
    const unsigned u = blockIdx.x * 256u + threadIdx.x;
    if (u < a.luma_units)
    {
        uint4 v = *reinterpret_cast<const uint4 *>(a.plane[0] + (size_t)u * 16);
        v.x = to_biplanar<PIX>(v.x); v.y = to_biplanar<PIX>(v.y); v.z = to_biplanar<PIX>(v.z); v.w = to_biplanar<PIX>(v.w);
        *reinterpret_cast<uint4 *>(a.stage + (size_t)u * 16) = v;
        return;
    }
    const unsigned c = u - a.luma_units;
    if (c >= a.chroma_units) return;
    const unsigned row = c / a.chroma_units_row, col = c - row * a.chroma_units_row;
    const size_t at = (size_t)row * a.cpitch + (size_t)col * 8;
    const uint2 cb = *reinterpret_cast<const uint2 *>(a.plane[1] + at);
    const uint2 cr = *reinterpret_cast<const uint2 *>(a.plane[2] + at);
    uint4 v;
    v.x = to_biplanar<PIX>(__builtin_amdgcn_perm(cr.x, cb.x, Sel<PIX>::zip_lo));
    v.y = to_biplanar<PIX>(__builtin_amdgcn_perm(cr.x, cb.x, Sel<PIX>::zip_hi));
    v.z = to_biplanar<PIX>(__builtin_amdgcn_perm(cr.y, cb.y, Sel<PIX>::zip_lo));
    v.w = to_biplanar<PIX>(__builtin_amdgcn_perm(cr.y, cb.y, Sel<PIX>::zip_hi));
    *reinterpret_cast<uint4 *>(a.stage + (size_t)a.luma_units * 16 + (size_t)row * a.spitch1 + (size_t)col * 16) = v;
}

template <typename PIX>
__global__ __launch_bounds__(256) void blend_bi_same_kernel(BlendArgs a, OverlayGroup G)
{
    blend_same_body<PIX, true>(a, G);
}

template <typename PIX>
__global__ __launch_bounds__(256) void blend_bi_subsample_kernel(BlendArgs a, OverlayGroup G)
{
    blend_subsample_body<PIX, true>(a, G);
}

} // namespace

void hbhip_bi_layout(int width, int height, int depth, BiLayout *l)
{
    const int bps = depth > 8 ? 2 : 1, cw = (width + 1) >> 1;
    l->pitch[0] = hbhip_align_up(width * bps, 64);
    l->pitch[1] = hbhip_align_up(2 * cw * bps, 64);
    l->row_bytes[0] = width * bps;
    l->row_bytes[1] = 2 * cw * bps;
    l->rows[0] = height;
    l->rows[1] = (height + 1) >> 1;
    l->bytes = (size_t)l->pitch[0] * l->rows[0] + (size_t)l->pitch[1] * l->rows[1];
}

int hbhip_bi_repack_launch(hbhip_ctx *ctx, hipStream_t stream, bool merge, uint8_t *stage, const hbhip_frame *fr)
{
    BiLayout l;
    hbhip_bi_layout(fr->width, fr->height, fr->depth, &l);
    const DevPicture &p = fr->pic;
    // what the kernels' addressing rests on (hbhip_frame_alloc gives exactly this)
    if (p.pitch[0] != l.pitch[0] || p.pitch[1] != p.pitch[2] || p.pitch[1] * 2 < l.pitch[1] || (p.pitch[1] & 7) ||
        p.height[0] != l.rows[0] || p.height[1] != l.rows[1] || p.height[2] != l.rows[1])
        return HBHIP_ERR_ARG;
    BiRepack a;
    a.stage = stage;
    for (int c = 0; c < 3; c++) a.plane[c] = p.plane[c];
    a.cpitch = p.pitch[1];
    a.spitch1 = l.pitch[1];
    a.luma_units = (unsigned)((size_t)l.pitch[0] * l.rows[0] / 16);
    a.stage_units_row = (unsigned)(l.pitch[1] / 16);
    a.chroma_units_row = merge ? a.stage_units_row : (unsigned)(p.pitch[1] / 8);
    a.chroma_units = a.chroma_units_row * (unsigned)l.rows[1];
    const dim3 grid((a.luma_units + a.chroma_units + 255) / 256), blk(256);
    if (merge)
    {
        if (p.bps == 1) HBHIP_LAUNCH_ON(ctx, stream, "bi_merge", bi_merge_kernel<uint8_t>, grid, blk, 0, a);
        else            HBHIP_LAUNCH_ON(ctx, stream, "bi_merge", bi_merge_kernel<uint16_t>, grid, blk, 0, a);
    }
    else
    {
        if (p.bps == 1) HBHIP_LAUNCH_ON(ctx, stream, "bi_split", bi_split_kernel<uint8_t>, grid, blk, 0, a);
        else            HBHIP_LAUNCH_ON(ctx, stream, "bi_split", bi_split_kernel<uint16_t>, grid, blk, 0, a);
    }
    HBHIP_CHECK(ctx, hipGetLastError());
    return HBHIP_OK;
}

int hbhip_bi_blend_launch(hbhip_ctx *ctx, bool subsample, int bps, dim3 grid, const BlendArgs &a, const OverlayGroup &g)
{
    const dim3 blk(64, 4);
    if (subsample)
    {
        if (bps == 1) HBHIP_LAUNCH(ctx, "blend_bi_subsample", blend_bi_subsample_kernel<uint8_t>, grid, blk, 0, a, g);
        else          HBHIP_LAUNCH(ctx, "blend_bi_subsample", blend_bi_subsample_kernel<uint16_t>, grid, blk, 0, a, g);
    }
    else
    {
        if (bps == 1) HBHIP_LAUNCH(ctx, "blend_bi", blend_bi_same_kernel<uint8_t>, grid, blk, 0, a, g);
        else          HBHIP_LAUNCH(ctx, "blend_bi", blend_bi_same_kernel<uint16_t>, grid, blk, 0, a, g);
    }
    return HBHIP_OK;
}
