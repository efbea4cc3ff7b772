// biplanar.hip — NV12 / P010LE on gfx950: the repack between a biplanar staging buffer and a planar 4:2:0 frame, and
// the reference's biplanar compositor forms applied to the staging buffer in place.
//
//   bi_split_kernel           staging -> the three planes of a planar frame (NV12: luma copied, chroma de-interleaved;
//                             P010LE: every sample >> 6 into a 10-bit planar frame)
//   bi_merge_kernel           the inverse (P010LE: every sample << 6, low six bits zero)
//   bi_surface_split_kernel / bi_surface_merge_kernel
//                             the same pair between a device surface - a pitch of its own per plane, the planes where their
//                             maker put them - and the frame, without a staging buffer (below)
//   bi_widen_merge_kernel     an 8-bit planar frame as P010LE, every sample t as t | t << 8, into the staging buffer or a
//                             surface (below)
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

// The arithmetic of one 16-byte unit of the merges, shared by the staging kernel and the surface kernel (they differ in
// addressing only): a luma unit, and 8 bytes of Cb and 8 of Cr into an interleaved unit.  The two splits keep theirs in
// their bodies: through such functions the compiler allots bi_surface_split_kernel's registers and orders its shifts
// another way, and the kernels are held to the instructions they had.
template <typename PIX> __device__ __forceinline__ uint4 luma_to_biplanar(uint4 v)
{
    v.x = to_biplanar<PIX>(v.x); v.y = to_biplanar<PIX>(v.y); v.z = to_biplanar<PIX>(v.z); v.w = to_biplanar<PIX>(v.w);
    return v;
}
template <typename PIX> __device__ __forceinline__ uint4 chroma_merge(uint2 cb, uint2 cr)
{
    uint4 v;
    v.x = to_biplanar<PIX>(__builtin_amdgcn_perm(cr.x, cb.x, Sel<PIX>::zip_lo));
    v.y = to_biplanar<PIX>(__builtin_amdgcn_perm(cr.x, cb.x, Sel<PIX>::zip_hi));
    v.z = to_biplanar<PIX>(__builtin_amdgcn_perm(cr.y, cb.y, Sel<PIX>::zip_lo));
    v.w = to_biplanar<PIX>(__builtin_amdgcn_perm(cr.y, cb.y, Sel<PIX>::zip_hi));
    return v;
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
        const uint4 v = *reinterpret_cast<const uint4 *>(a.plane[0] + (size_t)u * 16);
        *reinterpret_cast<uint4 *>(a.stage + (size_t)u * 16) = luma_to_biplanar<PIX>(v);
        return;
    }
    const unsigned c = u - a.luma_units;
    if (c >= a.chroma_units) return;
    const unsigned row = c / a.chroma_units_row, col = c - row * a.chroma_units_row;
    const size_t at = (size_t)row * a.cpitch + (size_t)col * 8;
    const uint2 cb = *reinterpret_cast<const uint2 *>(a.plane[1] + at);
    const uint2 cr = *reinterpret_cast<const uint2 *>(a.plane[2] + at);
    *reinterpret_cast<uint4 *>(a.stage + (size_t)a.luma_units * 16 + (size_t)row * a.spitch1 + (size_t)col * 16) = chroma_merge<PIX>(cb, cr);
}

// The same repack between a planar frame and a device surface (hbhip_surface): a picture whose two planes have a pitch of
// their own each (any multiple of 16 that holds the row), padded rows behind them, and need not lie back to back.  Rows on
// blockIdx.y - the luma rows, then the chroma rows - and one 16-byte unit of the interleaved side per lane along x: no
// division, and both sides are addressed by row and pitch.
//   split   writes EVERY unit of the frame's row, up to the frame's pitch: from the surface's row as far as the surface's
//           pitch reaches (its padding travels, as a host picture's does), zero beyond - the rule of bi_split_kernel.
//           Reads stay inside pitch * rows of either surface plane.
//   merge   writes [0, align16(row bytes)) of the surface's row and nothing else of the surface: the rest of the pitch, the
//           padded rows and whatever lies between the planes are not this library's.
struct BiSurface
{
    uint8_t *splane[2];              // the surface
    uint8_t *plane[3];               // the planar frame
    int spitch[2];
    int fpitch[2];                   // of the frame's luma plane / of its chroma planes
    unsigned rows0;                  // luma rows; the grid's y runs over them and the chroma rows behind them
    unsigned units[2];               // lanes with work in a luma / chroma row (split: the frame's row, merge: the samples')
    unsigned sunits[2];              // split: units the surface's row holds, spitch / 16
};

template <typename PIX>
__global__ __launch_bounds__(256) void bi_surface_split_kernel(BiSurface a)
{
    const unsigned u = blockIdx.x * 256u + threadIdx.x;
    if (blockIdx.y < a.rows0)
    {
        if (u >= a.units[0]) return;
        uint4 v = make_uint4(0, 0, 0, 0);
        if (u < a.sunits[0])
        {
            v = *reinterpret_cast<const uint4 *>(a.splane[0] + (size_t)blockIdx.y * a.spitch[0] + (size_t)u * 16);
            v.x = to_planar<PIX>(v.x); v.y = to_planar<PIX>(v.y); v.z = to_planar<PIX>(v.z); v.w = to_planar<PIX>(v.w);
        }
        *reinterpret_cast<uint4 *>(a.plane[0] + (size_t)blockIdx.y * a.fpitch[0] + (size_t)u * 16) = v;
        return;
    }
    if (u >= a.units[1]) return;
    const unsigned row = blockIdx.y - a.rows0;
    uint4 v = make_uint4(0, 0, 0, 0);
    if (u < a.sunits[1])
        v = *reinterpret_cast<const uint4 *>(a.splane[1] + (size_t)row * a.spitch[1] + (size_t)u * 16);
    uint2 cb, cr;
    cb.x = to_planar<PIX>(__builtin_amdgcn_perm(v.y, v.x, Sel<PIX>::even));
    cb.y = to_planar<PIX>(__builtin_amdgcn_perm(v.w, v.z, Sel<PIX>::even));
    cr.x = to_planar<PIX>(__builtin_amdgcn_perm(v.y, v.x, Sel<PIX>::odd));
    cr.y = to_planar<PIX>(__builtin_amdgcn_perm(v.w, v.z, Sel<PIX>::odd));
    const size_t at = (size_t)row * a.fpitch[1] + (size_t)u * 8;
    *reinterpret_cast<uint2 *>(a.plane[1] + at) = cb;
    *reinterpret_cast<uint2 *>(a.plane[2] + at) = cr;
}

template <typename PIX>
__global__ __launch_bounds__(256) void bi_surface_merge_kernel(BiSurface a)
{
    const unsigned u = blockIdx.x * 256u + threadIdx.x;
    if (blockIdx.y < a.rows0)
    {
        if (u >= a.units[0]) return;
        const uint4 v = *reinterpret_cast<const uint4 *>(a.plane[0] + (size_t)blockIdx.y * a.fpitch[0] + (size_t)u * 16);
        *reinterpret_cast<uint4 *>(a.splane[0] + (size_t)blockIdx.y * a.spitch[0] + (size_t)u * 16) = luma_to_biplanar<PIX>(v);
        return;
    }
    if (u >= a.units[1]) return;
    const unsigned row = blockIdx.y - a.rows0;
    const size_t at = (size_t)row * a.fpitch[1] + (size_t)u * 8;
    const uint2 cb = *reinterpret_cast<const uint2 *>(a.plane[1] + at);
    const uint2 cr = *reinterpret_cast<const uint2 *>(a.plane[2] + at);
    *reinterpret_cast<uint4 *>(a.splane[1] + (size_t)row * a.spitch[1] + (size_t)u * 16) = chroma_merge<PIX>(cb, cr);
}

// The widening merge: an 8-bit planar 4:2:0 frame into a P010LE picture, every sample t as the 16-bit word t | t << 8 - the
// byte twice, what libswscale's unscaled yuv420p -> p010le path writes (NOT t << 8: the low byte is t).  One
// kernel for both destinations, which differ in addressing only once the staging buffer's luma pitch, align64(2 w), is no
// longer the frame's, align64(w): rows on blockIdx.y as in the surface kernels, both sides by row and pitch.  A lane writes
// one 16-byte unit and reads 8 bytes of luma or 4 of Cb and 4 of Cr; one v_perm_b32 per dword written, nothing else.
//   staging   units = the destination's whole row (pitch / 16): the frame's row padding is read (8 * units <= align64(w),
//             4 * units <= align64(cw)) and the destination row's written, as in bi_merge_kernel
//   surface   units = align16(row bytes) / 16: [0, align16(row bytes)) of each sample row and nothing else of the surface
struct BiWiden
{
    uint8_t *dplane[2];              // the P010LE picture: a staging buffer's two planes, or a surface's
    const uint8_t *plane[3];         // the 8-bit planar frame
    int dpitch[2];
    int fpitch[2];                   // of the frame's luma plane / of its chroma planes
    unsigned rows0;                  // luma rows; the grid's y runs over them and the chroma rows behind them
    unsigned units[2];               // lanes with work in a luma / chroma row
};

__global__ __launch_bounds__(256) void bi_widen_merge_kernel(BiWiden a)
{
    const unsigned u = blockIdx.x * 256u + threadIdx.x;
    uint4 v;
    if (blockIdx.y < a.rows0)
    {
        if (u >= a.units[0]) return;
        const uint2 y = *reinterpret_cast<const uint2 *>(a.plane[0] + (size_t)blockIdx.y * a.fpitch[0] + (size_t)u * 8);
        v.x = __builtin_amdgcn_perm(y.x, y.x, 0x01010000u);
        v.y = __builtin_amdgcn_perm(y.x, y.x, 0x03030202u);
        v.z = __builtin_amdgcn_perm(y.y, y.y, 0x01010000u);
        v.w = __builtin_amdgcn_perm(y.y, y.y, 0x03030202u);
        *reinterpret_cast<uint4 *>(a.dplane[0] + (size_t)blockIdx.y * a.dpitch[0] + (size_t)u * 16) = v;
        return;
    }
    if (u >= a.units[1]) return;
    const unsigned row = blockIdx.y - a.rows0;
    const size_t at = (size_t)row * a.fpitch[1] + (size_t)u * 4;
    const unsigned cb = *reinterpret_cast<const unsigned *>(a.plane[1] + at);
    const unsigned cr = *reinterpret_cast<const unsigned *>(a.plane[2] + at);
    v.x = __builtin_amdgcn_perm(cr, cb, 0x04040000u);                  // cb0 cb0 cr0 cr0
    v.y = __builtin_amdgcn_perm(cr, cb, 0x05050101u);
    v.z = __builtin_amdgcn_perm(cr, cb, 0x06060202u);
    v.w = __builtin_amdgcn_perm(cr, cb, 0x07070303u);
    *reinterpret_cast<uint4 *>(a.dplane[1] + (size_t)row * a.dpitch[1] + (size_t)u * 16) = v;
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

int hbhip_bi_surface_launch(hbhip_ctx *ctx, hipStream_t stream, bool merge, const hbhip_surface *s, const hbhip_frame *fr)
{
    BiLayout l;
    hbhip_bi_layout(fr->width, fr->height, fr->depth, &l);
    const DevPicture &p = fr->pic;
    // what the kernels' addressing rests on: a frame as hbhip_frame_alloc lays it out, a surface as hbhip_surface_wrap admits it
    if (s->width != fr->width || s->height != fr->height || s->depth != fr->depth || p.pitch[1] != p.pitch[2] ||
        (p.pitch[0] & 15) || (p.pitch[1] & 7) || p.pitch[0] < hbhip_align_up(l.row_bytes[0], 16) ||
        p.pitch[1] * 2 < hbhip_align_up(l.row_bytes[1], 16) ||
        p.height[0] != l.rows[0] || p.height[1] != l.rows[1] || p.height[2] != l.rows[1] || l.rows[0] + l.rows[1] > 65535)
        return HBHIP_ERR_ARG;
    BiSurface a;
    for (int c = 0; c < 3; c++)
    {
        if (!p.plane[c] || ((uintptr_t)p.plane[c] & 15)) return HBHIP_ERR_ARG;
        a.plane[c] = p.plane[c];
    }
    for (int c = 0; c < 2; c++)
    {
        a.splane[c] = s->plane[c];
        a.spitch[c] = s->pitch[c];
        if (!s->plane[c] || ((uintptr_t)s->plane[c] & 15) || (s->pitch[c] & 15) || s->pitch[c] < l.row_bytes[c]) return HBHIP_ERR_ARG;
        a.sunits[c] = (unsigned)s->pitch[c] / 16;
        // merge: the samples' units (inside both pitches, see above); split: the frame's whole row, in units of the interleaved side
        a.units[c] = merge ? (unsigned)hbhip_align_up(l.row_bytes[c], 16) / 16 : c == 0 ? (unsigned)p.pitch[0] / 16 : (unsigned)p.pitch[1] / 8;
    }
    a.fpitch[0] = p.pitch[0];
    a.fpitch[1] = p.pitch[1];
    a.rows0 = (unsigned)l.rows[0];
    const unsigned most = a.units[0] > a.units[1] ? a.units[0] : a.units[1];
    const dim3 grid(hbhip_grid_x((most + 255) / 256), (unsigned)(l.rows[0] + l.rows[1])), blk(256);
    if (merge)
    {
        if (p.bps == 1) HBHIP_LAUNCH_ON(ctx, stream, "bi_surface_merge", bi_surface_merge_kernel<uint8_t>, grid, blk, 0, a);
        else            HBHIP_LAUNCH_ON(ctx, stream, "bi_surface_merge", bi_surface_merge_kernel<uint16_t>, grid, blk, 0, a);
    }
    else
    {
        if (p.bps == 1) HBHIP_LAUNCH_ON(ctx, stream, "bi_surface_split", bi_surface_split_kernel<uint8_t>, grid, blk, 0, a);
        else            HBHIP_LAUNCH_ON(ctx, stream, "bi_surface_split", bi_surface_split_kernel<uint16_t>, grid, blk, 0, a);
    }
    HBHIP_CHECK(ctx, hipGetLastError());
    return HBHIP_OK;
}

// bi_widen_merge_kernel from the 8-bit frame `fr` into the P010LE picture at dplane / dpitch; `whole_rows`: the staging rule
static int bi_widen_launch(hbhip_ctx *ctx, hipStream_t stream, uint8_t *const dplane[2], const int dpitch[2], bool whole_rows,
                           const hbhip_frame *fr)
{
    BiLayout l;
    hbhip_bi_layout(fr->width, fr->height, 10, &l);
    const DevPicture &p = fr->pic;
    if (fr->depth != 8 || p.bps != 1 || fr->lcw != 1 || fr->lch != 1 || p.pitch[1] != p.pitch[2] || (p.pitch[0] & 7) || (p.pitch[1] & 3) ||
        p.height[0] != l.rows[0] || p.height[1] != l.rows[1] || p.height[2] != l.rows[1] || l.rows[0] + l.rows[1] > 65535)
        return HBHIP_ERR_ARG;
    BiWiden a;
    for (int c = 0; c < 3; c++)
    {
        if (!p.plane[c] || ((uintptr_t)p.plane[c] & 15)) return HBHIP_ERR_ARG;
        a.plane[c] = p.plane[c];
    }
    a.fpitch[0] = p.pitch[0];
    a.fpitch[1] = p.pitch[1];
    for (int c = 0; c < 2; c++)
    {
        if (!dplane[c] || ((uintptr_t)dplane[c] & 15) || (dpitch[c] & 15) || dpitch[c] < l.row_bytes[c]) return HBHIP_ERR_ARG;
        a.dplane[c] = dplane[c];
        a.dpitch[c] = dpitch[c];
        a.units[c] = (unsigned)(whole_rows ? dpitch[c] : hbhip_align_up(l.row_bytes[c], 16)) / 16;
        // what a lane reads, 8 bytes of luma or 4 of either chroma plane a unit, stays inside the frame's row
        if ((size_t)a.units[c] * (c == 0 ? 8 : 4) > (size_t)a.fpitch[c]) return HBHIP_ERR_ARG;
    }
    a.rows0 = (unsigned)l.rows[0];
    const unsigned most = a.units[0] > a.units[1] ? a.units[0] : a.units[1];
    const dim3 grid(hbhip_grid_x((most + 255) / 256), (unsigned)(l.rows[0] + l.rows[1])), blk(256);
    if (whole_rows) HBHIP_LAUNCH_ON(ctx, stream, "bi_merge_widen", bi_widen_merge_kernel, grid, blk, 0, a);
    else            HBHIP_LAUNCH_ON(ctx, stream, "bi_surface_merge_widen", bi_widen_merge_kernel, grid, blk, 0, a);
    HBHIP_CHECK(ctx, hipGetLastError());
    return HBHIP_OK;
}

int hbhip_bi_widen_repack_launch(hbhip_ctx *ctx, hipStream_t stream, uint8_t *stage, const hbhip_frame *fr)
{
    BiLayout l;
    hbhip_bi_layout(fr->width, fr->height, 10, &l);
    uint8_t *const dplane[2] = {stage, stage + (size_t)l.pitch[0] * l.rows[0]};
    return bi_widen_launch(ctx, stream, dplane, l.pitch, true, fr);
}

int hbhip_bi_widen_surface_launch(hbhip_ctx *ctx, hipStream_t stream, const hbhip_surface *s, const hbhip_frame *fr)
{
    if (s->width != fr->width || s->height != fr->height || s->depth != 10) return HBHIP_ERR_ARG;
    return bi_widen_launch(ctx, stream, s->plane, s->pitch, false, fr);
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
