// rgb_pack.hip - an 8-bit planar 4:2:0 frame as a packed 32-bit RGB picture (bgra / rgba / argb / abgr), the repack of
// hbhip_frame_download_rgb32: what `format=bgra` behind a device-resident run asks of the download adapter (hb_get_preview's
// list).
//
// The arithmetic is tests/rgb32_model.py's, bit for bit - libswscale's unscaled yuv2rgb path in its C form, restated: chroma
// taken nearest (one Cb / Cr pair for its 2 x 2 luma block), every chroma term a WHOLE number of luma steps
//     off(c, inc) = (c * inc >> 16) - (inc >> 9)
// into a clipped luma ramp whose entry k is clip8((yb + k * cy) >> 16), alpha 255.  swscale keeps the ramp and the offsets
// as tables in memory; here the ramp is evaluated: per channel of a pixel one v_mad_i32_i24 (Y * cy + a, a = yb + off * cy
// worked out once per chroma pair, i.e. per four pixels) and one v_med3_i32 against [0, 0xffffff] - the clip done ahead of
// the >> 16, so that the result byte is byte 2 of the clipped word and v_perm_b32 picks it while it packs: two perms a
// pixel put three such bytes and the constant 0xff in their places.  No shift, no table, no LDS.
//
// The byte order is decided per launch, in the arguments: the kernel knows a first, a middle (green) and a third colour
// byte; R and B trade places by trading their chroma plane and coefficients, and where alpha goes is the two perm selectors.
//
// A lane has 4 pixels of two rows: a dword of Y from each row, 16 bits each of Cb and Cr, two 16-byte stores.  A width with
// width % 4 == 2 ends its rows in a lane with two live pixels, which stores 8 bytes a row: no byte beyond 4 * width of a
// destination row is written.  What that lane reads beyond the width lies inside the frame's row pitch (checked below).
#include "hbhip_internal.h"

namespace {

struct RgbPack
{
    uint8_t       *dst;
    const uint8_t *y, *c0, *c2;      // luma; the chroma plane of the first colour byte (Cr for R, Cb for B) and of the third
    int      dpitch, ypitch, cpitch;
    unsigned lanes, pairs, width;    // lanes with work in a row pair; row pairs; pixels a row
    int      cy;                     // a luma step, 16.16
    int      inc0, inc2;             // the chroma increments in luma steps, 16.16: of the first and the third colour byte,
    int      incg0, incg2;           // and green's two, for the plane c0 and the plane c2
    int      yb0, ybg, yb2;          // yb - (inc >> 9) * cy for each channel (green: both of its terms)
    unsigned sel_a, sel_b;           // v_perm_b32 selectors: where alpha goes
};

__device__ __forceinline__ int clip_word(int v) { return min(max(v, 0), 0x00ffffff); }   // one v_med3_i32; byte 2: clip8(v >> 16)

__device__ __forceinline__ unsigned pack_pixel(const RgbPack &a, int y, int a0, int ag, int a2)
{
    const unsigned x0 = (unsigned)clip_word(__mul24(y, a.cy) + a0);
    const unsigned g  = (unsigned)clip_word(__mul24(y, a.cy) + ag);
    const unsigned x2 = (unsigned)clip_word(__mul24(y, a.cy) + a2);
    return __builtin_amdgcn_perm(x2, __builtin_amdgcn_perm(g, x0, a.sel_a), a.sel_b);
}

__global__ __launch_bounds__(256) void rgb32_pack_kernel(RgbPack a)
{
    const unsigned lane = blockIdx.x * 64u + threadIdx.x, pair = blockIdx.y * 4u + threadIdx.y;
    if (lane >= a.lanes || pair >= a.pairs) return;
    const uint8_t *yrow = a.y + (size_t)(2 * pair) * a.ypitch + (size_t)lane * 4;
    const unsigned y0 = *reinterpret_cast<const unsigned *>(yrow);
    const unsigned y1 = *reinterpret_cast<const unsigned *>(yrow + a.ypitch);
    const size_t cat = (size_t)pair * a.cpitch + (size_t)lane * 2;
    const unsigned p0 = *reinterpret_cast<const uint16_t *>(a.c0 + cat);
    const unsigned p2 = *reinterpret_cast<const uint16_t *>(a.c2 + cat);
    unsigned top[4], bot[4];
#pragma unroll
    for (int k = 0; k < 2; k++)
    {
        const int s0 = (int)((p0 >> (8 * k)) & 255u), s2 = (int)((p2 >> (8 * k)) & 255u);
        const int a0 = __mul24(__mul24(s0, a.inc0) >> 16, a.cy) + a.yb0;
        const int a2 = __mul24(__mul24(s2, a.inc2) >> 16, a.cy) + a.yb2;
        const int ag = __mul24((__mul24(s0, a.incg0) >> 16) + (__mul24(s2, a.incg2) >> 16), a.cy) + a.ybg;
#pragma unroll
        for (int j = 2 * k; j < 2 * k + 2; j++)
        {
            top[j] = pack_pixel(a, (int)((y0 >> (8 * j)) & 255u), a0, ag, a2);
            bot[j] = pack_pixel(a, (int)((y1 >> (8 * j)) & 255u), a0, ag, a2);
        }
    }
    uint8_t *d = a.dst + (size_t)(2 * pair) * a.dpitch + (size_t)lane * 16;
    if (lane * 4u + 4u <= a.width)
    {
        *reinterpret_cast<uint4 *>(d) = make_uint4(top[0], top[1], top[2], top[3]);
        *reinterpret_cast<uint4 *>(d + a.dpitch) = make_uint4(bot[0], bot[1], bot[2], bot[3]);
    }
    else                                                               // the row's last two pixels
    {
        *reinterpret_cast<uint2 *>(d) = make_uint2(top[0], top[1]);
        *reinterpret_cast<uint2 *>(d + a.dpitch) = make_uint2(bot[0], bot[1]);
    }
}

// ff_yuv2rgb_coeffs' rows {crv, cbu, cgu, cgv} by HB_COLR_MAT_* number (2, unspecified: BT.601, as in swscale)
const int *coeff_row(int matrix)
{
    static const int r709[4] = {117489, 138438, 13975, 34925}, r601[4] = {104597, 132201, 25675, 53279},
                     rfcc[4] = {104448, 132798, 24759, 53109}, r240[4] = {117579, 136230, 16907, 35559},
                     r2020[4] = {110013, 140363, 12277, 42626};
    switch (matrix)
    {
        case 1: return r709;
        case 2: case 5: case 6: return r601;
        case 4: return rfcc;
        case 7: return r240;
        case 9: case 10: return r2020;
        default: return nullptr;
    }
}

} // namespace

bool hbhip_rgb32_matrix_ok(int matrix) { return coeff_row(matrix) != nullptr; }

int hbhip_rgb32_pitch(int width) { return hbhip_align_up(4 * width, 64); }

int hbhip_rgb32_pack_launch(hbhip_ctx *ctx, hipStream_t stream, uint8_t *dst, int dpitch, const hbhip_frame *fr, int order,
                            int matrix, int full_range)
{
    const DevPicture &p = fr->pic;
    const int *row = coeff_row(matrix);
    const int w = fr->width, h = fr->height;
    if (!row || order < HBHIP_RGB32_BGRA || order > HBHIP_RGB32_ABGR || fr->depth != 8 || p.bps != 1 || fr->lcw != 1 || fr->lch != 1 ||
        w < 2 || h < 2 || (w & 1) || (h & 1) || h / 2 > 4 * 65535)
        return HBHIP_ERR_ARG;
    RgbPack a;
    a.lanes = (unsigned)(w + 3) / 4;
    a.pairs = (unsigned)h / 2;
    a.width = (unsigned)w;
    // what the kernel's addressing rests on: 16-byte destination rows that hold 4 * width bytes; a lane's dword of Y and its
    // 16 bits of either chroma plane inside the frame's rows, the last lane of a width % 4 == 2 row included
    if (!dst || ((uintptr_t)dst & 15) || (dpitch & 15) || dpitch < 4 * w || p.pitch[1] != p.pitch[2] || (p.pitch[0] & 3) || (p.pitch[1] & 1) ||
        (size_t)a.lanes * 4 > (size_t)p.pitch[0] || (size_t)a.lanes * 2 > (size_t)p.pitch[1] ||
        p.height[0] != h || p.height[1] != h / 2 || p.height[2] != h / 2)
        return HBHIP_ERR_ARG;
    for (int c = 0; c < 3; c++)
        if (!p.plane[c] || ((uintptr_t)p.plane[c] & 3)) return HBHIP_ERR_ARG;

    // ff_yuv2rgb_c_init_tables at brightness 0, contrast and saturation 1 (C's division: towards zero)
    int64_t cy = 1 << 16, yb = 0, c[4] = {row[0], row[1], -(int64_t)row[2], -(int64_t)row[3]};     // crv, cbu, cgu, cgv
    if (!full_range) { cy = cy * 255 / 219; yb = -16 * cy; }
    else for (int k = 0; k < 4; k++) c[k] = c[k] * 224 / 255;
    for (int k = 0; k < 4; k++) c[k] = (c[k] * (1 << 16) + 0x8000) / cy;
    yb += 0x8000;
    const int64_t crv = c[0], cbu = c[1], cgu = c[2], cgv = c[3];
    const bool r_first = order == HBHIP_RGB32_RGBA || order == HBHIP_RGB32_ARGB;
    const bool a_first = order == HBHIP_RGB32_ARGB || order == HBHIP_RGB32_ABGR;
    a.dst = dst;
    a.y = p.plane[0];
    a.c0 = p.plane[r_first ? 2 : 1];
    a.c2 = p.plane[r_first ? 1 : 2];
    a.dpitch = dpitch;
    a.ypitch = p.pitch[0];
    a.cpitch = p.pitch[1];
    a.cy = (int)cy;
    a.inc0 = (int)(r_first ? crv : cbu);
    a.inc2 = (int)(r_first ? cbu : crv);
    a.incg0 = (int)(r_first ? cgv : cgu);
    a.incg2 = (int)(r_first ? cgu : cgv);
    a.yb0 = (int)(yb - (a.inc0 >> 9) * cy);
    a.yb2 = (int)(yb - (a.inc2 >> 9) * cy);
    a.ybg = (int)(yb - ((cgu >> 9) + (cgv >> 9)) * cy);
    // v_perm_b32(S0, S1, sel): selector bytes 0-3 take S1's bytes, 4-7 S0's, 0x0c is 0x00, 0x0d is 0xff.  The inner perm has
    // S0 = green, S1 = the first colour byte; the outer S0 = the third colour byte, S1 = the inner result; byte 2 of each
    a.sel_a = a_first ? 0x0c06020du : 0x0c0c0602u;
    a.sel_b = a_first ? 0x06020100u : 0x0d060100u;
    const dim3 grid(hbhip_grid_x((a.lanes + 63) / 64), (a.pairs + 3) / 4), blk(64, 4);
    HBHIP_LAUNCH_ON(ctx, stream, "rgb32_pack", rgb32_pack_kernel, grid, blk, 0, a);
    HBHIP_CHECK(ctx, hipGetLastError());
    return HBHIP_OK;
}
