// blend_body.h — what the planar compositor kernels (blend.hip) and the biplanar ones (biplanar.hip) share: the launch
// arguments and the two kernel bodies, one template each over the sample type and the frame's layout.
//
//   BI = false   planar frames: blend8on8 :425-509 / blend8on1x :511-604, blend_subsample_8on8 :236-328 / _8on1x :48-140
//   BI = true    NV12 / P010 in place: blend8onbi8 :606-691 / blend8onbi1x :693-786,
//                blend_subsample_8onbi8 :330-423 / _8onbi1x :142-234
//
// The biplanar forms differ from the planar ones in three places only:
//  * Cb and Cr are the even and odd samples of plane 1 (dst[1] = the plane, dst[2] = one sample further, step 2);
//  * the 16-bit form works on the MSB-aligned samples as stored: the overlay sample enters as av_bswap16 of an 8-bit value,
//    v << 8, while alpha and max stay those of the depth (a << 2, 1023) - :193, :214, :747, :778;
//  * blend_subsample_8onbi8 alone has no `oy + yz < height` / `ox + xz < width` bounds on its two inner loops (:388-390
//    against :294-296, :200-202, :106-108): an overlay that ends inside a chroma block weighs the samples beyond its edge
//    in, unblended.
#pragma once

#include "hbhip_internal.h"

struct OverlayDev
{
    const uint8_t *plane[4];
    int stride[4];
    int x, y, width, height;
};

constexpr int BL_GROUP = 8;          // overlays per launch
struct OverlayGroup
{
    OverlayDev o[BL_GROUP];
    int bx0[BL_GROUP], by0[BL_GROUP];    // blend_subsample_kernel: the first frame chroma sample the overlay touches
};

struct BlendArgs
{
    uint8_t *dst[3];
    int pitch[3];
    int width, height, cw, ch;       // frame luma and chroma dimensions
    int wshift, hshift, shift;
    unsigned coeff[2][2];            // chroma-location weights of the samples under one chroma sample
};

template <typename PIX> __device__ __forceinline__ PIX *row_of(uint8_t *plane, int pitch, int y)
{
    return reinterpret_cast<PIX *>(plane + (size_t)y * pitch);
}

// grid: overlay chroma samples (xx, yy) in the overlay's own coordinates
template <typename PIX, bool BI>
__device__ __forceinline__ void blend_same_body(const BlendArgs &a, const OverlayGroup &G)
{
    constexpr int CS = BI ? 2 : 1;
    const int ss = BI ? (sizeof(PIX) == 2 ? 8 : 0) : a.shift;
    const OverlayDev &o = G.o[blockIdx.z];
    const int xx = blockIdx.x * blockDim.x + threadIdx.x, yy = blockIdx.y * blockDim.y + threadIdx.y;
    const int left = o.x, top = o.y;
    const int x0 = left < 0 ? -left : 0, y0 = top < 0 ? -top : 0;
    int ww = o.width, hh = o.height;
    if (o.width - x0 > a.width - left) ww = a.width - left + x0;
    if (o.height - y0 > a.height - top) hh = a.height - top + y0;
    const unsigned max = (256u << a.shift) - 1;

    // the luma samples of this block
    for (int j = 0; j < (1 << a.hshift); j++)
        for (int i = 0; i < (1 << a.wshift); i++)
        {
            const int lx = (xx << a.wshift) + i, ly = (yy << a.hshift) + j;
            if (lx < x0 || lx >= ww || ly < y0 || ly >= hh) continue;
            const int dx = left + lx, dy = top + ly;
            if (dx >= a.width || dy >= a.height) continue;
            const unsigned al = (unsigned)o.plane[3][(size_t)ly * o.stride[3] + lx] << a.shift;
            const unsigned s = (unsigned)o.plane[0][(size_t)ly * o.stride[0] + lx] << ss;
            PIX *d = row_of<PIX>(a.dst[0], a.pitch[0], dy) + dx;
            *d = (PIX)(((unsigned)*d * (max - al) + s * al) / max);
        }
    // its chroma sample
    if (xx < (x0 >> a.wshift) || xx >= (ww >> a.wshift) || yy < (y0 >> a.hshift) || yy >= (hh >> a.hshift)) return;
    const int dx = (left >> a.wshift) + xx, dy = yy + (top >> a.hshift);
    if (dx < 0 || dy < 0 || dx >= a.cw || dy >= a.ch) return;
    const unsigned al = (unsigned)o.plane[3][(size_t)(yy << a.hshift) * o.stride[3] + (xx << a.wshift)] << a.shift;
#pragma unroll
    for (int c = 1; c < 3; c++)
    {
        const unsigned s = (unsigned)o.plane[c][(size_t)yy * o.stride[c] + xx] << ss;
        PIX *d = row_of<PIX>(a.dst[c], a.pitch[c], dy) + dx * CS;
        *d = (PIX)(((unsigned)*d * (max - al) + s * al) / max);
    }
}

// grid: frame chroma samples starting at (bx0, by0) = the first one the overlay touches
template <typename PIX, bool BI>
__device__ __forceinline__ void blend_subsample_body(const BlendArgs &a, const OverlayGroup &G)
{
    constexpr int CS = BI ? 2 : 1;
    constexpr bool BOUNDED = !(BI && sizeof(PIX) == 1);
    const int ss = BI ? (sizeof(PIX) == 2 ? 8 : 0) : a.shift;
    const OverlayDev &o = G.o[blockIdx.z];
    const int bx0 = G.bx0[blockIdx.z], by0 = G.by0[blockIdx.z];
    const int cx = bx0 + blockIdx.x * blockDim.x + threadIdx.x, cy = by0 + blockIdx.y * blockDim.y + threadIdx.y;
    const int x0 = o.x, y0 = o.y;
    const int ow = o.width <= a.width ? o.width : a.width;          // :74-75 with left == x0
    const int oh = o.height <= a.height ? o.height : a.height;
    const int xx = cx << a.wshift, yy = cy << a.hshift;
    const int ox = xx - x0, oy = yy - y0;
    if (cx >= a.cw || cy >= a.ch || ox >= ow || oy >= oh) return;
    const unsigned max = (256u << a.shift) - 1;

    PIX *du = row_of<PIX>(a.dst[1], a.pitch[1], cy) + cx * CS, *dv = row_of<PIX>(a.dst[2], a.pitch[2], cy) + cx * CS;
    const unsigned cur_u = *du, cur_v = *dv;
    unsigned acc_u = 0, acc_v = 0, total = 0;
    for (int yz = 0; yz < (1 << a.hshift) && (!BOUNDED || oy + yz < oh); yz++)
        for (int xz = 0; xz < (1 << a.wshift) && (!BOUNDED || ox + xz < ow); xz++)
        {
            const unsigned coeff = a.coeff[0][xz] * a.coeff[1][yz];
            unsigned ru = cur_u, rv = cur_v;
            if (ox + xz >= 0 && oy + yz >= 0 && (BOUNDED || (ox + xz < ow && oy + yz < oh)))
            {
                const size_t row = (size_t)(oy + yz);
                const int col = ox + xz;
                const unsigned al = (unsigned)o.plane[3][row * o.stride[3] + col] << a.shift;
                const unsigned su = (unsigned)o.plane[1][row * o.stride[1] + col] << ss;
                const unsigned sv = (unsigned)o.plane[2][row * o.stride[2] + col] << ss;
                ru = (ru * (max - al) + su * al + (max >> 1)) / max;
                rv = (rv * (max - al) + sv * al + (max >> 1)) / max;
                // the luma sample at the same place
                if (xx + xz < a.width && yy + yz < a.height)
                {
                    const unsigned sy = (unsigned)o.plane[0][row * o.stride[0] + col] << ss;
                    PIX *d = row_of<PIX>(a.dst[0], a.pitch[0], yy + yz) + xx + xz;
                    *d = (PIX)(((unsigned)*d * (max - al) + sy * al + (max >> 1)) / max);
                }
            }
            acc_u += coeff * ru;
            acc_v += coeff * rv;
            total += coeff;
        }
    if (total)
    {
        *du = (PIX)((acc_u + (total >> 1)) / total);
        *dv = (PIX)((acc_v + (total >> 1)) / total);
    }
}

// biplanar.hip: the BI = true kernels on ctx->stream (bps: bytes per sample)
int hbhip_bi_blend_launch(hbhip_ctx *ctx, bool subsample, int bps, dim3 grid, const BlendArgs &a, const OverlayGroup &g);
