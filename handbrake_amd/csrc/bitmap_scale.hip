// bitmap_scale.hip — the reference's scale_subtitle (libhb/rendersub.c:242-305) on gfx950: a decoded bitmap subtitle (PGS,
// DVB, VOBSUB: YUVA 4:4:4, 8 bits) taken to the frame's scale with libswscale's `lanczos + accurate_rnd` arithmetic, straight
// into the blend object's overlay store.  PARITY UNPINNED like the rest of the swscale family: libswscale is outside the
// reference tree; the arithmetic is that of oracle/alias_oracle.c:orc_cropscale_plane_sws with chroma_h = 0 - on a 4:4:4
// picture every plane, alpha included, takes the luma filter - and the tables are sws_filter.h's.
//
// One launch per bitmap: grid z = plane, a workgroup owns a BMS_TILE_W x BMS_TILE_H tile of the output and runs both passes,
// the 15-bit intermediates staying in LDS.
//   horizontal (hScale8To15_c):  a thread keeps one output column of the tile and walks the source rows the tile's output
//       rows tap, four rows apart from its neighbour wave's: min((sum q14 * src) >> 7, 32767) -> int16 in LDS.  Its column's
//       position and coefficients do not change from row to row; the tap count comes from the table (6 for an upscale, about
//       6 / factor below 1: 22 to 24 at 0.25), which is why the rows a tile taps are counted on the host and sized into the
//       launch's LDS instead of being a constant of the kernel.
//   vertical (yuv2planeX_8_c):   a thread owns four adjacent columns of one output row: an 8-byte LDS read per tap,
//       clip8(((64 << 12) + sum q12 * h) >> 19), one dword store.  Rows end inside their 16-byte-aligned stride, so the last
//       dword of a row needs no mask; what it writes past the width is the scaled value of a zero column, 0.
// A launch this small is bound by filling and draining the device, not by its arithmetic: the tables and source bytes are
// read through the caches as they are.
#include "bitmap_scale.h"

namespace {

__global__ __launch_bounds__(256) void bitmap_scale_kernel(BitmapScaleArgs a)
{
    extern __shared__ __align__(16) int16_t hbuf[];                       // [rows the tile taps][BMS_TILE_W]
    const int x0 = blockIdx.x * BMS_TILE_W, y0 = blockIdx.y * BMS_TILE_H;
    if (x0 >= a.dw || y0 >= a.dh) return;
    const int y1 = min(y0 + BMS_TILE_H, a.dh);
    int r0 = a.py[y0], r1 = r0 + a.ty;                                     // the source rows [r0, r1) the tile taps
    for (int y = y0 + 1; y < y1; y++)
    {
        r0 = min(r0, a.py[y]);
        r1 = max(r1, a.py[y] + a.ty);
    }
    const uint8_t *__restrict__ src = a.src[blockIdx.z];

    const int lx = threadIdx.x & (BMS_TILE_W - 1), gx = x0 + lx;
    const bool live = gx < a.dw;
    const uint8_t *col = src + (live ? a.px[gx] : 0);
    const short *__restrict__ q = a.qx + (size_t)(live ? gx : 0) * a.tx;
    for (int r = threadIdx.x / BMS_TILE_W; r < r1 - r0; r += 256 / BMS_TILE_W)
    {
        int val = 0;
        if (live)
        {
            const uint8_t *row = col + (size_t)(r0 + r) * a.spitch;
            for (int j = 0; j < a.tx; j++) val += (int)row[j] * (int)q[j];
            val = min(val >> 7, (1 << 15) - 1);
        }
        hbuf[r * BMS_TILE_W + lx] = (int16_t)val;
    }
    __syncthreads();

    const int gy = y0 + (int)threadIdx.x / (BMS_TILE_W / 4), c0 = 4 * (threadIdx.x & (BMS_TILE_W / 4 - 1));
    if (gy >= a.dh || x0 + c0 >= a.dw) return;
    const short *__restrict__ qv = a.qy + (size_t)gy * a.ty;
    const int16_t *h = hbuf + (a.py[gy] - r0) * BMS_TILE_W + c0;
    int acc[4] = { 64 << 12, 64 << 12, 64 << 12, 64 << 12 };
    for (int j = 0; j < a.ty; j++)
    {
        const short4 v = *reinterpret_cast<const short4 *>(h + j * BMS_TILE_W);
        const int c = qv[j];
        acc[0] += v.x * c; acc[1] += v.y * c; acc[2] += v.z * c; acc[3] += v.w * c;
    }
    unsigned out = 0;
#pragma unroll
    for (int k = 0; k < 4; k++) out |= (unsigned)min(max(acc[k] >> 19, 0), 255) << (8 * k);
    *reinterpret_cast<unsigned *>(a.dst[blockIdx.z] + (size_t)gy * a.dpitch + x0 + c0) = out;
}

} // namespace

int hbhip_bitmap_scale_launch(hbhip_ctx *ctx, const BitmapScaleArgs &a, int rows)
{
    if (rows < 1 || rows > BMS_MAX_ROWS || a.dw < 1 || a.dh < 1 || (a.dpitch & 15)) return HBHIP_ERR_UNSUPPORTED;
    const dim3 grid((a.dw + BMS_TILE_W - 1) / BMS_TILE_W, (a.dh + BMS_TILE_H - 1) / BMS_TILE_H, 4);
    HBHIP_LAUNCH(ctx, "bitmap_scale", bitmap_scale_kernel, grid, dim3(256), (size_t)rows * BMS_TILE_W * sizeof(int16_t), a);
    HBHIP_CHECK(ctx, hipGetLastError());
    return HBHIP_OK;
}
