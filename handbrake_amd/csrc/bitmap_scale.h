// bitmap_scale.h — what hbhip_blend_set_bitmaps (blend.hip) hands the bitmap subtitle scaler (bitmap_scale.hip): the
// tables of sws_filter.h and the packed source planes, uploaded in one copy, and the launch.
#pragma once

#include "hbhip_internal.h"

constexpr int BMS_TILE_W = 64;           // output columns of a workgroup's tile: 16 lanes of four
constexpr int BMS_TILE_H = 16;           // output rows of it: 256 threads, one dword of a row each in the vertical pass
constexpr int BMS_MAX_ROWS = 384;        // source rows a tile may tap: 48 KiB of 16-bit intermediates in LDS

struct BitmapScaleArgs
{
    const uint8_t *src[4];               // Y, Cb, Cr, alpha: sw x sh, rows `spitch` bytes apart
    uint8_t       *dst[4];               // the overlay's planes in the store: dw x dh, `dpitch` a multiple of 16
    int spitch, dpitch, dw, dh, tx, ty;  // tx / ty: taps of an output column / row
    const int   *px, *py;                // first tapped source column / row of an output column / row (folded at the edges)
    const short *qx, *qy;                // 14-bit / 12-bit coefficients, tx / ty of them an output column / row
};

// the four planes in one launch on ctx->stream; rows: the most source rows a tile row of BMS_TILE_H output rows taps
int hbhip_bitmap_scale_launch(hbhip_ctx *ctx, const BitmapScaleArgs &a, int rows);
