// ass_compose.h — what hbhip_blend_set_ass_images (blend.hip) hands the compose kernel (ass_compose.hip): the tables it
// uploads in one copy, [boxes][images][glyph bitmaps], and the launch.
#pragma once

#include "hbhip_internal.h"

// One glyph image (ASS_Image) in the render's coordinates.  Its bitmap sits in the packed buffer at `off`, rows of `w`
// bytes back to back.
struct AssImageDev
{
    int off, w, h, x, y;
    unsigned yuva;                       // Y | Cb << 8 | Cr << 16 | a << 24  (a: libass's transparency, 0 = opaque)
    int pad[2];
};

// One box of render_ssa_subs (rendersub.c:646-662) = one overlay of the blend object's store: origin in the render's
// coordinates, the four planes (Y Cb Cr A) and their 16-byte-aligned strides as hbhip_blend_set_overlays lays them out.
struct AssBoxDev
{
    uint8_t *plane[4];
    int stride[4];
    int x, y, w, h;
};

constexpr int ASS_BITS_PAD = 16;         // zero bytes in front of and behind the bitmaps: the dword pairs of the first
                                         // and last row reach up to 3 bytes before and 7 behind an image
constexpr int ASS_TILE_W = 256;          // luma columns of a wave: 64 lanes of four
constexpr int ASS_TILE_WAVES = 4;        // waves (= tile rows) of a workgroup

struct AssArgs
{
    const AssBoxDev   *box;
    const AssImageDev *img;
    const uint8_t     *bits;             // 16-byte aligned; AssImageDev::off counts from here and is >= ASS_BITS_PAD
    int n_img;
    unsigned cx[2], cy[2];               // chroma-location weights (hbhip_blend::coeff)
};

// all boxes in one launch on ctx->stream: grid = (tiles across the widest box, workgroups down the tallest, boxes)
int hbhip_ass_compose_launch(hbhip_ctx *ctx, int wshift, int hshift, dim3 grid, const AssArgs &a);
