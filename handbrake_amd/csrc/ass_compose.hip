// ass_compose.hip — the reference's compose_subsample_ass (libhb/rendersub.c:474-612) on gfx950: the glyph images libass
// renders for a text subtitle (SSA / ASS, SRT, TX3G, CC608) composed into the blend object's YUVA overlays, one per box of
// render_ssa_subs (:646-662), without the reference's 4-byte-per-pixel `compo` buffer.
//
// A lane owns four luma columns by (1 << hshift) rows of a box - whole chroma samples - and keeps their Y / Cb / Cr / A in
// registers.  It walks the images in list order (the result depends on it: the first writer of a pixel sets it, a later
// one blends, :525-542), subsamples the chroma (:576-598) and stores dwords (chroma of a 4:2:x overlay: two bytes).  A
// pixel has one owner: no LDS, no atomics.  A wave's tile is 256 columns by (1 << hshift) rows; box and image
// descriptors are wave-uniform (scalar loads), so an image that takes no part in the box (:503-505), misses the tile or
// is fully transparent is turned away by scalar compares before a lane looks at it.  Glyph rows start at arbitrary byte
// offsets: a lane reads the two aligned dwords around its four bytes and shifts them together (v_alignbyte_b32).
//
// Integer arithmetic as the reference has it, `/` included: bit-exact wherever the reference's result is defined.  Where
// a chroma sample has no weight (accu_c == 0, :593) the reference leaves what hb_frame_buffer_init's pool held; 0 is
// written here.  Such a sample lies under alpha 0 only and cannot reach a frame.
// The clipping of the chroma block at the box's bottom edge (:580) needs no code: an image lies wholly inside its box, so
// the rows beyond the edge keep alpha 0 and weigh nothing.
#include "ass_compose.h"

namespace {

__device__ __forceinline__ unsigned div255(unsigned x) { return ((x + ((x + 128) >> 8)) + 128) >> 8; }      // :476

// :523-542 for one pixel; `g` is the glyph's coverage there, `op` = 255 - the image's transparency
__device__ __forceinline__ void compose_pixel(unsigned g, unsigned op, unsigned fy, unsigned fu, unsigned fv,
                                              unsigned &Y, unsigned &U, unsigned &V, unsigned &A)
{
    const unsigned fa = div255(op * g);                                    // ssa_alpha :478-486
    if (!fa) return;
    if (A)
    {
        const unsigned ain = fa * 255, acomp = A * (255 - fa), res = ain + acomp;
        Y = (ain * fy + Y * acomp + (res >> 1)) / res;                     // ALPHA_BLEND :474-475
        U = (ain * fu + U * acomp + (res >> 1)) / res;
        V = (ain * fv + V * acomp + (res >> 1)) / res;
        A = div255(res);
    }
    else
    {
        Y = fy; U = fu; V = fv; A = fa;
    }
}

__device__ __forceinline__ unsigned pack4(const unsigned v[4]) { return v[0] | v[1] << 8 | v[2] << 16 | v[3] << 24; }

// grid: x = tiles of 256 luma columns, y = workgroups of 4 waves = 4 tile rows of (1 << HS) luma rows, z = box
template <int WS, int HS>
__global__ __launch_bounds__(ASS_TILE_W / 4 * ASS_TILE_WAVES) void ass_compose_kernel(AssArgs a)
{
    constexpr int R = 1 << HS;
    const AssBoxDev &bx = a.box[blockIdx.z];
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.y);
    const int tx0 = blockIdx.x * ASS_TILE_W, ty0 = (blockIdx.y * ASS_TILE_WAVES + wave) << HS;
    const int bw = bx.w, bh = bx.h, box_x = bx.x, box_y = bx.y;
    if (tx0 >= bw || ty0 >= bh) return;
    const int c0 = tx0 + 4 * threadIdx.x;                                  // the lane's first column, box coordinates

    unsigned Y[R][4] = {}, U[R][4] = {}, V[R][4] = {}, A[R][4] = {};       // calloc'd compo :494
    for (int i = 0; i < a.n_img; i++)
    {
        const AssImageDev im = a.img[i];
        // :503-505, where the box's x and y are unsigned: one pulled back past the origin (x1 = 0 under an odd crop, x = -1)
        // takes no image and stays empty
        if (!im.w || !im.h || (unsigned)im.x < (unsigned)box_x || im.x + im.w > box_x + bw ||
            (unsigned)im.y < (unsigned)box_y || im.y + im.h > box_y + bh)
            continue;
        const int ix0 = im.x - box_x, iy0 = im.y - box_y;
        if (ix0 >= tx0 + ASS_TILE_W || ix0 + im.w <= tx0 || iy0 >= ty0 + R || iy0 + im.h <= ty0) continue;
        const unsigned op = 255 - (im.yuva >> 24);
        if (!op) continue;                                                 // a == 255: ssa_alpha is 0 everywhere
        const unsigned fy = im.yuva & 255, fu = (im.yuva >> 8) & 255, fv = (im.yuva >> 16) & 255;
        // the lane's bytes [lo, hi) of its four lie inside the image
        const int lo = ix0 > c0 ? ix0 - c0 : 0, hi = ix0 + im.w - c0 < 4 ? ix0 + im.w - c0 : 4;
        if (lo >= hi) continue;
        const unsigned mask = (0xffffffffu << (8 * lo)) & (0xffffffffu >> (8 * (4 - hi)));
#pragma unroll
        for (int j = 0; j < R; j++)
        {
            const int r = ty0 + j - iy0;
            if (r < 0 || r >= im.h) continue;
            const int at = im.off + r * im.w + (c0 - ix0);                 // >= ASS_BITS_PAD - 3
            const unsigned *p = reinterpret_cast<const unsigned *>(a.bits + (at & ~3));
            const unsigned g = __builtin_amdgcn_alignbyte(p[1], p[0], (unsigned)at & 3u) & mask;
            if (!g) continue;
#pragma unroll
            for (int k = 0; k < 4; k++)
                compose_pixel((g >> (8 * k)) & 255, op, fy, fu, fv, Y[j][k], U[j][k], V[j][k], A[j][k]);
        }
    }

    if (c0 >= bw) return;                                                  // a row's dwords end inside its 16-byte-aligned stride
#pragma unroll
    for (int j = 0; j < R; j++)
        if (ty0 + j < bh)
        {
            *reinterpret_cast<unsigned *>(bx.plane[0] + (size_t)(ty0 + j) * bx.stride[0] + c0) = pack4(Y[j]);      // :573-574
            *reinterpret_cast<unsigned *>(bx.plane[3] + (size_t)(ty0 + j) * bx.stride[3] + c0) = pack4(A[j]);
        }
    // :576-598, the 4 >> WS chroma samples under the lane's columns.  As in the reference, every position of a block's row
    // reads the row's first pixel (:585-590 index without xz): a sample is made of the left column of its block, a row
    // weighing cy[yz] times the sum of the horizontal weights inside the box (xz + xx < width, :582).
    unsigned cu[4] = {}, cv[4] = {};
#pragma unroll
    for (int s = 0; s < (4 >> WS); s++)
    {
        const int k = s << WS;
        const unsigned wx = WS && c0 + k + 1 < bw ? a.cx[0] + a.cx[1] : a.cx[0];
        unsigned accu_a = 0, accu_b = 0, accu_c = 0;
#pragma unroll
        for (int yz = 0; yz < R; yz++)
        {
            const unsigned coeff = wx * a.cy[yz] * A[yz][k];
            accu_a += coeff * U[yz][k];
            accu_b += coeff * V[yz][k];
            accu_c += coeff;
        }
        if (accu_c)
        {
            cu[s] = (accu_a + (accu_c >> 1)) / accu_c;
            cv[s] = (accu_b + (accu_c >> 1)) / accu_c;
        }
    }
    const size_t crow = (size_t)(ty0 >> HS);
    if (WS)
    {
        *reinterpret_cast<unsigned short *>(bx.plane[1] + crow * bx.stride[1] + (c0 >> 1)) = (unsigned short)(cu[0] | cu[1] << 8);
        *reinterpret_cast<unsigned short *>(bx.plane[2] + crow * bx.stride[2] + (c0 >> 1)) = (unsigned short)(cv[0] | cv[1] << 8);
    }
    else
    {
        *reinterpret_cast<unsigned *>(bx.plane[1] + crow * bx.stride[1] + c0) = pack4(cu);
        *reinterpret_cast<unsigned *>(bx.plane[2] + crow * bx.stride[2] + c0) = pack4(cv);
    }
}

} // namespace

int hbhip_ass_compose_launch(hbhip_ctx *ctx, int wshift, int hshift, dim3 grid, const AssArgs &a)
{
    const dim3 blk(ASS_TILE_W / 4, ASS_TILE_WAVES);
    if (wshift == 1 && hshift == 1)      HBHIP_LAUNCH(ctx, "ass_compose", (ass_compose_kernel<1, 1>), grid, blk, 0, a);
    else if (wshift == 1 && hshift == 0) HBHIP_LAUNCH(ctx, "ass_compose", (ass_compose_kernel<1, 0>), grid, blk, 0, a);
    else if (wshift == 0 && hshift == 0) HBHIP_LAUNCH(ctx, "ass_compose", (ass_compose_kernel<0, 0>), grid, blk, 0, a);
    else return HBHIP_ERR_UNSUPPORTED;
    HBHIP_CHECK(ctx, hipGetLastError());
    return HBHIP_OK;
}
