// format.hip — `format=pix_fmts=...` (libhb/format.c:13-111) as real GPU filters: what libavfilter's auto-inserted
// same-size `scale` computes for the pair of pixel formats, in four forms:
//
//   format_kernel            the depth alone: libswscale's unscaled planar copy
//   format_resample_kernel   fewer chroma samples at equal depth, its SCALED form, a lower depth with or without them,
//                            and its DEEPEN form, fewer chroma samples at a higher depth
//   format_upsample_kernel   more chroma samples at equal or higher depth
//
// The last three are libswscale's general scaler at its default flags, bicubic.  PARITY UNPINNED: libswscale is not in
// the reference tree; the kernels are bit-exact against OUR restatements (oracle/alias_oracle.c:orc_format_plane,
// tests/format_resample_model.py, format_scaled_model.py, format_upsample_model.py, format_deepen_model.py).
#include "hbhip_internal.h"

#include <type_traits>
#include <vector>

#include "dot2.h"
#include "sws_filter.h"

namespace {

// ------------------------------------------------------------------ format (depth conversion)
// swscale_unscaled.c:planarCopyWrapper.  Up: shift (limited range, chroma) or top-bit replication (full-range luma); down:
// ordered dither then the overflow clamp tmp - (tmp >> depth).  One launch for the three planes, four samples per
// thread, HBM-bound (read in + write out).
constexpr int FMT_FRAMES = 16;
struct FormatArgs
{
    const uint8_t *src[FMT_FRAMES][3];
    uint8_t       *dst[FMT_FRAMES][3];
    int spitch[3], dpitch[3], w[3], h[3];
    int sdepth, ddepth, full_range;
};

// four samples per thread, moved as one dword (bytes) or two (16-bit samples) where the row has them; grid.z =
// 3 * frame + plane: the frames of a batch in one launch
template <typename SRC, typename DST>
__global__ __launch_bounds__(256) void format_kernel(FormatArgs a)
{
    const int c = blockIdx.z % 3, f = blockIdx.z / 3;
    const int x0 = (blockIdx.x * blockDim.x + threadIdx.x) * 4, y = blockIdx.y * blockDim.y + threadIdx.y;
    if (x0 >= a.w[c] || y >= a.h[c]) return;
    const SRC *s = reinterpret_cast<const SRC *>(a.src[f][c] + (size_t)y * a.spitch[c]);
    DST *d = reinterpret_cast<DST *>(a.dst[f][c] + (size_t)y * a.dpitch[c]);
    const bool shiftonly = c != 0 || !a.full_range;
    const int up = a.ddepth - a.sdepth;
    const bool whole = x0 + 3 < a.w[c];
    unsigned v4[4] = { 0, 0, 0, 0 };
    if (whole)
    {
        if (sizeof(SRC) == 1)
        {
            const uint32_t w = *reinterpret_cast<const uint32_t *>(s + x0);
#pragma unroll
            for (int i = 0; i < 4; i++) v4[i] = (w >> (8 * i)) & 0xffu;
        }
        else
        {
            const uint2 w = *reinterpret_cast<const uint2 *>(s + x0);
            v4[0] = w.x & 0xffffu; v4[1] = w.x >> 16; v4[2] = w.y & 0xffffu; v4[3] = w.y >> 16;
        }
    }
    else
        for (int i = 0; x0 + i < a.w[c]; i++) v4[i] = s[x0 + i];
    unsigned o4[4];
#pragma unroll
    for (int i = 0; i < 4; i++)
    {
        const int x = x0 + i;
        const unsigned v = v4[i];
        unsigned o;
        if (up == 0) o = v;
        else if (up > 0) o = shiftonly ? v << up : (v << up) | (v >> (2 * a.sdepth - a.ddepth));
        else
        {
            const int shift = -up;
            // dithers[shift - 1][y & 7][x & 7] of swscale_unscaled.c for shift 2 / 4 (2x2 / 4x4 ordered matrices)
            // one nibble per cell: {1,2;3,0} and {4,8,7,11; 12,0,15,3; 6,10,5,9; 14,2,13,1}
            constexpr uint64_t D4 = 0xB784ull | (0x3F0Cull << 16) | (0x95A6ull << 32) | (0x1D2Eull << 48);
            const unsigned dm = shift == 2 ? ((0x0321u >> (4 * ((y & 1) * 2 + (x & 1)))) & 15u)
                                           : (unsigned)((D4 >> (16 * (y & 3) + 4 * (x & 3))) & 15u);
            if (shiftonly)
            {
                const unsigned tmp = (v + dm) >> shift;
                o = tmp - (tmp >> a.ddepth);
            }
            else
                o = (v - (v >> a.ddepth) + dm) >> shift;                // full-range luma: DITHER_COPY's other arm
        }
        o4[i] = o;
    }
    if (whole)
    {
        if (sizeof(DST) == 1) *reinterpret_cast<uint32_t *>(d + x0) = o4[0] | (o4[1] << 8) | (o4[2] << 16) | (o4[3] << 24);
        else                  *reinterpret_cast<uint2 *>(d + x0) = make_uint2(o4[0] | (o4[1] << 16), o4[2] | (o4[3] << 16));
    }
    else
        for (int i = 0; x0 + i < a.w[c]; i++) d[x0 + i] = (DST)o4[i];
}

class FormatFilter : public BurstFilter
{
public:
    FormatFilter(hbhip_ctx *c, int full) : BurstFilter(c), full_range(full) {}
    int process_many(DevPicture *const *ins, DevPicture *const *outs, int n) override
    {
        return hbhip_for_each_burst<FMT_FRAMES, FormatArgs>(ctx, ins, outs, n, [&](FormatArgs &a, int nf, int, uintptr_t bits) {
            if ((bits & 7) != 0) return HBHIP_ERR_ARG;                       // planes and pitches of this library are 64-byte aligned
            for (int c = 0; c < 3; c++) { a.w[c] = in_geo.pw[c]; a.h[c] = in_geo.ph[c]; }
            a.sdepth = in_geo.depth; a.ddepth = out_geo.depth; a.full_range = full_range;
            const dim3 grid(hbhip_grid_x((a.w[0] + 255) / 256), (a.h[0] + 3) / 4, 3 * nf);
            if (in_geo.bps == 1 && out_geo.bps == 1)      HBHIP_LAUNCH(ctx, "format", (format_kernel<uint8_t, uint8_t>), grid, dim3(64, 4), 0, a);
            else if (in_geo.bps == 1)                     HBHIP_LAUNCH(ctx, "format", (format_kernel<uint8_t, uint16_t>), grid, dim3(64, 4), 0, a);
            else if (out_geo.bps == 1)                    HBHIP_LAUNCH(ctx, "format", (format_kernel<uint16_t, uint8_t>), grid, dim3(64, 4), 0, a);
            else                                          HBHIP_LAUNCH(ctx, "format", (format_kernel<uint16_t, uint16_t>), grid, dim3(64, 4), 0, a);
            return HBHIP_OK;
        });
    }
    int full_range;
};

// ------------------------------------------------------------------ format (the scaler: chroma down, scaled, up)
// When the target's chroma layout differs from the stream's, libavfilter's `scale` is libswscale's general scaler.  Luma
// runs through its identity filters; Cb and Cr are filtered with the tables of sws_filter(bicubic) - 14-bit horizontal,
// 12-bit vertical coefficients - and the intermediates of scale_sws_h_kernel / scale_sws_v_kernel (alias.hip):
// hScale8To15 / hScale16To15 by the SOURCE depth, yuv2planeX_8 / _10 / _12 by the TARGET's.  Chroma is left-sited whatever
// the stream's chroma_location says, the rule of the crop/scale drop-in's swscale branch; rows are centred (srcPos =
// dstPos = 128).
//
// What the down and the up kernel have in common.  They read the tables in a NOMINAL form (sws_filter.h: sws_nominal):
// every output row / column taps a fixed number of source samples from a position that is a compile-time function of
// its index and EVEN, sws_filter's rows moved into that window with zeros around them; create() checks that every row
// fits and declines a table that does not.  So both passes take their taps two at a time (v_dot2_i32_i16).  A thread owns
// four adjacent output columns (a dword of bytes, a qword of 16-bit samples) and a run of output rows; the source rows
// under them are loaded ONCE, taken through the horizontal pass (or the identity's shift) and kept in registers as
// 15-bit intermediates, a PAIR OF ROWS to a dword; the vertical pass reads registers only.  No LDS.  The vertical
// coefficients of a row are the same for a whole wave (a wave is one threadIdx.y) and come through scalar loads.
// grid.z = frame: the frames of a burst in one launch; grid.y = the workgroup rows of luma (a thread moves four samples
// of FS_LROWS rows), then those of Cb, then those of Cr; grid.x is sized for luma and the workgroups beyond a chroma
// plane return at once.  HP / VP: the chroma planes take a horizontal / a vertical pass.
//
// What differs by direction on the host: the window, the output rows a chroma thread makes by [HP][VP], the horizontal
// source / target positions, and the taps initFilter's clamp (size = min(size, src - 2)) must leave whole - a chroma
// plane smaller than that gets something else than a bicubic, nobody's to restate.
constexpr int FS_LROWS = 4;
struct FsDirection
{
    bool up;
    SwsNominalFrame frame;
    int rows[2][2];
    int hsrc_pos, hdst_pos, min_taps;
};
constexpr FsDirection FS_DOWN = { false, SWS_NOMINAL_DOWN, { { FS_LROWS, 8 }, { 8, 16 } }, 128, 64, 9 };
constexpr FsDirection FS_UP   = { true,  SWS_NOMINAL_UP,   { { 0, 8 }, { 4, 8 } },         64, 128, 5 };

struct FormatScalerArgs
{
    const uint8_t *src[FMT_FRAMES][3];
    uint8_t       *dst[FMT_FRAMES][3];
    int spitch[3], dpitch[3];
    int w, h, scw, sch, dcw, dch, sdepth, ddepth;     // luma size; chroma size of the source and of the target; depths
    int ly, cy;                               // grid.y: ly workgroup rows of luma, then cy of Cb, then cy of Cr
    const short *hq, *vq;                     // [column][taps] (columns padded to 4), [row][taps]
};

// The scaled form's extra argument: libswscale's ff_dither_8x8_128, row r in dwords 2r (columns 0 .. 3, a byte each) and
// 2r + 1 (columns 4 .. 7).
struct FormatScaledArgs : FormatScalerArgs
{
    uint32_t dither[16];
};

// the dither bytes of output row y, columns x0 .. x0 + 3 (x0 a multiple of 4): Y and Cb read the table at column x, Cr at
// x + 3 (yuv2planeX_8_c's offset argument, yuv2nv12cX_c's two halves) - bytes 3 .. 6, or 7, 0, 1, 2, of the row's eight
__device__ __forceinline__ uint32_t fr_dither4(const FormatScaledArgs &a, int y, int x0, bool cr)
{
    const uint32_t lo = a.dither[2 * (y & 7)], hi = a.dither[2 * (y & 7) + 1];
    const uint32_t p = (x0 & 4) ? hi : lo, q = (x0 & 4) ? lo : hi;
    return cr ? __builtin_amdgcn_alignbyte(q, p, 3u) : p;
}

// samples x0 .. x0 + 3 of a row (x0 a multiple of 4, possibly negative) as two dwords of 16-bit pairs; those outside
// [0, w) read as 0 and are never loaded
template <typename PIX>
__device__ __forceinline__ void fr_load_pairs(const PIX *row, int x0, int w, uint32_t *p)
{
    if (x0 >= 0 && x0 + 3 < w)
    {
        if (sizeof(PIX) == 1)
        {
            const uint32_t d = *reinterpret_cast<const uint32_t *>(row + x0);
            p[0] = __builtin_amdgcn_perm(0u, d, 0x0c010c00u);
            p[1] = __builtin_amdgcn_perm(0u, d, 0x0c030c02u);
        }
        else
        {
            const uint2 d = *reinterpret_cast<const uint2 *>(row + x0);
            p[0] = d.x; p[1] = d.y;
        }
    }
    else
    {
        uint32_t v[4];
#pragma unroll
        for (int i = 0; i < 4; i++) v[i] = (x0 + i >= 0 && x0 + i < w) ? (uint32_t)row[x0 + i] : 0u;
        p[0] = v[0] | (v[1] << 16); p[1] = v[2] | (v[3] << 16);
    }
}

// four samples as they were loaded - a dword of bytes, a qword of 16-bit samples - as two dwords of 16-bit pairs
__device__ __forceinline__ void fr_widen(uint32_t d, uint32_t *p)
{
    p[0] = __builtin_amdgcn_perm(0u, d, 0x0c010c00u);
    p[1] = __builtin_amdgcn_perm(0u, d, 0x0c030c02u);
}
__device__ __forceinline__ void fr_widen(uint2 d, uint32_t *p) { p[0] = d.x; p[1] = d.y; }

template <typename PIX>
__device__ __forceinline__ void fr_store4(PIX *row, int x0, int w, const int *o)
{
    if (x0 + 3 < w)
    {
        if (sizeof(PIX) == 1) *reinterpret_cast<uint32_t *>(row + x0) = (uint32_t)o[0] | ((uint32_t)o[1] << 8) | ((uint32_t)o[2] << 16) | ((uint32_t)o[3] << 24);
        else                  *reinterpret_cast<uint2 *>(row + x0) = make_uint2((uint32_t)o[0] | ((uint32_t)o[1] << 16), (uint32_t)o[2] | ((uint32_t)o[3] << 16));
    }
    else
        for (int i = 0; x0 + i < w; i++) row[x0 + i] = (PIX)o[i];
}

// The plane c of this workgroup row and the first of the `rows` rows of this thread row in it, one value a wave.
// luma: the caller's (int)blockIdx.y < a.ly, a constant where it has left the luma rows behind.
template <class Args>
__device__ __forceinline__ int fs_row0(const Args &a, bool luma, int rows, int &c)
{
    const int cby = (int)blockIdx.y - a.ly;
    c = luma ? 0 : 1 + cby / a.cy;
    return __builtin_amdgcn_readfirstlane((luma ? (int)blockIdx.y : cby % a.cy) * blockDim.y + threadIdx.y) * rows;
}

// The four columns' horizontal coefficients of a thread, in pairs: TAPS / 2 uint4 (16-byte aligned: x0 is a multiple of 4).
template <int TAPS>
__device__ __forceinline__ void fs_load_coef(const short *hq, int x0, uint32_t *hc)
{
    const uint4 *q = reinterpret_cast<const uint4 *>(hq + (size_t)x0 * TAPS);
#pragma unroll
    for (int k = 0; k < TAPS / 2; k++)
    {
        const uint4 t = q[k];
        hc[4 * k] = t.x; hc[4 * k + 1] = t.y; hc[4 * k + 2] = t.z; hc[4 * k + 3] = t.w;
    }
}

// The output stage.  yuv2planeX_8_c: the flat dither of 64 (round = 64 << 12, shift 19); yuv2planeX_10 / _12: half of the
// shift 27 - depth.  (The scaled form to 8 bits replaces the round term by the ordered dither, seed() below.)
struct FsStage { int shift, round, vmax; };
template <typename DPIX>
__device__ __forceinline__ FsStage fs_stage(int ddepth)
{
    const int shift = sizeof(DPIX) == 1 ? 19 : 27 - ddepth;
    return { shift, sizeof(DPIX) == 1 ? 64 << 12 : 1 << (shift - 1), (1 << ddepth) - 1 };
}

// the accumulators of output row j's four columns through it, to chroma plane c
template <typename DPIX, class Args>
__device__ __forceinline__ void fs_put(const Args &a, const FsStage &st, int f, int c, int x0, int j, const int *acc)
{
    int o[4];
#pragma unroll
    for (int i = 0; i < 4; i++) o[i] = min(max(acc[i] >> st.shift, 0), st.vmax);
    fr_store4(reinterpret_cast<DPIX *>(a.dst[f][c] + (size_t)j * a.dpitch[c]), x0, a.dcw, o);
}

// The scaler on identity filters: rows y0 .. y0 + FS_LROWS - 1 of plane c (w x h), columns x0 .. x0 + 3 < w + 3, each
// sample through op(row, column - x0, sample).  The loads go ahead of the arithmetic; a dword or a qword in and out.
template <typename PIX, typename DPIX, class Args, class Op>
__device__ __forceinline__ void fs_identity_rows(const Args &a, int f, int c, int x0, int y0, int w, int h, Op op)
{
    uint32_t p[FS_LROWS][2];
#pragma unroll
    for (int r = 0; r < FS_LROWS; r++)
        if (y0 + r < h) fr_load_pairs(reinterpret_cast<const PIX *>(a.src[f][c] + (size_t)(y0 + r) * a.spitch[c]), x0, w, p[r]);
#pragma unroll
    for (int r = 0; r < FS_LROWS; r++)
    {
        if (y0 + r >= h) break;
        int o[4];
#pragma unroll
        for (int i = 0; i < 4; i++) o[i] = op(y0 + r, i, (int)((p[r][i >> 1] >> (16 * (i & 1))) & 0xffffu));
        fr_store4(reinterpret_cast<DPIX *>(a.dst[f][c] + (size_t)(y0 + r) * a.dpitch[c]), x0, w, o);
    }
}

// ---- down: 4:2:2 -> 4:2:0, 4:4:4 -> 4:2:2 / 4:2:0.  Vertically target row j lies midway between source rows 2j and
// 2j + 1; horizontally target column i is co-sited with source column 2i (srcPos 128, dstPos 64).  Output j taps the
// FR_TAPS samples from 2j + FR_BASE on (a 2:1 bicubic filter is 7 - 9 taps at 2j - 3 or, for an odd source size, one
// sample further left).
//   4:2:2 -> 4:2:0   all ROWS + FR_TAPS / 2 - 1 row pairs are loaded ahead of the arithmetic;
//   4:4:4 -> 4:2:0   the window of FR_TAPS / 2 row pairs rolls down one pair an output row (the horizontal pass needs
//                    the registers the whole window would take);
//   4:4:4 -> 4:2:2   two rows a turn, the vertical identity applied to each half.
// At equal depth luma is a copy, the accesses of format_kernel.
//
// SC: the scaled form, a LOWER target depth - 10 -> 8, 12 -> 8, 12 -> 10 bits (DPIX: the target's sample type; Args:
// FormatScaledArgs).  The chroma passes are the same; what changes is the intermediate's shift (the source depth), the output
// stage (the target depth: to 8 bits its round term is the 8 x 8 ordered dither, a byte a column) and the store type.
// Luma is no copy then but the identity filter and the output stage, and so are Cb and Cr where neither pass is taken
// (4:2:0 -> 4:2:0, the planar step in front of the NV12 / P010LE repack).
// The equal-depth instantiations take the defaults and compile to the instructions they had before the form existed.
//
// DEEP (with SC): the deepen form, fewer chroma samples at a HIGHER target depth - 8 -> 10, 8 -> 12 (PIX a byte), 10 -> 12
// bits, DPIX 16 bits, always with a pass (Args: FormatScalerArgs, nothing is dithered).  What an encoder whose list holds
// only 10-bit formats gets behind an 8-bit 4:2:2 / 4:4:4 title (work.c:1525-1552, the second match_pix_fmt call).  The
// chroma passes again, hScale8To15 / hScale16To15 by the source and the flat round term of the target's yuv2planeX_10 /
// _12; luma through the identity and yuv2plane1_10 / _12, whose shift follows the target there: v << (ddepth - sdepth).
// Its horizontal pass loads a thread's sixteen samples ahead of one wait where all of them lie inside the plane (hpair).
constexpr int FR_TAPS = FS_DOWN.frame.taps, FR_BASE = FS_DOWN.frame.base;
template <typename PIX, bool HP, bool VP, typename DPIX = PIX, bool SC = false, class Args = FormatScalerArgs, bool DEEP = false>
__global__ __launch_bounds__(256, 4) void format_resample_kernel(Args a)
{
    static_assert(SC || ((HP || VP) && std::is_same<PIX, DPIX>::value), "equal depth: one pass at least, one sample type");
    static_assert(!DEEP || (SC && (HP || VP) && sizeof(DPIX) == 2), "deepen: one pass at least, a 16-bit target");
    const int f = blockIdx.z;
    const int x0 = (blockIdx.x * blockDim.x + threadIdx.x) * 4;
    const int ddepth = SC ? a.ddepth : a.sdepth;
    if constexpr (SC)
    {
        // the planes that take no pass: hScale16To15's one tap, v << (15 - depth) (hScale8To15's v << 7 is the same at 8
        // bits), then yuv2plane1_8 - (t + dither) >> 7 - or yuv2plane1_10, (t + 16) >> 5, clipped at the top (nothing is
        // negative here).  The scaled form's one 16-bit target has 10 bits, a constant; the deepen form's shift is the target's.
        const bool luma = (int)blockIdx.y < a.ly;
        if (luma || (!HP && !VP))
        {
            int c;
            const int y0 = fs_row0(a, luma, FS_LROWS, c);
            const int w = luma ? a.w : a.dcw, h = luma ? a.h : a.dch;
            if (x0 >= w || y0 >= h) return;
            const int up = 15 - a.sdepth, vmax = (1 << ddepth) - 1;
            const int down = 15 - (DEEP ? ddepth : 10);
            fs_identity_rows<PIX, DPIX>(a, f, c, x0, y0, w, h, [&](int y, int i, int v) __attribute__((always_inline)) {
                const int t = v << up;
                if constexpr (sizeof(DPIX) == 1) return min((t + (int)((fr_dither4(a, y, x0, c == 2) >> (8 * i)) & 0xffu)) >> 7, vmax);
                else                             return min((t + (1 << (down - 1))) >> down, vmax);
            });
            return;
        }
    }
    else if ((int)blockIdx.y < a.ly)
    {
        const int y0 = (blockIdx.y * blockDim.y + threadIdx.y) * FS_LROWS;
        if (x0 >= a.w) return;
        const uint8_t *s = a.src[f][0];
        uint8_t *d = a.dst[f][0];
        if (x0 + 3 < a.w)
        {
            typedef typename std::conditional<sizeof(PIX) == 1, uint32_t, uint2>::type V;
            V v[FS_LROWS];
#pragma unroll
            for (int r = 0; r < FS_LROWS; r++)
                if (y0 + r < a.h) v[r] = *reinterpret_cast<const V *>(s + (size_t)(y0 + r) * a.spitch[0] + (size_t)x0 * sizeof(PIX));
#pragma unroll
            for (int r = 0; r < FS_LROWS; r++)
                if (y0 + r < a.h) *reinterpret_cast<V *>(d + (size_t)(y0 + r) * a.dpitch[0] + (size_t)x0 * sizeof(PIX)) = v[r];
        }
        else
            for (int r = 0; r < FS_LROWS && y0 + r < a.h; r++)
                for (int i = 0; x0 + i < a.w; i++)
                    reinterpret_cast<PIX *>(d + (size_t)(y0 + r) * a.dpitch[0])[x0 + i] = reinterpret_cast<const PIX *>(s + (size_t)(y0 + r) * a.spitch[0])[x0 + i];
        return;
    }
    constexpr int ROWS = FS_DOWN.rows[HP][VP];                               // output rows a thread
    int c;
    const int j0 = fs_row0(a, false, ROWS, c);
    if (x0 >= a.dcw || j0 >= a.dch) return;
    const int sh = sizeof(PIX) == 1 ? 7 : a.sdepth - 1;                      // hScale8To15_c / hScale16To15_c
    const FsStage st = fs_stage<DPIX>(ddepth);
    const int round = st.round;
    const uint8_t *sp = a.src[f][c];
    const int spitch = a.spitch[c];
    uint32_t hc[HP ? 2 * FR_TAPS : 1];
    if (HP) fs_load_coef<FR_TAPS>(a.hq, x0, hc);                             // 80 bytes a thread
    // source rows sr, sr + 1 (clamped into the plane: the rows outside of it have coefficient 0) -> the four columns'
    // intermediates, row sr in the low and row sr + 1 in the high half of e[column]
    auto hpair = [&](int sr, uint32_t *e) {
        const PIX *ra = reinterpret_cast<const PIX *>(sp + (size_t)min(max(sr, 0), a.sch - 1) * spitch);
        const PIX *rb = reinterpret_cast<const PIX *>(sp + (size_t)min(max(sr + 1, 0), a.sch - 1) * spitch);
        if (HP)
        {
            uint32_t pa[8], pb[8];                                           // the sixteen samples under the four columns, in pairs
            const int s0 = 2 * x0 + FR_BASE;
            if (DEEP && s0 >= 0 && s0 + 15 < a.scw)
            {
                // the deepen form, all sixteen samples inside the plane: fr_load_pairs' first arm without its test, so that
                // the eight loads of a turn go out ahead of ONE wait (each arm of the general form below keeps its load
                // and a wait to itself, and a turn is a chain of eight round trips to memory)
                typedef typename std::conditional<sizeof(PIX) == 1, uint32_t, uint2>::type V;
                V da[4], db[4];
#pragma unroll
                for (int g = 0; g < 4; g++)
                {
                    da[g] = *reinterpret_cast<const V *>(ra + s0 + 4 * g);
                    db[g] = *reinterpret_cast<const V *>(rb + s0 + 4 * g);
                }
#pragma unroll
                for (int g = 0; g < 4; g++)
                {
                    fr_widen(da[g], pa + 2 * g);
                    fr_widen(db[g], pb + 2 * g);
                }
            }
            else
            {
                // (the position spelt as it always was, not s0 + 4 * g: the other association changes the instructions
                // of every instantiation with a horizontal pass)
#pragma unroll
                for (int g = 0; g < 4; g++)
                {
                    fr_load_pairs(ra, 2 * x0 + FR_BASE + 4 * g, a.scw, pa + 2 * g);
                    fr_load_pairs(rb, 2 * x0 + FR_BASE + 4 * g, a.scw, pb + 2 * g);
                }
            }
#pragma unroll
            for (int i = 0; i < 4; i++)
            {
                int va = 0, vb = 0;
#pragma unroll
                for (int u = 0; u < FR_TAPS / 2; u++)
                {
                    va = dot2(pa[i + u], hc[i * (FR_TAPS / 2) + u], va);
                    vb = dot2(pb[i + u], hc[i * (FR_TAPS / 2) + u], vb);
                }
                va = min(va >> sh, (1 << 15) - 1);
                vb = min(vb >> sh, (1 << 15) - 1);
                e[i] = ((uint32_t)va & 0xffffu) | ((uint32_t)vb << 16);
            }
        }
        else
        {
            // the identity filter, one tap of 1 << 14: (s << 14) >> sh, below 1 << 15 for every sample - both halves in one shift
            uint32_t pa[2], pb[2];
            fr_load_pairs(ra, x0, a.scw, pa);
            fr_load_pairs(rb, x0, a.scw, pb);
#pragma unroll
            for (int g = 0; g < 2; g++)
            {
                e[2 * g]     = __builtin_amdgcn_perm(pb[g], pa[g], 0x05040100u) << (14 - sh);
                e[2 * g + 1] = __builtin_amdgcn_perm(pb[g], pa[g], 0x07060302u) << (14 - sh);
            }
        }
    };
    auto put = [&](int j, const int *acc) { fs_put<DPIX>(a, st, f, c, x0, j, acc); };
    // the round term of output row j's four columns
    auto seed = [&](int j, int *acc) {
        if constexpr (SC && sizeof(DPIX) == 1)
        {
            const uint32_t dm = fr_dither4(a, j, x0, c == 2);
#pragma unroll
            for (int i = 0; i < 4; i++) acc[i] = (int)((dm >> (8 * i)) & 0xffu) << 12;
        }
        else
        {
#pragma unroll
            for (int i = 0; i < 4; i++) acc[i] = round;
        }
    };
    // output row j from the FR_TAPS / 2 row pairs at win
    auto vrow = [&](int j, const uint32_t (*win)[4]) {
        const uint32_t *vq = reinterpret_cast<const uint32_t *>(a.vq + (size_t)j * FR_TAPS);
        int acc[4] = { round, round, round, round };
        if constexpr (SC) seed(j, acc);
#pragma unroll
        for (int u = 0; u < FR_TAPS / 2; u++)
        {
            const uint32_t q = vq[u];
#pragma unroll
            for (int i = 0; i < 4; i++) acc[i] = dot2(win[u][i], q, acc[i]);
        }
        put(j, acc);
    };
    if (!HP)
    {
        constexpr int NP = ROWS + FR_TAPS / 2 - 1;
        uint32_t hp[NP][4];
#pragma unroll
        for (int k = 0; k < NP; k++) hpair(2 * (j0 + k) + FR_BASE, hp[k]);
#pragma unroll
        for (int r = 0; r < ROWS; r++)
            if (j0 + r < a.dch) vrow(j0 + r, hp + r);
    }
    else if (!VP)
    {
#pragma unroll
        for (int r = 0; r < ROWS; r += 2)
        {
            if (j0 + r >= a.dch) break;
            uint32_t e[4];
            hpair(j0 + r, e);
            int lo[4], hi[4];                                                // the identity filter: one tap of 1 << 12
#pragma unroll
            for (int i = 0; i < 4; i++) { lo[i] = round + ((int)(short)(e[i] & 0xffffu) << 12); hi[i] = round + (((int)e[i] >> 16) << 12); }
            if constexpr (SC)
            {
                int da[4], db[4];
                seed(j0 + r, da);
                seed(j0 + r + 1, db);
#pragma unroll
                for (int i = 0; i < 4; i++) { lo[i] += da[i] - round; hi[i] += db[i] - round; }
            }
            put(j0 + r, lo);
            if (j0 + r + 1 < a.dch) put(j0 + r + 1, hi);
        }
    }
    else
    {
        uint32_t win[FR_TAPS / 2][4] = {};
#pragma unroll 2
        for (int r = 1 - FR_TAPS / 2; r < ROWS && j0 + r < a.dch; r++)        // (the first FR_TAPS / 2 - 1 turns only fill the window)
        {
#pragma unroll
            for (int u = 0; u < FR_TAPS / 2 - 1; u++)
#pragma unroll
                for (int i = 0; i < 4; i++) win[u][i] = win[u + 1][i];
            hpair(2 * (j0 + r) + FR_BASE + FR_TAPS - 2, win[FR_TAPS / 2 - 1]);
            if (r >= 0) vrow(j0 + r, win);
        }
    }
}

// ---- up: 4:2:0 -> 4:2:2, 4:2:2 -> 4:4:4, 4:2:0 -> 4:4:4; 8 -> 8, 10 -> 10, 12 -> 12, 8 -> 10, 8 -> 12, 10 -> 12 bits: what
// an encoder that only takes 4:2:2 or 4:4:4 input gets behind a 4:2:0 title (work.c:1525-1552, the third match_pix_fmt
// call).  The tables of the 1:2 ratio - sws_filter(bicubic)'s x_inc <= 1 << 16 arm, four taps - and the flat round term:
// the depth does not fall, nothing is dithered.  Luma: v << (ddepth - sdepth), a copy at equal depth (no top-bit
// replication in either range, unlike format_kernel's full-range luma).
// Siting: target row j a quarter above (j even) / below (j odd) source row j / 2; target column i on source column i / 2
// for an even i, midway to the next for an odd one (srcPos 64, dstPos 128).  The four taps of output i lie in
// (i >> 1) - 1 .. (i >> 1) + 2 horizontally and (i >> 1) - 2 .. (i >> 1) + 2 vertically (an odd target size, 2 s - 1 for
// s, moves the positions by up to half a sample along the plane), both inside the UP_TAPS samples from
// 2 * (i >> 2) + UP_BASE on for all four outputs of a group.  So the window is the same for a thread's four columns - three
// sample pairs a source row, every output three v_dot2_i32_i16 - and for four adjacent output rows: a thread's eight
// rows read 8 / 2 + 4 source rows.  Without a vertical pass a thread makes four rows, each from its own source row.
constexpr int UP_TAPS = FS_UP.frame.taps, UP_BASE = FS_UP.frame.base;

// samples s0 .. s0 + 5 of a row (s0 even, possibly negative) as three dwords of 16-bit pairs; those outside [0, w) read as
// 0 and are never loaded (their coefficients are 0)
template <typename PIX>
__device__ __forceinline__ void up_load6(const PIX *row, int s0, int w, uint32_t *p)
{
    if (s0 >= 0 && s0 + 5 < w)
    {
#pragma unroll
        for (int g = 0; g < 3; g++)
        {
            if (sizeof(PIX) == 1) p[g] = __builtin_amdgcn_perm(0u, (uint32_t)*reinterpret_cast<const uint16_t *>(row + s0 + 2 * g), 0x0c010c00u);
            else                  p[g] = *reinterpret_cast<const uint32_t *>(row + s0 + 2 * g);
        }
    }
    else
    {
        uint32_t v[6];
#pragma unroll
        for (int i = 0; i < 6; i++) v[i] = (s0 + i >= 0 && s0 + i < w) ? (uint32_t)row[s0 + i] : 0u;
#pragma unroll
        for (int g = 0; g < 3; g++) p[g] = v[2 * g] | (v[2 * g + 1] << 16);
    }
}

template <typename PIX, typename DPIX, bool HP, bool VP>
__global__ __launch_bounds__(256, 4) void format_upsample_kernel(FormatScalerArgs a)
{
    static_assert((HP || VP) && sizeof(DPIX) >= sizeof(PIX), "one pass at least; the depth does not fall");
    const int f = blockIdx.z;
    const int x0 = (blockIdx.x * blockDim.x + threadIdx.x) * 4;
    if ((int)blockIdx.y < a.ly)
    {
        // the identity filters and the output stage: (v << (15 - sdepth) << 12 + round) >> shift = v << (ddepth - sdepth)
        const int y0 = (blockIdx.y * blockDim.y + threadIdx.y) * FS_LROWS;
        if (x0 >= a.w) return;
        const int up = a.ddepth - a.sdepth;
        fs_identity_rows<PIX, DPIX>(a, f, 0, x0, y0, a.w, a.h, [&](int, int, int v) __attribute__((always_inline)) { return v << up; });
        return;
    }
    constexpr int ROWS = FS_UP.rows[HP][VP];                                 // output rows a thread
    int c;
    const int j0 = fs_row0(a, false, ROWS, c);
    if (x0 >= a.dcw || j0 >= a.dch) return;
    const int sh = sizeof(PIX) == 1 ? 7 : a.sdepth - 1;                      // hScale8To15_c / hScale16To15_c
    const FsStage st = fs_stage<DPIX>(a.ddepth);
    const int round = st.round;
    const uint8_t *sp = a.src[f][c];
    const int spitch = a.spitch[c];
    uint32_t hc[HP ? 2 * UP_TAPS : 1];
    if (HP) fs_load_coef<UP_TAPS>(a.hq, x0, hc);                             // 48 bytes a thread
    // source row sr (clamped into the plane: the rows outside of it have coefficient 0) -> the four columns' intermediates
    auto hrow = [&](int sr, int *e) {
        const PIX *row = reinterpret_cast<const PIX *>(sp + (size_t)min(max(sr, 0), a.sch - 1) * spitch);
        if (HP)
        {
            uint32_t p[UP_TAPS / 2];                                         // the six samples under the four columns, in pairs
            up_load6(row, (x0 >> 1) + UP_BASE, a.scw, p);
#pragma unroll
            for (int i = 0; i < 4; i++)
            {
                int v = 0;
#pragma unroll
                for (int u = 0; u < UP_TAPS / 2; u++) v = dot2(p[u], hc[i * (UP_TAPS / 2) + u], v);
                e[i] = min(v >> sh, (1 << 15) - 1);
            }
        }
        else
        {
            // the identity filter, one tap of 1 << 14: (s << 14) >> sh
            uint32_t p[2];
            fr_load_pairs(row, x0, a.scw, p);
#pragma unroll
            for (int i = 0; i < 4; i++) e[i] = (int)((p[i >> 1] >> (16 * (i & 1))) & 0xffffu) << (14 - sh);
        }
    };
    auto put = [&](int j, const int *acc) { fs_put<DPIX>(a, st, f, c, x0, j, acc); };
    if (!VP)
    {
        int e[ROWS][4];
#pragma unroll
        for (int r = 0; r < ROWS; r++) hrow(j0 + r, e[r]);
#pragma unroll
        for (int r = 0; r < ROWS; r++)
        {
            if (j0 + r >= a.dch) break;
            int acc[4];                                                      // the identity filter: one tap of 1 << 12
#pragma unroll
            for (int i = 0; i < 4; i++) acc[i] = round + e[r][i] * (1 << 12);
            put(j0 + r, acc);
        }
    }
    else
    {
        // source rows (j0 >> 1) + UP_BASE + 2k and the one below it, row pair k: output rows j0 + 4g .. j0 + 4g + 3 read pairs g .. g + 2
        constexpr int NP = ROWS / 4 + UP_TAPS / 2 - 1;
        uint32_t hp[NP][4];
#pragma unroll
        for (int k = 0; k < NP; k++)
        {
            int ea[4], eb[4];
            hrow((j0 >> 1) + UP_BASE + 2 * k, ea);
            hrow((j0 >> 1) + UP_BASE + 1 + 2 * k, eb);
#pragma unroll
            for (int i = 0; i < 4; i++) hp[k][i] = ((uint32_t)ea[i] & 0xffffu) | ((uint32_t)eb[i] << 16);
        }
#pragma unroll
        for (int r = 0; r < ROWS; r++)
        {
            if (j0 + r >= a.dch) break;
            const uint32_t *vq = reinterpret_cast<const uint32_t *>(a.vq + (size_t)(j0 + r) * UP_TAPS);
            int acc[4] = { round, round, round, round };
#pragma unroll
            for (int u = 0; u < UP_TAPS / 2; u++)
            {
                const uint32_t q = vq[u];
#pragma unroll
                for (int i = 0; i < 4; i++) acc[i] = dot2(hp[(r >> 2) + u][i], q, acc[i]);
            }
            put(j0 + r, acc);
        }
    }
}

// two bools into template arguments: go(std::bool_constant<hp>(), std::bool_constant<vp>())
template <class Go>
void fs_pick(bool hp, bool vp, Go &&go)
{
    if (hp && vp) go(std::true_type(), std::true_type());
    else if (hp)  go(std::true_type(), std::false_type());
    else if (vp)  go(std::false_type(), std::true_type());
    else          go(std::false_type(), std::false_type());
}

// The host side of the three scaler forms; which one is `dir` and, down, whether the depth falls.
class FormatScalerFilter : public BurstFilter
{
public:
    FormatScalerFilter(hbhip_ctx *c, const FsDirection &d) : BurstFilter(c), dir(d) {}
    // sws_filter's rows in the kernel's nominal frame, to the device; HBHIP_ERR_UNSUPPORTED: a row has a tap outside of it
    int upload(int src, int dst, int one, int src_pos, int dst_pos, int pad, DevBuf<short> &buf)
    {
        std::vector<short> q;
        if (!sws_nominal(src, dst, one, src_pos, dst_pos, pad, dir.frame, q)) return HBHIP_ERR_UNSUPPORTED;
        if (const int rc = buf.alloc(ctx, q.size())) return rc;
        HBHIP_CHECK(ctx, hipMemcpy(buf.get(), q.data(), sizeof(short) * q.size(), hipMemcpyHostToDevice));
        return HBHIP_OK;
    }
    int setup()
    {
        const int s = dir.up ? -1 : 1;
        hpass = s * (out_geo.log2_cw - in_geo.log2_cw) > 0;
        vpass = s * (out_geo.log2_ch - in_geo.log2_ch) > 0;
        // left-sited chroma: position 128 at full resolution (4:4:4 has no siting), 128 >> 1 at half; rows: centred, 128 both
        int rc = hpass ? upload(in_geo.pw[1], out_geo.pw[1], 1 << 14, dir.hsrc_pos, dir.hdst_pos, 4, d_hq) : HBHIP_OK;
        if (rc == HBHIP_OK && vpass) rc = upload(in_geo.ph[1], out_geo.ph[1], 1 << 12, 128, 128, 1, d_vq);
        return rc;
    }
    // the walk over the bursts and what every form's arguments have in common; go(a, grid, HP, VP) launches
    template <class Args, class Go>
    int run(DevPicture *const *ins, DevPicture *const *outs, int n, Go &&go)
    {
        return hbhip_for_each_burst<FMT_FRAMES, Args>(ctx, ins, outs, n, [&](Args &a, int nf, int, uintptr_t bits) {
            if ((bits & 7) != 0) return HBHIP_ERR_ARG;                       // planes and pitches of this library are 64-byte aligned
            a.w = in_geo.width; a.h = in_geo.height; a.sdepth = in_geo.depth; a.ddepth = out_geo.depth;
            a.scw = in_geo.pw[1]; a.sch = in_geo.ph[1]; a.dcw = out_geo.pw[1]; a.dch = out_geo.ph[1];
            a.hq = d_hq.get(); a.vq = d_vq.get();
            a.ly = (a.h + 4 * FS_LROWS - 1) / (4 * FS_LROWS);
            const int rows = 4 * dir.rows[hpass][vpass];                     // output rows a workgroup
            a.cy = (a.dch + rows - 1) / rows;
            const dim3 grid(hbhip_grid_x((a.w + 255) / 256), a.ly + 2 * a.cy, nf);
            fs_pick(hpass, vpass, [&](auto hp, auto vp) { go(a, grid, hp, vp); });
            return HBHIP_OK;
        });
    }
    template <typename PIX>
    int run_down(DevPicture *const *ins, DevPicture *const *outs, int n)
    {
        return run<FormatScalerArgs>(ins, outs, n, [&](FormatScalerArgs &a, dim3 grid, auto hp, auto vp) {
            if constexpr (hp.value || vp.value)
                HBHIP_LAUNCH(ctx, "format_resample", (format_resample_kernel<PIX, hp.value, vp.value>), grid, dim3(64, 4), 0, a);
        });
    }
    template <typename DPIX>
    int run_scaled(DevPicture *const *ins, DevPicture *const *outs, int n)
    {
        // libswscale's ff_dither_8x8_128
        static const uint8_t dither[8][8] = {
            {  36,  68,  60,  92,  34,  66,  58,  90 }, { 100,   4, 124,  28,  98,   2, 122,  26 },
            {  52,  84,  44,  76,  50,  82,  42,  74 }, { 116,  20, 108,  12, 114,  18, 106,  10 },
            {  32,  64,  56,  88,  38,  70,  62,  94 }, {  96,   0, 120,  24, 102,   6, 126,  30 },
            {  48,  80,  40,  72,  54,  86,  46,  78 }, { 112,  16, 104,   8, 118,  22, 110,  14 } };
        return run<FormatScaledArgs>(ins, outs, n, [&](FormatScaledArgs &a, dim3 grid, auto hp, auto vp) {
            for (int r = 0; r < 8; r++)
                for (int k = 0; k < 8; k++) a.dither[2 * r + k / 4] |= (uint32_t)dither[r][k] << (8 * (k & 3));
            HBHIP_LAUNCH(ctx, "format_scaled", (format_resample_kernel<uint16_t, hp.value, vp.value, DPIX, true, FormatScaledArgs>), grid, dim3(64, 4), 0, a);
        });
    }
    template <typename PIX>
    int run_deepen(DevPicture *const *ins, DevPicture *const *outs, int n)
    {
        return run<FormatScalerArgs>(ins, outs, n, [&](FormatScalerArgs &a, dim3 grid, auto hp, auto vp) {
            if constexpr (hp.value || vp.value)
                HBHIP_LAUNCH(ctx, "format_deepen", (format_resample_kernel<PIX, hp.value, vp.value, uint16_t, true, FormatScalerArgs, true>), grid, dim3(64, 4), 0, a);
        });
    }
    template <typename PIX, typename DPIX>
    int run_up(DevPicture *const *ins, DevPicture *const *outs, int n)
    {
        return run<FormatScalerArgs>(ins, outs, n, [&](FormatScalerArgs &a, dim3 grid, auto hp, auto vp) {
            if constexpr (hp.value || vp.value)
                HBHIP_LAUNCH(ctx, "format_upsample", (format_upsample_kernel<PIX, DPIX, hp.value, vp.value>), grid, dim3(64, 4), 0, a);
        });
    }
    int process_many(DevPicture *const *ins, DevPicture *const *outs, int n) override
    {
        const bool s8 = in_geo.bps == 1, d8 = out_geo.bps == 1;
        if (dir.up)
            return d8 ? run_up<uint8_t, uint8_t>(ins, outs, n) : s8 ? run_up<uint8_t, uint16_t>(ins, outs, n) : run_up<uint16_t, uint16_t>(ins, outs, n);
        if (out_geo.depth > in_geo.depth) return s8 ? run_deepen<uint8_t>(ins, outs, n) : run_deepen<uint16_t>(ins, outs, n);
        if (out_geo.depth != in_geo.depth)                                   // the scaled form, with or without a pass
            return d8 ? run_scaled<uint8_t>(ins, outs, n) : run_scaled<uint16_t>(ins, outs, n);
        return s8 ? run_down<uint8_t>(ins, outs, n) : run_down<uint16_t>(ins, outs, n);
    }
    const FsDirection &dir;
    bool hpass = false, vpass = false;
    DevBuf<short> d_hq, d_vq;
};

// Behind the four scaler create functions.  Down: no dimension gains chroma samples, the depth does not grow, and one
// of the three shrinks (src_depth == dst_depth is the chroma down-sampling, else the scaled form).  Up: all of it the
// other way round, and one DIMENSION gains - the depth alone is hbhip_format_create's.  deepen (down only): the depth
// GROWS and one dimension loses chroma samples.
int format_scaler_make(hbhip_ctx *ctx, const FsDirection &dir, int width, int height, int src_depth, int dst_depth,
                       int src_log2_cw, int src_log2_ch, int dst_log2_cw, int dst_log2_ch, hbhip_filter **out, bool deepen = false)
{
    if (!ctx || !out) return HBHIP_ERR_ARG;
    *out = nullptr;
    for (int d : {src_depth, dst_depth})
        if (d != 8 && d != 10 && d != 12) return HBHIP_ERR_UNSUPPORTED;
    if (width < 1 || height < 1) return HBHIP_ERR_ARG;
    if (!hbhip_yuv_layout_ok(src_log2_cw, src_log2_ch) || !hbhip_yuv_layout_ok(dst_log2_cw, dst_log2_ch)) return HBHIP_ERR_UNSUPPORTED;
    const int s = dir.up ? -1 : 1;
    const int pw = s * (dst_log2_cw - src_log2_cw), ph = s * (dst_log2_ch - src_log2_ch), pd = s * (src_depth - dst_depth);
    if (deepen ? pw < 0 || ph < 0 || pd >= 0 || (!pw && !ph)
               : pw < 0 || ph < 0 || pd < 0 || (!pw && !ph && (dir.up || !pd))) return HBHIP_ERR_UNSUPPORTED;
    PicGeometry gi, go;
    gi.set(width, height, src_depth, src_log2_cw, src_log2_ch);
    go.set(width, height, dst_depth, dst_log2_cw, dst_log2_ch);
    // a chroma plane so small that initFilter's clamp cuts the taps short
    if ((pw && gi.pw[1] - 2 < dir.min_taps) || (ph && gi.ph[1] - 2 < dir.min_taps)) return HBHIP_ERR_UNSUPPORTED;
    FormatScalerFilter *f = hbhip_make_filter<FormatScalerFilter>(ctx, gi, go, dir);
    if (!f) return HBHIP_ERR_NOMEM;
    const int rc = f->setup();
    if (rc != HBHIP_OK) { delete f; return rc; }
    *out = f;
    return HBHIP_OK;
}

} // namespace

extern "C" int hbhip_format_create(hbhip_ctx *ctx, int width, int height, int src_depth, int dst_depth,
                                   int log2_chroma_w, int log2_chroma_h, int full_range, hbhip_filter **out)
{
    if (!ctx || !out) return HBHIP_ERR_ARG;
    *out = nullptr;
    for (int d : {src_depth, dst_depth})
        if (d != 8 && d != 10 && d != 12) return HBHIP_ERR_UNSUPPORTED;
    if (width < 1 || height < 1) return HBHIP_ERR_ARG;
    PicGeometry gi, go;
    gi.set(width, height, src_depth, log2_chroma_w, log2_chroma_h);
    go.set(width, height, dst_depth, log2_chroma_w, log2_chroma_h);
    *out = hbhip_make_filter<FormatFilter>(ctx, gi, go, full_range);
    return *out ? HBHIP_OK : HBHIP_ERR_NOMEM;
}

// (chroma_location, here and below: every value is taken as left-sited, the crop/scale drop-in's rule)
extern "C" int hbhip_format_resample_create(hbhip_ctx *ctx, int width, int height, int depth, int src_log2_cw, int src_log2_ch,
                                            int dst_log2_cw, int dst_log2_ch, int chroma_location, hbhip_filter **out)
{
    (void)chroma_location;
    return format_scaler_make(ctx, FS_DOWN, width, height, depth, depth, src_log2_cw, src_log2_ch, dst_log2_cw, dst_log2_ch, out);
}

extern "C" int hbhip_format_scaled_create(hbhip_ctx *ctx, int width, int height, int src_depth, int dst_depth, int src_log2_cw,
                                          int src_log2_ch, int dst_log2_cw, int dst_log2_ch, int chroma_location, hbhip_filter **out)
{
    (void)chroma_location;
    return format_scaler_make(ctx, FS_DOWN, width, height, src_depth, dst_depth, src_log2_cw, src_log2_ch, dst_log2_cw, dst_log2_ch, out);
}

extern "C" int hbhip_format_upsample_create(hbhip_ctx *ctx, int width, int height, int src_depth, int dst_depth, int src_log2_cw,
                                            int src_log2_ch, int dst_log2_cw, int dst_log2_ch, int chroma_location, hbhip_filter **out)
{
    (void)chroma_location;
    return format_scaler_make(ctx, FS_UP, width, height, src_depth, dst_depth, src_log2_cw, src_log2_ch, dst_log2_cw, dst_log2_ch, out);
}

extern "C" int hbhip_format_deepen_create(hbhip_ctx *ctx, int width, int height, int src_depth, int dst_depth, int src_log2_cw,
                                          int src_log2_ch, int dst_log2_cw, int dst_log2_ch, int chroma_location, hbhip_filter **out)
{
    (void)chroma_location;
    return format_scaler_make(ctx, FS_DOWN, width, height, src_depth, dst_depth, src_log2_cw, src_log2_ch, dst_log2_cw, dst_log2_ch, out, true);
}
