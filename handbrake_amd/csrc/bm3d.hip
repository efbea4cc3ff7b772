// bm3d.hip — FFmpeg's `bm3d` filter as libhb's bm3d.c configures it (bm3d.c:44-57: `sigma` and nothing else; an alias
// filter there, a real one here: libhb/bm3d_hip.c).  FFmpeg's source is not part of the reference, so the arithmetic is a
// restatement (parity unpinned); tests/bm3d_model.py restates the same independently in numpy float64.
//
// With every option but sigma at its default the group size is 1: no block matching, no transform along a group.  What
// runs, per plane: a 16 x 16 block at every origin 0, 4, 8, ... of each axis (the last one clamped to size - 16),
//     Y   = C X C^T            unnormalised DCT-II of the raw samples, C[k][n] = cos(pi (2n + 1) k / 32)
//     Y'  = |Y[u][v]| > thr[[u = 0] + [v = 0]] ? Y : 0,   retained = the number kept
//     X^  = D Y' D^T           the matching DCT-III, D[n][k] = C[k][n] * (k ? 1/8 : 1/16): all kept is the identity
//     num += w X^, den += w    over the block's samples, w = 1 / retained (1 when nothing is kept)
// and out = clip(rint(num / den)).
//
// The four 16 x 16 products run on v_mfma_f32_16x16x4_f32 (exact f32, an fmaf chain), four instructions each.  The
// instruction's result has its column on the lane (lane & 15) and its rows 4 (lane >> 4) + r in the four registers r; used
// as the A operand of the next product, register s as k-step s, it is read as its own transpose, so every product sums
// over the previous one's ROW index and leaves the previous COLUMN index as its row index - which is what a separable
// transform needs, with no lane movement and no LDS between the four:
//     T[c][u] = sum_r X[r][c] C[u][r]      A = the samples from LDS (row 4s + (lane >> 4), column lane & 15), B = cf[s]
//     Y[u][v] = sum_c T[c][u] C[v][c]      A = T's register s,  B = cp[s]   (the k of step s is 4 (lane >> 4) + s)
//     W[v][r] = sum_u Y'[u][v] D[r][u]     A = Y' register s,   B = dp[s]
//     X^[r][c] = sum_v W[v][r] D[c][v]     A = W's register s,  B = dp[s]
// so a lane holds 12 constants (cf, cp, dp) and the thresholding happens on Y in registers: lane (u = 4 q + r, v = l).
//
// Aggregation is deterministic and without atomics: one workgroup per 64 x 48 output tile, the tile's samples with a halo
// (16 towards lower indices, 15 towards higher: a block that starts on the tile's last sample, as a clamped last block
// may, ends 15 past it) staged once in LDS as float, num / den of the tile in LDS as float2.  Every block that overlaps
// the tile is computed here, whole, and adds the part that falls into the tile.  The blocks are walked in phases by the class of their origin on each axis -
// (origin / 4) mod 4 for the grid origins, a fifth class for a clamped origin off the grid - 16 phases, 25 where the plane's
// size is no multiple of 4: blocks of one phase are 16 apart or the only one, never overlap, and so add without conflicts;
// a barrier parts the phases.  The order in which a sample receives its blocks is fixed by the phase order alone.
// The tile: 19 x 15 block origins overlap it, 16 x 12 of them are its own share - 67 % of the transforms are useful;
// 64 x 64 would give 71 % but needs 82 KiB of LDS (one workgroup a CU short of two), 32 x 32 53 %.
#include "hbhip_internal.h"

#include <math.h>
#include <stdlib.h>
#include <new>

namespace {

// ---- the recalled definition, in one place (tests/bm3d_model.py: RECALLED) ---------------------------------------------
constexpr int   BM_BLOCK = 16, BM_BSTEP = 4, BM_GROUP = 1, BM_RANGE = 9, BM_MSTEP = 1;     // block, bstep, group, range, mstep
constexpr float BM_THMSE = 0.f, BM_HDTHR = 2.7f;                                           // thmse, hdthr (float options)
constexpr int   BM_ESTIM = 0, BM_PLANES = 7;                                               // estim = basic, planes
constexpr double BM_SIGMA_MAX = 99999.9;                                                   // sigma: a float option, 0 .. 99999.9

// thr[z], z = [u = 0] + [v = 0]: t0 * sqrt2^(1 + z); the 1 is the group index 0 at group size 1
void bm3d_thresholds(float sigma, int depth, float *thr)
{
    const double t0 = (double)BM_HDTHR * (double)sigma * M_SQRT2 * BM_BLOCK * BM_BLOCK * (double)(1 << (depth - 8)) / 255.0;
    thr[0] = (float)(t0 * M_SQRT2);
    thr[1] = (float)(t0 * 2.0);
    thr[2] = (float)(t0 * (2.0 * M_SQRT2));
}

// C[k][n] = cos(pi (2n + 1) k / 32), in double, rounded once
void bm3d_dct_table(float *dct)
{
    for (int k = 0; k < BM_BLOCK; k++)
        for (int n = 0; n < BM_BLOCK; n++)
            dct[k * BM_BLOCK + n] = (float)cos(M_PI * (double)((2 * n + 1) * k) / 32.0);
}

constexpr int BM_FRAMES = 16;
constexpr int BM_TW = 64, BM_TH = 48, BM_THREADS = 256, BM_WAVES = BM_THREADS / 64;
constexpr int BM_LO = 16, BM_HI = 15;                      // halo: towards lower indices (15 needed), towards higher
constexpr int BM_RH = BM_TH + BM_LO + BM_HI;               // staged rows
constexpr int BM_RG = (BM_TW + BM_LO + BM_HI + 3) / 4;     // staged 4-sample groups per row
constexpr int BM_RP = 112;     // staged row pitch in floats, 16 mod 32: the two rows a ds_read_b32 lane group reads share no bank
constexpr int BM_AP = 68;      // accumulator row pitch in float2, 4 mod 8: rows 4 apart (the two of a ds_read_b64 lane group) neither
static_assert(BM_RP >= 4 * BM_RG && BM_RP % 32 == 16 && BM_AP >= BM_TW && BM_AP % 8 == 4, "LDS pitches");
static_assert(BM_TW % 16 == 0 && BM_TH % 16 == 0, "a tile starts on the 16-sample phase grid");

struct Bm3dArgs
{
    const uint8_t *src[BM_FRAMES][3];
    uint8_t       *dst[BM_FRAMES][3];
    int spitch[3], dpitch[3], w[3], h[3];    // pitches in bytes, sizes in samples
    float thr[3];
    const float *dct;                        // C[k][n], 256 floats
    int maxv;
    int aligned;                             // every plane pointer and pitch a multiple of 8 bytes: 4-sample groups move as one
};

typedef float f32x4 __attribute__((ext_vector_type(4)));

// 4 samples as one register: a dword of bytes or a qword of shorts
template <typename T> struct Quad;
template <> struct Quad<uint8_t>  { using V = uint32_t; };
template <> struct Quad<uint16_t> { using V = uint64_t; };

// The origins of one class on one axis that overlap the tile [t0, t0 + tsize) of a plane of `size` samples: n of them,
// 16 apart from `first`.  Classes 0 .. 3: grid origins with (origin / 4) mod 4 = cls; class 4: size - 16 where that is off
// the grid.
__device__ __forceinline__ void bm3d_origins(int t0, int tsize, int size, int cls, int &first, int &n)
{
    const int last = size - BM_BLOCK;
    if (cls == 4)
    {
        first = last;
        n = (last % BM_BSTEP != 0 && last < t0 + tsize) ? 1 : 0;      // (last + 16 = size > t0: the tile lies in the plane)
        return;
    }
    int o = t0 - BM_BLOCK + BM_BSTEP * cls;                           // t0 is a multiple of 16
    if (o + BM_BLOCK <= t0 || o < 0) o += BM_BLOCK;
    const int lim = min(t0 + tsize - 1, last);
    first = o;
    n = lim >= o ? (lim - o) / BM_BLOCK + 1 : 0;
}

template <typename T>
__global__ __launch_bounds__(BM_THREADS) void bm3d_kernel(Bm3dArgs a)
{
    using V = typename Quad<T>::V;
    __shared__ __attribute__((aligned(16))) float s_in[BM_RH * BM_RP];
    __shared__ __attribute__((aligned(16))) float2 s_acc[BM_TH * BM_AP];
    const int f = blockIdx.z / 3, c = blockIdx.z % 3;
    const int w = a.w[c], h = a.h[c];
    const int X0 = blockIdx.x * BM_TW, Y0 = blockIdx.y * BM_TH;
    if (X0 >= w || Y0 >= h) return;                                    // (the grid is sized for the luma plane)
    const int tid = threadIdx.x;
    const bool aligned = a.aligned != 0;
    const int rx0 = X0 - BM_LO, ry0 = Y0 - BM_LO;                      // plane position of s_in[0]

    // ---- stage the samples as float (0 outside the plane: no block that is computed reads there) ----
    {
        const T *src = reinterpret_cast<const T *>(a.src[f][c]);
        const int sp = a.spitch[c] / (int)sizeof(T);
        for (int i = tid; i < BM_RH * BM_RG; i += BM_THREADS)
        {
            const int row = i / BM_RG, g = i % BM_RG;
            const int y = ry0 + row, x = rx0 + 4 * g;
            float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
            if (y >= 0 && y < h && x + 3 >= 0 && x < w)
            {
                const T *line = src + (size_t)y * sp;
                if (aligned && x >= 0 && x + 3 < w)
                {
                    const V q = *reinterpret_cast<const V *>(line + x);
                    v.x = (float)(T)(q);
                    v.y = (float)(T)(q >> (8 * sizeof(T)));
                    v.z = (float)(T)(q >> (16 * sizeof(T)));
                    v.w = (float)(T)(q >> (24 * sizeof(T)));
                }
                else
                {
                    if (x >= 0 && x < w)         v.x = (float)line[x];
                    if (x + 1 >= 0 && x + 1 < w) v.y = (float)line[x + 1];
                    if (x + 2 >= 0 && x + 2 < w) v.z = (float)line[x + 2];
                    if (x + 3 >= 0 && x + 3 < w) v.w = (float)line[x + 3];
                }
            }
            *reinterpret_cast<float4 *>(s_in + row * BM_RP + 4 * g) = v;
        }
        for (int i = tid; i < BM_TH * BM_AP; i += BM_THREADS) s_acc[i] = make_float2(0.f, 0.f);
    }

    // ---- the lane's share of the transform matrices ----
    const int lane = tid & 63, wave = tid >> 6;
    const int lc = lane & 15, lq = lane >> 4;
    float cf[4], cp[4], dp[4];
#pragma unroll
    for (int s = 0; s < 4; s++)
    {
        const int k = 4 * lq + s;
        cf[s] = a.dct[lc * 16 + 4 * s + lq];
        cp[s] = a.dct[lc * 16 + k];
        dp[s] = a.dct[k * 16 + lc] * (k == 0 ? 0.0625f : 0.125f);
    }
    const float th_first = a.thr[(lc == 0) + (lq == 0)];               // register 0: u = 4 lq, v = lc
    const float th_rest  = a.thr[(lc == 0)];                           // registers 1 .. 3: u > 0
    __syncthreads();

    // ---- the blocks, phase by phase ----
    for (int cy = 0; cy < 5; cy++)
    {
        int fy, ny;
        bm3d_origins(Y0, BM_TH, h, cy, fy, ny);
        if (ny == 0) continue;
        for (int cx = 0; cx < 5; cx++)
        {
            int fx, nx;
            bm3d_origins(X0, BM_TW, w, cx, fx, nx);
            if (nx == 0) continue;
            for (int b = wave; b < nx * ny; b += BM_WAVES)
            {
                const int bx = fx + BM_BLOCK * (b % nx), by = fy + BM_BLOCK * (b / nx);
                const float *p = s_in + (by - ry0 + lq) * BM_RP + (bx - rx0 + lc);
                f32x4 t = {0.f, 0.f, 0.f, 0.f}, y = t, u = t, o = t;
#pragma unroll
                for (int s = 0; s < 4; s++) t = __builtin_amdgcn_mfma_f32_16x16x4f32(p[4 * s * BM_RP], cf[s], t, 0, 0, 0);
#pragma unroll
                for (int s = 0; s < 4; s++) y = __builtin_amdgcn_mfma_f32_16x16x4f32(t[s], cp[s], y, 0, 0, 0);
                int kept = 0;
#pragma unroll
                for (int r = 0; r < 4; r++)
                {
                    const bool keep = fabsf(y[r]) > (r == 0 ? th_first : th_rest);
                    y[r] = keep ? y[r] : 0.f;
                    kept += __popcll(__ballot(keep));
                }
#pragma unroll
                for (int s = 0; s < 4; s++) u = __builtin_amdgcn_mfma_f32_16x16x4f32(y[s], dp[s], u, 0, 0, 0);
#pragma unroll
                for (int s = 0; s < 4; s++) o = __builtin_amdgcn_mfma_f32_16x16x4f32(u[s], dp[s], o, 0, 0, 0);
                const float wgt = kept > 0 ? 1.0f / (float)kept : 1.0f;
                const int tx = bx + lc - X0;
                if (tx >= 0 && tx < BM_TW)
                {
#pragma unroll
                    for (int r = 0; r < 4; r++)
                    {
                        const int ty = by + 4 * lq + r - Y0;
                        if (ty < 0 || ty >= BM_TH) continue;
                        float2 q = s_acc[ty * BM_AP + tx];
                        q.x += wgt * o[r];
                        q.y += wgt;
                        s_acc[ty * BM_AP + tx] = q;
                    }
                }
            }
            __syncthreads();
        }
    }

    // ---- every sample of the tile, once ----
    T *dst = reinterpret_cast<T *>(a.dst[f][c]);
    const int dpitch = a.dpitch[c] / (int)sizeof(T);
    for (int i = tid; i < BM_TH * (BM_TW / 4); i += BM_THREADS)
    {
        const int row = i / (BM_TW / 4), g = i % (BM_TW / 4);
        const int y = Y0 + row, x = X0 + 4 * g;
        if (y >= h || x >= w) continue;
        int v[4];
#pragma unroll
        for (int j = 0; j < 4; j++)
        {
            const float2 q = s_acc[row * BM_AP + 4 * g + j];
            v[j] = x + j < w ? min(max((int)rintf(q.x / q.y), 0), a.maxv) : 0;      // (den > 0: block 0 or the clamped one covers it)
        }
        T *line = dst + (size_t)y * dpitch;
        if (aligned && x + 3 < w)
        {
            V q = 0;
#pragma unroll
            for (int j = 0; j < 4; j++) q |= (V)(T)v[j] << (8 * sizeof(T) * j);
            *reinterpret_cast<V *>(line + x) = q;
        }
        else
            for (int j = 0; j < 4 && x + j < w; j++) line[x + j] = (T)v[j];
    }
}

class Bm3dFilter : public BurstFilter
{
public:
    Bm3dFilter(hbhip_ctx *c, const hbhip_bm3d_params &p) : BurstFilter(c), par(p) {}
    int process_many(DevPicture *const *ins, DevPicture *const *outs, int n) override
    {
        return hbhip_for_each_burst<BM_FRAMES, Bm3dArgs>(ctx, ins, outs, n, [&](Bm3dArgs &a, int nf, int, uintptr_t bits) {
            for (int c = 0; c < 3; c++)
            {
                a.w[c] = in_geo.pw[c]; a.h[c] = in_geo.ph[c];
                a.thr[c] = par.thr[c];
                if (((a.spitch[c] | a.dpitch[c]) & (in_geo.bps - 1)) != 0) return HBHIP_ERR_ARG;
            }
            a.dct = dct.get();
            a.maxv = (1 << in_geo.depth) - 1;
            a.aligned = (bits & 7) == 0;
            const dim3 grid(hbhip_grid_x((a.w[0] + BM_TW - 1) / BM_TW), (a.h[0] + BM_TH - 1) / BM_TH, 3 * nf);
            if (in_geo.bps == 2) HBHIP_LAUNCH(ctx, "bm3d", (bm3d_kernel<uint16_t>), grid, dim3(BM_THREADS), 0, a);
            else                 HBHIP_LAUNCH(ctx, "bm3d", (bm3d_kernel<uint8_t>), grid, dim3(BM_THREADS), 0, a);
            return HBHIP_OK;
        });
    }
    hbhip_bm3d_params par;
    DevBuf<float> dct;
};

} // namespace

// "key=value:..." -> the filter's parameters.  bm3d.c hands FFmpeg hb_dict_set_double(sigma), which reaches it as "%g" text,
// and FFmpeg parses that into a float option after checking the double against the option's range.
extern "C" int hbhip_bm3d_params_from_settings(const char *settings, int depth, hbhip_bm3d_params *p)
{
    if (!p) return HBHIP_ERR_ARG;
    memset(p, 0, sizeof(*p));
    if (depth != 8 && depth != 10 && depth != 12) return HBHIP_ERR_UNSUPPORTED;
    double sigma = 1;                                                   // bm3d.c:46
    for (const char *s = settings; s && *s; )
    {
        const char *end = strchr(s, ':');
        const size_t len = end ? (size_t)(end - s) : strlen(s);
        if (len > 6 && strncmp(s, "sigma=", 6) == 0)
        {
            char val[64];
            const size_t n = len - 6 < sizeof(val) - 1 ? len - 6 : sizeof(val) - 1;
            memcpy(val, s + 6, n);
            val[n] = 0;
            char *stop = nullptr;
            const double d = strtod(val, &stop);
            if (stop != val) sigma = d;                                 // hb_dict_extract_double: unparsable leaves the default
        }
        s = end ? end + 1 : s + len;
    }
    char buf[64];                                                       // as hb_dict hands it on
    snprintf(buf, sizeof(buf), "%g", sigma);
    const double d = strtod(buf, nullptr);                              // as FFmpeg parses it
    if (!(d >= 0.0 && d <= BM_SIGMA_MAX)) return HBHIP_ERR_UNSUPPORTED; // NaN, negative, past the option's range: the graph fails
    p->sigma = (float)d;
    p->block = BM_BLOCK; p->bstep = BM_BSTEP; p->group = BM_GROUP; p->range = BM_RANGE; p->mstep = BM_MSTEP;
    p->thmse = BM_THMSE; p->hdthr = BM_HDTHR;
    p->estim = BM_ESTIM; p->planes = BM_PLANES;
    bm3d_thresholds(p->sigma, depth, p->thr);
    bm3d_dct_table(p->dct);
    return HBHIP_OK;
}

extern "C" int hbhip_bm3d_create(hbhip_ctx *ctx, const hbhip_bm3d_params *p, int width, int height, int depth,
                                 int log2_chroma_w, int log2_chroma_h, hbhip_filter **out)
{
    if (!ctx || !p || !out) return HBHIP_ERR_ARG;
    *out = nullptr;
    if (depth != 8 && depth != 10 && depth != 12) return HBHIP_ERR_UNSUPPORTED;
    if (!hbhip_yuv_layout_ok(log2_chroma_w, log2_chroma_h)) return HBHIP_ERR_UNSUPPORTED;
    // the kernel is the filter at FFmpeg's defaults: anything else is another filter
    if (p->block != BM_BLOCK || p->bstep != BM_BSTEP || p->group != BM_GROUP || p->estim != BM_ESTIM || p->planes != BM_PLANES)
        return HBHIP_ERR_UNSUPPORTED;
    if (!(p->sigma >= 0.f) || !(p->thr[0] >= 0.f) || !(p->thr[1] >= 0.f) || !(p->thr[2] >= 0.f)) return HBHIP_ERR_ARG;
    if (width < 1 || height < 1) return HBHIP_ERR_ARG;
    PicGeometry g;
    g.set(width, height, depth, log2_chroma_w, log2_chroma_h);
    for (int c = 0; c < 3; c++)
        if (g.pw[c] < BM_BLOCK || g.ph[c] < BM_BLOCK) return HBHIP_ERR_UNSUPPORTED;      // the clamped origin would be negative
    Bm3dFilter *f = hbhip_make_filter<Bm3dFilter>(ctx, g, g, *p);
    if (!f) return HBHIP_ERR_NOMEM;
    int rc = f->dct.alloc(ctx, sizeof(p->dct) / sizeof(float));
    if (rc == HBHIP_OK && hipMemcpy(f->dct.get(), p->dct, sizeof(p->dct), hipMemcpyHostToDevice) != hipSuccess) rc = HBHIP_ERR_HIP;
    if (rc != HBHIP_OK)
    {
        delete f;
        return rc;
    }
    *out = f;
    return HBHIP_OK;
}
