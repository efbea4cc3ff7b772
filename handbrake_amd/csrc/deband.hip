// deband.hip — FFmpeg's `deband` filter as libhb's deband.c configures it (deband.c:35-80; an alias filter there, a
// real one here: libhb/deband_hip.c).  FFmpeg's source is not part of the reference, so the arithmetic is a restatement
// (parity unpinned); tests/deband_model.py restates the same independently in numpy.
//
// FFmpeg's filter, without coupling: an offset table (dx, dy) per luma position, built once per input size from a
// float hash of (x, y) with libm's sinf / cosf (config_input); then per plane p and sample (x, y), with the table read
// at [y * W + x] (W the luma width: chroma uses the table's top-left corner with the luma stride) and every coordinate
// clipped to the plane:
//     ref0 = src(y+dy, x+dx)  ref1 = src(y-dy, x+dx)  ref2 = src(y-dy, x-dx)  ref3 = src(y+dy, x-dx)
//     avg  = (ref0 + ref1 + ref2 + ref3) / 4
//     blur: |src - avg| < thr[p] ? avg : src          no blur: |src - ref_i| < thr[p] for every i ? avg : src
// The table is host code on purpose: the hash multiplies sinf's result by 43758.5, so one ulp of a different sinf
// moves offsets; FFmpeg calls the host's libm and so does this (tests/test_deband_cpu.py holds it to ctypes' libm).
//
// Two kernels, both out of place, up to 16 frames per launch with one workgroup walking every frame of its tile
// (grid.z = plane), the tile's offsets held in registers across the frames:
//   * deband_tile_kernel: a 128 x 32 output tile, the input with a halo of R rows and RP >= R columns (R the table's
//     largest |offset|) in LDS, loaded with clamped coordinates - src[clip(y')][clip(x')] is exact because the clip acts
//     on each axis alone.  The next frame's tile is fetched into registers while the current one is filtered.
//   * deband_gather_kernel: the same tile of outputs gathered from global memory with clamped addresses, for tables
//     whose halo does not fit (the cut-over: DB_TILE_GROUPS).
#include "hbhip_internal.h"

#include <math.h>
#include <algorithm>
#include <new>
#include <vector>

namespace {

// ---- the recalled arithmetic, in one place (tests/deband_model.py: HASH_*, the avg / test below) ---------------------
constexpr float HASH_X = 12.9898f, HASH_Y = 78.233f, HASH_SCALE = 43758.545f;

template <bool BLUR>
__device__ __forceinline__ int db_sample(int s, int r0, int r1, int r2, int r3, int thr)
{
    const int avg = (r0 + r1 + r2 + r3) >> 2;                        // (all four >= 0: FFmpeg's / 4)
    if (BLUR) return abs(s - avg) < thr ? avg : s;
    return (abs(s - r0) < thr && abs(s - r1) < thr && abs(s - r2) < thr && abs(s - r3) < thr) ? avg : s;
}

constexpr int DB_FRAMES = 16;
constexpr int DB_TW = 128, DB_TH = 32, DB_THREADS = 256;             // a thread: 4 adjacent samples x 4 rows
constexpr int DB_TILE_GROUPS = 16;      // 4-sample groups of the LDS tile each thread fetches at most: the tile kernel's reach

struct DebandArgs
{
    const uint8_t *src[DB_FRAMES][3];
    uint8_t       *dst[DB_FRAMES][3];
    int spitch[3], dpitch[3], w[3], h[3];    // pitches in bytes, sizes in samples
    int thr[3];
    int nf;
    int aligned;                             // every plane pointer and pitch a multiple of 8 bytes: 4-sample groups move as one
    const void *table;                       // (dx, dy) per luma position: int8 pairs (R <= 127) or int16 pairs
    int tw;                                  // the table's row length (the luma width)
    int R, RP;                               // halo rows, halo columns (R rounded up to 4)
};

// 4 samples as one register: a dword of bytes or a qword of shorts
template <typename T> struct Quad;
template <> struct Quad<uint8_t>  { using V = uint32_t; };
template <> struct Quad<uint16_t> { using V = uint64_t; };

template <typename T>
__device__ __forceinline__ int quad_get(typename Quad<T>::V v, int j) { return (int)(T)(v >> (8 * sizeof(T) * j)); }

// the offsets of the thread's 16 samples: (dx & 0xffff) | dy << 16
template <bool WIDE>
__device__ __forceinline__ void load_offsets(const DebandArgs &a, int c, int x0, int y0, int *off)
{
    const int w = a.w[c], h = a.h[c];
#pragma unroll
    for (int k = 0; k < 4; k++)
#pragma unroll
        for (int j = 0; j < 4; j++)
        {
            const int x = x0 + j, y = y0 + 8 * k;
            int o = 0;
            if (x < w && y < h)
            {
                const size_t at = (size_t)y * a.tw + x;
                if (WIDE) o = reinterpret_cast<const int32_t *>(a.table)[at];          // int16 dx, int16 dy: already packed
                else
                {
                    const int d = reinterpret_cast<const int16_t *>(a.table)[at];     // int8 dx, int8 dy
                    o = ((int)(int8_t)(d & 0xff) & 0xffff) | ((d >> 8) << 16);
                }
            }
            off[4 * k + j] = o;
        }
}

__device__ __forceinline__ int off_dx(int o) { return (int)(short)(o & 0xffff); }
__device__ __forceinline__ int off_dy(int o) { return o >> 16; }

// Per frame: what is derived from these registers is derived again instead of being kept for every frame (hoisted out of
// the frame loop, the 16 samples' addresses took 166 - 256 VGPRs)
template <int N>
__device__ __forceinline__ void opaque(int *v)
{
#pragma unroll
    for (int i = 0; i < N; i++) asm volatile("" : "+v"(v[i]));
}

// 4 results at (x0 .. x0+3, y): one store where the group is whole and aligned, else sample by sample
template <typename T>
__device__ __forceinline__ void store_quad(T *row, int x0, int w, bool aligned, const int *v)
{
    using V = typename Quad<T>::V;
    if (aligned && x0 + 3 < w)
    {
        V q = 0;
#pragma unroll
        for (int j = 0; j < 4; j++) q |= (V)(T)v[j] << (8 * sizeof(T) * j);
        *reinterpret_cast<V *>(row + x0) = q;
    }
    else
        for (int j = 0; j < 4 && x0 + j < w; j++) row[x0 + j] = (T)v[j];
}

// ---- tile kernel ---------------------------------------------------------------------------------------------------------
template <typename T, bool WIDE, bool BLUR>
__global__ __launch_bounds__(DB_THREADS) void deband_tile_kernel(DebandArgs a)
{
    using V = typename Quad<T>::V;
    extern __shared__ uint64_t lds_raw[];
    V *lds_v = reinterpret_cast<V *>(lds_raw);
    T *tile = reinterpret_cast<T *>(lds_raw);
    const int c = blockIdx.z;
    const int w = a.w[c], h = a.h[c];
    const int C0 = blockIdx.x * DB_TW, R0 = blockIdx.y * DB_TH;
    if (C0 >= w || R0 >= h) return;                                    // (the grid is sized for the luma plane)
    const int R = a.R, RP = a.RP;
    const int LW = DB_TW + 2 * RP, G = LW / 4, LH = DB_TH + 2 * R;     // LDS: LH rows of LW samples, G groups per row
    const int lx0 = C0 - RP, ly0 = R0 - R;                             // plane position of tile[0]
    const int ngroups = LH * G;
    const int sp = a.spitch[c] / (int)sizeof(T), dp = a.dpitch[c] / (int)sizeof(T);
    const bool aligned = a.aligned != 0;

    // the groups this thread fetches: LDS row << 16 | group, -1 past the tile
    int grp[DB_TILE_GROUPS];
#pragma unroll
    for (int k = 0; k < DB_TILE_GROUPS; k++)
    {
        const int i = threadIdx.x + k * DB_THREADS;
        grp[k] = i < ngroups ? (i / G) << 16 | (i % G) : -1;
    }
    auto fetch = [&](int f, V *pf) {
        const T *src = reinterpret_cast<const T *>(a.src[f][c]);
#pragma unroll
        for (int k = 0; k < DB_TILE_GROUPS; k++)
        {
            if (grp[k] < 0) continue;
            const int y = min(max(ly0 + (grp[k] >> 16), 0), h - 1);
            const int x = lx0 + 4 * (grp[k] & 0xffff);
            const T *row = src + (size_t)y * sp;
            if (aligned && x >= 0 && x + 3 < w) pf[k] = *reinterpret_cast<const V *>(row + x);
            else
            {
                V q = 0;
#pragma unroll
                for (int j = 0; j < 4; j++) q |= (V)row[min(max(x + j, 0), w - 1)] << (8 * sizeof(T) * j);
                pf[k] = q;
            }
        }
    };

    const int tx = (threadIdx.x % 32) * 4, ty = threadIdx.x / 32;      // samples (C0 + tx .. +3, R0 + ty + 8k)
    int off[16];
    load_offsets<WIDE>(a, c, C0 + tx, R0 + ty, off);
    const int thr = a.thr[c];
    V pf[DB_TILE_GROUPS];
    fetch(0, pf);
    for (int f = 0; f < a.nf; f++)
    {
        opaque<DB_TILE_GROUPS>(grp);
        opaque<16>(off);
#pragma unroll
        for (int k = 0; k < DB_TILE_GROUPS; k++)
            if (grp[k] >= 0) lds_v[(grp[k] >> 16) * G + (grp[k] & 0xffff)] = pf[k];
        __syncthreads();
        if (f + 1 < a.nf) fetch(f + 1, pf);                            // in flight while this frame is filtered
        T *dst = reinterpret_cast<T *>(a.dst[f][c]);
#pragma unroll
        for (int k = 0; k < 4; k++)
        {
            const int y = R0 + ty + 8 * k;
            if (y >= h) break;
            const int ly = y - ly0, lx = C0 + tx - lx0;
            const V sq = lds_v[(ly * LW + lx) / 4];
            int v[4];
#pragma unroll
            for (int j = 0; j < 4; j++)
            {
                const int dx = off_dx(off[4 * k + j]), dy = off_dy(off[4 * k + j]);
                const T *p = tile + ly * LW + lx + j;
                const int r0 = p[dy * LW + dx], r1 = p[-dy * LW + dx], r2 = p[-dy * LW - dx], r3 = p[dy * LW - dx];
                v[j] = db_sample<BLUR>(quad_get<T>(sq, j), r0, r1, r2, r3, thr);
            }
            store_quad<T>(dst + (size_t)y * dp, C0 + tx, w, aligned, v);
        }
        __syncthreads();
    }
}

// ---- gather kernel -------------------------------------------------------------------------------------------------------
template <typename T, bool WIDE, bool BLUR>
__global__ __launch_bounds__(DB_THREADS) void deband_gather_kernel(DebandArgs a)
{
    const int c = blockIdx.z;
    const int w = a.w[c], h = a.h[c];
    const int C0 = blockIdx.x * DB_TW, R0 = blockIdx.y * DB_TH;
    if (C0 >= w || R0 >= h) return;
    const int sp = a.spitch[c] / (int)sizeof(T), dp = a.dpitch[c] / (int)sizeof(T);
    const int tx = (threadIdx.x % 32) * 4, ty = threadIdx.x / 32;
    const int x0 = C0 + tx;
    if (x0 >= w) return;
    int off[16];
    load_offsets<WIDE>(a, c, x0, R0 + ty, off);
    const int thr = a.thr[c];
    for (int f = 0; f < a.nf; f++)
    {
        opaque<16>(off);
        const T *src = reinterpret_cast<const T *>(a.src[f][c]);
        T *dst = reinterpret_cast<T *>(a.dst[f][c]);
#pragma unroll
        for (int k = 0; k < 4; k++)
        {
            const int y = R0 + ty + 8 * k;
            if (y >= h) break;
            int v[4];
#pragma unroll
            for (int j = 0; j < 4; j++)
            {
                const int x = min(x0 + j, w - 1);
                const int dx = off_dx(off[4 * k + j]), dy = off_dy(off[4 * k + j]);
                const T *ya = src + (size_t)min(max(y + dy, 0), h - 1) * sp;
                const T *yb = src + (size_t)min(max(y - dy, 0), h - 1) * sp;
                const int xa = min(max(x + dx, 0), w - 1), xb = min(max(x - dx, 0), w - 1);
                v[j] = db_sample<BLUR>(src[(size_t)y * sp + x], ya[xa], yb[xa], yb[xb], ya[xb], thr);
            }
            store_quad<T>(dst + (size_t)y * dp, x0, w, a.aligned != 0, v);
        }
    }
}

class DebandFilter : public BurstFilter
{
public:
    DebandFilter(hbhip_ctx *c, const hbhip_deband_params &p) : BurstFilter(c), par(p) {}
    // the tile kernel's LDS bytes (0: its halo does not fit)
    int tile_bytes() const
    {
        const int LW = DB_TW + 2 * RP, LH = DB_TH + 2 * R;
        if ((size_t)LH * (LW / 4) > (size_t)DB_TILE_GROUPS * DB_THREADS) return 0;
        return LH * LW * in_geo.bps;
    }
    bool use_tile() const { return kernel == 1 || (kernel == 0 && tile_bytes() > 0); }
    template <bool WIDE, bool BLUR>
    void launch(const DebandArgs &a, dim3 grid)
    {
        const bool deep = in_geo.bps == 2;
        if (use_tile())
        {
            const int bytes = tile_bytes();
            if (deep) HBHIP_LAUNCH(ctx, "deband_tile", (deband_tile_kernel<uint16_t, WIDE, BLUR>), grid, dim3(DB_THREADS), bytes, a);
            else      HBHIP_LAUNCH(ctx, "deband_tile", (deband_tile_kernel<uint8_t, WIDE, BLUR>), grid, dim3(DB_THREADS), bytes, a);
        }
        else
        {
            if (deep) HBHIP_LAUNCH(ctx, "deband_gather", (deband_gather_kernel<uint16_t, WIDE, BLUR>), grid, dim3(DB_THREADS), 0, a);
            else      HBHIP_LAUNCH(ctx, "deband_gather", (deband_gather_kernel<uint8_t, WIDE, BLUR>), grid, dim3(DB_THREADS), 0, a);
        }
    }
    int process_many(DevPicture *const *ins, DevPicture *const *outs, int n) override
    {
        return hbhip_for_each_burst<DB_FRAMES, DebandArgs>(ctx, ins, outs, n, [&](DebandArgs &a, int nf, int, uintptr_t bits) {
            for (int c = 0; c < 3; c++)
            {
                a.w[c] = in_geo.pw[c]; a.h[c] = in_geo.ph[c];
                a.thr[c] = par.thr[c];
                if (((a.spitch[c] | a.dpitch[c]) & (in_geo.bps - 1)) != 0) return HBHIP_ERR_ARG;
            }
            a.nf = nf;
            a.aligned = (bits & 7) == 0;
            a.table = table.get();
            a.tw = in_geo.pw[0];
            a.R = R; a.RP = RP;
            const dim3 grid(hbhip_grid_x((a.w[0] + DB_TW - 1) / DB_TW), (a.h[0] + DB_TH - 1) / DB_TH, 3);
            if (wide_table) { if (par.blur) launch<true, true>(a, grid);  else launch<true, false>(a, grid); }
            else            { if (par.blur) launch<false, true>(a, grid); else launch<false, false>(a, grid); }
            return HBHIP_OK;
        });
    }
    hbhip_deband_params par;
    DevBuf<uint8_t> table;
    bool wide_table = false;
    int R = 0, RP = 0;
    int kernel = 0;                     // hbhip_deband_set_kernel
};

} // namespace

extern "C" int hbhip_deband_offsets(int width, int height, int range, float direction, int *x_pos, int *y_pos)
{
    if (width < 1 || height < 1 || !x_pos || !y_pos) return HBHIP_ERR_ARG;
    if (range > (1 << 30) || range < -(1 << 30)) return HBHIP_ERR_ARG;
    for (int y = 0; y < height; y++)
        for (int x = 0; x < width; x++)
        {
            // float throughout, one rounding per operation (HIPFLAGS: -ffp-contract=off)
            const float a = (float)x * HASH_X + (float)y * HASH_Y;
            float r = sinf(a) * HASH_SCALE;
            r = r - floorf(r);
            const float dir = direction < 0 ? -direction : r * direction;
            const int dist = range < 0 ? -range : (int)(r * (float)range);
            const size_t at = (size_t)y * width + x;
            x_pos[at] = (int)(cosf(dir) * (float)dist);
            y_pos[at] = (int)(sinf(dir) * (float)dist);
        }
    return HBHIP_OK;
}

extern "C" int hbhip_deband_create(hbhip_ctx *ctx, const hbhip_deband_params *p, int width, int height, int depth,
                                   int log2_chroma_w, int log2_chroma_h, hbhip_filter **out)
{
    if (!ctx || !p || !out) return HBHIP_ERR_ARG;
    *out = nullptr;
    if (depth != 8 && depth != 10 && depth != 12) return HBHIP_ERR_UNSUPPORTED;
    if (!hbhip_yuv_layout_ok(log2_chroma_w, log2_chroma_h)) return HBHIP_ERR_UNSUPPORTED;
    if (width < 1 || height < 1 || (p->blur != 0 && p->blur != 1)) return HBHIP_ERR_ARG;
    if (p->range > (1 << 30) || p->range < -(1 << 30)) return HBHIP_ERR_ARG;
    // the table, clamped to +-max(W, H): any |offset| >= a plane's size clips to the same edge in either sign
    const size_t n = (size_t)width * height;
    std::vector<int> xp, yp;
    try { xp.resize(n); yp.resize(n); } catch (...) { return HBHIP_ERR_NOMEM; }
    int rc = hbhip_deband_offsets(width, height, p->range, p->direction, xp.data(), yp.data());
    if (rc != HBHIP_OK) return rc;
    const int lim = width > height ? width : height;
    int R = 0;
    for (size_t i = 0; i < n; i++)
    {
        xp[i] = xp[i] > lim ? lim : (xp[i] < -lim ? -lim : xp[i]);
        yp[i] = yp[i] > lim ? lim : (yp[i] < -lim ? -lim : yp[i]);
        R = std::max(R, std::max(abs(xp[i]), abs(yp[i])));
    }
    const bool wide = R > 127;
    std::vector<int8_t> t8;
    std::vector<int16_t> t16;
    try { if (wide) t16.resize(2 * n); else t8.resize(2 * n); } catch (...) { return HBHIP_ERR_NOMEM; }
    for (size_t i = 0; i < n; i++)
        if (wide) { t16[2 * i] = (int16_t)xp[i]; t16[2 * i + 1] = (int16_t)yp[i]; }
        else      { t8[2 * i] = (int8_t)xp[i];   t8[2 * i + 1] = (int8_t)yp[i]; }
    PicGeometry g;
    g.set(width, height, depth, log2_chroma_w, log2_chroma_h);
    DebandFilter *f = hbhip_make_filter<DebandFilter>(ctx, g, g, *p);
    if (!f) return HBHIP_ERR_NOMEM;
    f->wide_table = wide;
    f->R = R;
    f->RP = (R + 3) & ~3;
    const size_t bytes = 2 * n * (wide ? sizeof(int16_t) : sizeof(int8_t));
    rc = f->table.alloc(ctx, bytes);
    if (rc == HBHIP_OK && hipMemcpy(f->table.get(), wide ? (const void *)t16.data() : (const void *)t8.data(), bytes, hipMemcpyHostToDevice) != hipSuccess)
        rc = HBHIP_ERR_HIP;
    if (rc != HBHIP_OK)
    {
        delete f;
        return rc;
    }
    *out = f;
    return HBHIP_OK;
}

extern "C" int hbhip_deband_set_kernel(hbhip_filter *f, int kernel)
{
    DebandFilter *d = dynamic_cast<DebandFilter *>(f);
    if (d == nullptr || kernel < 0 || kernel > 2) return HBHIP_ERR_ARG;
    if (kernel == 1 && d->tile_bytes() == 0) return HBHIP_ERR_UNSUPPORTED;
    d->kernel = kernel;
    return HBHIP_OK;
}
