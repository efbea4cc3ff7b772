// deblock.hip — FFmpeg's `deblock` filter as libhb's deblock.c configures it (deblock.c:37-86; an alias filter there,
// a real one here: libhb/deblock_hip.c).  FFmpeg's source is not part of the reference, so the arithmetic is a
// restatement (parity unpinned): the loop order is certain, the tap divisors below and the strong
// filter's fifth skip test (|B - A| and |E - F| against delta) are recalled.  tests/deblock_model.py restates the same
// independently in numpy.
//
// Order of FFmpeg's filter_frame (output = a copy of the input, filtered in place, every plane with the same block b):
//     vertical edges x = b, 2b, .. < w of rows 0 .. b-1;  then for y = b, 2b, .. < h: the horizontal edge at y across
//     every column, then the vertical edges of rows y .. y+b-1.
// A vertical edge filters a row across columns x-L .. x+L-1, a horizontal one a column across rows y-L .. y+L-1
// (L = 3 strong, 2 weak).  Two kernels (DESIGN §4.16 has the dependency argument):
//   * deblock_local_kernel: weak with any b, strong with b >= 6.  No two windows of one direction overlap, and what a
//     block row hands the next is a function of the input alone: every output sample depends on its own horizontal band
//     and vertical window only.  So tiles with a 5-sample halo are exact: V on the rows outside [y, y+L), H, V on the
//     rows inside [y, y+L) - three phases in LDS, every output sample written once.
//   * deblock_web_kernel: strong with b = 4 / 5, where windows overlap in both directions and the plane is one web.
//     One workgroup per plane walks the block rows in order in the output frame; a block row's vertical edges form a
//     left-to-right chain along each row, cut into segments that start `warmup` edges early from the unfiltered samples
//     (the chain forgets at every edge that does not fire) and are then repaired serially where the guess was wrong.
//     Exact for any input and any warm-up (0 makes every segment boundary a repair candidate: the tests force it).
#include "hbhip_internal.h"

#include <new>

namespace {

// ---- the recalled arithmetic, in one place (tests/deblock_model.py: WEAK_DIV / STRONG_DIV) -----------------------------
// the tap moves by delta / DIV[k] (C int division: truncates towards zero), towards the other side of the edge
constexpr int WEAK_DIV[4]   = { 8, 2, 2, 8 };            // A += d/8, B += d/2, C -= d/2, D -= d/8     (d = C - B)
constexpr int STRONG_DIV[6] = { 8, 4, 2, 2, 4, 8 };      // A..C += d/8, d/4, d/2; D..F -= d/2, d/4, d/8 (d = D - C)

struct DbThr { int ath, bth, gth, dth, maxv; };

__device__ __forceinline__ int db_clip(int v, int maxv) { return v < 0 ? 0 : (v > maxv ? maxv : v); }

// one edge: v[0 .. 2L-1] are the samples p[-L .. L-1] across it, filtered in place
template <bool STRONG>
__device__ __forceinline__ void db_edge(int *v, const DbThr &t)
{
    if (STRONG)
    {
        const int d = v[3] - v[2];
        if (abs(d) >= t.ath || abs(v[2] - v[1]) >= t.bth || abs(v[3] - v[4]) >= t.gth ||
            abs(v[1] - v[0]) >= t.dth || abs(v[4] - v[5]) >= t.dth) return;
        v[0] = db_clip(v[0] + d / STRONG_DIV[0], t.maxv);
        v[1] = db_clip(v[1] + d / STRONG_DIV[1], t.maxv);
        v[2] = db_clip(v[2] + d / STRONG_DIV[2], t.maxv);
        v[3] = db_clip(v[3] - d / STRONG_DIV[3], t.maxv);
        v[4] = db_clip(v[4] - d / STRONG_DIV[4], t.maxv);
        v[5] = db_clip(v[5] - d / STRONG_DIV[5], t.maxv);
    }
    else
    {
        const int d = v[2] - v[1];
        if (abs(d) >= t.ath || abs(v[1] - v[0]) >= t.bth || abs(v[2] - v[3]) >= t.gth) return;
        v[0] = db_clip(v[0] + d / WEAK_DIV[0], t.maxv);
        v[1] = db_clip(v[1] + d / WEAK_DIV[1], t.maxv);
        v[2] = db_clip(v[2] - d / WEAK_DIV[2], t.maxv);
        v[3] = db_clip(v[3] - d / WEAK_DIV[3], t.maxv);
    }
}

constexpr int DB_FRAMES = 16;
struct DeblockArgs
{
    const uint8_t *src[DB_FRAMES][3];
    uint8_t       *dst[DB_FRAMES][3];
    int spitch[3], dpitch[3], w[3], h[3];    // pitches in bytes, sizes in samples
    int block;
    DbThr thr;
};

// ---- local kernel ------------------------------------------------------------------------------------------------------
// A workgroup makes a DB_TW x DB_TH output tile from the input with a halo of DB_HX columns and DB_HY rows on each side
// (a band [y-3, y+3) or window [x-3, x+3) that reaches into the tile lies inside the halo: 5 would do; the columns take 8).
constexpr int DB_TW = 128, DB_TH = 32, DB_HX = 8, DB_HY = 5;
constexpr int DB_LW = DB_TW + 2 * DB_HX, DB_LH = DB_TH + 2 * DB_HY;

template <typename T, bool STRONG>
__global__ __launch_bounds__(256) void deblock_local_kernel(DeblockArgs a)
{
    constexpr int L = STRONG ? 3 : 2, N = 2 * L;
    __shared__ unsigned short t[DB_LH][DB_LW];
    const int c = blockIdx.z % 3, f = blockIdx.z / 3;
    const int w = a.w[c], h = a.h[c], b = a.block;
    const int C0 = blockIdx.x * DB_TW, R0 = blockIdx.y * DB_TH;
    if (C0 >= w || R0 >= h) return;                                  // (the grid is sized for the largest plane)
    const int lc0 = C0 - DB_HX, lr0 = R0 - DB_HY;                    // plane position of t[0][0]
    const int cs = max(lc0, 0), ce = min(C0 + DB_TW + DB_HX, w);     // loaded: columns [cs, ce), rows [rs, re)
    const int rs = max(lr0, 0), re = min(R0 + DB_TH + DB_HY, h);
    const T *src = reinterpret_cast<const T *>(a.src[f][c]);
    const int sp = a.spitch[c] / (int)sizeof(T);
    for (int i = threadIdx.x; i < (re - rs) * DB_LW; i += 256)
    {
        const int r = rs + i / DB_LW, x = lc0 + i % DB_LW;
        if (x >= cs && x < ce) t[r - lr0][x - lc0] = src[(size_t)r * sp + x];
    }
    __syncthreads();
    const DbThr thr = a.thr;

    // vertical edges whose whole window is loaded: x = xa, xa + b, .. <= xz
    const int xa = max(b, (cs + L + b - 1) / b * b), xz = min(ce - L, w - 1);
    const int nx = xz >= xa ? (xz - xa) / b + 1 : 0;
    // horizontal edges whose whole band is loaded
    const int ya = max(b, (rs + L + b - 1) / b * b), yz = min(re - L, h - 1);
    const int ny = yz >= ya ? (yz - ya) / b + 1 : 0;

    // phase 1 / 3: V on the rows outside (phase 1) / inside (phase 3) the lower half [y, y+L) of a band
    auto vpass = [&](bool lower_half) {
        for (int i = threadIdx.x; i < (re - rs) * nx; i += 256)
        {
            const int r = rs + i / nx, x = xa + (i % nx) * b;
            const int yb = r / b * b;
            if ((yb >= b && r - yb < L) != lower_half) continue;
            unsigned short *p = &t[r - lr0][x - L - lc0];
            int v[N];
#pragma unroll
            for (int k = 0; k < N; k++) v[k] = p[k];
            db_edge<STRONG>(v, thr);
#pragma unroll
            for (int k = 0; k < N; k++) p[k] = (unsigned short)v[k];
        }
    };
    vpass(false);
    __syncthreads();
    for (int i = threadIdx.x; i < ny * (ce - cs); i += 256)          // phase 2: H across every loaded column
    {
        const int y = ya + (i / (ce - cs)) * b, x = cs + i % (ce - cs);
        int v[N];
#pragma unroll
        for (int k = 0; k < N; k++) v[k] = t[y - L + k - lr0][x - lc0];
        db_edge<STRONG>(v, thr);
#pragma unroll
        for (int k = 0; k < N; k++) t[y - L + k - lr0][x - lc0] = (unsigned short)v[k];
    }
    __syncthreads();
    vpass(true);
    __syncthreads();

    T *dst = reinterpret_cast<T *>(a.dst[f][c]);
    const int dp = a.dpitch[c] / (int)sizeof(T);
    const int ow = min(DB_TW, w - C0), oh = min(DB_TH, h - R0);
    for (int i = threadIdx.x; i < oh * DB_TW; i += 256)
    {
        const int r = i / DB_TW, x = i % DB_TW;
        if (x < ow) dst[(size_t)(R0 + r) * dp + C0 + x] = (T)t[r + DB_HY][x + DB_HX];
    }
}

// ---- web kernel (strong, b = 4 / 5) ---------------------------------------------------------------------------------------
// The carried state of a row's chain: the OV = 6 - b samples the next window re-reads.
constexpr int DB_WEB_THREADS = 256;

struct WebRow
{
    const unsigned short *in;     // the row after the block row's horizontal edge (LDS)
    int b, ov, ne;                // block, carried samples, edges in the row
};

// edges [e0, e1) of one row from carried state `cs` (cs[0 .. ov-1]: the first window's leftmost samples); leaves the
// state behind edge e1-1 in cs.  out != nullptr: writes every sample the walk has finished (and, at the row's last edge,
// the carried ones too).
template <typename T>
__device__ void web_walk(const WebRow &r, int e0, int e1, int *cs, const DbThr &thr, T *out)
{
    for (int e = e0; e < e1; e++)
    {
        const int x = (e + 1) * r.b;
        int v[6];
        v[0] = cs[0];
        v[1] = r.ov == 2 ? cs[1] : r.in[x - 2];
#pragma unroll
        for (int k = 2; k < 6; k++) v[k] = r.in[x - 3 + k];
        db_edge<true>(v, thr);
        if (out != nullptr)
        {
            for (int k = 0; k < r.b; k++) out[x - 3 + k] = (T)v[k];
            if (e == r.ne - 1)
                for (int k = r.b; k < 6; k++) out[x - 3 + k] = (T)v[k];
        }
        cs[0] = v[r.b];
        cs[1] = r.ov == 2 ? v[5] : 0;
    }
}

__device__ __forceinline__ void web_entry(const WebRow &r, int e, int *cs)   // the unfiltered state in front of edge e
{
    const int x = (e + 1) * r.b;
    cs[0] = r.in[x - 3];
    cs[1] = r.ov == 2 ? r.in[x - 2] : 0;
}

template <typename T>
__global__ __launch_bounds__(DB_WEB_THREADS) void deblock_web_kernel(DeblockArgs a, int seg, int warmup, int rows_lds)
{
    extern __shared__ unsigned short smem[];
    const int c = blockIdx.z % 3, f = blockIdx.z / 3;
    const int w = a.w[c], h = a.h[c], b = a.block;
    const T *src = reinterpret_cast<const T *>(a.src[f][c]);
    T *dst = reinterpret_cast<T *>(a.dst[f][c]);
    const int sp = a.spitch[c] / (int)sizeof(T), dp = a.dpitch[c] / (int)sizeof(T);
    const DbThr thr = a.thr;
    for (int r = 0; r < h; r++)                                          // out = in, then filtered in place
        for (int x = threadIdx.x; x < w; x += DB_WEB_THREADS) dst[(size_t)r * dp + x] = src[(size_t)r * sp + x];
    __syncthreads();
    const int ne = (w - 1) / b, nseg = (ne + seg - 1) / seg;
    unsigned short *rows = smem;                                         // rows_lds rows of w samples
    unsigned short *ent = rows + rows_lds * w;                           // per (row, segment): entry state, 2 samples
    unsigned short *ext = ent + rows_lds * nseg * 2;                     //                     exit state
    for (int y = 0; y < h; y += b)
    {
        if (y > 0)                                                       // the horizontal edge at y, every column
        {
            for (int x = threadIdx.x; x < w; x += DB_WEB_THREADS)
            {
                int v[6];
#pragma unroll
                for (int k = 0; k < 6; k++) v[k] = dst[(size_t)(y - 3 + k) * dp + x];
                db_edge<true>(v, thr);
#pragma unroll
                for (int k = 0; k < 6; k++) dst[(size_t)(y - 3 + k) * dp + x] = (T)v[k];
            }
            __syncthreads();
        }
        if (ne == 0) continue;
        const int yn = min(b, h - y);
        for (int r0 = y; r0 < y + yn; r0 += rows_lds)
        {
            const int nr = min(rows_lds, y + yn - r0);
            for (int rr = 0; rr < nr; rr++)
                for (int x = threadIdx.x; x < w; x += DB_WEB_THREADS) rows[rr * w + x] = (unsigned short)dst[(size_t)(r0 + rr) * dp + x];
            __syncthreads();
            // speculative pass: every segment from a guessed entry state (its warm-up edges walked from unfiltered samples)
            for (int i = threadIdx.x; i < nr * nseg; i += DB_WEB_THREADS)
            {
                const int rr = i / nseg, s = i % nseg;
                const WebRow row = { rows + rr * w, b, 6 - b, ne };
                const int e0 = s * seg, e1 = min(ne, e0 + seg), ew = max(0, e0 - warmup);
                int cs[2];
                web_entry(row, ew, cs);
                web_walk<T>(row, ew, e0, cs, thr, nullptr);
                ent[2 * i] = (unsigned short)cs[0]; ent[2 * i + 1] = (unsigned short)cs[1];
                web_walk<T>(row, e0, e1, cs, thr, nullptr);
                ext[2 * i] = (unsigned short)cs[0]; ext[2 * i + 1] = (unsigned short)cs[1];
            }
            __syncthreads();
            // repair: along each row, a segment whose guessed entry is not its predecessor's exit is walked again
            if (threadIdx.x < nr)
            {
                const int rr = threadIdx.x;
                const WebRow row = { rows + rr * w, b, 6 - b, ne };
                for (int s = 1; s < nseg; s++)
                {
                    const int i = rr * nseg + s;
                    if (ent[2 * i] == ext[2 * i - 2] && ent[2 * i + 1] == ext[2 * i - 1]) continue;
                    int cs[2] = { ext[2 * i - 2], ext[2 * i - 1] };
                    ent[2 * i] = (unsigned short)cs[0]; ent[2 * i + 1] = (unsigned short)cs[1];
                    web_walk<T>(row, s * seg, min(ne, s * seg + seg), cs, thr, nullptr);
                    ext[2 * i] = (unsigned short)cs[0]; ext[2 * i + 1] = (unsigned short)cs[1];
                }
            }
            __syncthreads();
            // final pass: every segment from its settled entry, written to the output row
            for (int i = threadIdx.x; i < nr * nseg; i += DB_WEB_THREADS)
            {
                const int rr = i / nseg, s = i % nseg;
                const WebRow row = { rows + rr * w, b, 6 - b, ne };
                int cs[2];
                if (s == 0) web_entry(row, 0, cs);
                else { cs[0] = ent[2 * i]; cs[1] = ent[2 * i + 1]; }
                web_walk<T>(row, s * seg, min(ne, s * seg + seg), cs, thr, dst + (size_t)(r0 + rr) * dp);
            }
            __syncthreads();
        }
    }
}

constexpr int DB_WEB_SEG = 8;           // edges per segment
constexpr int DB_WEB_LDS = 48 * 1024;   // bytes of LDS the web kernel takes at most

class DeblockFilter : public BurstFilter
{
public:
    DeblockFilter(hbhip_ctx *c, const hbhip_deblock_params &p) : BurstFilter(c), par(p) {}
    bool web() const { return par.strong && par.block < 6; }
    // LDS of the web kernel for planes up to `w` samples wide: rows of the block row it holds at once (0: none fits)
    static int web_rows(int w, int b, int *bytes)
    {
        const int nseg = ((w - 1) / b + DB_WEB_SEG - 1) / DB_WEB_SEG;
        const int per_row = w * 2 + nseg * 8;
        const int rows = min(b, DB_WEB_LDS / per_row);
        *bytes = rows * per_row;
        return rows;
    }
    int process_many(DevPicture *const *ins, DevPicture *const *outs, int n) override
    {
        return hbhip_for_each_burst<DB_FRAMES, DeblockArgs>(ctx, ins, outs, n, [&](DeblockArgs &a, int nf, int, uintptr_t) {
            for (int c = 0; c < 3; c++)
            {
                a.w[c] = in_geo.pw[c]; a.h[c] = in_geo.ph[c];
                if (((a.spitch[c] | a.dpitch[c]) & (in_geo.bps - 1)) != 0) return HBHIP_ERR_ARG;
            }
            a.block = par.block;
            a.thr = { par.ath, par.bth, par.gth, par.dth, (1 << in_geo.depth) - 1 };
            const bool wide = in_geo.bps == 2;
            if (web())
            {
                int bytes = 0;
                const int rows = web_rows(in_geo.pw[0], par.block, &bytes);
                const dim3 grid(1, 1, 3 * nf);
                if (wide) HBHIP_LAUNCH(ctx, "deblock_web", deblock_web_kernel<uint16_t>, grid, dim3(DB_WEB_THREADS), bytes, a, DB_WEB_SEG, warmup, rows);
                else      HBHIP_LAUNCH(ctx, "deblock_web", deblock_web_kernel<uint8_t>, grid, dim3(DB_WEB_THREADS), bytes, a, DB_WEB_SEG, warmup, rows);
            }
            else
            {
                const dim3 grid(hbhip_grid_x((a.w[0] + DB_TW - 1) / DB_TW), (a.h[0] + DB_TH - 1) / DB_TH, 3 * nf);
                if (par.strong)
                {
                    if (wide) HBHIP_LAUNCH(ctx, "deblock", (deblock_local_kernel<uint16_t, true>), grid, dim3(256), 0, a);
                    else      HBHIP_LAUNCH(ctx, "deblock", (deblock_local_kernel<uint8_t, true>), grid, dim3(256), 0, a);
                }
                else
                {
                    if (wide) HBHIP_LAUNCH(ctx, "deblock", (deblock_local_kernel<uint16_t, false>), grid, dim3(256), 0, a);
                    else      HBHIP_LAUNCH(ctx, "deblock", (deblock_local_kernel<uint8_t, false>), grid, dim3(256), 0, a);
                }
            }
            return HBHIP_OK;
        });
    }
    hbhip_deblock_params par;
    int warmup = 4;                     // the web kernel's warm-up edges (hbhip_deblock_set_warmup)
};

// the window of a plane's last edge must end inside the plane (FFmpeg reads the line padding there otherwise)
bool deblock_plane_ok(int size, int b, bool strong)
{
    if (size <= b) return true;                        // no edge
    const int r = size % b;
    return strong ? (r != 1 && r != 2) : r != 1;
}

} // namespace

extern "C" int hbhip_deblock_create(hbhip_ctx *ctx, const hbhip_deblock_params *p, int width, int height, int depth,
                                    int log2_chroma_w, int log2_chroma_h, hbhip_filter **out)
{
    if (!ctx || !p || !out) return HBHIP_ERR_ARG;
    *out = nullptr;
    if (depth != 8 && depth != 10 && depth != 12) return HBHIP_ERR_UNSUPPORTED;
    if (width < 1 || height < 1 || p->block < 4 || p->block > 512) return HBHIP_ERR_ARG;
    PicGeometry g;
    g.set(width, height, depth, log2_chroma_w, log2_chroma_h);
    for (int c = 0; c < 3; c++)
        if (!deblock_plane_ok(g.pw[c], p->block, p->strong != 0) || !deblock_plane_ok(g.ph[c], p->block, p->strong != 0))
            return HBHIP_ERR_UNSUPPORTED;
    if (p->strong && p->block < 6)
    {
        int bytes = 0;
        if (DeblockFilter::web_rows(width, p->block, &bytes) < 1) return HBHIP_ERR_UNSUPPORTED;
    }
    hbhip_deblock_params q = *p;
    q.strong = p->strong != 0;
    *out = hbhip_make_filter<DeblockFilter>(ctx, g, g, q);
    return *out ? HBHIP_OK : HBHIP_ERR_NOMEM;
}

extern "C" int hbhip_deblock_set_warmup(hbhip_filter *f, int edges)
{
    DeblockFilter *d = dynamic_cast<DeblockFilter *>(f);
    if (d == nullptr || edges < 0) return HBHIP_ERR_ARG;
    d->warmup = edges;
    return HBHIP_OK;
}
