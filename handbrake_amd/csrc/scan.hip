// scan.hip — what the title scan does with the pixels of a preview (libhb/scan.c, libhb/hb.c) on gfx950, for pictures that
// are in HBM already: the black-border walk that gives a title its automatic crop (scan.c:986-1052 over row_all_dark /
// column_all_dark, :456-509) and hb_detect_comb (hb.c:1088-1167, called at scan.c:973).  Scan-time pictures are 8-bit
// limited-range yuv420p with even sizes (decavcodec.c:1359-1369), and that is all this file takes.
//
// The definition, all integer:
//  * c(v) = max(v, 16).  A row is dark when avg = (sum of c) / width < 32 and every |avg - c| <= 16, which is
//    max c - avg <= 16 && avg - min c <= 16: sum, min and max of the clamped samples are all a row has to give.  A column
//    the same over rows top .. height - 1 - bottom, so it hangs on the rows' answer.
//  * the walk: h4 = height / 4, w4 = width / 4, border = height / 100; top runs from `border` while rows are dark and
//    top < h4; if it never left `border`, rows 0 .. border - 1 decide: all dark -> 0, else the first that is not.  bottom
//    mirrors top; left / right run from 0 while columns are dark and < w4.  recorded = all four below h4 / w4.
//  * hb_detect_comb: per plane and column, n = 0, 2, .. < height - 4 over rows n .. n + 3: cc_1 counts |s1 - s3| < equal &&
//    |s1 - s2| > diff, cc_2 the same of s2, s4, s3.  The reference never resets cc_1 / cc_2 between planes, so plane k's
//    score (int)((cc_1 + cc_2) * 1000.0 / (width * height)) holds the counts of the planes before it: the kernel counts per
//    plane and the host adds them up in plane order.
//
// Five launches per picture on the context's stream, behind the frame's contents (hbhip_frame_use_on):
//   scan_row_stats   a wave per row of [0, h4) and [height - h4, height) - the rows the walk can reach, the `border` rows
//                    among them, and no others: 16-byte loads, a wave reduction, three stores.  It also resets what the
//                    later launches accumulate into (the column statistics, the combing counters).
//   scan_row_decide  one wave: the top / bottom walk, two ints to device memory - no host round trip in front of the columns.
//   scan_col_stats   columns [0, w4) and [width - w4, width) over rows top .. height - 1 - bottom, read from device memory;
//                    the grid covers the whole height whatever they are.  A thread takes four columns (one dword a row)
//                    of every 16th row of its 128-row band; LDS, then one integer atomic per column, band and statistic.
//   scan_col_decide  one wave: left / right and `recorded`.
//   scan_comb        the three planes in one grid: a thread takes four columns and eight row pairs (18 rows, each loaded
//                    once), a wave reduction, ONE 64-bit integer atomic per wave (cc_1 in the low, cc_2 in the high half).
// Integer adds, minima and maxima commute: the result does not depend on the order.  The record (four crops, the flag, the
// six counts: 48 bytes) is copied to pinned host memory behind the fifth launch; nothing else crosses the bus.
//
// Rows and columns are stored mirrored - entry i of the second half is row height - 1 - i / column width - 1 - i - so that
// the two walks of a pair are the same code.  Every load is a whole dword or four of them inside the row's pitch: frames are
// laid out with 64-byte rows (hbhip_frame_alloc), bytes beyond the width are read and masked.
#include "hbhip_internal.h"

namespace {

struct ScanRecord
{
    int top, bottom, left, right, recorded, pad;
    unsigned long long cc[3];                    // per plane: cc_1 | cc_2 << 32, that plane's own counts
};
static_assert(sizeof(ScanRecord) == HBHIP_SCAN_RECORD_BYTES, "the record is what hbhip.h says crosses the bus");

constexpr int kColBandRows = 128;                // rows of one scan_col_stats workgroup: 16 row lanes x 8 rows
constexpr int kCombPairs = 8;                    // row pairs of one scan_comb thread

__device__ __forceinline__ int wave_sum(int v)
{
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
    return v;
}
__device__ __forceinline__ int wave_min(int v)
{
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v = min(v, __shfl_xor(v, off, 64));
    return v;
}
__device__ __forceinline__ int wave_max(int v)
{
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v = max(v, __shfl_xor(v, off, 64));
    return v;
}

// row slot i -> picture row: [0, h4) from the top, [h4, 2 h4) from the bottom upwards
__global__ __launch_bounds__(256) void scan_row_stats_kernel(const uint8_t *__restrict__ luma, int pitch, int width, int height,
                                                             int h4, int w4, int *__restrict__ rows, int *__restrict__ cols,
                                                             ScanRecord *__restrict__ rec)
{
    const int tid = blockIdx.x * 256 + threadIdx.x;
    for (int i = tid; i < 2 * w4; i += gridDim.x * 256)
    {
        cols[3 * i] = 0; cols[3 * i + 1] = 255; cols[3 * i + 2] = 0;
    }
    if (tid < 3) rec->cc[tid] = 0;

    const int i = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (i >= 2 * h4) return;
    const int y = i < h4 ? i : height - 1 - (i - h4);
    const uint4 *row = reinterpret_cast<const uint4 *>(luma + (size_t)y * pitch);
    int sum = 0, mn = 255, mx = 0;
    for (int v = lane; 16 * v < width; v += 64)
    {
        const uint4 q = row[v];
        const unsigned d[4] = {q.x, q.y, q.z, q.w};
        const int valid = width - 16 * v;        // samples of this vector that are the row's
#pragma unroll
        for (int k = 0; k < 16; k++)
        {
            const int c = max((int)((d[k >> 2] >> (8 * (k & 3))) & 0xff), 16);
            const bool in = k < valid;
            sum += in ? c : 0;
            mn = in ? min(mn, c) : mn;
            mx = in ? max(mx, c) : mx;
        }
    }
    sum = wave_sum(sum); mn = wave_min(mn); mx = wave_max(mx);
    if (lane == 0)
    {
        rows[3 * i] = sum; rows[3 * i + 1] = mn; rows[3 * i + 2] = mx;
    }
}

// row_all_dark / column_all_dark on (sum, min, max) of the clamped samples; n = how many there were
__device__ __forceinline__ bool stat_dark(const int *s, int n)
{
    const int avg = s[0] / n;
    return avg < 32 && s[2] - avg <= 16 && avg - s[1] <= 16;
}

// the first entry of [lo, hi) that is not dark, else hi; the whole wave calls it and every lane gets the answer
__device__ __forceinline__ int first_not_dark(const int *stats, int n, int lo, int hi, int lane)
{
    int best = hi;
    for (int i = lo + lane; i < hi; i += 64)
        if (!stat_dark(stats + 3 * i, n)) { best = i; break; }
    return wave_min(best);
}

// scan.c:999-1017 (and :1018-1034 on the mirrored half)
__device__ __forceinline__ int walk_rows(const int *stats, int width, int h4, int border, int lane)
{
    int t = first_not_dark(stats, width, border, h4, lane);
    if (t <= border)
    {
        t = first_not_dark(stats, width, 0, border, lane);
        if (t >= border) t = 0;
    }
    return t;
}

__global__ __launch_bounds__(64) void scan_row_decide_kernel(const int *__restrict__ rows, int width, int h4, int border,
                                                             ScanRecord *__restrict__ rec)
{
    const int lane = threadIdx.x;
    const int top = walk_rows(rows, width, h4, border, lane);
    const int bottom = walk_rows(rows + 3 * h4, width, h4, border, lane);
    if (lane == 0) { rec->top = top; rec->bottom = bottom; }
}

// grid.x: 2 sides x gx groups of 16 dwords; grid.y: bands of kColBandRows rows from `top` on
__global__ __launch_bounds__(256) void scan_col_stats_kernel(const uint8_t *__restrict__ luma, int pitch, int width, int height,
                                                             int w4, int gx, const ScanRecord *__restrict__ rec,
                                                             int *__restrict__ cols)
{
    __shared__ int s_sum[64], s_mn[64], s_mx[64];
    const int r_end = height - rec->bottom;                       // rows [top, r_end)
    const int band = rec->top + blockIdx.y * kColBandRows;
    if (band >= r_end) return;                                    // (the whole workgroup: nothing below has started)
    const int side = blockIdx.x >= gx, group = blockIdx.x - side * gx;
    const int c0 = side ? width - w4 : 0, c1 = side ? width : w4;   // the side's columns [c0, c1)
    const int dx = threadIdx.x & 15, ry = threadIdx.x >> 4;
    const int d = (c0 >> 2) + group * 16 + dx;                    // this thread's dword of a row
    if (threadIdx.x < 64) { s_sum[threadIdx.x] = 0; s_mn[threadIdx.x] = 255; s_mx[threadIdx.x] = 0; }
    __syncthreads();
    if (4 * d < c1)
    {
        int sum[4] = {0, 0, 0, 0}, mn[4] = {255, 255, 255, 255}, mx[4] = {0, 0, 0, 0};
        const int last = min(band + kColBandRows, r_end);
#pragma unroll 8
        for (int r = band + ry; r < last; r += 16)
        {
            const unsigned q = *reinterpret_cast<const unsigned *>(luma + (size_t)r * pitch + 4 * d);
#pragma unroll
            for (int b = 0; b < 4; b++)
            {
                const int c = max((int)((q >> (8 * b)) & 0xff), 16);
                sum[b] += c; mn[b] = min(mn[b], c); mx[b] = max(mx[b], c);
            }
        }
        if (band + ry < last)
#pragma unroll
            for (int b = 0; b < 4; b++)
            {
                atomicAdd(&s_sum[4 * dx + b], sum[b]);
                atomicMin(&s_mn[4 * dx + b], mn[b]);
                atomicMax(&s_mx[4 * dx + b], mx[b]);
            }
    }
    __syncthreads();
    if (threadIdx.x < 64)
    {
        const int x = 4 * ((c0 >> 2) + group * 16) + threadIdx.x;  // the column behind this LDS entry
        if (x >= c0 && x < c1)
        {
            int *c = cols + 3 * (side ? w4 + (width - 1 - x) : x);
            atomicAdd(c, s_sum[threadIdx.x]);
            atomicMin(c + 1, s_mn[threadIdx.x]);
            atomicMax(c + 2, s_mx[threadIdx.x]);
        }
    }
}

// scan.c:1035-1052
__global__ __launch_bounds__(64) void scan_col_decide_kernel(const int *__restrict__ cols, int height, int h4, int w4,
                                                             ScanRecord *__restrict__ rec)
{
    const int lane = threadIdx.x;
    const int top = rec->top, bottom = rec->bottom;
    const int n = height - top - bottom;
    const int left = first_not_dark(cols, n, 0, w4, lane);
    const int right = first_not_dark(cols + 3 * w4, n, 0, w4, lane);
    if (lane == 0)
    {
        rec->left = left; rec->right = right;
        rec->recorded = top < h4 && bottom < h4 && left < w4 && right < w4;
        rec->pad = 0;
    }
}

struct CombArgs
{
    const uint8_t *plane[3];
    int pitch[3], w[3], h[3];
    int equal, diff;
};

// block (64, 4): a wave = 64 dword columns of one strip of kCombPairs row pairs; grid.z = plane, grid sized for luma
__global__ __launch_bounds__(256) void scan_comb_kernel(CombArgs a, ScanRecord *__restrict__ rec)
{
    const int k = blockIdx.z;
    const int w = a.w[k], h = a.h[k], pitch = a.pitch[k];
    const int d = blockIdx.x * 64 + threadIdx.x;
    const int npairs = h > 4 ? (h - 3) >> 1 : 0;                   // n = 0, 2, .. < h - 4
    const int p0 = (blockIdx.y * 4 + threadIdx.y) * kCombPairs;
    int c1 = 0, c2 = 0;
    if (4 * d < w && p0 < npairs)
    {
        const int p1 = min(p0 + kCombPairs, npairs);
        const int valid = w - 4 * d;                              // columns of this dword that are the plane's
        const uint8_t *col = a.plane[k] + (size_t)(2 * p0) * pitch + 4 * d;
        unsigned r0 = *reinterpret_cast<const unsigned *>(col);
        unsigned r1 = *reinterpret_cast<const unsigned *>(col + pitch);
        for (int p = p0; p < p1; p++)
        {
            col += 2 * (size_t)pitch;
            const unsigned r2 = *reinterpret_cast<const unsigned *>(col);
            const unsigned r3 = *reinterpret_cast<const unsigned *>(col + pitch);
#pragma unroll
            for (int b = 0; b < 4; b++)
            {
                const int s1 = (r0 >> (8 * b)) & 0xff, s2 = (r1 >> (8 * b)) & 0xff;
                const int s3 = (r2 >> (8 * b)) & 0xff, s4 = (r3 >> (8 * b)) & 0xff;
                const bool in = b < valid;
                c1 += in && abs(s1 - s3) < a.equal && abs(s1 - s2) > a.diff;
                c2 += in && abs(s2 - s4) < a.equal && abs(s2 - s3) > a.diff;
            }
            r0 = r2; r1 = r3;
        }
    }
    c1 = wave_sum(c1); c2 = wave_sum(c2);
    if (threadIdx.x == 0 && (c1 | c2))
        atomicAdd(&rec->cc[k], (unsigned long long)(unsigned)c1 | ((unsigned long long)(unsigned)c2 << 32));
}

struct Slot
{
    DevBuf<uint8_t> d_base;                      // record, row statistics, column statistics: one allocation
    ScanRecord  *d_rec = nullptr, *h_rec = nullptr;
    int         *d_rows = nullptr, *d_cols = nullptr;
    hipEvent_t   done = nullptr;
    hbhip_frame *frame = nullptr;
    int          threshold = 0;
};

} // namespace

struct hbhip_scan
{
    hbhip_ctx *ctx = nullptr;
    int width = 0, height = 0;
    PinnedBuf<ScanRecord> h_recs;                // one per slot
    std::vector<Slot *> slots, idle;
    std::deque<Slot *> inflight;

    ~hbhip_scan()
    {
        for (Slot *s : slots)
        {
            if (s->frame) hbhip_frame_release(s->frame);
            if (s->done) (void)hipEventDestroy(s->done);
            delete s;
        }
    }

    Slot *take_slot()
    {
        if (!idle.empty()) { Slot *s = idle.back(); idle.pop_back(); return s; }
        if ((int)slots.size() >= HBHIP_SCAN_INFLIGHT_MAX) return nullptr;
        Slot *s = new (std::nothrow) Slot;
        if (!s) return nullptr;
        const size_t rows_at = 64, cols_at = rows_at + sizeof(int) * 3 * 2 * (height / 4);
        const size_t bytes = cols_at + sizeof(int) * 3 * 2 * (width / 4);
        if (s->d_base.alloc(ctx, bytes) != HBHIP_OK ||
            hipEventCreateWithFlags(&s->done, hipEventDisableTiming) != hipSuccess)
        {
            (void)hipGetLastError();
            delete s;
            return nullptr;
        }
        s->d_rec = reinterpret_cast<ScanRecord *>(s->d_base.get());
        s->d_rows = reinterpret_cast<int *>(s->d_base.get() + rows_at);
        s->d_cols = reinterpret_cast<int *>(s->d_base.get() + cols_at);
        s->h_rec = h_recs.get() + slots.size();
        slots.push_back(s);
        return s;
    }
};

// what push refuses for the size alone (create asks the same of its own)
static int scan_size_check(int width, int height)
{
    if ((width | height) & 1) return HBHIP_ERR_UNSUPPORTED;
    if (width < 8 || height < 8 || width > 16384 || height > 16384) return HBHIP_ERR_UNSUPPORTED;
    return HBHIP_OK;
}

extern "C" int hbhip_scan_create(hbhip_ctx *ctx, int width, int height, hbhip_scan **out)
{
    if (!ctx || !out) return HBHIP_ERR_ARG;
    *out = nullptr;
    const int rc = scan_size_check(width, height);
    if (rc != HBHIP_OK) return rc;
    (void)hipSetDevice(ctx->device);
    hbhip_scan *s = new (std::nothrow) hbhip_scan;
    if (!s) return HBHIP_ERR_NOMEM;
    s->ctx = ctx; s->width = width; s->height = height;
    if (const int ra = s->h_recs.alloc(ctx, HBHIP_SCAN_INFLIGHT_MAX))
    {
        delete s;
        return ra;
    }
    *out = s;
    return HBHIP_OK;
}

extern "C" void hbhip_scan_destroy(hbhip_scan *s)
{
    if (!s) return;
    (void)hipSetDevice(s->ctx->device);
    (void)hipStreamSynchronize(s->ctx->stream);
    delete s;
}

extern "C" int hbhip_scan_inflight(hbhip_scan *s)
{
    return s ? (int)s->inflight.size() : 0;
}

// the five launches and the record's copy for the picture in `sl`
static int scan_queue(hbhip_scan *s, Slot *sl, const hbhip_frame *fr, int equal, int diff)
{
    hbhip_ctx *ctx = s->ctx;
    const DevPicture &pic = fr->pic;
    const int width = s->width, height = s->height;
    const int h4 = height / 4, w4 = width / 4, border = height / 100;
    HBHIP_LAUNCH(ctx, "scan_row_stats", scan_row_stats_kernel, dim3((2 * h4 + 3) / 4), dim3(256), 0,
                 (const uint8_t *)pic.plane[0], pic.pitch[0], width, height, h4, w4, sl->d_rows, sl->d_cols, sl->d_rec);
    HBHIP_LAUNCH(ctx, "scan_row_decide", scan_row_decide_kernel, dim3(1), dim3(64), 0,
                 (const int *)sl->d_rows, width, h4, border, sl->d_rec);
    // a side's columns lie in at most w4 / 4 + 2 dwords of a row (the right-hand side may start inside one)
    const int gx = (w4 / 4 + 2 + 15) / 16;
    HBHIP_LAUNCH(ctx, "scan_col_stats", scan_col_stats_kernel, dim3(2 * gx, (height + kColBandRows - 1) / kColBandRows), dim3(256), 0,
                 (const uint8_t *)pic.plane[0], pic.pitch[0], width, height, w4, gx, (const ScanRecord *)sl->d_rec, sl->d_cols);
    HBHIP_LAUNCH(ctx, "scan_col_decide", scan_col_decide_kernel, dim3(1), dim3(64), 0,
                 (const int *)sl->d_cols, height, h4, w4, sl->d_rec);
    CombArgs a;
    for (int c = 0; c < 3; c++)
    {
        a.plane[c] = pic.plane[c]; a.pitch[c] = pic.pitch[c]; a.w[c] = pic.width[c]; a.h[c] = pic.height[c];
    }
    a.equal = equal; a.diff = diff;
    const int npairs = (height - 3) >> 1;
    HBHIP_LAUNCH(ctx, "scan_comb", scan_comb_kernel, dim3(((width + 3) / 4 + 63) / 64, (npairs + 4 * kCombPairs - 1) / (4 * kCombPairs), 3),
                 dim3(64, 4), 0, a, sl->d_rec);
    HBHIP_CHECK(ctx, hipGetLastError());
    HBHIP_CHECK(ctx, hipMemcpyAsync(sl->h_rec, sl->d_rec, sizeof(ScanRecord), hipMemcpyDeviceToHost, ctx->stream));
    HBHIP_CHECK(ctx, hipEventRecord(sl->done, ctx->stream));
    ctx->bus_d2h += sizeof(ScanRecord);
    return HBHIP_OK;
}

extern "C" int hbhip_scan_push(hbhip_scan *s, hbhip_frame *fr, int pic_flags, const hbhip_scan_params *p)
{
    if (!s || !fr) return HBHIP_ERR_ARG;
    if (fr->depth != 8 || fr->lcw != 1 || fr->lch != 1) return HBHIP_ERR_UNSUPPORTED;
    const int size_rc = scan_size_check(fr->width, fr->height);
    if (size_rc != HBHIP_OK) return size_rc;
    if (fr->width != s->width || fr->height != s->height) return HBHIP_ERR_UNSUPPORTED;
    hbhip_ctx *ctx = s->ctx;
    if (fr->ctx->device != ctx->device) return HBHIP_ERR_ARG;
    for (int c = 0; c < 3; c++)                                   // (what hbhip_frame_alloc gives: the kernels load dwords and uint4)
        if (((uintptr_t)fr->pic.plane[c] & 15) || (fr->pic.pitch[c] & 15) || fr->pic.pitch[c] < hbhip_align_up(fr->pic.width[c], 16))
            return HBHIP_ERR_ARG;
    if ((int)s->inflight.size() >= HBHIP_SCAN_INFLIGHT_MAX) return HBHIP_ERR_STATE;
    static const hbhip_scan_params scan_c = {10, 30, 9, 10, 30, 9};                // scan.c:973
    if (!p) p = &scan_c;
    const bool prog = (pic_flags & 16) != 0;                                       // hb.c:1095-1101
    (void)hipSetDevice(ctx->device);
    Slot *sl = s->take_slot();
    if (!sl) return HBHIP_ERR_NOMEM;
    int rc = hbhip_frame_use_on(fr, ctx);
    if (rc == HBHIP_OK)
    {
        hbhip_frame_retain(fr);
        rc = scan_queue(s, sl, fr, prog ? p->prog_equal : p->color_equal, prog ? p->prog_diff : p->color_diff);
        if (rc != HBHIP_OK)
        {
            (void)hipStreamSynchronize(ctx->stream);              // whatever was queued reads the frame and the slot
            hbhip_frame_release(fr);
        }
    }
    if (rc != HBHIP_OK)
    {
        s->idle.push_back(sl);
        return rc;
    }
    sl->frame = fr;
    sl->threshold = prog ? p->prog_threshold : p->threshold;
    s->inflight.push_back(sl);
    return HBHIP_OK;
}

extern "C" int hbhip_scan_pull(hbhip_scan *s, hbhip_scan_result *out)
{
    if (!s || !out) return HBHIP_ERR_ARG;
    if (s->inflight.empty()) return HBHIP_AGAIN;
    hbhip_ctx *ctx = s->ctx;
    (void)hipSetDevice(ctx->device);
    Slot *sl = s->inflight.front();
    const hipError_t e = hipEventSynchronize(sl->done);
    s->inflight.pop_front();
    hbhip_frame_release(sl->frame);
    sl->frame = nullptr;
    s->idle.push_back(sl);
    if (e != hipSuccess) return ctx->fail(e, "scan: wait for the picture's record");
    const ScanRecord &r = *sl->h_rec;
    out->top = r.top; out->bottom = r.bottom; out->left = r.left; out->right = r.right;
    out->recorded = r.recorded;
    // hb.c:1104-1145: cc_1 / cc_2 run on from plane to plane
    PicGeometry g;
    g.set(s->width, s->height, 8, 1, 1);
    int cc_1 = 0, cc_2 = 0;
    for (int k = 0; k < 3; k++)
    {
        cc_1 += (int)(unsigned)(r.cc[k] & 0xffffffffu);
        cc_2 += (int)(unsigned)(r.cc[k] >> 32);
        out->cc[k] = (int)((cc_1 + cc_2) * 1000.0 / (g.pw[k] * g.ph[k]));
    }
    out->average_cc = (2 * out->cc[0] + (out->cc[1] / 2) + (out->cc[2] / 2)) / 3;   // :1149
    out->combed = out->average_cc > sl->threshold;
    return HBHIP_OK;
}
