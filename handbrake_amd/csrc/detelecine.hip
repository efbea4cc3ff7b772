// detelecine.hip — libhb's detelecine filter ("pullup", libhb/detelecine.c; the object hb_filter_detelecine) on gfx950.
//
// Pullup undoes 3:2 pulldown: every input picture is split into its fields, the fields go through a circular queue, and
// an output frame is woven from the first one to three fields of the queue once the metrics around them say where the
// film frames begin.  Two halves:
//
//  * Per pixel (the kernels below): for each field that enters the queue, three `int` arrays over the 8 x 8 blocks of
//    the metric plane inside the skip margins (detelecine.c:159-218, 230-265, 956-986) - `diffs` (sum of |a - b|
//    against the same-parity field two places back), `comb` (the two-sided line comb between the field and the one
//    before it) and `var` (4 x the sum of |a - a one field line down| over three field lines) - in ONE launch per
//    field; the max-reductions pullup_compute_breaks / pullup_compute_affinity take over them (:345-434) for every
//    field the decision asks about, in ONE launch per frame decision, and a few ints come back; the weave of the
//    output frame.  Field lines are two picture rows apart at every depth: the reference's 16-bit path keeps its field
//    stride in bytes and steps a uint16_t pointer by it (:242, :1050), which is the same two rows.
//  * The state machine (DetelecineFilter): the field queue, locks on the held pictures, breaks, affinity, the frame
//    length decision, the first picture passed through and the dropping of one-field frames, written as a restatement
//    of the reference's behaviour with the same order of queue operations.
//
// The metric arrays live in a device ring of slots that mirrors the reference's circular field queue slot for slot,
// including its growth (pullup_check_field_queue, :285-296): a slot keeps its arrays between uses, which is observable -
// a neighbour field with no picture leaves an array as it was (stale), a field compared with itself writes zeros
// (:245-252).  The host decides which case applies and tells the launch.
//
// The reductions are evaluated lazily, exactly for the set pullup_foo asks for (:436-446): one pass over the queue
// applies what needs no pixels (the flags, the shortcuts for fields of one picture) and collects the rest; one launch
// computes those maxima, one small read-back brings them home, and the results are applied in the queue's order.  That
// equals the reference's interleaved order: a deferred result only sets the `breaks` bits of the next two fields (ORs,
// which commute) or the `affinity` of its own field, and nothing in the pass reads either; a shortcut later in the
// pass writes the affinity of later fields only, and a field whose affinity a shortcut has set is never deferred.
//
// Output frames are always fresh pictures of the filter's pool, or - when both fields come from one input picture,
// and for the pass-through of the first input - that input picture itself, retained, without a copy.  The reference
// weaves in place into a held picture when it can (pullup_pack_frame, :910-935); a picture that has been handed on is
// shared and is not written here.  Every value is an exact integer, so the result is bit-exact by construction.
#include "hbhip_internal.h"

#include <vector>

namespace {

constexpr int DT_HELD_MAX = 10;          // pullup_init_context: nbuffers at least 10 (:604-607)
constexpr int DT_REQ_MAX = 64;           // reductions per launch (a decision asks for at most 2 per queued field)
constexpr int DT_BREAK_LEFT = 1, DT_BREAK_RIGHT = 2;
constexpr int DT_HAVE_BREAKS = 1, DT_HAVE_AFFINITY = 2;
constexpr int PIC_TFF = 0x0008, PIC_RFF = 0x0100;

// ---- block metrics ------------------------------------------------------------------------------------------------
// |a - b| summed over 8 samples: v_sad_u8 / v_sad_u16 on the packed samples
__device__ __forceinline__ unsigned sad8(const uint8_t *a, const uint8_t *b)
{
    const uint2 x = *reinterpret_cast<const uint2 *>(a), y = *reinterpret_cast<const uint2 *>(b);
    return __builtin_amdgcn_sad_u8(x.y, y.y, __builtin_amdgcn_sad_u8(x.x, y.x, 0u));
}
__device__ __forceinline__ unsigned sad8(const uint16_t *a, const uint16_t *b)
{
    const uint4 x = *reinterpret_cast<const uint4 *>(a), y = *reinterpret_cast<const uint4 *>(b);
    unsigned s = __builtin_amdgcn_sad_u16(x.x, y.x, 0u);
    s = __builtin_amdgcn_sad_u16(x.y, y.y, s);
    s = __builtin_amdgcn_sad_u16(x.z, y.z, s);
    return __builtin_amdgcn_sad_u16(x.w, y.w, s);
}

template <typename T> __device__ __forceinline__ void load8(const T *p, int v[8])
{
#pragma unroll
    for (int j = 0; j < 8; j++) v[j] = p[j];
}

struct MetricArgs
{
    const uint8_t *cur;      // the field's picture (metric plane)
    const uint8_t *older;    // the picture of the field two places back (diffs)
    const uint8_t *top;      // the pictures whose rows 0 / 1 the comb reads
    const uint8_t *bottom;
    int pitch;               // bytes
    int parity;
    int diff_mode;           // 0: leave the array as it is, 1: zeros, 2: compute
    int comb_mode;           // 0 / 2 as above
    int row0, col0;          // first row / first sample of the metric area (2 * junk_top, 8 * junk_left)
    int mw, mh;
    int *diffs, *comb, *var;
};

// One thread per 8 x 8 block: 4 field lines of 8 samples for diffs and comb, 3 + 1 for var.
template <typename T>
__global__ __launch_bounds__(256) void dt_metrics_kernel(MetricArgs a)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= a.mw * a.mh) return;
    const int by = i / a.mw, bx = i - by * a.mw;
    const int pe = a.pitch / (int)sizeof(T);                  // elements per row
    const int s = 2 * pe;                                     // one field line
    const size_t at = (size_t)(a.row0 + 8 * by) * pe + a.col0 + 8 * bx;
    const T *cur = reinterpret_cast<const T *>(a.cur) + at + (size_t)a.parity * pe;

    unsigned var = 0;
#pragma unroll
    for (int k = 0; k < 3; k++) var = var + sad8(cur + k * s, cur + (k + 1) * s);
    a.var[i] = (int)(4 * var);

    if (a.diff_mode == 1) a.diffs[i] = 0;
    else if (a.diff_mode == 2)
    {
        const T *old = reinterpret_cast<const T *>(a.older) + at + (size_t)a.parity * pe;
        unsigned d = 0;
#pragma unroll
        for (int k = 0; k < 4; k++) d = d + sad8(cur + k * s, old + k * s);
        a.diffs[i] = (int)d;
    }

    if (a.comb_mode == 2)
    {
        const T *t = reinterpret_cast<const T *>(a.top) + at;
        const T *b = reinterpret_cast<const T *>(a.bottom) + at + pe;
        int c = 0;
        int bu[8], tv[8], bv[8], tn[8];
        load8(b - s, bu);
#pragma unroll
        for (int k = 0; k < 4; k++)
        {
            load8(t + k * s, tv);
            load8(b + k * s, bv);
            load8(t + (k + 1) * s, tn);
#pragma unroll
            for (int j = 0; j < 8; j++)
                c += abs(2 * tv[j] - bu[j] - bv[j]) + abs(2 * bv[j] - tv[j] - tn[j]);
#pragma unroll
            for (int j = 0; j < 8; j++) bu[j] = bv[j];
        }
        a.comb[i] = c;
    }
}

// ---- the maxima -----------------------------------------------------------------------------------------------------
struct ReduceArgs
{
    const int *slots;        // slot k's arrays: diffs at slots + k * 3 * len, comb + len, var + 2 * len
    int len;
    int n;
    int kind[DT_REQ_MAX];    // 0: breaks (f2 = s0, f3 = s1), 1: affinity (prev = s0, f = s1, next = s2)
    int s0[DT_REQ_MAX], s1[DT_REQ_MAX], s2[DT_REQ_MAX];
    int *out;                // 2 per request: max(0, max l), max(0, max -l); zeroed before the launch
};

__device__ __forceinline__ int wave_max(int v)
{
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v = max(v, __shfl_xor(v, off, 64));
    return v;
}

// grid.y = request, grid.x = stretches of the arrays; a wave then LDS reduction, one atomicMax per block and value
__global__ __launch_bounds__(256) void dt_reduce_kernel(ReduceArgs a)
{
    __shared__ int s_hi[4], s_lo[4];
    const int r = blockIdx.y;
    const size_t per = (size_t)3 * a.len;
    int hi = 0, lo = 0;
    if (a.kind[r] == 0)
    {
        const int *d2 = a.slots + a.s0[r] * per, *d3 = a.slots + a.s1[r] * per;
        for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < a.len; i += gridDim.x * blockDim.x)
        {
            const int l = d2[i] - d3[i];
            hi = max(hi, l);
            lo = max(lo, -l);
        }
    }
    else
    {
        const int *p = a.slots + a.s0[r] * per, *f = a.slots + a.s1[r] * per, *n = a.slots + a.s2[r] * per;
        const int L = a.len;
        for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < L; i += gridDim.x * blockDim.x)
        {
            const int v = f[2 * L + i], lv = p[2 * L + i], rv = n[2 * L + i];
            const int lc = max(f[L + i] - (v + lv) + abs(v - lv), 0);
            const int rc = max(n[L + i] - (v + rv) + abs(v - rv), 0);
            const int l = lc - rc;
            hi = max(hi, l);
            lo = max(lo, -l);
        }
    }
    hi = wave_max(hi);
    lo = wave_max(lo);
    if ((threadIdx.x & 63) == 0) { s_hi[threadIdx.x >> 6] = hi; s_lo[threadIdx.x >> 6] = lo; }
    __syncthreads();
    if (threadIdx.x == 0)
    {
        hi = max(max(s_hi[0], s_hi[1]), max(s_hi[2], s_hi[3]));
        lo = max(max(s_lo[0], s_lo[1]), max(s_lo[2], s_lo[3]));
        if (hi > 0) atomicMax(&a.out[2 * r], hi);
        if (lo > 0) atomicMax(&a.out[2 * r + 1], lo);
    }
}

// ---- the weave --------------------------------------------------------------------------------------------------------
struct WeaveArgs
{
    const uint8_t *src[2][3];     // [row parity][plane]
    int src_pitch[2][3];
    uint8_t *dst[3];
    int dst_pitch[3];
    int row_bytes[3];             // rounded up to 16 (within every pitch: pitches are multiples of 64)
    int rows[3];
};

// 16 bytes per thread; grid.z = plane
__global__ __launch_bounds__(256) void dt_weave_kernel(WeaveArgs a)
{
    const int c = blockIdx.z;
    const int x = (blockIdx.x * blockDim.x + threadIdx.x) * 16;
    const int y = blockIdx.y;
    if (y >= a.rows[c] || x >= a.row_bytes[c]) return;
    const int p = y & 1;
    const uint4 v = *reinterpret_cast<const uint4 *>(a.src[p][c] + (size_t)y * a.src_pitch[p][c] + x);
    *reinterpret_cast<uint4 *>(a.dst[c] + (size_t)y * a.dst_pitch[c] + x) = v;
}

// ---- the state machine ------------------------------------------------------------------------------------------------
struct HeldPic                   // an input picture while any of its fields is queued or in the frame being made
{
    DevPicture *pic = nullptr;
    int lock[2] = {0, 0};
};

struct FieldSlot                 // a place of the circular field queue; `slot` names its metric arrays in HBM
{
    int parity = 0;
    HeldPic *buf = nullptr;
    unsigned flags = 0;
    int breaks = 0, affinity = 0;
    int slot = 0;
    FieldSlot *prev = nullptr, *next = nullptr;
};

struct FrameChoice
{
    int length = 0, parity = 0;
    HeldPic *taken[3] = {nullptr, nullptr, nullptr};
    HeldPic *out[2] = {nullptr, nullptr};
    bool whole = false;          // both output fields from one picture
};

} // namespace

struct DetelecineFilter : hbhip_filter
{
    hbhip_detelecine_params par{};
    int depth = 8;
    int half = 128, quarter = 64;
    int mw = 0, mh = 0, len = 0;
    PicturePool in_pool, out_pool;
    std::deque<DevPicture *> outq;
    std::vector<std::unique_ptr<FieldSlot>> nodes;
    std::vector<HeldPic *> held;
    FieldSlot *head = nullptr, *first = nullptr, *last = nullptr;
    bool frame_busy = false;
    int passthrough_left = 1;
    int next_flags = 0;
    DevBuf<int> d_slots;         // capacity * 3 * len ints
    int capacity = 0;
    DevBuf<int> d_out;           // 2 * DT_REQ_MAX
    PinnedBuf<int> h_out;
    hipEvent_t ev_out = nullptr;

    explicit DetelecineFilter(hbhip_ctx *c) : hbhip_filter(c) {}
    ~DetelecineFilter() override
    {
        (void)hipSetDevice(ctx->device);
        (void)hipStreamSynchronize(ctx->stream);
        for (DevPicture *p : outq) hbhip_pic_release(p, ctx);
        for (HeldPic *h : held) { hbhip_pic_release(h->pic, ctx); delete h; }
        if (ev_out) (void)hipEventDestroy(ev_out);
    }                                    // (the buffers go with their members, behind the wait above)

    int init()
    {
        if (const int rc = d_out.alloc(ctx, 2 * DT_REQ_MAX)) return rc;
        if (const int rc = h_out.alloc(ctx, 2 * DT_REQ_MAX)) return rc;
        HBHIP_CHECK(ctx, hipEventCreateWithFlags(&ev_out, hipEventDisableTiming));
        // the queue starts as nine places in a ring (pullup_make_field_queue(c, 8))
        for (int k = 0; k < 9; k++) { int rc = add_node(); if (rc != HBHIP_OK) return rc; }
        for (int k = 0; k < 9; k++)
        {
            nodes[k]->next = nodes[(k + 1) % 9].get();
            nodes[(k + 1) % 9]->prev = nodes[k].get();
        }
        head = nodes[0].get();
        return HBHIP_OK;
    }

    // a new place and its arrays, zeroed as calloc'd arrays are; the ring of slots grows by doubling, contents kept
    int add_node()
    {
        const int k = (int)nodes.size();
        if (len > 0 && k >= capacity)
        {
            const int cap = capacity ? 2 * capacity : 16;
            DevBuf<int> d;                                  // (a failure below frees it on the way out)
            const size_t per = (size_t)3 * len;
            if (const int rc = d.alloc(ctx, cap * per)) return rc;
            HBHIP_CHECK(ctx, hipMemsetAsync(d.get(), 0, cap * per * sizeof(int), ctx->stream));
            if (d_slots.get())
            {
                HBHIP_CHECK(ctx, hipMemcpyAsync(d.get(), d_slots.get(), capacity * per * sizeof(int), hipMemcpyDeviceToDevice, ctx->stream));
                HBHIP_CHECK(ctx, hipStreamSynchronize(ctx->stream));
            }
            d_slots = std::move(d);
            capacity = cap;
        }
        auto n = std::make_unique<FieldSlot>();
        n->slot = k;
        nodes.push_back(std::move(n));
        return HBHIP_OK;
    }
    int *slot_arrays(int k) const { return d_slots.get() + (size_t)k * 3 * len; }

    // ---- pictures and locks ----
    static void lock_pic(HeldPic *h, int parity)
    {
        if (!h) return;
        if (parity != 1) h->lock[0]++;
        if (parity != 0) h->lock[1]++;
    }
    static void unlock_pic(HeldPic *h, int parity)
    {
        if (!h) return;
        if (parity != 1) h->lock[0]--;
        if (parity != 0) h->lock[1]--;
    }
    void drop_free()                    // pictures with no field left go back to whoever made them
    {
        for (size_t i = 0; i < held.size();)
        {
            HeldPic *h = held[i];
            if (h->lock[0] > 0 || h->lock[1] > 0) { i++; continue; }
            hbhip_pic_release(h->pic, ctx);
            delete h;
            held.erase(held.begin() + (ptrdiff_t)i);
        }
    }
    int use(DevPicture *p)              // this context is about to read `p` (device-frame ordering rule)
    {
        return p->frame ? hbhip_frame_use_on(p->frame, ctx) : HBHIP_OK;
    }

    // ---- the field queue ----
    int measure(FieldSlot *f)
    {
        if (len == 0) return HBHIP_OK;
        const int mp = par.plane;
        FieldSlot *older = f->prev->prev, *before = f->prev;
        MetricArgs a{};
        a.cur = f->buf->pic->plane[mp];
        a.pitch = f->buf->pic->pitch[mp];
        a.parity = f->parity;
        a.diff_mode = !older->buf ? 0 : (older->buf == f->buf && older->parity == f->parity) ? 1 : 2;
        a.older = older->buf ? older->buf->pic->plane[mp] : a.cur;
        a.comb_mode = before->buf ? 2 : 0;
        FieldSlot *t = f->parity ? before : f, *b = f->parity ? f : before;
        a.top = a.comb_mode ? t->buf->pic->plane[mp] : a.cur;
        a.bottom = a.comb_mode ? b->buf->pic->plane[mp] : a.cur;
        if (a.diff_mode == 2 && older->buf->pic->pitch[mp] != a.pitch) return HBHIP_ERR_STATE;
        if (a.comb_mode == 2 && (t->buf->pic->pitch[mp] != a.pitch || b->buf->pic->pitch[mp] != a.pitch)) return HBHIP_ERR_STATE;
        a.row0 = 2 * par.skip_top;
        a.col0 = 8 * par.skip_left;
        a.mw = mw; a.mh = mh;
        int *arr = slot_arrays(f->slot);
        a.diffs = arr; a.comb = arr + len; a.var = arr + 2 * len;
        int rc = use(f->buf->pic);
        if (rc == HBHIP_OK && a.diff_mode == 2) rc = use(older->buf->pic);
        if (rc == HBHIP_OK && a.comb_mode == 2) rc = use(before->buf->pic);
        if (rc != HBHIP_OK) return rc;
        const dim3 grid((unsigned)((len + 255) / 256));
        if (depth > 8) HBHIP_LAUNCH(ctx, "dt_metrics_16", dt_metrics_kernel<uint16_t>, grid, dim3(256), 0, a);
        else           HBHIP_LAUNCH(ctx, "dt_metrics_8", dt_metrics_kernel<uint8_t>, grid, dim3(256), 0, a);
        HBHIP_CHECK(ctx, hipGetLastError());
        return HBHIP_OK;
    }

    int queue_length() const
    {
        if (!first || !last) return 0;
        int n = 1;
        for (const FieldSlot *f = first; f != last; f = f->next) n++;
        return n;
    }

    int submit_field(HeldPic *h, int parity)
    {
        if (head->next == first)                        // full: one more place between head and first
        {
            int rc = add_node();
            if (rc != HBHIP_OK) return rc;
            FieldSlot *n = nodes.back().get();
            n->prev = head;
            n->next = first;
            head->next = n;
            first->prev = n;
        }
        if (last && last->parity == parity) return HBHIP_OK;   // two fields of one parity in a row: the new one goes
        FieldSlot *f = head;
        f->parity = parity;
        f->buf = h;
        lock_pic(h, parity);
        f->flags = 0;
        f->breaks = 0;
        f->affinity = 0;
        int rc = measure(f);
        if (rc != HBHIP_OK) return rc;
        if (!first) first = head;
        last = head;
        head = head->next;
        return HBHIP_OK;
    }

    // ---- breaks, affinity, frame length ----
    struct Deferred { int kind; FieldSlot *f; };

    int reduce(const std::vector<Deferred> &todo, std::vector<int> &res)
    {
        res.assign(2 * todo.size(), 0);
        if (len == 0 || todo.empty()) return HBHIP_OK;
        for (size_t base = 0; base < todo.size(); base += DT_REQ_MAX)
        {
            const int n = (int)std::min<size_t>(DT_REQ_MAX, todo.size() - base);
            ReduceArgs a{};
            a.slots = d_slots.get(); a.len = len; a.n = n; a.out = d_out.get();
            for (int r = 0; r < n; r++)
            {
                const Deferred &d = todo[base + r];
                a.kind[r] = d.kind;
                if (d.kind == 0) { a.s0[r] = d.f->next->next->slot; a.s1[r] = d.f->next->next->next->slot; a.s2[r] = 0; }
                else             { a.s0[r] = d.f->prev->slot; a.s1[r] = d.f->slot; a.s2[r] = d.f->next->slot; }
            }
            HBHIP_CHECK(ctx, hipMemsetAsync(d_out.get(), 0, 2 * n * sizeof(int), ctx->stream));
            const unsigned gx = (unsigned)std::min(64, std::max(1, (len + 2047) / 2048));
            HBHIP_LAUNCH(ctx, "dt_reduce", dt_reduce_kernel, dim3(gx, (unsigned)n), dim3(256), 0, a);
            HBHIP_CHECK(ctx, hipGetLastError());
            HBHIP_CHECK(ctx, hipMemcpyAsync(h_out.get(), d_out.get(), 2 * n * sizeof(int), hipMemcpyDeviceToHost, ctx->stream));
            HBHIP_CHECK(ctx, hipEventRecord(ev_out, ctx->stream));
            HBHIP_CHECK(ctx, hipEventSynchronize(ev_out));
            for (int k = 0; k < 2 * n; k++) res[2 * base + k] = h_out.get()[k];
        }
        return HBHIP_OK;
    }

    // What pullup_foo works out before a decision: pixel-free parts at once, the maxima deferred (see the file header).
    int settle(int q)
    {
        std::vector<Deferred> todo;
        FieldSlot *f = first;
        for (int i = 0; i < q - 1; i++, f = f->next)
        {
            if (i < q - 3 && !(f->flags & DT_HAVE_BREAKS))
            {
                f->flags |= DT_HAVE_BREAKS;
                FieldSlot *f1 = f->next, *f2 = f1->next, *f3 = f2->next;
                const bool same02 = f->buf == f2->buf, same13 = f1->buf == f3->buf;
                if (same02 && !same13) f2->breaks |= DT_BREAK_RIGHT;
                else if (same13 && !same02) f1->breaks |= DT_BREAK_LEFT;
                else todo.push_back({0, f});
            }
            if (!(f->flags & DT_HAVE_AFFINITY))
            {
                f->flags |= DT_HAVE_AFFINITY;
                FieldSlot *f2 = f->next->next;
                if (f->buf == f2->buf)
                {
                    f->affinity = 1;
                    f->next->affinity = 0;
                    f2->affinity = -1;
                    f->next->flags |= DT_HAVE_AFFINITY;
                    f2->flags |= DT_HAVE_AFFINITY;
                }
                else todo.push_back({1, f});
            }
        }
        std::vector<int> res;
        int rc = reduce(todo, res);
        if (rc != HBHIP_OK) return rc;
        for (size_t k = 0; k < todo.size(); k++)
        {
            const int hi = res[2 * k], lo = res[2 * k + 1];
            FieldSlot *g = todo[k].f;
            if (todo[k].kind == 0)
            {
                if (hi + lo < half) continue;            // mostly quantisation noise
                if (hi > 4 * lo) g->next->breaks |= DT_BREAK_LEFT;
                if (lo > 4 * hi) g->next->next->breaks |= DT_BREAK_RIGHT;
            }
            else
            {
                if (hi + lo < quarter) continue;
                if (lo > 6 * hi) g->affinity = -1;
                else if (hi > 6 * lo) g->affinity = 1;
            }
        }
        return HBHIP_OK;
    }

    int frame_length(int *n)
    {
        *n = 0;
        const int q = queue_length();
        if (q < 4) return HBHIP_OK;
        int rc = settle(q);
        if (rc != HBHIP_OK) return rc;
        FieldSlot *f0 = first, *f1 = f0->next, *f2 = f1->next;
        if (f0->affinity == -1) { *n = 1; return HBHIP_OK; }
        int brk = 0;
        FieldSlot *g = f0;
        for (int i = 0; i < 3 && !brk; i++, g = g->next)
            if ((g->breaks & DT_BREAK_RIGHT) || (g->next->breaks & DT_BREAK_LEFT)) brk = i + 1;
        if (brk == 1 && par.strict_breaks < 0) brk = 0;
        switch (brk)
        {
            case 1:  *n = par.strict_breaks < 1 && f0->affinity == 1 && f1->affinity == -1 ? 2 : 1; break;
            case 2:  *n = f1->affinity == 1 ? 1 : 2; break;      // (the reference's strict-pairs test is never enabled)
            case 3:  *n = f2->affinity == 1 ? 2 : 3; break;
            default:
                if (f1->affinity == 1) *n = 1;
                else if (f1->affinity == -1) *n = 2;
                else if (f2->affinity == -1) *n = f0->affinity == 1 ? 3 : 1;
                else *n = 2;
        }
        return HBHIP_OK;
    }

    // pullup_get_frame: *got = false when no frame can be had
    int get_frame(FrameChoice &fr, bool *got)
    {
        *got = false;
        int n = 0;
        int rc = frame_length(&n);
        if (rc != HBHIP_OK) return rc;
        int aff = first ? first->next->affinity : 0;
        if (!n || frame_busy) return HBHIP_OK;
        frame_busy = true;
        fr = FrameChoice();
        fr.length = n;
        fr.parity = first->parity;
        for (int i = 0; i < n; i++)                 // the queue's locks pass to the frame
        {
            fr.taken[i] = first->buf;
            first->buf = nullptr;
            first = first->next;
        }
        if (n == 1) fr.out[fr.parity] = fr.taken[0];
        else if (n == 2) { fr.out[fr.parity] = fr.taken[0]; fr.out[fr.parity ^ 1] = fr.taken[1]; }
        else
        {
            if (aff == 0) aff = fr.taken[0] == fr.taken[1] ? -1 : 1;
            fr.out[fr.parity] = fr.taken[1 + aff];
            fr.out[fr.parity ^ 1] = fr.taken[1];
        }
        lock_pic(fr.out[0], 0);
        lock_pic(fr.out[1], 1);
        fr.whole = fr.out[0] == fr.out[1];
        if (fr.whole) lock_pic(fr.out[0], 2);
        *got = true;
        return HBHIP_OK;
    }

    void release_frame(FrameChoice &fr)
    {
        for (int i = 0; i < fr.length; i++) unlock_pic(fr.taken[i], fr.parity ^ (i & 1));
        unlock_pic(fr.out[0], 0);
        unlock_pic(fr.out[1], 1);
        if (fr.whole) unlock_pic(fr.out[0], 2);
        frame_busy = false;
        drop_free();
    }

    // the output picture of a frame of two or more fields (its one reference is the output's)
    int pack(const FrameChoice &fr, DevPicture **outp)
    {
        *outp = nullptr;
        if (fr.whole)
        {
            DevPicture *p = fr.out[0]->pic;
            hbhip_frame_retain(p->frame);           // handed on as it is: it stays ours too while its fields are queued
            *outp = p;
            return HBHIP_OK;
        }
        // the reference would need a pool picture here (neither output picture has its other field free) - and has
        // none when ten are held
        if (fr.out[0]->lock[1] && fr.out[1]->lock[0] && (int)held.size() >= DT_HELD_MAX) return HBHIP_ERR_STATE;
        DevPicture *o = out_pool.acquire();
        if (!o) return HBHIP_ERR_NOMEM;
        int rc = use(fr.out[0]->pic);
        if (rc == HBHIP_OK) rc = use(fr.out[1]->pic);
        if (rc != HBHIP_OK) { hbhip_pic_release(o, ctx); return rc; }
        WeaveArgs a{};
        unsigned gx = 1, gy = 1;
        for (int c = 0; c < 3; c++)
        {
            for (int p = 0; p < 2; p++)
            {
                a.src[p][c] = fr.out[p]->pic->plane[c];
                a.src_pitch[p][c] = fr.out[p]->pic->pitch[c];
            }
            a.dst[c] = o->plane[c];
            a.dst_pitch[c] = o->pitch[c];
            a.row_bytes[c] = hbhip_align_up(out_geo.pw[c] * out_geo.bps, 16);
            a.rows[c] = out_geo.ph[c];
            if (a.row_bytes[c] > std::min(std::min(a.src_pitch[0][c], a.src_pitch[1][c]), a.dst_pitch[c]))
            {
                hbhip_pic_release(o, ctx);
                return HBHIP_ERR_STATE;
            }
            gx = std::max(gx, (unsigned)((a.row_bytes[c] / 16 + 255) / 256));
            gy = std::max(gy, (unsigned)a.rows[c]);
        }
        HBHIP_LAUNCH(ctx, "dt_weave", dt_weave_kernel, dim3(gx, gy, 3), dim3(256), 0, a);
        HBHIP_CHECK(ctx, hipGetLastError());
        *outp = o;
        return HBHIP_OK;
    }

    void emit(DevPicture *p, int64_t tag)
    {
        p->tag = tag;
        outq.push_back(p);
    }

    // ---- one input picture (hb_detelecine_work, :1116-1275) ----
    int take(DevPicture *pic)
    {
        const int flags = pic->flags;
        const int64_t tag = pic->tag;
        if ((int)held.size() >= DT_HELD_MAX)            // no free picture in the reference's pool of ten
        {
            hbhip_pic_release(pic, ctx);
            return HBHIP_ERR_STATE;
        }
        HeldPic *h = new (std::nothrow) HeldPic();
        if (!h) { hbhip_pic_release(pic, ctx); return HBHIP_ERR_NOMEM; }
        h->pic = pic;
        held.push_back(h);
        lock_pic(h, 2);
        int parity = 1;                                 // bottom field first unless the picture or the settings say top
        if ((flags & PIC_TFF) || par.parity == 0) parity = 0;
        if (par.parity == 1) parity = 1;
        const bool rff = (flags & PIC_RFF) != 0;
        int rc = submit_field(h, parity);
        if (rc == HBHIP_OK) rc = submit_field(h, parity ^ 1);
        if (rc == HBHIP_OK && rff) rc = submit_field(h, parity);
        unlock_pic(h, 2);
        drop_free();
        if (rc != HBHIP_OK) return rc;

        FrameChoice fr;
        bool got = false;
        rc = get_frame(fr, &got);
        if (rc != HBHIP_OK) return rc;
        if (!got)
        {
            if (passthrough_left > 0)                   // the first input goes out as it came in
            {
                passthrough_left--;
                hbhip_frame_retain(pic->frame);
                emit(pic, tag);
            }
            return HBHIP_OK;
        }
        int tries = rff ? 3 : 2;                        // frames of one field are dropped: two more tries after RFF
        while (fr.length < 2)
        {
            release_frame(fr);
            if (--tries == 0) return HBHIP_OK;
            rc = get_frame(fr, &got);
            if (rc != HBHIP_OK) return rc;
            if (!got) return HBHIP_OK;
        }
        DevPicture *o = nullptr;
        rc = pack(fr, &o);
        release_frame(fr);
        if (rc != HBHIP_OK) return rc;
        emit(o, tag);
        return HBHIP_OK;
    }

    // ---- hbhip_filter ----
    DevPicture *acquire_input() override
    {
        DevPicture *p = in_pool.acquire();
        if (p) { p->refs = 0; p->flags = next_flags; }
        return p;
    }
    void adopt_input(DevPicture *p) override { p->refs = 0; p->flags = next_flags; }
    int submit(DevPicture *pic) override
    {
        next_flags = 0;
        if (!pic->frame) { hbhip_pic_release(pic, ctx); return HBHIP_ERR_STATE; }   // (pools are frame-backed)
        return take(pic);
    }
    int flush() override { return HBHIP_OK; }        // EOF: the reference emits nothing more (:1123-1128)
    int pending() override { return (int)outq.size(); }
    DevPicture *pop_output() override
    {
        if (outq.empty()) return nullptr;
        DevPicture *p = outq.front();
        outq.pop_front();
        return p;
    }
    void recycle_output(DevPicture *p) override { hbhip_pic_release(p, ctx); }
    int use_frames() override { frames_mode = true; return HBHIP_OK; }
};

extern "C" int hbhip_detelecine_create(hbhip_ctx *ctx, const hbhip_detelecine_params *p, int width, int height,
                                       int depth, int log2_chroma_w, int log2_chroma_h, hbhip_filter **out)
{
    if (!ctx || !p || !out || width < 1 || height < 1) return HBHIP_ERR_ARG;
    *out = nullptr;
    if ((depth != 8 && depth != 10 && depth != 12) || log2_chroma_w < 0 || log2_chroma_w > 1 ||
        log2_chroma_h < 0 || log2_chroma_h > 1)
        return HBHIP_ERR_UNSUPPORTED;
    PicGeometry g;
    g.set(width, height, depth, log2_chroma_w, log2_chroma_h);
    // a plane with an odd number of rows: the reference's weave leaves its last row as a recycled pool buffer had it
    for (int c = 0; c < 3; c++)
        if (g.ph[c] & 1) return HBHIP_ERR_UNSUPPORTED;
    hbhip_detelecine_params q = *p;
    // the safety zones (detelecine.c:1035-1039) and the metric plane's range (:1074-1077)
    q.skip_left = std::max(q.skip_left, 1);
    q.skip_right = std::max(q.skip_right, 1);
    q.skip_top = std::max(q.skip_top, 4);
    q.skip_bottom = std::max(q.skip_bottom, 4);
    if (q.plane < 0 || q.plane > 2) q.plane = 0;
    const int mw = (g.pw[q.plane] - 8 * (q.skip_left + q.skip_right)) >> 3;
    const int mh = (g.ph[q.plane] - 2 * (q.skip_top + q.skip_bottom)) >> 3;
    // margins wider than the plane: the reference walks negative block counts (no defined result)
    if (mw < 0 || mh < 0) return HBHIP_ERR_UNSUPPORTED;
    (void)hipSetDevice(ctx->device);
    DetelecineFilter *f = new (std::nothrow) DetelecineFilter(ctx);
    if (!f) return HBHIP_ERR_NOMEM;
    f->par = q;
    f->depth = depth;
    f->half = (1 << depth) / 2;
    f->quarter = (1 << depth) / 4;
    f->mw = mw; f->mh = mh; f->len = mw * mh;
    f->in_geo = f->out_geo = g;
    f->in_pool.configure(ctx, g);
    f->out_pool.configure(ctx, g);
    f->in_pool.use_frames(true);                 // every picture is a frame: outputs may be input pictures, retained
    f->out_pool.use_frames(true);
    const int rc = f->init();
    if (rc != HBHIP_OK) { delete f; return rc; }
    *out = f;
    return HBHIP_OK;
}

static int dt_flags(hbhip_filter *f, int pic_flags)
{
    DetelecineFilter *d = dynamic_cast<DetelecineFilter *>(f);
    if (!d) return HBHIP_ERR_ARG;
    d->next_flags = pic_flags;
    return HBHIP_OK;
}

extern "C" int hbhip_detelecine_push(hbhip_filter *f, const hbhip_host_frame *in, int64_t tag, int pic_flags)
{
    const int rc = dt_flags(f, pic_flags);
    return rc != HBHIP_OK ? rc : hbhip_filter_push(f, in, tag);
}

extern "C" int hbhip_detelecine_push_frame(hbhip_filter *f, hbhip_frame *fr, int64_t tag, int pic_flags)
{
    const int rc = dt_flags(f, pic_flags);
    return rc != HBHIP_OK ? rc : hbhip_filter_push_frame(f, fr, tag);
}
