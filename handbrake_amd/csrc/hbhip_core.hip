// hbhip_core.hip — context, stream, event-based per-kernel timing, device
// picture pool and the generic push/pull half of the C ABI (include/hbhip.h).
#include "hbhip_internal.h"

#include <algorithm>
#include <new>

// ---------------------------------------------------------------- ctx helpers
std::atomic<size_t> hbhip_live_bytes[2];

int hbhip_ctx::fail(hipError_t e, const char *what)
{
    std::lock_guard<std::recursive_mutex> lk(state_lock);
    last_error = std::string(what) + ": " + hipGetErrorString(e);
    (void)hipGetLastError();
    if (e == hipErrorOutOfMemory) return HBHIP_ERR_NOMEM;
    if (e == hipErrorNoDevice || e == hipErrorInvalidDevice) return HBHIP_ERR_NODEVICE;
    return HBHIP_ERR_HIP;
}

hipEvent_t hbhip_ctx::ev_get()
{
    if (!ev_pool.empty())
    {
        hipEvent_t e = ev_pool.back();
        ev_pool.pop_back();
        return e;
    }
    hipEvent_t e = nullptr;
    if (hipEventCreate(&e) != hipSuccess) return nullptr;
    return e;
}

hipEvent_t hbhip_ctx::sync_ev_get()
{
    {
        std::lock_guard<std::recursive_mutex> lk(state_lock);
        if (!sync_ev_pool.empty())
        {
            hipEvent_t e = sync_ev_pool.back();
            sync_ev_pool.pop_back();
            return e;
        }
    }
    hipEvent_t e = nullptr;
    if (hipEventCreateWithFlags(&e, hipEventDisableTiming) != hipSuccess) return nullptr;
    return e;
}

void hbhip_ctx::sync_ev_put(hipEvent_t e)
{
    if (!e) return;
    std::lock_guard<std::recursive_mutex> lk(state_lock);
    sync_ev_pool.push_back(e);
}

void IdleMark::record_now()
{
    std::lock_guard<std::mutex> lk(lock);
    if (recorded) return;
    closed.store(true, std::memory_order_release);     // whoever still sees it open attached before the record below
    (void)hipEventRecord(ev, stream);
    recorded = true;
}

std::shared_ptr<IdleMark> hbhip_ctx::mark()
{
    std::lock_guard<std::recursive_mutex> lk(state_lock);
    if (open_mark && open_mark->closed.load(std::memory_order_acquire)) open_mark.reset();   // recorded through a picture
    if (!open_mark)
    {
        std::shared_ptr<IdleMark> m = std::make_shared<IdleMark>();
        if (hipEventCreateWithFlags(&m->ev, hipEventDisableTiming) != hipSuccess)
        {
            (void)hipGetLastError();
            return nullptr;
        }
        m->stream = stream;
        open_mark = m;
        has_open_mark.store(true, std::memory_order_release);
    }
    return open_mark;
}

void hbhip_ctx::close_mark()
{
    std::shared_ptr<IdleMark> m;
    {
        std::lock_guard<std::recursive_mutex> lk(state_lock);
        m.swap(open_mark);
        has_open_mark.store(false, std::memory_order_release);
    }
    if (m) m->record_now();
}

// ctx's stream as it stands: its open mark.  No event to be had: the stream is waited out here and there is nothing to
// wait for (null).
static std::shared_ptr<IdleMark> stream_now(hbhip_ctx *ctx)
{
    std::shared_ptr<IdleMark> m = ctx->mark();
    if (!m) (void)hipStreamSynchronize(ctx->stream);
    return m;
}

static bool mark_passed(const std::shared_ptr<IdleMark> &m)
{
    if (!m) return true;
    m->record_now();
    if (hipEventQuery(m->ev) == hipSuccess) return true;
    (void)hipGetLastError();                           // hipErrorNotReady
    return false;
}

// `stream` behind the point `m` (nothing to do without one, or on m's own stream): every wait on a mark of a picture or a
// frame goes through here
static hipError_t wait_mark(hipStream_t stream, const std::shared_ptr<IdleMark> &m)
{
    if (!m || m->stream == stream) return hipSuccess;
    m->record_now();
    return hipStreamWaitEvent(stream, m->ev, 0);
}

void hbhip_pic_mark_idle(hbhip_ctx *ctx, DevPicture *p)
{
    if (ctx && p) p->idle = stream_now(ctx);
}

bool hbhip_pic_idle_done(DevPicture *p)
{
    return !p || (mark_passed(p->idle) && (!p->frame || mark_passed(p->frame->reader_idle)));
}

hipError_t hbhip_pic_wait_idle(hipStream_t stream, DevPicture *p)
{
    if (!p) return hipSuccess;
    hipError_t e = wait_mark(stream, p->idle);
    if (e == hipSuccess && p->frame) e = wait_mark(stream, p->frame->reader_idle);
    return e;
}

int hbhip_ctx::prof_name(const char *name)
{
    for (size_t i = 0; i < prof_stats.size(); i++)
        if (prof_stats[i].name == name) return (int)i;
    hbhip_prof_stat s;
    s.name = name;
    prof_stats.push_back(s);
    return (int)prof_stats.size() - 1;
}

void hbhip_ctx::prof_begin(const char *name)
{
    std::lock_guard<std::recursive_mutex> lk(state_lock);
    if (prof_pending.size() >= 8192) prof_resolve();
    hbhip_prof_pending p;
    p.name_idx = prof_name(name);
    p.ev0 = ev_get();
    p.ev1 = ev_get();
    if (p.ev0) (void)hipEventRecord(p.ev0, stream);
    prof_pending.push_back(p);
}

void hbhip_ctx::prof_end()
{
    std::lock_guard<std::recursive_mutex> lk(state_lock);
    if (prof_pending.empty()) return;
    hbhip_prof_pending &p = prof_pending.back();
    if (p.ev1) (void)hipEventRecord(p.ev1, stream);
}

void hbhip_ctx::prof_resolve()
{
    std::lock_guard<std::recursive_mutex> lk(state_lock);
    if (prof_pending.empty()) return;
    (void)hipStreamSynchronize(stream);
    for (auto &p : prof_pending)
    {
        float ms = 0.f;
        if (p.ev0 && p.ev1 && hipEventElapsedTime(&ms, p.ev0, p.ev1) == hipSuccess)
        {
            prof_stats[p.name_idx].launches++;
            prof_stats[p.name_idx].total_ms += ms;
        }
        if (p.ev0) ev_pool.push_back(p.ev0);
        if (p.ev1) ev_pool.push_back(p.ev1);
    }
    prof_pending.clear();
}

// ---------------------------------------------------------------- pool
PicturePool::~PicturePool()
{
    for (Owned *o : all_) delete o;
}

void PicturePool::configure(hbhip_ctx *ctx, const PicGeometry &g, int pitch_align, int pad_rows)
{
    ctx_ = ctx;
    geo_ = g;
    pitch_align_ = pitch_align;
    pad_rows_ = pad_rows;
}

DevPicture *PicturePool::acquire()
{
    if (frames_)
    {
        hbhip_frame *fr = nullptr;
        if (hbhip_frame_alloc(ctx_, geo_.width, geo_.height, geo_.depth, geo_.log2_cw, geo_.log2_ch, &fr) != HBHIP_OK) return nullptr;
        return &fr->pic;
    }
    if (!free_.empty())
    {
        // Most recently released first (warm in L2) when its last user ran on this pool's stream.  One last used on
        // ANOTHER stream (a later stage of a chain with a stream per stage) is only taken once that user is done:
        // waiting for it here would chain this stage's next batch behind the later stage's current one.  While there
        // is no such picture the pool grows (to a bound), after that the longest-released one is waited for.
        for (size_t i = free_.size(); i-- > 0;)
        {
            DevPicture *p = free_[i];
            if (p->idle && p->idle->stream != ctx_->stream && !hbhip_pic_idle_done(p)) continue;
            free_.erase(free_.begin() + (ptrdiff_t)i);
            return p;
        }
        if (all_.size() >= max_pictures_)
        {
            DevPicture *p = free_.front();
            free_.erase(free_.begin());
            (void)hbhip_pic_wait_idle(ctx_->stream, p);
            return p;
        }
    }
    Owned *o = new (std::nothrow) Owned();
    if (!o) return nullptr;
    DevPicture *p = &o->pic;
    size_t off[3], total = 0;
    for (int c = 0; c < 3; c++)
    {
        p->width[c] = geo_.pw[c];
        p->height[c] = geo_.ph[c];
        p->pitch[c] = hbhip_align_up(geo_.pw[c] * geo_.bps, pitch_align_);
        off[c] = total;
        total += (size_t)p->pitch[c] * (geo_.ph[c] + pad_rows_);
        total = (total + 255) & ~(size_t)255;
    }
    p->bps = geo_.bps;
    p->bytes = total;
    if (o->mem.alloc(ctx_, total) != HBHIP_OK)
    {
        delete o;
        return nullptr;
    }
    (void)hipMemsetAsync(o->mem.get(), 0, total, ctx_->stream);
    hbhip_pic_mark_idle(ctx_, p);          // an upload (on the copy stream) must not overtake the clearing
    for (int c = 0; c < 3; c++) p->plane[c] = o->mem.get() + off[c];
    p->owner = this;
    all_.push_back(o);
    return p;
}

void PicturePool::release(DevPicture *p, hbhip_ctx *last_user)
{
    if (!p) return;
    if (p->frame) { hbhip_frame_release(p->frame); return; }      // a frame's picture, whoever made it
    hbhip_pic_mark_idle(last_user ? last_user : ctx_, p);   // an upload into the recycled picture waits for this (hbhip_copy_h2d)
    free_.push_back(p);
}

// ---------------------------------------------------------------- copies
// Uploads carry the caller's row padding too (up to our pitch): a few reference
// filters read into it (lapsharp.c:145-157 when stride > width).
// The host frame and the device picture have the same strides and their planes lie one behind the other in both:
// the whole frame is one contiguous block on either side (hbhip_frame_alloc lays its frames out like hb_frame_buffer_init).
static bool same_layout(const DevPicture *p, uint8_t *const plane[3], const int stride[3])
{
    for (int c = 0; c < 3; c++)
    {
        if (stride[c] != p->pitch[c]) return false;
        if (c && plane[c] - plane[c - 1] != p->plane[c] - p->plane[c - 1]) return false;
        if (c && p->plane[c] - p->plane[c - 1] != (ptrdiff_t)p->pitch[c - 1] * p->height[c - 1]) return false;
    }
    return true;
}
static size_t layout_bytes(const DevPicture *p)
{
    return (size_t)(p->plane[2] - p->plane[0]) + (size_t)p->pitch[2] * p->height[2];
}
static bool host_planes_ok(const DevPicture *p, const hbhip_host_frame *hf)
{
    for (int c = 0; c < 3; c++)
        if (hf->plane[c] == nullptr || hf->stride[c] < p->width[c] * p->bps) return false;
    return true;
}

// The copy of a picture from / into host planes, queued on `stream`; *moved: what it sends over the bus (hbhip_ctx_bus_bytes).
// `one_block`: a host picture laid out like ours moves whole, row padding included.  The ends of a run and push say yes;
// pull and the submit pipe say no, as they always have: what their callers find in their row padding must not change.
static hipError_t queue_h2d(DevPicture *dst, const hbhip_host_frame *src, bool one_block, hipStream_t stream, size_t *moved)
{
    *moved = one_block && same_layout(dst, src->plane, src->stride) ? layout_bytes(dst) : 0;
    if (*moved) return hipMemcpyAsync(dst->plane[0], src->plane[0], *moved, hipMemcpyHostToDevice, stream);
    hipError_t e = hipSuccess;
    for (int c = 0; c < 3 && e == hipSuccess; c++)
    {
        const size_t row = (size_t)std::min(src->stride[c], dst->pitch[c]);     // the host's row padding, as far as our pitch reaches
        e = hipMemcpy2DAsync(dst->plane[c], dst->pitch[c], src->plane[c], src->stride[c], row, dst->height[c], hipMemcpyHostToDevice, stream);
        *moved += row * dst->height[c];
    }
    return e;
}

static hipError_t queue_d2h(const hbhip_host_frame *dst, const DevPicture *src, bool one_block, hipStream_t stream, size_t *moved)
{
    *moved = one_block && same_layout(src, dst->plane, dst->stride) ? layout_bytes(src) : 0;
    if (*moved) return hipMemcpyAsync(dst->plane[0], src->plane[0], *moved, hipMemcpyDeviceToHost, stream);
    hipError_t e = hipSuccess;
    for (int c = 0; c < 3 && e == hipSuccess; c++)
    {
        const size_t row = (size_t)src->width[c] * src->bps;                    // the samples only
        e = hipMemcpy2DAsync(dst->plane[c], dst->stride[c], src->plane[c], src->pitch[c], row, src->height[c], hipMemcpyDeviceToHost, stream);
        *moved += row * src->height[c];
    }
    return e;
}

static int hip_rc(hbhip_ctx *ctx, hipError_t e, const char *what) { return e == hipSuccess ? HBHIP_OK : ctx->fail(e, what); }

// the one way out of a copy that failed part-way: what is queued on `stream` must not outlive the call (it reads or writes
// the caller's planes); the borrowed event goes back to the pool with its scope
static int abandon(hipStream_t stream, int rc)
{
    (void)hipStreamSynchronize(stream);
    return rc;
}

int hbhip_wait_behind(hbhip_ctx *ctx, hipStream_t stream, const char *what)
{
    SyncEvent done(ctx);
    if (!done) return ctx->fail(hipErrorOutOfMemory, what);
    hipError_t e = hipEventRecord(done, stream);
    if (e == hipSuccess) e = hipEventSynchronize(done);
    return hip_rc(ctx, e, what);
}

// H2D on the upload stream, waited for; *moved: the bytes sent
static int copy_h2d_wait(hbhip_ctx *ctx, DevPicture *dst, const hbhip_host_frame *src, size_t *moved)
{
    if (!host_planes_ok(dst, src)) return HBHIP_ERR_ARG;
    SyncEvent done(ctx);
    if (!done) return ctx->fail(hipErrorOutOfMemory, "hipEventCreate(upload)");
    hipStream_t up = ctx->up();
    // whatever still reads the picture's previous contents was queued ahead of its idle mark when it was recycled
    hipError_t e = hbhip_pic_wait_idle(up, dst);
    if (e == hipSuccess) e = queue_h2d(dst, src, true, up, moved);
    if (e == hipSuccess) e = hipEventRecord(done, up);
    if (e != hipSuccess) return abandon(up, ctx->fail(e, "hipMemcpyAsync(upload)"));
    // The caller may free or reuse its planes as soon as we return (filter_loop closes buf_in, work.c:2566-2569):
    // wait for THIS copy - not for the kernels other filters have queued.  Once it has completed, work launched
    // on any stream afterwards sees the data.
    return hip_rc(ctx, hipEventSynchronize(done), "hipEventSynchronize(upload)");
}

int hbhip_copy_h2d(hbhip_ctx *ctx, DevPicture *dst, const hbhip_host_frame *src)
{
    size_t moved;
    return copy_h2d_wait(ctx, dst, src, &moved);
}

int hbhip_copy_d2h(hbhip_ctx *ctx, const hbhip_host_frame *dst, const DevPicture *src)
{
    if (!host_planes_ok(src, dst)) return HBHIP_ERR_ARG;
    SyncEvent ev(ctx);
    if (!ev) return ctx->fail(hipErrorOutOfMemory, "hipEventCreate(download)");
    hipStream_t down = ctx->down();
    size_t n = 0;
    // the picture's producers are on ctx->stream, all queued by now
    hipError_t e = hipEventRecord(ev, ctx->stream);
    if (e == hipSuccess) e = hipStreamWaitEvent(down, ev, 0);
    if (e == hipSuccess) e = queue_d2h(dst, src, false, down, &n);
    if (e == hipSuccess) e = hipEventRecord(ev, down);
    if (e != hipSuccess) return abandon(down, ctx->fail(e, "download: queue the copy"));
    return hip_rc(ctx, hipEventSynchronize(ev), "hipEventSynchronize(download)");
}

// Device-to-device copies of a picture's three planes as ONE kernel launch: hipMemcpy2DAsync makes a blit kernel per
// plane and brackets it with system-scope barrier packets - 25 us of idle queue per picture in the kernel trace of the
// NLMeans workload (tools/trace_gaps.py).
namespace {
struct PlaneCopy3
{
    const uint8_t *src[3];
    uint8_t       *dst[3];
    int spitch[3], dpitch[3], row_bytes[3], rows[3];
};

__global__ void __launch_bounds__(256) plane_copy3_kernel(PlaneCopy3 a)
{
    const int pl = blockIdx.z, y = blockIdx.y;
    if (y >= a.rows[pl]) return;
    const int x = (blockIdx.x * 256 + threadIdx.x) * 16;
    const int rb = a.row_bytes[pl];
    if (x >= rb) return;
    const uint8_t *s = a.src[pl] + (size_t)y * a.spitch[pl] + x;
    uint8_t *d = a.dst[pl] + (size_t)y * a.dpitch[pl] + x;
    if (x + 16 <= rb && (((uintptr_t)s | (uintptr_t)d) & 15) == 0)
        *reinterpret_cast<uint4 *>(d) = *reinterpret_cast<const uint4 *>(s);
    else
        for (int i = 0; i < 16 && x + i < rb; i++) d[i] = s[i];
}

int plane_copy3(hbhip_ctx *ctx, const PlaneCopy3 &a)
{
    int maxrow = 0, maxrows = 0;
    for (int c = 0; c < 3; c++) { maxrow = std::max(maxrow, a.row_bytes[c]); maxrows = std::max(maxrows, a.rows[c]); }
    HBHIP_LAUNCH(ctx, "copy_planes", plane_copy3_kernel, dim3((maxrow + 4095) / 4096, maxrows, 3), dim3(256), 0, a);
    HBHIP_CHECK(ctx, hipGetLastError());
    return HBHIP_OK;
}
} // namespace

int hbhip_copy_d2d_in(hbhip_ctx *ctx, DevPicture *dst, const hbhip_dev_frame *src)
{
    PlaneCopy3 a;
    for (int c = 0; c < 3; c++)
    {
        const size_t vis = (size_t)dst->width[c] * dst->bps;
        if (src->plane[c] == nullptr || src->stride[c] < (int)vis) return HBHIP_ERR_ARG;
        a.src[c] = (const uint8_t *)src->plane[c]; a.dst[c] = dst->plane[c];
        a.spitch[c] = src->stride[c]; a.dpitch[c] = dst->pitch[c];
        a.row_bytes[c] = std::min(src->stride[c], dst->pitch[c]);      // the caller's row padding travels too (up to our pitch)
        a.rows[c] = dst->height[c];
    }
    return plane_copy3(ctx, a);
}

int hbhip_copy_d2d_out(hbhip_ctx *ctx, const hbhip_dev_frame *dst, const DevPicture *src)
{
    PlaneCopy3 a;
    for (int c = 0; c < 3; c++)
    {
        const size_t row = (size_t)src->width[c] * src->bps;
        if (dst->plane[c] == nullptr || dst->stride[c] < (int)row) return HBHIP_ERR_ARG;
        a.src[c] = src->plane[c]; a.dst[c] = (uint8_t *)dst->plane[c];
        a.spitch[c] = src->pitch[c]; a.dpitch[c] = dst->stride[c];
        a.row_bytes[c] = (int)row; a.rows[c] = src->height[c];
    }
    return plane_copy3(ctx, a);
}

int hbhip_filter::process_dev_batch(const hbhip_dev_frame *in, int n_in, int64_t tag0,
                                    const hbhip_dev_frame *out, int out_cap, int *n_out)
{
    int produced = 0;
    for (int i = 0; i < n_in; i++)
    {
        int rc = hbhip_filter_push_dev(this, &in[i], tag0 + i);
        if (rc != HBHIP_OK) return rc;
        while (produced < out_cap && pending() > 0)
        {
            rc = hbhip_filter_pull_dev(this, &out[produced], nullptr);
            if (rc != HBHIP_OK) return rc;
            produced++;
        }
    }
    *n_out = produced;
    return HBHIP_OK;
}

// ---------------------------------------------------------------- C ABI
// ---- the on-box copy ceiling ("measure an on-box ... ceiling and report against both") -----------------
// A float4 grid-stride copy, the way /opt/skills/guides/MI355X_MICROARCH.md measures its 6.29 TB/s: 16 bytes per lane and
// trip, enough workgroups to fill every CU several times over, buffers far past the 256 MB Infinity Cache.
typedef float f32x4 __attribute__((ext_vector_type(4)));
// U float4 per lane in flight and trip; NT: non-temporal loads and stores (neither buffer is touched again)
template <int U, bool NT>
__global__ __launch_bounds__(1024) void copy_f4_kernel(const f32x4 *__restrict__ src, f32x4 *__restrict__ dst, size_t n)
{
    const size_t stride = (size_t)gridDim.x * blockDim.x;
    size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    for (; i + (size_t)(U - 1) * stride < n; i += (size_t)U * stride)
    {
        f32x4 v[U];
#pragma unroll
        for (int k = 0; k < U; k++) v[k] = NT ? __builtin_nontemporal_load(&src[i + (size_t)k * stride]) : src[i + (size_t)k * stride];
#pragma unroll
        for (int k = 0; k < U; k++)
        {
            if (NT) __builtin_nontemporal_store(v[k], &dst[i + (size_t)k * stride]);
            else dst[i + (size_t)k * stride] = v[k];
        }
    }
    for (; i < n; i += stride) dst[i] = src[i];
}

extern "C" {

static void surface_reap(hbhip_ctx *ctx, bool wait);     // device surfaces, below

int hbhip_abi_version(void) { return HBHIP_ABI_VERSION; }

int hbhip_mem_live(size_t *device_bytes, size_t *pinned_bytes)
{
    if (!device_bytes || !pinned_bytes) return HBHIP_ERR_ARG;
    *device_bytes = hbhip_live_bytes[0].load(std::memory_order_relaxed);
    *pinned_bytes = hbhip_live_bytes[1].load(std::memory_order_relaxed);
    return HBHIP_OK;
}

int hbhip_host_alloc(size_t bytes, void **out)
{
    if (!out) return HBHIP_ERR_ARG;
    *out = nullptr;
    if (hipHostMalloc(out, bytes ? bytes : 1, hipHostMallocDefault) != hipSuccess)
    {
        (void)hipGetLastError();
        *out = nullptr;
        return HBHIP_ERR_NOMEM;
    }
    return HBHIP_OK;
}

void hbhip_host_free(void *p)
{
    if (p) (void)hipHostFree(p);
}

int hbhip_device_count(void)
{
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess)
    {
        (void)hipGetLastError();
        return 0;
    }
    return n;
}

const char *hbhip_strerror(int code)
{
    switch (code)
    {
        case HBHIP_OK:              return "ok";
        case HBHIP_AGAIN:           return "no frame ready yet";
        case HBHIP_ERR_NODEVICE:    return "no usable HIP device";
        case HBHIP_ERR_HIP:         return "HIP runtime error (see hbhip_ctx_last_error)";
        case HBHIP_ERR_ARG:         return "invalid argument";
        case HBHIP_ERR_NOMEM:       return "out of (device) memory";
        case HBHIP_ERR_UNSUPPORTED: return "settings not supported by the HIP path";
        case HBHIP_ERR_STATE:       return "call not valid in this state";
        default:                    return "unknown hbhip error";
    }
}

// the copy streams, made when first asked for (hbhip_internal.h); without one the copies go to the context's own stream
static hipStream_t lazy_stream(hbhip_ctx *ctx, std::once_flag &once, hipStream_t &slot)
{
    std::call_once(once, [&] {
        (void)hipSetDevice(ctx->device);
        if (hipStreamCreateWithFlags(&slot, hipStreamNonBlocking) != hipSuccess) { (void)hipGetLastError(); slot = nullptr; }
    });
    return slot ? slot : ctx->stream;
}
hipStream_t hbhip_ctx::up() { return lazy_stream(this, up_once, up_stream); }
hipStream_t hbhip_ctx::down() { return lazy_stream(this, down_once, down_stream); }

static int ctx_create_common(int device, void *stream, bool adopt, hbhip_ctx **out)
{
    if (out == nullptr) return HBHIP_ERR_ARG;
    *out = nullptr;
    int n = hbhip_device_count();
    if (n <= 0 || device < 0 || device >= n) return HBHIP_ERR_NODEVICE;
    if (hipSetDevice(device) != hipSuccess)
    {
        (void)hipGetLastError();
        return HBHIP_ERR_NODEVICE;
    }
    hbhip_ctx *ctx = new (std::nothrow) hbhip_ctx();
    if (!ctx) return HBHIP_ERR_NOMEM;
    ctx->device = device;
    if (adopt)
    {
        ctx->stream = (hipStream_t)stream;
        ctx->own_stream = false;
    }
    else if (hipStreamCreateWithFlags(&ctx->stream, hipStreamNonBlocking) != hipSuccess)
    {
        (void)hipGetLastError();
        delete ctx;
        return HBHIP_ERR_HIP;
    }
#ifndef HBHIP_LAZY_COPY_STREAMS
    // The copy streams with the context.  (Made at their first use instead - -DHBHIP_LAZY_COPY_STREAMS - a chain whose
    // frames never leave the device has two streams fewer per context, which NLMeans alone likes (37.8 -> 38.7 k fps) and
    // the chain does not notice; but the host path's download stream, made last then, lands on a hardware queue it shares
    // with a busy compute stream: 4 070 -> 3 710 fps PCIe-inclusive, 56.9 -> 51.9 GB/s.  profiles/r6Z_streams_and_queues.log)
    (void)ctx->up(); (void)ctx->down();
#endif
    hipDeviceProp_t prop;
    if (hipGetDeviceProperties(&prop, device) == hipSuccess)
        snprintf(ctx->dev_name, sizeof(ctx->dev_name), "%s (%s, %d CUs)", prop.name,
                 prop.gcnArchName, prop.multiProcessorCount);
    *out = ctx;
    return HBHIP_OK;
}

int hbhip_ctx_create(int device, hbhip_ctx **out)
{
    return ctx_create_common(device, nullptr, false, out);
}

int hbhip_ctx_create_on_stream(int device, void *hip_stream, hbhip_ctx **out)
{
    return ctx_create_common(device, hip_stream, true, out);
}

void hbhip_ctx_destroy(hbhip_ctx *ctx)
{
    if (!ctx) return;
    (void)hipSetDevice(ctx->device);
    ctx->close_mark();
    (void)hipStreamSynchronize(ctx->stream);
    if (ctx->up_stream) { (void)hipStreamSynchronize(ctx->up_stream); (void)hipStreamDestroy(ctx->up_stream); }
    if (ctx->down_stream) { (void)hipStreamSynchronize(ctx->down_stream); (void)hipStreamDestroy(ctx->down_stream); }
    surface_reap(ctx, true);
    for (hbhip_surface *s : ctx->surface_pool) delete s;
    for (hipEvent_t e : ctx->sync_ev_pool) (void)hipEventDestroy(e);
    for (auto &p : ctx->prof_pending)
    {
        if (p.ev0) (void)hipEventDestroy(p.ev0);
        if (p.ev1) (void)hipEventDestroy(p.ev1);
    }
    for (hbhip_frame *fr : ctx->frame_pool) delete fr;
    for (hipEvent_t e : ctx->ev_pool) (void)hipEventDestroy(e);
    for (int i = 0; i < HBHIP_MAX_MARKS; i++)
        if (ctx->marks[i]) (void)hipEventDestroy(ctx->marks[i]);
    if (ctx->own_stream && ctx->stream) (void)hipStreamDestroy(ctx->stream);
    delete ctx;                                 // (bi_stage with it: every stream that used it has been waited out above)
}

int hbhip_ctx_sync(hbhip_ctx *ctx)
{
    if (!ctx) return HBHIP_ERR_ARG;
    // the mark of the pictures released since the last launch is recorded ahead of the wait, as hbhip_ctx_destroy does: behind
    // a sync every pooled picture IS idle, and the next hbhip_frame_alloc takes it instead of growing the pool past a mark
    // its own query has only just recorded
    if (ctx->has_open_mark.load(std::memory_order_acquire)) ctx->close_mark();
    HBHIP_CHECK(ctx, hipStreamSynchronize(ctx->stream));
    surface_reap(ctx, true);                   // (surface kernels still queued on the copy streams: waited for, their references dropped)
    return HBHIP_OK;
}

const char *hbhip_ctx_last_error(hbhip_ctx *ctx)
{
    if (!ctx) return "";
    // a copy per calling thread: the string itself may be rewritten by another filter's thread
    static thread_local std::string copy;
    std::lock_guard<std::recursive_mutex> lk(ctx->state_lock);
    copy = ctx->last_error;
    return copy.c_str();
}

int hbhip_ctx_device_name(hbhip_ctx *ctx, char *buf, int len)
{
    if (!ctx || !buf || len <= 0) return HBHIP_ERR_ARG;
    snprintf(buf, len, "%s", ctx->dev_name);
    return HBHIP_OK;
}

int hbhip_ctx_copy_bandwidth(hbhip_ctx *ctx, size_t bytes, int iters, double *gbps)
{
    if (!ctx || !gbps || bytes < (1u << 20) || iters < 1) return HBHIP_ERR_ARG;
    (void)hipSetDevice(ctx->device);
    DevBuf<float4> da, db;
    hipEvent_t e0 = nullptr, e1 = nullptr;
    const size_t n = bytes / sizeof(float4);
    int rc = HBHIP_OK;
    double best_ms = 0.0;
    if (da.alloc(ctx, n) != HBHIP_OK || db.alloc(ctx, n) != HBHIP_OK ||
        hipEventCreate(&e0) != hipSuccess || hipEventCreate(&e1) != hipSuccess)
        rc = ctx->fail(hipErrorOutOfMemory, "hbhip_ctx_copy_bandwidth: buffers");
    float4 *const a = da.get(), *const b = db.get();
    if (rc == HBHIP_OK && hipMemsetAsync(a, 1, n * sizeof(float4), ctx->stream) != hipSuccess) rc = HBHIP_ERR_HIP;
    // the ceiling is whatever the best of a few shapes reaches: 1 / 4 / 8 float4 in flight per lane, plain or non-temporal
    // accesses, 256 or 1024 lanes per workgroup, 8 or 32 workgroups per CU - and the runtime's own device-to-device copy
    struct Shape { int u, nt, block, per_cu; };
    static const Shape shapes[] = { {1, 0, 256, 8}, {4, 0, 256, 8}, {4, 1, 256, 8}, {8, 1, 256, 8}, {4, 0, 256, 32}, {4, 1, 256, 32},
                                    {4, 1, 1024, 2}, {8, 1, 1024, 2}, {8, 0, 512, 4}, {0, 0, 0, 0} /* hipMemcpyAsync */ };
    for (const Shape &sh : shapes)
        for (int i = 0; rc == HBHIP_OK && i < iters + 1; i++)                    // the first pass of a shape warms up
        {
            (void)hipEventRecord(e0, ctx->stream);
            if (sh.u == 0)
                (void)hipMemcpyAsync(b, a, n * sizeof(float4), hipMemcpyDeviceToDevice, ctx->stream);
            else
            {
                const dim3 grid(256 * sh.per_cu), block(sh.block);
                const f32x4 *pa = (const f32x4 *)a;
                f32x4 *pb = (f32x4 *)b;
                if (sh.u == 1)                copy_f4_kernel<1, false><<<grid, block, 0, ctx->stream>>>(pa, pb, n);
                else if (sh.u == 4 && !sh.nt) copy_f4_kernel<4, false><<<grid, block, 0, ctx->stream>>>(pa, pb, n);
                else if (sh.u == 4)           copy_f4_kernel<4, true><<<grid, block, 0, ctx->stream>>>(pa, pb, n);
                else if (!sh.nt)              copy_f4_kernel<8, false><<<grid, block, 0, ctx->stream>>>(pa, pb, n);
                else                          copy_f4_kernel<8, true><<<grid, block, 0, ctx->stream>>>(pa, pb, n);
            }
            (void)hipEventRecord(e1, ctx->stream);
            if (hipEventSynchronize(e1) != hipSuccess) { rc = ctx->fail(hipGetLastError(), "copy_f4_kernel"); break; }
            float ms = 0.f;
            (void)hipEventElapsedTime(&ms, e0, e1);
            if (i > 0 && (best_ms == 0.0 || ms < best_ms)) best_ms = ms;
        }
    if (e0) (void)hipEventDestroy(e0);
    if (e1) (void)hipEventDestroy(e1);
    if (rc == HBHIP_OK) *gbps = best_ms > 0.0 ? 2.0 * (double)(n * sizeof(float4)) / (best_ms * 1e-3) / 1e9 : 0.0;   // read + write
    return rc;
}

int hbhip_ctx_device_index(hbhip_ctx *ctx)
{
    return ctx ? ctx->device : -1;
}

int hbhip_ctx_profile_enable(hbhip_ctx *ctx, int on)
{
    if (!ctx) return HBHIP_ERR_ARG;
    std::lock_guard<std::recursive_mutex> lk(ctx->state_lock);
    if (!on) ctx->prof_resolve();
    ctx->profile = on != 0;
    return HBHIP_OK;
}

int hbhip_ctx_profile_reset(hbhip_ctx *ctx)
{
    if (!ctx) return HBHIP_ERR_ARG;
    ctx->prof_resolve();
    ctx->prof_stats.clear();
    return HBHIP_OK;
}

int hbhip_ctx_profile_count(hbhip_ctx *ctx)
{
    if (!ctx) return HBHIP_ERR_ARG;
    ctx->prof_resolve();
    return (int)ctx->prof_stats.size();
}

int hbhip_ctx_profile_get(hbhip_ctx *ctx, int idx, char *name, int name_len,
                          int64_t *launches, double *total_ms)
{
    if (!ctx || idx < 0 || idx >= (int)ctx->prof_stats.size()) return HBHIP_ERR_ARG;
    const hbhip_prof_stat &s = ctx->prof_stats[idx];
    if (name && name_len > 0) snprintf(name, name_len, "%s", s.name.c_str());
    if (launches) *launches = s.launches;
    if (total_ms) *total_ms = s.total_ms;
    return HBHIP_OK;
}

int hbhip_ctx_mark(hbhip_ctx *ctx, int slot)
{
    if (!ctx || slot < 0 || slot >= HBHIP_MAX_MARKS) return HBHIP_ERR_ARG;
    if (!ctx->marks[slot]) HBHIP_CHECK(ctx, hipEventCreate(&ctx->marks[slot]));
    HBHIP_CHECK(ctx, hipEventRecord(ctx->marks[slot], ctx->stream));
    return HBHIP_OK;
}

int hbhip_ctx_elapsed_ms(hbhip_ctx *ctx, int a, int b, double *ms)
{
    if (!ctx || !ms || a < 0 || b < 0 || a >= HBHIP_MAX_MARKS || b >= HBHIP_MAX_MARKS ||
        !ctx->marks[a] || !ctx->marks[b])
        return HBHIP_ERR_ARG;
    HBHIP_CHECK(ctx, hipEventSynchronize(ctx->marks[b]));
    float f = 0.f;
    HBHIP_CHECK(ctx, hipEventElapsedTime(&f, ctx->marks[a], ctx->marks[b]));
    *ms = f;
    return HBHIP_OK;
}

int hbhip_dev_alloc(hbhip_ctx *ctx, size_t bytes, void **out)
{
    if (!ctx || !out) return HBHIP_ERR_ARG;
    HBHIP_CHECK(ctx, hipSetDevice(ctx->device));
    HBHIP_CHECK(ctx, hipMalloc(out, bytes));
    return HBHIP_OK;
}

int hbhip_dev_free(hbhip_ctx *ctx, void *p)
{
    if (!ctx) return HBHIP_ERR_ARG;
    HBHIP_CHECK(ctx, hipStreamSynchronize(ctx->stream));
    HBHIP_CHECK(ctx, hipFree(p));
    return HBHIP_OK;
}

int hbhip_dev_upload(hbhip_ctx *ctx, void *dst, const void *src, size_t bytes)
{
    if (!ctx) return HBHIP_ERR_ARG;
    HBHIP_CHECK(ctx, hipMemcpyAsync(dst, src, bytes, hipMemcpyHostToDevice, ctx->stream));
    HBHIP_CHECK(ctx, hipStreamSynchronize(ctx->stream));
    return HBHIP_OK;
}

int hbhip_dev_download(hbhip_ctx *ctx, void *dst, const void *src, size_t bytes)
{
    if (!ctx) return HBHIP_ERR_ARG;
    HBHIP_CHECK(ctx, hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToHost, ctx->stream));
    HBHIP_CHECK(ctx, hipStreamSynchronize(ctx->stream));
    return HBHIP_OK;
}

// ---- device-resident frames -----------------------------------------------------
// How frames are ordered.  A job may run its filters on more than one context of a GPU (hbhip_host_ctx_for_role), so a
// frame may be written and read on several streams.  The rule, kept by the helpers below - the only code that touches
// `ready`, `complete`, `last_user` and `owner_used`, under the owner's frame_lock:
//  * The contents are complete behind the ready mark; without one, at once after a synchronous upload, else behind what
//    the current user - the context that last took the frame through hbhip_frame_use_on, or the owner - has queued so far.
//    A reader waits for that point and nothing else: a second stream is not to wait for what the first queued since.
//  * A context that reads or writes the frame takes it through hbhip_frame_use_on and becomes its current user, behind
//    the previous user's stream as it stands if that was another foreign context.  A writer marks the contents ready on
//    the current user's stream.
//  * The last reference gone, the frame goes idle behind its last foreign user's stream and behind its owner's (unless
//    only foreign contexts took it), as they stand then; it is filled again behind both marks.
static hbhip_ctx *current_user(const hbhip_frame *fr) { return fr->last_user ? fr->last_user : fr->ctx; }

static hipError_t order_after_contents(hbhip_frame *fr, hipStream_t stream)
{
    if (fr->ready) return wait_mark(stream, fr->ready);
    hbhip_ctx *user = current_user(fr);
    return fr->complete || user->stream == stream ? hipSuccess : wait_mark(stream, stream_now(user));
}

static hipError_t note_user(hbhip_frame *fr, hbhip_ctx *ctx)
{
    hbhip_ctx *prev = fr->last_user;
    const hipError_t e = prev && prev != fr->ctx && prev != ctx ? wait_mark(ctx->stream, stream_now(prev)) : hipSuccess;
    if (e == hipSuccess) { fr->last_user = ctx; fr->owner_used |= ctx == fr->ctx; }
    return e;
}

// null `ready`: a copy that has finished filled the frame
static void set_contents(hbhip_frame *fr, std::shared_ptr<IdleMark> ready) { fr->complete = !ready; fr->ready = std::move(ready); }

static void frame_idle(hbhip_frame *fr)
{
    hbhip_ctx *foreign = fr->last_user != fr->ctx ? fr->last_user : nullptr;
    fr->pic.idle = !foreign || fr->owner_used ? stream_now(fr->ctx) : nullptr;
    fr->reader_idle = foreign ? stream_now(foreign) : nullptr;
}

// a mark recorded on `stream` right now
static std::shared_ptr<IdleMark> record_mark(hipStream_t stream)
{
    std::shared_ptr<IdleMark> m = std::make_shared<IdleMark>();
    if (hipEventCreateWithFlags(&m->ev, hipEventDisableTiming) != hipSuccess || hipEventRecord(m->ev, stream) != hipSuccess)
    {
        (void)hipGetLastError();
        return nullptr;
    }
    m->stream = stream;
    m->recorded = true;
    m->closed.store(true, std::memory_order_release);
    return m;
}

// The two ends of a run.  A frame is filled on its context's upload stream and drained on its download stream, from and
// into a planar host picture, an NV12 / P010LE host picture or a device surface: the entry points below check their
// arguments and bring the step that is theirs, the protocol around it is here.  A step returns HBHIP_OK or the code of
// what failed (through ctx->fail where a HIP call did); then the stream is waited out (abandon) and the token stays null.
//
// fill: the stream behind whatever still reads the frame's previous contents (queued ahead of its idle marks when it was
// recycled); `queue(up, done)` queues the source's work and records `done` where the SOURCE is free again; the frame's
// ready mark behind all of it.  *token: `done`, for hbhip_ctx_upload_done.
extern "C++" {                                         // (templates, in the middle of the C ABI)
template <class Queue>
static int fill_frame(hbhip_frame *fr, const char *what, Queue queue, void **token, std::shared_ptr<IdleMark> *ready_out = nullptr)
{
    hbhip_ctx *ctx = fr->ctx;
    hipStream_t up = ctx->up();
    SyncEvent done(ctx);
    if (!done) return ctx->fail(hipErrorOutOfMemory, what);
    int rc = hip_rc(ctx, hbhip_pic_wait_idle(up, &fr->pic), what);
    if (rc == HBHIP_OK) rc = queue(up, done);
    std::shared_ptr<IdleMark> ready = rc == HBHIP_OK ? record_mark(up) : nullptr;
    if (rc == HBHIP_OK && !ready) rc = ctx->fail(hipErrorOutOfMemory, what);
    if (rc != HBHIP_OK) return abandon(up, rc);
    if (ready_out) *ready_out = ready;
    { std::lock_guard<std::mutex> lk(ctx->frame_lock); set_contents(fr, std::move(ready)); }
    *token = done.keep();
    return HBHIP_OK;
}

// drain: the stream behind the frame's contents; `queue(down)` queues the destination's work; the token's event behind it;
// `then(down)` what has to lie behind that event.  *token: the event, for hbhip_frame_download_wait.
template <class Queue, class Then>
static int drain_frame(hbhip_frame *fr, const char *what, Queue queue, Then then, void **token)
{
    hbhip_ctx *ctx = fr->ctx;
    hipStream_t down = ctx->down();
    SyncEvent ev(ctx);
    if (!ev) return ctx->fail(hipErrorOutOfMemory, what);
    hipError_t e;
    { std::lock_guard<std::mutex> lk(ctx->frame_lock); e = order_after_contents(fr, down); }
    int rc = hip_rc(ctx, e, what);
    if (rc == HBHIP_OK) rc = queue(down);
    if (rc == HBHIP_OK) rc = hip_rc(ctx, hipEventRecord(ev, down), what);
    if (rc == HBHIP_OK) rc = then(down);
    if (rc != HBHIP_OK) return abandon(down, rc);
    *token = ev.keep();
    return HBHIP_OK;
}

template <class Queue>
static int drain_frame(hbhip_frame *fr, const char *what, Queue queue, void **token)
{
    return drain_frame(fr, what, queue, [](hipStream_t) { return HBHIP_OK; }, token);
}
} // extern "C++"

hbhip_ctx *hbhip_frame_context(hbhip_frame *fr)
{
    return fr ? fr->ctx : nullptr;
}

int hbhip_frame_alloc(hbhip_ctx *ctx, int width, int height, int depth, int lcw, int lch, hbhip_frame **out)
{
    if (!ctx || !out || width < 1 || height < 1) return HBHIP_ERR_ARG;
    *out = nullptr;
    (void)hipSetDevice(ctx->device);
    std::unique_lock<std::mutex> lk(ctx->frame_lock);
    {
        // a frame whose last user has finished (its idle event has fired) can be filled at once; one that is still
        // being read would hold an upload back until the GPU gets there - take such a frame only when the pool has
        // grown to its bound (the oldest: the likeliest to be free soonest)
        int same = 0, pick = -1, oldest = -1;
        for (size_t i = 0; i < ctx->frame_pool.size(); i++)
        {
            hbhip_frame *fr = ctx->frame_pool[i];
            if (fr->width != width || fr->height != height || fr->depth != depth || fr->lcw != lcw || fr->lch != lch) continue;
            same++;
            if (oldest < 0) oldest = (int)i;
            if (hbhip_pic_idle_done(&fr->pic)) { pick = (int)i; break; }
        }
        (void)hipGetLastError();                                  // hipErrorNotReady of the queries
        if (pick < 0 && same >= 48) pick = oldest;
        if (pick >= 0)
        {
            hbhip_frame *fr = ctx->frame_pool[pick];
            ctx->frame_pool.erase(ctx->frame_pool.begin() + pick);
            fr->refs = 1;
            fr->ready.reset(); fr->last_user = nullptr; fr->complete = fr->owner_used = false;
            fr->pic.frame = fr;
            fr->pic.refs = 0; fr->pic.flags = 0; fr->pic.combed = 0; fr->pic.aux = 0; fr->pic.tag = 0;
            // taken although its users may still be running (the pool is at its bound): whoever fills it on this
            // context's stream does so behind them
            (void)hbhip_pic_wait_idle(ctx->stream, &fr->pic);
            *out = fr;
            return HBHIP_OK;
        }
    }
    lk.unlock();
    hbhip_frame *fr = new (std::nothrow) hbhip_frame();
    if (!fr) return HBHIP_ERR_NOMEM;
    fr->ctx = ctx; fr->width = width; fr->height = height; fr->depth = depth; fr->lcw = lcw; fr->lch = lch;
    PicGeometry g;
    g.set(width, height, depth, lcw, lch);
    // laid out exactly like hb_frame_buffer_init lays a host frame out (fifo.c:820-881: stride = the row rounded up to
    // 64 bytes, the planes one behind the other), so that a frame moves between the two in ONE 1-D copy
    size_t off[3], total = 0;
    for (int c = 0; c < 3; c++)
    {
        fr->pic.width[c] = g.pw[c];
        fr->pic.height[c] = g.ph[c];
        fr->pic.pitch[c] = hbhip_align_up(g.pw[c] * g.bps, 64);
        off[c] = total;
        total += (size_t)fr->pic.pitch[c] * g.ph[c];
    }
    total = (total + 255) & ~(size_t)255;
    fr->pic.bps = g.bps;
    fr->pic.bytes = total;
    if (const int rc = fr->mem.alloc(ctx, total))
    {
        delete fr;
        return rc;
    }
    (void)hipMemsetAsync(fr->mem.get(), 0, total, ctx->stream);
    hbhip_pic_mark_idle(ctx, &fr->pic);    // an upload (on the copy stream) must not overtake the clearing
    for (int c = 0; c < 3; c++) fr->pic.plane[c] = fr->mem.get() + off[c];
    fr->pic.frame = fr;
    *out = fr;
    return HBHIP_OK;
}

void hbhip_frame_retain(hbhip_frame *fr)
{
    if (!fr) return;
    std::lock_guard<std::mutex> lk(fr->ctx->frame_lock);
    fr->refs++;
}

void hbhip_frame_release(hbhip_frame *fr)
{
    if (!fr) return;
    std::lock_guard<std::mutex> lk(fr->ctx->frame_lock);
    if (--fr->refs > 0) return;
    (void)hipSetDevice(fr->ctx->device);
    frame_idle(fr);                           // its users are all queued by now
    fr->ctx->frame_pool.push_back(fr);
}

int hbhip_frame_use_on(hbhip_frame *fr, hbhip_ctx *ctx)
{
    if (!fr || !ctx || ctx->device != fr->ctx->device) return HBHIP_ERR_ARG;
    (void)hipSetDevice(ctx->device);
    std::lock_guard<std::mutex> lk(fr->ctx->frame_lock);
    hipError_t e = order_after_contents(fr, ctx->stream);
    if (e == hipSuccess) e = note_user(fr, ctx);
    return e == hipSuccess ? HBHIP_OK : ctx->fail(e, "use_on: order behind the frame's contents and earlier users");
}

// The writability test of a device picture (fifo.c:624-639 asks av_buffer_is_writable the same thing): a holder that
// sees 1 is the only one, and nobody else can take a reference except through it.
int hbhip_frame_refs(hbhip_frame *fr)
{
    if (!fr) return 0;
    std::lock_guard<std::mutex> lk(fr->ctx->frame_lock);
    return fr->refs;
}

// that test and a reference more in one step: taken only by the frame's one holder
static bool retain_if_sole(hbhip_frame *fr)
{
    std::lock_guard<std::mutex> lk(fr->ctx->frame_lock);
    if (fr->refs != 1) return false;
    fr->refs++;
    return true;
}

int hbhip_frame_describe(hbhip_frame *fr, hbhip_dev_frame *out, int *width, int *height)
{
    if (!fr || !out) return HBHIP_ERR_ARG;
    for (int c = 0; c < 3; c++)
    {
        out->plane[c] = fr->pic.plane[c];
        out->stride[c] = fr->pic.pitch[c];
    }
    if (width) *width = fr->width;
    if (height) *height = fr->height;
    return HBHIP_OK;
}

int hbhip_frame_copy(hbhip_frame *dst, hbhip_frame *src)
{
    if (!dst || !src) return HBHIP_ERR_ARG;
    if (dst->width != src->width || dst->height != src->height || dst->depth != src->depth ||
        dst->lcw != src->lcw || dst->lch != src->lch)
        return HBHIP_ERR_ARG;
    const int rc = hbhip_frame_use_on(src, dst->ctx);            // the copy reads src on dst's stream
    if (rc != HBHIP_OK) return rc;
    hbhip_dev_frame d;
    hbhip_frame_describe(src, &d, nullptr, nullptr);
    return hbhip_copy_d2d_in(dst->ctx, &dst->pic, &d);
}

int hbhip_frame_upload(hbhip_frame *fr, const hbhip_host_frame *src)
{
    if (!fr || !src) return HBHIP_ERR_ARG;
    (void)hipSetDevice(fr->ctx->device);
    size_t moved = 0;
    const int rc = copy_h2d_wait(fr->ctx, &fr->pic, src, &moved);      // returns when the copy has finished
    if (rc != HBHIP_OK) return rc;
    fr->ctx->bus_h2d += moved;
    std::lock_guard<std::mutex> lk(fr->ctx->frame_lock);
    set_contents(fr, nullptr);
    return HBHIP_OK;
}

// The pipelined H2D (the upload adapter keeps a few in flight, as the download adapter does with its copies): the copy is
// queued on the upload stream and the call returns; `src` must stay valid until hbhip_ctx_upload_done(token) says so.  The
// frame's ready mark lies right behind the copy.
int hbhip_frame_upload_async(hbhip_frame *fr, const hbhip_host_frame *src, void **token)
{
    if (!fr || !src || !token) return HBHIP_ERR_ARG;
    *token = nullptr;
    hbhip_ctx *ctx = fr->ctx;
    (void)hipSetDevice(ctx->device);
    if (!host_planes_ok(&fr->pic, src)) return HBHIP_ERR_ARG;
    size_t moved = 0;
    const int rc = fill_frame(fr, "upload", [&](hipStream_t up, hipEvent_t done) {
        hipError_t e = queue_h2d(&fr->pic, src, true, up, &moved);
        if (e == hipSuccess) e = hipEventRecord(done, up);
        return hip_rc(ctx, e, "hipMemcpyAsync(upload)");
    }, token);
    if (rc == HBHIP_OK) ctx->bus_h2d += moved;
    return rc;
}

// has the copy behind `token` finished (block != 0: wait for it)?  HBHIP_OK: yes, the source planes are free again and the
// token is spent; HBHIP_AGAIN: not yet (block == 0 only)
int hbhip_ctx_upload_done(hbhip_ctx *ctx, void *token, int block)
{
    if (!ctx || !token) return HBHIP_ERR_ARG;
    (void)hipSetDevice(ctx->device);
    hipEvent_t ev = (hipEvent_t)token;
    hipError_t e = block ? hipEventSynchronize(ev) : hipEventQuery(ev);
    if (e == hipErrorNotReady) { (void)hipGetLastError(); return HBHIP_AGAIN; }
    ctx->sync_ev_put(ev);
    surface_reap(ctx, false);
    return e == hipSuccess ? HBHIP_OK : ctx->fail(e, "upload: wait for the copy");
}

int hbhip_frame_download(hbhip_frame *fr, const hbhip_host_frame *dst)
{
    if (!fr || !dst) return HBHIP_ERR_ARG;
    void *token = nullptr;
    const int rc = hbhip_frame_download_async(fr, dst, &token);
    return rc != HBHIP_OK ? rc : hbhip_frame_download_wait(fr, token);
}

int hbhip_frame_mark_ready(hbhip_frame *fr)
{
    if (!fr) return HBHIP_ERR_ARG;
    (void)hipSetDevice(fr->ctx->device);
    std::lock_guard<std::mutex> lk(fr->ctx->frame_lock);
    set_contents(fr, stream_now(current_user(fr)));
    return HBHIP_OK;
}

// D2H on the download stream behind the frame's contents.  Several in flight keep the bus busy while the kernels of
// later frames run.
int hbhip_frame_download_async(hbhip_frame *fr, const hbhip_host_frame *dst, void **token)
{
    if (!fr || !dst || !token) return HBHIP_ERR_ARG;
    *token = nullptr;
    hbhip_ctx *ctx = fr->ctx;
    (void)hipSetDevice(ctx->device);
    if (!host_planes_ok(&fr->pic, dst)) return HBHIP_ERR_ARG;
    size_t moved = 0;
    const int rc = drain_frame(fr, "download", [&](hipStream_t down) {
        return hip_rc(ctx, queue_d2h(dst, &fr->pic, true, down, &moved), "hipMemcpyAsync(download)");
    }, token);
    if (rc == HBHIP_OK) ctx->bus_d2h += moved;
    return rc;
}

int hbhip_frame_download_wait(hbhip_frame *fr, void *token)
{
    if (!fr || !token) return HBHIP_ERR_ARG;
    hbhip_ctx *ctx = fr->ctx;
    (void)hipSetDevice(ctx->device);
    hipEvent_t ev = (hipEvent_t)token;
    const hipError_t e = hipEventSynchronize(ev);
    ctx->sync_ev_put(ev);
    surface_reap(ctx, false);
    return e == hipSuccess ? HBHIP_OK : ctx->fail(e, "hipEventSynchronize(download)");
}

// ---- biplanar host pictures (NV12 / P010LE) at the two ends of a run ----------------------------------------------
// The frame stays planar; the host picture goes through a staging buffer in its own layout and a repack kernel
// (biplanar.hip).  Same ordering rule as the planar copies: the split runs behind the H2D copy on the upload stream and
// the frame's ready mark is the split; the merge runs on the download stream behind the frame's contents and the D2H
// copy behind the merge.
static int surface_geometry_ok(int width, int height, int depth)
{
    return (depth == 8 || depth == 10) && width >= 2 && height >= 2;
}

// a frame the repack kernels take: 4:2:0, and what a surface may be
static bool bi_frame_ok(const hbhip_frame *fr)
{
    return fr->lcw == 1 && fr->lch == 1 && surface_geometry_ok(fr->width, fr->height, fr->depth);
}

// `widen`: the host picture is P010LE and the frame has 8 bits (hbhip_frame_download_widen)
static int bi_check(const hbhip_frame *fr, const hbhip_host_biplanar *hb, BiLayout *l, bool widen = false)
{
    if (!bi_frame_ok(fr) || (widen && fr->depth != 8)) return HBHIP_ERR_UNSUPPORTED;
    hbhip_bi_layout(fr->width, fr->height, widen ? 10 : fr->depth, l);
    for (int p = 0; p < 2; p++)
        if (hb->plane[p] == nullptr || hb->stride[p] < l->row_bytes[p]) return HBHIP_ERR_ARG;
    return HBHIP_OK;
}

// the context's staging buffer of direction `dir`, at least `bytes` long (bi_lock[dir] held).  Growing it waits the stream
// that uses it out first: earlier pairs may still be running.
static uint8_t *bi_stage(hbhip_ctx *ctx, int dir, size_t bytes, hipStream_t stream)
{
    DevBuf<uint8_t> &st = ctx->bi_stage[dir];
    if (st.count() < bytes && st.get()) (void)hipStreamSynchronize(stream);
    (void)st.reserve(ctx, bytes);
    return st.get();
}

// host picture <-> staging buffer: one 1-D copy when the host picture has the staging layout, else a 2-D copy per plane.
// *moved: what goes over the bus (hbhip_ctx_bus_bytes)
static hipError_t bi_copy(uint8_t *stage, const BiLayout &l, const hbhip_host_biplanar *hb, bool to_device, hipStream_t stream, size_t *moved)
{
    const hipMemcpyKind kind = to_device ? hipMemcpyHostToDevice : hipMemcpyDeviceToHost;
    *moved = 0;
    if (hb->stride[0] == l.pitch[0] && hb->stride[1] == l.pitch[1] &&
        hb->plane[1] == hb->plane[0] + (size_t)l.pitch[0] * l.rows[0])
    {
        *moved = l.bytes;
        return to_device ? hipMemcpyAsync(stage, hb->plane[0], l.bytes, kind, stream)
                         : hipMemcpyAsync(hb->plane[0], stage, l.bytes, kind, stream);
    }
    hipError_t e = hipSuccess;
    uint8_t *at = stage;
    for (int p = 0; p < 2 && e == hipSuccess; p++)
    {
        // up: the caller's row padding travels too (up to our pitch), as in the planar upload - the split hands it on to
        // the frame, whose readers read it; down: the samples only, as in the planar download
        const size_t row = to_device ? (size_t)std::min(hb->stride[p], l.pitch[p]) : (size_t)l.row_bytes[p];
        e = to_device ? hipMemcpy2DAsync(at, l.pitch[p], hb->plane[p], hb->stride[p], row, l.rows[p], kind, stream)
                      : hipMemcpy2DAsync(hb->plane[p], hb->stride[p], at, l.pitch[p], row, l.rows[p], kind, stream);
        at += (size_t)l.pitch[p] * l.rows[p];
        *moved += row * l.rows[p];
    }
    return e;
}

// `src` must stay valid until hbhip_ctx_upload_done(token) says so, as with hbhip_frame_upload_async
int hbhip_frame_upload_biplanar_async(hbhip_frame *fr, const hbhip_host_biplanar *src, void **token)
{
    if (!fr || !src || !token) return HBHIP_ERR_ARG;
    *token = nullptr;
    hbhip_ctx *ctx = fr->ctx;
    BiLayout l;
    int rc = bi_check(fr, src, &l);
    if (rc != HBHIP_OK) return rc;
    (void)hipSetDevice(ctx->device);
    size_t moved = 0;
    rc = fill_frame(fr, "upload (biplanar)", [&](hipStream_t up, hipEvent_t done) {
        std::lock_guard<std::mutex> lk(ctx->bi_lock[0]);
        uint8_t *stage = bi_stage(ctx, 0, l.bytes, up);
        hipError_t e = stage ? bi_copy(stage, l, src, true, up, &moved) : hipErrorOutOfMemory;
        if (e == hipSuccess) e = hipEventRecord(done, up);                    // the host picture is free behind the copy
        return e != hipSuccess ? ctx->fail(e, "upload (biplanar)") : hbhip_bi_repack_launch(ctx, up, false, stage, fr);
    }, token);
    if (rc == HBHIP_OK) ctx->bus_h2d += moved;
    return rc;
}

int hbhip_frame_upload_biplanar(hbhip_frame *fr, const hbhip_host_biplanar *src)
{
    void *token = nullptr;
    const int rc = hbhip_frame_upload_biplanar_async(fr, src, &token);
    return rc != HBHIP_OK ? rc : hbhip_ctx_upload_done(fr->ctx, token, 1);
}

// the merge into the staging buffer and the D2H copy behind it; `widen`: an 8-bit frame as P010LE (bi_widen_merge_kernel)
static int download_biplanar(hbhip_frame *fr, const hbhip_host_biplanar *dst, void **token, bool widen)
{
    if (!fr || !dst || !token) return HBHIP_ERR_ARG;
    *token = nullptr;
    hbhip_ctx *ctx = fr->ctx;
    BiLayout l;
    int rc = bi_check(fr, dst, &l, widen);
    if (rc != HBHIP_OK) return rc;
    (void)hipSetDevice(ctx->device);
    size_t moved = 0;
    rc = drain_frame(fr, "download (biplanar)", [&](hipStream_t down) {
        std::lock_guard<std::mutex> lk(ctx->bi_lock[1]);
        uint8_t *stage = bi_stage(ctx, 1, l.bytes, down);
        if (!stage) return ctx->fail(hipErrorOutOfMemory, "download (biplanar)");
        const int launched = widen ? hbhip_bi_widen_repack_launch(ctx, down, stage, fr) : hbhip_bi_repack_launch(ctx, down, true, stage, fr);
        return launched != HBHIP_OK ? launched : hip_rc(ctx, bi_copy(stage, l, dst, false, down, &moved), "download (biplanar)");
    }, token);
    if (rc == HBHIP_OK) ctx->bus_d2h += moved;
    return rc;
}

// `dst` and the frame must stay valid until hbhip_frame_download_wait(fr, token) has returned
int hbhip_frame_download_biplanar_async(hbhip_frame *fr, const hbhip_host_biplanar *dst, void **token)
{
    return download_biplanar(fr, dst, token, false);
}

int hbhip_frame_download_biplanar(hbhip_frame *fr, const hbhip_host_biplanar *dst)
{
    void *token = nullptr;
    const int rc = hbhip_frame_download_biplanar_async(fr, dst, &token);
    return rc != HBHIP_OK ? rc : hbhip_frame_download_wait(fr, token);
}

int hbhip_frame_download_widen_async(hbhip_frame *fr, const hbhip_host_biplanar *dst, void **token)
{
    return download_biplanar(fr, dst, token, true);
}

int hbhip_frame_download_widen(hbhip_frame *fr, const hbhip_host_biplanar *dst)
{
    void *token = nullptr;
    const int rc = hbhip_frame_download_widen_async(fr, dst, &token);
    return rc != HBHIP_OK ? rc : hbhip_frame_download_wait(fr, token);
}

// A packed 32-bit RGB host picture of an 8-bit 4:2:0 frame (rgb_pack.hip): the pack into the download staging buffer and
// the D2H copy behind it, ordered and finished like the biplanar download.  The copy moves 4 * width bytes a row and
// nothing of the caller's row padding: one block where the caller's rows and the staging buffer's are both exactly that long.
int hbhip_frame_download_rgb32_async(hbhip_frame *fr, uint8_t *dst, int stride, int order, int matrix, int full_range, void **token)
{
    if (!fr || !dst || !token) return HBHIP_ERR_ARG;
    *token = nullptr;
    hbhip_ctx *ctx = fr->ctx;
    if (fr->lcw != 1 || fr->lch != 1 || fr->depth != 8 || fr->width < 2 || fr->height < 2 || (fr->width & 1) || (fr->height & 1) ||
        !hbhip_rgb32_matrix_ok(matrix))
        return HBHIP_ERR_UNSUPPORTED;
    const int row = 4 * fr->width, pitch = hbhip_rgb32_pitch(fr->width), rows = fr->height;
    if (stride < row || order < HBHIP_RGB32_BGRA || order > HBHIP_RGB32_ABGR) return HBHIP_ERR_ARG;
    (void)hipSetDevice(ctx->device);
    const int rc = drain_frame(fr, "download (rgb32)", [&](hipStream_t down) {
        std::lock_guard<std::mutex> lk(ctx->bi_lock[1]);
        uint8_t *stage = bi_stage(ctx, 1, (size_t)pitch * rows, down);
        if (!stage) return ctx->fail(hipErrorOutOfMemory, "download (rgb32)");
        const int launched = hbhip_rgb32_pack_launch(ctx, down, stage, pitch, fr, order, matrix, full_range);
        if (launched != HBHIP_OK) return launched;
        const hipError_t e = stride == row && pitch == row
            ? hipMemcpyAsync(dst, stage, (size_t)row * rows, hipMemcpyDeviceToHost, down)
            : hipMemcpy2DAsync(dst, stride, stage, pitch, row, rows, hipMemcpyDeviceToHost, down);
        return hip_rc(ctx, e, "download (rgb32)");
    }, token);
    if (rc == HBHIP_OK) ctx->bus_d2h += (uint64_t)row * rows;
    return rc;
}

int hbhip_frame_download_rgb32(hbhip_frame *fr, uint8_t *dst, int stride, int order, int matrix, int full_range)
{
    void *token = nullptr;
    const int rc = hbhip_frame_download_rgb32_async(fr, dst, stride, order, matrix, full_range, &token);
    return rc != HBHIP_OK ? rc : hbhip_frame_download_wait(fr, token);
}

// ---- device surfaces (NV12 / P010LE pictures in HBM) at the two ends of a run -----------------------------------------
// No staging buffer and no bi_lock: the repack kernel reads or writes the surface where it lies.  The same ordering rule:
// the split runs on the upload stream behind the surface's contents and is the frame's ready mark, the merge on the
// download stream behind the frame's contents (and the surface's earlier readers) and is the surface's ready mark.
// the last reference has gone: a pooled surface goes back to its pool, a wrapped one to its owner (outside the lock)
static void surface_unref(hbhip_surface *s)
{
    {
        std::lock_guard<std::mutex> lk(s->ctx->surface_lock);
        if (--s->refs > 0) return;
        if (s->mem.get()) { s->ctx->surface_pool.push_back(s); return; }
    }
    if (s->release) s->release(s->opaque);
    delete s;
}

// drop the references of the kernels queued on `ctx` that have finished (all of them when `wait`: they are waited for)
static void surface_reap(hbhip_ctx *ctx, bool wait)
{
    std::vector<hbhip_ctx::SurfaceOp> gone;
    {
        std::lock_guard<std::mutex> lk(ctx->surface_lock);
        if (ctx->surface_ops.empty()) return;
        if (wait) gone.swap(ctx->surface_ops);
        else
        {
            size_t keep = 0;
            for (hbhip_ctx::SurfaceOp &op : ctx->surface_ops)
                if (mark_passed(op.done)) gone.push_back(std::move(op));
                else { if (&ctx->surface_ops[keep] != &op) ctx->surface_ops[keep] = std::move(op); keep++; }
            ctx->surface_ops.resize(keep);
            (void)hipGetLastError();                              // hipErrorNotReady of the queries
        }
    }
    for (hbhip_ctx::SurfaceOp &op : gone)
    {
        if (wait && op.done) (void)hipEventSynchronize(op.done->ev);
        surface_unref(op.s);
    }
}

int hbhip_surface_alloc(hbhip_ctx *ctx, int width, int height, int depth, int pitch_align, int rows_align, hbhip_surface **out)
{
    if (!ctx || !out) return HBHIP_ERR_ARG;
    *out = nullptr;
    if (pitch_align < 16 || (pitch_align & (pitch_align - 1)) || pitch_align > 4096 || rows_align < 1 || rows_align > 256)
        return HBHIP_ERR_ARG;
    if (!surface_geometry_ok(width, height, depth)) return HBHIP_ERR_UNSUPPORTED;
    (void)hipSetDevice(ctx->device);
    surface_reap(ctx, false);
    {
        std::lock_guard<std::mutex> lk(ctx->surface_lock);
        // the longest-released one first: the likeliest to have no reader left that an export into it would wait for
        for (size_t i = 0; i < ctx->surface_pool.size(); i++)
        {
            hbhip_surface *s = ctx->surface_pool[i];
            if (s->width != width || s->height != height || s->depth != depth || s->pitch_align != pitch_align ||
                s->rows_align != rows_align)
                continue;
            ctx->surface_pool.erase(ctx->surface_pool.begin() + (ptrdiff_t)i);
            s->refs = 1;
            *out = s;
            return HBHIP_OK;
        }
    }
    BiLayout l;
    hbhip_bi_layout(width, height, depth, &l);
    hbhip_surface *s = new (std::nothrow) hbhip_surface();
    if (!s) return HBHIP_ERR_NOMEM;
    s->ctx = ctx; s->width = width; s->height = height; s->depth = depth;
    s->pitch_align = pitch_align; s->rows_align = rows_align;
    const int rows0 = hbhip_align_up(height, rows_align);
    for (int p = 0; p < 2; p++) s->pitch[p] = hbhip_align_up(l.row_bytes[p], pitch_align);
    const size_t bytes = (size_t)s->pitch[0] * rows0 + (size_t)s->pitch[1] * ((rows0 + 1) / 2);
    if (const int rc = s->mem.alloc(ctx, bytes))
    {
        delete s;
        return rc;
    }
    s->plane[0] = s->mem.get();
    s->plane[1] = s->plane[0] + (size_t)s->pitch[0] * rows0;
    // padding and padded rows are never written by an export: cleared once, and the first export waits for that
    (void)hipMemsetAsync(s->plane[0], 0, bytes, ctx->stream);
    s->ready = stream_now(ctx);
    *out = s;
    return HBHIP_OK;
}

int hbhip_surface_wrap(hbhip_ctx *ctx, const hbhip_dev_surface *mem, int width, int height, int depth,
                       void (*release)(void *), void *opaque, hbhip_surface **out)
{
    if (!ctx || !mem || !out) return HBHIP_ERR_ARG;
    *out = nullptr;
    if (!mem->plane[0] || !mem->plane[1]) return HBHIP_ERR_ARG;
    if (!surface_geometry_ok(width, height, depth)) return HBHIP_ERR_UNSUPPORTED;
    BiLayout l;
    hbhip_bi_layout(width, height, depth, &l);
    for (int p = 0; p < 2; p++)
        if (((uintptr_t)mem->plane[p] & 15) || mem->pitch[p] < 0 || (mem->pitch[p] & 15)) return HBHIP_ERR_UNSUPPORTED;
    for (int p = 0; p < 2; p++)
        if (mem->pitch[p] < l.row_bytes[p]) return HBHIP_ERR_ARG;
    const uintptr_t b0 = (uintptr_t)mem->plane[0], e0 = b0 + (size_t)mem->pitch[0] * l.rows[0];
    const uintptr_t b1 = (uintptr_t)mem->plane[1], e1 = b1 + (size_t)mem->pitch[1] * l.rows[1];
    if (b0 < e1 && b1 < e0) return HBHIP_ERR_ARG;                 // the planes overlap
    hbhip_surface *s = new (std::nothrow) hbhip_surface();
    if (!s) return HBHIP_ERR_NOMEM;
    s->ctx = ctx; s->width = width; s->height = height; s->depth = depth;
    for (int p = 0; p < 2; p++) { s->plane[p] = (uint8_t *)mem->plane[p]; s->pitch[p] = mem->pitch[p]; }
    s->release = release;
    s->opaque = opaque;
    *out = s;
    return HBHIP_OK;
}

void hbhip_surface_retain(hbhip_surface *s)
{
    if (!s) return;
    std::lock_guard<std::mutex> lk(s->ctx->surface_lock);
    s->refs++;
}

void hbhip_surface_release(hbhip_surface *s)
{
    if (!s) return;
    hbhip_ctx *ctx = s->ctx;
    (void)hipSetDevice(ctx->device);
    surface_unref(s);
    surface_reap(ctx, false);
}

int hbhip_surface_describe(hbhip_surface *s, hbhip_dev_surface *out, int *width, int *height, int *depth)
{
    if (!s || !out) return HBHIP_ERR_ARG;
    for (int p = 0; p < 2; p++) { out->plane[p] = s->plane[p]; out->pitch[p] = s->pitch[p]; }
    if (width) *width = s->width;
    if (height) *height = s->height;
    if (depth) *depth = s->depth;
    return HBHIP_OK;
}

int hbhip_surface_set_ready_event(hbhip_surface *s, void *hip_event)
{
    if (!s) return HBHIP_ERR_ARG;
    std::lock_guard<std::mutex> lk(s->ctx->surface_lock);
    s->ready_event = (hipEvent_t)hip_event;
    return HBHIP_OK;
}

// `widen`: a depth-10 surface for an 8-bit frame (hbhip_frame_export_surface_widen)
static int surface_check(const hbhip_frame *fr, const hbhip_surface *s, bool widen = false)
{
    if (!bi_frame_ok(fr) || (widen && fr->depth != 8)) return HBHIP_ERR_UNSUPPORTED;
    if (s->depth != (widen ? 10 : fr->depth) || s->width != fr->width || s->height != fr->height) return HBHIP_ERR_UNSUPPORTED;
    if (s->ctx->device != fr->ctx->device) return HBHIP_ERR_ARG;
    return HBHIP_OK;
}

// the kernel is queued: the library's own reference on the surface until `done` has fired
static void surface_hold(hbhip_ctx *ctx, hbhip_surface *s, const std::shared_ptr<IdleMark> &done)
{
    hbhip_surface_retain(s);
    std::lock_guard<std::mutex> lk(ctx->surface_lock);
    ctx->surface_ops.push_back({s, done});
}

int hbhip_frame_import_surface_async(hbhip_frame *fr, hbhip_surface *src, void **token)
{
    if (!fr || !src || !token) return HBHIP_ERR_ARG;
    *token = nullptr;
    hbhip_ctx *ctx = fr->ctx;
    int rc = surface_check(fr, src);
    if (rc != HBHIP_OK) return rc;
    (void)hipSetDevice(ctx->device);
    surface_reap(ctx, false);
    std::shared_ptr<IdleMark> ready, earlier, m;
    hipEvent_t producer;
    {
        std::lock_guard<std::mutex> lk(src->ctx->surface_lock);
        ready = src->ready; producer = src->ready_event; earlier = src->read_idle;
    }
    rc = fill_frame(fr, "import (surface)", [&](hipStream_t up, hipEvent_t done) {
        hipError_t e = wait_mark(up, ready);
        if (e == hipSuccess && producer) e = hipStreamWaitEvent(up, producer, 0);
        if (e == hipSuccess) e = wait_mark(up, earlier);        // (another stream's import: an export then waits for ours alone)
        if (e != hipSuccess) return ctx->fail(e, "import: order behind the surface's contents");
        const int launched = hbhip_bi_surface_launch(ctx, up, false, src, fr);
        // the token's event ahead of the mark: once the library lets go of the surface (the mark has fired) the token is done
        return launched != HBHIP_OK ? launched : hip_rc(ctx, hipEventRecord(done, up), "import (surface)");
    }, token, &m);
    if (rc != HBHIP_OK) return rc;
    {
        std::lock_guard<std::mutex> lk(src->ctx->surface_lock);
        src->read_idle = m;
        if (producer && src->ready_event == producer)           // the first reader has waited for it: later ones wait for this one
        {
            src->ready_event = nullptr;
            src->ready = m;
        }
    }
    surface_hold(ctx, src, m);
    return HBHIP_OK;
}

int hbhip_frame_import_surface(hbhip_frame *fr, hbhip_surface *src)
{
    void *token = nullptr;
    const int rc = hbhip_frame_import_surface_async(fr, src, &token);
    return rc != HBHIP_OK ? rc : hbhip_ctx_upload_done(fr->ctx, token, 1);
}

// the merge into the surface; `widen`: an 8-bit frame into a depth-10 surface (bi_widen_merge_kernel)
static int export_surface(hbhip_frame *fr, hbhip_surface *dst, void **token, bool widen)
{
    if (!fr || !dst || !token) return HBHIP_ERR_ARG;
    *token = nullptr;
    hbhip_ctx *ctx = fr->ctx;
    int rc = surface_check(fr, dst, widen);
    if (rc != HBHIP_OK) return rc;
    (void)hipSetDevice(ctx->device);
    surface_reap(ctx, false);
    std::shared_ptr<IdleMark> ready, readers, m;
    hipEvent_t producer;
    {
        std::lock_guard<std::mutex> lk(dst->ctx->surface_lock);
        ready = dst->ready; producer = dst->ready_event; readers = dst->read_idle;
    }
    rc = drain_frame(fr, "export (surface)", [&](hipStream_t down) {
        hipError_t e = wait_mark(down, ready);                  // an earlier writer (another context's download stream; the clearing)
        if (e == hipSuccess && producer) e = hipStreamWaitEvent(down, producer, 0);
        if (e == hipSuccess) e = wait_mark(down, readers);
        if (e != hipSuccess) return ctx->fail(e, "export: order behind the surface's users");
        return widen ? hbhip_bi_widen_surface_launch(ctx, down, dst, fr) : hbhip_bi_surface_launch(ctx, down, true, dst, fr);
    }, [&](hipStream_t down) {                                // the surface's mark behind the token's event, as in the import
        m = record_mark(down);
        return m ? HBHIP_OK : ctx->fail(hipErrorOutOfMemory, "export (surface)");
    }, token);
    if (rc != HBHIP_OK) return rc;
    {
        std::lock_guard<std::mutex> lk(dst->ctx->surface_lock);
        dst->ready = m;
        dst->ready_event = nullptr;
        dst->read_idle.reset();
    }
    surface_hold(ctx, dst, m);
    return HBHIP_OK;
}

int hbhip_frame_export_surface_async(hbhip_frame *fr, hbhip_surface *dst, void **token)
{
    return export_surface(fr, dst, token, false);
}

int hbhip_frame_export_surface(hbhip_frame *fr, hbhip_surface *dst)
{
    void *token = nullptr;
    const int rc = hbhip_frame_export_surface_async(fr, dst, &token);
    return rc != HBHIP_OK ? rc : hbhip_frame_download_wait(fr, token);
}

int hbhip_frame_export_surface_widen_async(hbhip_frame *fr, hbhip_surface *dst, void **token)
{
    return export_surface(fr, dst, token, true);
}

int hbhip_frame_export_surface_widen(hbhip_frame *fr, hbhip_surface *dst)
{
    void *token = nullptr;
    const int rc = hbhip_frame_export_surface_widen_async(fr, dst, &token);
    return rc != HBHIP_OK ? rc : hbhip_frame_download_wait(fr, token);
}

int hbhip_ctx_bus_bytes(hbhip_ctx *ctx, uint64_t *h2d, uint64_t *d2h)
{
    if (!ctx) return HBHIP_ERR_ARG;
    if (h2d) *h2d = ctx->bus_h2d.load(std::memory_order_relaxed);
    if (d2h) *d2h = ctx->bus_d2h.load(std::memory_order_relaxed);
    return HBHIP_OK;
}

// ---- generic filter surface -------------------------------------------------
int hbhip_filter_push(hbhip_filter *f, const hbhip_host_frame *in, int64_t tag)
{
    if (!f || !in) return HBHIP_ERR_ARG;
    (void)hipSetDevice(f->ctx->device);
    DevPicture *pic = f->acquire_input();
    if (!pic) return HBHIP_ERR_NOMEM;
    pic->tag = tag;
    for (int c = 0; c < 3; c++) f->in_stride[c] = in->stride[c];
    f->in_is_dev = false;
    int rc = hbhip_copy_h2d(f->ctx, pic, in);          // returns when `in` has been consumed
    if (rc != HBHIP_OK)
    {
        f->abandon_input(pic);             // not submitted: back to its pool
        return rc;
    }
    return f->submit(pic);
}

int hbhip_filter_push_dev(hbhip_filter *f, const hbhip_dev_frame *in, int64_t tag)
{
    if (!f || !in) return HBHIP_ERR_ARG;
    (void)hipSetDevice(f->ctx->device);
    DevPicture *pic = f->acquire_input();
    if (!pic) return HBHIP_ERR_NOMEM;
    pic->tag = tag;
    for (int c = 0; c < 3; c++) f->in_stride[c] = in->stride[c];
    f->in_is_dev = true;
    int rc = hbhip_copy_d2d_in(f->ctx, pic, in);
    if (rc != HBHIP_OK)
    {
        f->abandon_input(pic);
        return rc;
    }
    return f->submit(pic);
}

// ---- frames in, frames out: the drop-ins of a device-resident run ---------------------------------------------
int hbhip_filter_use_frames(hbhip_filter *f)
{
    if (!f) return HBHIP_ERR_ARG;
    return f->use_frames();
}

// The frame becomes the filter's input picture - no copy - when the filter works on frames, the caller is the frame's
// only holder (a frame vfr has duplicated stays shared: it is copied, as before) and the geometry is the filter's; the
// filter keeps a reference of its own until it is done with the picture.
int hbhip_filter_push_frame(hbhip_filter *f, hbhip_frame *fr, int64_t tag)
{
    if (!f || !fr) return HBHIP_ERR_ARG;
    (void)hipSetDevice(f->ctx->device);
    int rc = hbhip_frame_use_on(fr, f->ctx);
    if (rc != HBHIP_OK) return rc;
    const PicGeometry &g = f->in_geo;
    const bool fits = fr->width == g.width && fr->height == g.height && fr->depth == g.depth && fr->lcw == g.log2_cw && fr->lch == g.log2_ch;
    if (!f->frames_mode || !fits || !retain_if_sole(fr))
    {
        hbhip_dev_frame d;
        hbhip_frame_describe(fr, &d, nullptr, nullptr);
        return hbhip_filter_push_dev(f, &d, tag);
    }
    DevPicture *pic = &fr->pic;
    pic->tag = tag;
    f->adopt_input(pic);
    for (int c = 0; c < 3; c++) f->in_stride[c] = pic->pitch[c];
    f->in_is_dev = true;
    return f->submit(pic);
}

// The next output as a frame: the picture itself when the filter works on frames (its reference passes to the caller), else
// a fresh frame the picture is copied into.  HBHIP_AGAIN: none pending.
int hbhip_filter_pull_frame(hbhip_filter *f, hbhip_frame **out, int64_t *tag)
{
    if (!f || !out) return HBHIP_ERR_ARG;
    *out = nullptr;
    (void)hipSetDevice(f->ctx->device);
    DevPicture *pic = f->pop_output();
    if (!pic) return HBHIP_AGAIN;
    if (tag) *tag = pic->tag;
    if (pic->frame)
    {
        *out = pic->frame;
        return HBHIP_OK;
    }
    const PicGeometry &g = f->out_geo;
    hbhip_frame *fr = nullptr;
    int rc = hbhip_frame_alloc(f->ctx, g.width, g.height, g.depth, g.log2_cw, g.log2_ch, &fr);
    if (rc == HBHIP_OK)
    {
        hbhip_dev_frame d;
        hbhip_frame_describe(fr, &d, nullptr, nullptr);
        rc = hbhip_copy_d2d_out(f->ctx, &d, pic);
        if (rc != HBHIP_OK) { hbhip_frame_release(fr); fr = nullptr; }
    }
    f->recycle_output(pic);
    *out = fr;
    return rc;
}

int hbhip_filter_pull(hbhip_filter *f, const hbhip_host_frame *out, int64_t *tag)
{
    if (!f || !out) return HBHIP_ERR_ARG;
    DevPicture *pic = f->pop_output();
    if (!pic) return HBHIP_AGAIN;
    if (tag) *tag = pic->tag;
    int rc = hbhip_copy_d2h(f->ctx, out, pic);         // returns when `out` is filled
    f->recycle_output(pic);
    return rc;
}

int hbhip_filter_pull_dev(hbhip_filter *f, const hbhip_dev_frame *out, int64_t *tag)
{
    if (!f || !out) return HBHIP_ERR_ARG;
    DevPicture *pic = f->pop_output();
    if (!pic) return HBHIP_AGAIN;
    if (tag) *tag = pic->tag;
    int rc = hbhip_copy_d2d_out(f->ctx, out, pic);
    f->recycle_output(pic);
    return rc;
}

int hbhip_filter_process_dev(hbhip_filter *f, const hbhip_dev_frame *in, int n_in, int64_t tag0,
                             const hbhip_dev_frame *out, int out_cap, int *n_out)
{
    if (!f || (n_in > 0 && !in) || !n_out) return HBHIP_ERR_ARG;
    (void)hipSetDevice(f->ctx->device);
    return f->process_dev_batch(in, n_in, tag0, out, out_cap, n_out);
}

// ---- pipelined host path ---------------------------------------------------------------
// push + pull of a one-in / one-out filter as ONE asynchronous submission: upload on the context's upload stream,
// the filter's kernels on the compute stream behind an event, the download on the download stream behind another.
// Nothing waits on the host; hbhip_filter_wait() later blocks on the oldest submission's last event only.  With two
// submissions in flight the H2D of frame n, the kernels of frame n-1 and the D2H of frame n-2 overlap - what the
// reference gets from keeping `threads` frames in flight (nlmeans.c:464-597, mt_frame_filter.c:45-237).
int hbhip_filter_submit_async(hbhip_filter *f, const hbhip_host_frame *in, const hbhip_host_frame *out, int64_t tag)
{
    if (!f || !in || !out) return HBHIP_ERR_ARG;
    hbhip_ctx *ctx = f->ctx;
    (void)hipSetDevice(ctx->device);
    DevPicture *pic = f->acquire_input();
    if (!pic) return HBHIP_ERR_NOMEM;
    DevPicture *o = f->acquire_output();
    if (!o)
    {
        f->abandon_input(pic);
        return HBHIP_ERR_UNSUPPORTED;              // not a one-in / one-out filter: use push / pull
    }
    SyncEvent ev(ctx), done(ctx);
    int rc = (ev && done) ? HBHIP_OK : HBHIP_ERR_NOMEM;
    if (rc == HBHIP_OK && !(host_planes_ok(pic, in) && host_planes_ok(o, out))) rc = HBHIP_ERR_ARG;
    auto fail = [&](int code) {
        // copies of the caller's `in` / `out` may be in flight: nothing of them may outlive this call
        if (ctx->up_stream) (void)hipStreamSynchronize(ctx->up_stream);
        (void)hipStreamSynchronize(ctx->stream);
        if (ctx->down_stream) (void)hipStreamSynchronize(ctx->down_stream);
        if (pic) f->abandon_input(pic);            // (already handed back once the kernels were queued)
        f->recycle_output(o);
        return code;
    };
    if (rc != HBHIP_OK) return fail(rc);
#define ASYNC_CHECK(expr) do { hipError_t e_ = (expr); if (e_ != hipSuccess) return fail(ctx->fail(e_, #expr)); } while (0)
    pic->tag = tag;
    for (int c = 0; c < 3; c++) f->in_stride[c] = in->stride[c];
    f->in_is_dev = false;
    ASYNC_CHECK(hbhip_pic_wait_idle(ctx->up(), pic));
    size_t moved;
    ASYNC_CHECK(queue_h2d(pic, in, false, ctx->up(), &moved));
    ASYNC_CHECK(hipEventRecord(ev, ctx->up()));
    ASYNC_CHECK(hipStreamWaitEvent(ctx->stream, ev, 0));
    rc = f->process_pair(pic, o);
    if (rc != HBHIP_OK) return fail(rc);
    hbhip_pic_release(pic, f->ctx);                // idle event behind the kernels that read it
    pic = nullptr;
    ASYNC_CHECK(hipEventRecord(ev, ctx->stream));
    ASYNC_CHECK(hipStreamWaitEvent(ctx->down(), ev, 0));
    ASYNC_CHECK(queue_d2h(out, o, false, ctx->down(), &moved));
    ASYNC_CHECK(hipEventRecord(done, ctx->down()));
#undef ASYNC_CHECK
    f->async_q.push_back({o, done.keep(), tag});
    return HBHIP_OK;
}

int hbhip_filter_wait(hbhip_filter *f, int64_t *tag)
{
    if (!f) return HBHIP_ERR_ARG;
    if (f->async_q.empty()) return HBHIP_AGAIN;
    (void)hipSetDevice(f->ctx->device);
    hbhip_filter::AsyncSlot s = f->async_q.front();
    f->async_q.pop_front();
    const hipError_t e = hipEventSynchronize(s.done);
    f->ctx->sync_ev_put(s.done);
    f->recycle_output(s.out);
    if (tag) *tag = s.tag;
    return e == hipSuccess ? HBHIP_OK : f->ctx->fail(e, "hipEventSynchronize(wait)");
}

int hbhip_filter_inflight(hbhip_filter *f)
{
    return f ? (int)f->async_q.size() : 0;
}

int hbhip_filter_flush(hbhip_filter *f)
{
    if (!f) return HBHIP_ERR_ARG;
    (void)hipSetDevice(f->ctx->device);
    return f->flush();
}

int hbhip_filter_pending(hbhip_filter *f)
{
    return f ? f->pending() : 0;
}

int hbhip_filter_defer(hbhip_filter *f, int on)
{
    if (!f) return HBHIP_ERR_ARG;
    (void)hipSetDevice(f->ctx->device);
    f->defer_launches(on != 0);
    return HBHIP_OK;
}

int hbhip_filter_kick(hbhip_filter *f)
{
    if (!f) return HBHIP_ERR_ARG;
    (void)hipSetDevice(f->ctx->device);
    return f->kick();
}

void hbhip_filter_destroy(hbhip_filter *f)
{
    if (!f) return;
    (void)hipSetDevice(f->ctx->device);
    while (!f->async_q.empty()) (void)hbhip_filter_wait(f, nullptr);
    (void)hipStreamSynchronize(f->ctx->stream);
    delete f;
}

hbhip_ctx *hbhip_filter_context(hbhip_filter *f)
{
    return f ? f->ctx : nullptr;
}

int hbhip_filter_out_geometry(hbhip_filter *f, int *width, int *height)
{
    if (!f) return HBHIP_ERR_ARG;
    if (width) *width = f->out_geo.width;
    if (height) *height = f->out_geo.height;
    return HBHIP_OK;
}

} // extern "C"
