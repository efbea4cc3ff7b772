/* hbhip.h — C ABI of libhbhip.so: libhb's per-pixel video-filter hot path as
 * hand-written HIP kernels for AMD Instinct MI355X (gfx950 / CDNA4).
 *
 * This is the drop-in boundary.  libhb stays C: each HIP-backed
 * hb_filter_object_t (handbrake_amd/libhb/<filter>_hip.c) keeps the reference's
 * init/work/close surface (libhb/handbrake/common.h:1670-1711) and only
 * translates hb_buffer_t <-> plane pointers before calling the functions below.
 * Plain pointers and sizes only; no C++ or torch types cross this boundary; no
 * exception crosses it either.  Every entry point names the reference
 * interface it replaces (paths relative to /root/reference/libhb).
 *
 * Conventions
 *   - return 0 (HBHIP_OK) on success, HBHIP_AGAIN (1) when a pull has no frame
 *     ready yet, negative HBHIP_ERR_* on failure (hbhip_strerror()).
 *   - the caller owns host memory; the library owns device memory and, unless
 *     one is adopted (hbhip_ctx_create_on_stream), one hipStream_t per context.
 *   - one caller thread per filter instance (that is what filter_loop gives,
 *     work.c:2527-2600); distinct instances / contexts are independent.
 *   - a missing GPU is an error (HBHIP_ERR_NODEVICE): there is NO CPU fallback
 *     inside this library.  libhb falls back by re-inserting its CPU filter
 *     when a HIP filter's init() fails (work.c:1861-1868 semantics).
 */
#ifndef HBHIP_H
#define HBHIP_H

#include <stdint.h>
#include <stddef.h>

#ifdef __cplusplus
extern "C" {
#endif

#define HBHIP_OK               0
#define HBHIP_AGAIN            1
#define HBHIP_ERR_NODEVICE    (-1)
#define HBHIP_ERR_HIP         (-2)
#define HBHIP_ERR_ARG         (-3)
#define HBHIP_ERR_NOMEM       (-4)
#define HBHIP_ERR_UNSUPPORTED (-5)
#define HBHIP_ERR_STATE       (-6)

#define HBHIP_ABI_VERSION 1

typedef struct hbhip_ctx    hbhip_ctx;
typedef struct hbhip_filter hbhip_filter;

/* A planar picture living in HOST memory: what hb_buffer_t.plane[] describes
 * (handbrake/internal.h:137-144).  stride in bytes. */
typedef struct hbhip_host_frame
{
    uint8_t *plane[3];
    int      stride[3];
} hbhip_host_frame;

/* A planar picture living in DEVICE memory (HBM).  Used by the device-resident
 * hand-off between adjacent HIP filters (the reference's
 * precedent is hb_buffer_t.storage_type = COREMEDIA, internal.h:152-153) and
 * by bench.py, whose inputs are resident in HBM before the timed region. */
typedef struct hbhip_dev_frame
{
    void *plane[3];
    int   stride[3];
} hbhip_dev_frame;

/* ---- library / context ------------------------------------------------------ */
int         hbhip_abi_version(void);
int         hbhip_device_count(void);                 /* hb_get_cpu_count() analogue, ports.c:292 */
const char *hbhip_strerror(int code);
int         hbhip_ctx_create(int device, hbhip_ctx **out);
/* Adopt an existing hipStream_t (passed as void*) instead of creating one. */
int         hbhip_ctx_create_on_stream(int device, void *hip_stream, hbhip_ctx **out);
void        hbhip_ctx_destroy(hbhip_ctx *ctx);
int         hbhip_ctx_sync(hbhip_ctx *ctx);           /* hipStreamSynchronize */
const char *hbhip_ctx_last_error(hbhip_ctx *ctx);     /* text of the last HIP failure */
int         hbhip_ctx_device_name(hbhip_ctx *ctx, char *buf, int len);
int         hbhip_ctx_device_index(hbhip_ctx *ctx);   /* the `device` it was created on; < 0 on a NULL context */
/* The on-box HBM ceiling: a float4 copy kernel over two buffers of `bytes` each (take them well past the 256 MB Infinity
 * Cache), best of `iters` timed passes with HIP events; *gbps = (read + write) bytes / time.  bench.py reports roofline
 * fractions against this as well as against the nominal 8 TB/s. */
int         hbhip_ctx_copy_bandwidth(hbhip_ctx *ctx, size_t bytes, int iters, double *gbps);

/* Per-kernel timing with HIP events on the context's stream (off by default).
 * When enabled every kernel launch is bracketed by two events; stats are read
 * back per kernel name.  bench.py derives roofline.achieved from these. */
int  hbhip_ctx_profile_enable(hbhip_ctx *ctx, int on);
int  hbhip_ctx_profile_reset(hbhip_ctx *ctx);
int  hbhip_ctx_profile_count(hbhip_ctx *ctx);         /* distinct kernel names seen (syncs) */
int  hbhip_ctx_profile_get(hbhip_ctx *ctx, int idx, char *name, int name_len,
                           int64_t *launches, double *total_ms);
/* Two user events on the stream, for whole-region timing. */
int  hbhip_ctx_mark(hbhip_ctx *ctx, int slot);        /* slot 0..7: record event */
int  hbhip_ctx_elapsed_ms(hbhip_ctx *ctx, int slot_a, int slot_b, double *ms); /* syncs slot_b */

/* Device memory helpers (thin hipMalloc/hipFree/hipMemcpy wrappers so a C host
 * never needs the HIP headers). */
/* Page-locked host memory (hipHostMalloc): frame buffers allocated from it make the H2D / D2H
 * copies of hbhip_filter_push / pull true DMA transfers instead of staged pageable copies.
 * What fifo.c's buffer pools would allocate from in a HIP build (hb_buffer_init, fifo.c:358-457). */
int  hbhip_host_alloc(size_t bytes, void **out);
void hbhip_host_free(void *p);
int  hbhip_dev_alloc(hbhip_ctx *ctx, size_t bytes, void **out);
int  hbhip_dev_free(hbhip_ctx *ctx, void *p);
int  hbhip_dev_upload(hbhip_ctx *ctx, void *dst, const void *src, size_t bytes);
int  hbhip_dev_download(hbhip_ctx *ctx, void *dst, const void *src, size_t bytes);
/* Bytes of device and of page-locked host memory the library itself holds right now, process-wide (contexts, pools,
 * filters; not what hbhip_host_alloc / hbhip_dev_alloc handed to the caller, nor memory a surface only wraps).  An object
 * gives back what it holds itself when it is destroyed; what its calls grew on the context - the frame and surface pools,
 * the staging buffers - stays with the context until hbhip_ctx_destroy, so a second create / use / destroy of the same
 * kind ends at the counts the first ended at, and a destroyed context at those from before it was made.  A create that
 * is refused leaves both counts as they were. */
int  hbhip_mem_live(size_t *device_bytes, size_t *pinned_bytes);

/* ---- device-resident frames (hand-off between adjacent HIP filters) -----------------
 * The reference's GPU precedent keeps frames on the device between its Metal filters
 * by giving hb_buffer_t a storage_type (COREMEDIA, internal.h:152-153) and bracketing the
 * run of GPU filters with an adapter (HB_FILTER_ADAPTER_VT, platform/macosx/adapter_vt.c).
 * hbhip_frame is the HIP equivalent of the CVPixelBuffer behind such a buffer: a
 * reference-counted picture in HBM, recycled through a per-context pool. */
typedef struct hbhip_frame hbhip_frame;
int  hbhip_frame_alloc(hbhip_ctx *ctx, int width, int height, int depth,
                       int log2_chroma_w, int log2_chroma_h, hbhip_frame **out);
void hbhip_frame_retain(hbhip_frame *fr);
void hbhip_frame_release(hbhip_frame *fr);            /* back to the pool at refcount 0 */
/* A frame may be read and written on more than one context of its GPU (a job with more than one HIP stream,
 * libhb/hbhip_registry.c).  Before a context queues work on a frame it takes it through hbhip_frame_use_on: its stream
 * waits for the frame's contents (the ready mark, nothing else of another stream) and the context becomes the frame's
 * current user.  The rule in full, idle marks included: hbhip_core.hip, "How frames are ordered". */
int  hbhip_frame_use_on(hbhip_frame *fr, hbhip_ctx *ctx);
int  hbhip_frame_refs(hbhip_frame *fr);               /* holders right now; 1 = the caller is the only one (it may write in place) */
int  hbhip_frame_describe(hbhip_frame *fr, hbhip_dev_frame *out, int *width, int *height);
hbhip_ctx *hbhip_frame_context(hbhip_frame *fr);      /* the context (device, stream) whose pool the frame belongs to */
int  hbhip_frame_copy(hbhip_frame *dst, hbhip_frame *src);                  /* same geometry, one GPU; D2D on dst's stream (use_on) */
int  hbhip_frame_upload(hbhip_frame *fr, const hbhip_host_frame *src);      /* H2D, returns when src is consumed */
int  hbhip_frame_download(hbhip_frame *fr, const hbhip_host_frame *dst);    /* D2H, synchronous */
/* The pipelined H2D: the copy is queued on the context's upload stream and the call returns; `src` must stay valid until
 * hbhip_ctx_upload_done(ctx, token, block) has answered HBHIP_OK (HBHIP_AGAIN: not yet; block != 0 waits).  The frame's
 * ready mark is the copy itself. */
int  hbhip_frame_upload_async(hbhip_frame *fr, const hbhip_host_frame *src, void **token);
int  hbhip_ctx_upload_done(hbhip_ctx *ctx, void *token, int block);
/* Whoever writes a frame marks its contents complete: the ready mark goes on the stream of the frame's current user
 * (the context that last took it through hbhip_frame_use_on, else its owner), and readers - a download among them -
 * wait for that point only, not for what other filter threads have queued since.  The pipelined D2H: queue the copy on
 * the download stream and return; `dst` and the frame must stay valid until hbhip_frame_download_wait(fr, token) has
 * returned.  A few in flight keep the bus busy (the download adapter). */
int  hbhip_frame_mark_ready(hbhip_frame *fr);
int  hbhip_frame_download_async(hbhip_frame *fr, const hbhip_host_frame *dst, void **token);
int  hbhip_frame_download_wait(hbhip_frame *fr, void *token);
/* Biplanar host pictures, NV12 and P010LE (what AMD's decoder hands out and its encoder takes in): plane 0 is luma,
 * plane 1 interleaved Cb Cr.  The frame itself stays planar - `fr` is a planar 4:2:0 frame of depth 8 (NV12) or 10 (P010LE:
 * samples >> 6 on the way in, << 6 on the way out) - and the repack is a kernel next to the copy, through a staging buffer
 * the context keeps.  The async forms follow the ordering rule above: the split runs behind the H2D copy and is the
 * frame's ready mark, the merge waits for the ready mark and the D2H copy for the merge; their tokens are finished with
 * hbhip_ctx_upload_done / hbhip_frame_download_wait.  HBHIP_ERR_UNSUPPORTED: another depth, a frame that is not 4:2:0, a
 * width or height below 2.
 * An upload reads min(stride, row bytes rounded up to 64) bytes of EVERY row of `src`, the last row of each plane
 * included - the row padding travels with the samples, as with hbhip_frame_upload - so each plane of `src` must be
 * readable for stride * rows bytes.  A download writes the samples of each row only, or, where `dst` has the layout of
 * hb_frame_buffer_init (64-byte rows, plane 1 right behind plane 0), the whole rows in one copy. */
typedef struct hbhip_host_biplanar { uint8_t *plane[2]; int stride[2]; } hbhip_host_biplanar;
int  hbhip_frame_upload_biplanar(hbhip_frame *fr, const hbhip_host_biplanar *src);
int  hbhip_frame_download_biplanar(hbhip_frame *fr, const hbhip_host_biplanar *dst);
int  hbhip_frame_upload_biplanar_async(hbhip_frame *fr, const hbhip_host_biplanar *src, void **token);
int  hbhip_frame_download_biplanar_async(hbhip_frame *fr, const hbhip_host_biplanar *dst, void **token);
/* P010LE from an 8-bit frame - what a 10-bit hardware encoder is fed from an 8-bit title: `fr` is a planar 4:2:0 frame of
 * depth 8, `dst` a P010LE host picture of its size, and every sample t of the three planes becomes the 16-bit word
 * t | t << 8 (the byte twice: libswscale's unscaled yuv420p -> p010le), widened inside the merge kernel.
 * Ordering, the token and what is written of `dst` are hbhip_frame_download_biplanar's, with P010LE's row bytes
 * (2 * width, 4 * ceil(width / 2)).  HBHIP_ERR_UNSUPPORTED: a frame that is not 4:2:0 at depth 8, a width or height below
 * 2; HBHIP_ERR_ARG: a plane that is missing or a stride below the row bytes.  The entry points above keep refusing a
 * frame whose depth is not the picture's. */
int  hbhip_frame_download_widen(hbhip_frame *fr, const hbhip_host_biplanar *dst);
int  hbhip_frame_download_widen_async(hbhip_frame *fr, const hbhip_host_biplanar *dst, void **token);   /* finished with hbhip_frame_download_wait */
/* A packed 32-bit RGB host picture from an 8-bit frame - what hb_get_preview's `format=bgra` asks for behind a device run:
 * `fr` is a planar 4:2:0 frame of depth 8 and even size, `dst` a one-plane picture of its size, 4 bytes a pixel in the
 * memory order `order` names, alpha 255.  The arithmetic is libswscale's unscaled yuv420p -> bgra path in its C form,
 * restated (chroma nearest, every chroma term a whole number of luma steps into a clipped luma ramp; DESIGN 4.6.11,
 * tests/rgb32_model.py), done in one kernel ahead of the copy.  `matrix` is an HB_COLR_MAT_* number (2, unspecified, is
 * taken as BT.601 as swscale does), `full_range` the frame's range; the result is full-range RGB.  Ordering, the staging
 * buffer and the token are hbhip_frame_download_biplanar's; 4 * width bytes of each of `dst`'s rows are written and nothing
 * else.  HBHIP_ERR_UNSUPPORTED: a frame that is not 4:2:0 at depth 8, an odd width or height, a size under 2 x 2, a matrix
 * with no coefficient row (RGB, YCgCo, ICtCp, the chroma-derived ones); HBHIP_ERR_ARG: a stride below 4 * width, an order
 * outside the enum. */
enum { HBHIP_RGB32_BGRA, HBHIP_RGB32_RGBA, HBHIP_RGB32_ARGB, HBHIP_RGB32_ABGR };
int  hbhip_frame_download_rgb32(hbhip_frame *fr, uint8_t *dst, int stride, int order, int matrix, int full_range);
int  hbhip_frame_download_rgb32_async(hbhip_frame *fr, uint8_t *dst, int stride, int order, int matrix, int full_range, void **token);   /* finished with hbhip_frame_download_wait */

/* ---- device surfaces: NV12 / P010LE pictures that already are, or stay, in HBM ------------------------------------------
 * What AMD's decoder hands out and AMF / VCE take in, without the host copy: a surface has a pitch of its own per plane
 * (any multiple of 16 that holds the row), rows padded as its maker likes, and its two planes in one allocation or two.
 * Import repacks a surface into a planar 4:2:0 frame (depth 8: NV12, depth 10: P010LE, samples >> 6), export the other way
 * (<< 6, low six bits zero), one kernel each (csrc/biplanar.hip), nothing over the bus.
 *  * Import writes every byte of the frame's rows, row padding included: what the surface's row holds as far as its pitch
 *    reaches, zero beyond.  It reads nothing outside pitch * rows of either plane.
 *  * Export writes the first align16(row bytes) bytes of each of the height / ceil(height / 2) sample rows (row bytes:
 *    width * bps, and 2 * ceil(width / 2) * bps) and nothing else of the surface.
 * Ordering is the frames' (hbhip_core.hip, "How frames are ordered"): an import runs on the frame's context's upload
 * stream behind the surface's contents - the last export into it, or the event of hbhip_surface_set_ready_event - and is
 * the frame's ready mark; an export runs on the download stream behind the frame's contents and every earlier import of the
 * surface, and is the surface's ready mark.  Nothing waits on the host; the library keeps a reference of its own on the
 * surface from the call until the queued kernel has finished.
 * Refused before anything is queued - HBHIP_ERR_UNSUPPORTED: a depth other than 8 / 10, a frame that is not 4:2:0, a
 * surface of another depth or size than the frame, a width or height below 2, a plane address or pitch that is no
 * multiple of 16; HBHIP_ERR_ARG: a pitch below the row bytes, planes that overlap, a surface of another GPU than the frame. */
typedef struct hbhip_dev_surface { void *plane[2]; int pitch[2]; } hbhip_dev_surface;   /* NV12 (depth 8) / P010LE (depth 10), device memory */
typedef struct hbhip_surface hbhip_surface;                                             /* reference-counted */
/* library-owned, recycled through a per-context pool like frames.  pitch_align >= 16 and a power of two; rows_align >= 1:
 * plane 1 starts at pitch * align(height, rows_align).  (256, 16) is what a video engine's allocator gives. */
int  hbhip_surface_alloc(hbhip_ctx *ctx, int width, int height, int depth, int pitch_align, int rows_align, hbhip_surface **out);
/* caller-owned memory (a decoder's picture): release(opaque) is called when the last reference has gone and nothing queued
 * reads or writes the memory any more - from whichever call of the library notices that first (the token calls,
 * hbhip_ctx_sync, the surface calls) */
int  hbhip_surface_wrap(hbhip_ctx *ctx, const hbhip_dev_surface *mem, int width, int height, int depth,
                        void (*release)(void *), void *opaque, hbhip_surface **out);
void hbhip_surface_retain(hbhip_surface *s);
void hbhip_surface_release(hbhip_surface *s);
int  hbhip_surface_describe(hbhip_surface *s, hbhip_dev_surface *out, int *width, int *height, int *depth);
/* a wrapped surface whose producer is still running: the hipEvent_t (as void*) the first reader has to wait for */
int  hbhip_surface_set_ready_event(hbhip_surface *s, void *hip_event);
int  hbhip_frame_import_surface(hbhip_frame *fr, hbhip_surface *src);
int  hbhip_frame_import_surface_async(hbhip_frame *fr, hbhip_surface *src, void **token);   /* finished with hbhip_ctx_upload_done */
int  hbhip_frame_export_surface(hbhip_frame *fr, hbhip_surface *dst);
int  hbhip_frame_export_surface_async(hbhip_frame *fr, hbhip_surface *dst, void **token);   /* finished with hbhip_frame_download_wait */
/* The export of a planar 4:2:0 frame of depth 8 into a DEPTH-10 surface of its size, every sample t as t | t << 8
 * (hbhip_frame_download_widen's arithmetic, one kernel, nothing over the bus).  What it writes of the surface and how it is
 * ordered are hbhip_frame_export_surface's: [0, align16(row bytes)) of the sample rows, behind the frame's contents and every
 * earlier import of the surface, and it is the surface's ready mark.  Refused before anything is queued -
 * HBHIP_ERR_UNSUPPORTED: a frame that is not 4:2:0 at depth 8, a surface that is not depth 10 or is of another size, a width
 * or height below 2; HBHIP_ERR_ARG: a surface of another GPU than the frame (pitches, addresses and overlap: what
 * hbhip_surface_wrap admits). */
int  hbhip_frame_export_surface_widen(hbhip_frame *fr, hbhip_surface *dst);
int  hbhip_frame_export_surface_widen_async(hbhip_frame *fr, hbhip_surface *dst, void **token);   /* finished with hbhip_frame_download_wait */
/* bytes the frame upload / download entry points (hbhip_frame_upload*, hbhip_frame_download*) have queued over the bus on
 * this context */
int  hbhip_ctx_bus_bytes(hbhip_ctx *ctx, uint64_t *h2d, uint64_t *d2h);

/* ---- frames in, frames out: what a drop-in inside a device-resident run uses instead of push_dev / pull_dev -----------
 * hbhip_filter_use_frames(f) (once, before the first push): the filter's pictures are frames of its context's pool.
 * hbhip_filter_push_frame: the frame becomes the filter's input picture without a copy (the filter holds a reference of its
 * own; a frame with other holders, or of another geometry, is copied as hbhip_filter_push_dev would).
 * hbhip_filter_pull_frame: the next output AS a frame (its one reference passes to the caller); HBHIP_AGAIN when none. */
int hbhip_filter_use_frames(hbhip_filter *f);
int hbhip_filter_push_frame(hbhip_filter *f, hbhip_frame *fr, int64_t tag);
int hbhip_filter_pull_frame(hbhip_filter *f, hbhip_frame **out, int64_t *tag);

/* ---- generic streaming surface of a filter instance ---------------------------
 * Mirrors hb_filter_object_t.work (common.h:1682-1685): push one input frame,
 * pull zero or more output frames, flush at EOF, destroy in close().
 * `tag` travels with the frame (the host filter keeps hb_buffer_t props by tag). */
int  hbhip_filter_push(hbhip_filter *f, const hbhip_host_frame *in, int64_t tag);
int  hbhip_filter_push_dev(hbhip_filter *f, const hbhip_dev_frame *in, int64_t tag);
int  hbhip_filter_pull(hbhip_filter *f, const hbhip_host_frame *out, int64_t *tag);
int  hbhip_filter_pull_dev(hbhip_filter *f, const hbhip_dev_frame *out, int64_t *tag);
/* Batch form of push_dev/pull_dev: push n_in frames (tags tag0, tag0+1, ...) and
 * pull every frame that becomes ready into out[0..out_cap); *n_out = frames
 * written.  One ABI crossing per batch instead of two per frame. */
int  hbhip_filter_process_dev(hbhip_filter *f, const hbhip_dev_frame *in, int n_in, int64_t tag0,
                              const hbhip_dev_frame *out, int out_cap, int *n_out);
/* Pipelined form of push + pull for filters that make one frame from one frame: queue the upload of `in`, the
 * filter, and the download into `out`, and return at once.  `in` and `out` must stay valid until hbhip_filter_wait()
 * has returned this submission (they finish in submission order; `tag` comes back with it).  Two or three submissions
 * in flight overlap H2D, kernels and D2H - the role `threads` frames in flight play in the reference
 * (nlmeans.c:464-597, mt_frame_filter.c:45-237).  HBHIP_ERR_UNSUPPORTED: not such a filter, use push / pull. */
int  hbhip_filter_submit_async(hbhip_filter *f, const hbhip_host_frame *in, const hbhip_host_frame *out, int64_t tag);
int  hbhip_filter_wait(hbhip_filter *f, int64_t *tag);      /* oldest submission done; HBHIP_AGAIN when none is in flight */
int  hbhip_filter_inflight(hbhip_filter *f);
int  hbhip_filter_flush(hbhip_filter *f);             /* input ended (HB_BUF_FLAG_EOF) */
int  hbhip_filter_pending(hbhip_filter *f);           /* frames a pull would return now */
/* Batching across work() calls: with defer on, a filter that gathers frames for a common launch (decomb / EEDI2:
 * the fields of several frames per launch, NLMeans) launches nothing until hbhip_filter_kick() - the frames pushed
 * meanwhile are pending but NOT complete until the kick has been given.  What libhb's filters do with `threads`
 * frames in flight (nlmeans.c:464-597): answer HB_FILTER_DELAY for a few frames, then emit a burst. */
int  hbhip_filter_defer(hbhip_filter *f, int on);
int  hbhip_filter_kick(hbhip_filter *f);
void hbhip_filter_destroy(hbhip_filter *f);
/* Output geometry (cropscale / rotate change it; init->geometry, cropscale.c:170-178). */
int  hbhip_filter_out_geometry(hbhip_filter *f, int *width, int *height);
hbhip_ctx *hbhip_filter_context(hbhip_filter *f);     /* the context the instance was created on */

/* ---- a run of adjacent HIP filters fused into one object ------------------------------------
 * The reference merges runs of libavfilter-backed filters into one filter object whose work()
 * pushes a frame through the whole graph (hb_avfilter_combine, hbavfilter.c:510-622); this is the
 * same for a run of HIP filters: one caller thread, pictures handed from stage to stage in HBM by
 * pointer (no copies between stages), a batch of frames walked stage by stage so that batching
 * stages (NLMeans) cover the batch in one launch.  The chain BORROWS the filters: consecutive
 * geometries must match, and after hbhip_chain_destroy the caller destroys them LAST STAGE FIRST
 * (a stage may still hold pictures of the stage before it).
 * Stages created on `ctx` all run on its stream.  Stages created on contexts of their own (same
 * device) run on THEIR streams - libhb's one thread per filter (work.c:2527-2600) as one stream per
 * filter: the chain orders each hand-over with an event, so the first stages start on the next batch
 * while the last ones finish this one.  Input frames must be complete in `ctx`'s stream order when
 * hbhip_chain_process_dev is called; output frames are complete after hbhip_chain_sync().
 * pic_flags / combed: per input frame, what hbhip_decomb_push carries (NULL = 0); out_tags: the
 * tag of each output frame (decomb stages shift tags as documented at hbhip_decomb_push). */
typedef struct hbhip_chain hbhip_chain;
int  hbhip_chain_create(hbhip_ctx *ctx, hbhip_filter *const *stages, int n_stages, hbhip_chain **out);
int  hbhip_chain_process_dev(hbhip_chain *c, const hbhip_dev_frame *in, const int *pic_flags, const int *combed,
                             int n_in, int64_t tag0, const hbhip_dev_frame *out, int64_t *out_tags, int out_cap,
                             int *n_out);
int  hbhip_chain_flush_dev(hbhip_chain *c, const hbhip_dev_frame *out, int64_t *out_tags, int out_cap, int *n_out);
int  hbhip_chain_pending(hbhip_chain *c);             /* finished frames waiting for room in `out` */
int  hbhip_chain_sync(hbhip_chain *c);                /* wait for every stage's stream */
void hbhip_chain_destroy(hbhip_chain *c);

/* ---- NLMeans  (replaces nlmeans.c:223-419 init tables + nlmeans_template.c:545-717) */
#define HBHIP_NLMEANS_FRAMES_MAX 32                   /* NLMEANS_FRAMES_MAX, nlmeans.c:87 */
typedef struct hbhip_nlmeans_params
{
    /* per plane Y,Cb,Cr, already cascaded/sanitised exactly as nlmeans.c:306-343 */
    double strength[3];
    double origin_tune[3];
    int    patch_size[3];
    int    range[3];
    int    nframes[3];
    int    prefilter[3];
    /* tables built on the host with libm, as nlmeans.c:345-358 does */
    float  exptable[3][128];
    float  weight_fact_table[3];
    int    diff_max[3];
} hbhip_nlmeans_params;

int hbhip_nlmeans_create(hbhip_ctx *ctx, const hbhip_nlmeans_params *p,
                         int width, int height, int depth,
                         int log2_chroma_w, int log2_chroma_h,
                         hbhip_filter **out);
/* Max frames processed per kernel launch when several are queued (default 8). */
int hbhip_nlmeans_set_batch(hbhip_filter *f, int frames);

/* What a frame's launches are: one per distinct patch size among the denoised planes, in ascending patch size.  A
 * launch runs ONE kernel form for all its planes - the widest tile pitch and the most general index form any of them
 * needs.  hbhip_nlmeans_plan() is what the filter itself dispatches from (csrc/nlmeans.hip); it needs no device and
 * no context. */
typedef struct hbhip_nlmeans_launch
{
    int      patch_size;    /* 0 in the generic kernels' entries of hbhip_nlmeans_forms() (any size, a kernel argument) */
    int      planes;        /* bit c: plane c is filtered by this launch */
    int      generic;       /* nlmeans_generic_kernel: every patch size but 3 / 5 / 7 / 9; the fields down to origin_f32 are 0 */
    int      wide;          /* the 16-bit sample kernels (depth 10 / 12) */
    int      fast;          /* the table-index form: 0 gated float, 1 float clamp, 2 integer multiply-high, 3 paired displacements */
    int      pitch;         /* tile pitch in dwords: 36 | 44 (bytes), 76 | 84 (16-bit samples) */
    int      pre;           /* prefiltered compare planes: twice the staged tiles */
    int      pairs;         /* fast 3: how many of frame 0's four displacement pairs share their distances, else 0 */
    int      origin_f32;    /* fast 3 at 8 bits: the origin term in single precision (every origin_tune of the launch is 1) */
    int      max_rh;        /* the largest search half-range of the launch */
    int      cmp_rows;      /* rows of a staged tile (0: generic) */
    int      job_arith;     /* a tile's job by arithmetic (1) or by a search of the job table (0) */
    int      tile_w, tile_h; /* output pixels of a workgroup's tile */
    unsigned lds_bytes;     /* dynamic LDS of the launch */
    /* the table-index constants of each plane of the launch (-1 / 0 / 0 for a plane that is not in it): the smallest patch
     * distance whose index is 127, or -1 where the table does not allow the clamp (then the launch is form 0); the
     * multiplier of the integer index, or 0 where there is none, and its shift (an 8-bit launch with a multiplier that
     * needs a shift, or without one, is form 1) */
    int      diff_cap[3];
    unsigned imul4[3];
    int      ishift[3];
} hbhip_nlmeans_launch;

/* The launches of one frame for these parameters and this geometry, at most 3; *n = how many.  Returns what
 * hbhip_nlmeans_create() would: HBHIP_ERR_ARG / HBHIP_ERR_UNSUPPORTED for parameters or planes the filter declines. */
int hbhip_nlmeans_plan(const hbhip_nlmeans_params *p, int width, int height, int depth,
                       int log2_chroma_w, int log2_chroma_h, hbhip_nlmeans_launch launches[3], int *n);
/* Every kernel instantiation the dispatcher holds, as the fields of a launch that select it (patch_size ... origin_f32);
 * writes at most `cap` entries, returns how many there are. */
int hbhip_nlmeans_forms(hbhip_nlmeans_launch *forms, int cap);

/* ---- Lapsharp  (replaces lapsharp_8, lapsharp.c:125-182) ------------------------ */
typedef struct hbhip_lapsharp_params
{
    double strength[3];   /* sanitised 0..1.5 (lapsharp.c:304-305)                         */
    int    kernel[3];     /* 0 lap, 1 isolap, 2 log, 3 isolog (lapsharp.c:80-86)           */
} hbhip_lapsharp_params;
int hbhip_lapsharp_create(hbhip_ctx *ctx, const hbhip_lapsharp_params *p, int width, int height,
                          int depth, int log2_chroma_w, int log2_chroma_h, hbhip_filter **out);

/* ---- Unsharp / chroma smooth (replace unsharp_8 unsharp.c:89-173 and
 *      chroma_smooth_8 chroma_smooth.c:87-172) ------------------------------------- */
typedef struct hbhip_blur_params
{
    int amount[3];        /* (int)(strength * 65536.0); 0 = plane is copied (unsharp.c:258) */
    int size[3];          /* odd 3..15 (unsharp.c:251-254)                                 */
} hbhip_blur_params;
int hbhip_unsharp_create(hbhip_ctx *ctx, const hbhip_blur_params *p, int width, int height,
                         int depth, int log2_chroma_w, int log2_chroma_h, hbhip_filter **out);
int hbhip_chroma_smooth_create(hbhip_ctx *ctx, const hbhip_blur_params *p, int width, int height,
                               int depth, int log2_chroma_w, int log2_chroma_h, hbhip_filter **out);

/* ---- hqdn3d (replaces hqdn3d_denoise_spatial/temporal/depth, denoise.c:102-201) --- */
typedef struct hbhip_hqdn3d_params
{
    /* coef[2*c] spatial, coef[2*c+1] temporal table of plane c, each built on the host
     * exactly as hqdn3d_precalc_coef builds it (denoise.c:78-94; entry 0 = strength != 0) */
    int16_t coef[6][8192];
} hbhip_hqdn3d_params;
int hbhip_hqdn3d_create(hbhip_ctx *ctx, const hbhip_hqdn3d_params *p, int width, int height,
                        int depth, int log2_chroma_w, int log2_chroma_h, hbhip_filter **out);

/* ---- Decomb (replaces decomb.c:495-612 frame logic + decomb_template.c:579-898
 *      line filters + eedi2_template.c passes) -------------------------------------- */
typedef struct hbhip_decomb_params
{
    int mode;                       /* MODE_DECOMB_* bits, decomb.h:13-18                  */
    int parity;                     /* -1 = from picture flags (decomb.c:519-528)          */
    /* EEDI2 (decomb.c:234-243) */
    int magnitude_threshold, variance_threshold, laplacian_threshold;
    int dilation_threshold, erosion_threshold, noise_threshold;
    int maximum_search_distance, post_processing;
} hbhip_decomb_params;
int hbhip_decomb_create(hbhip_ctx *ctx, const hbhip_decomb_params *p, int width, int height,
                        int depth, int log2_chroma_w, int log2_chroma_h, hbhip_filter **out);
/* push with the per-buffer state decomb looks at: s.flags (PIC_FLAG_*) and
 * s.combed (HB_COMB_*, set upstream by comb detect).  Pulled tags are
 * (input tag << 1) | field_index, field_index = 1 for the second frame of a bob pair. */
int hbhip_decomb_push(hbhip_filter *f, const hbhip_host_frame *in, int64_t tag, int pic_flags, int combed);
int hbhip_decomb_push_dev(hbhip_filter *f, const hbhip_dev_frame *in, int64_t tag, int pic_flags, int combed);
int hbhip_decomb_push_frame(hbhip_filter *f, hbhip_frame *fr, int64_t tag, int pic_flags, int combed);   /* as hbhip_filter_push_frame */
/* The reference's "Deinterlace" filter = FFmpeg yadif as deinterlace_init configures it
 * (deinterlace.c:72-143): spatial_check 0 = send_*_nospatial, bob = send_field (two frames per
 * input), selective = deint=interlaced (only frames whose s.combed is set), parity -1 / 0 (tff) /
 * 1 (bff).  Frames go in with hbhip_decomb_push[_dev] (flags + combed) and come out like decomb's.
 * Arithmetic of vf_yadif.c, parity unpinned (oracle/decomb_oracle.c:orc_yadif_ff_plane). */
int hbhip_yadif_create(hbhip_ctx *ctx, int spatial_check, int bob, int selective, int parity,
                       int width, int height, int depth, int log2_chroma_w, int log2_chroma_h,
                       hbhip_filter **out);
/* The reference's "Bwdif" filter = FFmpeg bwdif as deinterlace_init configures it (deinterlace.c:46, 72-143; the
 * spatial bit is yadif-only, :98-122): bob = send_field, selective = deint=interlaced, parity as above.  Same
 * push / pull surface as hbhip_yadif_create.  Arithmetic of vf_bwdif.c, parity unpinned
 * (oracle/decomb_oracle.c:orc_bwdif_plane, which follows platform/macosx/shaders/bwdif_vt.metal where the two agree). */
int hbhip_bwdif_create(hbhip_ctx *ctx, int bob, int selective, int parity,
                       int width, int height, int depth, int log2_chroma_w, int log2_chroma_h,
                       hbhip_filter **out);
/* Test hook: copy one plane of an EEDI2 scratch frame to the host (buffer 0..3 = eedi_half[],
 * 4..8 = eedi_full[], decomb.c:64-74); dst == NULL only queries stride/height. */
int hbhip_decomb_debug_eedi_plane(hbhip_filter *f, int buffer, int plane, uint8_t *dst, int dst_stride,
                                  int *stride, int *height);

/* ---- Detelecine / pullup (replaces detelecine.c:159-999 pullup and :1116-1275 hb_detelecine_work) --------------------
 * The field queue, breaks / affinity and the frame-length decision run on the host side of this library; the block
 * metrics, their maxima and the weave are kernels.  Push one picture at a time with its PIC_FLAG_* (top field first,
 * repeat first field); a pull then yields at most one frame, tagged with the pushed picture's tag: the first picture
 * itself, a frame woven from the queue, or nothing (a dropped or not yet complete frame).  The same picture may come
 * out again later as the frame of its own two fields - then without a copy, as a frame both sides hold.  At most ten
 * pictures are held; HBHIP_ERR_STATE where the reference would run out of its ten buffers.
 * Margins below the reference's safety zones (1, 1, 4, 4) are raised to them and a plane out of range means plane 0
 * (detelecine.c:1035-1039, 1074-1077).  HBHIP_ERR_UNSUPPORTED where the reference has no defined result: a plane with
 * an odd number of rows, margins wider than the metric plane. */
typedef struct hbhip_detelecine_params
{
    int skip_left, skip_right, skip_top, skip_bottom;   /* in 8-sample columns / field-line pairs (junk_*)          */
    int strict_breaks;                                  /* -1 default, 0, 1                                        */
    int plane;                                          /* metric plane 0..2                                       */
    int parity;                                         /* -1 = from the picture flags, 0 = top first, 1 = bottom  */
} hbhip_detelecine_params;
int hbhip_detelecine_create(hbhip_ctx *ctx, const hbhip_detelecine_params *p, int width, int height, int depth,
                            int log2_chroma_w, int log2_chroma_h, hbhip_filter **out);
int hbhip_detelecine_push(hbhip_filter *f, const hbhip_host_frame *in, int64_t tag, int pic_flags);
int hbhip_detelecine_push_frame(hbhip_filter *f, hbhip_frame *fr, int64_t tag, int pic_flags);   /* as hbhip_filter_push_frame */

/* ---- Comb detect (replaces comb_detect.c:1051-1072 comb_segmenter and the passes it
 *      runs: comb_detect_template.c:288-402/789-933, comb_detect.c:221-276, 384-454,
 *      556-622, 726-792, 901-966, 1029-1049) ------------------------------------------ */
typedef struct hbhip_comb_detect_params
{
    int mode, spatial_metric, motion_threshold, spatial_threshold;
    int filter_mode, block_threshold, block_width, block_height;
    float gamma_lut[256];           /* built on the host as comb_detect.c:1074-1081 does   */
} hbhip_comb_detect_params;
int hbhip_comb_detect_create(hbhip_ctx *ctx, const hbhip_comb_detect_params *p, int width, int height,
                             int depth, hbhip_filter **out);
/* store_ref (comb_detect.c:1007-1018): the luma plane becomes the newest of the
 * prev/cur/next ring.  luma == NULL repeats the newest plane (first frame / EOF). */
/* depth > 8: the gamma table has 1 << depth entries (comb_detect.c:1102, 1074-1081), more than
 * the params struct holds; hand it over before the first classify.  (depth 8 uses p->gamma_lut.) */
int hbhip_comb_detect_set_gamma_lut(hbhip_filter *f, const float *lut, int entries);
int hbhip_comb_detect_store(hbhip_filter *f, const uint8_t *luma, int stride);
int hbhip_comb_detect_store_dev(hbhip_filter *f, const void *luma, int stride);
/* comb_segmenter on the ring: *combed = HB_COMB_NONE/LIGHT/HEAVY for the middle plane. */
int hbhip_comb_detect_classify(hbhip_filter *f, int force_exhaustive, int *combed);
/* The same verdicts for n_frames (<= 16) frames at once, for callers that hold the lumas in HBM: frame i is judged
 * from lumas[i], lumas[i + 1], lumas[i + 2] (prev / cur / next as the ring would hold them - n_frames + 2 device
 * pointers, `stride` bytes a row, 4-byte aligned), bit i of force_bits = force_exhaustive for frame i.  Three
 * launches and one read-back whatever n_frames is; does not touch the ring.  8-bit, modes 0-3; with the mask filter on
 * (mode & 2) only filter-mode 2, the others are HBHIP_ERR_UNSUPPORTED. */
int hbhip_comb_detect_classify_many_dev(hbhip_filter *f, const void *const *lumas, int stride, int n_frames,
                                        unsigned force_bits, int *combed);
/* test hook: copy one mask of frame `frame` of the last classify (frame 0) or
 * classify_many (0 .. n-1) to `dst`: height rows of *stride bytes.
 * which: 0 the detector's mask, 1 the mask the block score read when a mask
 * filter is on, 2 the intermediate mask where one exists in HBM (else UNSUPPORTED). */
int hbhip_comb_detect_debug_mask(hbhip_filter *f, int frame, int which,
                                 uint8_t *dst, size_t dst_bytes, int *stride);

/* Mask overlay, modes 4 (MODE_MASK) / 8 (MODE_COMPOSITE): draw_mask_box + apply_mask (comb_detect_template.c:21-136)
 * on `frame`, which holds a COPY of the frame the last classify judged combed (process_frame, comb_detect.c:1519-1526).
 * plane_w / plane_h: samples per row and rows of each plane.  The box position is the one a single check thread
 * leaves (the reference's segment threads race on it, comb_detect.c:205-208); its outline stays in the mask, as in
 * the reference. */
int hbhip_comb_detect_overlay(hbhip_filter *f, const hbhip_host_frame *frame, const int plane_w[3], const int plane_h[3]);
int hbhip_comb_detect_overlay_dev(hbhip_filter *f, const hbhip_dev_frame *frame, const int plane_w[3], const int plane_h[3]);

/* ---- Alias family (libavfilter/zimg-backed in the reference; arithmetic external,
 *      parity pinned to oracle/alias_oracle.c only — see DESIGN.md) ------------------- */
/* rotate_init's transpose/hflip/vflip composition (rotate.c:169-256). angle 0/90/180/270. */
int hbhip_rotate_create(hbhip_ctx *ctx, int angle, int hflip, int width, int height, int depth,
                        int log2_chroma_w, int log2_chroma_h, hbhip_filter **out);
/* FFmpeg `monochrome=cb:cr:size:high` as grayscale_init sets it up (grayscale.c:43-61). */
int hbhip_grayscale_create(hbhip_ctx *ctx, double cb, double cr, double size, double high,
                           int width, int height, int depth, int log2_chroma_w, int log2_chroma_h,
                           hbhip_filter **out);
/* `crop` + `zscale=filter=lanczos` as crop_scale_init sets them up (cropscale.c:63-165). */
typedef struct hbhip_cropscale_params
{
    int width, height;                                   /* output size                   */
    int crop_top, crop_bottom, crop_left, crop_right;    /* cropscale.c:68-73             */
} hbhip_cropscale_params;
int hbhip_cropscale_create(hbhip_ctx *ctx, const hbhip_cropscale_params *p, int width, int height,
                           int depth, int log2_chroma_w, int log2_chroma_h, hbhip_filter **out);
/* The same with the stream's chroma sample location (AVCHROMA_LOC_*: 0 unspecified, 1 left, 2 center, 3 topleft, 4 top,
 * 5 bottomleft, 6 bottom), which zscale takes from the frame when its chromal / chromal_in are not set, as the reference
 * leaves them: a subsampled chroma direction is shifted by -raw * 0.5 * (1 - src / dst) source chroma samples, raw = -0.5
 * co-sited (left, top), 0 centred, +0.5 bottom.  hbhip_cropscale_create is this call with location 1; 0 is taken as 1.
 * A location outside 0..6 is HBHIP_ERR_ARG.  PARITY UNPINNED: zimg's rule as recalled (csrc/chroma_siting.h). */
int hbhip_cropscale_create_sited(hbhip_ctx *ctx, const hbhip_cropscale_params *p, int width, int height,
                                 int depth, int log2_chroma_w, int log2_chroma_h, int chroma_location, hbhip_filter **out);
/* The other branch of crop_scale_init (cropscale.c:159-165): `crop` + `scale=flags=lanczos+accurate_rnd`, which the
 * reference builds when hb_av_can_use_zscale() says no (an odd width or height, hbffmpeg.c:870-915) - libswscale's
 * arithmetic instead of zimg's (8-bit planes: hScale8To15 + yuv2planeX_8; 10 / 12-bit: hScale16To15 + yuv2planeX_10 / _12). */
int hbhip_cropscale_sws_create(hbhip_ctx *ctx, const hbhip_cropscale_params *p, int width, int height,
                               int depth, int log2_chroma_w, int log2_chroma_h, hbhip_filter **out);
/* FFmpeg `pad=width:height:x:y:color` as pad_init sets it up (pad.c:40-148): the picture at (x, y)
 * of a width x height one, the rest filled with fill[] (Y, Cb, Cr sample values, already converted
 * from the RGB colour the way drawutils.c:ff_draw_color does).  x, y multiples of the chroma subsampling. */
typedef struct hbhip_pad_params
{
    int width, height, x, y;
    int fill[3];
} hbhip_pad_params;
int hbhip_pad_create(hbhip_ctx *ctx, const hbhip_pad_params *p, int width, int height, int depth,
                     int log2_chroma_w, int log2_chroma_h, hbhip_filter **out);
/* FFmpeg `deblock=filter=..:block=..:alpha=..:beta=..:gamma=..:delta=..` as deblock_init sets it up (deblock.c:37-86):
 * strong (1) or weak (0), the block size 4..512 shared by every plane, and the integer thresholds FFmpeg derives from
 * the float options, (int)(option * ((1 << depth) - 1)) - the caller resolves them (libhb/deblock_hip.c).  Out of place:
 * every output sample is made from the input frame.  8/10/12-bit.  HBHIP_ERR_UNSUPPORTED for a plane whose last edge's
 * window would reach past it (size % block in {1, 2} strong, 1 weak, with an edge in the plane).  Arithmetic restated
 * (parity unpinned). */
typedef struct hbhip_deblock_params
{
    int strong;                          /* 1 = `strong` (six taps), 0 = `weak` (four)   */
    int block;                           /* `block`, 4..512                              */
    int ath, bth, gth, dth;              /* integer alpha / beta / gamma / delta         */
} hbhip_deblock_params;
int hbhip_deblock_create(hbhip_ctx *ctx, const hbhip_deblock_params *p, int width, int height, int depth,
                         int log2_chroma_w, int log2_chroma_h, hbhip_filter **out);
/* test hook: warm-up edges of the speculative row segments of the strong b = 4 / 5 kernel (default 4; 0 = every segment
 * starts cold, so that every boundary whose edge fires goes through the repair walk).  The result is the same for any value. */
int hbhip_deblock_set_warmup(hbhip_filter *f, int edges);
/* FFmpeg `deband=1thr=..:2thr=..:3thr=..:4thr=..:range=..:blur=..` as deband_init sets it up (deband.c:35-80):
 * `direction` and `coupling` keep FFmpeg's defaults.  thr[p] are the integer thresholds FFmpeg derives from the float
 * options, (int)(((1 << depth) - 1) * option) - the caller resolves them (libhb/deband_hip.c).  The per-position offset
 * table is built once, on the host, with libm (hbhip_deband_offsets).  Out of place: every output sample is made from
 * the input frame.  8/10/12-bit planar 4:2:0 / 4:2:2 / 4:4:4.  Arithmetic restated (parity unpinned). */
typedef struct hbhip_deband_params
{
    int   thr[3];                        /* integer 1thr / 2thr / 3thr                    */
    int   blur;                          /* 1: against the average, 0: against each ref   */
    int   range;                         /* |range| <= 2^30                               */
    float direction;                     /* FFmpeg's default: (float)(2 * M_PI)           */
} hbhip_deband_params;
int hbhip_deband_create(hbhip_ctx *ctx, const hbhip_deband_params *p, int width, int height, int depth,
                        int log2_chroma_w, int log2_chroma_h, hbhip_filter **out);
/* FFmpeg's offset table for a width x height luma plane (config_input), exactly: x_pos / y_pos[y * width + x], built
 * with the host's sinf / cosf / floorf in float, without contraction.  Needs no device.  HBHIP_ERR_ARG for a size < 1
 * or |range| > 2^30. */
int hbhip_deband_offsets(int width, int height, int range, float direction, int *x_pos, int *y_pos);
/* test / tool hook: which kernel runs - 0 the automatic choice (the LDS tile where its halo fits), 1 the
 * LDS tile (HBHIP_ERR_UNSUPPORTED where the halo does not fit), 2 the direct global gather.  The result is the same. */
int hbhip_deband_set_kernel(hbhip_filter *f, int kernel);
/* FFmpeg `bm3d=sigma=..` as bm3d_init sets it up (bm3d.c:44-57): every other option keeps FFmpeg's default, so the group
 * size is 1 and the filter is a sliding 16 x 16 DCT with a hard threshold and weighted aggregation over all three planes.
 * The fields after sigma are those defaults (recalled; the one table of csrc/bm3d.hip) and what follows from them: thr[z],
 * the threshold of a coefficient with z of its two frequencies zero, and dct[k * 16 + n] = cos(pi (2n + 1) k / 32), built
 * in double and rounded once.  Out of place.  8/10/12-bit planar 4:2:0 / 4:2:2 / 4:4:4; HBHIP_ERR_UNSUPPORTED for a plane
 * narrower or lower than 16 samples and for options other than the defaults.  Arithmetic restated (parity unpinned,
 * DESIGN.md §4.18). */
typedef struct hbhip_bm3d_params
{
    float sigma;                         /* as FFmpeg holds it: the "%g" text parsed into a float option */
    int   block, bstep, group, range, mstep;   /* 16, 4, 1, 9, 1                               */
    float thmse, hdthr;                  /* 0, 2.7                                        */
    int   estim, planes;                 /* 0 = basic, 7                                  */
    float thr[3];                        /* hdthr sigma sqrt2 16 16 2^(depth - 8) / 255 * sqrt2^(1 + z) */
    float dct[256];
} hbhip_bm3d_params;
/* `settings` ("sigma=3"; absent: 1, bm3d.c:46) -> parameters, through the "%g" text bm3d.c's double becomes on its way
 * into FFmpeg.  Needs no device.  HBHIP_OK, or HBHIP_ERR_UNSUPPORTED where FFmpeg's graph would fail (sigma NaN, negative
 * or above 99999.9) or for a depth other than 8 / 10 / 12. */
int hbhip_bm3d_params_from_settings(const char *settings, int depth, hbhip_bm3d_params *out);
int hbhip_bm3d_create(hbhip_ctx *ctx, const hbhip_bm3d_params *p, int width, int height, int depth,
                      int log2_chroma_w, int log2_chroma_h, hbhip_filter **out);
/* `format=pix_fmts=<fmt>` as format_init sets it up (format.c:13-111): libavfilter then converts with a same-size
 * `scale`, i.e. libswscale's unscaled planar copy.  Built: planar YUV depth changes 8 / 10 / 12 -> 8 / 10 / 12 with the
 * chroma subsampling unchanged (up: shift, full-range luma replicates the top bits; down: ordered dither - the
 * shift-only form for chroma and limited-range luma, (v - (v >> dst_depth) + d) >> shift for full-range luma, both arms of
 * swscale_unscaled.c's DITHER_COPY).  Arithmetic pinned to
 * oracle/alias_oracle.c:orc_format_plane only (parity unpinned). */
int hbhip_format_create(hbhip_ctx *ctx, int width, int height, int src_depth, int dst_depth,
                        int log2_chroma_w, int log2_chroma_h, int full_range, hbhip_filter **out);
/* The same filter when the target has FEWER chroma samples than the stream, at equal depth (8 / 10 / 12): 4:2:2 -> 4:2:0,
 * 4:4:4 -> 4:2:2, 4:4:4 -> 4:2:0.  libavfilter's `scale` is then libswscale's general scaler at its default flags: luma a
 * copy, Cb and Cr through the bicubic (B = 0, C = 0.6) integer tables - 14-bit horizontal, 12-bit vertical coefficients,
 * 15-bit intermediates.  Target row j lies midway between source rows 2j and 2j + 1, target column i on source column 2i
 * (left-sited chroma); `chroma_location` is accepted and every value is taken as left-sited, as the crop/scale filter's
 * swscale form does.  HBHIP_ERR_UNSUPPORTED: upsampling in either direction, equal subsampling, a depth outside
 * 8 / 10 / 12, a chroma plane under 11 samples in a direction that is resampled (libswscale shortens its filter there).
 * Arithmetic pinned to tests/format_resample_model.py only (parity unpinned). */
int hbhip_format_resample_create(hbhip_ctx *ctx, int width, int height, int depth, int src_log2_cw, int src_log2_ch,
                                 int dst_log2_cw, int dst_log2_ch, int chroma_location, hbhip_filter **out);
/* The same scaler pass when the target also, or only, has a LOWER depth: 10 -> 8, 12 -> 8, 12 -> 10 bits, with the three
 * pairs above or with the subsampling unchanged (4:2:0 -> 4:2:0, 4:2:2 -> 4:2:2, 4:4:4 -> 4:4:4: what libswscale does in
 * front of a semi-planar target, where it leaves the unscaled planar copy of hbhip_format_create).  Every plane, luma
 * included, runs through the horizontal pass or its identity (15-bit intermediates) and the output stage of the target's
 * depth: to 8 bits with the 8 x 8 ordered dither ff_dither_8x8_128 by the OUTPUT sample's row and column (Cr three columns
 * on), to 10 bits with a flat half.  No range conversion.  At src_depth == dst_depth this is
 * hbhip_format_resample_create.  HBHIP_ERR_UNSUPPORTED: a higher target depth, a depth outside 8 / 10 / 12, more chroma
 * samples in either direction, nothing to do at all, a chroma plane under 11 samples in a direction that is resampled.
 * Arithmetic pinned to tests/format_scaled_model.py only (parity unpinned). */
int hbhip_format_scaled_create(hbhip_ctx *ctx, int width, int height, int src_depth, int dst_depth, int src_log2_cw,
                               int src_log2_ch, int dst_log2_cw, int dst_log2_ch, int chroma_location, hbhip_filter **out);
/* The other direction: a target with MORE chroma samples than the stream, at equal or HIGHER depth - 4:2:0 -> 4:2:2 (a
 * vertical pass), 4:2:2 -> 4:4:4 (a horizontal pass), 4:2:0 -> 4:4:4 (both); 8 -> 8, 10 -> 10, 12 -> 12, 8 -> 10, 8 -> 12,
 * 10 -> 12 bits.  What an encoder that only takes 4:2:2 / 4:4:4 input gets behind a 4:2:0 title (work.c:1525-1552: the
 * third match_pix_fmt call takes the first entry of the encoder's list).  libswscale's general scaler again: Cb and Cr
 * through the bicubic tables of the 1:2 ratio (four taps: target column 2i on source column i, target rows 2j and 2j + 1 a
 * quarter above and below source row j), 15-bit intermediates, the output stage of the target's depth with its flat round
 * term (the depth does not fall: no dither).  Luma runs through the identity filters: a copy at equal depth, v << (dst_depth -
 * src_depth) above it in BOTH ranges - the scaler replicates no top bits, unlike hbhip_format_create's full-range 8 -> 10.
 * The target's chroma planes are -((-width) >> dst_log2_cw) by -((-height) >> dst_log2_ch).  `chroma_location`: every
 * value is taken as left-sited.  HBHIP_ERR_UNSUPPORTED: a depth outside 8 / 10 / 12, a lower target depth, fewer chroma
 * samples in either direction, equal subsampling, a chroma plane under 7 samples in a direction that is up-sampled
 * (libswscale shortens its filter there).  Arithmetic pinned to tests/format_upsample_model.py only (parity unpinned). */
int hbhip_format_upsample_create(hbhip_ctx *ctx, int width, int height, int src_depth, int dst_depth, int src_log2_cw,
                                 int src_log2_ch, int dst_log2_cw, int dst_log2_ch, int chroma_location, hbhip_filter **out);
/* FEWER chroma samples together with a HIGHER depth: 4:2:2 -> 4:2:0, 4:4:4 -> 4:2:2, 4:4:4 -> 4:2:0 at 8 -> 10, 8 -> 12 or
 * 10 -> 12 bits.  What an encoder whose list holds only 10-bit formats (SVT-AV1 and VP9 10-bit: yuv420p10le; ProRes and
 * DNxHR 10-bit: yuv422p10le) gets behind an 8-bit 4:2:2 / 4:4:4 title (work.c:1525-1552: the second match_pix_fmt call
 * takes any format with no more chroma, whatever its depth).  The general scaler of hbhip_format_resample_create, same
 * tables and siting: the horizontal pass or its identity by the SOURCE depth (hScale8To15: >> 7; hScale16To15:
 * >> (src_depth - 1); 15-bit intermediates, saturated at the top only), the output stage by the TARGET's
 * (yuv2planeX_10 / _12: the flat half of the shift 27 - dst_depth, no dither), clipped to [0, 2^dst_depth - 1].  Luma is
 * v << (dst_depth - src_depth) in both ranges, no top-bit replication: 255 -> 1020.  No range conversion.
 * `chroma_location`: every value is taken as left-sited.  HBHIP_ERR_UNSUPPORTED: an equal or lower target depth, a depth
 * outside 8 / 10 / 12, equal subsampling, more chroma samples in either direction, a chroma plane under 11 samples in a
 * direction that is resampled.  Arithmetic pinned to tests/format_deepen_model.py only (parity unpinned). */
int hbhip_format_deepen_create(hbhip_ctx *ctx, int width, int height, int src_depth, int dst_depth, int src_log2_cw,
                               int src_log2_ch, int dst_log2_cw, int dst_log2_ch, int chroma_location, hbhip_filter **out);
/* The zscale [-> format=gbrpf32le -> tonemap] -> zscale -> format graph colorspace_init builds
 * (colorspace.c:126-193): matrix / range / transfer / primaries conversion, with tone mapping
 * when the source transfer is SMPTE 2084 or ARIB STD-B67 and the transfer changes.  Colour ids
 * are the AVCOL_* = HB_COLR_* numbers (common.h), range 1 = tv, 2 = pc; tonemap ids are
 * vf_tonemap's.  Arithmetic pinned to oracle/colorspace_oracle.c only (parity unpinned).
 * 8/10/12-bit, 4:2:0 / 4:2:2 / 4:4:4.  HBHIP_ERR_UNSUPPORTED for conversions outside its tables.
 * Matrix ids beyond the plain Kr / Kb ones, on either side: 12 (chroma-derived-nc: Kr / Kb of that side's primaries),
 * 10 and 13 (bt2020c, chroma-derived-c: constant luminance, BT.2020 primaries only) and 14 (ICtCp: BT.2020 primaries
 * with SMPTE 2084 or ARIB STD-B67 only); 10, 13 and 14 always convert through linear light.  These have no oracle:
 * arithmetic pinned to tests/colour_model_wide.py within a code. */
enum { HBHIP_TONEMAP_NONE = 0, HBHIP_TONEMAP_LINEAR = 1, HBHIP_TONEMAP_GAMMA = 2, HBHIP_TONEMAP_CLIP = 3,
       HBHIP_TONEMAP_REINHARD = 4, HBHIP_TONEMAP_HABLE = 5, HBHIP_TONEMAP_MOBIUS = 6 };
typedef struct hbhip_colorspace_params
{
    int in_prim, in_transfer, in_matrix, in_range;       /* init->color_* (colorspace.c:96-99)      */
    int out_prim, out_transfer, out_matrix, out_range;   /* after the settings are applied (:101-120) */
    int tonemap;                                         /* HBHIP_TONEMAP_*; "hable" by default (:151) */
    double param;                                        /* NAN = the operator's default (:154-157)  */
    double desat;                                        /* carried; without effect, as in FFmpeg on GBR frames */
    double npl;                                          /* nominal peak luminance, 100 (:74)        */
    double peak;                                         /* determine_signal_peak (:37-49)           */
} hbhip_colorspace_params;
int hbhip_colorspace_create(hbhip_ctx *ctx, const hbhip_colorspace_params *p, int width, int height,
                            int depth, int log2_chroma_w, int log2_chroma_h, hbhip_filter **out);
/* The same with the stream's chroma sample location (AVCHROMA_LOC_*, as hbhip_cropscale_create_sited): a subsampled
 * direction is up- and down-sampled co-sited (up 2k: c[k], 2k + 1: (c[k] + c[k+1]) / 2; down 2k - 1 .. 2k + 1 with
 * 1/4 1/2 1/4) or centred (up 2k: c[k-1] / 4 + 3 c[k] / 4, 2k + 1: 3 c[k] / 4 + c[k+1] / 4; down 2k - 1 .. 2k + 2 with
 * 1/8 3/8 3/8 1/8), edges repeating.  Horizontally locations 0, 1, 3, 5 are co-sited and 2, 4, 6 centred; vertically 3
 * and 4 are co-sited (top) and everything else centred - vertical bottom (5, 6) too, an approximation.
 * hbhip_colorspace_create is this call with location 1.  A location outside 0..6 is HBHIP_ERR_ARG. */
int hbhip_colorspace_create_sited(hbhip_ctx *ctx, const hbhip_colorspace_params *p, int width, int height,
                                  int depth, int log2_chroma_w, int log2_chroma_h, int chroma_location, hbhip_filter **out);

/* ---- Frame-difference metric (replaces hb_motion_metric, motion_metric.c: the object vfr.c
 *      calls on consecutive frames to choose the one to drop, vfr.c:76-108, 380) ---------------
 * gamma_lut: the 1 << depth entries build_gamma_lut produces (:36-42), built by the caller. */
typedef struct hbhip_motion_metric hbhip_motion_metric;
int  hbhip_motion_metric_create(hbhip_ctx *ctx, int width, int height, int depth,
                                const unsigned *gamma_lut, int entries, hbhip_motion_metric **out);
/* hb_motion_metric_work (:268-279): luma planes of two frames -> the metric.  Synchronous. */
int  hbhip_motion_metric_run(hbhip_motion_metric *m, const uint8_t *luma_a, int stride_a,
                             const uint8_t *luma_b, int stride_b, float *out);             /* host planes */
int  hbhip_motion_metric_run_dev(hbhip_motion_metric *m, const void *luma_a, int stride_a,
                                 const void *luma_b, int stride_b, float *out);            /* planes in HBM */
void hbhip_motion_metric_destroy(hbhip_motion_metric *m);

/* ---- Title scan (replaces what scan.c does with the pixels of every preview: hb_detect_comb, hb.c:1088-1167, called at
 *      scan.c:973, and the black-border walk of scan.c:986-1052 over row_all_dark / column_all_dark, :456-509) -----------
 * For pictures that are in HBM already: five launches and one small record over the bus per picture, instead of the
 * picture itself.  Defined for what the scan decodes to (decavcodec.c:1359-1369): 8-bit planar 4:2:0 with even sizes.
 * All integer, bit-for-bit with the reference (DESIGN.md §4.19 has the definition).  Pictures are pushed as frames - an
 * NV12 surface through hbhip_frame_import_surface[_async] first - and their results pulled in push order; up to
 * HBHIP_SCAN_INFLIGHT_MAX may be in flight.  The object holds a reference on a pushed frame until its result is pulled.
 * Everything runs on the object's context's stream behind the frame's contents (hbhip_frame_use_on).
 * hbhip_ctx_bus_bytes of the object's context counts HBHIP_SCAN_RECORD_BYTES of D2H per pushed picture and nothing else.
 * Refused before anything is queued - HBHIP_ERR_UNSUPPORTED: a frame that is not 8-bit 4:2:0 planar, an odd width or
 * height, a size other than the object's, a width or height below 8 (create: the same, and a size above 16384);
 * HBHIP_ERR_ARG: a frame of another GPU than the object's; HBHIP_ERR_STATE: HBHIP_SCAN_INFLIGHT_MAX pictures in flight. */
#define HBHIP_SCAN_INFLIGHT_MAX 32
#define HBHIP_SCAN_RECORD_BYTES 48
typedef struct hbhip_scan hbhip_scan;
typedef struct hbhip_scan_params
{
    /* hb_detect_comb's six sensitivities; scan.c:973 passes 10, 30, 9, 10, 30, 9 */
    int color_equal, color_diff, threshold;
    int prog_equal, prog_diff, prog_threshold;
} hbhip_scan_params;
typedef struct hbhip_scan_result
{
    int top, bottom, left, right;        /* the picture's crop as scan.c:999-1044 leaves it                         */
    int recorded;                        /* scan.c:1049: all four below a quarter of the picture                    */
    int cc[3];                           /* hb_detect_comb's per-plane scores, the carried-over counts included     */
    int average_cc;                      /* hb.c:1149                                                               */
    int combed;                          /* hb_detect_comb's return value                                           */
} hbhip_scan_result;
int  hbhip_scan_create(hbhip_ctx *ctx, int width, int height, hbhip_scan **out);
void hbhip_scan_destroy(hbhip_scan *s);                /* waits for what is in flight and drops it */
/* pic_flags: the buffer's s.flags (bit 16 selects the prog_* triple, hb.c:1095-1101); p == NULL: scan.c's six numbers */
int  hbhip_scan_push(hbhip_scan *s, hbhip_frame *frame, int pic_flags, const hbhip_scan_params *p);
/* the oldest picture's result (waits for it); HBHIP_AGAIN when none is in flight */
int  hbhip_scan_pull(hbhip_scan *s, hbhip_scan_result *out);
int  hbhip_scan_inflight(hbhip_scan *s);

/* ---- A preview's JPEG (replaces hb_save_preview's tjCompressFromYUVPlanes, hb.c:583-629, which scan.c:979-982 calls for
 *      every preview when store_previews is set) -----------------------------------------------
 * The picture is a device frame and stays where it is: what comes back is the finished file.  Defined for what the scan
 * decodes to: 8-bit planar 4:2:0 with even sizes.  The file is the baseline JPEG libjpeg writes for these planes with its
 * DEFAULT DCT (the accurate integer one, jfdctint.c), byte for byte: JFIF 1.01 header, Annex K's tables scaled by `quality`
 * (jpeg_quality_scaling), Annex K's Huffman tables, 2x2 luma sampling, one scan, no restart markers.  hb.c:607 asks for
 * TJFLAG_FASTDCT, whose rounding of the AC coefficients differs; container, tables and entropy code are the same.
 * push queues a picture's launches on the context's stream behind the frame's contents, pull hands out the oldest
 * picture's file (waiting for it); up to HBHIP_JPEG_INFLIGHT_MAX may be in flight.  The object holds a reference on a
 * pushed frame until the pull.  Per pushed picture hbhip_ctx_bus_bytes of the object's context counts a 16-byte record and
 * the file's scan segment (the file less its 623-byte header and the end marker) of D2H, and nothing else.
 * Refusals, all before anything is queued - HBHIP_ERR_UNSUPPORTED: not 8-bit planar 4:2:0, an odd size, another size than
 * the object's, below 8 x 8 (create also: above 16384); HBHIP_ERR_ARG: a quality outside 1 .. 100, a frame of another GPU
 * than the object's; HBHIP_ERR_STATE: HBHIP_JPEG_INFLIGHT_MAX pictures in flight.
 * pull: `cap` bytes at dst; *size is the file's length.  A file longer than `cap` answers HBHIP_ERR_ARG with *size set to
 * the length it has, nothing written, and the picture is DROPPED (push it again): hbhip_jpeg_bound() is a capacity no file
 * of the object's size exceeds. */
#define HBHIP_JPEG_INFLIGHT_MAX 4
typedef struct hbhip_jpeg hbhip_jpeg;
int    hbhip_jpeg_create(hbhip_ctx *ctx, int width, int height, int quality, hbhip_jpeg **out);
void   hbhip_jpeg_destroy(hbhip_jpeg *j);            /* waits for what is in flight and drops it */
size_t hbhip_jpeg_bound(hbhip_jpeg *j);              /* a capacity no file of this size exceeds */
int    hbhip_jpeg_push(hbhip_jpeg *j, hbhip_frame *frame);
/* the oldest picture's file (waits for it); HBHIP_AGAIN when none is in flight */
int    hbhip_jpeg_pull(hbhip_jpeg *j, uint8_t *dst, size_t cap, size_t *size);
int    hbhip_jpeg_inflight(hbhip_jpeg *j);

/* ---- Subtitle compositor (replaces hb_blend, blend.c: the object rendersub.c hands every frame
 *      and the list of rendered overlays, rendersub.c:467, 1129-1161) -------------------------
 * Planar 8/10/12-bit frames; overlays are 8-bit Y/Cb/Cr/alpha bitmaps either in the frame's chroma
 * subsampling (blend8on8 / blend8on1x, blend.c:425-604) or 4:4:4 on a subsampled frame
 * (blend_subsample_8on8 / _8on1x, :48-328, weights from the chroma location, common.c:7054-7091). */
typedef struct hbhip_blend hbhip_blend;
typedef struct hbhip_overlay
{
    const uint8_t *plane[4];          /* Y, Cb, Cr, alpha (host memory) */
    int            stride[4];
    int            x, y, width, height;   /* hb_buffer_t.f.x / .y / .width / .height of the overlay */
} hbhip_overlay;
/* hb_blend_init (:788-846); chroma_location is the AVCHROMA_LOC_* number */
int  hbhip_blend_create(hbhip_ctx *ctx, int width, int height, int depth, int log2_chroma_w, int log2_chroma_h,
                        int chroma_location, int overlay_log2_chroma_w, int overlay_log2_chroma_h, hbhip_blend **out);
/* Upload the current overlay list (call again only when it changes: rendersub's `changed`).
 * The bitmaps are consumed when this returns. */
int  hbhip_blend_set_overlays(hbhip_blend *b, const hbhip_overlay *ov, int n);
/* hb_blend_work (:848-873): composite the overlays, in order, onto the frame in place. */
int  hbhip_blend_apply(hbhip_blend *b, const hbhip_host_frame *frame);       /* H2D, blend, D2H; synchronous */
int  hbhip_blend_apply_dev(hbhip_blend *b, const hbhip_dev_frame *frame);    /* frame already in HBM */
void hbhip_blend_destroy(hbhip_blend *b);                                    /* hb_blend_close (:875-885) */
/* The same object for biplanar 4:2:0 host frames, depth 8 (NV12) or 10 (P010LE): blend8onbi8 / blend8onbi1x (:606-786) and
 * blend_subsample_8onbi8 / _8onbi1x (:142-234, :330-423) on the samples as stored - P010 is composited MSB-aligned, not as
 * planar 10-bit.  Overlays are set with hbhip_blend_set_overlays.  Such an object answers HBHIP_ERR_ARG to hbhip_blend_apply
 * and _apply_dev, and one made by hbhip_blend_create answers it to hbhip_blend_apply_biplanar.  HBHIP_ERR_UNSUPPORTED:
 * another depth, a width or height below 2. */
int  hbhip_blend_create_biplanar(hbhip_ctx *ctx, int width, int height, int depth, int chroma_location,
                                 int overlay_log2_chroma_w, int overlay_log2_chroma_h, hbhip_blend **out);
int  hbhip_blend_apply_biplanar(hbhip_blend *b, const hbhip_host_biplanar *frame);   /* H2D, blend, D2H; synchronous */
/* Text subtitles (SSA / ASS, SRT, TX3G, CC608: everything libass renders).  What render_ssa_subs does behind ass_render_frame
 * (rendersub.c:623-665) when the list has changed: the boxes of hb_box_vec_append / _merge / _compact (:144-226), each pulled
 * back to a chroma sample of the cropped picture (:648-653) and placed at its position plus the crop (:658-659), and
 * compose_subsample_ass (:474-612) into one overlay per box - that part on the GPU (csrc/ass_compose.hip), straight into the
 * object's overlay store.  `img` is the ASS_Image list in list order: the 8-bit coverage bitmap, its position, the colour as
 * rgb2yuv_fn(color >> 8) gives it (Y = bits 16-23, Cr = 8-15, Cb = 0-7) and a = color & 0xff, libass's transparency (0 =
 * opaque).  Replaces the object's overlay list (n == 0 or no image with an area: clears it, clear_ssa_rendered_sub_cache
 * :614-621); the bitmaps are consumed when this returns.  Bit-exact with the reference, except that a chroma sample no
 * covered pixel contributes to (accu_c == 0, :593 - the reference leaves what its buffer pool held) is 0; it lies under
 * alpha 0.  For objects of hbhip_blend_create and of hbhip_blend_create_biplanar.  HBHIP_ERR_UNSUPPORTED where the object's
 * overlay subsampling is not the frame's (ssa_post_init never asks for that, :679-712); HBHIP_ERR_ARG for a negative
 * position or size, a stride below the width or a missing bitmap. */
typedef struct hbhip_ass_image { const uint8_t *bitmap; int stride, w, h, dst_x, dst_y;
                                 uint8_t y, cb, cr, a; } hbhip_ass_image;
int  hbhip_blend_set_ass_images(hbhip_blend *b, const hbhip_ass_image *img, int n, int crop_left, int crop_top);
/* Bitmap subtitles (PGS, DVB, VOBSUB).  What scale_subtitle (rendersub.c:242-377) makes of each decoded bitmap for a frame of
 * the object's size, for the whole list at once: factor = max(width / window_width, height / window_height) in double
 * (:249-266), used when it is more than 1 % off 1 (:267); size and position (int)(value * factor) (:273-283); the placement
 * rule of :311-375 with crop = job->crop (top, bottom, left, right).  The scaling itself - the reference's
 * SWS_LANCZOS | SWS_ACCURATE_RND context, run per frame - is one kernel per bitmap (csrc/bitmap_scale.hip), and it runs once
 * per subtitle: the object keeps what it has made under the caller's `key`.  A key seen before with the same source and
 * scaled size costs no copy and no launch; keys a call does not name are dropped.  Replaces the object's overlay list, in list
 * order; entries without an area (PGS "clear" packets, :1043-1055) are skipped, n == 0 empties the list.  The bitmaps are
 * consumed when this returns.  PARITY UNPINNED: libswscale's arithmetic as oracle/alias_oracle.c:orc_cropscale_plane_sws
 * restates it.  For objects of hbhip_blend_create and of hbhip_blend_create_biplanar.  HBHIP_ERR_UNSUPPORTED: an object whose
 * overlays are not 4:4:4 (:418, :1073), a factor outside [0.25, 4], a bitmap narrower or lower than 8 samples that has to
 * be scaled (libswscale clamps its tap count there); HBHIP_ERR_ARG: a negative size, a stride below the width, a missing
 * plane.  After any failure the list is empty. */
typedef struct hbhip_bitmap_sub
{
    const uint8_t *plane[4];          /* Y, Cb, Cr, alpha: 8-bit 4:4:4 (host memory) */
    int            stride[4];
    int            x, y, width, height;               /* hb_buffer_t.f.x / .y / .width / .height */
    int            window_width, window_height;       /* f.window_*: the canvas; <= 0: none */
    uint64_t       key;                               /* the caller's identity of this subtitle */
} hbhip_bitmap_sub;
int  hbhip_blend_set_bitmaps(hbhip_blend *b, const hbhip_bitmap_sub *sub, int n, const int crop[4]);
/* test hooks: scale launches, bitmaps uploaded and cache hits of hbhip_blend_set_bitmaps since the object was made; how many
 * overlays the object holds, and overlay `index` of its device store read back - xywh = its position and size, plane / stride
 * = where the Y, Cb, Cr and alpha planes go (plane == NULL: the geometry only) */
int  hbhip_blend_debug_bitmap_stats(hbhip_blend *b, int64_t *scaled, int64_t *uploaded, int64_t *hits);
int  hbhip_blend_debug_overlay_count(hbhip_blend *b);
int  hbhip_blend_debug_get_overlay(hbhip_blend *b, int index, uint8_t *const plane[4], const int stride[4], int xywh[4]);

/* ---- test hook ------------------------------------------------------------------------------
 * The EEDI2 mask passes of a batch run as ONE launch whose tiles wait for the previous field's tiles (csrc/eedi2_engine.h:
 * MaskChain).  A wait that runs out never aborts: the launch ends, and a repair pass behind it recomputes the batch's
 * masks field by field.  spin_limit > 0: polls a wait makes before it gives up, for every mask launch from now on
 * (1 = at once, i.e. every launch takes the repair path); 0: back to the default (about a second).  Returns how many
 * mask launches have been repaired in this process so far. */
unsigned hbhip_debug_mask_chain(int spin_limit);

#ifdef __cplusplus
}
#endif
#endif /* HBHIP_H */
