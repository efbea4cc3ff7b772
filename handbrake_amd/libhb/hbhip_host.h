/* hbhip_host.h — what the HIP-backed hb_filter_object_t implementations share:
 * the libhb types (real ones inside libhb, include/hbhip_libhb.h outside), the
 * C ABI of the device library, and a few helpers to move hb_buffer_t planes
 * through it.
 */
#ifndef HBHIP_HOST_H
#define HBHIP_HOST_H

#include "hbhip_libhb.h"
#include "hbhip.h"

/* One process-wide device context per GPU index, created on first use.  Filters of one job share it, i.e. they share
 * one stream, which is what lets adjacent HIP filters hand frames over in HBM without extra synchronisation.  The GPU
 * is the job's: init->job->hw_device_index (common.h:991) when it is >= 0, else the process default (HBHIP_DEVICE in
 * the environment, else 0) - libhb/hbhip_registry.c. */
int        hbhip_host_default_device(void);
int        hbhip_host_device_for(const hb_filter_init_t *init);
int        hbhip_host_job_index_is_hip(const hb_job_t *job);     /* hw_device_index names a HIP device (no other vendor's hw path in the job) */
hbhip_ctx *hbhip_host_ctx_on(int device);
hbhip_ctx *hbhip_host_ctx_for(const hb_filter_init_t *init);     /* what a drop-in's init() uses: the job's own stream on the job's GPU */
hbhip_ctx *hbhip_host_job_ctx(const hb_job_t *job);              /* the context a live job has leased, or NULL */
/* role 1 = the deinterlacing side of a job (comb detect, decomb, yadif, bwdif): a second context of the job's GPU unless
 * HBHIP_JOB_STREAMS=1, then the job's own; hbhip_host_use_frame: called by every consumer of a device frame in front of the
 * work that reads it (libhb/hbhip_registry.c) */
hbhip_ctx *hbhip_host_ctx_for_role(const hb_filter_init_t *init, int role);
int        hbhip_host_use_frame(hbhip_ctx *ctx, const hb_buffer_t *in);
hbhip_ctx *hbhip_host_ctx(void);                                 /* the process default's context */
void       hbhip_host_ctx_release(void);

/* The biplanar 4:2:0 formats the adapters and the compositor take (FFmpeg's numbers; names of this project's own, the
 * stand-in header has no enumerators for them) */
#define HBHIP_PIX_FMT_NV12   23
#define HBHIP_PIX_FMT_P010LE 158
static inline int hbhip_host_is_biplanar(int pix_fmt) { return pix_fmt == HBHIP_PIX_FMT_NV12 || pix_fmt == HBHIP_PIX_FMT_P010LE; }
/* The key hip_common.c adds to the settings of a `format=nv12 | p010le` entry inside a device-resident run (never a value of
 * the public `format=`): the Format drop-in then makes the planar step only, yuv420p / yuv420p10le, and the run's download
 * adapter repacks it.  hb_hip_filter_init_failed() strips it before the CPU filter sees the settings. */
#define HBHIP_FORMAT_PLANAR_STEP "hip-planar-step"
/* Its sibling on a `format=yuv422p... | yuv444p...` entry inside a run whose target has MORE chroma samples than the job's
 * frames (at equal or higher depth): the Format drop-in takes such a target only where this key stands, i.e. where the
 * frames already are in HBM.  Stripped wherever the key above is. */
#define HBHIP_FORMAT_UP_STEP "hip-up-step"
/* The third: on a `format=p010le` entry inside a run of 8-bit 4:2:0 frames (a yuv420p or nv12 job in front of a 10-bit
 * hardware encoder).  The Format drop-in passes such frames through, and the run's download adapter, which hip_common.c
 * gives format=p010le and this same key, widens them inside its repack (every sample t as t | t << 8).  Only under the key
 * does the adapter take format=p010le on an 8-bit run; it is no part of its settings template.  Stripped wherever the
 * other two are. */
#define HBHIP_FORMAT_WIDEN_STEP "hip-widen-step"
/* The fourth: on a `format=yuv420p10le | yuv422p10le | ...` entry inside a run whose target has FEWER chroma samples than
 * the job's frames and a HIGHER depth (an 8-bit 4:2:2 / 4:4:4 title in front of a 10-bit software encoder).  As with the up
 * step, the Format drop-in takes such a target only where this key stands, i.e. where the frames already are in HBM.
 * Stripped wherever the other three are. */
#define HBHIP_FORMAT_DEEPEN_STEP "hip-deepen-step"
/* The fifth: on a `format=bgra | rgba | argb | abgr` entry inside a run of 8-bit 4:2:0 frames - what hb_get_preview appends to
 * the list it filters a preview picture through (hb.c:945-959, AV_PIX_FMT_RGB32).  Built like the widen step: the Format
 * drop-in passes the frames through, and the run's download adapter, which hip_common.c gives the same `format=` value and
 * this same key, makes the packed picture inside its repack (hbhip_frame_download_rgb32).  Only under the
 * key does the adapter take an RGB format; stripped wherever the other four are. */
#define HBHIP_FORMAT_RGB_STEP "hip-rgb-step"
/* the HB_COLR_MAT_* numbers hbhip_frame_download_rgb32 has a coefficient row for (not RGB, YCgCo, ICtCp, chroma-derived) */
static inline int hbhip_host_rgb32_matrix_ok(int m) { return m == 1 || m == 2 || (m >= 4 && m <= 7) || m == 9 || m == 10; }
/* the four packed orders (FFmpeg's numbers, names of this project's own) and the HBHIP_RGB32_* order of one, else -1 */
#define HBHIP_PIX_FMT_ARGB 25
#define HBHIP_PIX_FMT_RGBA 26
#define HBHIP_PIX_FMT_ABGR 27
#define HBHIP_PIX_FMT_BGRA 28
static inline int hbhip_host_rgb32_order(int pix_fmt)
{
    return pix_fmt == HBHIP_PIX_FMT_BGRA ? HBHIP_RGB32_BGRA : pix_fmt == HBHIP_PIX_FMT_RGBA ? HBHIP_RGB32_RGBA :
           pix_fmt == HBHIP_PIX_FMT_ARGB ? HBHIP_RGB32_ARGB : pix_fmt == HBHIP_PIX_FMT_ABGR ? HBHIP_RGB32_ABGR : -1;
}
static inline void hbhip_host_biplanar_from_buf(hbhip_host_biplanar *f, const hb_buffer_t *b)
{
    for (int p = 0; p < 2; p++)
    {
        f->plane[p]  = b->plane[p].data;
        f->stride[p] = b->plane[p].stride;
    }
}

static inline void hbhip_host_frame_from_buf(hbhip_host_frame *f, const hb_buffer_t *b)
{
    for (int p = 0; p < 3; p++)
    {
        f->plane[p]  = b->plane[p].data;
        f->stride[p] = b->plane[p].stride;
    }
}

/* Allocate an output frame the way every reference filter does
 * (e.g. lapsharp.c:334-339): hb_frame_buffer_init + colour properties. */
static inline hb_buffer_t *hbhip_host_alloc_out(const hb_filter_init_t *o, int width, int height)
{
    hb_buffer_t *out = hb_frame_buffer_init(o->pix_fmt, width, height);
    if (out == NULL) return NULL;
    out->f.color_prim      = o->color_prim;
    out->f.color_transfer  = o->color_transfer;
    out->f.color_matrix    = o->color_matrix;
    out->f.color_range     = o->color_range;
    out->f.chroma_location = o->chroma_location;
    return out;
}

/* ---- device-resident hand-off -------------------------------------
 * Between hb_filter_hip_upload and hb_filter_hip_download the chain's frames stay in HBM:
 * init->hw_pix_fmt is set to AV_PIX_FMT_HBHIP by the upload adapter (as the reference's
 * VideoToolbox path sets hw_pix_fmt for its Metal filters), every HIP filter that sees it
 * takes and produces hb_buffer_t whose storage_type is HBHIP_DEVICE and whose `storage` is
 * an hbhip_frame*, and the download adapter restores host buffers. */
#define AV_PIX_FMT_HBHIP 0x48495001
static inline int hbhip_host_dev_io(const hb_filter_init_t *init) { return init->hw_pix_fmt == AV_PIX_FMT_HBHIP; }
static inline hbhip_frame *hbhip_host_frame_of(const hb_buffer_t *b)
{
    return b->storage_type == HBHIP_DEVICE ? (hbhip_frame *)b->storage : NULL;
}
/* The second storage type, at the two ends of a run only: an NV12 / P010LE picture that lies in device memory already (a
 * hardware decoder's) or stays there (for a hardware encoder).  `storage` is an hbhip_surface*; the buffer has no host
 * planes, f.fmt says NV12 or P010LE.  The reference's COREMEDIA buffers are the precedent again (vt_common.c:413-416).
 * The upload adapter imports such a buffer, the download adapter emits them under surface=1; nothing in between sees one. */
#if defined(HBHIP_IN_LIBHB) && defined(HBHIP_DEVICE) && !defined(HBHIP_SURFACE)
#define HBHIP_SURFACE (HBHIP_DEVICE + 1)      /* a build that spells INTEGRATION.md's enumerators as -D: the second follows the first */
#endif
static inline hbhip_surface *hbhip_host_surface_of(const hb_buffer_t *b)
{
    return b->storage_type == HBHIP_SURFACE ? (hbhip_surface *)b->storage : NULL;
}
/* hb_buffer_t shell around a surface (takes over the caller's reference): f.fmt = o->pix_fmt, NV12 / P010LE */
hb_buffer_t *hbhip_host_wrap_surface(hbhip_surface *s, const hb_filter_init_t *o, int width, int height);
/* HBHIP_ZERO_COPY=0: the drop-ins of a device-resident run copy frames into and out of pictures of their own again
 * (hbhip_filter_push_dev / pull_dev) instead of adopting them (hbhip_filter_use_frames) - for A/B measurements */
static inline int hbhip_host_zero_copy(void) { const char *e = getenv("HBHIP_ZERO_COPY"); return e == NULL || atoi(e) != 0; }
/* hb_buffer_t shell around a device frame (takes over the caller's reference). */
hb_buffer_t *hbhip_host_wrap_frame(hbhip_frame *fr, const hb_filter_init_t *o, int width, int height);
/* Feed `in` (host planes or device frame) to a device filter. */
int hbhip_host_push(hbhip_filter *dev, const hb_buffer_t *in, int64_t tag);
/* Next finished frame of a device filter as a fresh buffer: device-resident when dev_io,
 * else hb_frame_buffer_init() + download.  NULL on error. */
hb_buffer_t *hbhip_host_pull(hbhip_filter *dev, const hb_filter_init_t *o, int width, int height,
                             int dev_io, int64_t *tag);

/* destroy a device filter driven by hbhip_host_simple_work (drops what is still in its pipe) */
void hbhip_host_simple_destroy(hbhip_filter *dev);

extern hb_filter_object_t hb_filter_hip_upload;
extern hb_filter_object_t hb_filter_hip_download;
int hbhip_host_adapter_input_pix_fmt(const hb_filter_object_t *adapter);   /* AV_PIX_FMT_NONE before its init() */

/* Shared body of the stateless (one in, one out) HIP filters: EOF is forwarded
 * (e.g. lapsharp.c:326-331), otherwise the frame goes through the device filter
 * and comes back in a fresh hb_frame_buffer_init() buffer carrying the input's
 * properties (lapsharp.c:334-353). */
int hbhip_host_simple_work(hbhip_filter *dev, const hb_filter_init_t *output, const char *who,
                           int dev_io, hb_buffer_t **buf_in, hb_buffer_t **buf_out);

/* The skeleton of such a drop-in: the FIRST member of its hb_filter_private_s (`s`), so that the four functions below find
 * it behind filter->private_data.
 *   begin  allocates `size` zeroed bytes as the private data, fills input and dev_io from `init` and fetches the pixel
 *          format's descriptor (NULL when there is none: the caller decides what that means).  NULL: out of memory.
 *   fail   init() declines with an HBHIP_ERR_*: "<short_name>(hip): <hbhip_strerror>", the private data freed.  Returns 1.
 *   filter_work / close   what .work and .close point at; close alone is also the silent way out of a failed init(). */
typedef struct
{
    hbhip_filter    *dev;
    hb_filter_init_t input;
    hb_filter_init_t output;
    int              dev_io;
} hbhip_host_simple_t;
void *hbhip_host_simple_begin(hb_filter_object_t *filter, const hb_filter_init_t *init, size_t size,
                              const AVPixFmtDescriptor **desc);
int   hbhip_host_simple_fail(hb_filter_object_t *filter, int rc);
int   hbhip_host_simple_filter_work(hb_filter_object_t *filter, hb_buffer_t **buf_in, hb_buffer_t **buf_out);
void  hbhip_host_simple_close(hb_filter_object_t *filter);
/* planar YUV 4:2:0 / 4:2:2 / 4:4:4 at 8 / 10 / 12 bits */
int   hbhip_host_planar_yuv(const AVPixFmtDescriptor *desc);

/* The HIP drop-ins registered by this library (ids = the CPU filters' ids,
 * SURVEY Appendix D). */
extern hb_filter_object_t hb_filter_nlmeans_hip;
extern hb_filter_object_t hb_filter_lapsharp_hip;
extern hb_filter_object_t hb_filter_unsharp_hip;
extern hb_filter_object_t hb_filter_chroma_smooth_hip;
extern hb_filter_object_t hb_filter_denoise_hip;
extern hb_filter_object_t hb_filter_crop_scale_hip;
extern hb_filter_object_t hb_filter_grayscale_hip;
extern hb_filter_object_t hb_filter_rotate_hip;
extern hb_filter_object_t hb_filter_colorspace_hip;
extern hb_filter_object_t hb_filter_pad_hip;
extern hb_filter_object_t hb_filter_yadif_hip;
extern hb_filter_object_t hb_filter_bwdif_hip;
extern hb_filter_object_t hb_filter_format_hip;
/* the subtitle compositor object rendersub.c can use in place of hb_blend (blend.c:40-46) */
extern hb_blend_object_t  hb_blend_hip;
/* text subtitles: libass's glyph images of the frame's subtitle as the overlay list of a `blend` that is hb_blend_hip, composed
 * on the GPU `frame` lives on (render_ssa_subs, rendersub.c:623-665; INTEGRATION.md has the hook).  HBHIP_OK or HBHIP_ERR_*. */
int hb_blend_hip_set_ass_images(hb_blend_object_t *blend, const hb_buffer_t *frame, const hbhip_ass_image *img, int n,
                                const int crop[4]);
/* bitmap subtitles: the active decoded bitmaps of the frame (render_vobsubs / render_pgs_subs, rendersub.c:381-414, :1016-1067)
 * as the overlay list of a `blend` that is hb_blend_hip - scaled and placed as scale_subtitle (:242-377) would, on the GPU
 * `frame` lives on, once per subtitle (INTEGRATION.md has the hook).  A buffer is known by its address and s.start:
 * rendersub owns the buffers of its sub_list for as long as it lists them.  HBHIP_OK or HBHIP_ERR_*; after a failure the
 * device's list is empty and the caller takes scale_subtitle. */
int hb_blend_hip_set_bitmaps(hb_blend_object_t *blend, const hb_buffer_t *frame, hb_buffer_t *const *subs, int n,
                             const int crop[4]);
/* the frame-difference metric object vfr.c can use in place of hb_motion_metric (motion_metric.c:306-312) */
extern hb_motion_metric_object_t hb_motion_metric_hip;
extern hb_filter_object_t hb_filter_decomb_hip;
extern hb_filter_object_t hb_filter_comb_detect_hip;
extern hb_filter_object_t hb_filter_detelecine_hip;
extern hb_filter_object_t hb_filter_deblock_hip;
extern hb_filter_object_t hb_filter_deband_hip;
extern hb_filter_object_t hb_filter_bm3d_hip;

#ifndef HBHIP_IN_LIBHB
void hbhip_nlmeans_params_from_settings(const char *settings, int depth, hbhip_nlmeans_params *p);   /* bench / tests only */
int  hbhip_deblock_params_from_settings(const char *settings, int depth, int width, int height, int log2_cw, int log2_ch,
                                        hbhip_deblock_params *p);                                    /* tests / tools only */
int  hbhip_deband_params_from_settings(const char *settings, int depth, hbhip_deband_params *p);  /* tests / tools only */
#endif

/* hb_filter_get() analogue (common.c:5331-5495) for the HIP drop-ins. */
hb_filter_object_t *hbhip_filter_get(int filter_id);

#endif
