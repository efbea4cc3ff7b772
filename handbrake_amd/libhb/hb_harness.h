/* hb_harness.h — C interface of the filter-chain test/bench driver
 * (hb_harness.c).  Plain C types only so Python can bind it with ctypes. */
#ifndef HBHIP_HARNESS_H
#define HBHIP_HARNESS_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct hbh_chain_s hbh_chain_t;

typedef struct hbh_frame_info_s
{
    int     is_eof;
    int64_t start;
    int64_t stop;
    int     flags;
    int     combed;
    int     width;
    int     height;
    int     fmt;
    int     nplanes;
    int     plane_width[4];
    int     plane_height[4];
    int     plane_stride[4];
} hbh_frame_info_t;

/* protos[i] = address of a registered hb_filter_object_t (e.g. &hb_filter_nlmeans);
 * settings[i] = "key=value:key=value" or NULL. */
hbh_chain_t *hbh_chain_open(int nstages, void *const *protos, const char *const *settings,
                            int pix_fmt, int width, int height,
                            int vrate_num, int vrate_den);
/* The same chain built the way do_job() builds it: filters by ID from the registered (CPU) objects, the HIP swap
 * (hb_hip_setup_hw_filters) when use_hip, init with drop / CPU-fallback on failure (work.c:1820-1870). */
hbh_chain_t *hbh_job_open(int nfilters, const int *ids, const char *const *settings, int pix_fmt, int width, int height,
                          int vrate_num, int vrate_den, int use_hip);
/* A preview's filters built the way hb_get_preview builds them (hb.c:801-1063) with the hook of INTEGRATION.md 2b: the job's
 * filters by id, then the display rescale for `par` (rescale != 0) and `format=<pix_fmt_name>` (not NULL), added in front of
 * the init loop; the HIP swap when use_hip; the loop keeps what hb.c:850-861 keeps plus Format and the adapters.  The frames
 * are yuv420p.  Never threaded.  hbh_chain_stage: stage i's hb_filter_object_t (NULL beyond the last). */
hbh_chain_t *hbh_preview_open(int nfilters, const int *ids, const char *const *settings, int width, int height,
                              int par_num, int par_den, int rescale, const char *pix_fmt_name, int use_hip);
void *hbh_chain_stage(hbh_chain_t *c, int i);
/* job->hw_device_index (common.h:991) of jobs opened from now on: which GPU the job's drop-ins run on; -1 = not set */
void hbh_set_job_device(int index);
/* jobs opened from now on carry one subtitle track of this source (enum subsource: 0 VOBSUB, 6 PGSSUB, ...) marked for
 * burn-in, which is what makes rendersub.c's init find its track (:1199-1209); -1 = none */
void hbh_set_job_subtitle(int source);
/* "|"-separated names of the stages as initialised; returns their count */
int hbh_chain_describe(hbh_chain_t *c, char *buf, int len);
/* Chains opened from now on run every stage on its own thread with a fifo in front (filter_loop, work.c:2527-2600);
 * output is collected after hbh_chain_push_eof(), which joins the stages. */
void hbh_set_threaded(int on);
/* Threaded chains opened from now on drop the frames their last stage makes (a consumer that keeps up, e.g. an
 * encoder) and only count them: hbh_chain_produced() = frames made so far, callable while the stages run. */
void hbh_set_discard_output(int on);
int  hbh_chain_produced(hbh_chain_t *c);
/* threaded chains: milliseconds stage's thread has spent inside its filter's work() so far (which stage a pipeline waits for) */
double hbh_chain_stage_busy_ms(hbh_chain_t *c, int stage);
/* Colour description of the source for chains opened from now on (init->color_*; AVCOL_* numbers,
 * range 1 = tv, 2 = pc).  Default bt709 / tv. */
void hbh_set_source_color(int prim, int transfer, int matrix, int range);
/* Chroma sample location of the source for chains opened from now on (init->chroma_location and every frame's
 * f.chroma_location; AVCHROMA_LOC_* numbers).  Default 1 (left). */
void hbh_set_source_chroma_location(int chroma_location);
int  hbh_chain_push(hbh_chain_t *c, const uint8_t *const plane[3], const int stride[3],
                    int64_t start, int64_t stop, int flags, int combed);
/* `count` frames from `n_unique` prepared pictures (plane[3 * k + p], one stride per plane), numbered first, first + 1, ...:
 * filled by `nthreads` threads (the decoder's part in libhb), pushed in order; returns when the last one is in */
int  hbh_chain_feed(hbh_chain_t *c, const uint8_t *const *plane, const int stride[3], int n_unique, int first, int count,
                    int64_t duration, int flags, int nthreads);
/* Device surfaces at the ends of a chain (an hbhip_surface, include/hbhip.h; pix_fmt NV12 / P010LE): push takes over the
 * caller's reference, shown from pts for 3003 ticks; the feeder takes a reference per buffer through `retain` (the address of
 * hbhip_surface_retain) and numbers the buffers like hbh_chain_feed; pop hands the next output's surface and its reference
 * to the caller - 1 when the next output is not a surface buffer (it stays), -1 when there is none.  hbh_chain_peek
 * describes a surface buffer with nplanes = 0 (no host planes). */
int  hbh_chain_push_surface(hbh_chain_t *c, void *surface, int flags, int64_t pts);
int  hbh_chain_feed_surfaces(hbh_chain_t *c, void *const *surfaces, int n_unique, int first, int count, int64_t duration,
                             int flags, void (*retain)(void *));
int  hbh_chain_pop_surface(hbh_chain_t *c, void **surface);
int  hbh_chain_push_eof(hbh_chain_t *c);
int  hbh_chain_pending(hbh_chain_t *c);
int  hbh_chain_peek(hbh_chain_t *c, hbh_frame_info_t *info);
int  hbh_chain_pop(hbh_chain_t *c, uint8_t *const plane[3], const int stride[3]);
/* the layout hb_frame_buffer_init gives a frame (no chain needed); plane_width[3]: bytes from plane 0 to the last plane */
int  hbh_frame_layout(int pix_fmt, int width, int height, hbh_frame_info_t *info);
void hbh_chain_output_geometry(hbh_chain_t *c, int *width, int *height, int *vrate_num, int *vrate_den);
void hbh_chain_close(hbh_chain_t *c);

/* Run a frame-difference metric object (address of an hb_motion_metric_object_t) on two lumas. */
int hbh_motion_metric_run(const void *proto, int pix_fmt, int width, int height,
                          const uint8_t *luma_a, int stride_a, const uint8_t *luma_b, int stride_b, float *out);

/* The title scan's helper (libhb/scan_hip.c) on one preview: open_fn / picture_fn / close_fn are the addresses of
 * hb_hip_scan_open / _picture / _close; the helper is opened for open_width x open_height and handed a width x height buffer
 * of pix_fmt - a copy of plane / stride (storage_kind 0), or the shell around a picture in device memory whose reference the
 * call takes over: `storage` an hbhip_frame (1) or an NV12 hbhip_surface (2).  flags: the buffer's s.flags.  out: combed, top,
 * bottom, left, right, recorded.  0, 1 when open declined, 2 when picture did, -1 on an error of the harness's own. */
int hbh_scan_run(const void *open_fn, const void *picture_fn, const void *close_fn, int pix_fmt, int open_width, int open_height,
                 int width, int height, uint8_t *const plane[3], const int stride[3], void *storage, int storage_kind,
                 int flags, int out[6]);
/* The same through hb_hip_scan_picture_preview (preview_fn): the analysis and the preview's JPEG.  The file the helper
 * returns is copied to `jpeg` when its *jpeg_size bytes fit jpeg_cap, and freed; *returned_buffer: the helper left a buffer
 * behind (it must not when it answers non-zero). */
int hbh_scan_preview_run(const void *open_fn, const void *preview_fn, const void *close_fn, int pix_fmt, int open_width,
                         int open_height, int width, int height, uint8_t *const plane[3], const int stride[3], void *storage,
                         int storage_kind, int flags, int out[6], uint8_t *jpeg, size_t jpeg_cap, size_t *jpeg_size,
                         int *returned_buffer);

/* One rendered subtitle bitmap: 4 planes (Y, Cb, Cr, alpha; 8-bit), placed at (x, y) of the frame. */
typedef struct
{
    const uint8_t *plane[4];
    int            stride[4];
    int            x, y, width, height;
} hbh_overlay_t;
/* Run a compositor object (address of an hb_blend_object_t) on one frame, in place. */
int hbh_blend_run(const void *proto, int pix_fmt, int width, int height, int chroma_location, int overlay_fmt,
                  uint8_t *const plane[3], const int stride[3], int n_overlays, const hbh_overlay_t *ov, int passes);

/* The same for a text subtitle, playing render_ssa_subs (rendersub.c:623-665) with a compositor that takes libass's glyph
 * images itself: set_images(blend, frame, lists[k], n_images[k], crop) for every list in order - the address of
 * hb_blend_hip_set_ass_images, each list an array of hbhip_ass_image (include/hbhip.h) - then work() once with an empty overlay
 * list.  dev_frame != NULL: the frame is that device-resident one (an hbhip_frame, whose reference the call takes over) in
 * place of plane / stride; the frame work() returned comes back in *dev_frame_out, with a reference that is the caller's. */
int hbh_blend_run_ass(const void *proto, const void *set_images, int pix_fmt, int width, int height, int chroma_location,
                      int overlay_fmt, uint8_t *const plane[3], const int stride[3], void *dev_frame, void **dev_frame_out,
                      int n_lists, const int *n_images, const void *const *lists, const int crop[4]);

/* The same for bitmap subtitles, playing render_vobsubs / render_pgs_subs (rendersub.c:381-414, :1016-1067) with a compositor
 * that scales and places the decoded bitmaps itself.  `subs` are the n_subs decoded subtitles of the track - each becomes one
 * buffer, as in rendersub's sub_list, so that a subtitle listed by several calls is the same buffer in all of them.  Call k
 * hands set_bitmaps(blend, frame, buffers, n_listed[k], crop) the buffers lists[k][0 .. n_listed[k]) index into `subs` - the
 * address of hb_blend_hip_set_bitmaps - in order; then work() runs once with an empty overlay list.  dev_frame / dev_frame_out
 * as above. */
typedef struct
{
    hbh_overlay_t ov;                     /* the bitmap, 4:4:4, at (x, y) of its canvas */
    int           window_width, window_height;
    int64_t       start;
} hbh_bitmap_t;
int hbh_blend_run_bitmaps(const void *proto, const void *set_bitmaps, int pix_fmt, int width, int height, int chroma_location,
                          int overlay_fmt, uint8_t *const plane[3], const int stride[3], void *dev_frame, void **dev_frame_out,
                          int n_subs, const hbh_bitmap_t *subs, int n_calls, const int *n_listed, const int *const *lists,
                          const int crop[4]);

/* a decoded bitmap subtitle for the job's burn-in track (see hbh_set_job_subtitle): shown from start to stop (90 kHz, stop < 0:
 * until the next one) on a window_w x window_h canvas */
int hbh_chain_push_subtitle(hbh_chain_t *c, const hbh_overlay_t *ov, int64_t start, int64_t stop, int window_w, int window_h);

void hbhip_set_log_level(int level);

#ifdef __cplusplus
}
#endif
#endif
