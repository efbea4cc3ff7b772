/* hip_common.h — the two calls libhb's work.c makes to put the HIP drop-ins into a job (hip_common.c).
 * Counterpart of handbrake/platform/macosx/vt_common.h:hb_vt_setup_hw_filters. */
#ifndef HBHIP_HIP_COMMON_H
#define HBHIP_HIP_COMMON_H

/* sanitize_filter_list_post (work.c:1515-1523): swap CPU filters for HIP drop-ins in place, bracket runs of
 * drop-ins with the upload / download adapters. */
void hb_hip_setup_hw_filters(hb_job_t *job);
/* the filter init loop (work.c:1855-1868), when init() of job->list_filter[index] failed: if that filter is a HIP
 * drop-in, put the CPU filter of the same id and settings back in its place (fixing the adapters around it) and
 * return > 0 - the loop then CONTINUES AT index - (return value - 1) instead of dropping the filter; 0 = not ours. */
int  hb_hip_filter_init_failed(hb_job_t *job, int index, hb_filter_init_t *init);
/* do_job's clean-up, once the job's filters have been closed (work.c:2311-2321): the HIP stream the job had leased goes
 * back to the pool (libhb/hbhip_registry.c: concurrent jobs on one GPU run on streams of their own) */
void hb_hip_job_close(hb_job_t *job);
/* hb_avfilter_combine (hbavfilter.c:520-541): an aliased id whose object is a drop-in is a real filter */
int  hb_hip_filter_is_hip(const hb_filter_object_t *filter);
/* a filter that only handles the hb_buffer_t around a picture (vfr, rendersub, rpu): a member of a device-resident
 * run like the ones are_filters_supported() lists (platform/macosx/vt_common.c:424-448) */
int  hb_hip_filter_is_hw_transparent(const hb_filter_object_t *filter);

/* ---- the title scan (scan_hip.c): what scan.c:972-1052 computes from a preview, on the GPU ----
 * open once the preview size is known, picture() for every preview - a host yuv420p buffer, or one whose picture lies in
 * HBM -, close at the end of the title.  Every call answers 0 on success and non-zero where the caller keeps its CPU loops:
 * no GPU, HBHIP_DISABLE set, a picture that is not 8-bit 4:2:0 of even size >= 8 x 8, or of another size than open() was
 * given.  INTEGRATION.md has the hook. */
typedef struct hb_hip_scan_s hb_hip_scan_t;
typedef struct hb_hip_scan_picture_s
{
    int combed;                       /* hb_detect_comb( vid_buf, 10, 30, 9, 10, 30, 9 ), scan.c:973 */
    int top, bottom, left, right;     /* as scan.c:999-1044 leaves them                              */
    int recorded;                     /* the test of scan.c:1049: hand the four to record_crop       */
} hb_hip_scan_picture_t;
int  hb_hip_scan_open(hb_hip_scan_t **scan, int width, int height);
int  hb_hip_scan_picture(hb_hip_scan_t *scan, hb_buffer_t *vid_buf, hb_hip_scan_picture_t *out);
/* the same and, for a scan with store_previews set, the preview's file: what hb_save_preview( .., HB_PREVIEW_FORMAT_JPG )
 * writes (hb.c:583-629, quality 90) encoded on the GPU from the same picture, in a malloc()ed buffer that becomes the
 * caller's - write its *jpeg_size bytes under hb_get_tempory_filename's name and free() it.  The file is libjpeg's for these
 * planes with its default DCT (the reference asks for TJFLAG_FASTDCT: other AC rounding, same container and tables).  The
 * encoder is made at the first call.  Non-zero: nothing was returned, *jpeg is NULL. */
int  hb_hip_scan_picture_preview(hb_hip_scan_t *scan, hb_buffer_t *vid_buf, hb_hip_scan_picture_t *out, uint8_t **jpeg, size_t *jpeg_size);
void hb_hip_scan_close(hb_hip_scan_t **scan);

#endif
