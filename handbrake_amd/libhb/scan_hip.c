/* scan_hip.c — HIP-backed helper for the per-pixel part of libhb's title scan: what scan.c:972-1052 computes from every
 * preview, hb_detect_comb( vid_buf, 10, 30, 9, 10, 30, 9 ) (hb.c:1088-1167) and the black-border walk over row_all_dark /
 * column_all_dark (scan.c:456-509, :986-1052).
 *
 * scan.c opens the helper once it knows a title's preview size, hands it every preview and keeps its CPU loops for the
 * cases the helper declines - every call answers non-zero then: no GPU, HBHIP_DISABLE set, a picture that is not the 8-bit
 * yuv420p of even size the scan decodes to (decavcodec.c:1359-1369), or one of another size than the helper was opened
 * for.  The crop record, its sort and the median choice (scan.c:512-561, :1263-1340) stay in scan.c: a handful of ints.
 *
 * A preview that lies in HBM (storage_type HBHIP_DEVICE: an hbhip_frame; HBHIP_SURFACE: a decoder's NV12 picture, imported
 * first) is analysed where it is and 48 bytes come back; a host buffer is uploaded through the pipelined upload.
 *
 * With store_previews set scan.c:979-982 also writes every preview as a JPEG (hb_save_preview, hb.c:583-629: quality 90 on
 * one CPU thread).  hb_hip_scan_picture_preview() queues that file's encode (hbhip_jpeg_*) behind the analysis of the same
 * device picture and hands the finished file back: a preview in HBM is never downloaded.  INTEGRATION.md has both hooks.
 */
#include "hbhip_host.h"
#include "hip_common.h"

struct hb_hip_scan_s
{
    hbhip_ctx  *ctx;
    hbhip_scan *dev;
    hbhip_jpeg *jpeg;                  /* made at the first hb_hip_scan_picture_preview() */
    int         width, height;
};

#define SCAN_PREVIEW_QUALITY 90        /* hb.c:606 */

static int scan_disabled(void)
{
    const char *off = getenv("HBHIP_DISABLE");
    return off != NULL && atoi(off) != 0;
}

int hb_hip_scan_open(hb_hip_scan_t **scan, int width, int height)
{
    if (scan == NULL) return 1;
    *scan = NULL;
    if (scan_disabled() || hbhip_device_count() <= 0) return 1;
    hb_hip_scan_t *s = calloc(1, sizeof(*s));
    if (s == NULL) return 1;
    s->ctx = hbhip_host_ctx();
    s->width = width;
    s->height = height;
    const int rc = s->ctx == NULL ? HBHIP_ERR_NODEVICE : hbhip_scan_create(s->ctx, width, height, &s->dev);
    if (rc != HBHIP_OK)
    {
        hb_deep_log(2, "scan(hip): %dx%d previews stay on the CPU (%s)", width, height, hbhip_strerror(rc));
        free(s);
        return 1;
    }
    *scan = s;
    return 0;
}

void hb_hip_scan_close(hb_hip_scan_t **scan)
{
    if (scan == NULL || *scan == NULL) return;
    hbhip_jpeg_destroy((*scan)->jpeg);
    hbhip_scan_destroy((*scan)->dev);
    free(*scan);
    *scan = NULL;
}

/* the analysis of one preview and, with `jpeg` given, its file: queued together on the picture in HBM */
static int scan_picture(hb_hip_scan_t *s, hb_buffer_t *vid_buf, hb_hip_scan_picture_t *out, uint8_t **jpeg, size_t *jpeg_size)
{
    if (s == NULL || vid_buf == NULL || out == NULL || scan_disabled()) return 1;
    if (vid_buf->f.width != s->width || vid_buf->f.height != s->height) return 1;
    uint8_t *file = NULL;
    size_t file_cap = 0, file_size = 0;
    hbhip_frame   *fr = hbhip_host_frame_of(vid_buf);
    hbhip_surface *sf = hbhip_host_surface_of(vid_buf);
    void *token = NULL;
    int rc = HBHIP_OK, own = 0;
    if (fr == NULL)
    {
        /* a host picture or a decoder's surface: into a frame of the pool first */
        if (sf != NULL ? vid_buf->f.fmt != HBHIP_PIX_FMT_NV12 : vid_buf->f.fmt != AV_PIX_FMT_YUV420P) return 1;
        if ((s->width | s->height) & 1) return 1;
        if (hbhip_frame_alloc(s->ctx, s->width, s->height, 8, 1, 1, &fr) != HBHIP_OK) return 1;
        own = 1;
        if (sf != NULL)
            rc = hbhip_frame_import_surface_async(fr, sf, &token);
        else
        {
            hbhip_host_frame hf;
            hbhip_host_frame_from_buf(&hf, vid_buf);
            rc = hbhip_frame_upload_async(fr, &hf, &token);
        }
    }
    hbhip_scan_result r;
    memset(&r, 0, sizeof(r));
    if (rc == HBHIP_OK) rc = hbhip_scan_push(s->dev, fr, vid_buf->s.flags, NULL);
    if (rc == HBHIP_OK)
    {
        /* the file's launches behind the analysis's on the same stream: the one wait for the file covers both */
        int rj = HBHIP_OK;
        if (jpeg != NULL)
        {
            if (s->jpeg == NULL) rj = hbhip_jpeg_create(s->ctx, s->width, s->height, SCAN_PREVIEW_QUALITY, &s->jpeg);
            if (rj == HBHIP_OK)
            {
                file_cap = hbhip_jpeg_bound(s->jpeg);        /* (pages nobody writes cost nothing; cut to size below) */
                if ((file = malloc(file_cap)) == NULL) rj = HBHIP_ERR_NOMEM;
            }
            if (rj == HBHIP_OK) rj = hbhip_jpeg_push(s->jpeg, fr);
            if (rj == HBHIP_OK) rj = hbhip_jpeg_pull(s->jpeg, file, file_cap, &file_size);
        }
        rc = hbhip_scan_pull(s->dev, &r);
        if (rc == HBHIP_OK) rc = rj;
    }
    if (token != NULL)                                  /* the copy reads vid_buf, which is the caller's again on return */
    {
        const int done = hbhip_ctx_upload_done(s->ctx, token, 1);
        if (rc == HBHIP_OK) rc = done;
    }
    if (own) hbhip_frame_release(fr);
    if (rc != HBHIP_OK)
    {
        if (rc != HBHIP_ERR_UNSUPPORTED) hb_error("scan(hip): %s", hbhip_strerror(rc));
        free(file);
        return 1;
    }
    if (file != NULL)
    {
        uint8_t *fit = realloc(file, file_size);
        *jpeg = fit != NULL ? fit : file;
        *jpeg_size = file_size;
    }
    out->combed = r.combed;
    out->top = r.top;
    out->bottom = r.bottom;
    out->left = r.left;
    out->right = r.right;
    out->recorded = r.recorded;
    return 0;
}

int hb_hip_scan_picture(hb_hip_scan_t *s, hb_buffer_t *vid_buf, hb_hip_scan_picture_t *out)
{
    return scan_picture(s, vid_buf, out, NULL, NULL);
}

int hb_hip_scan_picture_preview(hb_hip_scan_t *s, hb_buffer_t *vid_buf, hb_hip_scan_picture_t *out, uint8_t **jpeg, size_t *jpeg_size)
{
    if (jpeg == NULL || jpeg_size == NULL) return 1;
    *jpeg = NULL;
    *jpeg_size = 0;
    return scan_picture(s, vid_buf, out, jpeg, jpeg_size);
}
