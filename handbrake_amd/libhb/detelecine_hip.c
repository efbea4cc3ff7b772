/* detelecine_hip.c — HIP-backed drop-in for libhb's detelecine filter object
 * (libhb/detelecine.c:113-130 template/object, :1006-1095 init, :1116-1275 work, :1097-1113 close).
 * Same keys, the same defaults (skip 1 / 1 / 4 / 4, strict-breaks -1, plane 0, parity -1) and the same
 * safety-zone clamping of the margins (:1025-1043).
 *
 * The pullup state machine and its kernels live with the pixels in csrc/detelecine.hip; this file keeps what is about
 * hb_buffer_t: the picture flags that say which field comes first and whether one repeats (:1162-1186), the output's
 * properties (those of the input just pushed, :1261), EOF.  Every input yields at most one output.  Inside a
 * device-resident run the frames go in and out as frames (no copy at either end); a frame woven from one input
 * picture's own two fields is that picture, handed on a second time.
 *
 * Declined in init() (the job then keeps the CPU filter, hb_hip_filter_init_failed): a plane with an odd number of
 * rows, skip margins wider than the metric plane, anything but 8 / 10 / 12-bit planar YUV.
 */
#include "hbhip_host.h"

struct hb_filter_private_s
{
    hbhip_filter    *dev;
    int64_t          next_tag;
    int              dev_io;
    hb_filter_init_t input;
    hb_filter_init_t output;
};

static int  detelecine_hip_init(hb_filter_object_t *filter, hb_filter_init_t *init);
static int  detelecine_hip_work(hb_filter_object_t *filter, hb_buffer_t **buf_in, hb_buffer_t **buf_out);
static void detelecine_hip_close(hb_filter_object_t *filter);

static const char detelecine_hip_template[] =
    "skip-left=^"HB_INT_REG"$:skip-right=^"HB_INT_REG"$:"
    "skip-top=^"HB_INT_REG"$:skip-bottom=^"HB_INT_REG"$:"
    "strict-breaks=^"HB_BOOL_REG"$:plane=^([012])$:parity=^([01])$:"
    "disable=^"HB_BOOL_REG"$";

hb_filter_object_t hb_filter_detelecine_hip =
{
    .id                = HB_FILTER_DETELECINE,
    .enforce_order     = 1,
    .name              = "Detelecine (pullup) (HIP)",
    .short_name        = "detelecine",
    .settings          = NULL,
    .init              = detelecine_hip_init,
    .work              = detelecine_hip_work,
    .close             = detelecine_hip_close,
    .settings_template = detelecine_hip_template,
};

static int detelecine_hip_init(hb_filter_object_t *filter, hb_filter_init_t *init)
{
    hb_filter_private_t *pv = calloc(1, sizeof(*pv));
    if (pv == NULL) return -1;
    filter->private_data = pv;
    pv->input = *init;
    pv->dev_io = hbhip_host_dev_io(init);

    const AVPixFmtDescriptor *desc = av_pix_fmt_desc_get(init->pix_fmt);
    if (desc == NULL || desc->nb_components != 3) goto fail;

    hbhip_detelecine_params p;
    memset(&p, 0, sizeof(p));
    int top = 4, bottom = 4, left = 1, right = 1;          /* :1022-1026 */
    p.strict_breaks = -1;
    p.plane = 0;
    p.parity = -1;
    hb_dict_extract_int(&top,    filter->settings, "skip-top");
    hb_dict_extract_int(&bottom, filter->settings, "skip-bottom");
    hb_dict_extract_int(&left,   filter->settings, "skip-left");
    hb_dict_extract_int(&right,  filter->settings, "skip-right");
    p.skip_top    = top    > 4 ? top    : 4;               /* the safety zones, :1035-1039 */
    p.skip_bottom = bottom > 4 ? bottom : 4;
    p.skip_left   = left   > 1 ? left   : 1;
    p.skip_right  = right  > 1 ? right  : 1;
    hb_dict_extract_int(&p.strict_breaks, filter->settings, "strict-breaks");
    hb_dict_extract_int(&p.plane,         filter->settings, "plane");
    hb_dict_extract_int(&p.parity,        filter->settings, "parity");
    if (p.plane < 0 || p.plane >= desc->nb_components) p.plane = 0;      /* :1074-1077 */

    hbhip_ctx *ctx = hbhip_host_ctx_for_role(init, 1);      /* the deinterlacing side of the job, as decomb */
    if (ctx == NULL) goto fail;
    int rc = hbhip_detelecine_create(ctx, &p, init->geometry.width, init->geometry.height, desc->comp[0].depth,
                                     desc->log2_chroma_w, desc->log2_chroma_h, &pv->dev);
    if (rc != HBHIP_OK)
    {
        hb_error("detelecine(hip): %s", hbhip_strerror(rc));
        goto fail;
    }
    if (pv->dev_io && hbhip_host_zero_copy()) hbhip_filter_use_frames(pv->dev);
    pv->output = *init;
    return 0;
fail:
    free(pv);
    filter->private_data = NULL;
    return -1;
}

static void detelecine_hip_close(hb_filter_object_t *filter)
{
    hb_filter_private_t *pv = filter->private_data;
    if (pv == NULL) return;
    if (pv->dev != NULL) hbhip_filter_destroy(pv->dev);
    free(pv);
    filter->private_data = NULL;
}

static int detelecine_hip_work(hb_filter_object_t *filter, hb_buffer_t **buf_in, hb_buffer_t **buf_out)
{
    hb_filter_private_t *pv = filter->private_data;
    hb_buffer_t *in = *buf_in;

    if (in->s.flags & HB_BUF_FLAG_EOF)                      /* :1123-1128: nothing is flushed */
    {
        *buf_out = in;
        *buf_in = NULL;
        return HB_FILTER_DONE;
    }

    int rc;
    hbhip_frame *fr = hbhip_host_frame_of(in);
    if (fr != NULL)
        rc = hbhip_detelecine_push_frame(pv->dev, fr, pv->next_tag++, in->s.flags);    /* no copy: the frame is the picture */
    else
    {
        hbhip_host_frame hf;
        hbhip_host_frame_from_buf(&hf, in);
        rc = hbhip_detelecine_push(pv->dev, &hf, pv->next_tag++, in->s.flags);
    }
    if (rc != HBHIP_OK)
    {
        hb_error("detelecine(hip): push: %s", hbhip_strerror(rc));
        return HB_FILTER_FAILED;
    }
    if (hbhip_filter_pending(pv->dev) > 0)
    {
        hb_buffer_t *out = hbhip_host_pull(pv->dev, &pv->output, in->f.width, in->f.height, pv->dev_io, NULL);
        if (out == NULL)
        {
            hb_error("detelecine(hip): pull failed");
            return HB_FILTER_FAILED;
        }
        hb_buffer_copy_props(out, in);                       /* :1261 */
        *buf_out = out;
    }
    return HB_FILTER_OK;
}
