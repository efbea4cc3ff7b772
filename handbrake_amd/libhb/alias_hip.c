/* alias_hip.c — HIP-backed drop-ins for the reference's libavfilter "alias" filters:
 *   hb_filter_crop_scale_hip  (libhb/cropscale.c:21-185)
 *   hb_filter_grayscale_hip   (libhb/grayscale.c:13-68)
 *   hb_filter_rotate_hip      (libhb/rotate.c:15-270)
 *
 * In the reference these objects have .skip = 1 and no work(): their init() only
 * builds settings for FFmpeg's crop/zscale, monochrome and transpose/hflip/vflip,
 * which hb_avfilter_combine later merges into one HB_FILTER_AVFILTER graph
 * (hbavfilter.c:510-622).  Here they are real filters (skip = 0, own work), exactly
 * as the reference's own HB_FILTER_*_VT GPU variants are; they must therefore be
 * left out of hb_avfilter_combine's switch.  Same settings keys,
 * same mutation of init->geometry / PAR / crop for the filters downstream.
 * The pixel arithmetic is FFmpeg's / zimg's in the reference and is NOT in its tree:
 * parity is pinned to oracle/alias_oracle.c only ("parity unpinned").
 */
#include "hbhip_host.h"

struct hb_filter_private_s { hbhip_host_simple_t s; };

/* ---- crop + scale ------------------------------------------------------------------ */
static int crop_scale_hip_init(hb_filter_object_t *filter, hb_filter_init_t *init);

static const char crop_scale_hip_template[] =
    "width=^"HB_INT_REG"$:height=^"HB_INT_REG"$:"
    "crop-top=^"HB_INT_REG"$:crop-bottom=^"HB_INT_REG"$:"
    "crop-left=^"HB_INT_REG"$:crop-right=^"HB_INT_REG"$";

hb_filter_object_t hb_filter_crop_scale_hip =
{
    .id                = HB_FILTER_CROP_SCALE,
    .enforce_order     = 1,
    .name              = "Crop and Scale (HIP)",
    .short_name        = "cropscale",
    .settings          = NULL,
    .init              = crop_scale_hip_init,
    .work              = hbhip_host_simple_filter_work,
    .close             = hbhip_host_simple_close,
    .settings_template = crop_scale_hip_template,
};

#ifdef HBHIP_IN_LIBHB
#define limit_rational hb_limit_rational
#else
/* hb_limit_rational (common.c:3912-3938), the same arithmetic: reduce by the gcd (hb_reduce64, :3947-3968); if a term
 * still reaches the limit, the larger one becomes the limit and the other is scaled by a double and truncated */
static void limit_rational(int *x, int *y, int64_t num, int64_t den, int limit)
{
    int64_t n = num, d = den;
    while (d) { int64_t t = d; d = n % d; n = t; }
    if (n) { num /= n; den /= n; }
    if (num < limit && den < limit)
    {
        *x = (int)num;
        *y = (int)den;
        return;
    }
    if (num > den)
    {
        double div = (double)limit / num;
        num = limit;
        den *= div;
    }
    else
    {
        double div = (double)limit / den;
        den = limit;
        num *= div;
    }
    *x = (int)num;
    *y = (int)den;
}
#endif

static int crop_scale_hip_init(hb_filter_object_t *filter, hb_filter_init_t *init)
{
    const AVPixFmtDescriptor *desc;
    hb_filter_private_t *pv = hbhip_host_simple_begin(filter, init, sizeof(*pv), &desc);
    if (pv == NULL || desc == NULL) { hbhip_host_simple_close(filter); return 1; }   /* (no message) */

    hbhip_cropscale_params p;
    memset(&p, 0, sizeof(p));
    hb_dict_extract_int(&p.crop_top, filter->settings, "crop-top");          /* cropscale.c:68-71 */
    hb_dict_extract_int(&p.crop_bottom, filter->settings, "crop-bottom");
    hb_dict_extract_int(&p.crop_left, filter->settings, "crop-left");
    hb_dict_extract_int(&p.crop_right, filter->settings, "crop-right");
    const int cropped_width  = init->geometry.width - p.crop_left - p.crop_right;
    const int cropped_height = init->geometry.height - p.crop_top - p.crop_bottom;
    p.width = cropped_width;
    p.height = cropped_height;
    hb_dict_extract_int(&p.width, filter->settings, "width");                /* :93-94 */
    hb_dict_extract_int(&p.height, filter->settings, "height");
    /* crop_scale_init has two scalers (cropscale.c:97-165): zscale=filter=lanczos where hb_av_can_use_zscale() agrees
     * (hbffmpeg.c:870-915: every dimension even, a planar YUV format), else swscale `lanczos+accurate_rnd`, which computes
     * something else.  The drop-in follows the same rule with the restatement of the same library (both parity unpinned:
     * neither library is in the reference tree).  The swscale form covers 8-bit planes (hScale8To15 / yuv2planeX_8) and
     * 10 / 12-bit planes (hScale16To15 / yuv2planeX_10, _12). */
    const int odd = (cropped_width & 1) || (cropped_height & 1) || (p.width & 1) || (p.height & 1);
    /* The swscale restatement has never met a real libswscale (vf_scale's chroma positions from chroma_location, its
     * field handling and its cascaded contexts for large ratios are what could differ silently), and unlike the zimg form
     * it has no second implementation to be held against: it is OPT-IN (HBHIP_SWSCALE=1).  Without it an odd size
     * declines here and the job keeps the reference's CPU filter (hb_hip_filter_init_failed). */
    if (odd)
    {
        const char *sws = getenv("HBHIP_SWSCALE");
        if (sws == NULL || atoi(sws) == 0) return hbhip_host_simple_fail(filter, HBHIP_ERR_UNSUPPORTED);
    }

    hbhip_ctx *ctx = hbhip_host_ctx_for(init);
    if (ctx == NULL) return hbhip_host_simple_fail(filter, HBHIP_ERR_NODEVICE);
    int rc = odd ? hbhip_cropscale_sws_create(ctx, &p, init->geometry.width, init->geometry.height, desc->comp[0].depth,
                                              desc->log2_chroma_w, desc->log2_chroma_h, &pv->s.dev)
                 /* zscale shifts chroma by the frame's chroma_location (hbffmpeg.c:130; cropscale.c:150-157 sets neither
                  * chromal nor chromal_in); the location itself goes on unchanged to the next filter */
                 : hbhip_cropscale_create_sited(ctx, &p, init->geometry.width, init->geometry.height, desc->comp[0].depth,
                                                desc->log2_chroma_w, desc->log2_chroma_h, init->chroma_location, &pv->s.dev);
    if (rc != HBHIP_OK) return hbhip_host_simple_fail(filter, rc);

    init->crop[0] = p.crop_top;                                              /* :168-178 */
    init->crop[1] = p.crop_bottom;
    init->crop[2] = p.crop_left;
    init->crop[3] = p.crop_right;
    limit_rational(&init->geometry.par.num, &init->geometry.par.den,
                   (int64_t)init->geometry.par.num * p.height * cropped_width,
                   (int64_t)init->geometry.par.den * p.width * cropped_height, 65535);
    init->geometry.width = p.width;
    init->geometry.height = p.height;
    pv->s.output = *init;
    return 0;
}

/* ---- grayscale ----------------------------------------------------------------------- */
static int grayscale_hip_init(hb_filter_object_t *filter, hb_filter_init_t *init);

static const char grayscale_hip_template[] =
    "cb=^"HB_FLOAT_REG"$:cr=^"HB_FLOAT_REG"$:size=^"HB_FLOAT_REG"$:high=^"HB_FLOAT_REG"$";

hb_filter_object_t hb_filter_grayscale_hip =
{
    .id                = HB_FILTER_GRAYSCALE,
    .enforce_order     = 1,
    .name              = "Grayscale (HIP)",
    .short_name        = "grayscale",
    .settings          = NULL,
    .init              = grayscale_hip_init,
    .work              = hbhip_host_simple_filter_work,
    .close             = hbhip_host_simple_close,
    .settings_template = grayscale_hip_template,
};

static int grayscale_hip_init(hb_filter_object_t *filter, hb_filter_init_t *init)
{
    const AVPixFmtDescriptor *desc;
    hb_filter_private_t *pv = hbhip_host_simple_begin(filter, init, sizeof(*pv), &desc);
    if (pv == NULL || desc == NULL) { hbhip_host_simple_close(filter); return 1; }   /* (no message) */
    double cb = 0, cr = 0, size = 1, high = 0;                               /* grayscale.c:43-48 */
    hb_dict_extract_double(&cb, filter->settings, "cb");
    hb_dict_extract_double(&cr, filter->settings, "cr");
    hb_dict_extract_double(&size, filter->settings, "size");
    hb_dict_extract_double(&high, filter->settings, "high");
    hbhip_ctx *ctx = hbhip_host_ctx_for(init);
    if (ctx == NULL) return hbhip_host_simple_fail(filter, HBHIP_ERR_NODEVICE);
    int rc = hbhip_grayscale_create(ctx, cb, cr, size, high, init->geometry.width, init->geometry.height,
                                    desc->comp[0].depth, desc->log2_chroma_w, desc->log2_chroma_h, &pv->s.dev);
    if (rc != HBHIP_OK) return hbhip_host_simple_fail(filter, rc);
    pv->s.output = *init;
    return 0;
}

/* ---- rotate -------------------------------------------------------------------------- */
static int rotate_hip_init(hb_filter_object_t *filter, hb_filter_init_t *init);

static const char rotate_hip_template[] =
    "angle=^(0|90|180|270)$:hflip=^"HB_BOOL_REG"$:disable=^"HB_BOOL_REG"$";

hb_filter_object_t hb_filter_rotate_hip =
{
    .id                = HB_FILTER_ROTATE,
    .enforce_order     = 1,
    .name              = "Rotate (HIP)",
    .short_name        = "rotate",
    .settings          = NULL,
    .init              = rotate_hip_init,
    .work              = hbhip_host_simple_filter_work,
    .close             = hbhip_host_simple_close,
    .settings_template = rotate_hip_template,
};

static int rotate_hip_init(hb_filter_object_t *filter, hb_filter_init_t *init)
{
    const AVPixFmtDescriptor *desc;
    hb_filter_private_t *pv = hbhip_host_simple_begin(filter, init, sizeof(*pv), &desc);
    if (pv == NULL || desc == NULL) { hbhip_host_simple_close(filter); return 1; }   /* (no message) */
    int angle = 0, flip = 0;
    hb_dict_extract_int(&angle, filter->settings, "angle");                  /* rotate.c:166-167 */
    hb_dict_extract_bool(&flip, filter->settings, "hflip");
    hbhip_ctx *ctx = hbhip_host_ctx_for(init);
    if (ctx == NULL) return hbhip_host_simple_fail(filter, HBHIP_ERR_NODEVICE);
    int rc = hbhip_rotate_create(ctx, angle, flip, init->geometry.width, init->geometry.height,
                                 desc->comp[0].depth, desc->log2_chroma_w, desc->log2_chroma_h, &pv->s.dev);
    if (rc != HBHIP_OK) return hbhip_host_simple_fail(filter, rc);
    if (angle == 90 || angle == 270)                                         /* rotate.c:195-214, 261-263 */
    {
        const int w = init->geometry.width, n = init->geometry.par.num;
        init->geometry.width = init->geometry.height;
        init->geometry.height = w;
        init->geometry.par.num = init->geometry.par.den;
        init->geometry.par.den = n;
    }
    pv->s.output = *init;
    return 0;
}

/* ---- format (libhb/format.c:13-111) -------------------------------------------------------------
 * In the reference this object has .skip = 1: format_init only writes `format=pix_fmts=<name>` for
 * libavfilter (:97-100) and sets init->pix_fmt (:107); the conversion itself is the `scale` filter
 * libavfilter auto-inserts, i.e. libswscale.  work.c adds it when the encoder wants another pixel format
 * than the pipeline's (work.c:1530-1549), typically 8 <-> 10 bits.  Here it is a real filter for what that
 * use needs (parity unpinned):
 *   - planar YUV depth changes with the subsampling unchanged (csrc/format.hip:format_kernel);
 *   - planar YUV chroma DOWN-sampling, 4:2:2 -> 4:2:0, 4:4:4 -> 4:2:2, 4:4:4 -> 4:2:0, at equal depth or together with a
 *     LOWER depth (format_resample_kernel, its scaled form): hb_get_best_pix_fmt never goes below the title's chroma or
 *     depth (common.c:7516-7604), so a 10-bit 4:2:2 source in front of an 8-bit 4:2:0 encoder gets `format=yuv420p` behind
 *     its yuv422p10le chain (work.c:1525-1552);
 *   - the PLANAR STEP of `format=nv12` / `format=p010le`, when hip_common.c has marked the entry with
 *     HBHIP_FORMAT_PLANAR_STEP: the frames become yuv420p / yuv420p10le here and the run's download adapter repacks them.
 *     libswscale takes every semi-planar target but the two exact repacks through its scaler, so a depth change alone is
 *     the scaled form too (yuv420p10le -> nv12 is NOT format_kernel's 10 -> 8); a stream that already is the planar
 *     step passes through.
 *   - `format=p010le` on 8-bit 4:2:0 frames, when hip_common.c has marked the entry with HBHIP_FORMAT_WIDEN_STEP: the frames
 *     pass through as they are, yuv420p, and the run's download adapter widens them inside its repack.
 *   - `format=bgra | rgba | argb | abgr` on 8-bit 4:2:0 frames of even size, when hip_common.c has marked the entry with
 *     HBHIP_FORMAT_RGB_STEP (hb_get_preview's list, hb.c:945-959): the frames pass through likewise and the download adapter
 *     makes the packed picture inside its repack.
 *   - planar YUV chroma UP-sampling, 4:2:0 -> 4:2:2, 4:2:2 -> 4:4:4, 4:2:0 -> 4:4:4, at equal or HIGHER depth
 *     (format_upsample_kernel), when hip_common.c has marked the entry with HBHIP_FORMAT_UP_STEP, i.e. behind another
 *     drop-in of a device-resident run.  The reference does ask for it: hb_get_best_pix_fmt chooses the pipeline's format
 *     from the title alone, never above its chroma (common.c:7516-7604), and for an encoder whose list holds only 4:2:2 or
 *     4:4:4 formats (x264 high422 / high444, x265 main422-10 / -12 / main444-8, common.c:2252-2384; ProRes, DNxHR) the
 *     two chroma-keeping match_pix_fmt calls of work.c:1525-1552 find nothing and the third, match_pix_fmt(..., 0, 0),
 *     returns the list's first entry: `format=yuv422p10le` behind a yuv420p chain.
 *   - planar YUV chroma DOWN-sampling together with a HIGHER depth, 8 -> 10, 8 -> 12, 10 -> 12 bits (format_resample_kernel's
 *     deepen form), when hip_common.c has marked the entry with HBHIP_FORMAT_DEEPEN_STEP, again behind another drop-in of
 *     a device-resident run.  The reference asks for this too: an 8-bit 4:2:2 / 4:4:4 title runs as yuv422p / yuv444p
 *     (common.c:7516-7604), and for an encoder whose list holds only 10-bit formats - SVT-AV1 10-bit (common.c:2267-2270,
 *     2397-2398) and VP9 10-bit (encavcodec.c:281-284, 2357-2358): yuv420p10le; ProRes and DNxHR 10-bit
 *     (encavcodec.c:286-289, 2384-2409): yuv422p10le - work.c's first match, which keeps chroma and depth, finds nothing
 *     and the second, match_pix_fmt(..., 1, 0), takes any entry with no more chroma whatever its depth:
 *     `format=yuv420p10le` behind a yuv422p or yuv444p chain, `format=yuv422p10le` behind a yuv444p one.
 * Any other target makes init() fail, which keeps the CPU filter (work.c:1861-1868): more chroma samples than the
 * stream has, or fewer at a higher depth, where nobody marked the entry (a lone `format` on host frames would pay a
 * round trip over the bus for a cheap filter), semi-planar targets that nobody marked (a lone `format=nv12` has no
 * adapter to repack for it) or above the stream's depth on 4:2:2 / 4:4:4 frames, RGB (the four packed orders where nobody marked the entry, every other RGB target always), a chroma plane too small for
 * swscale's taps (nine down, five up). */
static int format_hip_init(hb_filter_object_t *filter, hb_filter_init_t *init);
static int format_hip_work(hb_filter_object_t *filter, hb_buffer_t **buf_in, hb_buffer_t **buf_out);

static const char format_hip_template[] = "format=^"HB_ALL_REG"$";

hb_filter_object_t hb_filter_format_hip =
{
    .id                = HB_FILTER_FORMAT,
    .enforce_order     = 1,
    .name              = "Format (HIP)",
    .short_name        = "format",
    .settings          = NULL,
    .init              = format_hip_init,
    .work              = format_hip_work,
    .close             = hbhip_host_simple_close,
    .settings_template = format_hip_template,
};

static int format_hip_init(hb_filter_object_t *filter, hb_filter_init_t *init)
{
    const AVPixFmtDescriptor *desc;
    hb_filter_private_t *pv = hbhip_host_simple_begin(filter, init, sizeof(*pv), &desc);
    if (pv == NULL || desc == NULL) { hbhip_host_simple_close(filter); return 1; }   /* (no message) */
    char *format = NULL;
    hb_dict_extract_string(&format, filter->settings, "format");              /* format.c:46-52 */
    if (format == NULL)
    {
        pv->s.output = *init;                                                   /* nothing to do: frames pass through */
        return 0;
    }
    int dst_fmt = av_get_pix_fmt(format);                                     /* :107 */
    free(format);
    /* hip_common.c's mark on a `format=p010le` entry inside a run of 8-bit 4:2:0 frames: nothing to do here, the run's download
     * adapter widens inside its repack and says p010le downstream.  (A frame under 2 x 2 it would refuse: declined here.) */
    int widen_step = 0;
    hb_dict_extract_bool(&widen_step, filter->settings, HBHIP_FORMAT_WIDEN_STEP);
    if (widen_step && pv->s.dev_io && dst_fmt == HBHIP_PIX_FMT_P010LE && init->pix_fmt == AV_PIX_FMT_YUV420P &&
        init->geometry.width >= 2 && init->geometry.height >= 2)
    {
        pv->s.output = *init;
        return 0;
    }
    /* its mark on a `format=bgra | rgba | argb | abgr` entry inside a run of 8-bit 4:2:0 frames (hb_get_preview's list): nothing
     * to do here either, the download adapter makes the packed picture inside its repack.  Declined: a frame that is not
     * yuv420p of even size (swscale leaves its unscaled path at an odd height; the repack takes neither).  Without the mark
     * every RGB target is declined below, as it always was. */
    int rgb_step = 0;
    hb_dict_extract_bool(&rgb_step, filter->settings, HBHIP_FORMAT_RGB_STEP);
    if (rgb_step && pv->s.dev_io && hbhip_host_rgb32_order(dst_fmt) >= 0 && init->pix_fmt == AV_PIX_FMT_YUV420P &&
        hbhip_host_rgb32_matrix_ok(init->color_matrix) &&
        init->geometry.width >= 2 && init->geometry.height >= 2 && !(init->geometry.width & 1) && !(init->geometry.height & 1))
    {
        pv->s.output = *init;
        return 0;
    }
    /* hip_common.c's mark on a `format=nv12 | p010le` entry inside a run: make the planar frame the download adapter repacks */
    int planar_step = 0;
    hb_dict_extract_bool(&planar_step, filter->settings, HBHIP_FORMAT_PLANAR_STEP);
    planar_step = planar_step && pv->s.dev_io && hbhip_host_is_biplanar(dst_fmt);     /* (no run, no adapter to repack) */
    if (planar_step) dst_fmt = dst_fmt == HBHIP_PIX_FMT_NV12 ? AV_PIX_FMT_YUV420P : AV_PIX_FMT_YUV420P10;
    const AVPixFmtDescriptor *dd = av_pix_fmt_desc_get(dst_fmt);
    if (dd == NULL || dd->nb_components != desc->nb_components || desc->nb_components < 3)
        return hbhip_host_simple_fail(filter, HBHIP_ERR_UNSUPPORTED);
    /* a component per plane on both sides: NV12 / P010 (Cb and Cr on plane 1) are the adapters' business, not this filter's */
    for (int c = 0; c < 3; c++)
        if (dd->comp[c].plane != c || desc->comp[c].plane != c)
            return hbhip_host_simple_fail(filter, HBHIP_ERR_UNSUPPORTED);
    const int resample = dd->log2_chroma_w != desc->log2_chroma_w || dd->log2_chroma_h != desc->log2_chroma_h;
    const int sdepth = desc->comp[0].depth, ddepth = dd->comp[0].depth;
    /* hip_common.c's mark on an entry inside a run whose target has more chroma samples: no dimension loses any, one gains,
     * and the depth does not fall.  Without the mark (a lone drop-in on host frames) such a target is declined below. */
    int upsample = 0;
    hb_dict_extract_bool(&upsample, filter->settings, HBHIP_FORMAT_UP_STEP);
    upsample = upsample && pv->s.dev_io && !planar_step && resample && ddepth >= sdepth &&
               dd->log2_chroma_w <= desc->log2_chroma_w && dd->log2_chroma_h <= desc->log2_chroma_h;
    /* and its mark on an entry inside a run whose target has fewer chroma samples at a HIGHER depth: no dimension gains
     * any, one loses.  Declined below without the mark, like the up step. */
    int deepen = 0;
    hb_dict_extract_bool(&deepen, filter->settings, HBHIP_FORMAT_DEEPEN_STEP);
    deepen = deepen && pv->s.dev_io && !planar_step && resample && ddepth > sdepth &&
             dd->log2_chroma_w >= desc->log2_chroma_w && dd->log2_chroma_h >= desc->log2_chroma_h;
    /* a higher depth with another chroma layout that nobody marked; a biplanar target above the stream's depth */
    if (!upsample && !deepen && (resample || planar_step) && ddepth > sdepth)
        return hbhip_host_simple_fail(filter, HBHIP_ERR_UNSUPPORTED);
    if (planar_step && !resample && ddepth == sdepth)
    {
        pv->s.output = *init;                                                   /* the stream is the planar step already */
        return 0;
    }
    hbhip_ctx *ctx = hbhip_host_ctx_for(init);
    if (ctx == NULL) return hbhip_host_simple_fail(filter, HBHIP_ERR_NODEVICE);
    /* the scaler's path at a lower depth: with fewer chroma samples, or (semi-planar target) on its own */
    const int scaled = ddepth < sdepth && (resample || planar_step);
    /* (the create functions decline what is left: upsampling that nobody marked, other depths, planes too small) */
    int rc = upsample ? hbhip_format_upsample_create(ctx, init->geometry.width, init->geometry.height, sdepth, ddepth,
                                                     desc->log2_chroma_w, desc->log2_chroma_h, dd->log2_chroma_w,
                                                     dd->log2_chroma_h, init->chroma_location, &pv->s.dev)
           : deepen   ? hbhip_format_deepen_create(ctx, init->geometry.width, init->geometry.height, sdepth, ddepth,
                                                   desc->log2_chroma_w, desc->log2_chroma_h, dd->log2_chroma_w,
                                                   dd->log2_chroma_h, init->chroma_location, &pv->s.dev)
           : scaled   ? hbhip_format_scaled_create(ctx, init->geometry.width, init->geometry.height, sdepth, ddepth,
                                                   desc->log2_chroma_w, desc->log2_chroma_h, dd->log2_chroma_w,
                                                   dd->log2_chroma_h, init->chroma_location, &pv->s.dev)
           : resample ? hbhip_format_resample_create(ctx, init->geometry.width, init->geometry.height, sdepth,
                                                     desc->log2_chroma_w, desc->log2_chroma_h, dd->log2_chroma_w,
                                                     dd->log2_chroma_h, init->chroma_location, &pv->s.dev)
                      : hbhip_format_create(ctx, init->geometry.width, init->geometry.height, sdepth,
                                            ddepth, desc->log2_chroma_w, desc->log2_chroma_h,
                                            init->color_range == 2 /* AVCOL_RANGE_JPEG */, &pv->s.dev);
    if (rc != HBHIP_OK) return hbhip_host_simple_fail(filter, rc);
    init->pix_fmt = dst_fmt;
    pv->s.output = *init;
    return 0;
}

static int format_hip_work(hb_filter_object_t *filter, hb_buffer_t **buf_in, hb_buffer_t **buf_out)
{
    hb_filter_private_t *pv = filter->private_data;
    if (pv->s.dev == NULL)
    {
        *buf_out = *buf_in;
        *buf_in = NULL;
        return ((*buf_out)->s.flags & HB_BUF_FLAG_EOF) ? HB_FILTER_DONE : HB_FILTER_OK;
    }
    return hbhip_host_simple_filter_work(filter, buf_in, buf_out);
}
