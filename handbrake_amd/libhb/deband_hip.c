/* deband_hip.c — HIP-backed drop-in for hb_filter_deband (libhb/deband.c:21-80).
 *
 * In the reference this object has .skip = 1: deband_init only assembles the settings of FFmpeg's `deband` (1thr ..
 * 4thr, range, blur), which hb_avfilter_combine folds into HB_FILTER_AVFILTER.  Here it is a real filter with its own
 * work(), like deblock_hip.c, and has to be left out of hb_avfilter_combine's switch.  Same settings
 * keys and defaults.  What happens to the settings on their way into FFmpeg is restated in one function,
 * deband_hip_params(): the doubles become text with "%g" (hb_dict.c), FFmpeg parses each into a float option after
 * checking the double against the option's range [0.00003, 0.5], and its integer threshold is
 * (int)(((1 << depth) - 1) * option), a float product truncated.  `direction` keeps FFmpeg's default, 2 pi as a float
 * (recalled; parity unpinned).
 *
 * Declined (init fails, so the CPU filter is kept): a threshold outside [0.00003, 0.5] or blur outside {0, 1} (the graph
 * would fail to build), |range| > 2^30 (INT_MIN has no -range), and any format but planar YUV 4:2:0 / 4:2:2 / 4:4:4 at
 * 8 / 10 / 12 bits.
 */
#include "hbhip_host.h"

#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

struct hb_filter_private_s { hbhip_host_simple_t s; };

static int deband_hip_init(hb_filter_object_t *filter, hb_filter_init_t *init);

static const char deband_hip_template[] =                                    /* deband.c:15-18 */
    "1thr=^"HB_FLOAT_REG"$:2thr=^"HB_FLOAT_REG"$:"
    "3thr=^"HB_FLOAT_REG"$:4thr=^"HB_FLOAT_REG"$:"
    "range=^"HB_INT_REG"$:blur=^"HB_BOOL_REG"$";

hb_filter_object_t hb_filter_deband_hip =
{
    .id                = HB_FILTER_DEBAND,
    .enforce_order     = 1,
    .name              = "Deband (HIP)",
    .short_name        = "deband",
    .settings          = NULL,
    .init              = deband_hip_init,
    .work              = hbhip_host_simple_filter_work,
    .close             = hbhip_host_simple_close,
    .settings_template = deband_hip_template,
};

/* FFmpeg's option ranges (recalled) */
#define DEBAND_THR_MIN 0.00003
#define DEBAND_THR_MAX 0.5
#define DEBAND_RANGE_MAX (1 << 30)

/* settings -> kernel parameters; 0 = taken, else declined (a message says why) */
static int deband_hip_params(hb_dict_t *settings, int depth, hbhip_deband_params *p)
{
    double thr[4] = { 0.02, 0.02, 0.02, 0.02 };                             /* deband.c:52-53 */
    int range = 16, blur = 1;
    hb_dict_extract_double(&thr[0], settings, "1thr");
    hb_dict_extract_double(&thr[1], settings, "2thr");
    hb_dict_extract_double(&thr[2], settings, "3thr");
    hb_dict_extract_double(&thr[3], settings, "4thr");
    hb_dict_extract_int(&range, settings, "range");
    hb_dict_extract_int(&blur, settings, "blur");
    memset(p, 0, sizeof(*p));
    const int maxv = (1 << depth) - 1;
    for (int i = 0; i < 4; i++)
    {
        char buf[64];                                                        /* as hb_dict hands it on */
        snprintf(buf, sizeof(buf), "%g", thr[i]);
        const double d = strtod(buf, NULL);                                  /* as FFmpeg parses it */
        if (!(d >= DEBAND_THR_MIN && d <= DEBAND_THR_MAX)) { hb_log("deband(hip): %dthr %s outside the option's range", i + 1, buf); return 1; }
        if (i < 3) p->thr[i] = (int)((float)maxv * (float)d);
    }
    if (blur != 0 && blur != 1) { hb_log("deband(hip): blur %d is not a boolean", blur); return 1; }
    if (range > DEBAND_RANGE_MAX || range < -DEBAND_RANGE_MAX) { hb_log("deband(hip): range %d past +-2^30", range); return 1; }
    p->blur = blur;
    p->range = range;
    p->direction = (float)(2 * M_PI);                                        /* FFmpeg's default */
    return 0;
}

#ifndef HBHIP_IN_LIBHB
/* The same resolution from a "key=value:..." string, for tests and tools that drive the C ABI directly (the stand-in
 * runtime's parser; a build inside libhb has no use for it).  0 = taken. */
int hbhip_deband_params_from_settings(const char *settings, int depth, hbhip_deband_params *p)
{
    hb_dict_t *d = hbhip_dict_from_string(settings);
    const int rc = deband_hip_params(d, depth, p);
    hb_dict_free(&d);
    return rc;
}
#endif

static int deband_hip_init(hb_filter_object_t *filter, hb_filter_init_t *init)
{
    const AVPixFmtDescriptor *desc;
    hb_filter_private_t *pv = hbhip_host_simple_begin(filter, init, sizeof(*pv), &desc);
    if (pv == NULL) return 1;
    hbhip_deband_params p;
    int rc = hbhip_host_planar_yuv(desc) ? HBHIP_OK : HBHIP_ERR_UNSUPPORTED;
    if (rc == HBHIP_OK && deband_hip_params(filter->settings, desc->comp[0].depth, &p) != 0)
        rc = HBHIP_ERR_UNSUPPORTED;
    hbhip_ctx *ctx = rc == HBHIP_OK ? hbhip_host_ctx_for(init) : NULL;
    if (rc == HBHIP_OK && ctx == NULL) rc = HBHIP_ERR_NODEVICE;
    if (rc == HBHIP_OK)
        rc = hbhip_deband_create(ctx, &p, init->geometry.width, init->geometry.height, desc->comp[0].depth,
                                 desc->log2_chroma_w, desc->log2_chroma_h, &pv->s.dev);
    if (rc != HBHIP_OK) return hbhip_host_simple_fail(filter, rc);
    pv->s.output = *init;
    return 0;
}
