/* deblock_hip.c — HIP-backed drop-in for hb_filter_deblock (libhb/deblock.c:37-86).
 *
 * In the reference this object has .skip = 1: deblock_init only assembles the settings of FFmpeg's `deblock` (filter,
 * block, alpha, beta, gamma, delta), which hb_avfilter_combine folds into HB_FILTER_AVFILTER.  Here it is a real filter
 * with its own work(), like pad_hip.c, and has to be left out of hb_avfilter_combine's switch.  Same
 * settings keys and defaults.  What happens to the settings on their way into FFmpeg is restated in one function,
 * deblock_hip_params(): the doubles deblock.c computes become text with "%g" (hb_dict.c, through
 * hb_filter_settings_string), FFmpeg parses them into float options of range 0..1, and its integer thresholds are
 * (int)(option * ((1 << depth) - 1)), a float product truncated.  FFmpeg's defaults where deblock.c sets nothing
 * (filter strong, alpha 0.098, beta / gamma / delta 0.05) are recalled (parity unpinned).
 *
 * Declined (init fails, so the CPU filter is kept): an unknown strength, a block size outside FFmpeg's 4..512, a
 * threshold past FFmpeg's option range (thresh > 100: the graph would fail to build), and a plane whose last edge's
 * window would reach past the plane (FFmpeg reads the line padding there: no defined result to match).
 */
#include "hbhip_host.h"

#include <stdio.h>
#include <string.h>

struct hb_filter_private_s { hbhip_host_simple_t s; };

static int deblock_hip_init(hb_filter_object_t *filter, hb_filter_init_t *init);

static const char deblock_hip_template[] =                                   /* deblock.c:15-17 */
    "strength=^"HB_ALL_REG"$:thresh=^"HB_INT_REG"$:blocksize=^"HB_INT_REG"$:"
    "disable=^"HB_BOOL_REG"$";

hb_filter_object_t hb_filter_deblock_hip =
{
    .id                = HB_FILTER_DEBLOCK,
    .enforce_order     = 1,
    .name              = "Deblock (HIP)",
    .short_name        = "deblock",
    .settings          = NULL,
    .init              = deblock_hip_init,
    .work              = hbhip_host_simple_filter_work,
    .close             = hbhip_host_simple_close,
    .settings_template = deblock_hip_template,
};

/* FFmpeg's defaults for the options deblock.c leaves unset (recalled) */
#define DEBLOCK_DEFAULT_ALPHA 0.098f
#define DEBLOCK_DEFAULT_BGD   0.05f

/* a double as deblock.c hands it on ("%g") and as FFmpeg reads it back into a float option */
static float option_float(double v)
{
    char buf[64];
    snprintf(buf, sizeof(buf), "%g", v);
    return (float)strtod(buf, NULL);
}

static int plane_ok(int size, int b, int strong)
{
    if (size <= b) return 1;                                  /* no edge in the plane */
    const int r = size % b;
    return strong ? (r != 1 && r != 2) : r != 1;
}

/* settings -> kernel parameters; 0 = taken, else declined (a message says why) */
static int deblock_hip_params(hb_dict_t *settings, int depth, int width, int height, int log2_cw, int log2_ch,
                              hbhip_deblock_params *p)
{
    int thresh = -1, blocksize = 8;                                          /* deblock.c:53-59 */
    char *strength = NULL;
    hb_dict_extract_string(&strength, settings, "strength");
    hb_dict_extract_int(&thresh, settings, "thresh");
    hb_dict_extract_int(&blocksize, settings, "blocksize");
    memset(p, 0, sizeof(*p));
    p->strong = 1;                                                           /* FFmpeg's default filter */
    if (strength != NULL)
    {
        const int weak = !strcmp(strength, "weak"), strong = !strcmp(strength, "strong");
        free(strength);
        if (!weak && !strong) { hb_log("deblock(hip): unknown strength"); return 1; }
        p->strong = strong;
    }
    if (blocksize < 4 || blocksize > 512) { hb_log("deblock(hip): blocksize %d outside 4..512", blocksize); return 1; }
    p->block = blocksize;
    float alpha = DEBLOCK_DEFAULT_ALPHA, bgd = DEBLOCK_DEFAULT_BGD;
    if (thresh > 0)                                                          /* deblock.c:66-76 */
    {
        const double a = thresh * 0.010;
        alpha = option_float(a);
        bgd = option_float(a / 2);
        if (alpha > 1.0f || bgd > 1.0f) { hb_log("deblock(hip): thresh %d past the options' range", thresh); return 1; }
    }
    const int maxv = (1 << depth) - 1;
    p->ath = (int)(alpha * (float)maxv);
    p->bth = p->gth = p->dth = (int)(bgd * (float)maxv);
    const int cw = -((-width) >> log2_cw), ch = -((-height) >> log2_ch);
    if (!plane_ok(width, blocksize, p->strong) || !plane_ok(height, blocksize, p->strong) ||
        !plane_ok(cw, blocksize, p->strong) || !plane_ok(ch, blocksize, p->strong))
    {
        hb_log("deblock(hip): a plane's last edge reaches past the plane (%dx%d, block %d)", width, height, blocksize);
        return 1;
    }
    return 0;
}

#ifndef HBHIP_IN_LIBHB
/* The same resolution from a "key=value:..." string, for tests and tools that drive the C ABI directly (the stand-in
 * runtime's parser; a build inside libhb has no use for it).  0 = taken. */
int hbhip_deblock_params_from_settings(const char *settings, int depth, int width, int height, int log2_cw, int log2_ch,
                                       hbhip_deblock_params *p)
{
    hb_dict_t *d = hbhip_dict_from_string(settings);
    const int rc = deblock_hip_params(d, depth, width, height, log2_cw, log2_ch, p);
    hb_dict_free(&d);
    return rc;
}
#endif

static int deblock_hip_init(hb_filter_object_t *filter, hb_filter_init_t *init)
{
    const AVPixFmtDescriptor *desc;
    hb_filter_private_t *pv = hbhip_host_simple_begin(filter, init, sizeof(*pv), &desc);
    if (pv == NULL) return 1;
    hbhip_deblock_params p;
    int rc = desc == NULL ? HBHIP_ERR_ARG : HBHIP_OK;
    if (rc == HBHIP_OK &&
        deblock_hip_params(filter->settings, desc->comp[0].depth, init->geometry.width, init->geometry.height,
                           desc->log2_chroma_w, desc->log2_chroma_h, &p) != 0)
        rc = HBHIP_ERR_UNSUPPORTED;
    hbhip_ctx *ctx = rc == HBHIP_OK ? hbhip_host_ctx_for(init) : NULL;
    if (rc == HBHIP_OK && ctx == NULL) rc = HBHIP_ERR_NODEVICE;
    if (rc == HBHIP_OK)
        rc = hbhip_deblock_create(ctx, &p, init->geometry.width, init->geometry.height, desc->comp[0].depth,
                                  desc->log2_chroma_w, desc->log2_chroma_h, &pv->s.dev);
    if (rc != HBHIP_OK) return hbhip_host_simple_fail(filter, rc);
    pv->s.output = *init;
    return 0;
}
