/* bm3d_hip.c — HIP-backed drop-in for hb_filter_bm3d (libhb/bm3d.c:18-64).
 *
 * In the reference this object has .skip = 1: bm3d_init only hands FFmpeg's `bm3d` one option, sigma (default 1), with
 * hb_dict_set_double, and hb_avfilter_combine folds it into HB_FILTER_AVFILTER.  Here it is a real filter with its own
 * work(), like deband_hip.c, and has to be left out of hb_avfilter_combine's switch.  Same settings key
 * and default.  What happens to sigma on its way into FFmpeg - "%g" text, parsed into a float option with the range
 * 0 .. 99999.9 - and FFmpeg's defaults for every option bm3d.c leaves alone are restated in one place,
 * hbhip_bm3d_params_from_settings (csrc/bm3d.hip; recalled, parity unpinned).
 *
 * Declined (init fails, so the CPU filter is kept): sigma NaN, negative or above 99999.9 (the graph would fail to build),
 * a plane narrower or lower than 16 samples (no block fits), and any format but planar YUV 4:2:0 / 4:2:2 / 4:4:4 at
 * 8 / 10 / 12 bits.
 */
#include "hbhip_host.h"

#include <stdio.h>
#include <stdlib.h>
#include <string.h>

struct hb_filter_private_s { hbhip_host_simple_t s; };

static int bm3d_hip_init(hb_filter_object_t *filter, hb_filter_init_t *init);

static const char bm3d_hip_template[] =                                      /* bm3d.c:15-16 */
    "sigma=^"HB_FLOAT_REG"$";

hb_filter_object_t hb_filter_bm3d_hip =
{
    .id                = HB_FILTER_BM3D,
    .enforce_order     = 1,
    .name              = "BM3D (HIP)",
    .short_name        = "bm3d",
    .settings          = NULL,
    .init              = bm3d_hip_init,
    .work              = hbhip_host_simple_filter_work,
    .close             = hbhip_host_simple_close,
    .settings_template = bm3d_hip_template,
};

/* settings -> kernel parameters; 0 = taken, else declined (a message says why) */
static int bm3d_hip_params(hb_dict_t *settings, int depth, hbhip_bm3d_params *p)
{
    double sigma = 1;                                                        /* bm3d.c:46-48 */
    hb_dict_extract_double(&sigma, settings, "sigma");
    char text[64];                                                           /* bm3d.c:55, as hb_dict hands it on */
    snprintf(text, sizeof(text), "sigma=%g", sigma);
    if (hbhip_bm3d_params_from_settings(text, depth, p) != HBHIP_OK)
    {
        hb_log("bm3d(hip): %s outside the option's range", text);
        return 1;
    }
    return 0;
}

/* every plane holds a 16 x 16 block */
static int size_ok(const AVPixFmtDescriptor *desc, int width, int height)
{
    const int cw = -((-width) >> desc->log2_chroma_w), ch = -((-height) >> desc->log2_chroma_h);
    return cw >= 16 && ch >= 16 && width >= 16 && height >= 16;
}

static int bm3d_hip_init(hb_filter_object_t *filter, hb_filter_init_t *init)
{
    const AVPixFmtDescriptor *desc;
    hb_filter_private_t *pv = hbhip_host_simple_begin(filter, init, sizeof(*pv), &desc);
    if (pv == NULL) return 1;
    hbhip_bm3d_params p;
    int rc = hbhip_host_planar_yuv(desc) ? HBHIP_OK : HBHIP_ERR_UNSUPPORTED;
    if (rc == HBHIP_OK && bm3d_hip_params(filter->settings, desc->comp[0].depth, &p) != 0)
        rc = HBHIP_ERR_UNSUPPORTED;
    if (rc == HBHIP_OK && !size_ok(desc, init->geometry.width, init->geometry.height))
    {
        hb_log("bm3d(hip): a plane of %d x %d is smaller than a block", init->geometry.width, init->geometry.height);
        rc = HBHIP_ERR_UNSUPPORTED;
    }
    hbhip_ctx *ctx = rc == HBHIP_OK ? hbhip_host_ctx_for(init) : NULL;
    if (rc == HBHIP_OK && ctx == NULL) rc = HBHIP_ERR_NODEVICE;
    if (rc == HBHIP_OK)
        rc = hbhip_bm3d_create(ctx, &p, init->geometry.width, init->geometry.height, desc->comp[0].depth,
                               desc->log2_chroma_w, desc->log2_chroma_h, &pv->s.dev);
    if (rc != HBHIP_OK) return hbhip_host_simple_fail(filter, rc);
    pv->s.output = *init;
    return 0;
}
