/* hip_common.c — puts the HIP drop-ins into a job's filter list.
 *
 * The reference has exactly this for its Metal filters: sanitize_filter_list_post() calls
 * hb_vt_setup_hw_filters(job) (work.c:1515-1523), which swaps CPU filter objects for GPU ones IN PLACE with
 * replace_filter(job, CPU_ID, GPU_ID) and adds an adapter (platform/macosx/vt_common.c:486-540).
 * hb_hip_setup_hw_filters() is the same for HIP:
 *   1. every filter of job->list_filter that has a HIP drop-in (hbhip_filter_get, same id) is replaced by a copy of
 *      the drop-in carrying the same settings dict, at the same list position;
 *   2. every run of two or more drop-ins - adjacent, or with only "hw-transparent" filters between them (vfr,
 *      rendersub, rpu: hb_hip_filter_is_hw_transparent) - is bracketed by hb_filter_hip_upload / hb_filter_hip_download,
 *      so frames stay in HBM inside the run (a lone drop-in moves its own frames; adapters would only add two threads).
 *   3. a `format=nv12 | p010le` entry behind a drop-in of a planar YUV job is split: the Format drop-in is told (through
 *      HBHIP_FORMAT_PLANAR_STEP in its settings, never through the public `format=` value) to make yuv420p / yuv420p10le,
 *      and the run's download adapter gets format=nv12 | p010le and repacks on the GPU (mark_planar_steps).  The same walk
 *      marks a `format=yuv422p... | yuv444p...` entry behind a drop-in whose target has MORE chroma samples than the job's
 *      frames (HBHIP_FORMAT_UP_STEP): the Format drop-in takes such a target only there.  And `format=p010le` behind a
 *      drop-in of a yuv420p or nv12 job (HBHIP_FORMAT_WIDEN_STEP): the Format drop-in passes the 8-bit frames through and
 *      the download adapter, given format=p010le and the same key, widens them inside its repack.  And
 *      `format=bgra | rgba | argb | abgr` behind a drop-in of a yuv420p job (HBHIP_FORMAT_RGB_STEP), what hb_get_preview appends:
 *      built like the widen step, the adapter makes the packed picture inside its repack.  And a planar
 *      `format=yuv420p10le | yuv422p10le | ...` entry behind a drop-in whose target has FEWER chroma samples than the job's
 *      frames and a higher depth (HBHIP_FORMAT_DEEPEN_STEP), taken only there like the up step.
 * And one thing the VideoToolbox path does not need: a drop-in's init() may refuse settings it has no kernels for.
 * work.c drops a filter whose init fails (:1861-1868) - for a drop-in that would silently lose the filter, so the init
 * loop calls hb_hip_filter_init_failed() first, which puts the CPU filter back (and re-brackets the run around it).
 *
 * The aliased filters (crop/scale, rotate, pad, grayscale, colorspace, format, yadif, bwdif) are .skip = 1 objects in
 * the reference whose work happens in the combined HB_FILTER_AVFILTER (hb_avfilter_combine, hbavfilter.c:510-622);
 * a drop-in is a real filter (.skip = 0, own work()), and because the swap changes the object behind the id,
 * hb_avfilter_combine's switch (hbavfilter.c:520-541) must skip ids whose object is a drop-in: hb_hip_filter_is_hip().
 */
#include "hbhip_host.h"
#include "hip_common.h"

#ifndef HBHIP_IN_LIBHB
#define hb_dict_set_string(dict, key, val) hbhip_dict_set(dict, key, val)     /* hb_dict.h:164 */
#endif

static int is_adapter(const hb_filter_object_t *f)
{
    return f->id == HB_FILTER_HIP_UPLOAD || f->id == HB_FILTER_HIP_DOWNLOAD;
}

int hb_hip_filter_is_hip(const hb_filter_object_t *f)
{
    if (f == NULL) return 0;
    const hb_filter_object_t *p = hbhip_filter_get(f->id);
    return p != NULL && p->init == f->init;
}

static int force_swap(void)
{
    const char *force = getenv("HBHIP_FORCE_SWAP");           /* tests: swap even without a device, so that */
    return force != NULL && atoi(force) != 0;                 /* every init fails and the fallback is exercised */
}

static int hip_enabled(void)
{
    const char *off = getenv("HBHIP_DISABLE");
    if (off != NULL && atoi(off) != 0) return 0;
    if (force_swap()) return 1;
    return hbhip_device_count() > 0;
}

/* the format a job's runs give back: its own when that is NV12 / P010LE - unless the list holds a `format` filter, which
 * says itself what the frames are to become (the runs then end planar, as they always did) */
static int job_host_fmt(const hb_job_t *job)
{
    if (!hbhip_host_is_biplanar(job->input_pix_fmt) || hb_filter_find(job->list_filter, HB_FILTER_FORMAT) != NULL)
        return AV_PIX_FMT_NONE;
    return job->input_pix_fmt;
}

/* `host_fmt`: the job's own format when that is NV12 / P010LE.  The upload adapter sees it as the stream's format; the
 * download adapter is told to give it back (format=), so that what leaves the run is what the job's encoder expects. */
static hb_filter_object_t *new_adapter(int id, int host_fmt, const char *key)
{
    hb_filter_object_t *a = hb_filter_copy(hbhip_filter_get(id));
    if (a != NULL && a->settings == NULL) a->settings = hb_dict_init();
    if (a != NULL && id == HB_FILTER_HIP_DOWNLOAD && (hbhip_host_is_biplanar(host_fmt) || hbhip_host_rgb32_order(host_fmt) >= 0))
    {
        const AVPixFmtDescriptor *d = av_pix_fmt_desc_get(host_fmt);
        hb_dict_set_string(a->settings, "format", d->name);                      /* "nv12", "p010le"; "bgra", ... */
        if (key != NULL) hb_dict_set_string(a->settings, key, "1");
    }
    return a;
}

/* the NV12 / P010LE / packed RGB target of a Format drop-in entry that mark_planar_steps() has marked, else AV_PIX_FMT_NONE.
 * *key: the mark the download adapter shares with the entry - HBHIP_FORMAT_WIDEN_STEP (the target is P010LE and the frames
 * have 8 bits), HBHIP_FORMAT_RGB_STEP (the target is one of the four packed orders) - or NULL (the planar step) */
static int planar_step_target(const hb_filter_object_t *f, const char **key)
{
    int marked = 0, fmt = AV_PIX_FMT_NONE;
    char *name = NULL;
    *key = NULL;
    if (f == NULL || f->id != HB_FILTER_FORMAT || !hb_hip_filter_is_hip(f) || f->settings == NULL) return AV_PIX_FMT_NONE;
    if (hb_dict_extract_bool(&marked, f->settings, HBHIP_FORMAT_WIDEN_STEP) && marked) *key = HBHIP_FORMAT_WIDEN_STEP;
    else if (hb_dict_extract_bool(&marked, f->settings, HBHIP_FORMAT_RGB_STEP) && marked) *key = HBHIP_FORMAT_RGB_STEP;
    else if (!hb_dict_extract_bool(&marked, f->settings, HBHIP_FORMAT_PLANAR_STEP) || !marked) return AV_PIX_FMT_NONE;
    if (hb_dict_extract_string(&name, f->settings, "format") && name != NULL) fmt = av_get_pix_fmt(name);
    free(name);
    const int rgb = *key != NULL && strcmp(*key, HBHIP_FORMAT_RGB_STEP) == 0;
    if (rgb ? hbhip_host_rgb32_order(fmt) < 0 : *key != NULL ? fmt != HBHIP_PIX_FMT_P010LE : !hbhip_host_is_biplanar(fmt))
    {
        *key = NULL;
        return AV_PIX_FMT_NONE;
    }
    return fmt;
}

/* the five keys of mark_planar_steps(): nothing a CPU filter knows, and stale once the list in front has changed */
static void remove_marks(hb_dict_t *settings)
{
    hb_dict_remove(settings, HBHIP_FORMAT_RGB_STEP);
    hb_dict_remove(settings, HBHIP_FORMAT_PLANAR_STEP);
    hb_dict_remove(settings, HBHIP_FORMAT_UP_STEP);
    hb_dict_remove(settings, HBHIP_FORMAT_WIDEN_STEP);
    hb_dict_remove(settings, HBHIP_FORMAT_DEEPEN_STEP);
}

/* work.c appends `format=nv12` / `format=p010le` when the encoder wants one of them (work.c:1525-1552, match_pix_fmt).
 * Where such an entry stands behind a drop-in (transparent filters aside) of a planar YUV 4:2:0 / 4:2:2 / 4:4:4 job whose
 * depth is at least the target's, the frames need not leave the device a filter early: the entry is marked, its drop-in
 * makes the planar step, and bracket_runs() gives the download adapter behind it the biplanar format.  The entry keeps
 * `format=nv12`, so that the fallback hands the CPU filter its own settings (hb_hip_filter_init_failed strips the mark).
 * Not marked: an 8-bit 4:2:2 / 4:4:4 stream under p010le (a higher depth: init() declines it as before; 8-bit 4:2:0 gets
 * the widen step, below), and an entry with no drop-in in front of it - on a yuv420p job its planar step would be the
 * identity, and an interleave on the CPU is cheaper than a round trip over the bus.
 *
 * The same walk marks the UP step (HBHIP_FORMAT_UP_STEP).  work.c appends `format=yuv422p...` / `format=yuv444p...` to a
 * 4:2:0 chain when the encoder's list holds only such formats: hb_get_best_pix_fmt chooses the pipeline's format from the
 * title alone (common.c:7516-7604), the two chroma-keeping match_pix_fmt calls find nothing in the list and the third,
 * match_pix_fmt(..., 0, 0), returns its first entry (x264 high422 / high444, x265 main422-10 / -12 / main444-8,
 * common.c:2252-2384; ProRes, DNxHR).  Such an entry - a planar YUV 4:2:0 / 4:2:2 / 4:4:4 target at 8 / 10 / 12 bits that
 * loses chroma samples in no dimension, gains them in one at least and is no shallower than the job - is marked under the
 * same condition, a drop-in in front of it, and for the same reason; the Format drop-in takes such a target only where
 * the mark stands, so a lone `format=yuv422p` keeps its CPU filter as before.
 *
 * And the WIDEN step (HBHIP_FORMAT_WIDEN_STEP): `format=p010le` on a job of 8-bit 4:2:0 frames, what work.c appends for
 * every 8-bit title in front of AMD's 10-bit encoders (encavcodec.c:321-324, hb_get_best_pix_fmt never lifts the pipeline
 * above the title's depth, common.c:7516-7524).  On a yuv420p job and on an nv12 job alike - the upload adapter of an nv12
 * job's run makes yuv420p frames, and this is the one mark such a job gets - under the same condition, a drop-in in front.
 * The Format drop-in passes the frames through and the run's download adapter widens them inside its repack.  8-bit
 * 4:2:2 / 4:4:4 under p010le stay unmarked: the planar step from an 8-bit source in front of the repack is not built.
 *
 * And the DEEPEN step (HBHIP_FORMAT_DEEPEN_STEP): `format=yuv420p10le` behind a yuv422p or yuv444p chain, `format=yuv422p10le`
 * behind a yuv444p one.  An 8-bit 4:2:2 / 4:4:4 title runs at its own depth and chroma (common.c:7516-7604); an encoder
 * whose list holds only 10-bit formats (SVT-AV1 10-bit, common.c:2267-2270; VP9, ProRes and DNxHR 10-bit,
 * encavcodec.c:281-289) fails work.c's first match and passes the second, match_pix_fmt(..., 1, 0): any entry with no
 * more chroma, whatever its depth.  Such an entry - a planar YUV 4:2:0 / 4:2:2 / 4:4:4 target at 10 or 12 bits that gains
 * chroma samples in no dimension, loses them in one at least and is deeper than the job - is marked under the same
 * condition, a drop-in in front of it; without the mark the Format drop-in declines it as before.
 *
 * And the RGB step (HBHIP_FORMAT_RGB_STEP): `format=bgra` - or rgba, argb, abgr - on a job of yuv420p frames.  work.c appends no
 * such entry, hb.c does: hb_get_preview, behind every front-end's preview window, filters its picture through the job's
 * picture filters and a display rescale and ends the list in `format=<AV_PIX_FMT_RGB32>` (hb.c:945-959).  Under the same
 * condition, a drop-in in front, the entry is marked; the Format drop-in passes the frames through and the run's download
 * adapter, given the same `format=` value and key, makes the packed picture inside its repack.  yuv422p / yuv444p and deeper
 * jobs stay unmarked (the repack takes 8-bit 4:2:0), and a lone `format=bgra` keeps its CPU filter. */
static void mark_planar_steps(hb_job_t *job, int from)
{
    hb_list_t *list = job->list_filter;
    const AVPixFmtDescriptor *desc = av_pix_fmt_desc_get(job->input_pix_fmt);
    const int planar = hbhip_host_planar_yuv(desc);
    const int widens = job->input_pix_fmt == AV_PIX_FMT_YUV420P || job->input_pix_fmt == HBHIP_PIX_FMT_NV12;
    if (!planar && !widens) return;
    for (int i = from > 1 ? from : 1; i < hb_list_count(list); i++)
    {
        hb_filter_object_t *f = hb_list_item(list, i);
        if (f->id != HB_FILTER_FORMAT || !hb_hip_filter_is_hip(f) || f->settings == NULL) continue;
        char *name = NULL;
        if (!hb_dict_extract_string(&name, f->settings, "format") || name == NULL) { free(name); continue; }
        const int fmt = av_get_pix_fmt(name);
        free(name);
        const char *key = NULL;
        if (hbhip_host_rgb32_order(fmt) >= 0)
        {
            if (job->input_pix_fmt == AV_PIX_FMT_YUV420P) key = HBHIP_FORMAT_RGB_STEP;
        }
        else if (hbhip_host_is_biplanar(fmt))
        {
            if (widens && fmt == HBHIP_PIX_FMT_P010LE) key = HBHIP_FORMAT_WIDEN_STEP;
            else if (planar && desc->comp[0].depth >= (fmt == HBHIP_PIX_FMT_NV12 ? 8 : 10)) key = HBHIP_FORMAT_PLANAR_STEP;
        }
        else if (planar)
        {
            /* the up step: a planar YUV target that loses chroma samples in no dimension, gains them in one at least, and
             * is no shallower than the job's frames */
            const AVPixFmtDescriptor *dd = av_pix_fmt_desc_get(fmt);
            if (hbhip_host_planar_yuv(dd) && dd->log2_chroma_w <= desc->log2_chroma_w && dd->log2_chroma_h <= desc->log2_chroma_h &&
                (dd->log2_chroma_w < desc->log2_chroma_w || dd->log2_chroma_h < desc->log2_chroma_h) &&
                dd->comp[0].depth >= desc->comp[0].depth)
                key = HBHIP_FORMAT_UP_STEP;
            /* the deepen step: the other way round in chroma - gains in no dimension, loses in one at least - at 10 or 12
             * bits and deeper than the job's frames */
            else if (hbhip_host_planar_yuv(dd) && dd->log2_chroma_w >= desc->log2_chroma_w && dd->log2_chroma_h >= desc->log2_chroma_h &&
                     (dd->log2_chroma_w > desc->log2_chroma_w || dd->log2_chroma_h > desc->log2_chroma_h) &&
                     (dd->comp[0].depth == 10 || dd->comp[0].depth == 12) && dd->comp[0].depth > desc->comp[0].depth)
                key = HBHIP_FORMAT_DEEPEN_STEP;
        }
        if (key == NULL) continue;
        int j = i - 1;
        while (j >= from && hb_hip_filter_is_hw_transparent(hb_list_item(list, j))) j--;
        if (j < from || is_adapter(hb_list_item(list, j)) || !hb_hip_filter_is_hip(hb_list_item(list, j))) continue;
        hb_dict_set_string(f->settings, key, "1");
    }
}

/* vt_common.c:486-502, by position instead of by id */
static void replace_at(hb_list_t *list, int pos, hb_filter_object_t *proto)
{
    hb_filter_object_t *old = hb_list_item(list, pos);
    if (old->settings == NULL) return;                        /* replace_filter: no settings, no swap (:493-494) */
    hb_filter_object_t *nf = hb_filter_copy(proto);
    if (nf == NULL) return;
    hb_dict_free(&nf->settings);
    nf->settings = hb_value_dup(old->settings);
    hb_list_rem(list, old);
    hb_list_insert(list, pos, nf);
    hb_filter_close(&old);
}

/* Filters that never look at a picture's samples themselves, only at the hb_buffer_t around it: they sit INSIDE a
 * device-resident run without breaking it.  The reference has the same notion for its Metal pipeline -
 * are_filters_supported() (platform/macosx/vt_common.c:424-448) lists HB_FILTER_VFR, RENDER_SUB, FORMAT and RPU
 * beside the filters it has kernels for - and the first two choose their pixel helper by init->hw_pix_fmt:
 * vfr.c:76-108 the motion metric (hb_motion_metric_hip here), rendersub.c:1129-1161 the compositor (hb_blend_hip).
 * FORMAT has a drop-in of its own (format_hip.c); RPU only edits Dolby Vision side data (rpu.c).
 * Every preset-built job has a VFR between decomb (6) and NLMeans (16) (preset.c:2026-2048, ids common.h:1739-1751):
 * without this the run - and the frames - would leave the device there. */
int hb_hip_filter_is_hw_transparent(const hb_filter_object_t *f)
{
    if (f == NULL || hb_hip_filter_is_hip(f)) return 0;
    return f->id == HB_FILTER_VFR || f->id == HB_FILTER_RENDER_SUB || f->id == HB_FILTER_RPU;
}

/* Bracket, from position `from` on, every run [drop-in (drop-in | transparent)* drop-in] that holds at least two
 * drop-ins with hb_filter_hip_upload / hb_filter_hip_download (a lone drop-in moves its own frames; adapters would only
 * add two threads).  Transparent filters at either end of a run stay outside: nothing is gained by uploading for them. */
static void bracket_runs(hb_list_t *list, int from, int host_fmt)
{
    /* a drop-in cannot move biplanar frames itself: in an NV12 / P010LE job a lone one gets its adapters too */
    const int least = hbhip_host_is_biplanar(host_fmt) ? 1 : 2;
    for (int i = from; i < hb_list_count(list);)
    {
        if (!hb_hip_filter_is_hip(hb_list_item(list, i)) || is_adapter(hb_list_item(list, i))) { i++; continue; }
        int last = i, n = 1;
        for (int j = i + 1; j < hb_list_count(list); j++)
        {
            hb_filter_object_t *f = hb_list_item(list, j);
            if (is_adapter(f)) break;
            if (hb_hip_filter_is_hip(f)) { last = j; n++; }
            else if (!hb_hip_filter_is_hw_transparent(f)) break;
        }
        if (n >= least)
        {
            /* a run that ends in a marked `format=nv12 | p010le | bgra ...` entry leaves the device in that format */
            const char *key;
            const int step_fmt = planar_step_target(hb_list_item(list, last), &key);
            hb_list_insert(list, last + 1, new_adapter(HB_FILTER_HIP_DOWNLOAD, step_fmt != AV_PIX_FMT_NONE ? step_fmt : host_fmt, key));
            hb_list_insert(list, i, new_adapter(HB_FILTER_HIP_UPLOAD, host_fmt, NULL));
            last += 2;
        }
        i = last + 1;
    }
}

void hb_hip_setup_hw_filters(hb_job_t *job)
{
    if (job == NULL || job->list_filter == NULL || !hip_enabled()) return;
    if (job->hw_pix_fmt != AV_PIX_FMT_NONE) return;           /* another hw pipeline owns the frames */
    if (!force_swap() && hbhip_host_job_index_is_hip(job) && job->hw_device_index >= hbhip_device_count())
    {
        /* the job names an adapter (common.h:991, hb_json.c "AdapterIndex") this process has no GPU for */
        hb_log("hbhip: job asks for GPU %d, %d present: keeping the CPU filters", job->hw_device_index, hbhip_device_count());
        return;
    }
    hb_list_t *list = job->list_filter;
    for (int i = 0; i < hb_list_count(list); i++)
    {
        hb_filter_object_t *f = hb_list_item(list, i);
        if (is_adapter(f) || hb_hip_filter_is_hip(f)) continue;
        hb_filter_object_t *proto = hbhip_filter_get(f->id);
        if (proto != NULL) replace_at(list, i, proto);
    }
    mark_planar_steps(job, 0);
    bracket_runs(list, 0, job_host_fmt(job));
}

int hb_hip_filter_init_failed(hb_job_t *job, int index, hb_filter_init_t *init)
{
    if (job == NULL || job->list_filter == NULL) return 0;
    hb_list_t *list = job->list_filter;
    hb_filter_object_t *f = hb_list_item(list, index);
    if (f == NULL || is_adapter(f) || !hb_hip_filter_is_hip(f)) return 0;
    hb_filter_object_t *cpu = hb_filter_init(f->id);
    if (cpu == NULL) return 0;                                /* no CPU filter of that id: work.c drops it */
    if (cpu->init == f->init)                                 /* the id's own filter IS the drop-in: it would decline again */
    {
        hb_filter_close(&cpu);
        /* work.c drops the entry; a planar step that is not made leaves nothing for its download adapter to repack */
        hb_filter_object_t *next = hb_list_item(list, index + 1);
        const char *key;
        if (planar_step_target(f, &key) != AV_PIX_FMT_NONE && next != NULL && next->id == HB_FILTER_HIP_DOWNLOAD &&
            next->settings != NULL)
        {
            hb_dict_remove(next->settings, "format");
            hb_dict_remove(next->settings, HBHIP_FORMAT_WIDEN_STEP);       /* (they came together) */
            hb_dict_remove(next->settings, HBHIP_FORMAT_RGB_STEP);
        }
        return 0;
    }
    hb_dict_free(&cpu->settings);
    cpu->settings = f->settings ? hb_value_dup(f->settings) : hb_dict_init();
    remove_marks(cpu->settings);                              /* mark_planar_steps' keys are nothing the CPU filter knows */
    if (cpu->sub_filter != NULL)                              /* mt_frame wrapper: hb_add_filter_dict copies them down */
    {
        hb_dict_free(&cpu->sub_filter->settings);
        cpu->sub_filter->settings = hb_value_dup(cpu->settings);
    }
    hb_log("hbhip: '%s' keeps its CPU filter (the HIP drop-in declined these settings)", cpu->name);
    hb_list_rem(list, f);
    hb_filter_close(&f);

    /* everything from `index` on has not been initialised yet: take its adapters out, put the CPU filter in, and
     * bracket what is left of the runs afresh.  What lies before `index` has seen its init and stays as it is. */
    for (int i = index; i < hb_list_count(list);)
    {
        hb_filter_object_t *a = hb_list_item(list, i);
        if (!is_adapter(a)) { i++; continue; }
        hb_list_rem(list, a);
        hb_filter_close(&a);
    }
    int pos = index, ret = 1;
    if (hbhip_host_dev_io(init))
    {
        /* inside a device-resident run: the CPU filter needs host frames */
        hb_filter_object_t *prev = pos > 0 ? hb_list_item(list, pos - 1) : NULL;
        if (prev != NULL && prev->id == HB_FILTER_HIP_UPLOAD)
        {
            /* the run's own upload sits right in front: undo it instead of downloading straight again */
            const int host_fmt = hbhip_host_adapter_input_pix_fmt(prev);      /* NV12 / P010LE: the adapter had rewritten it */
            if (host_fmt != AV_PIX_FMT_NONE) init->pix_fmt = host_fmt;
            if (prev->close != NULL) prev->close(prev);
            hb_list_rem(list, prev);
            hb_filter_close(&prev);
            init->hw_pix_fmt = AV_PIX_FMT_NONE;
            pos--;
            ret = 2;                                          /* the CPU filter now sits one slot earlier */
        }
        else
            hb_list_insert(list, pos++, new_adapter(HB_FILTER_HIP_DOWNLOAD, job_host_fmt(job), NULL));
    }
    hb_list_insert(list, pos, cpu);
    /* what follows may have lost the drop-in it stood behind: mark afresh, then bracket */
    for (int i = pos + 1; i < hb_list_count(list); i++)
    {
        hb_filter_object_t *g = hb_list_item(list, i);
        if (g->id == HB_FILTER_FORMAT && g->settings != NULL) remove_marks(g->settings);
    }
    mark_planar_steps(job, pos + 1);
    bracket_runs(list, pos + 1, job_host_fmt(job));
    return ret;
}
