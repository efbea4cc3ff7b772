#!/usr/bin/env python3
"""Record tests/golden/ass_compose_*.npz: the overlays the reference's render_ssa_subs / compose_subsample_ass
(libhb/rendersub.c:474-665) make of the glyph-image lists of tests/ass_compose_model.py.

oracle/ref_wrap/wrap_rendersub.c stubs libass out (ass_render_frame returns NULL), so the compose loops are never reached
there.  This recorder therefore builds a wrapper translation unit of its own, in a temporary directory outside the
repository: the reference's unmodified rendersub.c, included where it lies, behind an ass_render_frame that returns an
injected list, and one exported function that runs render_ssa_subs on a private struct filled in by hand (the identity
for rgb2yuv_fn: an image's colour is then Y << 24 | Cr << 16 | Cb << 8 | a).  Nothing compiled and no reference text is
kept: only the planes and positions of the overlays.

    python tests/golden/make_ass_compose_golden.py --ref /path/to/reference [case names ...]

A chroma sample the reference does not define (accu_c == 0, :593) holds whatever the recorder's buffer pool held; the
tests compare chroma on the model's mask of defined samples only.
"""
import argparse
import ctypes as C
import os
import subprocess
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

from handbrake_amd import hbrt  # noqa: E402
import ass_compose_model as am  # noqa: E402

WRAPPER = r"""
#include "wrap_common.h"
#include <limits.h>
#include <inttypes.h>
#include <stdarg.h>
#define HANDBRAKE_EXTRADATA_H
enum { AV_PIX_FMT_NV12 = 23, AV_PIX_FMT_NV16 = 101, AV_PIX_FMT_NV24 = 188, AV_PIX_FMT_P010 = 158, AV_PIX_FMT_P012 = 207,
       AV_PIX_FMT_P016 = 170, AV_PIX_FMT_P210 = 197, AV_PIX_FMT_P212 = 209, AV_PIX_FMT_P216 = 199, AV_PIX_FMT_P410 = 198,
       AV_PIX_FMT_P412 = 210, AV_PIX_FMT_P416 = 200, AV_PIX_FMT_YUV420P16 = 47, AV_PIX_FMT_YUV422P16 = 49, AV_PIX_FMT_YUV444P16 = 51 };
enum { AVCOL_RANGE_MPEG = 1 };
enum { SWS_LANCZOS = 0x200, SWS_ACCURATE_RND = 0x40000, SWS_CS_DEFAULT = 5 };
struct SwsContext;
static struct SwsContext *hb_sws_get_context(int a, int b, int c, int d, int e, int f, int g, int h, int i, int j) { return NULL; }
static int sws_scale(struct SwsContext *c, const uint8_t *const s[], const int ss[], int y, int h, uint8_t *const d[], const int ds[]) { return -1; }
static void sws_freeContext(struct SwsContext *c) { }
static void hb_picture_fill(uint8_t *data[], int stride[], hb_buffer_t *b) { }
typedef int (*hb_csp_convert_f)(int);
static int hb_rgb2yuv(int rgb) { return rgb; }
static int hb_rgb2yuv_bt709(int rgb) { return rgb; }
static hb_csp_convert_f hb_get_rgb2yuv_function(int color_matrix) { return hb_rgb2yuv; }
static void hb_valog(int level, const char *prefix, const char *fmt, va_list args) { }

#include <ass/ass.h>
ASS_Library  *ass_library_init(void) { return NULL; }
void          ass_library_done(ASS_Library *l) { }
void          ass_set_message_cb(ASS_Library *l, void (*cb)(int, const char *, va_list, void *), void *d) { }
void          ass_set_extract_fonts(ASS_Library *l, int e) { }
void          ass_add_font(ASS_Library *l, const char *n, const char *d, int s) { }
void          ass_set_style_overrides(ASS_Library *l, char **o) { }
ASS_Renderer *ass_renderer_init(ASS_Library *l) { return NULL; }
void          ass_renderer_done(ASS_Renderer *r) { }
void          ass_set_use_margins(ASS_Renderer *r, int u) { }
void          ass_set_hinting(ASS_Renderer *r, int h) { }
void          ass_set_font_scale(ASS_Renderer *r, double s) { }
void          ass_set_line_spacing(ASS_Renderer *r, double s) { }
void          ass_set_fonts(ASS_Renderer *r, const char *f, const char *fam, int fc, const char *cfg, int upd) { }
void          ass_set_frame_size(ASS_Renderer *r, int w, int h) { }
void          ass_set_storage_size(ASS_Renderer *r, int w, int h) { }
void          ass_set_pixel_aspect(ASS_Renderer *r, double p) { }
ASS_Track    *ass_new_track(ASS_Library *l) { return NULL; }
void          ass_free_track(ASS_Track *t) { }
void          ass_set_check_readorder(ASS_Track *t, int c) { }
void          ass_process_codec_private(ASS_Track *t, const char *d, int s) { }
void          ass_process_chunk(ASS_Track *t, const char *d, int s, long long a, long long b) { }
void          ass_process_data(ASS_Track *t, const char *d, int s) { }

/* the injected list: what libass would have rendered for the frame, always `changed` */
static ASS_Image *rec_list;
ASS_Image *ass_render_frame(ASS_Renderer *r, ASS_Track *t, long long now, int *chg) { if (chg) *chg = 1; return rec_list; }

static hb_blend_object_t rec_blend;
#define hb_blend rec_blend
#include "rendersub.c"
#undef hb_blend

static hb_filter_private_t rec_pv;

/* render_ssa_subs on a private struct filled in by hand; returns the number of overlays */
HBREF_EXPORT int rec_run(int pix_fmt, int pix_fmt_alpha, int chroma_location, int crop_top, int crop_left, ASS_Image *list)
{
    hb_buffer_list_close(&rec_pv.rendered_sub_list);
    hb_box_vec_close(&rec_pv.boxes);
    memset(&rec_pv, 0, sizeof(rec_pv));
    const AVPixFmtDescriptor *desc = av_pix_fmt_desc_get(pix_fmt);
    rec_pv.pix_fmt_alpha = pix_fmt_alpha;
    rec_pv.wshift = desc->log2_chroma_w;
    rec_pv.hshift = desc->log2_chroma_h;
    rec_pv.crop[0] = crop_top;
    rec_pv.crop[2] = crop_left;
    rec_pv.rgb2yuv_fn = hb_rgb2yuv;
    hb_compute_chroma_smoothing_coefficient(rec_pv.chroma_coeffs, pix_fmt, chroma_location);
    rec_list = list;
    render_ssa_subs(&rec_pv, 0);
    return hb_buffer_list_count(&rec_pv.rendered_sub_list);
}

HBREF_EXPORT int rec_overlay(int index, int xywh[4], uint8_t *plane[4], int stride[4], int pw[4], int ph[4])
{
    hb_buffer_t *b = hb_buffer_list_head(&rec_pv.rendered_sub_list);
    while (b != NULL && index-- > 0) b = b->next;
    if (b == NULL) return -1;
    xywh[0] = b->f.x; xywh[1] = b->f.y; xywh[2] = b->f.width; xywh[3] = b->f.height;
    for (int p = 0; p < 4; p++)
    {
        plane[p] = b->plane[p].data; stride[p] = b->plane[p].stride;
        pw[p] = b->plane[p].width; ph[p] = b->plane[p].height;
    }
    return 0;
}
"""


class AssImage(C.Structure):
    pass


AssImage._fields_ = [("w", C.c_int), ("h", C.c_int), ("stride", C.c_int), ("bitmap", C.c_void_p), ("color", C.c_uint32),
                     ("dst_x", C.c_int), ("dst_y", C.c_int), ("next", C.POINTER(AssImage))]

# (format, (crop_left, crop_top), chroma location): every format at both crops left-sited, the other sitings where they
# change the weights
COMBOS = [(f, c, 1) for f in ("420", "422", "444") for c in ((0, 0), (1, 1))] + \
         [("420", (1, 0), 2), ("420", (0, 1), 3), ("422", (1, 1), 2), ("444", (1, 0), 3)]


def build_wrapper(ref, tmp):
    src, obj, lib = (os.path.join(tmp, n) for n in ("wrap_ass_compose.c", "wrap_ass_compose.o", "libass_compose_ref.so"))
    with open(src, "w") as f:
        f.write(WRAPPER)
    pkg = os.path.join(ROOT, "handbrake_amd")
    subprocess.check_call(["gcc", "-std=gnu99", "-O3", "-fPIC", "-fvisibility=default", "-ffp-contract=off", "-w",
                           "-I" + os.path.join(ROOT, "include"), "-I" + os.path.join(pkg, "libhb"),
                           "-I" + os.path.join(ROOT, "oracle", "ref_wrap"), "-I" + os.path.join(ROOT, "oracle", "shim"),
                           "-I" + os.path.join(ref, "libhb"), "-c", src, "-o", obj])
    subprocess.check_call(["gcc", "-shared", "-o", lib, obj, "-L" + pkg, "-lhbrt", "-lm", "-lpthread",
                           "-Wl,-rpath," + pkg, "-Wl,--no-undefined"])
    return lib


def run(lib, images, fmt, crop, loc):
    """the reference's overlays of one list: [(x, y, (Y, Cb, Cr, A))]"""
    nodes = (AssImage * max(len(images), 1))()
    keep = []
    for i, (bitmap, w, x, y, (cy, cb, cr, a)) in enumerate(images):
        bitmap = np.ascontiguousarray(bitmap)
        keep.append(bitmap)
        n = nodes[i]
        n.w, n.h, n.stride, n.bitmap = w, bitmap.shape[0], bitmap.strides[0], bitmap.ctypes.data
        n.color = cy << 24 | cr << 16 | cb << 8 | a
        n.dst_x, n.dst_y = x, y
        n.next = C.pointer(nodes[i + 1]) if i + 1 < len(images) else None
    count = lib.rec_run(am.FRAME_FMT[(fmt, 8)], am.OVERLAY_FMT[fmt], loc, crop[1], crop[0], C.byref(nodes[0]))
    out = []
    for k in range(count):
        g, st, pw, ph = ((C.c_int * 4)() for _ in range(4))
        pl = (C.c_void_p * 4)()
        assert lib.rec_overlay(k, g, pl, st, pw, ph) == 0
        planes = []
        for p in range(4):
            raw = np.frombuffer(C.string_at(pl[p], st[p] * ph[p]), np.uint8).reshape(ph[p], st[p])
            planes.append(raw[:, :pw[p]].copy())
        out.append((g[0], g[1], tuple(planes)))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ref", required=True, help="root of the reference tree (the directory that holds libhb/)")
    ap.add_argument("cases", nargs="*")
    a = ap.parse_args()
    hbrt.runtime()
    with tempfile.TemporaryDirectory() as tmp:
        lib = C.CDLL(build_wrapper(os.path.abspath(a.ref), tmp), mode=C.RTLD_GLOBAL)
        for name in am.CASES:
            if a.cases and name not in a.cases:
                continue
            # one table and one blob a file: a row = format, crop_left, crop_top, chroma location, x, y, width, height, chroma
            # width, chroma height, offset of the overlay's Y Cb Cr A planes (each rows x width, back to back) in `data`
            rows, blob, at = [], [], 0
            for fmt, crop, loc in COMBOS:
                _, _, images = am.build(name, fmt)
                for x, y, planes in run(lib, images, fmt, crop, loc):
                    rows.append([int(fmt), crop[0], crop[1], loc, x, y, planes[0].shape[1], planes[0].shape[0],
                                 planes[1].shape[1], planes[1].shape[0], at])
                    blob += [p.ravel() for p in planes]
                    at += sum(p.size for p in planes)
            path = os.path.join(HERE, f"ass_compose_{name}.npz")
            np.savez_compressed(path, table=np.array(rows, dtype=np.int32), data=np.concatenate(blob))
            print(f"{name}: {len(COMBOS)} combinations -> {os.path.getsize(path)} bytes")


if __name__ == "__main__":
    main()
