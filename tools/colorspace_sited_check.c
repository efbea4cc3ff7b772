/* colorspace_sited_check.c - the colour conversion's CPU checker with the two chroma siting axes.
 * TEST INFRASTRUCTURE ONLY: built as tools/libcolorspace_sited_check.so, loaded by tests/colorspace_sited_lib.py; nothing
 * of the product links or names it.
 *
 * oracle/colorspace_oracle.c is included unchanged for its plan, its per-pixel conversion and its quantiser
 * (build_plan / convert_px / quant); what this file adds is orc_colorspace_frame's frame loop once more, with the
 * up-sampling weights and the decimation taps of a direction chosen by its siting:
 *   co-sited  up   2k: c[k];  2k + 1: 1/2 c[k] + 1/2 c[k+1];            down  2k - 1 .. 2k + 1 with 1/4 1/2 1/4
 *   centred   up   2k: 1/4 c[k-1] + 3/4 c[k];  2k + 1: 3/4 c[k] + 1/4 c[k+1];   down  2k - 1 .. 2k + 2 with 1/8 3/8 3/8 1/8
 * edges repeat.  Operation order as the oracle's: rows first, then columns; a sample that is not interpolated is taken
 * as it is; every sum is a chain of fmaf() that starts with the product of the tap with the lowest index.
 * h_centred = 0, v_cosited = 0 is orc_colorspace_frame itself (left-sited horizontally, centred vertically), bit for bit:
 * tests/test_colorspace_sited_cpu.py.  PARITY UNPINNED like the oracle: which locations of a stream select which form
 * is handbrake_amd/csrc/chroma_siting.h's rule. */
#include "../oracle/colorspace_oracle.c"

/* the two source samples and their weights under position i of a subsampled direction of n chroma samples */
static void sited_up(int i, int n, int cosited, int *i0, int *i1, float *w0, float *w1)
{
    const int k = i >> 1;
    if (cosited)
    {
        *i0 = *i1 = k; *w0 = 1.f; *w1 = 0.f;
        if (i & 1) { *i1 = clampi(k + 1, 0, n - 1); *w0 = 0.5f; *w1 = 0.5f; }
    }
    else if (i & 1) { *i0 = k; *i1 = clampi(k + 1, 0, n - 1); *w0 = 0.75f; *w1 = 0.25f; }
    else            { *i0 = clampi(k - 1, 0, n - 1); *i1 = k; *w0 = 0.25f; *w1 = 0.75f; }
}

/* the decimation of one direction: taps at positions 2k - 1 ..; returns their number */
static int sited_down(int cosited, float w[4])
{
    if (cosited) { w[0] = 0.25f; w[1] = 0.5f; w[2] = 0.25f; w[3] = 0.f; return 3; }
    w[0] = 0.125f; w[1] = 0.375f; w[2] = 0.375f; w[3] = 0.125f;
    return 4;
}

int orc_colorspace_frame_sited(const orc_colorspace_params_t *cs, const void *const src[3], const int sstride[3],
                               void *const dst[3], const int dstride[3], int w, int h, int depth, int subw, int subh,
                               int h_centred, int v_cosited)
{
    plan_t p;
    if (depth < 8 || depth > 16 || build_plan(&p, cs, depth) != 0) return -1;
    const int bps = depth > 8 ? 2 : 1;
    const int cw = subw ? (w + 1) >> 1 : w, ch = subh ? (h + 1) >> 1 : h;
    float *oy = malloc(sizeof(float) * (size_t)w * h), *ou = malloc(sizeof(float) * (size_t)w * h),
          *ov = malloc(sizeof(float) * (size_t)w * h);
    for (int y = 0; y < h; y++)
        for (int x = 0; x < w; x++)
        {
            int r0 = y, r1 = y, c0 = x, c1 = x;
            float wy0 = 1.f, wy1 = 0.f, wx0 = 1.f, wx1 = 0.f;
            if (subh) sited_up(y, ch, v_cosited, &r0, &r1, &wy0, &wy1);
            if (subw) sited_up(x, cw, !h_centred, &c0, &c1, &wx0, &wx1);
            float uv[2];
            for (int k = 0; k < 2; k++)
            {
                const void *pl = src[1 + k];
                const float s00 = (sample(pl, sstride[1 + k], c0, r0, bps) - p.coff_in) * p.cmul_in;
                const float s10 = (sample(pl, sstride[1 + k], c0, r1, bps) - p.coff_in) * p.cmul_in;
                const float s01 = (sample(pl, sstride[1 + k], c1, r0, bps) - p.coff_in) * p.cmul_in;
                const float s11 = (sample(pl, sstride[1 + k], c1, r1, bps) - p.coff_in) * p.cmul_in;
                /* rows first (a sample that is not interpolated is taken as it is), then columns */
                const float a = subh && wy1 != 0.f ? fmaf(wy1, s10, wy0 * s00) : s00;
                const float b = subh && wy1 != 0.f ? fmaf(wy1, s11, wy0 * s01) : s01;
                uv[k] = subw && wx1 != 0.f ? fmaf(wx1, b, wx0 * a) : a;
            }
            const float yf = (sample(src[0], sstride[0], x, y, bps) - p.yoff_in) * p.ymul_in;
            float o[3];
            convert_px(&p, yf, uv[0], uv[1], o);
            oy[(size_t)y * w + x] = o[0];
            ou[(size_t)y * w + x] = o[1];
            ov[(size_t)y * w + x] = o[2];
        }
    for (int y = 0; y < h; y++)
        for (int x = 0; x < w; x++)
            store(dst[0], dstride[0], x, y, bps, quant(oy[(size_t)y * w + x], p.ymul_out, p.yoff_out, p.vmax));
    float wr[4], wc[4];
    const int nr = sited_down(v_cosited, wr), nc = sited_down(!h_centred, wc);
    for (int k = 0; k < 2; k++)
    {
        const float *o = k ? ov : ou;
        for (int cy = 0; cy < ch; cy++)
            for (int cx = 0; cx < cw; cx++)
            {
                float col[4];
                const int xc = subw ? 2 * cx : cx;
                for (int i = 0; i < nc; i++)
                {
                    const int xx = clampi(xc - 1 + i, 0, w - 1);
                    if (subh)
                    {
                        float s = wr[0] * o[(size_t)clampi(2 * cy - 1, 0, h - 1) * w + xx];
                        for (int j = 1; j < nr; j++) s = fmaf(wr[j], o[(size_t)clampi(2 * cy - 1 + j, 0, h - 1) * w + xx], s);
                        col[i] = s;
                    }
                    else
                        col[i] = o[(size_t)cy * w + xx];
                }
                float v = col[1];
                if (subw)
                {
                    v = wc[0] * col[0];
                    for (int i = 1; i < nc; i++) v = fmaf(wc[i], col[i], v);
                }
                store(dst[1 + k], dstride[1 + k], cx, cy, bps, quant(v, p.cmul_out, p.coff_out, p.vmax));
            }
    }
    free(oy); free(ou); free(ov);
    return 0;
}
