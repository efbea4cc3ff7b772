/* eedi2_oracle.c — CPU restatement of EEDI2 as decomb drives it (8-bit, and the 16-bit
 * template instantiation at depths 10 and 12; post-processing 0..3).
 * TEST INFRASTRUCTURE ONLY (see oracle.h).
 *
 * Follows the reference's libhb/templates/eedi2_template.c pass by pass and the
 * pass order of eedi2_interpolate_plane (templates/decomb_template.c:366-441).
 * The reference is one template with pixel = uint8_t (eedi2_planer_8) and pixel = uint16_t
 * (eedi2_planer_16, decomb.c:324-331); so is this: the passes are in eedi2_oracle_px.h, included
 * twice below.  Both are pinned plane by plane against the reference's own planers
 * (tests/test_oracle_vs_ref.py).
 * Things that look like mistakes but are the reference's behaviour, kept here:
 *   - build_edge_mask is CALLED with (magnitude, variance, laplacian) but DECLARED
 *     (mthresh, lthresh, vthresh) (decomb_template.c:391-393 vs eedi2_template.c:122):
 *     the variance test uses the laplacian setting and vice versa;
 *   - it clears only the upper half of the mask (eedi2_template.c:132): the lower
 *     half keeps whatever the previous run left there (the mask is stateful);
 *   - mark_directions_2x compares dmskp[x+1] with dmskpn[x-1] (:835);
 *   - every pass indexes a flat buffer, so "x-1-u" style offsets run into the
 *     neighbouring row / plane / padding (e.g. :395-447, :1194-1195, :1296-1310).
 *     The nine scratch frames are therefore laid out byte-for-byte as
 *     hb_frame_buffer_init lays them out (fifo.c:820-881) inside zeroed guards.
 *   - post-processing 2/3: the three plane threads of the reference share ONE set of
 *     derivative arrays (decomb.c:398-403, decomb_template.c:380-383), so its own
 *     output is a data race; the semantics pinned here (and by hbref_eedi2_run_serial
 *     in ref_wrap/wrap_decomb.c) are "planes one after the other, Y Cb Cr", arrays
 *     zeroed once at start (the reference mallocs them: fresh pages read as 0);
 *   - gaussian_blur_sqrt2's horizontal pass reads src[x+3] instead of src[x-3] at
 *     x == width-2 (:1589): an element of the next row / of the padding / of whatever
 *     another plane left in the shared array.  Kept, on the same flat arrays.
 *
 * What the reference does differently above 8 bits is marked "16:" where it happens: thresholds are
 * shifted by depth-8 or typed `pixel` so that they wrap at the sample width (nt * 13 with nt = 50 is
 * 138 at 8 bits), peak / neutral come from the depth, the limlut is << (depth-8) with its last two
 * entries (pixel)(-1) << shift, sums and squares are taken on samples >> (depth-8), and some of the
 * `>> 2` of the 8-bit code become `>> (2 + shift)` while others stay.  Those values belong to the
 * object (eedi2_depth_t, filled by `new`): objects of different depths can be run in turn.
 */
#include "oracle.h"

#include <stddef.h>
#include <stdlib.h>
#include <string.h>

#define GUARD   4096      /* samples */

static const uint8_t LIMLUT8[33] = { 6, 6, 7, 7, 8, 8, 9, 9, 9, 10, 10, 11, 11, 12, 12, 12, 12, 12, 12, 12,
                                     12, 12, 12, 12, 12, 12, 12, 12, 12, 12, 12, 255, 255 };   /* eedi2.c:21-25 as u8 */

/* what a pass needs to know about the depth */
typedef struct
{
    int shift, peak, neutral;     /* depth - 8, (1 << depth) - 1, 1 << (depth - 1) */
    int limlut[33];               /* eedi2_init_limlut (:23-33) */
} eedi2_depth_t;

static inline int iabs(int v) { return v < 0 ? -v : v; }
static inline int imin(int a, int b) { return a < b ? a : b; }
static inline int imax(int a, int b) { return a > b ? a : b; }

/* insertion sort of <= 9 values + the reference's midpoint rule (eedi2.c:65-80, e.g. :500-502) */
static int sorted_mid(int *v, int n)
{
    for (int i = 1; i < n; i++)
    {
        const int t = v[i];
        int j = i;
        while (j > 0 && v[j - 1] > t) { v[j] = v[j - 1]; j--; }
        v[j] = t;
    }
    return (n & 1) ? v[n >> 1] : (v[(n - 1) >> 1] + v[n >> 1] + 1) >> 1;
}

/* mean of the values within `lim` of mid, mixed with mid and rounded (:701 etc.);
 * returns the count of values used through *count. */
static int vote(const int *v, int n, int mid, int lim, int *count)
{
    int sum = 0, cnt = 0;
    for (int i = 0; i < n; i++)
        if (iabs(v[i] - mid) <= lim) { cnt++; sum += v[i]; }
    *count = cnt;
    return (int)(((float)(sum + mid) / (float)(cnt + 1)) + 0.5f);
}

/* Both blurs are symmetric FIR filters whose taps, where they would fall outside the row /
 * column, are replaced by their mirror image about the centre (the reference writes this as
 * doubled coefficients on the surviving side: 582 = 2*291 ... :1399-1424, :1549-1594). */
static inline int fold(int centre, int d, int n, int *partner)
{
    int lo = centre - d, hi = centre + d;
    if (lo < 0) lo = hi;
    if (hi >= n) hi = lo;
    *partner = hi;
    return lo;
}

/* eedi2_gaussian_blur_sqrt2 (:1539-1748): 9 taps on an int array, >>16 then >>18 */
static void gaussian_blur_sqrt2(const int *src, int *tmp, int *dst, int pitch, int width, int height)
{
    static const int W[5] = { 18508, 14415, 6809, 1951, 339 };
    for (int y = 0; y < height; y++)
    {
        const int *s = src + (size_t)y * pitch;
        int *t = tmp + (size_t)y * pitch;
        for (int x = 0; x < width; x++)
        {
            int acc = s[x] * W[0] + 32768;
            for (int d = 1; d <= 4; d++)
            {
                int hi, lo = fold(x, d, width, &hi);
                if (d == 3 && x == width - 2) lo = hi = x + 3;       /* :1589 reads x+3, past the row */
                acc += (s[lo] + s[hi]) * W[d];
            }
            t[x] = acc >> 16;
        }
    }
    for (int y = 0; y < height; y++)
        for (int x = 0; x < width; x++)
        {
            int acc = tmp[(size_t)y * pitch + x] * W[0] + 32768;
            for (int d = 1; d <= 4; d++)
            {
                int hi, lo = fold(y, d, height, &hi);
                acc += (tmp[(size_t)lo * pitch + x] + tmp[(size_t)hi * pitch + x]) * W[d];
            }
            dst[(size_t)y * pitch + x] = acc >> 18;
        }
}

#define PIXEL uint8_t
#define PX(n) n##_8
#define OBJ struct orc_eedi2
#define SHIFT 0       /* orc_eedi2_new passes depth 8: every shift by depth-8 folds away */
#include "eedi2_oracle_px.h"
#undef PIXEL
#undef PX
#undef OBJ
#define PIXEL uint16_t
#define PX(n) n##_16
#define OBJ struct orc_eedi2_16
#include "eedi2_oracle_px.h"
#undef PIXEL
#undef PX
#undef OBJ

orc_eedi2_t *orc_eedi2_new(int width, int height, const orc_eedi2_params_t *p) { return new_8(width, height, 8, p); }
void orc_eedi2_free(orc_eedi2_t *e) { free_8(e); }
const uint8_t *orc_eedi2_plane(orc_eedi2_t *e, int buffer, int plane, int *stride, int *height)
{
    return plane_8(e, buffer, plane, stride, height);
}
void orc_eedi2_run_partial(orc_eedi2_t *e, const uint8_t *const cur[3], const int stride[3], int tff, int npasses)
{
    run_partial_8(e, cur, stride, tff, npasses);
}
void orc_eedi2_run(orc_eedi2_t *e, const uint8_t *const cur[3], const int stride[3], int tff)
{
    run_partial_8(e, cur, stride, tff, 1000);
}

orc_eedi2_16_t *orc_eedi2_16_new(int width, int height, int depth, const orc_eedi2_params_t *p)
{
    return new_16(width, height, depth, p);
}
void orc_eedi2_16_free(orc_eedi2_16_t *e) { free_16(e); }
const uint16_t *orc_eedi2_16_plane(orc_eedi2_16_t *e, int buffer, int plane, int *stride, int *height)
{
    return plane_16(e, buffer, plane, stride, height);
}
void orc_eedi2_16_run_partial(orc_eedi2_16_t *e, const uint16_t *const cur[3], const int stride[3], int tff, int npasses)
{
    run_partial_16(e, cur, stride, tff, npasses);
}
void orc_eedi2_16_run(orc_eedi2_16_t *e, const uint16_t *const cur[3], const int stride[3], int tff)
{
    run_partial_16(e, cur, stride, tff, 1000);
}
