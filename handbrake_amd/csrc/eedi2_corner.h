// eedi2_corner.h - EEDI2 post-processing 2/3: junctions and corners (eedi2_template.c:1391-1904;
// decomb_template.c:432-441), for both engines: PIX = uint8_t (eedi2.hip) or uint16_t (eedi2_16.hip).
//
// The reference's three plane threads share ONE set of derivative arrays (decomb.c:398-403), so
// its own result is a data race; what is reproduced here is the defined order "Y, Cb, Cr one
// after the other" on the same flat arrays (oracle/ref_wrap/wrap_decomb.c:hbref_eedi2_run_serial).
// The flat layout matters: the horizontal pass of gaussian_blur_sqrt2 reads src[x+3] instead of
// src[x-3] at x == width-2 (:1589) — the next row, the row padding, or whatever another plane
// left there — so the planes run one after the other and index the arrays exactly as it does.
// Both blurs are symmetric FIRs whose out-of-range taps are mirrored about the centre (written
// in the reference as doubled coefficients on the surviving side).
#pragma once
#include "eedi2_engine.h"

template <typename PIX>
struct EediCornerArgs
{
    PIX     *src, *tmp;          // srcp (blurred in place) and tmpp of one plane
    int     *c[3];               // cx2, cy2, cxy (shared by the planes)
    int     *t[3];               // tmpc, one per array (the reference reuses one; nothing of it outlives a blur)
    int      pitch, width, height;   // half-height geometry of the plane, in samples
};

// What two of the kernels know of the sample depth: the differences are taken on samples >> shift, the mask's two special
// values are the depth's peak and neutral.  Kernel arguments at 10 / 12 bits; at 8 bits compile-time constants (0, 255,
// 128: the arguments are passed and not read).
template <typename PIX> __device__ __forceinline__ int corner_depth(int at8, int arg) { return sizeof(PIX) == 1 ? at8 : arg; }

__device__ __forceinline__ int fold_tap(int centre, int d, int n, int &hi)
{
    int lo = centre - d;
    hi = centre + d;
    if (lo < 0) lo = hi;
    if (hi >= n) hi = lo;
    return lo;
}

// (the kernels belong to the file that includes this header, like its other kernels: eedi2.hip and eedi2_16.hip each
// get their own eedi_blur_sqrt2)
namespace {

// eedi2_gaussian_blur1 (:1391-1527), one axis per launch: VERT = false src -> tmp, true tmp -> src
template <typename PIX, bool VERT>
__global__ void eedi_blur1(EediCornerArgs<PIX> A)
{
    const int x = blockIdx.x * blockDim.x + threadIdx.x, y = blockIdx.y * blockDim.y + threadIdx.y;
    if (x >= A.width || y >= A.height) return;
    const PIX *in = VERT ? A.tmp : A.src;
    PIX *out = VERT ? A.src : A.tmp;
    const int W[4] = { 26152, 15862, 3539, 291 };
    int acc = (int)in[(size_t)y * A.pitch + x] * W[0] + 32768;
#pragma unroll
    for (int d = 1; d <= 3; d++)
    {
        int hi;
        const int lo = fold_tap(VERT ? y : x, d, VERT ? A.height : A.width, hi);
        const size_t il = VERT ? (size_t)lo * A.pitch + x : (size_t)y * A.pitch + lo;
        const size_t ih = VERT ? (size_t)hi * A.pitch + x : (size_t)y * A.pitch + hi;
        acc += ((int)in[il] + (int)in[ih]) * W[d];
    }
    out[(size_t)y * A.pitch + x] = (PIX)(acc >> 16);
}

// eedi2_calc_derivatives (:1760-1848): differences against clamped neighbours
template <typename PIX>
__global__ void eedi_derivatives(EediCornerArgs<PIX> A, int depth_shift)
{
    const int x = blockIdx.x * blockDim.x + threadIdx.x, y = blockIdx.y * blockDim.y + threadIdx.y;
    if (x >= A.width || y >= A.height) return;
    const int shift = corner_depth<PIX>(0, depth_shift);
    const PIX *s = A.src + (size_t)y * A.pitch;
    const PIX *up = A.src + (size_t)max(y - 1, 0) * A.pitch, *dn = A.src + (size_t)min(y + 1, A.height - 1) * A.pitch;
    const int ix = ((int)s[min(x + 1, A.width - 1)] - (int)s[max(x - 1, 0)]) >> shift;
    const int iy = ((int)up[x] - (int)dn[x]) >> shift;
    const size_t at = (size_t)y * A.pitch + x;
    A.c[0][at] = (ix * ix) >> 1;
    A.c[1][at] = (iy * iy) >> 1;
    A.c[2][at] = (ix * iy) >> 1;
}

// eedi2_gaussian_blur_sqrt2 (:1539-1748), one axis per launch, the three arrays in blockIdx.z:
// VERT = false c -> t (>> 16, with the x+3 read of :1589), true t -> c (>> 18).  It touches no sample: PIX only names
// the argument struct.
template <typename PIX, bool VERT>
__global__ void eedi_blur_sqrt2(EediCornerArgs<PIX> A)
{
    const int x = blockIdx.x * blockDim.x + threadIdx.x, y = blockIdx.y * blockDim.y + threadIdx.y;
    if (x >= A.width || y >= A.height) return;
    const int *in = VERT ? A.t[blockIdx.z] : A.c[blockIdx.z];
    int *out = VERT ? A.c[blockIdx.z] : A.t[blockIdx.z];
    const int W[5] = { 18508, 14415, 6809, 1951, 339 };
    int acc = in[(size_t)y * A.pitch + x] * W[0] + 32768;
#pragma unroll
    for (int d = 1; d <= 4; d++)
    {
        int hi;
        int lo = fold_tap(VERT ? y : x, d, VERT ? A.height : A.width, hi);
        if (!VERT && d == 3 && x == A.width - 2) lo = hi = x + 3;
        const size_t il = VERT ? (size_t)lo * A.pitch + x : (size_t)y * A.pitch + lo;
        const size_t ih = VERT ? (size_t)hi * A.pitch + x : (size_t)y * A.pitch + hi;
        acc += (in[il] + in[ih]) * W[d];
    }
    out[(size_t)y * A.pitch + x] = acc >> (VERT ? 18 : 16);
}

// eedi2_post_process_corner (:1864-1904): msk = tmp2p2, dst = dst2p (row y from rows y+-1, which
// belong to the kept field and are never written here).  The response is evaluated in double, in
// the reference's operation order (int products, 0.09 * s * s, one subtraction, truncation).
template <typename PIX>
__global__ void eedi_post_corner(EediCornerArgs<PIX> A, const PIX *msk, PIX *dst, int field, int height, int depth_peak,
                                 int depth_neutral)
{
    const int x = blockIdx.x * blockDim.x + threadIdx.x, r = blockIdx.y * blockDim.y + threadIdx.y;
    const int y = 8 - field + 2 * r;
    if (x < 4 || x >= A.width - 4 || y >= height - 7) return;
    const size_t at = (size_t)y * A.pitch + x;
    const int m = msk[at];
    if (m == corner_depth<PIX>(255, depth_peak) || m == corner_depth<PIX>(128, depth_neutral)) return;
    bool hit = false;
#pragma unroll
    for (int k = 0; k < 2; k++)
    {
        const size_t i = (size_t)(3 + r + k) * A.pitch + x;
        const int a = A.c[0][i], b = A.c[1][i], c = A.c[2][i];
        const double s = (double)(a + b);
        const double resp = (double)(a * b - c * c) - 0.09 * s * s;
        hit |= (int)resp > 775;
    }
    if (hit) dst[at] = (PIX)(((int)dst[at - A.pitch] + (int)dst[at + A.pitch] + 1) >> 1);
}

} // namespace

// The passes for fields f0 .. f0 + n - 1 of the batch on st, field after field and plane after plane: the derivative
// arrays carry values from plane to plane and from field to field (above).  name: the six launches' profiler names.
// (A member template that launches kernels of this file's anonymous namespace: each engine's file instantiates it for its
// own PIX and no other - the same PIX in two files would be two different functions under one name.)
template <typename PIX>
void EediEngineBase::enqueue_corner(int f0, int n, hbhip_ctx *lc, hipStream_t st, const char *const (&name)[6])
{
    const int s0 = start_ + f0;
    const EediFrame srcp = at_slot(half_[0], s0), tmpp = at_slot(half_[2], s0);
    const EediFrame dst2p = at_slot(full_[0], s0), tmp2p2 = at_slot(full_[1], s0);
    const dim3 blk(64, 4);
    for (int f = 0; f < n; f++)
    {
        const int tff = (int)((tffbits_ >> (f0 + f)) & 1u);
        const size_t foff = (size_t)f * slot_bytes_;
        for (int c = 0; c < 3; c++)
        {
            EediCornerArgs<PIX> A;
            A.src = (PIX *)(srcp.plane[c] + foff); A.tmp = (PIX *)(tmpp.plane[c] + foff);
            for (int i = 0; i < 3; i++) { A.c[i] = deriv_[i].get(); A.t[i] = deriv_tmp_[i].get(); }
            A.pitch = srcp.stride[c] / (int)sizeof(PIX); A.width = srcp.width[c]; A.height = srcp.height[c];
            const dim3 g1((A.width + 63) / 64, (A.height + 3) / 4, 1), g3(g1.x, g1.y, 3);
            HBHIP_LAUNCH_ON(lc, st, name[0], (eedi_blur1<PIX, false>), g1, blk, 0, A);
            HBHIP_LAUNCH_ON(lc, st, name[1], (eedi_blur1<PIX, true>), g1, blk, 0, A);
            HBHIP_LAUNCH_ON(lc, st, name[2], eedi_derivatives<PIX>, g1, blk, 0, A, geo_.depth - 8);
            HBHIP_LAUNCH_ON(lc, st, name[3], (eedi_blur_sqrt2<PIX, false>), g3, blk, 0, A);
            HBHIP_LAUNCH_ON(lc, st, name[4], (eedi_blur_sqrt2<PIX, true>), g3, blk, 0, A);
            const int rows = (dst2p.height[c] - 7 - (8 - tff) + 1) / 2;      // y = 8-field, 10-field, ... < height-7
            if (rows > 0)
                HBHIP_LAUNCH_ON(lc, st, name[5], eedi_post_corner<PIX>, dim3((A.width + 63) / 64, (rows + 3) / 4, 1), blk, 0, A,
                                (const PIX *)(tmp2p2.plane[c] + foff), (PIX *)(dst2p.plane[c] + foff), tff, dst2p.height[c],
                                (1 << geo_.depth) - 1, 1 << (geo_.depth - 1));
        }
    }
}
