// lapsharp_rowdot.h - the arithmetic of lapsharp3_wide_kernel (sharpen.hip): the 3 x 3 Laplacian of 8-bit samples as byte dot
// products, shared with tools/lapsharp_rowdot_check.hip, which runs the same text on the host
// (tests/test_lapsharp_rowdot_cpu.py).  Every function is __host__ __device__; the builtins have plain forms beside them.
//
// Both 3 x 3 tables (lapsharp.c:37-52) are symmetric with corner a <= 0, edge b <= 0, centre c > 0.  With l / m / r the
// left / own / right sample of a pixel in one row,
//     U = |a| l + |b| m + |a| r        what the row gives to the rows above and below it, negated
//     H = |b| l         + |b| r        what it gives to its own row beside the centre, negated
// and the nine-tap sum of row y is c m[y] - (U[y-1] + H[y] + U[y+1]): the taps go in as magnitudes (v_dot4_u32_u8 takes
// unsigned bytes) and the sign comes in where the rows combine.  A pixel's window is the dword (l, m, r, x): the fourth
// byte meets a zero tap.  The mix as one float multiply (lap_float_mix, sharpen.hip) wants sum - kinv centre, which is
// (c - kinv) m - N with N the bracket above: kinv folds into the centre tap.
#pragma once
#include <hip/hip_runtime.h>
#include <cstdint>

#define LRD_FN __host__ __device__ __forceinline__

// v_alignbyte_b32: bytes sh .. sh + 3 of the eight bytes {hi, lo}, sh in 0 .. 3
LRD_FN uint32_t lrd_alignbyte(uint32_t hi, uint32_t lo, int sh)
{
#if defined(__HIP_DEVICE_COMPILE__)
    return __builtin_amdgcn_alignbyte(hi, lo, (uint32_t)sh);
#else
    return (uint32_t)(((((uint64_t)hi) << 32) | lo) >> (8 * sh));
#endif
}

// v_dot4_u32_u8: acc + the sum of the four byte products
LRD_FN uint32_t lrd_udot4(uint32_t x, uint32_t taps, uint32_t acc)
{
#if defined(__HIP_DEVICE_COMPILE__)
    return __builtin_amdgcn_udot4(x, taps, acc, false);
#else
    for (int k = 0; k < 4; k++) acc += ((x >> (8 * k)) & 0xffu) * ((taps >> (8 * k)) & 0xffu);
    return acc;
#endif
}

// the tap dwords of a table; false where the table is not of the shape above (the caller keeps lapsharp3_rows_kernel)
struct LrdTaps { uint32_t tu, th; int c; };
LRD_FN bool lrd_taps(int a, int b, int c, LrdTaps &t)
{
    if (a > 0 || b > 0 || c < 0 || a < -255 || b < -255 || c > 255) return false;
    const uint32_t ma = (uint32_t)-a, mb = (uint32_t)-b;
    t.tu = ma | (mb << 8) | (ma << 16);
    t.th = mb | (mb << 16);
    t.c = c;
    return true;
}

// The window of pixel p of a thread's NDW dwords: ext[] = the dword to the left, the thread's own, the dword to the right
// (bytes x0 - 4 .. x0 + 4 NDW + 3); the window starts one byte left of the pixel.
template <int NDW>
LRD_FN uint32_t lrd_window(const uint32_t (&ext)[NDW + 2], int p)
{
    const int o = 3 + p;
    return (o & 3) ? lrd_alignbyte(ext[(o >> 2) + 1], ext[o >> 2], o & 3) : ext[o >> 2];
}

LRD_FN uint32_t lrd_row_u(uint32_t win, const LrdTaps &t) { return lrd_udot4(win, t.tu, 0u); }
LRD_FN uint32_t lrd_row_h(uint32_t win, const LrdTaps &t) { return lrd_udot4(win, t.th, 0u); }
// N of a pixel from the H of its own row and the U of the rows above and below (one v_add3_u32)
LRD_FN uint32_t lrd_neg_sum(uint32_t h_own, uint32_t u_above, uint32_t u_below) { return h_own + u_above + u_below; }
// the reference's accumulator (lapsharp.c:148-172): fits int16 for both tables
LRD_FN int lrd_acc(int centre, uint32_t n, const LrdTaps &t) { return t.c * centre - (int)n; }

// The one-float-multiply mix for byte k of the thread's dword `own`: (int)((float)(acc - kinv centre) * mixf) + centre,
// clamped to 0 .. 255, as a float that holds the clamped integer's value BEFORE the clamp - the caller packs it with
// v_cvt_pk_u8_f32, which saturates.  ckf = (float)(c - kinv).  Every intermediate is an integer below 2^24 in magnitude
// ((c - kinv) * 255 + 20 * 255), so the fused multiply-add is exact and the product has the one rounding the reference
// form has; the truncation is v_trunc_f32 and the last sum is exact.
template <int K>
LRD_FN float lrd_mix_fast(uint32_t own, uint32_t n, float ckf, float mixf)
{
    const float fm = (float)((own >> (8 * K)) & 0xffu);                   // v_cvt_f32_ubyteK
#if defined(__HIP_DEVICE_COMPILE__)
    const float t = __builtin_fmaf(ckf, fm, -(float)n);
    return __builtin_truncf(t * mixf) + fm;
#else
    const float t = __builtin_fmaf(ckf, fm, -(float)n);
    const volatile float prod = t * mixf;                                 // one rounding, as v_mul_f32
    return __builtin_truncf(prod) + fm;
#endif
}
// what v_cvt_pk_u8_f32 makes of such a float
LRD_FN uint32_t lrd_sat_u8(float v) { return v <= 0.f ? 0u : v >= 255.f ? 255u : (uint32_t)v; }
