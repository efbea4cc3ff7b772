// eedi2_dirmap_vote.h - eedi2_filter_dir_map's vote (eedi2_template.c:649-707) for the FOUR pixels of a thread's dword, shared
// by k_dir_map_fe / k_dir_map4 (eedi2.hip) and tools/dirmap_vote_check.hip, which runs the same text on the host
// (tests/test_dir_map_vote_cpu.py).  Every function is __host__ __device__; the two builtins have plain forms beside them.
//
// Two horizontally adjacent pixels ride in the 16-bit halves of a dword (v_pk_min/max_u16, v_pk_sub/mad_u16).  What the four
// pixels share is made once:
//   - the three rows of the 3 x 6 neighbourhood (columns -1 .. 4) are unpacked as the column pairs X = (-1, 0), Y = (1, 2),
//     Z = (3, 4): 9 v_perm.  A peak (no value: the reference leaves it out of order[], :659-668) becomes DMV_ABSENT, above
//     every value, with 32-bit operations on both halves at once.
//   - every COLUMN is sorted once (3 exchanges per column pair); the pairs (0, 1) and (2, 3) come out of the sorted ones
//     with one v_alignbit each.  A pixel pair's nine slots are then three sorted triples, whichever rows they came from:
//     the vote is a sum and a count, and the midpoint an order statistic - neither asks where a value stood.
//   - ranks 1 .. 4 of the nine (all the midpoint of 4 .. 9 present values can need) are selected from the three sorted
//     triples by dmv_ranks1to4: 21 min / max instead of the 9-input sorting network's 39 that reach them.
#pragma once
#include <hip/hip_runtime.h>
#include <cstdint>

#define DMV_FN __host__ __device__ __forceinline__

typedef uint16_t dmv_h2 __attribute__((ext_vector_type(2)));
typedef int16_t dmv_i2 __attribute__((ext_vector_type(2)));
DMV_FN dmv_h2 dmv_pk(uint32_t v) { return __builtin_bit_cast(dmv_h2, v); }
DMV_FN uint32_t dmv_un(dmv_h2 v) { return __builtin_bit_cast(uint32_t, v); }
DMV_FN dmv_h2 dmv_pk1(uint32_t both) { return dmv_pk(both * 0x00010001u); }
DMV_FN dmv_h2 dmv_min(dmv_h2 a, dmv_h2 b) { return __builtin_elementwise_min(a, b); }
DMV_FN dmv_h2 dmv_max(dmv_h2 a, dmv_h2 b) { return __builtin_elementwise_max(a, b); }
DMV_FN void dmv_cswap(dmv_h2 &a, dmv_h2 &b) { const dmv_h2 lo = dmv_min(a, b), hi = dmv_max(a, b); a = lo; b = hi; }
// The compiler reads a sign bit that is shifted out or spread over its half as a comparison and, there being no packed
// compare, takes the halves apart for it (a v_cmp and a v_cndmask per half and a v_perm to put them together again):
// DMV_KEEP(x) hides where a 32-bit value came from, so that the packed shift stays one.
#if defined(__HIP_DEVICE_COMPILE__)
#define DMV_KEEP(x) asm("" : "+v"(x))
#define DMV_MAD24(a, b, c) (__umul24((a), (b)) + (c))                   /* v_mad_u32_u24 */
#else
#define DMV_KEEP(x) (void)(x)
#define DMV_MAD24(a, b, c) (((a) & 0xffffffu) * ((b) & 0xffffffu) + (c))  /* the same 24 bits of each factor on the host */
#endif
// 0xffff in every half that is negative as a 16-bit integer (v_pk_ashrrev_i16)
DMV_FN uint32_t dmv_neg_mask(dmv_h2 v)
{
    uint32_t m = dmv_un(__builtin_bit_cast(dmv_h2, (dmv_i2)(__builtin_bit_cast(dmv_i2, v) >> 15)));
    DMV_KEEP(m);
    return m;
}
// [a < b] per half as 0 / 1, halves below 2^15 (the borrow of a - b)
DMV_FN dmv_h2 dmv_lt(dmv_h2 a, dmv_h2 b) { return (dmv_h2)((dmv_h2)(a - b) >> 15); }

// v_perm_b32: byte k of the result is byte sel[k] of {hi, lo} (0-3 = lo, 4-7 = hi), 0 for a selector of 12
DMV_FN uint32_t dmv_perm(uint32_t hi, uint32_t lo, uint32_t sel)
{
#if defined(__HIP_DEVICE_COMPILE__)
    return __builtin_amdgcn_perm(hi, lo, sel);
#else
    const uint64_t w = ((uint64_t)hi << 32) | lo;
    uint32_t r = 0;
    for (int k = 0; k < 4; k++)
    {
        const uint32_t s = (sel >> (8 * k)) & 0xffu;
        r |= (s < 8 ? (uint32_t)((w >> (8 * s)) & 0xffu) : s == 12 ? 0u : 0xffu) << (8 * k);
    }
    return r;
#endif
}
// bytes a and b of the 8-byte window {hi, lo} as the halves of a dword
#define DMV_BYTES(hi, lo, a, b) dmv_perm((hi), (lo), 0x0c000c00u | ((uint32_t)(b) << 16) | (uint32_t)(a))
// the halves (lo.high, hi.low): the column pair between two neighbouring ones (v_alignbit_b32)
DMV_FN uint32_t dmv_between(uint32_t hi, uint32_t lo) { return (lo >> 16) | (hi << 16); }

// (int)((float)a / (float)b + 0.5f) of the votes (a = sum + mid <= 2559, b = count + 1 <= 10), given 4a + 2b + 1 and 4b.
// The float expression equals floor((2a + b) / 2b) there (tests/test_eedi2_identities_cpu.py); with 2a + b = 2b q + r,
// (4a + 2b + 1) / 4b = q + (2r + 1) / 4b lies at least 1 / 40 away from every integer, and the product with v_rcp_f32's
// reciprocal (1 ulp) is off by less than 10257 x 2^-22: the truncation is q, with no compare behind it
// (every case: tests/test_dir_map_vote_cpu.py with the reciprocal pushed 4 ulp either way; on the GPU: tools/vote_avg_check.hip).
DMV_FN int dmv_vote_quot(uint32_t num, uint32_t den)
{
#if defined(__HIP_DEVICE_COMPILE__)
    const float r = __builtin_amdgcn_rcpf((float)den);
#else
    const float r = 1.0f / (float)den;
#endif
    return (int)((float)num * r);
}
DMV_FN int dmv_vote_avg(int a, int b) { return dmv_vote_quot(4u * (uint32_t)a + 2u * (uint32_t)b + 1u, 4u * (uint32_t)b); }

// limlut[d >> 2] + 1 for d = |mid - neutral| < 2^15, both halves.  limlut (eedi2.c:21-25 as 8-bit pixels) in closed form:
// min(12, 6 + ((i - [i >= 8]) >> 1)), 255 from i = 31 on (tests/test_eedi2_identities_cpu.py::test_limlut_closed_form);
// [i >= 8] = min(i >> 3, 1), and i >= 31 <=> d >= 124 <=> bit 15 of d + (2^15 - 124)
DMV_FN dmv_h2 dmv_lim1(dmv_h2 d)
{
    const dmv_h2 i = d >> 2;
    const dmv_h2 g = dmv_min((dmv_h2)(i >> 3), dmv_pk1(1));
    const dmv_h2 l1 = dmv_min((dmv_h2)(((i - g) >> 1) + dmv_pk1(7)), dmv_pk1(13));
    uint32_t far = dmv_un((dmv_h2)(d + dmv_pk1(0x8000 - 124)));
    DMV_KEEP(far);
    return dmv_max(l1, dmv_pk((far >> 7) & 0x01000100u));
}

constexpr uint32_t DMV_ABSENT = 0x7fffu;       // 0x00ff + 0x7f00: above every value, below 2^15

// Ranks 1 .. 4 (rank 0 = the smallest) of the nine values of three sorted triples a0 <= a1 <= a2, b0 .., c0 ...
// Sort the three lows, the three mids, the three highs among themselves: a 3 x 3 tableau l / m / h whose rows and columns
// both ascend (the k-th smallest mid is above the k-th smallest low).  An entry in row r, column c has at least
// (r + 1)(c + 1) - 1 entries below it: l0 is rank 0, and m2, h1, h2 have five or more below them, so ranks 1 .. 4 are the
// four smallest of { l1, m0, l2, h0, m1 }, of which l1, m0 <= m1, l1 <= l2, m0 <= h0: s1 = min(l1, m0), and the rest is the
// merge of (max(l1, m0), m1) with (l2, h0) sorted, its top left out.  12 + 9 min / max
// (every 0 / 1 / absent input against a sort: tests/test_dir_map_vote_cpu.py).
DMV_FN void dmv_ranks1to4(dmv_h2 a0, dmv_h2 a1, dmv_h2 a2, dmv_h2 b0, dmv_h2 b1, dmv_h2 b2, dmv_h2 c0, dmv_h2 c1, dmv_h2 c2,
                          dmv_h2 &s1, dmv_h2 &s2, dmv_h2 &s3, dmv_h2 &s4)
{
    dmv_cswap(a0, b0); dmv_cswap(b0, c0); dmv_cswap(a0, b0);          // lows: l1 = b0, l2 = c0
    dmv_cswap(a1, b1); dmv_cswap(b1, c1); dmv_cswap(a1, b1);          // mids: m0 = a1, m1 = b1
    const dmv_h2 h0 = dmv_min(dmv_min(a2, b2), c2);
    s1 = dmv_min(b0, a1);
    dmv_h2 x = dmv_max(b0, a1), c = c0, d = h0;
    dmv_cswap(c, d);
    s2 = dmv_min(x, c);
    const dmv_h2 t = dmv_max(x, c), u = dmv_min(b1, d);
    s3 = dmv_min(t, u);
    s4 = dmv_max(t, u);
}

// The vote of one pixel pair: its nine slots as three sorted column triples (peaks = DMV_ABSENT), absent = how many of them
// are peaks, per half, in units of 0x0100.  val = the rounded average of the votes per half (low byte), cnt = the votes.
// With fewer than 4 values the midpoint may be a DMV_ABSENT or half of one; the limit is then 255 and the bounds of the
// vote leave out every value and, the upper one being capped at DMV_ABSENT, every absent slot: cnt = 0.
DMV_FN void dmv_pair_vote(const dmv_h2 *A, const dmv_h2 *B, const dmv_h2 *C, uint32_t absent, uint32_t &val, uint32_t &cnt)
{
    dmv_h2 s1, s2, s3, s4;
    dmv_ranks1to4(A[0], A[1], A[2], B[0], B[1], B[2], C[0], C[1], C[2], s1, s2, s3, s4);
    // midpoint of the n = 9 - absent present values: n <= 5 <=> absent >= 4, n <= 7 <=> absent >= 2, n even <=> absent odd
    const dmv_h2 ab = dmv_pk(absent), one = dmv_pk1(1);
    const uint32_t m5 = dmv_neg_mask(dmv_pk1(0x03ff) - ab), m7 = dmv_neg_mask(dmv_pk1(0x01ff) - ab);
    const uint32_t meven = dmv_neg_mask(ab << 7);
#define DMV_SEL(m, x, y) (((m) & (x)) | (~(m) & (y)))                    /* v_bfi_b32 */
    const uint32_t hi = DMV_SEL(m5, dmv_un(s2), DMV_SEL(m7, dmv_un(s3), dmv_un(s4)));
    const uint32_t lo = DMV_SEL(m5, dmv_un(s1), DMV_SEL(m7, dmv_un(s2), dmv_un(s3)));
    const dmv_h2 mid = dmv_pk(DMV_SEL(meven, dmv_un((dmv_h2)((dmv_pk(lo) + dmv_pk(hi) + one) >> 1)), hi));
#undef DMV_SEL
    // the vote (:685-697): values within lim = limlut[|mid - neutral| >> 2] of the midpoint, mid - lim - 1 < v < mid + lim + 1
    // as the signs of two differences (an absent slot is never below the capped upper bound)
    const dmv_i2 t = __builtin_bit_cast(dmv_i2, (dmv_h2)(mid - dmv_pk1(128)));
    const dmv_h2 lim1 = dmv_lim1(__builtin_bit_cast(dmv_h2, __builtin_elementwise_max(t, (dmv_i2)(-t))));
    const dmv_h2 above = dmv_min((dmv_h2)(mid + lim1), dmv_pk1(DMV_ABSENT));
    uint32_t below_ = dmv_un((dmv_h2)(mid - lim1));
    DMV_KEEP(below_);                                                  // (or every slot adds lim1 to its value first)
    const dmv_h2 below = dmv_pk(below_);
    dmv_h2 sum = mid;
    uint32_t n = 0;
    const dmv_h2 *cols[3] = { A, B, C };
#pragma unroll
    for (int i = 0; i < 9; i++)
    {
        const dmv_h2 v = cols[i / 3][i % 3];
        const uint32_t in = ((dmv_un((dmv_h2)(v - above)) & dmv_un((dmv_h2)(below - v))) >> 15) & 0x00010001u;
        n += in;
        sum += dmv_pk(in) * v;
    }
    // (4 (sum + mid) + 2 (n + 1) + 1) / (4 (n + 1)), see dmv_vote_quot
    const uint32_t num = dmv_un((dmv_h2)((sum << 2) + (dmv_pk(n) << 1) + dmv_pk1(3))), den = (n << 2) + 0x00040004u;
    val = (uint32_t)dmv_vote_quot(num & 0xffffu, den & 0xffffu) | ((uint32_t)dmv_vote_quot(num >> 16, den >> 16) << 16);
    cnt = n;
}

// The three rows as column pairs X = (-1, 0), Y = (1, 2), Z = (3, 4), peaks lifted to DMV_ABSENT; aX / aY / aZ = the peaks of
// each column, per half, in units of 0x0100 (the carry of value + 1 into bit 8, both halves with one 32-bit addition)
DMV_FN void dmv_unpack(const uint32_t (*w)[3], dmv_h2 *X, dmv_h2 *Y, dmv_h2 *Z, uint32_t &aX, uint32_t &aY, uint32_t &aZ)
{
    aX = aY = aZ = 0;
#pragma unroll
    for (int r = 0; r < 3; r++)
    {
        uint32_t v[3] = { DMV_BYTES(w[r][1], w[r][0], 3, 4), DMV_BYTES(w[r][1], w[r][0], 5, 6), DMV_BYTES(w[r][2], w[r][1], 3, 4) };
        uint32_t *a[3] = { &aX, &aY, &aZ };
#pragma unroll
        for (int k = 0; k < 3; k++)
        {
            const uint32_t peak = (v[k] + 0x00010001u) & 0x01000100u;   // 0x0100 per half that holds 255
            *a[k] += peak;
            v[k] = DMV_MAD24(peak >> 8, 0x7f00u, v[k]);                 // -> DMV_ABSENT (both factors within 24 bits)
        }
        X[r] = dmv_pk(v[0]); Y[r] = dmv_pk(v[1]); Z[r] = dmv_pk(v[2]);
    }
}
// the peaks among the nine slots of the two pixels between the column pairs L and R (units of 0x0100)
DMV_FN uint32_t dmv_pair_absent(uint32_t aL, uint32_t aR) { return aL + dmv_between(aR, aL) + aR; }

// eedi2_filter_dir_map for the four pixels of a dword: rows above / own / below as the bytes x - 4 .. x + 7 (u0 u1 u2, c0 c1 c2,
// d0 d1 d2; a row that does not count - the first / last rows of the _2x forms - all 0xff).  Returns the pass's value for
// each pixel as its byte; the caller takes them for the pixels the pass works on.  PAIRS: bit 0 = pixels 0 and 1 wanted,
// bit 1 = pixels 2 and 3 (the ring of a tile needs one pixel of a dword).
template <int PAIRS>
DMV_FN uint32_t dir_map_quad(uint32_t u0, uint32_t u1, uint32_t u2, uint32_t c0, uint32_t c1, uint32_t c2, uint32_t d0, uint32_t d1, uint32_t d2)
{
    const uint32_t w[3][3] = { { u0, u1, u2 }, { c0, c1, c2 }, { d0, d1, d2 } };
    dmv_h2 X[3], Y[3], Z[3];
    uint32_t aX, aY, aZ;
    dmv_unpack(w, X, Y, Z, aX, aY, aZ);
    dmv_cswap(X[0], X[1]); dmv_cswap(X[1], X[2]); dmv_cswap(X[0], X[1]);
    dmv_cswap(Y[0], Y[1]); dmv_cswap(Y[1], Y[2]); dmv_cswap(Y[0], Y[1]);
    dmv_cswap(Z[0], Z[1]); dmv_cswap(Z[1], Z[2]); dmv_cswap(Z[0], Z[1]);
    uint32_t val01 = 0, val23 = 0, cnt01 = 0, cnt23 = 0;
    if (PAIRS & 1)
    {
        dmv_h2 XY[3];
#pragma unroll
        for (int k = 0; k < 3; k++) XY[k] = dmv_pk(dmv_between(dmv_un(Y[k]), dmv_un(X[k])));
        dmv_pair_vote(X, XY, Y, dmv_pair_absent(aX, aY), val01, cnt01);
    }
    if (PAIRS & 2)
    {
        dmv_h2 YZ[3];
#pragma unroll
        for (int k = 0; k < 3; k++) YZ[k] = dmv_pk(dmv_between(dmv_un(Z[k]), dmv_un(Y[k])));
        dmv_pair_vote(Y, YZ, Z, dmv_pair_absent(aY, aZ), val23, cnt23);
    }
    // the four pixels as bytes: a value with 5 votes, or with 4 where the pixel itself holds one (:698-706), else a peak
    const uint32_t vals = dmv_perm(val23, val01, 0x06040200u), cnts = dmv_perm(cnt23, cnt01, 0x06040200u);
    const uint32_t peak_c = (((c1 & 0x7f7f7f7fu) + 0x01010101u) & c1) & 0x80808080u;       // 0x80 per byte of c1 that is 0xff
    const uint32_t own = (~peak_c >> 7) & 0x01010101u;
    const uint32_t k = (cnts + own + 0x7b7b7b7bu) & 0x80808080u;                             // votes + [own value] >= 5
    const uint32_t keep = k | (k - (k >> 7));
    return vals | ~keep;
}
