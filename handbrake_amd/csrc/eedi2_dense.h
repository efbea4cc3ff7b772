// eedi2_dense.h - the row walk of the dense calc_directions search (calc_dir_dense, eedi2.hip).  calc_dir_dense16 keeps
// its whole-array trip: the same walk measured slower there.
#pragma once
#include <hip/hip_runtime.h>
#include <cstdint>

// The sums of one direction of a trip, walked down the row pairs r = 0 .. R + 2 of a column of R rows: push(r, P_r, Q_r)
// forms the partial sums that end at pair r, and once pair j + 3 is in, cands(j, ..) gives the five candidates of row j
// (diff (b) = S_{j+1} + S_{j+2}, diffa = diff + S_j, diffc = diff + S_{j+3}, diffe = P_j + .. + P_{j+3}, diffd = Q_j + .. +
// Q_{j+3}; X: the poison of a step row j does not take).  The arrays are indexed by unrolled constants: they are names,
// not storage - what is live at a time is the last four pairs' sums.
template <int R, bool PRED>
struct CdRun
{
    static constexpr int NE = R + 3;
    uint32_t P[NE], Q[NE], S[NE], P2[NE], Q2[NE], S2[NE], S3[NE];
    __device__ __forceinline__ void push(int r, uint32_t p, uint32_t q)
    {
        P[r] = p; Q[r] = q; S[r] = p + q;
        if (r >= 1) { P2[r - 1] = P[r - 1] + p; Q2[r - 1] = Q[r - 1] + q; }
        if (!PRED && r >= 1) S2[r - 1] = S[r - 1] + S[r];
        if (!PRED && r >= 2) S3[r - 2] = S2[r - 2] + S[r];          // diffc of a row is diffa of the next one
    }
    __device__ __forceinline__ void cands(int j, uint32_t X, uint32_t &ca, uint32_t &cb, uint32_t &cc, uint32_t &cd, uint32_t &ce) const
    {
        if (PRED)
        {
            cb = S[j + 1] + S[j + 2] + X; ca = cb + S[j]; cc = cb + S[j + 3];
            ce = P2[j] + P2[j + 2] + X;   cd = Q2[j] + Q2[j + 2] + X;
        }
        else
        {
            cb = S2[j + 1]; ca = S3[j]; cc = S3[j + 1];
            ce = P2[j] + P2[j + 2]; cd = Q2[j] + Q2[j + 2];
        }
    }
};

// An empty asm on the five keys of row j once its candidates are folded in: the walk's rows stay in order, so that the
// compiler does not hoist the table reads and SADs of later rows above it and keep them all live
#define CD_FENCE_KEYS(j) asm volatile("" : "+v"(ka[j]), "+v"(kb[j]), "+v"(kc[j]), "+v"(kd[j]), "+v"(ke[j]))
