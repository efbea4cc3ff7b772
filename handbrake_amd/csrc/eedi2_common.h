// eedi2_common.h - the small device helpers of the EEDI2 kernels that do not depend on the sample width, shared by
// eedi2.hip (8-bit samples) and eedi2_16.hip (10 / 12-bit samples).  Pairs that differ in formulation, not just in the
// samples they see (mid9 / mid9q, vote1 / vote1q), stay with their kernels.
#pragma once
#include <hip/hip_runtime.h>
#include <cstdint>

// (internal to the file that includes this header, like the kernels that use them)
namespace {

__device__ __forceinline__ int iabs(int v) { return v < 0 ? -v : v; }

// insertion sort + midpoint rule (eedi2.c:65-80)
__device__ __forceinline__ int sorted_mid(int *v, int n)
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

// Register-only variant for the dir-map kernels: the candidates sit in fixed slots (an absent one holds a value larger
// than any sample and farther from any midpoint than any vote limit: ABSENT in eedi2.hip, ABSENT16 in eedi2_16.hip), a
// sorting network orders them, and the n present values are then the first n -- no data-dependent loop, no indexed
// register file.
__device__ __forceinline__ void cswap(int &a, int &b)
{
    const int lo = min(a, b), hi = max(a, b);
    a = lo; b = hi;
}

// midpoint of the n present values among 6 slots (n >= 3); the slots end up sorted
__device__ __forceinline__ int mid6(int &v0, int &v1, int &v2, int &v3, int &v4, int &v5, int n)
{
    cswap(v0, v5); cswap(v1, v3); cswap(v2, v4);
    cswap(v1, v2); cswap(v3, v4);
    cswap(v0, v3); cswap(v2, v5);
    cswap(v0, v1); cswap(v2, v3); cswap(v4, v5);
    cswap(v1, v2); cswap(v3, v4);
    // n = 3..6: lower middle index 1,1,2,2 ; upper 1,2,2,3
    const int lo = n <= 4 ? v1 : v2;
    const int hi = n <= 3 ? v1 : (n <= 5 ? v2 : v3);
    return (n & 1) ? hi : (lo + hi + 1) >> 1;
}

// calc_directions: bit t of a mask row's window - a peak among columns start + t .. + 2 (len + 2 <= 63 bits of the
// row's bitmap)
__device__ __forceinline__ uint64_t calc_dir_window(const uint64_t *bits, int start, uint64_t lenmask)
{
    const int wq = start >> 6, sh = start & 63;
    const uint64_t lo = bits[wq], hi = bits[wq + 1];
    const uint64_t w = sh ? (lo >> sh) | (hi << (64 - sh)) : lo;
    return (w | (w >> 1) | (w >> 2)) & lenmask;
}

// interpolate_lattice's 2-state maps.  later o earlier: the map that applies `earlier` first (the lane / pass
// composition against the pixel-by-pixel walk: tests/test_eedi2_identities_cpu.py::
// test_lattice_resolve_scan_equals_the_serial_walk, tests/test_eedi2_resolve_wave_cpu.py)
__device__ __forceinline__ unsigned lr_compose(unsigned later, unsigned earlier)
{
    return ((later >> (earlier & 1u)) & 1u) | (((later >> ((earlier >> 1) & 1u)) & 1u) << 1);
}

// Two 16-bit values in the halves of a dword, for the packed instructions (v_pk_min_u16 / v_pk_max_u16, v_pk_sub / add /
// mad_u16): two horizontally adjacent 8-bit pixels widened, or two 16-bit samples as they lie in memory.
typedef uint16_t u16x2 __attribute__((ext_vector_type(2)));
typedef int16_t i16x2 __attribute__((ext_vector_type(2)));
__device__ __forceinline__ u16x2 pk(uint32_t v) { return __builtin_bit_cast(u16x2, v); }
__device__ __forceinline__ uint32_t un(u16x2 v) { return __builtin_bit_cast(uint32_t, v); }
__device__ __forceinline__ u16x2 pk1(uint32_t both) { return pk(both * 0x00010001u); }
// [a < b] per half as 0 / 1 for halves below 2^15: the borrow of a - b (two packed instructions; written as a comparison
// or as min(saturated difference, 1) the compiler unpacks it into a compare and a select per half)
__device__ __forceinline__ u16x2 pk_lt(u16x2 a, u16x2 b) { return (u16x2)((u16x2)(a - b) >> 15); }
__device__ __forceinline__ void cswap2(u16x2 &a, u16x2 &b)
{
    const u16x2 lo = __builtin_elementwise_min(a, b), hi = __builtin_elementwise_max(a, b);
    a = lo; b = hi;
}

} // namespace
