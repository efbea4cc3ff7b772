// dot2.h — two 16-bit taps a v_dot2_i32_i16: a.lo * b.lo + a.hi * b.hi + acc, the halves signed.  The one copy behind the
// Lanczos kernels (alias.hip) and the format scaler (format.hip).
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

typedef short s16x2 __attribute__((ext_vector_type(2)));
__device__ __forceinline__ int dot2(uint32_t a, uint32_t b, int acc)
{
    return __builtin_amdgcn_sdot2(__builtin_bit_cast(s16x2, a), __builtin_bit_cast(s16x2, b), acc, false);
}
