// Order-preserving 32-bit images of fp32 values, shared by the radix select of diarize.hip and the radix sort of verif.hip.
#pragma once

#include <cstdint>

namespace mv {

// unsigned key with the order of the floats (-0 and +0 share one key, as they compare equal)
__device__ __forceinline__ uint32_t order_key(float x) {
    uint32_t u = __builtin_bit_cast(uint32_t, x);
    if (u == 0x80000000u) u = 0u;
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}

// order_key with every NaN, of either sign, on the one key above +inf: a sort by this key leaves NaNs last, as numpy does
__device__ __forceinline__ uint32_t sort_key(float x) {
    const uint32_t u = __builtin_bit_cast(uint32_t, x);
    return (u & 0x7FFFFFFFu) > 0x7F800000u ? 0xFFFFFFFFu : order_key(x);
}

// a float with that sort_key: the value itself, but +0 for -0 and the quiet NaN 0x7FFFFFFF for any NaN
__device__ __forceinline__ float sort_key_value(uint32_t key) {
    const uint32_t u = (key & 0x80000000u) ? (key & 0x7FFFFFFFu) : ~key;
    return __builtin_bit_cast(float, u);
}

}  // namespace mv
