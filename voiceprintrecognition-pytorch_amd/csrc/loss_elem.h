// The element types of the loss kernels (marginloss.hip, sphereface2.hip, triplet.hip): fp32, fp16 and bf16 values of a matrix row as floats,
// one at a time or as 16-byte pieces.
#pragma once
#include "kernels.h"

namespace mv {

struct bf16_t {
    uint16_t bits;
};

template <class T>
struct MlElem;
template <>
struct MlElem<float> {
    static __device__ __forceinline__ float ld(const float* p) { return *p; }
    static __device__ __forceinline__ void st(float* p, float v) { *p = v; }
    // n floats at a 16-byte aligned address, n a multiple of 4
    template <int n>
    static __device__ __forceinline__ void ldv(const float* p, float (&e)[n]) {
#pragma unroll
        for (int i = 0; i < n / 4; ++i) {
            const float4v v = *reinterpret_cast<const float4v*>(p + 4 * i);
#pragma unroll
            for (int c = 0; c < 4; ++c) e[4 * i + c] = v[c];
        }
    }
    template <int n>
    static __device__ __forceinline__ void stv(float* p, const float (&e)[n]) {
#pragma unroll
        for (int i = 0; i < n / 4; ++i) *reinterpret_cast<float4v*>(p + 4 * i) = float4v{e[4 * i], e[4 * i + 1], e[4 * i + 2], e[4 * i + 3]};
    }
};
template <>
struct MlElem<half_t> {
    static __device__ __forceinline__ float ld(const half_t* p) { return (float)*p; }
    static __device__ __forceinline__ void st(half_t* p, float v) { *p = (half_t)v; }
    template <int n>
    static __device__ __forceinline__ void ldv(const half_t* p, float (&e)[n]) {
#pragma unroll
        for (int i = 0; i < n / 8; ++i) {
            const half8v v = *reinterpret_cast<const half8v*>(p + 8 * i);
#pragma unroll
            for (int c = 0; c < 8; ++c) e[8 * i + c] = (float)v[c];
        }
    }
    template <int n>
    static __device__ __forceinline__ void stv(half_t* p, const float (&e)[n]) {
#pragma unroll
        for (int i = 0; i < n / 8; ++i) {
            half8v v;
#pragma unroll
            for (int c = 0; c < 8; ++c) v[c] = (half_t)e[8 * i + c];
            *reinterpret_cast<half8v*>(p + 8 * i) = v;
        }
    }
};
__device__ __forceinline__ float bf16_value(uint16_t bits) { return __builtin_bit_cast(float, (uint32_t)bits << 16); }
// round to nearest even; every NaN becomes the quiet NaN 0x7FC0
__device__ __forceinline__ uint16_t bf16_round(float v) {
    const uint32_t u = __builtin_bit_cast(uint32_t, v);
    if (v != v) return (uint16_t)0x7FC0;
    return (uint16_t)((u + 0x7FFFu + ((u >> 16) & 1u)) >> 16);
}
template <>
struct MlElem<bf16_t> {
    static __device__ __forceinline__ float ld(const bf16_t* p) { return bf16_value(p->bits); }
    static __device__ __forceinline__ void st(bf16_t* p, float v) { p->bits = bf16_round(v); }
    template <int n>
    static __device__ __forceinline__ void ldv(const bf16_t* p, float (&e)[n]) {
#pragma unroll
        for (int i = 0; i < n / 8; ++i) {
            const half8v v = *reinterpret_cast<const half8v*>(p + 8 * i);   // eight 16-bit words; never used as fp16 values
#pragma unroll
            for (int c = 0; c < 8; ++c) e[8 * i + c] = bf16_value(__builtin_bit_cast(uint16_t, (half_t)v[c]));
        }
    }
    template <int n>
    static __device__ __forceinline__ void stv(bf16_t* p, const float (&e)[n]) {
#pragma unroll
        for (int i = 0; i < n / 8; ++i) {
            half8v v;
#pragma unroll
            for (int c = 0; c < 8; ++c) v[c] = __builtin_bit_cast(half_t, bf16_round(e[8 * i + c]));
            *reinterpret_cast<half8v*>(p + 8 * i) = v;
        }
    }
};

}  // namespace mv
