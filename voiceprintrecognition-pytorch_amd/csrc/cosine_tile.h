// The value of ONE element of a 16 x 16 tile of x . w^T (optionally a cosine) on the f32 MFMA, as linear_f32_kernel (linear.hip) computes it and
// as the fused cosine + top-k search (search.hip) has to reproduce it bit for bit.  An element's value depends on nothing but its own row of x
// and row of w, through this recipe:
//   * NW waves split K: wave q takes the K blocks of 16 with index == q (mod NW), in ascending order;
//   * per block four v_mfma_f32_16x16x4_f32 (component e = 0 .. 3 of the lanes' float4): lane group g supplies k = 16 b + 4 g + e, zeros
//     behind K -- a k-ordered fmaf chain per element inside each MFMA;
//   * for a cosine every lane (row i, group g) keeps the fmaf chains of the squares of what it loaded, folded over the four groups by two
//     shfl_xor steps (16, then 32).  The chains are spelled fmaf, not `s += x * x`: whether the compiler contracts the latter depends on what
//     the SLP vectoriser made of the loop around it (the U = 8 main loop of the 16-wave kernel had two of its eight blocks as packed multiplies
//     + adds, the four-wave kernel none), and two kernels must agree in every bit;
//   * the wave sums are added in wave order 0 .. NW - 1 from 0.0f, and a cosine is v / (max(|x|, tiny) * max(|w|, tiny)).
// How the operands reach the registers (16-byte loads, guarded loads, fragments kept across tiles) changes no bit.
#pragma once
#include "kernels.h"

namespace mv {

__device__ __forceinline__ float4v load4_guard(const float* row, int k, int K, bool vec_ok) {
    if (vec_ok && k + 3 < K) return *reinterpret_cast<const float4v*>(row + k);
    float4v v;
#pragma unroll
    for (int e = 0; e < 4; ++e) v[e] = (k + e < K) ? row[k + e] : 0.0f;
    return v;
}

// the lanes' float4 of x and of w for the K block that starts at k0 (k = k0 + 4 g of lane group g)
// (the choice between the 16-byte load and the guarded one is made per WAVE: decided per lane, both forms run one after the other under
//  complementary masks into the same registers, and the second waits -- s_waitcnt vmcnt(0) -- for the first: two round trips per block)
__device__ __forceinline__ void tile_load_block(const float* xrow, const float* wrow, int k0, int g, int K, bool vec, float4v& xa, float4v& wb) {
    const int k = k0 + 4 * g;
    if (vec && k0 + 16 <= K) {
        xa = *MV_GLOBAL_PTR(float4v, xrow + k);
        wb = *MV_GLOBAL_PTR(float4v, wrow + k);
    } else {
        xa = load4_guard(xrow, k, K, false);
        wb = load4_guard(wrow, k, K, false);
    }
}

// one K block of 16 of one wave
__device__ __forceinline__ void tile_block_step(const float4v& xa, const float4v& wb, float4v& acc, float& sqx, float& sqw, int cosine) {
#pragma unroll
    for (int e = 0; e < 4; ++e) acc = __builtin_amdgcn_mfma_f32_16x16x4f32(xa[e], wb[e], acc, 0, 0, 0);
    if (cosine) {
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            sqx = __builtin_fmaf(xa[e], xa[e], sqx);
            sqw = __builtin_fmaf(wb[e], wb[e], sqw);
        }
    }
}

// a lane's chain of squares -> the wave's sum for the lane's row (the same value in the four lane groups)
__device__ __forceinline__ float tile_norm_fold(float sq) {
    sq += __shfl_xor(sq, 16);
    sq += __shfl_xor(sq, 32);
    return sq;
}

// element (r, c) of the tile from the waves' accumulators red[wave][r][c] and squared norms nrm[0][wave][r] (x), nrm[1][wave][c] (w)
template <int NW>
__device__ __forceinline__ float tile_finish(const float (*red)[16][17], const float (*nrm)[NW][16], int r, int c, int cosine) {
    float v = 0.0f, sx = 0.0f, sw = 0.0f;
#pragma unroll
    for (int q = 0; q < NW; ++q) {
        v += red[q][r][c];
        sx += nrm[0][q][r];
        sw += nrm[1][q][c];
    }
    if (cosine) {
        const float nx = sqrtf(sx);
        const float nw = sqrtf(sw);
        v = v / (fmaxf(nx, 1.17549435e-38f) * fmaxf(nw, 1.17549435e-38f));
    }
    return v;
}

}  // namespace mv
