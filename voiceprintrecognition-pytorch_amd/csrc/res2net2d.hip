// The three layers of Res2Net (mvector/models/res2net.py) that no other backbone has, on the S16 maps of conv2ds.hip (s16map.h):
//
//   conv2d_stem7_kernel   features fp32 [B, T, F] -> S16 [B, Ho, Wo, C16] = relu(conv7x7(stride 3, zero padding 1) + bias)   (res2net.py:98-100, 157-159)
//   maxpool3s2_kernel     MaxPool2d(3, stride 2, padding 1) behind the stem (res2net.py:101, 160): the (hi, lo) pair of the window's largest value, copied
//   avgpool3_kernel       AvgPool2d(3, stride, padding 1) on the last channel slice of a 'stage' block (res2net.py:35, 75): divisor 9 everywhere
//
// All three are passes in the shape of se2d_gate_kernel: channel-last, a thread owns 8 channels of one output pixel (the hi piece and the lo
// piece of a unit, 16 bytes each), a grid-stride loop with an unconditional store.  Every sum has ONE order, fixed by the window: a row's bits
// depend neither on the batch it sits in nor on the grid.
#include "kernels.h"
#include "s16map.h"

namespace mv {

constexpr int STEM7_K = 7, STEM7_TAPS = 49, STEM7_STRIDE = 3, STEM7_PAD = 1;
constexpr int STEM7_MAX_C = 256;   // 32 groups of 8 maps: the grid's second dimension

static int stem7_out(int n) { return (n + 2 * STEM7_PAD - STEM7_K) / STEM7_STRIDE + 1; }
static int pool3_out(int n, int stride) { return (n - 1) / stride + 1; }   // (n + 2 - 3) / stride + 1

// H = frequency, W = time (as conv2d_first_kernel).  A workgroup works on ONE group of 8 output maps (blockIdx.y), so its 8 x 49 weights are the same
// for every lane: the compiler keeps them in scalar registers (no LDS, no per-lane weight traffic).  Consecutive lanes take consecutive FREQUENCY
// rows of one time step: their taps are 12 bytes apart in the feature rows (coalesced reads).  C is a multiple of 8, so a group is either real or
// the padding of the last unit (C % 16 == 8), which skips the taps and stores relu(0): exact zeros.  acc = bias, then the 49 products in the order
// (df, dt), each one fma.
__global__ __launch_bounds__(256) void conv2d_stem7_kernel(const float* __restrict__ feats, half_t* __restrict__ out, const float* __restrict__ w,
                                                           const float* __restrict__ bias, int B, int T, int F, int C, int C16, int Ho, int Wo,
                                                           unsigned* __restrict__ peak) {
    const int cg = blockIdx.y, c0 = cg * 8;
    const int64_t total = (int64_t)B * Ho * Wo;
    float pk = 0.0f;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
        const int ho = (int)(i % Ho);   // frequency fastest
        const int wo = (int)((i / Ho) % Wo);
        const int b = (int)(i / ((int64_t)Wo * Ho));
        const int64_t pix = ((int64_t)b * Ho + ho) * Wo + wo;
        const float* fb = feats + (int64_t)b * T * F;
        float o[8];
#pragma unroll
        for (int e = 0; e < 8; ++e) o[e] = c0 < C ? bias[c0 + e] : 0.0f;
#pragma unroll 1
        for (int df = 0; df < (c0 < C ? STEM7_K : 0); ++df) {   // (one row of taps at a time: its 8 x 7 weights fit the scalar registers; none for a padding group)
            const int ff = ho * STEM7_STRIDE - STEM7_PAD + df;
            float x[STEM7_K];
#pragma unroll
            for (int dt = 0; dt < STEM7_K; ++dt) {
                const int tt = wo * STEM7_STRIDE - STEM7_PAD + dt;
                x[dt] = (ff >= 0 && ff < F && tt >= 0 && tt < T) ? fb[(int64_t)tt * F + ff] : 0.0f;
            }
#pragma unroll
            for (int e = 0; e < 8; ++e) {
                const float* wr = w + (int64_t)(c0 + e) * STEM7_TAPS + df * STEM7_K;
#pragma unroll
                for (int dt = 0; dt < STEM7_K; ++dt) o[e] = fmaf(wr[dt], x[dt], o[e]);
            }
        }
#pragma unroll
        for (int e = 0; e < 8; ++e) o[e] = fmaxf(o[e], 0.0f);
        half_t* unit = out + (pix * C16 + (cg >> 1) * 16) * 2 + (cg & 1) * 8;
        s16_store4(unit, float4v{o[0], o[1], o[2], o[3]});
        s16_store4(unit + 4, float4v{o[4], o[5], o[6], o[7]});
        pk = s16_peak_of(s16_peak_of(pk, float4v{o[0], o[1], o[2], o[3]}), float4v{o[4], o[5], o[6], o[7]});
    }
    if (peak != nullptr) s16_peak_commit(peak, pk * CS_XSCALE);   // (uniform condition: every lane arrives)
}

int conv2d_stem7_s16_launch(const float* feats, half_t* out, const float* w, const float* bias, int B, int T, int F, int C, hipStream_t stream, unsigned* peak) {
    MV_REQUIRE(feats != nullptr && out != nullptr && w != nullptr && bias != nullptr, "conv2d_stem7: null pointer");
    MV_REQUIRE(B > 0 && T > 0 && F > 0 && C > 0, "conv2d_stem7: sizes must be positive");
    MV_REQUIRE(F >= 5 && T >= 5, "conv2d_stem7: the 7x7 window with padding 1 needs at least 5 bins and 5 frames");
    MV_REQUIRE(C % 8 == 0 && C <= STEM7_MAX_C, "conv2d_stem7: output maps must be a multiple of 8, at most 256");
    MV_REQUIRE((reinterpret_cast<uintptr_t>(out) & 15) == 0, "conv2d_stem7: the map must be 16-byte aligned");
    MV_REQUIRE((int64_t)T * F < ((int64_t)1 << 30), "conv2d_stem7: one utterance's features too large");
    const int C16 = (int)round_up(C, 16), Ho = stem7_out(F), Wo = stem7_out(T);
    const int64_t total = (int64_t)B * Ho * Wo;
    const int grid = (int)(ceil_div(total, 256) < 16384 ? ceil_div(total, 256) : 16384);
    MV_LAUNCH(conv2d_stem7_kernel, (grid, C16 / 8, 1), (256, 1, 1), 0, stream, feats, out, w, bias, B, T, F, C, C16, Ho, Wo, peak);
    return check_launch("conv2d_stem7_kernel");
}

// ---- the two 3x3 windows.  Thread = (output pixel, group cg of 8 channels): hi piece at (cg >> 1) * 32 + (cg & 1) * 8 halves, lo piece 16 behind.
// A tap outside the map is read at the clamped position (always a valid address) and left out of the result.  Taps in the order (dh, dw).
// AVG = false: the largest merged value hi + lo of the window wins and its two halves are copied as they are (the first of equals; a NaN wins and stays).
// AVG = true : the merged values of the taps inside the map summed in fp32, divided by 9 (count_include_pad), split again.
// Channels C .. of the last unit are written as zero bits.
template <bool AVG>
__global__ __launch_bounds__(256) void pool3_kernel(const half_t* x, int64_t ldx, half_t* y, int64_t ldy, int H, int W, int Ho, int Wo, int C, int groups,
                                                    int stride, int64_t total) {
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
        const int64_t pix = i / groups;
        const int cg = (int)(i - pix * groups);
        const int wo = (int)(pix % Wo);
        const int ho = (int)((pix / Wo) % Ho);
        const int64_t b = pix / ((int64_t)Wo * Ho);
        const int off = (cg >> 1) * 32 + (cg & 1) * 8, c = cg * 8;
        const half_t* xb = x + b * H * W * ldx * 2 + off;
        float best[8], acc[8];
        half8v bh, bl;
#pragma unroll
        for (int e = 0; e < 8; ++e) {
            best[e] = -INFINITY;
            acc[e] = 0.0f;
            bh[e] = (half_t)0.0f;
            bl[e] = (half_t)0.0f;
        }
#pragma unroll
        for (int dh = 0; dh < 3; ++dh) {
            const int h = ho * stride - 1 + dh;
            const int hc = h < 0 ? 0 : (h >= H ? H - 1 : h);
#pragma unroll
            for (int dw = 0; dw < 3; ++dw) {
                const int w = wo * stride - 1 + dw;
                const int wc = w < 0 ? 0 : (w >= W ? W - 1 : w);
                const bool inside = h == hc && w == wc;
                const half_t* xp = xb + ((int64_t)hc * W + wc) * ldx * 2;
                const half8v vh = *reinterpret_cast<const half8v*>(xp), vl = *reinterpret_cast<const half8v*>(xp + 16);
#pragma unroll
                for (int e = 0; e < 8; ++e) {
                    const float v = (float)vh[e] + (float)vl[e];
                    if (AVG) {
                        acc[e] += inside ? v : 0.0f;
                    } else {
                        const bool take = inside && (v > best[e] || v != v);
                        best[e] = take ? v : best[e];
                        bh[e] = take ? vh[e] : bh[e];
                        bl[e] = take ? vl[e] : bl[e];
                    }
                }
            }
        }
        half_t* yp = y + pix * ldy * 2 + off;
        if (AVG) {
            float o[8];
#pragma unroll
            for (int e = 0; e < 8; ++e) o[e] = c + e < C ? acc[e] * CS_XSCALE_INV / 9.0f : 0.0f;
            s16_store4(yp, float4v{o[0], o[1], o[2], o[3]});
            s16_store4(yp + 4, float4v{o[4], o[5], o[6], o[7]});
        } else {
#pragma unroll
            for (int e = 0; e < 8; ++e) {
                bh[e] = c + e < C ? bh[e] : (half_t)0.0f;
                bl[e] = c + e < C ? bl[e] : (half_t)0.0f;
            }
            *reinterpret_cast<half8v*>(yp) = bh;
            *reinterpret_cast<half8v*>(yp + 16) = bl;
        }
    }
}

static int pool3_launch(const char* name, bool avg, const half_t* x, int64_t ldx, half_t* y, int64_t ldy, int B, int H, int W, int C, int stride,
                        hipStream_t stream) {
    const std::string n(name);
    MV_REQUIRE(x != nullptr && y != nullptr, n + ": null pointer");
    MV_REQUIRE(B > 0 && H > 0 && W > 0 && C > 0, n + ": sizes must be positive");
    MV_REQUIRE(stride == 1 || stride == 2, n + ": the stride must be 1 or 2");
    MV_REQUIRE(ldx >= C && ldy >= C && ldx % 16 == 0 && ldy % 16 == 0, n + ": every leading dimension must be a multiple of 16, at least C");
    MV_REQUIRE((reinterpret_cast<uintptr_t>(x) & 15) == 0 && (reinterpret_cast<uintptr_t>(y) & 15) == 0, n + ": maps must be 16-byte aligned");
    MV_REQUIRE((int64_t)H * W < ((int64_t)1 << 30), n + ": too many pixels");
    const int Ho = pool3_out(H, stride), Wo = pool3_out(W, stride);
    const int groups = (int)round_up(C, 16) / 8;
    const int64_t total = (int64_t)B * Ho * Wo * groups;
    const int64_t wgs = ceil_div(total, 256);
    const int grid = (int)(wgs < ((int64_t)1 << 20) ? wgs : (int64_t)1 << 20);
    if (avg) {
        MV_LAUNCH(pool3_kernel<true>, ((unsigned)grid, 1, 1), (256, 1, 1), 0, stream, x, ldx, y, ldy, H, W, Ho, Wo, C, groups, stride, total);
    } else {
        MV_LAUNCH(pool3_kernel<false>, ((unsigned)grid, 1, 1), (256, 1, 1), 0, stream, x, ldx, y, ldy, H, W, Ho, Wo, C, groups, stride, total);
    }
    return check_launch(avg ? "avgpool3_kernel" : "maxpool3s2_kernel");
}

int maxpool3s2_s16_launch(const half_t* x, int64_t ldx, half_t* y, int64_t ldy, int B, int H, int W, int C, hipStream_t stream) {
    return pool3_launch("maxpool3s2", false, x, ldx, y, ldy, B, H, W, C, 2, stream);
}

int avgpool3_s16_launch(const half_t* x, int64_t ldx, half_t* y, int64_t ldy, int B, int H, int W, int C, int stride, hipStream_t stream) {
    return pool3_launch("avgpool3", true, x, ldx, y, ldy, B, H, W, C, stride, stream);
}

}  // namespace mv

extern "C" {

int mv_conv2d_stem7_s16(const float* feats, void* out, const float* w, const float* bias, int32_t B, int32_t T, int32_t F, int32_t C, mv_stream_t stream) {
    return mv::conv2d_stem7_s16_launch(feats, static_cast<half_t*>(out), w, bias, B, T, F, C, static_cast<hipStream_t>(stream), nullptr);
}

int mv_conv2d_stem7_peak_s16(const float* feats, void* out, const float* w, const float* bias, int32_t B, int32_t T, int32_t F, int32_t C, uint32_t* peak,
                             mv_stream_t stream) {
    return mv::conv2d_stem7_s16_launch(feats, static_cast<half_t*>(out), w, bias, B, T, F, C, static_cast<hipStream_t>(stream), peak);
}

int mv_maxpool3s2_s16(const void* x, int64_t ldx, void* y, int64_t ldy, int32_t B, int32_t H, int32_t W, int32_t C, mv_stream_t stream) {
    return mv::maxpool3s2_s16_launch(static_cast<const half_t*>(x), ldx, static_cast<half_t*>(y), ldy, B, H, W, C, static_cast<hipStream_t>(stream));
}

int mv_avgpool3_s16(const void* x, int64_t ldx, void* y, int64_t ldy, int32_t B, int32_t H, int32_t W, int32_t C, int32_t stride, mv_stream_t stream) {
    return mv::avgpool3_s16_launch(static_cast<const half_t*>(x), ldx, static_cast<half_t*>(y), ldy, B, H, W, C, stride, static_cast<hipStream_t>(stream));
}

}  // extern "C"
