// The squeeze-and-excitation layer of ResNetSE on S16 maps (s16map.h) and the hand-over from a map to the rows the pooling heads read.
//
//   se2d_squeeze_kernel    s[b, c] = mean over the H x W pixels of a map (AdaptiveAvgPool2d(1)): partial sums of SE2D_CHUNK pixels, then a finish pass
//   se2d_excite_kernel     g = sigmoid(W2 . relu(W1 . s + b1) + b2), fp32 operands summed in fp64, one workgroup per utterance
//   se2d_gate_kernel       y = relu(x * g[b, c] + res) on S16 maps, 8 channels per thread; optionally reports the largest value it wanted to store
//   s16_rows_kernel        S16 [B, H, W, ld] -> fp16 [B, W, ldy] with column c * H + h: x.reshape(B, -1, W) laid out channel-last
//
// Every sum has ONE order, fixed by the shape of a single utterance's map: a row's bits depend neither on the batch it sits in nor on the grid.
#include "kernels.h"
#include "s16map.h"

namespace mv {

constexpr int SE2D_CHUNK = MV_SE2D_SQUEEZE_CHUNK;   // pixels per partial sum: a constant, so the chunking follows (H, W) alone

// A pixel of C16 channels is C16 / 4 pieces of 16 bytes: per unit of 16 channels [hi 0-7 | hi 8-15 | lo 0-7 | lo 8-15].  Thread = (pixel lane, piece):
// consecutive lanes read consecutive pieces.  The sums are carried in fp64 (the addends are fp16 values: the additions are exact or round at 2^-53),
// so the rounding of the result is that of the finished mean to fp32.
__global__ __launch_bounds__(256) void se2d_squeeze_kernel(const half_t* x, int64_t ld, int P, int C16, double* part, int nchunks) {
    __shared__ double red[256][8];
    const int tid = threadIdx.x, b = blockIdx.y, k = blockIdx.x;
    const int npieces = C16 >> 2, lanes = 256 / npieces;
    const int piece = tid % npieces, pl = tid / npieces;
    const int p0 = k * SE2D_CHUNK, p1 = p0 + SE2D_CHUNK < P ? p0 + SE2D_CHUNK : P;
    double acc[8] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    if (pl < lanes) {
        const half_t* xp = x + ((int64_t)b * P * ld) * 2 + piece * 8;
        for (int p = p0 + pl; p < p1; p += lanes) {
            const half8v v = *reinterpret_cast<const half8v*>(xp + (int64_t)p * ld * 2);
#pragma unroll
            for (int e = 0; e < 8; ++e) acc[e] += (double)(float)v[e];
        }
    }
#pragma unroll
    for (int e = 0; e < 8; ++e) red[tid][e] = acc[e];
    __syncthreads();
    for (int c = tid; c < C16; c += 256) {   // hi + lo of channel c over the pixel lanes, lane 0 first
        const int hp = (c >> 4) * 4 + ((c & 15) >> 3), lp = hp + 2, e = c & 7;
        double s = 0.0;
        for (int l = 0; l < lanes; ++l) s += red[l * npieces + hp][e] + red[l * npieces + lp][e];
        part[((int64_t)b * nchunks + k) * C16 + c] = s;
    }
}

__global__ __launch_bounds__(256) void se2d_squeeze_finish_kernel(const double* part, int nchunks, int C16, int C, int P, float* s, int64_t total) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= total) return;
    const int64_t b = i / C;
    const int c = (int)(i - b * C);
    const double* p = part + b * nchunks * C16 + c;
    double sum = 0.0;
    for (int k = 0; k < nchunks; ++k) sum += p[(int64_t)k * C16];
    s[i] = (float)(sum / ((double)CS_XSCALE * (double)P));
}

static int se2d_chunks(int H, int W) { return (int)ceil_div((int64_t)H * W, SE2D_CHUNK); }

size_t se2d_squeeze_ws_floats(int B, int H, int W, int C) {
    if (B <= 0 || H <= 0 || W <= 0 || C <= 0) return 0;
    return (size_t)2 * B * se2d_chunks(H, W) * (size_t)round_up(C, 16);   // doubles
}

int se2d_squeeze_launch(const half_t* x, int64_t ld, int B, int H, int W, int C, float* s, float* ws, size_t ws_floats, hipStream_t stream) {
    MV_REQUIRE(x != nullptr && s != nullptr && ws != nullptr, "se2d_squeeze: null pointer");
    MV_REQUIRE(B > 0 && H > 0 && W > 0 && C > 0, "se2d_squeeze: sizes must be positive");
    MV_REQUIRE(ld >= C && ld % 16 == 0, "se2d_squeeze: the leading dimension must be a multiple of 16, at least C");
    MV_REQUIRE(C <= 1024 && B <= 65535 && (int64_t)H * W < ((int64_t)1 << 30), "se2d_squeeze: at most 1024 channels, 65535 utterances, 2^30 pixels");
    MV_REQUIRE((reinterpret_cast<uintptr_t>(x) & 15) == 0 && (reinterpret_cast<uintptr_t>(ws) & 7) == 0, "se2d_squeeze: map 16-byte, workspace 8-byte aligned");
    MV_REQUIRE(ws_floats >= se2d_squeeze_ws_floats(B, H, W, C), "se2d_squeeze: workspace too small (mv_se2d_squeeze_workspace_floats)");
    const int C16 = (int)round_up(C, 16), nchunks = se2d_chunks(H, W), P = H * W;
    double* part = reinterpret_cast<double*>(ws);
    MV_LAUNCH(se2d_squeeze_kernel, ((unsigned)nchunks, (unsigned)B, 1), (256, 1, 1), 0, stream, x, ld, P, C16, part, nchunks);
    int rc = check_launch("se2d_squeeze_kernel");
    if (rc != MV_OK) return rc;
    const int64_t total = (int64_t)B * C;
    MV_LAUNCH(se2d_squeeze_finish_kernel, ((unsigned)ceil_div(total, 256), 1, 1), (256, 1, 1), 0, stream, part, nchunks, C16, C, P, s, total);
    return check_launch("se2d_squeeze_finish_kernel");
}

// ---- excitation: two small dense layers per utterance.  A dot product is a strided partial sum per lane and a butterfly over the lanes of its
// group (a wave for the C-long sums of layer 1, 16 lanes for the R-long sums of layer 2): one order for every launch.  Operands are fp32; the
// products (exact in fp64) are summed in fp64 and the sigmoid is evaluated there, so the hidden unit and the gate are each rounded to fp32 once.
template <int G>
__device__ __forceinline__ double se2d_dot(const float* w, const float* v, int n, int lane) {
    double a = 0.0;
    for (int i = lane; i < n; i += G) a += (double)w[i] * (double)v[i];
#pragma unroll
    for (int off = G / 2; off >= 1; off >>= 1) a += __shfl_xor(a, off);
    return a;
}

__global__ __launch_bounds__(256) void se2d_excite_kernel(const float* s, const float* w1, const float* b1, const float* w2, const float* b2, float* g,
                                                          int C, int R) {
    MV_DYN_SMEM(smem);
    float* sv = reinterpret_cast<float*>(smem);   // [C] squeeze, then [R] hidden
    float* hv = sv + C;
    const int tid = threadIdx.x, b = blockIdx.x;
    for (int i = tid; i < C; i += 256) sv[i] = s[(int64_t)b * C + i];
    __syncthreads();
    for (int j = tid >> 6; j < R; j += 4) {   // (wave-uniform trip count: every lane of a wave takes part in its butterflies)
        const double z = se2d_dot<64>(w1 + (int64_t)j * C, sv, C, tid & 63) + (double)b1[j];
        if ((tid & 63) == 0) hv[j] = z < 0.0 ? 0.0f : (float)z;
    }
    __syncthreads();
    for (int c0 = 0; c0 < C; c0 += 16) {      // (uniform over the workgroup)
        const int c = c0 + (tid >> 4);
        const double z = se2d_dot<16>(w2 + (int64_t)(c < C ? c : 0) * R, hv, R, tid & 15);
        if (c < C && (tid & 15) == 0) g[(int64_t)b * C + c] = (float)(1.0 / (1.0 + exp(-(z + (double)b2[c]))));
    }
}

int se2d_excite_launch(const float* s, const float* w1, const float* b1, const float* w2, const float* b2, float* g, int B, int C, int R, hipStream_t stream) {
    MV_REQUIRE(s != nullptr && w1 != nullptr && b1 != nullptr && w2 != nullptr && b2 != nullptr && g != nullptr, "se2d_excite: null pointer");
    MV_REQUIRE(B > 0 && C > 0 && R > 0, "se2d_excite: sizes must be positive");
    MV_REQUIRE(C <= 1024 && R <= 1024, "se2d_excite: at most 1024 channels and 1024 hidden units");
    MV_LAUNCH(se2d_excite_kernel, ((unsigned)B, 1, 1), (256, 1, 1), (size_t)(C + R) * sizeof(float), stream, s, w1, b1, w2, b2, g, C, R);
    return check_launch("se2d_excite_kernel");
}

// ---- gate + residual + ReLU: one group of 8 channels (hi piece + lo piece, 16 bytes each) per thread and operand.  Channels >= C of a padded unit
// take the gate 0: with the exact zeros x and res hold there they stay exact zeros.  A NaN travels on (s16map.h).
__global__ __launch_bounds__(256) void se2d_gate_kernel(const half_t* x, int64_t ldx, const float* g, const half_t* res, int64_t ldr, half_t* y,
                                                        int64_t ldy, int P, int C, int groups, int64_t total, unsigned* peak) {
    float pk = 0.0f;
    const bool vec_gate = (C & 7) == 0;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
        const int64_t pix = i / groups;
        const int cg = (int)(i - pix * groups);
        const int b = (int)(pix / P);
        const int off = (cg >> 1) * 32 + (cg & 1) * 8, c = cg * 8;
        const half_t* xp = x + pix * ldx * 2 + off;
        const half_t* rp = res + pix * ldr * 2 + off;
        const half8v xh = *reinterpret_cast<const half8v*>(xp), xl = *reinterpret_cast<const half8v*>(xp + 16);
        const half8v rh = *reinterpret_cast<const half8v*>(rp), rl = *reinterpret_cast<const half8v*>(rp + 16);
        float gv[8];
        const float* gp = g + (int64_t)b * C + c;
        if (vec_gate && c < C) {
            const float4v g0 = *reinterpret_cast<const float4v*>(gp), g1 = *reinterpret_cast<const float4v*>(gp + 4);
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                gv[e] = g0[e];
                gv[4 + e] = g1[e];
            }
        } else {
#pragma unroll
            for (int e = 0; e < 8; ++e) gv[e] = c + e < C ? gp[e] : 0.0f;
        }
        float o[8];
#pragma unroll
        for (int e = 0; e < 8; ++e) {
            const float xv = ((float)xh[e] + (float)xl[e]) * CS_XSCALE_INV, rv = ((float)rh[e] + (float)rl[e]) * CS_XSCALE_INV;
            const float v = xv * gv[e] + rv;
            o[e] = v < 0.0f ? 0.0f : v;
        }
        half_t* yp = y + pix * ldy * 2 + off;
        s16_store4(yp, float4v{o[0], o[1], o[2], o[3]});
        s16_store4(yp + 4, float4v{o[4], o[5], o[6], o[7]});
        pk = s16_peak_of(s16_peak_of(pk, float4v{o[0], o[1], o[2], o[3]}), float4v{o[4], o[5], o[6], o[7]});
    }
    if (peak != nullptr) s16_peak_commit(peak, pk * CS_XSCALE);   // (uniform condition: every lane arrives)
}

int se2d_gate_res_relu_launch(const half_t* x, int64_t ldx, const float* g, const half_t* res, int64_t ldr, half_t* y, int64_t ldy, int B, int H, int W,
                              int C, hipStream_t stream, unsigned* peak) {
    MV_REQUIRE(x != nullptr && g != nullptr && res != nullptr && y != nullptr, "se2d_gate: null pointer");
    MV_REQUIRE(B > 0 && H > 0 && W > 0 && C > 0, "se2d_gate: sizes must be positive");
    MV_REQUIRE(ldx >= C && ldr >= C && ldy >= C && ldx % 16 == 0 && ldr % 16 == 0 && ldy % 16 == 0,
               "se2d_gate: every leading dimension must be a multiple of 16, at least C");
    MV_REQUIRE((reinterpret_cast<uintptr_t>(x) & 15) == 0 && (reinterpret_cast<uintptr_t>(res) & 15) == 0 && (reinterpret_cast<uintptr_t>(y) & 15) == 0 &&
                   (reinterpret_cast<uintptr_t>(g) & 15) == 0,
               "se2d_gate: maps and gates must be 16-byte aligned");
    MV_REQUIRE((int64_t)H * W < ((int64_t)1 << 30), "se2d_gate: too many pixels");
    const int groups = (int)round_up(C, 16) / 8;
    const int64_t total = (int64_t)B * H * W * groups;
    const int64_t wgs = ceil_div(total, 256);
    const int grid = (int)(wgs < ((int64_t)1 << 20) ? wgs : (int64_t)1 << 20);
    MV_LAUNCH(se2d_gate_kernel, ((unsigned)grid, 1, 1), (256, 1, 1), 0, stream, x, ldx, g, res, ldr, y, ldy, H * W, C, groups, total, peak);
    return check_launch("se2d_gate_kernel");
}

// ---- S16 map -> fp16 rows.  A workgroup takes (utterance, time step w, tile of 64 channels): the H x 64 values go through LDS transposed to
// [channel][h], which is a CONTIGUOUS run of the output row (columns c0 * H ...), written 16 bytes per lane.  The last tile adds the zero columns.
constexpr int ROWS_CT = 64;

__global__ __launch_bounds__(256) void s16_rows_kernel(const half_t* x, int64_t ld, int H, int W, int C, half_t* y, int64_t ldy) {
    MV_DYN_SMEM(smem);
    half_t* t = reinterpret_cast<half_t*>(smem);   // [ROWS_CT * H]
    const int tid = threadIdx.x, c0 = blockIdx.x * ROWS_CT, w = blockIdx.y, b = blockIdx.z;
    const int nreal = C - c0 < ROWS_CT ? C - c0 : ROWS_CT;
    const bool last = c0 + ROWS_CT >= C;
    const int ncols = nreal * H;                                         // real columns of this tile
    const int64_t col0 = (int64_t)c0 * H;
    const int span = last ? (int)((((int64_t)C * H + 7) & ~(int64_t)7) - col0) : ncols;   // a multiple of 8 (ROWS_CT * H is one)
    for (int i = tid; i < H * (ROWS_CT / 8); i += 256) {
        const int h = i / (ROWS_CT / 8), cl = (i - h * (ROWS_CT / 8)) * 8;
        if (cl >= nreal) continue;
        const int c = c0 + cl;
        const half_t* xp = x + (((int64_t)b * H + h) * W + w) * ld * 2 + (c >> 4) * 32 + (c & 8);
        const half8v vh = *reinterpret_cast<const half8v*>(xp), vl = *reinterpret_cast<const half8v*>(xp + 16);
#pragma unroll
        for (int e = 0; e < 8; ++e)
            if (cl + e < nreal) t[(cl + e) * H + h] = (half_t)(((float)vh[e] + (float)vl[e]) * CS_XSCALE_INV);
    }
    for (int i = ncols + tid; i < span; i += 256) t[i] = (half_t)0.0f;
    __syncthreads();
    half_t* yr = y + ((int64_t)b * W + w) * ldy;
    for (int i = tid * 8; i < span; i += 256 * 8) {
        half8v v;
#pragma unroll
        for (int e = 0; e < 8; ++e) v[e] = t[i + e];
        *reinterpret_cast<half8v*>(yr + col0 + i) = v;
    }
    if (last) {   // a pitch beyond round_up(C * H, 8): zero groups of 8
        half8v z;
#pragma unroll
        for (int e = 0; e < 8; ++e) z[e] = (half_t)0.0f;
        for (int64_t i = col0 + span + (int64_t)tid * 8; i < ldy; i += 256 * 8) *reinterpret_cast<half8v*>(yr + i) = z;
    }
}

int s16_map_to_rows_launch(const half_t* x, int64_t ld, int B, int H, int W, int C, half_t* y, int64_t ldy, hipStream_t stream) {
    MV_REQUIRE(x != nullptr && y != nullptr, "s16_map_to_rows: null pointer");
    MV_REQUIRE(B > 0 && H > 0 && W > 0 && C > 0, "s16_map_to_rows: sizes must be positive");
    MV_REQUIRE(ld >= C && ld % 16 == 0, "s16_map_to_rows: the leading dimension must be a multiple of 16, at least C");
    MV_REQUIRE(ldy >= (int64_t)C * H && ldy % 8 == 0, "s16_map_to_rows: the row pitch must be a multiple of 8, at least C * H");
    MV_REQUIRE(H <= 256 && W <= 65535 && B <= 65535 && (int64_t)C * H < ((int64_t)1 << 30), "s16_map_to_rows: at most 256 frequency rows, 65535 time steps and utterances");
    MV_REQUIRE((reinterpret_cast<uintptr_t>(x) & 15) == 0 && (reinterpret_cast<uintptr_t>(y) & 15) == 0, "s16_map_to_rows: buffers must be 16-byte aligned");
    MV_LAUNCH(s16_rows_kernel, ((unsigned)ceil_div(C, ROWS_CT), (unsigned)W, (unsigned)B), (256, 1, 1), (size_t)ROWS_CT * H * sizeof(half_t), stream, x, ld, H, W,
              C, y, ldy);
    return check_launch("s16_rows_kernel");
}

}  // namespace mv

extern "C" {

size_t mv_se2d_squeeze_workspace_floats(int32_t B, int32_t H, int32_t W, int32_t C) { return mv::se2d_squeeze_ws_floats(B, H, W, C); }

int mv_se2d_squeeze_s16(const void* x, int64_t ld, int32_t B, int32_t H, int32_t W, int32_t C, float* s, float* workspace, size_t workspace_floats,
                        mv_stream_t stream) {
    return mv::se2d_squeeze_launch(static_cast<const half_t*>(x), ld, B, H, W, C, s, workspace, workspace_floats, static_cast<hipStream_t>(stream));
}

int mv_se2d_excite_f32(const float* s, const float* w1, const float* b1, const float* w2, const float* b2, float* g, int32_t B, int32_t C, int32_t R,
                       mv_stream_t stream) {
    return mv::se2d_excite_launch(s, w1, b1, w2, b2, g, B, C, R, static_cast<hipStream_t>(stream));
}

int mv_se2d_gate_res_relu_s16(const void* x, int64_t ldx, const float* g, const void* res, int64_t ldres, void* y, int64_t ldy, int32_t B, int32_t H,
                              int32_t W, int32_t C, uint32_t* peak, mv_stream_t stream) {
    return mv::se2d_gate_res_relu_launch(static_cast<const half_t*>(x), ldx, g, static_cast<const half_t*>(res), ldres, static_cast<half_t*>(y), ldy, B, H, W,
                                         C, static_cast<hipStream_t>(stream), peak);
}

int mv_s16_map_to_rows_f16(const void* x, int64_t ld, int32_t B, int32_t H, int32_t W, int32_t C, void* y, int64_t ldy, mv_stream_t stream) {
    return mv::s16_map_to_rows_launch(static_cast<const half_t*>(x), ld, B, H, W, C, static_cast<half_t*>(y), ldy, static_cast<hipStream_t>(stream));
}

}  // extern "C"
