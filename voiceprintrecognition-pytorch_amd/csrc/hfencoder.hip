// HuggingFace (Wav2Vec2 / WavLM) front-end: AudioFeaturizer(use_hf_model=True), mvector/data_utils/featurizer.py:20-39,60-76 of the reference, which keeps
// `outputs.extract_features` alone -- the convolutional feature encoder followed by feature_projection.layer_norm (the transformer behind it is never
// evaluated here).  Activations are channel-last fp16 [B, T, C]; statistics and normalisations are fp32 (sums that can cancel: fp64).
//
//   processor   per-row z-score of the waveform, (x - mean) / sqrt(var + 1e-7) over the row's own samples   hf_wave_stats_kernel + on load in layer 0
//   layer 0     1 -> C0, k0 taps, stride s0, exact fp32 on the vector unit (33 MFLOP per second of audio)
//     "group"   GroupNorm(C0, C0): per (utterance, channel) over all frames.  The conv runs TWICE: hf_l0_kernel<STATS> leaves fp64 sums per
//               128-frame chunk, hf_l0_finish_kernel adds the chunks in chunk order, hf_l0_kernel<APPLY> evaluates the conv again, normalises,
//               GELU, stores fp16 -- the largest tensor of the path is written once and never read un-normalised.
//     "layer"   hf_l0_kernel<APPLY> stores conv + bias as fp16, hf_rows_kernel<LN_GELU> normalises the frame in place.
//   layers 1..  valid strided convs through conv1d_launch (stride s, pad 0: the persistent tap kernel on wide layers, the one-shot tiles otherwise),
//               bias in its epilogue; then hf_rows_kernel in place: GELU ("group") or LayerNorm(C) + affine + GELU ("layer").
//   output      hf_rows_kernel<LN_F32>: feature_projection.layer_norm -> fp32 [B, T', C];  hf_cmn_mask_kernel: time mean over all T' frames in the
//               order of cmn_mask_kernel (4 time phases, then their sum) and zeros from round(ratio * T') on.
//
// Every reduction is a function of the row's own length: a wave per frame (LayerNorm), fixed 128-frame chunks added in order (GroupNorm), one
// workgroup per waveform row (z-score), 4 phases (time mean).  Nothing depends on B, the launch form or the stream; the convs are conv1d_launch's,
// whose tile families accumulate in one order.
//
// The row's own length is an ARGUMENT of the four kernels that reduce over it or mask by it: mv_hfenc_forward passes no length array and every row
// holds L samples; mv_hfenc_forward_varlen passes num_samples and row b holds n_b = clamp(num_samples[b], 0, L) -- the same code, the same
// summation orders, so row b comes out bit for bit as the forward gives it alone as a [1, n_b] batch.  The convs are valid (no padding): frame
// t < T_i(n_b) of layer i reads frames < T_{i-1}(n_b) only, whatever lies behind them.  So
//   z-score     over the row's n_b samples (mean 0, sd 1 at n_b = 0);
//   layer 0     T0_b = T_0(n_b) frames: a chunk loads and counts its frames below T0_b only (samples at or behind n_b are never read), the
//               GroupNorm sums run over ceil(T0_b / 128) chunks and divide by T0_b; frames at or behind T0_b are stored as zeros;
//   layers 1..  and hf_rows_kernel run over all T_i(L) frames: behind a row's own count they hold finite filler that no valid frame reads;
//   output      the time mean over T'_b = T'(n_b) frames, zeros (by selection) from T'_b on.  A row below the receptive field is all zero.
#include <vector>

#include "kernels.h"
#include "model.h"

namespace mv {

constexpr int HF_THREADS = 256;
constexpr int HF_L0_FR = 128;     // frames of layer 0 per workgroup: the chunk of the GroupNorm sums
constexpr int HF_L0_MAX_S = 8;    // largest stride of layer 0
constexpr int HF_L0_MAX_K = 16;   // largest kernel of layer 0
constexpr int HF_MAX_C = 1024;    // widest frame a wave holds in registers (16 per lane)
constexpr float HF_ENC_EPS = 1e-5f;   // GroupNorm / LayerNorm of the feature encoder (nn defaults)

// frames behind one valid (unpadded) strided conv: n -> floor((n - k) / s) + 1, 0 as soon as no whole window fits
__host__ __device__ __forceinline__ int64_t hf_conv_frames(int64_t n, int k, int s) { return n >= k ? (n - k) / s + 1 : 0; }

// kernels and strides of the layers, by value into the kernels that need a row's frame count behind several layers
struct HfGeom {
    int n;
    int k[MV_HFENC_MAX_LAYERS], s[MV_HFENC_MAX_LAYERS];
};

__host__ __device__ __forceinline__ int64_t hf_frames_behind(const HfGeom& g, int64_t samples) {
    for (int i = 0; i < g.n; ++i) samples = hf_conv_frames(samples, g.k[i], g.s[i]);
    return samples;
}

// valid samples of row b: all L (no length array: the fixed-length forward) or clamp(num_samples[b], 0, L)
__device__ __forceinline__ int64_t hf_row_len(const int64_t* num_samples, int b, int64_t L) {
    if (num_samples == nullptr) return L;
    const int64_t n = num_samples[b];
    return n < 0 ? 0 : (n > L ? L : n);
}

__device__ __forceinline__ float hf_gelu(float v) { return 0.5f * v * (1.0f + erff(v * 0.70710678118654752440f)); }

__device__ __forceinline__ float wave_sum(float v) {
    for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off);
    return v;
}

// sum of one double per thread over the workgroup, in a fixed tree; every thread returns the total
__device__ __forceinline__ double block_sum_f64(double v, double* red) {
    const int tid = threadIdx.x;
    __syncthreads();
    red[tid] = v;
    __syncthreads();
    for (int n = HF_THREADS / 2; n > 0; n >>= 1) {
        if (tid < n) red[tid] += red[tid + n];
        __syncthreads();
    }
    return red[0];
}

// mean and sqrt(var + 1e-7) (biased variance) of every waveform row over its own n samples: Wav2Vec2FeatureExtractor.zero_mean_unit_var_norm.
// One workgroup per row.  n = 0: mean 0, sd 1 (nothing is loaded with them).
__global__ __launch_bounds__(HF_THREADS) void hf_wave_stats_kernel(const float* wav, int64_t L, int64_t stride, const int64_t* num_samples,
                                                                   float* stats) {
    __shared__ double red[HF_THREADS];
    const float* row = wav + (int64_t)blockIdx.x * stride;
    const int64_t n = hf_row_len(num_samples, blockIdx.x, L);
    if (n == 0) {   // (uniform per workgroup)
        if (threadIdx.x == 0) {
            stats[2 * blockIdx.x] = 0.0f;
            stats[2 * blockIdx.x + 1] = 1.0f;
        }
        return;
    }
    double s = 0.0;
    for (int64_t i = threadIdx.x; i < n; i += HF_THREADS) s += (double)row[i];
    const double mean = block_sum_f64(s, red) / (double)n;
    double q = 0.0;
    for (int64_t i = threadIdx.x; i < n; i += HF_THREADS) {
        const double d = (double)row[i] - mean;
        q += d * d;
    }
    const double var = block_sum_f64(q, red) / (double)n;
    if (threadIdx.x == 0) {
        stats[2 * blockIdx.x] = (float)mean;
        stats[2 * blockIdx.x + 1] = sqrtf((float)var + 1e-7f);
    }
}

struct HfL0Args {
    const float* wav;      // [B, L] rows wav_stride apart
    int64_t L, wav_stride;
    const int64_t* num_samples;   // [B] valid samples of every row (variable-length form) or null: L
    const float* wstats;   // [B][2] mean, std of the row (do_normalize) or null
    const float* w;        // [C][k] fp32
    const float* bias;     // [C] or null
    const float* gamma;    // GroupNorm affine ("group") or null
    const float* beta;
    float* cstats;         // [B][C][2] mean, rstd ("group": written by hf_l0_finish_kernel, read by APPLY)
    double* partial;       // [B][nchunk][C][2] sum, sum of squares (STATS)
    half_t* y;             // [B, T1, C]
    int T1, C, k, s, nchunk;
};

// One workgroup = one 128-frame chunk of one utterance, every channel: the chunk's samples (z-scored on load) sit in LDS, a thread keeps its
// channel's taps in registers and walks the frames.  STATS: fp64 sum / sum of squares of the chunk per channel.  APPLY: GroupNorm + GELU (gamma
// given) or the bare conv + bias, stored fp16 -- consecutive threads store consecutive channels of a frame.  The chunk holds its frames below the
// row's own T0_b = T_0(n_b): STATS counts those alone (a chunk behind them leaves, its sums are never read), APPLY stores zeros from T0_b on
// and skips the convolution where the whole chunk lies behind it.  Every branch on T0_b is uniform per workgroup.
template <bool STATS, int KT>
__global__ __launch_bounds__(HF_THREADS) void hf_l0_kernel(HfL0Args a) {
    __shared__ float xs[HF_L0_FR * HF_L0_MAX_S + HF_L0_MAX_K];
    const int tid = threadIdx.x, chunk = blockIdx.x, b = blockIdx.y;
    const int t0 = chunk * HF_L0_FR;
    const int nslot = a.T1 - t0 < HF_L0_FR ? a.T1 - t0 : HF_L0_FR;     // frames of the chunk in the padded row
    const int T0b = (int)hf_conv_frames(hf_row_len(a.num_samples, b, a.L), a.k, a.s);
    const int nf = T0b - t0 < nslot ? T0b - t0 : nslot;          // ... of which the row's own (<= 0: the chunk lies behind them)
    if (nf <= 0) {
        if constexpr (!STATS) {
            half_t* y = a.y + ((int64_t)b * a.T1 + t0) * a.C;
            for (int i = tid; i < nslot * a.C; i += HF_THREADS) y[i] = (half_t)0.0f;
        }
        return;
    }
    const int ns = (nf - 1) * a.s + a.k;                       // samples of the chunk (inside the row's own: t0 + nf <= T0_b)
    const float* row = a.wav + (int64_t)b * a.wav_stride + (int64_t)t0 * a.s;
    float mean = 0.0f, sd = 1.0f;
    if (a.wstats != nullptr) {
        mean = a.wstats[2 * b];
        sd = a.wstats[2 * b + 1];
    }
    for (int i = tid; i < HF_L0_FR * HF_L0_MAX_S + HF_L0_MAX_K; i += HF_THREADS) xs[i] = i < ns ? (row[i] - mean) / sd : 0.0f;
    __syncthreads();
    for (int c = tid; c < a.C; c += HF_THREADS) {
        float w[KT];
#pragma unroll
        for (int j = 0; j < KT; ++j) w[j] = j < a.k ? a.w[c * a.k + j] : 0.0f;   // (taps beyond k: exact zeros on the zero-filled tail of xs)
        const float bias = a.bias != nullptr ? a.bias[c] : 0.0f;
        if constexpr (STATS) {
            double s = 0.0, q = 0.0;
            for (int f = 0; f < nf; ++f) {
                float v = bias;
#pragma unroll
                for (int j = 0; j < KT; ++j) v = fmaf(w[j], xs[f * a.s + j], v);
                s += (double)v;
                q += (double)v * (double)v;
            }
            double* p = a.partial + (((int64_t)b * a.nchunk + chunk) * a.C + c) * 2;
            p[0] = s;
            p[1] = q;
        } else {
            float m = 0.0f, r = 1.0f, g = 1.0f, be = 0.0f;
            const bool norm = a.gamma != nullptr;
            if (norm) {
                m = a.cstats[((int64_t)b * a.C + c) * 2];
                r = a.cstats[((int64_t)b * a.C + c) * 2 + 1];
                g = a.gamma[c];
                be = a.beta[c];
            }
            half_t* y = a.y + ((int64_t)b * a.T1 + t0) * a.C + c;
            for (int f = 0; f < nf; ++f) {
                float v = bias;
#pragma unroll
                for (int j = 0; j < KT; ++j) v = fmaf(w[j], xs[f * a.s + j], v);
                if (norm) v = hf_gelu((v - m) * r * g + be);
                y[(int64_t)f * a.C] = (half_t)v;
            }
            for (int f = nf; f < nslot; ++f) y[(int64_t)f * a.C] = (half_t)0.0f;
        }
    }
}

// GroupNorm statistics of layer 0: the fp64 sums of the row's own ceil(T0_b / 128) chunks added in chunk order -> mean, 1 / sqrt(biased var + eps)
// per (utterance, channel) over its T0_b frames.  T0_b = 0: mean 0, rstd 1 (no frame is normalised with them).
__global__ void hf_l0_finish_kernel(const double* partial, int B, int nchunk, int C, const int64_t* num_samples, int64_t L, int k0, int s0, float eps,
                                    float* cstats) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= (int64_t)B * C) return;
    const int b = (int)(i / C), c = (int)(i - (int64_t)b * C);
    const int T1 = (int)hf_conv_frames(hf_row_len(num_samples, b, L), k0, s0);
    if (T1 == 0) {
        cstats[2 * i] = 0.0f;
        cstats[2 * i + 1] = 1.0f;
        return;
    }
    const int own = (T1 + HF_L0_FR - 1) / HF_L0_FR;
    double s = 0.0, q = 0.0;
    for (int ch = 0; ch < own; ++ch) {
        const double* p = partial + (((int64_t)b * nchunk + ch) * C + c) * 2;
        s += p[0];
        q += p[1];
    }
    const double mean = s / (double)T1;
    double var = q / (double)T1 - mean * mean;
    if (var < 0.0) var = 0.0;
    cstats[2 * i] = (float)mean;
    cstats[2 * i + 1] = (float)(1.0 / sqrt(var + (double)eps));
}

enum { HF_ROWS_GELU = MV_HF_ROWS_GELU, HF_ROWS_LN_GELU = MV_HF_ROWS_LN_GELU, HF_ROWS_LN_F32 = MV_HF_ROWS_LN_F32 };

// One wave per frame of a channel-last fp16 tensor, C <= 1024 values in registers.  GELU: elementwise, in place.  LN_GELU: LayerNorm over the C
// channels (two passes over the registers, biased variance) + affine + GELU, fp16 out.  LN_F32: LayerNorm + affine, fp32 out (the features).
// PER8: C == 512, a lane holds 8 consecutive channels (one 16-byte load); otherwise channel j * 64 + lane.  A width always takes the same form.
template <int MODE, bool PER8>
__global__ __launch_bounds__(HF_THREADS) void hf_rows_kernel(const half_t* x, void* yv, const float* gamma, const float* beta, float eps,
                                                             int64_t n_rows, int C) {
    const int lane = threadIdx.x & 63;
    const int64_t r = (int64_t)blockIdx.x * (HF_THREADS / 64) + (threadIdx.x >> 6);
    if (r >= n_rows) return;   // (whole waves leave: no barrier below)
    constexpr int N = PER8 ? 8 : HF_MAX_C / 64;
    const int per = C / 64;
    const half_t* xr = x + r * C;
    float v[N];
    if constexpr (PER8) {
        const half8v h = *reinterpret_cast<const half8v*>(xr + lane * 8);
#pragma unroll
        for (int j = 0; j < 8; ++j) v[j] = (float)h[j];
    } else {
#pragma unroll
        for (int j = 0; j < N; ++j) v[j] = j < per ? (float)xr[j * 64 + lane] : 0.0f;
    }
    if constexpr (MODE != HF_ROWS_GELU) {
        float s = 0.0f;
#pragma unroll
        for (int j = 0; j < N; ++j) s += v[j];
        const float mean = wave_sum(s) / (float)C;
        float q = 0.0f;
#pragma unroll
        for (int j = 0; j < N; ++j) {
            const float d = (PER8 || j < per) ? v[j] - mean : 0.0f;
            q += d * d;
        }
        const float rstd = 1.0f / sqrtf(wave_sum(q) / (float)C + eps);
#pragma unroll
        for (int j = 0; j < N; ++j) {
            const int c = PER8 ? lane * 8 + j : j * 64 + lane;
            if (PER8 || j < per) v[j] = (v[j] - mean) * rstd * gamma[c] + beta[c];
        }
    }
    if constexpr (MODE == HF_ROWS_LN_F32) {
        float* yr = reinterpret_cast<float*>(yv) + r * C;
        if constexpr (PER8) {
            float4v o0 = {v[0], v[1], v[2], v[3]}, o1 = {v[4], v[5], v[6], v[7]};
            *reinterpret_cast<float4v*>(yr + lane * 8) = o0;
            *reinterpret_cast<float4v*>(yr + lane * 8 + 4) = o1;
        } else {
#pragma unroll
            for (int j = 0; j < N; ++j)
                if (j < per) yr[j * 64 + lane] = v[j];
        }
    } else {
        half_t* yr = reinterpret_cast<half_t*>(yv) + r * C;
        if constexpr (PER8) {
            half8v o;
#pragma unroll
            for (int j = 0; j < 8; ++j) o[j] = (half_t)hf_gelu(v[j]);
            *reinterpret_cast<half8v*>(yr + lane * 8) = o;
        } else {
#pragma unroll
            for (int j = 0; j < N; ++j)
                if (j < per) yr[j * 64 + lane] = (half_t)hf_gelu(v[j]);
        }
    }
}

// AudioFeaturizer.forward behind the model (featurizer.py:79-90): minus the mean over ALL frames of the row, then zeros from round(ratio * T) on
// -- the semantics and the summation order of the other front-ends' cmn_mask_kernel (4 time phases, then their sum).  The row's frames are all T
// (no length array) or Tb = T'(n_b) of its own samples: the mean runs over and divides by Tb, frames from Tb on are zeros (selected, never
// multiplied: what lies there is filler), Tb = 0 is an all-zero row.  Workgroup = (utterance, 64 channels).
__global__ __launch_bounds__(HF_THREADS) void hf_cmn_mask_kernel(float* out, const float* lens_ratio, const int64_t* num_samples, int64_t L, HfGeom g,
                                                                 int T, int C, int cmn) {
    __shared__ float part[4][64];
    const int b = blockIdx.x, c = blockIdx.y * 64 + (threadIdx.x & 63), ph = threadIdx.x >> 6;
    const int Tb = num_samples != nullptr ? (int)hf_frames_behind(g, hf_row_len(num_samples, b, L)) : T;
    float* o = out + (int64_t)b * T * C + c;
    float s = 0.0f;
    if (cmn)
        for (int t = ph; t < Tb; t += 4) s += o[(int64_t)t * C];
    part[ph][threadIdx.x & 63] = s;
    __syncthreads();
    const int l = threadIdx.x & 63;
    const float mean = cmn && Tb > 0 ? (part[0][l] + part[1][l] + part[2][l] + part[3][l]) / (float)Tb : 0.0f;
    int mask_len = Tb;
    if (lens_ratio != nullptr) mask_len = (int)rintf(lens_ratio[b] * (float)T);
    for (int t = ph; t < T; t += 4) o[(int64_t)t * C] = t < mask_len ? o[(int64_t)t * C] - mean : 0.0f;
}

template <int MODE>
static int hf_rows_launch(const half_t* x, void* y, const float* gamma, const float* beta, float eps, int64_t n_rows, int C, hipStream_t stream) {
    const int64_t grid = ceil_div(n_rows, HF_THREADS / 64);
    MV_REQUIRE(grid < ((int64_t)1 << 31), "mv_hfenc_forward: too many frames for one launch");
    if (C == 512)
        MV_LAUNCH((hf_rows_kernel<MODE, true>), ((unsigned)grid, 1, 1), (HF_THREADS, 1, 1), 0, stream, x, y, gamma, beta, eps, n_rows, C);
    else
        MV_LAUNCH((hf_rows_kernel<MODE, false>), ((unsigned)grid, 1, 1), (HF_THREADS, 1, 1), 0, stream, x, y, gamma, beta, eps, n_rows, C);
    return check_launch("hf_rows_kernel");
}

static int hf_wave_stats_launch(const float* wav, int B, int64_t L, int64_t wav_stride, const int64_t* num_samples, float* stats, hipStream_t stream) {
    MV_LAUNCH(hf_wave_stats_kernel, (B, 1, 1), (HF_THREADS, 1, 1), 0, stream, wav, L, wav_stride, num_samples, stats);
    return check_launch("hf_wave_stats_kernel");
}

template <bool STATS>
static void hf_l0_launch(const HfL0Args& a, int B, hipStream_t stream) {
    if (a.k <= 10)
        MV_LAUNCH((hf_l0_kernel<STATS, 10>), (a.nchunk, B, 1), (HF_THREADS, 1, 1), 0, stream, a);
    else
        MV_LAUNCH((hf_l0_kernel<STATS, HF_L0_MAX_K>), (a.nchunk, B, 1), (HF_THREADS, 1, 1), 0, stream, a);
}

// layer 0 of B rows.  gamma given ("group"): STATS into a.partial, the chunk sums into a.cstats, APPLY with GroupNorm + GELU; otherwise
// ("layer", before its row pass) APPLY alone stores conv + bias.
static int hf_layer0_launch(const HfL0Args& a, int B, hipStream_t stream) {
    int rc;
    if (a.gamma != nullptr) {
        hf_l0_launch<true>(a, B, stream);
        if ((rc = check_launch("hf_l0_kernel<STATS>"))) return rc;
        const int64_t bc = (int64_t)B * a.C;
        MV_LAUNCH(hf_l0_finish_kernel, ((unsigned)ceil_div(bc, HF_THREADS), 1, 1), (HF_THREADS, 1, 1), 0, stream, (const double*)a.partial, B, a.nchunk,
                  a.C, a.num_samples, a.L, a.k, a.s, HF_ENC_EPS, a.cstats);
        if ((rc = check_launch("hf_l0_finish_kernel"))) return rc;
    }
    hf_l0_launch<false>(a, B, stream);
    return check_launch("hf_l0_kernel<APPLY>");
}

static int hf_cmn_mask_launch(float* out, const float* lens_ratio, const int64_t* num_samples, int64_t L, const HfGeom& g, int B, int T, int C, int cmn,
                              hipStream_t stream) {
    MV_LAUNCH(hf_cmn_mask_kernel, (B, C / 64, 1), (HF_THREADS, 1, 1), 0, stream, out, lens_ratio, num_samples, L, g, T, C, cmn);
    return check_launch("hf_cmn_mask_kernel");
}

// the width rule of mv_hfenc_create, for the layer-level entry points
static int hf_check_width(const char* who, int C) {
    if (C < 64 || C > HF_MAX_C || C % 64 != 0)
        return fail(MV_ERR_UNSUPPORTED, std::string(who) + ": C = " + std::to_string(C) + ": the kernels are built for widths that are multiples of 64 up to 1024");
    return MV_OK;
}

}  // namespace mv

struct MvHfEncoder {
    MvHfEncoderCfg cfg;
    std::vector<void*> owned;
    float* w0 = nullptr;                            // layer 0: [C0][k0] fp32
    float* bias[MV_HFENC_MAX_LAYERS] = {};          // conv bias (conv_bias) or null
    float* ln_w[MV_HFENC_MAX_LAYERS] = {};          // conv_layers.i.layer_norm (layer 0 in "group" mode, every layer in "layer" mode)
    float* ln_b[MV_HFENC_MAX_LAYERS] = {};
    half_t* w[MV_HFENC_MAX_LAYERS] = {};       // layers 1..: packed fp16 [Cout][k][Cin]
    float* proj_w = nullptr;                        // feature_projection.layer_norm
    float* proj_b = nullptr;
    ~MvHfEncoder() {
        for (void* p : owned) hipFree(p);
    }
};

namespace {

using namespace mv;

// frames behind every layer (hf_conv_frames, the device's own count), 0 as soon as a layer has no whole window
void hf_frames(const MvHfEncoderCfg& c, int64_t L, int64_t* T) {
    int64_t n = L;
    for (int i = 0; i < c.num_layers; ++i) {
        n = hf_conv_frames(n, c.conv_kernel[i], c.conv_stride[i]);
        T[i] = n;
    }
}

int64_t hf_receptive_field(const MvHfEncoderCfg& c) {
    int64_t n = 1;
    for (int i = c.num_layers - 1; i >= 0; --i) n = (n - 1) * c.conv_stride[i] + c.conv_kernel[i];
    return n;
}

struct HfScratch {
    float* wstats;
    double* partial;
    float* cstats;
    half_t* buf[2];
    size_t bytes;
};

HfScratch hf_carve(const MvHfEncoderCfg& c, int B, const int64_t* T, void* ws) {
    Carver cv(ws);
    HfScratch s;
    const int64_t nchunk = ceil_div(T[0], HF_L0_FR);
    s.wstats = cv.take<float>((size_t)B * 2);
    s.partial = cv.take<double>(c.feat_extract_norm == MV_HF_NORM_GROUP ? (size_t)B * nchunk * c.conv_dim[0] * 2 : 0);
    s.cstats = cv.take<float>((size_t)B * c.conv_dim[0] * 2);
    size_t n[2] = {0, 0};
    for (int i = 0; i < c.num_layers; ++i) {
        const size_t e = (size_t)B * (size_t)T[i] * c.conv_dim[i];
        if (e > n[i & 1]) n[i & 1] = e;
    }
    s.buf[0] = cv.take<half_t>(n[0]);
    s.buf[1] = cv.take<half_t>(n[1]);
    s.bytes = cv.total();
    return s;
}

int hf_copy_vec(MvHfEncoder* h, const Weights& w, const std::string& name, int64_t numel, float** out) {
    const float* d = nullptr;
    int rc = w.dev(name, numel, &d);
    if (rc != MV_OK) return rc;
    void* p = nullptr;
    MV_HIP_OK(hipMalloc(&p, (size_t)numel * sizeof(float)));
    h->owned.push_back(p);
    MV_HIP_OK(hipMemcpy(p, d, (size_t)numel * sizeof(float), hipMemcpyDeviceToDevice));
    *out = static_cast<float*>(p);
    return MV_OK;
}

int hf_create(const MvHfEncoderCfg* cfg, const MvTensorRef* tensors, int32_t n, MvHfEncoder* h) {
    const MvHfEncoderCfg& c = *cfg;
    MV_REQUIRE(c.num_layers >= 1 && c.num_layers <= MV_HFENC_MAX_LAYERS, "mv_hfenc_create: num_layers must be 1 .. MV_HFENC_MAX_LAYERS (8)");
    if (c.activation != MV_ACT_GELU)
        return fail(MV_ERR_UNSUPPORTED, "mv_hfenc_create: feat_extract_activation must be gelu (MV_ACT_GELU); code " + std::to_string(c.activation) + " is not built");
    MV_REQUIRE(c.feat_extract_norm == MV_HF_NORM_GROUP || c.feat_extract_norm == MV_HF_NORM_LAYER,
               "mv_hfenc_create: feat_extract_norm must be MV_HF_NORM_GROUP or MV_HF_NORM_LAYER");
    MV_REQUIRE(c.layer_norm_eps > 0.0f, "mv_hfenc_create: layer_norm_eps must be positive");
    for (int i = 0; i < c.num_layers; ++i) {
        if (c.conv_dim[i] < 64 || c.conv_dim[i] > HF_MAX_C || c.conv_dim[i] % 64 != 0)
            return fail(MV_ERR_UNSUPPORTED, "mv_hfenc_create: conv_dim[" + std::to_string(i) + "] = " + std::to_string(c.conv_dim[i]) +
                                                ": the kernels are built for widths that are multiples of 64 up to 1024");
        MV_REQUIRE(c.conv_kernel[i] >= 1 && c.conv_stride[i] >= 1, "mv_hfenc_create: conv_kernel / conv_stride must be positive");
        MV_REQUIRE(c.conv_kernel[i] <= 64 && c.conv_stride[i] <= 64, "mv_hfenc_create: conv_kernel / conv_stride above 64");
    }
    if (c.conv_kernel[0] > HF_L0_MAX_K || c.conv_stride[0] > HF_L0_MAX_S)
        return fail(MV_ERR_UNSUPPORTED, "mv_hfenc_create: layer 0 is built for conv_kernel[0] <= 16 and conv_stride[0] <= 8");
    h->cfg = c;
    Weights w;
    int rc = w.init(tensors, n);
    if (rc != MV_OK) return rc;
    const std::string fe = "feature_extractor.conv_layers.";
    if ((rc = hf_copy_vec(h, w, fe + "0.conv.weight", (int64_t)c.conv_dim[0] * c.conv_kernel[0], &h->w0))) return rc;
    for (int i = 0; i < c.num_layers; ++i) {
        const std::string p = fe + std::to_string(i);
        if (c.conv_bias && (rc = hf_copy_vec(h, w, p + ".conv.bias", c.conv_dim[i], &h->bias[i]))) return rc;
        if (c.feat_extract_norm == MV_HF_NORM_LAYER || i == 0) {
            if ((rc = hf_copy_vec(h, w, p + ".layer_norm.weight", c.conv_dim[i], &h->ln_w[i]))) return rc;
            if ((rc = hf_copy_vec(h, w, p + ".layer_norm.bias", c.conv_dim[i], &h->ln_b[i]))) return rc;
        }
        if (i == 0) continue;
        const float* dw = nullptr;
        if ((rc = w.dev(p + ".conv.weight", (int64_t)c.conv_dim[i] * c.conv_dim[i - 1] * c.conv_kernel[i], &dw))) return rc;
        void* pk = nullptr;
        MV_HIP_OK(hipMalloc(&pk, (size_t)mv_conv1d_packed_elems(c.conv_dim[i], c.conv_dim[i - 1], c.conv_kernel[i]) * sizeof(half_t)));
        h->owned.push_back(pk);
        h->w[i] = static_cast<half_t*>(pk);
        if ((rc = mv_conv1d_pack_weight(dw, c.conv_dim[i], c.conv_dim[i - 1], c.conv_kernel[i], pk, nullptr))) return rc;
    }
    const int CL = c.conv_dim[c.num_layers - 1];
    if ((rc = hf_copy_vec(h, w, "feature_projection.layer_norm.weight", CL, &h->proj_w))) return rc;
    if ((rc = hf_copy_vec(h, w, "feature_projection.layer_norm.bias", CL, &h->proj_b))) return rc;
    MV_HIP_OK(hipDeviceSynchronize());
    return MV_OK;
}

}  // namespace

extern "C" {

void mv_hfenc_default_cfg(MvHfEncoderCfg* cfg) {
    static const int32_t k[7] = {10, 3, 3, 3, 3, 2, 2}, s[7] = {5, 2, 2, 2, 2, 2, 2};
    memset(cfg, 0, sizeof(*cfg));
    cfg->num_layers = 7;
    for (int i = 0; i < 7; ++i) {
        cfg->conv_dim[i] = 512;
        cfg->conv_kernel[i] = k[i];
        cfg->conv_stride[i] = s[i];
    }
    cfg->feat_extract_norm = MV_HF_NORM_GROUP;
    cfg->conv_bias = 0;
    cfg->do_normalize = 1;
    cfg->activation = MV_ACT_GELU;
    cfg->layer_norm_eps = 1e-5f;
    cfg->subtract_time_mean = 1;
}

int mv_hfenc_create(const MvHfEncoderCfg* cfg, const MvTensorRef* tensors, int32_t num_tensors, MvHfEncoder** out) {
    MV_REQUIRE(cfg != nullptr && out != nullptr, "mv_hfenc_create: null argument");
    MvHfEncoder* h = new MvHfEncoder();
    const int rc = hf_create(cfg, tensors, num_tensors, h);
    if (rc != MV_OK) {
        delete h;
        return rc;
    }
    *out = h;
    return MV_OK;
}

int mv_hfenc_destroy(MvHfEncoder* h) {
    delete h;
    return MV_OK;
}

int mv_hfenc_num_frames(const MvHfEncoder* h, int64_t num_samples, int64_t* num_frames) {
    MV_REQUIRE(h != nullptr && num_frames != nullptr, "mv_hfenc_num_frames: null argument");
    int64_t T[MV_HFENC_MAX_LAYERS];
    hf_frames(h->cfg, num_samples, T);
    *num_frames = T[h->cfg.num_layers - 1];
    return MV_OK;
}

int mv_hfenc_workspace_bytes(const MvHfEncoder* h, int32_t B, int64_t L, size_t* bytes) {
    MV_REQUIRE(h != nullptr && bytes != nullptr, "mv_hfenc_workspace_bytes: null argument");
    MV_REQUIRE(B >= 0 && L >= 0, "mv_hfenc_workspace_bytes: negative size");
    int64_t T[MV_HFENC_MAX_LAYERS];
    hf_frames(h->cfg, L, T);
    *bytes = B == 0 || T[h->cfg.num_layers - 1] <= 0 ? 0 : hf_carve(h->cfg, B, T, nullptr).bytes;
    return MV_OK;
}

}  // extern "C"

namespace {

// The forward of both forms: lens_ratio (batch form, or neither) or num_samples (variable-length form: a device array the kernels read), never both.
// ev (optional, num_layers + 2 events): recorded in front of layer 0 (the z-score counts as layer 0's), behind every layer and behind the tail
int hf_forward(const MvHfEncoder* h, const float* wav, int32_t B, int64_t L, int64_t wav_stride, const float* lens_ratio, const int64_t* num_samples,
               float* out, void* workspace, size_t workspace_bytes, mv_stream_t stream_, hipEvent_t* ev) {
    MV_REQUIRE(h != nullptr && wav != nullptr && out != nullptr, "mv_hfenc_forward: null argument");
    MV_REQUIRE((reinterpret_cast<uintptr_t>(out) & 15) == 0, "mv_hfenc_forward: out must be 16-byte aligned");
    MV_REQUIRE(B > 0 && B <= 65535, "mv_hfenc_forward: batch size must be 1 .. 65535");
    MV_REQUIRE(wav_stride >= L, "mv_hfenc_forward: wav_stride below the row length");
    const MvHfEncoderCfg& c = h->cfg;
    const int n = c.num_layers;
    int64_t T[MV_HFENC_MAX_LAYERS];
    hf_frames(c, L, T);
    if (T[n - 1] <= 0)
        return fail(MV_ERR_INVALID_ARGUMENT, "mv_hfenc_forward: a waveform of " + std::to_string(L) + " samples is shorter than the encoder's receptive field of " +
                                                 std::to_string(hf_receptive_field(c)) + " samples: no frame");
    MV_REQUIRE((int64_t)B * T[0] < ((int64_t)1 << 31) - 512, "mv_hfenc_forward: too many frames for 32-bit row indexing");
    const HfScratch s = hf_carve(c, B, T, workspace);
    if (workspace == nullptr || workspace_bytes < s.bytes || (reinterpret_cast<uintptr_t>(workspace) & 15) != 0)
        return fail(MV_ERR_WORKSPACE, "mv_hfenc_forward: workspace of " + std::to_string(s.bytes) + " bytes (16-byte aligned) required");
    hipStream_t stream = static_cast<hipStream_t>(stream_);
    int rc;
    const bool group = c.feat_extract_norm == MV_HF_NORM_GROUP;

    if (ev != nullptr) MV_HIP_OK(hipEventRecord(ev[0], stream));
    if (c.do_normalize && (rc = hf_wave_stats_launch(wav, B, L, wav_stride, num_samples, s.wstats, stream))) return rc;
    HfL0Args a = {};
    a.wav = wav;
    a.L = L;
    a.wav_stride = wav_stride;
    a.num_samples = num_samples;
    a.wstats = c.do_normalize ? s.wstats : nullptr;
    a.w = h->w0;
    a.bias = h->bias[0];
    a.gamma = group ? h->ln_w[0] : nullptr;
    a.beta = group ? h->ln_b[0] : nullptr;
    a.partial = s.partial;
    a.cstats = s.cstats;
    a.y = s.buf[0];
    a.T1 = (int)T[0];
    a.C = c.conv_dim[0];
    a.k = c.conv_kernel[0];
    a.s = c.conv_stride[0];
    a.nchunk = (int)ceil_div(T[0], HF_L0_FR);
    if ((rc = hf_layer0_launch(a, B, stream))) return rc;
    if (!group && (rc = hf_rows_launch<HF_ROWS_LN_GELU>(s.buf[0], s.buf[0], h->ln_w[0], h->ln_b[0], HF_ENC_EPS, (int64_t)B * T[0], a.C, stream))) return rc;
    if (ev != nullptr) MV_HIP_OK(hipEventRecord(ev[1], stream));

    for (int i = 1; i < n; ++i) {
        MvConv1dDesc d = {};
        d.x = s.buf[(i - 1) & 1];
        d.ldx = c.conv_dim[i - 1];
        d.y = s.buf[i & 1];
        d.ldy = c.conv_dim[i];
        d.x_dtype = d.y_dtype = MV_DT_F16;
        d.w_packed = h->w[i];
        d.bias = h->bias[i];
        d.B = B;
        d.T_in = (int)T[i - 1];
        d.T_out = (int)T[i];
        d.cin = c.conv_dim[i - 1];
        d.cout = c.conv_dim[i];
        d.k = c.conv_kernel[i];
        d.dilation = 1;
        d.stride = c.conv_stride[i];
        d.pad = 0;
        d.pad_mode = MV_PAD_ZERO;
        if ((rc = conv1d_launch(d, stream))) return rc;
        const int64_t rows = (int64_t)B * T[i];
        if (group)
            rc = hf_rows_launch<HF_ROWS_GELU>(s.buf[i & 1], s.buf[i & 1], nullptr, nullptr, 0.0f, rows, c.conv_dim[i], stream);
        else
            rc = hf_rows_launch<HF_ROWS_LN_GELU>(s.buf[i & 1], s.buf[i & 1], h->ln_w[i], h->ln_b[i], HF_ENC_EPS, rows, c.conv_dim[i], stream);
        if (rc != MV_OK) return rc;
        if (ev != nullptr) MV_HIP_OK(hipEventRecord(ev[i + 1], stream));
    }
    const int CL = c.conv_dim[n - 1], TL = (int)T[n - 1];
    if ((rc = hf_rows_launch<HF_ROWS_LN_F32>(s.buf[(n - 1) & 1], out, h->proj_w, h->proj_b, c.layer_norm_eps, (int64_t)B * TL, CL, stream))) return rc;
    HfGeom g = {};
    g.n = n;
    for (int i = 0; i < n; ++i) {
        g.k[i] = c.conv_kernel[i];
        g.s[i] = c.conv_stride[i];
    }
    if ((rc = hf_cmn_mask_launch(out, lens_ratio, num_samples, L, g, B, TL, CL, c.subtract_time_mean ? 1 : 0, stream))) return rc;
    if (ev != nullptr) MV_HIP_OK(hipEventRecord(ev[n + 1], stream));
    return MV_OK;
}

}  // namespace

extern "C" {

// ---- the kernels of the forward one at a time (layer-level checks): the launch helpers of hf_forward behind argument checks of their own ----

int mv_hfenc_wave_stats(const float* wav, int32_t B, int64_t L, int64_t wav_stride, const int64_t* num_samples, float* stats, mv_stream_t stream) {
    MV_REQUIRE(wav != nullptr && stats != nullptr, "mv_hfenc_wave_stats: null argument");
    MV_REQUIRE(B > 0 && B <= 65535, "mv_hfenc_wave_stats: batch size must be 1 .. 65535");
    MV_REQUIRE(L >= 0 && wav_stride >= L, "mv_hfenc_wave_stats: wav_stride below the row length");
    return hf_wave_stats_launch(wav, B, L, wav_stride, num_samples, stats, static_cast<hipStream_t>(stream));
}

int mv_hfenc_layer0_workspace_bytes(int32_t B, int64_t L, int32_t C, int32_t k, int32_t s, size_t* bytes) {
    MV_REQUIRE(bytes != nullptr, "mv_hfenc_layer0_workspace_bytes: null argument");
    MV_REQUIRE(B >= 0 && L >= 0 && C >= 0 && k >= 1 && s >= 1, "mv_hfenc_layer0_workspace_bytes: negative size");
    *bytes = (size_t)B * (size_t)ceil_div(hf_conv_frames(L, k, s), HF_L0_FR) * (size_t)C * 2 * sizeof(double);
    return MV_OK;
}

int mv_hfenc_layer0(const float* wav, int32_t B, int64_t L, int64_t wav_stride, const int64_t* num_samples, const float* wstats, const float* w,
                    const float* bias, const float* gamma, const float* beta, int32_t C, int32_t k, int32_t s, void* y, float* cstats, void* workspace,
                    size_t workspace_bytes, mv_stream_t stream) {
    MV_REQUIRE(wav != nullptr && w != nullptr && y != nullptr, "mv_hfenc_layer0: null argument");
    MV_REQUIRE((gamma == nullptr) == (beta == nullptr), "mv_hfenc_layer0: gamma and beta come together (GroupNorm) or not at all");
    MV_REQUIRE(B > 0 && B <= 65535, "mv_hfenc_layer0: batch size must be 1 .. 65535");
    MV_REQUIRE(L >= 0 && wav_stride >= L, "mv_hfenc_layer0: wav_stride below the row length");
    int rc;
    if ((rc = hf_check_width("mv_hfenc_layer0", C))) return rc;
    if (k < 1 || s < 1 || k > HF_L0_MAX_K || s > HF_L0_MAX_S)
        return fail(MV_ERR_UNSUPPORTED, "mv_hfenc_layer0: layer 0 is built for 1 <= k <= 16 and 1 <= s <= 8");
    const int64_t T0 = hf_conv_frames(L, k, s);
    MV_REQUIRE(T0 > 0, "mv_hfenc_layer0: a waveform shorter than the kernel: no frame");
    MV_REQUIRE((int64_t)B * T0 < ((int64_t)1 << 31) - 512, "mv_hfenc_layer0: too many frames for 32-bit row indexing");
    HfL0Args a = {};
    a.wav = wav;
    a.L = L;
    a.wav_stride = wav_stride;
    a.num_samples = num_samples;
    a.wstats = wstats;
    a.w = w;
    a.bias = bias;
    a.gamma = gamma;
    a.beta = beta;
    a.partial = static_cast<double*>(workspace);
    a.cstats = cstats;
    a.y = static_cast<half_t*>(y);
    a.T1 = (int)T0;
    a.C = C;
    a.k = k;
    a.s = s;
    a.nchunk = (int)ceil_div(T0, HF_L0_FR);
    if (gamma != nullptr) {
        MV_REQUIRE(cstats != nullptr, "mv_hfenc_layer0: GroupNorm needs cstats");
        const size_t need = (size_t)B * a.nchunk * C * 2 * sizeof(double);
        if (workspace == nullptr || workspace_bytes < need || (reinterpret_cast<uintptr_t>(workspace) & 7) != 0)
            return fail(MV_ERR_WORKSPACE, "mv_hfenc_layer0: workspace of " + std::to_string(need) + " bytes (8-byte aligned) required");
    }
    return hf_layer0_launch(a, B, static_cast<hipStream_t>(stream));
}

int mv_hfenc_rows(const void* x, void* y, const float* gamma, const float* beta, float eps, int64_t n_rows, int32_t C, int32_t mode,
                  mv_stream_t stream_) {
    MV_REQUIRE(x != nullptr && y != nullptr, "mv_hfenc_rows: null argument");
    MV_REQUIRE(mode == MV_HF_ROWS_GELU || mode == MV_HF_ROWS_LN_GELU || mode == MV_HF_ROWS_LN_F32,
               "mv_hfenc_rows: mode must be MV_HF_ROWS_GELU, MV_HF_ROWS_LN_GELU or MV_HF_ROWS_LN_F32");
    MV_REQUIRE(n_rows > 0, "mv_hfenc_rows: n_rows must be positive");
    int rc;
    if ((rc = hf_check_width("mv_hfenc_rows", C))) return rc;
    if (mode != MV_HF_ROWS_GELU) {
        MV_REQUIRE(gamma != nullptr && beta != nullptr, "mv_hfenc_rows: LayerNorm needs gamma and beta");
        MV_REQUIRE(eps > 0.0f, "mv_hfenc_rows: eps must be positive");
    }
    if (mode == MV_HF_ROWS_LN_F32) MV_REQUIRE(x != y, "mv_hfenc_rows: the fp32 output cannot share the fp16 input's buffer");
    if (C == 512)
        MV_REQUIRE(((reinterpret_cast<uintptr_t>(x) | reinterpret_cast<uintptr_t>(y)) & 15) == 0,
                   "mv_hfenc_rows: x and y must be 16-byte aligned at C = 512 (16-byte loads and stores)");
    hipStream_t stream = static_cast<hipStream_t>(stream_);
    const half_t* xh = static_cast<const half_t*>(x);
    switch (mode) {
        case MV_HF_ROWS_GELU: return hf_rows_launch<HF_ROWS_GELU>(xh, y, nullptr, nullptr, 0.0f, n_rows, C, stream);
        case MV_HF_ROWS_LN_GELU: return hf_rows_launch<HF_ROWS_LN_GELU>(xh, y, gamma, beta, eps, n_rows, C, stream);
        default: return hf_rows_launch<HF_ROWS_LN_F32>(xh, y, gamma, beta, eps, n_rows, C, stream);
    }
}

int mv_hfenc_cmn_mask(float* out, int32_t B, int32_t T, int32_t C, const float* lens_ratio, const int64_t* num_samples, int64_t L,
                      const int32_t* conv_kernel, const int32_t* conv_stride, int32_t num_layers, int32_t cmn, mv_stream_t stream) {
    MV_REQUIRE(out != nullptr, "mv_hfenc_cmn_mask: null argument");
    MV_REQUIRE(lens_ratio == nullptr || num_samples == nullptr, "mv_hfenc_cmn_mask: lens_ratio or num_samples, not both");
    MV_REQUIRE(B > 0 && B <= 65535, "mv_hfenc_cmn_mask: batch size must be 1 .. 65535");
    MV_REQUIRE(T > 0, "mv_hfenc_cmn_mask: T must be positive");
    int rc;
    if ((rc = hf_check_width("mv_hfenc_cmn_mask", C))) return rc;
    HfGeom g = {};
    if (num_samples != nullptr) {   // the row's own frame count comes from its samples: T has to be the count of a full row
        MV_REQUIRE(conv_kernel != nullptr && conv_stride != nullptr, "mv_hfenc_cmn_mask: num_samples needs the layers' kernels and strides");
        MV_REQUIRE(num_layers >= 1 && num_layers <= MV_HFENC_MAX_LAYERS, "mv_hfenc_cmn_mask: num_layers must be 1 .. MV_HFENC_MAX_LAYERS (8)");
        g.n = num_layers;
        for (int i = 0; i < num_layers; ++i) {
            MV_REQUIRE(conv_kernel[i] >= 1 && conv_stride[i] >= 1 && conv_kernel[i] <= 64 && conv_stride[i] <= 64,
                       "mv_hfenc_cmn_mask: conv_kernel / conv_stride must be 1 .. 64");
            g.k[i] = conv_kernel[i];
            g.s[i] = conv_stride[i];
        }
        MV_REQUIRE(L >= 0 && hf_frames_behind(g, L) == T, "mv_hfenc_cmn_mask: T is not the frame count of L samples behind these layers");
    }
    return hf_cmn_mask_launch(out, lens_ratio, num_samples, L, g, B, T, C, cmn ? 1 : 0, static_cast<hipStream_t>(stream));
}

int mv_hfenc_forward(const MvHfEncoder* h, const float* wav, int32_t B, int64_t L, int64_t wav_stride, const float* lens_ratio, float* out,
                     void* workspace, size_t workspace_bytes, mv_stream_t stream) {
    return hf_forward(h, wav, B, L, wav_stride, lens_ratio, nullptr, out, workspace, workspace_bytes, stream, nullptr);
}

int mv_hfenc_forward_varlen(const MvHfEncoder* h, const float* wav, int32_t B, int64_t L, int64_t wav_stride, const int64_t* num_samples, float* out,
                            void* workspace, size_t workspace_bytes, mv_stream_t stream) {
    MV_REQUIRE(num_samples != nullptr, "mv_hfenc_forward_varlen: null length array");
    return hf_forward(h, wav, B, L, wav_stride, nullptr, num_samples, out, workspace, workspace_bytes, stream, nullptr);
}

int mv_hfenc_forward_timed(const MvHfEncoder* h, const float* wav, int32_t B, int64_t L, int64_t wav_stride, const float* lens_ratio, float* out,
                           void* workspace, size_t workspace_bytes, mv_stream_t stream, float* stage_ms_host, int32_t num_stages) {
    MV_REQUIRE(h != nullptr && stage_ms_host != nullptr, "mv_hfenc_forward_timed: null argument");
    const int n = h->cfg.num_layers;
    MV_REQUIRE(num_stages == n + 1, "mv_hfenc_forward_timed: num_stages must be num_layers + 1 (every layer, then the tail)");
    static hipEvent_t ev[MV_HFENC_MAX_LAYERS + 2] = {};   // (created once on the device current then, kept: a measurement hook for one device, not thread-safe -- like mv_profile_*)
    static bool have = false;
    if (!have) {
        for (hipEvent_t& e : ev) MV_HIP_OK(hipEventCreate(&e));
        have = true;
    }
    const int rc = hf_forward(h, wav, B, L, wav_stride, lens_ratio, nullptr, out, workspace, workspace_bytes, stream, ev);
    if (rc != MV_OK) return rc;
    MV_HIP_OK(hipEventSynchronize(ev[n + 1]));
    for (int i = 0; i <= n; ++i) MV_HIP_OK(hipEventElapsedTime(&stage_ms_host[i], ev[i], ev[i + 1]));
    return MV_OK;
}

}  // extern "C"
