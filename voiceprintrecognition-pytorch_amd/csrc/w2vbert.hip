// The Wav2Vec2-BERT (facebook/w2v-bert-2.0) front-end for gfx950: what AudioFeaturizer(use_hf_model=True) keeps of that model is
// `extract_features` = feature_projection.layer_norm(input_features), and input_features is the SeamlessM4TFeatureExtractor's work, which the
// reference does on the host in numpy, one utterance at a time (transformers.audio_utils.spectrogram, a Python loop over frames):
//   waveform * 2^15 -> Kaldi log-mel, 80 bins -> per bin over the row's T frames (x - mean) / sqrt(var(ddof = 1) + 1e-7) -> zero frames up to a
//   multiple of 2 -> pairs of frames stacked into 160 columns -> LayerNorm over the columns -> time mean and mask (featurizer.py:79-90).
//
// Launches of one forward, ordered by the stream alone (no workgroup waits for another):
//   1. the log-mel: the Fbank kernels (fbank.hip) through an Fbank handle this handle owns, whose window table carries the 2^15 -- a power of two,
//      so it commutes with every rounding of the linear steps up to the power spectrum and the handle featurises 2^15 * waveform exactly without a
//      pass over the waveform; raw rows [B, T, 80] to the workspace (no time mean, no mask; the variable-length form leaves zeros behind T_b);
//   2. w2v_binstats_kernel: per (row, bin) mean and unbiased variance over the row's T_b frames: centred two-pass in fp64, one fixed order;
//   3. w2v_rows_kernel: one wave per stacked frame: normalise, stack, LayerNorm over 160 columns with 16-byte loads and stores;
//   4. w2v_cmn_mask_kernel: time mean over the row's T2_b stacked frames (fp64, one fixed order), subtract, mask -- in place on the output.
// Every sum has an order that depends on the row's own frame count alone: a row's bits do not depend on the batch, the stream or what the
// buffers held.  Scratch is the caller's workspace; the handle holds tables only.
#include "frontend_common.h"
#include "model.h"

#include <memory>
#include <vector>

namespace mv {

constexpr int W2V_BINS = 80;                       // mel bins: a frame is 320 bytes
constexpr int W2V_STRIDE = 2;                      // frames stacked per output row
constexpr int W2V_COLS = W2V_BINS * W2V_STRIDE;    // 160 columns: a stacked frame is 640 bytes
constexpr int W2V_WIN = 400, W2V_SHIFT = 160;      // 25 ms / 10 ms at 16 kHz
constexpr int W2V_MIN_SAMPLES = W2V_WIN + W2V_SHIFT;   // two frames: below, var(ddof = 1) has nothing to divide by
constexpr int W2V_SUM_THREADS = 640;               // the column-sum kernels: 8 x 80 or 4 x 160 threads
constexpr int W2V_SUM_TILE = 16;                   // frames per partial sum
constexpr int W2V_ROWS_WAVES = 4;                  // w2v_rows_kernel: stacked frames (waves) per workgroup
constexpr float W2V_NORM_EPS = 1e-7f;              // SeamlessM4TFeatureExtractor: sqrt(var + 1e-7)

// frames of a row of n samples (snip_edges); the front-end gives a row below two frames none
__host__ __device__ inline int64_t w2v_frames(int64_t n) { return n < W2V_MIN_SAMPLES ? 0 : 1 + (n - W2V_WIN) / W2V_SHIFT; }

// T_b: the row's own frames in the variable-length form, T in the batch form
__device__ __forceinline__ int w2v_row_frames(const int64_t* num_samples, int b, int64_t L, int T) {
    if (num_samples == nullptr) return T;
    int64_t n = num_samples[b];
    n = n < 0 ? 0 : (n > L ? L : n);
    const int64_t t = w2v_frames(n);
    return (int)(t < T ? t : T);
}

// The sum over rows 0 .. n - 1 of column c = tid % COLS of x [n][COLS] (SQ: of (x - centre)^2), fp64, in ONE order that depends on n alone:
// thread group g = tid / COLS of G = 640 / COLS adds the partial sums of the 16-row tiles g, g + G, ... in tile order, each partial summed in row
// order; the G group sums are added in group order.  Every thread returns its column's sum; ends on a barrier behind every read of x.
template <int COLS, bool SQ>
__device__ __forceinline__ double w2v_col_sum(const float* x, int n, int tid, double centre, double* red) {
    constexpr int G = W2V_SUM_THREADS / COLS;
    const int g = tid / COLS, c = tid - g * COLS;
    double run = 0.0;
    for (int t0 = g * W2V_SUM_TILE; t0 < n; t0 += G * W2V_SUM_TILE) {
        const int t1 = t0 + W2V_SUM_TILE < n ? t0 + W2V_SUM_TILE : n;
        double part = 0.0;
        for (int t = t0; t < t1; ++t) {
            double v = (double)x[(int64_t)t * COLS + c];
            if (SQ) {
                v -= centre;
                v *= v;
            }
            part += v;
        }
        run += part;
    }
    red[g * COLS + c] = run;
    __syncthreads();
    double s = 0.0;
#pragma unroll
    for (int k = 0; k < G; ++k) s += red[k * COLS + c];
    __syncthreads();   // red is free again
    return s;
}

// one workgroup per row: mean and unbiased variance of every bin over the row's T_b frames
__global__ __launch_bounds__(W2V_SUM_THREADS) void w2v_binstats_kernel(const float* x, int T, const int64_t* num_samples, int64_t L, float* mean,
                                                                       float* var) {
    __shared__ double red[W2V_SUM_THREADS];
    const int b = blockIdx.x, tid = threadIdx.x;
    const int Tb = w2v_row_frames(num_samples, b, L, T);
    const float* xb = x + (int64_t)b * T * W2V_BINS;
    const double sum = w2v_col_sum<W2V_BINS, false>(xb, Tb, tid, 0.0, red);
    const double m = Tb > 0 ? sum / (double)Tb : 0.0;
    const double ss = w2v_col_sum<W2V_BINS, true>(xb, Tb, tid, m, red);
    if (tid < W2V_BINS) {
        mean[(int64_t)b * W2V_BINS + tid] = (float)m;
        var[(int64_t)b * W2V_BINS + tid] = Tb > 1 ? (float)(ss / (double)(Tb - 1)) : 0.0f;
    }
}

__device__ __forceinline__ float w2v_wave_sum(float v) {
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) v += __shfl_xor(v, off);
    return v;
}

// one wave per stacked frame (b, t2): lane l < 40 holds columns 4 l .. 4 l + 3 = bins 4 (l % 20) .. of frame 2 t2 + l / 20
__global__ __launch_bounds__(W2V_ROWS_WAVES * 64) void w2v_rows_kernel(const float* x, const float* mean, const float* var, const float* ln_w,
                                                                       const float* ln_b, float eps, int T, int T2, int64_t n_rows,
                                                                       const int64_t* num_samples, int64_t L, float* out) {
    const int lane = threadIdx.x & 63;
    const int64_t r = (int64_t)blockIdx.x * W2V_ROWS_WAVES + (threadIdx.x >> 6);
    if (r >= n_rows) return;   // (whole waves: no barrier below)
    const int b = (int)(r / T2), t2 = (int)(r - (int64_t)b * T2);
    const int Tb = w2v_row_frames(num_samples, b, L, T);
    const bool active = lane < W2V_COLS / 4;
    const int s = lane >= W2V_BINS / 4 ? 1 : 0, cg = lane - s * (W2V_BINS / 4);
    const int t = W2V_STRIDE * t2 + s;
    float4v* dst = reinterpret_cast<float4v*>(out + r * W2V_COLS) + lane;
    const float4v zero4 = float4v{0.0f, 0.0f, 0.0f, 0.0f};
    if (W2V_STRIDE * t2 >= Tb) {   // wave-uniform: behind the row's own stacked frames
        if (active) *dst = zero4;
        return;
    }
    float4v z = zero4;
    if (active && t < Tb) {   // a frame at or behind T_b inside the last stacked frame is zeros, not a normalised value
        const float4v xv = *(reinterpret_cast<const float4v*>(x + ((int64_t)b * T + t) * W2V_BINS) + cg);
        const float4v mv4 = *(reinterpret_cast<const float4v*>(mean + (int64_t)b * W2V_BINS) + cg);
        const float4v vv = *(reinterpret_cast<const float4v*>(var + (int64_t)b * W2V_BINS) + cg);
#pragma unroll
        for (int i = 0; i < 4; ++i) z[i] = (xv[i] - mv4[i]) / sqrtf(vv[i] + W2V_NORM_EPS);
    }
    const float mu = w2v_wave_sum((z[0] + z[1]) + (z[2] + z[3])) / (float)W2V_COLS;   // (idle lanes add zeros)
    float4v d = zero4;
    if (active) d = z - float4v{mu, mu, mu, mu};
    const float v = w2v_wave_sum((d[0] * d[0] + d[1] * d[1]) + (d[2] * d[2] + d[3] * d[3])) / (float)W2V_COLS;
    const float rstd = 1.0f / sqrtf(v + eps);
    if (active) {
        const float4v w4 = *(reinterpret_cast<const float4v*>(ln_w) + lane), b4 = *(reinterpret_cast<const float4v*>(ln_b) + lane);
        float4v y;
#pragma unroll
        for (int i = 0; i < 4; ++i) y[i] = d[i] * rstd * w4[i] + b4[i];
        *dst = y;
    }
}

// one workgroup per row, in place: the time mean over the row's T2_b stacked frames, then the mask (featurizer.py:79-90)
__global__ __launch_bounds__(W2V_SUM_THREADS) void w2v_cmn_mask_kernel(float* out, int T, int T2, const float* lens_ratio, const int64_t* num_samples,
                                                                       int64_t L, int cmn) {
    __shared__ double red[W2V_SUM_THREADS];
    __shared__ __attribute__((aligned(16))) float tmean[W2V_COLS];
    const int b = blockIdx.x, tid = threadIdx.x;
    const int Tb = w2v_row_frames(num_samples, b, L, T);
    const int T2b = (Tb + W2V_STRIDE - 1) / W2V_STRIDE;
    float* ob = out + (int64_t)b * T2 * W2V_COLS;
    double sum = 0.0;
    if (cmn) sum = w2v_col_sum<W2V_COLS, false>(ob, T2b, tid, 0.0, red);   // (uniform)
    if (tid < W2V_COLS) tmean[tid] = cmn && T2b > 0 ? (float)(sum / (double)T2b) : 0.0f;
    __syncthreads();
    int mask_len = T2b;
    if (lens_ratio != nullptr) mask_len = (int)rintf(lens_ratio[b] * (float)T2);   // round half to even
    constexpr int Q = W2V_COLS / 4;
    const int total = T2 * Q;
    for (int i = tid; i < total; i += W2V_SUM_THREADS) {
        const int t = i / Q, cg = i - t * Q;
        float4v* p = reinterpret_cast<float4v*>(ob) + i;
        const float4v m4 = *(reinterpret_cast<const float4v*>(tmean) + cg);
        *p = t < mask_len ? *p - m4 : float4v{0.0f, 0.0f, 0.0f, 0.0f};
    }
}

// ---- launch helpers: the forward and the kernel-level entry points go through these

static int w2v_binstats_launch(const float* x, int B, int T, const int64_t* num_samples, int64_t L, float* mean, float* var, hipStream_t st) {
    MV_LAUNCH(w2v_binstats_kernel, ((unsigned)B, 1, 1), (W2V_SUM_THREADS, 1, 1), 0, st, x, T, num_samples, L, mean, var);
    return check_launch("w2v_binstats_kernel");
}

static int w2v_rows_launch(const float* x, const float* mean, const float* var, const float* ln_w, const float* ln_b, float eps, int B, int T,
                           const int64_t* num_samples, int64_t L, float* out, hipStream_t st) {
    const int T2 = (T + W2V_STRIDE - 1) / W2V_STRIDE;
    const int64_t n_rows = (int64_t)B * T2;
    MV_LAUNCH(w2v_rows_kernel, ((unsigned)ceil_div(n_rows, W2V_ROWS_WAVES), 1, 1), (W2V_ROWS_WAVES * 64, 1, 1), 0, st, x, mean, var, ln_w, ln_b, eps, T, T2,
              n_rows, num_samples, L, out);
    return check_launch("w2v_rows_kernel");
}

static int w2v_cmn_mask_launch(float* out, int B, int T, int T2, const float* lens_ratio, const int64_t* num_samples, int64_t L, int cmn, hipStream_t st) {
    MV_LAUNCH(w2v_cmn_mask_kernel, ((unsigned)B, 1, 1), (W2V_SUM_THREADS, 1, 1), 0, st, out, T, T2, lens_ratio, num_samples, L, cmn);
    return check_launch("w2v_cmn_mask_kernel");
}

}  // namespace mv

struct MvW2vBert {
    MvW2vBertCfg cfg;
    MvFbank* fbank = nullptr;   // 80-bin Kaldi log-mel on 2^15 * waveform: no time mean, no mask
    float* ln_w = nullptr;      // feature_projection.layer_norm [160]
    float* ln_b = nullptr;
    ~MvW2vBert() {
        mv_fbank_destroy(fbank);
        hipFree(ln_w);
        hipFree(ln_b);
    }
};

namespace {

using namespace mv;

struct W2vScratch {
    float* mel;     // [B, T, 80]
    float* mean;    // [B, 80]
    float* var;     // [B, 80]
    void* fbank;    // the Fbank handle's own sections
    size_t fbank_bytes, bytes;
};

int w2v_carve(const MvW2vBert* h, int B, int64_t L, int64_t T, void* ws, W2vScratch* s) {
    Carver cv(ws);
    s->mel = cv.take<float>((size_t)B * (size_t)T * W2V_BINS);
    s->mean = cv.take<float>((size_t)B * W2V_BINS);
    s->var = cv.take<float>((size_t)B * W2V_BINS);
    int rc;
    if ((rc = mv_fbank_workspace_bytes(h->fbank, B, L, &s->fbank_bytes))) return rc;
    s->fbank = cv.take<char>(s->fbank_bytes);
    s->bytes = cv.total();
    return MV_OK;
}

// both forms: lens_ratio (batch form, or neither) or num_samples (variable-length form), never both
int w2v_forward(const char* fn, const MvW2vBert* h, const float* wav, int32_t B, int64_t L, int64_t wav_stride, const float* lens_ratio,
                const int64_t* num_samples, bool varlen, float* out, void* workspace, size_t workspace_bytes, mv_stream_t stream) {
    const std::string who(fn);
    MV_REQUIRE(h != nullptr, who + ": null handle");
    MV_REQUIRE(B >= 0 && L >= 0, who + ": negative size");
    MV_REQUIRE(wav_stride >= L, who + ": wav_stride below the row length");
    if (B == 0) return MV_OK;
    MV_REQUIRE(!varlen || num_samples != nullptr, who + ": null length array");
    if (!varlen && L < W2V_MIN_SAMPLES)
        return fail(MV_ERR_INVALID_ARGUMENT, who + ": a waveform of " + std::to_string(L) + " samples has fewer than two frames (560 samples): the per-bin "
                                                 "variance (ddof = 1) has nothing to divide by, and below 400 samples the extractor has no frame");
    const int64_t T = L < W2V_WIN ? 0 : 1 + (L - W2V_WIN) / W2V_SHIFT;
    if (T == 0) return MV_OK;   // (variable-length form: an empty output)
    const int64_t T2 = ceil_div(T, W2V_STRIDE);
    MV_REQUIRE(wav != nullptr && out != nullptr, who + ": null buffer");
    MV_REQUIRE((reinterpret_cast<uintptr_t>(out) & 15) == 0, who + ": out must be 16-byte aligned");
    MV_REQUIRE(T * W2V_COLS < (int64_t)1 << 31 && ceil_div((int64_t)B * T2, W2V_ROWS_WAVES) < (int64_t)1 << 31, who + ": too many frames for 32-bit indexing");
    W2vScratch s;
    int rc;
    if ((rc = w2v_carve(h, B, L, T, workspace, &s))) return rc;
    if (workspace == nullptr || workspace_bytes < s.bytes || (reinterpret_cast<uintptr_t>(workspace) & 15) != 0)
        return fail(MV_ERR_WORKSPACE, who + ": workspace of " + std::to_string(s.bytes) + " bytes (16-byte aligned) required");
    hipStream_t st = static_cast<hipStream_t>(stream);
    if (varlen)
        rc = mv_fbank_forward_varlen_ws(h->fbank, wav, B, L, wav_stride, num_samples, s.mel, s.fbank, s.fbank_bytes, stream);
    else
        rc = mv_fbank_forward_ws(h->fbank, wav, B, L, wav_stride, nullptr, s.mel, s.fbank, s.fbank_bytes, stream);
    if (rc != MV_OK) return rc;
    if ((rc = w2v_binstats_launch(s.mel, B, (int)T, num_samples, L, s.mean, s.var, st))) return rc;
    if ((rc = w2v_rows_launch(s.mel, s.mean, s.var, h->ln_w, h->ln_b, h->cfg.layer_norm_eps, B, (int)T, num_samples, L, out, st))) return rc;
    const int cmn = h->cfg.subtract_time_mean ? 1 : 0;
    if (!cmn && lens_ratio == nullptr) return MV_OK;   // (the row pass has written the zero rows of the variable-length form)
    return w2v_cmn_mask_launch(out, B, (int)T, (int)T2, lens_ratio, num_samples, L, cmn, st);
}

// the shape checks of the kernel-level entry points
int w2v_check_rows(const std::string& who, int32_t B, int32_t T, const int64_t* num_samples, int64_t L) {
    MV_REQUIRE(B > 0, who + ": B must be positive");
    MV_REQUIRE(T >= 2, who + ": T must be at least 2 (the unbiased variance of one frame has nothing to divide by)");
    MV_REQUIRE((int64_t)T * W2V_COLS < (int64_t)1 << 31, who + ": too many frames for 32-bit indexing");
    if (num_samples != nullptr) MV_REQUIRE(L >= 0 && w2v_frames(L) == T, who + ": T is not the frame count of L samples");
    return MV_OK;
}

}  // namespace

extern "C" {

int mv_w2vbert_create(const MvW2vBertCfg* cfg, const float* ln_weight, const float* ln_bias, MvW2vBert** out) {
    MV_REQUIRE(cfg != nullptr && ln_weight != nullptr && ln_bias != nullptr && out != nullptr, "mv_w2vbert_create: null argument");
    if (cfg->num_mel_bins != W2V_BINS)
        return fail(MV_ERR_UNSUPPORTED, "mv_w2vbert_create: num_mel_bins = " + std::to_string(cfg->num_mel_bins) + ": the kernels are built for 80 mel bins");
    if (cfg->stride != W2V_STRIDE)
        return fail(MV_ERR_UNSUPPORTED, "mv_w2vbert_create: stride = " + std::to_string(cfg->stride) + ": the kernels are built for stride 2");
    if (cfg->sampling_rate != 16000)
        return fail(MV_ERR_UNSUPPORTED, "mv_w2vbert_create: sampling_rate = " + std::to_string(cfg->sampling_rate) + ": the kernels are built for 16000 Hz");
    MV_REQUIRE(cfg->layer_norm_eps > 0.0f, "mv_w2vbert_create: layer_norm_eps must be positive");
    std::unique_ptr<MvW2vBert> h(new MvW2vBert());
    h->cfg = *cfg;
    MvFbankCfg fc;
    mv_fbank_default_cfg(&fc);   // 25 / 10 ms, Povey, pre-emphasis 0.97, DC removal, log power, 20 Hz .. Nyquist, snip_edges
    fc.sample_frequency = (float)cfg->sampling_rate;
    fc.num_mel_bins = cfg->num_mel_bins;
    fc.subtract_time_mean = 0;
    int rc;
    if ((rc = fbank_create_scaled(&fc, 32768.0f, &h->fbank))) return rc;   // the extractor's waveform * 2^15, in the window table
    for (int i = 0; i < 2; ++i) {
        float** dst = i == 0 ? &h->ln_w : &h->ln_b;
        MV_HIP_OK(hipMalloc(reinterpret_cast<void**>(dst), W2V_COLS * sizeof(float)));
        MV_HIP_OK(hipMemcpy(*dst, i == 0 ? ln_weight : ln_bias, W2V_COLS * sizeof(float), hipMemcpyHostToDevice));
    }
    *out = h.release();
    return MV_OK;
}

int mv_w2vbert_destroy(MvW2vBert* h) {
    delete h;
    return MV_OK;
}

int mv_w2vbert_num_frames(const MvW2vBert* h, int64_t num_samples, int64_t* num_frames) {
    MV_REQUIRE(h != nullptr && num_frames != nullptr, "mv_w2vbert_num_frames: null argument");
    *num_frames = num_samples < W2V_WIN ? 0 : ceil_div(1 + (num_samples - W2V_WIN) / W2V_SHIFT, W2V_STRIDE);
    return MV_OK;
}

int mv_w2vbert_workspace_bytes(const MvW2vBert* h, int32_t B, int64_t L, size_t* bytes) {
    MV_REQUIRE(h != nullptr && bytes != nullptr, "mv_w2vbert_workspace_bytes: null argument");
    MV_REQUIRE(B >= 0 && L >= 0, "mv_w2vbert_workspace_bytes: negative size");
    *bytes = 0;
    if (B == 0 || L < W2V_WIN) return MV_OK;
    W2vScratch s;
    const int rc = w2v_carve(h, B, L, 1 + (L - W2V_WIN) / W2V_SHIFT, nullptr, &s);
    if (rc == MV_OK) *bytes = s.bytes;
    return rc;
}

int mv_w2vbert_forward(const MvW2vBert* h, const float* wav, int32_t B, int64_t L, int64_t wav_stride, const float* lens_ratio, float* out,
                       void* workspace, size_t workspace_bytes, mv_stream_t stream) {
    return w2v_forward("mv_w2vbert_forward", h, wav, B, L, wav_stride, lens_ratio, nullptr, false, out, workspace, workspace_bytes, stream);
}

int mv_w2vbert_forward_varlen(const MvW2vBert* h, const float* wav, int32_t B, int64_t L, int64_t wav_stride, const int64_t* num_samples, float* out,
                              void* workspace, size_t workspace_bytes, mv_stream_t stream) {
    return w2v_forward("mv_w2vbert_forward_varlen", h, wav, B, L, wav_stride, nullptr, num_samples, true, out, workspace, workspace_bytes, stream);
}

int mv_w2vbert_binstats_f32(const float* x, int32_t B, int32_t T, const int64_t* num_samples, int64_t L, float* mean, float* var, mv_stream_t stream) {
    MV_REQUIRE(x != nullptr && mean != nullptr && var != nullptr, "mv_w2vbert_binstats_f32: null argument");
    int rc;
    if ((rc = w2v_check_rows("mv_w2vbert_binstats_f32", B, T, num_samples, L))) return rc;
    return w2v_binstats_launch(x, B, T, num_samples, L, mean, var, static_cast<hipStream_t>(stream));
}

int mv_w2vbert_rows_f32(const float* x, const float* mean, const float* var, const float* ln_weight, const float* ln_bias, float eps, int32_t B,
                        int32_t T, const int64_t* num_samples, int64_t L, float* out, mv_stream_t stream) {
    MV_REQUIRE(x != nullptr && mean != nullptr && var != nullptr && ln_weight != nullptr && ln_bias != nullptr && out != nullptr,
               "mv_w2vbert_rows_f32: null argument");
    MV_REQUIRE(eps > 0.0f, "mv_w2vbert_rows_f32: eps must be positive");
    int rc;
    if ((rc = w2v_check_rows("mv_w2vbert_rows_f32", B, T, num_samples, L))) return rc;
    MV_REQUIRE(ceil_div((int64_t)B * ceil_div(T, W2V_STRIDE), W2V_ROWS_WAVES) < (int64_t)1 << 31, "mv_w2vbert_rows_f32: too many frames for 32-bit indexing");
    const uintptr_t all = reinterpret_cast<uintptr_t>(x) | reinterpret_cast<uintptr_t>(mean) | reinterpret_cast<uintptr_t>(var) |
                          reinterpret_cast<uintptr_t>(ln_weight) | reinterpret_cast<uintptr_t>(ln_bias) | reinterpret_cast<uintptr_t>(out);
    MV_REQUIRE((all & 15) == 0, "mv_w2vbert_rows_f32: x, mean, var, ln_weight, ln_bias and out must be 16-byte aligned (16-byte loads and stores)");
    return w2v_rows_launch(x, mean, var, ln_weight, ln_bias, eps, B, T, num_samples, L, out, static_cast<hipStream_t>(stream));
}

int mv_w2vbert_cmn_mask_f32(float* out, int32_t B, int32_t T2, const float* lens_ratio, const int64_t* num_samples, int64_t L, int32_t cmn,
                            mv_stream_t stream) {
    MV_REQUIRE(out != nullptr, "mv_w2vbert_cmn_mask_f32: null argument");
    MV_REQUIRE(lens_ratio == nullptr || num_samples == nullptr, "mv_w2vbert_cmn_mask_f32: lens_ratio or num_samples, not both");
    MV_REQUIRE(B > 0 && T2 > 0, "mv_w2vbert_cmn_mask_f32: B and T2 must be positive");
    MV_REQUIRE((int64_t)T2 * W2V_COLS < (int64_t)1 << 31, "mv_w2vbert_cmn_mask_f32: too many frames for 32-bit indexing");
    MV_REQUIRE((reinterpret_cast<uintptr_t>(out) & 15) == 0, "mv_w2vbert_cmn_mask_f32: out must be 16-byte aligned");
    int T = W2V_STRIDE * T2;   // batch form: the kernel needs T2_b = T2 only
    if (num_samples != nullptr) {
        const int64_t TL = L < W2V_WIN ? 0 : 1 + (L - W2V_WIN) / W2V_SHIFT;
        MV_REQUIRE(L >= 0 && ceil_div(TL, W2V_STRIDE) == T2, "mv_w2vbert_cmn_mask_f32: T2 is not the stacked frame count of L samples");
        T = (int)TL;
    }
    return w2v_cmn_mask_launch(out, B, T, T2, lens_ratio, num_samples, L, cmn ? 1 : 0, static_cast<hipStream_t>(stream));
}

}  // extern "C"
