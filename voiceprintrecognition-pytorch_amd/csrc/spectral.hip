// Spectrogram and MFCC front-ends for gfx950 (torchaudio.transforms.Spectrogram / MFCC(**method_args), featurizer.py:43-50 of the
// reference) followed by AudioFeaturizer's time-mean subtraction and length mask (featurizer.py:77-90).
//
// Spectrogram: a MvMelSpec handle in spectrogram mode (melspec.hip).  n_fft = 400 runs melspec_tile_kernel<0, 0, true> -- the real FFT of
// the MelSpectrogram path with the 201 power bins written as the features, time mean and mask in the same launch; any other geometry
// stft_power_kernel + cmn_mask_kernel reading its padded bin rows.
//
// MFCC, three launches after the mel stage:
//   mel stage             the MelSpectrogram kernels with the time mean off and no mask: mel power [B, T, n_mels] in the caller workspace
//   mfcc_db_max_kernel    (log_mels = 0 only) per utterance: max over its frames and mels of 10 log10(max(mel, 1e-10))
//   mfcc_dct_kernel       per utterance: floor = max over the batch of those maxima - top_db (torchaudio.functional.amplitude_to_DB takes
//                         ONE amax over a [B, n_mels, T] tensor: it packs B as channels of one item), db = max(dB, floor) (or
//                         log(mel + 1e-6)), DCT-II on exact fp32 FMAs in a fixed order, the time mean over all frames, the mask,
//                         one write of [T, n_mfcc]
// The batch-wide maximum is a global dependency: it is a launch boundary, not a grid barrier, and it never leaves the device.
#include <memory>
#include <vector>

#include "frontend_common.h"
#include "kernels.h"
#include "spectral.h"

namespace mv {

constexpr int MFCC_THREADS = 256;
constexpr int MFCC_FR = 32;               // frames per DCT chunk (their dB rows are staged in LDS)
constexpr int MFCC_DCT_LDS_MAX = 16384;   // n_mels * n_mfcc floats up to which the DCT table is copied to LDS (64 KB)
constexpr size_t MFCC_LDS = 150 * 1024;   // dynamic LDS budget of mfcc_dct_kernel

__device__ __forceinline__ float mfcc_db(float x) { return 10.0f * log10f(fmaxf(x, 1e-10f)); }

// rowmax[b] = max over the row's frames x n_mels of mfcc_db(mel): all T frames, or the row's own (variable-length form; -inf for a row
// without frames).  max is exact, so the reduction order does not matter.
__global__ __launch_bounds__(MFCC_THREADS) void mfcc_db_max_kernel(const float* mel, int T, int n_mels, RowLens rows, float* rowmax) {
    __shared__ float red[MFCC_THREADS / 64];
    const float* p = mel + (int64_t)blockIdx.x * T * n_mels;
    int64_t Lb;
    const int64_t n = (int64_t)row_frames(rows, blockIdx.x, 0, T, &Lb) * n_mels;
    float m = -INFINITY;
    for (int64_t i = threadIdx.x; i < n; i += MFCC_THREADS) m = fmaxf(m, mfcc_db(p[i]));
    for (int off = 32; off > 0; off >>= 1) m = fmaxf(m, __shfl_xor(m, off));
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = m;
    __syncthreads();
    if (threadIdx.x == 0) {
        float r = red[0];
        for (int w = 1; w < MFCC_THREADS / 64; ++w) r = fmaxf(r, red[w]);
        rowmax[blockIdx.x] = r;
    }
}

struct MfccArgs {
    const float* mel;        // [B, T, n_mels] power
    const float* rowmax;     // [B] (log_mels = 0)
    const float* dct;        // [n_mels][n_mfcc]
    const float* lens_ratio;
    float* out;              // [B, T, n_mfcc]
    int B, T, n_mels, n_mfcc, log_mels, cmn, tile_rows;
    float top_db;
    RowLens rows;            // per-row lengths (variable-length form) or none
};

// One workgroup per utterance.  LDS: [DCT table if DCT_LDS][MFCC_FR][n_mels] dB rows, [tile_rows][n_mfcc] coefficients waiting for the
// time mean; coefficient rows beyond tile_rows are written to `out` and re-read.
template <bool DCT_LDS>
__global__ __launch_bounds__(MFCC_THREADS) void mfcc_dct_kernel(MfccArgs a) {
    MV_DYN_SMEM(smem);
    __shared__ float part[4][64];
    __shared__ float mean[256];
    const int tid = threadIdx.x, b = blockIdx.x;
    const int nm = a.n_mels, nc = a.n_mfcc;
    // T frames: the batch's, or this row's own (variable-length form: the chunks, the time mean and its summation order follow T alone;
    // the output keeps a.T rows, zero behind T)
    int64_t Lb;
    const int T = row_frames(a.rows, b, 0, a.T, &Lb);
    float* base = reinterpret_cast<float*>(smem);
    const float* dct = a.dct;
    if constexpr (DCT_LDS) {
        for (int i = tid; i < nm * nc; i += MFCC_THREADS) base[i] = a.dct[i];
        dct = base;
        base += (nm * nc + 3) & ~3;
    }
    float* xs = base;                      // [MFCC_FR][n_mels]
    float* tile = xs + MFCC_FR * nm;       // [tile_rows][n_mfcc]
    const float* mel = a.mel + (int64_t)b * a.T * nm;
    float* orow = a.out + (int64_t)b * a.T * nc;
    float floor_db = -INFINITY;
    if (!a.log_mels) {
        float m = -INFINITY;
        if (a.rows.num_samples != nullptr) m = a.rowmax[b];            // variable-length form: the row's own loudest value
        else for (int i = 0; i < a.B; ++i) m = fmaxf(m, a.rowmax[i]);   // uniform: scalar loads
        floor_db = m - a.top_db;
    }
    for (int t0 = 0; t0 < T; t0 += MFCC_FR) {
        const int nf = T - t0 < MFCC_FR ? T - t0 : MFCC_FR;
        __syncthreads();   // (previous chunk's rows consumed; first chunk: the DCT table is in place)
        for (int i = tid; i < nf * nm; i += MFCC_THREADS) {
            const float x = mel[(int64_t)t0 * nm + i];
            xs[i] = a.log_mels ? logf(x + 1e-6f) : fmaxf(mfcc_db(x), floor_db);
        }
        __syncthreads();
        for (int i = tid; i < nf * nc; i += MFCC_THREADS) {
            const int f = i / nc, k = i - f * nc;
            const float* xr = xs + f * nm;
            float s = 0.0f;
            for (int m = 0; m < nm; ++m) s = fmaf(xr[m], dct[m * nc + k], s);
            const int t = t0 + f;
            if (t < a.tile_rows) MV_AS_LDS(float, tile)[t * nc + k] = s;
            else MV_AS_GLOBAL(float, orow)[(int64_t)t * nc + k] = s;
        }
    }
    __syncthreads();
    auto raw = [&](int t, int c) {   // (address-space casts on both sides: a select between the two pointers would be a FLAT access)
        if (t < a.tile_rows) return MV_AS_LDS(float, tile)[t * nc + c];
        return MV_AS_GLOBAL(float, orow)[(int64_t)t * nc + c];
    };
    // column means over ALL frames in the fixed order of cmn_mask_kernel (4 time phases, then their sum)
    for (int c0 = 0; c0 < nc; c0 += 64) {
        const int c = c0 + (tid & 63), ph = tid >> 6;
        float s = 0.0f;
        if (c < nc)
            for (int t = ph; t < T; t += 4) s += raw(t, c);
        part[ph][tid & 63] = s;
        __syncthreads();
        if (tid < 64 && c0 + tid < nc) mean[c0 + tid] = a.cmn && T > 0 ? (part[0][tid] + part[1][tid] + part[2][tid] + part[3][tid]) / (float)T : 0.0f;
        __syncthreads();
    }
    int mask_len = T;
    if (a.lens_ratio != nullptr) mask_len = (int)rintf(a.lens_ratio[b] * (float)T);
    for (int i = tid; i < a.T * nc; i += MFCC_THREADS) {
        const int t = i / nc, c = i - t * nc;
        MV_AS_GLOBAL(float, orow)[i] = t < mask_len ? raw(t, c) - mean[c] : 0.0f;
    }
}

}  // namespace mv

struct MvSpectrogram {
    MvMelSpec* core = nullptr;
};

struct MvMfcc {
    MvMfccCfg cfg;
    MvMelSpec* mel = nullptr;
    float* d_dct = nullptr;   // [n_mels][n_mfcc]
    bool dct_lds = false;
};

namespace {

size_t align256(size_t n) { return (n + 255) & ~(size_t)255; }

// the caller workspace of an MFCC forward: the mel stage's own workspace, behind it the mel stage's output [B, T, n_mels] and the per-utterance
// maxima [B]; every section starts on a multiple of 256 bytes
struct MfccWorkspace {
    size_t mel, rowmax, total;   // offsets of the last two sections (mel = the bytes of the first), bytes in all
};

MfccWorkspace mfcc_workspace(const MvMfcc* h, int32_t B, int64_t L) {
    int64_t T = 0;
    mv_melspec_num_frames(h->mel, L, &T);
    MfccWorkspace w;
    w.mel = align256(mv_melspec_workspace_bytes(h->mel, B, L));
    w.rowmax = w.mel + align256((size_t)B * (size_t)T * h->cfg.mel.n_mels * sizeof(float));
    w.total = w.rowmax + align256((size_t)B * sizeof(float));
    return w;
}

}  // namespace

extern "C" {

void mv_spectrogram_default_cfg(MvSpectrogramCfg* cfg) {
    cfg->n_fft = 400;
    cfg->win_length = 400;
    cfg->hop_length = 200;
    cfg->pad = 0;
    cfg->power = 2.0f;
    cfg->normalized = MV_STFT_NORM_NONE;
    cfg->center = 1;
    cfg->pad_mode = MV_STFT_PAD_REFLECT;
    cfg->subtract_time_mean = 1;
    cfg->window = nullptr;
}

int mv_spectrogram_create(const MvSpectrogramCfg* cfg, MvSpectrogram** out) {
    MV_REQUIRE(cfg != nullptr && out != nullptr, "mv_spectrogram_create: null argument");
    MvMelSpecCfg m;
    mv_melspec_default_cfg(&m);
    m.n_fft = cfg->n_fft;
    m.win_length = cfg->win_length;
    m.hop_length = cfg->hop_length;
    m.pad = cfg->pad;
    m.power = cfg->power;
    m.normalized = cfg->normalized;
    m.center = cfg->center ? 1 : 0;
    m.pad_mode = cfg->pad_mode;
    m.subtract_time_mean = cfg->subtract_time_mean ? 1 : 0;
    m.window = cfg->window;
    m.n_mels = 1;   // (no mel stage in spectrogram mode)
    std::unique_ptr<MvSpectrogram> h(new MvSpectrogram());
    const int rc = mv::melspec_create_mode(&m, true, &h->core);   // (checks the fields above under this call's name)
    if (rc != MV_OK) return rc;
    *out = h.release();
    return MV_OK;
}

int mv_spectrogram_info(const MvSpectrogram* h, int32_t* kernel) {
    MV_REQUIRE(h != nullptr && kernel != nullptr, "mv_spectrogram_info: null argument");
    return mv_melspec_info(h->core, kernel);
}

int mv_spectrogram_destroy(MvSpectrogram* h) {
    if (h == nullptr) return MV_OK;
    mv_melspec_destroy(h->core);
    delete h;
    return MV_OK;
}

int mv_spectrogram_num_frames(const MvSpectrogram* h, int64_t num_samples, int64_t* num_frames) {
    MV_REQUIRE(h != nullptr && num_frames != nullptr, "mv_spectrogram_num_frames: null argument");
    return mv_melspec_num_frames(h->core, num_samples, num_frames);
}

size_t mv_spectrogram_workspace_bytes(const MvSpectrogram* h, int32_t B, int64_t L) {
    return h == nullptr ? 0 : mv_melspec_workspace_bytes(h->core, B, L);
}

int mv_spectrogram_forward(const MvSpectrogram* h, const float* wav, int32_t B, int64_t L, int64_t wav_stride,
                           const float* lens_ratio, float* out, void* workspace, size_t workspace_bytes, mv_stream_t stream) {
    MV_REQUIRE(h != nullptr, "mv_spectrogram_forward: null handle");
    return mv_melspec_forward(h->core, wav, B, L, wav_stride, lens_ratio, out, workspace, workspace_bytes, stream);
}

int mv_spectrogram_forward_varlen(const MvSpectrogram* h, const float* wav, int32_t B, int64_t L, int64_t wav_stride,
                                  const int64_t* num_samples, float* out, void* workspace, size_t workspace_bytes, mv_stream_t stream) {
    MV_REQUIRE(h != nullptr, "mv_spectrogram_forward_varlen: null handle");
    MV_REQUIRE(num_samples != nullptr, "mv_spectrogram_forward_varlen: null length array");
    return mv_melspec_forward_varlen(h->core, wav, B, L, wav_stride, num_samples, out, workspace, workspace_bytes, stream);
}

void mv_mfcc_default_cfg(MvMfccCfg* cfg) {
    mv_melspec_default_cfg(&cfg->mel);
    cfg->mel.subtract_time_mean = 0;
    cfg->n_mfcc = 40;
    cfg->dct_norm = MV_DCT_NORM_ORTHO;
    cfg->log_mels = 0;
    cfg->top_db = 80.0f;
    cfg->subtract_time_mean = 1;
}

int mv_mfcc_create(const MvMfccCfg* cfg, MvMfcc** out) {
    MV_REQUIRE(cfg != nullptr && out != nullptr, "mv_mfcc_create: null argument");
    MV_REQUIRE(cfg->n_mfcc >= 1, "mv_mfcc_create: n_mfcc must be positive");
    MV_REQUIRE(cfg->n_mfcc <= cfg->mel.n_mels, "mv_mfcc_create: Cannot select more MFCC coefficients than # mel bins");
    MV_REQUIRE(cfg->dct_norm == MV_DCT_NORM_NONE || cfg->dct_norm == MV_DCT_NORM_ORTHO, "mv_mfcc_create: norm must be None or 'ortho'");
    MV_REQUIRE(cfg->log_mels == 0 || cfg->log_mels == 1, "mv_mfcc_create: log_mels must be 0 or 1");
    MV_REQUIRE(cfg->top_db >= 0.0f && cfg->top_db < 1e30f, "mv_mfcc_create: top_db must be a non-negative finite value");
    std::unique_ptr<MvMfcc, decltype(&mv_mfcc_destroy)> h(new MvMfcc(), mv_mfcc_destroy);   // (every early return destroys it)
    h->cfg = *cfg;
    h->cfg.mel.window = nullptr;   // (read by the mel stage's create, not kept)
    MvMelSpecCfg m = cfg->mel;
    m.subtract_time_mean = 0;
    int rc = mv::melspec_create_mode(&m, false, &h->mel);
    if (rc != MV_OK) return rc;
    // torchaudio.functional.create_dct(n_mfcc, n_mels, norm): dct[m][k] = cos(pi / n_mels * (m + 0.5) * k), 'ortho' scales column 0 by
    // 1 / sqrt(2) and everything by sqrt(2 / n_mels), None everything by 2
    const int nm = cfg->mel.n_mels, nc = cfg->n_mfcc;
    const double pi = 3.14159265358979323846;
    std::vector<float> dct((size_t)nm * nc);
    for (int mm = 0; mm < nm; ++mm)
        for (int k = 0; k < nc; ++k) {
            double v = cos(pi / nm * (mm + 0.5) * k);
            if (cfg->dct_norm == MV_DCT_NORM_ORTHO) v *= (k == 0 ? 1.0 / sqrt(2.0) : 1.0) * sqrt(2.0 / nm);
            else v *= 2.0;
            dct[(size_t)mm * nc + k] = (float)v;
        }
    hipError_t e = hipMalloc(reinterpret_cast<void**>(&h->d_dct), dct.size() * sizeof(float));
    if (e == hipSuccess) e = hipMemcpy(h->d_dct, dct.data(), dct.size() * sizeof(float), hipMemcpyHostToDevice);
    if (e != hipSuccess) return mv::fail(MV_ERR_HIP, std::string("mv_mfcc_create: ") + hipGetErrorString(e));
    h->dct_lds = nm * nc <= mv::MFCC_DCT_LDS_MAX;
    if ((h->dct_lds ? MV_SET_MAX_SMEM(mv::mfcc_dct_kernel<true>, (int)mv::MFCC_LDS) : MV_SET_MAX_SMEM(mv::mfcc_dct_kernel<false>, (int)mv::MFCC_LDS)) != hipSuccess)
        return mv::fail(MV_ERR_HIP, "mv_mfcc_create: cannot reserve dynamic LDS for mfcc_dct_kernel");
    *out = h.release();
    return MV_OK;
}

int mv_mfcc_info(const MvMfcc* h, int32_t* mel_kernel, int32_t* dct_lds) {
    MV_REQUIRE(h != nullptr && mel_kernel != nullptr && dct_lds != nullptr, "mv_mfcc_info: null argument");
    *dct_lds = h->dct_lds ? 1 : 0;
    return mv_melspec_info(h->mel, mel_kernel);
}

int mv_mfcc_destroy(MvMfcc* h) {
    if (h == nullptr) return MV_OK;
    mv_melspec_destroy(h->mel);
    hipFree(h->d_dct);
    delete h;
    return MV_OK;
}

int mv_mfcc_num_frames(const MvMfcc* h, int64_t num_samples, int64_t* num_frames) {
    MV_REQUIRE(h != nullptr && num_frames != nullptr, "mv_mfcc_num_frames: null argument");
    return mv_melspec_num_frames(h->mel, num_samples, num_frames);
}

size_t mv_mfcc_workspace_bytes(const MvMfcc* h, int32_t B, int64_t L) {
    return h == nullptr || B <= 0 ? 0 : mfcc_workspace(h, B, L).total;
}

static int mfcc_forward_rows(const MvMfcc* h, const float* wav, int32_t B, int64_t L, int64_t wav_stride, const float* lens_ratio,
                             const int64_t* num_samples, float* out, void* workspace, size_t workspace_bytes, mv_stream_t stream);

int mv_mfcc_forward(const MvMfcc* h, const float* wav, int32_t B, int64_t L, int64_t wav_stride,
                    const float* lens_ratio, float* out, void* workspace, size_t workspace_bytes, mv_stream_t stream) {
    return mfcc_forward_rows(h, wav, B, L, wav_stride, lens_ratio, nullptr, out, workspace, workspace_bytes, stream);
}

int mv_mfcc_forward_varlen(const MvMfcc* h, const float* wav, int32_t B, int64_t L, int64_t wav_stride,
                           const int64_t* num_samples, float* out, void* workspace, size_t workspace_bytes, mv_stream_t stream) {
    MV_REQUIRE(num_samples != nullptr, "mv_mfcc_forward_varlen: null length array");
    return mfcc_forward_rows(h, wav, B, L, wav_stride, nullptr, num_samples, out, workspace, workspace_bytes, stream);
}

// both forms: lens_ratio (batch form, or neither) or num_samples (variable-length form: own frames, time mean and dB floor per row)
static int mfcc_forward_rows(const MvMfcc* h, const float* wav, int32_t B, int64_t L, int64_t wav_stride, const float* lens_ratio,
                             const int64_t* num_samples, float* out, void* workspace, size_t workspace_bytes, mv_stream_t stream) {
    MV_REQUIRE(h != nullptr, "mv_mfcc_forward: null handle");
    MV_REQUIRE(B >= 0 && L >= 0 && wav_stride >= L, "mv_mfcc_forward: bad batch geometry");
    MV_REQUIRE(lens_ratio == nullptr || num_samples == nullptr, "mv_mfcc_forward: lens_ratio and num_samples are mutually exclusive");
    int64_t T = 0;
    mv_melspec_num_frames(h->mel, L, &T);
    if (B == 0 || T == 0) return MV_OK;
    MV_REQUIRE(wav != nullptr && out != nullptr && workspace != nullptr, "mv_mfcc_forward: null buffer");
    MV_REQUIRE((reinterpret_cast<uintptr_t>(workspace) & 15) == 0, "mv_mfcc_forward: workspace must be 16-byte aligned");
    const MfccWorkspace sec = mfcc_workspace(h, B, L);
    MV_REQUIRE(workspace_bytes >= sec.total, "mv_mfcc_forward: workspace too small (mv_mfcc_workspace_bytes)");
    MV_REQUIRE((int64_t)T * h->cfg.mel.n_mels < ((int64_t)1 << 31) && (int64_t)T * h->cfg.n_mfcc < ((int64_t)1 << 31), "mv_mfcc_forward: too many frames");
    char* ws = static_cast<char*>(workspace);
    float* mel = reinterpret_cast<float*>(ws + sec.mel);
    float* rowmax = reinterpret_cast<float*>(ws + sec.rowmax);
    int rc = mv::melspec_forward_rows(h->mel, wav, B, L, wav_stride, nullptr, num_samples, mel, ws, sec.mel, stream);
    if (rc != MV_OK) return rc;
    const mv::RowLens row_lens = mv::melspec_row_lens(h->mel, num_samples, L);
    hipStream_t st = static_cast<hipStream_t>(stream);
    const int nm = h->cfg.mel.n_mels, nc = h->cfg.n_mfcc;
    if (!h->cfg.log_mels) {
        MV_LAUNCH(mv::mfcc_db_max_kernel, ((unsigned)B, 1, 1), (mv::MFCC_THREADS, 1, 1), 0, st, mel, (int)T, nm, row_lens, rowmax);
        rc = mv::check_launch("mfcc_db_max_kernel");
        if (rc != MV_OK) return rc;
    }
    mv::MfccArgs a;
    a.mel = mel; a.rowmax = rowmax; a.dct = h->d_dct; a.lens_ratio = lens_ratio; a.out = out;
    a.B = B; a.T = (int)T; a.n_mels = nm; a.n_mfcc = nc; a.log_mels = h->cfg.log_mels; a.cmn = h->cfg.subtract_time_mean ? 1 : 0;
    a.top_db = h->cfg.top_db;
    a.rows = row_lens;
    const size_t fixed = ((h->dct_lds ? (size_t)((nm * nc + 3) & ~3) : 0) + (size_t)mv::MFCC_FR * nm) * sizeof(float);
    const int64_t rows = (int64_t)((mv::MFCC_LDS - fixed) / ((size_t)nc * sizeof(float)));
    a.tile_rows = (int)(rows < T ? rows : T);
    const size_t smem = fixed + (size_t)a.tile_rows * nc * sizeof(float);
    if (h->dct_lds) MV_LAUNCH(mv::mfcc_dct_kernel<true>, ((unsigned)B, 1, 1), (mv::MFCC_THREADS, 1, 1), smem, st, a);
    else MV_LAUNCH(mv::mfcc_dct_kernel<false>, ((unsigned)B, 1, 1), (mv::MFCC_THREADS, 1, 1), smem, st, a);
    return mv::check_launch("mfcc_dct_kernel");
}

}  // extern "C"
