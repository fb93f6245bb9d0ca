/* libmvector_hip.so -- C ABI of the MI355X-native (gfx950) embedding-extraction hot path.
 *
 * The reference (yeyupiaoling/VoiceprintRecognition-Pytorch, mvector 1.1.1) is pure Python and has
 * NO native / FFI / operator boundary for this path (setup.py:56 ``ext_modules=[]``), so there is no
 * reference FFI to mirror symbol-for-symbol.  The drop-in boundary is the Python surface
 * (AudioFeaturizer / build_model / model classes / MVectorPredictor); this header is the C ABI that a
 * maintainer binds UNDER that surface (ctypes stub shown in INTEGRATION.md).  Each entry point cites
 * the reference code whose device work it replaces.
 *
 * Conventions
 *   - plain pointers and sizes only; every data pointer is a DEVICE pointer on the current HIP
 *     device unless its name ends in ``_host``;
 *   - the caller (PyTorch) owns inputs, outputs and workspaces; handles own only derived constants
 *     (window / filterbank tables, pre-packed fp16 weights) allocated at create time;
 *   - stream-ordered: work is enqueued on ``stream`` (a hipStream_t passed as void*), nothing in a
 *     ``*_forward`` call synchronises the device; ``*_create`` / ``*_destroy`` may synchronise;
 *   - every function returns MV_OK (0) or a negative MV_ERR_* code and records a message readable
 *     through mv_last_error() (thread-local).  Handles are immutable after create, so forwards on
 *     different streams with different workspaces may run concurrently.
 */
#ifndef MVECTOR_HIP_H
#define MVECTOR_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif
/* The library is built with -fvisibility=hidden: the entry points declared in this header are its ONLY dynamic exports besides the HIP
 * runtime's kernel handles (tests/test_native_library.py checks `nm -D` against this list). */
#if defined(__GNUC__)
#pragma GCC visibility push(default)
#endif

#define MV_OK 0
#define MV_ERR_INVALID_ARGUMENT (-1)
#define MV_ERR_HIP (-2)
#define MV_ERR_UNSUPPORTED (-3)
#define MV_ERR_WORKSPACE (-4)
#define MV_ERR_MISSING_TENSOR (-5)
#define MV_ERR_NOT_CONVERGED (-6) /* mv_laplacian_eig_lowest ran out of iterations; MvEigInfo carries the residual */

#define MV_ABI_VERSION 5

typedef void* mv_stream_t; /* hipStream_t */

const char* mv_last_error(void);
int mv_abi_version(void);

/* ------------------------------------------------------------------------------------------------
 * Front-end 1: Kaldi log-mel filterbank + per-utterance time-mean subtraction + length mask.
 * Replaces KaldiFbank.forward (mvector/data_utils/featurizer.py:119-132 ->
 * torchaudio.compliance.kaldi.fbank) fused with AudioFeaturizer.forward's normalisation and mask
 * (featurizer.py:77-90).  Arithmetic as restated in oracle/frontend.py::kaldi_fbank.
 * ------------------------------------------------------------------------------------------------ */
typedef struct MvFbankCfg {
    float sample_frequency;       /* 16000 */
    float frame_length_ms;        /* 25 */
    float frame_shift_ms;         /* 10 */
    int32_t num_mel_bins;         /* 80 (4 .. 128: torchaudio's get_mel_banks asserts num_bins > 3) */
    float low_freq;               /* 20 (0 <= low_freq < Nyquist, low_freq < high_freq: refused otherwise, as get_mel_banks asserts) */
    float high_freq;              /* 0 => Nyquist (+ high_freq if <= 0, as Kaldi); beyond Nyquist: refused (get_mel_banks asserts) */
    float preemphasis_coefficient;/* 0.97 */
    int32_t remove_dc_offset;     /* 1 */
    int32_t use_power;            /* 1 */
    int32_t use_log_fbank;        /* 1 */
    int32_t subtract_time_mean;   /* 1: featurizer.py:79 (mean over ALL frames, padded ones included) */
    /* ---- since ABI 4: the further kaldi.fbank keyword arguments featurizer.py:128 forwards (**kwargs) ---- */
    int32_t window_type;          /* MV_WINDOW_POVEY (0) | HAMMING | HANNING | RECTANGULAR | BLACKMAN */
    float blackman_coeff;         /* 0.42 (window_type BLACKMAN only) */
    int32_t snip_edges;           /* 1: frames lie inside the signal.  0: T = (L + shift / 2) / shift frames, the signal mirrored at both ends
                                   * (needs the caller workspace of mv_fbank_forward_ws: the mirrored rows are written there first) */
    int32_t subtract_mean;        /* 0.  kaldi.fbank's own subtract_mean: column means over the utterance's frames, BEFORE the wrapper's mean */
    float min_duration;           /* 0 s: shorter signals give no frames */
    float vtln_warp;              /* 1.0 = no vocal-tract-length warp of the filter edges; otherwise kaldi's 3-piece linear warp between */
    float vtln_low, vtln_high;    /* 100, -500 (negative: + Nyquist) */
    int32_t kernel;               /* MV_FBANK_KERNEL_AUTO (0) | MV_FBANK_KERNEL_GENERIC (fbank_kernel) | MV_FBANK_KERNEL_TILE (fbank_tile_kernel;
                                   * create fails when the mel geometry has no instantiation).  Both kernels implement the same contract; the
                                   * field exists so that tests and tools/bench_fbank.py can run either on any geometry. */
    /* ---- since ABI 5 ---- */
    int64_t min_samples;          /* > 0: the threshold of min_duration in SAMPLES, ceil(min_duration * sample_frequency) evaluated by the caller in
                                   * double as torchaudio compares (`len(waveform) < min_duration * sample_frequency`): the float32 field above
                                   * rounds 0.1 / 0.2 / 0.3 s upwards and a clip of exactly min_duration lost its frames.  0: derived
                                   * from min_duration. */
    int32_t use_energy;           /* 0.  1: one more column, the log energy of every frame -- out is [B, T, num_mel_bins + 1] (kaldi.fbank's use_energy;
                                   * AudioFeaturizer.feature_dim, featurizer.py:110-111, keeps reporting num_mel_bins, as the reference's does).  The
                                   * mel columns come from the same kernels through the caller workspace (mv_fbank_workspace_bytes; the forwards
                                   * without a workspace refuse), the energy column from fbank_energy_kernel; time mean and mask cover it too. */
    int32_t raw_energy;           /* 1: energy of the frame after the DC removal, before pre-emphasis and window; 0: of the windowed frame */
    float energy_floor;           /* 1.0: log energies below log(energy_floor) are raised to it; 0 = no floor (kaldi.fbank's rule) */
    int32_t htk_compat;           /* 0: the energy is column 0; 1: the last column */
} MvFbankCfg;

enum { MV_WINDOW_POVEY = 0, MV_WINDOW_HAMMING = 1, MV_WINDOW_HANNING = 2, MV_WINDOW_RECTANGULAR = 3, MV_WINDOW_BLACKMAN = 4 };
enum { MV_FBANK_KERNEL_AUTO = 0, MV_FBANK_KERNEL_GENERIC = 1, MV_FBANK_KERNEL_TILE = 2 };

typedef struct MvFbank MvFbank;

void mv_fbank_default_cfg(MvFbankCfg* cfg);
int mv_fbank_create(const MvFbankCfg* cfg, MvFbank** out);
int mv_fbank_destroy(MvFbank* h);
/* T = 1 + (L - window) / shift, or 0 when L < window (snip_edges = 1); (L + shift / 2) / shift (snip_edges = 0); 0 below min_duration */
int mv_fbank_num_frames(const MvFbank* h, int64_t num_samples, int64_t* num_frames);
/* which kernel this handle launches: *tile_kernel = 1 for fbank_tile_kernel (mel geometry of the reference configurations:
 * 80 bins / 16 kHz / 512-point FFT), 0 for the generic fbank_kernel; pass_steps[2] = FFT bins each mel MFMA pass walks */
int mv_fbank_info(const MvFbank* h, int32_t* tile_kernel, int32_t* pass_steps);
/* wav: [B, L] fp32 rows ``wav_stride`` elements apart.  lens_ratio: [B] fp32 or NULL
 * (featurizer.py:80-90: frames t >= round_half_even(ratio * T) are zeroed).  out: [B, T, num_mel_bins]
 * fp32, contiguous ([B, T, num_mel_bins + 1] with MvFbankCfg.use_energy, which needs mv_fbank_forward_ws). */
int mv_fbank_forward(const MvFbank* h, const float* wav, int32_t B, int64_t L, int64_t wav_stride,
                     const float* lens_ratio, float* out, mv_stream_t stream);
/* The same forward with a caller workspace.  A batch of fewer utterances than the chip has CUs (predict()'s single utterance,
 * predict_batch()'s 32) is faster as several workgroups per utterance + a finish pass; that form needs per-CALL scratch for the
 * column sums of every 4-frame group, which the handle must not own (two forwards on two streams share the handle).
 * mv_fbank_workspace_bytes reports what this (B, L) needs on the current device (0 = none); `workspace` must be 16-byte aligned
 * and stay untouched until the forward has run on `stream`.  With a NULL or short workspace -- and in mv_fbank_forward /
 * mv_fbank_forward_varlen -- every utterance runs on one workgroup.  The two forms produce IDENTICAL bits: the time mean of an
 * utterance is summed in one fixed order (csrc/fbank.hip, FbankArgs) that depends on its own length only, never on the batch
 * size, the form or the stream. */
int mv_fbank_workspace_bytes(const MvFbank* h, int32_t B, int64_t L, size_t* bytes);
int mv_fbank_forward_ws(const MvFbank* h, const float* wav, int32_t B, int64_t L, int64_t wav_stride, const float* lens_ratio,
                        float* out, void* workspace, size_t workspace_bytes, mv_stream_t stream);

/* Variable-length batch: row b holds num_samples[b] <= L valid samples (device array, int64).  Every utterance is
 * featurised on its own -- frame count, time mean -- and rows beyond its frame count are zero in the [B, T(L), F] output:
 * the result of the reference's evaluation path, which featurises per utterance (mvector/data_utils/reader.py:100-106)
 * and zero-pads the features (collate_fn.py:11-19). */
int mv_fbank_forward_varlen(const MvFbank* h, const float* wav, int32_t B, int64_t L, int64_t wav_stride,
                            const int64_t* num_samples, float* out, mv_stream_t stream);
/* the same with the caller workspace of mv_fbank_workspace_bytes(h, B, L): what snip_edges = 0 handles need (the mirrored rows) */
int mv_fbank_forward_varlen_ws(const MvFbank* h, const float* wav, int32_t B, int64_t L, int64_t wav_stride, const int64_t* num_samples,
                               float* out, void* workspace, size_t workspace_bytes, mv_stream_t stream);

/* ------------------------------------------------------------------------------------------------
 * Front-end 2: MelSpectrogram (power STFT, centre/reflect padding, HTK mel filterbank, NO log) +
 * time-mean subtraction + mask.  Replaces torchaudio.transforms.MelSpectrogram(**method_args)
 * (featurizer.py:41-42) and featurizer.py:77-90.  Oracle: oracle/frontend.py::mel_spectrogram.
 * ------------------------------------------------------------------------------------------------ */
typedef struct MvMelSpecCfg {
    int32_t sample_rate; /* 16000 */
    int32_t n_fft;       /* 400 */
    int32_t win_length;  /* 400 (<= n_fft) */
    int32_t hop_length;  /* 200 */
    float f_min;         /* 0 */
    float f_max;         /* sample_rate / 2 */
    int32_t n_mels;      /* 128 */
    float power;         /* 2.0; any positive exponent of |X| (the FFT kernels take 2, the dense-DFT kernel every other one) */
    int32_t center;      /* 1 */
    int32_t subtract_time_mean;
    /* ---- since ABI 4: further MelSpectrogram(**method_args) keyword arguments (featurizer.py:41-42), all of them tables ---- */
    int32_t mel_scale;   /* MV_MEL_HTK (0) | MV_MEL_SLANEY */
    int32_t norm;        /* 0 = None | MV_MEL_NORM_SLANEY (1): filter j times 2 / (f[j + 2] - f[j]) */
    int32_t normalized;  /* 0 = False | MV_STFT_NORM_WINDOW (1; True): spectrum / sqrt(sum window^2) | MV_STFT_NORM_FRAME_LENGTH (2): / sqrt(n_fft) */
    const float* window; /* NULL = periodic Hann | HOST array [win_length]: what window_fn(win_length, **wkwargs) returned (copied at create) */
    /* ---- since ABI 5 ---- */
    int32_t pad;         /* 0.  Zeros in front of and behind the signal before the transform (torchaudio.functional.spectrogram's `pad`) */
    int32_t pad_mode;    /* MV_STFT_PAD_REFLECT (0) | CONSTANT | REPLICATE | CIRCULAR: how torch.stft(center=True) extends the signal by n_fft / 2.
                          * pad > 0 or a mode other than reflect writes the extended signal to the caller workspace first (one more pass over the
                          * waveform for a non-default argument); the transform kernels then run on it unchanged */
} MvMelSpecCfg;

enum { MV_STFT_PAD_REFLECT = 0, MV_STFT_PAD_CONSTANT = 1, MV_STFT_PAD_REPLICATE = 2, MV_STFT_PAD_CIRCULAR = 3 };

enum { MV_MEL_HTK = 0, MV_MEL_SLANEY = 1 };
enum { MV_MEL_NORM_NONE = 0, MV_MEL_NORM_SLANEY = 1 };
enum { MV_STFT_NORM_NONE = 0, MV_STFT_NORM_WINDOW = 1, MV_STFT_NORM_FRAME_LENGTH = 2 };

typedef struct MvMelSpec MvMelSpec;

void mv_melspec_default_cfg(MvMelSpecCfg* cfg);
int mv_melspec_create(const MvMelSpecCfg* cfg, MvMelSpec** out);
/* *tile_kernel = 1 when the handle launches melspec_tile_kernel (n_fft = 400 as a real FFT fused with mel + CMN + mask in one
 * launch), 0 for the dense-DFT kernels (any other geometry) */
int mv_melspec_info(const MvMelSpec* h, int32_t* tile_kernel);
int mv_melspec_destroy(MvMelSpec* h);
int mv_melspec_num_frames(const MvMelSpec* h, int64_t num_samples, int64_t* num_frames);
size_t mv_melspec_workspace_bytes(const MvMelSpec* h, int32_t B, int64_t L);
int mv_melspec_forward(const MvMelSpec* h, const float* wav, int32_t B, int64_t L, int64_t wav_stride,
                       const float* lens_ratio, float* out, void* workspace, size_t workspace_bytes,
                       mv_stream_t stream);
/* Variable-length batch (additive since ABI 5; also mv_spectrogram_forward_varlen and mv_mfcc_forward_varlen below): row b holds
 * n_b = clamp(num_samples[b], 0, L) valid samples (device array, int64, B entries; NULL is refused).  Row b is featurised exactly as the
 * same handle's forward featurises it alone as a [1, n_b] batch without a ratio, and BIT FOR BIT so -- the reference's evaluation path,
 * which featurises per utterance (mvector/data_utils/reader.py:100-106) and zero-pads the features (collate_fn.py:11-19):
 *   - T_b = what *_num_frames(h, n_b) returns; the output keeps the shape [B, T(L), F] and its rows t >= T_b are zero;
 *   - the samples behind n_b are never read into a result;
 *   - centre padding takes the mirror / edge value / wrap-around / zeros at n_b (every pad_mode, and pad > 0), center = 0 frames lie inside n_b;
 *   - the time mean is taken over the row's T_b frames, summed in an order that depends on T_b alone (not on T(L), B or the stream);
 *   - MFCC with log_mels = 0: the dB floor is (the ROW's loudest value) - top_db.  The batch coupling of mv_mfcc_forward stays as it is.
 * A row the reference cannot featurise -- torch.stft raises (n_b + 2 pad <= n_fft / 2 under reflect, < n_fft / 2 under circular padding),
 * there is nothing to pad (n_b + 2 pad == 0, any pad_mode), or no frame fits (n_b + 2 pad < n_fft with center = 0) -- yields an all-zero row
 * and no fault, whatever subtract_time_mean says; the reference's dataset skips such items.
 * The geometry checks are those of the forward on (B, L); the workspace is the one mv_*_workspace_bytes(h, B, L) reports. */
int mv_melspec_forward_varlen(const MvMelSpec* h, const float* wav, int32_t B, int64_t L, int64_t wav_stride,
                              const int64_t* num_samples, float* out, void* workspace, size_t workspace_bytes,
                              mv_stream_t stream);

/* ------------------------------------------------------------------------------------------------
 * Front-end 3: Spectrogram (power STFT, the linear-frequency bins are the features) + time-mean
 * subtraction + mask.  Replaces torchaudio.transforms.Spectrogram(**method_args) (featurizer.py:43-44)
 * and featurizer.py:77-90.  Output [B, T, n_fft / 2 + 1].  The STFT fields mean what they mean in
 * MvMelSpecCfg.  n_fft = 400: one launch (melspec_tile_kernel's FFT); any other n_fft: dense DFT +
 * cmn_mask_kernel.  Additive since ABI 5.
 * ------------------------------------------------------------------------------------------------ */
typedef struct MvSpectrogramCfg {
    int32_t n_fft;       /* 400 */
    int32_t win_length;  /* 400 (<= n_fft) */
    int32_t hop_length;  /* 200 */
    int32_t pad;         /* 0 */
    float power;         /* 2.0; any positive exponent of |X| (power=None, the complex spectrogram, is refused) */
    int32_t normalized;  /* MV_STFT_NORM_* */
    int32_t center;      /* 1 */
    int32_t pad_mode;    /* MV_STFT_PAD_* */
    int32_t subtract_time_mean; /* 1 */
    const float* window; /* NULL = periodic Hann | HOST array [win_length] (copied at create) */
} MvSpectrogramCfg;

typedef struct MvSpectrogram MvSpectrogram;

void mv_spectrogram_default_cfg(MvSpectrogramCfg* cfg);
int mv_spectrogram_create(const MvSpectrogramCfg* cfg, MvSpectrogram** out);
/* *kernel = 1 for the fused n_fft = 400 launch, 0 for the dense DFT */
int mv_spectrogram_info(const MvSpectrogram* h, int32_t* kernel);
int mv_spectrogram_destroy(MvSpectrogram* h);
int mv_spectrogram_num_frames(const MvSpectrogram* h, int64_t num_samples, int64_t* num_frames);
size_t mv_spectrogram_workspace_bytes(const MvSpectrogram* h, int32_t B, int64_t L);
int mv_spectrogram_forward(const MvSpectrogram* h, const float* wav, int32_t B, int64_t L, int64_t wav_stride,
                           const float* lens_ratio, float* out, void* workspace, size_t workspace_bytes,
                           mv_stream_t stream);
/* every row on its own length: the semantics of mv_melspec_forward_varlen */
int mv_spectrogram_forward_varlen(const MvSpectrogram* h, const float* wav, int32_t B, int64_t L, int64_t wav_stride,
                                  const int64_t* num_samples, float* out, void* workspace, size_t workspace_bytes,
                                  mv_stream_t stream);

/* ------------------------------------------------------------------------------------------------
 * Front-end 4: MFCC (mel power -> dB with a top_db floor, or log(mel + 1e-6) -> DCT-II) + time-mean
 * subtraction + mask.  Replaces torchaudio.transforms.MFCC(**method_args) and featurizer.py:77-90.
 * Output [B, T, n_mfcc].  With log_mels = 0 the floor is (max dB over the WHOLE batch of the call)
 * - top_db, as torchaudio's amplitude_to_DB on a [B, n_mels, T] tensor: a row's features depend on
 * the other rows of the call.  The batch max stays on the device (no host synchronisation).
 * Additive since ABI 5.
 * ------------------------------------------------------------------------------------------------ */
enum { MV_DCT_NORM_NONE = 0, MV_DCT_NORM_ORTHO = 1 };

typedef struct MvMfccCfg {
    MvMelSpecCfg mel;    /* the mel stage (subtract_time_mean is ignored: the mean is taken of the coefficients) */
    int32_t n_mfcc;      /* 40, <= mel.n_mels */
    int32_t dct_norm;    /* MV_DCT_NORM_ORTHO (1) | MV_DCT_NORM_NONE */
    int32_t log_mels;    /* 0 */
    float top_db;        /* 80 (>= 0) */
    int32_t subtract_time_mean; /* 1 */
} MvMfccCfg;

typedef struct MvMfcc MvMfcc;

void mv_mfcc_default_cfg(MvMfccCfg* cfg);
int mv_mfcc_create(const MvMfccCfg* cfg, MvMfcc** out);
/* *mel_kernel = what mv_melspec_info reports for the mel stage; *dct_lds = 1 when the DCT table is held in LDS */
int mv_mfcc_info(const MvMfcc* h, int32_t* mel_kernel, int32_t* dct_lds);
int mv_mfcc_destroy(MvMfcc* h);
int mv_mfcc_num_frames(const MvMfcc* h, int64_t num_samples, int64_t* num_frames);
size_t mv_mfcc_workspace_bytes(const MvMfcc* h, int32_t B, int64_t L);
int mv_mfcc_forward(const MvMfcc* h, const float* wav, int32_t B, int64_t L, int64_t wav_stride,
                    const float* lens_ratio, float* out, void* workspace, size_t workspace_bytes,
                    mv_stream_t stream);
/* every row on its own length, its own dB floor included: the semantics of mv_melspec_forward_varlen */
int mv_mfcc_forward_varlen(const MvMfcc* h, const float* wav, int32_t B, int64_t L, int64_t wav_stride,
                           const int64_t* num_samples, float* out, void* workspace, size_t workspace_bytes,
                           mv_stream_t stream);

/* ------------------------------------------------------------------------------------------------
 * Front-end 5: a HuggingFace Wav2Vec2 / WavLM model's `extract_features` + time-mean subtraction + mask.  Replaces
 * AudioFeaturizer(use_hf_model=True) (featurizer.py:20-39: AutoModel + AutoFeatureExtractor; forward :60-76 keeps
 * outputs.extract_features alone) and featurizer.py:77-90.  What is evaluated: the processor's per-row z-score
 * (x - mean) / sqrt(var + 1e-7) over the whole padded row (do_normalize; over the row's own samples in mv_hfenc_forward_varlen), the convolutional feature encoder
 * (feature_extractor.conv_layers.*: unpadded strided Conv1d -> GroupNorm on layer 0 ("group") or LayerNorm on every layer
 * ("layer") -> exact GELU) and feature_projection.layer_norm; the transformer behind them, whose output the reference
 * discards, is not.  Layer 0 runs in exact fp32; the other layers are fp16-operand convolutions on channel-last fp16
 * activations (csrc/hfencoder.hip).  Output [B, T', conv_dim[last]] fp32.  Additive since ABI 5.
 * ------------------------------------------------------------------------------------------------ */
#define MV_HFENC_MAX_LAYERS 8
#define MV_HF_NORM_GROUP 0
#define MV_HF_NORM_LAYER 1
#define MV_ACT_GELU 4 /* exact (erf) GELU: the only feat_extract_activation the encoder is built for (not an MvConv1dDesc activation) */
typedef struct MvHfEncoderCfg {
    int32_t num_layers;                         /* 7; 1 .. MV_HFENC_MAX_LAYERS */
    int32_t conv_dim[MV_HFENC_MAX_LAYERS];      /* {512 x 7}: multiples of 64 up to 1024 (other widths are refused by name) */
    int32_t conv_kernel[MV_HFENC_MAX_LAYERS];   /* {10,3,3,3,3,2,2}; layer 0: <= 16 */
    int32_t conv_stride[MV_HFENC_MAX_LAYERS];   /* {5,2,2,2,2,2,2}; layer 0: <= 8 */
    int32_t feat_extract_norm;                  /* MV_HF_NORM_GROUP | MV_HF_NORM_LAYER */
    int32_t conv_bias;                          /* 0 | 1: conv_layers.i.conv.bias */
    int32_t do_normalize;                       /* the processor's z-score of every waveform row */
    int32_t activation;                         /* MV_ACT_GELU; anything else is refused */
    float layer_norm_eps;                       /* of feature_projection.layer_norm (config.layer_norm_eps, 1e-5); the encoder's own norms use 1e-5 */
    int32_t subtract_time_mean;                 /* 1: featurizer.py:79 */
} MvHfEncoderCfg;

typedef struct MvHfEncoder MvHfEncoder;

void mv_hfenc_default_cfg(MvHfEncoderCfg* cfg);   /* the wav2vec2-base geometry */
/* tensors: the fp32 state_dict of the Wav2Vec2Model / WavLMModel under its own key names (device pointers); read are
 *   feature_extractor.conv_layers.{i}.conv.weight [conv_dim[i], conv_dim[i-1] (1 for i = 0), conv_kernel[i]], .conv.bias (conv_bias),
 *   feature_extractor.conv_layers.{i}.layer_norm.weight / .bias (i = 0 in "group" mode, every i in "layer" mode),
 *   feature_projection.layer_norm.weight / .bias.
 * A missing one: MV_ERR_MISSING_TENSOR; a mis-shaped one: MV_ERR_INVALID_ARGUMENT; both name the tensor.  The handle owns the packed
 * weights and no mutable state: forwards on different streams with different workspaces may run concurrently. */
struct MvTensorRef;   /* declared with the backbones below */
int mv_hfenc_create(const MvHfEncoderCfg* cfg, const struct MvTensorRef* tensors, int32_t num_tensors, MvHfEncoder** out);
int mv_hfenc_destroy(MvHfEncoder* h);
/* T' after every layer's n -> floor((n - k) / s) + 1; <= 0 when the waveform is shorter than the receptive field (400 samples) */
int mv_hfenc_num_frames(const MvHfEncoder* h, int64_t num_samples, int64_t* num_frames);
int mv_hfenc_workspace_bytes(const MvHfEncoder* h, int32_t B, int64_t L, size_t* bytes);
/* wav [B, L] fp32 rows wav_stride apart; lens_ratio [B] fp32 or NULL (frames t >= round_half_even(ratio * T') are zeroed);
 * out [B, T', conv_dim[last]] fp32 contiguous, 16-byte aligned; workspace: mv_hfenc_workspace_bytes(h, B, L) bytes, 16-byte aligned, untouched until the
 * forward has run on `stream`.  A waveform shorter than the receptive field is refused (the reference's Conv1d raises there).  A row's
 * bits depend on the row alone: not on B, the other rows or the stream. */
int mv_hfenc_forward(const MvHfEncoder* h, const float* wav, int32_t B, int64_t L, int64_t wav_stride, const float* lens_ratio,
                     float* out, void* workspace, size_t workspace_bytes, mv_stream_t stream);
/* Variable-length batch (additive since ABI 5; the contract of mv_melspec_forward_varlen): row b holds n_b = clamp(num_samples[b], 0, L) valid
 * samples (device array, int64, B entries, read on the device only; NULL is refused).  Frames 0 .. T'(n_b) - 1 of row b are what mv_hfenc_forward
 * of the same handle gives for that row alone as a [1, n_b] batch without a ratio, and BIT FOR BIT so ("group" and "layer" mode, with and without
 * do_normalize, conv_bias and subtract_time_mean); the output keeps the shape [B, T'(L), conv_dim[last]] and its frames t >= T'(n_b) are zero:
 *   - the z-score, layer 0's GroupNorm statistics and the time mean run over the row's own n_b samples / T_0(n_b) / T'(n_b) frames, summed in
 *     orders that depend on these counts alone (not on L, B, the other rows or the stream);
 *   - the samples behind n_b are never read into a result (NaN included): layer 0 loads them as zeros and stores zeros behind the row's own
 *     frames; the further layers run over all T_i(L) frames and hold finite filler behind a row's own count, which no valid frame reads;
 *   - a row below the receptive field (n_b = 0 included) is all zero and no error, whatever subtract_time_mean says.
 * The call is refused when T'(L) <= 0, as mv_hfenc_forward refuses it; the other checks are those of the forward on (B, L), the workspace is
 * the one mv_hfenc_workspace_bytes(h, B, L) reports. */
int mv_hfenc_forward_varlen(const MvHfEncoder* h, const float* wav, int32_t B, int64_t L, int64_t wav_stride, const int64_t* num_samples,
                            float* out, void* workspace, size_t workspace_bytes, mv_stream_t stream);
/* The same forward with HIP events between its stages (tools/bench_hf_frontend.py; a measurement hook like mv_profile_*: not thread-safe, WAITS for
 * the forward, ONE DEVICE per process -- its events are created at the first call, on the device current then, and kept).  stage_ms_host: HOST array of num_stages = num_layers + 1 floats = milliseconds of layer 0 (with the z-score), of every further layer
 * (conv + its GELU / LayerNorm pass) and of the tail (feature_projection.layer_norm + time mean + mask). */
int mv_hfenc_forward_timed(const MvHfEncoder* h, const float* wav, int32_t B, int64_t L, int64_t wav_stride, const float* lens_ratio,
                           float* out, void* workspace, size_t workspace_bytes, mv_stream_t stream, float* stage_ms_host, int32_t num_stages);

/* The kernels of the forward one at a time (additive since ABI 5; layer-level checks -- the forward reaches its kernels through the same launch
 * code).  All pointers are device pointers; a refused call names what is wrong and launches nothing.  Widths C: multiples of 64 up to 1024.
 *
 * mv_hfenc_wave_stats: stats [B][2] = (mean, sqrt(biased var + 1e-7)) of every row over its own n_b = clamp(num_samples[b], 0, L) samples
 *   (num_samples NULL: L); n_b = 0 gives (0, 1). */
int mv_hfenc_wave_stats(const float* wav, int32_t B, int64_t L, int64_t wav_stride, const int64_t* num_samples, float* stats, mv_stream_t stream);
/* mv_hfenc_layer0: the 1 -> C conv of k <= 16 taps at stride s <= 8 over (wav - mean) / sd (wstats [B][2] as mv_hfenc_wave_stats leaves them, or
 *   NULL: the samples as they are), w [C][k] fp32, bias [C] or NULL; y [B, T0, C] fp16, T0 = floor((L - k) / s) + 1 >= 1.
 *   gamma and beta given ("group" mode): GroupNorm(C, C) over the row's own T0_b frames (eps 1e-5) + exact GELU; cstats [B][C][2] receives
 *   (mean, rstd), (0, 1) where T0_b = 0; workspace: mv_hfenc_layer0_workspace_bytes, 8-byte aligned (the fp64 sums of the 128-frame chunks).
 *   gamma and beta NULL ("layer" mode before its row pass): conv + bias stored as fp16; cstats and workspace are not touched.
 *   Frames t >= T0_b of a row are zeros; samples at or behind n_b are never read. */
int mv_hfenc_layer0_workspace_bytes(int32_t B, int64_t L, int32_t C, int32_t k, int32_t s, size_t* bytes);
int mv_hfenc_layer0(const float* wav, int32_t B, int64_t L, int64_t wav_stride, const int64_t* num_samples, const float* wstats, const float* w,
                    const float* bias, const float* gamma, const float* beta, int32_t C, int32_t k, int32_t s, void* y, float* cstats,
                    void* workspace, size_t workspace_bytes, mv_stream_t stream);
/* mv_hfenc_rows: one pass over n_rows frames of C fp16 channels.  MV_HF_ROWS_GELU: y = gelu(x), fp16 (gamma, beta, eps unused);
 *   MV_HF_ROWS_LN_GELU: y = gelu(LayerNorm(x) * gamma + beta), fp16; MV_HF_ROWS_LN_F32: y = LayerNorm(x) * gamma + beta, fp32 (y != x).
 *   The fp16 modes may run in place (y == x).  C = 512: x and y 16-byte aligned. */
#define MV_HF_ROWS_GELU 0
#define MV_HF_ROWS_LN_GELU 1
#define MV_HF_ROWS_LN_F32 2
int mv_hfenc_rows(const void* x, void* y, const float* gamma, const float* beta, float eps, int64_t n_rows, int32_t C, int32_t mode,
                  mv_stream_t stream);
/* mv_hfenc_cmn_mask: out [B, T, C] fp32 in place: minus the mean over the row's frames (cmn != 0), then zeros behind the mask length.
 *   lens_ratio [B] or NULL: all T frames count, zeros from round_half_even(ratio * T) on.  num_samples [B] or NULL (not both): the row's frames
 *   are Tb = its clamp(num_samples[b], 0, L) samples carried through num_layers valid convs (conv_kernel, conv_stride: HOST arrays; T must be
 *   the count of L samples); the mean runs over Tb frames, zeros from Tb on whatever lies there. */
int mv_hfenc_cmn_mask(float* out, int32_t B, int32_t T, int32_t C, const float* lens_ratio, const int64_t* num_samples, int64_t L,
                      const int32_t* conv_kernel, const int32_t* conv_stride, int32_t num_layers, int32_t cmn, mv_stream_t stream);

/* ------------------------------------------------------------------------------------------------
 * Front-end 6: a HuggingFace Wav2Vec2-BERT model's (facebook/w2v-bert-2.0) `extract_features` + time-mean subtraction + mask
 * (csrc/w2vbert.hip).  For Wav2Vec2BertModel that is feature_projection.layer_norm(input_features), and input_features is what the
 * SeamlessM4TFeatureExtractor computes on the host: waveform * 2^15 -> Kaldi log-mel (80 bins, 25 / 10 ms at 16 kHz, Povey window, pre-emphasis
 * 0.97, DC removal, 512-point transform, mel banks 20 Hz .. Nyquist, floor 1.192092955078125e-07, snip_edges) -> per mel bin over the row's T
 * frames (x - mean) / sqrt(var(ddof = 1) + 1e-7) -> zero frames up to a multiple of `stride` -> `stride` frames stacked into stride * 80
 * columns; then the model's LayerNorm over those columns and featurizer.py:79-90.  The log-mel runs on an Fbank handle of this handle's own
 * whose window table carries the 2^15 (exact: a power of two); frames T = 1 + (n - 400) / 160 for n >= 400, stacked frames T2 = ceil(T / stride).
 * Output [B, T2, stride * num_mel_bins] fp32.  None of the transformer is evaluated.  Additive since ABI 5.
 * ------------------------------------------------------------------------------------------------ */
typedef struct MvW2vBertCfg {
    int32_t num_mel_bins;        /* 80; anything else: MV_ERR_UNSUPPORTED */
    int32_t stride;              /* 2; anything else: MV_ERR_UNSUPPORTED */
    int32_t sampling_rate;       /* 16000; anything else: MV_ERR_UNSUPPORTED */
    float layer_norm_eps;        /* of feature_projection.layer_norm (config.layer_norm_eps); positive */
    int32_t subtract_time_mean;  /* 1: featurizer.py:79 */
} MvW2vBertCfg;

typedef struct MvW2vBert MvW2vBert;

/* ln_weight, ln_bias: feature_projection.layer_norm.{weight, bias}, stride * num_mel_bins fp32 each, HOST pointers (copied).  The handle owns
 * its tables and no mutable state: forwards on different streams with different workspaces may run concurrently. */
int mv_w2vbert_create(const MvW2vBertCfg* cfg, const float* ln_weight, const float* ln_bias, MvW2vBert** out);
int mv_w2vbert_destroy(MvW2vBert* h);
/* stacked frames T2 of a row of num_samples samples (0 below 400 samples) */
int mv_w2vbert_num_frames(const MvW2vBert* h, int64_t num_samples, int64_t* num_frames);
int mv_w2vbert_workspace_bytes(const MvW2vBert* h, int32_t B, int64_t L, size_t* bytes);
/* wav [B, L] fp32 rows wav_stride apart; lens_ratio [B] fp32 or NULL (stacked frames t >= round_half_even(ratio * T2) are zeroed); out
 * [B, T2, stride * num_mel_bins] fp32 contiguous, 16-byte aligned; workspace: mv_w2vbert_workspace_bytes(h, B, L) bytes, 16-byte aligned.  Every
 * row is normalised over all T frames of the padded length L (the reference's behaviour behind collate_fn).  L < 560 (fewer than two frames: the
 * reference's var(ddof = 1) is NaN, below 400 samples its extractor raises) is refused by name.  Launches only, no host synchronisation; a row's
 * bits depend on the row alone: not on B, the other rows, the stream or what out and the workspace held.  B = 0 returns MV_OK and touches
 * nothing.  MV_ERR_INVALID_ARGUMENT: a null pointer, negative sizes, wav_stride < L, a misaligned out; MV_ERR_WORKSPACE: a short or misaligned
 * workspace. */
int mv_w2vbert_forward(const MvW2vBert* h, const float* wav, int32_t B, int64_t L, int64_t wav_stride, const float* lens_ratio, float* out,
                       void* workspace, size_t workspace_bytes, mv_stream_t stream);
/* Variable-length batch: row b holds n_b = clamp(num_samples[b], 0, L) valid samples (device array, int64, B entries, read on the device only).
 * Row b is featurised as if alone -- own T_b, own per-bin statistics, own zero half-frame when T_b is odd, own time mean over its T2_b stacked
 * frames, zeros behind -- and BIT FOR BIT equals mv_w2vbert_forward of the same handle on that row as a [1, n_b] batch without a ratio.  A row with
 * n_b < 560 is all zero; samples at or behind n_b are never read (NaN included).  The output keeps the shape [B, T2(L), .]; T2(L) = 0 touches
 * nothing. */
int mv_w2vbert_forward_varlen(const MvW2vBert* h, const float* wav, int32_t B, int64_t L, int64_t wav_stride, const int64_t* num_samples,
                              float* out, void* workspace, size_t workspace_bytes, mv_stream_t stream);
/* The new kernels of the forward one at a time (kernel-level checks; the forward reaches them through the same launch code).  Device pointers;
 * built for 80 bins and stride 2; a refused call names what is wrong and launches nothing.  num_samples [B] int64 or NULL: the row's frames are
 * T_b = frames of clamp(num_samples[b], 0, L) samples, 0 below 560 samples (T must then be the frame count of L samples); NULL: T_b = T.
 *
 * mv_w2vbert_binstats_f32: x [B, T, 80] fp32 -> mean, var [B, 80] fp32: per bin over the row's T_b >= 2 frames the mean and the unbiased variance,
 *   centred two-pass in fp64 in one fixed order (partial sums of 16-frame tiles folded in tile order), rounded once to fp32; (0, 0) where T_b = 0. */
int mv_w2vbert_binstats_f32(const float* x, int32_t B, int32_t T, const int64_t* num_samples, int64_t L, float* mean, float* var, mv_stream_t stream);
/* mv_w2vbert_rows_f32: z = (x - mean) / sqrt(var + 1e-7), zeros for frames t >= T_b; frames 2 t2, 2 t2 + 1 stacked into 160 columns; LayerNorm over
 *   them (biased variance, eps) times ln_weight plus ln_bias -> out [B, ceil(T / 2), 160] fp32; stacked frames at or behind ceil(T_b / 2) are zero
 *   rows.  x, mean, var, ln_weight, ln_bias and out 16-byte aligned (16-byte loads and stores). */
int mv_w2vbert_rows_f32(const float* x, const float* mean, const float* var, const float* ln_weight, const float* ln_bias, float eps, int32_t B,
                        int32_t T, const int64_t* num_samples, int64_t L, float* out, mv_stream_t stream);
/* mv_w2vbert_cmn_mask_f32: out [B, T2, 160] fp32 in place: minus the mean over the row's stacked frames (cmn != 0; summed in fp64 in one fixed
 *   order, rounded once), then zeros behind the mask length.  lens_ratio [B] or NULL: all T2 frames count, zeros from round_half_even(ratio * T2)
 *   on.  num_samples [B] or NULL (not both; T2 must be the count of L samples): the mean runs over the row's own T2_b frames, zeros from T2_b on. */
int mv_w2vbert_cmn_mask_f32(float* out, int32_t B, int32_t T2, const float* lens_ratio, const int64_t* num_samples, int64_t L, int32_t cmn,
                            mv_stream_t stream);

/* ------------------------------------------------------------------------------------------------
 * Backbones.  A model handle is built from the reference-layout fp32 ``state_dict`` (same key names
 * and shapes as the reference modules, so ``model.pth`` loads unchanged: mvector/utils/checkpoint.py:
 * 11-51).  create() folds eval-mode BatchNorm into per-channel scale/shift, packs conv weights to the
 * fp16 [Cout][tap][Cin] layout the MFMA kernels read, and keeps fp32 copies of the small dense layers.
 * ------------------------------------------------------------------------------------------------ */
typedef struct MvTensorRef {
    const char* name;   /* state_dict key relative to the backbone, e.g. "blocks.0.conv.conv.weight" */
    const float* data;  /* device pointer, fp32, contiguous */
    int64_t numel;
} MvTensorRef;

typedef struct MvModel MvModel;

/* EcapaTdnn.forward (mvector/models/ecapa_tdnn.py:253-283), pooling_type "ASP" (other heads: mv_ecapa_create_pooled below). */
typedef struct MvEcapaCfg {
    int32_t input_size;          /* F, any positive width: not a multiple of 8 -> zero-padded to round_up(F, 8) on the device (bits of that width
                                  * with zero-padded features and first-layer weights) */
    int32_t embd_dim;            /* 192 */
    int32_t channels[5];         /* {512,512,512,512,1536} */
    int32_t kernel_sizes[5];     /* {5,3,3,3,1} */
    int32_t dilations[5];        /* {1,2,3,4,1} */
    int32_t attention_channels;  /* 128 */
    int32_t res2net_scale;       /* 8 */
    int32_t se_channels;         /* 128 */
    int32_t global_context;      /* 1 */
} MvEcapaCfg;
int mv_ecapa_create(const MvEcapaCfg* cfg, const MvTensorRef* tensors, int32_t num_tensors, MvModel** out);

/* CAMPPlus.forward (mvector/models/campplus.py:353-357). */
typedef struct MvCamppCfg {
    int32_t input_size;    /* F (80) */
    int32_t embd_dim;      /* 192 in configs/cam++.yml:58; class default 512 */
    int32_t growth_rate;   /* 32 */
    int32_t bn_size;       /* 4 */
    int32_t init_channels; /* 128 */
    int32_t head_precision; /* MV_CAMPP_HEAD_AUTO (0): decided at create from three probe utterances; _F16 / _F32 pin it -- e.g. the
                             * same value on every rank of a distributed run, so that enrol and verify embeddings share one numerics */
    int32_t xvector_probe;  /* since ABI 5.  MV_CAMPP_XVEC_PROBE_ON (0): create also measures what the fp16 operands of the x-vector part cost on the
                             * three probe utterances (MV_INFO_CAMPP_XVEC_*; ~330 small exact-fp32 launches, once); _OFF (1) skips it */
} MvCamppCfg;
#define MV_CAMPP_XVEC_PROBE_ON 0
#define MV_CAMPP_XVEC_PROBE_OFF 1
#define MV_CAMPP_HEAD_AUTO 0
#define MV_CAMPP_HEAD_F16 1
#define MV_CAMPP_HEAD_F32 2
int mv_campp_create(const MvCamppCfg* cfg, const MvTensorRef* tensors, int32_t num_tensors, MvModel** out);

/* TDNN.forward (mvector/models/tdnn.py:46-68), pooling_type "ASP" (other heads: mv_tdnn_create_pooled below). */
typedef struct MvTdnnCfg {
    int32_t input_size; /* F, any positive width: not a multiple of 8 -> a zero-padded fp32 copy at round_up(F, 8) in the workspace */
    int32_t channels; /* 512 */
    int32_t embd_dim; /* 192 */
} MvTdnnCfg;
int mv_tdnn_create(const MvTdnnCfg* cfg, const MvTensorRef* tensors, int32_t num_tensors, MvModel** out);

/* The pooling heads of EcapaTdnn and TDNN (the reference's `pooling_type`, mvector/models/pooling.py), over the pooling input x [B, C, T]:
 *   MV_POOL_ASP  attentive statistics pooling: weighted mean | weighted std   -> 2C   (what mv_ecapa_create / mv_tdnn_create build)
 *   MV_POOL_SAP  self-attentive pooling: sum_t softmax_t(W2 . tanh(W1 . x + b1) + b2) x   -> C  (bottleneck 128: keys <pool>.linear1.*, .linear2.*)
 *   MV_POOL_TAP  mean over time   -> C
 *   MV_POOL_TSP  mean | unbiased variance over time (torch.var: NaN at T = 1)   -> 2C
 * Behind the head: EcapaTdnn asp_bn -> fc (SAP / TAP / TSP: asp_bn is a plain BatchNorm1d, keys asp_bn.*; ASP: asp_bn.norm.*), TDNN bn5 ->
 * linear -> bn6 -- folded into one exact-fp32 layer as for ASP.  The _pooled create calls take one of these codes; MV_POOL_ASP builds the same
 * handle as the plain create call.  An unknown code, or a state_dict without the chosen head's tensors, is refused with MV_ERR_INVALID_ARGUMENT /
 * MV_ERR_MISSING_TENSOR and a message. */
#define MV_POOL_ASP 0
#define MV_POOL_SAP 1
#define MV_POOL_TAP 2
#define MV_POOL_TSP 3
int mv_ecapa_create_pooled(const MvEcapaCfg* cfg, int32_t pooling_type, const MvTensorRef* tensors, int32_t num_tensors, MvModel** out);

/* EcapaTdnn with any number of SE-Res2Net blocks and grouped TDNN convolutions (the reference constructor's `channels` / `kernel_sizes` /
 * `dilations` of any length >= 3 and its `groups`, ecapa_tdnn.py:146-216).  N = nblocks SE-Res2Net blocks, arrays of N + 2 entries:
 *   entry 0       blocks.0 (input_size -> channels[0], kernel_sizes[0] taps, groups[0])
 *   entry i       SE-Res2Net block i = 1..N (channels[i-1] -> channels[i]; its tdnn1 and tdnn2 are 1x1 with groups[i]; the Res2Net, SE and shortcut
 *                 convolutions are not grouped)
 *   entry N + 1   the MFA (sum of the N block widths -> channels[N + 1], which must equal that sum; groups[N + 1])
 * Indexing is by position, as the reference's: with N = 4 and its default 5-entry `groups`, pass groups[4] for both block 4 and the MFA.
 * Every grouped layer's in and out widths must be divisible by its group count (torch's rule).  A grouped 1x1 layer whose groups are
 * mv_conv1d_grouped_native runs as a grouped GEMM; the other grouped layers (blocks.0, an MFA with kernel_sizes[N + 1] > 1, narrow groups) are
 * expanded at create into their block-diagonal dense weight (exact zeros).  mv_model_info reports how many of each (MV_INFO_ECAPA_*).
 * Refused with a message: nblocks outside 1..MV_ECAPA_MAX_BLOCKS, channels[N + 1] != sum of the block widths, a width not divisible by its
 * groups, a non-positive group count.  MvEcapaCfg / mv_ecapa_create / mv_ecapa_create_pooled are unchanged: an extended config with nblocks = 3
 * and every group count 1 builds the same handle as they do. */
#define MV_ECAPA_MAX_BLOCKS 16
typedef struct MvEcapaCfgEx {
    int32_t input_size;          /* F, as in MvEcapaCfg */
    int32_t embd_dim;
    int32_t nblocks;             /* N, 1 .. MV_ECAPA_MAX_BLOCKS */
    int32_t channels[MV_ECAPA_MAX_BLOCKS + 2];       /* first N + 2 entries used */
    int32_t kernel_sizes[MV_ECAPA_MAX_BLOCKS + 2];
    int32_t dilations[MV_ECAPA_MAX_BLOCKS + 2];
    int32_t groups[MV_ECAPA_MAX_BLOCKS + 2];         /* >= 1 */
    int32_t attention_channels;
    int32_t res2net_scale;
    int32_t se_channels;
    int32_t global_context;
} MvEcapaCfgEx;
int mv_ecapa_create_ex(const MvEcapaCfgEx* cfg, int32_t pooling_type, const MvTensorRef* tensors, int32_t num_tensors, MvModel** out);
int mv_tdnn_create_pooled(const MvTdnnCfg* cfg, int32_t pooling_type, const MvTensorRef* tensors, int32_t num_tensors, MvModel** out);

/* ERes2Net.forward / ERes2NetV2.forward (mvector/models/eres2net.py:266-287 / 441-456): 2-D Res2Net blocks with AFF
 * fusion, temporal statistics pooling (pooling.py:130-148), seg_1 (+ optional ReLU -> seg_bn_1 -> seg_2). */
typedef struct MvEres2Cfg {
    int32_t version;       /* 1 = ERes2Net, 2 = ERes2NetV2 */
    int32_t input_size;    /* F (80); must be a multiple of 8 */
    int32_t embd_dim;      /* 192 */
    int32_t num_blocks[4]; /* {3,4,6,3} */
    int32_t m_channels;    /* 32 */
    int32_t mul_channel;   /* ERes2Net only: 1 */
    int32_t expansion;     /* 2 */
    int32_t base_width;    /* ERes2Net 32, ERes2NetV2 26 */
    int32_t scale;         /* 2 */
    int32_t two_emb_layer; /* 0 */
} MvEres2Cfg;
int mv_eres2net_create(const MvEres2Cfg* cfg, const MvTensorRef* tensors, int32_t num_tensors, MvModel** out);

/* ResNetSE.forward (mvector/models/resnet_se.py:65-145): conv3x3 stem, four stages of SE bottleneck blocks (1x1 -> 3x3 (stride) -> 1x1 -> squeeze /
 * excitation gate -> + residual -> ReLU) on S16 maps, x.reshape(B, -1, T') -> the pooling head `pooling_type` (MV_POOL_*, prefix `pooling.`) ->
 * bn2 -> linear -> bn3 folded into one exact-fp32 layer.  Entry point added under ABI 5.
 * Refused with a message: input_size not a multiple of 8; a num_filters entry that is not a multiple of 16 or is above 512; a stage without
 * blocks; a reduction that leaves no hidden unit; a pooling_type outside MV_POOL_ASP .. MV_POOL_TSP; a missing tensor.  The forward needs at least 9
 * frames (two time steps behind three stride-2 stages).
 * The network's ReLU has no upper bound and S16 maps saturate at |value| = 1023.5: every launch that stores a map reports the largest value it
 * wanted to store to one device word of the handle, read through mv_model_info (MV_INFO_RESNETSE_*; never on the forward path).
 * MV_RESNETSE_NO_PEAK or-ed into pooling_type builds the handle WITHOUT that word (the conv launches then run the instantiation without the
 * tracking code; the two keys report -1): for tools that measure what the tracking costs, not for serving. */
#define MV_RESNETSE_NO_PEAK 0x100
typedef struct MvResNetSeCfg {
    int32_t input_size;     /* F (80); must be a multiple of 8 */
    int32_t layers[4];      /* {3,4,6,3} */
    int32_t num_filters[4]; /* {32,64,128,256}: multiples of 16, at most 512 */
    int32_t embd_dim;       /* 192 */
    int32_t pooling_type;   /* MV_POOL_* */
    int32_t reduction;      /* 8 */
} MvResNetSeCfg;
int mv_resnetse_create(const MvResNetSeCfg* cfg, const MvTensorRef* tensors, int32_t num_tensors, MvModel** out);

/* Res2Net.forward (mvector/models/res2net.py:89-174): conv7x7 stride-3 stem + MaxPool2d(3, 2, 1), four stages of Bottle2neck blocks (1x1 into `scale`
 * slices of `width` channels -> a 3x3 conv (stride) per slice but the last, hierarchical sums in the 'normal' blocks -> the last slice passed on
 * ('normal') or AvgPool2d(3, stride, 1)-ed ('stage') -> 1x1 + residual -> ReLU) on S16 maps, x.reshape(B, -1, T') -> the pooling head
 * `pooling_type` (MV_POOL_*, prefix `pooling.`) -> bn2 -> linear -> bn3 folded into one exact-fp32 layer.  Entry point added under ABI 5.
 * Refused with a message: scale outside 1..8; m_channels not a multiple of 8 or above 256 (the stem's limits); a stage without
 * blocks; a block width floor(planes * base_width / 64) below 4; an input_size whose frequency size behind the four stages
 * (h1 = (F - 5) / 3 + 1, h2 = (h1 - 1) / 2 + 1, then three times (h - 1) / 2 + 1) differs from input_size / base_width (the reference's own
 * forward fails on such a model); a pooling_type outside MV_POOL_ASP .. MV_POOL_TSP; a missing tensor.  The forward needs at least 5 frames.
 * Saturation: as ResNetSE -- one device word per handle, MV_INFO_S16_PEAK / MV_INFO_S16_SATURATED; MV_RES2NET_NO_PEAK or-ed into pooling_type
 * builds the handle without it. */
#define MV_RES2NET_NO_PEAK 0x100
typedef struct MvRes2NetCfg {
    int32_t input_size;   /* F (80) */
    int32_t m_channels;   /* 32: a multiple of 8, at most 256 */
    int32_t layers[4];    /* {3,4,6,3} */
    int32_t base_width;   /* 32 */
    int32_t scale;        /* 2: 1..8 */
    int32_t embd_dim;     /* 192 */
    int32_t pooling_type; /* MV_POOL_* */
} MvRes2NetCfg;
int mv_res2net_create(const MvRes2NetCfg* cfg, const MvTensorRef* tensors, int32_t num_tensors, MvModel** out);

int mv_model_destroy(MvModel* m);
int mv_model_embd_dim(const MvModel* m, int32_t* embd_dim);
/* Model-specific facts (tests, logs).  Keys:
 *   MV_INFO_CAMPP_HEAD_F32     1.0 when the CAM++ handle evaluates its FCM head in the exact form (since ABI 3: hi + lo fp16 operand pairs through the
 *                              conv2ds kernels; before: fp32 maps through the conv2d kernels), 0.0 for the fp16 head;
 *   MV_INFO_CAMPP_CALIBRATION  largest 1 - cos between the embeddings of the two heads over the handle's three probe utterances
 *                              (mv_campp_create; -1 when MvCamppCfg.head_precision pinned the head);
 *   MV_INFO_CAMPP_PROBE0 + p   the figure of probe p = 0..2 (white uniform / white bell-shaped / smooth voiced-like). */
#define MV_INFO_CAMPP_HEAD_F32 1
#define MV_INFO_CAMPP_CALIBRATION 2
#define MV_INFO_CAMPP_PROBE0 3
/* since ABI 4 -- the range of the exact head.  Its S16 maps hold 64 * gain * value in fp16 pairs (|.| <= 65504); gain = 2^k (k <= 0) is chosen at
 * create so that the probes' largest map value sits 16 x below that bound (the head is positively homogeneous, so the gain is exact).
 *   MV_INFO_CAMPP_HEAD_GAIN_LOG2  k
 *   MV_INFO_CAMPP_PROBE_PEAK      largest map value over the probes (real units)
 *   MV_INFO_CAMPP_HEAD_PEAK       largest map value the exact head has wanted to store on the caller's inputs since create (real units; waits for the device)
 *   MV_INFO_CAMPP_HEAD_SATURATED  1.0 when one of them exceeded the range and was clamped (the embedding of that call is not to be trusted) */
#define MV_INFO_CAMPP_HEAD_GAIN_LOG2 6
/* since ABI 5 -- what the head probes cannot see (campplus.py:295-357 behind the head): the x-vector part always runs on fp16 operands.  create
 * evaluates it once more in exact fp32 on the three probes (same head rows, the caller's fp32 weights, exact-fp32 GEMMs) and reports
 *   MV_INFO_CAMPP_XVEC_SENSITIVITY   largest 1 - cos between the shipped and the exact x-vector part over the probes (-1: probe switched off)
 *   MV_INFO_CAMPP_XVEC_PROBE0 + p    probe p's figure.
 * Above MV_CAMPP_XVEC_WARN the 1e-4 contract (1 - cos against the reference's fp32 forward) is at risk on this checkpoint whatever head runs: there
 * is no exact form of the x-vector part; the Python surface warns (mvector/models/campplus.py). */
#define MV_INFO_CAMPP_XVEC_SENSITIVITY 10
#define MV_INFO_CAMPP_XVEC_PROBE0 11
#define MV_CAMPP_XVEC_WARN 2.5e-5f
#define MV_INFO_CAMPP_PROBE_PEAK 7
#define MV_INFO_CAMPP_HEAD_PEAK 8
#define MV_INFO_CAMPP_HEAD_SATURATED 9
/* EcapaTdnn handles (mv_ecapa_create*): how their grouped convolutions run (0 on an ungrouped model)
 *   MV_INFO_ECAPA_GROUPED_NATIVE     grouped layers on the grouped GEMM (mv_conv1d_grouped_native)
 *   MV_INFO_ECAPA_GROUPED_EXPANDED   grouped layers expanded into a block-diagonal dense weight
 *   MV_INFO_ECAPA_EXPANDED_1X1       of those, the 1x1 ones
 *   MV_INFO_ECAPA_BLOCKS             N, the number of SE-Res2Net blocks */
#define MV_INFO_ECAPA_GROUPED_NATIVE 20
#define MV_INFO_ECAPA_GROUPED_EXPANDED 21
#define MV_INFO_ECAPA_EXPANDED_1X1 22
#define MV_INFO_ECAPA_BLOCKS 23
/* ResNetSE and Res2Net handles (mv_resnetse_create, mv_res2net_create): the range of their S16 maps on the caller's inputs since create (both WAIT
 * FOR THE DEVICE: diagnostics)
 *   MV_INFO_S16_PEAK        largest |map value| a launch wanted to store (real units; -1 on a handle built with MV_*_NO_PEAK)
 *   MV_INFO_S16_SATURATED   1.0 when it exceeded 1023.5 and was clamped (the embeddings of that call are not to be trusted)
 * The MV_INFO_RESNETSE_* names are the same keys. */
#define MV_INFO_S16_PEAK 30
#define MV_INFO_S16_SATURATED 31
#define MV_INFO_RESNETSE_PEAK MV_INFO_S16_PEAK
#define MV_INFO_RESNETSE_SATURATED MV_INFO_S16_SATURATED
int mv_model_info(const MvModel* m, int32_t key, float* value);
int mv_model_workspace_bytes(const MvModel* m, int32_t B, int32_t T, size_t* bytes);
/* feats: [B, T, F] fp32 (the AudioFeaturizer output layout); emb: [B, embd_dim] fp32. */
int mv_model_forward(const MvModel* m, const float* feats, int32_t B, int32_t T, float* emb, void* workspace,
                     size_t workspace_bytes, mv_stream_t stream);

/* ------------------------------------------------------------------------------------------------
 * Cosine scoring: S[i, j] = <a_i, b_j> / (|a_i| |b_j|).  Replaces sklearn cosine_similarity at
 * mvector/predict.py:174 and mvector/trainer.py:457-459, and predict.py:275-279 (contrast).
 * ------------------------------------------------------------------------------------------------ */
int mv_cosine_f32(const float* a, int32_t n, const float* b, int32_t m, int32_t dim, float* scores,
                  mv_stream_t stream);
/* in-place row L2 normalisation (predict.py:165-166) */
int mv_l2_normalize_f32(float* x, int32_t n, int32_t dim, mv_stream_t stream);

/* ------------------------------------------------------------------------------------------------
 * Speaker search (added within ABI 5): per query the k best gallery rows by cosine similarity, without the [n, m] score matrix.
 * Replaces the score matrix + np.argmax per query of mvector/predict.py:169-183 (__retrieval).
 *   q [n, dim], g [m, dim] fp32 rows of any alignment -> scores [n, k] fp32, index [n, k] int32, best candidate in slot 0.
 * Arithmetic: the score of (query i, row j) is the value mv_cosine_f32(q, n, g, m, dim, ...) writes for that pair -- it compares == as a
 *   float, or both are NaN (a -0 comes out as +0, a NaN as the quiet NaN 0x7FFFFFFF).  dim is limited to 1 .. 2047, the range in which
 *   mv_cosine_f32 runs its four-wave kernel; a larger dim is refused with MV_ERR_UNSUPPORTED.
 * Order: descending by the order-preserving key of the score, in which -0 and +0 are one value and every NaN ranks above +inf (as np.argmax
 *   and torch.topk treat it); equal keys by the LOWER row index first.  For k > m the slots behind m hold index -1 and score -inf (all of
 *   them for m == 0).  n == 0 returns MV_OK and touches nothing.  1 <= k <= 64.
 * The gallery is walked by S slices: slice s takes the rows [16 floor(s T / S), 16 floor((s + 1) T / S)), T = ceil(m / 16); slices_hint > 0
 *   pins S (tests; at most T and 4096), 0 lets the library choose from the chip.  The result does not depend on S, on the batch a query sits
 *   in, or on the stream.  Two ordinary launches (slices, then a merge per query); no workgroup waits for another.
 * workspace: device memory, 8-byte aligned, of the size the companion reports for the same arguments (S * n * k * 8 bytes, independent of m;
 *   0 for arguments the call refuses).  Neither the workspace nor the outputs need initialising.
 * Refused with MV_ERR_INVALID_ARGUMENT and a message: a null pointer, negative n or m, k outside 1 .. 64, dim below 1; MV_ERR_WORKSPACE: a
 *   workspace smaller than reported.
 * ------------------------------------------------------------------------------------------------ */
size_t mv_cosine_topk_workspace_bytes(int32_t n, int32_t m, int32_t dim, int32_t k, int32_t slices_hint);
int mv_cosine_topk_f32(const float* q, int32_t n, const float* g, int32_t m, int32_t dim, int32_t k, float* scores, int32_t* index,
                       int32_t slices_hint, void* workspace, size_t workspace_bytes, mv_stream_t stream);

/* ------------------------------------------------------------------------------------------------
 * Cohort score normalisation (added within ABI 5): Z-, T-, S-norm and adaptive S-norm of a trials x enrolments score matrix.
 *
 * mv_cohort_stats_f32: x [n, dim], cohort [m, dim] fp32 rows -> mean [n], std [n] fp32 of each row's top_n cohort scores.
 *   Cohort scores: the score of (x_i, cohort_j) is the float mv_cosine_f32(x, n, cohort, m, dim, ...) writes for that pair, bit for bit
 *     (the same launcher writes them, chunk by chunk, into the workspace).
 *   Selection: the N' = min(top_n, m) largest of the row by the order-preserving key of the score, in which -0 and +0 are one value and
 *     every NaN ranks above +inf; equal keys by the LOWER cohort index first (equal keys are equal values: the rule only fixes which
 *     entries are summed, the statistics do not depend on it).
 *   Statistics: mean = sum x / N', std = sqrt(sum (x - mean)^2 / N') (population form, two passes), accumulated in fp64 in one fixed order
 *     -- every thread of the row's workgroup adds the kept entries of its own contiguous index segment in ascending order, the partial sums
 *     are folded by a halving tree -- and rounded once to fp32.  No floating-point atomics.  The order depends on m alone (through the
 *     workgroup size of its tier), never on n, on the chunking or on the stream.  A NaN among the selected scores gives NaN / NaN for that row
 *     only; N' equal values v give mean == v and std == 0 exactly.
 *   The n rows are walked in chunks of R rows: R = rows_hint when positive (tests), else the library's choice, which keeps the chunk's
 *     R * m scores well inside the Infinity Cache.  The result does not depend on R.  Two ordinary launches per chunk; no workgroup waits for
 *     another, nothing is allocated, the call does not synchronise.
 *   workspace: device memory, 4-byte aligned, of the size the companion reports for the same arguments: R * m * 4 bytes, at most 64 MiB
 *     whatever n is unless rows_hint asks for more (0 for arguments the call refuses).  It needs no initialising.
 *   Refused with MV_ERR_INVALID_ARGUMENT and a message: a null pointer, negative n, m < 1, top_n < 1, dim < 1; MV_ERR_UNSUPPORTED:
 *     m > MV_COHORT_MAX_ROWS; MV_ERR_WORKSPACE: a workspace smaller than reported.  n == 0 returns MV_OK and touches nothing.
 *
 * mv_score_norm_f32: scores [n_trials, n_enroll] fp32 (contiguous) -> out of the same shape; out == scores is allowed.  For trial t,
 *   enrolment e and raw score s, each operation one correctly rounded fp32 operation in this order (no contraction, no reciprocal), so the
 *   result equals the same expression in numpy.float32 bit for bit; std == 0 is not guarded:
 *     MV_SNORM_Z: (s - enroll_mean[e]) / enroll_std[e]
 *     MV_SNORM_T: (s - trial_mean[t]) / trial_std[t]
 *     MV_SNORM_S: 0.5f * ((s - trial_mean[t]) / trial_std[t] + (s - enroll_mean[e]) / enroll_std[e])
 *   With statistics of top_n < m this is the adaptive form (AS-norm), with top_n >= m plain S-norm.  The statistics of the side a mode does
 *   not use may be null.  n_trials * n_enroll <= 2^31 - 1.  One launch; an empty matrix touches nothing.
 *   Refused with MV_ERR_INVALID_ARGUMENT and a message: a null pointer for a required argument, negative sizes, more than 2^31 - 1
 *   elements, an unknown mode.
 * ------------------------------------------------------------------------------------------------ */
#define MV_SNORM_S 0
#define MV_SNORM_Z 1
#define MV_SNORM_T 2
#define MV_COHORT_MAX_ROWS 32768
size_t mv_cohort_stats_workspace_bytes(int32_t n, int32_t m, int32_t dim, int32_t rows_hint);
int mv_cohort_stats_f32(const float* x, int32_t n, const float* cohort, int32_t m, int32_t dim, int32_t top_n, float* mean, float* std,
                        int32_t rows_hint, void* workspace, size_t workspace_bytes, mv_stream_t stream);
int mv_score_norm_f32(const float* scores, int64_t n_trials, int64_t n_enroll, const float* trial_mean, const float* trial_std,
                      const float* enroll_mean, const float* enroll_std, int32_t mode, float* out, mv_stream_t stream);

/* ------------------------------------------------------------------------------------------------
 * Layer-level entry points (same kernels the model forwards launch; exported so that the parity
 * tests can pin each kernel against the oracle layer by layer).
 * ------------------------------------------------------------------------------------------------ */
#define MV_PAD_ZERO 0
#define MV_PAD_REFLECT 1
#define MV_ACT_NONE 0
#define MV_ACT_RELU 1
#define MV_ACT_TANH 2
#define MV_ACT_SIGMOID 3
#define MV_DT_F32 0
#define MV_DT_F16 1

/* ------------------------------------------------------------------------------------------------
 * 2-D convolution layer of the ERes2Net family (eres2net.py:23-30: conv1x1 / conv3x3, zero padding k/2, no conv
 * bias) on channel-last maps [B, H = frequency, W = time, C], channels padded to multiples of 16 -- the semantics of
 * mv_conv2ds_forward below (split fp16 operands on S16 maps: the family is too deep for plain fp16 operands at the 1e-4 cosine
 * bar) and of the fp32-operand yard-stick tools/yardstick/conv2d_f32.hip:
 *   y = epi( sum_taps W . in + bias ),  in = x | x + x2 (eres2net.py:92) | cat(x, x2) (AFF, eres2net.py:49)
 *   epi 0: clamp(v [+ res], lo, hi)   -- BatchNorm folded into W / bias, ReLU(0..20) eres2net.py:12-15, residual :103-105
 *   epi 1: SiLU (AFF local_att, eres2net.py:41)
 *   epi 2: res * (1 + tanh v) + res2 * (1 - tanh v)   (AFF output, eres2net.py:50-52)
 * ------------------------------------------------------------------------------------------------ */
#define MV_EPI_CLAMP 0
#define MV_EPI_SILU 1
#define MV_EPI_AFF 2
/* (The fp32-operand form of these layers -- MvConv2dDesc, mv_conv2d_pack_weight / _packed_elems / _forward, ABI 1-3 -- left the library with ABI 4: no
 * model handle had run it since round 4; it is the exact-fp32 yard-stick under tools/yardstick/.) */
/* first ERes2Net conv: features fp32 [B, T, F] -> fp32 [B, F, T, C] = relu(conv3x3(1 -> C) + bias), w fp32 [C][9] */
int mv_conv2d_first(const float* feats, float* out, const float* w, const float* bias, int32_t B, int32_t T, int32_t F,
                    int32_t C, mv_stream_t stream);
/* temporal statistics pooling of fp32 [B, H, W, ld] (C real channels) -> fp32 [B, 2*C*H]: mean | sqrt(unbiased var + 1e-8),
 * index c*H + h as the reference flattens [B, C, H] */
int mv_tstp_f32(const float* x, int64_t ld, int32_t B, int32_t H, int32_t W, int32_t C, float* stats, mv_stream_t stream);

/* ------------------------------------------------------------------------------------------------
 * The same layers on the fp16 matrix pipe with split operands (csrc/conv2ds.hip; what mv_eres2net_create's handles run since ABI 3).
 * Maps are "S16": channel-last with 4 bytes per channel like the fp32 maps above (same pointers, leading dimensions and
 * 16-channel slices), but a unit of 16 channels holds [16 x hi | 16 x lo] fp16 of 64 * value (hi = fp16(V), lo = fp16(V - hi)):
 * 22 significant bits, |value| saturates at 1023.5.  mv_map_split_f32 / mv_map_merge_f32 convert n = pixels * ld fp32
 * elements (whole units) to and from that form.  Weights: mv_conv2ds_pack_weight scales a layer by a power of two, splits it the
 * same way into [cout16][k*k][round_up(cin16, 32) / 16 units][32] (mv_conv2ds_packed_elems 4-byte elements) and returns the factor
 * `oscale` the accumulator is multiplied with (synchronises the stream: weights are read back to the host).
 *   y = epi( oscale * sum_taps W . in + bias ),  in = x | cat(x, x2)  (x2 != NULL: cin1 channels from x, the rest from x2)
 *   epi as above; optionally y2 = y + add (the input of the next 3x3 conv of a Res2Net block, eres2net.py:92)
 * ------------------------------------------------------------------------------------------------ */
int64_t mv_conv2ds_packed_elems(int32_t cout, int32_t cin, int32_t ks);
int mv_conv2ds_pack_weight(const float* w, const float* out_scale, int32_t cout, int32_t cin, int32_t ks, void* packed, float* oscale,
                           mv_stream_t stream);
int mv_map_split_f32(const float* x, void* y, int64_t n, mv_stream_t stream);
int mv_map_merge_f32(const void* x, float* y, int64_t n, mv_stream_t stream);
typedef struct MvConv2dsDesc {
    const void* x;       /* S16 [B, H, W, ldx] */
    const void* x2;      /* optional: channels cin1 .. cin16 of the input come from here (AFF concatenation, eres2net.py:49) */
    int32_t cin1;
    int64_t ldx, ldx2;
    const void* w;       /* from mv_conv2ds_pack_weight */
    const float* bias;   /* [cout16] */
    float oscale;        /* from mv_conv2ds_pack_weight */
    const void* res;     /* epi 0: optional residual; epi 2: first AFF operand; S16 [B, Ho, Wo, ldres] */
    const void* res2;    /* epi 2: second AFF operand */
    int64_t ldres, ldres2;
    const void* add;     /* optional with y2: S16 [B, Ho, Wo, ldadd] */
    int64_t ldadd;
    void* y;             /* S16 [B, Ho, Wo, ldy], Ho = (H + 2*(ks/2) - ks)/stride + 1, Wo likewise */
    int64_t ldy;
    void* y2;            /* optional second output y + add */
    int64_t ldy2;
    int32_t B, H, W, cin16, cout16, ks, stride, epi;
    float lo, hi;
    int32_t cin_alg, cout_alg; /* channel counts of the layer before padding (0: same as cin16 / cout16): profile accounting only */
    int32_t stride_w;          /* stride along W when it differs from `stride` (then the stride along H); 0 = same (the CAM++ head strides the
                                * frequency axis only, campplus.py:221-292) */
    uint32_t* peak;            /* optional device word (since ABI 4): the kernel max-es in the bits of the largest |64 * value| it wanted to store BEFORE the
                                * clamp to the fp16 range (positive floats order like unsigned integers); >= 65504.0f means the S16 split saturated */
    int32_t nbw_hint, ct_hint, rows_hint, ring_hint, wgs_hint, spw_hint, nprod_hint; /* 0 = the launcher's choice; otherwise blocks of 16 output channels per wave
                                           * (1..3), blocks per workgroup, rows per 3x3 tile (1..8), LDS ring stages (>= 2), workgroups per CU
                                           * (1 | 2), segments per consumer wave (8 | 4 | 2 | 1), producer waves: launch shapes for tests and tools/bench_conv2d.py (never the bits of a result) */
    int32_t wg_hint;           /* since ABI 5.  0 = the launcher's choice (the chip's workgroup slots); otherwise the workgroups per channel tile are
                                * min(wg_hint, B * pixel tiles): a small layer then walks several tiles per workgroup on a large chip (tests; the counterpart
                                * of MvConv1dDesc.persist_blocks_hint; never the bits of a result).  Negative: refused */
} MvConv2dsDesc;
int mv_conv2ds_forward(const MvConv2dsDesc* d, mv_stream_t stream);
/* What mv_conv2ds_forward would launch for `d`, without launching (additive since ABI 5).  cus = 0 plans for the current device; any other value for a
 * chip of that many compute units.  The descriptor goes through the same checks and the same plan as a forward call, so a refused descriptor returns
 * that call's error code and message.  kernel: the row of csrc/conv2ds.hip's kernel table, "conv2ds_kernel<KS, NBW, SPW, MAXT, TRACK>" as spelled
 * there (a static string owned by the library); nbw / spw / track repeat its parameters (blocks of 16 output channels and 16-pixel segments per
 * consumer wave; track = 1 with a peak word).  ncons / nprod: consumer and producer waves; ns: LDS ring stages; pp: transfers per producer wave and
 * stage (padded); wgs_per_cu: workgroups per compute unit the ring was sized for; rows: output rows per 3x3 tile (1x1: 8 segments); ct: blocks per
 * channel tile, ctiles of them; tiles: pixel tiles per utterance; wg_per_ct: workgroups per channel tile (each walks the pixel tiles
 * widx, widx + wg_per_ct, ... of all B * tiles); grid = wg_per_ct * ctiles; stages_per_tile: K stages of one tile; lds_bytes: dynamic LDS. */
typedef struct MvConv2dsPlanInfo {
    const char* kernel;
    int32_t nbw, spw, track;
    int32_t ncons, nprod, ns, pp, wgs_per_cu;
    int32_t rows, ct, ctiles, tiles, wg_per_ct, grid;
    int32_t stages_per_tile;
    int32_t lds_bytes;
} MvConv2dsPlanInfo;
int mv_conv2ds_plan_info(const MvConv2dsDesc* d, int32_t cus, MvConv2dsPlanInfo* out);
/* the first conv and the pooling with S16 maps on the map side */
int mv_conv2d_first_s16(const float* feats, void* out, const float* w, const float* bias, int32_t B, int32_t T, int32_t F,
                        int32_t C, mv_stream_t stream);
int mv_tstp_s16(const void* x, int64_t ld, int32_t B, int32_t H, int32_t W, int32_t C, float* stats, mv_stream_t stream);

/* ------------------------------------------------------------------------------------------------
 * The SE layer of ResNetSE on S16 maps [B, H, W, ld] with C real channels (csrc/se2d.hip; resnet_se.py:47-62, 36-42), and the hand-over of a map
 * to the pooling heads.  Added under ABI 5.  Every entry point refuses null pointers, non-positive sizes, ld < C and ld % 16 != 0 with a message.
 *   mv_se2d_squeeze_s16        s[b, c] = mean over the H * W pixels, fp32 [B, C].  Partial sums over MV_SE2D_SQUEEZE_CHUNK consecutive pixels
 *                              (in fp64) into the caller's workspace of mv_se2d_squeeze_workspace_floats(B, H, W, C) floats (8-byte aligned), then
 *                              a finish pass in chunk order: no atomics, the bits of a row do not depend on B.
 *   mv_se2d_excite_f32         g = sigmoid(W2 . relu(W1 . s + b1) + b2): s [B, C], w1 [R, C], b1 [R], w2 [C, R], b2 [C], g [B, C] fp32
 *                              (products summed in fp64 in one fixed order); C <= 1024, 1 <= R <= 1024.
 *   mv_se2d_gate_res_relu_s16  y = relu(x * g[b, c] + res), x / res / y S16 with their own leading dimensions (y may be x or res); channels C ..
 *                              of a padded unit stay exact zeros; peak (optional device word) as MvConv2dsDesc.peak.
 *   mv_s16_map_to_rows_f16     fp16 y[b, w, c * H + h] = x[b, h, w, c] (x.reshape(B, -1, W), channel-last), row pitch ldy >= C * H, a multiple
 *                              of 8; columns C * H .. ldy - 1 zero.  H <= 256.
 * ------------------------------------------------------------------------------------------------ */
#define MV_SE2D_SQUEEZE_CHUNK 256
size_t mv_se2d_squeeze_workspace_floats(int32_t B, int32_t H, int32_t W, int32_t C);
int mv_se2d_squeeze_s16(const void* x, int64_t ld, int32_t B, int32_t H, int32_t W, int32_t C, float* s, float* workspace, size_t workspace_floats,
                        mv_stream_t stream);
int mv_se2d_excite_f32(const float* s, const float* w1, const float* b1, const float* w2, const float* b2, float* g, int32_t B, int32_t C, int32_t R,
                       mv_stream_t stream);
int mv_se2d_gate_res_relu_s16(const void* x, int64_t ldx, const float* g, const void* res, int64_t ldres, void* y, int64_t ldy, int32_t B, int32_t H,
                              int32_t W, int32_t C, uint32_t* peak, mv_stream_t stream);
int mv_s16_map_to_rows_f16(const void* x, int64_t ld, int32_t B, int32_t H, int32_t W, int32_t C, void* y, int64_t ldy, mv_stream_t stream);

/* ------------------------------------------------------------------------------------------------
 * The layers only Res2Net has, on S16 maps (csrc/res2net2d.hip; res2net.py:98-101, 35, 75).  Added under ABI 5.  Every entry point refuses null
 * pointers, non-positive sizes, ld < C, ld % 16 != 0 and a stride other than 1 or 2 with a message.
 *   mv_conv2d_stem7_s16       features fp32 [B, T, F] -> S16 [B, Ho, Wo, round_up(C, 16)] = relu(conv7x7(stride 3, zero padding 1) + bias), H =
 *                             frequency, W = time, Ho = (F + 2 - 7) / 3 + 1, Wo likewise from T; w fp32 [C][49] (BatchNorm folded), products
 *                             accumulated in fp32 in one fixed tap order; channels C .. of the last unit are exact zeros.  F >= 5, T >= 5 (where
 *                             torch's Conv2d refuses too), C a multiple of 8, at most 256.
 *   mv_conv2d_stem7_peak_s16  the same with the optional device word `peak` of MvConv2dsDesc.peak (largest |64 * value| before the clamp).
 *   mv_maxpool3s2_s16         MaxPool2d(3, stride 2, padding 1): Ho = (H - 1) / 2 + 1, Wo likewise; taps outside the map take no part; the output
 *                             pixel is the (hi, lo) pair of the window's largest merged value, copied as it is; padded channels of the last unit
 *                             are zero bits.
 *   mv_avgpool3_s16           AvgPool2d(3, stride 1 | 2, padding 1, count_include_pad): the merged values of the taps inside the map summed in fp32
 *                             in a fixed order, divided by 9 and split again.
 * x and y may be channel slices of wider maps: a pointer at a 16-channel unit with the map's leading dimension.
 * ------------------------------------------------------------------------------------------------ */
int mv_conv2d_stem7_s16(const float* feats, void* out, const float* w, const float* bias, int32_t B, int32_t T, int32_t F, int32_t C,
                        mv_stream_t stream);
int mv_conv2d_stem7_peak_s16(const float* feats, void* out, const float* w, const float* bias, int32_t B, int32_t T, int32_t F, int32_t C,
                             uint32_t* peak, mv_stream_t stream);
int mv_maxpool3s2_s16(const void* x, int64_t ldx, void* y, int64_t ldy, int32_t B, int32_t H, int32_t W, int32_t C, mv_stream_t stream);
int mv_avgpool3_s16(const void* x, int64_t ldx, void* y, int64_t ldy, int32_t B, int32_t H, int32_t W, int32_t C, int32_t stride,
                    mv_stream_t stream);

/* pack [Cout][Cin][k] fp32 (nn.Conv1d layout) -> fp16 [Cout_pad][k][Cin_pad]; returns element count */
int64_t mv_conv1d_packed_elems(int32_t cout, int32_t cin, int32_t k);
int mv_conv1d_pack_weight(const float* w, int32_t cout, int32_t cin, int32_t k, void* packed_f16, mv_stream_t stream);

typedef struct MvConv1dDesc {
    /* y[b, t, co] = epilogue( sum_{j, ci} W[co, j, ci] * in(b, t*stride - pad + j*dilation, ci) )
     * in(.) = x (+ x2) optionally passed through relu(x*in_scale+in_shift); channel-last tensors. */
    const void* x;        /* [B, T_in, ldx] */
    const void* x2;       /* optional second input added to x (Res2Net: ecapa_tdnn.py:47), same ld/dtype */
    int32_t x_dtype;      /* MV_DT_F32 | MV_DT_F16 */
    int64_t ldx;          /* elements between consecutive time steps of x (>= cin) */
    int64_t ldx2;
    const float* in_scale; /* optional [cin]: pre-activation BatchNorm folded (campplus.py:139-141) */
    const float* in_shift;
    const void* w_packed; /* from mv_conv1d_pack_weight */
    const float* bias;    /* optional [cout] */
    const float* row_bias;/* optional [B, cout]: per-utterance bias (hoisted ASP context, pooling.py:110-117) */
    int32_t pre_act;      /* activation applied to (acc + bias) BEFORE the affine (TDNNBlock: ReLU, models/utils.py:138) */
    const float* scale;   /* optional [cout] folded BatchNorm scale */
    const float* shift;
    int32_t post_act;     /* activation after the affine */
    const float* gate;    /* optional [B, n_seg, cout] multiplicative gate (CAM mask, campplus.py:94-99) */
    int32_t gate_seg_len; /* frames per gate segment */
    void* y;              /* [B, T_out, ldy] */
    int32_t y_dtype;
    int64_t ldy;
    const void* add_src;  /* optional fp16 [B, T_out, ld_add]: second output sum_dst = y + add_src, i.e. the input */
    void* sum_dst;        /* x_{j+1} + y_j of the next Res2Net step (ecapa_tdnn.py:47) produced by this step's epilogue */
    int64_t ld_add, ld_sum;
    int32_t B, T_in, T_out, cin, cout, k, dilation, stride, pad, pad_mode;
    int32_t tile;         /* workgroup tile: 0 = choose (256x256 for wide layers that fill the chip, 64x64 for small problems, else 128x128 / 128x160), 64, 128, 160, 256 */
    /* optional fused time statistics of y (SE squeeze ecapa_tdnn.py:79, ASP global mean / std pooling.py:104-109): fp32 partial
     * buffers of mv_conv1d_stats_elems(B, T_out, cout) floats each; stat_sq may be NULL (mean only).  Only on the persistent
     * 1x1 path: fp16 in/out, cout % 256 == 0, cin % 64 == 0, no row_bias / gate, T_out >= 64.  Finish with
     * mv_conv1d_stats_finish. */
    float* stat_sum;
    float* stat_sq;
    /* optional fused time statistics of the INPUT x (the ASP global mean / std, pooling.py:104-109, taken from the x tiles the hidden
     * 1x1 conv of the attention streams through LDS anyway): fp32 partial buffers of mv_conv1d_in_stats_elems(B, T_in, cin) floats
     * each (sums and sums of squares per (utterance, 160-frame tile, channel)).  Only on the direct fp16 path with the 128 x 160 tile:
     * k = 1, stride 1, no padding, T_out == T_in, cout <= 128, no x2 / in_scale.  Finish with mv_conv1d_in_stats_finish. */
    float* in_stat_sum;
    float* in_stat_sq;
    int32_t persist_blocks_hint;  /* 0 = one resident workgroup per CU; otherwise that many (rounded up to 8) workgroups walk the tiles of the
                                   * persistent kernels -- tests make small problems walk several tiles per workgroup; never the bits of a result
                                   * (since ABI 4; replaces the MV_CONV_PERSIST_BLOCKS environment hook: no getenv is left in the library) */
    uint64_t* clock_probe;        /* since ABI 5, optional: device array [resident workgroups (<= CUs rounded up to 8)][4].  The dense 1x1 persistent
                                   * (ring) kernel leaves {shader-clock cycles at entry, at exit, 100 MHz reference at entry, at exit} of every
                                   * workgroup there: (exit - entry cycles) / (exit - entry reference ticks) x 100 MHz = the shader clock the launch
                                   * SUSTAINED (bench.py's `box` block prices the 2.5 PFLOP/s peak's 2.4 GHz against it).  Other kernels ignore it. */
} MvConv1dDesc;
int mv_conv1d_forward(const MvConv1dDesc* d, mv_stream_t stream);
/* Grouped 1-D convolution (nn.Conv1d(groups = g), the `groups` of TDNNBlock, mvector/models/utils.py:120-138).  The weight is the grouped nn.Conv1d
 * layout fp32 [cout][cin / g][k]; d->cin / d->cout are the layer's whole widths.  Two forms, chosen by the geometry alone:
 *   native    (mv_conv1d_grouped_native = 1: k = 1, cin / g a multiple of 64, cout / g a multiple of 128): the weights are packed PER GROUP
 *             (fp16 [cout_pad][cin / g], the dense packing of the grouped weight), and every tile of output channels -- all inside one group --
 *             reads only its group's K slice of x, columns (co / (cout / g)) * (cin / g) .. + cin / g: a grouped GEMM that multiplies no zero block.
 *             Groups of 256 and more output channels run on the dense layers' persistent ring kernel where those do (conv1d_ring_grouped_kernel),
 *             narrower ones on the one-shot 128-channel tiles.  fp16 x only: no x2, in_scale / in_shift or fused statistics.
 *   expanded  (everything else: narrower groups, k > 1): the pack call writes the block-diagonal dense [cout][k][cin] weight and the forward is
 *             the dense one -- the zero weights add exact zeros, so the result is the grouped convolution's, at the dense layer's cost.
 * mv_conv1d_grouped_packed_elems: fp16 elements of the packed weight (-1 when cin or cout is not divisible by g).  groups = 1 is the dense layer. */
int32_t mv_conv1d_grouped_native(int32_t cout, int32_t cin, int32_t k, int32_t groups);
int64_t mv_conv1d_grouped_packed_elems(int32_t cout, int32_t cin, int32_t k, int32_t groups);
int mv_conv1d_pack_weight_grouped(const float* w, int32_t cout, int32_t cin, int32_t k, int32_t groups, void* packed_f16, mv_stream_t stream);
int mv_conv1d_forward_grouped(const MvConv1dDesc* d, int32_t groups, mv_stream_t stream);
/* Which kernels mv_conv1d_forward / mv_conv1d_forward_grouped (groups as passed there) would launch for `d`, without launching (additive since
 * ABI 5).  cus = 0 plans for the current device; any other value for a chip of that many compute units.  The descriptor goes through the same checks
 * and the same plan as a forward call, so a refused descriptor returns that call's error code and message.  The names are the rows of csrc/conv1d.hip's
 * kernel table as spelled there ("CK_GLDS_128", ...), static strings owned by the library; in_stats_kernel is "CK_IN_STATS" when the input statistics
 * run as a launch of their own in front of the conv, tail_kernel the kernel of the ring walk's last partial round (tail_nv tiles, each cut
 * tail_split x tail_split); both are "" when there is no such launch.  n_tiles x co_tiles: the main kernel's tiles over rows and output channels;
 * grid: its workgroups. */
typedef struct MvConv1dPlanInfo {
    const char* kernel;
    const char* in_stats_kernel;
    const char* tail_kernel;
    int32_t n_tiles, co_tiles, grid, tail_nv, tail_split;
} MvConv1dPlanInfo;
int mv_conv1d_plan_info(const MvConv1dDesc* d, int32_t groups, int32_t cus, MvConv1dPlanInfo* out);
/* floats in one partial-statistics buffer, and the reduction of the partial rows to per-utterance mean[b, c] (and
 * std[b, c] = sqrt(max(E[(y - mean)^2], clamp_eps)) when stat_sq / std are given).  `shift` = the BatchNorm shift passed to the
 * conv (the moments are taken about it), NULL if the conv had none. */
int64_t mv_conv1d_stats_elems(int32_t B, int32_t T_out, int32_t cout);
/* per-utterance mean[b, c] and std[b, c] = sqrt(max(E[x^2] - mean^2, clamp_eps)) of the conv INPUT from the in_stat_* partials */
int64_t mv_conv1d_in_stats_elems(int32_t B, int32_t T_in, int32_t cin);
int mv_conv1d_in_stats_finish(const float* in_stat_sum, const float* in_stat_sq, int32_t B, int32_t T_in, int32_t cin, float* mean,
                              float* std, int64_t ld_out, float clamp_eps, mv_stream_t stream);
int mv_conv1d_stats_finish(const float* stat_sum, const float* stat_sq, const float* shift, int32_t B, int32_t T_out, int32_t cout,
                           float* mean, float* std, int64_t ld_out, float clamp_eps, mv_stream_t stream);

/* Fused Res2Net chain (mvector/models/ecapa_tdnn.py:39-51): x, y fp16 [B, T, C]; `groups` channel groups of width C/groups;
 * y[..., 0:w] = x[..., 0:w];  y_j = BN(ReLU(conv_j(x_j + y_{j-1}))) for j = 1..groups-1 with reflect "same" padding.
 * Arrays of groups-1 pointers (host arrays of device pointers): packed weights, bias, folded BN scale / shift.
 * One workgroup per utterance up to 320 frames; longer utterances are cut into chunks of equal length that carry the chain's receptive field
 * ((groups-1) * dilation * (k-1)/2 frames) as halo on either side, one workgroup each.  Returns MV_ERR_UNSUPPORTED unless width is 64 or 128. */
int mv_res2net_chain_f16(const void* x, void* y, const void* const* w_packed, const float* const* bias,
                         const float* const* scale, const float* const* shift, int32_t B, int32_t T, int32_t C,
                         int32_t groups, int32_t k, int32_t dilation, mv_stream_t stream);

/* y[b, o] = act( sum_k x[b, k] * w[o, k] + bias[o] ) in exact fp32 (f32 MFMA).
 * ONE summation order per ENTRY POINT, not across them: this call sums K in one sweep (the direct kernel); mv_linear_f32_ws with a sufficient
 * workspace sums layers of K >= 2048 as slices of 384 added in slice order (what the model handles run) -- the two differ in the last bits
 * (~1e-7 relative) on such layers, and mv_linear_f32_ws with a NULL / short workspace IS this call.  "A row's bits depend on the row only"
 * holds within either form for every batch size; a caller that compares bits across the two forms must pick one. */
int mv_linear_f32(const float* x, int64_t ldx, const float* w, const float* bias, int32_t act, float* y, int64_t ldy,
                  int32_t B, int32_t K, int32_t O, mv_stream_t stream);
/* The same layer with a caller workspace (ABI 4): long reductions (K >= 2048, any number of rows: the [256, 6144] x [192, 6144] final layer of
 * EcapaTdnn-1024) run as K slices of 384 on 32 x 32 output tiles + a second launch that adds the slices' partial sums in slice order -- a fixed order,
 * so a row's bits depend on the row only.  mv_linear_f32_workspace_floats = floats that form needs (0: the direct kernel runs either way); with a
 * NULL or short workspace the call is mv_linear_f32. */
size_t mv_linear_f32_workspace_floats(int32_t B, int32_t K, int32_t O);
int mv_linear_f32_ws(const float* x, int64_t ldx, const float* w, const float* bias, int32_t act, float* y, int64_t ldy, int32_t B, int32_t K, int32_t O,
                     float* workspace, size_t workspace_floats, mv_stream_t stream);

/* mean (and optionally std = sqrt(clamp(E[(x-mean)^2], eps)), or unbiased std) over time of a
 * channel-last fp16 tensor [B, T, ld] -> fp32 [B, C].  std may be NULL. */
int mv_time_stats_f16(const void* x, int64_t ld, int32_t B, int32_t T, int32_t C, float* mean, float* std,
                      int32_t unbiased, float clamp_eps, mv_stream_t stream);

/* Pre-activation written out once: y[n, c] = fp16(relu(x[n, c] * scale[c] + shift[c])) over channel-last fp16 rows (eval BatchNorm
 * folded to scale / shift + ReLU in front of a 1x1 conv: the CAM++ transit layers, mvector/models/campplus.py:186-189), so that the
 * conv behind it takes the direct global -> LDS path instead of transforming on load.  C % 8 == 0, 16-byte aligned rows / parameters. */
int mv_bn_relu_rows_f16(const void* x, int64_t ldx, const float* scale, const float* shift, void* y, int64_t ldy, int64_t n_rows,
                        int32_t C, mv_stream_t stream);

/* The time reductions and element-wise row passes between the GEMMs of the backbones, one entry point per launcher of the model forwards (added
 * within ABI 5: layer-level entry points of the parity tests).  fp16 rows are channel-last and 16-byte aligned (pointer and pitch) unless noted; a call
 * a launcher cannot run returns MV_ERR_INVALID_ARGUMENT and launches nothing.  A NaN input gives a NaN output in every one of them; values beyond
 * the fp16 range saturate at +-65504.
 *   mv_time_stats_ex_f16     mv_time_stats_f16 with every argument of the launcher: the output pitch ld_out >= C (CAM++ StatsPool writes mean | std into
 *                            one [B, 2C] row: std = mean + C, ld_out = 2C) and the optional pre-activation v = relu(x * in_scale[c] + in_shift[c])
 *                            (both NULL: none).  x needs ld % 8 == 0 only; a C that is no multiple of 8 takes scalar loads in its last lane.
 *   mv_seg_mean_f16          ctx[b, s, c] = mean_t x[b, t, c] + mean over segment s of seg_len frames (the last one over its true length), fp32
 *                            [B, ceil(T / seg_len), C]; C % 8 == 0.
 *   mv_se_gate_residual_f16  out[n, c] = fp16(gate[b(n), c] * y[n, c] + res[n, c]) over n = b * T + t; gate fp32 [B, C]; out and res may be column
 *                            slices of one buffer as long as they do not overlap; C % 8 == 0.
 *   mv_asp_hidden_act_f16    zh[b, t, a] = fp16(tanh(relu(zh[b, t, a] + row_bias[b, a]) * scale[a] + shift[a])) in place on [B * T, A], A % 8 == 0.
 *   mv_cast_pad_f16          dst[b, t', 0:F] = fp16(src[b, reflect(t' - pad), 0:F]) for t' in [0, T + 2 pad), columns F..ldd-1 zero; src fp32
 *                            [B, T, F] (16-byte aligned when ldd == F, which needs F % 8 == 0; any F and 4-byte alignment when ldd = round_up(F, 8)).
 *   mv_cast_rows_f16         dst[n, 0:C] = fp16(src[n, 0:C]), columns C..ldd-1 zero; src fp32 at pitch lds >= C, no alignment beyond the element's.
 *   mv_copy_slice_f16        dst[n, 0:C] = src[n, 0:C] between fp16 rows of different pitch; C % 8 == 0.
 *   mv_pad_rows_f32          dst[n, 0:F] = src[n, 0:F] (fp32 rows of width F, exact copy), columns F..ldd-1 zero; ldd % 4 == 0, dst 16-byte aligned. */
int mv_time_stats_ex_f16(const void* x, int64_t ld, int32_t B, int32_t T, int32_t C, float* mean, float* std, int64_t ld_out, int32_t unbiased,
                         float clamp_eps, const float* in_scale, const float* in_shift, mv_stream_t stream);
int mv_seg_mean_f16(const void* x, int64_t ld, int32_t B, int32_t T, int32_t C, int32_t seg_len, float* ctx, mv_stream_t stream);
int mv_se_gate_residual_f16(const void* y, int64_t ldy, const float* gate, const void* res, int64_t ldr, void* out, int64_t ldo, int32_t B,
                            int32_t T, int32_t C, mv_stream_t stream);
int mv_asp_hidden_act_f16(void* zh, const float* row_bias, const float* scale, const float* shift, int32_t B, int32_t T, int32_t A,
                          mv_stream_t stream);
int mv_cast_pad_f16(const float* src, void* dst, int32_t B, int32_t T, int32_t F, int64_t ldd, int32_t pad, mv_stream_t stream);
int mv_cast_rows_f16(const float* src, int64_t lds, void* dst, int64_t ldd, int64_t n_rows, int32_t C, mv_stream_t stream);
int mv_copy_slice_f16(const void* src, int64_t lds, void* dst, int64_t ldd, int32_t C, int64_t n_rows, mv_stream_t stream);
int mv_pad_rows_f32(const float* src, int32_t F, float* dst, int64_t ldd, int64_t n_rows, mv_stream_t stream);

/* Per-kernel-class timing with HIP events recorded on the launch stream (used by bench.py for its roofline legs; off by
 * default, not thread-safe).  work = algorithmic FLOPs (MV_PROF_CONV1D: 2*B*T_out*cin*cout*k per launch) or algorithmic
 * bytes (MV_PROF_FBANK: B*(4*L + 4*T*num_mel_bins) per launch).  mv_profile_read waits for the recorded launches. */
#define MV_PROF_CONV1D 0
#define MV_PROF_FBANK 1
#define MV_PROF_CONV2D 2 /* work = 2*B*Ho*Wo*cin*cout*ks*ks FLOPs on the layer's own (unpadded) channel counts */
#define MV_PROF_CONV1D_RING 3 /* since ABI 5: the launches of the dense 1x1 persistent (ring) GEMM alone -- a subset of MV_PROF_CONV1D, which keeps counting them */
#define MV_PROF_MARGIN_SUMS 4 /* since ABI 5: the second pass of mv_margin_ce_forward over the logits (margin_seg_kernel<.., 1>); work = the logits' bytes */
int mv_profile_enable(int32_t on);
int mv_profile_read(int32_t kernel_class, int32_t* calls, double* total_ms, double* total_work, int32_t reset);

/* int16 PCM rows [B, L] -> float32 waveforms in [-1, 1) (sample / 32768) on the device, zero beyond num_samples[b] (device
 * int64 array, NULL = L everywhere).  normalize != 0: per-row dB normalisation over the true length, gain =
 * 10^((target_db - 10 log10(mean x^2)) / 20) -- AudioSegment.normalize as called at mvector/predict.py:210-211; rows whose gain
 * would exceed max_gain_db (digital silence; the reference raises ValueError) are left unscaled and flagged in too_quiet[b]
 * (device int32 array, may be NULL). */
int mv_wave_prepare_i16(const int16_t* pcm, int64_t pcm_stride, const int64_t* num_samples, int32_t B, int64_t L, int32_t normalize,
                        float target_db, float max_gain_db, float* wav, int64_t wav_stride, int32_t* too_quiet, mv_stream_t stream);

/* ------------------------------------------------------------------------------------------------
 * 16-bit PCM of another rate and channel count -> mono float32 waveforms at the target rate (added within ABI 5): the channel mean, the
 * resampling and the dB normalisation that mvector/predict.py:185-212 does per file on the host (AudioSegment.from_file, resample, normalize).
 *   x[i] = (float)(sum_c pcm[i, c]) * (1 / 32768) / channels -- the bits of (pcm.astype(float32) / 32768).mean(axis=1);
 *   g = gcd(dst, src), up = dst / g, down = src / g, half = 10 max(up, down),
 *   h = scipy.signal.firwin(2 half + 1, 1 / max(up, down), window=('kaiser', 5.0)) * up, designed in fp64 and rounded to fp32 -- the filter of
 *   scipy.signal.resample_poly(x, up, down) with its defaults;
 *   y[m] = sum_j x[j] h[m down + half - j up] for 0 <= m < n_out = ceil(n_in up / down): zero padding at both ends, the group delay removed.
 * Every output is ONE fp32 fmaf chain over its K = ceil((2 half + 1) / up) taps, in the order j = (m down + half) / up downwards: a row's
 * bits depend on its own samples only -- not on the batch, the stream or the call.  up = down = 1 (a pure down-mix) copies x.
 * The handle owns the table and no mutable state: one handle may drive several streams at once.
 * ------------------------------------------------------------------------------------------------ */
#define MV_RESAMPLER_MAX_RATE 1024 /* largest max(up, down) mv_resampler_create takes */
typedef struct MvResampler MvResampler;
typedef struct MvResamplerInfo {
    int32_t up, down, half, K; /* as defined above */
    int32_t tile;              /* outputs of a row one workgroup computes (tile edges are row-relative) */
    int32_t table_in_lds;      /* 0: the ratio's table and source span do not fit into LDS together, the table is read from global memory */
} MvResamplerInfo;
/* refused by name: a rate <= 0; max(up, down) > MV_RESAMPLER_MAX_RATE */
int mv_resampler_create(int32_t src_rate, int32_t dst_rate, MvResampler** out);
int mv_resampler_destroy(MvResampler* h);
int mv_resampler_info(const MvResampler* h, MvResamplerInfo* info);
/* the 2 half + 1 fp32 coefficients in filter order into HOST memory (n must be 2 half + 1; for up = down = 1 the unit impulse) */
int mv_resampler_taps(const MvResampler* h, float* taps_host, int32_t n);
int64_t mv_resampler_out_len(const MvResampler* h, int64_t n_in); /* ceil(n_in up / down) */
size_t mv_resampler_workspace_bytes(const MvResampler* h, int32_t B, int64_t L_in);
/* pcm: interleaved int16 frames [B, L_in, channels], rows pcm_stride ELEMENTS apart (no alignment beyond int16's is assumed), channels 1 .. 8;
 * num_frames: device int64 [B] or NULL (= L_in), clamped to [0, L_in].  wav: [B, L_out] fp32 rows wav_stride apart, L_out >=
 * mv_resampler_out_len(L_in); row b holds its n_out = out_len(num_frames[b]) samples and zeros behind them.  num_out (device int64 [B], may be
 * NULL) receives n_out.  normalize / target_db / max_gain_db / too_quiet: the dB normalisation of mv_wave_prepare_i16 (same gain formula, same
 * flags), the mean square taken over the row's n_out resampled samples: per-tile partial sums (fp32 over a thread's <= 4 outputs, fp64 across)
 * go to the workspace, a second launch adds them in a fixed order and scales the row.  workspace: device memory, 8-byte aligned, of the size the
 * companion reports; nothing is allocated per call and no workgroup waits for another. */
int mv_resampler_forward_i16(const MvResampler* h, const int16_t* pcm, int64_t pcm_stride, int32_t channels, const int64_t* num_frames, int32_t B,
                             int64_t L_in, int32_t normalize, float target_db, float max_gain_db, float* wav, int64_t wav_stride, int64_t L_out,
                             int64_t* num_out, int32_t* too_quiet, void* workspace, size_t workspace_bytes, mv_stream_t stream);

/* ------------------------------------------------------------------------------------------------
 * Speaker diarization behind the embeddings (mvector/infer_utils/speaker_diarization.py; added within ABI 5).
 * Every sum runs in one fixed order: results are bit-identical from run to run and on any stream.
 * ------------------------------------------------------------------------------------------------ */
/* Chunk rows out of ONE resident waveform wav[L] (fp32): rows[i] = wav[start[i] : start[i] + len[i]] followed by zeros up to chunk_len
 * (start / len: device int64 arrays of n entries, clamped to the waveform and to chunk_len).  normalize != 0: the dB normalisation of
 * the int16 entry point above with the same gain formula, max_gain_db and too_quiet flags, the mean square (an fp64 sum) taken over all
 * chunk_len samples, zeros included -- the reference's predict_batch normalises the already padded chunk. */
int mv_wave_chunks_f32(const float* wav, int64_t L, const int64_t* start, const int64_t* len, int32_t n, int64_t chunk_len, int32_t normalize,
                       float target_db, float max_gain_db, float* rows, int64_t rows_stride, int32_t* too_quiet, mv_stream_t stream);

/* Cosine matrix S [N, N] fp32 -> M [N, N] fp32 and degree [N] fp64 (SpectralCluster.p_pruning, the symmetrisation and get_laplacian):
 * per row the n_prune smallest entries are dropped (n_prune = the reference's int((1 - pval) * N), computed by the caller); among equal
 * values the LOWER column index is dropped first (numpy's default argsort leaves the order of ties open: this rule is the library's);
 * M_ij = 0.5f * (kept_ij ? S_ij : 0 + kept_ji ? S_ji : 0) in fp32, M_ii = 0; degree_i = sum_j |M_ij| in fp64.
 * 1 <= N <= 16384 (a row of keys is 64 KiB of LDS there and M is 1 GiB), 0 <= n_prune < N; M must not alias S.  workspace: device
 * memory of the size the companion function reports (0 for an N it refuses). */
size_t mv_affinity_laplacian_workspace_bytes(int32_t N);
int mv_affinity_laplacian_f32(const float* S, int32_t N, int32_t n_prune, float* M, double* degree, void* workspace, size_t workspace_bytes,
                              mv_stream_t stream);

/* The m lowest eigenpairs of L = diag(degree) - M (M fp32 [N, N] symmetric with a zero diagonal, degree fp64 [N], both on the device) by
 * Chebyshev-filtered subspace iteration in fp64 on a block of vectors: seeded fixed start block, then per iteration a scaled Chebyshev filter
 * of the given degree that damps [largest Ritz value, ub], ub = 2 max degree; Cholesky-QR twice on column-scaled vectors; Rayleigh-Ritz;
 * stop when the largest residual |L v_i - lambda_i v_i|_2 of the m wanted columns is <= tol * ub.  On a non-positive Cholesky pivot the
 * iteration is repeated from the last Ritz vectors with half the filter degree (counted in MvEigInfo.retries).
 * lambdas [m] (ascending) and info are HOST memory; vecs [N, m] fp64 row-major is device memory.  The b x b problems are solved on the
 * host between launches: THIS CALL SYNCHRONISES ITS STREAM (several times) and has returned its results when it returns.
 * 2 <= N <= 16384, 1 <= m <= min(16, N), block 0 (= min(32, N)) or m .. min(32, N).  Out of iterations: MV_ERR_NOT_CONVERGED, with lambdas,
 * vecs and info holding the last Ritz pairs.  workspace: device memory, 16-byte aligned, of the size the companion reports (0 for a cfg it
 * refuses); nothing is allocated on the device per call. */
typedef struct MvEigCfg {
    int32_t m;         /* wanted eigenpairs */
    int32_t block;     /* vectors iterated; 0 = min(32, N) */
    int32_t degree;    /* Chebyshev filter degree = products with L per iteration besides the Rayleigh-Ritz one */
    int32_t max_iters;
    double tol;        /* relative to ub */
    uint64_t seed;     /* of the start block */
} MvEigCfg;
typedef struct MvEigInfo {
    int32_t iterations;
    int32_t products;  /* block products with L */
    int32_t retries;   /* iterations repeated with half the filter degree */
    int32_t converged;
    double residual;   /* largest of the m wanted columns, absolute */
    double ub;         /* 2 max degree */
} MvEigInfo;
void mv_laplacian_eig_default_cfg(MvEigCfg* cfg); /* m 16, block 0, degree 16, max_iters 60, tol 1e-6 */
size_t mv_laplacian_eig_lowest_workspace_bytes(int32_t N, const MvEigCfg* cfg);
int mv_laplacian_eig_lowest(const float* M, const double* degree, int32_t N, const MvEigCfg* cfg, double* lambdas, double* vecs, MvEigInfo* info,
                            void* workspace, size_t workspace_bytes, mv_stream_t stream);

/* ------------------------------------------------------------------------------------------------
 * Verification metrics of an evaluation (mvector/metric/metrics.py behind MVectorTrainer.evaluate; added within ABI 5).
 * Integer counts and single fp64 operations only: results are bit-identical from run to run and on any stream.  Every step is a chain
 * of ordinary launches ordered by the stream; no workgroup waits for another one.
 * ------------------------------------------------------------------------------------------------ */
/* Ascending stable sort of N fp32 scores with their flat indices: sorted_scores[i] = scores[sorted_index[i]], in the order of
 * numpy.argsort(scores, kind='stable') -- equal scores (-0 == +0 among them) keep their index order, NaNs of either sign come last in
 * index order.  A -0 comes out as +0 and a NaN as the quiet NaN 0x7FFFFFFF; every other value keeps its bits.
 * LSD radix sort over four 8-bit digits of the order-preserving key, tiles of mv_sort_scores_tile() keys.  1 <= N <= 2^31 - 1.
 * scores, sorted_scores [N] and sorted_index [N] are distinct device buffers; workspace: device memory, 16-byte aligned, of the size the
 * companion reports (0 for an N it refuses). */
int32_t mv_sort_scores_tile(void);
size_t mv_sort_scores_workspace_bytes(int64_t N);
int mv_sort_scores_f32(const float* scores, int64_t N, float* sorted_scores, uint32_t* sorted_index, void* workspace, size_t workspace_bytes,
                       mv_stream_t stream);

/* EER, minDCF and threshold ingredients of the score matrix scores [n_trials, n_enroll] (fp32, row-major, device), trial (i, j) being a
 * target when trial_labels[i] == enroll_labels[j] (device int32 arrays).  With the N = n_trials * n_enroll scores in stable ascending order,
 * T_i = targets among positions 0 .. i, I_i = i + 1 - T_i, and in fp64, each operation rounded once (no contraction):
 *   fnr_i = T_i / NT,  fpr_i = 1 - I_i / NI,  c_i = (c_miss * fnr_i) * p_target + (c_fa * fpr_i) * (1 - p_target)
 * the result holds i1 = the first i with fnr_i - fpr_i >= 0 (-1: none), i2 = the last i with fnr_i - fpr_i < 0 (-1: none), T at both,
 * min_i c_i and the score at sorted position i1.  The interpolation of the EER and the division by the default cost are the caller's
 * (metrics.verification_metrics).  No target or no impostor trial is reported (n_target / n_impostor = 0; the other fields then mean
 * nothing), not refused.  sorted_scores [N] fp32 and tgt_cum [N] uint32 (= T) are optional device outputs (NULL: not written).
 * result is HOST memory: THIS CALL SYNCHRONISES ITS STREAM and has returned its result when it returns.  1 <= N <= 2^31 - 1,
 * 0 < p_target < 1, c_miss >= 0, c_fa >= 0.  workspace: device memory, 16-byte aligned, of the size the companion reports (0 for a shape
 * it refuses); nothing is allocated per call. */
typedef struct MvVerifCfg {
    double p_target;
    double c_miss;
    double c_fa;
} MvVerifCfg;
typedef struct MvVerifResult {
    int64_t n_target;    /* NT */
    int64_t n_impostor;  /* NI */
    int64_t i1;
    int64_t i2;
    int64_t tgt_i1;      /* T at i1 */
    int64_t tgt_i2;      /* T at i2 */
    double min_cost;     /* min_i c_i, not yet divided by the default cost */
    float score_i1;      /* the threshold */
    int32_t reserved;
} MvVerifResult;
size_t mv_verif_metrics_workspace_bytes(int64_t n_trials, int64_t n_enroll);
int mv_verif_metrics_f32(const float* scores, int64_t n_trials, int64_t n_enroll, const int32_t* trial_labels, const int32_t* enroll_labels,
                         const MvVerifCfg* cfg, MvVerifResult* result, float* sorted_scores, uint32_t* tgt_cum, void* workspace,
                         size_t workspace_bytes, mv_stream_t stream);

/* Attentive-statistics pooling tail (mvector/models/pooling.py:117-125): attention logits = W2 . h (the bias of the
 * projection is constant over time and cancels in the softmax over time), softmax over time, weighted mean / std.
 *   h  fp16 [B, T, A] (tanh output, |h| <= 1),  w2_packed = mv_conv1d_pack_weight of  W2[C, A, 1] * log2(e),
 *   x  fp16 [B, T, ldx],  gmean fp32 [B, gmean_ld] or NULL (centre of the second moment),  out fp32 [B, 2C] = mean | std.
 * logit_bound_log2 = max_c sum_k |W2[c,k]| * log2(e) selects the form without max subtraction when it is in [0, 60];
 * pass a negative value for the online-softmax form (any weights). */
int mv_asp_pool_f16(const void* h, const void* w2_packed, const void* x, int64_t ldx, const float* gmean, int64_t gmean_ld,
                    float* out, int32_t B, int32_t T, int32_t C, int32_t A, float logit_bound_log2, mv_stream_t stream);

/* Self-attentive pooling tail (the SAP head, pooling.py:50-65): the mean-only form of mv_asp_pool_f16 on the same kernels.
 *   h  fp16 [B, T, A] = tanh(W1 . x + b1) (the conv1d layer with its bias and MV_ACT_TANH),  w2_packed = mv_conv1d_pack_weight of linear2's
 *   W2[C, A, 1] * log2(e) (its bias is constant over time and cancels in the softmax),  x fp16 [B, T, ldx],  out fp32 [B, C] = sum_t softmax_t(W2 . h) x.
 * logit_bound_log2 as mv_asp_pool_f16. */
int mv_sap_pool_f16(const void* h, const void* w2_packed, const void* x, int64_t ldx, float* out, int32_t B, int32_t T, int32_t C, int32_t A,
                    float logit_bound_log2, mv_stream_t stream);
/* Mean and UNBIASED variance over time (the TSP head, pooling.py:29-47) of a channel-last fp16 tensor [B, T, ld] (ld % 8 == 0, 16-byte
 * aligned rows): out[b * ld_out + c] = mean, out[b * ld_out + C + c] = var (ld_out >= 2C).  Centred two-pass form, a fixed summation order per
 * (utterance, channel) whatever B is; a constant channel has variance exactly 0, and T = 1 gives NaN (0 / 0, as torch.var). */
int mv_time_mean_var_f16(const void* x, int64_t ld, int32_t B, int32_t T, int32_t C, float* out, int64_t ld_out, mv_stream_t stream);

/* One 3x3 Conv2d of the CAM++ front-end (FCM, mvector/models/campplus.py:221-292: BasicResBlock.conv1 / conv2 (+ shortcut) and
 * FCM.conv2) on channel-last fp16 maps with 32 feature maps, eval BatchNorm already folded into w / bias, ReLU at the end:
 *   x  fp16 [B, Fin, T, 32];  stride sf (1 | 2) on the frequency axis, zero padding 1;  y fp16, element (b, fo, t, co) at
 *   y + b * y_sB + fo * y_sF + t * y_sT + co (strides in elements);  Fout = (Fin - 1) / sf + 1;
 *   w  fp16 [9 or 10][32 co][32 ci], tap = 3 * df + dt;  bias fp32 [32];
 *   mode2 = 0: none;  1: tenth tap = the block's strided 1x1 shortcut conv (+BN) on x2 [B, F2, T, 32] at row fo * sf2;
 *   2: identity residual, x2 added before the ReLU.  Layer-level entry point of the parity tests. */
int mv_fcm_conv3x3_f16(const void* x, int32_t Fin, int32_t sf, const void* x2, int32_t F2, int32_t sf2, int32_t mode2, const void* w,
                       const float* bias, void* y, int64_t y_sB, int64_t y_sF, int64_t y_sT, int32_t B, int32_t T, int32_t Fout,
                       mv_stream_t stream);

/* One BasicResBlock of the CAM++ front-end (mvector/models/campplus.py:221-254) as ONE launch:
 *   mid = ReLU(BN1(conv3x3, stride (sf, 1))(x)),  y = ReLU(BN2(conv3x3)(mid) + shortcut(x));  the intermediate map stays on the chip.
 *   x fp16 [B, Fin, T, 32];  Fout = (Fin - 1) / sf + 1;  y element (b, fo, t, co) at y + b * y_sB + fo * y_sF + t * y_sT + co;
 *   w1 fp16 [9][32 co][32 ci] (tap = 3 * df + dt, BN1 folded), b1 fp32 [32];  w2 fp16 [9 | 10][32][32] (BN2 folded), b2 fp32 [32];
 *   shortcut != 0: tap 9 of w2 is the block's strided 1x1 shortcut conv with its BatchNorm folded (its shift is part of b2);
 *   shortcut == 0: identity residual (sf must be 1). */
int mv_fcm_block_f16(const void* x, int32_t Fin, int32_t sf, const void* w1, const float* b1, const void* w2, const float* b2,
                     int32_t shortcut, void* y, int64_t y_sB, int64_t y_sF, int64_t y_sT, int32_t B, int32_t T, mv_stream_t stream);

/* The FIRST BasicResBlock of the CAM++ front-end together with the conv in front of it (campplus.py:262-264,283-285: head.conv1 + bn1 +
 * ReLU, then head.layer1[0], stride (2, 1) with its shortcut conv) as ONE launch: the 32-map image of the features is evaluated inside the
 * kernel and never written.  feats fp32 [B, T, F];  c1a = mv_fcm_c1_pack of the folded conv weights, c1b fp32 [32] = the folded BN shift;
 * the other arguments as mv_fcm_block_f16 with sf = 2, shortcut = 1.  The conv weights act as fp16 (like every other conv of the fp16
 * head), the features exactly (as x_hi + x_lo). */
int mv_fcm_block_c1_f16(const float* feats, int32_t F, const void* c1a, const float* c1b, const void* w1, const float* b1, const void* w2,
                        const float* b2, void* y, int64_t y_sB, int64_t y_sF, int64_t y_sT, int32_t B, int32_t T, mv_stream_t stream);
/* host -> host: w fp32 [32 maps][3 mel taps][3 time taps] (BatchNorm scale folded) -> out fp16 [2][64][8], the MFMA operand order of the kernel */
int mv_fcm_c1_pack(const float* w, void* out);

/* The dense layers of one CAM++ block (CAMDenseTDNNLayer, mvector/models/campplus.py:114-181), in place on a channel-last fp16 concat buffer
 * x [B, T2, ldx]: layer l = 0 .. nlayers - 1 reads channels [0, c_in + 32 l) and writes channels [c_in + 32 l, c_in + 32 (l + 1)); growth 32,
 * bottleneck 128.  Per layer
 *   h = ReLU(BN2(W1 . ReLU(BN1(x)))),  ctx = mean_T(h) + mean over the frame's seg_len-frame segment (the last one over its true length),
 *   y = conv_k3,dil(h, zero padding) * sigmoid(Wb . ReLU(Wa . ctx + ba) + bb).
 * Parameters: host arrays of nlayers device pointers -- w1 = mv_conv1d_pack_weight of linear1.weight [128, cin, 1], wl the same of
 * cam_layer.linear_local.weight [32, 128, 3]; bn1_s / bn1_t fp32 [cin], bn2_s / bn2_t fp32 [128] (eval BatchNorm folded to scale / shift);
 * wa fp32 [64][128], ba [64], wb [32][64], bb [32].
 * form: which of the library's launch forms runs.  MV_CAM_FORM_AUTO = the choice the CAM++ handle's forward makes (the same code): the block
 * kernel for the whole block where it takes the geometry, else per layer the one-launch kernel, else the two-launch long form.  A pinned form
 * that does not take the geometry returns MV_ERR_UNSUPPORTED with a message naming the form -- it never runs another one:
 *   MV_CAM_FORM_BLOCK  all layers in one launch: T2 <= 160, c_in >= 128, nlayers <= 24, c_in + 32 nlayers <= 1056, dil 1..2, at most 2 segments
 *   MV_CAM_FORM_LAYER  one launch per layer: T2 <= 160, cin <= 1984, dil 1..2, at most 2 segments
 *   MV_CAM_FORM_LONG   two launches per layer over chunks of up to 160 frames: T2 > 160, cin <= 1984, dil 1..2, seg_len >= 80
 * forms_used (optional, host, nlayers entries): the form each layer ran.  ldx % 8 == 0, ldx >= c_in + 32 nlayers; columns beyond that are not
 * touched.  workspace: mv_cam_dense_block_workspace_bytes(B, T2, nlayers) bytes of device memory, 16-byte aligned (the long form's bottleneck rows
 * and partial sums, the device copy of the layer table); the call allocates nothing.  The layer table is copied SYNCHRONOUSLY after a wait for
 * `stream`: a layer-level entry point of the parity tests, not a hot-path call. */
#define MV_CAM_FORM_AUTO 0
#define MV_CAM_FORM_BLOCK 1
#define MV_CAM_FORM_LAYER 2
#define MV_CAM_FORM_LONG 3
int mv_cam_dense_block_workspace_bytes(int32_t B, int32_t T2, int32_t nlayers, size_t* bytes);
int mv_cam_dense_block_f16(void* x, int64_t ldx, int32_t B, int32_t T2, int32_t c_in, int32_t nlayers, const void* const* w1,
                           const float* const* bn1_s, const float* const* bn1_t, const float* const* bn2_s, const float* const* bn2_t,
                           const void* const* wl, const float* const* wa, const float* const* ba, const float* const* wb, const float* const* bb,
                           int32_t dil, int32_t seg_len, int32_t form, int32_t* forms_used, void* workspace, size_t workspace_bytes,
                           mv_stream_t stream);

/* Energy voice activity detection (Kaldi's compute-vad restated) of B fp32 waveform rows: per row the maximal runs [a, b) of speech frames.
 *   frames    row b has n_b = num_samples[b] samples (device int64 [B], clamped to 0 .. L; NULL: every row has L).  T_b = 0 if n_b < frame_length,
 *             else 1 + (n_b - frame_length) / frame_shift; frame t = x[t * frame_shift, t * frame_shift + frame_length).  T(L) is the count for n = L.
 *   logE_t    fp64, v_i = (double)x_i * scale:  m = (sum v) / frame_length,  e = sum (v - m)^2,  logE = log(e < eps ? eps : e), eps = 2^-23 (the
 *             comparison is written with <: a NaN energy stays NaN).  Both sums in one order: 32 lanes per frame, lane j adds the elements
 *             j, j + 32, .. in ascending order (the squares by fma), the 32 lane sums fold by a butterfly over the lane offsets 16, 8, 4, 2, 1.
 *   thr_b     energy_threshold + energy_mean_scale * (S / T_b), S the sum of the row's logE: per tile of MV_VAD_TILE_FRAMES frames a halving
 *             tree over the tile's (zero-padded) entries, then thread j of 256 adds the tiles j, j + 256, .. in ascending order and a halving
 *             tree folds the 256 sums.  No atomics on floats: the same bits on every run, stream and batch.  T_b = 0 gives NaN (0 / 0).
 *   decision  over the frames lo = max(0, t - frames_context) .. hi = min(T_b - 1, t + frames_context): den = hi - lo + 1, num = how many of them
 *             have logE > thr; speech iff (double)num >= (double)den * proportion_threshold.
 *   runs      maximal stretches [a, b) of speech frames in ascending order as pairs of int32: num_runs[b] is the row's true count, the first
 *             min(num_runs[b], max_runs) pairs of runs [B, max_runs, 2] are written and nothing behind them.
 * A row with T_b = 0 has no runs; a NaN sample makes thr NaN, every logE > thr false and (proportion_threshold > 0) the row free of runs.
 * wav row b starts at wav + b * wav_stride (wav_stride >= L, any 4-byte alignment: 16-byte loads where the address allows, scalar loads
 * otherwise).  num_frames [B] int32 = T_b.  Optional device outputs (NULL: not written): log_energy [B, T(L)] fp64, threshold [B] fp64, decisions
 * [B, T(L)] uint8 -- entries at t >= T_b are written as zeros.  Five ordinary launches on `stream` (energies, thresholds, decisions + boundary
 * counts per tile, one scan of the counts, the scatter of the boundaries): no workgroup waits for another, the call does not synchronise and
 * allocates nothing.  workspace: device memory, 16-byte aligned, of the size the companion reports (0 for arguments it refuses); what it and the
 * outputs held before does not matter.  B = 0 returns MV_OK and touches nothing.  MV_ERR_INVALID_ARGUMENT: a null cfg or required pointer
 * (runs may be NULL when max_runs = 0), negative B / L / max_runs, wav_stride < L, 1 <= frame_shift <= frame_length <= 4096 violated,
 * frames_context outside 0 .. 64, a non-finite real field, B * (T(L) + 1) above 2^31 - 1.  MV_ERR_WORKSPACE: a short workspace.
 * The defaults are compute-vad's: 400 / 160 samples (25 / 10 ms at 16 kHz), context 0, 5.0, 0.5, 0.6; scale 32768 turns [-1, 1) samples into the
 * int16 range its thresholds assume. */
#define MV_VAD_TILE_FRAMES 256
typedef struct MvVadCfg {
    int32_t frame_length;          /* samples */
    int32_t frame_shift;           /* samples */
    int32_t frames_context;
    int32_t reserved;
    double energy_threshold;
    double energy_mean_scale;
    double proportion_threshold;
    double scale;
} MvVadCfg;
size_t mv_vad_energy_workspace_bytes(const MvVadCfg* cfg, int32_t B, int64_t L);
int mv_vad_energy_f32(const MvVadCfg* cfg, const float* wav, int64_t wav_stride, const int64_t* num_samples, int32_t B, int64_t L,
                      int32_t* num_frames, int32_t* num_runs, int32_t* runs, int32_t max_runs, double* log_energy, double* threshold,
                      uint8_t* decisions, void* workspace, size_t workspace_bytes, mv_stream_t stream);

/* The runs of speech frames of mv_vad_energy_f32 (its device outputs num_frames, num_runs, runs as they are) -> per row the speech regions in
 * samples, in integers throughout.  Row b has n_b = num_samples[b] samples (device int64 [B], clamped to 0 .. L; NULL: every row has L), T_b =
 * num_frames[b] frames and R_b = num_runs[b] runs; the four steps (mvector/infer_utils/vad.py, EnergyVad.smooth, is the same definition in numpy):
 *   1. run [a, b) covers the samples [a * frame_shift, b * frame_shift); a run with b >= T_b (it reaches the last frame) ends at n_b;
 *   2. neighbours whose gap (next start - end) is shorter than min_silence are joined;
 *   3. joined regions shorter than min_speech are dropped;
 *   4. every region left grows by speech_pad on both sides, stopped at 0, at n_b, and at end + gap / 2 (rounded down) of the gap to a neighbour,
 *      on either side of that gap.
 * regions [B, max_runs, 2] int32: the first num_regions[b] pairs [start, end) of a row are written and nothing behind them; kept [B] int64: the
 * sum of the row's region lengths.  A row with num_runs[b] > max_runs (a truncated run list) cannot be smoothed: num_regions[b] = -1, kept[b] =
 * -1, nothing else is written for it.  Steps 2 and 3 are flag -> exclusive scan -> compaction over tiles of MV_VAD_REGION_TILE runs, one
 * workgroup per row walking its tiles in order with the scan values carried (a row may have any number of runs); two ordinary launches on
 * `stream`: no workgroup waits for another, no atomics, the call does not synchronise and allocates nothing.  workspace: device memory, 16-byte
 * aligned, mv_vad_regions_workspace_bytes(B, max_runs) bytes (the joined regions before step 4; 0 for B <= 0 or max_runs <= 0); what it and the
 * outputs held before does not matter.  B = 0 returns MV_OK and touches nothing.  MV_ERR_INVALID_ARGUMENT: a null cfg or required pointer
 * (runs, regions and the workspace may be NULL when max_runs = 0), negative B / L / max_runs, frame_shift < 1, a negative min_silence /
 * min_speech / speech_pad, L above 2^31 - 1 (sample positions are int32), regions overlapping runs.  MV_ERR_WORKSPACE: a short workspace. */
#define MV_VAD_REGION_TILE 256
typedef struct MvVadSmoothCfg {
    int32_t frame_shift;           /* samples, as all four */
    int32_t min_silence;
    int32_t min_speech;
    int32_t speech_pad;
} MvVadSmoothCfg;
size_t mv_vad_regions_workspace_bytes(int32_t B, int32_t max_runs);
int mv_vad_regions_i32(const MvVadSmoothCfg* cfg, const int32_t* num_frames, const int32_t* num_runs, const int32_t* runs, int32_t max_runs,
                       const int64_t* num_samples, int32_t B, int64_t L, int32_t* num_regions, int32_t* regions, int64_t* kept, void* workspace,
                       size_t workspace_bytes, mv_stream_t stream);

/* Row b of out [B, L_out] = wav[b, s_j : e_j) of the row's first min(num_regions[b], max_regions) regions (regions [B, max_regions, 2] int32, as
 * mv_vad_regions_i32 writes them) one behind the other in list order, then zeros up to L_out.  Every region is clamped to [0, n_b] (n_b as above);
 * one with e <= s is empty; the regions need not be ordered or disjoint.  out_samples[b] int64 = the row's total, also where it exceeds L_out (the
 * first L_out samples are written then).  A row with num_regions[b] < 0 (skipped by mv_vad_regions_i32) is all zeros with out_samples[b] = -1.
 * Samples are copied as 32-bit words, never computed with: the bits of a NaN or a -0.0 arrive unchanged.  wav row b starts at wav + b *
 * wav_stride, out row b at out + b * out_stride (any 4-byte alignment: 16-byte loads and stores where an address allows, 4-byte ones otherwise).
 * Two ordinary launches on `stream`: one workgroup per row scans the region lengths into the workspace; then workgroups of MV_WAVE_GATHER_TILE
 * outputs each find the region of their first output by binary search and keep the next MV_VAD_REGION_TILE regions in LDS (regions behind those are
 * searched in the workspace).  No workgroup waits for another, no atomics, no synchronisation, no allocation.  out must not overlap wav.
 * workspace: device memory, 16-byte aligned, mv_wave_gather_workspace_bytes(B, max_regions) bytes (0 for B <= 0 or a negative max_regions).  B = 0
 * returns MV_OK and touches nothing.  MV_ERR_INVALID_ARGUMENT: a null required pointer (regions may be NULL when max_regions = 0, wav when L = 0,
 * out when L_out = 0), negative B / L / L_out / max_regions, wav_stride < L, out_stride < L_out, wav or out not 4-byte aligned, out overlapping
 * wav, B * ceil(L_out / MV_WAVE_GATHER_TILE) above 2^31 - 1.  MV_ERR_WORKSPACE: a short workspace. */
#define MV_WAVE_GATHER_TILE 4096
size_t mv_wave_gather_workspace_bytes(int32_t B, int32_t max_regions);
int mv_wave_gather_f32(const float* wav, int64_t wav_stride, const int64_t* num_samples, const int32_t* num_regions, const int32_t* regions,
                       int32_t max_regions, int32_t B, int64_t L, float* out, int64_t out_stride, int64_t L_out, int64_t* out_samples,
                       void* workspace, size_t workspace_bytes, mv_stream_t stream);

/* ------------------------------------------------------------------------------------------------
 * Margin-softmax classification losses (added within ABI 5): CE, AM, ARM, AAM and sub-centre AAM as one fused forward and one fused backward
 * over the logit matrix (csrc/marginloss.hip).
 *
 * logits [B, N * K]: row b starts at logits + b * stride elements (stride >= N * K), element type `dtype` (MV_DT_F32, MV_DT_F16, MV_DT_BF16;
 *   16-bit elements are converted to fp32 on load, everything after that is fp32 or fp64 whatever the dtype).  labels int64 [B] on the device.
 * Centre cosine: c_j = max_k logits[b, j * K + k], the lowest k on ties (that column receives the gradient).  K = 1 unless kind is
 *   MV_LOSS_SUBCENTER.
 * z_j, fp32, one correctly rounded operation at a time in this order, no contraction (y = labels[b], s = cfg.scale):
 *     MV_LOSS_CE        z_j = c_j
 *     MV_LOSS_AM        z_j = s * c_j (j != y),  z_y = s * (c_y - margin)
 *     MV_LOSS_ARM       the AM values, then z_j <- (z_j - z_y < 0) ? 0 : z_j  (a zeroed column stays in the softmax with value 0)
 *     MV_LOSS_AAM, MV_LOSS_SUBCENTER
 *                       z_j = s * c_j (j != y);  sine = sqrt(1 - c_y * c_y), phi = c_y * cos_m - sine * sin_m,
 *                       z_y = s * (c_y > 0 ? phi : c_y) with easy_margin, else s * (c_y > th ? phi : c_y - mmm).  No clamp: |c_y| > 1 is NaN.
 *   cos_m, sin_m, th, mmm are the caller's (cos(margin), sin(margin), cos(pi - margin), 1 + cos(pi - margin), formed in double, passed as floats).
 * Row loss, fp64: lse = M + log(sum_j exp(z_j - M)), M = max_j z_j;  loss_b = (1 - eps) (lse - z_y) + eps (lse - sum_j z_j / N)  (the second
 *   term only for eps > 0);  loss = sum_b loss_b / B.  loss and loss_rows are these rounded once to fp32.
 * Summation order (what makes a row's bits its own): the N centres are cut into segments of MV_MARGIN_SEG; inside a segment thread t of the 256
 *   owns the chunks t, t + 256, ... of MV_MARGIN_CHUNK consecutive centres and adds exp(z_j - M) and z_j in ascending j, in fp64; the 256
 *   partial sums are folded by a halving tree (red[t] += red[t + h], h = 128 .. 1); the segments are added in ascending order; the rows of the batch
 *   mean in ascending b.  M is exact in any order.  None of it depends on B, on the other rows, on the dtype, on the row's alignment (16-byte
 *   loads where the row starts on a 16-byte boundary and K <= 3, element loads otherwise -- the same values to the same threads), on what the
 *   buffers held or on the stream.  No floating-point atomics, no workgroup waits for another: three ordinary launches (segment maxima; segment
 *   sums; one workgroup that finishes rows and mean), nothing allocated, no synchronisation.
 * Outputs of the forward: loss fp32 [1]; loss_rows fp32 [B]; pred int32 [B] = argmax_j c_j, the lowest j on ties, NaN cosines never chosen
 *   (0 for a row of NaNs); saved fp64 [B, MV_MARGIN_SAVED]: {M, log(sum_j exp(z_j - M)), z_y, loss_b}.
 * Backward: out[b, j * K + k] = (g / B) (p_j - q_j) dz_j [k = argmax], p_j = exp(z_j - lse) in fp64, q_j = (1 - eps) [j = y] + eps / N,
 *   dz_j = s (1 for CE; 0 on ARM's zeroed columns; s (cos_m + c_y sin_m / sqrt(1 - c_y c_y)) on the phi branch of the target), rounded once to
 *   the dtype.  g = *grad_out, an fp32 scalar on the device.  One element-wise launch; every row scalar comes from `saved`, a thread reads the
 *   K-groups it owns before it writes them, so out == logits with out_stride == stride (in place) is allowed; any other overlap is refused.
 * A label outside [0, N): no access outside the row; loss_rows[b], loss and every column of the row's gradient are NaN, pred[b] is valid,
 *   other rows are as without it.  A NaN logit: the row's loss and its gradient (at the argmax columns) are NaN.
 * workspace: device memory, 16-byte aligned, mv_margin_ce_workspace_bytes(B, N, K) bytes (0 for arguments the forward refuses); needs no
 *   initialising.  B = 0 returns MV_OK and touches nothing.
 * MV_ERR_INVALID_ARGUMENT with a message: a null pointer; negative B or N (N = 0 with B > 0 too); K outside 1 .. 8; K != 1 with a kind other than
 *   MV_LOSS_SUBCENTER; stride (out_stride) below N * K; eps outside [0, 1); an unknown kind or dtype; N * K above 2^31 - 1; B * stride
 *   beyond int64; B * segments above 2^31 - 1; out overlapping logits other than in place.  MV_ERR_WORKSPACE: a short or misaligned workspace.
 * ------------------------------------------------------------------------------------------------ */
#define MV_LOSS_CE 0
#define MV_LOSS_AM 1
#define MV_LOSS_ARM 2
#define MV_LOSS_AAM 3
#define MV_LOSS_SUBCENTER 4
#define MV_DT_BF16 2
#define MV_MARGIN_SEG 4096
#define MV_MARGIN_CHUNK 8
#define MV_MARGIN_SAVED 4
typedef struct {
    int32_t kind;        /* MV_LOSS_* */
    int32_t K;           /* sub-centres per class */
    int32_t easy_margin; /* AAM / sub-centre: the c_y > 0 rule */
    float margin;        /* AM / ARM */
    float scale;
    float cos_m, sin_m, th, mmm; /* AAM / sub-centre */
    float eps;           /* label smoothing */
} MvMarginLossCfg;
size_t mv_margin_ce_workspace_bytes(int64_t B, int64_t N, int32_t K);
int mv_margin_ce_forward(const MvMarginLossCfg* cfg, const void* logits, int32_t dtype, const int64_t* labels, int64_t B, int64_t N, int64_t stride,
                         float* loss, float* loss_rows, int32_t* pred, double* saved, void* workspace, size_t workspace_bytes, mv_stream_t stream);
int mv_margin_ce_backward(const MvMarginLossCfg* cfg, const void* logits, int32_t dtype, const int64_t* labels, int64_t B, int64_t N, int64_t stride,
                          const double* saved, const float* grad_out, void* out, int64_t out_stride, mv_stream_t stream);

/* ------------------------------------------------------------------------------------------------
 * SphereFace2 (added within ABI 5): a logistic loss over every column of the cosine matrix with a learnable bias, as one streaming forward and
 * one element-wise backward (csrc/sphereface2.hip).  There are no sub-centres (no K).
 *
 * logits [B, N]: cosines; row b starts at logits + b * stride elements (stride >= N), element type `dtype` (MV_DT_F32, MV_DT_F16, MV_DT_BF16;
 *   16-bit elements are converted to fp32 on load, everything after that is fp32 or fp64 whatever the dtype -- the torch expression evaluates
 *   half logits in half, this is more exact).  labels int64 [B] on the device.  bias: a DEVICE pointer to one fp32 (the module's parameter),
 *   read on the device; nothing synchronises.
 * The front, fp32, one correctly rounded operation at a time in this order, no contraction, a correctly rounded sqrt (s = cfg.scale,
 *   m = cfg.margin, b = *bias, c = logits[b, j], y = labels[b]):
 *     g(x) = 2 * h^t - 1 with h = (x + 1) / 2 and h^t = (..(h * h) * h..), t - 1 multiplications from the left.  That is what torch.pow does
 *       for t <= 3; for larger t torch calls powf, and THE PRODUCT IS THE DEFINITION here.  t is an integer in 1 .. MV_SF2_MAX_T.
 *     MV_SF2_TYPE_C   zp = s * (g(c) - m) + b,  zn = s * (g(c) + m) + b
 *     MV_SF2_TYPE_A   sine = sqrt(1 - c * c);  toward = c > th ? c * cos_m - sine * sin_m : c - mmm;  away = c * cos_m + sine * sin_m;
 *                     zp = s * g(toward) + b,  zn = s * g(away) + b.  No clamp: |c| > 1 is NaN.
 *   cos_m, sin_m, th, mmm are the caller's (cos(margin), sin(margin), cos(pi - margin), 1 + cos(pi - margin), formed in double, passed as floats).
 *   Only the branch a column needs is evaluated: zp at j = y, zn elsewhere.  The torch expression evaluates both for every column and multiplies
 *   one by zero, so a column whose UNUSED branch is NaN or infinite is NaN there and finite here.
 * Behind the front, fp64 (lambda = (double)cfg.lanbuda):  softplus(x) = max(x, 0) + log1p(exp(-|x|)) and sigma(x) = (x >= 0 ? 1 : e) / (1 + e),
 *   e = exp(-|x|), share the one exp.  l_j = lambda softplus(-zp) at the target, (1 - lambda) softplus(zn) elsewhere;
 *   w_j = -lambda sigma(-zp) at the target, (1 - lambda) sigma(zn) elsewhere;  loss_b = sum_j l_j;  loss = sum_b loss_b / B.  loss and loss_rows
 *   are these rounded once to fp32.
 * Summation order: that of the margin-softmax losses above -- segments of MV_MARGIN_SEG columns; inside a segment thread t of the 256 owns the
 *   chunks t, t + 256, ... of MV_MARGIN_CHUNK consecutive columns and adds l_j and w_j in ascending j; the 256 partial sums through the halving
 *   tree; segments in ascending order; rows in ascending b.  Nothing depends on B, on the other rows, on the dtype, on the row's alignment
 *   (16-byte loads where the row starts on a 16-byte boundary, element loads otherwise -- the same values to the same threads), on what the
 *   buffers held or on the stream.  No floating-point atomics, no workgroup waits for another, nothing allocated, no synchronisation.  Forward:
 *   two launches (segments; one workgroup that finishes rows and mean).  The loss needs no row maximum and no second read of the logits.
 * Outputs of the forward: loss fp32 [1]; loss_rows fp32 [B]; pred int32 [B] = argmax_j c_j by the rules of mv_margin_ce_forward (the lowest j on
 *   ties, NaN cosines never chosen, 0 for a row of NaNs); saved fp64 [B, MV_SF2_SAVED] = {loss_b, sum_j w_j}.
 * Backward: out[b, j] = (g / B) w_j dz_j, rounded once to fp32 and for 16-bit logits from there to the dtype; g = *grad_out, an fp32 scalar on
 *   the device.  dz_j = s t h^(t-1) dx_j in fp64: h the fp32 h of the front (that of the argument of g), h^(t-1) by t - 2 multiplications from
 *   the left; dx = 1 for type C; for type A, with c taken to fp64 and sine = sqrt(1 - c c) there, dx = (c > th ? cos_m + c sin_m / sine : 1)
 *   at the target and cos_m - c sin_m / sine elsewhere.  bias_grad fp32 [1] = (g / B) sum_b saved[b, 1], rows in ascending b.  One launch:
 *   element-wise, a thread reads the chunk it owns before it writes it, so out == logits with out_stride == stride (in place) is allowed and
 *   any other overlap is refused; one more workgroup of the same launch adds the bias gradient.  `saved` is needed for the bias gradient only.
 * A label outside [0, N): no access outside the row; loss_rows[b], loss, every column of the row's gradient and bias_grad are NaN, pred[b] is
 *   valid, the loss_rows and gradients of the other rows are as without it.  A NaN logit: its row's loss, its own gradient and bias_grad are NaN.
 * workspace: device memory, 16-byte aligned, mv_sphereface2_workspace_bytes(B, N) bytes (0 for arguments the forward refuses); needs no
 *   initialising.  B = 0 returns MV_OK and touches nothing.
 * MV_ERR_INVALID_ARGUMENT with a message: a null pointer (cfg, logits, labels, bias, an output, saved, grad_out, out, bias_grad, workspace);
 *   negative B or N (N = 0 with B > 0 too); an unknown margin_type or dtype; t outside 1 .. 8; lanbuda outside [0, 1]; stride (out_stride)
 *   below N; N above 2^31 - 1; B above 2^31 - 1; B * stride (B * out_stride) beyond int64; B * segments above 2^31 - 1; in the backward
 *   B * column tiles + 1 above 2^31 - 1 (a column tile is 256 chunks of MV_MARGIN_CHUNK columns; the + 1 is the bias gradient's workgroup); out
 *   overlapping logits other than in place.  MV_ERR_WORKSPACE: a short or misaligned workspace.
 * ------------------------------------------------------------------------------------------------ */
#define MV_SF2_TYPE_C 0
#define MV_SF2_TYPE_A 1
#define MV_SF2_MAX_T 8
#define MV_SF2_SAVED 2
typedef struct {
    int32_t margin_type; /* MV_SF2_TYPE_* */
    int32_t t;           /* the exponent of g, 1 .. MV_SF2_MAX_T */
    float scale;
    float margin;        /* type C */
    float lanbuda;       /* the weight of the target column; every other column weighs 1 - lanbuda */
    float cos_m, sin_m, th, mmm; /* type A */
} MvSphereFace2Cfg;
size_t mv_sphereface2_workspace_bytes(int64_t B, int64_t N);
int mv_sphereface2_forward(const MvSphereFace2Cfg* cfg, const void* logits, int32_t dtype, const int64_t* labels, const float* bias, int64_t B,
                           int64_t N, int64_t stride, float* loss, float* loss_rows, int32_t* pred, double* saved, void* workspace,
                           size_t workspace_bytes, mv_stream_t stream);
int mv_sphereface2_backward(const MvSphereFace2Cfg* cfg, const void* logits, int32_t dtype, const int64_t* labels, const float* bias, int64_t B,
                            int64_t N, int64_t stride, const double* saved, const float* grad_out, void* out, int64_t out_stride,
                            float* bias_grad, mv_stream_t stream);

/* ------------------------------------------------------------------------------------------------
 * Triplet loss on angular margin with batch-hard mining (added within ABI 5; csrc/triplet.hip).  The cross-entropy term of the reference's
 * class is NOT part of these entry points: the caller adds mv_margin_ce_forward with MV_LOSS_CE.
 *
 * features [B, D]: row i starts at features + i * stride elements (stride >= D), element type `dtype` (MV_DT_F32, MV_DT_F16, MV_DT_BF16).  The
 *   values are upcast on load and EVERYTHING AFTER THAT IS fp64.  labels int64 [B] on the device, any values, any multiset (the reference's
 *   dist[is_pos].view(bs, -1) needs classes of equal size; this does not).  B <= MV_TRIPLET_MAX_B, 1 <= D <= MV_TRIPLET_MAX_D.
 * Forward.  n_i = sqrt(sum_d f_id^2);  f^_i = f_i / n_i with cfg.normalize, f_i without;  sim_ij = sum_d f^_id f^_jd.
 *   Order of the sums, a function of D alone: for n_i thread t of 256 adds f_id^2 by fma over d = t, t + 256, ... in ascending d from 0, and the
 *   256 partial sums are folded by the halving tree (red[t] += red[t + h], h = 128 .. 1); sim_ij is acc = fma(f^_jd, f^_id, acc) over
 *   d = 0 .. D - 1 in ascending d from 0 -- the same for every pair, and a product commutes, so sim_ij and sim_ji are the same bits.
 *   Mining: ap_i = the smallest sim_ij over the rows j of i's label (i itself included), p_i its index; an_i = the largest over the rows of
 *   another label, q_i its index.  THE LOWER INDEX WINS TIES.  A NaN candidate makes the value NaN (the lowest NaN's index), as torch.min /
 *   torch.max.  A row with no other label has an = -inf and q = -1 (ranking term 0, `over` counts 1, no gradient through it).  The [B, B]
 *   matrix is never stored.
 *   Terms: rank_i = max(0, margin - (ap_i - an_i)) (NaN stays NaN);  short_i = ap_value - ap_i where that is > 0, else 0;
 *   over_i = an_i - an_value where that is > 0, ELSE 1 (the reference's rule).
 *   loss = sum_i rank_i / B + [add_absolute] absolute_loss_weight (sum_i over_i / B + sum_i short_i / B), rows added in ascending i; rounded once
 *   to fp32.
 *   Outputs: loss fp32 [1]; mined fp64 [B, 2] = {ap_i, an_i}; index int32 [B, 2] = {p_i, q_i}.  They are what the backward reads.
 * Backward.  alpha_i = d loss / d ap_i = -[margin - (ap_i - an_i) >= 0] / B - [add_absolute][ap_value - ap_i > 0] weight / B;
 *   beta_i = d loss / d an_i = [margin - (ap_i - an_i) >= 0] / B + [add_absolute][an_i - an_value > 0] weight / B  (the hinge passes its
 *   gradient where its argument is >= 0, as torch.clamp; the two where-terms where their condition holds; 1 / B is formed first).
 *   dF^_i = alpha_i f^_{p_i} + beta_i f^_{q_i} + sum_{b: p_b = i} alpha_b f^_b + sum_{b: q_b = i} beta_b f^_b: the two own terms first (the
 *   second only for q_i >= 0), then b ascending, at one b the p term before the q term, each by fma.  It is a gather: workgroup i scans the
 *   index lists; no atomics.  With normalize, df_i = (dF^_i - (dF^_i . f^_i) f^_i) / n_i, the dot product in the order of n_i's sum.
 *   out[i, d] = g df_id, g = *grad_out (an fp32 scalar on the device), ROUNDED ONCE from fp64 to the features' dtype.
 *   The coefficients are multiplied in even where they are 0, so a NaN row reaches every gradient row the torch expression's dense products
 *   carry it to; a zero-norm row with normalize is such a row (0 / 0).  An index outside what the forward writes (p outside [0, B), q outside
 *   [-1, B)) makes the row NaN and nothing is read through it.
 * No hidden state: nothing is kept between the calls (the backward forms f^ and n again from the features, bit for bit); no atomics, no
 *   workgroup waits for another, nothing allocated, no synchronisation.  Forward: three launches (rows; mining, MV_TRIPLET_ANCHORS anchors per
 *   workgroup; one workgroup for the terms).  Backward: two (rows; the gather).
 * workspace: device memory, 16-byte aligned, mv_triplet_workspace_bytes(B, D) bytes (0 for arguments the forward refuses): f^ in fp64 row-major
 *   and transposed, and n; needs no initialising.  B = 0 returns MV_OK and touches nothing.
 * MV_ERR_INVALID_ARGUMENT with a message: a null pointer; negative B or D; B above MV_TRIPLET_MAX_B; D outside 1 .. MV_TRIPLET_MAX_D; an unknown
 *   dtype; stride (out_stride) below D; B * stride (B * out_stride) beyond int64; out overlapping features.  MV_ERR_WORKSPACE: a short or
 *   misaligned workspace.
 * ------------------------------------------------------------------------------------------------ */
#define MV_TRIPLET_MAX_B 4096
#define MV_TRIPLET_MAX_D 2048
#define MV_TRIPLET_ANCHORS 4
typedef struct {
    double margin;
    double absolute_loss_weight;
    double ap_value, an_value;
    int32_t normalize;    /* divide every row by its norm first */
    int32_t add_absolute; /* the two absolute terms */
} MvTripletCfg;
size_t mv_triplet_workspace_bytes(int64_t B, int64_t D);
int mv_triplet_forward(const MvTripletCfg* cfg, const void* features, int32_t dtype, const int64_t* labels, int64_t B, int64_t D, int64_t stride,
                       float* loss, double* mined, int32_t* index, void* workspace, size_t workspace_bytes, mv_stream_t stream);
int mv_triplet_backward(const MvTripletCfg* cfg, const void* features, int32_t dtype, int64_t B, int64_t D, int64_t stride, const double* mined,
                        const int32_t* index, const float* grad_out, void* out, int64_t out_stride, void* workspace, size_t workspace_bytes,
                        mv_stream_t stream);

#if defined(__GNUC__)
#pragma GCC visibility pop
#endif
#ifdef __cplusplus
}
#endif
#endif /* MVECTOR_HIP_H */
