// Internal link between melspec.hip (which owns MvMelSpec) and spectral.hip (the Spectrogram and MFCC entry points)
#pragma once
#include "frontend_common.h"

namespace mv {

// mv_melspec_create with a mode: spectrogram = true makes a handle whose features are the n_fft / 2 + 1 power bins (no mel stage);
// every mv_melspec_* call then works on it, writing [B, T, n_fft / 2 + 1].  The configuration is checked here for both callers; a refusal
// names mv_spectrogram_create in spectrogram mode, mv_melspec_create otherwise
int melspec_create_mode(const MvMelSpecCfg* cfg, bool spectrogram, MvMelSpec** out);

// mv_melspec_forward (num_samples == nullptr) and mv_melspec_forward_varlen (lens_ratio == nullptr) in one: the MFCC mel stage runs either
int melspec_forward_rows(const MvMelSpec* h, const float* wav, int32_t B, int64_t L, int64_t wav_stride, const float* lens_ratio,
                         const int64_t* num_samples, float* out, void* workspace, size_t workspace_bytes, mv_stream_t stream);
// the per-row geometry of a handle for the kernels behind the mel stage (frame counts of the rows of a variable-length call)
RowLens melspec_row_lens(const MvMelSpec* h, const int64_t* num_samples, int64_t L);

}  // namespace mv
