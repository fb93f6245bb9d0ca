// Internal link between melspec.hip (which owns MvMelSpec) and spectral.hip (the Spectrogram and MFCC entry points)
#pragma once
#include "common.h"

namespace mv {

// mv_melspec_create with a mode: spectrogram = true makes a handle whose features are the n_fft / 2 + 1 power bins (no mel stage);
// every mv_melspec_* call then works on it, writing [B, T, n_fft / 2 + 1]
int melspec_create_mode(const MvMelSpecCfg* cfg, bool spectrogram, MvMelSpec** out);

}  // namespace mv
