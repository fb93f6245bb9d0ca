"""Cases and bars shared by tests/test_hf_frontend.py (CPU / emulator) and tests/test_gpu_hf_frontend.py (device).

Tolerance on the feature tensor -- not invented: tests/hf_ref.py carries the rounding model of the device path (the fp32 evaluation with a round to
fp16 exactly where csrc/hfencoder.hip stores or feeds fp16).  Its distance from the fp64 arbiter was measured on every case's own input on the CPU
(`python tests/hf_cases.py` prints the table); the bar of a case is TWICE that, max-abs and mean-abs: summation order inside the MFMA and `erff`
differ from torch's, and a factor of 2 over a model of the same rounding sites is the headroom the pooling and spectral tests of this suite use.
MODEL_DISTANCE holds the measured (max-abs, mean-abs); bars() doubles it.  The features are O(1) (LayerNorm output, gains about 1)."""
import json
import os

import numpy as np
import torch

import hf_ref
from oracle import frontend, weights

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden')
FIXTURES = ('hf_wav2vec2_group', 'hf_wav2vec2_layer', 'hf_wavlm_group', 'hf_wavlm_layer')
BASE = dict(conv_kernel=[10, 3, 3, 3, 3, 2, 2], conv_stride=[5, 2, 2, 2, 2, 2, 2], feat_extract_activation='gelu', layer_norm_eps=1e-5)


def load_fixture(name):
    """(cfg dict, state_dict, wav [3, 8000], the HF model's extract_features)"""
    z = np.load(os.path.join(GOLDEN, name + '.npz'))
    cfg = json.loads(bytes(z['config']).decode())
    sd = {k[3:]: torch.from_numpy(z[k]) for k in z.files if k.startswith('sd/')}
    return cfg, sd, torch.from_numpy(z['wav']), torch.from_numpy(z['extract_features'])


def seeded_model(norm, width=512, conv_bias=None, do_normalize=True, seed=5):
    """a wav2vec2-base-geometry front-end of `width` channels with weights drawn at test time (never committed)"""
    cfg = dict(BASE, conv_dim=[width] * 7, feat_extract_norm=norm, conv_bias=(norm == 'layer') if conv_bias is None else conv_bias,
               do_normalize=do_normalize)
    sd = weights.make_state_dict(hf_ref.state_dict_shapes(cfg), seed)
    for k in sd:   # norm gains around 1 (make_state_dict draws every 1-D weight around 0)
        if k.endswith('layer_norm.weight'):
            sd[k] = sd[k] + 1.0
    return cfg, sd


RATIO3 = [1.0, 0.61, 0.35]   # ragged: round(0.61 * T), round(0.35 * T)

# name -> (model, B, L, lens_ratio); model = fixture name | ('seeded', norm)
CASES = {
    # emulator (small L: the emulator runs every lane as a fiber)
    'fix_wav2vec2_group': ('hf_wav2vec2_group', 3, 8000, RATIO3),
    'fix_wav2vec2_layer': ('hf_wav2vec2_layer', 3, 8000, RATIO3),
    'fix_wavlm_group': ('hf_wavlm_group', 3, 8000, None),
    'fix_wavlm_layer': ('hf_wavlm_layer', 3, 8000, RATIO3),
    'w512_group_L800': (('seeded', 'group'), 1, 800, [0.5]),
    'w512_layer_L800': (('seeded', 'layer'), 1, 800, [0.5]),
    # device: L = 16000 -> 3199 / 1599 / 799 / 399 / 199 / 99 / 49 frames (all odd); L = 20635 -> 4126 / 2062 / 1030 / 514 / 256 / 128 / 64 (all
    # even); L = 400: exactly one frame; B = 130 at L = 4000 (799 / 399 / 199 / 99 / 49 / 24 / 12): several 256-row tiles in every layer
    'w512_group_L16000': (('seeded', 'group'), 3, 16000, RATIO3),
    'w512_layer_L16000': (('seeded', 'layer'), 3, 16000, RATIO3),
    'w512_group_L20635': (('seeded', 'group'), 3, 20635, RATIO3),
    'w512_layer_L20635': (('seeded', 'layer'), 3, 20635, None),
    'w512_group_L400': (('seeded', 'group'), 3, 400, None),
    'w512_layer_L400': (('seeded', 'layer'), 3, 400, None),
    'w512_group_B130': (('seeded', 'group'), 130, 4000, None),
}

# cases compared WITHOUT the time mean (one frame minus its own mean is zero whatever the encoder computed)
NO_CMN = ('w512_group_L400', 'w512_layer_L400')


def reference(name, cfg, sd, wav, ratio, dtype=torch.float64, fp16_sites=False):
    if name in NO_CMN:
        return hf_ref.extract_features(sd, cfg, wav, dtype, fp16_sites)
    return hf_ref.featurize(sd, cfg, wav, ratio, dtype, fp16_sites)


# measured on the CPU: rounding model (fp32 + fp16 sites) vs the fp64 arbiter, (max-abs, mean-abs) over the featurizer output of the case
MODEL_DISTANCE = {
    'fix_wav2vec2_group': (7.679e-03, 5.286e-04),   # fp32 restatement: 2.6e-06 max-abs; |ref| max 4.76
    'fix_wav2vec2_layer': (7.173e-03, 5.120e-04),   # fp32 restatement: 5.0e-06 max-abs; |ref| max 5.12
    'fix_wavlm_group': (7.417e-03, 6.759e-04),      # fp32 restatement: 3.6e-06 max-abs; |ref| max 4.01
    'fix_wavlm_layer': (8.525e-03, 5.452e-04),      # fp32 restatement: 3.8e-06 max-abs; |ref| max 4.53
    'w512_group_L800': (3.505e-03, 2.672e-04),      # fp32 restatement: 3.4e-06 max-abs; |ref| max 2.50 (2 frames, one masked)
    'w512_layer_L800': (3.080e-03, 2.633e-04),      # fp32 restatement: 2.9e-06 max-abs; |ref| max 1.76 (2 frames, one masked)
    'w512_group_L16000': (7.887e-03, 4.811e-04),    # fp32 restatement: 3.5e-06 max-abs; |ref| max 4.92
    'w512_layer_L16000': (9.979e-03, 4.746e-04),    # fp32 restatement: 4.6e-06 max-abs; |ref| max 4.63
    'w512_group_L20635': (9.079e-03, 4.831e-04),    # fp32 restatement: 4.3e-06 max-abs; |ref| max 4.86
    'w512_layer_L20635': (8.986e-03, 6.965e-04),    # fp32 restatement: 4.4e-06 max-abs; |ref| max 5.00
    'w512_group_L400': (7.858e-03, 7.651e-04),      # fp32 restatement: 2.6e-06 max-abs; |ref| max 5.15 (no time mean)
    'w512_layer_L400': (6.144e-03, 7.450e-04),      # fp32 restatement: 2.7e-06 max-abs; |ref| max 5.13 (no time mean)
    'w512_group_B130': (9.778e-03, 7.150e-04),      # fp32 restatement: 4.5e-06 max-abs; |ref| max 5.79
}


def frames_of(L):
    out, n = [], L
    for k, s in zip(BASE['conv_kernel'], BASE['conv_stride']):
        n = (n - k) // s + 1
        out.append(n)
    return out


def build(name):
    """(cfg, sd, wav [B, L] fp32, lens_ratio tensor or None)"""
    model, B, L, ratio = CASES[name]
    if isinstance(model, str):
        cfg, sd, wav, _ = load_fixture(model)
        assert wav.shape == (B, L)
    else:
        cfg, sd = seeded_model(model[1])
        wav = frontend.synth_waveforms(B, L, seed=11)
        if B >= 3:
            wav[2, (L * 5) // 8:] = 0.0   # a zero-padded row
    return cfg, sd, wav.float().contiguous(), None if ratio is None else torch.tensor(ratio, dtype=torch.float32)


def bars(name):
    mx, mean = MODEL_DISTANCE[name]
    return 2.0 * mx, 2.0 * mean


def distances(got, ref64):
    d = (got.double().cpu() - ref64).abs()
    return d.max().item(), d.mean().item()


if __name__ == '__main__':
    for name in CASES:
        cfg, sd, wav, ratio = build(name)
        ref = reference(name, cfg, sd, wav, ratio)
        model = reference(name, cfg, sd, wav, ratio, torch.float32, True)
        f32 = reference(name, cfg, sd, wav, ratio, torch.float32)
        mx, mean = distances(model, ref)
        print(f"    '{name}': ({mx:.3e}, {mean:.3e}),   # fp32 restatement: {distances(f32, ref)[0]:.1e} max-abs; frames {frames_of(wav.shape[1])}; |ref| max {ref.abs().max():.2f}")
