"""Restatement of what AudioFeaturizer(use_hf_model=True) keeps of a HuggingFace Wav2Vec2BertModel (facebook/w2v-bert-2.0):
`extract_features` = feature_projection.layer_norm(input_features), with input_features as the SeamlessM4TFeatureExtractor computes them, then
the wrapper's time mean and mask -- from the two LayerNorm tensors and a config dict, without `transformers`.

  1. waveform * 2^15;  2. Kaldi log-mel = oracle.frontend.kaldi_fbank(_f64) with FBANK_ARGS;  3. per mel bin over the row's T frames
  (x - mean) / sqrt(var(ddof = 1) + 1e-7);  4. zero frames up to a multiple of stride = 2;  5. pairs of frames stacked into 160 columns;
  6. LayerNorm over the columns (layer_norm_eps);  7. time mean over the stacked frames and the length mask (featurizer.py:79-90).

``dtype=torch.float64`` is the arbiter, ``torch.float32`` the rounding model of the device path (same rounding sites, other summation orders),
pinned to the HF code by the fixtures under tests/golden/hf_w2vbert_*.npz."""
import torch

from oracle import frontend

FBANK_ARGS = dict(sample_frequency=16000, num_mel_bins=80, low_freq=20, high_freq=0, preemphasis_coefficient=0.97, window_type='povey', dither=0)
NORM_EPS = 1e-7
MIN_SAMPLES = 560   # two frames: the fewest the per-bin variance (ddof = 1) can be taken over


def num_frames(n):
    return 0 if n < 400 else 1 + (n - 400) // 160


def num_stacked(n, stride=2):
    return -(-num_frames(n) // stride)


def log_mel(wav, dtype=torch.float64):
    """wav [B, L] fp32 -> [B, T, 80]: steps 1 and 2 (the product with 2^15 is exact in fp32)"""
    fb = frontend.kaldi_fbank_f64 if dtype == torch.float64 else frontend.kaldi_fbank
    x = torch.as_tensor(wav, dtype=torch.float32) * 32768.0
    return torch.stack([fb(row, **FBANK_ARGS) for row in x]).to(dtype)


def bin_stats(mel):
    """mel [B, T, 80] -> (mean, var(ddof = 1)) [B, 80] in mel's dtype"""
    m = mel.mean(1)
    return m, ((mel - m.unsqueeze(1)) ** 2).sum(1) / (mel.shape[1] - 1)


def layer_norm(x, w, b, eps):
    m = x.mean(-1, keepdim=True)
    v = ((x - m) ** 2).mean(-1, keepdim=True)
    return (x - m) / torch.sqrt(v + eps) * w + b


def rows(mel, mean, var, ln_w, ln_b, eps, stride=2):
    """steps 3 .. 6 on mel [B, T, 80] with given statistics -> [B, ceil(T / stride), stride * 80]"""
    dtype = mel.dtype
    z = (mel - mean.unsqueeze(1)) / torch.sqrt(var.unsqueeze(1) + torch.tensor(NORM_EPS, dtype=dtype))
    B, T, F = z.shape
    if T % stride:
        z = torch.cat([z, z.new_zeros(B, stride - T % stride, F)], 1)   # zero frames, not normalised values
    z = z.reshape(B, z.shape[1] // stride, F * stride)
    return layer_norm(z, ln_w.to(dtype), ln_b.to(dtype), eps)


def extract_features(ln_w, ln_b, cfg, wav, dtype=torch.float64):
    """wav [B, L] (L >= 560) -> [B, T2, 160] = outputs.extract_features: every row over all frames of the padded length"""
    mel = log_mel(wav, dtype)
    mean, var = bin_stats(mel)
    return rows(mel, mean, var, ln_w, ln_b, float(cfg.get('layer_norm_eps', 1e-5)), int(cfg.get('stride', 2)))


def wrapper(feature, lens_ratio=None, cmn=True):
    """AudioFeaturizer.forward behind the model (featurizer.py:79-90)"""
    if cmn:
        feature = feature - feature.mean(1, keepdim=True)
    if lens_ratio is not None:
        T = feature.shape[1]
        mask_lens = torch.round(torch.as_tensor(lens_ratio, dtype=torch.float32) * T).long().unsqueeze(1)
        mask = (torch.arange(T).repeat(feature.shape[0], 1) < mask_lens).unsqueeze(-1)
        feature = torch.where(mask, feature, torch.zeros_like(feature))
    return feature


def featurize(ln_w, ln_b, cfg, wav, lens_ratio=None, dtype=torch.float64, cmn=True):
    return wrapper(extract_features(ln_w, ln_b, cfg, wav, dtype), lens_ratio, cmn)


def featurize_varlen(ln_w, ln_b, cfg, wav, num_samples, dtype=torch.float64, cmn=True):
    """the per-row variant: row b featurised alone on wav[b, :n_b], zeros behind its stacked frames; a row below 560 samples is all zero"""
    wav = torch.as_tensor(wav, dtype=torch.float32)
    B, L = wav.shape
    out = torch.zeros(B, num_stacked(L), 160, dtype=dtype)
    for b, n in enumerate(int(v) for v in num_samples):
        n = min(max(n, 0), L)
        if n < MIN_SAMPLES:
            continue
        f = featurize(ln_w, ln_b, cfg, wav[b:b + 1, :n], None, dtype, cmn)
        out[b, :f.shape[1]] = f[0]
    return out
