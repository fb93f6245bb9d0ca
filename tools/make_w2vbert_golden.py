"""Fixtures of the Wav2Vec2-BERT front-end (tests/golden/hf_w2vbert_*.npz): a tiny random-weights Wav2Vec2BertModel (one layer, hidden size 32)
and a default SeamlessM4TFeatureExtractor, saved to a temporary folder and loaded back through AutoModel / AutoFeatureExtractor as the reference's
AudioFeaturizer(use_hf_model=True) loads them; nothing is fetched.  Stored per fixture: the config and processor fields the front-end reads (JSON),
the two tensors of feature_projection.layer_norm, the input and the model's `extract_features` on it.  Prints the fp64 restatement's
(tests/w2vbert_ref.py) distance from `extract_features` per fixture -- HF normalises in float32 numpy --, which tests/test_w2vbert_frontend.py
records.  Run on the CPU:  python tools/make_w2vbert_golden.py"""
import json
import os
import sys
import tempfile

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))
GOLDEN = os.path.join(ROOT, 'tests', 'golden')

# name -> (B, L, first zero sample of the last row or None)
FIXTURES = {
    'hf_w2vbert_even': (3, 8000, 5000),    # 48 frames, 24 stacked; one row zero-padded: its statistics run over the padding too
    'hf_w2vbert_odd': (2, 16160, None),    # 99 frames, 50 stacked: the last one half zeros
}
CONFIG_KEYS = ('model_type', 'feature_projection_input_dim', 'layer_norm_eps')
PROCESSOR_KEYS = ('num_mel_bins', 'stride', 'sampling_rate', 'padding_value', 'padding_side')


def save_model(folder, seed=0, **processor_args):
    """a random-weights model + its processor under `folder` (what AutoModel / AutoFeatureExtractor.from_pretrained read)"""
    from transformers import SeamlessM4TFeatureExtractor, Wav2Vec2BertConfig, Wav2Vec2BertModel
    torch.manual_seed(seed)
    cfg = Wav2Vec2BertConfig(hidden_size=32, num_hidden_layers=1, num_attention_heads=2, intermediate_size=64, feature_projection_input_dim=160,
                             vocab_size=8, conv_depthwise_kernel_size=3, left_max_position_embeddings=8, right_max_position_embeddings=4)
    model = Wav2Vec2BertModel(cfg).eval()
    with torch.no_grad():   # the norm is born as (1, 0): give the affine something to do
        ln = model.feature_projection.layer_norm
        ln.weight.copy_(torch.empty_like(ln.weight).uniform_(0.5, 1.5))
        ln.bias.copy_(torch.empty_like(ln.bias).uniform_(-0.3, 0.3))
    model.save_pretrained(folder)
    SeamlessM4TFeatureExtractor(**processor_args).save_pretrained(folder)
    return folder


def front_end_fields(model, processor):
    cfg = {k: v for k, v in model.config.to_dict().items() if k in CONFIG_KEYS}
    cfg.update({k: getattr(processor, k) for k in PROCESSOR_KEYS})
    return cfg


def burst_waveforms(B, L, seed):
    import w2vbert_cases
    return w2vbert_cases.burst_waveforms(B, L, seed)


def make(name, seed):
    from transformers import AutoFeatureExtractor, AutoModel
    import w2vbert_ref
    B, L, zero_from = FIXTURES[name]
    with tempfile.TemporaryDirectory() as folder:
        save_model(folder, seed)
        processor = AutoFeatureExtractor.from_pretrained(folder)
        model = AutoModel.from_pretrained(folder).eval()
    wav = burst_waveforms(B, L, seed).numpy().astype(np.float32)
    if zero_from is not None:
        wav[B - 1, zero_from:] = 0.0
    inputs = processor(wav, sampling_rate=16000, return_tensors='pt')   # as the reference calls it (featurizer.py:69)
    with torch.no_grad():
        feats = model(**inputs).extract_features
    cfg = front_end_fields(model, processor)
    sd = model.state_dict()
    ln_w, ln_b = sd['feature_projection.layer_norm.weight'], sd['feature_projection.layer_norm.bias']
    arrays = {'config': np.frombuffer(json.dumps(cfg, sort_keys=True).encode(), dtype=np.uint8), 'wav': wav,
              'extract_features': feats.numpy().astype(np.float32),
              'sd/feature_projection.layer_norm.weight': ln_w.numpy().astype(np.float32),
              'sd/feature_projection.layer_norm.bias': ln_b.numpy().astype(np.float32)}
    path = os.path.join(GOLDEN, name + '.npz')
    np.savez(path, **arrays)
    f64 = w2vbert_ref.extract_features(ln_w, ln_b, cfg, torch.from_numpy(wav), torch.float64)
    f32 = w2vbert_ref.extract_features(ln_w, ln_b, cfg, torch.from_numpy(wav), torch.float32)
    print(f'{path}: {os.path.getsize(path) / 1024:.0f} KiB, extract_features {tuple(feats.shape)}, |features| max {feats.abs().max():.2f}; '
          f'fp64 restatement - HF {(f64 - feats.double()).abs().max():.3e} max-abs, fp32 restatement - HF {(f32 - feats).abs().max():.3e}')


if __name__ == '__main__':
    for i, n in enumerate(FIXTURES):
        make(n, 200 + i)
