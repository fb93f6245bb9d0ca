"""Fixtures of the HuggingFace front-end (tests/golden/hf_*.npz): tiny random-weights Wav2Vec2Model / WavLMModel, saved to a temporary folder and
loaded back through AutoModel / AutoFeatureExtractor as the reference's AudioFeaturizer(use_hf_model=True) loads them; nothing is fetched.  Stored per
fixture: the config and the processor's do_normalize (JSON), the tensors the front-end reads, a [3, 8000] input with one zero-padded row and the
model's `extract_features` on it.  Run on the CPU:  python tools/make_hf_golden.py

tests/test_hf_frontend.py pins tests/hf_ref.py (the restatement every other test compares against) to these, so that the GPU machine needs no
`transformers`."""
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

# name -> (model type, feat_extract_norm, conv_bias, do_normalize): both norm modes, conv_bias and do_normalize both ways, both model types
FIXTURES = {
    'hf_wav2vec2_group': ('wav2vec2', 'group', False, True),
    'hf_wav2vec2_layer': ('wav2vec2', 'layer', True, True),
    'hf_wavlm_group': ('wavlm', 'group', True, False),
    'hf_wavlm_layer': ('wavlm', 'layer', False, False),
}
FRONT_KEYS = ('conv_dim', 'conv_kernel', 'conv_stride', 'feat_extract_norm', 'feat_extract_activation', 'conv_bias', 'layer_norm_eps', 'model_type')


def tiny_config(model_type, norm, conv_bias):
    from transformers import Wav2Vec2Config, WavLMConfig
    cls = {'wav2vec2': Wav2Vec2Config, 'wavlm': WavLMConfig}[model_type]
    return cls(conv_dim=(64,) * 7, conv_kernel=(10, 3, 3, 3, 3, 2, 2), conv_stride=(5, 2, 2, 2, 2, 2, 2), feat_extract_norm=norm,
               conv_bias=conv_bias, hidden_size=32, num_hidden_layers=1, num_attention_heads=2, intermediate_size=64,
               num_conv_pos_embeddings=16, num_conv_pos_embedding_groups=2, vocab_size=8, layer_norm_eps=1e-5,
               do_stable_layer_norm=(norm == 'layer'))


def save_model(folder, model_type, norm, conv_bias, do_normalize, seed):
    """a random-weights model + its processor under `folder` (what AutoModel / AutoFeatureExtractor.from_pretrained read)"""
    from transformers import Wav2Vec2FeatureExtractor, Wav2Vec2Model, WavLMModel
    torch.manual_seed(seed)
    model = {'wav2vec2': Wav2Vec2Model, 'wavlm': WavLMModel}[model_type](tiny_config(model_type, norm, conv_bias)).eval()
    with torch.no_grad():   # the norms are born as (1, 0): give every affine something to do
        for name, p in model.named_parameters():
            if 'layer_norm' in name and (name.startswith('feature_extractor') or name.startswith('feature_projection')):
                p.copy_(torch.empty_like(p).uniform_(0.5, 1.5) if name.endswith('weight') else torch.empty_like(p).uniform_(-0.3, 0.3))
            elif name.endswith('conv.bias') and name.startswith('feature_extractor'):
                p.copy_(torch.empty_like(p).uniform_(-0.2, 0.2))
    model.save_pretrained(folder)
    Wav2Vec2FeatureExtractor(feature_size=1, sampling_rate=16000, padding_value=0.0, do_normalize=do_normalize,
                             return_attention_mask=(norm == 'layer')).save_pretrained(folder)
    return folder


def make(name, seed):
    from transformers import AutoFeatureExtractor, AutoModel
    from oracle import frontend
    model_type, norm, conv_bias, do_normalize = FIXTURES[name]
    with tempfile.TemporaryDirectory() as folder:
        save_model(folder, model_type, norm, conv_bias, do_normalize, seed)
        processor = AutoFeatureExtractor.from_pretrained(folder)
        model = AutoModel.from_pretrained(folder).eval()
    wav = frontend.synth_waveforms(3, 8000, seed=seed).numpy().astype(np.float32)
    wav[2, 5000:] = 0.0   # a zero-padded row: the z-score runs over the padding too
    inputs = processor(wav, sampling_rate=16000, return_tensors='pt')
    with torch.no_grad():
        feats = model(**inputs).extract_features
    cfg = {k: v for k, v in model.config.to_dict().items() if k in FRONT_KEYS}
    cfg['do_normalize'] = bool(processor.do_normalize)
    arrays = {'config': np.frombuffer(json.dumps(cfg, sort_keys=True).encode(), dtype=np.uint8), 'wav': wav,
              'extract_features': feats.numpy().astype(np.float32)}
    for k, v in model.state_dict().items():
        if k.startswith('feature_extractor.') or k.startswith('feature_projection.layer_norm.'):
            arrays['sd/' + k] = v.numpy().astype(np.float32)
    path = os.path.join(GOLDEN, name + '.npz')
    np.savez(path, **arrays)
    print(f'{path}: {os.path.getsize(path) / 1024:.0f} KiB, extract_features {tuple(feats.shape)}')


if __name__ == '__main__':
    for i, n in enumerate(FIXTURES):
        make(n, 100 + i)
