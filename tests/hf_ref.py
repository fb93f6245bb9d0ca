"""Restatement of what AudioFeaturizer(use_hf_model=True) keeps of a HuggingFace Wav2Vec2Model / WavLMModel: the processor's z-score, the
convolutional feature encoder and feature_projection.layer_norm (`extract_features`), then the wrapper's time mean and mask -- from a plain
state_dict and a config dict, without `transformers`.  ``dtype=torch.float64`` is the arbiter, ``torch.float32`` the fp32 restatement (pinned to
the HF code by the fixtures under tests/golden/hf_*.npz); ``fp16_sites=True`` is the ROUNDING MODEL of the device path: the fp32 restatement with a
round to fp16 exactly where csrc/hfencoder.hip stores or feeds fp16 --
  * layer 0 ("group"): the GELU output;  ("layer"): the conv output, then the LayerNorm + GELU output;
  * layers 1..: the conv weights; the conv (+ bias) output; the GELU / LayerNorm + GELU output computed from that stored value;
  * the final LayerNorm reads the last fp16 tensor and stays fp32."""
import torch
import torch.nn.functional as F

ENC_EPS = 1e-5   # GroupNorm / LayerNorm of the feature encoder (nn defaults)


def num_frames(cfg, n):
    for k, s in zip(cfg['conv_kernel'], cfg['conv_stride']):
        n = (n - k) // s + 1 if n >= k else 0
    return n


def receptive_field(cfg):
    n = 1
    for k, s in zip(reversed(cfg['conv_kernel']), reversed(cfg['conv_stride'])):
        n = (n - 1) * s + k
    return n


def state_dict_shapes(cfg):
    """{key: shape} of the tensors the front-end reads (for oracle.weights.make_state_dict)"""
    shapes, cin = {}, 1
    for i, (c, k) in enumerate(zip(cfg['conv_dim'], cfg['conv_kernel'])):
        p = f'feature_extractor.conv_layers.{i}'
        shapes[p + '.conv.weight'] = (c, cin, k)
        if cfg.get('conv_bias', False):
            shapes[p + '.conv.bias'] = (c,)
        if cfg.get('feat_extract_norm', 'group') == 'layer' or i == 0:
            shapes[p + '.layer_norm.weight'] = (c,)
            shapes[p + '.layer_norm.bias'] = (c,)
        cin = c
    shapes['feature_projection.layer_norm.weight'] = (cin,)
    shapes['feature_projection.layer_norm.bias'] = (cin,)
    return shapes


def _h(x, on):
    return x.half().to(x.dtype) if on else x


def _gelu(x):
    return 0.5 * x * (1.0 + torch.erf(x * 0.70710678118654752440))


def _layer_norm(x, w, b, eps):
    """over the last axis, biased variance"""
    m = x.mean(-1, keepdim=True)
    v = ((x - m) ** 2).mean(-1, keepdim=True)
    return (x - m) / torch.sqrt(v + eps) * w + b


def extract_features(sd, cfg, wav, dtype=torch.float64, fp16_sites=False, taps=None):
    """wav [B, L] -> [B, T', conv_dim[-1]] = outputs.extract_features.  ``taps``: optional list that receives every layer's output [B, T, C]"""
    assert not fp16_sites or dtype == torch.float32
    g = lambda k: sd[k].detach().to('cpu', dtype)   # noqa: E731
    x = torch.as_tensor(wav).detach().to('cpu', dtype)
    if cfg.get('do_normalize', True):   # Wav2Vec2FeatureExtractor.zero_mean_unit_var_norm on every (padded) row
        m = x.mean(1, keepdim=True)
        x = (x - m) / torch.sqrt(((x - m) ** 2).mean(1, keepdim=True) + 1e-7)
    act = cfg.get('feat_extract_activation', 'gelu')
    if act != 'gelu':
        raise NotImplementedError(act)
    layer_mode = cfg.get('feat_extract_norm', 'group') == 'layer'
    x = x.unsqueeze(1)   # [B, 1, L]
    for i, (k, s) in enumerate(zip(cfg['conv_kernel'], cfg['conv_stride'])):
        p = f'feature_extractor.conv_layers.{i}'
        w = g(p + '.conv.weight')
        bias = g(p + '.conv.bias') if cfg.get('conv_bias', False) else None
        if x.shape[-1] < k:
            raise RuntimeError('Kernel size can\'t be greater than actual input size')
        x = F.conv1d(x, _h(w, fp16_sites and i > 0), bias, stride=s)
        x = _h(x, fp16_sites and (i > 0 or layer_mode))
        if layer_mode:
            x = _layer_norm(x.transpose(1, 2), g(p + '.layer_norm.weight'), g(p + '.layer_norm.bias'), ENC_EPS).transpose(1, 2)
        elif i == 0:   # GroupNorm(C, C): per (utterance, channel) over time
            m = x.mean(2, keepdim=True)
            v = ((x - m) ** 2).mean(2, keepdim=True)
            x = (x - m) / torch.sqrt(v + ENC_EPS) * g(p + '.layer_norm.weight')[None, :, None] + g(p + '.layer_norm.bias')[None, :, None]
        x = _h(_gelu(x), fp16_sites)
        if taps is not None:
            taps.append(x.transpose(1, 2))
    return _layer_norm(x.transpose(1, 2), g('feature_projection.layer_norm.weight'), g('feature_projection.layer_norm.bias'),
                       float(cfg.get('layer_norm_eps', 1e-5)))


def wrapper(feature, lens_ratio=None):
    """AudioFeaturizer.forward behind the model (featurizer.py:79-90)"""
    feature = feature - feature.mean(1, keepdim=True)
    if lens_ratio is not None:
        T = feature.shape[1]
        mask_lens = torch.round(torch.as_tensor(lens_ratio, dtype=torch.float32) * T).long().unsqueeze(1)
        mask = (torch.arange(T).repeat(feature.shape[0], 1) < mask_lens).unsqueeze(-1)
        feature = torch.where(mask, feature, torch.zeros_like(feature))
    return feature


def featurize(sd, cfg, wav, lens_ratio=None, dtype=torch.float64, fp16_sites=False):
    return wrapper(extract_features(sd, cfg, wav, dtype, fp16_sites), lens_ratio)
