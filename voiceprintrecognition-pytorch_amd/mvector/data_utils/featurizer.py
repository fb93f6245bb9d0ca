"""AudioFeaturizer with the reference's constructor / forward / feature_dim contract
(mvector/data_utils/featurizer.py:9-111), backed by the fused HIP front-end kernels.

Device rule
-----------
* ``use_hf_model=True`` with a HuggingFace Wav2Vec2-BERT model (``facebook/w2v-bert-2.0``, the reference configs' example): ``extract_features`` is
  ``feature_projection.layer_norm`` over the SeamlessM4TFeatureExtractor's ``input_features`` (waveform * 2^15, 80-bin Kaldi log-mel, per-bin
  normalisation over time, pairs of frames stacked to 160 columns).  CUDA tensors run all of it in ``mv_w2vbert_forward`` / ``_forward_varlen``,
  one native call per batch; CPU tensors run the HF processor on the numpy rows and the LayerNorm in torch, as the reference does.
* ``use_hf_model=True`` (``feature_method`` = a local folder or cached name of a HuggingFace Wav2Vec2 / WavLM model): the reference keeps
  ``outputs.extract_features`` alone -- the processor's z-score, the convolutional feature encoder and ``feature_projection.layer_norm``.  CUDA
  tensors run them in ``mv_hfenc_forward`` (``forward_varlen``: ``mv_hfenc_forward_varlen``, one call per batch) and stay on the device (the reference calls ``.numpy()`` and cannot take them at all); CPU tensors run
  the HF module's own ``feature_extractor`` + ``feature_projection.layer_norm`` in torch.  The transformer behind them, whose output the reference
  throws away, is never evaluated.
* CUDA (ROCm) tensors: ``mv_fbank_forward`` / ``mv_melspec_forward`` / ``mv_spectrogram_forward`` / ``mv_mfcc_forward`` --
  waveform batch in HBM -> STFT (+ mel + log / dB + DCT) + time-mean subtraction + length mask, output on the same device.
  MFCC with ``log_mels=False`` floors the dB at (loudest value of the whole call) - 80, as torchaudio does on a batch: a row's
  MFCC features depend on the other rows of the same call (``forward_varlen`` featurises each row alone, through
  ``mv_*_forward_varlen``: one call per batch for all four methods).
  There is no fallback on this path: a missing libmvector_hip.so raises.
* CPU tensors (``use_gpu=False`` predictors, DataLoader worker processes after fork -- they must not touch
  HIP): a batched torch implementation of the same arithmetic (``_cpu_frontend``), as the reference itself
  always runs its featurizer on the CPU.

Unlike the reference, nothing forces the features back to the CPU: the caller keeps the waveforms on the
device and the model consumes the features there.
"""
import torch
from torch import nn

from mvector.data_utils import _cpu_frontend
from mvector.utils.logger import logger


class AudioFeaturizer(nn.Module):
    """音频特征器

    :param feature_method: 所使用的预处理方法 (``Fbank`` / ``MelSpectrogram`` / ``Spectrogram`` / ``MFCC``), or with ``use_hf_model`` the
        local folder / cached name of a HuggingFace ``wav2vec2``, ``wavlm`` or ``wav2vec2-bert`` model
    :param use_hf_model: 是否使用HF上的Wav2Vec2类似模型提取音频特征
    :param method_args: 预处理方法的参数
    """

    def __init__(self, feature_method='MelSpectrogram', use_hf_model=False, method_args={}):
        super().__init__()
        self._method_args = dict(method_args or {})
        self._feature_method = feature_method
        self.use_hf_model = use_hf_model
        self._native = {}  # device index -> native handle (built lazily; never pickled)
        if use_hf_model:
            self._load_hf_model(feature_method)
            logger.info(f'使用模型【{feature_method}】提取特征')
            return
        if feature_method not in ('Fbank', 'MelSpectrogram', 'Spectrogram', 'MFCC'):
            raise Exception(f'预处理方法 {self._feature_method} 不存在!')
        _cpu_frontend.validate_args(feature_method, self._method_args)
        logger.info(f'使用【{feature_method}】提取特征')

    HF_MODEL_TYPES = ('wav2vec2', 'wavlm', 'wav2vec2-bert')

    def _load_hf_model(self, name):
        """AutoModel / AutoFeatureExtractor as the reference loads them (featurizer.py:26-32); kept are the config, the processor's
        do_normalize and the two modules behind ``extract_features`` -- the transformer is dropped"""
        from transformers import AutoFeatureExtractor, AutoModel
        processor = AutoFeatureExtractor.from_pretrained(name)
        model = AutoModel.from_pretrained(name).eval()
        cfg = model.config.to_dict()
        if cfg.get('model_type') not in self.HF_MODEL_TYPES:
            raise NotImplementedError(f"HuggingFace model_type {cfg.get('model_type')!r} is not implemented; the front-end is built for "
                                      f'{list(self.HF_MODEL_TYPES)}')
        for p in model.parameters():
            p.requires_grad_(False)
        if cfg['model_type'] == 'wav2vec2-bert':
            return self._keep_w2vbert(cfg, processor, model)
        if cfg.get('feat_extract_activation', 'gelu') != 'gelu':
            raise NotImplementedError(f"feat_extract_activation {cfg.get('feat_extract_activation')!r} is not implemented (only 'gelu')")
        keys = ('model_type', 'conv_dim', 'conv_kernel', 'conv_stride', 'feat_extract_norm', 'feat_extract_activation', 'conv_bias', 'layer_norm_eps')
        self._hf_cfg = {k: cfg[k] for k in keys if k in cfg}
        self._hf_cfg['do_normalize'] = bool(getattr(processor, 'do_normalize', True))
        # (a tuple: not registered as sub-modules -- the featurizer has no parameters of its own, and .to(device) must not move what only CPU tensors use)
        self._hf_modules = (model.feature_extractor, model.feature_projection.layer_norm)
        self._hf_sd = {k: v.detach().float().cpu() for k, v in model.state_dict().items()
                       if k.startswith('feature_extractor.') or k.startswith('feature_projection.layer_norm.')}

    def _keep_w2vbert(self, cfg, processor, model):
        """Wav2Vec2-BERT (w2v-bert-2.0): `extract_features` is feature_projection.layer_norm over the processor's input_features.  Kept are
        feature_projection_input_dim and layer_norm_eps of the config, the processor (CPU tensors run it) with its num_mel_bins, stride,
        sampling_rate, padding_value and padding_side, and the LayerNorm; the rest of the model is dropped.  Refused by name: what the
        library refuses, and a processor that would not pad with zero frames on the right."""
        keep = {'model_type': cfg['model_type'], 'feature_projection_input_dim': int(cfg['feature_projection_input_dim']),
                'layer_norm_eps': float(cfg.get('layer_norm_eps', 1e-5))}
        for k, want in (('num_mel_bins', 80), ('stride', 2), ('sampling_rate', 16000), ('padding_value', 0.0), ('padding_side', 'right')):
            keep[k] = getattr(processor, k, want)
            if keep[k] != want:
                raise NotImplementedError(f"Wav2Vec2-BERT front-end: the processor's {k} = {keep[k]!r} is not implemented (only {want!r})")
        if keep['feature_projection_input_dim'] != keep['num_mel_bins'] * keep['stride']:
            raise NotImplementedError(f"Wav2Vec2-BERT front-end: feature_projection_input_dim = {keep['feature_projection_input_dim']} is not "
                                      f"num_mel_bins * stride = {keep['num_mel_bins'] * keep['stride']}")
        if not keep['layer_norm_eps'] > 0:
            raise NotImplementedError(f"Wav2Vec2-BERT front-end: layer_norm_eps = {keep['layer_norm_eps']!r} is not positive")
        self._hf_cfg = keep
        self._hf_modules = (processor, model.feature_projection.layer_norm)
        self._hf_sd = {k: v.detach().float().cpu() for k, v in model.state_dict().items() if k.startswith('feature_projection.layer_norm.')}

    def _hf_min_samples(self):
        """the shortest waveform the front-end featurises: the encoder's receptive field (400 samples on the base geometry); two frames, 560
        samples, for Wav2Vec2-BERT (the per-bin variance over one frame has nothing to divide by)"""
        if self._hf_cfg['model_type'] == 'wav2vec2-bert':
            return 560
        n = 1
        for k, st in zip(reversed(self._hf_cfg['conv_kernel']), reversed(self._hf_cfg['conv_stride'])):
            n = (n - 1) * st + k
        return n

    def _hf_cpu(self, waveforms, input_lens_ratio):
        x = waveforms
        if self._hf_cfg['model_type'] == 'wav2vec2-bert':   # the reference's own arithmetic: the HF processor on the numpy rows, then the LayerNorm
            processor, ln = self._hf_modules
            if x.shape[1] < 560:
                raise ValueError(f'Wav2Vec2-BERT front-end: a waveform of {x.shape[1]} samples has fewer than two frames (560 samples)')
            inputs = processor(x.numpy(), sampling_rate=16000, return_tensors='pt')
            with torch.no_grad():
                feature = ln(inputs['input_features'].float())
            return self._hf_wrap(feature, input_lens_ratio)
        if self._hf_cfg['do_normalize']:   # Wav2Vec2FeatureExtractor.zero_mean_unit_var_norm over the whole (padded) row
            x = (x - x.mean(1, keepdim=True)) / torch.sqrt(x.var(1, unbiased=False, keepdim=True) + 1e-7)
        fe, ln = self._hf_modules
        with torch.no_grad():
            feature = ln(fe(x).transpose(1, 2))
        return self._hf_wrap(feature, input_lens_ratio)

    @staticmethod
    def _hf_wrap(feature, input_lens_ratio):
        feature = feature - feature.mean(1, keepdim=True)
        if input_lens_ratio is not None:
            T = feature.shape[1]
            mask_lens = torch.round(input_lens_ratio.to(torch.float32) * T).long().unsqueeze(1)
            mask = (torch.arange(T).repeat(feature.shape[0], 1) < mask_lens).unsqueeze(-1)
            feature = torch.where(mask, feature, torch.zeros_like(feature))
        return feature

    def __getstate__(self):
        state = self.__dict__.copy()
        state['_native'] = {}
        return state

    def _handle(self, device):
        key = device.index if device.index is not None else torch.cuda.current_device()
        h = self._native.get(key)
        if h is None:
            from mvector import _hip
            with torch.cuda.device(key):
                if self.use_hf_model and self._hf_cfg['model_type'] == 'wav2vec2-bert':
                    h = _hip.W2vBert(self._hf_cfg, self._hf_sd, device=torch.device('cuda', key))
                elif self.use_hf_model:
                    h = _hip.HfEncoder(self._hf_cfg, self._hf_sd, device=torch.device('cuda', key))
                elif self._feature_method == 'Fbank':
                    h = _hip.Fbank(self._method_args)
                elif self._feature_method == 'Spectrogram':
                    h = _hip.Spectrogram(self._method_args)
                elif self._feature_method == 'MFCC':
                    h = _hip.Mfcc(self._method_args)
                else:
                    h = _hip.MelSpec(self._method_args)
            self._native[key] = h
        return h

    def forward(self, waveforms, input_lens_ratio=None):
        """waveforms: [L] or [B, L] float32 -> [B, T, feature_dim] float32 on the same device."""
        if len(waveforms.shape) == 1:
            waveforms = waveforms.unsqueeze(0)
        if waveforms.dtype != torch.float32:
            waveforms = waveforms.float()
        if waveforms.is_cuda:
            with torch.cuda.device(waveforms.device):
                return self._handle(waveforms.device)(waveforms, input_lens_ratio)
        if self.use_hf_model:
            return self._hf_cpu(waveforms, input_lens_ratio)
        return _cpu_frontend.featurize(waveforms, input_lens_ratio, self._feature_method, self._method_args)

    def forward_varlen(self, waveforms, num_samples):
        """Zero-padded waveforms [B, L] + true lengths int64 [B] -> [B, T(L), feature_dim]: every row is featurised on its
        own length (own frame count, own padding, own time mean, own MFCC dB floor) and rows beyond it are zero -- what the
        reference's evaluation path gets from per-utterance featurisation + ``collate_fn`` padding.  CUDA tensors: one native
        call per batch for every method and for the HuggingFace front-end (``mv_*_forward_varlen``, ``mv_hfenc_forward_varlen``), no per-row
        loop and no host synchronisation; a row too short for the transform -- below the encoder's receptive field (400 samples; two frames, 560 samples, for Wav2Vec2-BERT) with
        ``use_hf_model`` -- is all zero.  CPU tensors: the per-row loop, with the same all-zero rows."""
        if waveforms.dtype != torch.float32:
            waveforms = waveforms.float()
        if waveforms.is_cuda:
            with torch.cuda.device(waveforms.device):
                return self._handle(waveforms.device)(waveforms, None, num_samples)
        T = self.forward(waveforms[:1]).size(1)
        out = torch.zeros((waveforms.size(0), T, self.feature_dim), dtype=torch.float32, device=waveforms.device)
        lens = [int(n) for n in torch.as_tensor(num_samples).tolist()]   # (one read-back for the whole batch)
        min_len = self._hf_min_samples() if self.use_hf_model else 0
        for i in range(waveforms.size(0)):
            n = min(max(lens[i], 0), waveforms.size(1))
            if n < min_len:
                continue   # no frame fits: an all-zero row, as the other front-ends leave it
            f = self.forward(waveforms[i, :n])
            out[i, :f.size(1)] = f[0]
        return out

    @property
    def feature_dim(self):
        if self.use_hf_model:
            # what the reference's 1 s probe returns (featurizer.py:35-39): extract_features.shape[2]
            if self._hf_cfg['model_type'] == 'wav2vec2-bert':
                return self._hf_cfg['feature_projection_input_dim']
            return self._hf_cfg['conv_dim'][-1]
        if self._feature_method == 'MelSpectrogram':
            return self._method_args.get('n_mels', 128)
        elif self._feature_method == 'Spectrogram':
            return self._method_args.get('n_fft', 400) // 2 + 1
        elif self._feature_method == 'MFCC':
            return self._method_args.get('n_mfcc', 40)
        elif self._feature_method == 'Fbank':
            return self._method_args.get('num_mel_bins', 23)
        else:
            raise Exception('没有{}预处理方法'.format(self._feature_method))


class KaldiFbank(nn.Module):
    """The reference's Fbank module (featurizer.py:114-132: ``Kaldi.fbank(waveform, **kwargs)`` per utterance, stacked):
    ``[Batch, Length]`` -> ``[Batch, Feature, Length]`` log-mel energies, no mean subtraction.  ``AudioFeaturizer`` does not go through it
    here (its Fbank, time mean and mask are one launch); the class exists for code that uses it directly.  CUDA tensors run the same HIP
    kernel with the time-mean subtraction switched off, CPU tensors the batched torch restatement -- like ``AudioFeaturizer``."""

    def __init__(self, **kwargs):
        super().__init__()
        self.kwargs = kwargs
        _cpu_frontend.validate_args('Fbank', self.kwargs)
        self._native = {}

    def __getstate__(self):
        state = self.__dict__.copy()
        state['_native'] = {}
        return state

    def forward(self, waveforms):
        if waveforms.dim() == 3 and waveforms.size(1) == 1:   # rows given as [1, Length] (the reference unsqueezes 1-D rows to that)
            waveforms = waveforms[:, 0]
        if waveforms.dim() != 2:
            raise ValueError(f'KaldiFbank expects [Batch, Length] waveforms, got {tuple(waveforms.shape)}')
        if waveforms.dtype != torch.float32:
            waveforms = waveforms.float()
        if waveforms.is_cuda:
            key = waveforms.device.index if waveforms.device.index is not None else torch.cuda.current_device()
            with torch.cuda.device(key):
                h = self._native.get(key)
                if h is None:
                    from mvector import _hip
                    h = self._native[key] = _hip.Fbank(self.kwargs, subtract_time_mean=False)
                feats = h(waveforms)
        else:
            feats = _cpu_frontend.fbank_batch(waveforms, self.kwargs)
        return feats.transpose(1, 2)
