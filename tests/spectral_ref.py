"""Restatement of torchaudio 2.4.0's Spectrogram and MFCC transforms and of AudioFeaturizer's wrapper around them (time-mean
subtraction over all frames, length mask), for the Spectrogram / MFCC front-end tests.  ``dtype=torch.float32`` is the fp32
restatement, ``dtype=torch.float64`` the arbiter: the same rules evaluated in double precision."""
import math

import torch
import torch.nn.functional as F

from oracle.frontend import melscale_fbanks

SPEC_DEFAULTS = dict(n_fft=400, win_length=None, hop_length=None, pad=0, window_fn=torch.hann_window, power=2.0, normalized=False,
                     wkwargs=None, center=True, pad_mode='reflect', onesided=True, return_complex=None)
MEL_DEFAULTS = dict(sample_rate=16000, n_fft=400, win_length=None, hop_length=None, f_min=0.0, f_max=None, pad=0, n_mels=128,
                    window_fn=torch.hann_window, power=2.0, normalized=False, wkwargs=None, center=True, pad_mode='reflect',
                    onesided=True, norm=None, mel_scale='htk')
MFCC_DEFAULTS = dict(sample_rate=16000, n_mfcc=40, dct_type=2, norm='ortho', log_mels=False, melkwargs=None)
TOP_DB = 80.0   # torchaudio.transforms.MFCC.__init__: self.top_db = 80.0


def _args(defaults, kwargs, what):
    unknown = set(kwargs) - set(defaults)
    if unknown:
        raise TypeError(f'{what} got unexpected keyword arguments {sorted(unknown)}')
    a = dict(defaults)
    a.update(kwargs)
    return a


def power_spectrogram(wav, dtype=torch.float32, **kwargs):
    """torchaudio.functional.spectrogram as torchaudio.transforms.Spectrogram calls it: [B, L] -> [B, n_fft // 2 + 1, T]"""
    a = _args(SPEC_DEFAULTS, kwargs, 'Spectrogram')
    n_fft = a['n_fft']
    win = a['win_length'] if a['win_length'] is not None else n_fft        # Spectrogram.__init__: win_length or n_fft
    hop = a['hop_length'] if a['hop_length'] is not None else win // 2    # ... hop_length or win_length // 2
    # window_fn(win_length, **wkwargs), evaluated once (the arbiter asks torch's window functions for its own precision)
    window = a['window_fn'](win, **(a['wkwargs'] or {}), **({} if dtype == torch.float32 else dict(dtype=dtype))).to(dtype)
    x = torch.as_tensor(wav).to(dtype)
    if a['pad'] > 0:                                                      # spectrogram(): F.pad(waveform, (pad, pad), "constant")
        x = F.pad(x, (a['pad'], a['pad']), 'constant')
    frame_length_norm = a['normalized'] == 'frame_length'                 # spectrogram(): _get_spec_norms(normalized)
    window_norm = a['normalized'] in (True, 'window')
    spec = torch.stft(x, n_fft, hop, win, window, center=a['center'], pad_mode=a['pad_mode'], normalized=frame_length_norm,
                      onesided=True, return_complex=True)
    if window_norm:
        spec = spec / window.pow(2.0).sum().sqrt()
    return spec.abs() if a['power'] == 1.0 else spec.abs().pow(a['power'])


def mel_spectrogram(wav, dtype=torch.float32, **kwargs):
    """torchaudio.transforms.MelSpectrogram = Spectrogram(power) + MelScale(melscale_fbanks): [B, n_mels, T]"""
    a = _args(MEL_DEFAULTS, kwargs, 'MelSpectrogram')
    f_max = a['f_max'] if a['f_max'] is not None else float(a['sample_rate'] // 2)
    spec = power_spectrogram(wav, dtype, **{k: a[k] for k in SPEC_DEFAULTS if k in a})
    fb = melscale_fbanks(a['n_fft'] // 2 + 1, a['f_min'], f_max, a['n_mels'], a['sample_rate'], a['norm'], a['mel_scale']).to(dtype)
    return torch.matmul(spec.transpose(-1, -2), fb).transpose(-1, -2)


def dct_matrix(n_mfcc, n_mels, norm='ortho', dtype=torch.float32):
    """torchaudio.functional.create_dct: [n_mels, n_mfcc]"""
    n = torch.arange(float(n_mels), dtype=dtype)
    k = torch.arange(float(n_mfcc), dtype=dtype).unsqueeze(1)
    dct = torch.cos(math.pi / float(n_mels) * (n + 0.5) * k)
    if norm is None:
        dct *= 2.0
    else:
        assert norm == 'ortho'
        dct[0] *= 1.0 / math.sqrt(2.0)
        dct *= math.sqrt(2.0 / float(n_mels))
    return dct.t()


def amplitude_to_db(x, top_db=TOP_DB):
    """torchaudio.functional.amplitude_to_DB(x, multiplier=10, amin=1e-10, db_multiplier=log10(max(amin, ref=1)) = 0, top_db): a 3-D
    [B, n_mels, T] input is reshaped to (1, B, n_mels, T) -- B becomes the channels of ONE item -- and one amax is taken over it"""
    x_db = 10.0 * torch.log10(torch.clamp(x, min=1e-10))
    x_db -= 10.0 * 0.0
    shape = x_db.size()
    packed_channels = shape[-3] if x_db.dim() > 2 else 1
    x_db = x_db.reshape(-1, packed_channels, shape[-2], shape[-1])
    x_db = torch.max(x_db, (x_db.amax(dim=(-3, -2, -1)) - top_db).view(-1, 1, 1, 1))
    return x_db.reshape(shape)


def mfcc(wav, dtype=torch.float32, **kwargs):
    """torchaudio.transforms.MFCC.forward: [B, n_mfcc, T]"""
    a = _args(MFCC_DEFAULTS, kwargs, 'MFCC')
    mel = mel_spectrogram(wav, dtype, sample_rate=a['sample_rate'], **(a['melkwargs'] or {}))
    if a['log_mels']:
        mel = torch.log(mel + 1e-6)      # MFCC.forward: log_offset = 1e-6
    else:
        mel = amplitude_to_db(mel)
    dct = dct_matrix(a['n_mfcc'], mel.shape[-2], a['norm'], dtype)
    return torch.matmul(mel.transpose(-1, -2), dct).transpose(-1, -2)


def featurize(wav, lens_ratio, method, method_args=None, dtype=torch.float32):
    """AudioFeaturizer.forward of the reference (featurizer.py:53-91): transform, transpose to [B, T, D], subtract the time mean over
    ALL frames, zero the frames t >= round_half_even(ratio * T)"""
    fn = {'Spectrogram': power_spectrogram, 'MFCC': mfcc}[method]
    feats = fn(wav, dtype, **(method_args or {})).transpose(1, 2)
    feats = feats - feats.mean(1, keepdim=True)
    if lens_ratio is not None:
        T = feats.shape[1]
        keep = torch.arange(T).view(1, T, 1) < torch.round(torch.as_tensor(lens_ratio).float() * T).long().view(-1, 1, 1)
        feats = torch.where(keep, feats, torch.zeros_like(feats))
    return feats
