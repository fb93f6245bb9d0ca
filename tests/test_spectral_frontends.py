"""Spectrogram and MFCC front-ends (AudioFeaturizer('Spectrogram' / 'MFCC')): the CPU featurizer and the emulator build of the HIP
kernels against the restatement in tests/spectral_ref.py, which is itself checked against independent code first."""
import numpy as np
import pytest
import scipy.fft
import torch

import layer_checks as lc
import spectral_ref as sr
from emu_lib import emu_cdll
from mvector import _hip
from mvector.data_utils.featurizer import AudioFeaturizer
from oracle import frontend


def _wav(B, L, seed):
    return frontend.synth_waveforms(B, L, seed=seed)


# ---- the restatement against independent code ----

@pytest.mark.parametrize('n_mfcc,n_mels', [(13, 40), (40, 128), (80, 80)])
def test_restated_dct_is_scipy_dct2_ortho(n_mfcc, n_mels):
    ref = scipy.fft.dct(np.eye(n_mels), type=2, norm='ortho', axis=0)[:n_mfcc].T
    assert np.abs(sr.dct_matrix(n_mfcc, n_mels, 'ortho', torch.float64).numpy() - ref).max() < 1e-12
    assert np.abs(sr.dct_matrix(n_mfcc, n_mels, None, torch.float64).numpy() - 2 * scipy.fft.dct(np.eye(n_mels), type=2, axis=0)[:n_mfcc].T / 2).max() < 1e-9


def test_restated_spectrogram_is_rfft_power():
    wav = _wav(2, 4000, 1).double()
    n_fft, hop = 400, 200
    x = np.pad(wav.numpy(), ((0, 0), (n_fft // 2, n_fft // 2)), mode='reflect')
    T = 1 + 4000 // hop
    frames = np.stack([x[:, t * hop:t * hop + n_fft] for t in range(T)], axis=1)
    win = 0.5 - 0.5 * np.cos(2 * np.pi * np.arange(n_fft) / n_fft)
    ref = np.abs(np.fft.rfft(frames * win, axis=-1)) ** 2          # [B, T, 201]
    got = sr.power_spectrogram(wav, torch.float64).transpose(1, 2).numpy()
    assert np.abs(got - ref).max() < 1e-9 * np.abs(ref).max()


def test_restated_mel_stage_is_oracle_mel_spectrogram():
    wav = _wav(2, 6000, 2)
    for kw in ({}, dict(n_mels=40), dict(n_fft=512, n_mels=80)):
        a = sr.mel_spectrogram(wav, torch.float32, **kw)
        b = frontend.mel_spectrogram(wav, **kw)
        assert torch.equal(a, b), kw


def test_restated_db_floor_is_batch_wide():
    x = torch.tensor([[[1e6, 1.0]], [[1e-3, 1e-12]]])          # [B = 2, n_mels = 1, T = 2]
    db = sr.amplitude_to_db(x)
    assert db[1, 0, 0].item() == pytest.approx(60.0 - 80.0 + 0.0, abs=1e-4) or db[1, 0, 0].item() == pytest.approx(-30.0, abs=1e-4)
    assert db[1, 0, 1].item() == pytest.approx(60.0 - 80.0, abs=1e-4)   # the quiet row is floored at the loud row's max - 80


# ---- the CPU featurizer against the restatement ----

SPEC_CASES = [{}, dict(n_fft=512), dict(n_fft=600), dict(hop_length=160), dict(normalized=True), dict(normalized='frame_length'),
              dict(pad=37), dict(pad_mode='constant'), dict(n_fft=512, win_length=400, hop_length=128), dict(power=1.0), dict(center=False)]
MFCC_CASES = [{}, dict(n_mfcc=13), dict(n_mfcc=80), dict(norm=None), dict(log_mels=True), dict(melkwargs=dict(n_mels=40), n_mfcc=13),
              dict(melkwargs=dict(n_mels=80, n_fft=512, hop_length=160), n_mfcc=40), dict(melkwargs=dict(n_fft=600))]


@pytest.mark.parametrize('args', SPEC_CASES, ids=str)
def test_cpu_spectrogram_matches_restatement(args):
    wav, ratio = _wav(3, 8000, 3), torch.tensor([1.0, 0.6, 0.83])
    fz = AudioFeaturizer('Spectrogram', method_args=args)
    out = fz(wav, ratio)
    ref = sr.featurize(wav, ratio, 'Spectrogram', args)
    assert out.shape == ref.shape and out.shape[2] == fz.feature_dim
    assert (out - ref).abs().max().item() <= 1e-5 * ref.abs().max().item()


@pytest.mark.parametrize('args', MFCC_CASES, ids=str)
def test_cpu_mfcc_matches_restatement(args):
    wav, ratio = _wav(3, 8000, 4), torch.tensor([1.0, 0.6, 0.83])
    fz = AudioFeaturizer('MFCC', method_args=args)
    out = fz(wav, ratio)
    ref = sr.featurize(wav, ratio, 'MFCC', args)
    assert out.shape == ref.shape and out.shape[2] == fz.feature_dim
    assert (out - ref).abs().max().item() < 1e-3


# ---- argument errors: the exception types torchaudio raises ----

@pytest.mark.parametrize('method,args,exc', [
    ('Spectrogram', dict(n_mels=40), TypeError), ('Spectrogram', dict(power=None), NotImplementedError),
    ('Spectrogram', dict(onesided=False), NotImplementedError), ('Spectrogram', dict(normalized='x'), ValueError),
    ('MFCC', dict(dct_type=3), ValueError), ('MFCC', dict(n_mfcc=41, melkwargs=dict(n_mels=40)), ValueError),
    ('MFCC', dict(norm='backward'), AssertionError), ('MFCC', dict(n_mels=40), TypeError),
    ('MFCC', dict(melkwargs=dict(sample_rate=8000)), TypeError), ('MFCC', dict(melkwargs=dict(window='x')), TypeError),
    ('MelSpectrogram', dict(power=None), NotImplementedError), ('MelSpectrogram', dict(onesided=False), NotImplementedError),
    ('MelSpectrogram', dict(normalized='x'), ValueError), ('MelSpectrogram', dict(pad_mode='x'), NotImplementedError),
    ('MelSpectrogram', dict(n_mfcc=13), TypeError), ('MelSpectrogram', dict(norm='x'), ValueError),
    ('MelSpectrogram', dict(mel_scale='x'), ValueError)])
def test_argument_errors(method, args, exc):
    with pytest.raises(exc):
        AudioFeaturizer(method, method_args=args)
    cls = {'Spectrogram': _hip.Spectrogram, 'MFCC': _hip.Mfcc, 'MelSpectrogram': _hip.MelSpec}[method]
    with pytest.raises(exc):
        cls(args, cdll=emu_cdll())


def test_native_create_refuses_tampered_configs():
    cd = emu_cdll()
    import ctypes
    for field, value, msg in [('n_fft', 2, 'n_fft out of range'), ('win_length', 500, 'win_length'), ('hop_length', 0, 'hop_length'),
                              ('power', 0.0, 'power'), ('pad_mode', 9, 'pad_mode'), ('normalized', 7, 'normalized')]:
        cfg = _hip.MvSpectrogramCfg()
        cd.mv_spectrogram_default_cfg(ctypes.byref(cfg))
        setattr(cfg, field, value)
        h = ctypes.c_void_p()
        assert cd.mv_spectrogram_create(ctypes.byref(cfg), ctypes.byref(h)) != 0
        assert msg in cd.mv_last_error().decode()
    for field, value, msg in [('n_mfcc', 0, 'n_mfcc'), ('n_mfcc', 129, 'Cannot select more MFCC coefficients'), ('dct_norm', 2, 'norm'),
                              ('log_mels', 3, 'log_mels'), ('top_db', -1.0, 'top_db')]:
        cfg = _hip.MvMfccCfg()
        cd.mv_mfcc_default_cfg(ctypes.byref(cfg))
        setattr(cfg, field, value)
        h = ctypes.c_void_p()
        assert cd.mv_mfcc_create(ctypes.byref(cfg), ctypes.byref(h)) != 0
        assert msg in cd.mv_last_error().decode()
    cfg = _hip.MvMfccCfg()
    cd.mv_mfcc_default_cfg(ctypes.byref(cfg))
    cfg.mel.n_fft = 1
    assert cd.mv_mfcc_create(ctypes.byref(cfg), ctypes.byref(ctypes.c_void_p())) != 0
    assert 'n_fft' in cd.mv_last_error().decode()
    h = _hip.Mfcc({}, cdll=cd)
    wav = _wav(1, 4000, 5)
    assert cd.mv_mfcc_forward(h._h, wav.data_ptr(), 1, 4000, 4000, None, wav.data_ptr(), wav.data_ptr(), 16, None) != 0
    assert 'workspace' in cd.mv_last_error().decode()


# ---- batch coupling of the dB floor ----

def _loud_quiet():
    wav = _wav(2, 8000, 6)
    wav[0] *= 100.0    # loud row: its max dB is > 80 dB above much of the quiet row
    wav[1] *= 1e-3
    return wav


def test_cpu_mfcc_floor_couples_rows_of_a_call():
    wav = _loud_quiet()
    fz = AudioFeaturizer('MFCC')
    both = fz(wav)
    ref = sr.featurize(wav, None, 'MFCC', {})
    assert (both - ref).abs().max().item() < 1e-3
    db = sr.amplitude_to_db(sr.mel_spectrogram(wav))
    loud_max = db[0].max().item()
    assert db[1].min().item() == pytest.approx(loud_max - 80.0, abs=1e-3)   # the quiet row sits on the loud row's floor
    alone = fz(wav[1:])
    assert (alone[0] - both[1]).abs().max().item() > 1.0
    assert (alone - sr.featurize(wav[1:], None, 'MFCC', {})).abs().max().item() < 1e-3


# ---- emulator runs of the kernels ----

def _emu_case(method, wav, ratio, args, tol):
    cls = {'Spectrogram': _hip.Spectrogram, 'MFCC': _hip.Mfcc}[method]
    out = cls(args, cdll=emu_cdll())(wav, ratio)
    ref = sr.featurize(wav, ratio, method, args, torch.float64).float()
    assert out.shape == ref.shape
    if method == 'Spectrogram':
        bound = 1e-4 * ref.abs().amax(dim=(1, 2), keepdim=True) + 1e-6
        assert bool(((out - ref).abs() <= bound).all()), ((out - ref).abs().max().item(), args)
    else:
        assert (out - ref).abs().max().item() <= tol, ((out - ref).abs().max().item(), args)
    if ratio is not None:
        T = out.shape[1]
        for b in range(out.shape[0]):
            n = int(torch.round(ratio[b] * T))
            assert bool((out[b, n:] == 0).all())
    return out


def test_emu_spectrogram_default_geometry():
    """n_fft 400 = melspec_tile_kernel<spectrogram>: T = 241 > the 136 rows held in LDS, a masked row, edge frames"""
    assert _hip.Spectrogram({}, cdll=emu_cdll()).info()['kernel'] == 'melspec_tile_kernel (spectrogram)'
    wav = _wav(2, 48000, 7)
    _emu_case('Spectrogram', wav, torch.tensor([0.71, 1.0]), {}, None)
    _emu_case('Spectrogram', wav[:1, :5003], None, {}, None)                        # odd length, T = 26 (a ragged last quad)
    _emu_case('Spectrogram', wav[:1, :3000], None, dict(power=1.0, hop_length=160), None)
    _emu_case('Spectrogram', wav[:1, :3000], None, dict(pad=20, pad_mode='replicate', normalized=True), None)


def test_emu_spectrogram_dense_geometries():
    """power-of-two and other n_fft: stft_power_kernel + cmn_mask_kernel reading the padded bin rows"""
    wav = _wav(2, 2400, 8)
    for args in (dict(n_fft=512, hop_length=256), dict(n_fft=600), dict(n_fft=256, win_length=200, hop_length=80, center=False)):
        assert _hip.Spectrogram(args, cdll=emu_cdll()).info()['kernel'] == 'stft_power_kernel (dense DFT)'
        _emu_case('Spectrogram', wav, torch.tensor([1.0, 0.55]), args, None)


@pytest.mark.parametrize('method,args', [('MelSpectrogram', dict(n_fft=600, n_mels=80)), ('Spectrogram', dict(n_fft=600))], ids=str)
def test_emu_dense_path_time_mean_and_mask(method, args):
    """n_fft 600 = the dense DFT, whose time mean and mask are cmn_mask_kernel: in place behind the mel projection (80 columns: one block
    of 64 and a tail of 16), from stft_power_kernel's padded bin rows for the Spectrogram (301 columns in rows of 304); the second row masked"""
    wav, ratio = _wav(2, 6000, 12), torch.tensor([1.0, 0.55])
    if method == 'Spectrogram':
        _emu_case(method, wav, ratio, args, None)
        return
    h = _hip.MelSpec(args, cdll=emu_cdll())
    assert h.info()['kernel'] == 'stft_power_kernel (dense DFT)'
    lc.melspec_case(emu_cdll(), 'cpu', wav, ratio, args)
    out = h(wav, ratio)
    assert bool((out[1, int(torch.round(ratio[1] * out.shape[1])):] == 0).all()) and bool((out[0] != 0).any())


def test_emu_mfcc_default_geometry():
    """mel stage on melspec_tile_kernel, T = 241 frames (eight DCT chunks, the last one ragged), a masked row"""
    assert _hip.Mfcc({}, cdll=emu_cdll()).info() == {'mel_kernel': 'melspec_tile_kernel', 'dct_lds': True}
    wav = _wav(2, 48000, 9)
    _emu_case('MFCC', wav, torch.tensor([0.71, 1.0]), {}, 2e-3)
    _emu_case('MFCC', wav[:1, :5003], None, {}, 2e-3)


@pytest.mark.parametrize('args', [dict(log_mels=True), dict(norm=None), dict(n_mfcc=13, melkwargs=dict(n_mels=40)),
                                  dict(n_mfcc=80, melkwargs=dict(n_fft=512, n_mels=80)), dict(melkwargs=dict(n_fft=600, n_mels=64))], ids=str)
def test_emu_mfcc_options(args):
    wav = _wav(2, 3000, 10)
    _emu_case('MFCC', wav, torch.tensor([1.0, 0.5]), args, 5e-3)


def test_emu_mfcc_dct_table_in_global_memory():
    """n_mels x n_mfcc above the LDS copy of the table: mfcc_dct_kernel<false>, and more rows than the coefficient tile holds"""
    args = dict(n_mfcc=160, melkwargs=dict(n_fft=512, n_mels=256, hop_length=16))
    assert not _hip.Mfcc(args, cdll=emu_cdll()).info()['dct_lds']
    wav = _wav(1, 5000, 11)
    _emu_case('MFCC', wav, torch.tensor([0.9]), args, 5e-3)


def test_emu_mfcc_floor_couples_rows_of_a_call():
    wav = _loud_quiet()
    h = _hip.Mfcc({}, cdll=emu_cdll())
    both = h(wav)
    ref = sr.featurize(wav, None, 'MFCC', {}, torch.float64).float()
    assert (both - ref).abs().max().item() < 2e-3
    alone = h(wav[1:])
    assert (alone - sr.featurize(wav[1:], None, 'MFCC', {}, torch.float64).float()).abs().max().item() < 2e-3
    assert (alone[0] - both[1]).abs().max().item() > 1.0
