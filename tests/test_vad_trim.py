"""Speech-only embedding without a GPU: the kernels behind the VAD (csrc/vad.hip: mv_vad_regions_i32, mv_wave_gather_f32) on the emulator build
against EnergyVad.smooth and the numpy concatenation (tests/vad_trim_checks.py; tests/test_gpu_vad_trim.py runs the same checks on the device),
the host layers of EnergyVad.regions / .trim, and predict / predict_batch with ``vad=`` on the CPU predictor."""
import os

import numpy as np
import pytest
import torch

import vad_checks as vc
import vad_trim_checks as tc
from helpers import load_case


@pytest.fixture(scope='module')
def emu():
    import emu_lib
    return emu_lib.emu_cdll()


@pytest.mark.parametrize('smoothing', sorted(tc.SMOOTHINGS))
def test_emu_regions_equal_smooth_on_synthetic_run_lists(emu, smoothing):
    tc.check_regions_equal_smooth(emu, 'cpu', smoothing)


def test_emu_regions_of_the_hand_written_cases(emu):
    tc.check_hand_written_cases(emu, 'cpu')


def test_emu_truncated_run_list_is_reported_and_skipped(emu):
    tc.check_truncated_row(emu, 'cpu')


def test_emu_gather_copies_the_bits_of_every_region(emu):
    tc.check_gather(emu, 'cpu')


@pytest.mark.parametrize('setting,smoothing', [('default', 'default'), ('recipe', 'default'), ('default', 'tight'), ('recipe', 'tight')])
def test_emu_trim_equals_the_numpy_path(emu, setting, smoothing):
    tc.check_trim_chain(emu, 'cpu', setting, smoothing)


def test_emu_no_hidden_state(emu):
    tc.check_no_hidden_state(emu, 'cpu')


def test_emu_refusals_by_name(emu):
    tc.check_refusals(emu, 'cpu')


def test_the_library_exports_regions_and_gather():
    import ctypes
    import __graft_entry__
    from mvector import _hip
    cdll = ctypes.CDLL(__graft_entry__.build())
    header = open(os.path.join(os.path.dirname(os.path.abspath(__graft_entry__.__file__)), 'include', 'mvector_hip.h')).read()
    for name in ('mv_vad_regions_workspace_bytes', 'mv_vad_regions_i32', 'mv_wave_gather_workspace_bytes', 'mv_wave_gather_f32'):
        assert hasattr(cdll, name) and name in _hip.EXPORTED_SYMBOLS and name + '(' in header, name
    assert f'#define MV_VAD_REGION_TILE {_hip.MV_VAD_REGION_TILE}\n' in header and f'#define MV_WAVE_GATHER_TILE {_hip.MV_WAVE_GATHER_TILE}\n' in header
    assert 'typedef struct MvVadSmoothCfg' in header
    assert [f for f, _ in _hip.MvVadSmoothCfg._fields_] == ['frame_shift', 'min_silence', 'min_speech', 'speech_pad']
    assert ctypes.sizeof(_hip.MvVadSmoothCfg) == 16 and ctypes.sizeof(_hip.MvVadCfg) == 48
    cdll.mv_abi_version.restype = ctypes.c_int
    assert cdll.mv_abi_version() == 5


# ------------------------------------------------------------------ host layers
def test_host_regions_and_trim_are_smooth_and_a_concatenation():
    x, bursts = vc.synthetic_recording()
    vad = tc.energy_vad()
    dec = vad.frames(x)[0]
    want = vad.smooth(vad.runs_of(dec), dec.shape[0], x.shape[0])
    num, reg, kept = vad.regions(x)
    assert num == len(bursts) == want.shape[0] and reg.shape == ((dec.shape[0] + 1) // 2, 2) and reg.dtype == np.int32
    assert np.array_equal(reg[:num], want) and not reg[num:].any() and kept == (want[:, 1] - want[:, 0]).sum()
    out, k = vad.trim(x)
    assert out.shape == x.shape and out.dtype == np.float32 and k == kept
    assert np.array_equal(out[:k], np.concatenate([x[s:e] for s, e in want])) and not out[k:].any()
    t_out, t_k = vad.trim(torch.from_numpy(x))                        # a CPU tensor runs the numpy path
    assert isinstance(t_out, np.ndarray) and np.array_equal(t_out, out) and t_k == k
    short = x[:7 * 16000 + 33]
    batch = np.zeros((3, x.shape[0]), dtype=np.float32)
    batch[0], batch[1, :short.shape[0]], batch[2, :399] = x, short, x[:399]
    b_out, b_k = vad.trim(batch, lengths=[x.shape[0], short.shape[0], 399])   # every row as if it were alone
    assert b_out.shape == batch.shape and b_k.tolist() == [k, vad.trim(short)[1], 0] and np.array_equal(b_out[0], out) and not b_out[2].any()
    assert np.array_equal(b_out[1, :short.shape[0]], vad.trim(short)[0])
    assert vad.trim(np.zeros(16000, dtype=np.float32))[1] == 0


# ------------------------------------------------------------------ the CPU predictor
def _noisy_clip(seconds, seed, lead=0.5, sr=16000):
    """bursts of speech-like noise with ``lead`` seconds of the noise floor in front of and behind them"""
    return vc.synthetic_recording(seconds=seconds, seed=seed, bursts=((lead, 0.45 * seconds), (0.45 * seconds + 0.6, seconds - lead)))[0]


def test_cpu_predictor_embeds_the_speech_only(tmp_path):
    import scipy.io.wavfile as wavfile
    from mvector.predict import MVectorPredictor
    man, sd, _, _, _ = load_case('tdnn')
    (tmp_path / 'model').mkdir()
    torch.save({'0.' + k: v for k, v in sd.items()}, str(tmp_path / 'model' / 'model.pth'))
    cfg = dict(dataset_conf=dict(dataset=dict(min_duration=0.3, sample_rate=16000, use_dB_normalization=True, target_dB=-20), eval_conf=dict(batch_size=2)),
               preprocess_conf=dict(feature_method='Fbank', method_args=dict(sample_frequency=16000, num_mel_bins=80)),
               model_conf=dict(model='TDNN', model_args=dict(embd_dim=192)))
    with pytest.MonkeyPatch.context() as mp:
        mp.setenv('CUDA_VISIBLE_DEVICES', os.environ.get('CUDA_VISIBLE_DEVICES', ''))   # (the CPU predictor sets it: restored afterwards)
        p = MVectorPredictor(cfg, model_path=str(tmp_path / 'model'), use_gpu=False)
    files = []
    for i, (seconds, seed) in enumerate(((3.0, 31), (4.2, 32), (3.4, 33))):
        files.append(str(tmp_path / f'clip{i}.wav'))
        wavfile.write(files[-1], 16000, np.round(32768.0 * _noisy_clip(seconds, seed)).clip(-32768, 32767).astype(np.int16))
    got = p.predict_batch(files, vad=True)
    # the definition restated: load and normalise as always, trim every waveform on the host, NO second normalisation, pad, ratios of the kept lengths
    vad = tc.energy_vad()
    loaded = [np.asarray(p._load_audio(f).samples, dtype=np.float32) for f in files]
    trimmed = []
    for x in loaded:
        dec = vad.frames(x)[0]
        regions = vad.smooth(vad.runs_of(dec), dec.shape[0], x.shape[0])
        assert regions.shape[0] == 2
        trimmed.append(np.concatenate([x[s:e] for s, e in regions]))
        speech = x.shape[0] - int(1.6 * 16000)   # the bursts; an edge costs at most its ramp and gains at most speech_pad and two frame shifts
        assert speech - 4 * int(vc.RAMP * 16000) <= trimmed[-1].shape[0] <= speech + 4 * (vad.speech_pad + 2 * 160)
    longest = max(t.shape[0] for t in trimmed)
    padded = np.zeros((len(trimmed), longest), dtype=np.float32)
    for i, t in enumerate(trimmed):
        padded[i, :t.shape[0]] = t
    with torch.no_grad():
        feats = p._audio_featurizer(torch.from_numpy(padded), torch.tensor([t.shape[0] / longest for t in trimmed], dtype=torch.float32))
        want = torch.cat([p.predictor(feats[i:i + 32]).data for i in range(0, len(files), 32)]).numpy()
    assert got.shape == want.shape == (3, 192) and np.array_equal(got, want)
    assert np.abs(got - p.predict_batch(files)).max() > 1e-3          # the silence mattered
    # vad=None is the call without the argument; an EnergyVad is used as given; predict follows predict_batch's definition
    assert np.array_equal(p.predict_batch(files, vad=None), p.predict_batch(files)) and np.array_equal(p.predict(files[0], vad=None), p.predict(files[0]))
    assert np.array_equal(p.predict_batch(files, vad=tc.energy_vad()), got)
    with torch.no_grad():
        one = p.predictor(p._audio_featurizer(torch.from_numpy(trimmed[1])[None])).data.numpy()[0]
    assert np.array_equal(p.predict(files[1], vad=True), one)
    # no speech left: the short-audio assertion, with the item's index.  The VAD's threshold is relative to the recording's mean log energy and sees the
    # dB-normalised waveform, so stationary noise of any level counts as speech once it is normalised: here a faint floor with one 10 ms click, which
    # takes the gain, is speech for less than min_speech and is dropped
    click = np.round(np.random.default_rng(3).standard_normal(32000)).astype(np.int16)
    click[16000:16160] = 20000
    files.append(str(tmp_path / 'click.wav'))
    wavfile.write(files[-1], 16000, click)
    with pytest.raises(AssertionError, match=r'音频太短.*item 3'):
        p.predict_batch(files, vad=True)
    with pytest.raises(AssertionError, match=r'音频太短.*item 0'):
        p.predict(files[3], vad=True)
    assert p.predict_batch(files).shape == (4, 192)                   # without the VAD the file is long enough
    # ... and a file of silence (a floor of three int16 steps rms) where the configuration does not normalise
    cfg['dataset_conf']['dataset']['use_dB_normalization'] = False
    with pytest.MonkeyPatch.context() as mp:
        mp.setenv('CUDA_VISIBLE_DEVICES', os.environ.get('CUDA_VISIBLE_DEVICES', ''))
        q = MVectorPredictor(cfg, model_path=str(tmp_path / 'model'), use_gpu=False)
    silence = str(tmp_path / 'silence.wav')
    wavfile.write(silence, 16000, np.round(3.0 * np.random.default_rng(4).standard_normal(32000)).astype(np.int16))
    with pytest.raises(AssertionError, match=r'音频太短.*item 1'):
        q.predict_batch([files[0], silence, files[1]], vad=True)
    assert q.predict_batch([files[0], silence, files[1]]).shape == (3, 192)
    from mvector.infer_utils.vad import EnergyVad
    with pytest.raises(AssertionError, match='8000 Hz'):
        p.predict_batch(files[:1], vad=EnergyVad(sample_rate=8000))
    from mvector.data_utils.audio import AudioSegment
    assert not hasattr(AudioSegment, 'vad')
