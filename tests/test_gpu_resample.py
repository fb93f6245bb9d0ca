"""The down-mix + polyphase resampler on the device: the checks of tests/resample_checks.py on the product library (also on a second stream),
and the predictor's 'pcm16_resampled' batch path against the CPU predictor."""
import os

import numpy as np
import pytest
import torch

import resample_checks as rc

pytestmark = pytest.mark.gpu
DEV = 'cuda'


@pytest.mark.parametrize('src,dst', rc.FILTER_RATES)
def test_gpu_filter_table_is_scipys(src, dst):
    rc.check_filter_table(None, src, dst)


def test_gpu_refusals_by_name():
    rc.check_refusals(None, DEV)


@pytest.mark.parametrize('channels', [2, 3, 8])
def test_gpu_downmix_is_the_host_mean_bit_for_bit(channels):
    rc.check_downmix(None, DEV, channels)


@pytest.mark.parametrize('src,dst,channels', rc.RESAMPLE_CASES)
def test_gpu_resample_within_the_rounding_bound_of_fp64(src, dst, channels):
    rc.check_resample(None, DEV, src, dst, channels, second_stream=True)


def test_gpu_normalize():
    rc.check_normalize(None, DEV)


def test_gpu_table_in_global_memory_at_an_extreme_ratio():
    rc.check_extreme_ratio(None, DEV)


# ------------------------------------------------------------------ the predictor
def cos_dist(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return 1.0 - (a * b).sum(-1) / (np.linalg.norm(a, axis=-1) * np.linalg.norm(b, axis=-1))


def _as_int16(x):
    return np.round(x).clip(-32768, 32767).astype(np.int16)


@pytest.fixture(scope='module')
def predictor_files(tmp_path_factory):
    """TDNN golden weights as in test_gpu_predictor_matches_oracle; four real clips written as 44.1 kHz stereo, 8 kHz mono, 48 kHz mono and 16 kHz
    mono files of 0.5 - 1 s (resampled on the host in fp64, the stereo channels differ), and the same four clips as 16 kHz mono files"""
    import scipy.io.wavfile as wavfile
    from scipy.signal import resample_poly
    from helpers import GOLDEN, load_case
    d = tmp_path_factory.mktemp('resample_predictor')
    man, sd, _, _, _ = load_case('tdnn')
    (d / 'model').mkdir()
    torch.save({'0.' + k: v for k, v in sd.items()}, str(d / 'model' / 'model.pth'))
    clips = [c.astype(np.float64) for c in np.load(os.path.join(GOLDEN, 'real_audio.npz'))['pcm16']]
    cuts = [clips[0][:16000], clips[1][:12000], clips[2][:8000], clips[3][:14500]]
    hi = resample_poly(cuts[0], 441, 160)
    stereo = np.stack([_as_int16(0.9 * hi), _as_int16(0.6 * hi + 200.0 * np.sin(np.arange(hi.shape[0]) * 0.01))], axis=1)
    written = [(44100, stereo), (8000, _as_int16(resample_poly(cuts[1], 1, 2))), (48000, _as_int16(resample_poly(cuts[2], 3, 1))),
               (16000, _as_int16(cuts[3]))]
    mixed, plain = [], []
    for i, (rate, data) in enumerate(written):
        assert 0.5 <= data.shape[0] / rate <= 1.0
        mixed.append(str(d / f'mixed{i}.wav'))
        wavfile.write(mixed[-1], rate, data)
        plain.append(str(d / f'plain{i}.wav'))
        wavfile.write(plain[-1], 16000, _as_int16(cuts[i]))
    cfg = dict(dataset_conf=dict(dataset=dict(min_duration=0.3, sample_rate=16000, use_dB_normalization=True, target_dB=-20),
                                 eval_conf=dict(batch_size=2)),
               preprocess_conf=dict(feature_method='Fbank', method_args=dict(sample_frequency=16000, num_mel_bins=80)),
               model_conf=dict(model='TDNN', model_args=dict(embd_dim=192)))
    return cfg, str(d / 'model'), mixed, plain, cuts, stereo, d


def test_gpu_predict_batch_resamples_on_the_device(predictor_files, monkeypatch):
    import scipy.io.wavfile as wavfile
    from mvector.predict import MVectorPredictor
    cfg, model_dir, mixed, plain, cuts, _, _ = predictor_files
    gpu = MVectorPredictor(cfg, model_path=model_dir, use_gpu=True)
    got = gpu.predict_batch(mixed)
    assert gpu._last_batch_path == 'pcm16_resampled' and got.shape == (4, 192)
    monkeypatch.setenv('CUDA_VISIBLE_DEVICES', os.environ.get('CUDA_VISIBLE_DEVICES', ''))   # (the CPU predictor sets it: restored afterwards)
    cpu = MVectorPredictor(cfg, model_path=model_dir, use_gpu=False)
    want = cpu.predict_batch(mixed)
    worst = cos_dist(got, want).max()
    print(f'pcm16_resampled against the CPU predictor: 1 - cos max {worst:.2e}')
    assert worst <= 1e-4, worst
    with open(mixed[0], 'rb') as f:
        as_bytes = [f.read()] + mixed[1:]
    assert np.array_equal(gpu.predict_batch(as_bytes), got) and gpu._last_batch_path == 'pcm16_resampled'   # bytes and paths: the same bits
    silent = str(os.path.join(os.path.dirname(mixed[0]), 'silent.wav'))
    wavfile.write(silent, 44100, np.zeros((30000, 2), dtype=np.int16))
    with pytest.raises(ValueError, match='无法将段规范化'):        # digital silence: the ValueError of the pcm16 path
        gpu.predict_batch(mixed[:2] + [silent])
    assert gpu._last_batch_path == 'pcm16_resampled'
    gpu.predict_batch(plain)
    assert gpu._last_batch_path == 'pcm16'                       # all at 16 kHz mono: the path it was
    gpu.predict_batch([c.astype(np.float32) / 32768.0 for c in cuts])
    assert gpu._last_batch_path == 'host'                        # ndarrays: the host path, as before


def test_gpu_gallery_of_44k_stereo_files_is_enrolled_on_the_device(predictor_files, monkeypatch):
    import scipy.io.wavfile as wavfile
    from scipy.signal import resample_poly
    from mvector.predict import MVectorPredictor
    cfg, model_dir, mixed, plain, cuts, stereo, d = predictor_files
    db = d / 'audio_db'
    for user, clip in (('alice', cuts[0]), ('bob', cuts[1])):
        (db / user).mkdir(parents=True)
        hi = _as_int16(resample_poly(clip, 441, 160))
        wavfile.write(str(db / user / '0.wav'), 44100, np.stack([hi, hi], axis=1))
    seen = []
    batch = MVectorPredictor.predict_batch

    def spy(self, audios_data, *a, **k):
        out = batch(self, audios_data, *a, **k)
        seen.append((self._last_batch_path, [type(x).__name__ for x in audios_data]))
        return out
    monkeypatch.setattr(MVectorPredictor, 'predict_batch', spy)
    p = MVectorPredictor(cfg, threshold=0.3, audio_db_path=str(db), model_path=model_dir, use_gpu=True)
    monkeypatch.undo()
    assert seen == [('pcm16_resampled', ['str', 'str'])], seen     # the chunk went down as paths
    assert sorted(p.get_users()) == ['alice', 'bob']
    assert p.recognition(plain[0])[0] == 'alice' and p.recognition(plain[1])[0] == 'bob'
