"""Speech-only embedding on the device: the checks of tests/vad_trim_checks.py on the product library (also a second stream), EnergyVad.regions /
.trim on CUDA tensors against their numpy path, and predict_batch(vad=True) on the GPU predictor against the use_gpu=False predictor."""
import os

import numpy as np
import pytest
import torch

import vad_trim_checks as tc

pytestmark = pytest.mark.gpu
DEV = 'cuda'


@pytest.mark.parametrize('smoothing', sorted(tc.SMOOTHINGS))
def test_gpu_regions_equal_smooth_on_synthetic_run_lists(smoothing):
    counts = tc.check_regions_equal_smooth(None, DEV, smoothing)
    print(f'{smoothing}: regions per row {counts} of runs per row {[r.shape[0] for r in tc.run_batch(smoothing)[1]]}')


def test_gpu_regions_of_the_hand_written_cases():
    tc.check_hand_written_cases(None, DEV)


def test_gpu_truncated_run_list_is_reported_and_skipped():
    tc.check_truncated_row(None, DEV)


def test_gpu_gather_copies_the_bits_of_every_region():
    tc.check_gather(None, DEV)


@pytest.mark.parametrize('setting,smoothing', [('default', 'default'), ('recipe', 'default'), ('default', 'tight'), ('recipe', 'tight')])
def test_gpu_trim_equals_the_numpy_path(setting, smoothing):
    kept = tc.check_trim_chain(None, DEV, setting, smoothing)
    print(f'{setting} / {smoothing}: kept {kept}')


def test_gpu_no_hidden_state():
    tc.check_no_hidden_state(None, DEV, second_stream=True)


def test_gpu_refusals_by_name():
    tc.check_refusals(None, DEV)


# ------------------------------------------------------------------ the predictor
def test_gpu_predictor_embeds_the_speech_only(tmp_path, monkeypatch):
    """the golden clips (1 s each) with 0.5 s of low noise on both sides, as 16 kHz files (the pcm16 path), as arrays (the host path) and one
    of them at 8 kHz (the resampled path): the kept lengths are the CPU predictor's, the embeddings within the standing 1 - cos <= 1e-4 of its"""
    import scipy.io.wavfile as wavfile
    from helpers import GOLDEN, cos_dist, load_case
    from mvector.predict import MVectorPredictor
    man, sd, _, _, _ = load_case('tdnn')
    (tmp_path / 'model').mkdir()
    torch.save({'0.' + k: v for k, v in sd.items()}, str(tmp_path / 'model' / 'model.pth'))
    cfg = dict(dataset_conf=dict(dataset=dict(min_duration=0.3, sample_rate=16000, use_dB_normalization=True, target_dB=-20), eval_conf=dict(batch_size=2)),
               preprocess_conf=dict(feature_method='Fbank', method_args=dict(sample_frequency=16000, num_mel_bins=80)),
               model_conf=dict(model='TDNN', model_args=dict(embd_dim=192)))
    rng = np.random.default_rng(17)
    clips = [c.astype(np.float64) for c in np.load(os.path.join(GOLDEN, 'real_audio.npz'))['pcm16']]
    files, arrays = [], []
    for i, c in enumerate(clips):
        padded = np.round(np.concatenate([3.0 * rng.standard_normal(8000), c, 3.0 * rng.standard_normal(8000 + 160 * i)])).clip(-32768, 32767).astype(np.int16)
        files.append(str(tmp_path / f'padded{i}.wav'))
        wavfile.write(files[-1], 16000, padded)
        arrays.append(padded.astype(np.float32) / 32768.0)
    low = str(tmp_path / 'padded_8k.wav')
    wavfile.write(low, 8000, np.round(np.concatenate([3.0 * rng.standard_normal(4000), clips[0][::2], 3.0 * rng.standard_normal(4000)])).astype(np.int16))

    kept = {}

    def spy(predictor, name):
        inner = predictor._trim_batch

        def wrapped(wav, lens, vad):
            out = inner(wav, lens, vad)
            kept.setdefault(name, []).append(out[1])
            return out
        predictor._trim_batch = wrapped
    gpu = MVectorPredictor(cfg, model_path=str(tmp_path / 'model'), use_gpu=True)
    spy(gpu, 'gpu')
    got_files = gpu.predict_batch(files, vad=True)
    assert gpu._last_batch_path == 'pcm16'
    got_arrays = gpu.predict_batch([a.copy() for a in arrays], vad=True)
    assert gpu._last_batch_path == 'host'
    got_mixed = gpu.predict_batch([low] + files[1:], vad=True)
    assert gpu._last_batch_path == 'pcm16_resampled' and got_mixed.shape == (len(files), 192)
    for audio, path in ((files, 'pcm16'), (arrays, 'host'), ([low] + files[1:], 'pcm16_resampled')):   # ... which vad= does not change
        gpu.predict_batch([a.copy() if isinstance(a, np.ndarray) else a for a in audio])
        assert gpu._last_batch_path == path
    one = gpu.predict(files[2], vad=True)
    monkeypatch.setenv('CUDA_VISIBLE_DEVICES', os.environ.get('CUDA_VISIBLE_DEVICES', ''))   # (the CPU predictor sets it: restored afterwards)
    cpu = MVectorPredictor(cfg, model_path=str(tmp_path / 'model'), use_gpu=False)
    spy(cpu, 'cpu')
    want_files = cpu.predict_batch(files, vad=True)
    want_arrays = cpu.predict_batch([a.copy() for a in arrays], vad=True)
    want_one = cpu.predict(files[2], vad=True)
    assert kept['gpu'][0] == kept['cpu'][0] and kept['gpu'][1] == kept['cpu'][1] and kept['gpu'][3] == kept['cpu'][2], kept
    lengths = [a.shape[0] for a in arrays]
    assert all(0.3 * 16000 <= k < n - 8000 for k, n in zip(kept['cpu'][0], lengths)), (kept['cpu'][0], lengths)   # at least half of the padding is gone
    worst = [float(cos_dist(a, b).max()) for a, b in ((got_files, want_files), (got_arrays, want_arrays), (one[None], want_one[None]))]
    print(f'kept {kept["cpu"][0]} of {lengths} samples; predict_batch(vad=True) against the CPU predictor: 1 - cos max {worst[0]:.2e} (pcm16 path), '
          f'{worst[1]:.2e} (host path), predict(vad=True) {worst[2]:.2e}')
    assert max(worst) <= 1e-4, worst
    assert float(cos_dist(got_files, gpu.predict_batch(files)).max()) > 1e-4      # the padding mattered
    click = np.round(rng.standard_normal(32000)).astype(np.int16)
    click[16000:16160] = 20000                                    # speech for less than min_speech: nothing is left (tests/test_vad_trim.py)
    wavfile.write(str(tmp_path / 'click.wav'), 16000, click)
    with pytest.raises(AssertionError, match=r'音频太短.*item 1'):
        gpu.predict_batch([files[0], str(tmp_path / 'click.wav')], vad=True)
