"""Variable-length batches of the MelSpectrogram / Spectrogram / MFCC front-ends on the MI355X (mv_*_forward_varlen): the checks of
tests/varlen_checks.py on the device, and the paths the native calls open -- AudioFeaturizer.forward_varlen as one call,
MVectorTrainer.evaluate on waveform batches and MVectorPredictor.predict_batch's int16 upload for every feature method."""
import numpy as np
import pytest
import torch

import varlen_checks as vc
from helpers import cos_dist, load_case
from oracle import frontend

pytestmark = pytest.mark.gpu
DEV = torch.device('cuda:0')


def _lib():
    from mvector import _hip
    return _hip.lib()


@pytest.mark.parametrize('idx', range(len(vc.CASES)), ids=vc.CASE_IDS)
def test_gpu_rows_match_the_second_implementation(idx):
    vc.oracle_rows_case(_lib(), DEV, idx)


@pytest.mark.parametrize('idx', range(len(vc.CASES)), ids=vc.CASE_IDS)
def test_gpu_rows_the_reference_cannot_featurise_are_zero(idx):
    vc.oracle_rows_case(_lib(), DEV, idx, vc.LENS_SHORT)


@pytest.mark.parametrize('idx', range(len(vc.CASES)), ids=vc.CASE_IDS)
def test_gpu_row_bits_are_those_of_the_row_alone(idx):
    vc.bit_identity_case(_lib(), DEV, idx)


def test_gpu_mfcc_floor_is_the_rows_own():
    vc.mfcc_floor_case(_lib(), DEV)


def test_gpu_handles_refuse_both_lengths():
    padded, _, n = vc.batch()
    for method in vc.HANDLES:
        h = vc.make_handle(_lib(), method, {})
        with pytest.raises(ValueError):
            h(padded.to(DEV), torch.ones(len(vc.LENS), device=DEV), n.to(DEV))


class _Counting:
    """stands in for a native handle: counts the forwards that go through it"""

    def __init__(self, handle):
        self.handle, self.calls = handle, 0

    def __call__(self, *args, **kwargs):
        self.calls += 1
        return self.handle(*args, **kwargs)

    def __getattr__(self, name):
        return getattr(self.handle, name)


@pytest.mark.parametrize('method', ['MelSpectrogram', 'Spectrogram', 'MFCC'])
def test_gpu_featurizer_forward_varlen_is_one_native_call(method):
    from mvector.data_utils.featurizer import AudioFeaturizer
    fz = AudioFeaturizer(method)
    padded, _, n = vc.batch()
    padded, n = padded.to(DEV), n.to(DEV)
    h = fz._handle(DEV)
    key = next(iter(fz._native))
    fz._native[key] = counter = _Counting(h)
    out = fz.forward_varlen(padded, n)
    assert counter.calls == 1
    assert torch.equal(out, h(padded, None, n))
    for b, nb in enumerate(vc.LENS):     # what the per-row loop gave: every row featurised alone
        alone = h(padded[b:b + 1, :nb])[0]
        assert torch.equal(out[b, :alone.shape[0]], alone) and bool((out[b, alone.shape[0]:] == 0).all())


# ---- evaluate / predict_batch with the STFT front-ends ----

MEL80 = dict(n_mels=80)   # the TDNN golden checkpoint takes 80 features


def _make_eval_set(tmp_path, method, method_args, n_spk=4, per_spk=4, seed=9, num_workers=2):
    """the small TDNN eval set of tests/test_eval_path.py (wav files of different lengths + enrol / trial lists + checkpoint), rebuilt here
    with another feature method"""
    import scipy.io.wavfile as wavfile
    man, sd, _, _, _ = load_case('tdnn')
    model_dir = tmp_path / 'model'
    model_dir.mkdir()
    torch.save({'0.' + k: v for k, v in sd.items()}, str(model_dir / 'model.pth'))
    rng = np.random.default_rng(seed)
    lines = {'enroll': [], 'trials': []}
    paths = []
    for spk in range(n_spk):
        base = frontend.synth_waveforms(1, 16000, seed=100 + spk)[0].numpy()
        for u in range(per_spk):
            n = int(rng.integers(9000, 16000))
            x = base[:n] + 0.02 * rng.standard_normal(n).astype(np.float32)
            pcm = np.clip(x * 20000, -32768, 32767).astype(np.int16)
            path = str(tmp_path / f's{spk}_u{u}.wav')
            wavfile.write(path, 16000, pcm)
            paths.append(path)
            lines['enroll' if u == 0 else 'trials'].append(f'{path}\t{spk}\n')
    for k, v in lines.items():
        with open(str(tmp_path / f'{k}.txt'), 'w') as f:
            f.writelines(v)
    cfg = dict(dataset_conf=dict(dataset=dict(min_duration=0.3, sample_rate=16000, use_dB_normalization=True, target_dB=-20),
                                 eval_conf=dict(batch_size=4, max_duration=20), dataLoader=dict(num_workers=num_workers),
                                 enroll_list=str(tmp_path / 'enroll.txt'), trials_list=str(tmp_path / 'trials.txt')),
               preprocess_conf=dict(feature_method=method, method_args=method_args),
               model_conf=dict(model='TDNN', model_args=dict(embd_dim=192)))
    return cfg, str(model_dir), paths


def test_gpu_trainer_evaluates_melspectrogram_on_waveform_batches(tmp_path):
    from mvector.trainer import MVectorTrainer
    cfg, model_dir, _ = _make_eval_set(tmp_path, 'MelSpectrogram', MEL80)
    gpu = MVectorTrainer(cfg, use_gpu=True)
    assert gpu._waveform_batches
    eer, dcf, thr = gpu.evaluate(resume_model=model_dir)
    assert gpu._loaders() is True      # waveform items: the dataset featurises nothing on the host
    cpu = MVectorTrainer(cfg, use_gpu=False)
    assert not cpu._waveform_batches
    c_eer, c_dcf, c_thr = cpu.evaluate(resume_model=model_dir)
    print(f'MelSpectrogram evaluate: GPU EER {eer:.4f} minDCF {dcf:.4f} thr {thr:.4f}; CPU {c_eer:.4f} {c_dcf:.4f} {c_thr:.4f}')
    # the tolerances tests/test_eval_path.py uses for Fbank: fp16 activations move individual scores by ~1e-4; the rank-based metrics move
    # only if two trials swap order
    assert abs(eer - c_eer) < 2e-2 and abs(dcf - c_dcf) < 5e-2 and abs(thr - c_thr) < 5e-3, (eer, c_eer, dcf, c_dcf, thr, c_thr)


@pytest.mark.parametrize('method,args', [('MFCC', dict(n_mfcc=80)), ('MelSpectrogram', MEL80)], ids=['mfcc', 'melspectrogram'])
def test_gpu_predictor_uploads_int16_for_every_feature_method(tmp_path, method, args):
    import scipy.io.wavfile as wavfile
    from mvector.predict import MVectorPredictor
    cfg, model_dir, _ = _make_eval_set(tmp_path, method, args, n_spk=1, per_spk=1)
    rng = np.random.default_rng(3)
    pcms = [(rng.standard_normal(n) * 3000 * (1 + i)).astype(np.int16) for i, n in enumerate((16000, 12000, 9000, 14500))]
    paths = []
    for i, p in enumerate(pcms):
        paths.append(str(tmp_path / f'p{i}.wav'))
        wavfile.write(paths[-1], 16000, p)
    gpu = MVectorPredictor(cfg, model_path=model_dir, use_gpu=True)
    e_pcm = gpu.predict_batch(paths)
    assert gpu._last_batch_path == 'pcm16' and e_pcm.shape == (4, 192)
    e_host = gpu.predict_batch([p.astype(np.float32) / 32768.0 for p in pcms])      # ndarray input: the general host path
    d = cos_dist(e_host, e_pcm).max()
    print(f'{method} predictor: int16 upload vs host path 1 - cos {d:.2e}')
    assert gpu._last_batch_path == 'host' and d < 1e-6
