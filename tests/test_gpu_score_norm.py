"""Cohort score normalisation on the device: the checks of tests/score_norm_checks.py on the product library (also the largest cohort, which
the emulator is too slow for, and a second stream), ScoreNormalizer on CUDA tensors, MVectorTrainer.evaluate_normalized and
MVectorPredictor.contrast_normalized on the GPU."""
import os

import numpy as np
import pytest
import torch

import score_norm_checks as snc

pytestmark = pytest.mark.gpu
DEV = 'cuda'


@pytest.mark.parametrize('n,m,dim,top_n', snc.CASES + snc.DEVICE_CASES)
def test_gpu_statistics_against_the_fp64_oracle(n, m, dim, top_n):
    (mean, std), ref = snc.check_stats_case(None, DEV, n, m, dim, top_n)
    with np.errstate(invalid='ignore', divide='ignore'):
        print(f'({n}, {m}, {dim}, {top_n}): max |mean - ref| / |ref| {np.max(np.abs(mean - ref[0]) / np.abs(ref[0])):.3g}, '
              f'max |std - ref| / ref {np.max(np.abs(std - ref[1]) / ref[1]):.3g} (bar 2^-23 = {snc.EPS32:.3g} + b), '
              f'b_mean <= {ref[2].max():.3g}, b_std <= {ref[3].max():.3g}')


def test_gpu_ties_at_the_cut():
    snc.check_ties(None, DEV)


def test_gpu_special_values_and_no_rows():
    snc.check_special_values(None, DEV)


def test_gpu_no_hidden_state():
    snc.check_no_hidden_state(None, DEV, second_stream=True)


def test_gpu_refusals_by_name():
    snc.check_refusals(None, DEV)


def test_gpu_normalisation_equals_the_numpy_float32_expression():
    snc.check_normalisation(None, DEV)


def test_gpu_score_normalizer_on_cuda_tensors_is_the_two_native_calls():
    from mvector import _hip
    from mvector.metric.score_norm import ScoreNormalizer
    g = torch.Generator().manual_seed(12)
    cohort, trials, enrol = (torch.randn(r, 192, generator=g).to(DEV) for r in (500, 9, 4))
    raw = _hip.cosine(trials, enrol)
    for mode in ('s', 'z', 't'):
        sn = ScoreNormalizer(cohort, top_n=100, mode=mode)
        assert sn.cohort.is_cuda                               # a CUDA tensor stays on the device
        t_stats, e_stats = _hip.cohort_stats(trials, cohort, 100), _hip.cohort_stats(enrol, cohort, 100)
        want = _hip.score_norm(raw, t_stats, e_stats, mode)
        got = sn.normalize(raw, trial_embeddings=trials, enroll_embeddings=enrol)
        assert got.is_cuda and got.data_ptr() != raw.data_ptr() and torch.equal(got, want)
        assert torch.equal(sn.normalize(raw, trial_stats=t_stats, enroll_stats=e_stats), want)
        for a, b in zip(sn.stats(trials), t_stats):
            assert a.is_cuda and torch.equal(a, b)
        # against the host restatement.  Its scores come from another fp32 summation order: a cosine is a sum of 192 products with sum |x y| <= 1,
        # so either sum is within 192 * 2^-24 of the exact one (and the two within twice that); the mean of the N largest entries of a row moves
        # by no more than the largest change of an entry
        hm, _ = ScoreNormalizer(cohort.cpu(), top_n=100, mode=mode).stats(trials.cpu())
        assert np.abs(hm - t_stats[0].cpu().numpy()).max() <= 2 * 192 * 2.0 ** -24
        work = raw.clone()
        assert sn.normalize(work, trial_embeddings=trials, enroll_embeddings=enrol, out=work) is work and torch.equal(work, want)
    # a host cohort beside device scores is moved once and kept
    sn = ScoreNormalizer(cohort.cpu().numpy(), top_n=100)
    assert torch.equal(sn.normalize(raw, trial_embeddings=trials, enroll_embeddings=enrol),
                       _hip.score_norm(raw, _hip.cohort_stats(trials, cohort, 100), _hip.cohort_stats(enrol, cohort, 100), 's'))
    assert isinstance(sn.cohort, np.ndarray) and sn._other.is_cuda


def test_gpu_trainer_evaluate_normalized_is_the_device_composition(tmp_path):
    from mvector import _hip
    from mvector.metric.metrics import verification_metrics
    from mvector.metric.score_norm import ScoreNormalizer, cohort_means
    from mvector.trainer import MVectorTrainer
    cfg, model_dir, cohort_list = snc.make_eval_set(tmp_path, n_spk=4, per_spk=3, n_cohort=6, seed=9)
    t = MVectorTrainer(cfg, use_gpu=True)
    before = t.evaluate(resume_model=model_dir)
    for top_n, mode, per_speaker in ((4, 's', True), (300, 'z', False)):
        got = t.evaluate_normalized(cohort_list, top_n=top_n, mode=mode, resume_model=model_dir, per_speaker=per_speaker)
        (ef, el), (tf, tl), (cf, cl) = snc.embed_lists(t, cohort_list)
        assert ef.is_cuda and cf.is_cuda
        cohort = torch.from_numpy(cohort_means(cf, cl)).to(DEV) if per_speaker else cf
        assert cohort.shape == ((6 if per_speaker else 12), 192)
        sn = ScoreNormalizer(cohort, top_n=top_n, mode=mode)
        want = verification_metrics(sn.normalize(_hip.cosine(tf, ef), trial_embeddings=tf, enroll_embeddings=ef), tl, el)
        print(f'top_n {top_n} mode {mode} per_speaker {per_speaker}: evaluate {before} -> evaluate_normalized {got}')
        assert got == want and all(isinstance(v, float) for v in got), (got, want)
    assert t.evaluate(resume_model=model_dir) == before            # evaluate itself returns what it returned


def test_gpu_predictor_contrast_normalized_is_the_one_by_one_composition(tmp_path):
    import scipy.io.wavfile as wavfile
    from helpers import GOLDEN, load_case
    from mvector import _hip
    from mvector.metric.score_norm import ScoreNormalizer
    from mvector.predict import MVectorPredictor
    man, sd, _, _, _ = load_case('tdnn')
    (tmp_path / 'model').mkdir()
    torch.save({'0.' + k: v for k, v in sd.items()}, str(tmp_path / 'model' / 'model.pth'))
    paths = []
    for j, pcm in enumerate(np.load(os.path.join(GOLDEN, 'real_audio.npz'))['pcm16'][:2]):
        paths.append(str(tmp_path / f'u{j}.wav'))
        wavfile.write(paths[-1], 16000, pcm[:16000])
    cfg = dict(dataset_conf=dict(dataset=dict(min_duration=0.3, sample_rate=16000, use_dB_normalization=True, target_dB=-20),
                                 eval_conf=dict(batch_size=2)),
               preprocess_conf=dict(feature_method='Fbank', method_args=dict(sample_frequency=16000, num_mel_bins=80)),
               model_conf=dict(model='TDNN', model_args=dict(embd_dim=192)))
    p = MVectorPredictor(cfg, threshold=0.3, audio_db_path=str(tmp_path / 'audio_db'), model_path=str(tmp_path / 'model'), use_gpu=True)
    g = torch.Generator().manual_seed(4)
    cohort = torch.randn(400, 192, generator=g).to(DEV)
    sn = ScoreNormalizer(cohort, top_n=50)
    e1, e2 = p._embed(paths[0]), p._embed(paths[1])
    want = _hip.score_norm(_hip.cosine(e1, e2), _hip.cohort_stats(e1, cohort, 50), _hip.cohort_stats(e2, cohort, 50), 's')
    got = p.contrast_normalized(paths[0], paths[1], sn)
    print('contrast', p.contrast(paths[0], paths[1]), '-> contrast_normalized', got)
    assert isinstance(got, float) and want.shape == (1, 1) and got == float(want[0, 0])
