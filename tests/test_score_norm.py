"""Cohort score normalisation without a GPU: the kernels of csrc/scorenorm.hip on the emulator build against the fp64 oracle of
tests/score_norm_checks.py (tests/test_gpu_score_norm.py runs the same checks on the device), and the host layers: ScoreNormalizer on CPU
tensors, cohort_means, MVectorTrainer.evaluate_normalized and MVectorPredictor.contrast_normalized on the CPU."""
import os

import numpy as np
import pytest
import torch

import score_norm_checks as snc
from helpers import GOLDEN, load_case


@pytest.fixture(scope='module')
def emu():
    import emu_lib
    return emu_lib.emu_cdll()


@pytest.mark.parametrize('n,m,dim,top_n', snc.CASES)
def test_emu_statistics_against_the_fp64_oracle(emu, n, m, dim, top_n):
    snc.check_stats_case(emu, 'cpu', n, m, dim, top_n)


def test_emu_ties_at_the_cut(emu):
    snc.check_ties(emu, 'cpu')


def test_emu_special_values_and_no_rows(emu):
    snc.check_special_values(emu, 'cpu')


def test_emu_no_hidden_state(emu):
    snc.check_no_hidden_state(emu, 'cpu')


def test_emu_refusals_by_name(emu):
    snc.check_refusals(emu, 'cpu')


def test_emu_normalisation_equals_the_numpy_float32_expression(emu):
    snc.check_normalisation(emu, 'cpu')


def test_the_library_exports_the_score_normalisation():
    import ctypes
    import __graft_entry__
    from mvector import _hip
    cdll = ctypes.CDLL(__graft_entry__.build())
    for name in ('mv_cohort_stats_workspace_bytes', 'mv_cohort_stats_f32', 'mv_score_norm_f32'):
        assert hasattr(cdll, name) and name in _hip.EXPORTED_SYMBOLS, name
    header = open(os.path.join(os.path.dirname(os.path.abspath(__graft_entry__.__file__)), 'include', 'mvector_hip.h')).read()
    for macro, value in (('MV_SNORM_S', _hip.MV_SNORM_S), ('MV_SNORM_Z', _hip.MV_SNORM_Z), ('MV_SNORM_T', _hip.MV_SNORM_T),
                         ('MV_COHORT_MAX_ROWS', _hip.MV_COHORT_MAX_ROWS)):
        assert f'#define {macro} {value}\n' in header, macro
    cdll.mv_abi_version.restype = ctypes.c_int
    assert cdll.mv_abi_version() == 5


# ------------------------------------------------------------------ host layers
def _restated_stats(x, cohort, top_n):
    """the definition written out once more, independently of mvector.metric.score_norm: row-by-row float32 scores, the oracle's selection,
    fp64 sums in the order of the selection"""
    tiny = np.float32(1.17549435e-38)
    dots = np.stack([(cohort * row).sum(axis=1) for row in x])
    cos = dots / (np.maximum(np.linalg.norm(x, axis=1), tiny)[:, None] * np.maximum(np.linalg.norm(cohort, axis=1), tiny)[None, :])
    kept = snc.top_values(cos.astype(np.float32), top_n).astype(np.float64)
    mean = kept.sum(axis=1) / kept.shape[1]
    std = np.sqrt(((kept - mean[:, None]) ** 2).sum(axis=1) / kept.shape[1])
    return mean.astype(np.float32), std.astype(np.float32)


def test_score_normalizer_on_cpu_tensors_equals_the_restatement():
    from mvector.metric.score_norm import ScoreNormalizer
    g = torch.Generator().manual_seed(12)
    cohort, trials, enrol = torch.randn(90, 24, generator=g), torch.randn(7, 24, generator=g), torch.randn(4, 24, generator=g)
    cohort[5] = cohort[40]                                     # a tie inside the cohort
    scores = torch.randn(7, 4, generator=g) * 0.2
    for top_n in (30, 90, 300):
        sn = ScoreNormalizer(cohort, top_n=top_n)
        assert isinstance(sn.cohort, np.ndarray)               # a CPU tensor stays on the host
        tm, ts = sn.stats(trials)
        em, es = sn.stats(enrol.numpy())
        want_t, want_e = _restated_stats(trials.numpy(), cohort.numpy(), top_n), _restated_stats(enrol.numpy(), cohort.numpy(), top_n)
        for got, want in ((tm, want_t[0]), (ts, want_t[1]), (em, want_e[0]), (es, want_e[1])):
            assert isinstance(got, np.ndarray) and got.dtype == np.float32 and got.tobytes() == want.tobytes()
        for mode in ('s', 'z', 't'):
            sn_m = ScoreNormalizer(cohort.numpy(), top_n=top_n, mode=mode)
            want = snc.numpy_norm(scores.numpy(), want_t[0], want_t[1], want_e[0], want_e[1], mode)
            out = sn_m.normalize(scores, trial_embeddings=trials, enroll_embeddings=enrol)
            assert isinstance(out, torch.Tensor) and out.dtype == torch.float32 and not out.is_cuda
            snc.assert_same_floats(out.numpy(), want, f'embeddings, mode {mode}')
            out = sn_m.normalize(scores.numpy(), trial_stats=(tm, ts), enroll_stats=(em, es))
            assert isinstance(out, np.ndarray)
            snc.assert_same_floats(out, want, f'precomputed statistics, mode {mode}')
        # the side a mode does not use needs nothing; a used side needs one of the two
        z = ScoreNormalizer(cohort, top_n=top_n, mode='z').normalize(scores, enroll_embeddings=enrol)
        snc.assert_same_floats(z.numpy(), snc.numpy_norm(scores.numpy(), want_t[0], want_t[1], want_e[0], want_e[1], 'z'), 'z, no trial side')
        with pytest.raises(ValueError, match='trial_embeddings or trial_stats'):
            sn.normalize(scores, enroll_embeddings=enrol)
    for bad in (1, 0, -3):
        with pytest.raises(ValueError, match='below 2'):
            ScoreNormalizer(cohort, top_n=bad)
    with pytest.raises(ValueError, match='mode'):
        ScoreNormalizer(cohort, mode='as')


def test_cohort_means_equal_a_plain_fp64_loop():
    from mvector.metric.score_norm import cohort_means
    g = torch.Generator().manual_seed(2)
    emb = torch.randn(11, 6, generator=g)
    labels = [4, 9, 4, 2, 9, 9, 4, 7, 2, 4, 9]
    want = []
    for spk in (4, 9, 2, 7):                                   # order of first appearance
        acc, cnt = np.zeros(6, dtype=np.float64), 0
        for row, lab in zip(emb.numpy(), labels):
            if lab == spk:
                acc, cnt = acc + row.astype(np.float64), cnt + 1
        want.append((acc / cnt).astype(np.float32))
    for lab in (labels, np.array(labels, dtype=np.int32), torch.tensor(labels)):
        got = cohort_means(emb, lab)
        assert got.dtype == np.float32 and got.tobytes() == np.stack(want).tobytes()
    assert cohort_means(emb.numpy()[:0], []).shape == (0, 6)


def test_trainer_evaluate_normalized_cpu_is_the_numpy_composition(tmp_path):
    from mvector.metric.metrics import verification_metrics
    from mvector.metric.score_norm import ScoreNormalizer, cohort_means
    from mvector.trainer import MVectorTrainer
    cfg, model_dir, cohort_list = snc.make_eval_set(tmp_path)
    t = MVectorTrainer(cfg, use_gpu=False)
    before = t.evaluate(resume_model=model_dir)
    for top_n, mode, per_speaker in ((3, 's', True), (300, 'z', True), (4, 't', False)):
        got = t.evaluate_normalized(cohort_list, top_n=top_n, mode=mode, resume_model=model_dir, per_speaker=per_speaker)
        (ef, el), (tf, tl), (cf, cl) = snc.embed_lists(t, cohort_list)
        cohort = cohort_means(cf, cl) if per_speaker else cf.numpy()
        assert cohort.shape == ((5 if per_speaker else 10), 192)
        raw = (torch.nn.functional.normalize(tf, dim=1) @ torch.nn.functional.normalize(ef, dim=1).t()).numpy().astype(np.float32)
        sn = ScoreNormalizer(cohort, top_n=top_n, mode=mode)
        want = verification_metrics(sn.normalize(raw, trial_embeddings=tf.numpy(), enroll_embeddings=ef.numpy()), tl, el)
        assert got == want and all(isinstance(v, float) for v in got), (got, want)
    assert t.evaluate(resume_model=model_dir) == before            # evaluate itself returns what it returned
    assert got != before


def test_cpu_predictor_contrast_normalized_is_the_one_by_one_composition(tmp_path):
    import scipy.io.wavfile as wavfile
    from mvector.metric.score_norm import ScoreNormalizer, cosine_scores
    from mvector.predict import MVectorPredictor
    man, sd, _, _, _ = load_case('tdnn')
    (tmp_path / 'model').mkdir()
    torch.save({'0.' + k: v for k, v in sd.items()}, str(tmp_path / 'model' / 'model.pth'))
    paths = []
    for j, pcm in enumerate(np.load(os.path.join(GOLDEN, 'real_audio.npz'))['pcm16']):
        paths.append(str(tmp_path / f'u{j}.wav'))
        wavfile.write(paths[-1], 16000, pcm)
    cfg = dict(dataset_conf=dict(dataset=dict(min_duration=0.3, sample_rate=16000, use_dB_normalization=True, target_dB=-20),
                                 eval_conf=dict(batch_size=2)),
               preprocess_conf=dict(feature_method='Fbank', method_args=dict(sample_frequency=16000, num_mel_bins=80)),
               model_conf=dict(model='TDNN', model_args=dict(embd_dim=192)))
    with pytest.MonkeyPatch.context() as mp:
        mp.setenv('CUDA_VISIBLE_DEVICES', os.environ.get('CUDA_VISIBLE_DEVICES', ''))   # (the CPU predictor sets it: restored afterwards)
        p = MVectorPredictor(cfg, threshold=0.3, audio_db_path=str(tmp_path / 'audio_db'), model_path=str(tmp_path / 'model'), use_gpu=False)
    g = torch.Generator().manual_seed(4)
    sn = ScoreNormalizer(torch.randn(40, 192, generator=g), top_n=10)
    e1, e2 = p.predict(paths[0])[None, :], p.predict(paths[1])[None, :]
    want = sn.normalize(cosine_scores(e1, e2), trial_embeddings=e1, enroll_embeddings=e2)
    got = p.contrast_normalized(paths[0], paths[1], sn)
    assert isinstance(got, float) and want.shape == (1, 1) and got == float(want[0, 0])
    tm, ts = sn.stats(e1)
    em, es = sn.stats(e2)
    s = np.float32(cosine_scores(e1, e2)[0, 0])
    assert got == float(np.float32(0.5) * ((s - tm[0]) / ts[0] + (s - em[0]) / es[0]))
