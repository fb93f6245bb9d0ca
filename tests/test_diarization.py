"""Speaker diarization without a GPU: the host classes (mvector/infer_utils/speaker_diarization.py) against fixtures written by the REFERENCE's
own classes (tools/make_diarization_golden.py), and the kernels of csrc/diarize.hip on the emulator build against the host restatement, fp64
numpy and scipy.  The same kernel checks run on the device in tests/test_gpu_diarization.py (tests/diarization_checks.py holds them)."""
import json
import os
import types

import numpy as np
import pytest
import torch

import diarization_checks as dc
from helpers import GOLDEN


@pytest.fixture(scope='module')
def emu():
    import emu_lib
    return emu_lib.emu_cdll()


# ------------------------------------------------------------------ host classes vs the reference's fixtures
def test_chunk_tables_match_the_reference():
    from mvector.infer_utils.speaker_diarization import SpeakerDiarization
    z = np.load(os.path.join(GOLDEN, 'diarization_chunks.npz'))
    sd = SpeakerDiarization(sample_rate=1000)
    for name in ('below', 'exact', 'above', 'ragged', 'one_over'):   # below, at and above one chunk; a length that is no multiple of the shift
        n = int(z[f'{name}_n'])
        data = np.arange(1, n + 1, dtype=np.float32)
        segs = sd._chunk([[2.5, 2.5 + n / 1000, data]])
        assert np.array_equal(np.array([[s[0], s[1]] for s in segs]), z[f'{name}_times']), name
        assert np.array_equal(np.stack([s[2] for s in segs]), z[f'{name}_rows']), name

        # chunk_table: the same chunks as (first sample in the recording, samples before the padding)
        rec = types.SimpleNamespace(samples=np.concatenate([np.zeros(2500, dtype=np.float32), data, np.zeros(4000, dtype=np.float32)]), sample_rate=1000)
        sd5 = SpeakerDiarization(sample_rate=1000)
        sd5._check_audio_list = lambda audio: None   # the regions of this fixture are shorter than the 5 s the check asks for
        times, starts, lens, chunk_len = sd5.chunk_table(rec, vad_segments=[dict(start=2.5, end=2.5 + n / 1000)])
        assert chunk_len == 1500 and [t[:2] for t in times] == [[s[0], s[1]] for s in segs]
        for st, ln, s in zip(starts, lens, segs):
            row = np.zeros(1500, dtype=np.float32)
            row[:ln] = rec.samples[st:st + ln]
            assert np.array_equal(row, s[2]), name


@pytest.mark.parametrize('n', dc.GOLDEN_N)
def test_host_pruning_laplacian_labels_and_centres_match_the_reference(n):
    from mvector.infer_utils.speaker_diarization import SpeakerDiarization, SpectralCluster
    g = dc.golden(n)
    X = g['X'].astype(np.float32)
    sc = SpectralCluster()
    assert sc.n_prune(n) == int(g['n_prune'])
    if 'sim' in g:   # on the reference's own fp32 similarity: bit-equal pruning, symmetrisation and Laplacian
        assert np.abs(sc.get_sim_mat(X) - g['sim']).max() <= 4 * 2.0 ** -24   # a few fp32 roundings of values <= 1 (the BLAS may sum in another order)
        pruned = sc.p_pruning(g['sim'].copy())
        sym = 0.5 * (pruned + pruned.T)
        lap = sc.get_laplacian(sym)
        assert sym.dtype == lap.dtype == np.float32
        assert np.array_equal(sym, g['M']) and np.array_equal(lap, g['L'])
    sd = SpeakerDiarization()
    labels = sd._correct_labels(sc(X.copy()))
    assert np.array_equal(labels, g['labels'])
    merged, centres = sd.clustering(X.copy())
    assert np.array_equal(merged, g['merged'])
    assert centres.dtype == np.float32 and np.abs(centres - g['centres']).max() <= 1e-6
    segments = [[0.75 * i, 0.75 * i + 1.5, None] for i in range(n)]
    assert sd.postprocess(segments, merged) == json.loads(str(g['postprocess']))
    assert sd.clustering(X.copy(), speaker_num=2)[0].max() + 1 <= 2   # the oracle count bypasses the gap rule


def _misc():
    with open(os.path.join(GOLDEN, 'diarization_misc.json')) as f:
        return json.load(f)


def test_merge_by_cos_smooth_and_postprocess_match_the_reference():
    from mvector.infer_utils.speaker_diarization import SpeakerDiarization
    sd = SpeakerDiarization()
    misc = _misc()
    names = [c['name'] for c in misc['merge']]
    assert names == ['pair_above', 'pair_below', 'all_merge']
    for c in misc['merge']:   # a pair above 0.78 merges, a pair below stays
        out = sd._merge_by_cos(np.array(c['labels']), [np.array(r) for r in c['centres']], c['threshold'])
        assert out.tolist() == c['out'], c['name']
    assert max(misc['merge'][0]['out']) == 1 and max(misc['merge'][1]['out']) == 2 and max(misc['merge'][2]['out']) == 0
    assert [c['name'] for c in misc['smooth']] == ['first_short', 'middle_short_left', 'middle_short_right', 'last_short', 'nothing_short']
    for c in misc['smooth']:
        out = sd._smooth([list(r) for r in c['res']])
        assert [[float(r[0]), float(r[1]), int(r[2])] for r in out] == c['out'], c['name']
    for c in misc['postprocess']:
        out = sd.postprocess([s + [None] for s in c['segments']], np.array(c['labels']))
        assert out == c['out'], c['name']


def test_segments_audio_needs_vad_segments_without_a_vad_method():
    from mvector.data_utils.audio import AudioSegment
    from mvector.infer_utils.speaker_diarization import SpeakerDiarization
    seg = AudioSegment.from_ndarray(np.zeros(16000 * 8, dtype=np.float32), 16000)
    sd = SpeakerDiarization()
    if not hasattr(seg, 'vad'):
        with pytest.raises(NotImplementedError, match='yeaudio.*vad_segments|vad_segments.*yeaudio'):
            sd.segments_audio(seg)
    chunks = sd.segments_audio(seg, vad_segments=[dict(start=0.5, end=3.0), dict(start=4.0, end=7.25)])
    assert len(chunks) == 3 + 4 and all(c[2].shape == (24000,) for c in chunks)
    with pytest.raises(AssertionError):
        sd.segments_audio(seg, vad_segments=[dict(start=0.5, end=3.0)])   # under 5 s of speech


def test_speaker_diarization_is_part_of_the_predictor_surface():
    import inspect
    from mvector.predict import MVectorPredictor
    sig = inspect.signature(MVectorPredictor.speaker_diarization)
    assert list(sig.parameters) == ['self', 'audio_data', 'sample_rate', 'speaker_num', 'search_audio_db', 'vad_segments']
    assert sig.parameters['vad_segments'].default is None


def test_device_path_refuses_more_than_16_eigenpairs(emu):
    from mvector.infer_utils.speaker_diarization import SpectralCluster
    X = torch.from_numpy(dc.golden(33)['X'].astype(np.float32))
    with pytest.raises(ValueError, match='speaker_num'):
        SpectralCluster(cdll=emu)(X, oracle_num=17)


# ------------------------------------------------------------------ the kernels on the emulator
def test_emu_wave_chunks(emu):
    dc.check_wave_chunks(emu, 'cpu')


@pytest.mark.parametrize('n', [5, 33, 65])   # nothing pruned; ragged against any 32 / 64 tiling
def test_emu_affinity_laplacian(emu, n):
    dc.check_affinity(emu, 'cpu', n)


def test_emu_affinity_tie_rule(emu):
    dc.check_tie_rule(emu, 'cpu')


@pytest.mark.parametrize('n', [5, 31, 33, 65])
def test_emu_laplacian_eig_lowest(emu, n):
    dc.check_eig(emu, 'cpu', n)


def test_emu_eig_reports_non_convergence(emu):
    dc.check_not_converged(emu, 'cpu', 65)


def test_emu_refusals_by_name(emu):
    dc.check_refusals(emu, 'cpu')


@pytest.mark.parametrize('n', [33, 40])
def test_emu_spectral_cluster_on_a_tensor_gives_the_golden_labels(emu, n):
    dc.check_spectral_cluster_golden(emu, 'cpu', n)
