"""The fused cosine + top-k search on the device: the checks of tests/search_checks.py on the product library (also at sizes the emulator is
too slow for, and on a second stream), and MVectorPredictor.search / recognition_batch / recognition on the GPU predictor."""
import os

import numpy as np
import pytest
import torch

import search_checks as sc

pytestmark = pytest.mark.gpu
DEV = 'cuda'


@pytest.mark.parametrize('n,m,dim,k', sc.EQUAL_CASES + sc.WIDE_CASES)
def test_gpu_topk_is_the_topk_of_the_cosine_matrix(n, m, dim, k):
    sc.check_equals_cosine(None, DEV, n, m, dim, k)


@pytest.mark.parametrize('n,m,dim,k,hint', sc.LARGE_CASES)
def test_gpu_topk_of_a_large_gallery(n, m, dim, k, hint):
    sc.check_equals_cosine(None, DEV, n, m, dim, k, hints=(0, hint))


def test_gpu_topk_rows_off_the_16_byte_grid():
    sc.check_equals_cosine(None, DEV, 17, 17, 192, 5, hints=(0, 2), misalign=True)


def test_gpu_topk_with_more_than_64_slices():
    sc.check_equals_cosine(None, DEV, 2, 1700, 16, 3, hints=(100, 0, 64, 65))   # the merge runs four waves above 64 lists, one below


def test_gpu_ties_go_to_the_lower_row_across_slice_boundaries():
    sc.check_ties(None, DEV)


def test_gpu_special_values_and_empty_sides():
    sc.check_special_values(None, DEV)


def test_gpu_no_hidden_state():
    sc.check_no_hidden_state(None, DEV, second_stream=True)


def test_gpu_refusals_by_name():
    sc.check_refusals(None, DEV)


# ------------------------------------------------------------------ the predictor
@pytest.fixture(scope='module')
def predictor_files(tmp_path_factory):
    """TDNN golden weights and the four real clips as 16 kHz mono files, as test_gpu_register_recognition_remove_user_device_gallery uses
    them; the second clip also as a 44.1 kHz stereo file"""
    import scipy.io.wavfile as wavfile
    from scipy.signal import resample_poly
    from helpers import GOLDEN, load_case
    d = tmp_path_factory.mktemp('search_gpu')
    man, sd, _, _, _ = load_case('tdnn')
    (d / 'model').mkdir()
    torch.save({'0.' + k: v for k, v in sd.items()}, str(d / 'model' / 'model.pth'))
    paths = []
    clips = np.load(os.path.join(GOLDEN, 'real_audio.npz'))['pcm16']
    for j, pcm in enumerate(clips):
        paths.append(str(d / f'u{j}.wav'))
        wavfile.write(paths[-1], 16000, pcm[:16000])
    hi = np.round(resample_poly(clips[1][:16000].astype(np.float64), 441, 160)).clip(-32768, 32767).astype(np.int16)
    other_rate = str(d / 'u1_44k.wav')
    wavfile.write(other_rate, 44100, np.stack([hi, hi], axis=1))
    cfg = dict(dataset_conf=dict(dataset=dict(min_duration=0.3, sample_rate=16000, use_dB_normalization=True, target_dB=-20),
                                 eval_conf=dict(batch_size=2)),
               preprocess_conf=dict(feature_method='Fbank', method_args=dict(sample_frequency=16000, num_mel_bins=80)),
               model_conf=dict(model='TDNN', model_args=dict(embd_dim=192)))
    return cfg, str(d / 'model'), paths, other_rate, d


def test_gpu_predictor_search_and_recognition_batch(predictor_files):
    from mvector.predict import MVectorPredictor
    cfg, model_dir, paths, other_rate, d = predictor_files
    p = MVectorPredictor(cfg, threshold=0.3, audio_db_path=str(d / 'audio_db'), model_path=model_dir, use_gpu=True)
    assert p.register(paths[0], 'alice')[0] and p.register(paths[1], 'bob')[0] and p.register(paths[2], 'carol')[0]
    dg = p._device_gallery
    assert dg.users == ['alice', 'bob', 'carol'] and dg.uploads == 0
    each = [p.recognition(a) for a in paths]
    assert [e[0] for e in each[:3]] == ['alice', 'bob', 'carol']
    batch = p.recognition_batch(paths)
    print('recognition per item:', each, '\nrecognition_batch:   ', batch)
    assert batch == each
    for a in paths:
        top = p.search(a, top_k=3)
        assert len(top) == 3 and sorted(n for n, _ in top) == ['alice', 'bob', 'carol']
        assert [s for _, s in top] == sorted((s for _, s in top), reverse=True)
        assert top[0] == p.recognition(a, threshold=-1.0)
    p.threshold = 0.3
    assert len(p.search(paths[0])) == 3 and len(p.search(paths[0], top_k=1)) == 1          # stops at the number of users
    # the top-1 of the search is what the score matrix + arg-max of the same embedding gives
    from mvector import _hip
    emb = p._embed(paths[3])
    row = _hip.cosine(emb, dg.matrix()).cpu().numpy()[0]
    assert p.search(paths[3], top_k=1)[0] == [dg.users[int(np.argmax(row))], round(float(row.max()), 5)]
    # a mixed list with a file of another sample rate (resampled as recognition() resamples it), bytes and an array among the items
    with open(paths[2], 'rb') as f:
        as_bytes = f.read()
    import scipy.io.wavfile as wavfile
    floats = wavfile.read(paths[3])[1].astype(np.float32) / 32768.0
    mixed_items = [paths[0], other_rate, as_bytes, floats]
    mixed = p.recognition_batch(mixed_items)
    assert mixed == [p.recognition(a) for a in mixed_items] and [r[0] for r in mixed[:3]] == ['alice', 'bob', 'carol']
    assert dg.uploads == 0                                                                  # nothing went up for any of it
    assert p.remove_user('bob') and p.recognition_batch(paths[:3])[1] == p.recognition(paths[1])
    assert [n for n, _ in p.search(paths[1], top_k=5)] in (['alice', 'carol'], ['carol', 'alice'])
