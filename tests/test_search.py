"""The fused cosine + top-k search without a GPU: the kernels of csrc/search.hip on the emulator build against the cosine matrix of the same
library (tests/search_checks.py holds the checks; tests/test_gpu_search.py runs them on the device), and the host layers: DeviceGallery.search
on CPU tensors, MVectorPredictor.search / recognition_batch on the CPU predictor."""
import os

import numpy as np
import pytest
import torch

import search_checks as sc
from helpers import GOLDEN, load_case


@pytest.fixture(scope='module')
def emu():
    import emu_lib
    return emu_lib.emu_cdll()


@pytest.mark.parametrize('n,m,dim,k', sc.EQUAL_CASES + sc.WIDE_CASES)
def test_emu_topk_is_the_topk_of_the_cosine_matrix(emu, n, m, dim, k):
    sc.check_equals_cosine(emu, 'cpu', n, m, dim, k)


def test_emu_topk_rows_off_the_16_byte_grid(emu):
    sc.check_equals_cosine(emu, 'cpu', 17, 17, 192, 5, hints=(0, 2), misalign=True)


def test_emu_topk_with_more_than_64_slices(emu):
    sc.check_equals_cosine(emu, 'cpu', 2, 1700, 16, 3, hints=(100, 0))      # the merge runs four waves above 64 lists, one below


def test_emu_ties_go_to_the_lower_row_across_slice_boundaries(emu):
    sc.check_ties(emu, 'cpu')


def test_emu_special_values_and_empty_sides(emu):
    sc.check_special_values(emu, 'cpu')


def test_emu_no_hidden_state(emu):
    sc.check_no_hidden_state(emu, 'cpu')


def test_emu_refusals_by_name(emu):
    sc.check_refusals(emu, 'cpu')


def test_the_library_exports_the_search():
    import ctypes
    import __graft_entry__
    from mvector import _hip
    cdll = ctypes.CDLL(__graft_entry__.build())
    for name in ('mv_cosine_topk_workspace_bytes', 'mv_cosine_topk_f32'):
        assert hasattr(cdll, name) and name in _hip.EXPORTED_SYMBOLS, name


# ------------------------------------------------------------------ host layers
def _numpy_scores(q, g):
    """DeviceGallery.search's scores on CPU tensors, restated: dot / (max(|q|, tiny) max(|g|, tiny)) in float32, every dot product summed on
    its own (a matrix product's bits depend on where a column sits)"""
    tiny = np.float32(1.17549435e-38)
    dots = np.stack([(g * row).sum(axis=1) for row in q])
    return dots / (np.maximum(np.linalg.norm(q, axis=1), tiny)[:, None] * np.maximum(np.linalg.norm(g, axis=1), tiny)[None, :])


def test_keys_and_rule_of_the_host_restatement():
    from mvector.infer_utils.gallery import sort_keys, top_k_of_scores
    x = np.array([[0.5, -0.0, 0.0, np.nan, np.inf, -np.inf, 0.5, -1.0, 1e-45, -1e-45]], dtype=np.float32)
    x[0, 6] = np.float32(0.5)
    assert np.array_equal(sort_keys(x).astype(np.uint64), sc.keys_of(x))
    s, i = top_k_of_scores(x, 12)
    assert i[0].tolist() == [3, 4, 0, 6, 8, 1, 2, 9, 7, 5, -1, -1] and np.isneginf(s[0, 10:]).all() and np.isnan(s[0, 0])
    sc.assert_same((s, i), sc.reference(x, 12), 'host rule')
    s, i = top_k_of_scores(np.zeros((2, 0), dtype=np.float32), 3)
    assert (i == -1).all() and np.isneginf(s).all()


def test_device_gallery_search_on_cpu_tensors():
    from mvector.infer_utils.gallery import DeviceGallery
    g = torch.Generator().manual_seed(3)
    dg = DeviceGallery('cpu', 24, capacity=2)
    rows = torch.randn(6, 24, generator=g)
    for j, name in enumerate(['a', 'b', 'c', 'd', 'e', 'b']):     # 'b' twice: its row is a sum
        dg.add(name, rows[j])
    dg.add('f', 2.0 * rows[0])                                    # the same direction as 'a': a tie that the lower row wins
    uploads = dg.uploads
    q = torch.cat([rows[:1], torch.randn(4, 24, generator=g)])
    s, i = dg.search(q, 4)
    assert s.dtype == torch.float32 and i.dtype == torch.int32 and s.shape == (5, 4)
    sc.assert_same((s.numpy(), i.numpy()), sc.reference(_numpy_scores(q.numpy(), dg.matrix().numpy()), 4), 'six users')
    assert [dg.users[j] for j in i[0, :2].tolist()] == ['a', 'f'] and s[0, 0] == s[0, 1]
    assert dg.remove('c') and dg.users == ['a', 'b', 'd', 'e', 'f']    # a user removed in the middle: the rows behind it moved up
    s, i = dg.search(q, 8)
    sc.assert_same((s.numpy(), i.numpy()), sc.reference(_numpy_scores(q.numpy(), dg.matrix().numpy()), 8), 'after remove')
    assert (i[:, 5:] == -1).all() and [dg.users[j] for j in i[0, :2].tolist()] == ['a', 'f']
    s1, i1 = dg.search(q[2], 1)                                    # one query as a vector
    assert s1.shape == (1, 1) and i1[0, 0] == i[2, 0]
    sh, ih = dg.search(q, 8, to_host=True)                         # the same as numpy arrays
    assert isinstance(sh, np.ndarray) and sh.tobytes() == s.numpy().tobytes() and ih.tobytes() == i.numpy().tobytes()
    assert dg.uploads == uploads
    with pytest.raises(AssertionError):
        dg.search(q, 65)
    # 5000 synthetic users written straight into the sums
    big = DeviceGallery('cpu', 32, capacity=8192)
    big.sums[:5000] = torch.randn(5000, 32, generator=g)
    big.sums[4000] = big.sums[17]
    big.users = [f'u{j}' for j in range(5000)]
    big._row_of = {u: j for j, u in enumerate(big.users)}
    q = torch.cat([big.sums[17:18] * 0.5, torch.randn(6, 32, generator=g)])
    s, i = big.search(q, 10)
    sc.assert_same((s.numpy(), i.numpy()), sc.reference(_numpy_scores(q.numpy(), big.matrix().numpy()), 10), '5000 users')
    assert i[0, :2].tolist() == [17, 4000] and big.uploads == 0


@pytest.fixture(scope='module')
def cpu_predictor(tmp_path_factory):
    """the CPU predictor on the TDNN golden weights with three of the four real clips enrolled through the gallery folder"""
    import scipy.io.wavfile as wavfile
    from mvector.predict import MVectorPredictor
    d = tmp_path_factory.mktemp('search_cpu')
    man, sd, _, _, _ = load_case('tdnn')
    (d / 'model').mkdir()
    torch.save({'0.' + k: v for k, v in sd.items()}, str(d / 'model' / 'model.pth'))
    paths = []
    for j, pcm in enumerate(np.load(os.path.join(GOLDEN, 'real_audio.npz'))['pcm16']):
        paths.append(str(d / f'u{j}.wav'))
        wavfile.write(paths[-1], 16000, pcm)
    for user, j in (('alice', 0), ('bob', 1), ('carol', 2)):
        (d / 'audio_db' / user).mkdir(parents=True)
        wavfile.write(str(d / 'audio_db' / user / '0.wav'), 16000, np.load(os.path.join(GOLDEN, 'real_audio.npz'))['pcm16'][j])
    cfg = dict(dataset_conf=dict(dataset=dict(min_duration=0.3, sample_rate=16000, use_dB_normalization=True, target_dB=-20),
                                 eval_conf=dict(batch_size=2)),
               preprocess_conf=dict(feature_method='Fbank', method_args=dict(sample_frequency=16000, num_mel_bins=80)),
               model_conf=dict(model='TDNN', model_args=dict(embd_dim=192)))
    with pytest.MonkeyPatch.context() as mp:
        mp.setenv('CUDA_VISIBLE_DEVICES', os.environ.get('CUDA_VISIBLE_DEVICES', ''))   # (the CPU predictor sets it: restored afterwards)
        p = MVectorPredictor(cfg, threshold=0.3, audio_db_path=str(d / 'audio_db'), model_path=str(d / 'model'), use_gpu=False)
    return p, paths


def test_cpu_predictor_recognition_batch_is_recognition_per_item(cpu_predictor):
    p, paths = cpu_predictor
    each = [p.recognition(a) for a in paths]
    assert [e[0] for e in each[:3]] == ['alice', 'bob', 'carol']
    assert p.recognition_batch(paths) == each
    assert p.recognition_batch([]) == []
    high = p.recognition_batch(paths, threshold=0.9999)
    assert high == [p.recognition(a) for a in paths] and high[3] == [None, None]
    p.threshold = 0.3


def test_cpu_predictor_search(cpu_predictor):
    p, paths = cpu_predictor
    for a in paths:
        top = p.search(a, top_k=3)
        assert len(top) == 3 and sorted(n for n, _ in top) == ['alice', 'bob', 'carol']
        assert [s for _, s in top] == sorted((s for _, s in top), reverse=True)
        assert top[0] == p.recognition(a, threshold=-1.0)
    p.threshold = 0.3
    assert len(p.search(paths[0])) == 3 and len(p.search(paths[0], top_k=1)) == 1    # stops at the number of users
    assert p.search(paths[0], top_k=2) == p.search(paths[0], top_k=3)[:2]
