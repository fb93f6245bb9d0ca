"""Verification metrics on the device: the kernel checks of tests/verif_metric_checks.py on the product library (tile edges, a table scan of
more than one trip, a second stream), metrics.verification_metrics on device tensors against the reference's floats, and
MVectorTrainer.evaluate(use_gpu=True) against the host functions on the same device scores."""
import os

import numpy as np
import pytest
import torch

import verif_metric_checks as vc
from helpers import load_case
from oracle import frontend

DEV = 'cuda'
TILE = 4096
# the scan of the [digit][tile] table works in chunks of 1024 entries and one workgroup scans the chunk sums 256 per trip: more than
# 256 * 1024 / 256 = 1024 tiles make it take a second trip (the grids are not capped: one workgroup per tile and per chunk)
MANY_TILES_N = 1100 * TILE + 5


@pytest.mark.gpu
def test_gpu_sort_tile_is_what_the_sizes_assume():
    assert vc.sort_tile(None) == TILE


@pytest.mark.gpu
@pytest.mark.parametrize('n', vc.sort_sizes(TILE))
def test_gpu_sort_scores(n):
    vc.check_sort(None, DEV, n)


@pytest.mark.gpu
def test_gpu_sort_scores_table_scan_of_more_than_one_trip():
    vc.check_sort(None, DEV, MANY_TILES_N, kinds=('normal', 'ties17'))


@pytest.mark.gpu
@pytest.mark.parametrize('name', vc.CASES)
def test_gpu_metrics_equal_the_reference(name):
    vc.check_golden(None, DEV, name)
    vc.check_golden_public(DEV, name)


@pytest.mark.gpu
def test_gpu_cross_label_ties_follow_the_flat_index():
    vc.check_cross_label_ties(None, DEV, second_stream=True)


@pytest.mark.gpu
def test_gpu_edges_and_refusals():
    vc.check_edges_raw(None, DEV)
    vc.check_edges_public(DEV)


@pytest.mark.gpu
def test_gpu_transposed_matrix_gives_the_same_metrics():
    vc.check_transpose_invariance(None, DEV)


# ------------------------------------------------------------------ evaluate
def _make_eval_set(tmp_path, n_spk=4, per_spk=4, seed=9):
    """a small TDNN evaluation: wav files of different lengths, enrol / trial lists and the golden TDNN checkpoint (Fbank, 80 bins)"""
    import scipy.io.wavfile as wavfile
    man, sd, _, _, _ = load_case('tdnn')
    model_dir = tmp_path / 'model'
    model_dir.mkdir()
    torch.save({'0.' + k: v for k, v in sd.items()}, str(model_dir / 'model.pth'))
    rng = np.random.default_rng(seed)
    lines = {'enroll': [], 'trials': []}
    for spk in range(n_spk):
        base = frontend.synth_waveforms(1, 16000, seed=100 + spk)[0].numpy()
        for u in range(per_spk):
            n = int(rng.integers(9000, 16000))
            x = base[:n] + 0.02 * rng.standard_normal(n).astype(np.float32)
            path = str(tmp_path / f's{spk}_u{u}.wav')
            wavfile.write(path, 16000, np.clip(x * 20000, -32768, 32767).astype(np.int16))
            lines['enroll' if u == 0 else 'trials'].append(f'{path}\t{spk}\n')
    for k, v in lines.items():
        with open(str(tmp_path / f'{k}.txt'), 'w') as f:
            f.writelines(v)
    cfg = dict(dataset_conf=dict(dataset=dict(min_duration=0.3, sample_rate=16000, use_dB_normalization=True, target_dB=-20),
                                 eval_conf=dict(batch_size=4, max_duration=20), dataLoader=dict(num_workers=0),
                                 enroll_list=str(tmp_path / 'enroll.txt'), trials_list=str(tmp_path / 'trials.txt')),
               preprocess_conf=dict(feature_method='Fbank', method_args=dict(sample_frequency=16000, num_mel_bins=80)),
               model_conf=dict(model='TDNN', model_args=dict(embd_dim=192)))
    return cfg, str(model_dir)


@pytest.mark.gpu
def test_gpu_evaluate_returns_what_the_host_functions_compute_from_the_same_scores(tmp_path, monkeypatch):
    from mvector.metric import metrics
    from mvector.trainer import MVectorTrainer
    cfg, model_dir = _make_eval_set(tmp_path)
    import mvector.trainer as trainer_mod
    seen = []
    inner = trainer_mod.verification_metrics
    monkeypatch.setattr(trainer_mod, 'verification_metrics', lambda *a, **kw: seen.append(a) or inner(*a, **kw))
    gpu = MVectorTrainer(cfg, use_gpu=True)
    got = gpu.evaluate(resume_model=model_dir)
    # what evaluate handed over: the device score matrix and the two label vectors, nothing N-sized from the host
    assert len(seen) == 1 and seen[0][0].is_cuda and seen[0][0].shape == (12, 4)
    trial_labels, enroll_labels = (np.asarray(x.cpu()) for x in seen[0][1:3])
    assert trial_labels.shape == (12,) and enroll_labels.shape == (4,)
    # the parent's host path on the same device scores: download, label matrix, the three reference functions
    scores = seen[0][0].cpu().numpy().astype(np.float32).reshape(-1)
    labels = (trial_labels[:, None] == enroll_labels[None, :]).astype(np.int32).reshape(-1)
    assert labels.sum() == 12
    assert np.intersect1d(scores[labels == 1], scores[labels == 0]).size == 0, 'a target score equals an impostor score: numpy leaves that order open'
    fnr, fpr, _ = metrics.compute_fnr_fpr(scores, labels)
    eer, thr = metrics.compute_eer(fnr, fpr, scores)
    want = (float(eer), float(metrics.compute_dcf(fnr, fpr)), float(thr))
    print(f'evaluate: device {got!r}, host functions on the same scores {want!r}')
    assert got == want and all(type(v) is float for v in got)
    # with save_image_path the call asks for the curve, finishes with the same floats and writes the figure when matplotlib is there
    out_dir = tmp_path / 'curve'
    assert gpu.evaluate(resume_model=model_dir, save_image_path=str(out_dir)) == want
    try:
        import matplotlib  # noqa: F401
    except ImportError:
        assert not out_dir.exists()
    else:
        assert os.path.getsize(str(out_dir / 'result.png')) > 0
