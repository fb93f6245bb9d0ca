"""Energy VAD on the device: the checks of tests/vad_checks.py on the product library (also a second stream), EnergyVad on CUDA tensors
against its numpy path, and MVectorPredictor.vad on the GPU feeding speaker_diarization, against the use_gpu=False predictor."""
import numpy as np
import pytest
import torch

import vad_checks as vc

pytestmark = pytest.mark.gpu
DEV = 'cuda'
RECIPE = dict(energy_threshold=5.5, frames_context=2, proportion_threshold=0.12)


def test_gpu_log_energy_against_the_fp64_oracle():
    worst_e, worst_t = vc.check_log_energy(None, DEV)
    print(f'log energy: largest |logE - ref| / bar {worst_e:.3g}, largest |thr - ref| / bar {worst_t:.3g} (bars: 4 L 2^-53 max(1, |logE|) and the threshold bar derived from it)')


@pytest.mark.parametrize('name', vc.RUN_CASES)
def test_gpu_decisions_and_runs_equal_the_oracle(name):
    _, refs, (worst_e, worst_t) = vc.check_case(None, DEV, name)
    print(f'{name}: frames {[r["T"] for r in refs]}, runs {[len(r["runs"]) for r in refs]}, smallest |logE - thr| {min(r["margin"] for r in refs):.3g}, '
          f'|logE - ref| / bar {worst_e:.3g}, |thr - ref| / bar {worst_t:.3g}')


def test_gpu_row_stride_and_unaligned_row_pointer():
    vc.check_layouts(None, DEV)


def test_gpu_truncated_run_list_reports_the_true_count():
    vc.check_truncated_runs(None, DEV)


def test_gpu_no_hidden_state():
    vc.check_no_hidden_state(None, DEV, second_stream=True)


def test_gpu_refusals_by_name():
    vc.check_refusals(None, DEV)


def test_gpu_energy_vad_on_cuda_tensors_equals_the_numpy_path():
    from mvector.infer_utils.vad import EnergyVad
    x, bursts = vc.synthetic_recording()
    y, _ = vc.synthetic_recording(seconds=9.0, seed=8, bursts=((0.0, 1.7), (2.6, 5.5), (6.3, 9.0)))   # speech from the first to the last sample
    for kw in (dict(), RECIPE):
        vad = EnergyVad(**kw)
        for wav in (x, y):
            host = vad(wav)
            got = vad(torch.from_numpy(wav).to(DEV))
            assert got == host and len(host) >= 3, (got, host)
            dec, log_e, thr = vad.frames(torch.from_numpy(wav).to(DEV))
            hdec, hlog, hthr = vad.frames(wav)
            assert dec.is_cuda and dec.dtype == torch.uint8 and np.array_equal(dec.cpu().numpy(), hdec)
            assert np.abs(log_e.cpu().numpy() - hlog).max() <= 4 * 400 * vc.U * np.abs(hlog).max() and abs(float(thr) - hthr) <= 1e-12
        vc.assert_brackets(vad(torch.from_numpy(x).to(DEV)), bursts, vad)
        batch = np.zeros((3, x.shape[0]), dtype=np.float32)
        batch[0], batch[1, :y.shape[0]], batch[2, :399] = x, y, x[:399]
        lengths = [x.shape[0], y.shape[0], 399]
        assert vad(torch.from_numpy(batch).to(DEV), lengths=lengths) == vad(batch, lengths=lengths) == [vad(x), vad(y), []]
    bad = x.copy()
    bad[5000] = np.nan
    assert EnergyVad()(torch.from_numpy(bad).to(DEV)) == []


def turns_recording(sr=16000, seed=21):
    """a recording built like tests/test_gpu_diarization.py's: two alternating harmonic voices (the second one speaks in syllables), here with
    0.6 s of the noise floor between the turns and in front of the first one, every turn setting in and dying away over vad_checks.RAMP
    -> (samples fp32, the turns [(start s, end s, speaker)])"""
    from test_gpu_diarization import _voice
    rng = np.random.default_rng(seed)
    voices = [dict(f0=120.0, formants=((500.0, 1.0), (1500.0, 0.5), (2500.0, 0.25)), gate_rate=0),
              dict(f0=220.0, formants=((850.0, 1.0), (1200.0, 0.7), (3200.0, 0.4)), gate_rate=4)]
    turns = [(0.6, 4.1, 0), (4.7, 8.05, 1), (8.65, 12.4, 0), (13.0, 16.35, 1), (16.95, 20.4, 0), (21.0, 24.35, 1)]
    x = np.zeros(int(25.0 * sr))
    for st, ed, w in turns:
        n0, n1 = int(round(st * sr)), int(round(ed * sr))
        x[n0:n1] = vc.soft_edges(n1 - n0, sr) * _voice(np.arange(n1 - n0) / sr, sr, **voices[w])
    x += 0.003 * rng.standard_normal(x.shape[0])
    return (0.3 * x / np.abs(x).max()).astype(np.float32), turns


def test_gpu_predictor_vad_feeds_speaker_diarization(tmp_path):
    from mvector.predict import MVectorPredictor
    from test_gpu_diarization import write_ecapa_model
    cfg, model_dir = write_ecapa_model(tmp_path)
    wav, turns = turns_recording()
    cpu = MVectorPredictor(cfg, model_path=model_dir, use_gpu=False)
    gpu = MVectorPredictor(cfg, model_path=model_dir, use_gpu=True)
    segs = gpu.vad(wav.copy())
    assert segs == cpu.vad(wav.copy()), (segs, cpu.vad(wav.copy()))
    vc.assert_brackets(segs, [t[:2] for t in turns], gpu.energy_vad)
    print('turns', [t[:2] for t in turns], '-> vad', segs)
    want = cpu.speaker_diarization(wav.copy(), vad_segments=segs)
    got = gpu.speaker_diarization(wav.copy(), vad_segments=gpu.vad(wav.copy()))
    print('speaker_diarization', got)
    assert got == want and len(want) >= 2, (got, want)
    with pytest.raises(NotImplementedError, match='vad_segments'):
        gpu.speaker_diarization(wav.copy())
