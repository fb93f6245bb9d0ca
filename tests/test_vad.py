"""Energy VAD without a GPU: the kernels of csrc/vad.hip on the emulator build against the fp64 oracle of tests/vad_checks.py
(tests/test_gpu_vad.py runs the same checks on the device), and the host layers: the segment smoothing against hand-written cases, EnergyVad
on numpy arrays and CPU tensors, MVectorPredictor.vad on the CPU feeding SpeakerDiarization."""
import os

import numpy as np
import pytest
import torch

import vad_checks as vc
from helpers import load_case


@pytest.fixture(scope='module')
def emu():
    import emu_lib
    return emu_lib.emu_cdll()


def test_emu_log_energy_against_the_fp64_oracle(emu):
    vc.check_log_energy(emu, 'cpu')


@pytest.mark.parametrize('name', vc.RUN_CASES)
def test_emu_decisions_and_runs_equal_the_oracle(emu, name):
    vc.check_case(emu, 'cpu', name)


def test_emu_row_stride_and_unaligned_row_pointer(emu):
    vc.check_layouts(emu, 'cpu')


def test_emu_truncated_run_list_reports_the_true_count(emu):
    vc.check_truncated_runs(emu, 'cpu')


def test_emu_no_hidden_state(emu):
    vc.check_no_hidden_state(emu, 'cpu')


def test_emu_refusals_by_name(emu):
    vc.check_refusals(emu, 'cpu')


def test_the_library_exports_the_vad():
    import ctypes
    import __graft_entry__
    from mvector import _hip
    cdll = ctypes.CDLL(__graft_entry__.build())
    for name in ('mv_vad_energy_workspace_bytes', 'mv_vad_energy_f32'):
        assert hasattr(cdll, name) and name in _hip.EXPORTED_SYMBOLS, name
    header = open(os.path.join(os.path.dirname(os.path.abspath(__graft_entry__.__file__)), 'include', 'mvector_hip.h')).read()
    assert f'#define MV_VAD_TILE_FRAMES {_hip.MV_VAD_TILE_FRAMES}\n' in header
    for name in ('mv_vad_energy_workspace_bytes', 'mv_vad_energy_f32', 'typedef struct MvVadCfg'):
        assert name in header, name
    assert [f for f, _ in _hip.MvVadCfg._fields_ if f != 'reserved'] == list(_hip.VAD_DEFAULTS)
    assert ctypes.sizeof(_hip.MvVadCfg) == 48
    cdll.mv_abi_version.restype = ctypes.c_int
    assert cdll.mv_abi_version() == 5


def test_the_package_audio_segment_has_no_vad_method():
    """speaker_diarization without vad_segments keeps raising: the VAD is a call of its own"""
    from mvector.data_utils.audio import AudioSegment
    assert not hasattr(AudioSegment, 'vad')


# ------------------------------------------------------------------ host layers
def _vad(**kw):
    from mvector.infer_utils.vad import EnergyVad
    return EnergyVad(**kw)


def test_segment_smoothing_against_hand_written_cases():
    vad = _vad()   # 16 kHz: shift 160, min_silence 4800, min_speech 4000, speech_pad 480 samples
    assert (vad.cfg['frame_length'], vad.cfg['frame_shift'], vad.min_silence, vad.min_speech, vad.speech_pad) == (400, 160, 4800, 4000, 480)
    T = 200
    n = 199 * 160 + 400
    smooth = lambda runs, v=vad: v.smooth(np.array(runs).reshape(-1, 2), T, n).tolist()
    # a gap of 29 frames (4640 samples) is joined, one of 30 frames (4800) stays
    assert smooth([[10, 50], [79, 120]]) == [[1600 - 480, 19200 + 480]]
    assert smooth([[10, 50], [80, 120]]) == [[1600 - 480, 8000 + 480], [12800 - 480, 19200 + 480]]
    # 24 frames (3840 samples) are dropped, 25 (4000) stay; the joining comes first: two short runs 10 frames apart are one long region
    assert smooth([[10, 34]]) == [] and smooth([[10, 35]]) == [[1600 - 480, 5600 + 480]]
    assert smooth([[10, 22], [32, 44]]) == [[1600 - 480, 7040 + 480]]
    # the padding stops at 0 and at n; a run that reaches the last frame ends with the recording, not at T * shift
    assert smooth([[1, 40]]) == [[0, 6400 + 480]]
    assert smooth([[150, 199]]) == [[24000 - 480, n]] and 199 * 160 + 480 > n
    assert smooth([[150, 200]]) == [[24000 - 480, n]] and 200 * 160 != n
    assert smooth([]) == [] and smooth([[3, 5]]) == []
    # ... and at the middle of the gap to a neighbour (a gap of 3 frames that a min_silence of 20 ms keeps)
    tight = _vad(min_silence=0.02, min_speech=0.01, speech_pad=0.03)
    assert smooth([[10, 20], [23, 40]], tight) == [[1600 - 480, 3200 + 240], [3680 - 240, 6400 + 480]]
    assert smooth([[10, 20], [22, 40]], tight) == [[1600 - 480, 3200 + 160], [3520 - 160, 6400 + 480]]
    secs = vad.to_seconds(np.array([[1120, 19680]]), n)
    assert secs == [dict(start=0.07, end=1.23)]


def test_segments_pass_the_diarization_checks_for_any_length():
    """an end at the recording's last sample survives the millisecond rounding of SpeakerDiarization._vad_list"""
    from mvector.data_utils.audio import AudioSegment
    from mvector.infer_utils.speaker_diarization import SpeakerDiarization
    vad = _vad()
    for extra in (0, 1, 7, 9, 15, 16, 100, 159):
        n = 6 * 16000 + extra
        x = vc.burst_signal(n, [(10, 99999)], 3)
        segs = vad(x)
        assert len(segs) == 1 and 0 < segs[0]['start'] < 0.1 and segs[0]['end'] <= n / 16000
        assert n / 16000 - segs[0]['end'] < 1e-3
        out = SpeakerDiarization().segments_audio(AudioSegment.from_ndarray(x, 16000), vad_segments=segs)
        assert len(out) >= 6


def test_energy_vad_on_numpy_cpu_tensors_and_batches():
    x, bursts = vc.synthetic_recording()
    for kw in (dict(), dict(energy_threshold=5.5, frames_context=2, proportion_threshold=0.12)):
        vad = _vad(**kw)
        segs = vad(x)
        vc.assert_brackets(segs, bursts, vad)
        assert all(a['end'] <= b['start'] for a, b in zip(segs, segs[1:]))
        assert vad(torch.from_numpy(x)) == segs                       # a CPU tensor runs the numpy path
        dec, log_e, thr = vad.frames(x)
        ref = vc.oracle_row(x, dict(vc.DEFAULT, **{k: v for k, v in vad.cfg.items()}))
        assert ref['margin'] > 1e-6 and np.array_equal(dec, ref['dec']) and isinstance(dec, np.ndarray) and dec.dtype == np.uint8
        assert np.abs(log_e - ref['log_e']).max() <= 4 * 400 * vc.U * np.abs(ref['log_e']).max() and abs(thr - ref['thr']) <= 1e-12
        assert vad.runs_of(dec).tolist() == ref['runs']
        # a batch with the rows' own lengths: every row as if it were alone
        short = x[:7 * 16000 + 33]
        batch = np.zeros((3, x.shape[0]), dtype=np.float32)
        batch[0], batch[1, :short.shape[0]], batch[2, :399] = x, short, x[:399]
        got = vad(batch, lengths=[x.shape[0], short.shape[0], 399])
        assert got == [segs, vad(short), []] and vad(torch.from_numpy(batch), lengths=torch.tensor([x.shape[0], short.shape[0], 399])) == got
        bdec, blog, bthr = vad.frames(batch, lengths=[x.shape[0], short.shape[0], 399])
        assert bdec.shape == blog.shape == (3, dec.shape[0]) and np.array_equal(bdec[0], dec) and not bdec[2].any() and np.isnan(bthr[2])
        assert np.array_equal(bdec[1, :vad.num_frames(short.shape[0])], vad.frames(short)[0]) and not bdec[1, vad.num_frames(short.shape[0]):].any()
    # a NaN sample: no speech at all
    bad = x.copy()
    bad[5000] = np.nan
    assert _vad()(bad) == []
    for kw, fragment in ((dict(frame_length_ms=300), 'frame_length <= 4096'), (dict(frame_shift_ms=30), 'frame_shift <= frame_length'),
                         (dict(frames_context=65), 'frames_context'), (dict(scale=float('inf')), 'non-finite')):
        with pytest.raises(ValueError, match=fragment):
            _vad(**kw)


def test_cpu_predictor_vad_feeds_speaker_diarization(tmp_path):
    from mvector.infer_utils.speaker_diarization import SpeakerDiarization
    from mvector.predict import MVectorPredictor
    man, sd, _, _, _ = load_case('tdnn')
    (tmp_path / 'model').mkdir()
    torch.save({'0.' + k: v for k, v in sd.items()}, str(tmp_path / 'model' / 'model.pth'))
    cfg = dict(dataset_conf=dict(dataset=dict(min_duration=0.3, sample_rate=16000, use_dB_normalization=True, target_dB=-20), eval_conf=dict(batch_size=2)),
               preprocess_conf=dict(feature_method='Fbank', method_args=dict(sample_frequency=16000, num_mel_bins=80)),
               model_conf=dict(model='TDNN', model_args=dict(embd_dim=192)))
    with pytest.MonkeyPatch.context() as mp:
        mp.setenv('CUDA_VISIBLE_DEVICES', os.environ.get('CUDA_VISIBLE_DEVICES', ''))   # (the CPU predictor sets it: restored afterwards)
        p = MVectorPredictor(cfg, model_path=str(tmp_path / 'model'), use_gpu=False)
    x, bursts = vc.synthetic_recording()
    segs = p.vad(x.copy())
    vc.assert_brackets(segs, bursts, p.energy_vad)
    from mvector.infer_utils.vad import EnergyVad
    recipe = EnergyVad(energy_threshold=5.5, frames_context=2, proportion_threshold=0.12)
    vc.assert_brackets(p.vad(x.copy(), vad=recipe), bursts, recipe)
    seg = p._load_audio(x.copy())
    chunks = SpeakerDiarization().segments_audio(seg, vad_segments=segs)   # none of its assertions fires
    assert len(chunks) >= len(bursts) and all(c[2].shape == (24000,) for c in chunks)
    with pytest.raises(NotImplementedError, match='vad_segments'):
        p.speaker_diarization(x.copy())
    with pytest.raises(AssertionError, match='8000 Hz'):
        p.vad(x.copy(), vad=EnergyVad(sample_rate=8000))
