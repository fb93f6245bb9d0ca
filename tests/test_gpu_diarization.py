"""Speaker diarization on the device: the kernel checks of tests/diarization_checks.py on the product library (multi-tile, odd N, the split-K
path, more than one round of workgroups, a second stream), SpectralCluster on a device tensor against the reference's labels, and
MVectorPredictor.speaker_diarization on a synthetic two-speaker recording against the use_gpu=False predictor."""
import numpy as np
import pytest
import torch

import diarization_checks as dc
from helpers import cos_dist, load_case

DEV = 'cuda'
SIZES = [5, 33, 65, 300, 301, 1200]


@pytest.mark.gpu
def test_gpu_wave_chunks():
    dc.check_wave_chunks(None, DEV)


@pytest.mark.gpu
def test_gpu_affinity_tie_rule_and_refusals():
    dc.check_tie_rule(None, DEV)
    dc.check_refusals(None, DEV)


@pytest.mark.gpu
@pytest.mark.parametrize('n', SIZES)
def test_gpu_affinity_and_laplacian_eig_lowest(n):
    """check_eig runs check_affinity first: M bit-equal to the host restatement, degree within 1e-12, then the solver's bars and a second stream"""
    dc.check_eig(None, DEV, n, second_stream=True)


@pytest.mark.gpu
def test_gpu_eig_reports_non_convergence():
    dc.check_not_converged(None, DEV, 65)


@pytest.mark.gpu
@pytest.mark.parametrize('n', dc.GOLDEN_N)
def test_gpu_spectral_cluster_on_a_device_tensor_gives_the_golden_labels(n):
    dc.check_spectral_cluster_golden(None, DEV, n)


# ------------------------------------------------------------------ the predictor
def _voice(tt, sr, f0, formants, gate_rate):
    """harmonics of f0 (a little vibrato) under a formant envelope; gate_rate > 0 cuts it into syllables (60 % on, 12.5 ms ramps)"""
    f = f0 * (1 + 0.02 * np.sin(2 * np.pi * 4.0 * tt))
    phase = 2 * np.pi * np.cumsum(f) / sr
    y = np.zeros_like(tt)
    for h in range(1, int(3800 / (1.02 * f0))):
        amp = 0.02 + sum(g * np.exp(-0.5 * ((h * f - fc) / 180.0) ** 2) for fc, g in formants)
        y += amp * np.sin(h * phase)
    if gate_rate:
        ph = (tt * gate_rate) % 1.0
        y = y * np.clip(np.minimum(ph, 0.6 - ph) / 0.05, 0, 1)
    return y


def two_speaker_recording(seconds=16, sr=16000, seed=21):
    """Two alternating harmonic 'speakers' (f0 about 120 and 220 Hz, different formant envelopes), turns of 3-4 s -> (samples fp32, the turns as
    [(start s, end s, speaker)]).  The front-end's mean normalisation removes a stationary envelope from every chunk and a random network maps what
    is left to nearly parallel embeddings (1 - cos of a few per cent between any two signals), so the second voice also differs in its rhythm: it
    speaks in syllables (4 per second) where the first one holds its tone.  With that the host classes find two speakers on this recording."""
    rng = np.random.default_rng(seed)
    voices = [dict(f0=120.0, formants=((500.0, 1.0), (1500.0, 0.5), (2500.0, 0.25)), gate_rate=0),
              dict(f0=220.0, formants=((850.0, 1.0), (1200.0, 0.7), (3200.0, 0.4)), gate_rate=4)]
    turns, t, who = [], 0.0, 0
    while t < seconds:
        d = min(float(rng.uniform(3.0, 4.0)), seconds - t)
        if seconds - (t + d) < 1.0:
            d = seconds - t
        turns.append((t, t + d, who))
        t, who = t + d, 1 - who
    x = np.zeros(seconds * sr)
    for st, ed, w in turns:
        n0, n1 = int(round(st * sr)), int(round(ed * sr))
        x[n0:n1] = _voice(np.arange(n1 - n0) / sr, sr, **voices[w])
    x += 0.003 * rng.standard_normal(x.shape[0])
    return (0.3 * x / np.abs(x).max()).astype(np.float32), turns


def write_ecapa_model(tmp_path):
    """a tiny EcapaTdnn with torch's seeded default initialisation, saved as the predictor loads it (the fixture weights of ecapa_tiny carry random
    BatchNorm statistics and biases: their embeddings of ANY two signals stay above the 0.78 at which similar speakers are merged)"""
    from mvector.models import EcapaTdnn
    man, _, _, _, _ = load_case('ecapa_tiny')
    args = {k: v for k, v in man['kwargs'].items() if k != 'input_size'}
    torch.manual_seed(5)
    model = EcapaTdnn(input_size=80, **args).eval()
    model_dir = tmp_path / 'model'
    model_dir.mkdir()
    torch.save({'0.' + k: v for k, v in model.state_dict().items()}, str(model_dir / 'model.pth'))
    cfg = dict(dataset_conf=dict(dataset=dict(min_duration=0.3, sample_rate=16000, use_dB_normalization=True, target_dB=-20), eval_conf=dict(batch_size=4)),
               preprocess_conf=dict(feature_method='Fbank', method_args=dict(sample_frequency=16000, num_mel_bins=80)),
               model_conf=dict(model='EcapaTdnn', model_args=args))
    return cfg, str(model_dir)


@pytest.mark.gpu
def test_gpu_predictor_speaker_diarization(tmp_path):
    from mvector.predict import MVectorPredictor
    cfg, model_dir = write_ecapa_model(tmp_path)
    wav, turns = two_speaker_recording()
    vad = [dict(start=0.0, end=16.0)]
    cpu = MVectorPredictor(cfg, model_path=model_dir, use_gpu=False)
    want = cpu.speaker_diarization(wav.copy(), vad_segments=vad)
    assert sorted({t['speaker'] for t in want}) == [0, 1], want       # the host classes find the two speakers on this recording
    # ... in the order they speak; a turn starts within one chunk length (1.5 s) of the true change, the resolution of chunk labels
    assert len(want) == len(turns) and all(abs(t['start'] - u[0]) <= 1.5 and t['speaker'] == u[2] for t, u in zip(want, turns)), (want, turns)

    db = tmp_path / 'audio_db'
    # threshold 0.9: an enrolled speaker's own centre scores about 1 against the enrolment, another speaker's below the 0.78 that keeps two speakers apart
    gpu = MVectorPredictor(cfg, threshold=0.9, audio_db_path=str(db), model_path=model_dir, use_gpu=True)
    with pytest.raises(NotImplementedError, match='vad_segments'):
        gpu.speaker_diarization(wav.copy())
    # the chunk embeddings: wave_chunks + device front-end / backbone against predict_batch on the same host chunks
    seg = gpu._load_audio(wav.copy())
    sd = gpu.speaker_diarize
    segments = sd.segments_audio(seg, vad_segments=vad)
    times, starts, lens, chunk_len = sd.chunk_table(seg, vad_segments=vad)
    assert [t[:2] for t in times] == [s[:2] for s in segments] and chunk_len == 24000
    emb_dev = gpu._embed_chunks_device(seg.samples, starts, lens, chunk_len)
    assert emb_dev.is_cuda and emb_dev.shape == (len(segments), 192)
    emb_host = cpu.predict_batch([s[2] for s in segments])
    d = cos_dist(emb_dev.cpu(), emb_host).max().item()
    print(f'speaker_diarization: {len(segments)} chunks, wave_chunks path vs predict_batch 1 - cos {d:.2e}')
    assert d <= 1e-4, d

    got = gpu.speaker_diarization(wav.copy(), vad_segments=vad)
    assert got == want, (got, want)
    assert gpu.speaker_diarization(wav.copy(), speaker_num=2, vad_segments=vad) == want
    # one of the two speakers enrolled: that speaker's turns carry the name, the other one stays a stranger
    first = turns[0]
    assert gpu.register(wav[int(first[0] * 16000):int(first[1] * 16000)].copy(), 'alice')[0]
    named = gpu.speaker_diarization(wav.copy(), search_audio_db=True, vad_segments=vad)
    assert [(t['start'], t['end']) for t in named] == [(t['start'], t['end']) for t in want]
    for t, w in zip(named, want):
        assert t['speaker'] == ('alice' if w['speaker'] == first[2] else f"陌生人{w['speaker']}"), named
