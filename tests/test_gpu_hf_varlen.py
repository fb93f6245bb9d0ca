"""Variable-length batches of the HuggingFace (Wav2Vec2 / WavLM) front-end on the MI355X (mv_hfenc_forward_varlen), width 512, both norms: every
row bit for bit what the fixed-length forward gives for it alone and zero behind its own frames (a NaN tail included), many rows, two streams on
one handle, the fp64 arbiter, AudioFeaturizer.forward_varlen as one native call, and end-to-end embeddings.  Cases and checks:
tests/hf_varlen_cases.py."""
import functools
import json
import os

import pytest
import torch

import hf_cases as hc
import hf_ref
import hf_varlen_cases as vc
from helpers import cos_dist
from oracle import frontend, models as omodels, weights

pytestmark = pytest.mark.gpu
DEV = torch.device('cuda:0')
NORMS = ['group', 'layer']


@functools.lru_cache(maxsize=None)
def _handle(norm, cmn=True):
    from mvector import _hip
    cfg, sd = hc.seeded_model(norm)
    return _hip.HfEncoder(cfg, {k: v.to(DEV) for k, v in sd.items()}, subtract_time_mean=cmn)


@functools.lru_cache(maxsize=None)
def _first(norm, cmn=True):
    """(cfg, sd, wav on the host, wav on the device, the variable-length output): computed once, shared, never written to"""
    cfg, sd, wav = vc.gpu_batch(norm)
    dwav = wav.to(DEV)
    return cfg, sd, wav, dwav, _handle(norm, cmn)(dwav, None, torch.tensor(vc.GPU_LENS, device=DEV))


@functools.lru_cache(maxsize=None)
def _many(norm):
    wav, lens = vc.many_batch()
    dwav = wav.to(DEV)
    return dwav, lens, _handle(norm)(dwav, None, torch.tensor(lens, device=DEV))


@pytest.mark.parametrize('cmn', [True, False], ids=['cmn', 'no_cmn'])
@pytest.mark.parametrize('norm', NORMS)
def test_gpu_row_bits_are_those_of_the_row_alone(norm, cmn):
    """L = 4000, n = [4000, 400, 399, 0, 2565, 2570, 404, 405]; without the time mean as well (one frame minus its own mean is zero)"""
    _, _, _, dwav, out = _first(norm, cmn)
    h = _handle(norm, cmn)
    vc.check_rows(h, dwav, vc.GPU_LENS, out=out)
    assert bool(torch.isfinite(out).all())
    for b, n in enumerate(vc.GPU_LENS):
        if n >= 400 and not (cmn and h.num_frames(n) == 1):
            assert out[b].abs().max().item() > 0.0, b
    # the tail is never read into a result
    n = torch.tensor(vc.GPU_LENS, device=DEV)
    for value in (float('nan'), 1e4):
        assert torch.equal(h(vc.with_tail(dwav, vc.GPU_LENS, value), None, n), out), value


@pytest.mark.parametrize('norm', NORMS)
def test_gpu_many_rows(norm):
    """B = 130 at L = 4000, seeded uniform lengths in [0, 4000]: several 256-row conv tiles in every layer"""
    dwav, lens, out = _many(norm)
    rows = vc.many_rows(lens)
    short = [b for b, n in enumerate(lens) if n < 400]
    assert len(rows) >= 10 and len(short) >= 3 and min(lens) < 400 and max(lens) > 3600
    vc.check_rows(_handle(norm), dwav, lens, rows=rows + short, out=out)
    assert bool(torch.isfinite(out).all())


@pytest.mark.parametrize('norm', NORMS)
def test_gpu_two_streams_one_handle(norm):
    dwav, lens, whole = _many(norm)
    h = _handle(norm)
    n = torch.tensor(lens, device=DEV)
    torch.cuda.synchronize()
    streams = [torch.cuda.Stream(DEV), torch.cuda.Stream(DEV)]
    outs = []
    for s, rows in zip(streams, (slice(0, 8), slice(8, 16))):
        with torch.cuda.stream(s):
            outs.append(h(dwav[rows], None, n[rows]))
    torch.cuda.synchronize()
    assert torch.equal(outs[0], whole[0:8]) and torch.equal(outs[1], whole[8:16])
    assert torch.equal(h(dwav[129:], None, n[129:]), whole[129:])      # B = 1


@pytest.mark.parametrize('b', vc.GPU_ARBITER_ROWS)
@pytest.mark.parametrize('norm', NORMS)
def test_gpu_rows_meet_the_fp64_arbiter(norm, b):
    cfg, sd, wav, _, out = _first(norm)
    vc.check_arbiter(f'w512_{norm}_L4000_row{b}', out[b], cfg, sd, wav, vc.GPU_LENS, b)


class _Counting:
    """stands in for a native handle: counts the forwards that go through it"""

    def __init__(self, handle):
        self.handle, self.calls = handle, 0

    def __call__(self, *args, **kwargs):
        self.calls += 1
        return self.handle(*args, **kwargs)

    def __getattr__(self, name):
        return getattr(self.handle, name)


def test_gpu_featurizer_forward_varlen_is_one_native_call(tmp_path):
    pytest.importorskip('transformers')
    import sys
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'tools'))
    import make_hf_golden as mk
    from mvector.data_utils.featurizer import AudioFeaturizer
    mk.save_model(str(tmp_path), 'wav2vec2', 'group', False, True, seed=4)
    fz = AudioFeaturizer(feature_method=str(tmp_path), use_hf_model=True)
    lens = [8000, 399, 5000, 0, 400]
    padded = frontend.synth_waveforms(len(lens), 8000, seed=9).to(DEV)
    n = torch.tensor(lens, device=DEV)
    h = fz._handle(DEV)
    key = next(iter(fz._native))
    fz._native[key] = counter = _Counting(h)
    out = fz.forward_varlen(padded, n)
    assert counter.calls == 1
    assert out.is_cuda and torch.equal(out, h(padded, None, n))
    vc.check_rows(h, padded, lens, out=out)     # what the per-row loop gave: every row featurised alone, short rows all zero


@pytest.mark.parametrize('norm', NORMS)
def test_gpu_end_to_end_embeddings(norm):
    """the tiny EcapaTdnn at input_size 512 on the forward_varlen features of three rows of different lengths, every row cut to its own frames,
    against the oracle model on the fp64 features of that row alone: the project's 1 - cos <= 1e-4"""
    from mvector.models import EcapaTdnn
    with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'manifest_ecapa_tiny.json')) as f:
        man = json.load(f)
    model = EcapaTdnn(**dict(man['kwargs'], input_size=512))
    sd = weights.make_state_dict(weights.shapes_of(model.state_dict()), man['seed'])
    model.load_state_dict(sd)
    model.eval().to(DEV)
    cfg, hsd = hc.seeded_model(norm)
    lens = [16000, 12345, 9000]
    wav = frontend.synth_waveforms(3, 16000, seed=11).float()
    feats = _handle(norm)(vc.with_tail(wav, lens, float('nan')).to(DEV), None, torch.tensor(lens, device=DEV))
    for b, n in enumerate(lens):
        ref = hf_ref.featurize(hsd, cfg, wav[b:b + 1, :n], None, torch.float64).float()
        with torch.no_grad():
            emb = model(feats[b:b + 1, :ref.shape[1]].contiguous())
        d = float(torch.as_tensor(cos_dist(emb.cpu(), omodels.ecapa_tdnn(sd, ref))).max())
        print(f'end to end ({norm}), row {b} (n = {n}, {ref.shape[1]} frames): 1 - cos = {d:.3e}')
        assert d <= 1e-4
