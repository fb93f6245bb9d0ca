"""The HuggingFace (Wav2Vec2 / WavLM) front-end on the MI355X: device against the fp64 arbiter of tests/hf_ref.py under the bars of
tests/hf_cases.py (twice the rounding model's own distance), the refusal of a waveform below the receptive field, bit-identity across batch sizes
and streams, CUDA in -> CUDA out through AudioFeaturizer, and end-to-end embeddings."""
import functools
import json
import os

import pytest
import torch

import hf_cases as hc
import hf_ref
from helpers import cos_dist
from oracle import frontend, models as omodels, weights

pytestmark = pytest.mark.gpu
DEV = torch.device('cuda:0')


@functools.lru_cache(maxsize=None)
def _handle(norm, cmn=True):
    from mvector import _hip
    cfg, sd = hc.seeded_model(norm)
    return _hip.HfEncoder(cfg, {k: v.to(DEV) for k, v in sd.items()}, subtract_time_mean=cmn)


def _check(name, got, ref, f32):
    assert got.shape == ref.shape and bool(torch.isfinite(got).all())
    mx, mean = hc.distances(got, ref)
    bmx, bmean = hc.bars(name)
    print(f'{name}: device max-abs {mx:.3e} (bar {bmx:.3e}) mean-abs {mean:.3e} (bar {bmean:.3e}); fp32 restatement max-abs {f32[0]:.1e} '
          f'mean-abs {f32[1]:.1e}')
    assert mx <= bmx and mean <= bmean


@pytest.mark.parametrize('name', ['w512_group_L16000', 'w512_layer_L16000', 'w512_group_L20635', 'w512_layer_L20635', 'w512_group_L400',
                                  'w512_layer_L400', 'w512_group_B130'])
def test_gpu_width_512_meets_the_fp64_arbiter(name):
    cfg, sd, wav, ratio = hc.build(name)
    h = _handle(cfg['feat_extract_norm'], name not in hc.NO_CMN)
    got = h(wav.to(DEV), None if ratio is None else ratio.to(DEV))
    ref = hc.reference(name, cfg, sd, wav, ratio)
    _check(name, got, ref, hc.distances(hc.reference(name, cfg, sd, wav, ratio, torch.float32), ref))
    assert got.shape[1] == hc.frames_of(wav.shape[1])[-1]
    if ratio is not None:
        T = got.shape[1]
        for b, r in enumerate(ratio):
            n = int(torch.round(r * T))
            if n < T:
                assert got[b, n:].abs().max().item() == 0.0


@pytest.mark.parametrize('name', ['fix_wav2vec2_group', 'fix_wav2vec2_layer', 'fix_wavlm_group', 'fix_wavlm_layer'])
def test_gpu_tiny_fixtures_meet_the_fp64_arbiter(name):
    from mvector import _hip
    cfg, sd, wav, ratio = hc.build(name)
    got = _hip.HfEncoder(cfg, {k: v.to(DEV) for k, v in sd.items()})(wav.to(DEV), None if ratio is None else ratio.to(DEV))
    ref = hc.reference(name, cfg, sd, wav, ratio)
    _check(name, got, ref, hc.distances(hc.reference(name, cfg, sd, wav, ratio, torch.float32), ref))


def test_gpu_waveform_below_the_receptive_field_is_refused():
    h = _handle('group')
    with pytest.raises(RuntimeError, match='399 samples is shorter than the encoder.s receptive field of 400'):
        h(torch.zeros(3, 399, device=DEV))
    assert h(frontend.synth_waveforms(3, 400, seed=1).to(DEV)).shape == (3, 1, 512)


@pytest.mark.parametrize('norm', ['group', 'layer'])
def test_gpu_row_bits_do_not_depend_on_batch_or_stream(norm):
    h = _handle(norm)
    wav = frontend.synth_waveforms(130, 4000, seed=3).to(DEV)
    whole = h(wav)
    for B in (1, 8):
        assert torch.equal(h(wav[:B]), whole[:B]), B
    assert torch.equal(h(wav[129:]), whole[129:])
    torch.cuda.synchronize()
    streams = [torch.cuda.Stream(DEV), torch.cuda.Stream(DEV)]
    outs = []
    for s, rows in zip(streams, (slice(0, 8), slice(8, 16))):
        with torch.cuda.stream(s):
            outs.append(h(wav[rows]))
    torch.cuda.synchronize()
    assert torch.equal(outs[0], whole[0:8]) and torch.equal(outs[1], whole[8:16])


def test_gpu_audio_featurizer_keeps_cuda_tensors_on_the_device(tmp_path):
    pytest.importorskip('transformers')
    import sys
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'tools'))
    import make_hf_golden as mk
    from mvector.data_utils.featurizer import AudioFeaturizer
    mk.save_model(str(tmp_path), 'wav2vec2', 'group', False, True, seed=4)
    fz = AudioFeaturizer(feature_method=str(tmp_path), use_hf_model=True)
    wav = frontend.synth_waveforms(3, 8000, seed=9)
    ratio = torch.tensor(hc.RATIO3)
    got = fz(wav.to(DEV), ratio.to(DEV))
    assert got.is_cuda and got.shape == (3, 24, 64) and fz.feature_dim == 64
    cpu = fz(wav, ratio)   # the HF modules in torch fp32
    d = (got.cpu() - cpu).abs()
    print(f'AudioFeaturizer CUDA vs CPU: max-abs {d.max().item():.3e} mean-abs {d.mean().item():.3e}')
    bmx = 2 * max(v[0] for k, v in hc.MODEL_DISTANCE.items() if k.startswith('fix_'))   # (the loosest bar of the 64-wide fixtures of this geometry)
    assert d.max().item() <= bmx
    vl = fz.forward_varlen(wav.to(DEV), torch.tensor([8000, 8000, 5000]))
    assert vl.is_cuda and torch.equal(vl[0], fz(wav[:1].to(DEV))[0])
    t2 = hf_ref.num_frames(hc.BASE, 5000)
    assert torch.equal(vl[2, :t2], fz(wav[2:3, :5000].to(DEV))[0]) and vl[2, t2:].abs().max().item() == 0.0


@pytest.mark.parametrize('norm', ['group', 'layer'])
def test_gpu_end_to_end_embeddings(norm):
    """an EcapaTdnn of input_size 512 fed by the device features against the oracle model fed by the fp64-restated features: the project's
    1 - cos <= 1e-4"""
    from mvector.models import EcapaTdnn
    with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'manifest_ecapa_tiny.json')) as f:
        man = json.load(f)
    kwargs = dict(man['kwargs'], input_size=512)
    model = EcapaTdnn(**kwargs)
    sd = weights.make_state_dict(weights.shapes_of(model.state_dict()), man['seed'])
    model.load_state_dict(sd)
    model.eval().to(DEV)
    cfg, hsd, wav, ratio = hc.build(f'w512_{norm}_L16000')
    feats = _handle(norm)(wav.to(DEV), ratio.to(DEV))
    feats_ref = hf_ref.featurize(hsd, cfg, wav, ratio, torch.float64).float()
    with torch.no_grad():
        emb = model(feats)
    emb_ref = omodels.ecapa_tdnn(sd, feats_ref)
    d = cos_dist(emb.cpu(), emb_ref)
    print(f'end to end ({norm}): 1 - cos = {d}')
    assert float(torch.as_tensor(d).max()) <= 1e-4
