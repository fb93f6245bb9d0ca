"""The Wav2Vec2-BERT (w2v-bert-2.0) front-end on the MI355X: device against the fp64 arbiter of tests/w2vbert_ref.py under the bars of
tests/w2vbert_cases.py (twice the fp32 restatement's own distance), the two kernels alone, bit-identity across batch sizes and streams, the
variable-length form row by row, CUDA in -> CUDA out through AudioFeaturizer, and end-to-end embeddings."""
import functools
import json
import os
import sys

import numpy as np
import pytest
import torch

import w2vbert_cases as wc
import w2vbert_ref as ref
from helpers import cos_dist
from oracle import models as omodels, weights

pytestmark = pytest.mark.gpu
DEV = torch.device('cuda:0')


@functools.lru_cache(maxsize=None)
def _handle(cmn=True):
    return wc.handle(None, cmn, DEV)


@pytest.mark.parametrize('name', list(wc.CASES))
def test_gpu_case_meets_the_fp64_arbiter(name):
    got, r64 = wc.run(name, None, DEV)
    assert got.is_cuda
    print(wc.check_case(name, got, r64))


@functools.lru_cache(maxsize=None)
def _varlen():
    wav = wc.varlen_input().to(DEV)
    return wav, wc.forward_prefilled(_handle(), wav, None, wc.VARLEN_LENS)


def test_gpu_varlen_meets_the_fp64_arbiter():
    got = _varlen()[1]
    mx, mean = wc.distances(got, wc.varlen_reference())
    bmx, bmean = wc.bars('varlen')
    print(f'varlen: device max-abs {mx:.3e} (bar {bmx:.3e}) mean-abs {mean:.3e} (bar {bmean:.3e})')
    assert bool(torch.isfinite(got).all()) and mx <= bmx and mean <= bmean


def test_gpu_varlen_rows_equal_their_single_row_forward():
    wav, got = _varlen()
    h = _handle()
    for b, n in enumerate(wc.VARLEN_LENS):
        if n < ref.MIN_SAMPLES:
            assert got[b].abs().max().item() == 0.0
            continue
        alone = h(wav[b:b + 1, :n].contiguous())
        t2 = alone.shape[1]
        assert t2 == ref.num_stacked(n) and torch.equal(got[b, :t2], alone[0]) and (t2 == got.shape[1] or got[b, t2:].abs().max().item() == 0.0)


def test_gpu_row_bits_do_not_depend_on_batch_or_stream():
    h = _handle()
    wav = wc.build('L4000_B130')[2].to(DEV)
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


# ---- the two kernels alone ----

@functools.lru_cache(maxsize=None)
def _stage():
    mel = wc.stage_input()
    return mel, wc.stage_stats_f64(mel), wc.stage_stats_f64(mel, wc.STAGE_LENS)


def _ulps(got, want64):
    return np.abs(got.astype(np.float64) - want64) / np.spacing(np.abs(want64.astype(np.float32))).astype(np.float64)


@pytest.mark.parametrize('varlen', [False, True])
def test_gpu_binstats_within_one_ulp_of_fp64(varlen):
    from mvector import _hip
    mel, full, own = _stage()
    mean64, var64 = own if varlen else full
    mean, var = _hip.w2vbert_binstats(mel.to(DEV), wc.STAGE_LENS if varlen else None, wc.STAGE_L if varlen else None)
    live = [b for b in range(3) if not (varlen and wc.STAGE_LENS[b] < ref.MIN_SAMPLES)]
    um, uv = _ulps(mean.cpu().numpy()[live], mean64[live]).max(), _ulps(var.cpu().numpy()[live], var64[live]).max()
    print(f'binstats varlen={varlen}: device mean {um:.2f} ulp, var {uv:.2f} ulp')
    assert um <= 1.0 and uv <= 1.0
    if varlen:
        assert mean[2].abs().max().item() == 0 and var[2].abs().max().item() == 0


@pytest.mark.parametrize('varlen', [False, True])
def test_gpu_rows_meet_the_fp64_stage(varlen):
    from mvector import _hip
    mel, full, own = _stage()
    lens = wc.STAGE_LENS if varlen else None
    mean, var = (torch.from_numpy(a).float() for a in (own if varlen else full))
    ln_w, ln_b = wc.layer_norm_tensors()
    out = torch.full((3, 99, 160), float('nan'), device=DEV)
    got = _hip.w2vbert_rows(mel.to(DEV), mean.to(DEV), var.to(DEV), ln_w.to(DEV), ln_b.to(DEV), 1e-5, lens, wc.STAGE_L if varlen else None, out=out)
    mx, mn = wc.distances(got, wc.stage_rows(mel, mean, var, torch.float64, lens))
    bmx, bmn = wc.stage_bars('rows_varlen' if varlen else 'rows')
    print(f'rows varlen={varlen}: device max-abs {mx:.3e} (bar {bmx:.3e}) mean-abs {mn:.3e} (bar {bmn:.3e})')
    assert bool(torch.isfinite(got).all()) and mx <= bmx and mn <= bmn
    if varlen:
        assert got[1, 50:].abs().max().item() == 0 and got[2].abs().max().item() == 0


# ---- the Python surface and the model behind it ----

def test_gpu_audio_featurizer_keeps_cuda_tensors_on_the_device(tmp_path):
    pytest.importorskip('transformers')
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'tools'))
    import make_w2vbert_golden as mk
    from mvector.data_utils.featurizer import AudioFeaturizer
    mk.save_model(str(tmp_path), seed=4)
    fz = AudioFeaturizer(feature_method=str(tmp_path), use_hf_model=True)
    wav = wc.build('L8000_B3')[2]
    ratio = torch.tensor([1.0, 0.5, 0.8])
    got = fz(wav.to(DEV), ratio.to(DEV))
    assert got.is_cuda and got.shape == (3, 24, 160) and fz.feature_dim == 160
    cpu = fz(wav, ratio)   # the HF processor in numpy + the LayerNorm in torch fp32
    d = (got.cpu() - cpu).abs()
    bmx = 2 * max(v[0] for v in wc.MODEL_DISTANCE.values())   # the loosest case bar
    print(f'AudioFeaturizer CUDA vs CPU: max-abs {d.max().item():.3e} mean-abs {d.mean().item():.3e} (bar {bmx:.3e})')
    assert d.max().item() <= bmx
    vl = fz.forward_varlen(wav.to(DEV), torch.tensor([8000, 559, 5000]))
    assert vl.is_cuda and torch.equal(vl[0], fz(wav[:1].to(DEV))[0]) and vl[1].abs().max().item() == 0.0
    t2 = ref.num_stacked(5000)
    assert torch.equal(vl[2, :t2], fz(wav[2:3, :5000].to(DEV))[0]) and vl[2, t2:].abs().max().item() == 0.0


def test_gpu_end_to_end_embeddings():
    """an EcapaTdnn of input_size 160 fed by the device features against the oracle model fed by the fp64-restated features: the project's
    1 - cos <= 1e-4"""
    from mvector.models import EcapaTdnn
    with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'manifest_ecapa_tiny.json')) as f:
        man = json.load(f)
    model = EcapaTdnn(**dict(man['kwargs'], input_size=160))
    sd = weights.make_state_dict(weights.shapes_of(model.state_dict()), man['seed'])
    model.load_state_dict(sd)
    model.eval().to(DEV)
    ln_w, ln_b, wav, ratio, cmn = wc.build('L16160_B2')
    feats = _handle()(wav.to(DEV))
    feats_ref = ref.featurize(ln_w, ln_b, wc.CFG, wav, None, torch.float64).float()
    with torch.no_grad():
        emb = model(feats)
    emb_ref = omodels.ecapa_tdnn(sd, feats_ref)
    d = cos_dist(emb.cpu(), emb_ref)
    print(f'end to end: 1 - cos = {d}')
    assert float(torch.as_tensor(d).max()) <= 1e-4
