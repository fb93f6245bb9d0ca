"""The HuggingFace (Wav2Vec2 / WavLM) front-end, AudioFeaturizer(use_hf_model=True), on the CPU and on the emulator build of
csrc/hfencoder.hip: the restatement tests/hf_ref.py against the fixtures of the HF code (tools/make_hf_golden.py), the native handle
against the restatement's fp64 arbiter under the bars of tests/hf_cases.py, the refusals, and the Python surface."""
import ctypes
import pickle

import pytest
import torch

import hf_cases as hc
import hf_ref
from emu_lib import emu_cdll
from mvector import _hip
from mvector.data_utils.featurizer import AudioFeaturizer


# ---- the restatement against the HF code's own output ----

@pytest.mark.parametrize('name', hc.FIXTURES)
def test_restatement_meets_the_hf_fixture(name):
    """fp32 restatement vs the HF model's extract_features, to fp32 rounding.  Bound: the features are O(1) behind a LayerNorm; each of the 7
    layers is a dot product of K <= 192 terms (<= sqrt(K) < 16 units of fp32 rounding as a random walk) followed by a normalisation that keeps the
    scale -- 7 * 16 * 2^-24 * max|features|, ~4e-5 at |features| ~ 6.  The fp64 arbiter must sit inside the same bound."""
    cfg, sd, wav, gold = hc.load_fixture(name)
    assert gold.shape == (3, hf_ref.num_frames(cfg, 8000), 64) and wav[2, 5000:].abs().max() == 0
    bound = 7 * 16 * 2.0 ** -24 * gold.abs().max().item()
    f32 = hf_ref.extract_features(sd, cfg, wav, torch.float32)
    f64 = hf_ref.extract_features(sd, cfg, wav, torch.float64)
    d32, d64 = (f32 - gold).abs().max().item(), (f64 - gold.double()).abs().max().item()
    print(f'{name}: fp32 restatement - HF {d32:.2e}, fp64 arbiter - HF {d64:.2e}, bound {bound:.2e}')
    assert d32 <= bound and d64 <= bound


def test_fixtures_cover_both_modes_biases_and_processors():
    seen = set()
    for name in hc.FIXTURES:
        cfg = hc.load_fixture(name)[0]
        assert cfg['conv_dim'] == [64] * 7 and cfg['model_type'] in ('wav2vec2', 'wavlm')
        seen.add((cfg['feat_extract_norm'], cfg['conv_bias'], cfg['do_normalize']))
    assert {s[0] for s in seen} == {'group', 'layer'} and {s[1] for s in seen} == {False, True} and {s[2] for s in seen} == {False, True}


# ---- the native handle on the emulator ----

def _run(name, cdll):
    cfg, sd, wav, ratio = hc.build(name)
    h = _hip.HfEncoder(cfg, sd, subtract_time_mean=name not in hc.NO_CMN, cdll=cdll)
    got = h(wav, ratio)
    ref = hc.reference(name, cfg, sd, wav, ratio)
    return got, ref, hc.distances(hc.reference(name, cfg, sd, wav, ratio, torch.float32), ref)


@pytest.mark.parametrize('name', ['fix_wav2vec2_group', 'fix_wav2vec2_layer', 'fix_wavlm_group', 'fix_wavlm_layer', 'w512_group_L800',
                                  'w512_layer_L800'])
def test_emulated_handle_meets_the_fp64_arbiter(name):
    got, ref, f32 = _run(name, emu_cdll())
    assert got.shape == ref.shape and torch.isfinite(got).all()
    mx, mean = hc.distances(got, ref)
    bmx, bmean = hc.bars(name)
    print(f'{name}: handle max-abs {mx:.3e} (bar {bmx:.3e}) mean-abs {mean:.3e} (bar {bmean:.3e}); fp32 restatement max-abs {f32[0]:.1e}')
    assert mx <= bmx and mean <= bmean
    ratio = hc.CASES[name][3]
    if ratio is not None:   # zero behind round(ratio * T'), exactly
        T = got.shape[1]
        for b, r in enumerate(ratio):
            n = int(torch.round(torch.tensor(r, dtype=torch.float32) * T))
            assert got[b, n:].abs().max().item() == 0.0 if n < T else True
            assert got[b, :n].abs().max().item() > 0.0


def test_emulated_row_bits_do_not_depend_on_the_batch():
    cfg, sd, wav, _ = hc.build('fix_wav2vec2_group')
    h = _hip.HfEncoder(cfg, sd, cdll=emu_cdll())
    wav = wav[:, :2400].contiguous()
    whole = h(wav)
    for b in range(3):
        assert torch.equal(h(wav[b:b + 1])[0], whole[b])
    ms = []   # the timed form is the same launch sequence: same bits, one figure per layer and one for the tail
    assert torch.equal(h(wav, stage_ms=ms), whole) and len(ms) == 8


def test_num_frames_and_workspace():
    cfg, sd = hc.seeded_model('group', width=64)
    h = _hip.HfEncoder(cfg, sd, cdll=emu_cdll())
    for L in (399, 400, 404, 405, 16000, 20635):
        assert h.num_frames(L) == hf_ref.num_frames(cfg, L)
    need = ctypes.c_size_t()
    _hip.check(h._cdll.mv_hfenc_workspace_bytes(h._h, 2, 800, ctypes.byref(need)), h._cdll)
    assert need.value >= 2 * 159 * 64 * 2 + 2 * 79 * 64 * 2


def test_refusals_name_what_is_wrong():
    cdll = emu_cdll()
    cfg, sd = hc.seeded_model('group', width=64)
    with pytest.raises(NotImplementedError, match="feat_extract_activation 'relu'"):
        _hip.HfEncoder(dict(cfg, feat_extract_activation='relu'), sd, cdll=cdll)
    with pytest.raises(RuntimeError, match=r'conv_dim\[3\] = 96.*multiples of 64'):
        _hip.HfEncoder(dict(cfg, conv_dim=[64, 64, 64, 96, 64, 64, 64]), sd, cdll=cdll)
    with pytest.raises(RuntimeError, match=r'conv_dim\[0\] = 2048'):
        _hip.HfEncoder(dict(cfg, conv_dim=[2048] + [64] * 6), sd, cdll=cdll)
    missing = {k: v for k, v in sd.items() if k != 'feature_extractor.conv_layers.4.conv.weight'}
    with pytest.raises(RuntimeError, match="missing 'feature_extractor.conv_layers.4.conv.weight'"):
        _hip.HfEncoder(cfg, missing, cdll=cdll)
    with pytest.raises(RuntimeError, match="missing 'feature_extractor.conv_layers.0.conv.bias'"):
        _hip.HfEncoder(dict(cfg, conv_bias=True), {k: v for k, v in sd.items()}, cdll=cdll)
    bad = dict(sd)
    bad['feature_projection.layer_norm.weight'] = torch.ones(65)
    with pytest.raises(RuntimeError, match="'feature_projection.layer_norm.weight' has 65 elements, expected 64"):
        _hip.HfEncoder(cfg, bad, cdll=cdll)
    with pytest.raises(RuntimeError, match="missing 'feature_extractor.conv_layers.1.layer_norm.weight'"):
        _hip.HfEncoder(dict(cfg, feat_extract_norm='layer'), sd, cdll=cdll)
    # a raw config with another activation code
    c = _hip.MvHfEncoderCfg()
    cdll.mv_hfenc_default_cfg(ctypes.byref(c))
    assert c.num_layers == 7 and list(c.conv_kernel)[:7] == [10, 3, 3, 3, 3, 2, 2] and c.activation == _hip.MV_ACT_GELU
    c.activation = _hip.MV_ACT_RELU
    refs, keep, _ = _hip._tensor_refs(sd)
    out = ctypes.c_void_p()
    assert cdll.mv_hfenc_create(ctypes.byref(c), refs, len(keep), ctypes.byref(out)) == -3
    assert b'gelu' in cdll.mv_last_error()
    # shorter than the receptive field: no frame (the reference's Conv1d raises there)
    h = _hip.HfEncoder(cfg, sd, cdll=cdll)
    with pytest.raises(RuntimeError, match='399 samples is shorter than the encoder.s receptive field of 400'):
        h(torch.zeros(2, 399))
    assert h(torch.randn(2, 400)).shape == (2, 1, 64)


def test_exports_present():
    names = ['mv_hfenc_default_cfg', 'mv_hfenc_create', 'mv_hfenc_destroy', 'mv_hfenc_num_frames', 'mv_hfenc_workspace_bytes', 'mv_hfenc_forward',
             'mv_hfenc_forward_timed']
    cdll = emu_cdll()
    for n in names:
        assert n in _hip.EXPORTED_SYMBOLS and hasattr(cdll, n)
    assert cdll.mv_abi_version() == 5


# ---- the Python surface (needs `transformers` to build a model folder from a fixture) ----

@pytest.fixture(scope='module')
def hf_folders(tmp_path_factory):
    transformers = pytest.importorskip('transformers')
    import os
    import sys
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'tools'))
    import make_hf_golden as mk
    out = {}
    for name in ('hf_wav2vec2_group', 'hf_wavlm_layer'):
        model_type, norm, conv_bias, do_normalize = mk.FIXTURES[name]
        folder = str(tmp_path_factory.mktemp(name))
        mk.save_model(folder, model_type, norm, conv_bias, do_normalize, seed=0)
        model = transformers.AutoModel.from_pretrained(folder)   # the fixture's front-end weights into the folder's model
        _, sd, _, _ = hc.load_fixture(name)
        res = model.load_state_dict(sd, strict=False)
        assert not res.unexpected_keys
        model.save_pretrained(folder)
        out[name] = folder
    return out


@pytest.mark.parametrize('name', ['hf_wav2vec2_group', 'hf_wavlm_layer'])
def test_audio_featurizer_on_a_model_folder(hf_folders, name):
    cfg, sd, wav, gold = hc.load_fixture(name)
    fz = AudioFeaturizer(feature_method=hf_folders[name], use_hf_model=True, method_args={'use_gpu': False})
    assert fz.feature_dim == 64 and fz.use_hf_model
    ratio = torch.tensor(hc.RATIO3)
    got = fz(wav, ratio)
    ref = hf_ref.wrapper(gold, ratio)   # the HF model's own output under the reference's wrapper
    bound = 2 * 7 * 16 * 2.0 ** -24 * gold.abs().max().item()   # (the bound of test_restatement_meets_the_hf_fixture, once more for the mean)
    assert got.shape == ref.shape and (got - ref).abs().max().item() <= bound
    T = got.shape[1]
    assert got[1, round(0.61 * T):].abs().max() == 0 and got[2, round(0.35 * T):].abs().max() == 0
    full = fz(wav)
    assert full.mean(1).abs().max().item() < 1e-5                  # time mean over all frames removed
    assert fz(wav[0]).shape == (1, T, 64)                          # a 1-D waveform is one row
    # pickling drops native handles and keeps the model
    fz._native = {0: object()}
    clone = pickle.loads(pickle.dumps(fz))
    assert clone._native == {} and torch.equal(clone(wav), full)
    # per-row lengths on the CPU: every row on its own
    short = fz.forward_varlen(wav, torch.tensor([8000, 399, 400]))   # below the receptive field: an all-zero row, no error
    assert short[1].abs().max() == 0 and short[2, 0].abs().max() == 0 and short[2, 1:].abs().max() == 0 and short[0].abs().max() > 0
    vl = fz.forward_varlen(wav, torch.tensor([8000, 8000, 5000]))
    assert torch.allclose(vl[2, :fz(wav[2, :5000]).shape[1]], fz(wav[2, :5000])[0]) and vl[2, fz(wav[2, :5000]).shape[1]:].abs().max() == 0


def test_audio_featurizer_refuses_other_model_types(tmp_path):
    transformers = pytest.importorskip('transformers')
    cfg = transformers.HubertConfig(conv_dim=(64,) * 7, hidden_size=32, num_hidden_layers=1, num_attention_heads=2, intermediate_size=64,
                                    num_conv_pos_embeddings=16, num_conv_pos_embedding_groups=2)
    transformers.HubertModel(cfg).save_pretrained(str(tmp_path))
    transformers.Wav2Vec2FeatureExtractor().save_pretrained(str(tmp_path))
    with pytest.raises(NotImplementedError, match="model_type 'hubert'"):
        AudioFeaturizer(feature_method=str(tmp_path), use_hf_model=True)
