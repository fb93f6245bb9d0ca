"""The Wav2Vec2-BERT (w2v-bert-2.0) front-end, AudioFeaturizer(use_hf_model=True), on the CPU and on the emulator build of csrc/w2vbert.hip:
the restatement tests/w2vbert_ref.py against the fixtures of the HF code (tools/make_w2vbert_golden.py), the native handle and its kernels
against the restatement's fp64 arbiter under the bars of tests/w2vbert_cases.py, the refusals, and the Python surface."""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

import w2vbert_cases as wc
import w2vbert_ref as ref
from emu_lib import emu_cdll
from mvector import _hip
from mvector.data_utils.featurizer import AudioFeaturizer

# what tools/make_w2vbert_golden.py printed when the fixtures were written: fp64 restatement - HF's extract_features, max-abs.  HF normalises
# in float32 numpy (x - mean of values around 15, over sqrt(var)): that, not the restatement, is the distance.
GOLDEN_DISTANCE = {'hf_w2vbert_even': 3.392e-05, 'hf_w2vbert_odd': 1.069e-05}


# ---- the restatement against the HF code's own output ----

@pytest.mark.parametrize('name', wc.FIXTURES)
def test_restatement_meets_the_hf_fixture(name):
    cfg, ln_w, ln_b, wav, gold = wc.load_fixture(name)
    assert cfg['model_type'] == 'wav2vec2-bert' and cfg['feature_projection_input_dim'] == 160 and cfg['stride'] == 2
    assert gold.shape == (wav.shape[0], ref.num_stacked(wav.shape[1]), 160)
    if name == 'hf_w2vbert_even':
        assert wav.shape == (3, 8000) and wav[2, 5000:].abs().max() == 0
    else:
        assert wav.shape == (2, 16160) and ref.num_frames(16160) == 99 and gold.shape[1] == 50
    d64 = (ref.extract_features(ln_w, ln_b, cfg, wav, torch.float64) - gold.double()).abs().max().item()
    print(f'{name}: fp64 restatement - HF {d64:.3e} (recorded {GOLDEN_DISTANCE[name]:.3e})')
    assert d64 <= 2 * GOLDEN_DISTANCE[name]


@pytest.mark.parametrize('name', list(wc.CASES) + ['varlen'])
def test_case_inputs_keep_every_bin_std_above_half(name):
    assert wc.check_bin_std(name) >= 0.5


# ---- the native handle on the emulator ----

@pytest.mark.parametrize('name', list(wc.CASES))
def test_emulated_handle_meets_the_fp64_arbiter(name):
    got, r64 = wc.run(name, emu_cdll())
    print(wc.check_case(name, got, r64))


@pytest.fixture(scope='module')
def varlen_run():
    h = wc.handle(emu_cdll())
    wav = wc.varlen_input()
    return h, wav, wc.forward_prefilled(h, wav, None, wc.VARLEN_LENS)


def test_emulated_varlen_meets_the_fp64_arbiter(varlen_run):
    _, _, got = varlen_run
    r64 = wc.varlen_reference()
    mx, mean = wc.distances(got, r64)
    bmx, bmean = wc.bars('varlen')
    print(f'varlen: max-abs {mx:.3e} (bar {bmx:.3e}) mean-abs {mean:.3e} (bar {bmean:.3e})')
    assert torch.isfinite(got).all() and mx <= bmx and mean <= bmean


def test_emulated_varlen_rows_equal_their_single_row_forward(varlen_run):
    h, wav, got = varlen_run
    for b, n in enumerate(wc.VARLEN_LENS):
        if n < ref.MIN_SAMPLES:
            assert got[b].abs().max().item() == 0.0   # 559 samples: all zero, no error
            continue
        alone = h(wav[b:b + 1, :n].contiguous())
        t2 = alone.shape[1]
        assert t2 == ref.num_stacked(n) and torch.equal(got[b, :t2], alone[0]) and (t2 == got.shape[1] or got[b, t2:].abs().max().item() == 0.0)
    assert got[3, 1, 80:].abs().max().item() > 0   # 720 samples, 3 frames: the zero half-frame is zeros BEFORE the LayerNorm, not behind it


def test_emulated_row_bits_do_not_depend_on_the_batch():
    h = wc.handle(emu_cdll())
    wav = wc.build('L8000_B3')[2][:, :2400].contiguous()
    whole = h(wav)
    for b in range(3):
        assert torch.equal(h(wav[b:b + 1])[0], whole[b])


# ---- the two kernels alone ----

@pytest.fixture(scope='module')
def stage():
    mel = wc.stage_input()
    return mel, wc.stage_stats_f64(mel), wc.stage_stats_f64(mel, wc.STAGE_LENS)


def _ulps(got, want64):
    """distance of fp32 `got` from the fp64 value in units of the fp32 spacing at that value"""
    want32 = want64.astype(np.float32)
    return np.abs(got.astype(np.float64) - want64) / np.spacing(np.abs(want32)).astype(np.float64)


@pytest.mark.parametrize('varlen', [False, True])
def test_emulated_binstats_within_one_ulp_of_fp64(stage, varlen):
    mel, full, own = stage
    mean64, var64 = own if varlen else full
    mean, var = _hip.w2vbert_binstats(mel, wc.STAGE_LENS if varlen else None, wc.STAGE_L if varlen else None, cdll=emu_cdll())
    live = [b for b in range(3) if not (varlen and wc.STAGE_LENS[b] < ref.MIN_SAMPLES)]
    um, uv = _ulps(mean.numpy()[live], mean64[live]).max(), _ulps(var.numpy()[live], var64[live]).max()
    print(f'binstats varlen={varlen}: mean {um:.2f} ulp, var {uv:.2f} ulp')
    assert um <= 1.0 and uv <= 1.0
    if varlen:
        assert mean[2].abs().max() == 0 and var[2].abs().max() == 0   # a row without frames


@pytest.mark.parametrize('varlen', [False, True])
def test_emulated_rows_meet_the_fp64_stage(stage, varlen):
    mel, full, own = stage
    lens = wc.STAGE_LENS if varlen else None
    mean, var = (torch.from_numpy(a).float() for a in (own if varlen else full))
    ln_w, ln_b = wc.layer_norm_tensors()
    out = torch.full((3, 99, 160), float('nan'))
    got = _hip.w2vbert_rows(mel, mean, var, ln_w, ln_b, 1e-5, lens, wc.STAGE_L if varlen else None, out=out, cdll=emu_cdll())
    mx, mn = wc.distances(got, wc.stage_rows(mel, mean, var, torch.float64, lens))
    bmx, bmn = wc.stage_bars('rows_varlen' if varlen else 'rows')
    print(f'rows varlen={varlen}: max-abs {mx:.3e} (bar {bmx:.3e}) mean-abs {mn:.3e} (bar {bmn:.3e})')
    assert torch.isfinite(got).all() and mx <= bmx and mn <= bmn
    if varlen:
        assert got[1, 50:].abs().max() == 0 and got[2].abs().max() == 0 and got[1, 49, 80:].abs().max() > 0


def test_emulated_cmn_mask_in_place():
    g = torch.Generator().manual_seed(5)
    x = torch.randn(2, 37, 160, generator=g) + 3.0
    got = _hip.w2vbert_cmn_mask(x.clone(), torch.tensor([1.0, 0.5]), cdll=emu_cdll())
    want = ref.wrapper(x.double(), [1.0, 0.5])
    assert (got.double() - want).abs().max().item() <= 2.0 ** -22 and got[1, 18:].abs().max() == 0   # one rounding of the mean, one of the difference, at |x| < 8


# ---- the library surface ----

def test_exports_present():
    names = ['mv_w2vbert_create', 'mv_w2vbert_destroy', 'mv_w2vbert_num_frames', 'mv_w2vbert_workspace_bytes', 'mv_w2vbert_forward',
             'mv_w2vbert_forward_varlen', 'mv_w2vbert_binstats_f32', 'mv_w2vbert_rows_f32', 'mv_w2vbert_cmn_mask_f32']
    cdll = emu_cdll()
    for n in names:
        assert n in _hip.EXPORTED_SYMBOLS and hasattr(cdll, n)
    assert cdll.mv_abi_version() == 5
    h = wc.handle(cdll)
    for n in (0, 399, 400, 559, 560, 719, 720, 8000, 16160):
        assert h.num_frames(n) == ref.num_stacked(n)


def _refused(cdll, rc, code, fragment):
    assert rc == code and fragment in cdll.mv_last_error().decode(), (rc, cdll.mv_last_error())


def test_refusals_name_what_is_wrong():
    cdll = emu_cdll()
    ln_w, ln_b = wc.layer_norm_tensors()
    UNSUPPORTED, INVALID, WORKSPACE = -3, -1, -4

    def create(**kw):
        c = _hip.MvW2vBertCfg(80, 2, 16000, 1e-5, 1)
        for k, v in kw.items():
            setattr(c, k, v)
        h = ctypes.c_void_p()
        return cdll.mv_w2vbert_create(ctypes.byref(c), ln_w.data_ptr(), ln_b.data_ptr(), ctypes.byref(h)), h

    _refused(cdll, create(num_mel_bins=64)[0], UNSUPPORTED, 'num_mel_bins = 64')
    _refused(cdll, create(stride=3)[0], UNSUPPORTED, 'stride = 3')
    _refused(cdll, create(sampling_rate=8000)[0], UNSUPPORTED, 'sampling_rate = 8000')
    _refused(cdll, create(layer_norm_eps=0.0)[0], INVALID, 'layer_norm_eps must be positive')
    c = _hip.MvW2vBertCfg(80, 2, 16000, 1e-5, 1)
    out_h = ctypes.c_void_p()
    _refused(cdll, cdll.mv_w2vbert_create(ctypes.byref(c), None, ln_b.data_ptr(), ctypes.byref(out_h)), INVALID, 'null argument')
    with pytest.raises(RuntimeError, match='stride = 3'):
        _hip.W2vBert(dict(wc.CFG, stride=3), {'feature_projection.layer_norm.weight': torch.ones(240), 'feature_projection.layer_norm.bias': torch.zeros(240)},
                     cdll=cdll)
    with pytest.raises(ValueError, match='has 160 elements, expected stride . num_mel_bins = 240'):
        _hip.W2vBert(dict(wc.CFG, stride=3), {'feature_projection.layer_norm.weight': ln_w, 'feature_projection.layer_norm.bias': ln_b}, cdll=cdll)

    rc, h = create()
    assert rc == 0
    wav, out = torch.zeros(2, 800), torch.zeros(2, 2, 160)
    need = ctypes.c_size_t()
    assert cdll.mv_w2vbert_workspace_bytes(h, 2, 800, ctypes.byref(need)) == 0 and need.value > 2 * 3 * 80 * 4
    ws = torch.zeros(need.value + 16, dtype=torch.uint8)
    fwd = lambda *a: cdll.mv_w2vbert_forward(h, *a, None)   # noqa: E731
    _refused(cdll, fwd(None, 2, 800, 800, None, out.data_ptr(), ws.data_ptr(), need.value), INVALID, 'null buffer')
    _refused(cdll, fwd(wav.data_ptr(), -1, 800, 800, None, out.data_ptr(), ws.data_ptr(), need.value), INVALID, 'negative size')
    _refused(cdll, fwd(wav.data_ptr(), 2, 800, 799, None, out.data_ptr(), ws.data_ptr(), need.value), INVALID, 'wav_stride below the row length')
    _refused(cdll, fwd(wav.data_ptr(), 2, 559, 800, None, out.data_ptr(), ws.data_ptr(), need.value), INVALID, '559 samples has fewer than two frames')
    _refused(cdll, fwd(wav.data_ptr(), 2, 800, 800, None, out.data_ptr(), ws.data_ptr(), need.value - 1), WORKSPACE, 'workspace of')
    _refused(cdll, fwd(wav.data_ptr(), 2, 800, 800, None, out.data_ptr(), ws.data_ptr() + 4, need.value), WORKSPACE, '16-byte aligned')
    _refused(cdll, fwd(wav.data_ptr(), 2, 800, 800, None, out.data_ptr(), None, 0), WORKSPACE, 'workspace of')
    _refused(cdll, cdll.mv_w2vbert_forward_varlen(h, wav.data_ptr(), 2, 800, 800, None, out.data_ptr(), ws.data_ptr(), need.value, None), INVALID,
             'null length array')
    _refused(cdll, cdll.mv_w2vbert_forward(None, wav.data_ptr(), 2, 800, 800, None, out.data_ptr(), ws.data_ptr(), need.value, None), INVALID, 'null handle')
    # B = 0 touches nothing: null buffers are not even looked at
    assert fwd(None, 0, 800, 800, None, None, None, 0) == 0
    # the kernel entry points
    mel = torch.zeros(1, 3, 80)
    m, v = torch.zeros(1, 80), torch.zeros(1, 80)
    _refused(cdll, cdll.mv_w2vbert_binstats_f32(mel.data_ptr(), 1, 1, None, 0, m.data_ptr(), v.data_ptr(), None), INVALID, 'T must be at least 2')
    _refused(cdll, cdll.mv_w2vbert_binstats_f32(None, 1, 3, None, 0, m.data_ptr(), v.data_ptr(), None), INVALID, 'null argument')
    lens = torch.tensor([700])
    _refused(cdll, cdll.mv_w2vbert_binstats_f32(mel.data_ptr(), 1, 3, lens.data_ptr(), 900, m.data_ptr(), v.data_ptr(), None), INVALID,
             'T is not the frame count of L samples')
    o = torch.zeros(1, 2, 160)
    _refused(cdll, cdll.mv_w2vbert_rows_f32(mel.data_ptr(), m.data_ptr(), v.data_ptr(), ln_w.data_ptr(), ln_b.data_ptr(), 0.0, 1, 3, None, 0, o.data_ptr(), None),
             INVALID, 'eps must be positive')
    _refused(cdll, cdll.mv_w2vbert_rows_f32(mel.data_ptr() + 4, m.data_ptr(), v.data_ptr(), ln_w.data_ptr(), ln_b.data_ptr(), 1e-5, 1, 3, None, 0, o.data_ptr(),
                                            None), INVALID, '16-byte aligned')
    r = torch.ones(1)
    _refused(cdll, cdll.mv_w2vbert_cmn_mask_f32(o.data_ptr(), 1, 2, r.data_ptr(), lens.data_ptr(), 720, 1, None), INVALID, 'not both')
    assert cdll.mv_w2vbert_destroy(h) == 0


# ---- the Python surface (needs `transformers` to write a model folder) ----

@pytest.fixture(scope='module')
def mk():
    pytest.importorskip('transformers')
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'tools'))
    import make_w2vbert_golden
    return make_w2vbert_golden


def test_audio_featurizer_on_a_model_folder(mk, tmp_path):
    import transformers
    cfg, ln_w, ln_b, wav, gold = wc.load_fixture('hf_w2vbert_even')
    folder = mk.save_model(str(tmp_path), seed=0)
    model = transformers.AutoModel.from_pretrained(folder)   # the fixture's LayerNorm into the folder's model
    with torch.no_grad():
        model.feature_projection.layer_norm.weight.copy_(ln_w)
        model.feature_projection.layer_norm.bias.copy_(ln_b)
    model.save_pretrained(folder)
    fz = AudioFeaturizer(feature_method=folder, use_hf_model=True, method_args={'use_gpu': False})
    assert fz.feature_dim == 160 and fz.use_hf_model and fz._hf_min_samples() == 560
    ratio = torch.tensor([1.0, 0.5, 0.8])
    got = fz(wav, ratio)
    want = ref.wrapper(gold, ratio)   # the HF model's own output under the reference's wrapper
    assert got.shape == want.shape and (got - want).abs().max().item() <= 1e-5   # the same fp32 arithmetic: the time mean's summation order alone
    assert got[1, 12:].abs().max() == 0 and got[2, 19:].abs().max() == 0 and got[2, :19].abs().max() > 0
    vl = fz.forward_varlen(wav, torch.tensor([8000, 559, 720]))
    assert vl.shape == got.shape and vl[1].abs().max() == 0 and vl[2, 2:].abs().max() == 0 and torch.allclose(vl[2, :2], fz(wav[2, :720])[0])


def test_audio_featurizer_refuses_what_the_library_refuses(mk, tmp_path):
    a, b = tmp_path / 'left', tmp_path / 'stride3'
    mk.save_model(str(a), padding_side='left')
    with pytest.raises(NotImplementedError, match="padding_side = 'left'"):
        AudioFeaturizer(feature_method=str(a), use_hf_model=True)
    mk.save_model(str(b), stride=3)
    with pytest.raises(NotImplementedError, match='stride = 3'):
        AudioFeaturizer(feature_method=str(b), use_hf_model=True)
