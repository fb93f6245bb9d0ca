"""Variable-length batches of the HuggingFace (Wav2Vec2 / WavLM) front-end, mv_hfenc_forward_varlen, on the emulator build of csrc/hfencoder.hip:
every row bit for bit what the fixed-length forward gives for it alone, zeros behind its own frames, independence of the tail and of the batch,
the C == 512 form against the fp64 arbiter, the refusals, the exports and AudioFeaturizer's CPU path.  Cases and checks: tests/hf_varlen_cases.py."""
import ctypes
import functools

import pytest
import torch

import hf_cases as hc
import hf_ref
import hf_varlen_cases as vc
from emu_lib import emu_cdll
from mvector import _hip
from mvector.data_utils.featurizer import AudioFeaturizer


def _handle(cfg, sd, cmn=True):
    return _hip.HfEncoder(cfg, sd, subtract_time_mean=cmn, cdll=emu_cdll())


@functools.lru_cache(maxsize=None)
def _batch(name, cmn):
    """(handle, wav [11, 1300], the variable-length output of the whole batch): computed once, shared by the tests below, never written to"""
    cfg, sd, wav = vc.emu_batch(name)
    h = _handle(cfg, sd, cmn)
    return h, wav, h(wav, None, torch.tensor(vc.EMU_LENS))


def test_the_lengths_sit_where_the_table_says():
    for n, t in vc.EMU_T0.items():
        assert hc.frames_of(n)[0] == t, n
    for n, t in vc.EMU_TL.items():
        assert max(hf_ref.num_frames(hc.BASE, n), 0) == t, n
    assert hf_ref.receptive_field(hc.BASE) == 400
    assert hc.frames_of(2565)[0] == 512 and hc.frames_of(2570)[0] == 513
    seen = {(hc.load_fixture(f)[0]['feat_extract_norm'], hc.load_fixture(f)[0]['conv_bias'], hc.load_fixture(f)[0]['do_normalize'])
            for f in hc.FIXTURES}
    assert seen == {('group', False, True), ('layer', True, True), ('group', True, False), ('layer', False, False)}


# ---- bit identity, zeros, the tail and the batch: the four fixtures (both modes x both biases, do_normalize on and off) ----

@pytest.mark.parametrize('cmn', [True, False], ids=['cmn', 'no_cmn'])
@pytest.mark.parametrize('name', hc.FIXTURES)
def test_emu_row_bits_are_those_of_the_row_alone(name, cmn):
    h, wav, out = _batch(name, cmn)
    vc.check_rows(h, wav, vc.EMU_LENS, out=out)
    assert bool(torch.isfinite(out).all())
    for b, n in enumerate(vc.EMU_LENS):
        if n < 400:
            continue
        if cmn and h.num_frames(vc.clamp(n, vc.EMU_L)) == 1:
            assert out[b].abs().max().item() == 0.0      # one frame (n = 400 .. 719) minus its own mean: why the case runs without the mean too
        else:
            assert out[b].abs().max().item() > 0.0


def test_emu_fixed_length_forward_is_the_same_code_at_full_length():
    """mv_hfenc_forward passes no lengths and the kernels take n_b = L: the bits of the variable-length call with every length = L"""
    for name in ('hf_wav2vec2_group', 'hf_wav2vec2_layer'):
        h, wav, _ = _batch(name, True)
        wav = wav[:2]
        assert torch.equal(h(wav, None, torch.tensor([vc.EMU_L, vc.EMU_L + 7])), h(wav))


@pytest.mark.parametrize('name', ['hf_wav2vec2_group', 'hf_wav2vec2_layer'])
def test_emu_result_does_not_depend_on_the_tail(name):
    """do_normalize fixtures (the waveform statistics skip the tail), without the time mean (so that the one-frame rows are not trivially zero)"""
    h, wav, out = _batch(name, False)
    n = torch.tensor(vc.EMU_LENS)
    for value in (float('nan'), 1e4):
        assert torch.equal(h(vc.with_tail(wav, vc.EMU_LENS, value), None, n), out), value


@pytest.mark.parametrize('name', ['hf_wavlm_group', 'hf_wav2vec2_layer'])
def test_emu_row_bits_do_not_depend_on_the_batch(name):
    h, wav, out = _batch(name, False)
    n = torch.tensor(vc.EMU_LENS)
    for b in vc.BATCH_ROWS:
        assert torch.equal(h(wav[b:b + 1], None, n[b:b + 1])[0], out[b]), b
    # ... nor on L: the row in a narrower padded batch
    b = 6
    narrow = h(wav[b:b + 1, :700], None, n[b:b + 1])
    assert torch.equal(narrow[0], out[b, :narrow.shape[1]]) and bool((out[b, narrow.shape[1]:] == 0).all())


# ---- width 512: the C == 512 form of hf_rows_kernel ----

@pytest.mark.parametrize('norm', ['group', 'layer'])
def test_emu_width_512(norm):
    cfg, sd, wav = vc.w512_batch(norm)
    h = _handle(cfg, sd)
    out = vc.check_rows(h, wav, vc.W512_LENS)
    vc.check_arbiter(f'w512_{norm}_L800_row0', out[0], cfg, sd, wav, vc.W512_LENS, 0)


# ---- refusals ----

def test_refusals_name_what_is_wrong():
    cdll = emu_cdll()
    cfg, sd = hc.seeded_model('group', width=64)
    h = _handle(cfg, sd)
    wav = torch.zeros(2, 800)
    n = torch.tensor([800, 500])
    with pytest.raises(ValueError, match='mutually exclusive'):
        h(wav, torch.ones(2), n)
    with pytest.raises(ValueError, match='mutually exclusive'):
        h(wav, lens_ratio=torch.ones(2), num_samples=n)
    with pytest.raises(ValueError, match='shape'):
        h(wav, None, n[:1])
    with pytest.raises(RuntimeError, match='399 samples is shorter than the encoder.s receptive field of 400'):
        h(torch.zeros(2, 399), None, torch.tensor([399, 10]))
    need = ctypes.c_size_t()
    _hip.check(cdll.mv_hfenc_workspace_bytes(h._h, 2, 800, ctypes.byref(need)), cdll)
    ws = torch.empty(need.value, dtype=torch.uint8)
    out = torch.empty(2, h.num_frames(800), 64)
    assert cdll.mv_hfenc_forward_varlen(h._h, wav.data_ptr(), 2, 800, 800, None, out.data_ptr(), ws.data_ptr(), need.value, None) != 0
    assert b'mv_hfenc_forward_varlen: null length array' in cdll.mv_last_error()
    assert cdll.mv_hfenc_forward_varlen(h._h, wav.data_ptr(), 2, 800, 800, n.data_ptr(), out.data_ptr(), ws.data_ptr(), need.value - 16, None) != 0
    assert b'workspace of ' + str(need.value).encode() + b' bytes' in cdll.mv_last_error()
    assert cdll.mv_hfenc_forward_varlen(h._h, wav.data_ptr(), 2, 800, 800, n.data_ptr(), out.data_ptr(), ws.data_ptr(), need.value, None) == 0


# ---- exports and ABI ----

def test_exports_present_and_abi_unchanged():
    cdll = emu_cdll()
    assert 'mv_hfenc_forward_varlen' in _hip.EXPORTED_SYMBOLS and hasattr(cdll, 'mv_hfenc_forward_varlen')
    assert cdll.mv_hfenc_forward_varlen.argtypes is not None and len(cdll.mv_hfenc_forward_varlen.argtypes) == 10
    assert cdll.mv_abi_version() == 5


def test_handle_takes_num_samples_third():
    cfg, sd, wav = vc.emu_batch('hf_wav2vec2_group')
    h = _handle(cfg, sd)
    wav, n = wav[5:9], torch.tensor(vc.EMU_LENS[5:9])
    out = h(wav, None, n)
    assert torch.equal(h(wav, num_samples=n), out)
    assert torch.equal(h(wav, None, n.to(torch.int32)), out) and torch.equal(h(wav, None, vc.EMU_LENS[5:9]), out)
    ms = []   # stage_ms stays a keyword of the fixed-length forward
    assert torch.equal(h(wav, stage_ms=ms), h(wav)) and len(ms) == 8
    with pytest.raises(ValueError):
        h(wav, None, n, stage_ms=[])


# ---- AudioFeaturizer on the CPU: still the per-row loop ----

@pytest.fixture(scope='module')
def hf_folder(tmp_path_factory):
    transformers = pytest.importorskip('transformers')
    import os
    import sys
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'tools'))
    import make_hf_golden as mk
    name = 'hf_wav2vec2_group'
    model_type, norm, conv_bias, do_normalize = mk.FIXTURES[name]
    folder = str(tmp_path_factory.mktemp(name))
    mk.save_model(folder, model_type, norm, conv_bias, do_normalize, seed=0)
    model = transformers.AutoModel.from_pretrained(folder)   # the fixture's front-end weights into the folder's model
    res = model.load_state_dict(hc.load_fixture(name)[1], strict=False)
    assert not res.unexpected_keys
    model.save_pretrained(folder)
    return name, folder


def test_cpu_featurizer_forward_varlen_keeps_the_per_row_loop(hf_folder, monkeypatch):
    name, folder = hf_folder
    cfg, sd, wav, gold = hc.load_fixture(name)
    fz = AudioFeaturizer(feature_method=folder, use_hf_model=True)
    lens = [8000, 399, 5000]
    calls = []
    forward = fz.forward
    monkeypatch.setattr(fz, 'forward', lambda w, r=None: calls.append(tuple(w.shape)) or forward(w, r))
    out = fz.forward_varlen(wav, torch.tensor(lens))
    assert calls == [(1, 8000), (8000,), (5000,)]   # the probe of T, then every row that has a frame, alone
    bound = 2 * 7 * 16 * 2.0 ** -24 * gold.abs().max().item()   # (test_hf_frontend.py's bound against the HF model's own output)
    assert out.shape == gold.shape and (out[0] - hf_ref.wrapper(gold[:1])[0]).abs().max().item() <= bound
    assert out[1].abs().max().item() == 0.0
    t2 = hf_ref.num_frames(cfg, 5000)
    assert torch.equal(out[2, :t2], forward(wav[2, :5000])[0]) and out[2, t2:].abs().max().item() == 0.0
