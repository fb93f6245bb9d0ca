"""Feature widths that are not multiples of 8 (Spectrogram's 201 bins, Fbank's default 23, MFCC 13 / 20, ...) under the SIMT emulator: the
zero-padding kernels against a numpy statement, EcapaTdnn (window and per-tap first conv), TDNN and CAM++ against the host package's torch
forward, and the padding contract -- a model at F = 201 gives the bits of the same model at F = 208 with zero-padded features and first-layer
weights."""
import os

import numpy as np
import pytest
import torch

from emu_lib import emu_cdll
from helpers import cos_dist
from mvector import _hip

# the zero-padding launchers of csrc/pool.hip through their layer-level entry points (mv_cast_pad_f16 makes the choice EcapaModel::forward makes: the
# ragged kernel whenever ldd != F)


def _pad_f16(src, dst, B, T, F, ldd, pad):
    return emu_cdll().mv_cast_pad_f16(src, dst, B, T, F, ldd, pad, None)


def _pad_f32(src, F, dst, ldd, n_rows):
    return emu_cdll().mv_pad_rows_f32(src, F, dst, ldd, n_rows, None)


def _round8(n):
    return (n + 7) // 8 * 8


def _features(B, T, F, seed):
    x = torch.randn(B, T, F, generator=torch.Generator().manual_seed(seed)) * 3
    x[0, 0, 0], x[-1, -1, -1] = 1.0e6, -7.0e4    # beyond the fp16 range: saturated like the aligned cast
    if F > 2:
        x[0, 1, 2] = 65519.0                       # rounds to inf in fp16 without the clamp
    return x


# ------------------------------------------------------------------------------------------------ kernels

@pytest.mark.parametrize('F', [1, 7, 13, 201, 257])
@pytest.mark.parametrize('pad_kind', ['0', '2', 'T-1'])
def test_emu_cast_reflect_pad_ragged(F, pad_kind):
    B, T = 2, 9
    pad = {'0': 0, '2': 2, 'T-1': T - 1}[pad_kind]
    ldd = _round8(F)
    x = _features(B, T, F, F + pad)
    out = torch.full((B * (T + 2 * pad) * ldd,), float('nan'), dtype=torch.float16)
    _hip.check(_pad_f16(x.data_ptr(), out.data_ptr(), B, T, F, ldd, pad), emu_cdll())
    want = np.zeros((B, T + 2 * pad, ldd), np.float16)
    xp = np.pad(x.numpy(), ((0, 0), (pad, pad), (0, 0)), mode='reflect')
    want[:, :, :F] = np.clip(xp, -65504.0, 65504.0).astype(np.float16)
    got = out.view(B, T + 2 * pad, ldd).numpy()
    assert np.array_equal(got.view(np.uint16), want.view(np.uint16))   # bitwise: the pad columns are +0, no NaN of the prefill survives


@pytest.mark.parametrize('F,ldd', [(1, 8), (7, 8), (13, 16), (201, 208), (257, 264), (13, 20), (16, 16)])
def test_emu_pad_rows_f32(F, ldd):
    n = 37
    x = _features(1, n, F, F)[0]
    x[3, 0] = float('inf')
    out = torch.full((n, ldd), float('nan'))
    _hip.check(_pad_f32(x.data_ptr(), F, out.data_ptr(), ldd, n), emu_cdll())
    want = torch.zeros(n, ldd)
    want[:, :F] = x                                       # an exact copy: no clamp, the first conv converts to fp16 itself
    assert torch.equal(out.view(torch.int32), want.view(torch.int32))


def test_emu_pad_kernels_refuse_bad_arguments():
    x = torch.zeros(2, 5, 13)
    y16 = torch.zeros(2 * 15 * 16, dtype=torch.float16)
    y32 = torch.zeros(10, 16)
    cases = [
        (lambda: _pad_f16(x.data_ptr(), y16.data_ptr(), 2, 5, 13, 16, 5), 'pad < T'),      # pad >= T
        (lambda: _pad_f16(x.data_ptr(), y16.data_ptr(), 2, 5, 13, 16, -1), 'pad < T'),
        (lambda: _pad_f16(None, y16.data_ptr(), 2, 5, 13, 16, 2), 'null tensor'),
        (lambda: _pad_f16(x.data_ptr(), None, 2, 5, 13, 16, 2), 'null tensor'),
        (lambda: _pad_f16(x.data_ptr(), y16.data_ptr(), 2, 5, 13, 12, 2), 'multiple of 8'),  # ldd < F
        (lambda: _pad_f16(x.data_ptr(), y16.data_ptr(), 2, 5, 13, 20, 2), 'multiple of 8'),
        (lambda: _pad_f32(None, 13, y32.data_ptr(), 16, 10), 'null tensor'),
        (lambda: _pad_f32(x.data_ptr(), 13, None, 16, 10), 'null tensor'),
        (lambda: _pad_f32(x.data_ptr(), 13, y32.data_ptr(), 8, 10), 'multiple of 4'),
        (lambda: _pad_f32(x.data_ptr(), 13, y32.data_ptr(), 14, 10), 'multiple of 4'),
    ]
    for call, msg in cases:
        with pytest.raises(RuntimeError, match=msg):
            _hip.check(call(), emu_cdll())
    assert torch.count_nonzero(y16) == 0 and torch.count_nonzero(y32) == 0   # nothing was launched


# ------------------------------------------------------------------------------------------------ models

def _ecapa_kw(F, dil0):
    return dict(input_size=F, channels=[64, 64, 64, 64, 192], dilations=[dil0, 2, 3, 4, 1])


def _tdnn_kw(F):
    return dict(input_size=F, channels=64, embd_dim=64)


def _model(cls, kw, seed=9):
    import mvector.models as M
    from oracle import weights
    m = getattr(M, cls)(**kw)
    sd = weights.make_state_dict(weights.shapes_of(m.state_dict()), seed)
    m.load_state_dict(sd)
    return m.eval(), sd


def _native(kind, m, sd, x):
    return _hip.Model(kind, m._native_cfg(), sd, cdll=emu_cdll()).forward(x).cpu()


MODEL_CASES = [('EcapaTdnn', 'window'), ('EcapaTdnn', 'per-tap'), ('TDNN', '')]


def _case(cls, form, F):
    if cls == 'EcapaTdnn':
        return 'ecapa', _ecapa_kw(F, 1 if form == 'window' else 2), 40, 'blocks.0.conv.conv.weight'
    return 'tdnn', _tdnn_kw(F), 40, 'td_layer1.weight'


@pytest.mark.parametrize('F', [13, 23, 201])
@pytest.mark.parametrize('cls,form', MODEL_CASES, ids=['ecapa-window', 'ecapa-per-tap', 'tdnn'])
def test_emu_model_at_ragged_feature_width_matches_torch(cls, form, F):
    kind, kw, T, _ = _case(cls, form, F)
    m, sd = _model(cls, kw)
    ok, why = m._native_supported()
    assert ok, why
    x = torch.randn(2, T, F, generator=torch.Generator().manual_seed(F)) * 2
    with torch.no_grad():
        ref = m(x)
    emb = _native(kind, m, sd, x)
    d = cos_dist(emb, ref).max().item()
    assert d < 1e-5, d


@pytest.mark.parametrize('cls,form', MODEL_CASES, ids=['ecapa-window', 'ecapa-per-tap', 'tdnn'])
def test_emu_ragged_width_gives_the_bits_of_the_zero_padded_width(cls, form):
    """the correctness contract of the padding: F = 201 against F = 208 with zero-padded features and zero first-layer weight columns"""
    kind, kw, T, wname = _case(cls, form, 201)
    m, sd = _model(cls, kw)
    kind208, kw208, _, _ = _case(cls, form, 208)
    m208, _ = _model(cls, kw208)
    sd208 = dict(sd)
    w = sd[wname]
    sd208[wname] = torch.cat([w, torch.zeros(w.shape[0], 7, w.shape[2])], dim=1)
    x = torch.randn(3, T, 201, generator=torch.Generator().manual_seed(1)) * 2
    x208 = torch.cat([x, torch.zeros(3, T, 7)], dim=2)
    a = _native(kind, m, sd, x)
    b = _native(kind208, m208, sd208, x208)
    assert torch.equal(a, b)


@pytest.mark.skipif(os.environ.get('MV_SLOW_EMU') != '1', reason='~4 min per width under the emulator; set MV_SLOW_EMU=1 (covered on the GPU by '
                    'test_gpu_campp_at_ragged_feature_width_matches_oracle)')
@pytest.mark.parametrize('F', [13, 23])
def test_emu_campp_at_ragged_feature_width(F):
    """CAM++ rounds the frequency axis up itself (F8 = ceil(F / 8) rows of 32 after the FCM head); odd heights through the strided head
    convs, both head precisions, against the host package's torch forward"""
    m, sd = _model('CAMPPlus', dict(input_size=F, embd_dim=64, init_channels=64))
    ok, why = m._native_supported()
    assert ok, why
    x = torch.randn(1, 40, F, generator=torch.Generator().manual_seed(F)) * 2
    with torch.no_grad():
        ref = m(x)
    for head in (1, 2):
        cfg = m._native_cfg()
        cfg.head_precision, cfg.xvector_probe = head, 1
        emb = _hip.Model('campp', cfg, sd, cdll=emu_cdll()).forward(x).cpu()
        d = cos_dist(emb, ref).max().item()
        assert d < (1e-3 if head == 1 else 1e-5), (head, d)
