"""The SAP / TAP / TSP pooling heads of TDNN and EcapaTdnn (pooling_type, mvector/models/pooling.py) under the SIMT emulator: the two new
kernels (mv_sap_pool_f16: the mean-only form of the attentive pooling kernels; mv_time_mean_var_f16: mean | unbiased variance) against the
fp64 arbiter of tests/pooling_ref.py, the arbiter against the reference's goldens, the pooled handles (mv_*_create_pooled) against those
goldens and against the package's torch forward, the refusals, and the Python gates."""
import ctypes
import os

import numpy as np
import pytest
import torch

import pooling_ref as pr
from emu_lib import emu_cdll
from helpers import cos_dist, load_case
from mvector import _hip

LOG2E = 1.4426950408889634


def _pack(w):
    """nn.Conv1d weight [cout, cin, 1] fp32 -> the packed fp16 operand (mv_conv1d_pack_weight)"""
    cdll = emu_cdll()
    cout, cin, k = w.shape
    out = torch.empty(int(cdll.mv_conv1d_packed_elems(cout, cin, k)), dtype=torch.float16)
    _hip.check(cdll.mv_conv1d_pack_weight(w.contiguous().data_ptr(), cout, cin, k, out.data_ptr(), None), cdll)
    return out


def _mean_var(x, C=None):
    B, T, ld = x.shape
    C = C or ld
    out = torch.full((B, 2 * C), float('inf'))
    _hip.check(emu_cdll().mv_time_mean_var_f16(x.data_ptr(), ld, B, T, C, out.data_ptr(), 2 * C, None), emu_cdll())
    return out


def _sap(h, w2, x, bound=None):
    """h fp16 [B, T, A], w2 fp32 [C, A] (the linear2 weight), x fp16 [B, T, C] -> out [B, C] and the fp64 arbiter on the operands the kernel sees"""
    B, T, A = h.shape
    C = w2.shape[0]
    packed = _pack((w2 * LOG2E).reshape(C, A, 1))
    if bound is None:
        bound = float(w2.double().abs().sum(1).max()) * LOG2E * 1.001
    out = torch.full((B, C), float('inf'))
    _hip.check(emu_cdll().mv_sap_pool_f16(h.data_ptr(), packed.data_ptr(), x.data_ptr(), C, out.data_ptr(), B, T, C, A, bound, None), emu_cdll())
    w2h = (w2 * LOG2E).half().double().numpy() / LOG2E    # the fp16-rounded projection the kernel multiplies with
    ref = pr.sap_from_logits(h.double().numpy() @ w2h.T, x.double().numpy())
    return out.numpy(), ref


def _rows(B, T, C, seed, scale=1.5, shift=0.3):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(B, T, C, generator=g) * scale + shift).half()


# ------------------------------------------------------------------------------------------------ mean | unbiased variance

T_SWEEP = [1, 2, 15, 64, 65, 298, 1000]
C_SWEEP = [192, 512, 1536, 3072, 200]     # 200: not a multiple of 256 (nor of 128: a partial channel group)


@pytest.mark.parametrize('T', T_SWEEP)
@pytest.mark.parametrize('C', C_SWEEP)
def test_emu_time_mean_var_matches_fp64(T, C):
    x = _rows(2, T, C, seed=T * 7 + C)
    x[1, :, 3] = 0.8125                                    # constant channel
    x[0, :, 7] = (3.0e4 + 8.0 * torch.arange(T) % 5).half()   # |mean| >> std: 3e4 + {0, 8, ..} (E[x^2] - mean^2 loses it all in fp32)
    out = _mean_var(x).double().numpy()
    ref = pr.tsp(x.double().numpy())
    if T == 1:
        assert np.isnan(out[:, C:]).all()                  # torch.var of one sample: 0 / 0
        assert np.array_equal(out[:, :C], ref[:, :C])      # a single row's mean is that row
        return
    assert out[1, C + 3] == 0.0 and out[1, 3] == 0.8125    # exactly
    err_m = np.abs(out[:, :C] - ref[:, :C]).max()
    rel_v = (np.abs(out[:, C:] - ref[:, C:]) / np.maximum(ref[:, C:], 1e-3)).max()
    assert err_m < 2e-5 * max(1.0, np.abs(ref[:, :C]).max() / 1e3) and rel_v < 2e-5, (err_m, rel_v)


def test_emu_time_mean_var_cancellation_row():
    """a channel at 1024 + {0, 1, 2, 3} (fp16 exact): mean 1025.5, population variance 1.25 -- E[x^2] - mean^2 in fp32 (1e6 - 1e6) keeps ~0.06 of it"""
    T = 400
    x = torch.zeros(1, T, 64, dtype=torch.float16)
    x[0, :, 0] = (1024 + torch.arange(T) % 4).half()
    out = _mean_var(x)
    assert out[0, 0].item() == 1025.5
    assert abs(out[0, 64].item() - 1.25 * T / (T - 1)) < 1e-6 * 1.25, out[0, 64].item()


def test_emu_time_mean_var_rows_do_not_depend_on_the_batch():
    x = _rows(5, 301, 264, seed=3)
    full = _mean_var(x)
    for b in range(5):
        assert torch.equal(_mean_var(x[b:b + 1].contiguous()), full[b:b + 1])


def test_emu_time_mean_var_refuses_bad_arguments():
    x = _rows(2, 10, 64, seed=1)
    out = torch.zeros(2, 128)
    f = emu_cdll().mv_time_mean_var_f16
    cases = [((None, 64, 2, 10, 64, out.data_ptr(), 128), 'null tensor'), ((x.data_ptr(), 64, 2, 10, 64, None, 128), 'null tensor'),
             ((x.data_ptr(), 64, 0, 10, 64, out.data_ptr(), 128), 'bad geometry'), ((x.data_ptr(), 64, 2, 0, 64, out.data_ptr(), 128), 'bad geometry'),
             ((x.data_ptr(), 60, 2, 10, 60, out.data_ptr(), 120), '16-byte'), ((x.data_ptr(), 64, 2, 10, 72, out.data_ptr(), 144), 'ld >= C'),
             ((x.data_ptr(), 64, 2, 10, 64, out.data_ptr(), 127), 'leading dimension')]
    for args, msg in cases:
        with pytest.raises(RuntimeError, match=msg):
            _hip.check(f(*args, None), emu_cdll())
    assert torch.count_nonzero(out) == 0


# ------------------------------------------------------------------------------------------------ SAP pooling

SAP_T = [(T, 512) for T in T_SWEEP] + [(T, 200) for T in (1, 15, 65, 298)] + [(65, C) for C in (192, 1536, 3072)] + [(298, 3072)]


@pytest.mark.parametrize('T,C', SAP_T)
def test_emu_sap_pool_matches_fp64(T, C):
    g = torch.Generator().manual_seed(T + C)
    A = 128
    h = torch.tanh(torch.randn(2, T, A, generator=g) * 1.5).half()
    w2 = (torch.rand(C, A, generator=g) * 2 - 1) * 0.08
    x = _rows(2, T, C, seed=C - T)
    out, ref = _sap(h, w2, x)
    err = np.abs(out - ref).max() / max(1.0, np.abs(ref).max())
    assert err < 2e-5, err


@pytest.mark.parametrize('C', [512, 200])
def test_emu_sap_pool_logits_at_the_bound(C):
    """rows whose logit sits AT the bound the NOMAX form relies on: h = sign(W2[c*]) (tanh saturated) gives channel c* the logit
    sum_k |W2[c*, k]| = the bound, 58 in the kernel's log2 units (a weight of 2^58); the other rows sit far below -- one row takes all the weight"""
    A, T = 128, 65
    g = torch.Generator().manual_seed(C)
    w2 = (torch.rand(C, A, generator=g) * 2 - 1)
    w2 = w2 / w2.abs().sum(1, keepdim=True).max() * (58.0 / LOG2E)     # max_c sum_k |W2| * log2(e) = 58
    cstar = int(w2.abs().sum(1).argmax())
    h = torch.tanh(torch.randn(2, T, A, generator=g)).half()
    h[0, 17] = torch.sign(w2[cstar]).half()
    h[1, :] = torch.sign(w2[cstar]).half()                # every row at the bound: a uniform softmax for c*
    x = _rows(2, T, C, seed=5)
    out, ref = _sap(h, w2, x)
    assert np.isfinite(out).all()
    assert abs(out[0, cstar] - float(x[0, 17, cstar])) < 1e-3
    assert abs(out[1, cstar] - ref[1, cstar]) < 1e-4
    err = np.abs(out - ref).max() / max(1.0, np.abs(ref).max())
    assert err < 2e-5, err


def test_emu_sap_pool_unbounded_logits_take_the_online_form():
    """a negative bound (unknown weights): the online-softmax form, still the same softmax"""
    g = torch.Generator().manual_seed(2)
    h = torch.tanh(torch.randn(2, 40, 128, generator=g)).half()
    w2 = (torch.rand(200, 128, generator=g) * 2 - 1) * 0.5
    out, ref = _sap(h, w2, _rows(2, 40, 200, seed=2), bound=-1.0)
    assert np.abs(out - ref).max() < 2e-5 * max(1.0, np.abs(ref).max())


# ------------------------------------------------------------------------------------------------ goldens

HEADS = ['sap', 'tap', 'tsp']
GOLDENS = [f'tdnn_{p}' for p in HEADS] + [f'ecapa_{p}_tiny' for p in HEADS] + [f'ecapa_{p}_c1024' for p in HEADS]


def _module(man, sd):
    import mvector.models as M
    m = getattr(M, man['model'])(**man['kwargs'])
    m.load_state_dict(sd)
    return m.eval()


@pytest.mark.parametrize('case', GOLDENS)
def test_fp64_arbiter_matches_the_reference_goldens(case):
    """tests/pooling_ref.py (fp64 heads and tails on the package modules' backbone in fp64) reproduces the reference's own fp32 embedding"""
    man, sd, x, emb, _ = load_case(case)
    assert man['kwargs']['pooling_type'] == case.split('_')[1].upper()
    got = pr.embed(_module(man, sd), sd, x)
    d = cos_dist(got, emb).max().item()
    assert d < 1e-7, d


def _kind(man):
    return {'TDNN': 'tdnn', 'EcapaTdnn': 'ecapa'}[man['model']]


@pytest.mark.parametrize('case', [c for c in GOLDENS if 'c1024' not in c] + [
    pytest.param(c, marks=pytest.mark.skipif(os.environ.get('MV_SLOW_EMU') != '1', reason='minutes under the emulator; set MV_SLOW_EMU=1 '
                                             '(covered on the GPU by test_gpu_pooled_handle_matches_reference_golden)')) for c in GOLDENS if 'c1024' in c])
def test_emu_pooled_handle_matches_reference_golden(case):
    man, sd, x, emb, _ = load_case(case)
    m = _module(man, sd)
    got = _hip.Model(_kind(man), m._native_cfg(), sd, cdll=emu_cdll(), pooling_type=man['kwargs']['pooling_type']).forward(x)
    d = cos_dist(got, emb).max().item()
    print(f'{case}: 1 - cos {d:.2e}')
    assert d < 1e-5, d


def test_ecapa_tsp_runs_through_the_c_abi():
    """EcapaTdnn + TSP: built by the library (the Python gate keeps refusing it, see _native_supported) -- the handle against the fp64 arbiter"""
    man, sd, x, emb, _ = load_case('ecapa_tsp_tiny')
    m = _module(man, sd)
    got = _hip.Model('ecapa', m._native_cfg(), sd, cdll=emu_cdll(), pooling_type=_hip.MV_POOL_TSP).forward(x)
    assert cos_dist(got, pr.embed(m, sd, x)).max().item() < 1e-5


# ------------------------------------------------------------------------------------------------ other constructor arguments

ARG_CASES = [
    ('TDNN', dict(input_size=40, channels=128, embd_dim=96), 30),
    ('TDNN', dict(input_size=23, channels=256, embd_dim=192), 40),          # ragged feature width, a ring-kernel width (256)
    ('EcapaTdnn', dict(input_size=40, embd_dim=96, channels=[128, 128, 128, 128, 384]), 30),
    ('EcapaTdnn', dict(input_size=80, channels=[64, 64, 64, 64, 192], attention_channels=64, dilations=[2, 2, 3, 4, 1]), 24),  # SAP's bottleneck stays 128
]


@pytest.mark.parametrize('pool', ['SAP', 'TAP', 'TSP'])
@pytest.mark.parametrize('idx', range(len(ARG_CASES)))
def test_emu_pooled_handle_other_arguments_match_torch(idx, pool):
    import mvector.models as M
    from oracle import weights
    cls, kw, T = ARG_CASES[idx]
    m = getattr(M, cls)(pooling_type=pool, **kw)
    sd = weights.make_state_dict(weights.shapes_of(m.state_dict()), 17 + idx)
    m.load_state_dict(sd)
    m.eval()
    x = torch.randn(3, T, kw['input_size'], generator=torch.Generator().manual_seed(idx)) * 2
    with torch.no_grad():
        ref = m(x)
    got = _hip.Model(_kind(dict(model=cls)), m._native_cfg(), sd, cdll=emu_cdll(), pooling_type=pool).forward(x)
    assert got.shape == ref.shape
    d = cos_dist(got, ref).max().item()
    assert d < 1e-5, d


# ------------------------------------------------------------------------------------------------ refusals and gates

def _tiny(cls, pool):
    import mvector.models as M
    from oracle import weights
    kw = dict(input_size=40, channels=64, embd_dim=32) if cls == 'TDNN' else dict(input_size=40, channels=[64, 64, 64, 64, 192])
    m = getattr(M, cls)(pooling_type=pool, **kw)
    sd = weights.make_state_dict(weights.shapes_of(m.state_dict()), 1)
    m.load_state_dict(sd)
    return m.eval(), sd


@pytest.mark.parametrize('cls', ['TDNN', 'EcapaTdnn'])
def test_pooled_create_refuses_unknown_codes_and_missing_weights(cls):
    kind = _kind(dict(model=cls))
    m, sd = _tiny(cls, 'SAP')
    fn = f'mv_{kind}_create_pooled'
    for code in (4, -1, 99):
        with pytest.raises(RuntimeError, match=rf'{fn}: pooling_type {code} is not MV_POOL_ASP'):
            _hip.Model(kind, m._native_cfg(), sd, cdll=emu_cdll(), pooling_type=code)
    with pytest.raises(ValueError, match="pooling_type 'XYZ'"):
        _hip.Model(kind, m._native_cfg(), sd, cdll=emu_cdll(), pooling_type='XYZ')
    prefix = 'pooling' if cls == 'TDNN' else 'asp'
    for key in (f'{prefix}.linear1.weight', f'{prefix}.linear1.bias', f'{prefix}.linear2.weight'):
        bad = {k: v for k, v in sd.items() if k != key}
        with pytest.raises(RuntimeError, match=f"missing '{key}'"):
            _hip.Model(kind, m._native_cfg(), bad, cdll=emu_cdll(), pooling_type='SAP')
    # a TAP state_dict asked for the TSP head: the tail's BatchNorm has half the width the head gives
    m_tap, sd_tap = _tiny(cls, 'TAP')
    with pytest.raises(RuntimeError, match='elements, expected'):
        _hip.Model(kind, m_tap._native_cfg(), sd_tap, cdll=emu_cdll(), pooling_type='TSP')
    # an ASP state_dict asked for a head it does not have
    m_asp, sd_asp = _tiny(cls, 'ASP')
    with pytest.raises(RuntimeError, match='missing'):
        _hip.Model(kind, m_asp._native_cfg(), sd_asp, cdll=emu_cdll(), pooling_type='SAP')


def test_pooled_create_refusals_at_the_c_abi():
    cdll = emu_cdll()
    m, sd = _tiny('TDNN', 'TAP')
    refs = (_hip.MvTensorRef * 1)()
    h = ctypes.c_void_p()
    assert cdll.mv_tdnn_create_pooled(None, 2, refs, 1, ctypes.byref(h)) != 0
    assert b'null argument' in cdll.mv_last_error()
    assert cdll.mv_tdnn_create_pooled(ctypes.byref(m._native_cfg()), 5, refs, 1, ctypes.byref(h)) != 0
    assert b'pooling_type 5' in cdll.mv_last_error()
    assert cdll.mv_ecapa_create_pooled(ctypes.byref(_tiny('EcapaTdnn', 'TAP')[0]._native_cfg()), 2, refs, 0, ctypes.byref(h)) != 0
    assert b'empty tensor list' in cdll.mv_last_error()
    assert not h.value


def test_other_backbones_take_no_pooling_type():
    with pytest.raises(ValueError, match='only the ecapa and tdnn handles'):
        _hip.Model('campp', _hip.MvCamppCfg(), {'x': torch.zeros(1)}, cdll=emu_cdll(), pooling_type='TAP')


@pytest.mark.parametrize('cls,pool', [('TDNN', 'SAP'), ('TDNN', 'TAP'), ('TDNN', 'TSP'), ('EcapaTdnn', 'SAP'), ('EcapaTdnn', 'TAP')])
def test_native_supported_for_the_new_heads(cls, pool):
    m, _ = _tiny(cls, pool)
    ok, why = m._native_supported()
    assert ok, why
    assert m._native_pooling_type() == pool


def test_ecapa_tsp_gate_still_refuses_by_name():
    m, _ = _tiny('EcapaTdnn', 'TSP')
    ok, why = m._native_supported()
    assert not ok and 'pooling_type' in why and 'TSP' in why
