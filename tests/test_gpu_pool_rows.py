"""The time reductions and element-wise row passes of csrc/pool.hip on the MI355X, one kernel at a time: the case functions of tests/layer_checks.py
(fp64 references, bars derived from each kernel's summation order, sentinel pitch columns, NaN-filled outputs) through the product library -- the
same cases tests/test_pool_rows.py runs under the emulator.  Each case prints its largest error / bar ratio."""
import pytest
import torch

import layer_checks as lc
from test_pool_rows import CAST_F, CAST_PAD, CAST_ROWS, PAD_ROWS, SEG, TS_C, TS_T, _pad

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'


def _lib():
    from mvector import _hip
    return _hip.lib()


@pytest.mark.parametrize('C,ld', TS_C)
@pytest.mark.parametrize('T', TS_T)
def test_gpu_time_stats_edges(T, C, ld):
    lc.time_stats_ex_case(_lib(), DEV, B=2, T=T, C=C, ld=ld)
    if T > 1:
        lc.time_stats_ex_case(_lib(), DEV, B=2, T=T, C=C, ld=ld, unbiased=1, eps=0.0, seed=1)


def test_gpu_time_stats_three_forms_on_the_same_rows():
    lc.time_stats_forms_case(_lib(), DEV)


@pytest.mark.parametrize('C', [264, 261])
@pytest.mark.parametrize('out_pad', [0, 8])
def test_gpu_time_stats_preactivation_and_output_pitch(out_pad, C):
    lc.time_stats_preact_case(_lib(), DEV, C=C, out_pad=out_pad)


@pytest.mark.parametrize('C,pre', [(264, False), (261, False), (261, True)])
def test_gpu_time_stats_nan_frame(C, pre):
    lc.time_stats_nan_case(_lib(), DEV, C=C, pre=pre)


def test_gpu_time_stats_nan_frame_large_grid_forms():
    lc.time_stats_nan_case(_lib(), DEV, T=33, C=136, ld=144, B_big=1025)


def test_gpu_time_stats_row_bits_do_not_depend_on_the_batch_size():
    lc.time_stats_batch_rows_case(_lib(), DEV)


def test_gpu_time_stats_refusals():
    m = lc.time_stats_refusal_case(_lib(), DEV)
    assert 'unbiased' in m[0] and 'output leading dimension' in m[1] and '16-byte aligned' in m[2], m


@pytest.mark.parametrize('C', [8, 136])
@pytest.mark.parametrize('T,seg_len', SEG)
def test_gpu_seg_mean(T, seg_len, C):
    lc.seg_mean_case(_lib(), DEV, T=T, seg_len=seg_len, C=C)


def test_gpu_seg_mean_nan_and_batch_rows():
    lc.seg_mean_nan_case(_lib(), DEV)
    lc.seg_mean_batch_rows_case(_lib(), DEV)


@pytest.mark.parametrize('own', [False, True], ids=['slices', 'own'])
def test_gpu_se_gate_residual(own):
    lc.se_gate_residual_case(_lib(), DEV, own=own)


def test_gpu_se_gate_residual_ragged_last_workgroup():
    lc.se_gate_residual_case(_lib(), DEV, B=1, T=29, C=72)


@pytest.mark.parametrize('where', ['y', 'res', 'gate'])
def test_gpu_se_gate_residual_nan(where):
    lc.se_gate_nan_case(_lib(), DEV, where)


def test_gpu_se_gate_residual_row_bits_do_not_depend_on_the_batch_size():
    lc.se_gate_batch_rows_case(_lib(), DEV)


@pytest.mark.parametrize('A', [8, 136])
def test_gpu_asp_hidden_act(A):
    lc.asp_hidden_act_case(_lib(), DEV, A=A)
    lc.asp_hidden_nan_case(_lib(), DEV, A=A)


@pytest.mark.parametrize('nan', [False, True], ids=['', 'nan'])
@pytest.mark.parametrize('pad_kind', CAST_PAD)
@pytest.mark.parametrize('F', CAST_F)
def test_gpu_cast_pad(F, pad_kind, nan):
    lc.cast_pad_case(_lib(), DEV, F=F, pad=_pad(pad_kind), nan=nan)


@pytest.mark.parametrize('nan', [False, True], ids=['', 'nan'])
@pytest.mark.parametrize('C,ldd', CAST_ROWS)
def test_gpu_cast_rows(C, ldd, nan):
    lc.cast_rows_case(_lib(), DEV, C=C, ldd=ldd, nan=nan)


def test_gpu_copy_slice():
    lc.copy_slice_case(_lib(), DEV)


@pytest.mark.parametrize('F,ldd', PAD_ROWS)
def test_gpu_pad_rows_f32(F, ldd):
    lc.pad_rows_f32_case(_lib(), DEV, F=F, ldd=ldd)


def test_gpu_bn_relu_rows_keeps_nan():
    lc.bn_relu_rows_nan_case(_lib(), DEV)


def test_gpu_nan_feature_through_ecapa_tiny_is_reported():
    """Not asserted (the layer-level NaN cases above are the contract; the conv1d epilogues between them are another matter): what one NaN feature
    value gives at the embedding of ecapa_tiny is PRINTED."""
    from helpers import load_case
    from mvector import _hip
    man, sd, x, _, _ = load_case('ecapa_tiny')
    kw = man['kwargs']
    cfg = _hip.MvEcapaCfg()
    cfg.input_size, cfg.embd_dim = kw['input_size'], kw.get('embd_dim', 192)
    ch = kw.get('channels', [512, 512, 512, 512, 1536])
    for i in range(5):
        cfg.channels[i], cfg.kernel_sizes[i], cfg.dilations[i] = ch[i], [5, 3, 3, 3, 1][i], [1, 2, 3, 4, 1][i]
    cfg.attention_channels, cfg.res2net_scale, cfg.se_channels, cfg.global_context = 128, 8, 128, 1
    m = _hip.Model('ecapa', cfg, {k: v.to(DEV) for k, v in sd.items()}, cdll=_lib())
    x = x[:2].clone()
    x[0, x.shape[1] // 2, 3] = float('nan')
    emb = m.forward(x.to(DEV)).cpu()
    print(f'ecapa_tiny with one NaN feature in utterance 0: {int(torch.isnan(emb[0]).sum())} of {emb.shape[1]} embedding values NaN '
          f'(utterance 1, no NaN: {int(torch.isnan(emb[1]).sum())})')
