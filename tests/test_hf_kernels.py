"""csrc/hfencoder.hip one kernel at a time, CPU tier: the self-checks of the per-element bounds of tests/hf_kernel_checks.py (no launch: each bound
admits the fp32 rounding model and rejects every applicable mutant on the case's own operands), then the cases, the refusals and the
composition of the forward from its pieces under the SIMT emulator.  The device tier is tests/test_gpu_hf_kernels.py."""
import os
import re

import pytest
import torch

import hf_kernel_checks as hk
from emu_lib import emu_cdll
from mvector import _hip

CASES = [(fam, name) for fam, (cases, _, _) in hk.FAMILIES.items() for name in cases]


# ---- the bounds, on the CPU alone ---------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('family,name', CASES, ids=lambda v: v)
def test_bound_admits_the_rounding_model_and_rejects_every_mutant(family, name):
    model, wrong = hk.model_ratios(family, name)
    print(f'{family} {name}: rounding model {model:.3f}; ' + ', '.join(f'{m} {r:.3g}' for m, r in wrong.items()))
    assert model <= 1.0, (family, name, model)
    for m, r in wrong.items():
        assert r > 1.0, f'{family} {name}: the bound does not see the mutant {m} (ratio {r:.3g})'


def test_every_mutant_is_applied_somewhere_in_every_family_it_belongs_to():
    want = {'wave': {'unbiased', 'eps_swap', 'eps_x100'},
            'layer0': {'tanh_gelu', 'unbiased', 'eps_swap', 'eps_x100', 'drop_tap', 'frames_plus', 'frames_minus'},
            'rows': {'tanh_gelu', 'unbiased', 'eps_swap', 'eps_x100'},
            'cmn': {'mean_unmasked', 'half_up', 'frames_plus', 'frames_minus'}}
    for fam, (cases, operands, mutants) in hk.FAMILIES.items():
        seen = set()
        for name in cases:
            seen |= set(mutants(operands(name)))
        assert seen == want[fam] and seen <= set(hk.MUTANTS), (fam, seen)


def test_cases_cover_the_shapes_at_which_the_kernels_take_another_path():
    assert {hk.WAVE_CASES[n][0] for n in hk.WAVE_CASES} == {1, 255, 256, 257, 1000}
    l0 = hk.L0_CASES.values()
    assert {(c['k'], c['s']) for c in l0} == {(10, 5), (3, 2), (1, 1), (11, 1), (16, 8)}
    assert {c['C'] for c in l0} == {64, 320, 512} and {c['T0'] for c in l0} == {1, 127, 128, 129, 257}
    assert {(c['mode'], c['bias']) for c in l0} >= {('group', False), ('group', True), ('layer', True)} and {c['wstats'] for c in l0} == {False, True}
    assert any(c['k'] == 16 and c['s'] == 8 and c['T0'] == 128 for c in l0) and any(c['extra'] for c in l0)
    rows = set(hk.ROWS_CASES.values())
    assert {(m, C) for m, C, _ in rows} == {(m, C) for m in hk.MODES for C in (64, 192, 512, 576, 1024)} and {R for _, _, R in rows} == {1, 4, 5, 9}
    cmn = hk.CMN_CASES.values()
    assert {c[0] for c in cmn} == {1, 3, 4, 5, 7, 50} and {c[1] for c in cmn} == {64, 192} and {c[2] for c in cmn} == {0, 1}
    o = hk.cmn_operands('T5_C192_ratio')
    assert o.ratio.tolist()[:4] == [0.0, 1.0, pytest.approx(1.2), 0.5] and o.mask[:4] == [0, 5, 6, 2] and hk.cmn_operands('T7_C64_ratio').mask[3] == 4
    assert hk.cmn_operands('T5_C64_samples').Tb[:3] == [0, 1, 5]
    o = hk.l0_operands('k10s5_C64_varlen_group')
    assert o.T0b == [0, 1, 128, 129, 257] and all(bool(torch.isnan(o.wav[b, n:]).all()) for b, n in enumerate(o.lens))


def test_operands_carry_the_variances_the_eps_mutants_need():
    """a quiet waveform row (3e-4), a layer-0 channel at output variance 1e-4, LayerNorm rows at variance 1e-5"""
    o = hk.wave_operands('L1000')
    assert 1e-4 < o.wav[3, :1000].std().item() < 1e-3
    o = hk.l0_operands('k10s5_C512_T257_group')
    v = hk.l0_eval(o, parts=True)[2]
    assert v[0, :, hk.LOWVAR_CH].var(unbiased=False).item() == pytest.approx(1e-4, rel=0.2)
    for name, row in (('ln_f32_C512_R4', 3), ('ln_gelu_C576_R1', 0)):
        assert hk.rows_operands(name).x[row].double().var(unbiased=False).item() == pytest.approx(1e-5, rel=0.3)


def test_one_launch_site_per_kernel_instantiation():
    """hfencoder.hip names each kernel in one MV_LAUNCH: the forward and the layer-level entry points share the launch helpers"""
    with open(os.path.join(os.path.dirname(_hip.__file__), '..', 'csrc', 'hfencoder.hip')) as f:
        sites = re.findall(r'MV_LAUNCH\(\(?(hf_\w+(?:<[^>]*>)?)', f.read())
    assert sorted(sites) == ['hf_cmn_mask_kernel', 'hf_l0_finish_kernel', 'hf_l0_kernel<STATS, 10>', 'hf_l0_kernel<STATS, HF_L0_MAX_K>',
                             'hf_rows_kernel<MODE, false>', 'hf_rows_kernel<MODE, true>', 'hf_wave_stats_kernel'], sites


# ---- the cases under the emulator ---------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('name', list(hk.WAVE_CASES))
def test_emu_wave_statistics(name):
    hk.wave_run(emu_cdll(), 'cpu', name)


@pytest.mark.parametrize('name', list(hk.L0_CASES))
def test_emu_layer0(name):
    hk.l0_run(emu_cdll(), 'cpu', name)


@pytest.mark.parametrize('name', list(hk.ROWS_CASES))
def test_emu_rows(name):
    hk.rows_run(emu_cdll(), 'cpu', name)


def test_emu_rows_gelu_on_every_finite_fp16_value():
    hk.gelu_exhaustive_run(emu_cdll(), 'cpu')


@pytest.mark.parametrize('name', list(hk.CMN_CASES))
def test_emu_time_mean_and_mask(name):
    hk.cmn_run(emu_cdll(), 'cpu', name)


def test_emu_entry_points_refuse_by_name_and_launch_nothing():
    hk.refusal_case(emu_cdll(), 'cpu')


def test_exports_present():
    for n in ('mv_hfenc_wave_stats', 'mv_hfenc_layer0_workspace_bytes', 'mv_hfenc_layer0', 'mv_hfenc_rows', 'mv_hfenc_cmn_mask'):
        assert n in _hip.EXPORTED_SYMBOLS and hasattr(emu_cdll(), n)
    assert emu_cdll().mv_abi_version() == 5


# ---- the pieces are what the forward runs ---------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('fixture', ['hf_wav2vec2_group', 'hf_wav2vec2_layer'])
def test_emu_forward_composed_from_its_pieces_has_the_forwards_bits(fixture):
    hk.composition_case(emu_cdll(), 'cpu', fixture)


def test_emu_varlen_forward_composed_from_its_pieces_has_the_forwards_bits():
    hk.composition_case(emu_cdll(), 'cpu', 'hf_wav2vec2_group', varlen=True)
