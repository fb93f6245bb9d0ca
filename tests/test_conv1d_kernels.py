"""conv1d, CPU tier: the per-element bound's self-checks, the launch plan of every pinned case and of the production layer shapes
(mv_conv1d_plan_info on the emulator build of the library: nothing is launched), and the pinned cases of tests/conv1d_cases.py under the SIMT
emulator.  The device tier is tests/test_gpu_conv1d_kernels.py."""
import ctypes
import os
import re

import pytest
import torch

import conv1d_cases as cc
import ecapa_variant_checks as ev
import layer_checks as lc
from emu_lib import emu_cdll
from mvector import _hip

SLOW = os.environ.get('MV_SLOW_EMU') == '1'


# ---- the bound, on the CPU alone ----------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('name', list(cc.PINNED))
def test_bound_admits_the_fp32_rounding_model_and_sees_a_dropped_product(name):
    """No kernel: the fp32 evaluation rounded to fp16 (the layer checks' reference so far) stays within the derived bound of the fp64 reference
    on the case's own inputs; a reference without the product of the last input channel at tap 0 does not."""
    o = cc.operands(name)
    ref64, bnd = cc.reference(o)
    assert torch.isfinite(ref64).all() and bool((bnd > 0).all())
    mx, mean, med = cc.ratios(cc.model32(o), ref64, bnd)
    print(f'{name}: cin * k = {o.cin * o.k}, fp32 model max ratio {mx:.3f} mean {mean:.3f}, median bound {med:.2e}')
    assert mx <= 1.0, (name, mx)
    wrong, _, _ = cc.ratios(cc.reference(o, drop_term=True)[0], ref64, bnd)
    assert wrong > 1.0, (name, wrong)


def test_half_ulp_of_fp16():
    v = torch.tensor([0.0, 2.0 ** -26, 2.0 ** -14, 1.0, 1.5, 2.0, 1000.0, 65504.0], dtype=torch.float64)
    want = torch.tensor([2.0 ** -25, 2.0 ** -25, 2.0 ** -25, 2.0 ** -11, 2.0 ** -11, 2.0 ** -10, 2.0 ** -2, 2.0 ** 4], dtype=torch.float64)
    assert torch.equal(cc.half_ulp_fp16(v), want)
    x = torch.cat([torch.linspace(-70000.0, 70000.0, 200001), torch.linspace(-2.0, 2.0, 200001), torch.linspace(-1e-4, 1e-4, 20001)])
    r = x.clamp(-65504.0, 65504.0)     # (fp32 values: one rounding on the way to fp16)
    assert bool(((r.half().double() - r.double()).abs() <= cc.half_ulp_fp16(r.double().abs())).all())


# ---- the plan -----------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('name', list(cc.PINNED))
def test_pinned_case_plans_its_row_on_every_chip(name):
    want = cc.PINNED[name]['expect']
    for cus, plan in cc.plans(emu_cdll(), name).items():
        got = {k: plan[k] for k in want}
        assert got == want, (name, cus, plan)


def test_grouped_case_plans_the_grouped_ring_kernel_on_every_chip():
    for cus in cc.PLAN_CUS:
        assert ev.grouped_conv_case(emu_cdll(), 'cpu', plan_cus=cus, **cc.GROUPED['cfg'])['kernel'] == cc.GROUPED['kernel'], cus


def test_every_row_of_the_kernel_table_is_pinned():
    named = {cc.GROUPED['kernel']}
    for c in cc.PINNED.values():
        named |= {c['expect']['kernel'], c['expect']['in_stats_kernel'], c['expect']['tail_kernel']} - {''}
    with open(os.path.join(os.path.dirname(_hip.__file__), '..', 'csrc', 'conv1d.hip')) as f:
        src = f.read()
    enum = src[src.index('enum ConvKernel {'):src.index('CK_COUNT')]
    rows = set(re.findall(r'\bCK_[A-Z0-9_]+', enum))
    assert len(rows) == 16 and named == rows, sorted(rows ^ named)


def test_unpinned_cases_move_with_the_chip():
    """why the cases pin: CONV_CASES[24] (input statistics, 3 utterances of 298 frames, tile 0) is two launches on the MI355X and the fused kernel
    on the emulator's 8 compute units; twenty such utterances do the same on a quarter of the MI355X"""
    p = lc.conv1d_case(emu_cdll(), 'cpu', seed=24, plan_cus=(8, 256), **lc.CONV_CASES[24])
    assert (p[8]['in_stats_kernel'], p[8]['kernel']) == ('', 'CK_GLDS_160_IN_STATS')
    assert (p[256]['in_stats_kernel'], p[256]['kernel']) == ('CK_IN_STATS', 'CK_GLDS_64')
    p = lc.conv1d_case(emu_cdll(), 'cpu', seed=24, plan_cus=(64, 256), **dict(lc.CONV_CASES[24], B=20))
    assert (p[64]['in_stats_kernel'], p[64]['kernel']) == ('', 'CK_GLDS_160_IN_STATS')
    assert (p[256]['in_stats_kernel'], p[256]['kernel']) == ('CK_IN_STATS', 'CK_GLDS_64')


def test_plan_info_refuses_what_the_forward_refuses():
    cdll = emu_cdll()
    with pytest.raises(RuntimeError, match='reflect padding needs pad < T_in'):
        lc.conv1d_case(cdll, 'cpu', T=3, k=3, dil=4, plan_cus=(256,))
    with pytest.raises(RuntimeError, match='256-wide tiles need the plain fp16 path'):
        lc.conv1d_case(cdll, 'cpu', tile=256, plan_cus=(256,))
    with pytest.raises(RuntimeError, match='fused time statistics need the persistent 1x1 kernel'):
        lc.conv1d_case(cdll, 'cpu', stats=1, plan_cus=(256,))
    d = cc.production_desc('ecapa_block_1x1', 8)
    info = _hip.MvConv1dPlanInfo()
    assert cdll.mv_conv1d_plan_info(None, 1, 0, ctypes.byref(info)) != 0 and b'null argument' in cdll.mv_last_error()
    assert cdll.mv_conv1d_plan_info(ctypes.byref(d), 1, -1, ctypes.byref(info)) != 0 and b'cus must be' in cdll.mv_last_error()
    assert cdll.mv_conv1d_plan_info(ctypes.byref(d), 0, 256, ctypes.byref(info)) != 0 and b'groups must be positive' in cdll.mv_last_error()
    assert cdll.mv_conv1d_plan_info(ctypes.byref(d), 3, 256, ctypes.byref(info)) != 0 and b'divisible by groups' in cdll.mv_last_error()
    # cus = 0 is the device at hand: the emulator's chip
    assert _hip.conv1d_plan_info(d, 1, 0, cdll) == _hip.conv1d_plan_info(d, 1, 8, cdll)


@pytest.mark.parametrize('key', list(cc.PRODUCTION_PLAN), ids=lambda k: f'{k[0]}-B{k[1]}')
def test_plan_at_production_shapes_on_256_compute_units(key):
    assert cc.production_plan(emu_cdll(), *key) == cc.PRODUCTION_PLAN[key]


def test_production_table_covers_the_stated_batches():
    want = {(n, B) for n in cc.PRODUCTION_LAYERS for B in (cc.CAMPP_BATCHES if n.startswith('campp') else cc.ECAPA_BATCHES)}
    assert set(cc.PRODUCTION_PLAN) == want


# ---- the pinned cases under the emulator ------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('name', list(cc.PINNED))
def test_emu_pinned_case(name):
    if name in cc.SLOW_EMU and not SLOW:
        pytest.skip('10 to 20 s under the emulator; set MV_SLOW_EMU=1 (runs on the GPU in test_gpu_conv1d_kernels)')
    cc.run(emu_cdll(), 'cpu', name)


def test_emu_grouped_ring_kernel_within_the_bound():
    assert ev.grouped_conv_case(emu_cdll(), 'cpu', bound=True, expect_kernel=cc.GROUPED['kernel'], **cc.GROUPED['cfg'])


@pytest.mark.parametrize('name', list(cc.SAME_BITS))
def test_emu_tile_families_give_the_same_bits(name):
    cc.same_bits_case(emu_cdll(), 'cpu', name)
