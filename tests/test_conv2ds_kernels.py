"""conv2ds, CPU tier: the per-element bound's self-checks, the launch plan of every pinned case and of the production layer shapes
(mv_conv2ds_plan_info on the emulator build of the library: nothing is launched), and the pinned cases and same-bits groups of
tests/conv2ds_cases.py under the SIMT emulator.  The device tier is tests/test_gpu_conv2ds_kernels.py."""
import ctypes
import os
import re

import pytest
import torch

import conv2ds_cases as cc
import layer_checks as lc
from emu_lib import emu_cdll
from mvector import _hip

SLOW = os.environ.get('MV_SLOW_EMU') == '1'
BOUNDED = [n for n in cc.PINNED if 'nan_at' not in cc.PINNED[n]['cfg']]
CROSS_TERM_MAX_K = 64     # up to this cin * ks^2 the accumulation term is small enough for the bound to see a missing Wlo.Xhi


# ---- the bound, on the CPU alone ----------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('name', BOUNDED)
def test_bound_admits_the_fp32_model_and_sees_a_dropped_product_and_a_dropped_cross_term(name):
    """No kernel: the three-term sum and the epilogue evaluated in fp32 stay within the derived bound of the fp64 reference on the case's own
    operands; a reference without one whole product does not, and one without the Wlo.Xhi term does not either where cin * ks^2 <= 64."""
    o = cc.operands(name)
    ref, bnd, ref2, bnd2 = cc.reference(o)
    assert torch.isfinite(ref).all() and bool((bnd > 0).all())
    y, y2 = cc.model32(o)
    mx, mean, med = cc.ratios(y, ref, bnd)
    print(f'{name}: cin * ks^2 = {o.cin * o.ks * o.ks}, fp32 model max ratio {mx:.3f} mean {mean:.3f}, median bound {med:.2e}')
    assert mx <= 1.0, (name, mx)
    if y2 is not None:
        assert cc.ratios(y2, ref2, bnd2)[0] <= 1.0, name
    wrong = cc.ratios(cc.reference(o, drop='product')[0], ref, bnd)[0]
    assert wrong > 1.0, (name, wrong)
    cross = cc.ratios(cc.reference(o, drop='cross')[0], ref, bnd)[0]
    print(f'{name}: dropped product {wrong:.1f}, without Wlo.Xhi {cross:.2f}')
    if o.cin * o.ks * o.ks <= CROSS_TERM_MAX_K:
        assert cross > 1.0, (name, cross)


def test_some_pinned_cases_are_small_enough_to_see_the_cross_term():
    small = [n for n in BOUNDED if (lambda c: c.get('cin', 16) * c.get('ks', 3) ** 2)(cc.PINNED[n]['cfg']) <= CROSS_TERM_MAX_K]
    assert len(small) >= 20, small


def test_split_error_bounds_the_store():
    x = torch.cat([torch.linspace(-1100.0, 1100.0, 200001), torch.linspace(-2.0, 2.0, 200001), torch.linspace(-1e-4, 1e-4, 20001)])
    r = x.clamp(-cc.SAT, cc.SAT)
    assert bool(((cc.store16(r) - r.double()).abs() <= cc.split_error(r.double().abs())).all())
    assert cc.split_error(torch.tensor([0.0], dtype=torch.float64)).item() == 2.0 ** -25 / 64.0


@pytest.mark.parametrize('name', ['peak_second_out_b1', 'peak_second_out_b2', 'peak_second_out_b3'])
def test_peak_cases_have_the_larger_map_in_the_second_output(name):
    ref, _, ref2, _ = cc.reference(cc.operands(name))
    assert ref2.abs().max().item() > 1.5 * ref.abs().max().item()


# ---- the plan -----------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('name', list(cc.PINNED))
def test_pinned_case_plans_its_row_on_every_chip(name):
    want = cc.PINNED[name]['expect']
    for cus, plan in cc.plans(emu_cdll(), name).items():
        got = {k: plan[k] for k in want}
        assert got == want, (name, cus, plan)


def _table_rows():
    with open(os.path.join(os.path.dirname(_hip.__file__), '..', 'csrc', 'conv2ds.hip')) as f:
        src = f.read()
    table = src[src.index('const CsKernelRow CS_KERNELS[] = {'):src.index('#undef MV_CS_ROW')]
    return [f'conv2ds_kernel<{m}>' for m in re.findall(r'MV_CS_ROW\((\d, \d, \d, \d+, (?:true|false))\)', table)]


def test_every_row_of_the_kernel_table_is_pinned_or_unreachable():
    rows = _table_rows()
    pinned = {c['expect']['kernel'] for c in cc.PINNED.values()}
    assert len(rows) == 40 and len(set(rows)) == 40
    assert not pinned & set(cc.UNREACHABLE) and pinned | set(cc.UNREACHABLE) == set(rows), sorted(set(rows) ^ (pinned | set(cc.UNREACHABLE)))
    for row, (cfg, message) in cc.UNREACHABLE.items():
        with pytest.raises(RuntimeError, match=message):
            lc.conv2ds_case(emu_cdll(), 'cpu', plan_cus=(256,), **cfg)
    # what is no row cannot be asked for either
    for (ks, nbw, spw), message in cc.NOT_ROWS.items():
        assert cc.kernel_name(ks, nbw, spw, False) not in rows
        with pytest.raises(RuntimeError, match=re.escape(message)):
            lc.conv2ds_case(emu_cdll(), 'cpu', ks=ks, cin=32, cout=16 * nbw, nbw=nbw, spw=spw, plan_cus=(256,))


def test_every_epilogue_runs_with_one_and_with_several_blocks_per_wave():
    seen = {(epi, min(c['expect']['nbw'], 2)) for n, c in cc.PINNED.items() if n.startswith('row_') for epi in cc.EPILOGUES if n.endswith('_' + epi)}
    assert seen == {(epi, b) for epi in cc.EPILOGUES for b in (1, 2)}
    nan = {min(cc.PINNED[n]['expect']['nbw'], 2) for n in cc.PINNED if n.startswith('nan_')}
    assert nan == {2}     # (one block per wave: S16_RANGE_CASES of test_emu_kernels.py / test_gpu_parity.py)


@pytest.mark.parametrize('name', cc.WALKS)
def test_walk_cases_walk(name):
    """each workgroup walks at least three tiles, some stop a round early, and the ring carries across an utterance boundary"""
    cfg, p = cc.PINNED[name]['cfg'], cc.plans(emu_cdll(), name, cus=(256,))[256]
    ptiles = cfg['B'] * p['tiles']
    assert cfg['B'] >= 2 and ptiles // p['wg_per_ct'] >= 3 and ptiles % p['wg_per_ct'] != 0 and p['tiles'] % p['wg_per_ct'] != 0, p


def test_walk_cases_cover_the_ring_depths_and_stage_counts():
    seen = {}
    for name in cc.WALKS:
        e = cc.PINNED[name]['expect']
        ks, spt, ns = int(e['kernel'][len('conv2ds_kernel<')]), e['stages_per_tile'], e['ns']
        seen.setdefault((ks, e['track']), set()).add(ns)
        seen.setdefault(('stages', ks), set()).update(what for what, holds in (('one', spt == 1), ('ns - 1', spt == ns - 1), ('> ns', spt > ns)) if holds)
    for ks, deepest in ((1, 3), (3, 4)):
        assert seen[('stages', ks)] == {'one', 'ns - 1', '> ns'}, seen
        for track in (0, 1):
            assert seen[(ks, track)] == set(range(2, deepest + 1)), seen
        # the deepest ring is the launcher's maximum: a deeper one is refused
        big = next(n for n in cc.WALKS if cc.PINNED[n]['expect']['ns'] == deepest and cc.PINNED[n]['expect']['kernel'].startswith(f'conv2ds_kernel<{ks}'))
        with pytest.raises(RuntimeError, match='no launch shape fits'):
            lc.conv2ds_case(emu_cdll(), 'cpu', plan_cus=(256,), **dict(cc.PINNED[big]['cfg'], ring=deepest + 1))


def test_producer_forms():
    e = lambda n: cc.PINNED[n]['expect']
    assert {e(n)['nprod'] for n in cc.PINNED} >= {1, 2, 3, 4}
    for name, transfers in (('producers_2_padded', 15), ('producers_4_padded', 15)):     # 5 patch rows x 3 column groups of 8
        assert e(name)['nprod'] * e(name)['pp'] > transfers and transfers % e(name)['nprod'] != 0
    for name in ('six_consumers_two_producers', 'six_consumers_four_stages'):
        assert (e(name)['nbw'], e(name)['ncons'], e(name)['nprod']) == (2, 6, 2) and e(name)['stages_per_tile'] <= 4


def test_unpinned_cases_move_with_the_chip():
    """why the cases pin: CONV2DS_CASES[14] (3x3 48 -> 48 on 21 x 50, no hints) runs tiles of 8 rows on the emulator's 8 compute units and of 3 rows
    on the MI355X; CONV2DS_CASES[18] ("shortest ring") walks 9 tiles per workgroup there and one tile per workgroup here"""
    p = lc.conv2ds_case(emu_cdll(), 'cpu', plan_cus=(8, 256), **lc.CONV2DS_CASES[14])
    assert (p[8]['rows'], p[256]['rows']) == (8, 3) and p[8]['kernel'] == p[256]['kernel']
    p = lc.conv2ds_case(emu_cdll(), 'cpu', plan_cus=(8, 256), **lc.CONV2DS_CASES[18])
    assert (p[8]['wg_per_ct'], 2 * p[8]['tiles']) == (8, 18) and (p[256]['wg_per_ct'], 2 * p[256]['tiles']) == (48, 48)
    # ... and wg_hint takes the chip out of it, without touching anything else
    q = lc.conv2ds_case(emu_cdll(), 'cpu', plan_cus=(8, 256), **dict(lc.CONV2DS_CASES[18], rows=3, wg=5))
    assert q[8] == q[256] and q[256]['wg_per_ct'] == 5 and {k: v for k, v in q[256].items() if k not in ('wg_per_ct', 'grid')} == \
        {k: v for k, v in p[256].items() if k not in ('wg_per_ct', 'grid')}


def test_plan_info_refuses_what_the_forward_refuses():
    cdll = emu_cdll()
    plan = lambda **cfg: lc.conv2ds_case(cdll, 'cpu', plan_cus=(256,), **cfg)
    with pytest.raises(RuntimeError, match='wg_hint must be 0'):
        plan(wg=-1)
    with pytest.raises(RuntimeError, match='blocks per wave must be 1..3'):
        plan(nbw=4)
    with pytest.raises(RuntimeError, match='rows per tile must be 1..8'):
        plan(rows=9)
    with pytest.raises(RuntimeError, match='channel tile too wide'):
        plan(cout=208, ct=13, nbw=1)
    with pytest.raises(RuntimeError, match='kernel 1 or 3, stride 1 or 2'):
        plan(stride=3)
    d = cc.production_desc(cc.PRODUCTION_MODELS['eres2net'][0]['layer1.0.conv1'], 8)
    info = _hip.MvConv2dsPlanInfo()
    assert cdll.mv_conv2ds_plan_info(None, 0, ctypes.byref(info)) != 0 and b'null argument' in cdll.mv_last_error()
    assert cdll.mv_conv2ds_plan_info(ctypes.byref(d), 0, None) != 0 and b'null argument' in cdll.mv_last_error()
    assert cdll.mv_conv2ds_plan_info(ctypes.byref(d), -1, ctypes.byref(info)) != 0 and b'cus must be' in cdll.mv_last_error()
    d.wg_hint = -1      # the forward says the same, before it launches anything
    assert cdll.mv_conv2ds_forward(ctypes.byref(d), None) != 0 and b'wg_hint must be 0' in cdll.mv_last_error()
    d.wg_hint = 0
    # cus = 0 is the device at hand: the emulator's chip
    assert _hip.conv2ds_plan_info(d, 0, cdll) == _hip.conv2ds_plan_info(d, 8, cdll)


PRODUCTION = cc.load_production_plan()


def test_production_table_covers_the_models_and_batches():
    assert set(PRODUCTION) == set(cc.production_keys())


@pytest.mark.parametrize('model', list(cc.PRODUCTION_MODELS))
def test_plan_at_production_shapes_on_256_compute_units(model):
    for key in cc.production_keys():
        if key[0] == model:
            assert cc.production_plan(emu_cdll(), *key) == PRODUCTION[key], key


def test_every_instantiation_the_models_run_is_pinned():
    pinned = {c['expect']['kernel'] for c in cc.PINNED.values()}
    assert {'conv2ds_kernel' + v[0] for v in PRODUCTION.values()} <= pinned
    tracked = {k[0] for k, v in PRODUCTION.items() if v[0].endswith('true>')}
    assert tracked == {'resnet_se', 'res2net', 'campp_head'}


# ---- the pinned cases and the same-bits groups under the emulator ----------------------------------------------------------------------------------

@pytest.mark.parametrize('name', list(cc.PINNED))
def test_emu_pinned_case(name):
    if name in cc.SLOW_EMU and not SLOW:
        pytest.skip('10 s and more under the emulator; set MV_SLOW_EMU=1 (runs on the GPU in test_gpu_conv2ds_kernels)')
    cc.run(emu_cdll(), 'cpu', name)


@pytest.mark.parametrize('name', list(cc.SAME_BITS))
def test_emu_launch_shapes_give_the_same_bits(name):
    if name in cc.SLOW_EMU_SAME_BITS and not SLOW:
        pytest.skip('10 s and more under the emulator; set MV_SLOW_EMU=1 (runs on the GPU in test_gpu_conv2ds_kernels)')
    cc.same_bits_case(emu_cdll(), 'cpu', name)
