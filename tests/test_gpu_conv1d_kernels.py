"""conv1d on the MI355X, one row of the kernel table at a time: the pinned cases of tests/conv1d_cases.py -- the row asserted from
mv_conv1d_plan_info for the device before the launch, conv1d_case's structural assertions, every output element within its derived bound of the
fp64 reference -- the grouped ring kernel, and the one accumulation order of the tile families (the same bits whatever the tile).  Each case prints
its row, max and mean ratio and median bound (`pytest -s`; profiles/conv1d_kernels_gpu.log)."""
import pytest

import conv1d_cases as cc
import ecapa_variant_checks as ev

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'


def _lib():
    from mvector import _hip
    return _hip.lib()


@pytest.mark.parametrize('name', list(cc.PINNED))
def test_gpu_pinned_case_runs_its_row_within_the_bound(name):
    cc.run(_lib(), DEV, name)


def test_gpu_grouped_ring_kernel_within_the_bound():
    assert ev.grouped_conv_case(_lib(), DEV, bound=True, expect_kernel=cc.GROUPED['kernel'], log=print, **cc.GROUPED['cfg'])


@pytest.mark.parametrize('name', list(cc.SAME_BITS))
def test_gpu_tile_families_give_the_same_bits(name):
    """conv1d_plan: "Every tile family accumulates in one order, so a different choice gives the same bits" -- held here at the layer"""
    cc.same_bits_case(_lib(), DEV, name)
