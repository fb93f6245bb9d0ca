"""conv2ds on the MI355X, one row of the kernel table at a time: the pinned cases of tests/conv2ds_cases.py -- the row and the launch shape asserted
from mv_conv2ds_plan_info for the device before the launch, conv2ds_case's assertions (the 2e-5 x scale tolerance, sentinels, peak word, NaNs),
every output element within its derived bound of the fp64 reference -- and the one sum of every launch shape (the same S16 words and peak bits
whatever the blocks per wave, pixel groups, rows, ring, producers, channel tiles and workgroups).  Each case prints its row, max and mean ratio
and median bound (`pytest -s`; profiles/conv2ds_kernels_gpu.log)."""
import pytest

import conv2ds_cases as cc

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'


def _lib():
    from mvector import _hip
    return _hip.lib()


@pytest.mark.parametrize('name', list(cc.PINNED))
def test_gpu_pinned_case_runs_its_row_within_the_bound(name):
    cc.run(_lib(), DEV, name)


@pytest.mark.parametrize('name', list(cc.SAME_BITS))
def test_gpu_launch_shapes_give_the_same_bits(name):
    """conv2ds.hip: "none changes a bit of the result -- every output element is the same K-ordered sum in every shape" -- held here at the layer"""
    cc.same_bits_case(_lib(), DEV, name)
