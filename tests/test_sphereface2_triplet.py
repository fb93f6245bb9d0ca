"""SphereFace2 and the triplet loss without a GPU: the kernels of csrc/sphereface2.hip and csrc/triplet.hip on the emulator build against the
fp64 oracles of tests/sphereface2_checks.py and tests/triplet_checks.py (tests/test_gpu_sphereface2_triplet.py runs the same checks on the
device), the reference's own results (tests/golden/margin_loss.npz), and what the library, the binding and the header agree on."""
import os

import numpy as np
import pytest

import sphereface2_checks as sfc
import triplet_checks as tpc
from helpers import GOLDEN


@pytest.fixture(scope='module')
def emu():
    import emu_lib
    return emu_lib.emu_cdll()


@pytest.fixture(scope='module')
def golden():
    return np.load(os.path.join(GOLDEN, 'margin_loss.npz'))


@pytest.mark.parametrize('t', sfc.TS)
@pytest.mark.parametrize('name', sfc.TYPES)
def test_emu_sphereface2_against_the_fp64_oracle(emu, name, t):
    sfc.check_type(emu, 'cpu', name, t)


def test_sphereface2_labels_reach_columns_0_last_and_both_sides_of_a_segment():
    sfc.check_labels_cover_the_columns()


def test_emu_sphereface2_half_inputs_are_the_fp32_path_on_the_upcast_logits(emu):
    sfc.check_half_inputs(emu, 'cpu')


def test_emu_sphereface2_in_place_backward(emu):
    sfc.check_in_place(emu, 'cpu')


def test_emu_sphereface2_no_hidden_state(emu):
    sfc.check_no_hidden_state(emu, 'cpu')


def test_emu_sphereface2_labels_out_of_range(emu):
    sfc.check_bad_labels(emu, 'cpu')


def test_emu_sphereface2_nan_logit(emu):
    sfc.check_nan_logit(emu, 'cpu')


def test_emu_sphereface2_refusals_by_name(emu):
    sfc.check_refusals(emu, 'cpu')


def test_emu_sphereface2_meets_the_reference_within_the_bound_of_its_fp32_front(emu, golden):
    sfc.check_golden(emu, 'cpu', golden)


# Every case the device runs, cut into items of one or two kernel runs each: the emulator runs a workgroup's threads as fibres and every
# cross-lane step as a rendezvous of them all, and (257, 513) -- 65 workgroups of 320 threads -- takes three to four seconds a run.
@pytest.mark.parametrize('normalize', (True, False))
@pytest.mark.parametrize('seed', tpc.SEEDS)
@pytest.mark.parametrize('pattern', tpc.PATTERNS)
@pytest.mark.parametrize('B,D', tpc.SHAPES)
def test_emu_triplet_against_the_fp64_oracle(emu, B, D, pattern, seed, normalize):
    tpc.check_shape(emu, 'cpu', B, D, seeds=(seed,), patterns=(pattern,), normalizes=(normalize,), halves=())


@pytest.mark.parametrize('dtype', ('float16', 'bfloat16'))
@pytest.mark.parametrize('pattern', ('pairs', 'singleton'))
@pytest.mark.parametrize('B,D', tpc.SHAPES)
def test_emu_triplet_16_bit_features(emu, B, D, pattern, dtype):
    import torch
    tpc.check_shape(emu, 'cpu', B, D, seeds=(), patterns=(pattern,), halves=(getattr(torch, dtype),))


def test_triplet_oracle_is_autograd_of_the_torch_expression():
    tpc.check_against_torch_autograd()


def test_emu_triplet_no_hidden_state(emu):
    tpc.check_no_hidden_state(emu, 'cpu')


def test_emu_triplet_zero_norm_row(emu):
    tpc.check_zero_norm_row(emu, 'cpu')


def test_emu_triplet_refusals_by_name(emu):
    tpc.check_refusals(emu, 'cpu')


def test_emu_triplet_meets_the_reference(emu, golden):
    tpc.check_golden(emu, 'cpu', golden)


def test_the_library_exports_sphereface2_and_triplet(emu):
    import ctypes
    import __graft_entry__
    from mvector import _hip
    cdll = ctypes.CDLL(__graft_entry__.build())
    header = open(os.path.join(os.path.dirname(os.path.abspath(__graft_entry__.__file__)), 'include', 'mvector_hip.h')).read()
    for name in ('mv_sphereface2_workspace_bytes', 'mv_sphereface2_forward', 'mv_sphereface2_backward', 'mv_triplet_workspace_bytes',
                 'mv_triplet_forward', 'mv_triplet_backward'):
        assert hasattr(cdll, name) and hasattr(emu, name) and name in _hip.EXPORTED_SYMBOLS and name + '(' in header, name
    for macro in ('MV_SF2_TYPE_C', 'MV_SF2_TYPE_A', 'MV_SF2_MAX_T', 'MV_SF2_SAVED', 'MV_TRIPLET_MAX_B', 'MV_TRIPLET_MAX_D', 'MV_TRIPLET_ANCHORS',
                  'MV_MARGIN_SEG', 'MV_MARGIN_CHUNK'):
        assert f'#define {macro} {getattr(_hip, macro)}\n' in header, macro
    cdll.mv_abi_version.restype = ctypes.c_int
    assert cdll.mv_abi_version() == 5


def test_cpu_tensors_run_the_torch_expression_and_leave_pred_empty():
    import torch
    from mvector import loss as L
    inputs = {'features': torch.randn(4, 8), 'logits': torch.rand(4, 12) * 1.8 - 0.9}
    labels = torch.tensor([0, 0, 3, 3])
    for module in (L.SphereFace2(), L.TripletAngularMarginLoss()):
        assert torch.isfinite(module(inputs, labels)) and module.pred is None
