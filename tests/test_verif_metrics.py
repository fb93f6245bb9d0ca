"""Verification metrics without a GPU: the host restatement of metrics.verification_metrics against fixtures written by the REFERENCE's own
metrics.py (tools/make_verif_metrics_golden.py), and the kernels of csrc/verif.hip on the emulator build with CPU tensors.  The same kernel
checks run on the device in tests/test_gpu_verif_metrics.py (tests/verif_metric_checks.py holds them)."""
import numpy as np
import pytest

import verif_metric_checks as vc


@pytest.fixture(scope='module')
def emu():
    import emu_lib
    return emu_lib.emu_cdll()


# ------------------------------------------------------------------ the host restatement vs the reference's fixtures
@pytest.mark.parametrize('name', vc.CASES)
def test_host_restatement_equals_the_reference(name):
    vc.check_golden_public(None, name)


def test_host_restatement_equals_the_existing_functions_without_cross_label_ties():
    from mvector.metric import metrics
    scores, tl, el, _ = vc.case('costs')
    flat, labels = scores.reshape(-1), (tl[:, None] == el[None, :]).astype(np.int32).reshape(-1)
    fnr, fpr, _ = metrics.compute_fnr_fpr(flat, labels)
    eer, thr = metrics.compute_eer(fnr, fpr, flat)
    assert metrics.verification_metrics(scores, tl, el) == (float(eer), float(metrics.compute_dcf(fnr, fpr)), float(thr))


def test_host_edges_raise_the_documented_exceptions():
    vc.check_edges_public(None)


# ------------------------------------------------------------------ the kernels on the emulator
def test_emu_sort_tile_is_what_the_sizes_assume(emu):
    assert vc.sort_tile(emu) == 4096


@pytest.mark.parametrize('n', vc.sort_sizes(4096))
def test_emu_sort_scores(emu, n):
    vc.check_sort(emu, 'cpu', n)


@pytest.mark.parametrize('name', vc.CASES)
def test_emu_metrics_equal_the_reference(emu, name):
    vc.check_golden(emu, 'cpu', name)


def test_emu_cross_label_ties_follow_the_flat_index(emu):
    vc.check_cross_label_ties(emu, 'cpu')


def test_emu_edges_and_refusals(emu):
    vc.check_edges_raw(emu, 'cpu')


def test_emu_transposed_matrix_gives_the_same_metrics(emu):
    vc.check_transpose_invariance(emu, 'cpu')
