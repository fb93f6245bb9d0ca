"""csrc/hfencoder.hip on the MI355X, one kernel at a time: the cases of tests/hf_kernel_checks.py through the layer-level entry points of the product
library -- every output element within its derived bound of the fp64 reference, nothing written outside the result -- the refusals, and the
forward composed from its pieces, bit for bit.  Each case prints its largest |got - ref| / bound (`pytest -s`; profiles/hf_kernels_gpu.log)."""
import pytest

import hf_kernel_checks as hk

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'


def _lib():
    from mvector import _hip
    return _hip.lib()


@pytest.mark.parametrize('name', list(hk.WAVE_CASES))
def test_gpu_wave_statistics(name):
    hk.wave_run(_lib(), DEV, name)


@pytest.mark.parametrize('name', list(hk.L0_CASES))
def test_gpu_layer0(name):
    hk.l0_run(_lib(), DEV, name)


@pytest.mark.parametrize('name', list(hk.ROWS_CASES))
def test_gpu_rows(name):
    hk.rows_run(_lib(), DEV, name)


def test_gpu_rows_gelu_on_every_finite_fp16_value():
    hk.gelu_exhaustive_run(_lib(), DEV)


@pytest.mark.parametrize('name', list(hk.CMN_CASES))
def test_gpu_time_mean_and_mask(name):
    hk.cmn_run(_lib(), DEV, name)


def test_gpu_entry_points_refuse_by_name_and_launch_nothing():
    hk.refusal_case(_lib(), DEV)


@pytest.mark.parametrize('fixture', ['hf_wav2vec2_group', 'hf_wav2vec2_layer'])
def test_gpu_forward_composed_from_its_pieces_has_the_forwards_bits(fixture):
    hk.composition_case(_lib(), DEV, fixture)


def test_gpu_varlen_forward_composed_from_its_pieces_has_the_forwards_bits():
    hk.composition_case(_lib(), DEV, 'hf_wav2vec2_group', varlen=True)
