"""mv_fbank_create and the mv_fbank_forward* entry points of the product library on the MI355X: every refusal's code and message, which message
wins when two fields are wrong, and the two returns that are not refusals.  All host checks that return before any launch.  Cases:
tests/fbank_refusal_cases.py."""
import pytest

import fbank_refusal_cases as rc

pytestmark = pytest.mark.gpu


def product_lib():
    from mvector import _hip
    return _hip.lib()


@pytest.mark.parametrize('idx', range(len(rc.CREATE_CASES)), ids=[c[0] for c in rc.CREATE_CASES])
def test_gpu_fbank_create_refuses(idx):
    rc.check_create(product_lib(), idx)


@pytest.mark.parametrize('idx', range(len(rc.FORWARD_CASES)), ids=[c[0] for c in rc.FORWARD_CASES])
def test_gpu_fbank_forward_refuses(idx):
    rc.check_forward(product_lib(), 'cuda', idx)
