"""mv_fbank_create and the mv_fbank_forward* entry points on the emulator build: every refusal's code and message, which message wins when two
fields are wrong, and the two returns that are not refusals (no rows, no frames).  Cases: tests/fbank_refusal_cases.py."""
import pytest

import fbank_refusal_cases as rc
from emu_lib import emu_cdll


@pytest.mark.parametrize('idx', range(len(rc.CREATE_CASES)), ids=[c[0] for c in rc.CREATE_CASES])
def test_emu_fbank_create_refuses(idx):
    rc.check_create(emu_cdll(), idx)


@pytest.mark.parametrize('idx', range(len(rc.FORWARD_CASES)), ids=[c[0] for c in rc.FORWARD_CASES])
def test_emu_fbank_forward_refuses(idx):
    rc.check_forward(emu_cdll(), 'cpu', idx)
