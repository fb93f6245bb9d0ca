"""The time reductions and element-wise row passes of csrc/pool.hip, one kernel at a time, under the SIMT emulator: every launcher the model forwards
call through its layer-level entry point, against an fp64 reference of the same operation (tests/layer_checks.py: the bars are derived there).
tests/test_gpu_pool_rows.py runs the same case functions on the device."""
import os
import subprocess
import sys

import pytest

import layer_checks as lc
from emu_lib import emu_cdll

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = 'cpu'

# T around every boundary of the 16-row phases and of the four-rows-in-flight loop (t + 48 < T); C = 264: one active lane in the last channel group,
# C = 261: five channels in the last lane, on the scalar path
TS_T = [1, 15, 16, 17, 48, 49, 113, 298]
TS_C = [(264, 272), (261, 272)]
SEG = [(1, 100), (100, 100), (101, 100), (250, 100), (30, 7)]
CAST_F = [8, 80, 13, 201]
CAST_PAD = ['0', '2', 'T-1']
CAST_ROWS = [(13, 16), (80, 80), (201, 208)]
PAD_ROWS = [(1, 8), (7, 8), (13, 16), (201, 208), (257, 264), (13, 20), (16, 16)]


def _pad(kind, T=9):
    return {'0': 0, '2': 2, 'T-1': T - 1}[kind]


@pytest.mark.parametrize('C,ld', TS_C)
@pytest.mark.parametrize('T', TS_T)
def test_emu_time_stats_edges(T, C, ld):
    lc.time_stats_ex_case(emu_cdll(), DEV, B=2, T=T, C=C, ld=ld)
    if T > 1:
        lc.time_stats_ex_case(emu_cdll(), DEV, B=2, T=T, C=C, ld=ld, unbiased=1, eps=0.0, seed=1)


def test_emu_time_stats_three_forms_on_the_same_rows():
    """(2050 workgroups: half a minute under the emulator, whatever T is -- the large-grid forms' NaN channels ride in this call's data; the bitwise
    NaN comparison of the large grid runs on the device only)"""
    lc.time_stats_forms_case(emu_cdll(), DEV)


@pytest.mark.parametrize('C', [264, 261])
@pytest.mark.parametrize('out_pad', [0, 8])
def test_emu_time_stats_preactivation_and_output_pitch(out_pad, C):
    lc.time_stats_preact_case(emu_cdll(), DEV, C=C, out_pad=out_pad)


@pytest.mark.parametrize('C,pre', [(264, False), (261, False), (261, True)])
def test_emu_time_stats_nan_frame(C, pre):
    lc.time_stats_nan_case(emu_cdll(), DEV, C=C, pre=pre)


def test_emu_time_stats_row_bits_do_not_depend_on_the_batch_size():
    lc.time_stats_batch_rows_case(emu_cdll(), DEV)


def test_emu_time_stats_refusals():
    m = lc.time_stats_refusal_case(emu_cdll(), DEV)
    assert 'unbiased' in m[0] and 'output leading dimension' in m[1] and '16-byte aligned' in m[2], m


@pytest.mark.parametrize('C', [8, 136])
@pytest.mark.parametrize('T,seg_len', SEG)
def test_emu_seg_mean(T, seg_len, C):
    lc.seg_mean_case(emu_cdll(), DEV, T=T, seg_len=seg_len, C=C)


def test_emu_seg_mean_nan_and_batch_rows():
    lc.seg_mean_nan_case(emu_cdll(), DEV)
    lc.seg_mean_batch_rows_case(emu_cdll(), DEV)


@pytest.mark.parametrize('own', [False, True], ids=['slices', 'own'])
def test_emu_se_gate_residual(own):
    lc.se_gate_residual_case(emu_cdll(), DEV, own=own)


def test_emu_se_gate_residual_ragged_last_workgroup():
    lc.se_gate_residual_case(emu_cdll(), DEV, B=1, T=29, C=72)     # 261 groups of 8: one full workgroup and five lanes of a second


@pytest.mark.parametrize('where', ['y', 'res', 'gate'])
def test_emu_se_gate_residual_nan(where):
    lc.se_gate_nan_case(emu_cdll(), DEV, where)


def test_emu_se_gate_residual_row_bits_do_not_depend_on_the_batch_size():
    lc.se_gate_batch_rows_case(emu_cdll(), DEV)


@pytest.mark.parametrize('A', [8, 136])
def test_emu_asp_hidden_act(A):
    lc.asp_hidden_act_case(emu_cdll(), DEV, A=A)
    lc.asp_hidden_nan_case(emu_cdll(), DEV, A=A)


@pytest.mark.parametrize('nan', [False, True], ids=['', 'nan'])
@pytest.mark.parametrize('pad_kind', CAST_PAD)
@pytest.mark.parametrize('F', CAST_F)
def test_emu_cast_pad(F, pad_kind, nan):
    lc.cast_pad_case(emu_cdll(), DEV, F=F, pad=_pad(pad_kind), nan=nan)


@pytest.mark.parametrize('nan', [False, True], ids=['', 'nan'])
@pytest.mark.parametrize('C,ldd', CAST_ROWS)
def test_emu_cast_rows(C, ldd, nan):
    lc.cast_rows_case(emu_cdll(), DEV, C=C, ldd=ldd, nan=nan)


def test_emu_copy_slice():
    lc.copy_slice_case(emu_cdll(), DEV)


@pytest.mark.parametrize('F,ldd', PAD_ROWS)
def test_emu_pad_rows_f32(F, ldd):
    lc.pad_rows_f32_case(emu_cdll(), DEV, F=F, ldd=ldd)


def test_emu_bn_relu_rows_keeps_nan():
    lc.bn_relu_rows_nan_case(emu_cdll(), DEV)


def test_emu_pool_rows_reject_bad_arguments():
    """tools/emu_bad_args.py --only pool: every pointer of the new entry points null, every integer 0 and -1 -- refused with a message or harmless, none
    crashes (own process: a crash must not take pytest down)"""
    r = subprocess.run([sys.executable, os.path.join(ROOT, 'tools', 'emu_bad_args.py'), '--only', 'pool'], capture_output=True, text=True, cwd=ROOT)
    assert r.returncode == 0, r.stdout + r.stderr
    summary = [l for l in r.stdout.splitlines() if 'SUMMARY' in l]
    assert summary and '0 crashed' in summary[0], r.stdout
    accepted = [l for l in r.stdout.splitlines() if 'ACCEPTED' in l][0]
    # what may be accepted: std = NULL (optional), any value of the `unbiased` flag, pad = 0 -- valid calls, not unchecked arguments
    allowed = {'mv_time_stats_ex_f16.arg6=None', 'mv_time_stats_ex_f16.arg8=0', 'mv_time_stats_ex_f16.arg8=-1', 'mv_cast_pad_f16.arg6=0'}
    got = {item.strip() for item in accepted.split('ACCEPTED', 1)[1].split(';') if item.strip()}
    assert got <= allowed, got - allowed
