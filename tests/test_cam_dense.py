"""CAM++ dense layers without a GPU: the bars of tests/cam_cases.py can see the bugs their cases are named after (CPU, fp64), and the three launch
forms run under the emulator at layer level (mv_cam_dense_block_f16 on the emulator build of the same sources)."""
import os
import subprocess
import sys

import pytest
import torch

import cam_cases as cc
import cam_ref
import layer_checks as lc
from emu_lib import emu_cdll

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize('name', list(cc.CASES))
def test_a_wrong_layer_lies_outside_the_bars_of_the_case(name):
    """For every deliberately wrong reference that differs from the layer at the case's shape (cam_cases.edges): its distance from the TRUE fp64
    reference, on the rounding model's chain, exceeds the case's bar -- a device that computed the wrong layer could not pass.  Also: the committed
    MODEL_DISTANCE entry is what the CPU measures, and the reference's gates are spread."""
    c = cc.CASES[name]
    chain, layers = cc.model_chain(name)
    ref, gates = cam_ref.teacher_forced(chain, c['c_in'], layers, c['dil'], c['seg_len'], return_gates=True)
    cc.check_gate_spread(gates, name)
    mx, mean = cc.distances(cc.new_channels(chain, c), ref)
    tmx, tmean = cc.MODEL_DISTANCE[name]
    assert abs(mx - tmx) <= 2e-3 * tmx and abs(mean - tmean) <= 2e-3 * tmean, f"'{name}': ({mx:.3e}, {mean:.3e}) measured, table ({tmx:.3e}, {tmean:.3e})"
    bmx, bmean = cc.bars(name)
    for which in cc.edges(name):
        dmx, dmean = cc.distances(cc.wrong_reference(name, chain, layers, which), ref)
        assert dmx > bmx + mx, f'{name}: the wrong layer `{which}` is {dmx:.3e} from the reference, inside the bar {bmx:.3e} (+ the model\'s own {mx:.3e})'


def test_every_wrong_layer_is_required_somewhere():
    seen = {w for name in cc.CASES for w in cc.edges(name)}
    assert seen == set(cam_ref.WRONG) | {'stale_tile'}
    for form in (1, 2, 3):   # ... and in every form, except what a form's geometry excludes
        per = {w for n, c in cc.CASES.items() if cc.run_form(c) == form for w in cc.edges(n)}
        assert per == seen, (form, seen - per)


def test_the_rounding_model_is_the_reference_without_its_fp16_sites():
    """dense_layer in fp32 without rounding sites agrees with fp64 to fp32 accuracy: the model's distance is its fp16 sites, not a second algorithm"""
    c = cc.CASES['block_T101_d2']
    x0, layers = cc.build('block_T101_d2')
    y64 = cam_ref.dense_layer(x0, layers[0], c['dil'], c['seg_len'])
    y32 = cam_ref.dense_layer(x0, layers[0], c['dil'], c['seg_len'], torch.float32)
    assert (y32.double() - y64).abs().max().item() < 2e-5


@pytest.mark.parametrize('name', cc.EMU_CASES)
def test_emu_cam_dense(name):
    lc.cam_dense_case(emu_cdll(), 'cpu', name)


@pytest.mark.parametrize('name', list(cc.REFUSALS))
def test_emu_cam_dense_pinned_form_outside_its_geometry_is_refused(name):
    msg = lc.cam_dense_refusal_case(emu_cdll(), 'cpu', *cc.REFUSALS[name])
    assert 'does not take this geometry' in msg


def test_emu_cam_dense_rejects_bad_arguments():
    """tools/emu_bad_args.py --only cam: null pointers, nlayers 0 and 25, T2 0, ldx not a multiple of 8, ldx < c_out, a pinned form outside its
    geometry, a short workspace -- every one refused with a message, none crashes (own process: a crash must not take pytest down)"""
    r = subprocess.run([sys.executable, os.path.join(ROOT, 'tools', 'emu_bad_args.py'), '--only', 'cam'], capture_output=True, text=True, cwd=ROOT)
    assert r.returncode == 0, r.stdout + r.stderr
    summary = [l for l in r.stdout.splitlines() if 'SUMMARY' in l]
    assert summary and ' 0 accepted' in summary[0] and '0 crashed' in summary[0], r.stdout
