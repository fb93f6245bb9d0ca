"""The CAM++ dense layers on the MI355X, one launch form at a time (mv_cam_dense_block_f16 with the form pinned): every layer of a launch against the
fp64 layer of tests/cam_ref.py on the device's own input channels, under the bars of tests/cam_cases.py (twice the rounding model's own distance);
untouched inputs and pitch columns, finite outputs over a NaN-filled output region, the same bits for a row whatever the batch, the branch form 0
takes, and the refusal of a pinned form outside its geometry."""
import pytest
import torch

import cam_cases as cc
import layer_checks as lc

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'


def _lib():
    from mvector import _hip
    return _hip.lib()


@pytest.mark.parametrize('name', cc.GPU_CASES)
def test_gpu_cam_dense_layers_meet_the_fp64_layer(name):
    lc.cam_dense_case(_lib(), DEV, name)


# (form, T2, c_in, nlayers, dil[, seg_len]): two segments and a ragged last tile in each; the long form with a chunk that touches three segments
ROWS = {1: (150, 128, 3, 2), 2: (101, 96, 2, 2), 3: (321, 32, 2, 2, 80)}


@pytest.mark.parametrize('form', sorted(ROWS))
def test_gpu_cam_dense_row_bits_do_not_depend_on_the_batch_size(form):
    lc.cam_dense_batch_rows_case(_lib(), DEV, form, *ROWS[form])


def test_gpu_cam_dense_forms_agree_on_shared_geometries():
    """No bit-identity across forms is promised (the block kernel takes the context sums from the fp32 h, the per-layer kernel from the rounded one:
    tests/cam_ref.py), so none is asserted: the largest difference between the block kernel and the per-layer kernel on geometries both take is
    PRINTED -- on the first layer, where the two forms see the same input, and over all layers, each form on its own chain.  (The long form shares no
    geometry with the other two: T2 > 160 against T2 <= 160.)"""
    from mvector import _hip
    for name in ('block_T101_d2', 'block_T160_d1', 'block_T17_d1'):
        c = cc.CASES[name]
        x0, layers = cc.build(name)
        params = lc.cam_dense_params(_lib(), DEV, layers)
        got = {}
        for form in (_hip.CAM_FORM_BLOCK, _hip.CAM_FORM_LAYER):
            got[form], _ = lc.cam_dense_launch(_lib(), DEV, x0, params, c['c_in'], c['nlayers'], c['dil'], c['seg_len'], form, 8)
        first = slice(c['c_in'], c['c_in'] + 32)
        d_first = (got[1][..., first].float() - got[2][..., first].float()).abs().max().item()
        d_all = (cc.new_channels(got[1], c).float() - cc.new_channels(got[2], c).float()).abs().max().item()
        print(f'cam_dense forms 1 vs 2 on {name}: first layer max-abs {d_first:.3e}, all layers (each form on its own chain) {d_all:.3e}')
        assert all(bool(torch.isfinite(cc.new_channels(g, c).float()).all()) for g in got.values())


@pytest.mark.parametrize('name', list(cc.REFUSALS))
def test_gpu_cam_dense_pinned_form_outside_its_geometry_is_refused(name):
    msg = lc.cam_dense_refusal_case(_lib(), DEV, *cc.REFUSALS[name])
    assert 'does not take this geometry' in msg
