"""ResNetSE under the SIMT emulator and on the host: the kernels of csrc/se2d.hip each against fp64 of the merged S16 inputs, the handle
(mv_resnetse_create, _hip.Model('resnet_se')) against the reference's goldens, the package module (mvector/models/resnet_se.py) against
the same goldens on the CPU, the refusals of the C ABI and the saturation keys.  The checks and their bars are in resnet_se_checks.py;
tests/test_gpu_resnet_se.py runs them on the device."""
import ctypes
import os

import pytest
import torch

import resnet_se_checks as rc
from emu_lib import emu_cdll
from mvector import _hip

CPU = torch.device('cpu')


# ------------------------------------------------------------------------------------------------ per kernel

@pytest.mark.parametrize('shape', rc.SQUEEZE_SHAPES)
def test_emu_squeeze_matches_fp64(shape):
    """Measured (max-abs against fp64, kernel / torch's fp32 mean; the same figures on the emulator and on the MI355X): (2,3,5,16) 1.03e-7 /
    1.71e-7; (3,8,41,32) 2.89e-8 / 9.28e-8; (1,80,98,64) 1.43e-8 / 4.75e-8; the planes of 255 / 256 / 257 pixels 2.58e-8 / 8.12e-8, 2.85e-8 /
    8.02e-8, 2.85e-8 / 5.62e-8.  The sums are carried in fp64: what is left is the rounding of the finished mean to fp32."""
    rc.check_squeeze(emu_cdll(), CPU, shape)


@pytest.mark.parametrize('C,R', rc.EXCITE_SHAPES)
def test_emu_excite_matches_fp64(C, R):
    """Measured (max-abs against fp64, kernel / torch's fp32 evaluation on this CPU): (32, 4) 3.06e-8 / 1.77e-7; (96, 12) 4.78e-8 / 1.12e-7;
    (512, 64) 8.49e-8 / 2.46e-7.  The kernel sums the fp32 products in fp64 and rounds the hidden unit and the gate once each."""
    rc.check_excite(emu_cdll(), CPU, C, R)


@pytest.mark.parametrize('shape', rc.MAP_SHAPES)
def test_emu_gate_matches_the_s16_round_trip_of_torch(shape):
    """The (3, 8, 41, 32, 48) map carries a padded unit (channels 32..47), res always has its own leading dimension (ld + 16), x has both signs.
    The format's own round trip (split -> merge of an fp32 value) is within 2^-22 relative + 2^-31: below the bar, which therefore stands as set."""
    rc.check_gate(emu_cdll(), CPU, shape)


def test_emu_gate_channels_padded_from_48_to_64_stay_zero():
    """48 channels in a map of 64, gated in place: channels 48 .. 63 are zeros before and zero bits after"""
    rc.check_gate(emu_cdll(), CPU, (2, 5, 9, 48, 64), in_place=True)


def test_emu_gate_padding_inside_a_unit_is_written_as_zeros():
    """40 channels: the kernel owns the unit 32 .. 47 and writes zero bits over the NaN fill in 40 .. 47 (no gate exists there); 48 .. 63 are not its"""
    rc.check_gate(emu_cdll(), CPU, (2, 5, 9, 40, 64))


def test_emu_gate_reports_the_peak_before_the_clamp():
    rc.check_gate_peak(emu_cdll(), CPU)


@pytest.mark.parametrize('H,W,C', rc.ROWS_SHAPES)
def test_emu_rows_are_the_permuted_fp16_of_the_map(H, W, C):
    rc.check_rows(emu_cdll(), CPU, H, W, C)


def test_emu_rows_zero_a_longer_pitch():
    rc.check_rows(emu_cdll(), CPU, 3, 7, 96, pitch_extra=24)


# ------------------------------------------------------------------------------------------------ bits do not depend on the batch

def test_emu_squeeze_and_gate_rows_do_not_depend_on_the_batch():
    cdll = emu_cdll()
    B, H, W, C, ld = 3, 8, 41, 32, 48
    x, _ = rc.make_map(cdll, CPU, B, H, W, C, ld, seed=1)
    r, _ = rc.make_map(cdll, CPU, B, H, W, C, ld, seed=2)
    g = torch.rand(B, C, generator=torch.Generator().manual_seed(3))
    s_full, y_full = rc.squeeze(cdll, x, C), rc.gate(cdll, x, g, r, C)
    for b in range(B):
        xb, rb, gb = x[b:b + 1].contiguous(), r[b:b + 1].contiguous(), g[b:b + 1].contiguous()
        assert (rc.np_bits(rc.squeeze(cdll, xb, C)) == rc.np_bits(s_full[b:b + 1])).all()
        assert (rc.np_bits(rc.gate(cdll, xb, gb, rb, C)) == rc.np_bits(y_full[b:b + 1])).all()


def test_emu_tiny_model_rows_do_not_depend_on_the_batch():
    h, x, _ = rc.handle(emu_cdll(), CPU, 'resnetse_tiny_asp')
    full = h.forward(x)
    assert x.shape[0] == 3
    for b in range(3):
        assert (rc.np_bits(h.forward(x[b:b + 1].contiguous())) == rc.np_bits(full[b:b + 1])).all()


# ------------------------------------------------------------------------------------------------ goldens

@pytest.mark.parametrize('name', rc.GOLDENS[:5] + [
    pytest.param('resnetse_default', marks=pytest.mark.skipif(os.environ.get('MV_SLOW_EMU') != '1', reason='11 min 38 s under the emulator, where it '
                 'passes at 1 - cos 2.8e-9 (9.12 M parameters, 16 blocks on 80 x 98 maps); set MV_SLOW_EMU=1 (the GPU suite runs it: '
                 'test_gpu_handle_matches_reference_golden)'))])
def test_emu_handle_matches_reference_golden(name):
    rc.check_golden(emu_cdll(), CPU, name)


# ------------------------------------------------------------------------------------------------ module level

@pytest.mark.parametrize('name', rc.GOLDENS)
def test_module_cpu_forward_matches_reference_golden(name):
    man, sd, x, emb, _ = rc.case(name)
    m = rc.module(man, sd)   # load_state_dict(strict=True) with the manifest's shapes
    assert {k: list(v.shape) for k, v in m.state_dict().items()} == man['shapes']
    with torch.no_grad():
        got = m(x)
    assert torch.allclose(got, emb, atol=1e-4, rtol=1e-4), (got - emb).abs().max().item()
    ok, why = m._native_supported()
    assert ok, why
    assert m.embd_dim == man['kwargs']['embd_dim'] if 'embd_dim' in man['kwargs'] else m.embd_dim == 192


def test_module_keeps_the_reference_surface():
    from mvector.models.resnet_se import ResNetSE, SEBottleneck, SELayer
    m = ResNetSE(16, layers=[1, 1, 1, 1], num_filters=[16, 16, 32, 32], embd_dim=64)
    assert m.embd_dim == 64 and m.inplanes == 64 and SEBottleneck.expansion == 2
    assert isinstance(m.layer1[0], SEBottleneck) and isinstance(m.layer1[0].se, SELayer)
    assert m.layer1[0].downsample is not None and m.layer1[0].stride == 1 and m.layer2[0].stride == (2, 2)
    assert all(float(b.weight.detach().min()) == 1.0 and float(b.bias.detach().abs().max()) == 0.0 for b in m.modules() if isinstance(b, torch.nn.BatchNorm2d))
    with pytest.raises(Exception, match='XYZ'):
        ResNetSE(16, pooling_type='XYZ')
    x = torch.randn(2, 20, 16)
    assert m.train()(x).shape == (2, 64)   # training mode: the torch graph
    assert not m.__dict__.get('_native_handles')


@pytest.mark.parametrize('kw,why', [(dict(input_size=16, num_filters=[24, 16, 32, 32]), 'num_filters'), (dict(input_size=20), 'input_size')])
def test_module_names_what_the_library_refuses(kw, why):
    from mvector.models.resnet_se import ResNetSE
    ok, reason = ResNetSE(**dict(dict(layers=[1, 1, 1, 1], num_filters=[16, 16, 32, 32]), **kw))._native_supported()
    assert not ok and why in reason


def test_resnet_se_kind_takes_its_head_from_its_config_not_from_the_model_argument():
    with pytest.raises(ValueError, match='only the ecapa and tdnn handles'):
        _hip.Model('resnet_se', rc.tiny_cfg(), {'x': torch.zeros(1)}, cdll=emu_cdll(), pooling_type='TAP')


# ------------------------------------------------------------------------------------------------ refusals at the C ABI

def test_create_refusals():
    cdll = emu_cdll()
    sd = rc.case('resnetse_tiny_asp')[1]
    for cfg, msg in [(rc.tiny_cfg(input_size=20), 'input_size must be a multiple of 8'),
                     (rc.tiny_cfg(num_filters=[24, 16, 32, 32]), 'num_filters must be multiples of 16, at most 512 (entry 0)'),
                     (rc.tiny_cfg(num_filters=[16, 16, 32, 528]), 'num_filters must be multiples of 16, at most 512 (entry 3)'),
                     (rc.tiny_cfg(layers=[1, 0, 1, 1]), 'every stage needs a block (stage 2)'),
                     (rc.tiny_cfg(pooling_type=4), 'pooling_type 4 is not MV_POOL_ASP'),
                     (rc.tiny_cfg(pooling_type=-1), 'pooling_type -1 is not MV_POOL_ASP'),
                     (rc.tiny_cfg(reduction=64), 'without a hidden unit')]:
        code, text = rc.create_rc(cdll, cfg, sd)
        assert code != 0 and msg in text, (msg, text)
    for key in ('conv1.weight', 'layer1.0.se.fc.0.weight', 'layer1.0.downsample.0.weight', 'layer3.0.bn2.running_var', 'pooling.conv.conv.weight',
                'bn3.running_mean', 'linear.weight'):
        code, text = rc.create_rc(cdll, rc.tiny_cfg(), {k: v for k, v in sd.items() if k != key})
        assert code != 0 and f"missing '{key}'" in text, (key, text)
    code, text = rc.create_rc(cdll, rc.tiny_cfg(pooling_type=_hip.MV_POOL_SAP), sd)     # an ASP state_dict asked for the SAP head
    assert code != 0 and 'missing' in text
    h = ctypes.c_void_p()
    assert cdll.mv_resnetse_create(None, None, 0, ctypes.byref(h)) != 0 and b'null argument' in cdll.mv_last_error()
    assert cdll.mv_resnetse_create(ctypes.byref(rc.tiny_cfg()), None, 0, ctypes.byref(h)) != 0 and b'empty tensor list' in cdll.mv_last_error()
    assert not h.value
    assert rc.create_rc(cdll, rc.tiny_cfg(), sd) == (0, '')


def test_forward_refuses_eight_frames():
    h, x, _ = rc.handle(emu_cdll(), CPU, 'resnetse_tiny_asp')
    with pytest.raises(RuntimeError, match='at least 9 frames'):
        h.workspace_bytes(1, 8)
    ws = torch.empty(h.workspace_bytes(3, 9), dtype=torch.uint8)
    emb = torch.zeros(3, 64)
    feats = x[:, :8].contiguous()
    code = emu_cdll().mv_model_forward(h._h, feats.data_ptr(), 3, 8, emb.data_ptr(), ws.data_ptr(), ws.numel(), None)
    assert code != 0 and b'at least 9 frames' in emu_cdll().mv_last_error()
    assert torch.count_nonzero(emb) == 0
    assert torch.isfinite(h.forward(x[:, :9].contiguous())).all()   # nine frames: two time steps at the head


def test_layer_entry_points_refuse_bad_arguments():
    cdll = emu_cdll()
    m = torch.zeros(2, 3, 5, 16)
    s, g, ws = torch.zeros(2, 16), torch.zeros(2, 16), torch.zeros(64)
    y16 = torch.zeros(2, 5, 48, dtype=torch.float16)
    w1, b1, w2, b2 = torch.zeros(4, 16), torch.zeros(4), torch.zeros(16, 4), torch.zeros(16)
    P = lambda t: t.data_ptr()   # noqa: E731
    cases = [
        (cdll.mv_se2d_squeeze_s16, (None, 16, 2, 3, 5, 16, P(s), P(ws), 64), 'null pointer'),
        (cdll.mv_se2d_squeeze_s16, (P(m), 16, 2, 3, 5, 16, None, P(ws), 64), 'null pointer'),
        (cdll.mv_se2d_squeeze_s16, (P(m), 16, 2, 3, 5, 16, P(s), None, 64), 'null pointer'),
        (cdll.mv_se2d_squeeze_s16, (P(m), 16, 0, 3, 5, 16, P(s), P(ws), 64), 'sizes must be positive'),
        (cdll.mv_se2d_squeeze_s16, (P(m), 16, 2, 3, 0, 16, P(s), P(ws), 64), 'sizes must be positive'),
        (cdll.mv_se2d_squeeze_s16, (P(m), 16, 2, 3, 5, 0, P(s), P(ws), 64), 'sizes must be positive'),
        (cdll.mv_se2d_squeeze_s16, (P(m), 16, 2, 3, 5, 32, P(s), P(ws), 64), 'leading dimension'),
        (cdll.mv_se2d_squeeze_s16, (P(m), 24, 2, 3, 5, 16, P(s), P(ws), 64), 'leading dimension'),
        (cdll.mv_se2d_squeeze_s16, (P(m), 16, 2, 3, 5, 16, P(s), P(ws), 63), 'workspace too small'),
        (cdll.mv_se2d_excite_f32, (None, P(w1), P(b1), P(w2), P(b2), P(g), 2, 16, 4), 'null pointer'),
        (cdll.mv_se2d_excite_f32, (P(s), P(w1), P(b1), P(w2), P(b2), None, 2, 16, 4), 'null pointer'),
        (cdll.mv_se2d_excite_f32, (P(s), P(w1), P(b1), P(w2), P(b2), P(g), 0, 16, 4), 'sizes must be positive'),
        (cdll.mv_se2d_excite_f32, (P(s), P(w1), P(b1), P(w2), P(b2), P(g), 2, 16, 0), 'sizes must be positive'),
        (cdll.mv_se2d_excite_f32, (P(s), P(w1), P(b1), P(w2), P(b2), P(g), 2, 1040, 4), 'at most 1024'),
        (cdll.mv_se2d_gate_res_relu_s16, (None, 16, P(g), P(m), 16, P(m), 16, 2, 3, 5, 16, None), 'null pointer'),
        (cdll.mv_se2d_gate_res_relu_s16, (P(m), 16, None, P(m), 16, P(m), 16, 2, 3, 5, 16, None), 'null pointer'),
        (cdll.mv_se2d_gate_res_relu_s16, (P(m), 16, P(g), P(m), 16, P(m), 16, 2, 0, 5, 16, None), 'sizes must be positive'),
        (cdll.mv_se2d_gate_res_relu_s16, (P(m), 16, P(g), P(m), 8, P(m), 16, 2, 3, 5, 16, None), 'leading dimension'),
        (cdll.mv_se2d_gate_res_relu_s16, (P(m), 16, P(g), P(m), 16, P(m), 24, 2, 3, 5, 16, None), 'leading dimension'),
        (cdll.mv_se2d_gate_res_relu_s16, (P(m), 16, P(g), P(m), 16, P(m), 16, 2, 3, 5, 17, None), 'leading dimension'),
        (cdll.mv_s16_map_to_rows_f16, (None, 16, 2, 3, 5, 16, P(y16), 48), 'null pointer'),
        (cdll.mv_s16_map_to_rows_f16, (P(m), 16, 2, 3, 5, 16, None, 48), 'null pointer'),
        (cdll.mv_s16_map_to_rows_f16, (P(m), 16, 2, 3, 5, 0, P(y16), 48), 'sizes must be positive'),
        (cdll.mv_s16_map_to_rows_f16, (P(m), 16, -1, 3, 5, 16, P(y16), 48), 'sizes must be positive'),
        (cdll.mv_s16_map_to_rows_f16, (P(m), 20, 2, 3, 5, 16, P(y16), 48), 'leading dimension'),
        (cdll.mv_s16_map_to_rows_f16, (P(m), 16, 2, 3, 5, 32, P(y16), 96), 'leading dimension'),
        (cdll.mv_s16_map_to_rows_f16, (P(m), 16, 2, 3, 5, 16, P(y16), 40), 'row pitch'),
        (cdll.mv_s16_map_to_rows_f16, (P(m), 16, 2, 3, 5, 16, P(y16), 52), 'row pitch'),
    ]
    for fn, args, msg in cases:
        with pytest.raises(RuntimeError, match=msg):
            _hip.check(fn(*args, None), cdll)
    assert cdll.mv_se2d_squeeze_workspace_floats(0, 3, 5, 16) == 0 and cdll.mv_se2d_squeeze_workspace_floats(2, 3, 5, 16) == 2 * 2 * 16
    for t in (s, g, ws, y16):
        assert torch.count_nonzero(t) == 0


# ------------------------------------------------------------------------------------------------ saturation keys

def test_saturation_keys():
    cdll = emu_cdll()
    h, x, _ = rc.handle(cdll, CPU, 'resnetse_tiny_asp')
    assert h.resnet_se_range() == {'peak': 0.0, 'saturated': False}    # nothing has run
    h.forward(x)
    r = h.resnet_se_range()
    assert not r['saturated'] and 0.0 < r['peak'] < 65504.0 / 64 and h.info(_hip.MV_INFO_RESNETSE_SATURATED) == 0.0
    assert 10.0 < r['peak'] < 40.0     # (the reference's maps of this fixture reach 21.3)

    def hot(sd):
        sd['conv1.weight'] = sd['conv1.weight'] * 1e4
    hh, x, _ = rc.handle(cdll, CPU, 'resnetse_tiny_asp', edit=hot)
    hh.forward(x)
    assert hh.info(_hip.MV_INFO_RESNETSE_SATURATED) == 1.0 and hh.info(_hip.MV_INFO_RESNETSE_PEAK) > 65504.0 / 64
    with pytest.raises(RuntimeError, match='no such key'):
        hh.info(8)
    man, sd, _, _, _ = rc.case('resnetse_tiny_asp')
    cfg = rc.module(man, sd)._native_cfg()
    cfg.pooling_type |= _hip.MV_RESNETSE_NO_PEAK       # the tools' handle without the word: the same bits, the keys say -1
    plain = _hip.Model('resnet_se', cfg, sd, cdll=cdll)
    assert (rc.np_bits(plain.forward(x)) == rc.np_bits(h.forward(x))).all()
    assert plain.info(_hip.MV_INFO_RESNETSE_PEAK) == -1.0 and plain.info(_hip.MV_INFO_RESNETSE_SATURATED) == -1.0
