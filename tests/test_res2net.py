"""Res2Net under the SIMT emulator and on the host: the kernels of csrc/res2net2d.hip against torch on the merged S16 inputs, the handle
(mv_res2net_create, _hip.Model('res2net')) against the reference's goldens, the package module (mvector/models/res2net.py) against the same
goldens on the CPU, the refusals of the C ABI and the saturation keys.  The checks and their bars are in res2net_checks.py;
tests/test_gpu_res2net.py runs them on the device."""
import ctypes
import os
import re
import subprocess

import pytest
import torch

import res2net_checks as rc
from emu_lib import emu_cdll
from mvector import _hip

CPU = torch.device('cpu')
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ['mv_res2net_create', 'mv_conv2d_stem7_s16', 'mv_conv2d_stem7_peak_s16', 'mv_maxpool3s2_s16', 'mv_avgpool3_s16']


# ------------------------------------------------------------------------------------------------ per kernel

@pytest.mark.parametrize('shape', rc.POOL_SHAPES)
def test_emu_maxpool_copies_the_largest_pair_of_the_window(shape):
    """max-abs 0 against torch's max_pool2d(3, 2, 1) of the merged input on every shape, emulator and MI355X; (2, 6, 10, 40, 64): the kernel writes
    zero bits over the NaN fill in channels 40 .. 47 and leaves 48 .. 63 alone."""
    rc.check_maxpool(emu_cdll(), CPU, shape)


@pytest.mark.parametrize('stride', [1, 2])
@pytest.mark.parametrize('shape', rc.POOL_SHAPES)
def test_emu_avgpool_matches_the_s16_round_trip_of_torch(shape, stride):
    """Measured, emulator and MI355X alike: largest error / bound 0.000 on every shape and stride (the kernel adds the taps in torch's order and
    divides by 9 as torch does, so the fp32 values agree before the one rounding into S16); max-abs against fp64: kernel 2.7e-8 .. 9.1e-7, torch's
    fp32 2.7e-8 .. 5.3e-7 (the kernel's figure carries the S16 rounding of its output as well)."""
    rc.check_avgpool(emu_cdll(), CPU, shape, stride)


@pytest.mark.parametrize('stride', [1, 2])
def test_emu_avgpool_on_a_slice_of_wider_maps(stride):
    rc.check_avgpool_slice(emu_cdll(), CPU, stride)


@pytest.mark.parametrize('shape', rc.STEM_SHAPES)
def test_emu_stem_matches_fp64(shape):
    """Measured (max-abs against fp64, kernel / torch's fp32 conv2d on the CPU; the same kernel figures on the emulator and on the MI355X):
    (2, 5, 5, 16) 2.41e-7 / 2.82e-7; (2, 7, 8, 16) 7.39e-7 / 7.39e-7; (3, 41, 16, 24) 1.41e-6 / 1.45e-6; (1, 98, 80, 32) 3.28e-6 / 3.28e-6
    (format terms 7.2e-7 .. 1.9e-6).  The (3, 41, 16, 24) case has 24 maps in a unit pair of 32: channels 24 .. 31 are zero bits."""
    rc.check_stem(emu_cdll(), CPU, shape)


def test_emu_stem_reports_the_peak_before_the_clamp():
    rc.check_stem_peak(emu_cdll(), CPU)


def test_emu_kernel_rows_do_not_depend_on_the_batch():
    rc.check_batch_independence(emu_cdll(), CPU)


# ------------------------------------------------------------------------------------------------ goldens

@pytest.mark.parametrize('name', rc.GOLDENS[:6] + [
    pytest.param('res2net_default', marks=pytest.mark.skipif(os.environ.get('MV_SLOW_EMU') != '1', reason='minutes under the emulator (5.61 M parameters, '
                 '16 blocks); set MV_SLOW_EMU=1 (the GPU suite runs it: test_gpu_handle_matches_reference_golden)'))])
def test_emu_handle_matches_reference_golden(name):
    """Measured under the emulator (1 - cos, largest over the batch): tiny asp / sap / tap / tsp 2.5e-8 / 4.4e-8 / 1.2e-8 / 1.5e-7, tiny_s4 4.9e-8,
    tiny_s1 2.1e-7; largest map value 62.3 / 65.0 / 61.3, as the golden tool printed for the reference."""
    rc.check_golden(emu_cdll(), CPU, name)


def test_emu_tiny_model_rows_do_not_depend_on_the_batch():
    h, x, _ = rc.handle(emu_cdll(), CPU, 'res2net_tiny_s4')
    full = h.forward(x)
    for b in range(x.shape[0]):
        assert (rc.np_bits(h.forward(x[b:b + 1].contiguous())) == rc.np_bits(full[b:b + 1])).all()


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
    assert m.embd_dim == man['kwargs'].get('embd_dim', 192)


def test_module_keeps_the_reference_surface():
    from mvector.models.res2net import Bottle2neck, Res2Net
    m = Res2Net(32, m_channels=16, layers=[1, 2, 1, 1], base_width=32, scale=2, embd_dim=64)
    assert m.embd_dim == 64 and m.inplanes == 512 and m.base_width == 32 and m.scale == 2 and Bottle2neck.expansion == 4
    b0, b1 = m.layer2[0], m.layer2[1]
    assert isinstance(b0, Bottle2neck) and (b0.stype, b1.stype) == ('stage', 'normal') and b0.width == 16 and b0.nums == 1 and b0.scale == 2
    assert isinstance(b0.pool, torch.nn.AvgPool2d) and not hasattr(b1, 'pool') and b0.downsample is not None and b1.downsample is None
    assert isinstance(m.max_pool, torch.nn.MaxPool2d) and m.conv1.kernel_size == (7, 7) and m.conv1.stride == (3, 3) and m.conv1.padding == (1, 1)
    assert len(b0.convs) == len(b0.bns) == 1 and b0.convs[0].stride == (2, 2)
    assert all(float(b.weight.detach().min()) == 1.0 and float(b.bias.detach().abs().max()) == 0.0 for b in m.modules() if isinstance(b, torch.nn.BatchNorm2d))
    with pytest.raises(Exception, match='XYZ'):
        Res2Net(32, pooling_type='XYZ')
    x = torch.randn(2, 40, 32)
    assert m.train()(x).shape == (2, 64)   # training mode: the torch graph
    assert not m.__dict__.get('_native_handles')


@pytest.mark.parametrize('kw,why', [(dict(input_size=64, base_width=16), 'frequency size'), (dict(m_channels=12), 'm_channels'),
                                    (dict(scale=9), 'scale'), (dict(base_width=8, input_size=8), 'width')])
def test_module_names_what_the_library_refuses(kw, why):
    from mvector.models.res2net import Res2Net
    ok, reason = Res2Net(**dict(dict(input_size=32, m_channels=16, layers=[1, 1, 1, 1], base_width=32, scale=2), **kw))._native_supported()
    assert not ok and why in reason, reason


def test_res2net_kind_takes_its_head_from_its_config_not_from_the_model_argument():
    with pytest.raises(ValueError, match='only the ecapa and tdnn handles'):
        _hip.Model('res2net', rc.tiny_cfg(), {'x': torch.zeros(1)}, cdll=emu_cdll(), pooling_type='TAP')


# ------------------------------------------------------------------------------------------------ refusals at the C ABI

def _random_sd(**kw):
    from mvector.models.res2net import Res2Net
    torch.manual_seed(0)
    return Res2Net(**kw).state_dict()


def test_create_refusals():
    cdll = emu_cdll()
    sd = rc.case('res2net_tiny_asp')[1]
    for cfg, msg in [(rc.tiny_cfg(input_size=64, base_width=16), 'input_size // base_width = 4 differs from the frequency size 2'),
                     (rc.tiny_cfg(m_channels=12), 'm_channels must be a multiple of 8'),
                     (rc.tiny_cfg(m_channels=264), 'm_channels must be at most 256'),
                     (rc.tiny_cfg(input_size=8, base_width=8), 'block width floor(planes * base_width / 64) below 4 in layer1.0'),
                     (rc.tiny_cfg(scale=0), 'scale must be 1..8'),
                     (rc.tiny_cfg(scale=9), 'scale must be 1..8'),
                     (rc.tiny_cfg(layers=[1, 0, 1, 1]), 'every stage needs a block (stage 2)'),
                     (rc.tiny_cfg(pooling_type=4), 'pooling_type 4 is not MV_POOL_ASP'),
                     (rc.tiny_cfg(pooling_type=-1), 'pooling_type -1 is not MV_POOL_ASP')]:
        code, text = rc.create_rc(cdll, cfg, sd)
        assert code != 0 and msg in text, (msg, text)
    for key in ('conv1.weight', 'bn1.running_var', 'layer1.0.convs.0.weight', 'layer1.0.downsample.0.weight', 'layer3.0.bns.0.running_var',
                'layer4.0.conv3.weight', 'pooling.conv.conv.weight', 'bn3.running_mean', 'linear.weight'):
        code, text = rc.create_rc(cdll, rc.tiny_cfg(), {k: v for k, v in sd.items() if k != key})
        assert code != 0 and f"missing '{key}'" in text, (key, text)
    code, text = rc.create_rc(cdll, rc.tiny_cfg(pooling_type=_hip.MV_POOL_SAP), sd)     # an ASP state_dict asked for the SAP head
    assert code != 0 and 'missing' in text
    h = ctypes.c_void_p()
    assert cdll.mv_res2net_create(None, None, 0, ctypes.byref(h)) != 0 and b'null argument' in cdll.mv_last_error()
    assert cdll.mv_res2net_create(ctypes.byref(rc.tiny_cfg()), None, 0, ctypes.byref(h)) != 0 and b'empty tensor list' in cdll.mv_last_error()
    assert not h.value
    assert rc.create_rc(cdll, rc.tiny_cfg(), sd) == (0, '')


def test_create_takes_an_input_size_whose_frequency_chain_happens_to_fit():
    """input_size 48, base_width 32: frequency 15 -> 8 -> 8 -> 4 -> 2 -> 1 and 48 // 32 = 1"""
    kw = dict(input_size=48, m_channels=16, layers=[1, 1, 1, 1], base_width=32, scale=2, embd_dim=64)
    assert rc.create_rc(emu_cdll(), rc.tiny_cfg(input_size=48), _random_sd(**kw)) == (0, '')
    from mvector.models.res2net import Res2Net
    assert Res2Net(**kw)._native_supported() == (True, '')


def test_forward_refuses_four_frames():
    h, x, _ = rc.handle(emu_cdll(), CPU, 'res2net_tiny_tap')
    with pytest.raises(RuntimeError, match='at least 5 frames'):
        h.workspace_bytes(1, 4)
    ws = torch.empty(h.workspace_bytes(3, 5), dtype=torch.uint8)
    emb = torch.zeros(3, 64)
    feats = x[:, :4].contiguous()
    code = emu_cdll().mv_model_forward(h._h, feats.data_ptr(), 3, 4, emb.data_ptr(), ws.data_ptr(), ws.numel(), None)
    assert code != 0 and b'at least 5 frames' in emu_cdll().mv_last_error()
    assert torch.count_nonzero(emb) == 0
    assert torch.isfinite(h.forward(x[:, :5].contiguous())).all()   # five frames: one time step at the head, which the average takes


def test_layer_entry_points_refuse_bad_arguments():
    cdll = emu_cdll()
    m, y = torch.zeros(2, 3, 5, 16), torch.zeros(2, 3, 5, 16)
    x, o = torch.zeros(2, 8, 8), torch.zeros(2, 2, 2, 16)
    w, b = torch.zeros(16, 49), torch.zeros(16)
    P = lambda t: t.data_ptr()   # noqa: E731
    cases = [
        (cdll.mv_conv2d_stem7_s16, (None, P(o), P(w), P(b), 2, 8, 8, 16), 'null pointer'),
        (cdll.mv_conv2d_stem7_s16, (P(x), None, P(w), P(b), 2, 8, 8, 16), 'null pointer'),
        (cdll.mv_conv2d_stem7_s16, (P(x), P(o), None, P(b), 2, 8, 8, 16), 'null pointer'),
        (cdll.mv_conv2d_stem7_s16, (P(x), P(o), P(w), None, 2, 8, 8, 16), 'null pointer'),
        (cdll.mv_conv2d_stem7_s16, (P(x), P(o), P(w), P(b), 0, 8, 8, 16), 'sizes must be positive'),
        (cdll.mv_conv2d_stem7_s16, (P(x), P(o), P(w), P(b), 2, 8, 8, 0), 'sizes must be positive'),
        (cdll.mv_conv2d_stem7_s16, (P(x), P(o), P(w), P(b), 2, 4, 8, 16), 'at least 5 bins and 5 frames'),
        (cdll.mv_conv2d_stem7_s16, (P(x), P(o), P(w), P(b), 2, 8, 4, 16), 'at least 5 bins and 5 frames'),
        (cdll.mv_conv2d_stem7_s16, (P(x), P(o), P(w), P(b), 2, 8, 8, 272), 'a multiple of 8, at most 256'),
        (cdll.mv_conv2d_stem7_s16, (P(x), P(o), P(w), P(b), 2, 8, 8, 12), 'a multiple of 8, at most 256'),
        (cdll.mv_conv2d_stem7_peak_s16, (P(x), None, P(w), P(b), 2, 8, 8, 16, None), 'null pointer'),
        (cdll.mv_maxpool3s2_s16, (None, 16, P(y), 16, 2, 3, 5, 16), 'null pointer'),
        (cdll.mv_maxpool3s2_s16, (P(m), 16, None, 16, 2, 3, 5, 16), 'null pointer'),
        (cdll.mv_maxpool3s2_s16, (P(m), 16, P(y), 16, 2, 0, 5, 16), 'sizes must be positive'),
        (cdll.mv_maxpool3s2_s16, (P(m), 16, P(y), 16, 2, 3, 5, -16), 'sizes must be positive'),
        (cdll.mv_maxpool3s2_s16, (P(m), 16, P(y), 16, 2, 3, 5, 32), 'leading dimension'),
        (cdll.mv_maxpool3s2_s16, (P(m), 24, P(y), 16, 2, 3, 5, 16), 'leading dimension'),
        (cdll.mv_maxpool3s2_s16, (P(m), 16, P(y), 8, 2, 3, 5, 16), 'leading dimension'),
        (cdll.mv_avgpool3_s16, (None, 16, P(y), 16, 2, 3, 5, 16, 1), 'null pointer'),
        (cdll.mv_avgpool3_s16, (P(m), 16, None, 16, 2, 3, 5, 16, 1), 'null pointer'),
        (cdll.mv_avgpool3_s16, (P(m), 16, P(y), 16, 2, 3, 0, 16, 1), 'sizes must be positive'),
        (cdll.mv_avgpool3_s16, (P(m), 16, P(y), 16, 2, 3, 5, 17, 1), 'leading dimension'),
        (cdll.mv_avgpool3_s16, (P(m), 16, P(y), 40, 2, 3, 5, 16, 1), 'leading dimension'),
        (cdll.mv_avgpool3_s16, (P(m), 16, P(y), 16, 2, 3, 5, 16, 0), 'stride must be 1 or 2'),
        (cdll.mv_avgpool3_s16, (P(m), 16, P(y), 16, 2, 3, 5, 16, 3), 'stride must be 1 or 2'),
    ]
    for fn, args, msg in cases:
        with pytest.raises(RuntimeError, match=msg):
            _hip.check(fn(*args, None), cdll)
    for t in (y, o):
        assert torch.count_nonzero(t) == 0


# ------------------------------------------------------------------------------------------------ saturation keys

def test_saturation_keys():
    cdll = emu_cdll()
    assert (_hip.MV_INFO_S16_PEAK, _hip.MV_INFO_S16_SATURATED) == (30, 31) == (_hip.MV_INFO_RESNETSE_PEAK, _hip.MV_INFO_RESNETSE_SATURATED)
    h, x, _ = rc.handle(cdll, CPU, 'res2net_tiny_asp')
    assert h.s16_range() == {'peak': 0.0, 'saturated': False} == h.resnet_se_range()    # nothing has run
    h.forward(x)
    r = h.s16_range()
    assert not r['saturated'] and h.info(_hip.MV_INFO_S16_SATURATED) == 0.0
    assert 62.3 / 2 < r['peak'] < 62.3 * 2     # (the reference's maps of this fixture reach 62.3: tools/make_res2net_golden.py)

    def hot(sd):
        sd['conv1.weight'] = sd['conv1.weight'] * 1e4
    hh, x, _ = rc.handle(cdll, CPU, 'res2net_tiny_asp', edit=hot)
    hh.forward(x)
    assert hh.s16_range()['saturated'] and hh.info(_hip.MV_INFO_S16_PEAK) > 65504.0 / 64
    with pytest.raises(RuntimeError, match='no such key'):
        hh.info(8)
    man, sd, _, _, _ = rc.case('res2net_tiny_asp')
    cfg = rc.module(man, sd)._native_cfg()
    cfg.pooling_type |= _hip.MV_RES2NET_NO_PEAK       # the tools' handle without the word: the same bits, the keys say -1
    plain = _hip.Model('res2net', cfg, sd, cdll=cdll)
    assert (rc.np_bits(plain.forward(x)) == rc.np_bits(h.forward(x))).all()
    assert plain.info(_hip.MV_INFO_S16_PEAK) == -1.0 and plain.info(_hip.MV_INFO_S16_SATURATED) == -1.0


# ------------------------------------------------------------------------------------------------ exports

def test_new_symbols_are_declared_bound_and_exported():
    with open(os.path.join(ROOT, 'include', 'mvector_hip.h')) as f:
        header = f.read()
    for s in NEW_SYMBOLS:
        assert re.search(r'\bint ' + s + r'\(', header), s
        assert s in _hip.EXPORTED_SYMBOLS
    for name in ('MV_INFO_S16_PEAK 30', 'MV_INFO_S16_SATURATED 31', 'MV_INFO_RESNETSE_PEAK MV_INFO_S16_PEAK', 'MV_ABI_VERSION 5'):
        assert '#define ' + name in header, name
    import __graft_entry__
    lib = __graft_entry__.build()
    dyn = subprocess.run(['nm', '-D', '--defined-only', lib], capture_output=True, text=True, check=True).stdout
    exported = {line.split()[-1] for line in dyn.splitlines() if line.strip()}
    assert not [s for s in NEW_SYMBOLS if s not in exported]
