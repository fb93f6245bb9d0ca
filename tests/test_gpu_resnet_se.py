"""ResNetSE on the MI355X: the per-kernel checks of tests/test_resnet_se.py (same shapes, same bars: resnet_se_checks.py) on the device, the
six reference goldens through the handle and through the package module's CUDA forward, the batch / stream independence of an embedding's
bits, and the module's routing (eval CUDA forward = the native handle; train() drops it)."""
import pytest
import torch

import resnet_se_checks as rc
from helpers import cos_dist
from mvector import _hip

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def dev():
    return torch.device('cuda:0')


@pytest.fixture(scope='module')
def lib():
    return _hip.lib()


@pytest.mark.parametrize('shape', rc.SQUEEZE_SHAPES)
def test_gpu_squeeze_matches_fp64(lib, dev, shape):
    rc.check_squeeze(lib, dev, shape)


@pytest.mark.parametrize('C,R', rc.EXCITE_SHAPES)
def test_gpu_excite_matches_fp64(lib, dev, C, R):
    rc.check_excite(lib, dev, C, R)


@pytest.mark.parametrize('shape', rc.MAP_SHAPES + [(2, 5, 9, 40, 64)])
def test_gpu_gate_matches_the_s16_round_trip_of_torch(lib, dev, shape):
    rc.check_gate(lib, dev, shape)


def test_gpu_gate_channels_padded_from_48_to_64_stay_zero(lib, dev):
    rc.check_gate(lib, dev, (2, 5, 9, 48, 64), in_place=True)


def test_gpu_gate_reports_the_peak_before_the_clamp(lib, dev):
    rc.check_gate_peak(lib, dev)


@pytest.mark.parametrize('H,W,C', rc.ROWS_SHAPES)
def test_gpu_rows_are_the_permuted_fp16_of_the_map(lib, dev, H, W, C):
    rc.check_rows(lib, dev, H, W, C)
    if C == 96:
        rc.check_rows(lib, dev, H, W, C, pitch_extra=24)


def test_gpu_squeeze_and_gate_rows_do_not_depend_on_the_batch(lib, dev):
    B, H, W, C, ld = 3, 8, 41, 32, 48
    x, _ = rc.make_map(lib, dev, B, H, W, C, ld, seed=1)
    r, _ = rc.make_map(lib, dev, B, H, W, C, ld, seed=2)
    g = torch.rand(B, C, generator=torch.Generator().manual_seed(3)).to(dev)
    s_full, y_full = rc.squeeze(lib, x, C), rc.gate(lib, x, g, r, C)
    for b in range(B):
        xb, rb, gb = x[b:b + 1].contiguous(), r[b:b + 1].contiguous(), g[b:b + 1].contiguous()
        assert (rc.np_bits(rc.squeeze(lib, xb, C)) == rc.np_bits(s_full[b:b + 1])).all()
        assert (rc.np_bits(rc.gate(lib, xb, gb, rb, C)) == rc.np_bits(y_full[b:b + 1])).all()


@pytest.mark.parametrize('name', rc.GOLDENS)
def test_gpu_handle_matches_reference_golden(lib, dev, name):
    """Measured on the MI355X (1 - cos, largest over the batch; profiles/resnet_se_gpu.log): tiny asp / sap / tap / tsp 9.0e-9 / 1.3e-8 / 3.4e-9 /
    5.0e-8, tiny2 9.6e-9, default 2.8e-9."""
    rc.check_golden(lib, dev, name)


@pytest.mark.parametrize('name', rc.GOLDENS)
def test_gpu_module_forward_matches_reference_golden(dev, name):
    man, sd, x, emb, _ = rc.case(name)
    m = rc.module(man, sd).to(dev)
    assert not m.__dict__.get('_native_handles')
    got = m(x.to(dev))
    assert len(m.__dict__['_native_handles']) == 1       # the CUDA eval forward took the native path: the handle exists
    d = cos_dist(got.cpu(), emb).max().item()
    print(f'{name} (module): 1 - cos {d:.2e}')
    assert d <= 1e-4, d
    if name == 'resnetse_tiny_asp':
        h = next(iter(m.__dict__['_native_handles'].values()))[0]
        assert not h.resnet_se_range()['saturated']
        m.train()
        assert not m.__dict__['_native_handles']          # train() drops it
        xg = x.to(dev).requires_grad_(True)
        m.eval()(xg).sum().backward()                     # a forward that needs input gradients: the torch graph
        assert xg.grad is not None and not m.__dict__['_native_handles']


def test_gpu_embedding_bits_do_not_depend_on_batch_or_stream(lib, dev):
    h, x, _ = rc.handle(lib, dev, 'resnetse_tiny_asp')
    full = h.forward(x)
    torch.cuda.synchronize()
    for b in range(3):
        assert (rc.np_bits(h.forward(x[b:b + 1].contiguous())) == rc.np_bits(full[b:b + 1])).all()
    side = torch.cuda.Stream(device=dev)
    side.wait_stream(torch.cuda.current_stream(dev))
    with torch.cuda.stream(side):
        other = h.forward(x)                               # a workspace of its own (keyed by stream)
    side.synchronize()
    assert len(h._ws) == 2
    assert (rc.np_bits(other) == rc.np_bits(full)).all()


def test_gpu_saturation_keys(lib, dev):
    def hot(sd):
        sd['conv1.weight'] = sd['conv1.weight'] * 1e4
    h, x, _ = rc.handle(lib, dev, 'resnetse_tiny_asp', edit=hot)
    h.forward(x)
    assert h.resnet_se_range()['saturated']
    ok, x, _ = rc.handle(lib, dev, 'resnetse_tiny_asp')
    ok.forward(x)
    r = ok.resnet_se_range()
    assert not r['saturated'] and 10.0 < r['peak'] < 40.0
