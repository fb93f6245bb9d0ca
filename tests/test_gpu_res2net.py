"""Res2Net on the MI355X: the per-kernel checks of tests/test_res2net.py (same shapes, same bars: res2net_checks.py) on the device, the seven
reference goldens through the handle and through the package module's CUDA forward, the batch / stream independence of an embedding's bits,
the module's routing (eval CUDA forward = the native handle; train() drops it) and the saturation keys."""
import pytest
import torch

import res2net_checks as rc
from helpers import cos_dist
from mvector import _hip

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def dev():
    return torch.device('cuda:0')


@pytest.fixture(scope='module')
def lib():
    return _hip.lib()


@pytest.mark.parametrize('shape', rc.POOL_SHAPES)
def test_gpu_maxpool_copies_the_largest_pair_of_the_window(lib, dev, shape):
    rc.check_maxpool(lib, dev, shape)


@pytest.mark.parametrize('stride', [1, 2])
@pytest.mark.parametrize('shape', rc.POOL_SHAPES)
def test_gpu_avgpool_matches_the_s16_round_trip_of_torch(lib, dev, shape, stride):
    rc.check_avgpool(lib, dev, shape, stride)


@pytest.mark.parametrize('stride', [1, 2])
def test_gpu_avgpool_on_a_slice_of_wider_maps(lib, dev, stride):
    rc.check_avgpool_slice(lib, dev, stride)


@pytest.mark.parametrize('shape', rc.STEM_SHAPES)
def test_gpu_stem_matches_fp64(lib, dev, shape):
    rc.check_stem(lib, dev, shape)


def test_gpu_stem_reports_the_peak_before_the_clamp(lib, dev):
    rc.check_stem_peak(lib, dev)


def test_gpu_kernel_rows_do_not_depend_on_the_batch(lib, dev):
    rc.check_batch_independence(lib, dev)


@pytest.mark.parametrize('name', rc.GOLDENS)
def test_gpu_handle_matches_reference_golden(lib, dev, name):
    """Measured on the MI355X (1 - cos, largest over the batch; profiles/res2net_gpu.log): tiny asp / sap / tap / tsp 2.5e-8 / 4.6e-8 / 1.3e-8 /
    1.5e-7, tiny_s4 4.9e-8, tiny_s1 2.1e-7, default 3.0e-8 (largest map value 30.1)."""
    rc.check_golden(lib, dev, name)


@pytest.mark.parametrize('name', rc.GOLDENS)
def test_gpu_module_forward_matches_reference_golden(dev, name):
    man, sd, x, emb, _ = rc.case(name)
    m = rc.module(man, sd).to(dev)
    assert not m.__dict__.get('_native_handles')
    got = m(x.to(dev))
    assert len(m.__dict__['_native_handles']) == 1       # the CUDA eval forward took the native path: exactly one handle exists
    d = cos_dist(got.cpu(), emb).max().item()
    print(f'{name} (module): 1 - cos {d:.2e}')
    assert d <= 1e-4, d
    if name == 'res2net_tiny_asp':
        m(x.to(dev))
        assert len(m.__dict__['_native_handles']) == 1    # ... and a second forward builds no other
        h = next(iter(m.__dict__['_native_handles'].values()))[0]
        assert not h.s16_range()['saturated']
        m.train()
        assert not m.__dict__['_native_handles']          # train() drops it
        xg = x.to(dev).requires_grad_(True)
        m.eval()(xg).sum().backward()                     # a forward that needs input gradients: the torch graph
        assert xg.grad is not None and not m.__dict__['_native_handles']


def test_gpu_embedding_bits_do_not_depend_on_batch_or_stream(lib, dev):
    h, x, _ = rc.handle(lib, dev, 'res2net_tiny_asp')
    full = h.forward(x)
    torch.cuda.synchronize()
    assert x.shape[0] == 3
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
    h, x, _ = rc.handle(lib, dev, 'res2net_tiny_asp', edit=hot)
    h.forward(x)
    assert h.s16_range()['saturated'] and h.resnet_se_range()['saturated']
    ok, x, _ = rc.handle(lib, dev, 'res2net_tiny_asp')
    ok.forward(x)
    r = ok.s16_range()
    assert not r['saturated'] and 62.3 / 2 < r['peak'] < 62.3 * 2     # (the reference's maps of this fixture reach 62.3)
