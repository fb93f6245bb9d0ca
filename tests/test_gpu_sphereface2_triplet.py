"""SphereFace2 and the triplet loss on the device: the checks of tests/sphereface2_checks.py and tests/triplet_checks.py on the product library
(also the shape of 10^6 columns the emulator is too slow for, every seed of the large triplet shapes, and a second stream), the two classes of
mvector.loss on CUDA tensors, and SpeakerIdentification -> loss -> backward() through the torch graph."""
import os

import numpy as np
import pytest
import torch

import margin_loss_checks as mlc
import sphereface2_checks as sfc
import triplet_checks as tpc
from helpers import GOLDEN

pytestmark = pytest.mark.gpu
DEV = 'cuda'
DTYPES = (torch.float32, torch.float16, torch.bfloat16)


@pytest.fixture(scope='module')
def golden():
    return np.load(os.path.join(GOLDEN, 'margin_loss.npz'))


@pytest.mark.parametrize('t', sfc.TS)
@pytest.mark.parametrize('name', sfc.TYPES)
def test_gpu_sphereface2_against_the_fp64_oracle(name, t):
    sfc.check_type(None, DEV, name, t)


@pytest.mark.parametrize('name', ('C', 'A'))
def test_gpu_sphereface2_a_million_columns(name):
    sfc.check_device_shape(None, DEV, name)


def test_gpu_sphereface2_half_inputs_are_the_fp32_path_on_the_upcast_logits():
    sfc.check_half_inputs(None, DEV)


def test_gpu_sphereface2_in_place_backward():
    sfc.check_in_place(None, DEV)


def test_gpu_sphereface2_no_hidden_state():
    sfc.check_no_hidden_state(None, DEV, second_stream=True)


def test_gpu_sphereface2_labels_out_of_range():
    sfc.check_bad_labels(None, DEV)


def test_gpu_sphereface2_nan_logit():
    sfc.check_nan_logit(None, DEV)


def test_gpu_sphereface2_refusals_by_name():
    sfc.check_refusals(None, DEV)


def test_gpu_sphereface2_meets_the_reference_within_the_bound_of_its_fp32_front(golden):
    sfc.check_golden(None, DEV, golden)


@pytest.mark.parametrize('B,D', tpc.SHAPES)
def test_gpu_triplet_against_the_fp64_oracle(B, D):
    tpc.check_shape(None, DEV, B, D)


def test_gpu_triplet_no_hidden_state():
    tpc.check_no_hidden_state(None, DEV, second_stream=True)


def test_gpu_triplet_zero_norm_row():
    tpc.check_zero_norm_row(None, DEV)


def test_gpu_triplet_refusals_by_name():
    tpc.check_refusals(None, DEV)


def test_gpu_triplet_meets_the_reference(golden):
    tpc.check_golden(None, DEV, golden)


# ------------------------------------------------------------------ host layers
def test_gpu_sphereface2_class_is_the_two_native_calls():
    from mvector import _hip
    from mvector.loss import SphereFace2
    for dtype in DTYPES:
        for margin_type in ('C', 'A'):
            p = dict(margin=0.25, scale=30.0, lanbuda=0.7, t=3, margin_type=margin_type)
            module = SphereFace2(**p).to(DEV)
            with torch.no_grad():
                module.bias.fill_(-0.5)
            logits, _ = mlc.make_logits(5, 777, 1, 3, device=DEV, dtype=dtype)
            labels = mlc.make_labels(5, 777, 0).to(DEV)
            x = logits.clone().requires_grad_(True)
            loss = module({'features': None, 'logits': x}, labels)
            (loss * 0.5).backward()
            want_loss, _, want_pred, saved = _hip.sphereface2_forward(logits, labels, module.bias, **p)
            want_grad, want_bias = _hip.sphereface2_backward(logits, labels, module.bias, saved, torch.tensor(0.5, device=DEV), **p)
            assert loss.dtype == torch.float32 and torch.equal(loss.detach(), want_loss), (dtype, margin_type)
            assert x.grad.dtype == dtype and torch.equal(x.grad, want_grad), (dtype, margin_type)
            assert module.bias.grad.shape == (1, 1) and torch.equal(module.bias.grad.reshape(1), want_bias), (dtype, margin_type)
            assert module.pred.dtype == torch.int32 and torch.equal(module.pred, want_pred)
            # update() travels with the next call
            module.update(margin=0.4)
            again = module({'features': None, 'logits': logits}, labels)
            assert torch.equal(again, _hip.sphereface2_forward(logits, labels, module.bias, **dict(p, margin=0.4))[0])
            assert not torch.equal(again, want_loss)
    # a second derivative is refused with a message
    module = SphereFace2().to(DEV)
    x = mlc.make_logits(2, 9, 1, 1, device=DEV)[0].clone().requires_grad_(True)
    loss = module({'features': None, 'logits': x}, torch.tensor([1, 2], device=DEV))
    (g,) = torch.autograd.grad(loss, x, create_graph=True)
    with pytest.raises(RuntimeError, match='no second derivative'):
        g.sum().backward()
    # no fallback between the paths: fp64 logits on the device run the torch expression, and give the torch expression's result
    xd = mlc.make_logits(3, 50, 1, 2, device=DEV)[0].double()
    yd = torch.tensor([0, 49, 7], device=DEV)
    module = SphereFace2().to(DEV).double()
    got = module({'features': None, 'logits': xd}, yd)
    assert got.dtype == torch.float64 and module.pred is None
    want = SphereFace2().double()({'features': None, 'logits': xd.cpu()}, yd.cpu())
    assert abs(float(got.detach()) - float(want.detach())) < 1e-12


def test_gpu_triplet_class_is_the_native_calls():
    from mvector import _hip
    from mvector.loss import TripletAngularMarginLoss
    for dtype in DTYPES:
        for eps in (0.0, 0.1):
            module = TripletAngularMarginLoss(margin=0.5, absolute_loss_weight=0.7, label_smoothing=eps)
            p = dict(margin=0.5, normalize=True, add_absolute=True, absolute_loss_weight=0.7, ap_value=0.8, an_value=0.4)
            ce_p = dict(kind='ce', margin=0.0, scale=1.0, label_smoothing=eps)
            features, _ = tpc.make_features(6, 24, 0, dtype=dtype, device=DEV)
            logits, _ = mlc.make_logits(6, 40, 1, 3, device=DEV, dtype=dtype)
            labels = torch.tensor([3, 3, 17, 17, 39, 39], device=DEV)
            f, x = features.clone().requires_grad_(True), logits.clone().requires_grad_(True)
            loss = module({'features': f, 'logits': x}, labels)
            (loss * 0.5).backward()
            half = torch.tensor(0.5, device=DEV)
            t_loss, mined, index = _hip.triplet_forward(features, labels, **p)
            ce_loss, _, want_pred, saved = _hip.margin_ce_forward(logits, labels, **ce_p)
            assert loss.dtype == torch.float32 and torch.equal(loss.detach(), t_loss + ce_loss), (dtype, eps)
            assert f.grad.dtype == dtype and torch.equal(f.grad, _hip.triplet_backward(features, labels, mined, index, half, **p)), (dtype, eps)
            assert x.grad.dtype == dtype and torch.equal(x.grad, _hip.margin_ce_backward(logits, labels, saved, half, **ce_p)), (dtype, eps)
            assert torch.equal(module.pred, want_pred)
            # update() travels with the next call
            module.update(margin=0.9)
            again = module({'features': features, 'logits': logits}, labels)
            assert torch.equal(again, _hip.triplet_forward(features, labels, **dict(p, margin=0.9))[0] + ce_loss) and not torch.equal(again, loss)
    # a second derivative is refused with a message
    f = tpc.make_features(4, 8, 1, device=DEV)[0].clone().requires_grad_(True)
    logits = mlc.make_logits(4, 9, 1, 1, device=DEV)[0]
    loss = TripletAngularMarginLoss()({'features': f, 'logits': logits}, torch.tensor([1, 1, 2, 2], device=DEV))
    (g,) = torch.autograd.grad(loss, f, create_graph=True)
    with pytest.raises(RuntimeError, match='no second derivative'):
        g.sum().backward()
    # no fallback between the paths: fp64 tensors on the device run the torch expression, and give the torch expression's result
    fd, xd = tpc.make_features(6, 24, 2, device=DEV)[0].double(), mlc.make_logits(6, 50, 1, 2, device=DEV)[0].double()
    yd = torch.tensor([0, 0, 7, 7, 49, 49], device=DEV)
    module = TripletAngularMarginLoss()
    got = module({'features': fd, 'logits': xd}, yd)
    assert got.dtype == torch.float64 and module.pred is None
    assert abs(float(got) - float(TripletAngularMarginLoss()({'features': fd.cpu(), 'logits': xd.cpu()}, yd.cpu()))) < 1e-12


def test_gpu_speaker_identification_to_sphereface2_and_triplet_to_backward():
    from mvector.loss import SphereFace2, TripletAngularMarginLoss
    from mvector.models.fc import SpeakerIdentification
    torch.manual_seed(0)
    labels = torch.tensor([0, 4, 9, 4, 1, 0], device=DEV)
    for make in (lambda: SphereFace2(margin_type='C'), lambda: SphereFace2(margin_type='A'), lambda: TripletAngularMarginLoss()):
        loss = make().to(DEV)
        feats = torch.randn(6, 24, device=DEV, requires_grad=True)
        head = SpeakerIdentification(24, 10).to(DEV)
        value = loss(head(feats), labels)
        value.backward()
        assert torch.isfinite(value) and loss.pred.shape == (6,) and loss.pred.dtype == torch.int32
        assert head.weight.grad.abs().sum() > 0 and feats.grad.abs().sum() > 0
        # the same step through the torch expression, in fp64 on the CPU
        loss64 = make().double()
        head64 = SpeakerIdentification(24, 10).double()
        head64.load_state_dict({k: v.detach().cpu().double() for k, v in head.state_dict().items()})
        f64 = feats.detach().cpu().double().requires_grad_(True)
        value64 = loss64(head64(f64), labels.cpu())
        value64.backward()
        assert torch.allclose(value.detach().cpu().double(), value64.detach(), rtol=1e-3, atol=1e-5)
        assert torch.allclose(head.weight.grad.cpu().double(), head64.weight.grad, rtol=1e-3, atol=1e-5)
        assert torch.allclose(feats.grad.cpu().double(), f64.grad, rtol=1e-3, atol=1e-5)
        if isinstance(loss, SphereFace2):
            assert torch.allclose(loss.bias.grad.cpu().double(), loss64.bias.grad, rtol=1e-3, atol=1e-5)
