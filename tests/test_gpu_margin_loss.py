"""The margin-softmax losses on the device: the checks of tests/margin_loss_checks.py on the product library (also the two shapes of 10^6
columns the emulator is too slow for, and a second stream), the five native classes of mvector.loss on CUDA tensors, and
SpeakerIdentification -> loss -> backward() through the torch graph."""
import pytest
import torch

import margin_loss_checks as mlc

pytestmark = pytest.mark.gpu
DEV = 'cuda'


@pytest.mark.parametrize('name', sorted(mlc.KINDS))
def test_gpu_forward_and_backward_against_the_fp64_oracle(name):
    mlc.check_kind(None, DEV, name)


@pytest.mark.parametrize('B,N,K,name', mlc.DEVICE_SHAPES)
def test_gpu_a_million_columns(B, N, K, name):
    mlc.check_device_shape(None, DEV, B, N, K, name)


def test_gpu_half_inputs_are_the_fp32_path_on_the_upcast_logits():
    mlc.check_half_inputs(None, DEV)


def test_gpu_in_place_backward():
    mlc.check_in_place(None, DEV)


def test_gpu_no_hidden_state():
    mlc.check_no_hidden_state(None, DEV, second_stream=True)


def test_gpu_labels_out_of_range():
    mlc.check_bad_labels(None, DEV)


def test_gpu_nan_logit():
    mlc.check_nan_logit(None, DEV)


def test_gpu_refusals_by_name():
    mlc.check_refusals(None, DEV)


def test_gpu_native_classes_are_the_two_native_calls():
    from mvector import _hip
    from mvector import loss as L
    for dtype in (torch.float32, torch.float16, torch.bfloat16):
        for module, p in ((L.CELoss(label_smoothing=0.1), dict(kind='ce', margin=0.0, scale=1.0, label_smoothing=0.1)),
                          (L.AMLoss(margin=0.3, scale=30), dict(kind='am', margin=0.3, scale=30)),
                          (L.ARMLoss(margin=0.3, scale=30), dict(kind='arm', margin=0.3, scale=30)),
                          (L.AAMLoss(margin=0.25, easy_margin=True), dict(kind='aam', margin=0.25, scale=32, easy_margin=True)),
                          (L.SubCenterLoss(margin=0.25, K=3, label_smoothing=0.1),
                           dict(kind='subcenter', margin=0.25, scale=32, K=3, label_smoothing=0.1))):
            K = p.get('K', 1)
            logits, _ = mlc.make_logits(5, 777, K, 3, device=DEV, dtype=dtype)
            labels = mlc.make_labels(5, 777, 0).to(DEV)
            x = logits.clone().requires_grad_(True)
            loss = module({'features': None, 'logits': x}, labels)
            (loss * 0.5).backward()
            want_loss, _, want_pred, saved = _hip.margin_ce_forward(logits, labels, **p)
            want_grad = _hip.margin_ce_backward(logits, labels, saved, torch.tensor(0.5, device=DEV), **p)
            assert loss.dtype == torch.float32 and torch.equal(loss.detach(), want_loss), (dtype, p['kind'])
            assert x.grad.dtype == dtype and torch.equal(x.grad, want_grad), (dtype, p['kind'])
            assert torch.equal(module.pred, want_pred)
            # update() travels with the next call
            if p['kind'] != 'ce':
                module.update(margin=0.4)
                again = module({'features': None, 'logits': logits}, labels)
                assert torch.equal(again, _hip.margin_ce_forward(logits, labels, **dict(p, margin=0.4))[0]) and not torch.equal(again, want_loss)
    # a second derivative is refused with a message
    x = mlc.make_logits(2, 9, 1, 1, device=DEV)[0].clone().requires_grad_(True)
    loss = L.AAMLoss()({'features': None, 'logits': x}, torch.tensor([1, 2], device=DEV))
    (g,) = torch.autograd.grad(loss, x, create_graph=True)
    with pytest.raises(RuntimeError, match='no second derivative'):
        g.sum().backward()
    # no fallback between the paths: fp64 logits on the device run the torch expression, and give the torch expression's result
    xd = mlc.make_logits(3, 50, 1, 2, device=DEV)[0].double()
    yd = torch.tensor([0, 49, 7], device=DEV)
    m = L.AAMLoss()
    got = m({'features': None, 'logits': xd}, yd)
    assert got.dtype == torch.float64 and m.pred is None
    assert abs(float(got) - float(L.AAMLoss()({'features': None, 'logits': xd.cpu()}, yd.cpu()))) < 1e-12


def test_gpu_speaker_identification_to_loss_to_backward():
    from mvector.loss import AAMLoss, SubCenterLoss
    from mvector.models.fc import SpeakerIdentification
    torch.manual_seed(0)
    labels = torch.tensor([0, 4, 9, 4, 1, 0], device=DEV)
    for K, loss in ((1, AAMLoss(label_smoothing=0.1)), (3, SubCenterLoss(K=3))):
        feats = torch.randn(6, 24, device=DEV, requires_grad=True)
        head = SpeakerIdentification(24, 10, K=K).to(DEV)
        value = loss(head(feats), labels)
        value.backward()
        assert torch.isfinite(value) and loss.pred.shape == (6,) and loss.pred.dtype == torch.int32
        assert head.weight.grad.abs().sum() > 0 and feats.grad.abs().sum() > 0
        # the same step through the torch expression, in fp64 on the CPU
        head64 = SpeakerIdentification(24, 10, K=K).double()
        head64.load_state_dict({k: v.detach().cpu().double() for k, v in head.state_dict().items()})
        f64 = feats.detach().cpu().double().requires_grad_(True)
        loss(head64(f64), labels.cpu()).backward()
        assert torch.allclose(head.weight.grad.cpu().double(), head64.weight.grad, rtol=1e-3, atol=1e-5)
        assert torch.allclose(feats.grad.cpu().double(), f64.grad, rtol=1e-3, atol=1e-5)
